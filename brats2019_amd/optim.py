"""Drop-in for `torch.optim.Adam` in the reference's training call (main.py:133-137: `optimizer=optim.Adam`, lr 2e-5, weight_decay
1e-6, amsgrad=True; instantiated by `Trainer.train`, train.py:82-83), running the update as the HIP kernel `ru_adam_step`.

`Adam(params, lr, betas, eps, weight_decay, amsgrad)` is a `torch.optim.Optimizer`: param groups, `zero_grad()`, LR schedulers
(`StepLR` rewrites `group["lr"]`) and `state_dict()` / `load_state_dict()` behave as torch's -- the state keeps torch's own layout
(`state[p] = {"step", "exp_avg", "exp_avg_sq"[, "max_exp_avg_sq"]}`), so a checkpoint written by either optimizer resumes under the
other (train.py:92-94, 320-324).  What differs is where the state lives and how many launches a step takes: the moment tensors of a
group are views of THREE flat buffers laid out like the parameters' own flat buffer (model.UNet aliases every nn.Parameter to one
float32 buffer; the executor writes every gradient into one bucket), so `step()` is one kernel launch per contiguous RUN of
parameters that have a gradient -- three for the shipped network (the never-executed deepest decoder stage keeps grad=None,
model.py:420, and is skipped exactly as torch.optim.Adam skips it) -- instead of ~15 foreach kernels over 86 tensors.
Parameters or gradients that are not laid out that way (any other model) take one launch per tensor.  HIP-only: CPU tensors raise.

The rest of the recipe (csrc/optim.hip), all of it opt-in and on the same flat buffers:

  * `SGD(params, lr, momentum, dampening, weight_decay, nesterov)`: `torch.optim.SGD`'s update and state layout (`state[p]["momentum_buffer"]`,
    views of ONE flat buffer), one `ru_sgd_step` launch per run;
  * `AdamW(...)`: `Adam`'s surface with decoupled weight decay (`torch.optim.AdamW`), `ru_adamw_step`;
  * `clip_grad_norm_(parameters, max_norm, optimizer=None)`: the float64 global norm as a 0-dim device tensor, never synchronising.  Handed one
    of this module's optimizers it leaves the gradients alone: the device coefficient is folded into that optimizer's next `step()`;
  * `PolyLR(optimizer, max_steps, exponent)`: `lr = base * (1 - step / max_steps) ** exponent`;
  * `EMA(model, decay)`: an exponential moving average of the weights in one flat shadow buffer, `update()` / `swap()`;
  * `sgd_step_host`, `adamw_step_host`, `clip_coef_host`, `ema_host`: float64 numpy restatements of the kernels' formulas (test infrastructure).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L


class _FlatOptimizer(torch.optim.Optimizer):
    """What Adam, AdamW and SGD share: per-parameter state tensors that are views of flat buffers laid out like the parameters' own flat buffer
    (so that a step is one launch per contiguous run), and the clipping coefficient `clip_grad_norm_` leaves for the next `step()`."""
    _HAS_STEP = True               # the state carries torch's per-parameter "step" counter

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._flat = {}            # group index -> flat-state plan
        self._pending_coef = None  # float32[1] on the device, from clip_grad_norm_(..., optimizer=self); consumed by the next step()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._flat = {}
        self._pending_coef = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)          # deep-copies the state onto the parameters' device: the aliasing is re-made lazily
        self._flat = {}

    def _name(self):
        return "brats2019_amd.optim." + type(self).__name__

    def _state_keys(self, group):
        raise NotImplementedError

    def _plan(self, gi, group):
        """Lay the group's state out like its parameters: if every parameter is a contiguous float32 slice of one allocation span,
        the state tensors become views of flat buffers covering the same span at the same offsets (existing state is copied in)."""
        plan = self._flat.get(gi)
        params = [p for p in group["params"]]
        keys = self._state_keys(group)
        sig = (keys,) + tuple((p.data_ptr(), p.dtype, p.device) for p in params)     # (a flipped amsgrad flag needs the third buffer)
        if plan is not None and plan["sig"] == sig:
            return plan
        for p in params:
            if not p.is_cuda:
                raise RuntimeError("%s: parameters must live on a ROCm GPU (HIP-only path; no CPU fallback)" % self._name())
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("%s: contiguous float32 parameters only" % self._name())
        lo = min(p.data_ptr() for p in params)
        hi = max(p.data_ptr() + 4 * p.numel() for p in params)
        span = (hi - lo) // 4
        dev = params[0].device
        total = sum(p.numel() for p in params)
        flat_ok = span <= 2 * total + 1024 and all(p.device == dev for p in params)       # one allocation span, not scattered tensors
        bufs = {k: torch.zeros(span if flat_ok else 0, dtype=torch.float32, device=dev) for k in keys}
        order = sorted(range(len(params)), key=lambda i: params[i].data_ptr())
        plan = dict(sig=sig, lo=lo, span=span, flat=flat_ok, bufs=bufs, order=order, keys=keys)
        for p in params:                     # state that exists already (load_state_dict, an earlier plan) moves into the flat buffers
            if p in self.state and self.state[p]:
                self._init_state(plan, p, create=self._HAS_STEP)
        self._flat[gi] = plan
        return plan

    def _init_state(self, plan, p, create=True):
        """torch's lazy state initialisation (zeros, step 0) -- with the state tensors as views of the group's flat buffers.  create=False
        moves what exists and leaves an absent (or None) entry as it is."""
        st = self.state[p]
        off = (p.data_ptr() - plan["lo"]) // 4
        for k in plan["keys"]:
            old = st.get(k)
            if old is None and not create:
                continue
            if plan["flat"]:
                view = plan["bufs"][k][off:off + p.numel()].view_as(p)
                if old is not None and old.data_ptr() != view.data_ptr():
                    view.copy_(old.to(device=p.device, dtype=torch.float32))
                st[k] = view
            elif old is None or not (old.is_cuda and old.dtype == torch.float32 and old.is_contiguous()):
                st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format) if old is None else old.to(device=p.device, dtype=torch.float32).contiguous()
        if self._HAS_STEP and "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)              # torch.optim.Adam's default: a CPU scalar tensor
        return st

    def _grad(self, p):
        g = p.grad
        if g is None:
            return None
        if g.is_sparse:
            raise RuntimeError("%s does not support sparse gradients" % type(self).__name__)
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(device=p.device, dtype=torch.float32).contiguous()
            p.grad = g
        return g

    def _take_coef(self):
        """(the pending coefficient's tensor, its device pointer): the caller keeps the tensor until its launches are queued"""
        coef, self._pending_coef = self._pending_coef, None
        return coef, (None if coef is None else C.c_void_p(coef.data_ptr()))

    @staticmethod
    def _lr(group):
        lr = group["lr"]
        return float(lr.item()) if isinstance(lr, torch.Tensor) else float(lr)


class Adam(_FlatOptimizer):
    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **unsupported):
        for k, v in unsupported.items():
            # accepted-and-ignored when they have torch's defaults; anything that would change the arithmetic is refused
            if k in ("foreach", "fused", "capturable", "differentiable", "maximize", "decoupled_weight_decay") and not v:
                continue
            raise NotImplementedError("%s: option %s=%r is not implemented by the HIP kernel" % (self._name(), k, v))
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    # ------------------------------------------------------------------ flat state
    _KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def _state_keys(self, group):
        return self._KEYS if group["amsgrad"] else self._KEYS[:2]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        stream = L.stream()
        coef_tensor, coef = self._take_coef()
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            plan = self._plan(gi, group)
            ams = bool(group["amsgrad"])
            b1, b2 = group["betas"]
            lr = self._lr(group)
            # runs: consecutive (in memory) parameters with a gradient whose gradients and moments are consecutive at the same stride
            runs = []      # [w_ptr, g_ptr, m_ptr, v_ptr, vmax_ptr, numel, step]
            for i in plan["order"]:
                p = params[i]
                g = self._grad(p)
                if g is None:
                    continue
                st = self.state[p]
                if "step" not in st or any(k not in st for k in plan["keys"]):      # lazy init; also a state loaded without `max_exp_avg_sq` under amsgrad
                    st = self._init_state(plan, p)
                stp = st["step"]
                k = int(stp.item() if isinstance(stp, torch.Tensor) else stp) + 1
                if isinstance(stp, torch.Tensor):
                    stp += 1
                else:
                    st["step"] = k
                n = p.numel()
                ptrs = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                        st["max_exp_avg_sq"].data_ptr() if ams else 0)
                if runs:
                    r = runs[-1]
                    if r[6] == k and all(r[j] + 4 * r[5] == ptrs[j] for j in range(4 + int(ams))):
                        r[5] += n
                        continue
                runs.append([ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], n, k])
            for w, g, m, v, vm, n, k in runs:
                if coef is None and not self._DECOUPLED:
                    L.check(lib.ru_adam_step(w, g, m, v, vm if ams else None, n, lr, float(b1), float(b2), float(group["eps"]),
                                             float(group["weight_decay"]), k, stream), "ru_adam_step")
                else:          # AdamW, or a clipping coefficient is pending: the same arithmetic on coef * g (decoupled = 0)
                    L.check(lib.ru_adamw_step(w, g, m, v, vm if ams else None, n, lr, float(b1), float(b2), float(group["eps"]),
                                              float(group["weight_decay"]), int(self._DECOUPLED), k, coef, stream), "ru_adamw_step")
            self.__dict__["last_launches"] = len(runs)
        del coef_tensor                    # held until here: its memory must not be handed out again before the launches that read it are queued
        return loss


class AdamW(Adam):
    """`torch.optim.AdamW`: the decay multiplies the weights (`w *= 1 - lr * weight_decay`) and never enters the moments."""
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **unsupported):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **unsupported)


class SGD(_FlatOptimizer):
    """`torch.optim.SGD` (momentum, dampening, weight decay, Nesterov) as one `ru_sgd_step` launch per run."""
    _HAS_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **unsupported):
        for k, v in unsupported.items():
            if k in ("foreach", "fused", "differentiable", "maximize") and not v:
                continue
            raise NotImplementedError("%s: option %s=%r is not implemented by the HIP kernel" % (self._name(), k, v))
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("%s: a tensor learning rate is not implemented by the HIP kernel" % self._name())
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)

    def _state_keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        stream = L.stream()
        coef_tensor, coef = self._take_coef()
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            plan = self._plan(gi, group)
            mom = float(group["momentum"])
            runs = []      # [w_ptr, g_ptr, buf_ptr, numel, first]
            for i in plan["order"]:
                p = params[i]
                g = self._grad(p)
                if g is None:
                    continue
                buf, first = 0, False
                if mom != 0:
                    st = self.state[p]
                    first = st.get("momentum_buffer") is None          # torch: the first step CLONES d into the buffer, whatever the dampening
                    if first:
                        st = self._init_state(plan, p)
                    buf = st["momentum_buffer"].data_ptr()
                n = p.numel()
                ptrs = (p.data_ptr(), g.data_ptr(), buf)
                if runs:
                    r = runs[-1]
                    if r[4] == first and all(r[j] + 4 * r[3] == ptrs[j] for j in range(3 if mom != 0 else 2)):
                        r[3] += n
                        continue
                runs.append([ptrs[0], ptrs[1], ptrs[2], n, first])
            for w, g, buf, n, first in runs:
                L.check(lib.ru_sgd_step(w, g, buf if mom != 0 else None, n, self._lr(group), mom, float(group["dampening"]), float(group["weight_decay"]),
                                        int(bool(group["nesterov"])), int(first), coef, stream), "ru_sgd_step")
            self.__dict__["last_launches"] = len(runs)
        del coef_tensor                    # (as in Adam.step)
        return loss


# ---------------------------------------------------------------------- gradient clipping
def _runs_of(tensors):
    """[(tensor of the run's first element, numel)]: tensors that follow one another in memory form one run"""
    runs = []
    for t in sorted(tensors, key=lambda t: t.data_ptr()):
        if runs and runs[-1][0].data_ptr() + 4 * runs[-1][1] == t.data_ptr():
            runs[-1][1] += t.numel()
        elif t.numel():
            runs.append([t, t.numel()])
    return runs


def clip_grad_norm_(parameters, max_norm, optimizer=None):
    """`torch.nn.utils.clip_grad_norm_(parameters, max_norm)` (2-norm, error_if_nonfinite=False) without a host synchronisation: the norm over the
    gradients that are not None is summed in float64 by `ru_gradnorm_partial` (one launch per contiguous run: three on the network's aliased
    bucket, one per tensor where nothing is adjacent) and `ru_gradnorm_finalize`, and returned as a 0-dim float64 device tensor.

    `optimizer` one of this module's (and stepping the same parameters): the gradients are NOT rewritten -- the device coefficient
    `min(1, max_norm / (norm + 1e-6))` waits in the optimizer, whose next `step()` folds it into its update and clears it.
    Otherwise the gradients are scaled in place by `ru_scale_by`.  A non-finite norm gives a non-finite coefficient, as torch's."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError("clip_grad_norm_: max_norm must be a non-negative number, got %r" % (max_norm,))
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros((), dtype=torch.float64)
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.device != dev:
            raise RuntimeError("brats2019_amd.optim.clip_grad_norm_: gradients must live on one ROCm GPU (HIP-only path; no CPU fallback)")
        if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
            raise TypeError("brats2019_amd.optim.clip_grad_norm_: contiguous dense float32 gradients only")
    lib = L.load()
    stream = L.stream()
    runs = _runs_of(grads)
    slots = [int(lib.ru_gradnorm_slots(n)) for _, n in runs]
    ws = torch.empty(max(sum(slots), 1), dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=torch.float64, device=dev)
    coef = torch.empty(1, dtype=torch.float32, device=dev)
    first = 0
    for (t, n), k in zip(runs, slots):
        L.check(lib.ru_gradnorm_partial(C.c_void_p(t.data_ptr()), n, first, L.ptr(ws), ws.numel() * 8, stream), "ru_gradnorm_partial")
        first += k
    L.check(lib.ru_gradnorm_finalize(L.ptr(ws), first, max_norm, L.ptr(out), L.ptr(coef), stream), "ru_gradnorm_finalize")
    if isinstance(optimizer, _FlatOptimizer):
        optimizer._pending_coef = coef
    else:
        for t, n in runs:
            L.check(lib.ru_scale_by(C.c_void_p(t.data_ptr()), n, L.ptr(coef), stream), "ru_scale_by")
    clip_grad_norm_.last_launches = len(runs) + 1 + (0 if isinstance(optimizer, _FlatOptimizer) else len(runs))
    return out


# ---------------------------------------------------------------------- learning-rate schedule
class PolyLR(torch.optim.lr_scheduler.LRScheduler):
    """`lr = base_lr * (1 - step / max_steps) ** exponent`, 0 from `max_steps` on; `step()` once per iteration, as Trainer steps its scheduler."""

    def __init__(self, optimizer, max_steps, exponent=0.9, last_epoch=-1):
        if not max_steps > 0:
            raise ValueError("PolyLR: max_steps must be positive, got %r" % (max_steps,))
        self.max_steps = max_steps
        self.exponent = exponent
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        frac = max(0.0, 1.0 - self.last_epoch / self.max_steps)
        return [base * frac ** self.exponent for base in self.base_lrs]

    def resume_at(self, step):
        """Continue at `step` iterations done (the schedule is a closed form of the count): what Trainer calls after it restored a checkpoint."""
        self.last_epoch = int(step)
        for group, lr in zip(self.optimizer.param_groups, self.get_lr()):
            group["lr"] = lr
        self._last_lr = [group["lr"] for group in self.optimizer.param_groups]


# ---------------------------------------------------------------------- exponential moving average of the weights
class EMA(object):
    """`shadow = decay * shadow + (1 - decay) * w` after every optimizer step, in ONE flat float32 buffer over the parameters' span (initialised
    to the weights), one `ru_ema_update` launch per live run.  `swap()` exchanges the live and the averaged weights in place -- swap in,
    evaluate or save, swap back -- and drops the executor's packed weight copies (`UNet.freeze_params` caches them until the weights move).
    Parameters the network never executes (model.UNet's deepest decoder stage) never change: they are their own average and are left out."""

    def __init__(self, model, decay):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("EMA: decay must lie in [0, 1], got %r" % (decay,))
        self.model, self.decay = model, decay
        self.swapped = False
        self.num_updates = 0
        net = model.module if hasattr(model, "module") else model
        self._net = net
        dead = set()
        if hasattr(net, "_get_engine"):
            dead = {k for k, v in net._get_engine().layout.entries.items() if v[2]}
        named = [(k, p) for k, p in net.named_parameters()]
        if hasattr(net, "_flat_params") and all(p.is_cuda for _, p in named):
            net._flat_params()                       # model.UNet aliases its parameters to one flat buffer at the first forward: do it now, they must not move later
        for _, p in named:
            if not p.is_cuda:
                raise RuntimeError("brats2019_amd.optim.EMA: parameters must live on a ROCm GPU (HIP-only path; no CPU fallback)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("brats2019_amd.optim.EMA: contiguous float32 parameters only")
        lo = min(p.data_ptr() for _, p in named)
        hi = max(p.data_ptr() + 4 * p.numel() for _, p in named)
        span, total = (hi - lo) // 4, sum(p.numel() for _, p in named)
        dev = named[0][1].device
        flat_ok = span <= 2 * total + 1024 and all(p.device == dev for _, p in named)
        pad = (lo % 16) // 4                                  # the shadow sits at the parameters' offset from a 16-byte boundary: 16-byte lanes
        self._store = torch.zeros((span if flat_ok else total) + pad, dtype=torch.float32, device=dev)
        self.shadow = self._store[pad:]
        self._views, self._live, off = {}, [], 0
        with torch.no_grad():
            for k, p in named:
                o = (p.data_ptr() - lo) // 4 if flat_ok else off
                self._views[k] = self.shadow[o:o + p.numel()].view_as(p)
                self._views[k].copy_(p.detach())
                off += p.numel()
                if k not in dead and p.numel():
                    self._live.append((p, self._views[k]))
        self._sig = tuple(p.data_ptr() for _, p in named)
        self._params = [p for _, p in named]
        # runs: live parameters that follow one another in memory, and whose shadows do
        self._runs = []
        for p, v in sorted(self._live, key=lambda pv: pv[0].data_ptr()):
            if self._runs:
                r = self._runs[-1]
                if r[0] + 4 * r[2] == p.data_ptr() and r[1] + 4 * r[2] == v.data_ptr():
                    r[2] += p.numel()
                    continue
            self._runs.append([p.data_ptr(), v.data_ptr(), p.numel()])

    def _check(self):
        if tuple(p.data_ptr() for p in self._params) != self._sig:
            raise RuntimeError("brats2019_amd.optim.EMA: the model's parameters moved (.cuda() / .to() / a replaced Parameter) since the EMA was built; build a new one")

    @torch.no_grad()
    def update(self):
        if self.swapped:
            raise RuntimeError("brats2019_amd.optim.EMA: update() while the averaged weights are swapped in; swap() back first")
        self._check()
        lib, stream = L.load(), L.stream()
        for w, e, n in self._runs:
            L.check(lib.ru_ema_update(e, w, n, self.decay, stream), "ru_ema_update")
        self.num_updates += 1
        self.last_launches = len(self._runs)

    @torch.no_grad()
    def swap(self):
        self._check()
        lib, stream = L.load(), L.stream()
        for w, e, n in self._runs:
            L.check(lib.ru_swap_f32(w, e, n, stream), "ru_swap_f32")
        self.swapped = not self.swapped
        if hasattr(self._net, "_unfreeze"):
            self._net._unfreeze()                    # the weights moved: packed copies of the old ones must not serve another forward
        self.last_launches = len(self._runs)

    def state_dict(self):
        if self.swapped:
            raise RuntimeError("brats2019_amd.optim.EMA: state_dict() while the averaged weights are swapped in; swap() back first")
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow": {k: v.detach().clone() for k, v in self._views.items()}}

    @torch.no_grad()
    def load_state_dict(self, state):
        shadow = state["shadow"]
        if set(shadow) != set(self._views):
            raise KeyError("EMA.load_state_dict: parameter names differ: %s" % sorted(set(shadow) ^ set(self._views))[:4])
        for k, v in self._views.items():
            v.copy_(shadow[k].to(device=v.device, dtype=torch.float32))
        self.decay = float(state["decay"])
        self.num_updates = int(state.get("num_updates", 0))


# ---------------------------------------------------------------------- float64 numpy restatements (test infrastructure)
def clip_coef_host(grads, max_norm):
    """(norm, coef) of `torch.nn.utils.clip_grad_norm_`: the 2-norm over all arrays, coef = min(1, max_norm / (norm + 1e-6)), in float64"""
    tot = 0.0
    for g in grads:
        g = np.asarray(g, dtype=np.float64)
        tot += float(np.sum(g * g))
    norm = math.sqrt(tot) if not math.isnan(tot) else float("nan")
    c = max_norm / (norm + 1e-6)
    return norm, (c if math.isnan(c) else min(1.0, c))


def sgd_step_host(w, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, coef=None):
    """`ru_sgd_step` in float64: returns (w, buf); `buf is None` is the first step (and stays None without momentum)"""
    lr, momentum, dampening, weight_decay = float(lr), float(momentum), float(dampening), float(weight_decay)
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    d = (g if coef is None else float(coef) * g) + weight_decay * w
    u = d
    if momentum != 0:
        buf = d.copy() if buf is None else momentum * np.asarray(buf, dtype=np.float64) + (1.0 - dampening) * d
        u = d + momentum * buf if nesterov else buf
    return w - lr * u, buf


def adamw_step_host(w, g, m, v, vmax, lr, b1, b2, eps, weight_decay, decoupled, step, coef=None):
    """`ru_adamw_step` in float64: returns (w, m, v, vmax); vmax None = no amsgrad; `step` is 1-based"""
    lr, b1, b2, eps, weight_decay = float(lr), float(b1), float(b2), float(eps), float(weight_decay)
    w, g, m, v = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v))
    gc = g if coef is None else float(coef) * g
    if decoupled:
        w = w * (1.0 - lr * weight_decay)
    else:
        gc = gc + weight_decay * w
    m = m + (gc - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * gc * gc
    vm = v
    if vmax is not None:
        vmax = vm = np.maximum(np.asarray(vmax, dtype=np.float64), v)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(vm) / math.sqrt(bc2) + eps
    return w - (lr / bc1) * (m / denom), m, v, vmax


def ema_host(ema, w, decay):
    """`ru_ema_update` in float64"""
    decay = float(decay)
    return decay * np.asarray(ema, dtype=np.float64) + (1.0 - decay) * np.asarray(w, dtype=np.float64)
