"""Drop-in for the reference's `loss` module on the hot path: `Dice_loss_joint(index, priority)` and
`BCE_Loss(index, bg_weight)` with the reference call convention `forward(x_list, y_list) -> 0-dim tensor`
(loss.py:64-79,98-122), backed by the two-phase HIP criterion kernels:

  phase 1  ru_criterion_sums : per-class sum(p*g), sum(p^2+g) and the BCE log-sum of this rank's shard
  (data-parallel: all-reduce the [2C+1] float64 sums -- the Dice sums couple the GLOBAL batch, loss.py:114-115)
  phase 2  ru_criterion_grad : d loss / d p from the global sums

`FusedCriterion` is the training criterion of main.py:126-128 -- (Dice + BCE(bg 1e-2)) / 2 -- in one pass of
each phase; the separate modules stay available so `criterion=[Dice_loss_joint(), BCE_Loss()]` lists keep working
(train.py:203-205).

The reference's other criteria on the same output -- MSE_Loss, CE_Loss, Dice1D, GDL_joint, sens_loss_joint, Dice_loss_separate
(loss.py:15-195) -- and lists of any of them go through the criterion-list kernels (csrc/criteria.hip): one moments pass, one
all-reduce of [7C+1] float64 totals, one evaluate launch, one gradient pass.

Beyond the reference: FocalLoss, TverskyLoss (focal-Tversky with gamma = 4/3) and TopKLoss (csrc/hardcrit.hip; definitions in
INTEGRATION.md), each its own autograd function, with float64 host restatements focal_host, tversky_host and topk_host.

BoundaryLoss and HausdorffDTLoss (csrc/boundary.hip; definitions in INTEGRATION.md) weigh each voxel by its exact Euclidean distance to the
boundary of the target (and, for the latter, of the thresholded prediction); the maps are made on the device in every step
(ops.signed_sqdist).  Host restatements: signed_sqdist_host, boundary_host, hddt_host.

LesionWiseDiceLoss (csrc/lesion_loss.hip; definition in INTEGRATION.md) is the training-side counterpart of ops.lesion_metrics: the blob
loss on Dice_loss_joint's Dice, one Dice per ground-truth lesion over the background and that lesion alone, averaged over lesions and then
over the (sample, channel) pairs that hold one.  The target is labelled on the device in every step (bit-parallel dilation, union-find
labelling, 64-bit fixed-point per-lesion sums: no float atomics, identical bytes from identical inputs).  Host restatement with scipy's
labelling: lesion_dice_host (lesion_labels_host).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops


def _all_reduce_sums(sums, group):
    import torch.distributed as dist
    if group is not False and dist.is_available() and dist.is_initialized():
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=None if group in (None, True) else group)
        return dist.get_world_size(None if group in (None, True) else group)
    return 1


_HAND_OVER_DEPTH = 0          # process-wide on purpose: autograd runs the backward of device tensors on its own thread


class hand_over_to_network:
    """`with loss.hand_over_to_network(): loss.backward()` -- what the Trainer loop does (train.py:210).  Inside it the backward of a
    criterion whose `pred` is DIRECTLY model.UNet's output does not write d(loss)/d(pred): it describes it to the network's autograd node,
    which forms it inside its first backward pass (ru_unet_backward_criterion).  The price is stated here rather than paid silently: within
    the context d(loss)/d(probs) does not exist as a tensor, so it must not be asked for (autograd.grad(loss, probs), retain_grad, hooks on
    the probabilities -- the two latter are detected and switch the hand-over off).  Outside the context every backward writes the gradient."""

    def __enter__(self):
        global _HAND_OVER_DEPTH
        _HAND_OVER_DEPTH += 1
        return self

    def __exit__(self, *exc):
        global _HAND_OVER_DEPTH
        _HAND_OVER_DEPTH -= 1
        return False


def _observed(pred):
    """somebody wants to SEE d(loss)/d(pred): retain_grad() or a tensor hook on the probabilities"""
    return bool(getattr(pred, "retains_grad", False)) or bool(getattr(pred, "_backward_hooks", None))


def _hand_over(pred, gt, sums, count, w_dice, w_bce, bg_weight, priority, gout):
    """Backward of a criterion whose `pred` is DIRECTLY the output of model.UNet's autograd node, inside `hand_over_to_network()`: instead of
    writing d(loss)/d(pred) (a 100 MB pass that the network's backward reads straight back), describe it to that node -- it forms the
    gradient inside its first pass (ru_unet_backward_criterion) -- and return a zero-stride placeholder of pred's shape.  Returns None when
    the hand-over does not apply (not enabled, another producer of pred, the probabilities are observed, d/d(input) wanted): the caller then
    writes the gradient.  The description never outlives the graph task that created it (a callback at its end clears it), so a backward
    that stops short of the network (autograd.grad(loss, probs)) cannot leak it into the next one."""
    node = pred.grad_fn
    if node is None or not getattr(node, "accepts_criterion", False) or type(node).__name__ != "_UNetFnBackward":
        return None
    if getattr(node, "pending_criterion", None) is not None:
        # a second criterion on the same probabilities (the list evaluated module by module): both gradients are written out -- the
        # first one's placeholder is zeros, so autograd's sum is this tensor
        pc, node.pending_criterion = node.pending_criterion, None
        first = ops.criterion_grad(pred, pc["target"], pc["sums"], pc["count"], pc["w_dice"], pc["w_bce"], pc["bg_weight"], pc["priority"]).mul_(pc["gout"].to(torch.float32))
        return first.add_(ops.criterion_grad(pred, gt, sums, count, w_dice, w_bce, bg_weight, priority).mul_(gout.to(torch.float32)))
    if _HAND_OVER_DEPTH <= 0 or _observed(pred):
        return None
    dummy = torch.zeros((), dtype=pred.dtype, device=pred.device).expand(pred.shape)
    node.pending_criterion = dict(target=gt, sums=sums, count=count, w_dice=w_dice, w_bce=w_bce, bg_weight=bg_weight, priority=priority, gout=gout, dummy=dummy)

    def _clear():                                     # end of THIS graph task: whether or not the network's node ran, nothing stays behind
        node.pending_criterion = None
    torch.autograd.Variable._execution_engine.queue_callback(_clear)
    return dummy


class _CriterionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, w_dice, w_bce, bg_weight, priority, group):
        sums = ops.criterion_sums(pred, gt, bg_weight)
        world = _all_reduce_sums(sums, group)
        count = float(pred.numel()) * world
        out = ops.criterion_losses(sums, count, priority, w_dice, w_bce)
        ctx.save_for_backward(pred, gt, sums)
        ctx.cfg = (count, w_dice, w_bce, bg_weight, priority)
        return out[0].to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt, sums = ctx.saved_tensors
        count, w_dice, w_bce, bg_weight, priority = ctx.cfg
        dp = _hand_over(pred, gt, sums, count, w_dice, w_bce, bg_weight, priority, gout)
        if dp is None:
            dp = ops.criterion_grad(pred, gt, sums, count, w_dice, w_bce, bg_weight, priority)
            dp.mul_(gout.to(dp.dtype))
        return dp, None, None, None, None, None, None


class _PairFn(torch.autograd.Function):
    """[Dice_loss_joint, BCE_Loss] evaluated together (train.py:203-205: loss = (dice + bce) / 2): ONE sums pass gives both values,
    ONE gradient pass gives d loss / d p.  Returns (loss, dice, bce); only `loss` is differentiable."""

    @staticmethod
    def forward(ctx, pred, gt, bg_weight, priority, group):
        sums = ops.criterion_sums(pred, gt, bg_weight)
        world = _all_reduce_sums(sums, group)
        count = float(pred.numel()) * world
        out = ops.criterion_losses(sums, count, priority, 0.5, 0.5).to(torch.float32)
        ctx.save_for_backward(pred, gt, sums)
        ctx.cfg = (count, bg_weight, priority)
        loss, dice, bce = out[0], out[1], out[2]
        ctx.mark_non_differentiable(dice, bce)
        return loss, dice, bce

    @staticmethod
    def backward(ctx, gout, _gd, _gb):
        pred, gt, sums = ctx.saved_tensors
        count, bg_weight, priority = ctx.cfg
        dp = _hand_over(pred, gt, sums, count, 0.5, 0.5, bg_weight, priority, gout)
        if dp is None:
            dp = ops.criterion_grad(pred, gt, sums, count, 0.5, 0.5, bg_weight, priority)
            dp.mul_(gout.to(dp.dtype))
        return dp, None, None, None, None


def fuse_criterion_list(criterion):
    """`criterion=[Dice_loss_joint(index, priority), BCE_Loss(index, bg_weight)]` (main.py:126-128, either order, same index) ->
    a callable `(x_list, y_list) -> (loss, [value per list entry])` with loss == sum(values) / 2 exactly as train.py:203-205 forms it,
    computed by one pass of each criterion phase instead of two.  Any other list of the device criteria below on one tensor index, with
    one `data_parallel` -> the same contract through the criterion-list kernels (`_fuse_terms`).  Anything else -> None (the caller
    evaluates the list as written)."""
    if not isinstance(criterion, (tuple, list)) or len(criterion) != 2:
        return _fuse_terms(criterion)
    kinds = [type(c) for c in criterion]
    if sorted(k.__name__ for k in kinds) != ["BCE_Loss", "Dice_loss_joint"] or not all(k in (Dice_loss_joint, BCE_Loss) for k in kinds):
        return _fuse_terms(criterion)
    dice = criterion[0] if kinds[0] is Dice_loss_joint else criterion[1]
    bce = criterion[0] if kinds[0] is BCE_Loss else criterion[1]
    if dice.index != bce.label_index or dice.data_parallel != bce.data_parallel:
        return None
    dice_first = kinds[0] is Dice_loss_joint

    def run(x, y):
        assert x[dice.index].shape == y[dice.index].shape                  # loss.py:71,107
        loss, d, b = _PairFn.apply(x[dice.index], y[dice.index], float(bce.bg_weight), float(dice.priority), dice.data_parallel)
        return loss, ([d, b] if dice_first else [b, d])
    return run


class _LossBase(nn.Module):
    """`data_parallel`: False (reference semantics, single process), or True / a process group: all-reduce the partial
    sums so that every rank forms the GLOBAL-batch loss the reference computes on GPU 0 under nn.DataParallel."""

    def __init__(self):
        super().__init__()
        self.data_parallel = False

    def _run(self, x, y, index, w_dice, w_bce, bg_weight, priority):
        assert x[index].shape == y[index].shape                   # loss.py:71,107
        return _CriterionFn.apply(x[index], y[index], w_dice, w_bce, bg_weight, priority, self.data_parallel)


class Dice_loss_joint(_LossBase):
    """loss.py:98-122: priority * (1 - mean_c 2(I_c+1e-6)/(U_c+2e-6)), sums over batch and space jointly."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        self.index = index
        self.priority = priority

    def forward(self, x, y):
        return self._run(x, y, self.index, 1.0, 0.0, 1.0, float(self.priority))


class BCE_Loss(_LossBase):
    """loss.py:64-79: -mean(g log(p+1e-6) + bg_weight (1-g) log(1+1e-6-p))."""

    def __init__(self, index=0, bg_weight=1):
        super().__init__()
        self.label_index = index
        self.bg_weight = bg_weight

    def forward(self, x, y):
        return self._run(x, y, self.label_index, 0.0, 1.0, float(self.bg_weight), 1.0)


class FusedCriterion(_LossBase):
    """(Dice_loss_joint(priority) + BCE_Loss(bg_weight)) / 2 == train.py:203-205 applied to main.py:126-128."""

    def __init__(self, index=0, priority=1, bg_weight=1e-2):
        super().__init__()
        self.index, self.priority, self.bg_weight = index, priority, bg_weight

    def forward(self, x, y):
        return self._run(x, y, self.index, 0.5, 0.5, float(self.bg_weight), float(self.priority))


# ------------------------------------------------------------------ criterion lists (loss.py:15-195; csrc/criteria.hip)
_LOG_KINDS = ("BCE_Loss", "CE_Loss")


def _index_of(c):
    return c.label_index if isinstance(c, (BCE_Loss, Dice1D)) else c.index


def _term(c, weight):
    """(kind, weight in the total, priority, bg_weight) of ru_crit_eval for a criterion module"""
    return (type(c).__name__, weight, float(getattr(c, "priority", 1)), float(getattr(c, "bg_weight", 1)))


class _TermsFn(torch.autograd.Function):
    """A list of criterion terms on one (pred, gt) pair: one moments pass, one all-reduce of the [7C+1] totals, one evaluate launch
    (values and the per-row gradient coefficients), and in backward one gradient pass that writes d(loss)/d(pred).  Returns
    (sum_t weight_t * value_t, value per term); only the first is differentiable."""

    @staticmethod
    def forward(ctx, pred, gt, terms, group):
        logs = any(t[0] in _LOG_KINDS for t in terms)
        moments = ops.crit_moments(pred, gt, _lib.CRIT_MASK_ALL if logs else _lib.CRIT_MASK_ALL & ~_lib.CRIT_MASK_LOGS)
        totals = ops.crit_reduce(moments)
        world = _all_reduce_sums(totals, group)
        values, coef = ops.crit_eval(totals, moments, terms, float(pred.numel()) * world, int(pred.shape[0]) * world)
        ctx.save_for_backward(pred, gt, coef)
        ctx.logs = logs
        out = values.to(torch.float32)
        rest = tuple(out[1:])
        ctx.mark_non_differentiable(*rest)
        return (out[0],) + rest

    @staticmethod
    def backward(ctx, gout, *_):
        pred, gt, coef = ctx.saved_tensors
        dp = ops.crit_grad(pred, gt, coef, gout, ctx.logs)
        return dp.to(pred.dtype), None, None, None


def _fuse_terms(criterion):
    """fuse_criterion_list for any list of 1..8 device criteria on the same tensor index with the same `data_parallel`:
    (loss, [value per entry]) with loss = sum(values) / len(list) (train.py:203-205).  A lone Dice_loss_joint or BCE_Loss is left as
    written: on its own it hands its gradient over to the network's backward, which this path does not."""
    if not isinstance(criterion, (tuple, list)) or not 1 <= len(criterion) <= _lib.CRIT_MAX_TERMS:
        return None
    if not all(type(c) in _TERM_CLASSES for c in criterion):
        return None
    if len(criterion) == 1 and type(criterion[0]) in (Dice_loss_joint, BCE_Loss):
        return None
    index, group = _index_of(criterion[0]), criterion[0].data_parallel
    if any(_index_of(c) != index or c.data_parallel != group for c in criterion):
        return None

    def run(x, y):
        assert x[index].shape == y[index].shape
        w = 1.0 / len(criterion)
        out = _TermsFn.apply(x[index], y[index], tuple(_term(c, w) for c in criterion), group)
        return out[0], list(out[1:])
    return run


class _TermLoss(_LossBase):
    """One of the reference's criteria as a one-term list.  Its backward writes d(loss)/d(pred) -- one more ~100 MB pass at
    4 x 3 x 128^3 -- and is not handed over to the network's backward (hand_over_to_network applies to Dice_loss_joint / BCE_Loss only);
    a list that mixes them gets the right gradient either way (model.py's "somebody else also used the probabilities" branch)."""

    def forward(self, x, y):
        index = _index_of(self)
        assert x[index].shape == y[index].shape
        return _TermsFn.apply(x[index], y[index], (_term(self, 1.0),), self.data_parallel)[0]


class MSE_Loss(_TermLoss):
    """loss.py:15-29: priority * mean((p - g)^2).  See _TermLoss for the cost of its backward."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        self.index = index
        self.priority = priority


class CE_Loss(_TermLoss):
    """loss.py:52-61: -mean(g log(p + 1e-6)).  See _TermLoss for the cost of its backward."""

    def __init__(self, index=0):
        super().__init__()
        self.index = index


class Dice1D(_TermLoss):
    """loss.py:81-96: 1 - 2 mean_c (sum_{n,v} pg + 1) / (sum_{n,v} (p + g) + 2).  See _TermLoss for the cost of its backward."""

    def __init__(self, label_index=0):
        super().__init__()
        self.label_index = label_index


class GDL_joint(_TermLoss):
    """loss.py:125-150: generalised Dice over channels 1.., w_c = 1 / sum_{n,v} g; priority * (1 - 2 sum w_c (I_c + 1) / sum w_c (U_c + 1)).
    A class absent from the (global) batch makes w_c infinite and the value and gradient NaN, as in the reference.  See _TermLoss for
    the cost of its backward."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        self.index = index
        self.priority = priority


class sens_loss_joint(_TermLoss):
    """loss.py:153-174: priority * (1 - mean_c (sum pg + 1) / (sum g + 1)), all channels.  See _TermLoss for the cost of its backward."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        self.index = index
        self.priority = priority


class Dice_loss_separate(_TermLoss):
    """loss.py:176-195: 1 - mean over samples and channels 1.. of (2 sum pg + 1) / (sum (p^2 + g) + 1).  `priority` is stored and, as in
    the reference, not used.  Under data parallelism the mean runs over the global batch.  See _TermLoss for the cost of its backward."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        self.index = index
        self.priority = priority


_TERM_CLASSES = (Dice_loss_joint, BCE_Loss, MSE_Loss, CE_Loss, Dice1D, GDL_joint, sens_loss_joint, Dice_loss_separate)


# ------------------------------------------------------------------ focal, Tversky, top-k (csrc/hardcrit.hip)
# Not in the reference's loss.py: the criteria people train with against lesion-wise scoring.  Each is its own autograd function that
# always writes d(loss)/d(pred), as _TermLoss does; none is in _TERM_CLASSES, so a list that contains one is evaluated as written.
class _FocalFn(torch.autograd.Function):
    """One sum pass, one all-reduce of the float64 sum, and in backward one gradient pass."""

    @staticmethod
    def forward(ctx, pred, gt, gamma, a1, a0w, group):
        total = ops.focal_sum(pred, gt, gamma, a1, a0w)
        world = _all_reduce_sums(total, group)
        count = float(pred.numel()) * world
        ctx.save_for_backward(pred, gt)
        ctx.cfg = (gamma, a1, a0w, count)
        return (total[0] / count).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt = ctx.saved_tensors
        gamma, a1, a0w, count = ctx.cfg
        return ops.focal_grad(pred, gt, gamma, a1, a0w, count, gout).to(pred.dtype), None, None, None, None, None


class _TverskyFn(torch.autograd.Function):
    """The moments pass of the criterion lists (no log moments), its reduce and all-reduce, one evaluate launch, and in backward one
    ru_crit_grad launch with the coefficients the evaluate wrote."""

    @staticmethod
    def forward(ctx, pred, gt, alpha, beta, gamma, smooth, priority, group):
        moments = ops.crit_moments(pred, gt, _lib.CRIT_MASK_ALL & ~_lib.CRIT_MASK_LOGS)
        totals = ops.crit_reduce(moments)
        _all_reduce_sums(totals, group)
        value, coef = ops.tversky_eval(totals, int(pred.shape[0]), int(pred.shape[1]), alpha, beta, gamma, smooth, priority)
        ctx.save_for_backward(pred, gt, coef)
        return value[0].to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt, coef = ctx.saved_tensors
        return ops.crit_grad(pred, gt, coef, gout, False).to(pred.dtype), None, None, None, None, None, None, None


def _topk_count(numel, k):
    """nnU-Net's rule: int(numel * k / 100), at least 1"""
    return max(1, int(numel * k / 100))


class _TopKFn(torch.autograd.Function):
    """An exact selection within this rank's shard (ru_topk_select), one all-reduce of the float64 value, and in backward one gradient
    pass over the stored keys."""

    @staticmethod
    def forward(ctx, pred, gt, k, bg_weight, group):
        K = _topk_count(pred.numel(), k)
        out, state, keys = ops.topk_select(pred, gt, K, bg_weight)
        value = out[:1].clone()
        world = _all_reduce_sums(value, group)
        ctx.save_for_backward(pred, gt, keys, state)
        ctx.cfg = (K, bg_weight, world)
        return (value[0] / world).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt, keys, state = ctx.saved_tensors
        K, bg_weight, world = ctx.cfg
        return ops.topk_grad(pred, gt, keys, state, K, bg_weight, world, gout).to(pred.dtype), None, None, None, None


class FocalLoss(_LossBase):
    """mean of -(a1 g (1-p)^gamma log(p+1e-6) + a0 bg_weight (1-g) p^gamma log((1+1e-6)-p)); a1 = alpha, a0 = 1 - alpha when alpha is given,
    else both 1.  gamma = 0, alpha = None is BCE_Loss.  0 < gamma < 1 is refused: its gradient is infinite at p = 0 or 1, which a
    saturated sigmoid reaches.  Under data parallelism the mean runs over the global batch."""

    def __init__(self, index=0, gamma=2.0, alpha=None, bg_weight=1):
        super().__init__()
        _check_focal(gamma, alpha, bg_weight)
        self.index, self.gamma, self.alpha, self.bg_weight = index, gamma, alpha, bg_weight

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        a1, a0 = (1.0, 1.0) if self.alpha is None else (float(self.alpha), 1.0 - float(self.alpha))
        return _FocalFn.apply(x[self.index], y[self.index], float(self.gamma), a1, a0 * float(self.bg_weight), self.data_parallel)


class TverskyLoss(_LossBase):
    """priority * mean_c (1 - TI_c)^(1/gamma), TI_c = (TP + s) / (TP + alpha FP + beta FN + s) with TP = sum pg, FP = sum p - TP,
    FN = sum g - TP over batch and space jointly, as Dice_loss_joint sums.  gamma = 4/3 is the focal-Tversky loss.  Under data
    parallelism the sums run over the global batch."""

    def __init__(self, index=0, alpha=0.3, beta=0.7, gamma=1.0, smooth=1.0, priority=1):
        super().__init__()
        _check_tversky(alpha, beta, gamma, smooth)
        self.index, self.alpha, self.beta, self.gamma, self.smooth, self.priority = index, alpha, beta, gamma, smooth, priority

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        return _TverskyFn.apply(x[self.index], y[self.index], float(self.alpha), float(self.beta), float(self.gamma), float(self.smooth),
                                float(self.priority), self.data_parallel)


class TopKLoss(_LossBase):
    """The mean of the K = max(1, int(numel * k / 100)) largest per-element BCE values -(g log(p+1e-6) + bg_weight (1-g) log((1+1e-6)-p)):
    nnU-Net's top-k rule on the region BCE.  The selection is exact and stays on the device; elements that tie at the threshold share
    the remaining weight equally.  Under data parallelism each rank selects within its own shard and the value is the mean over ranks."""

    def __init__(self, index=0, k=10.0, bg_weight=1):
        super().__init__()
        _check_topk(k, bg_weight)
        self.index, self.k, self.bg_weight = index, k, bg_weight

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        return _TopKFn.apply(x[self.index], y[self.index], float(self.k), float(self.bg_weight), self.data_parallel)


# ------------------------------------------------------------------ boundary and Hausdorff-DT losses (csrc/boundary.hip)
# Criteria on exact distance maps of the masks x > 0.5, made on the device in every step, so they follow zoom, rotation and elastic
# augmentation.  Like the classes above each always writes d(loss)/d(pred), and neither is in _TERM_CLASSES.
class _BoundaryFn(torch.autograd.Function):
    """The target's map (three transform passes), one sum pass, one all-reduce of the float64 sum, and in backward one gradient pass
    that reads the map alone."""

    @staticmethod
    def forward(ctx, pred, gt, priority, group):
        s_g = ops.signed_sqdist(gt)
        total = ops.boundary_sum(pred, s_g)
        world = _all_reduce_sums(total, group)
        count = float(pred.numel()) * world
        ctx.save_for_backward(s_g)
        ctx.cfg = (priority, count, pred.dtype)
        return (total[0] * (priority / count)).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        (s_g,) = ctx.saved_tensors
        priority, count, dtype = ctx.cfg
        return ops.boundary_grad(s_g, priority / count, gout).to(dtype), None, None, None


class _HausdorffDTFn(torch.autograd.Function):
    """The maps of the target and of the thresholded prediction, one sum pass, one all-reduce of the float64 sum, and in backward one
    gradient pass; the maps are constants under differentiation."""

    @staticmethod
    def forward(ctx, pred, gt, alpha, priority, group):
        s_p, s_g = ops.signed_sqdist(pred), ops.signed_sqdist(gt)
        total = ops.hddt_sum(pred, gt, s_p, s_g, alpha)
        world = _all_reduce_sums(total, group)
        count = float(pred.numel()) * world
        ctx.save_for_backward(pred, gt, s_p, s_g)
        ctx.cfg = (alpha, priority, count)
        return (total[0] * (priority / count)).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt, s_p, s_g = ctx.saved_tensors
        alpha, priority, count = ctx.cfg
        return ops.hddt_grad(pred, gt, s_p, s_g, alpha, priority / count, gout).to(pred.dtype), None, None, None, None


class BoundaryLoss(_LossBase):
    """priority * mean(p * phi_G): Kervadec et al.'s boundary loss.  phi_G is the level set of the target mask G = g > 0.5 of each
    (sample, channel): the Euclidean distance F to G outside it, -(F - 1) inside, 0 for an empty or full channel.  The
    value may be negative.  `priority` is read on every call, so an increasing schedule is an assignment between epochs.  Under data
    parallelism the mean runs over the global batch."""

    def __init__(self, index=0, priority=1):
        super().__init__()
        _check_boundary(priority)
        self.index, self.priority = index, priority

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        _check_boundary(self.priority)
        _check_extents("BoundaryLoss", x[self.index].shape)
        return _BoundaryFn.apply(x[self.index], y[self.index], float(self.priority), self.data_parallel)


class HausdorffDTLoss(_LossBase):
    """priority * mean((p - g)^2 (F_P^alpha + F_G^alpha)): Karimi & Salehi's distance-transform loss in the form of MONAI's
    HausdorffDTLoss.  F_P, F_G are the unsigned Euclidean distances to the boundary of P = p > 0.5 and G = g > 0.5 of each (sample,
    channel), 0 for an empty or full channel, and constants under differentiation.  `priority` is read on every call.  Under data
    parallelism the mean runs over the global batch."""

    def __init__(self, index=0, alpha=2.0, priority=1):
        super().__init__()
        _check_hddt(alpha, priority)
        self.index, self.alpha, self.priority = index, alpha, priority

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        _check_hddt(self.alpha, self.priority)
        _check_extents("HausdorffDTLoss", x[self.index].shape)
        return _HausdorffDTFn.apply(x[self.index], y[self.index], float(self.alpha), float(self.priority), self.data_parallel)


# ------------------------------------------------------------------ lesion-wise Dice loss (csrc/lesion_loss.hip)
# The target is labelled on the device in every step, so the lesions follow zoom, rotation and elastic augmentation.  Like the classes above
# it always writes d(loss)/d(pred) and is not in _TERM_CLASSES: a list that contains it is evaluated as written.
class _LesionDiceFn(torch.autograd.Function):
    """Labelling, one sum pass and one evaluate launch; one all-reduce of two float64 numbers (the sum of the pair losses and the number of
    pairs with a kept lesion); in backward one gradient pass that reads the global pair count on the device."""

    @staticmethod
    def forward(ctx, pred, gt, priority, dilation, min_volume, group):
        totals, _, labels, state = ops.lesion_loss_forward(pred, gt, dilation, min_volume)
        _all_reduce_sums(totals, group)
        ctx.save_for_backward(pred, gt, labels, state, totals)
        ctx.priority = priority
        value = torch.where(totals[1] > 0, totals[0] / totals[1].clamp(min=1.0), torch.zeros_like(totals[0]))
        return (value * priority).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        pred, gt, labels, state, totals = ctx.saved_tensors
        return ops.lesion_loss_grad(pred, gt, labels, state, totals, ctx.priority, gout).to(pred.dtype), None, None, None, None, None


class LesionWiseDiceLoss(_LossBase):
    """priority * the mean over the (sample, channel) pairs that hold a kept lesion of 1 - mean_i Dice_i: the blob loss (Kofler et al. 2022)
    on Dice_loss_joint's Dice.  The lesions of a pair are the parts of the target mask G = g > 0.5 inside each 26-connected component of G
    dilated `dilation` times by the 18-neighbour structure -- ops.lesion_metrics' grouping --, kept when larger than `min_volume` voxels;
    Dice_i = 2 (I + 1e-6) / (U + 2e-6) with I = sum p g, U = sum (p^2 + g) over the background (not G) and lesion i, the other lesions
    masked out.  The labelling is a constant under differentiation; voxels of a dropped lesion get no gradient; a batch without any
    kept lesion gives exactly 0.  Inputs are float32 [N, C, D, H, W] with FINITE values in [0, 1]; the target may be soft.
    `priority` is read on every call.  Under data parallelism the mean runs over the pairs of the global batch."""

    def __init__(self, index=0, priority=1, dilation=3, min_volume=0):
        super().__init__()
        _check_lesion_dice(priority, dilation, min_volume)
        self.index, self.priority, self.dilation, self.min_volume = index, priority, dilation, min_volume

    def forward(self, x, y):
        assert x[self.index].shape == y[self.index].shape
        _check_lesion_dice(self.priority, self.dilation, self.min_volume)
        _check_extents("LesionWiseDiceLoss", x[self.index].shape)
        return _LesionDiceFn.apply(x[self.index], y[self.index], float(self.priority), int(self.dilation), int(self.min_volume), self.data_parallel)


def _check_lesion_dice(priority, dilation, min_volume):
    import numbers
    if not _finite(priority):
        raise ValueError("LesionWiseDiceLoss: priority must be a finite number, got %r" % (priority,))
    if not (isinstance(dilation, numbers.Integral) and not isinstance(dilation, bool) and 0 <= dilation <= MAX_EXTENT):
        raise ValueError("LesionWiseDiceLoss: dilation must be an integer in [0, %d], got %r" % (MAX_EXTENT, dilation))
    if not (isinstance(min_volume, numbers.Integral) and not isinstance(min_volume, bool) and min_volume >= 0):
        raise ValueError("LesionWiseDiceLoss: min_volume must be an integer >= 0, got %r" % (min_volume,))


def _finite(v):
    import math
    import numbers
    return isinstance(v, numbers.Real) and math.isfinite(v)


def _check_boundary(priority):
    if not _finite(priority):
        raise ValueError("BoundaryLoss: priority must be a finite number, got %r" % (priority,))


def _check_hddt(alpha, priority):
    if not (_finite(alpha) and alpha > 0):
        raise ValueError("HausdorffDTLoss: alpha must be positive and finite, got %r" % (alpha,))
    if not _finite(priority):
        raise ValueError("HausdorffDTLoss: priority must be a finite number, got %r" % (priority,))


MAX_EXTENT = 512          # csrc/mask_bits.hpp: every axis of a distance-transformed volume


def _check_extents(who, shape):
    if len(shape) != 5:
        raise ValueError("%s: expected [N, C, D, H, W] tensors, got shape %s" % (who, tuple(shape)))
    if not all(1 <= int(v) <= MAX_EXTENT for v in shape[2:]):
        raise ValueError("%s: every axis of the volume must be in [1, %d], got %s" % (who, MAX_EXTENT, tuple(shape[2:])))


def _check_focal(gamma, alpha, bg_weight):
    if not (gamma == 0 or gamma >= 1):
        raise ValueError("FocalLoss: gamma must be 0 or at least 1 (0 < gamma < 1 has an infinite gradient at p = 0 or 1), got %r" % (gamma,))
    if alpha is not None and not 0 <= alpha <= 1:
        raise ValueError("FocalLoss: alpha must lie in [0, 1], got %r" % (alpha,))
    if not bg_weight >= 0:
        raise ValueError("FocalLoss: bg_weight must not be negative, got %r" % (bg_weight,))


def _check_tversky(alpha, beta, gamma, smooth):
    if not (alpha >= 0 and beta >= 0):
        raise ValueError("TverskyLoss: alpha and beta must not be negative, got %r, %r" % (alpha, beta))
    if not gamma >= 1:
        raise ValueError("TverskyLoss: gamma must be at least 1, got %r" % (gamma,))
    if not smooth > 0:
        raise ValueError("TverskyLoss: smooth must be positive, got %r" % (smooth,))


def _check_topk(k, bg_weight):
    if not 0 < k <= 100:
        raise ValueError("TopKLoss: k is a percentage in (0, 100], got %r" % (k,))
    if not bg_weight >= 0:
        raise ValueError("TopKLoss: bg_weight must not be negative, got %r" % (bg_weight,))


# ------------------------------------------------------------------ float64 host restatements (numpy only; nothing shared with the device path)
def _host_operands(p, g):
    """p, g as float64 and the two log arguments as BCE_Loss forms them: p + 1e-6 and (1 + 1e-6) - p in float32"""
    import numpy as np
    p32 = np.ascontiguousarray(np.asarray(p, dtype=np.float32))
    pe = (p32 + np.float32(1e-6)).astype(np.float64)
    qe = (np.float32(1.0 + 1e-6) - p32).astype(np.float64)
    return p32.astype(np.float64), np.asarray(g, dtype=np.float64), pe, qe


def focal_host(p, g, gamma=2.0, alpha=None, bg_weight=1):
    """FocalLoss in float64 -> (value, d value / d p)."""
    import numpy as np
    _check_focal(gamma, alpha, bg_weight)
    pd, gd, pe, qe = _host_operands(p, g)
    a1, a0 = (1.0, 1.0) if alpha is None else (float(alpha), 1.0 - float(alpha))
    a0 *= float(bg_weight)
    lp, lq, om = np.log(pe), np.log(qe), 1.0 - pd
    if gamma == 0:
        f = -(a1 * gd * lp + a0 * (1.0 - gd) * lq)
        df = -a1 * gd / pe + a0 * (1.0 - gd) / qe
    else:
        f = -(a1 * gd * om ** gamma * lp + a0 * (1.0 - gd) * pd ** gamma * lq)
        df = (-a1 * gd * (om ** gamma / pe - gamma * om ** (gamma - 1.0) * lp)
              - a0 * (1.0 - gd) * (gamma * pd ** (gamma - 1.0) * lq - pd ** gamma / qe))
    return float(f.mean()), df / f.size


def tversky_host(p, g, alpha=0.3, beta=0.7, gamma=1.0, smooth=1.0, priority=1):
    """TverskyLoss in float64 on [N, C, ...] arrays -> (value, d value / d p)."""
    import numpy as np
    _check_tversky(alpha, beta, gamma, smooth)
    pd, gd = np.asarray(p, dtype=np.float32).astype(np.float64), np.asarray(g, dtype=np.float64)
    C = pd.shape[1]
    axes = (0,) + tuple(range(2, pd.ndim))
    shape = (1, C) + (1,) * (pd.ndim - 2)
    tp = (pd * gd).sum(axis=axes)
    fp, fn = pd.sum(axis=axes) - tp, gd.sum(axis=axes) - tp
    den = tp + alpha * fp + beta * fn + smooth
    u = 1.0 - (tp + smooth) / den
    value = priority * np.mean(u ** (1.0 / gamma))
    o = -priority / C * (1.0 / gamma) * u ** (1.0 / gamma - 1.0)
    a = o * (den - (tp + smooth) * (1.0 - alpha - beta)) / den ** 2
    c = -o * alpha * (tp + smooth) / den ** 2
    return float(value), a.reshape(shape) * gd + c.reshape(shape)


def topk_host_threshold(p, g, k=10.0, bg_weight=1):
    """(l, K, t, n_gt, n_eq) of TopKLoss in float64: the per-element values, the count, the K-th largest value (NaN ranks above all, as in
    torch.topk), how many lie above it and how many equal it."""
    import numpy as np
    _check_topk(k, bg_weight)
    pd, gd, pe, qe = _host_operands(p, g)
    l = -(gd * np.log(pe) + float(bg_weight) * (1.0 - gd) * np.log(qe)) + 0.0
    K = _topk_count(l.size, k)
    flat = l.reshape(-1)
    t = float(np.partition(flat, flat.size - K)[flat.size - K])          # numpy orders NaN last, that is highest
    nans = int(np.isnan(flat).sum())
    if np.isnan(t):
        return l, K, t, 0, nans
    return l, K, t, int((flat > t).sum()) + nans, int((flat == t).sum())


def topk_host(p, g, k=10.0, bg_weight=1):
    """TopKLoss in float64 -> (value, d value / d p); ties at the threshold share the remaining weight equally."""
    import numpy as np
    l, K, t, n_gt, n_eq = topk_host_threshold(p, g, k, bg_weight)
    pd, gd, pe, qe = _host_operands(p, g)
    dl = float(bg_weight) * (1.0 - gd) / qe - gd / pe
    above = (l > t) | np.isnan(l)
    value = (l[above].sum() + (K - n_gt) * t) / K
    w = np.where(above, 1.0 / K, np.where(l == t, (K - n_gt) / (max(n_eq, 1) * K), 0.0))
    return float(value), dl * w


def _sqdist_to_host(sites):
    """exact squared Euclidean distance of every voxel of a [D, H, W] grid to the nearest True voxel of `sites`: the separable minimum
    f(i) = min_j f(j) + (i - j)^2 over each axis in turn, by brute force in int64"""
    import numpy as np
    f = np.where(sites, 0, 1 << 40).astype(np.int64)
    for axis in (2, 1, 0):
        i = np.arange(f.shape[axis], dtype=np.int64)
        cost = (i[:, None] - i[None, :]) ** 2
        f = np.moveaxis((np.moveaxis(f, axis, -1)[..., None, :] + cost).min(axis=-1), -1, axis)
    return f


def signed_sqdist_host(x):
    """ops.signed_sqdist in numpy (no scipy): x [..., D, H, W] -> int32 of x's shape, one mask x > 0.5 per leading index; + the squared
    distance to the mask outside it, - the squared distance to its complement inside, 0 everywhere for an empty or full mask."""
    import numpy as np
    x = np.asarray(x, dtype=np.float32)
    if x.ndim < 3:
        raise ValueError("expected a [..., D, H, W] array, got shape %s" % (x.shape,))
    if not all(1 <= v <= MAX_EXTENT for v in x.shape[-3:]):
        raise ValueError("signed_sqdist_host: every axis of the volume must be in [1, %d], got %s" % (MAX_EXTENT, x.shape[-3:]))
    masks = (x > np.float32(0.5)).reshape((-1,) + x.shape[-3:])
    out = np.zeros(masks.shape, dtype=np.int32)
    for k, m in enumerate(masks):
        if m.any() and not m.all():
            out[k] = np.where(m, -_sqdist_to_host(~m), _sqdist_to_host(m))
    return out.reshape(x.shape)


def _phi_host(s):
    import numpy as np
    F = np.sqrt(np.abs(s).astype(np.float64))
    return np.where(s > 0, F, np.where(s < 0, -(F - 1.0), 0.0))


def boundary_host(p, g, priority=1):
    """BoundaryLoss in float64 -> (value, d value / d p)."""
    import numpy as np
    _check_boundary(priority)
    pd = np.asarray(p, dtype=np.float32).astype(np.float64)
    _check_extents("boundary_host", pd.shape)
    phi = _phi_host(signed_sqdist_host(g))
    return float(priority * (pd * phi).sum() / pd.size), priority * phi / pd.size


def hddt_host(p, g, alpha=2.0, priority=1):
    """HausdorffDTLoss in float64 -> (value, d value / d p); the distance maps are constants."""
    import numpy as np
    _check_hddt(alpha, priority)
    pd, gd = np.asarray(p, dtype=np.float32).astype(np.float64), np.asarray(g, dtype=np.float32).astype(np.float64)
    _check_extents("hddt_host", pd.shape)
    w = (np.abs(signed_sqdist_host(p)).astype(np.float64) ** (alpha / 2.0) + np.abs(signed_sqdist_host(g)).astype(np.float64) ** (alpha / 2.0))
    d = pd - gd
    return float(priority * (d * d * w).sum() / pd.size), 2.0 * priority * d * w / pd.size


LESION_SCALE = 2.0 ** 35          # csrc/lesion_loss.hip: the fixed-point scale of the per-lesion sums


def lesion_labels_host(g, dilation=3):
    """The lesions of a [D, H, W] target as csrc/lesion_loss.hip labels them (scipy): -> (labels int32: -1 outside G = g > 0.5, else the
    smallest linear index of the voxel's 26-connected component of G dilated `dilation` times by the 18-neighbour structure; roots int64,
    ascending: one per component)."""
    import numpy as np
    from scipy import ndimage
    G = np.asarray(g, dtype=np.float32) > np.float32(0.5)
    Z = ndimage.binary_dilation(G, ndimage.generate_binary_structure(3, 2), iterations=int(dilation)) if int(dilation) > 0 else G
    comp, n = ndimage.label(Z, structure=np.ones((3, 3, 3), dtype=bool))
    flat = comp.reshape(-1)
    ids, first = np.unique(flat, return_index=True)                 # the first voxel of a component in raster order is its smallest index
    roots = first[ids > 0].astype(np.int64)
    assert len(roots) == n and np.all(np.diff(roots) > 0)           # scipy numbers the components in that order
    root_of = np.concatenate([[-1], roots])
    return np.where(G, root_of[comp], -1).astype(np.int32), roots


def lesion_dice_host(p, g, priority=1, dilation=3, min_volume=0, quantised=True):
    """LesionWiseDiceLoss in float64 with scipy's labelling -> (value, d value / d p as float64, table).  quantised=True forms the per-voxel
    integers of csrc/lesion_loss.hip (rint of the exact float64 products times 2^35), sums them as int64 and goes on from those sums, as the
    device does; quantised=False sums the float64 products themselves.  table[n][c] = dict(labels: int32 [D, H, W] in the device's
    convention, root, vol: the lesions in ascending root order (the dropped ones included), kept: bool per lesion, and with quantised
    qI, qU, qI0, qU0 as int64 (a lesion's own sums and the background's; ops.lesion_loss_table's columns), else I, U, I0, U0 as float64)."""
    import numpy as np
    _check_lesion_dice(priority, dilation, min_volume)
    p32, g32 = np.ascontiguousarray(np.asarray(p, dtype=np.float32)), np.ascontiguousarray(np.asarray(g, dtype=np.float32))
    _check_extents("lesion_dice_host", p32.shape)
    if p32.shape != g32.shape:
        raise ValueError("lesion_dice_host: shapes differ: %s, %s" % (p32.shape, g32.shape))
    pd, gd = p32.astype(np.float64), g32.astype(np.float64)
    N, C = pd.shape[:2]
    V = int(np.prod(pd.shape[2:]))
    table, pairs = [], []
    for n in range(N):
        table.append([])
        for c in range(C):
            labels, roots = lesion_labels_host(g32[n, c], dilation)
            lf, pf, gf = labels.reshape(-1), pd[n, c].reshape(-1), gd[n, c].reshape(-1)
            slot = np.searchsorted(roots, lf) + 1                    # 1 + the lesion's rank; 0 = background
            slot[lf < 0] = 0
            vol = np.bincount(slot, minlength=len(roots) + 1)[1:].astype(np.int64)
            if quantised:
                qi = np.rint(pf * gf * LESION_SCALE).astype(np.int64)
                qu = np.rint(pf * pf * LESION_SCALE).astype(np.int64) + np.rint(gf * LESION_SCALE).astype(np.int64)
                sI, sU = np.zeros(len(roots) + 1, dtype=np.int64), np.zeros(len(roots) + 1, dtype=np.int64)
                np.add.at(sI, slot, qi)
                np.add.at(sU, slot, qu)
                I = (sI[0] + sI[1:]).astype(np.float64) * (1.0 / LESION_SCALE)
                U = (sU[0] + sU[1:]).astype(np.float64) * (1.0 / LESION_SCALE)
                entry = dict(qI=sI[1:].copy(), qU=sU[1:].copy(), qI0=int(sI[0]), qU0=int(sU[0]))
            else:
                sI = np.bincount(slot, weights=pf * gf, minlength=len(roots) + 1)
                sU = np.bincount(slot, weights=pf * pf + gf, minlength=len(roots) + 1)
                I, U = sI[0] + sI[1:], sU[0] + sU[1:]
                entry = dict(I=sI[1:].copy(), U=sU[1:].copy(), I0=float(sI[0]), U0=float(sU[0]))
            kept = vol > int(min_volume)
            num, den = I + 1e-6, U + 2e-6
            dice, a, b = 2.0 * num / den, 2.0 / den, 4.0 * num / (den * den)
            L = int(kept.sum())
            sd = sa = sb = 0.0
            for i in np.nonzero(kept)[0]:                            # ascending root order
                sd, sa, sb = sd + float(dice[i]), sa + float(a[i]), sb + float(b[i])
            entry.update(labels=labels, root=roots, vol=vol, kept=kept)
            table[-1].append(entry)
            pairs.append((slot, np.where(kept, a, 0.0), np.where(kept, b, 0.0), sa, sb, L, 1.0 - sd / L if L else 0.0))
    M = sum(1 for q in pairs if q[5] >= 1)
    total = 0.0
    for q in pairs:
        if q[5] >= 1:
            total += q[6]
    grad = np.zeros((N * C, V), dtype=np.float64)
    for k, (slot, a, b, sa, sb, L, _) in enumerate(pairs):
        if M == 0 or L == 0:
            continue
        s = float(priority) / (M * float(L))
        av, bv = np.concatenate([[sa], a])[slot], np.concatenate([[sb], b])[slot]
        grad[k] = s * (bv * pd.reshape(N * C, V)[k] - av * gd.reshape(N * C, V)[k])
    value = float(priority) * total / M if M else 0.0
    return value, grad.reshape(pd.shape), table
