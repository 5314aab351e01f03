"""Thin tensor-level wrappers over the op entry points of libresunet_hip.so.  They allocate outputs and
scratch with torch (device memory plumbing) and pass raw pointers through the C-ABI; every function
documents the reference call site it stands in for.  Used by loss.py / train.py and by the per-op parity
tests; the network itself goes through engine.py (one C call per forward/backward)."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L

LEAKY_SLOPE = 1e-2


def _dims5(x):
    if x.dim() != 5:
        raise ValueError("expected an NCDHW tensor, got shape %s" % (tuple(x.shape),))
    return [int(v) for v in x.shape]


def _prep(t):
    L.require_gpu()
    if t is None:
        return None
    return t.contiguous().float() if (not t.is_contiguous() or t.dtype != torch.float32) else t


def conv3d(x, w, bias=None, precision="f32", out=None):
    """nn.Conv3d forward as built at model.py:72-73,336,348 (k=3,s=1,p=1), :361-363 (k=2,s=2), :393,401 (k=1).
    `precision`: "f32" (exact) or "bf16x3" (split-bf16, 3 MFMA products; k=3 only)."""
    x, w, bias = _prep(x), _prep(w), _prep(bias)
    lib = L.load()
    n, cin, d, h, wd = _dims5(x)
    cout, k = int(w.shape[0]), int(w.shape[2])
    if int(w.shape[1]) != cin:
        raise ValueError("weight expects %d input channels, input has %d" % (int(w.shape[1]), cin))
    out_sp = (d, h, wd) if k != 2 else (d // 2, h // 2, wd // 2)
    y = _out(out, (n, cout) + out_sp, x.device)
    ws = L.workspace(lib.ru_conv3d_workspace_bytes(n, cin, cout, d, h, wd, k), x.device)
    L.check(lib.ru_conv3d_fwd_p(L.f32(x), L.f32(w), L.ptr(bias, True), L.f32(y), n, cin, cout, d, h, wd, k, L.PRECISIONS[precision],
                                L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_fwd")
    return y


def conv3d_bwd_data(dy, w, in_spatial, precision="f32", out=None):
    """Data gradient of the conv above; `in_spatial` = (D,H,W) of the conv INPUT."""
    dy, w = _prep(dy), _prep(w)
    lib = L.load()
    n = int(dy.shape[0])
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    d, h, wd = [int(v) for v in in_spatial]
    dx = _out(out, (n, cin, d, h, wd), dy.device)
    ws = L.workspace(lib.ru_conv3d_workspace_bytes(n, cin, cout, d, h, wd, k), dy.device)
    L.check(lib.ru_conv3d_bwd_data_p(L.f32(dy), L.f32(w), L.f32(dx), n, cin, cout, d, h, wd, k, L.PRECISIONS[precision],
                                     L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_bwd_data")
    return dx


def conv3d_bwd_weight(x, dy, k, with_bias=False, precision="f32", out=None, out_db=None):
    """Weight (and bias) gradient of the conv above."""
    x, dy = _prep(x), _prep(dy)
    lib = L.load()
    n, cin, d, h, wd = _dims5(x)
    cout = int(dy.shape[1])
    dw = _out(out, (cout, cin, k, k, k), x.device)
    db = _out(out_db, (cout,), x.device) if with_bias else None
    ws = L.workspace(lib.ru_conv3d_workspace_bytes(n, cin, cout, d, h, wd, k), x.device)
    L.check(lib.ru_conv3d_bwd_weight_p(L.f32(x), L.f32(dy), L.f32(dw), L.ptr(db, True), n, cin, cout, d, h, wd, k, L.PRECISIONS[precision],
                                       L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_bwd_weight")
    return (dw, db) if with_bias else dw


def conv3d_splitk(x, w, bias=None, ksplit=0, out=None):
    """The exact-f32 k = 3 forward in its split-K form (ru_conv3d_fwd_splitk), as the engine runs its small exact-f32 shapes: `ksplit` partial tensors over
    slices of the 8-channel input chunks, summed in slice order.  ksplit = 0: the factor of ncdhw_conv3_inst(...).ksplit; 1: the plain launch."""
    x, w, bias = _prep(x), _prep(w), _prep(bias)
    lib = L.load()
    n, cin, d, h, wd = _dims5(x)
    cout = int(w.shape[0])
    if int(w.shape[1]) != cin or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError("expected a [Cout, %d, 3, 3, 3] weight, got %s" % (cin, tuple(w.shape)))
    y = _out(out, (n, cout, d, h, wd), x.device)
    ws = L.workspace(lib.ru_conv3d_fwd_splitk_workspace_bytes(n, cin, cout, d, h, wd, int(ksplit)), x.device)
    L.check(lib.ru_conv3d_fwd_splitk(L.f32(x), L.f32(w), L.ptr(bias, True), L.f32(y), n, cin, cout, d, h, wd, int(ksplit),
                                     L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_fwd_splitk")
    return y


# What a launch of the NCDHW family chooses: host-only queries of the functions the launchers switch on (no device needed).
Conv3F32Inst = collections.namedtuple("Conv3F32Inst", "tz ty kc nt ksplit")
Wgrad3Inst = collections.namedtuple("Wgrad3Inst", "kernel ot ct x16 dy16 nbx ntile")
NcdhwWgrad1Inst = collections.namedtuple("NcdhwWgrad1Inst", "ot ct nbx nchunk")
CONV1_ROUTES = ("conv1_mfma_kernel", "conv1_kernel<1,4>", "conv1_kernel<4,16>")


def ncdhw_conv3_inst(n, cin, cout, d, h, w):
    """conv3_f32_kernel<tz, ty, kc, nt> of an exact-f32 k = 3 convolution of cin -> cout channels (the data gradient: the forward's cout -> cin) and the split
    factor the engine takes for the shape (ru_conv3_f32_inst)."""
    p = L.load().ru_conv3_f32_inst(n, cin, cout, d, h, w)
    if p < 0:
        raise ValueError("ru_conv3_f32_inst refused the shape")
    return Conv3F32Inst(p & 15, (p >> 4) & 15, (p >> 8) & 15, (p >> 12) & 15, p >> 16)


def ncdhw_wgrad3_inst(n, cin, cout, d, h, w, precision="f32", x_c16=False, dy_c16=False):
    """the kernel of the k = 3 weight gradient (ru_wgrad3_inst): kernel "f32" (wgrad3_f32_kernel), "sb" (wgrad3_sb_kernel) or "tr" (the transpose-read kernel)."""
    out = (C.c_int * 7)()
    L.check(L.load().ru_wgrad3_inst(n, cin, cout, d, h, w, L.PRECISIONS[precision], int(x_c16) | (int(dy_c16) << 1), out), "ru_wgrad3_inst")
    return Wgrad3Inst(("f32", "sb", "tr")[out[0]], out[1], out[2], bool(out[3]), bool(out[4]), out[5], out[6])


def ncdhw_conv1_route(n, cin, cout, v):
    """the kernel of the pointwise launch behind k = 1 and k = 2 (ru_conv1_inst): one of CONV1_ROUTES."""
    r = L.load().ru_conv1_inst(n, cin, cout, v)
    if r < 0:
        raise ValueError("ru_conv1_inst refused the shape")
    return CONV1_ROUTES[r]


def ncdhw_wgrad1_inst(n, cin, cout, v):
    """wgrad1_f32_kernel<ot, ct> of the k = 1 / k = 2 weight gradient on NCDHW tensors and its walk: nbx workgroups per channel group over n * nchunk chunks."""
    out = (C.c_int * 3)()
    L.check(L.load().ru_wgrad1_inst(n, cin, cout, v, out), "ru_wgrad1_inst")
    return NcdhwWgrad1Inst(out[0] & 15, (out[0] >> 4) & 15, out[1], out[2])


def group_norm(x, gamma, beta, groups=8, eps=1e-5, slope=1.0, residual=None):
    """nn.GroupNorm(8, C) (model.py:95-96,338) + LeakyReLU(slope) (model.py:93-94; 1.0 = none) + optional
    residual add (model.py:115).  Returns (y, mean[N*G], rstd[N*G])."""
    x, gamma, beta, residual = _prep(x), _prep(gamma), _prep(beta), _prep(residual)
    lib = L.load()
    n, c = int(x.shape[0]), int(x.shape[1])
    v = x.numel() // (n * c)
    y = torch.empty_like(x)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = L.workspace(lib.ru_groupnorm_workspace_bytes(n, c, v), x.device)
    L.check(lib.ru_groupnorm_fwd(L.f32(x), L.f32(gamma), L.f32(beta), L.ptr(residual, True), L.f32(y), L.f32(mean), L.f32(rstd),
                                 n, c, v, groups, eps, slope, L.ptr(ws), ws.numel(), L.stream()), "ru_groupnorm_fwd")
    return y, mean, rstd


def group_norm_bwd(x, gamma, beta, mean, rstd, dy, groups=8, slope=1.0):
    """Backward of lrelu(GN(x)); returns (dx, dgamma, dbeta)."""
    x, gamma, beta, dy = _prep(x), _prep(gamma), _prep(beta), _prep(dy)
    lib = L.load()
    n, c = int(x.shape[0]), int(x.shape[1])
    v = x.numel() // (n * c)
    dx = torch.empty_like(x)
    dgamma = torch.empty_like(gamma)
    dbeta = torch.empty_like(beta)
    ws = L.workspace(lib.ru_groupnorm_workspace_bytes(n, c, v), x.device)
    L.check(lib.ru_groupnorm_bwd(L.f32(x), L.f32(gamma), L.f32(beta), L.f32(mean), L.f32(rstd), L.f32(dy), L.f32(dx), L.f32(dgamma),
                                 L.f32(dbeta), n, c, v, groups, slope, L.ptr(ws), ws.numel(), L.stream()), "ru_groupnorm_bwd")
    return dx, dgamma, dbeta


def leaky_relu(x, slope=LEAKY_SLOPE):
    x = _prep(x)
    y = torch.empty_like(x)
    L.check(L.load().ru_leaky_relu_fwd(L.f32(x), L.f32(y), x.numel(), slope, L.stream()), "ru_leaky_relu_fwd")
    return y


def leaky_relu_bwd(y, dy, slope=LEAKY_SLOPE):
    y, dy = _prep(y), _prep(dy)
    dx = torch.empty_like(y)
    L.check(L.load().ru_leaky_relu_bwd(L.f32(y), L.f32(dy), L.f32(dx), y.numel(), slope, L.stream()), "ru_leaky_relu_bwd")
    return dx


def _out(out, shape, device):
    """the output tensor of an op that takes one (`out`: a caller's contiguous float32 tensor of that shape, e.g. prefilled with NaN)"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape %s" % (tuple(shape),))
    return out


def upsample2x(x, out=None):
    """model.Trilinear(scale=2) (model.py:7-14)."""
    x = _prep(x)
    n, c, d, h, w = _dims5(x)
    y = _out(out, (n, c, 2 * d, 2 * h, 2 * w), x.device)
    L.check(L.load().ru_upsample2x_trilinear_fwd(L.f32(x), L.f32(y), n, c, d, h, w, L.stream()), "ru_upsample2x_trilinear_fwd")
    return y


def upsample2x_bwd(dy, out=None):
    dy = _prep(dy)
    n, c, d2, h2, w2 = _dims5(dy)
    dx = _out(out, (n, c, d2 // 2, h2 // 2, w2 // 2), dy.device)
    L.check(L.load().ru_upsample2x_trilinear_bwd(L.f32(dy), L.f32(dx), n, c, d2 // 2, h2 // 2, w2 // 2, L.stream()),
            "ru_upsample2x_trilinear_bwd")
    return dx


def sigmoid(x):
    x = _prep(x)
    y = torch.empty_like(x)
    L.check(L.load().ru_sigmoid_fwd(L.f32(x), L.f32(y), x.numel(), L.stream()), "ru_sigmoid_fwd")
    return y


def criterion_sums(p, g, bg_weight=1e-2):
    """Phase 1 of the criterion (loss.py:76-79,114-115): float64 device tensor [2C+1] =
    (sum p*g per class, sum p^2+g per class, BCE log-sum) over THIS shard, no epsilons."""
    p, g = _prep(p), _prep(g)
    if p.shape != g.shape:
        raise AssertionError("prediction/target shape mismatch")      # loss.py:71,107 assert
    lib = L.load()
    n, c = int(p.shape[0]), int(p.shape[1])
    v = p.numel() // (n * c)
    sums = torch.empty(2 * c + 1, dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_criterion_workspace_bytes(n, c, v), p.device)
    L.check(lib.ru_criterion_sums(L.f32(p), L.f32(g), L.ptr(sums), n, c, v, bg_weight, L.ptr(ws), ws.numel(), L.stream()),
            "ru_criterion_sums")
    return sums


def criterion_grad(p, g, sums, count, w_dice=0.5, w_bce=0.5, bg_weight=1e-2, priority=1.0):
    """Phase 2: d(w_dice*Dice + w_bce*BCE)/dp from GLOBAL sums / element count."""
    p, g = _prep(p), _prep(g)
    n, c = int(p.shape[0]), int(p.shape[1])
    v = p.numel() // (n * c)
    dp = torch.empty_like(p)
    L.check(L.load().ru_criterion_grad(L.f32(p), L.f32(g), L.ptr(sums), float(count), w_dice, w_bce, bg_weight, priority,
                                       L.f32(dp), n, c, v, L.stream()), "ru_criterion_grad")
    return dp


def head_grad(p, dp=None, *, target=None, sums=None, count=None, w_dice=0.5, w_bce=0.5, bg_weight=1e-2, priority=1.0, generic=False, with_dlog=False):
    """The head of the backward pass, one route at a time (ru_head_grad_l): d = dp * p * (1 - p) (model.py:431) and db[c] = sum over n, v of d (model.py:348)
    from p [N, C, ...].  Returns (d4 [N, V, 4], db [C], dlog [N, C, V]), each prefilled with NaN, None where the route does not write it.
    dp given: the 4-channel pass (dlog only with with_dlog, by the flat sigmoid backward behind it).  dp None: the same pass with the criterion's gradient
    formed on the way from (target, sums, count -- default p.numel()) as criterion_grad forms it.  generic: the flat sigmoid backward into dlog, then the bias
    gradient over it (any C and V; no d4)."""
    p, dp, target = _prep(p), _prep(dp), _prep(target)
    lib = L.load()
    n, c, v = _rows(p)
    route = 2 if generic else (0 if dp is not None else 1)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=p.device)
    d4 = None if route == 2 else new(n, v, 4)
    dlog = new(n, c, v) if (route == 2 or (route == 0 and with_dlog)) else None
    db = new(c)
    ws = L.workspace(lib.ru_head_grad_l_workspace_bytes(n, c, v, route), p.device)
    L.check(lib.ru_head_grad_l(L.f32(p), L.ptr(dp, True), L.ptr(target, True), L.ptr(sums, True), float(count if count is not None else p.numel()),
                               w_dice, w_bce, bg_weight, priority, L.ptr(d4, True), L.f32(db), L.ptr(dlog, True), n, c, v, route,
                               L.ptr(ws), ws.numel(), L.stream()), "ru_head_grad_l")
    return d4, db, dlog


def criterion_losses(sums, count, priority=1.0, w_dice=0.5, w_bce=0.5):
    """float64 DEVICE tensor [3] = (w_dice*dice + w_bce*bce, dice, bce) from (global) sums -- one launch, no host sync."""
    c = (sums.numel() - 1) // 2
    out = torch.empty(3, dtype=torch.float64, device=sums.device)
    L.check(L.load().ru_criterion_value_device(L.ptr(sums), c, float(count), float(priority), float(w_dice), float(w_bce), L.ptr(out), L.stream()),
            "ru_criterion_value_device")
    return out


def criterion_value(sums, count, priority=1.0):
    """(dice, bce) as float64 0-dim DEVICE tensors from (global) sums -- no host sync."""
    out = criterion_losses(sums, count, priority)
    return out[1], out[2]                                                            # loss.py:114-122, loss.py:79


def _rows(p):
    n, c = int(p.shape[0]), int(p.shape[1])
    return n, c, p.numel() // max(n * c, 1)


def crit_moments(p, g, mask=L.CRIT_MASK_ALL):
    """Criterion lists, pass 1 (loss.py:15-195): float64 device tensor [N, C, 7] of per-row moments over THIS shard --
    sum pg, sum p^2, sum p, sum g, sum g log(p+1e-6), sum (1-g) log((1+1e-6)-p), sum (p-g)^2.  Without a bit of
    `CRIT_MASK_LOGS` in `mask` the two log moments are skipped (written as 0)."""
    p, g = _prep(p), _prep(g)
    if p.shape != g.shape:
        raise AssertionError("prediction/target shape mismatch")
    lib = L.load()
    n, c, v = _rows(p)
    m = torch.empty((n, c, L.CRIT_MOMENTS), dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_crit_moments_workspace_bytes(n, c, v), p.device)
    L.check(lib.ru_crit_moments(L.f32(p), L.f32(g), n, c, v, int(mask), L.ptr(m), L.ptr(ws), ws.numel(), L.stream()), "ru_crit_moments")
    return m


def crit_reduce(moments):
    """[C*7 + 1] float64: per-channel totals over the shard's samples, then the sum of Dice_loss_separate's per-sample terms -- the
    buffer that is all-reduced across data-parallel ranks."""
    n, c = int(moments.shape[0]), int(moments.shape[1])
    out = torch.empty(c * L.CRIT_MOMENTS + 1, dtype=torch.float64, device=moments.device)
    L.check(L.load().ru_crit_reduce(L.ptr(moments), n, c, L.ptr(out), L.stream()), "ru_crit_reduce")
    return out


def crit_eval(totals, moments, terms, count, n_global):
    """terms: list of (kind name, weight, priority, bg_weight).  -> (values float64 [1 + len(terms)] = (weighted total, value per term),
    coef float32 [N, C, 5] = the per-row coefficients of d(total)/dp), from the (all-reduced) totals and this shard's moments."""
    n, c = int(moments.shape[0]), int(moments.shape[1])
    arr = (L.CritTerm * max(len(terms), 1))(*[L.CritTerm(L.CRIT_KINDS[k], float(w), float(pr), float(bg)) for k, w, pr, bg in terms])
    values = torch.empty(1 + len(terms), dtype=torch.float64, device=moments.device)
    coef = torch.empty((n, c, 5), dtype=torch.float32, device=moments.device)
    L.check(L.load().ru_crit_eval(L.ptr(totals), L.ptr(moments), n, c, float(count), float(n_global), C.cast(arr, C.c_void_p), len(terms),
                                  L.ptr(values), L.ptr(coef), L.stream()), "ru_crit_eval")
    return values, coef


def crit_grad(p, g, coef, scale=None, with_logs=True):
    """Criterion lists, pass 2: dp = a g + b p + c + d g/(p+1e-6) + e (1-g)/((1+1e-6)-p) with a..e = coef[n, c], times `scale`
    (a float32 device scalar, autograd's incoming gradient) when given.  with_logs=False skips d and e (no CE / BCE term)."""
    p, g = _prep(p), _prep(g)
    n, c, v = _rows(p)
    dp = torch.empty_like(p)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_crit_grad(L.f32(p), L.f32(g), L.ptr(coef), L.ptr(sc, True), n, c, v, int(bool(with_logs)), L.f32(dp), L.stream()),
            "ru_crit_grad")
    return dp


def _pair(p, g):
    p, g = _prep(p), _prep(g)
    if p.shape != g.shape:
        raise AssertionError("prediction/target shape mismatch")
    return p, g


def focal_sum(p, g, gamma, a1, a0w):
    """Focal loss, pass 1 (csrc/hardcrit.hip): float64 device tensor [1] = the sum over THIS shard of
    -(a1 g (1-p)^gamma log(p+1e-6) + a0w (1-g) p^gamma log((1+1e-6)-p)); the loss is the (all-reduced) sum over the global count."""
    p, g = _pair(p, g)
    lib = L.load()
    out = torch.empty(1, dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_focal_workspace_bytes(p.numel()), p.device)
    L.check(lib.ru_focal_sum(L.f32(p), L.f32(g), p.numel(), float(gamma), float(a1), float(a0w), L.ptr(out), L.ptr(ws), ws.numel(), L.stream()),
            "ru_focal_sum")
    return out


def focal_grad(p, g, gamma, a1, a0w, count, scale=None):
    """Focal loss, pass 2: dp = df/dp / count, times `scale` (a float32 device scalar, autograd's incoming gradient) when given."""
    p, g = _pair(p, g)
    dp = torch.empty_like(p)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_focal_grad(L.f32(p), L.f32(g), p.numel(), float(gamma), float(a1), float(a0w), float(count), L.ptr(sc, True), L.f32(dp),
                                   L.stream()), "ru_focal_grad")
    return dp


def tversky_eval(totals, n, c, alpha, beta, gamma, smooth, priority):
    """From crit_reduce's (all-reduced) totals -> (value float64 [1], coef float32 [n, c, 5] for crit_grad(..., with_logs=False))."""
    value = torch.empty(1, dtype=torch.float64, device=totals.device)
    coef = torch.empty((n, c, 5), dtype=torch.float32, device=totals.device)
    L.check(L.load().ru_tversky_eval(L.ptr(totals), int(n), int(c), float(alpha), float(beta), float(gamma), float(smooth), float(priority),
                                     L.ptr(value), L.ptr(coef), L.stream()), "ru_tversky_eval")
    return value, coef


def topk_select(p, g, K, bg_weight=1.0):
    """The K largest per-element BCE values l of THIS shard, exactly (radix select on the device, no host sync) ->
    (out float64 [2] = (their mean, the threshold t), state int64 [4] = (key of t, K - n_gt, n_gt, n_eq), keys int32 [numel]: l stored
    once as order-preserving keys, which topk_grad reads back)."""
    p, g = _pair(p, g)
    lib = L.load()
    n = p.numel()
    keys = torch.empty(n, dtype=torch.int32, device=p.device)
    state = torch.empty(4, dtype=torch.int64, device=p.device)
    out = torch.empty(2, dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_topk_workspace_bytes(n), p.device)
    L.check(lib.ru_topk_select(L.f32(p), L.f32(g), n, int(K), float(bg_weight), L.ptr(keys), L.ptr(state), L.ptr(out), L.ptr(ws), ws.numel(),
                               L.stream()), "ru_topk_select")
    return out, state, keys


def topk_grad(p, g, keys, state, K, bg_weight=1.0, world=1, scale=None):
    """d(mean of the K largest l)/dp / world: dl/dp / K above the threshold, dl/dp (K - n_gt) / (n_eq K) at it, 0 below; times `scale`."""
    p, g = _pair(p, g)
    dp = torch.empty_like(p)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_topk_grad(L.f32(p), L.f32(g), L.ptr(keys), L.ptr(state), p.numel(), int(K), float(bg_weight), float(world),
                                  L.ptr(sc, True), L.f32(dp), L.stream()), "ru_topk_grad")
    return dp


def signed_sqdist(x):
    """Exact signed squared Euclidean distance maps (csrc/boundary.hip): x float32 [..., D, H, W], one mask x > 0.5 per leading index ->
    int32 tensor of x's shape: + the squared distance to the nearest voxel of the mask outside it, - the squared distance to the nearest
    voxel not in the mask inside it, 0 everywhere for an empty or full mask.  Unit spacing, every axis at most 512; no host sync."""
    x = _prep(x)
    if x.dim() < 3:
        raise ValueError("expected a [..., D, H, W] tensor, got shape %s" % (tuple(x.shape),))
    d, h, w = [int(v) for v in x.shape[-3:]]
    if max(d, h, w) > 512 or min(d, h, w) < 1:
        raise ValueError("signed_sqdist: every axis of the volume must be in [1, 512], got %s" % ((d, h, w),))
    items = x.numel() // (d * h * w)
    lib = L.load()
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    ws = L.workspace(lib.ru_signed_sqdist_workspace_bytes(items, d, h, w), x.device)
    L.check(lib.ru_signed_sqdist(L.f32(x), items, d, h, w, L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), "ru_signed_sqdist")
    return out


def _map_of(s, like):
    if s.dtype != torch.int32 or s.shape != like.shape or not s.is_contiguous():
        raise ValueError("a distance map must be a contiguous int32 tensor of the prediction's shape (ops.signed_sqdist)")
    return s


def boundary_sum(p, s_g):
    """Boundary loss, pass 1: float64 device tensor [1] = the sum over THIS shard of p * phi_G, phi formed from the int32 map s_g =
    signed_sqdist(g); the loss is priority * the (all-reduced) sum / the global count."""
    p = _prep(p)
    s_g = _map_of(s_g, p)
    lib = L.load()
    out = torch.empty(1, dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_boundary_workspace_bytes(p.numel()), p.device)
    L.check(lib.ru_boundary_sum(L.f32(p), L.ptr(s_g), p.numel(), L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), "ru_boundary_sum")
    return out


def boundary_grad(s_g, coef, scale=None):
    """Boundary loss, pass 2: dp = coef * phi_G (coef = priority / global count), times `scale` (a float32 device scalar) when given."""
    if s_g.dtype != torch.int32 or not s_g.is_contiguous():
        raise ValueError("a distance map must be a contiguous int32 tensor (ops.signed_sqdist)")
    dp = torch.empty(s_g.shape, dtype=torch.float32, device=s_g.device)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_boundary_grad(L.ptr(s_g), s_g.numel(), float(coef), L.ptr(sc, True), L.f32(dp), L.stream()), "ru_boundary_grad")
    return dp


def hddt_sum(p, g, s_p, s_g, alpha):
    """Hausdorff-DT loss, pass 1: float64 device tensor [1] = the sum over THIS shard of (p - g)^2 (F_P^alpha + F_G^alpha) with the
    unsigned distances F = sqrt(|s|) of the int32 maps s_p = signed_sqdist(p), s_g = signed_sqdist(g)."""
    p, g = _pair(p, g)
    s_p, s_g = _map_of(s_p, p), _map_of(s_g, p)
    lib = L.load()
    out = torch.empty(1, dtype=torch.float64, device=p.device)
    ws = L.workspace(lib.ru_boundary_workspace_bytes(p.numel()), p.device)
    L.check(lib.ru_hddt_sum(L.f32(p), L.f32(g), L.ptr(s_p), L.ptr(s_g), p.numel(), float(alpha), L.ptr(out), L.ptr(ws), ws.numel(), L.stream()),
            "ru_hddt_sum")
    return out


def hddt_grad(p, g, s_p, s_g, alpha, coef, scale=None):
    """Hausdorff-DT loss, pass 2: dp = coef * 2 (p - g) (F_P^alpha + F_G^alpha) (coef = priority / global count), times `scale`."""
    p, g = _pair(p, g)
    s_p, s_g = _map_of(s_p, p), _map_of(s_g, p)
    dp = torch.empty_like(p)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_hddt_grad(L.f32(p), L.f32(g), L.ptr(s_p), L.ptr(s_g), p.numel(), float(alpha), float(coef), L.ptr(sc, True), L.f32(dp),
                                  L.stream()), "ru_hddt_grad")
    return dp


def _lesion_loss_args(who, p, g, dilation=0, min_volume=0):
    if p.dim() != 5 or tuple(p.shape) != tuple(g.shape):
        raise ValueError("%s: expected two [N, C, D, H, W] tensors of one shape, got %s and %s" % (who, tuple(p.shape), tuple(g.shape)))
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        raise ValueError("%s: expected float32 tensors, got %s and %s" % (who, p.dtype, g.dtype))
    if not all(1 <= int(v) <= 512 for v in p.shape[2:]) or int(p.shape[0]) < 1 or int(p.shape[1]) < 1:
        raise ValueError("%s: every axis of the volume must be in [1, 512], got %s" % (who, tuple(p.shape)))
    if int(dilation) != dilation or int(min_volume) != min_volume or int(dilation) < 0 or int(min_volume) < 0:
        raise ValueError("%s: dilation %r and min_volume %r must be integers >= 0" % (who, dilation, min_volume))
    return _prep(p), _prep(g)


def _lesion_loss_state(n, c, d, h, w):
    import ctypes
    off = (ctypes.c_size_t * 5)()
    nbytes = L.load().ru_lesion_loss_state_bytes(n, c, d, h, w, off)
    if not nbytes:
        raise ValueError("lesion loss: unsupported shape %s" % ((n, c, d, h, w),))
    return int(nbytes), [int(v) for v in off]


def lesion_loss_forward(p, g, dilation=3, min_volume=0):
    """Lesion-wise Dice loss, pass 1 (csrc/lesion_loss.hip; include/resunet_hip.h states the definition): p, g float32 [N, C, D, H, W] with
    finite values in [0, 1] -> (totals float64 [2] = (the sum of the pair losses of THIS shard's pairs with a kept lesion, their number),
    stats int64 [N, C, 2] = (lesions, kept lesions), labels int32 of p's shape: -1 outside G = g > 0.5, else the smallest linear index of
    the voxel's component of the dilated target, state: an opaque uint8 tensor for lesion_loss_grad and lesion_loss_table).  The loss is
    priority * totals[0] / totals[1] of the all-reduced totals (0 when totals[1] is 0).  No host sync; two calls give identical bytes."""
    p, g = _lesion_loss_args("lesion_loss_forward", p, g, dilation, min_volume)
    n, c, d, h, w = _dims5(p)
    lib = L.load()
    nstate, _ = _lesion_loss_state(n, c, d, h, w)
    totals = torch.empty(2, dtype=torch.float64, device=p.device)
    stats = torch.empty((n, c, 2), dtype=torch.int64, device=p.device)
    labels = torch.empty(p.shape, dtype=torch.int32, device=p.device)
    state = torch.empty(nstate, dtype=torch.uint8, device=p.device)
    ws = L.workspace(lib.ru_lesion_loss_workspace_bytes(n, c, d, h, w), p.device)
    L.check(lib.ru_lesion_loss_forward(L.f32(p), L.f32(g), n, c, d, h, w, int(dilation), int(min_volume), L.ptr(labels), L.ptr(state),
                                       L.ptr(totals), L.ptr(stats), L.ptr(ws), ws.numel(), L.stream()), "ru_lesion_loss_forward")
    return totals, stats, labels, state


def _lesion_loss_saved(who, p, labels, state, totals):
    n, c, d, h, w = _dims5(p)
    nstate, off = _lesion_loss_state(n, c, d, h, w)
    if labels.dtype != torch.int32 or labels.shape != p.shape or not labels.is_contiguous():
        raise ValueError("%s: labels must be a contiguous int32 tensor of the prediction's shape (ops.lesion_loss_forward)" % who)
    if state.dtype != torch.uint8 or state.numel() != nstate or not state.is_contiguous():
        raise ValueError("%s: state must be the uint8 tensor ops.lesion_loss_forward returned for this shape" % who)
    if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 2 or not totals.is_contiguous()):
        raise ValueError("%s: totals must be a contiguous float64 tensor [2]" % who)
    return (n, c, d, h, w), off


def lesion_loss_grad(p, g, labels, state, totals_global, priority, scale=None):
    """Lesion-wise Dice loss, pass 2: dp = d loss / d p from what lesion_loss_forward left and the (all-reduced) totals, whose pair count
    is read on the device; times `scale` (a float32 device scalar) when given, inside the one rounding to float32.  Exact zeros on the
    voxels of a dropped lesion, on a pair without a kept lesion, and everywhere when no pair of the global batch has one."""
    p, g = _lesion_loss_args("lesion_loss_grad", p, g)
    (n, c, d, h, w), _ = _lesion_loss_saved("lesion_loss_grad", p, labels, state, totals_global)
    import math
    if not math.isfinite(float(priority)):
        raise ValueError("lesion_loss_grad: priority must be finite, got %r" % (priority,))
    dp = torch.empty_like(p)
    sc = None if scale is None else scale.detach().to(torch.float32).contiguous()
    L.check(L.load().ru_lesion_loss_grad(L.f32(p), L.f32(g), L.ptr(labels), L.ptr(state), L.ptr(totals_global), float(priority), L.ptr(sc, True),
                                         L.f32(dp), n, c, d, h, w, L.stream()), "ru_lesion_loss_grad")
    return dp


def lesion_loss_table(labels, state):
    """Test and debug helper (synchronises): what lesion_loss_forward summed, as int64 numpy.  -> a list over n of lists over c of dicts
    {root, vol, qI, qU: arrays over the lesions of (n, c) in ascending root order, the dropped ones included; qI0, qU0: the background's
    sums}.  qI, qU are the lesion's own sums (its domain's sums are qI0 + qI, qU0 + qU), in units of 2^-35."""
    (n, c, d, h, w), off = _lesion_loss_saved("lesion_loss_table", labels, labels, state, None)
    nk, v = n * c, d * h * w
    raw = state.cpu().numpy()
    pairs = raw[off[0]:off[0] + nk * 64].view("<i8").reshape(nk, 8)
    vol = raw[off[1]:off[1] + nk * v * 4].view("<i4").reshape(nk, v)
    qi = raw[off[2]:off[2] + nk * v * 8].view("<i8").reshape(nk, v)
    qu = raw[off[3]:off[3] + nk * v * 8].view("<i8").reshape(nk, v)
    out = []
    for i in range(n):
        row = []
        for j in range(c):
            k = i * c + j
            root = vol[k].nonzero()[0]
            row.append(dict(root=root.astype("int64"), vol=vol[k][root].astype("int64"), qI=qi[k][root].copy(), qU=qu[k][root].copy(),
                            qI0=int(pairs[k, 5]), qU0=int(pairs[k, 6])))
        out.append(row)
    return out


def adam_amsgrad_step(w, g, m, v, vmax, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam(amsgrad=True) update on flat float32 buffers (main.py:133-137)."""
    L.check(L.load().ru_adam_amsgrad_step(L.f32(w), L.f32(g), L.f32(m), L.f32(v), L.f32(vmax), w.numel(), lr, betas[0], betas[1],
                                          eps, weight_decay, int(step), L.stream()), "ru_adam_amsgrad_step")


TTA_FLIP_BITS = {1: 1, 2: 2, 3: 4}      # axis of a [C,D,H,W] array -> flip bit (D, H, W)


def tta_merge(probs, flip_axes, want_mean=False):
    """Un-flip + average K predictions of flipped copies (test.py:134-138), threshold at 0.5 (test.py:144).
    probs: [K,C,D,H,W]; flip_axes: per copy the tuple of [C,D,H,W] axes that copy was flipped along.
    Returns (mask uint8 [C,D,H,W], counts uint64-as-int64 [C], mean or None)."""
    probs = _prep(probs)
    k, c, d, h, w = [int(v) for v in probs.shape]
    mask, counts, mean = _merge_outputs(c, (d, h, w), probs.device, want_mean)
    L.check(L.load().ru_tta_merge(L.f32(probs), k, _flip_bits(flip_axes), L.ptr(mean, True), L.ptr(mask), L.ptr(counts), c, d, h, w, L.stream()), "ru_tta_merge")
    return mask, counts, mean


def compose_labels(mask, counts, et_min=32):
    """test.py:153-159: labels {0,1,2,4} from the WT/TC/ET masks; ET only if more than `et_min` ET voxels."""
    v = mask.numel() // int(mask.shape[0])
    labels = torch.empty(tuple(mask.shape[1:]), dtype=torch.uint8, device=mask.device)
    L.check(L.load().ru_compose_labels(L.ptr(mask), L.ptr(counts), int(et_min), L.ptr(labels), v, L.stream()), "ru_compose_labels")
    return labels


def _ints(v):
    import ctypes
    v = [int(x) for x in v]
    return (ctypes.c_int * len(v))(*v)


def _flip_bits(flip_axes):
    flips = 0
    for i, axes in enumerate(flip_axes):
        for ax in axes:
            flips |= TTA_FLIP_BITS[ax] << (3 * i)
    return flips


# The merge family (csrc/ensemble.hip: tta_merge*, ens_*, unc_accumulate*, unc_finalize) shares its box, its outputs and the checks of its running sums.
def _merge_box(probs, lo=None, size=None):
    probs = _prep(probs)
    if probs.dim() == 4:
        probs = probs[None]                                            # an already merged prediction: one copy, no flips
    k, c, d, h, w = [int(v) for v in probs.shape]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    size = (d, h, w) if size is None else tuple(int(v) for v in size)
    return probs, (k, c, d, h, w), lo, size


def _merge_outputs(c, size, device, want_mean):
    mask = torch.empty((c,) + tuple(size), dtype=torch.uint8, device=device)
    counts = torch.empty(c, dtype=torch.int64, device=device)
    mean = torch.empty((c,) + tuple(size), dtype=torch.float32, device=device) if want_mean else None
    return mask, counts, mean


def _merge_sums(who, c, size, acc=None, acc2=None):
    for name, t in (("acc", acc), ("acc2", acc2)):
        if t is not None and (tuple(t.shape) != (c,) + size or t.dtype != torch.float32):
            raise ValueError("%s: %s %s does not match %d channels of a %s box" % (who, name, tuple(t.shape), c, size))


def tile_gather(data, tile_shape, origins):
    """loader_helper.copy (:42-60) for T tiles in one launch: data [N,C,D,H,W] -> [T*N, C, *tile_shape], tile t = the zero-padded
    block starting at origins[t] (= get_indices' index_min; may be negative)."""
    data = _prep(data)
    n, c, d, h, w = _dims5(data)
    t = len(origins)
    td, th, tw = (int(v) for v in tile_shape)
    tiles = torch.empty((t * n, c, td, th, tw), dtype=torch.float32, device=data.device)
    L.check(L.load().ru_tile_gather(L.f32(data), L.f32(tiles), n, c, d, h, w, t, _ints([v for o in origins for v in o]), td, th, tw, L.stream()),
            "ru_tile_gather")
    return tiles


def tile_scatter(out, tiles, origins, border, center):
    """loader_helper.copy_back (:82-97) for T tiles in one launch: the centre block of tile t goes to out[..., origins[t] + border ...]."""
    tiles = _prep(tiles)
    if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32):
        raise ValueError("tile_scatter: `out` must be a contiguous float32 device tensor (it is written in place)")
    n, c, d, h, w = _dims5(out)
    t = len(origins)
    td, th, tw = (int(v) for v in tiles.shape[2:])
    if int(tiles.shape[0]) != t * n or int(tiles.shape[1]) != c:
        raise ValueError("tile_scatter: tiles %s do not match %d tiles of a %s volume" % (tuple(tiles.shape), t, tuple(out.shape)))
    L.check(L.load().ru_tile_scatter(L.f32(tiles), L.f32(out), n, c, d, h, w, t, _ints([v for o in origins for v in o]), td, th, tw,
                                     _ints(border), _ints(center), L.stream()), "ru_tile_scatter")
    return out


def _blend_geometry(who, volume_shape, tile_shape, starts, profiles):
    """Host-side checks of the blend entries (before the library is loaded) -> (per-axis start lists, tile extents)."""
    tile = [int(v) for v in tile_shape]
    starts = [[int(v) for v in s] for s in starts]
    if len(tile) != 3 or len(starts) != 3 or any(t <= 0 for t in tile) or any(not s for s in starts):
        raise ValueError("%s: three positive tile extents and three non-empty start lists are needed" % who)
    if tile[2] % 4:
        raise ValueError("%s: the tile width %d is not a multiple of 4" % (who, tile[2]))
    for s, t, n in zip(starts, tile, volume_shape):
        if s[0] != 0 or any(b <= a or b > a + t for a, b in zip(s, s[1:])) or s[-1] >= int(n) or s[-1] + t < int(n):
            raise ValueError("%s: tile starts %s do not cover an axis of %d voxels with tiles of %d (start at 0, strictly increasing, no gap)" % (who, s, int(n), t))
    if not (isinstance(profiles, torch.Tensor) and profiles.dim() == 1 and int(profiles.numel()) == sum(tile) and profiles.dtype == torch.float32):
        raise ValueError("%s: `profiles` must be a float32 tensor of td + th + tw = %d values" % (who, sum(tile)))
    return starts, tile


def blend_accumulate(acc, tiles, starts, profiles, t0=0):
    """Fold the predictions of the tiles t0 .. t0+T-1 (`tiles` [T*N, C, td, th, tw], the layout of `tile_gather`) into the running
    window-weighted sum `acc` [N,C,D,H,W] in place (csrc/blend.hip).  `starts` = the three per-axis start lists, tile index =
    (iz*ny + iy)*nx + ix; `profiles` = device float32 [td+th+tw].  The calls of one volume come in rising t0 and cover every tile once;
    the first touch of a voxel is written, so `acc` needs no memset."""
    if not (isinstance(acc, torch.Tensor) and acc.dim() == 5 and acc.dtype == torch.float32 and acc.is_contiguous()):
        raise ValueError("blend_accumulate: `acc` must be a contiguous float32 [N,C,D,H,W] tensor (it is written in place)")
    n, c, d, h, w = _dims5(acc)
    if tiles.dim() != 5 or int(tiles.shape[1]) != c or int(tiles.shape[0]) % n:
        raise ValueError("blend_accumulate: tiles %s do not match a %s volume" % (tuple(tiles.shape), tuple(acc.shape)))
    starts, (td, th, tw) = _blend_geometry("blend_accumulate", (d, h, w), tiles.shape[2:], starts, profiles)
    t = int(tiles.shape[0]) // n
    ntiles = len(starts[0]) * len(starts[1]) * len(starts[2])
    if not (0 <= int(t0) and t >= 1 and int(t0) + t <= ntiles):
        raise ValueError("blend_accumulate: tiles %d .. %d of %d" % (int(t0), int(t0) + t - 1, ntiles))
    tiles = _prep(tiles)
    L.check(L.load().ru_blend_accumulate(L.f32(tiles), L.f32(acc), L.f32(profiles), n, c, d, h, w, td, th, tw, _ints(starts[0]), len(starts[0]),
                                         _ints(starts[1]), len(starts[1]), _ints(starts[2]), len(starts[2]), int(t0), t, L.stream()), "ru_blend_accumulate")
    return acc


def blend_finalize(acc, tile_shape, starts, profiles, out=None):
    """`acc` / Wn with the summed window Wn recomputed from the geometry (csrc/blend.hip) -> `out` (default: in place)."""
    if not (isinstance(acc, torch.Tensor) and acc.dim() == 5 and acc.dtype == torch.float32 and acc.is_contiguous()):
        raise ValueError("blend_finalize: `acc` must be a contiguous float32 [N,C,D,H,W] tensor")
    out = acc if out is None else out
    if tuple(out.shape) != tuple(acc.shape) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("blend_finalize: `out` must be a contiguous float32 tensor of acc's shape")
    n, c, d, h, w = _dims5(acc)
    starts, (td, th, tw) = _blend_geometry("blend_finalize", (d, h, w), tile_shape, starts, profiles)
    L.require_gpu()
    L.check(L.load().ru_blend_finalize(L.f32(acc), L.f32(out), L.f32(profiles), n, c, d, h, w, td, th, tw, _ints(starts[0]), len(starts[0]),
                                       _ints(starts[1]), len(starts[1]), _ints(starts[2]), len(starts[2]), L.stream()), "ru_blend_finalize")
    return out


def case_bbox(image):
    """test.py:47-49 on the device: per modality {min z, y, x, max z, y, x} of the non-zero voxels -> int64 numpy [C,6] (one small copy to
    the host: the crop extents fix the shapes of everything downstream); all-zero modality: {-1,-1,-1, 0,0,0} as loader_helper.bbox3."""
    image = _prep(image)
    c, d, h, w = (int(v) for v in image.shape)
    box = torch.empty((c, 6), dtype=torch.int32, device=image.device)
    L.check(L.load().ru_case_bbox(L.f32(image), L.ptr(box), c, d, h, w, L.stream()), "ru_case_bbox")
    b = box.cpu().numpy().astype("int64")
    empty = b[:, 3] < 0
    b[empty, :3] = -1
    b[empty, 3:] = 0
    return b


def case_stats(image, lo, size):
    """float64 device tensor [C,3] = count(x > 0), sum x, sum x^2 over the crop box (test.py:103-111)."""
    image = _prep(image)
    c, d, h, w = (int(v) for v in image.shape)
    lib = L.load()
    stats = torch.empty((c, 3), dtype=torch.float64, device=image.device)
    ws = L.workspace(lib.ru_case_workspace_bytes(c, d, h, w), image.device)
    L.check(lib.ru_case_stats(L.f32(image), L.ptr(stats), c, d, h, w, _ints(lo), _ints(size), L.ptr(ws), ws.numel(), L.stream()), "ru_case_stats")
    return stats


def case_prepare(image, stats, lo, size, pad_left, padded, flip_axes):
    """[K,C,*padded] = the K test-time flips of the crop, zero-padded and z-scored (test.py:85-120) -- the batch the network takes."""
    image = _prep(image)
    c, d, h, w = (int(v) for v in image.shape)
    k = len(flip_axes)
    batch = torch.empty((k, c) + tuple(int(v) for v in padded), dtype=torch.float32, device=image.device)
    L.check(L.load().ru_case_prepare(L.f32(image), L.ptr(stats), L.f32(batch), c, d, h, w, _ints(lo), _ints(size), _ints(pad_left), _ints(padded),
                                     k, _flip_bits(flip_axes), L.stream()), "ru_case_prepare")
    return batch


def tta_merge_box(probs, flip_axes, lo, size, want_mean=False):
    """tta_merge restricted to the box [lo, lo+size) of the padded prediction (test.py:134-144 with the padding removed):
    (mask uint8 [C,*size], counts int64 [C], mean or None)."""
    probs = _prep(probs)
    k, c, d, h, w = [int(v) for v in probs.shape]                      # five dimensions, as tta_merge: no merged [C,D,H,W] form here
    mask, counts, mean = _merge_outputs(c, tuple(int(v) for v in size), probs.device, want_mean)
    L.check(L.load().ru_tta_merge_box(L.f32(probs), k, _flip_bits(flip_axes), L.ptr(mean, True), L.ptr(mask), L.ptr(counts), c, d, h, w,
                                      _ints(lo), _ints(size), L.stream()), "ru_tta_merge_box")
    return mask, counts, mean


def cc_reject(labels, ratio=0.1):
    """test.py:162-164 in place on a uint8 device label volume [D,H,W]: 26-connected components of labels > 0, components smaller than
    ratio * (voxels - most frequent label's voxels) are zeroed (test.py:51-62)."""
    if not (labels.is_cuda and labels.is_contiguous() and labels.dtype == torch.uint8 and labels.dim() == 3):
        raise ValueError("cc_reject: contiguous uint8 device tensor [D,H,W]")
    d, h, w = (int(v) for v in labels.shape)
    lib = L.load()
    ws = L.workspace(lib.ru_cc_workspace_bytes(d, h, w), labels.device)
    L.check(lib.ru_cc_reject(L.ptr(labels), d, h, w, float(ratio), L.ptr(ws), ws.numel(), L.stream()), "ru_cc_reject")
    return labels


REGION_NAMES = ("wt", "tc", "et")      # the order of the model's channels and of every per-region parameter


def postprocess_params(min_volume=0, min_confidence=0.0, keep_largest=False, fill_holes=False):
    """The per-region parameters of `postprocess_regions` (a scalar or a triple WT, TC, ET each) as the integers the kernels and the host
    restatement compare: (min_volume [3], T [3] = floor(min_confidence * 65536.0) in float64, keep_largest bits, fill_holes bits)."""
    import math

    def triple(v, name):
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
            return (v, v, v)
        if len(v) != 3:
            raise ValueError("postprocess_regions: %s takes a scalar or one value per region (WT, TC, ET), got %r" % (name, v))
        return tuple(v)

    mv = [int(v) for v in triple(min_volume, "min_volume")]
    mc = [float(v) for v in triple(min_confidence, "min_confidence")]
    if any(v < 0 for v in mv) or any(int(a) != a for a in triple(min_volume, "min_volume")):
        raise ValueError("postprocess_regions: min_volume %r: integers >= 0" % (min_volume,))
    if any(not 0.0 <= c <= 1.0 for c in mc):
        raise ValueError("postprocess_regions: min_confidence %r: values in [0, 1]" % (min_confidence,))
    thr = [int(math.floor(c * 65536.0)) for c in mc]
    bits = lambda v, name: sum(1 << k for k, b in enumerate(triple(v, name)) if bool(b))
    return mv, thr, bits(keep_largest, "keep_largest"), bits(fill_holes, "fill_holes")


def postprocess_regions(x, probs=None, min_volume=0, min_confidence=0.0, keep_largest=False, fill_holes=False, nest=False, want_stats=False):
    """Region-wise post-processing on the device (include/resunet_hip.h, ru_postprocess_regions; INTEGRATION.md states the definition).
    x: uint8 device masks [3, D, H, W] (WT, TC, ET; non-zero = foreground) -> (masks uint8 [3, D, H, W] of 0 / 1, counts int64 [3]), or a
    uint8 device label volume [D, H, W] with values {0, 1, 2, 4} (3 read as 4, above 4 background) -> (labels, counts of WT, TC, ET).
    Per region, a scalar or a triple each: 26-connected components below `min_volume` voxels go; with `probs` (float32 [3, D, H, W], masks
    only) those whose mean probability is below `min_confidence`; with `keep_largest` all but the largest survivor; `fill_holes` fills
    the enclosed 6-connected background; `nest` cuts TC to WT and ET to TC.  want_stats appends int64 [3, 5] = (components found, removed
    by volume, by confidence only, by keep_largest, voxels filled), for a label volume [3, 6] with the invalid voxels (above 4) last.
    `x` is not written; nothing synchronises; two calls give identical bytes."""
    mv, thr, kl, fh = postprocess_params(min_volume, min_confidence, keep_largest, fill_holes)
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and (x.dim() == 3 or (x.dim() == 4 and int(x.shape[0]) == L.POSTPROCESS_REGIONS))):
        raise ValueError("postprocess_regions: uint8 masks [3, D, H, W] or a uint8 label volume [D, H, W]")
    kind = L.POSTPROCESS_LABELS if x.dim() == 3 else L.POSTPROCESS_MASKS
    if any(thr) and probs is None:
        raise ValueError("postprocess_regions: min_confidence > 0 needs the probabilities")
    if probs is not None and (kind == L.POSTPROCESS_LABELS or tuple(probs.shape) != tuple(x.shape)):
        raise ValueError("postprocess_regions: probabilities go with masks and have their shape, got %s for %s" % (tuple(probs.shape), tuple(x.shape)))
    L.require_gpu()
    x = x.contiguous()
    d, h, w = (int(v) for v in x.shape[-3:])
    lib = L.load()
    out = torch.empty_like(x)
    counts = torch.empty(L.POSTPROCESS_REGIONS, dtype=torch.int64, device=x.device)
    stats = torch.empty((L.POSTPROCESS_REGIONS, L.POSTPROCESS_STATS), dtype=torch.int64, device=x.device)
    ws = L.workspace(lib.ru_postprocess_workspace_bytes(kind, d, h, w), x.device)
    L.check(lib.ru_postprocess_regions(L.ptr(x), L.f32(_prep(probs)) if probs is not None and any(thr) else None, kind, d, h, w,
                                       (C.c_longlong * 3)(*mv), (C.c_ulonglong * 3)(*thr), kl, fh, int(bool(nest)), L.ptr(out), L.ptr(counts),
                                       L.ptr(stats), L.ptr(ws), ws.numel(), L.stream()), "ru_postprocess_regions")
    if not want_stats:
        return out, counts
    return out, counts, (stats if kind == L.POSTPROCESS_LABELS else stats[:, :5].contiguous())


def paste_labels(lab, full_shape, lo):
    """test.py:167-168: uint8 device volume `full_shape`, zero except the box at `lo`, which holds `lab`."""
    if not (lab.is_cuda and lab.is_contiguous() and lab.dtype == torch.uint8 and lab.dim() == 3):
        raise ValueError("paste_labels: contiguous uint8 device tensor [d,h,w]")
    full = torch.empty(tuple(int(v) for v in full_shape), dtype=torch.uint8, device=lab.device)
    d, h, w = (int(v) for v in full.shape)
    L.check(L.load().ru_paste_labels(L.ptr(lab), L.ptr(full), d, h, w, _ints(lo), _ints(lab.shape), L.stream()), "ru_paste_labels")
    return full


def ens_accumulate(probs, flip_axes=((),), acc=None, lo=None, size=None):
    """One model of an ensemble (csrc/ensemble.hip): acc [C,*size] float32 takes S_m = S_(m-1) + p_m with p_m the un-flipped mean of
    probs [K,C,D,H,W] on the box [lo, lo+size) (test.py:134-144), in float32 in call order.  acc=None starts a sum (S_1 = p_1, written
    without a memset).  probs [C,D,H,W] with the defaults accumulates an already merged prediction.  Returns acc."""
    probs, (k, c, d, h, w), lo, size = _merge_box(probs, lo, size)
    first = acc is None
    if first:
        acc = torch.empty((c,) + size, dtype=torch.float32, device=probs.device)
    _merge_sums("ens_accumulate", c, size, acc)
    L.check(L.load().ru_ens_accumulate(L.f32(probs), k, _flip_bits(flip_axes), L.f32(acc), int(first), c, d, h, w, _ints(lo), _ints(size), L.stream()),
            "ru_ens_accumulate")
    return acc


def ens_finalize(acc, m, want_mean=False):
    """The sum of `m` models -> (mask uint8 = acc / m > 0.5, counts int64 [C], mean = acc / m or None): `sum(data_files) / len(data_files)`
    of the reference's notebooks in float32 (a true division), then test.py:144."""
    if not (acc.is_cuda and acc.is_contiguous() and acc.dtype == torch.float32 and acc.dim() >= 2):
        raise ValueError("ens_finalize: contiguous float32 device tensor [C, ...]")
    c = int(acc.shape[0])
    mask, counts, mean = _merge_outputs(c, acc.shape[1:], acc.device, want_mean)
    L.check(L.load().ru_ens_finalize(L.f32(acc), int(m), L.ptr(mean, True), L.ptr(mask), L.ptr(counts), c, acc.numel() // c, L.stream()), "ru_ens_finalize")
    return mask, counts, mean


def ens_accumulate_finalize(probs, flip_axes, acc, m, lo=None, size=None, want_mean=False):
    """The LAST model's ens_accumulate fused with ens_finalize (one pass, acc is not written; acc=None: an ensemble of one): the same
    (mask, counts, mean or None), bit for bit."""
    probs, (k, c, d, h, w), lo, size = _merge_box(probs, lo, size)
    _merge_sums("ens_accumulate_finalize", c, size, acc)
    mask, counts, mean = _merge_outputs(c, size, probs.device, want_mean)
    L.check(L.load().ru_ens_accumulate_finalize(L.f32(probs), k, _flip_bits(flip_axes), L.ptr(acc, True), int(acc is None), int(m), L.ptr(mean, True),
                                                L.ptr(mask), L.ptr(counts), c, d, h, w, _ints(lo), _ints(size), L.stream()), "ru_ens_accumulate_finalize")
    return mask, counts, mean


def ens_argmax(acc, m):
    """The class rule of the reference's notebooks on the sum of `m` class maps [C,D,H,W]: argmax over the channels of acc / m (first
    maximum wins, as np.argmax), 3 -> 4; uint8 [D,H,W]."""
    if not (acc.is_cuda and acc.is_contiguous() and acc.dtype == torch.float32 and acc.dim() >= 2):
        raise ValueError("ens_argmax: contiguous float32 device tensor [C, ...]")
    c = int(acc.shape[0])
    labels = torch.empty(tuple(acc.shape[1:]), dtype=torch.uint8, device=acc.device)
    L.check(L.load().ru_ens_argmax(L.f32(acc), int(m), L.ptr(labels), c, acc.numel() // c, L.stream()), "ru_ens_argmax")
    return labels


def paste_probs(mean, full_shape, lo):
    """paste_labels for float channels: float32 device volume [C,*full_shape], zero except the box at `lo`, which holds mean [C,d,h,w]."""
    if not (mean.is_cuda and mean.is_contiguous() and mean.dtype == torch.float32 and mean.dim() == 4):
        raise ValueError("paste_probs: contiguous float32 device tensor [C,d,h,w]")
    c = int(mean.shape[0])
    full = torch.empty((c,) + tuple(int(v) for v in full_shape), dtype=torch.float32, device=mean.device)
    d, h, w = (int(v) for v in full.shape[1:])
    L.check(L.load().ru_paste_probs(L.f32(mean), L.f32(full), c, d, h, w, _ints(lo), _ints(mean.shape[1:]), L.stream()), "ru_paste_probs")
    return full


def unc_accumulate(probs, flip_axes=((),), acc=None, acc2=None, lo=None, size=None):
    """ens_accumulate plus the second-moment sum (csrc/uncertainty.hip), one pass over probs [K,C,D,H,W]: acc takes S_m exactly as
    ens_accumulate writes it, acc2 [C,*size] takes T_m = T_(m-1) + q_m with q_m = ((o0*o0 + o1*o1) + o2*o2) + o3*o3 of the un-flipped
    copies, float32 without fma.  acc=None (then acc2 too) starts both sums.  Returns (acc, acc2)."""
    probs, (k, c, d, h, w), lo, size = _merge_box(probs, lo, size)
    first = acc is None
    if first != (acc2 is None):
        raise ValueError("unc_accumulate: acc and acc2 start together")
    if first:
        acc = torch.empty((c,) + size, dtype=torch.float32, device=probs.device)
        acc2 = torch.empty((c,) + size, dtype=torch.float32, device=probs.device)
    _merge_sums("unc_accumulate", c, size, acc, acc2)
    L.check(L.load().ru_unc_accumulate(L.f32(probs), k, _flip_bits(flip_axes), L.f32(acc), L.f32(acc2), int(first), c, d, h, w, _ints(lo), _ints(size),
                                       L.stream()), "ru_unc_accumulate")
    return acc, acc2


def _unc_measure(measure):
    if measure not in L.UNC_MEASURES:
        raise ValueError("uncertainty measure %r: one of %s" % (measure, sorted(L.UNC_MEASURES)))
    return L.UNC_MEASURES[measure]


def unc_accumulate_finalize(probs, flip_axes, acc, acc2, m, measure="std", lo=None, size=None, want_mean=False):
    """The LAST member's unc_accumulate fused with the finalize: ens_accumulate_finalize's (mask, counts, mean or None), bit for bit, plus
    the uint8 uncertainty map [C,*size] (0 certain .. 100 uncertain) of `measure` "std" or "entropy".  acc = acc2 = None: an ensemble of
    one; acc2 may also be None with "entropy"."""
    probs, (k, c, d, h, w), lo, size = _merge_box(probs, lo, size)
    kind = _unc_measure(measure)
    if acc is None and acc2 is not None or acc is not None and acc2 is None and measure == "std":
        raise ValueError("unc_accumulate_finalize: the std measure needs both running sums")
    _merge_sums("unc_accumulate_finalize", c, size, acc, acc2)
    mask, counts, mean = _merge_outputs(c, size, probs.device, want_mean)
    unc = torch.empty((c,) + size, dtype=torch.uint8, device=probs.device)
    L.check(L.load().ru_unc_accumulate_finalize(L.f32(probs), k, _flip_bits(flip_axes), L.ptr(acc, True), L.ptr(acc2, True), int(acc is None), int(m), kind,
                                                L.ptr(mean, True), L.ptr(mask), L.ptr(counts), L.ptr(unc), c, d, h, w, _ints(lo), _ints(size), L.stream()),
            "ru_unc_accumulate_finalize")
    return mask, counts, mean, unc


def unc_finalize(acc, acc2, m, k=1, measure="std", want_mean=False):
    """ens_finalize plus the uncertainty map, from the stored sums of `m` members of `k` copies each (saved predictions: k = 1).
    acc2 may be None with "entropy".  Returns (mask, counts, mean or None, unc uint8)."""
    if not (acc.is_cuda and acc.is_contiguous() and acc.dtype == torch.float32 and acc.dim() >= 2):
        raise ValueError("unc_finalize: contiguous float32 device tensor [C, ...]")
    kind = _unc_measure(measure)
    c = int(acc.shape[0])
    if acc2 is None and measure == "std":
        raise ValueError("unc_finalize: the std measure needs the second-moment sum")
    _merge_sums("unc_finalize", c, tuple(acc.shape[1:]), acc2=acc2)
    mask, counts, mean = _merge_outputs(c, acc.shape[1:], acc.device, want_mean)
    unc = torch.empty(tuple(acc.shape), dtype=torch.uint8, device=acc.device)
    L.check(L.load().ru_unc_finalize(L.f32(acc), L.ptr(acc2, True), int(m), int(k), kind, L.ptr(mean, True), L.ptr(mask), L.ptr(counts), L.ptr(unc), c,
                                     acc.numel() // c, L.stream()), "ru_unc_finalize")
    return mask, counts, mean, unc


def paste_u8c(maps, full_shape, lo):
    """paste_labels for uint8 channels: [C,*full_shape], zero except the box at `lo`, which holds maps [C,d,h,w]."""
    if not (maps.is_cuda and maps.is_contiguous() and maps.dtype == torch.uint8 and maps.dim() == 4):
        raise ValueError("paste_u8c: contiguous uint8 device tensor [C,d,h,w]")
    c = int(maps.shape[0])
    full = torch.empty((c,) + tuple(int(v) for v in full_shape), dtype=torch.uint8, device=maps.device)
    d, h, w = (int(v) for v in full.shape[1:])
    L.check(L.load().ru_paste_u8c(L.ptr(maps), L.ptr(full), c, d, h, w, _ints(lo), _ints(maps.shape[1:]), L.stream()), "ru_paste_u8c")
    return full


def unc_histogram(pred, target, unc):
    """One pass over a case for the uncertainty score: pred, target uint8 label volumes [D,H,W] with values {0,1,2,3,4}, unc uint8
    [3,D,H,W] -> (hist int64 [3,101,4]: exact voxel counts per region (WT, TC, ET), map value and class (TP, FP, FN, TN); invalid int64
    [1]: voxels with a label outside 0..4 or a map value above 100, which are in no bin)."""
    for name, t in (("pred", pred), ("target", target), ("unc", unc)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8):
            raise ValueError("unc_histogram: %s must be a contiguous uint8 device tensor" % name)
    if pred.dim() != 3 or tuple(target.shape) != tuple(pred.shape) or tuple(unc.shape) != (L.UNC_REGIONS,) + tuple(pred.shape):
        raise ValueError("unc_histogram: shapes %s / %s / %s, expected [D,H,W], [D,H,W], [3,D,H,W]" % (tuple(pred.shape), tuple(target.shape), tuple(unc.shape)))
    d, h, w = (int(v) for v in pred.shape)
    hist = torch.empty((L.UNC_REGIONS, L.UNC_LEVELS, L.UNC_CLASSES), dtype=torch.int64, device=pred.device)
    invalid = torch.empty(1, dtype=torch.int64, device=pred.device)
    L.check(L.load().ru_unc_histogram(L.ptr(pred), L.ptr(target), L.ptr(unc), d, h, w, L.ptr(hist), L.ptr(invalid), L.stream()), "ru_unc_histogram")
    return hist, invalid


def unc_score(hist, thresholds=(25, 50, 75, 100), acc=None, out=None):
    """The BraTS uncertainty score from unc_histogram's counts, one launch: float64 [3,4] = per region (score, AUC_Dice, AUC_FTP, AUC_FTN)
    over the strictly rising integer `thresholds` (include/resunet_hip.h, ru_unc_score); acc (float64 [3,4] or None) += the result."""
    assert hist.dtype == torch.int64 and hist.is_contiguous() and tuple(hist.shape) == (L.UNC_REGIONS, L.UNC_LEVELS, L.UNC_CLASSES)
    assert acc is None or (acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == L.UNC_REGIONS * 4)
    if out is None:
        out = torch.empty((L.UNC_REGIONS, 4), dtype=torch.float64, device=hist.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == L.UNC_REGIONS * 4
    L.check(L.load().ru_unc_score(L.ptr(hist), _ints(thresholds), len(thresholds), L.ptr(out), L.ptr(acc, True), L.stream()), "ru_unc_score")
    return out


def dice_counts(pred, target):
    """metrics.Dice.update counting step (metrics.py:116-127): int64 device tensor [N,C,2] = (#(p>.5 & g>.5), #(p>.5) + #(g>.5))."""
    pred, target = _prep(pred), _prep(target)
    assert pred.shape == target.shape                                  # metrics.py:112
    n, c = int(pred.shape[0]), int(pred.shape[1])
    v = pred.numel() // (n * c)
    counts = torch.empty((n, c, 2), dtype=torch.int64, device=pred.device)
    L.check(L.load().ru_dice_counts(L.f32(pred), L.f32(target), L.ptr(counts), n, c, v, L.stream()), "ru_dice_counts")
    return counts


def dice_accumulate(counts, acc, nacc):
    """metrics.py:124-130 on the device: acc[c] += batch mean of 2*num/den (float32 ratio, NaN -> 1; float64 mean), c < nacc."""
    n, c = int(counts.shape[0]), int(counts.shape[1])
    assert counts.dtype == torch.int64 and counts.is_contiguous() and acc.dtype == torch.float64 and acc.numel() >= nacc
    L.check(L.load().ru_dice_accumulate(L.ptr(counts), L.ptr(acc), n, c, int(nacc), L.stream()), "ru_dice_accumulate")
    return acc


HAUSDORFF_MAX_EXTENT = 512


def hausdorff_sq(pred, target, mode=0):
    """Hausdorff_ITK / Hausdorff_ITKWT.update measuring step (metrics.py:198-263) on the device: int64 device tensor [N,K,4] =
    (max over P of d^2 to G, max over G of d^2 to P, #P, #G) with exact integer squared distances between voxel centres.
    mode 0: K = C masks `x > 0.5`; mode 1: K = 1 mask `argmax over dim 1 > 0`.  Every extent must be <= 512 (else RuntimeError)."""
    if mode not in (0, 1):
        raise ValueError("hausdorff_sq: mode is 0 (per channel > 0.5) or 1 (argmax > 0)")
    pred, target = _prep(pred), _prep(target)
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("hausdorff_sq: shapes differ: %s vs %s" % (tuple(pred.shape), tuple(target.shape)))
    n, c, d, h, w = _dims5(pred)
    lib = L.load()
    out = torch.empty((n, c if mode == 0 else 1, 4), dtype=torch.int64, device=pred.device)
    ws = L.workspace(lib.ru_hausdorff_workspace_bytes(n, c, d, h, w, mode), pred.device)
    L.check(lib.ru_hausdorff_sq(L.f32(pred), L.f32(target), n, c, d, h, w, mode, L.ptr(out), L.ptr(ws), ws.numel(), L.stream()),
            "ru_hausdorff_sq")
    return out


def hausdorff_accumulate(sq, acc, nacc, mode=0):
    """metrics.py:208-230 / 248-265 on the device: acc[i] += batch mean of the reference's result[n, i] (i < nacc) from hausdorff_sq's
    output -- sqrt in float64, 1e6 for an empty mask, the reference's i-1 index slip for a channel empty on both sides (mode 0)."""
    n, k = int(sq.shape[0]), int(sq.shape[1])
    assert sq.dtype == torch.int64 and sq.is_contiguous() and acc.dtype == torch.float64 and acc.numel() >= nacc
    L.check(L.load().ru_hausdorff_accumulate(L.ptr(sq), L.ptr(acc), n, k, int(nacc), int(mode), L.stream()), "ru_hausdorff_accumulate")
    return acc


OVERLAP_BOTH_EMPTY = float("nan")       # Dice_ITK for a label absent from both images (RU_OVERLAP_BOTH_EMPTY; not checked against SimpleITK)


def label_confusion(pred, target):
    """Per-sample confusion matrix of labels (metrics.py:135-185, validate.py:66-97) on the device, one pass, exact integer counts:
    -> (conf int64 [N, L, L] with conf[n, a, b] = #voxels labelled a in `pred` and b in `target`, invalid int64 [N] or None).
    float32 [N, C, ...] probabilities: label = argmax over C (torch's rules), L = C <= 8 (else ValueError).  uint8 [N, ...] label
    volumes: 4 counts as 3, L = 4; invalid[n] counts the voxels where either value is outside 0..4 (they are in no bin)."""
    if tuple(pred.shape) != tuple(target.shape) or pred.dtype != target.dtype or pred.dim() < 2:
        raise ValueError("label_confusion: needs two tensors of one shape and dtype with a batch axis, got %s %s / %s %s"
                         % (tuple(pred.shape), pred.dtype, tuple(target.shape), target.dtype))
    n = int(pred.shape[0])
    if pred.dtype == torch.uint8:
        L.require_gpu()
        pred, target = pred.contiguous(), target.contiguous()
        kind, c, lab = L.CONF_LABEL, 1, 4
        v = pred.numel() // max(n, 1)
    else:
        pred, target = _prep(pred), _prep(target)
        kind, c = L.CONF_PROB, int(pred.shape[1])
        if c > L.OVERLAP_MAX_LABELS:
            raise ValueError("label_confusion: %d channels, the kernel counts at most %d" % (c, L.OVERLAP_MAX_LABELS))
        lab = c
        v = pred.numel() // max(n * c, 1)
    conf = torch.empty((n, lab, lab), dtype=torch.int64, device=pred.device)
    invalid = torch.empty(n, dtype=torch.int64, device=pred.device) if kind == L.CONF_LABEL else None
    L.check(L.load().ru_label_confusion(L.ptr(pred), L.ptr(target), kind, n, c, v, L.ptr(conf), L.ptr(invalid, allow_none=True), L.stream()),
            "ru_label_confusion")
    return conf, invalid


def overlap_accumulate(conf, acc, nacc, mode, out=None):
    """From label_confusion's conf [N, L, L] (int64, device), one launch: mode "itk" (Dice_ITK: label i = 1..nacc -> acc[i-1] += batch
    mean of ITK's Dice, float64; OVERLAP_BOTH_EMPTY for an absent label), "wt" (DiceWT: acc[0] += batch mean of the float32 whole-tumour
    ratio), "validate" (validate.py: out[n] = [d1, d2, d3, dWT], acc += their sum over n).  `out`: float64 [N, nacc] or None."""
    n, lab = int(conf.shape[0]), int(conf.shape[1])
    assert conf.dtype == torch.int64 and conf.is_contiguous() and conf.shape == (n, lab, lab)
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= nacc
    assert out is None or (out.dtype == torch.float64 and out.is_contiguous() and out.numel() == n * nacc)
    L.check(L.load().ru_overlap_accumulate(L.ptr(conf), n, lab, L.OVERLAP_MODES[mode], int(nacc), L.ptr(acc), L.ptr(out, allow_none=True),
                                           L.stream()), "ru_overlap_accumulate")
    return acc


def dice1d_accumulate(counts, acc, classes):
    """metrics.py:41-50 on the device from dice_counts' [N, C, 2]: acc[c] += batch mean of 2*I / (S + 1e-6) (float32 ratio), c < classes."""
    n, c = int(counts.shape[0]), int(counts.shape[1])
    assert counts.dtype == torch.int64 and counts.is_contiguous() and acc.dtype == torch.float64 and acc.numel() >= classes
    L.check(L.load().ru_dice1d_accumulate(L.ptr(counts), L.ptr(acc), n, c, int(classes), L.stream()), "ru_dice1d_accumulate")
    return acc


def rmse_sums(pred, target):
    """RMSE's two sums on the device: float64 [2] = (sum of (pred - target)^2, element count), from ru_crit_moments over the tensors taken as
    one row -- the buffer a data-parallel RMSE all-reduces before the square root."""
    pred, target = _prep(pred), _prep(target)
    if pred.shape != target.shape:
        raise AssertionError("prediction/target shape mismatch")
    lib = L.load()
    v = pred.numel()
    buf = torch.empty(L.CRIT_MOMENTS + 1, dtype=torch.float64, device=pred.device)    # the 7 moments, then the count
    ws = L.workspace(lib.ru_crit_moments_workspace_bytes(1, 1, v), pred.device)
    L.check(lib.ru_crit_moments(L.f32(pred), L.f32(target), 1, 1, v, 0, L.ptr(buf), L.ptr(ws), ws.numel(), L.stream()), "ru_crit_moments")
    buf[L.CRIT_MOMENTS:].fill_(float(v))
    return buf[L.CRIT_M_D2:]


def rmse_accumulate(sums, acc):
    """acc[0] += sqrt(sums[0] / sums[1]) on the device (metrics.py:69-71)."""
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == 2 and acc.dtype == torch.float64
    L.check(L.load().ru_rmse_accumulate(L.ptr(sums), L.ptr(acc), L.stream()), "ru_rmse_accumulate")
    return acc


def _calib_nb(who, nb):
    nb = int(nb)
    if not (L.CALIB_MIN_NB <= nb <= L.CALIB_MAX_NB and nb & (nb - 1) == 0):
        raise ValueError("%s: nb = %d is no power of two in %d..%d" % (who, nb, L.CALIB_MIN_NB, L.CALIB_MAX_NB))
    return nb


def calib_histogram(pred, target, nb=L.CALIB_DEFAULT_NB):
    """One integer pass for calibration scoring and the threshold search (include/resunet_hip.h, ru_calib_histogram): pred float32
    [N,C,...] probabilities, C <= 8; target float32 of the same shape (y = g > 0.5) or a uint8 label volume [N,...] (C = 3: the regions
    WT, TC, ET) -> (hist int64 [N,C,nb+1,2]: voxels per bin k = ceil(p*nb) and class y; conf int64 [N,C,nb+1,2]: sums of r = floor(p*2^24);
    sq int64 [N,C,2,2]: per y the sums of the low and high 32-bit halves of r*r; invalid int64 [N,C]: voxels with p outside [0, 1], a NaN
    target or a label above 4, which are in no bin).  Contiguous views at any 4-byte alignment are taken as they are."""
    nb = _calib_nb("calib_histogram", nb)
    L.require_gpu()
    if not (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() >= 3):
        raise ValueError("calib_histogram: pred must be a float32 device tensor [N,C,...], got %s %s" % (tuple(pred.shape), pred.dtype))
    if not target.is_cuda or target.dtype not in (torch.float32, torch.uint8):
        raise ValueError("calib_histogram: target must be a float32 or uint8 device tensor, got %s" % target.dtype)
    pred, target = pred.contiguous(), target.contiguous()
    n, c = int(pred.shape[0]), int(pred.shape[1])
    v = pred.numel() // max(n * c, 1)
    if target.dtype == torch.uint8:
        kind = L.CALIB_TARGET_LABELS
        if c != 3 or int(target.shape[0]) != n or target.numel() != n * v:
            raise ValueError("calib_histogram: a label volume %s needs pred [N,3,...] of the same extents, got %s" % (tuple(target.shape), tuple(pred.shape)))
    else:
        kind = L.CALIB_TARGET_REGIONS
        if tuple(target.shape) != tuple(pred.shape):
            raise ValueError("calib_histogram: shapes differ: %s vs %s" % (tuple(pred.shape), tuple(target.shape)))
    if not (1 <= c <= L.CALIB_MAX_C and n >= 1 and 1 <= v <= 1 << 31):
        raise ValueError("calib_histogram: %d channels (1..%d), %d samples, %d voxels (1..2^31)" % (c, L.CALIB_MAX_C, n, v))
    dev = pred.device
    hist = torch.empty((n, c, nb + 1, 2), dtype=torch.int64, device=dev)
    conf = torch.empty((n, c, nb + 1, 2), dtype=torch.int64, device=dev)
    sq = torch.empty((n, c, 2, 2), dtype=torch.int64, device=dev)
    invalid = torch.empty((n, c), dtype=torch.int64, device=dev)
    L.check(L.load().ru_calib_histogram(L.ptr(pred), L.ptr(target), kind, n, c, v, nb, L.ptr(hist), L.ptr(conf), L.ptr(sq), L.ptr(invalid), L.stream()),
            "ru_calib_histogram")
    return hist, conf, sq, invalid


def calib_pool(c, nb, device):
    """Zeroed running state for calib_accumulate: (pool_hist int64 [C,nb+1,2], pool_conf int64 [C,nb+1,2], pool_sq int64 [C,2,2],
    curve_acc float64 [C,3,nb+1])."""
    nb = _calib_nb("calib_pool", nb)
    return (torch.zeros((c, nb + 1, 2), dtype=torch.int64, device=device), torch.zeros((c, nb + 1, 2), dtype=torch.int64, device=device),
            torch.zeros((c, 2, 2), dtype=torch.int64, device=device), torch.zeros((c, 3, nb + 1), dtype=torch.float64, device=device))


def calib_accumulate(hist, conf, sq, pool, want_curves=False):
    """One launch (ru_calib_accumulate): pool = calib_pool's tuple; the pooled tables += calib_histogram's per-sample tables (pool_sq is
    kept carried: low word < 2^32), curve_acc [C,3,nb+1] += the sum over the samples of the (Dice, sensitivity, specificity) curves at
    the thresholds b / nb, b = 0..nb.  Returns curves float64 [N,C,3,nb+1] with want_curves, else None."""
    n, c, k = int(hist.shape[0]), int(hist.shape[1]), int(hist.shape[2])
    nb = _calib_nb("calib_accumulate", k - 1)
    pool_hist, pool_conf, pool_sq, curve_acc = pool
    for name, t, shape in (("hist", hist, (n, c, k, 2)), ("conf", conf, (n, c, k, 2)), ("sq", sq, (n, c, 2, 2)), ("pool_hist", pool_hist, (c, k, 2)),
                           ("pool_conf", pool_conf, (c, k, 2)), ("pool_sq", pool_sq, (c, 2, 2))):
        if not (t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError("calib_accumulate: %s must be a contiguous int64 tensor %s, got %s %s" % (name, shape, tuple(t.shape), t.dtype))
    if not (curve_acc.dtype == torch.float64 and curve_acc.is_contiguous() and tuple(curve_acc.shape) == (c, 3, k)):
        raise ValueError("calib_accumulate: curve_acc must be a contiguous float64 tensor %s" % ((c, 3, k),))
    curves = torch.empty((n, c, 3, k), dtype=torch.float64, device=hist.device) if want_curves else None
    L.check(L.load().ru_calib_accumulate(L.ptr(hist), L.ptr(conf), L.ptr(sq), n, c, nb, L.ptr(pool_hist), L.ptr(pool_conf), L.ptr(pool_sq), L.ptr(curve_acc),
                                         L.ptr(curves, allow_none=True), L.stream()), "ru_calib_accumulate")
    return curves


def calib_summary(pool_hist, pool_conf, pool_sq, bins=16):
    """From the pooled tables, one launch (ru_calib_summary) -> (out float64 [C,7] = ECE, MCE, Brier, mean confidence, prevalence, n,
    non-empty coarse bins; table float64 [C,bins,3] = n_m, conf_m, freq_m).  `bins` divides nb."""
    c, k = int(pool_hist.shape[0]), int(pool_hist.shape[1])
    nb, bins = _calib_nb("calib_summary", k - 1), int(bins)
    if bins < 1 or nb % bins:
        raise ValueError("calib_summary: bins = %d must divide nb = %d" % (bins, nb))
    for name, t, shape in (("pool_hist", pool_hist, (c, k, 2)), ("pool_conf", pool_conf, (c, k, 2)), ("pool_sq", pool_sq, (c, 2, 2))):
        if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError("calib_summary: %s must be a contiguous int64 device tensor %s" % (name, shape))
    out = torch.empty((c, 7), dtype=torch.float64, device=pool_hist.device)
    table = torch.empty((c, bins, 3), dtype=torch.float64, device=pool_hist.device)
    L.check(L.load().ru_calib_summary(L.ptr(pool_hist), L.ptr(pool_conf), L.ptr(pool_sq), c, nb, bins, L.ptr(out), L.ptr(table), L.stream()), "ru_calib_summary")
    return out, table


def region_thresholds(thresholds, c):
    """A scalar or a sequence of c thresholds -> a list of c Python floats (rounded to float32, as the kernel compares)."""
    import numpy as np
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if t.size == 1:
        t = np.repeat(t, c)
    if t.size != c or np.isnan(t).any():
        raise ValueError("thresholds: a scalar or %d values without NaN, got %r" % (c, thresholds))
    return [float(np.float32(x)) for x in t]


def threshold_regions(probs, thresholds):
    """probs float32 [C,...] -> (mask uint8 = p > t[c] (NaN gives 0), counts int64 [C]: exact voxels set), one launch
    (ru_threshold_regions).  At 0.5 these are ens_finalize's mask and counts on the same mean, bit for bit."""
    if not (probs.is_cuda and probs.is_contiguous() and probs.dtype == torch.float32 and probs.dim() >= 2):
        raise ValueError("threshold_regions: contiguous float32 device tensor [C, ...]")
    import ctypes
    c = int(probs.shape[0])
    if not 1 <= c <= L.CALIB_MAX_C:
        raise ValueError("threshold_regions: %d channels, 1..%d" % (c, L.CALIB_MAX_C))
    t = region_thresholds(thresholds, c)
    mask = torch.empty(probs.shape, dtype=torch.uint8, device=probs.device)
    counts = torch.empty(c, dtype=torch.int64, device=probs.device)
    L.check(L.load().ru_threshold_regions(L.ptr(probs), c, probs.numel() // c, (ctypes.c_float * c)(*t), L.ptr(mask), L.ptr(counts), L.stream()),
            "ru_threshold_regions")
    return mask, counts


# ---------------------------------------------------------------------- engine-internal voxel-major layout (tests / probes)
HD95_EMPTY = 373.12866                  # sqrt(240^2 + 240^2 + 155^2): the diagonal of a BraTS volume


def surface_metrics(pred, target, empty_value=HD95_EMPTY):
    """The BraTS challenge numbers per sample and region on the device (include/resunet_hip.h, ru_surface_metrics):
    -> (values float64 [N, K, 4] = (Dice, sensitivity, specificity, HD95), counts int64 [N, K, 6] = (|P|, |G|, TP, |dP|, |dG|, invalid)).
    float32 [N, C, D, H, W]: P = pred > 0.5, G = target > 0.5 per channel, K = C.  uint8 label volumes [N, D, H, W]: K = 3 regions
    WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4}; counts[n, :, 5] is the number of voxels of sample n where either value is above 4.
    HD95 is numpy.percentile(surface distances, 95), 0 when both masks are empty and `empty_value` when one is.  Every extent must be
    <= 512 (else RuntimeError).  Nothing is allocated but the outputs and the workspace; nothing synchronises."""
    if tuple(pred.shape) != tuple(target.shape) or pred.dtype != target.dtype:
        raise ValueError("surface_metrics: shapes or dtypes differ: %s %s / %s %s" % (tuple(pred.shape), pred.dtype, tuple(target.shape), target.dtype))
    if pred.dtype == torch.uint8:
        if pred.dim() != 4:
            raise ValueError("surface_metrics: uint8 label volumes are [N, D, H, W], got %s" % (tuple(pred.shape),))
        L.require_gpu()
        pred, target = pred.contiguous(), target.contiguous()
        kind, (n, d, h, w), c, k = L.SURFACE_LABEL, (int(v) for v in pred.shape), 1, L.SURFACE_REGIONS
    else:
        pred, target = _prep(pred), _prep(target)
        kind, (n, c, d, h, w) = L.SURFACE_PROB, _dims5(pred)
        k = c
    lib = L.load()
    values = torch.empty((n, k, 4), dtype=torch.float64, device=pred.device)
    counts = torch.empty((n, k, L.SURFACE_COUNTS), dtype=torch.int64, device=pred.device)
    ws = L.workspace(lib.ru_surface_workspace_bytes(kind, n, c, d, h, w), pred.device)
    L.check(lib.ru_surface_metrics(L.ptr(pred), L.ptr(target), kind, n, c, d, h, w, float(empty_value), L.ptr(values), L.ptr(counts),
                                   L.ptr(ws), ws.numel(), L.stream()), "ru_surface_metrics")
    return values, counts


def surface_accumulate(values, acc, nacc, column):
    """acc[i] += batch mean of surface_metrics' values[:, i, column] (float64, on the device), i < nacc; column is one of
    "dice", "sensitivity", "specificity", "hd95"."""
    n, k = int(values.shape[0]), int(values.shape[1])
    assert values.dtype == torch.float64 and values.is_contiguous() and values.shape == (n, k, 4)
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= nacc
    L.check(L.load().ru_surface_accumulate(L.ptr(values), L.ptr(acc), n, k, int(nacc), L.SURFACE_COLUMNS[column], L.stream()),
            "ru_surface_accumulate")
    return acc


LESION_MAX = 1024                       # default capacity of the per-lesion arrays (ground-truth lesions per sample and region)


def lesion_metrics(pred, target, dilation=3, min_volume=50, empty_value=HD95_EMPTY, want_table=False, max_lesions=LESION_MAX):
    """Lesion-wise Dice and HD95 per sample and region on the device (include/resunet_hip.h, ru_lesion_metrics, states the definition):
    -> (summary float64 [N, K, 2] = (LesionDice, LesionHD95), counts int64 [N, K, 6] = (n_gt, n_kept, n_tp, n_fn, n_fp, invalid)), and
    with want_table a third tensor float64 [N, K, max_lesions, 5] = (vol_i, |M_i|, tp_i, Dice_i, HD95_i), rows from n_gt on zero.
    Inputs as for surface_metrics: float32 [N, C, D, H, W] (masks `> 0.5`, K = C) or uint8 label volumes [N, D, H, W] (K = 3 regions WT,
    TC, ET).  Ground-truth lesions are the 26-connected components of the mask dilated `dilation` times by the 18-neighbour structure;
    those of at most `min_volume` voxels are not scored.  More than `max_lesions` lesions in one (sample, region) raises RuntimeError.
    The call synchronises once (the lesion counts size the HD95 batches)."""
    if tuple(pred.shape) != tuple(target.shape) or pred.dtype != target.dtype:
        raise ValueError("lesion_metrics: shapes or dtypes differ: %s %s / %s %s" % (tuple(pred.shape), pred.dtype, tuple(target.shape), target.dtype))
    if int(dilation) < 0 or int(min_volume) < 0 or int(max_lesions) < 1:
        raise ValueError("lesion_metrics: dilation %s and min_volume %s must be >= 0, max_lesions %s >= 1" % (dilation, min_volume, max_lesions))
    if pred.dtype == torch.uint8:
        if pred.dim() != 4:
            raise ValueError("lesion_metrics: uint8 label volumes are [N, D, H, W], got %s" % (tuple(pred.shape),))
        L.require_gpu()
        pred, target = pred.contiguous(), target.contiguous()
        kind, (n, d, h, w), c, k = L.SURFACE_LABEL, (int(v) for v in pred.shape), 1, L.SURFACE_REGIONS
    else:
        pred, target = _prep(pred), _prep(target)
        kind, (n, c, d, h, w) = L.SURFACE_PROB, _dims5(pred)
        k = c
    lib = L.load()
    summary = torch.empty((n, k, 2), dtype=torch.float64, device=pred.device)
    counts = torch.empty((n, k, L.LESION_COUNTS), dtype=torch.int64, device=pred.device)
    table = torch.zeros((n, k, int(max_lesions), L.LESION_TABLE_COLUMNS), dtype=torch.float64, device=pred.device) if want_table else None
    ws = L.workspace(lib.ru_lesion_workspace_bytes(kind, n, c, d, h, w, int(max_lesions)), pred.device)
    L.check(lib.ru_lesion_metrics(L.ptr(pred), L.ptr(target), kind, n, c, d, h, w, int(dilation), int(min_volume), float(empty_value),
                                  L.ptr(summary), L.ptr(counts), L.ptr(table, allow_none=True), int(max_lesions), L.ptr(ws), ws.numel(),
                                  L.stream()), "ru_lesion_metrics")
    return (summary, counts, table) if want_table else (summary, counts)


def lesion_accumulate(summary, acc, nacc, column):
    """acc[i] += batch mean of lesion_metrics' summary[:, i, column] (float64, on the device), i < nacc; column is "dice" or "hd95"."""
    n, k = int(summary.shape[0]), int(summary.shape[1])
    assert summary.dtype == torch.float64 and summary.is_contiguous() and summary.shape == (n, k, 2)
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= nacc
    L.check(L.load().ru_lesion_accumulate(L.ptr(summary), L.ptr(acc), n, k, int(nacc), L.LESION_COLUMNS[column], L.stream()),
            "ru_lesion_accumulate")
    return acc


def tolerance_bins(tolerances):
    """For each tolerance tau (a float in voxels at unit spacing, >= 0, finite or inf) the largest integer b >= 0 with
    numpy.sqrt(numpy.float64(b)) <= tau, clamped to 2**32 - 1: the limit on the exact integer SQUARED distance that makes the kernel's
    test `s <= b` mean what numpy means by `sqrt(s) <= tau`.  floor(tau**2) corrected by steps of one, since tau**2 is rounded.
    -> list of ints.  ValueError for a negative or NaN tolerance and for more than SURFACE_MAX_TOL of them."""
    taus = [np.float64(t) for t in tolerances]
    if len(taus) > L.SURFACE_MAX_TOL:
        raise ValueError("tolerance_bins: %d tolerances, one call takes at most %d" % (len(taus), L.SURFACE_MAX_TOL))
    top, out = 2 ** 32 - 1, []
    for tau in taus:
        if not tau >= 0:                                                              # negative or NaN
            raise ValueError("tolerance_bins: tolerance %r: must be >= 0" % (float(tau),))
        if tau >= 65536.0:                                                            # sqrt(2**32 - 1) < 65536: every bin a uint32 can name
            out.append(top)
            continue
        b = int(np.floor(tau * tau))
        while b < top and np.sqrt(np.float64(b + 1)) <= tau:
            b += 1
        while b > 0 and np.sqrt(np.float64(b)) > tau:
            b -= 1
        out.append(b)
    return out


def _distance_args(who, pred, target, tolerances):
    """the checks that need no device, then surface_metrics' preparation -> (pred, target, kind, n, c, d, h, w, k, bins as a C array, T)"""
    if tuple(pred.shape) != tuple(target.shape) or pred.dtype != target.dtype:
        raise ValueError("%s: shapes or dtypes differ: %s %s / %s %s" % (who, tuple(pred.shape), pred.dtype, tuple(target.shape), target.dtype))
    bins = tolerance_bins(tolerances)
    if pred.dtype == torch.uint8:
        if pred.dim() != 4:
            raise ValueError("%s: uint8 label volumes are [N, D, H, W], got %s" % (who, tuple(pred.shape)))
        L.require_gpu()
        pred, target = pred.contiguous(), target.contiguous()
        kind, (n, d, h, w), c, k = L.SURFACE_LABEL, (int(v) for v in pred.shape), 1, L.SURFACE_REGIONS
    else:
        pred, target = _prep(pred), _prep(target)
        kind, (n, c, d, h, w) = L.SURFACE_PROB, _dims5(pred)
        k = c
    return pred, target, kind, n, c, d, h, w, k, (C.c_uint * max(len(bins), 1))(*bins), len(bins)


def surface_distances(pred, target, tolerances=(1.0,), empty_value=HD95_EMPTY):
    """surface_metrics and, from the same histogram of surface distances, the normalized surface Dice at each of T <= 8 `tolerances`, the
    average symmetric surface distance and the Hausdorff distance (include/resunet_hip.h, ru_surface_distances):
    -> (values [N, K, 4], counts [N, K, 6], extras float64 [N, K, T + 2] = (NSD_0 .. NSD_T-1, ASSD, HD)); values and counts are
    surface_metrics' byte for byte.  Tolerances are in voxels at unit spacing (tolerance_bins states how `<=` is decided).  Both masks
    empty: NSD 1, ASSD = HD = 0; exactly one empty: NSD 0, ASSD = HD = `empty_value`.  One more launch than surface_metrics, the same
    workspace; nothing synchronises, the tolerances travel as kernel arguments."""
    pred, target, kind, n, c, d, h, w, k, bins, t = _distance_args("surface_distances", pred, target, tolerances)
    lib = L.load()
    values = torch.empty((n, k, 4), dtype=torch.float64, device=pred.device)
    counts = torch.empty((n, k, L.SURFACE_COUNTS), dtype=torch.int64, device=pred.device)
    extras = torch.empty((n, k, t + 2), dtype=torch.float64, device=pred.device)
    ws = L.workspace(lib.ru_surface_workspace_bytes(kind, n, c, d, h, w), pred.device)
    L.check(lib.ru_surface_distances(L.ptr(pred), L.ptr(target), kind, n, c, d, h, w, float(empty_value), bins, t, L.ptr(values), L.ptr(counts),
                                     L.ptr(extras), L.ptr(ws), ws.numel(), L.stream()), "ru_surface_distances")
    return values, counts, extras


def surface_extras_accumulate(extras, acc, nacc, column):
    """acc[i] += batch mean of extras[:, i, column] (float64, on the device), i < nacc, for surface_distances' extras or lesion_distances'
    summary_ex: rows of any width, `column` an index into them."""
    n, k, ncols = (int(v) for v in extras.shape)
    assert extras.dtype == torch.float64 and extras.is_contiguous() and 0 <= int(column) < ncols
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= nacc
    L.check(L.load().ru_surface_extras_accumulate(L.ptr(extras), L.ptr(acc), n, k, int(nacc), ncols, int(column), L.stream()),
            "ru_surface_extras_accumulate")
    return acc


def lesion_distances(pred, target, tolerances=(1.0,), dilation=3, min_volume=50, empty_value=HD95_EMPTY, want_table=False, max_lesions=LESION_MAX):
    """lesion_metrics and the lesion-wise surface Dice and average surface distance of the same matching (include/resunet_hip.h,
    ru_lesion_distances): -> (summary [N, K, 2], counts [N, K, 6], summary_ex float64 [N, K, T + 1] = (LesionNSD_0 .. LesionNSD_T-1,
    LesionASSD)), and with want_table: table [N, K, max_lesions, 5] and table_ex float64 [N, K, max_lesions, T + 2] = (NSD_i per
    tolerance, ASSD_i, HD_i), rows from n_gt on zero.  summary, counts and table are lesion_metrics' byte for byte.  A missed lesion has
    NSD 0 and ASSD `empty_value`; a false-positive component adds NSD 0 and ASSD `empty_value`.  Synchronises once, as lesion_metrics."""
    if int(dilation) < 0 or int(min_volume) < 0 or int(max_lesions) < 1:
        raise ValueError("lesion_distances: dilation %s and min_volume %s must be >= 0, max_lesions %s >= 1" % (dilation, min_volume, max_lesions))
    pred, target, kind, n, c, d, h, w, k, bins, t = _distance_args("lesion_distances", pred, target, tolerances)
    lib = L.load()
    summary = torch.empty((n, k, 2), dtype=torch.float64, device=pred.device)
    counts = torch.empty((n, k, L.LESION_COUNTS), dtype=torch.int64, device=pred.device)
    summary_ex = torch.empty((n, k, t + 1), dtype=torch.float64, device=pred.device)
    table = torch.zeros((n, k, int(max_lesions), L.LESION_TABLE_COLUMNS), dtype=torch.float64, device=pred.device) if want_table else None
    table_ex = torch.zeros((n, k, int(max_lesions), t + 2), dtype=torch.float64, device=pred.device) if want_table else None
    ws = L.workspace(lib.ru_lesion_distances_workspace_bytes(kind, n, c, d, h, w, int(max_lesions), t), pred.device)
    L.check(lib.ru_lesion_distances(L.ptr(pred), L.ptr(target), kind, n, c, d, h, w, int(dilation), int(min_volume), float(empty_value), bins, t,
                                    L.ptr(summary), L.ptr(counts), L.ptr(table, allow_none=True), L.ptr(summary_ex),
                                    L.ptr(table_ex, allow_none=True), int(max_lesions), L.ptr(ws), ws.numel(), L.stream()), "ru_lesion_distances")
    return (summary, counts, summary_ex, table, table_ex) if want_table else (summary, counts, summary_ex)


def to_c16(x):
    """NCDHW [N,C,D,H,W] -> C16 storage [N,C/16,D,H,W,16] (device kernel ru_layout_convert)."""
    x = _prep(x)
    n, c, d, h, w = _dims5(x)
    y = torch.empty((n, c // 16, d, h, w, 16), dtype=torch.float32, device=x.device)
    L.check(L.load().ru_layout_convert(L.f32(x), L.f32(y), n, c, d * h * w, 1, L.stream()), "ru_layout_convert")
    return y


def from_c16(x):
    x = _prep(x)
    n, cb, d, h, w, _ = (int(v) for v in x.shape)
    y = torch.empty((n, cb * 16, d, h, w), dtype=torch.float32, device=x.device)
    L.check(L.load().ru_layout_convert(L.f32(x), L.f32(y), n, cb * 16, d * h * w, 0, L.stream()), "ru_layout_convert")
    return y


def upsample2x_c16(x, out_slope=1.0, out=None):
    """Trilinear x2 on a C16 tensor [N,C/16,D,H,W,16]; LeakyReLU(out_slope) fused on the output (1 = none)."""
    x = _prep(x)
    n, cb, d, h, w, _ = (int(v) for v in x.shape)
    y = _out(out, (n, cb, 2 * d, 2 * h, 2 * w, 16), x.device)
    L.check(L.load().ru_upsample2x_trilinear_fwd_l(L.f32(x), L.f32(y), n, cb * 16, d, h, w, float(out_slope), L.stream()),
            "ru_upsample2x_trilinear_fwd_l")
    return y


def upsample2x_bwd_c16(dy, out=None):
    dy = _prep(dy)
    n, cb, d2, h2, w2, _ = (int(v) for v in dy.shape)
    dx = _out(out, (n, cb, d2 // 2, h2 // 2, w2 // 2, 16), dy.device)
    L.check(L.load().ru_upsample2x_trilinear_bwd_l(L.f32(dy), L.f32(dx), n, cb * 16, d2 // 2, h2 // 2, w2 // 2, L.stream()),
            "ru_upsample2x_trilinear_bwd_l")
    return dx


def to_split_c16(x_c16):
    """fp32 voxel-major [N,CB,D,H,W,16] -> the SPLIT form of the same storage size that gn_bwd_apply16 publishes and the gradient
    convolutions read: per voxel and block 64 bytes = [hi bf16 ch0-7 | hi ch8-15 | lo ch0-7 | lo ch8-15], hi = bf16(v), lo = bf16(v - hi)."""
    hi = x_c16.to(torch.bfloat16)
    lo = (x_c16 - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32)


def conv3d_layout(x, w, bias=None, in_c16=False, out_c16=False, few_channels=False, in_split=False, exact_f32=False, activations=False, gradient=False):
    """3x3x3 split-bf16 convolution on tensors in NCDHW or C16 storage (x: 5-D NCDHW or 6-D C16); few_channels: NCDHW input
    with Cin <= 4 through the 4-channel tap-pair kernel; activations: x is an activation tensor (a forward convolution), which lets the
    shapes that have the kernel take the fp16 + MX-fp8 product scheme (conv3_mx.hpp), as the engine's forward convolutions do; gradient: x is a
    gradient tensor -- 16 -> 16 voxel-major shapes take the gradient-operand form of the scheme, as the engine's 16-channel data-gradient convolutions do."""
    x, w, bias = _prep(x), _prep(w), _prep(bias)
    if in_c16:
        n, cb, d, h, wd, _ = (int(v) for v in x.shape)
        cin = cb * 16
    else:
        n, cin, d, h, wd = _dims5(x)
    cout = int(w.shape[0])
    y = torch.empty((n, cout // 16, d, h, wd, 16) if out_c16 else (n, cout, d, h, wd), dtype=torch.float32, device=x.device)
    lib = L.load()
    flags = int(in_c16) | (int(out_c16) << 1) | (int(few_channels) << 2) | (int(in_split) << 3) | (int(exact_f32) << 4) | (int(activations) << 5) | (int(gradient) << 6)
    ws = L.workspace(lib.ru_conv3_l_workspace_bytes(n, cin, cout, d, h, wd, flags), x.device)
    L.check(lib.ru_conv3d_fwd_l(L.f32(x), L.f32(w), L.ptr(bias, True), L.f32(y), n, cin, cout, d, h, wd, flags, L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_fwd_l")
    return y


def conv3d_bwd_weight_layout(x, dy, x_c16=False, dy_c16=False, out=None):
    """3x3x3 split-bf16 weight gradient on tensors in NCDHW or C16 storage."""
    x, dy = _prep(x), _prep(dy)
    if x_c16:
        n, cb, d, h, wd, _ = (int(v) for v in x.shape)
        cin = cb * 16
    else:
        n, cin, d, h, wd = _dims5(x)
    cout = int(dy.shape[1]) * 16 if dy_c16 else int(dy.shape[1])
    dw = _out(out, (cout, cin, 3, 3, 3), x.device)
    lib = L.load()
    ws = L.workspace(lib.ru_conv3d_workspace_bytes(n, cin, cout, d, h, wd, 3), x.device)
    L.check(lib.ru_conv3d_bwd_weight_l(L.f32(x), L.f32(dy), L.f32(dw), n, cin, cout, d, h, wd, int(x_c16) | (int(dy_c16) << 1),
                                       L.ptr(ws), ws.numel(), L.stream()), "ru_conv3d_bwd_weight_l")
    return dw


Conv1Result = collections.namedtuple("Conv1Result", "y y1 partials nblk inst")
Wgrad1Result = collections.namedtuple("Wgrad1Result", "dw dx0 dx1 inst")


def conv1_inst(packed):
    """ru_conv1_l's kernel report -> (COB, S2D, NSLOT, PAIR) of conv1_16_kernel."""
    return packed & 15, (packed >> 4) & 15, (packed >> 8) & 15, bool((packed >> 12) & 1)


def wgrad1_inst(packed):
    """ru_wgrad1_l's kernel report -> (OT, CT, stride-2 kernel, fused data gradient)."""
    return packed & 15, (packed >> 4) & 15, bool(packed & 256), bool(packed & 512)


def conv1x1_c16(x0, w, x1=None, add=None, out_slope=1.0, mask=None, mask_slope=LEAKY_SLOPE, cout0=0, s2d=0,
                bst_y=None, bst_k=None, bst_slope=LEAKY_SLOPE):
    """One launch of the voxel-major pointwise convolution (ru_conv1_l; model.py:393,401,424 and the 2x2x2 stride-2 conv of model.py:361-363
    with its transpose).  s2d = 0: w is [Cout, ldw] as the kernel reads it, x1 the second half of a concat, cout0 > 0 splits the output in (y, y1);
    s2d = 1 (gather): x0 is the fine tensor, w the reference's [Cout, Cin, 2, 2, 2]; s2d = 2 (scatter): x0 is the coarse tensor, w the reference's
    [C0, Cfine, 2, 2, 2], y the fine tensor.  bst_*: fused GroupNorm-backward sums, returned as partials [N, C, nblk, 2]."""
    x0, w, x1, add, mask, bst_y, bst_k = (_prep(t) for t in (x0, w, x1, add, mask, bst_y, bst_k))
    lib = L.load()
    n, cb0, d, h, wd, _ = (int(v) for v in x0.shape)
    c0, c1 = cb0 * 16, (int(x1.shape[1]) * 16 if x1 is not None else 0)
    dc, hc, wc, ldw = d, h, wd, 0
    if s2d == 0:
        cout, ldw = int(w.shape[0]), int(w.shape[1])
        out_sp, cstat = (d, h, wd), cout
    elif s2d == 1:
        cout, c0 = int(w.shape[0]), 8 * c0
        dc, hc, wc = d // 2, h // 2, wd // 2
        out_sp, cstat = (dc, hc, wc), cout
    else:
        cout = 8 * int(w.shape[1])
        out_sp, cstat = (2 * d, 2 * h, 2 * wd), cout // 8
    v = dc * hc * wc
    dev = x0.device
    y1 = None
    if cout0:
        y = torch.empty((n, cout0 // 16) + (d, h, wd) + (16,), dtype=torch.float32, device=dev)
        y1 = torch.empty((n, (cout - cout0) // 16) + (d, h, wd) + (16,), dtype=torch.float32, device=dev)
    else:
        y = torch.empty((n, cstat // 16) + out_sp + (16,), dtype=torch.float32, device=dev)
    part, cap = None, 0
    if bst_y is not None:
        cap = n * cstat * ((v + 255) // 256) * max(cout // 16, 1) * 2          # nblk <= voxel groups x channel groups
        part = torch.zeros(cap, dtype=torch.float32, device=dev)
    ws = L.workspace(lib.ru_conv1_l_workspace_bytes(c0, cout, s2d), dev)
    nblk, inst = C.c_int(0), C.c_int(0)
    L.check(lib.ru_conv1_l(L.f32(x0), c0, L.ptr(x1, True), c1, L.f32(w), ldw, L.f32(y), L.ptr(y1, True), cout0, L.ptr(add, True), float(out_slope),
                           L.ptr(mask, True), float(mask_slope), n, cout, v, s2d, dc, hc, wc, L.ptr(bst_y, True), L.ptr(bst_k, True), float(bst_slope),
                           L.ptr(part, True), cap, C.byref(nblk), C.byref(inst), L.ptr(ws), ws.numel(), L.stream()), "ru_conv1_l")
    if part is not None:
        part = part[:n * cstat * nblk.value * 2].view(n, cstat, nblk.value, 2)
    return Conv1Result(y, y1, part, nblk.value, inst.value)


def conv1x1_bwd_weight_c16(x, dy, x1=None, ldw=None, s2d=False, tap_split=False, dg_w=None, dg_mask_slope=LEAKY_SLOPE):
    """One launch of the voxel-major 1x1x1 weight gradient (ru_wgrad1_l): dw [Cout, ldw] (tap_split: the reference's [Cout, Cin/8, 2, 2, 2]).  x1: the
    second half of a concat; s2d: x is the FINE tensor of a stride-2 conv; dg_w [Cout, dg_ldw]: the fused data gradient (dx0 like x, dx1 like x1,
    the latter through the LeakyReLU-backward mask of x1)."""
    x, dy, x1, dg_w = (_prep(t) for t in (x, dy, x1, dg_w))
    lib = L.load()
    n, cbo, d, h, wd, _ = (int(v) for v in dy.shape)
    c0 = int(x.shape[1]) * 16
    cin = 8 * c0 if s2d else c0 + (int(x1.shape[1]) * 16 if x1 is not None else 0)
    cout, v = cbo * 16, d * h * wd
    ldw = cin if ldw is None else int(ldw)
    dev = x.device
    dw = torch.zeros((cout, cin // 8, 2, 2, 2) if tap_split else (cout, ldw), dtype=torch.float32, device=dev)
    dx0 = torch.empty_like(x) if dg_w is not None else None
    dx1 = torch.empty_like(x1) if dg_w is not None and x1 is not None else None
    ws = L.workspace(lib.ru_wgrad1_l_workspace_bytes(n, cin, cout, v), dev)
    inst = C.c_int(0)
    L.check(lib.ru_wgrad1_l(L.f32(x), L.ptr(x1, True), c0 if x1 is not None else 0, L.f32(dy), L.f32(dw), ldw, n, cin, cout, v, 1, int(bool(s2d)), d, h, wd,
                            cin // 8 if tap_split else 0, L.ptr(dg_w, True), int(dg_w.shape[1]) if dg_w is not None else 0, L.ptr(dx0, True), L.ptr(dx1, True),
                            float(dg_mask_slope), C.byref(inst), L.ptr(ws), ws.numel(), L.stream()), "ru_wgrad1_l")
    return Wgrad1Result(dw, dx0, dx1, inst.value)


Conv3Result = collections.namedtuple("Conv3Result", "y in_sum partials nblk route fin", defaults=(None,))
GnStats = collections.namedtuple("GnStats", "mean rstd scale shift bst_k")
GnBwdCoef = collections.namedtuple("GnBwdCoef", "coef dgamma dbeta")
GnBwdResult = collections.namedtuple("GnBwdResult", "dx dgamma dbeta coef partials")
Conv3Route = collections.namedtuple("Conv3Route", "family tz ty in16 out16 multi bst add np head grad")
CONV3_FAMILIES = {1: "sb", 2: "sb2", 3: "sb2c4", 4: "wz32", 5: "wz32mx", 6: "mx", 7: "f32c", 8: "wz16"}


def conv3_route(packed):
    """ru_conv3_l's kernel report (conv3_sb_route / conv3_f32c_route) -> (family, TZ, TY, IN16, OUT16, MULTI, BST, ADD, NP, HEAD, GRAD)."""
    bit = lambda b: bool((packed >> b) & 1)
    return Conv3Route(CONV3_FAMILIES.get(packed & 15, "none"), (packed >> 4) & 15, (packed >> 8) & 15, bit(12), bit(13), bit(14), bit(15), bit(16),
                      (packed >> 20) & 3, bit(17), bit(18))


def conv3_fused(x, w, bias=None, in_c16=False, out_c16=False, few_channels=False, in_split=False, exact_f32=False, activations=False, gradient=False,
                add=None, in_scale=None, in_shift=None, in_slope=LEAKY_SLOPE, in_res=None, in_sum_out=None, sigmoid=False, products=0,
                bst_y=None, bst_k=None, bst_slope=LEAKY_SLOPE, stats=None, weight_mode=0, pack_training=False, y=None,
                tail=0, tail_gamma=None, tail_beta=None, tail_mean=None, tail_rstd=None, tail_want_k=False, tail_s2_sign=1, tail_groups=8, tail_eps=1e-5,
                tail_override=None, tail_workspace=None, tail_keep_ticket=False):
    """One launch of the 3x3x3 family with the operands the engine fuses into it (ru_conv3_l; layout flags as conv3d_layout).  in_scale / in_shift [N, Cin]: the
    GroupNorm apply + LeakyReLU(in_slope) formed in the staging; in_res (voxel-major): added to the transformed input, the sum written to in_sum_out (a tensor
    like x, or True to allocate one); add: joined in the store; stats: per-workgroup (sum, sumsq) of the stored value before the sigmoid -- or, with bst_y /
    bst_k [N, 3, Cout], the GroupNorm-backward sums -- returned as partials [N, Cout, nblk, 2] (default: on with bst_y); weight_mode = 1: w is the FORWARD
    convolution's [Cin, Cout, 3, 3, 3] and is packed as its data gradient.  pack_training: w is packed as a training step packs it (flag bit 7: the forms the RU_*
    switches launch, no direct fragments where a forward convolution of this shape takes a Winograd-z / MX route) -- a launch whose route reads a form the pack
    lacks is refused.  y: the output tensor to write (default: a new one).  route: decode with conv3_route.
    tail = 1 / 2: the launch's last workgroup finalizes the partials (ru_fin_desc): 1 with tail_gamma / tail_beta -> fin = GnStats (bst_k with tail_want_k); 2 (the
    partials are the GroupNorm-backward sums of bst_*) with tail_gamma and the GroupNorm's tail_mean / tail_rstd -> fin = GnBwdCoef.  tail_override: dict of nblk / N / C
    handed to the launcher in place of the launch's own.  With a tail, fin = (the finalized tensors, the workspace tensor used); tail_workspace: that tensor of an
    earlier call of the same shape, to be used again -- with tail_keep_ticket its ticket word is NOT zeroed before the launch (the finisher left it at zero)."""
    x, w, bias, add, in_scale, in_shift, in_res, bst_y, bst_k = (_prep(t) for t in (x, w, bias, add, in_scale, in_shift, in_res, bst_y, bst_k))
    if in_c16:
        n, cb, d, h, wd, _ = (int(v) for v in x.shape)
        cin = cb * 16
    else:
        n, cin, d, h, wd = _dims5(x)
    cout = int(w.shape[1 if weight_mode else 0])
    dev = x.device
    if y is None:
        y = torch.empty((n, cout // 16, d, h, wd, 16) if out_c16 else (n, cout, d, h, wd), dtype=torch.float32, device=dev)
    if in_sum_out is True:
        in_sum_out = torch.full_like(x, float("nan"))
    part, cap = None, 0
    if stats is None:
        stats = bst_y is not None
    if stats:
        cap = n * cout * max(((d + 1) // 2) * ((h + 1) // 2) * ((wd + 15) // 16), 1024) * 2      # nblk <= the (2,2,16) tiles of a sample, or one per workgroup
        part = torch.full((cap,), float("nan"), dtype=torch.float32, device=dev)
    flags = (int(in_c16) | (int(out_c16) << 1) | (int(few_channels) << 2) | (int(in_split) << 3) | (int(exact_f32) << 4) | (int(activations) << 5)
             | (int(gradient) << 6) | (int(pack_training) << 7))
    lib = L.load()
    fd, fin = None, None
    if tail:
        tail_gamma, tail_beta, tail_mean, tail_rstd = (_prep(t) for t in (tail_gamma, tail_beta, tail_mean, tail_rstd))
        new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        fd = L.FinDesc(kind=int(tail), G=int(tail_groups), s2_sign=int(tail_s2_sign), keep_ticket=int(bool(tail_keep_ticket)), eps=float(tail_eps),
                       gamma=L.f32(tail_gamma), **{k: int(v) for k, v in (tail_override or {}).items()})
        if tail == 1:
            fin = GnStats(new(n * tail_groups), new(n * tail_groups), new(n, cout), new(n, cout), new(n, 3, cout) if tail_want_k else None)
            fd.beta, fd.mean, fd.rstd, fd.scale, fd.shift, fd.bst_k = (L.ptr(t, True) for t in (tail_beta,) + tuple(fin))
        else:
            fin = GnBwdCoef(new(n, cout, 3), new(cout), new(cout))
            fd.mean, fd.rstd, fd.coef, fd.dgamma, fd.dbeta = (L.ptr(t, True) for t in (tail_mean, tail_rstd) + tuple(fin))
    ws = tail_workspace if tail_workspace is not None else L.workspace(lib.ru_conv3_l_workspace_bytes(n, cin, cout, d, h, wd, flags | (256 if tail else 0)), dev)
    nblk, route = C.c_int(0), C.c_int(0)
    L.check(lib.ru_conv3_l(L.f32(x), L.f32(w), L.ptr(bias, True), L.f32(y), n, cin, cout, d, h, wd, flags, int(weight_mode), L.ptr(add, True),
                           L.ptr(in_scale, True), L.ptr(in_shift, True), float(in_slope), L.ptr(in_res, True), L.ptr(in_sum_out, True), int(bool(sigmoid)),
                           int(products), L.ptr(bst_y, True), L.ptr(bst_k, True), float(bst_slope), L.ptr(part, True), cap, C.byref(nblk), C.byref(route),
                           L.ptr(ws), ws.numel(), L.stream(), C.byref(fd) if fd is not None else None), "ru_conv3_l")
    if part is not None:
        part = part[:n * cout * nblk.value * 2].view(n, cout, nblk.value, 2)
    return Conv3Result(y, in_sum_out, part, nblk.value, route.value, (fin, ws) if fin is not None else None)


def _c16_dims(x):
    n, cb, d, h, w, _ = (int(v) for v in x.shape)
    return n, cb * 16, d * h * w


def gn_finalize(partials, gamma, beta, V, centred=False, want_k=False, groups=8, eps=1e-5):
    """One launch of the GroupNorm finalize (ru_gn_finalize_l) on partials [N, C, nblk, 2] -- (sum, sumsq) pairs as the convolution epilogues publish them, or with
    centred the (sum, M2) pairs of the NCDHW statistics pass: GnStats(mean [N*G], rstd [N*G], scale [N, C], shift [N, C], bst_k [N, 3, C] or None)."""
    partials, gamma, beta = _prep(partials), _prep(gamma), _prep(beta)
    n, c, nblk, _ = (int(v) for v in partials.shape)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=partials.device)
    r = GnStats(new(n * groups), new(n * groups), new(n, c), new(n, c), new(n, 3, c) if want_k else None)
    L.check(L.load().ru_gn_finalize_l(L.f32(partials), nblk, L.f32(gamma), L.f32(beta), L.f32(r.mean), L.f32(r.rstd), L.f32(r.scale), L.f32(r.shift),
                                      L.ptr(r.bst_k, True), n, c, int(V), int(groups), float(eps), int(bool(centred)), L.stream()), "ru_gn_finalize_l")
    return r


def gn_apply_c16(x, scale, shift, slope, res=None, res_scale=None, res_shift=None, res_slope=1.0):
    """One launch of the voxel-major GroupNorm apply (ru_gn_apply_l): y = res' + lrelu(x*scale + shift, slope) on x [N, C/16, D, H, W, 16]; res' is nothing, res, or
    lrelu(res*res_scale + res_shift, res_slope) -- a GroupNorm output that was never written."""
    x, scale, shift, res, res_scale, res_shift = (_prep(t) for t in (x, scale, shift, res, res_scale, res_shift))
    n, c, v = _c16_dims(x)
    y = torch.full_like(x, float("nan"))
    L.check(L.load().ru_gn_apply_l(L.f32(x), L.f32(scale), L.f32(shift), L.ptr(res, True), L.ptr(res_scale, True), L.ptr(res_shift, True), L.f32(y), n, c, v,
                                   float(slope), float(res_slope), L.stream()), "ru_gn_apply_l")
    return y


def gn_bwd_finalize(partials, gamma, mean, rstd, V, s2_sign, groups=8):
    """One launch of the GroupNorm-backward finalize (ru_gn_bwd_finalize_l) on partials [N, C, nblk, 2] of (S1, S2): GnBwdCoef(coef [N, C, 3], dgamma [C], dbeta [C])."""
    partials, gamma, mean, rstd = _prep(partials), _prep(gamma), _prep(mean), _prep(rstd)
    n, c, nblk, _ = (int(v) for v in partials.shape)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=partials.device)
    r = GnBwdCoef(new(n, c, 3), new(c), new(c))
    L.check(L.load().ru_gn_bwd_finalize_l(L.f32(partials), nblk, L.f32(gamma), L.f32(mean), L.f32(rstd), L.f32(r.coef), L.f32(r.dgamma), L.f32(r.dbeta),
                                          n, c, int(V), int(groups), int(s2_sign), L.stream()), "ru_gn_bwd_finalize_l")
    return r


def gn_bwd_c16(x, dact, gamma, scale, shift, mean, rstd, slope, tail=False, split=False, stop_after_finalize=False, groups=8, workspace=None, keep_ticket=False):
    """The voxel-major GroupNorm backward as the engine chains it (ru_gn_bwd_l): the reduction over (x, dact), the finalize -- in the reduction's tail or as its own
    launch -- and the apply, plain or in split form (to_split_c16's).  GnBwdResult(dx or None, dgamma, dbeta, coef [N, C, 3], partials [N, C, nblk, 2]).  workspace:
    a uint8 tensor of ru_gn_bwd_l_workspace_bytes(N, C, V) to use (default: a new one); keep_ticket: its ticket word is NOT zeroed before the launch (the finisher
    of an earlier call on the same workspace left it at zero)."""
    x, dact, gamma, scale, shift, mean, rstd = (_prep(t) for t in (x, dact, gamma, scale, shift, mean, rstd))
    n, c, v = _c16_dims(x)
    lib = L.load()
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=x.device)
    dx = None if stop_after_finalize else torch.full_like(x, float("nan"))
    r = GnBwdResult(dx, new(c), new(c), new(n, c, 3), new(n, c, lib.ru_gn_bwd_l_nblk(v), 2))
    ws = workspace if workspace is not None else L.workspace(lib.ru_gn_bwd_l_workspace_bytes(n, c, v), x.device)
    flags = int(bool(tail)) | (int(bool(split)) << 1) | (int(bool(stop_after_finalize)) << 2) | (int(bool(keep_ticket)) << 3)
    L.check(lib.ru_gn_bwd_l(L.f32(x), L.f32(dact), L.f32(gamma), L.f32(scale), L.f32(shift), L.f32(mean), L.f32(rstd), float(slope), L.ptr(dx, True),
                            L.f32(r.dgamma), L.f32(r.dbeta), L.f32(r.coef), L.f32(r.partials), n, c, v, int(groups), flags, L.ptr(ws), ws.numel(), L.stream()),
            "ru_gn_bwd_l")
    return r


Wgrad3Result = collections.namedtuple("Wgrad3Result", "dw gb_out inst")


def wgrad3_inst(packed):
    """ru_wgrad3_l's kernel report (wgrad3_tr_inst) -> (OT, XS, DS, NP) of wgrad3_tz_kernel; None where the launch is refused."""
    return None if packed < 0 else (packed & 15, (packed >> 4) & 15, (packed >> 8) & 15, (packed >> 12) & 15)


def wgrad3_fused(x, dy, in_scale=None, in_shift=None, in_slope=LEAKY_SLOPE, dy_split=False, x_c4=False, dy_c4=False, swapped=False, products=0, gb_g16=False,
                 dw_cin=0, dw_cout=0, gb_y=None, gb_d=None, gb_scale=None, gb_shift=None, gb_coef=None, gb_slope=LEAKY_SLOPE, gb_out=False, deferred=False,
                 cin=None, cout=None):
    """One launch of the transpose-read 3x3x3 weight gradient with the operands the engine fuses into it (ru_wgrad3_l).  x, dy, gb_y, gb_d: voxel-major
    [N, C/16, D, H, W, 16]; with x_c4 / dy_c4 that side is NCDHW with <= 4 channels (dw_cin / dw_cout of them) and is copied to the 4-channel form.  dy_split: dy is
    in split form (to_split_c16).  gb_*: the GroupNorm-backward apply forms dy in the staging (dy may be None); gb_out = True allocates the published tensor
    prefilled with NaN (split form, or the gradient-operand form with gb_g16).  dw: [dw_cout, dw_cin, 3, 3, 3], swapped: [dw_cin, dw_cout, 3, 3, 3] (the
    convolution's own [Cout, Cin]).  cin / cout: the channel counts the launch is told when a 4-channel side should stand beside more than one block (16
    otherwise; such a launch is refused).  inst: decode with wgrad3_inst."""
    x, dy, in_scale, in_shift, gb_y, gb_d, gb_scale, gb_shift, gb_coef = (_prep(t) for t in (x, dy, in_scale, in_shift, gb_y, gb_d, gb_scale, gb_shift, gb_coef))
    side = gb_y if gb_y is not None else dy
    if x_c4:
        n, _, d, h, wd = _dims5(x)
        cin = int(cin or 16)
    else:
        n, cb, d, h, wd, _ = (int(v) for v in x.shape)
        cin = cb * 16
    cout = int(cout or 16) if (dy_c4 and gb_y is None) else int(side.shape[1]) * 16
    dev = x.device
    ci, co = (dw_cin or cin), (dw_cout or cout)
    dw = torch.full((ci, co, 3, 3, 3) if swapped else (co, ci, 3, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    if gb_out is True:
        gb_out = torch.full((n, cout // 16, d, h, wd, 16), float("nan"), dtype=torch.float32, device=dev)
    elif gb_out is False:
        gb_out = None
    flags = int(dy_split) | (int(x_c4) << 1) | (int(dy_c4) << 2) | (int(swapped) << 3) | (int(gb_g16) << 4) | (int(deferred) << 5)
    lib = L.load()
    ws = L.workspace(lib.ru_wgrad3_l_workspace_bytes(n, cin, cout, d, h, wd, flags), dev)
    inst = C.c_int(0)
    L.check(lib.ru_wgrad3_l(L.f32(x), L.ptr(dy, True), L.f32(dw), n, cin, cout, d, h, wd, flags, int(products), L.ptr(in_scale, True), L.ptr(in_shift, True),
                            float(in_slope), int(dw_cin), int(dw_cout), L.ptr(gb_y, True), L.ptr(gb_d, True), L.ptr(gb_scale, True), L.ptr(gb_shift, True),
                            L.ptr(gb_coef, True), float(gb_slope), L.ptr(gb_out, True), C.byref(inst), L.ptr(ws), ws.numel(), L.stream()), "ru_wgrad3_l")
    return Wgrad3Result(dw, gb_out, inst.value)
