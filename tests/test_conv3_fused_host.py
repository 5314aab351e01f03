"""The float64 restatements that tests/test_conv3_fused.py holds the fused operands of the 3x3x3 convolution family to (Conv3Args: in_scale / in_shift / in_slope,
in_res / in_sum_out, bias, add, sigmoid, stat_partials, bst_*, products, the data-gradient packing), that file's inputs and bars, and the proof -- on the CPU
alone -- that (a) the restatements are the reference's operations, (b) the exact family is exact, (c) the bars can fail.

Restatements (float64, NCDHW): explicit zero padding AFTER the transform, a plain 27-tap loop of einsums over channels, explicit + bias, + add, sigmoid, sums over
the value after `add` and before the sigmoid; the GroupNorm-backward sums are bst_terms of tests/test_pointwise_c16_host.py with d = the convolution output
including `add`; weight_mode 1 is w.transpose(0, 1) with the three tap axes flipped.  Each is compared with the oracle's autograd at 1e-11.

Inputs of the GPU file: CASES below.  Exact family: every operand a small integer or a power of two, slope 0.5 -- test_exact_family_is_exact shows that every
operand, product sum, transformed value, output and sum of summands of the float64 reference is an integer below 2^24, so float32 arithmetic in ANY order gives
the reference exactly.  Real family: seeded normal values, per-sample scale / shift / bst_k, a negative scale in every sample, shifts away from zero.

Mutants (test_mutants_exceed_the_bars_of_the_gpu_tests): the transform applied to the padding; shift of sample 0 used for sample 1; one 16-voxel row dropped from /
counted twice in a sum; statistics before `add`; `u >= thr`; one operand rounded to bf16 (a lost lo x hi product); un-mirrored taps in gradient mode -- each on
the GPU file's own inputs against the GPU file's own bar.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_pointwise_c16_host import bst_terms, draw, draw_bst

U24, U23 = 2.0 ** -24, 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- restatements
def lrelu(x, slope):
    return np.where(x > 0, x, x * slope)


def dgrad_weight(w):
    """weight_mode 1: the forward convolution's [Cf_out, Cf_in, 3, 3, 3] as the weight of its data gradient: channels transposed, taps mirrored"""
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3, 4)[:, :, ::-1, ::-1, ::-1])


def conv3_padded(xp, w):
    """y[n,o,z,y,x] = sum_{c,i,j,k} w[o,c,i,j,k] xp[n,c,z+i,y+j,x+k] on an input that already carries its one-voxel border: torch's float64 cross-correlation
    without padding (test_prologue_... proves it against the explicit tap loop below)"""
    return torch.nn.functional.conv3d(torch.from_numpy(np.ascontiguousarray(xp, np.float64)), torch.from_numpy(np.ascontiguousarray(w, np.float64))).numpy()


def conv3_taps(xp, w):
    """the same as 27 explicit taps"""
    d, h, wd = (s - 2 for s in xp.shape[2:])
    y = 0.0
    for i in range(3):
        for j in range(3):
            for k in range(3):
                y = y + np.einsum("oc,ncdhw->nodhw", w[:, :, i, j, k], xp[:, :, i:i + d, j:j + h, k:k + wd])
    return y


def pad0(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))


def staged(x, scale=None, shift=None, slope=1.0, in_res=None, transform_padding=False):
    """what the convolution reads, border included: pad0(lrelu(x * scale[n,c] + shift[n,c], slope) + in_res); -> (padded, the unpadded sum = in_sum_out).
    Mutant transform_padding: the border is transformed like a voxel of value 0."""
    if scale is None:
        t = x
    else:
        sc, sh = scale[:, :, None, None, None], shift[:, :, None, None, None]
        t = lrelu(x * sc + sh, slope)
    s = t + in_res if in_res is not None else t
    if transform_padding and scale is not None:
        p = lrelu(pad0(x) * sc + sh, slope) + (pad0(in_res) if in_res is not None else 0.0)
        return p, s
    return pad0(s), s


def ref_conv3(x, w, scale=None, shift=None, slope=1.0, in_res=None, bias=None, add=None, sigmoid=False, weight_mode=0, transform_padding=False, mirror=True):
    """-> dict: conv (the convolution term), pre (+ bias + add: what the statistics see), y (the stored output), in_sum.  Mutant mirror = False: weight_mode 1
    without the tap flip."""
    if weight_mode:
        w = dgrad_weight(w) if mirror else np.ascontiguousarray(w.transpose(1, 0, 2, 3, 4))
    xp, s = staged(x, scale, shift, slope, in_res, transform_padding)
    conv = conv3_padded(xp, w)
    pre = conv
    if bias is not None:
        pre = pre + bias[None, :, None, None, None]
    if add is not None:
        pre = pre + add
    y = 1.0 / (1.0 + np.exp(-pre)) if sigmoid else pre
    return dict(conv=conv, pre=pre, y=y, in_sum=s)


def stat_terms(pre):
    """summands of (sum, sumsq) per (sample, channel): [N, C, V, 2]"""
    n, c = pre.shape[:2]
    v = pre.reshape(n, c, -1)
    return np.stack([v, v * v], axis=-1)


def bst_terms_ge(d, bst_y, bst_k, slope):
    """mutant: dh = u >= thr ? d : d*slope"""
    n, c = d.shape[:2]
    d, y = d.reshape(n, c, -1), bst_y.reshape(n, c, -1)
    u = y * bst_k[:, 0, :, None] + bst_k[:, 1, :, None]
    dh = np.where(u >= bst_k[:, 2, :, None], d, d * slope)
    return np.stack([dh, dh * u], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- bars
# class -> (kind, coefficient(s)): the bar the project states for that kernel class on plain launches (tests/test_hip_c16.py, tests/test_hip_ops.py)
CLASS_BARS = {"x3": ("rms", 6e-5), "mx": ("rms", 1.2e-4), "mxg": ("l2max", 2.5e-4, 5e-4), "p1": ("l2", 2.0 ** -8), "f32": ("elem", 1e-5)}


def conv_excess(got, ref, klass, fused=False, sigmoid=False):
    """error / bar of a stored output (<= 1 passes).  ref: ref_conv3's dict.  The convolution term carries the class bar; `fused` (a bias or an `add` joined in
    float32) adds 2^-23 |pre| per element; behind the sigmoid (slope <= 1/4) the whole bar is divided by 4 and 4 * 2^-24 is added for expf."""
    got = np.asarray(got, np.float64)
    conv, pre, y = ref["conv"], ref["pre"], ref["y"]
    assert got.shape == y.shape, (got.shape, y.shape)
    err = np.abs(got - y)
    extra = U23 * np.abs(pre) if fused else 0.0
    bar = CLASS_BARS[klass]
    if bar[0] == "rms":
        b = bar[1] * np.sqrt((conv ** 2).mean()) + extra
    elif bar[0] == "elem":
        b = bar[1] + bar[1] * np.abs(conv) + extra
    else:
        assert not sigmoid
        l2 = np.sqrt((err ** 2).sum()) / (bar[1] * np.sqrt((conv ** 2).sum()) + (U23 * np.sqrt((pre ** 2).sum()) if fused else 0.0))
        if bar[0] == "l2":
            return float(l2)
        return max(float(l2), float((err / (bar[2] * np.abs(conv).max() + extra)).max()))
    if sigmoid:
        b = b / 4 + 4 * U24
    return float((err / b).max())


def in_sum_excess(got, x, scale, shift, slope, in_res):
    """in_sum_out = lrelu(x*scale + shift) + in_res in float32: one rounding each for the product, the sum, the slope and the residual add"""
    sc, sh = scale[:, :, None, None, None], shift[:, :, None, None, None]
    v = x * sc + sh
    t = lrelu(v, slope)
    bar = U24 * (np.abs(x * sc) + np.abs(v) + np.abs(t) + np.abs(t + in_res)) * (1 + 1e-6) + 1e-300
    return float((np.abs(np.asarray(got, np.float64) - (t + in_res)) / bar).max())


def sums_excess(got, terms, length):
    """statistic sums [N, C, 2] (partials added in float64) against the float64 sums of `terms` [N, C, V, 2]: the worst-case float32 summation bound
    length * 2^-24 * sum |term|, length = the number of terms one partial accumulates"""
    got = np.asarray(got, np.float64)
    assert got.shape == terms.shape[:2] + (2,), (got.shape, terms.shape)
    return float((np.abs(got - terms.sum(2)) / (length * U24 * np.abs(terms).sum(2) + 1e-300)).max())


def exact_excess(got, ref):
    """exact family: any difference is a failure (inf), equality is 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return 0.0 if np.array_equal(got, ref) else float("inf")


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases and inputs
def R(family, tz, ty, in16, out16, multi=False, bst=False, add=False, np_=3, head=False, grad=False):
    return (family, tz, ty, in16, out16, multi, bst, add, np_, head, grad)


def case(name, n, cin, cout, dhw, route, klass="x3", **kw):
    c = dict(name=name, n=n, cin=cin, cout=cout, dhw=dhw, route=route, klass=klass, in16=True, out16=True, few=False, split=False, f32=False, act=False, grad=False,
             wm=0, transform=False, res=False, sum_out=False, bias=False, add=False, sigmoid=False, products=0, bst=False, stats=False, exact=False)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


S60, S76, WHOLE, DEEP, WZ, WZR = (30, 30, 60), (30, 30, 76), (32, 64, 64), (16, 32, 64), (32, 32, 32), (32, 30, 44)
SB2 = R("sb2", 4, 8, True, True)
CASES = []
for ex in (True, False):
    tag = "exact" if ex else "real"
    # persistent 16 -> 16: ragged on D, H, W; a whole-tile shape; runs of two tiles (320 tiles on 256 workgroups)
    CASES += [case("sb2_16_scale_stats_" + tag, 2, 16, 16, S60, SB2, transform=True, stats=True, exact=ex),
              case("sb2_16_add_stats_" + tag, 2, 16, 16, S60, R("sb2", 4, 8, True, True, add=True), add=True, stats=True, exact=ex),
              case("sb2_16_whole_scale_add_stats_" + tag, 1, 16, 16, WHOLE, R("sb2", 4, 8, True, True, add=True), transform=True, add=True, stats=True, exact=ex),
              case("sb2_16_runs_bst_add_" + tag, 2, 16, 16, S76, R("sb2", 4, 8, True, True, bst=True, add=True), split=True, wm=1, bst=True, add=True, exact=ex)]
    # data-gradient mode: split-form input, all four (BST, ADD), 16 -> 16 and 32 -> 32 (MULTI); one product with BST + ADD
    for b in (False, True):
        for a in (False, True):
            CASES += [case("dgrad_split_16_b%d_a%d_%s" % (b, a, tag), 2, 16, 16, S60, R("sb2", 4, 8, True, True, bst=b, add=a), split=True, wm=1, bst=b, add=a, exact=ex),
                      case("dgrad_split_32_b%d_a%d_%s" % (b, a, tag), 2, 32, 32, DEEP, R("sb2", 4, 8, True, True, multi=True, bst=b, add=a), split=True, wm=1, bst=b, add=a,
                           exact=ex)]
    CASES += [case("dgrad_p1_16_" + tag, 2, 16, 16, S60, R("sb2", 4, 8, True, True, bst=True, add=True, np_=1), klass="p1", split=True, wm=1, bst=True, add=True, products=1,
                   exact=ex),
              case("dgrad_p1_32_" + tag, 2, 32, 32, DEEP, R("sb2", 4, 8, True, True, multi=True, bst=True, add=True, np_=1), klass="p1", split=True, wm=1, bst=True, add=True,
                   products=1, exact=ex)]
    # persistent MULTI forward, 64 -> 32: `add` keeps it off the Winograd-z route
    CASES += [case("sb2_64_32_scale_add_stats_" + tag, 2, 64, 32, DEEP, R("sb2", 4, 8, True, True, multi=True, add=True), transform=True, add=True, stats=True, exact=ex)]
    # one-stage tiles (2,4), (2,2) with W % 4 != 0 on the voxel-major pair; (2,8) through bias + voxel-major output (no statistics there: refused by design)
    CASES += [case("sb_24_scale_add_stats_" + tag, 1, 16, 16, (8, 16, 18), R("sb", 2, 4, True, True), transform=True, add=True, stats=True, exact=ex),
              case("sb_22_scale_add_stats_" + tag, 1, 64, 64, (8, 16, 30), R("sb", 2, 2, True, True), transform=True, add=True, stats=True, exact=ex),
              case("sb_28_scale_add_bias_" + tag, 2, 16, 16, (30, 30, 62), R("sb", 2, 8, True, True), transform=True, add=True, bias=True, exact=ex),
              case("sb_24_ncdhw_scale_add_stats_" + tag, 1, 16, 16, (8, 16, 16), R("sb", 2, 4, False, False), in16=False, out16=False, transform=True, add=True, stats=True,
                   exact=ex)]
    # stem: 4 and 3 channels through the 4-channel copy (sb2c4 <true, false>), and the head's data gradient 3 -> 16 with the GroupNorm-backward sums (<true, true>)
    CASES += [case("stem_c4_stats_" + tag, 2, 4, 16, S60, R("sb2c4", 4, 8, False, True), in16=False, few=True, stats=True, exact=ex),
              case("stem_c3_stats_" + tag, 2, 3, 16, S60, R("sb2c4", 4, 8, False, True), in16=False, few=True, stats=True, exact=ex),
              case("head_dgrad_c3_bst_" + tag, 2, 3, 16, S60, R("sb2c4", 4, 8, False, True, bst=True), in16=False, few=True, wm=1, bst=True, exact=ex)]
    # exact-f32 voxel-major kernel: its three tiles with in_scale + statistics, the NCDHW stem
    CASES += [case("f32c_48_scale_stats_" + tag, 2, 16, 16, S60, R("f32c", 4, 8, True, True), klass="f32", f32=True, transform=True, stats=True, exact=ex),
              case("f32c_28_scale_stats_" + tag, 1, 16, 16, (31, 30, 60), R("f32c", 2, 8, True, True), klass="f32", f32=True, transform=True, stats=True, exact=ex),
              case("f32c_24_scale_stats_" + tag, 1, 32, 16, (8, 16, 18), R("f32c", 2, 4, True, True), klass="f32", f32=True, transform=True, stats=True, exact=ex),
              case("f32c_stem_stats_" + tag, 2, 4, 16, S60, R("f32c", 4, 8, False, True), klass="f32", f32=True, in16=False, stats=True, exact=ex)]
    # Winograd-z (in_scale + statistics are the only fused operands it takes), the fp16 + MX-fp8 forward kernels, the gradient-operand kernel
    CASES += [case("wz32_scale_stats_" + tag, 2, 32, 32, WZ, R("wz32", 2, 8, True, True, multi=True), transform=True, stats=True, exact=ex),
              case("wz32_ragged_scale_stats_" + tag, 2, 32, 32, WZR, R("wz32", 2, 8, True, True, multi=True), transform=True, stats=True, exact=ex),
              case("wz32mx_scale_stats_" + tag, 2, 32, 32, WZR, R("wz32mx", 2, 8, True, True, multi=True), klass="mx", act=True, transform=True, stats=True, exact=ex),
              case("mx_scale_stats_" + tag, 2, 16, 16, S60, R("mx", 4, 8, True, True), klass="mx", act=True, transform=True, stats=True, exact=ex)]
    for b in (False, True):
        for a in (False, True):
            CASES += [case("mxg_b%d_a%d_%s" % (b, a, tag), 2, 16, 16, S60, R("mx", 4, 8, True, True, bst=b, add=a, grad=True), klass="mxg", grad=True, wm=1, bst=b, add=a,
                           exact=ex)]
# head: 16 -> 3 and 16 -> 1, voxel-major in, NCDHW out, bias + sigmoid; with the last Residual block formed in the staging and without; the exact-f32 head form
HEAD = R("sb2", 4, 8, True, False, head=True)
for ex in (True, False):
    tag = "exact" if ex else "real"
    CASES += [case("head3_res_sum_" + tag, 2, 16, 3, S60, HEAD, out16=False, transform=True, res=True, sum_out=True, bias=True, sigmoid=True, exact=ex),
              case("head1_res_sum_" + tag, 2, 16, 1, S60, HEAD, out16=False, transform=True, res=True, sum_out=True, bias=True, sigmoid=True, exact=ex),
              case("head3_plain_" + tag, 2, 16, 3, S60, HEAD, out16=False, bias=True, sigmoid=True, exact=ex),
              case("head3_f32c_res_" + tag, 2, 16, 3, S60, R("f32c", 4, 8, True, False, head=True), klass="f32", f32=True, out16=False, transform=True, res=True, bias=True,
                   sigmoid=True, exact=ex)]
# the 16 -> 1 head without the Residual block; the (2,2) one-stage tile on whole tiles (W % 16 == 0)
for ex in (True, False):
    tag = "exact" if ex else "real"
    CASES += [case("head1_plain_" + tag, 2, 16, 1, S60, HEAD, out16=False, bias=True, sigmoid=True, exact=ex),
              case("sb_22_whole_scale_add_stats_" + tag, 1, 64, 64, (8, 16, 32), R("sb", 2, 2, True, True), transform=True, add=True, stats=True, exact=ex)]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
EXACT_SLOPE, REAL_SLOPE = 0.5, 0.01


def _ints(seed, lo, hi, *shape):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, shape, generator=g).numpy().astype(np.float32)


def _pick(seed, values, *shape):
    return np.asarray(values, np.float32)[_ints(seed, 0, len(values) - 1, *shape).astype(np.int64)]


def split_value(x):
    """what the split form hi + lo holds of a float32 tensor (ops.to_split_c16's arithmetic), in float64"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy().astype(np.float64) + lo.numpy().astype(np.float64)


def make_inputs(c):
    """float32 numpy operands of a case (what the device is fed), keyed like ops.conv3_fused's arguments; seeds derive from the case's position"""
    seed = 1000 + 20 * CASES.index(c)
    n, cin, cout, sp = c["n"], c["cin"], c["cout"], c["dhw"]
    wshape = (cin, cout, 3, 3, 3) if c["wm"] else (cout, cin, 3, 3, 3)
    i = {}
    if c["exact"]:
        even = 2.0 if c["bst"] else 1.0                               # d * slope stays an integer
        i["x"] = _ints(seed, -1, 1, n, cin, *sp) if c["transform"] else _ints(seed, -2, 2, n, cin, *sp)
        nz = _ints(seed + 1, 0, 16 * cin - 1, *wshape) == 0            # sparse weights (one to two taps per output channel) keep every sum of squares below 2^24
        i["w"] = (_pick(seed + 2, [-1, 1], *wshape) * nz * even).astype(np.float32)
        if c["transform"]:
            i["scale"] = _pick(seed + 3, [-2, 2], n, cin)             # even: a negative x*scale + shift times the slope 0.5 stays an integer
            i["scale"][:, 0] = -2.0
            i["shift"] = _pick(seed + 4, [-2, 2], n, cin)
        if c["res"]:
            i["res"] = _ints(seed + 5, -2, 2, n, cin, *sp)
        if c["bias"]:
            i["bias"] = _ints(seed + 6, -3, 3, cout) * even
        if c["add"]:
            i["add"] = _ints(seed + 7, -3, 3, n, cout, *sp) * even
        if c["bst"]:
            i["bst_y"] = _ints(seed + 8, -3, 3, n, cout, *sp)
            i["bst_k"] = np.stack([_pick(seed + 9, [-2, -1, 1, 2], n, cout), _ints(seed + 10, -2, 2, n, cout), _ints(seed + 11, -1, 1, n, cout)], axis=1)
    else:
        i["x"] = draw(seed, n, cin, *sp)
        i["w"] = draw(seed + 1, *wshape, scale=(27 * cin) ** -0.5)
        if c["transform"]:
            s = draw(seed + 3, n, cin)
            i["scale"] = (np.where(s < 0, -1.0, 1.0) * (0.5 + np.abs(s))).astype(np.float32)
            i["scale"][:, 0] = -np.abs(i["scale"][:, 0])
            h = draw(seed + 4, n, cin) * 0.5
            i["shift"] = np.where(np.abs(h) < 0.1, np.where(h < 0, -0.1, 0.1), h).astype(np.float32)
        if c["res"]:
            i["res"] = draw(seed + 5, n, cin, *sp)
        if c["bias"]:
            i["bias"] = draw(seed + 6, cout)
        if c["add"]:
            i["add"] = draw(seed + 7, n, cout, *sp)
        if c["bst"]:
            i["bst_y"], i["bst_k"] = draw_bst(seed + 8, n, cout, sp)
    return i


def reference(c, i, **mutant):
    """ref_conv3 of a case in float64; a split-form input is what hi + lo holds"""
    f8 = lambda a: None if a is None else np.asarray(a, np.float64)
    x = split_value(i["x"]) if c["split"] else f8(i["x"])
    return ref_conv3(x, f8(i["w"]), f8(i.get("scale")), f8(i.get("shift")), case_slope(c), f8(i.get("res")), f8(i.get("bias")), f8(i.get("add")), c["sigmoid"],
                     c["wm"], **mutant)


def case_slope(c):
    return EXACT_SLOPE if c["exact"] else REAL_SLOPE


def case_terms(c, i, ref):
    """float64 summands [N, C, V, 2] of the statistics a case asks for, from the value `ref['pre']` (or any array passed as ref)"""
    pre = ref["pre"] if isinstance(ref, dict) else ref
    if c["bst"]:
        t, margin = bst_terms(pre, i["bst_y"].astype(np.float64), i["bst_k"].astype(np.float64), case_slope(c))
        assert c["exact"] or margin >= 1e-3, margin
        return t
    return stat_terms(pre)


def partial_length(c, nblk):
    """terms one statistics partial accumulates at most: whole tiles of a workgroup's run x the voxels of a tile"""
    tz, ty = c["route"][1], c["route"][2]
    d, h, w = c["dhw"]
    if c["route"][0] in ("wz32", "wz32mx"):
        ntile, tile = (d // 2) * -(-h // 8) * -(-w // 16), 2 * 8 * 16
    else:
        ntile, tile = -(-d // tz) * -(-h // ty) * -(-w // 16), tz * ty * 16
    if c["route"][0] == "sb":
        return tile                                                   # one-stage kernel: one partial per tile
    return -(-c["n"] * ntile // nblk) * tile


# ---------------------------------------------------------------------------------------------------------------- restatements against the oracle
def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


def _gn(x, gamma, beta):
    """GroupNorm as (scale, shift) [N, C] and (mean, rstd) [N, C] in float64"""
    n, c = x.shape[:2]
    cpg = c // O.GN_GROUPS
    xg = x.reshape(n, O.GN_GROUPS, -1)
    mean, rstd = np.repeat(xg.mean(-1), cpg, 1), np.repeat(1.0 / np.sqrt(xg.var(-1) + O.GN_EPS), cpg, 1)
    return gamma[None] * rstd, beta[None] - gamma[None] * rstd * mean, mean, rstd


SMALL = [(2, 16, 8, (3, 4, 5)), (1, 8, 16, (2, 5, 3))]                 # N, Cin, Cout, spatial


def _small(si, n, cin, cout, sp):
    x, w, b = (draw(500 + 10 * si + t, *s).astype(np.float64) for t, s in enumerate([(n, cin) + sp, (cout, cin, 3, 3, 3), (cout,)]))
    gamma = draw(503 + 10 * si, cin).astype(np.float64) + np.where(np.arange(cin) % 2 == 0, 1.0, -1.0) * 1.5      # both signs
    beta = draw(504 + 10 * si, cin).astype(np.float64) * 0.5 + 0.2
    return x, w, b, gamma, beta


def test_prologue_and_epilogue_restatement_is_groupnorm_lrelu_conv3d():
    """GroupNorm -> LeakyReLU -> Conv3d (+ bias) + residual -> sigmoid, model.py:72-73 order; the padding is Conv3d's own, i.e. applied after the transform"""
    for si, (n, cin, cout, sp) in enumerate(SMALL):
        x, w, b, gamma, beta = _small(si, n, cin, cout, sp)
        add = draw(505 + 10 * si, n, cout, *sp).astype(np.float64)
        scale, shift, _, _ = _gn(x, gamma, beta)
        z = O.leaky_relu(O.group_norm(_t(x), _t(gamma), _t(beta)))
        pre = torch.nn.functional.conv3d(z, _t(w), _t(b), padding=1) + _t(add)
        r = ref_conv3(x, w, scale, shift, O.LEAKY_SLOPE, bias=b, add=add, sigmoid=True)
        _close(r["pre"], pre.numpy())
        _close(r["y"], torch.sigmoid(pre).numpy())
        _close(r["in_sum"], z.numpy())
        _close(conv3_taps(pad0(r["in_sum"]), w), r["conv"])
        _close(stat_terms(r["pre"]).sum(2)[..., 0], pre.numpy().reshape(n, cout, -1).sum(-1), 1e-10)
        _close(stat_terms(r["pre"]).sum(2)[..., 1], (pre.numpy() ** 2).reshape(n, cout, -1).sum(-1), 1e-10)


def test_data_gradient_packing_is_the_input_gradient_of_conv3d():
    """autograd's input gradient of Conv3d is the convolution of dy with the transposed, mirrored weight (weight_mode 1), `add` joining a skip gradient"""
    for si, (n, cin, cout, sp) in enumerate(SMALL):
        x, w, _, _, _ = _small(si, n, cin, cout, sp)
        dy, skip = draw(506 + 10 * si, n, cout, *sp).astype(np.float64), draw(507 + 10 * si, n, cin, *sp).astype(np.float64)
        tx = _t(x, True)
        (torch.nn.functional.conv3d(tx, _t(w), padding=1) * _t(dy)).sum().backward()
        _close(ref_conv3(dy, w, add=skip, weight_mode=1)["pre"], tx.grad.numpy() + skip)
        _close(conv3_padded(pad0(dy), dgrad_weight(w)), tx.grad.numpy())


def test_fused_backward_sums_are_the_group_norm_backward_of_the_data_gradient():
    """z = leaky_relu(group_norm(a)); out = conv3d(z): the data gradient d of the conv (weight_mode 1) with bst_y = a and the constants the engine publishes
    (k1 = sign(gamma) rstd, k2 = -sign(gamma) mean rstd, thr = -beta / |gamma|) gives dbeta = S1 and dgamma = sign(gamma) S2'"""
    for si, (n, cin, cout, sp) in enumerate(SMALL):
        a, w, _, gamma, beta = _small(si, n, cin, cout, sp)
        dy = draw(508 + 10 * si, n, cout, *sp).astype(np.float64)
        _, _, mean, rstd = _gn(a, gamma, beta)
        sg = np.sign(gamma)[None, :]
        k = np.stack([sg * rstd, -sg * mean * rstd, np.broadcast_to((-beta / np.abs(gamma))[None, :], (n, cin))], axis=1)
        d = ref_conv3(dy, w, weight_mode=1)["pre"]
        terms, margin = bst_terms(d, a, k, O.LEAKY_SLOPE)
        assert margin > 1e-7
        sums = terms.sum(2)
        for s in range(n):
            tg, tb = _t(gamma, True), _t(beta, True)
            z = O.leaky_relu(O.group_norm(_t(a[s:s + 1]), tg, tb))
            (torch.nn.functional.conv3d(z, _t(w), padding=1) * _t(dy[s:s + 1])).sum().backward()
            _close(sums[s, :, 0], tb.grad.numpy(), 1e-9)
            _close(sums[s, :, 1] * np.sign(gamma), tg.grad.numpy(), 1e-9)


def test_in_res_restatement_is_the_residual_block_before_the_head():
    """model.py:112-116: the block's output x + relu2(norm2(conv2)) is what the head convolution reads; in_res = x, the transform = norm2 + LeakyReLU of conv2's output,
    in_sum_out = the block output, and the padding applies to the sum"""
    for si, (n, cin, cout, sp) in enumerate([(2, 16, 3, (3, 4, 5)), (1, 16, 1, (2, 5, 3))]):
        y2, w, b, gamma, beta = _small(si, n, cin, cout, sp)
        xin = draw(509 + 10 * si, n, cin, *sp).astype(np.float64)
        scale, shift, _, _ = _gn(y2, gamma, beta)
        block = _t(xin) + O.leaky_relu(O.group_norm(_t(y2), _t(gamma), _t(beta)))
        out = torch.sigmoid(torch.nn.functional.conv3d(block, _t(w), _t(b), padding=1))
        r = ref_conv3(y2, w, scale, shift, O.LEAKY_SLOPE, in_res=xin, bias=b, sigmoid=True)
        _close(r["in_sum"], block.numpy())
        _close(r["y"], out.numpy())


# ---------------------------------------------------------------------------------------------------------------- the exact family
def _is_int_below(a, what, bound=2.0 ** 24):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a, np.round(a)), what
    assert float(np.abs(a).max(initial=0.0)) < bound, (what, float(np.abs(a).max()))


EXACT_CASES = [c["name"] for c in CASES if c["exact"]]


@pytest.mark.parametrize("name", EXACT_CASES)
def test_exact_family_is_exact(name):
    """every exact case the GPU file asserts equality on: operands, transformed values, the staged sum, the sums of |product| of every output, the outputs, every
    summand of the statistics and the sum of |summand| per (sample, channel) are integers below 2^24: float32 arithmetic gives them exactly in any order, and the
    split form holds every operand in its hi half"""
    c = CASE_BY_NAME[name]
    i = make_inputs(c)
    for k, v in i.items():
        _is_int_below(v, (name, k), 256.0)
        assert np.array_equal(torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy(), v), (name, k)        # 8 significant bits: lo = 0
    assert not c["transform"] or (i["shift"] != 0).all() and (i["scale"] < 0).any(1).all()
    r = reference(c, i)
    for k in ("conv", "pre", "in_sum"):
        _is_int_below(r[k], (name, k))
    f8 = lambda a: np.asarray(a, np.float64)
    wabs = np.abs(dgrad_weight(f8(i["w"])) if c["wm"] else f8(i["w"]))
    mag = conv3_padded(pad0(np.abs(r["in_sum"])), wabs) + (np.abs(f8(i["bias"]))[None, :, None, None, None] if c["bias"] else 0.0) + (np.abs(f8(i["add"])) if c["add"] else 0.0)
    _is_int_below(mag, (name, "sum of |product|"))
    if c["stats"] or c["bst"]:
        t = case_terms(c, i, r)
        _is_int_below(t, (name, "summands"))
        _is_int_below(np.abs(t).sum(2), (name, "sum of |summand|"))
    if c["bst"]:                                                  # ties u == thr exist, so `>` against `>=` is visible
        u = f8(i["bst_y"]) * f8(i["bst_k"])[:, 0, :, None, None, None] + f8(i["bst_k"])[:, 1, :, None, None, None]
        assert (u == f8(i["bst_k"])[:, 2, :, None, None, None]).any(), name


def test_real_family_draws_what_the_gpu_file_promises():
    for c in CASES:
        if c["exact"] or c["dhw"] != S60:
            continue
        i = make_inputs(c)
        if c["transform"]:
            assert (i["scale"] < 0).any(1).all() and float(np.abs(i["shift"]).min()) >= 0.1 and not np.array_equal(i["scale"][0], i["scale"][1])
        if c["bst"]:
            assert not np.array_equal(i["bst_k"][0], i["bst_k"][1])
            _, margin = bst_terms(np.ones(i["bst_y"].shape), i["bst_y"].astype(np.float64), i["bst_k"].astype(np.float64))
            assert margin >= 1e-3


# ---------------------------------------------------------------------------------------------------------------- mutants
def test_mutants_exceed_the_bars_of_the_gpu_tests():
    """each mutant on a GPU case's own inputs against that case's own bar (the unmutated restatement has excess 0 by construction)"""
    rows = []
    f8 = lambda a: np.asarray(a, np.float64)
    for name in ("sb_24_scale_add_stats_real", "sb_24_scale_add_stats_exact"):
        c = CASE_BY_NAME[name]
        i = make_inputs(c)
        good = reference(c, i)
        exc = (lambda got, ref: exact_excess(got, ref["y"])) if c["exact"] else (lambda got, ref: conv_excess(got, ref, c["klass"], fused=True))
        rows.append(("transform applied to the padding, %s" % name, exc(reference(c, i, transform_padding=True)["y"], good)))
        terms = case_terms(c, i, good)
        length = partial_length(c, 0)
        sums = lambda t: exact_excess(t.sum(2), terms.sum(2)) if c["exact"] else sums_excess(t.sum(2), terms, length)
        # one 16-voxel row (the last of the volume) dropped / counted twice: against the summation bar of the whole sample's sum, and against equality
        rows.append(("one row dropped from a sum, %s" % name, sums(terms[:, :, :-16])))
        rows.append(("one row counted twice, %s" % name, sums(np.concatenate([terms, terms[:, :, -16:]], axis=2))))
        rows.append(("statistics before add, %s" % name, sums(stat_terms(good["pre"] - f8(i["add"])))))
    # the same lost / doubled row at the largest sum of the file, 2 x 30 x 30 x 60 with runs of one tile: equality sees it, and so does the summation bar
    for name in ("sb2_16_scale_stats_exact", "sb2_16_scale_stats_real"):
        c = CASE_BY_NAME[name]
        i = make_inputs(c)
        terms = case_terms(c, i, reference(c, i))
        sums = lambda t: exact_excess(t.sum(2), terms.sum(2)) if c["exact"] else sums_excess(t.sum(2), terms, partial_length(c, 256))
        rows.append(("one row dropped from a sum, %s" % name, sums(terms[:, :, :-16])))
        rows.append(("one row counted twice, %s" % name, sums(np.concatenate([terms, terms[:, :, -16:]], axis=2))))
    # shift of sample 0 used for sample 1
    c = CASE_BY_NAME["sb2_16_scale_stats_real"]
    i = make_inputs(c)
    good = reference(c, i)
    bad = dict(i, shift=np.stack([i["shift"][0], i["shift"][0]]))
    rows.append(("shift of sample 0 used for sample 1", conv_excess(reference(c, bad)["y"], good, "x3")))
    # the lo x hi product dropped: one operand rounded to bf16
    lost = dict(i, x=torch.from_numpy(i["x"]).to(torch.bfloat16).to(torch.float32).numpy())
    rows.append(("lo x hi product dropped", conv_excess(reference(c, lost)["y"], good, "x3")))
    # u >= thr on the exact family's ties; un-mirrored taps in gradient mode
    for name in ("dgrad_split_16_b1_a1_exact", "dgrad_split_16_b1_a1_real"):
        c = CASE_BY_NAME[name]
        i = make_inputs(c)
        good = reference(c, i)
        if c["exact"]:
            terms = case_terms(c, i, good)
            ge = bst_terms_ge(good["pre"], f8(i["bst_y"]), f8(i["bst_k"]), case_slope(c))
            rows.append(("u >= thr, %s" % name, exact_excess(ge.sum(2), terms.sum(2))))
            rows.append(("un-mirrored taps, %s" % name, exact_excess(reference(c, i, mirror=False)["y"], good["y"])))
        else:
            rows.append(("un-mirrored taps, %s" % name, conv_excess(reference(c, i, mirror=False)["y"], good, "x3", fused=True)))
    for name, ex in rows:
        print("  mutant %-66s error / bar %.3g" % (name, ex))
    for name, ex in rows:
        assert ex > 1.0, (name, ex)
