"""The float64 restatements that tests/test_ncdhw_convs.py holds the NCDHW convolution family to -- conv3_f32_kernel<TZ, TY, KC, NT> and its split-K form
(csrc/conv3_f32.hip), wgrad3_f32_kernel / wgrad1_f32_kernel / wgrad_reduce_kernel (csrc/wgrad_f32.hip), the NCDHW and mixed-layout wgrad3_sb_kernel
(csrc/wgrad_sb.hip), conv1_launch's three routes with the transposes and s2d_kernel / d2s_kernel (csrc/pointwise.hip) -- that file's cases, inputs and bars, and the
proof, on the CPU alone, that (a) the restatements are the reference's operations, (b) the exact family is exact, (c) every case reaches the instantiation it was
written for, (d) every bar can fail.

Restatements (float64, NCDHW, cross-correlation, zero padding):
  k = 3 forward     y[n][o][v] = bias[o] + sum_{c,tap} w[o][c][tap] pad0(x)[n][c][v + tap]                 27 explicit taps, one matrix product each
  k = 3 data grad   dx = the forward of dy with w's channels exchanged and its taps mirrored
  k = 3 weight grad dw[o][c][tap] = sum_{n,v} dy[n][o][v] pad0(x)[n][c][v + tap],  db[o] = sum_{n,v} dy[n][o][v]
  k = 1             y = W x per voxel, dx = W^T dy, dw = sum_{n,v} dy x^T
  k = 2, stride 2   the same three on the space-to-depth tensor (channel c*8 + tap at the coarse voxel), w read as [Cout][Cin*8]: the reference's [Cout][Cin][2][2][2] order
  split-K           sum, in slice order, of the forwards over the ksplit slices of the 8-channel input chunks
each proven against the oracle's autograd in float64 (oracle/resunet_oracle.py: conv3x3x3, conv1x1x1, conv2x2x2_s2) on small ragged shapes.

Bars (error / bar <= 1 passes) -- the project's float32 contract (tests/test_hip_ops.py) and the three-product bar of tests/test_wgrad3_fused.py; none is derived
from a measurement:
  forward and data-gradient tensors   1e-5 + 1e-5 |ref| per element
  dw, db                              2e-4 max |ref|
  three-product split-bf16 dw         2e-5 max |ref| per element

Two input families per case.  exact: x, dy in {-2 .. 2}, w and bias in {-1, -1/2, 0, 1/2, 1}; test_exact_family_is_exact proves per case that every operand is a
multiple of the case's unit (1/2 where a weight is an operand, 1 for the weight gradients), that (number of products) * max |a| * max |b| + max |bias| -- a bound of
the sum of |product| of any output element, hence of every partial sum in any order -- stays below 2^24 units, and that every operand is a bf16 value (hi exact,
lo == 0): float32 arithmetic in any order, and the three split-bf16 products, give the reference exactly.  real: seeded normal values, weights scaled by
(k^3 Cin)^-1/2.

Mutants of the reference (test_every_bar_can_fail): one tap of the stencil's border dropped, the data gradient's taps left un-mirrored, one tile of a walk
dropped, one split-K slice dropped, the two halves of an OT = 2 pair exchanged.  Each breaks exact equality; each exceeds the real bar, "one tile of 600" included
(the test prints every mutant's error / bar: the tile of 600 is 91 times the bar on these inputs -- recorded, not asserted, as the only mutant whose size
shrinks with the walk's length; the smallest of the others is the tile of 24 at 291).
Nothing here needs a GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O


# ---------------------------------------------------------------------------------------------------------------- restatements
def pad0(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))


def ref_conv3(x, w, bias=None, drop_tap=None):
    """k = 3 forward.  Mutant drop_tap: that tap (0 .. 26) is left out."""
    n, ci, d, h, wd = x.shape
    co = w.shape[0]
    xp = pad0(np.asarray(x, np.float64))
    w = np.asarray(w, np.float64)
    y = np.zeros((n, co, d * h * wd))
    for tap in range(27):
        if tap == drop_tap:
            continue
        i, j, k = tap // 9, (tap // 3) % 3, tap % 3
        y += np.matmul(w[:, :, i, j, k], xp[:, :, i:i + d, j:j + h, k:k + wd].reshape(n, ci, -1))
    if bias is not None:
        y += np.asarray(bias, np.float64)[None, :, None]
    return y.reshape(n, co, d, h, wd)


def ref_dgrad3(dy, w, mirror=True):
    """k = 3 data gradient.  Mutant mirror = False: the taps are not mirrored."""
    wt = np.asarray(w, np.float64).transpose(1, 0, 2, 3, 4)
    return ref_conv3(dy, np.ascontiguousarray(wt[:, :, ::-1, ::-1, ::-1] if mirror else wt))


def ref_wgrad3(x, dy, drop_tile=None):
    """k = 3 weight gradient.  Mutant drop_tile = (n, z0, y0, x0, tz, ty): the voxels of that tile (tz x ty x 16) contribute nothing."""
    n, ci, d, h, wd = x.shape
    co = dy.shape[1]
    xp = pad0(np.asarray(x, np.float64))
    g = np.array(dy, np.float64)
    if drop_tile is not None:
        s, z0, y0, x0, tz, ty = drop_tile
        g[s, :, z0:z0 + tz, y0:y0 + ty, x0:x0 + 16] = 0.0
    g = g.reshape(n, co, -1)
    dw = np.zeros((co, ci, 3, 3, 3))
    for tap in range(27):
        i, j, k = tap // 9, (tap // 3) % 3, tap % 3
        xs = xp[:, :, i:i + d, j:j + h, k:k + wd].reshape(n, ci, -1)
        dw[:, :, i, j, k] = np.matmul(g, xs.transpose(0, 2, 1)).sum(0)
    return dw


def ref_db(dy):
    return np.asarray(dy, np.float64).sum((0, 2, 3, 4))


def swap_ot_halves(dw):
    """mutant: output channels 16 q .. 16 q + 15 and 16 (q ^ 1) .. exchanged within every complete pair of 16-channel blocks"""
    out = np.array(dw)
    for o0 in range(0, dw.shape[0] - 31, 32):
        out[o0:o0 + 16], out[o0 + 16:o0 + 32] = dw[o0 + 16:o0 + 32], dw[o0:o0 + 16]
    return out


def splitk_slices(cin, ks):
    """channel ranges of the ks slices: CinP = Cin rounded up to 8, CinP / ks channels each (the launcher refuses a factor that does not divide the chunks)"""
    cinp = -(-cin // 8) * 8
    assert (cinp // 8) % ks == 0
    span = cinp // ks
    return [(z * span, min((z + 1) * span, cin)) for z in range(ks)]


def ref_splitk(x, w, ks, drop_slice=None):
    """split-K forward: the per-slice forwards summed in slice order.  Mutant drop_slice."""
    y = 0.0
    for z, (a, b) in enumerate(splitk_slices(x.shape[1], ks)):
        if z != drop_slice and b > a:
            y = y + ref_conv3(x[:, a:b], w[:, a:b])
    return y


def ref_conv1(x, w):
    n, ci = x.shape[:2]
    w2 = np.asarray(w, np.float64).reshape(w.shape[0], ci)
    return np.matmul(w2, np.asarray(x, np.float64).reshape(n, ci, -1)).reshape((n, w.shape[0]) + x.shape[2:])


def ref_dgrad1(dy, w):
    n, co = dy.shape[:2]
    w2 = np.asarray(w, np.float64).reshape(co, -1)
    return np.matmul(w2.T, np.asarray(dy, np.float64).reshape(n, co, -1)).reshape((n, w2.shape[1]) + dy.shape[2:])


def ref_wgrad1(x, dy):
    n, ci = x.shape[:2]
    co = dy.shape[1]
    return np.matmul(np.asarray(dy, np.float64).reshape(n, co, -1), np.asarray(x, np.float64).reshape(n, ci, -1).transpose(0, 2, 1)).sum(0)


def s2d(x):
    """[N][C][D][H][W] -> [N][C*8][D/2][H/2][W/2], channel c*8 + (i*4 + j*2 + k) = fine voxel (2z+i, 2y+j, 2x+k)"""
    n, c, d, h, w = x.shape
    t = x.reshape(n, c, d // 2, 2, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 5, 7, 2, 4, 6)
    return np.ascontiguousarray(t).reshape(n, c * 8, d // 2, h // 2, w // 2)


def d2s(t, c):
    n, _, dc, hc, wc = t.shape
    x = t.reshape(n, c, 2, 2, 2, dc, hc, wc).transpose(0, 1, 5, 2, 6, 3, 7, 4)
    return np.ascontiguousarray(x).reshape(n, c, 2 * dc, 2 * hc, 2 * wc)


def ref_conv2(x, w):
    return ref_conv1(s2d(np.asarray(x, np.float64)), np.asarray(w, np.float64).reshape(w.shape[0], -1))


def ref_dgrad2(dy, w):
    return d2s(ref_dgrad1(dy, np.asarray(w, np.float64).reshape(w.shape[0], -1)), w.shape[1])


def ref_wgrad2(x, dy):
    return ref_wgrad1(s2d(np.asarray(x, np.float64)), dy).reshape(dy.shape[1], x.shape[1], 2, 2, 2)


# ---------------------------------------------------------------------------------------------------------------- bars
def _pair(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return got, ref


def tensor_excess(got, ref):
    """forward and data-gradient tensors: worst |got - ref| / (1e-5 + 1e-5 |ref|) over every element"""
    got, ref = _pair(got, ref)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))).max())


def reduction_excess(got, ref, rel=2e-4):
    """dw and db: worst |got - ref| / (rel * max |ref|); rel = 2e-5 for the three-product split-bf16 dw"""
    got, ref = _pair(got, ref)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - ref).max() / (rel * np.abs(ref).max()))


def sb_excess(got, ref):
    return reduction_excess(got, ref, 2e-5)


def exact_excess(got, ref):
    got, ref = _pair(got, ref)
    return 0.0 if np.array_equal(got, ref) else float("inf")


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases
# conv3_f32_kernel<TZ, TY, KC, NT>
I4841, I2481, I2482, I2881, I2882, I4881, I4882 = (4, 8, 4, 1), (2, 4, 8, 1), (2, 4, 8, 2), (2, 8, 8, 1), (2, 8, 8, 2), (4, 8, 8, 1), (4, 8, 8, 2)
CONV3_INSTS = (I4841, I2481, I2482, I2881, I2882, I4881, I4882)              # conv3_launch's dispatch table
MFMA, K14, K416 = "conv1_mfma_kernel", "conv1_kernel<1,4>", "conv1_kernel<4,16>"
BIG = (23, 63, 125)          # 12 x 8 x 8 = 768 tiles of (2, 8, 16), 384 of (4, 8, 16) per sample
CASES = []


def _add(kind, name, n, cin, cout, dhw, **kw):
    base = dict(kind=kind, n=n, cin=cin, cout=cout, dhw=dhw, bias=False, precision="f32", x_c16=False, dy_c16=False, ksplit=0, walk=False)
    assert set(kw) - {"fwd", "dgrad", "w3", "w1", "nparts", "db"} <= set(base), kw
    for exact in (True, False):
        CASES.append(dict(base, name="%s_%s" % (name, "exact" if exact else "real"), exact=exact, **kw))


# ---- conv3_f32_kernel, forward (pack mode 0) and data gradient (pack mode 1: Cout -> Cin channels, so its instantiation is that of the exchanged pair)
_add("conv3", "c3_3_16_w18", 1, 3, 16, (5, 9, 18), fwd=I4841, dgrad=I2481)
_add("conv3", "c3_4_8", 2, 4, 8, (5, 7, 18), fwd=I4841, dgrad=I2481)
_add("conv3", "c3_8_16", 1, 8, 16, (5, 7, 18), fwd=I2481, dgrad=I2481)
_add("conv3", "c3_24_40", 1, 24, 40, (5, 7, 18), fwd=I2481, dgrad=I2481)          # three chunks; Cout pad 48 at nt = 1: a half-dead last block
_add("conv3", "c3_16_3_bias", 1, 16, 3, (5, 7, 18), bias=True, fwd=I2481, dgrad=I4841)
_add("conv3", "c3_8_32_512", 1, 8, 32, (31, 30, 62), fwd=I2482, dgrad=I2481)       # 16 x 8 x 4 = 512 workgroups of (2, 4) at nt = 2
_add("conv3", "c3_8_16_big", 1, 8, 16, BIG, fwd=I2881, dgrad=I2881)
_add("conv3", "c3_8_16_big_n2", 2, 8, 16, BIG, fwd=I4881, dgrad=I4881)             # 768 workgroups of (4, 8): the tile index crosses the sample boundary
_add("conv3", "c3_8_32_big", 1, 8, 32, BIG, fwd=I2882, dgrad=I2881)
_add("conv3", "c3_8_32_big_n2", 2, 8, 32, BIG, fwd=I4882, dgrad=I4881)
_add("conv3", "c3_8_48_halfdead", 1, 8, 48, (21, 57, 113), fwd=I4882, dgrad=I2481)  # 384 tiles x 2 block pairs = 768: the smallest grid; the second pair half dead
# ---- split-K (forward): the factor conv3_f32_ksplit gives, and the same factor given
_add("splitk", "sk_32_32", 1, 32, 32, (4, 4, 16), ksplit=2, fwd=I2481)
_add("splitk", "sk_48_16", 1, 48, 16, (4, 4, 16), ksplit=2, fwd=I2481)            # three chunks per slice
_add("splitk", "sk_64_64", 1, 64, 64, (8, 8, 16), ksplit=4, fwd=I2481)
_add("splitk", "sk_128_128", 1, 128, 128, (4, 8, 16), ksplit=8, fwd=I2481)
_add("splitk", "sk_64_16_320", 1, 64, 16, (16, 32, 80), ksplit=2, fwd=I2481)       # 320 workgroups: blocks * 2 ks <= 1024 stops the factor at 2
_add("splitk", "sk_24_16_plain", 1, 24, 16, (4, 4, 16), ksplit=1, fwd=I2481)       # three chunks: factor 1, the plain launch
# ---- wgrad3_f32_kernel<TZ, TY, OT, CT>: w3 = (kernel, OT, CT, X16, DY16); nparts = partial gradients the reduction sums (2 nbx at OT = 1, nbx at OT = 2)
F11, F22 = ("f32", 1, 1, False, False), ("f32", 2, 2, False, False)
_add("wgrad3", "w3_16_16_walk", 2, 16, 16, (23, 40, 70), w3=F11, walk=True)        # 600 tiles on 512 workgroups across the sample boundary
_add("wgrad3", "w3_3_16_db", 2, 3, 16, (5, 9, 18), w3=F11, db=True)                # Cin % 4 != 0: the scalar reduction
_add("wgrad3", "w3_16_3_db", 2, 16, 3, (5, 9, 18), w3=F11, db=True)
_add("wgrad3", "w3_16_32", 1, 16, 32, (5, 9, 18), w3=F11)                          # two groups
_add("wgrad3", "w3_32_16", 1, 32, 16, (5, 9, 18), w3=F11)
_add("wgrad3", "w3_64_64_walk", 1, 64, 64, (8, 16, 144), w3=F22, walk=True)        # 144 tiles on 128 workgroups
_add("wgrad3", "w3_48_80", 1, 48, 80, (5, 9, 18), w3=F22)                          # half-dead block pairs on both sides
_add("wgrad3", "w3_red_126", 1, 16, 16, (13, 17, 33), w3=F11, nparts=126)          # 63 tiles: below nparts >= 128, 64 outputs per reduction workgroup
_add("wgrad3", "w3_red_128", 1, 16, 16, (15, 9, 49), w3=F11, nparts=128)           # 64 tiles: 16 outputs per workgroup, float4 items
_add("wgrad3", "w3_red_128_scalar", 1, 3, 16, (15, 9, 49), w3=F11, nparts=128)     # ... scalar items
_add("wgrad3", "w3_16_16_walk_bf16x3_w70", 2, 16, 16, (23, 40, 70), w3=F11, walk=True, precision="bf16x3")     # W % 4 != 0: the f32 kernel
# ---- wgrad3_sb_kernel<TZ, 4, OT, X16, DY16> on NCDHW tensors and on the two mixed layouts (ru_conv3d_bwd_weight_l)
for tag, xc, dc in (("", False, False), ("_x16", True, False), ("_dy16", False, True)):
    _add("wsb", "sb_16_16_walk" + tag, 2, 16, 16, (23, 40, 72), precision="bf16x3", x_c16=xc, dy_c16=dc, w3=("sb", 1, 1, xc, dc), walk=True)      # 600 on 512
    _add("wsb", "sb_32_32_walk" + tag, 1, 32, 32, (16, 32, 104), precision="bf16x3", x_c16=xc, dy_c16=dc, w3=("sb", 2, 1, xc, dc), walk=True)     # 448 on 384
_add("wsb", "sb_16_48", 1, 16, 48, (5, 8, 20), precision="bf16x3", w3=("sb", 2, 1, False, False))      # OT = 2 with an odd block count
_add("wsb", "sb_16_48_x16", 1, 16, 48, (5, 8, 20), precision="bf16x3", x_c16=True, w3=("sb", 2, 1, True, False))
# ---- k = 1: fwd / dgrad = the route of conv1_launch, w1 = wgrad1_f32_kernel<OT, CT>
_add("k1", "k1_32_16_mfma", 1, 32, 16, (4, 4, 4), fwd=MFMA, dgrad=K14, w1=(1, 2))
_add("k1", "k1_35_19_mfma_ragged", 1, 35, 19, (3, 5, 7), fwd=MFMA, dgrad=K14, w1=(2, 2))      # channel counts no multiple of 4 / 16, V no multiple of 64
_add("k1", "k1_32_48", 1, 32, 48, (3, 5, 7), fwd=MFMA, dgrad=MFMA, w1=(2, 2))
_add("k1", "k1_16_16_v63", 1, 16, 16, (3, 3, 7), fwd=K14, dgrad=K14, w1=(1, 1))            # V % 4 != 0
_add("k1", "k1_16_16_small", 1, 16, 16, (4, 4, 4), fwd=K14, dgrad=K14, w1=(1, 1))          # V % 4 == 0, fewer than 32 channels, a small grid
_add("k1", "k1_16_64_vec", 2, 16, 64, (31, 33, 32), fwd=K416, dgrad=MFMA, w1=(2, 1))       # 32 x 4 x 2 = 256 workgroups: the float4 route
_add("k1", "k1_64_16_vec", 2, 64, 16, (31, 33, 32), fwd=MFMA, dgrad=K416, w1=(1, 2))       # ... in the data gradient
_add("k1", "k1_16_64_v1more", 2, 16, 64, (1, 1, 32737), fwd=K14, dgrad=MFMA, w1=(2, 1))    # one voxel more: the vector route is lost
_add("k1", "k1_16_16_chunkwalk", 2, 16, 16, (1, 1, 66000), fwd=K14, dgrad=K14, w1=(1, 1), walk=True)      # 516 chunks on 512 workgroups
# ---- k = 2, stride 2: the pointwise launch sees Cin * 8 channels at the coarse grid
_add("k2", "k2_3_5", 2, 3, 5, (4, 6, 10), fwd=K14, dgrad=K14, w1=(1, 2))
_add("k2", "k2_4_16_mfma", 1, 4, 16, (4, 4, 8), fwd=MFMA, dgrad=K14, w1=(1, 2))
_add("k2", "k2_2_64_vec", 2, 2, 64, (62, 66, 64), fwd=K416, dgrad=MFMA, w1=(2, 1))          # 16 -> 64 at 31 x 33 x 32 coarse voxels
_add("k2", "k2_8_16_vec", 2, 8, 16, (62, 66, 64), fwd=MFMA, dgrad=K416, w1=(1, 2))          # the data gradient 16 -> 64 = 8 Cin
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def out_dhw(c):
    return tuple(v // 2 for v in c["dhw"]) if c["kind"] == "k2" else c["dhw"]


def ksize(c):
    return {"k1": 1, "k2": 2}.get(c["kind"], 3)


def _ints(seed, lo, hi, *shape):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, shape, generator=g).numpy().astype(np.float32)


def _normal(seed, *shape):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(*shape, generator=g).numpy()


def make_inputs(c):
    """float32 NCDHW operands of a case: x, w [Cout][Cin][k][k][k], b (or None), dy (the shape of the output); seeds derive from the case's name"""
    seed = 9000 + 10 * sorted(CASE_BY_NAME).index(c["name"])
    k = ksize(c)
    xs, ws, ys = (c["n"], c["cin"]) + c["dhw"], (c["cout"], c["cin"], k, k, k), (c["n"], c["cout"]) + out_dhw(c)
    if c["exact"]:
        x, dy = _ints(seed, -2, 2, *xs), _ints(seed + 1, -2, 2, *ys)
        w, b = _ints(seed + 2, -2, 2, *ws) * 0.5, _ints(seed + 3, -2, 2, c["cout"]) * 0.5
    else:
        x, dy = _normal(seed, *xs), _normal(seed + 1, *ys)
        w, b = _normal(seed + 2, *ws) * (k ** 3 * c["cin"]) ** -0.5, _normal(seed + 3, c["cout"])
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f(x), w=f(w), b=f(b) if c["bias"] else None, dy=f(dy))


def reference(c, i):
    """float64 results of a case: the tensors the device test stores and compares"""
    kind = c["kind"]
    if kind == "conv3":
        return dict(y=ref_conv3(i["x"], i["w"], i["b"]), dx=ref_dgrad3(i["dy"], i["w"]))
    if kind == "splitk":
        return dict(y=ref_splitk(i["x"], i["w"], c["ksplit"]))
    if kind in ("wgrad3", "wsb"):
        r = dict(dw=ref_wgrad3(i["x"], i["dy"]))
        if c.get("db"):
            r["db"] = ref_db(i["dy"])
        return r
    if kind == "k1":
        return dict(y=ref_conv1(i["x"], i["w"]), dx=ref_dgrad1(i["dy"], i["w"]), dw=ref_wgrad1(i["x"], i["dy"]).reshape(i["w"].shape))
    assert kind == "k2"
    return dict(y=ref_conv2(i["x"], i["w"]), dx=ref_dgrad2(i["dy"], i["w"]), dw=ref_wgrad2(i["x"], i["dy"]))


def pointwise_shape(c):
    """(Cin, Cout, V) as the pointwise launch behind k = 1 / k = 2 sees them"""
    v = int(np.prod(out_dhw(c)))
    return (c["cin"] * 8 if c["kind"] == "k2" else c["cin"]), c["cout"], v


def chosen(c, ops):
    """what the library says it launches for a case (host-only queries): the dict of the case's own inst keys"""
    n, cin, cout, (d, h, w) = c["n"], c["cin"], c["cout"], c["dhw"]
    got = {}
    if c["kind"] in ("conv3", "splitk"):
        f = ops.ncdhw_conv3_inst(n, cin, cout, d, h, w)
        got["fwd"] = tuple(f[:4])
        if c["kind"] == "conv3":
            got["dgrad"] = tuple(ops.ncdhw_conv3_inst(n, cout, cin, d, h, w)[:4])
        else:
            got["ksplit"] = f.ksplit
    elif c["kind"] in ("wgrad3", "wsb"):
        i = ops.ncdhw_wgrad3_inst(n, cin, cout, d, h, w, precision=c["precision"], x_c16=c["x_c16"], dy_c16=c["dy_c16"])
        got["w3"], got["walk"] = tuple(i[:5]), i.ntile > i.nbx
        if "nparts" in c:
            got["nparts"] = i.nbx * (1 if i.ot == 2 else 2)
    else:
        pc, po, v = pointwise_shape(c)
        i = ops.ncdhw_wgrad1_inst(n, pc, po, v)
        got["fwd"], got["dgrad"] = ops.ncdhw_conv1_route(n, pc, po, v), ops.ncdhw_conv1_route(n, po, pc, v)
        got["w1"], got["walk"] = (i.ot, i.ct), n * i.nchunk > i.nbx
    return got


def written_for(c):
    return {k: c[k] for k in ("fwd", "dgrad", "w3", "w1", "nparts") if k in c} | ({"walk": c["walk"]} if c["kind"] not in ("conv3", "splitk") else {}) | (
        {"ksplit": c["ksplit"]} if c["kind"] == "splitk" else {})


# ---------------------------------------------------------------------------------------------------------------- proofs
def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).requires_grad_(grad)


def _close(got, ref):
    got, ref = _pair(got, ref)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()


def _small(seed, *shape):
    return _normal(seed, *shape).astype(np.float64)


def test_k3_restatements_are_the_reference_convolution():
    for seed, (n, ci, co, sp) in enumerate(((2, 3, 5, (4, 5, 6)), (1, 8, 4, (3, 2, 7)), (1, 1, 1, (1, 1, 1)))):
        x, w, b, dy = _small(seed, n, ci, *sp), _small(seed + 50, co, ci, 3, 3, 3), _small(seed + 60, co), _small(seed + 70, n, co, *sp)
        tx, tw, tb = _t(x, True), _t(w, True), _t(b, True)
        y = O.conv3x3x3(tx, tw, tb)
        (y * _t(dy)).sum().backward()
        _close(ref_conv3(x, w, b), y.detach().numpy())
        _close(ref_conv3(x, w), O.conv3x3x3(_t(x), _t(w)).numpy())
        _close(ref_dgrad3(dy, w), tx.grad.numpy())
        _close(ref_wgrad3(x, dy), tw.grad.numpy())
        _close(ref_db(dy), tb.grad.numpy())


def test_split_k_restatement_is_the_whole_convolution_in_float64():
    x, w = _small(1, 1, 48, 3, 4, 5), _small(2, 7, 48, 3, 3, 3)
    for ks in (1, 2, 3, 6):
        _close(ref_splitk(x, w, ks), O.conv3x3x3(_t(x), _t(w)).numpy())
    assert splitk_slices(48, 2) == [(0, 24), (24, 48)] and splitk_slices(20, 3) == [(0, 8), (8, 16), (16, 20)]
    with pytest.raises(AssertionError):
        splitk_slices(48, 4)


def test_k1_and_k2_restatements_are_the_reference_convolutions():
    for seed, (n, ci, co, sp) in enumerate(((2, 3, 5, (4, 2, 6)), (1, 8, 4, (2, 2, 2)))):
        for k, conv in ((1, O.conv1x1x1), (2, O.conv2x2x2_s2)):
            so = tuple(v // k for v in sp)
            x, w, dy = _small(seed, n, ci, *sp), _small(seed + 50, co, ci, k, k, k), _small(seed + 70, n, co, *so)
            tx, tw = _t(x, True), _t(w, True)
            y = conv(tx, tw)
            (y * _t(dy)).sum().backward()
            f, g, h = (ref_conv1, ref_dgrad1, lambda a, b: ref_wgrad1(a, b).reshape(w.shape)) if k == 1 else (ref_conv2, ref_dgrad2, ref_wgrad2)
            _close(f(x, w), y.detach().numpy())
            _close(g(dy, w), tx.grad.numpy())
            _close(h(x, dy), tw.grad.numpy())
    x = _small(9, 2, 3, 4, 6, 2)
    assert np.array_equal(d2s(s2d(x), 3), x)
    assert s2d(x)[1, 2 * 8 + 5, 1, 2, 0] == x[1, 2, 2 * 1 + 1, 2 * 2 + 0, 2 * 0 + 1]          # channel c*8 + (i*4 + j*2 + k)


def _is_bf16(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return bool(((b & 0xffff) == 0).all())


@pytest.mark.parametrize("c", [c for c in CASES if c["exact"]], ids=[c["name"] for c in CASES if c["exact"]])
def test_exact_family_is_exact(c):
    """every operand a multiple of the unit and a bf16 value; (products per output) * max |a| * max |b| (+ max |bias|), which bounds the sum of |product| of every
    output element and so every partial sum in any order, below 2^24 units"""
    i = make_inputs(c)
    k3, nvox = ksize(c) ** 3, c["n"] * int(np.prod(out_dhw(c)))
    amax = lambda a: float(np.abs(a).max())
    for a in i.values():
        if a is not None:
            assert _is_bf16(a) and np.array_equal(a * 2, np.rint(a * 2))
    assert np.array_equal(i["x"], np.rint(i["x"])) and np.array_equal(i["dy"], np.rint(i["dy"]))
    half = 0.5
    bounds = {}
    if c["kind"] in ("conv3", "splitk", "k1", "k2"):
        bounds["y"] = (k3 * c["cin"] * amax(i["x"]) * amax(i["w"]) + (amax(i["b"]) if c["bias"] else 0.0)) / half
    if c["kind"] in ("conv3", "k1", "k2"):
        bounds["dx"] = k3 * c["cout"] * amax(i["dy"]) * amax(i["w"]) / half          # (k = 2: one tap per fine voxel; k^3 over-counts)
    if c["kind"] in ("wgrad3", "wsb", "k1", "k2"):
        bounds["dw"] = nvox * amax(i["x"]) * amax(i["dy"])
    if c.get("db"):
        bounds["db"] = nvox * amax(i["dy"])
    assert bounds and max(bounds.values()) < 2.0 ** 24, bounds


@pytest.fixture(scope="module")
def ops():
    from brats2019_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from brats2019_amd import build
        build.build(verbose=False)
    from brats2019_amd import ops as m
    return m


def test_every_case_reaches_what_it_was_written_for(ops):
    """the host-only queries (the functions the launchers switch on) against every case's own record; the device test asserts the same again beside its launches"""
    bad = [(c["name"], written_for(c), chosen(c, ops)) for c in CASES if chosen(c, ops) != written_for(c)]
    assert not bad, bad


def test_the_cases_cover_every_switch(ops):
    seen = {c["fwd"] for c in CASES if c["kind"] == "conv3"} | {c["dgrad"] for c in CASES if c["kind"] == "conv3"}
    assert seen == set(CONV3_INSTS)
    assert {c["ksplit"] for c in CASES if c["kind"] == "splitk"} == {1, 2, 4, 8}
    assert {c["w3"] for c in CASES if c["kind"] == "wgrad3"} == {F11, F22}
    # every wgrad3_sb_kernel instantiation wgrad3_launch can reach: both voxel-major goes to the transpose-read kernel, so <., true, true> has no caller
    assert {c["w3"] for c in CASES if c["kind"] == "wsb"} == {("sb", ot, 1, x, d) for ot in (1, 2) for x, d in ((False, False), (True, False), (False, True))}
    assert ops.ncdhw_wgrad3_inst(2, 16, 16, 23, 40, 72, precision="bf16x3", x_c16=True, dy_c16=True).kernel == "tr"
    pw = [c for c in CASES if c["kind"] in ("k1", "k2")]
    assert {c["fwd"] for c in pw} == {c["dgrad"] for c in pw} == {MFMA, K14, K416}
    assert {c["w1"] for c in pw if c["kind"] == "k1"} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    for kind in ("wgrad3", "wsb", "k1"):
        assert any(c["walk"] for c in CASES if c["kind"] == kind), kind
    nparts = {c["nparts"] for c in CASES if "nparts" in c}
    assert min(nparts) < 128 <= max(nparts)
    assert {c["cin"] % 4 == 0 for c in CASES if c["kind"] == "wgrad3"} == {True, False}            # both sides of the reduction's float4 condition


def _both(name):
    out = []
    for fam in ("exact", "real"):
        c = CASE_BY_NAME["%s_%s" % (name, fam)]
        out.append((c, make_inputs(c)))
    return out


def test_every_bar_can_fail():
    """each mutant of the reference breaks exact equality on the exact family and exceeds the bar of the real family"""
    def check(what, good, mutant, excess, assert_real=True):
        for (c, _), g, m in zip(pairs, good, mutant):
            if c["exact"]:
                assert exact_excess(m, g) == float("inf"), (what, c["name"])
            else:
                e = excess(m, g)
                print("  %-34s %-22s mutant error / bar %.3g" % (what, c["name"], e))
                assert e > 1.0 or not assert_real, (what, c["name"], e)
    # one tap of the stencil's border (tap 26 = (+1, +1, +1)); un-mirrored data-gradient taps
    pairs = _both("c3_8_16")
    check("forward without tap 26", [ref_conv3(i["x"], i["w"]) for _, i in pairs], [ref_conv3(i["x"], i["w"], drop_tap=26) for _, i in pairs], tensor_excess)
    check("data gradient, taps not mirrored", [ref_dgrad3(i["dy"], i["w"]) for _, i in pairs], [ref_dgrad3(i["dy"], i["w"], mirror=False) for _, i in pairs], tensor_excess)
    # one tile of a walk: one of 24, and one of 600 -- the last of the second round (tile 599: sample 1, the last (2, 8, 16) tile), recorded, not asserted
    pairs = _both("w3_3_16_db")
    check("weight gradient, 1 tile of 24", [ref_wgrad3(i["x"], i["dy"]) for _, i in pairs], [ref_wgrad3(i["x"], i["dy"], (1, 4, 8, 16, 2, 8)) for _, i in pairs],
          reduction_excess)
    pairs = _both("w3_16_16_walk")
    check("weight gradient, 1 tile of 600", [ref_wgrad3(i["x"], i["dy"]) for _, i in pairs], [ref_wgrad3(i["x"], i["dy"], (1, 22, 32, 64, 2, 8)) for _, i in pairs],
          reduction_excess, assert_real=False)
    pairs = _both("sb_16_48")
    check("split-bf16 dw, 1 tile of 12", [ref_wgrad3(i["x"], i["dy"]) for _, i in pairs], [ref_wgrad3(i["x"], i["dy"], (0, 4, 4, 16, 2, 4)) for _, i in pairs], sb_excess)
    # one split-K slice
    pairs = _both("sk_64_64")
    check("split-K without slice 2", [ref_splitk(i["x"], i["w"], 4) for _, i in pairs], [ref_splitk(i["x"], i["w"], 4, drop_slice=2) for _, i in pairs], tensor_excess)
    # the halves of an OT = 2 pair
    pairs = _both("w3_48_80")
    good = [ref_wgrad3(i["x"], i["dy"]) for _, i in pairs]
    check("OT = 2 halves exchanged", good, [swap_ot_halves(g) for g in good], reduction_excess)
    # and the bars pass what they should: the float32 rounding of the reference
    for c, i in _both("c3_8_16"):
        r = reference(c, i)
        assert tensor_excess(r["y"].astype(np.float32), r["y"]) <= 1.0 and exact_excess(r["y"], r["y"]) == 0.0
