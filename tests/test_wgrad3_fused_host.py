"""The float64 restatements that tests/test_wgrad3_fused.py holds every instantiation of the transpose-read 3x3x3 weight gradient to (wgrad3_tz_kernel<OT, XS, DS, NP>
of csrc/wgrad_tr.hip, driven one launch at a time through ru_wgrad3_l / ops.wgrad3_fused), that file's cases, inputs and bars, and the proof -- on the CPU alone --
that (a) the restatements are the reference's operations, (b) the exact family is exact, (c) the encoders of the two published forms meet the bars derived from
the formats, (d) every bar can fail.

Restatements (float64, NCDHW):
  weight gradient   dw[o][c][tap] = sum_{n,v} dy[n][o][v] * pad0(act(x))[n][c][v + tap], act(x) = max(u, slope*u), u = x*scale[n][c] + shift[n][c]: the zero border
                    is put around the ACTIVATED tensor; proven against torch.nn.grad.conv3d_weight and autograd in float64
  fused apply       dy = cA * ((y*scale + shift) > 0 ? d : d*slope) + (cB*y + cC) per (n, channel): gn_bwd_apply16_launch's expression, proven to be the input gradient
                    of GroupNorm -> LeakyReLU given the finalize coefficients
  swapped form      T[t][o'][c'] = sum_v dy'[v][o'] x'[v + t][c'] stored as dW[c'][o'][26 - t]: proven to be conv3d_weight(input = dy', grad_output = x')
  truncation        dw[:dw_cout, :dw_cin] of the padded blocks
Published forms (csrc/ru_common.h; 64 bytes per voxel and 16-channel block), numpy encoders and decoders written from the format:
  split form        uint16[32]: bf16 RNE hi of channels 0-15, then bf16 RNE of the exact residual v - hi of channels 0-15
  gradient operand  the same 16 hi, then per channel half 8 bytes e4m3(lo / 2^(e-8)) and 8 bytes e4m3(v / 2^e), saturating; 2^e = 2^(E - 7), E the exponent of the
                    largest |hi| of the voxel's 16 channels (biased exponent byte E + 120, floor 9)
Bars (error / bar <= 1 passes).  dw: three products 2e-5 * max |ref| per element (tests/test_hip_c16.py), one product relative L2 2^-8 (class p1 of
tests/test_conv3_fused_host.py).  Published tensor, per element, with F = the float32 roundings of the apply expression (2^-24 of |cA| |d*slope|, |cA*dh|, |cB*y|,
|cB*y + cC| and |dy|) and A = the voxel's largest |dy| * (1 + 2^-7):
  split form        2^-16 (|dy| + F) + F                       (RNE to 8 significant bits, half an ulp <= 2^-8 |value|, twice: the residual's residual)
  gradient operand  hi + lo code: 2^-12 (|dy| + F) + 2^-25 A + F   (4 significant bits, half an ulp <= 2^-4, of a residual <= 2^-8 |dy|; subnormal codes step 2^-9
                                                                   at scale 2^(E-15), half a step <= 2^-25 A)
                    value code:   2^-4 (|dy| + F) + 2^-17 A + F    (4 significant bits; subnormal codes step 2^-9 at scale 2^(E-7))
test_encoders_meet_the_format_bars shows the numpy encoders applied to the float32-rounded reference inside these bars, with F = 0 and with F (the test prints the
error / bar it measures: 0.50 split form, 0.94 gradient-operand form on these inputs).

Two input families per case.  exact: small integers and powers of two (scale, shift in {-2, 2}, apply coefficients powers of two, slope 0.5), optionally one operand
with a 2^-8 fraction so that lo packets are not empty; test_exact_family_is_exact proves every operand, every intermediate of the apply, and the sum of |product| of
every dw element an integer multiple of the case's unit (2^-8 with fractions, else 1) below 2^23 units, the lo x lo product (which the kernels drop) zero, and hi + lo equal to the value: float32 arithmetic
in any order gives the reference exactly.  real: seeded normal values, scale with a negative and a zero channel, a large shift, |y*scale + shift| >= 1e-3.
Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_pointwise_c16_host import draw

U24 = 2.0 ** -24
EXACT_SLOPE, REAL_SLOPE = 0.5, 0.01
FINE = 2.0 ** -8


# ---------------------------------------------------------------------------------------------------------------- restatements
def lrelu(u, slope):
    return np.maximum(u, slope * u) if slope <= 1 else np.where(u > 0, u, u * slope)


def pad0(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))


def staged(x, scale=None, shift=None, slope=1.0, transform_padding=False):
    """what the weight gradient reads of x, border included.  Mutant transform_padding: the border is transformed like a voxel of value 0."""
    if scale is None:
        return pad0(x)
    sc, sh = scale[:, :, None, None, None], shift[:, :, None, None, None]
    if transform_padding:
        return lrelu(pad0(x) * sc + sh, slope)
    return pad0(lrelu(x * sc + sh, slope))


def wgrad_padded(xp, dy):
    """dw[o,c,i,j,k] = sum_{n,z,y,x} dy[n,o,z,y,x] xp[n,c,z+i,y+j,x+k]: 27 explicit taps"""
    n, co = dy.shape[:2]
    ci = xp.shape[1]
    d, h, w = dy.shape[2:]
    g = dy.reshape(n, co, -1)
    dw = np.zeros((co, ci, 3, 3, 3))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                xs = xp[:, :, i:i + d, j:j + h, k:k + w].reshape(n, ci, -1)
                dw[:, :, i, j, k] = np.einsum("nov,ncv->oc", g, xs, optimize=True)
    return dw


def swapped_form(t, mirror=True):
    """T[o'][c'][taps] -> dW[c'][o'][mirrored taps].  Mutant mirror = False."""
    t = t.transpose(1, 0, 2, 3, 4)
    return np.ascontiguousarray(t[:, :, ::-1, ::-1, ::-1] if mirror else t)


def ref_apply(y, d, scale, shift, coef, slope, ge=False):
    """-> (dy, float32-rounding term F of the device's expression, min |y*scale + shift|).  Mutant ge: `>=` at the threshold."""
    b = lambda a: a[:, :, None, None, None]
    u = y * b(scale) + b(shift)
    dh = np.where((u >= 0) if ge else (u > 0), d, d * slope)
    ca, cb, cc = b(coef[:, :, 0]), b(coef[:, :, 1]), b(coef[:, :, 2])
    lin = cb * y + cc
    dy = ca * dh + lin
    f = U24 * (np.abs(ca * d * slope) + np.abs(ca * dh) + np.abs(cb * y) + np.abs(lin) + np.abs(dy)) * (1 + 1e-6)
    return dy, f, float(np.abs(u).min())


# ---------------------------------------------------------------------------------------------------------------- the published forms
def bf16_bits(a):
    """float32 -> bf16 bit patterns, round to nearest even (finite values)"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def e4m3_encode(v):
    """float64 -> OCP e4m3 codes (bias 7, 3 mantissa bits, subnormals step 2^-9, largest value 448, no infinity), round to nearest even, saturating"""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    ex = np.maximum(np.frexp(a)[1] - 1, -6)
    q = np.ldexp(1.0, ex - 3)
    r = np.minimum(np.rint(a / q) * q, 448.0)
    ex = np.maximum(np.frexp(r)[1] - 1, -6)
    sub = r < 2.0 ** -6
    mant = np.where(sub, r * 2.0 ** 9, (r / np.ldexp(1.0, ex) - 1.0) * 8)
    code = np.where(sub, 0, ex + 7).astype(np.int64) * 8 + mant.astype(np.int64)
    return (code | (np.signbit(v).astype(np.int64) << 7)).astype(np.uint8)


def e4m3_decode(code):
    code = np.asarray(code, np.uint8).astype(np.int64)
    e, m = (code >> 3) & 15, code & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * np.ldexp(1.0, e - 7))
    return np.where(code & 128, -mag, mag)


def split_encode(v32):
    """[..., 16] float32 -> uint8 [..., 64] split form"""
    v32 = np.ascontiguousarray(v32, np.float32)
    hi = bf16_bits(v32)
    lo = bf16_bits((v32.astype(np.float64) - bf16_value(hi)).astype(np.float32))            # the residual is exact in float32
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=-1)).view(np.uint8)


def split_decode(b, zero_lo=False):
    """-> hi + lo in float64.  Mutant zero_lo: the lo packets read as zero."""
    u = np.ascontiguousarray(b, np.uint8).view(np.uint16)
    return bf16_value(u[..., :16]) + (0.0 if zero_lo else bf16_value(u[..., 16:]))


def g16_exponent(hi_value, per_half=False):
    """the scale exponent e of a voxel from its 16 hi values [..., 16] -> [..., 16] (broadcast).  Mutant per_half: each channel half takes its own."""
    a = np.abs(hi_value).astype(np.float32)
    amax = np.repeat(a.reshape(a.shape[:-1] + (2, 8)).max(-1), 8, axis=-1) if per_half else np.broadcast_to(a.max(-1, keepdims=True), a.shape)
    byte = np.maximum(((np.ascontiguousarray(amax).view(np.uint32) >> 23) & 0xff).astype(np.int64) - 7, 9)      # mxg_exponent_byte
    return byte - 127


def g16_encode(v32, per_half=False):
    """[..., 16] float32 -> uint8 [..., 64] gradient-operand form"""
    v32 = np.ascontiguousarray(v32, np.float32)
    hi = bf16_bits(v32)
    v = v32.astype(np.float64)
    lo = v - bf16_value(hi)
    e = g16_exponent(bf16_value(hi), per_half)
    l8, x8 = e4m3_encode(lo / np.ldexp(1.0, e - 8)), e4m3_encode(v / np.ldexp(1.0, e))
    return np.concatenate([np.ascontiguousarray(hi).view(np.uint8), l8[..., :8], x8[..., :8], l8[..., 8:], x8[..., 8:]], axis=-1)


def g16_decode(b, zero_lo=False):
    """-> (hi + lo code * 2^(e-8), value code * 2^e), e from the stored hi values of the whole voxel"""
    b = np.ascontiguousarray(b, np.uint8)
    hi = bf16_value(np.ascontiguousarray(b[..., :32]).view(np.uint16))
    e = g16_exponent(hi)
    l8 = np.concatenate([b[..., 32:40], b[..., 48:56]], axis=-1)
    x8 = np.concatenate([b[..., 40:48], b[..., 56:64]], axis=-1)
    return hi + (0.0 if zero_lo else e4m3_decode(l8) * np.ldexp(1.0, e - 8)), e4m3_decode(x8) * np.ldexp(1.0, e)


def canon(b, g16):
    """bytes of a published tensor with the sign of a zero e4m3 code cleared (a zero carries no sign the reader could use)"""
    b = np.array(b, np.uint8)
    if g16:
        codes = b[..., 32:]
        codes[codes == 0x80] = 0
    return b


def blocks(t):
    """NCDHW [N, C, D, H, W] -> voxel-major [N, C/16, D, H, W, 16]"""
    n, c = t.shape[:2]
    return np.ascontiguousarray(t.reshape((n, c // 16, 16) + t.shape[2:]).transpose(0, 1, 3, 4, 5, 2))


# ---------------------------------------------------------------------------------------------------------------- bars
def dw_excess(got, ref, products):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    if products == 1:
        return float(np.sqrt(((got - ref) ** 2).sum()) / (2.0 ** -8 * np.sqrt((ref ** 2).sum())))
    return float(np.abs(got - ref).max() / (2e-5 * np.abs(ref).max()))


def exact_excess(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return 0.0 if np.array_equal(got, ref) else float("inf")


def pub_bars(ref, f):
    """(split, residual-code, value-code) bars of a published tensor from the float64 reference and its rounding term F (both voxel-major [N, C/16, D, H, W, 16])"""
    v = np.abs(ref)
    a = v.max(-1, keepdims=True) * (1 + 2.0 ** -7)
    return 2.0 ** -16 * (v + f) + f, 2.0 ** -12 * (v + f) + 2.0 ** -25 * a + f, 2.0 ** -4 * (v + f) + 2.0 ** -17 * a + f


def pub_excess(b, ref, f, g16, **mutant):
    """worst error / bar of the published bytes b [N, C/16, D, H, W, 64] against the float64 reference (voxel-major, as its rounding term f)"""
    bs, bl, bx = pub_bars(ref, f)
    if not g16:
        dec = split_decode(b, **mutant)
        return float("inf") if np.isnan(dec).any() else float((np.abs(dec - ref) / bs).max())
    dl, dx = g16_decode(b, **mutant)
    if np.isnan(dl).any() or np.isnan(dx).any():
        return float("inf")
    return max(float((np.abs(dl - ref) / bl).max()), float((np.abs(dx - ref) / bx).max()))


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases and inputs
RAG, ONE, BIG3, BIG7 = (2, (5, 11, 19)), (1, (2, 8, 16)), (3, (3, 88, 128)), (1, (7, 88, 384))
M32, M64A, M64B, M128 = (2, (3, 70, 120)), (2, (3, 24, 96)), (2, (7, 24, 96)), (2, (5, 24, 48))


def case(name, shape, cin, cout, inst, exact, **kw):
    c = dict(name=name + ("_exact" if exact else "_real"), n=shape[0], dhw=shape[1], cin=cin, cout=cout, inst=inst, exact=exact, transform=False, dy_split=False, x_c4=False,
             dy_c4=False, swapped=False, products=0, gb=None, dw_cin=0, dw_cout=0, deferred=False)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


CASES = []
for ex in (True, False):
    both = lambda *a, **k: CASES.append(case(*a, exact=ex, **k))
    only_exact = lambda *a, **k: ex and CASES.append(case(*a, exact=True, **k))
    # plain and transformed gradient over the channel pairs: OT = 1 / 2, mixed, odd block counts on either side (32 -> 48, 16 -> 48, 32 -> 80: the last block had no
    # workgroup before wtr_choose learnt to count), one item, ragged on every axis across a sample boundary
    both("one_item_16", ONE, 16, 16, (1, 0, 0, 3))
    both("rag_16_16_scale", RAG, 16, 16, (1, 0, 0, 3), transform=True)
    both("rag_32_32", RAG, 32, 32, (2, 0, 0, 3))
    both("cols_128_128_scale", M128, 128, 128, (2, 0, 0, 3), transform=True)
    both("rag_32_16_scale", RAG, 32, 16, (1, 0, 0, 3), transform=True)
    both("rag_16_32", RAG, 16, 32, (2, 0, 0, 3))
    both("rag_48_32_scale", RAG, 48, 32, (2, 0, 0, 3), transform=True)
    both("rag_32_48_scale", RAG, 32, 48, (1, 0, 0, 3), transform=True)
    both("rag_80_16", RAG, 80, 16, (1, 0, 0, 3))
    both("rag_16_48", RAG, 16, 48, (1, 0, 0, 3))
    both("rag_32_80_scale", RAG, 32, 80, (1, 0, 0, 3), transform=True)
    both("rag_16_16_truncated", RAG, 16, 16, (1, 0, 0, 3), dw_cin=5, dw_cout=7)
    # workgroups that walk more than one column of the ring: 264 columns on 256 workgroups at D = 3 and D = 7 (column strides 6 and 10), 144 on 128, 36 on 32
    both("cols_16_d3_scale", BIG3, 16, 16, (1, 0, 0, 3), transform=True)
    both("cols_16_d7", BIG7, 16, 16, (1, 0, 0, 3))
    both("cols_64_d3_scale", M64A, 64, 64, (2, 0, 0, 3), transform=True)
    both("cols_64_d7", M64B, 64, 64, (2, 0, 0, 3))
    # split-form dy (three products; one product exists for two output blocks only)
    for tag, sh16, sh32 in (("rag", RAG, RAG), ("cols", BIG3, M32)):
        both(tag + "_split_16_scale", sh16, 16, 16, (1, 0, 1, 3), dy_split=True, transform=True)
        both(tag + "_split_32_scale", sh32, 32, 32, (2, 0, 1, 3), dy_split=True, transform=True)
        both(tag + "_split_32_p1_scale", sh32, 32, 32, (2, 0, 1, 1), dy_split=True, transform=True, products=1)
        # a 4-channel dy (the head's gradient, unswapped), three products and one
        both(tag + "_dyc4_scale", sh16, 16, 16, (1, 0, 2, 3), dy_c4=True, dw_cout=3, transform=True)
        both(tag + "_dyc4_p1", sh16, 16, 16, (1, 0, 2, 1), dy_c4=True, dw_cout=3, products=1)
        # the packed-tap form of a 4-channel x: the stem with 4 real channels and with fewer, with split-form dy, one product, and the swapped head with 3
        both(tag + "_xc4", sh16, 16, 16, (1, 2, 0, 3), x_c4=True, dw_cin=4)
        both(tag + "_xc4_split", sh16, 16, 16, (1, 2, 1, 3), x_c4=True, dw_cin=4, dy_split=True)
        both(tag + "_xc4_p1", sh16, 16, 16, (1, 2, 0, 1), x_c4=True, dw_cin=4, products=1)
        both(tag + "_head_swapped", sh16, 16, 16, (1, 2, 0, 3), x_c4=True, dw_cin=3, swapped=True)
        # the fused GroupNorm-backward apply: published in the split form, in the gradient-operand form, not at all (stem); one product; two output blocks
        both(tag + "_gb_split_scale", sh16, 16, 16, (1, 0, 3, 3), gb="split", transform=True)
        both(tag + "_gb_g16_scale", sh16, 16, 16, (1, 0, 4, 3), gb="g16", transform=True)
        both(tag + "_gb_p1_scale", sh16, 16, 16, (1, 0, 3, 1), gb="split", transform=True, products=1)
        both(tag + "_gb_32_scale", sh32, 32, 32, (2, 0, 3, 3), gb="split", transform=True)
        both(tag + "_gb_stem", sh16, 16, 16, (1, 2, 3, 3), gb="none", x_c4=True, dw_cin=4)
        both(tag + "_gb_stem_p1", sh16, 16, 16, (1, 2, 3, 1), gb="none", x_c4=True, dw_cin=4, products=1)
    both("rag_xc4_c2", RAG, 16, 16, (1, 2, 0, 3), x_c4=True, dw_cin=2)
    # deferred-reduction twins (the batch kernel)
    only_exact("rag_32_48_deferred", RAG, 32, 48, (1, 0, 0, 3), transform=True, deferred=True)
    only_exact("cols_16_d3_deferred", BIG3, 16, 16, (1, 0, 0, 3), transform=True, deferred=True)
    only_exact("rag_head_swapped_deferred", RAG, 16, 16, (1, 2, 0, 3), x_c4=True, dw_cin=3, swapped=True, deferred=True)
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
TWINS = {"rag_32_48_deferred_exact": "rag_32_48_scale_exact", "cols_16_d3_deferred_exact": "cols_16_d3_scale_exact", "rag_head_swapped_deferred_exact": "rag_head_swapped_exact"}


def case_slope(c):
    return EXACT_SLOPE if c["exact"] else REAL_SLOPE


def _ints(seed, lo, hi, *shape):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, shape, generator=g).numpy().astype(np.float32)


def _pick(seed, values, *shape):
    return np.asarray(values, np.float32)[_ints(seed, 0, len(values) - 1, *shape).astype(np.int64)]


def fine_operand(c):
    """which operand of an exact case carries 2^-8 fractions (non-empty lo packets): none with one product (operands must be bf16 values) or above 5000 voxels
    (the sums must stay below 2^23 units); else dy where it is formed by the apply or x is untransformed, x otherwise"""
    vox = c["n"] * int(np.prod(c["dhw"]))
    if not c["exact"] or c["products"] == 1 or vox > 5000:
        return None
    return "dy" if (c["gb"] or not c["transform"]) else "x"


def trained_like(seed, n, ch):
    """(scale, shift) [N, C] float32: scales of both signs away from zero, channel 0 negative, channel 1 zero, shifts away from zero, channel 2 large"""
    s, h = draw(seed, n, ch), draw(seed + 1, n, ch) * 0.5
    scale = (np.where(s < 0, -1.0, 1.0) * (0.5 + np.abs(s))).astype(np.float32)
    scale[:, 0] = -np.abs(scale[:, 0])
    shift = np.where(np.abs(h) < 0.1, np.where(h < 0, -0.1, 0.1), h).astype(np.float32)
    if ch > 2:
        scale[:, 1] = 0.0
        shift[:, 2] = 6.0
    return scale, shift


def make_inputs(c):
    """float32 NCDHW numpy operands of a case (x, dy with their REAL channel counts for the 4-channel sides); seeds derive from the case's name"""
    seed = 5000 + 40 * sorted(CASE_BY_NAME).index(TWINS.get(c["name"], c["name"]))
    n, sp = c["n"], c["dhw"]
    cx = c["dw_cin"] if c["x_c4"] else c["cin"]
    cy = c["dw_cout"] if c["dy_c4"] else c["cout"]
    fine = fine_operand(c)
    i = {}
    if c["exact"]:
        i["x"] = _ints(seed, -1, 1, n, cx, *sp) + (_ints(seed + 1, -1, 1, n, cx, *sp) * FINE if fine == "x" else 0)
        if c["transform"]:
            i["scale"], i["shift"] = _pick(seed + 2, [-2, 2], n, c["cin"]), _pick(seed + 3, [-2, 2], n, c["cin"])
            i["scale"][:, 0] = -2.0
        if c["gb"]:
            i["gb_y"], i["gb_d"] = _ints(seed + 4, -3, 3, n, cy, *sp), 2 * _ints(seed + 5, -2, 2, n, cy, *sp)
            i["gb_scale"], i["gb_shift"] = _pick(seed + 6, [-2, -1, 1, 2], n, cy), _ints(seed + 7, -2, 2, n, cy)
            i["gb_scale"][:, 0] = -1.0
            cb = _pick(seed + 9, [-FINE, FINE, 1, -1] if fine == "dy" else [-1, 1], n, cy)
            i["gb_coef"] = np.stack([_pick(seed + 8, [-2, -1, 1, 2], n, cy), cb, _ints(seed + 10, -2, 2, n, cy)], axis=2)
        else:
            i["dy"] = _ints(seed + 4, -2, 2, n, cy, *sp) + (_ints(seed + 5, -1, 1, n, cy, *sp) * FINE if fine == "dy" else 0)
    else:
        i["x"] = draw(seed, n, cx, *sp)
        if c["transform"]:
            i["scale"], i["shift"] = trained_like(seed + 2, n, c["cin"])
        if c["gb"]:
            y, i["gb_d"] = draw(seed + 4, n, cy, *sp), draw(seed + 5, n, cy, *sp)
            i["gb_scale"], i["gb_shift"] = trained_like(seed + 6, n, cy)
            sc, sh = (a.astype(np.float64)[:, :, None, None, None] for a in (i["gb_scale"], i["gb_shift"]))
            u = y * sc + sh
            push = np.where(u >= 0, 1.0, -1.0) * 4e-3 / np.where(sc == 0, 1.0, sc)
            i["gb_y"] = np.where((np.abs(u) < 2e-3) & (sc != 0), y + push, y).astype(np.float32)
            i["gb_coef"] = (draw(seed + 8, n, cy, 3) * np.asarray([1.0, 0.3, 0.3], np.float32)).astype(np.float32)
        else:
            i["dy"] = draw(seed + 4, n, cy, *sp)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in i.items()}


def split_value(t):
    """what the split form holds of a float32 NCDHW tensor, in float64 (per element: the channel grouping does not matter)"""
    hi = bf16_value(bf16_bits(t))
    return hi + bf16_value(bf16_bits((np.asarray(t, np.float64) - hi).astype(np.float32)))


def reference(c, i, transform_padding=False, ge=False, mirror=True, drop_last_plane=False, ring_reuse=False, lose_lo=False, lose_last_block=False):
    """float64 reference of a case -> dict(dw, dy, f): dw as the launch returns it (swapped / truncated), dy / f the applied gradient and its rounding term (fused
    apply only).  The keyword arguments are the mutants of test_mutants_exceed_every_bar."""
    f8 = lambda a: None if a is None else np.asarray(a, np.float64)
    x = f8(i["x"])
    dy = f = None
    if c["gb"]:
        dy, f, margin = ref_apply(f8(i["gb_y"]), f8(i["gb_d"]), f8(i["gb_scale"]), f8(i["gb_shift"]), f8(i["gb_coef"]), case_slope(c), ge)
        assert c["exact"] or margin >= 1e-3, margin
        g = dy
    else:
        g = split_value(i["dy"]) if c["dy_split"] else f8(i["dy"])
    sc, sh = f8(i.get("scale")), f8(i.get("shift"))
    if sc is not None and c["x_c4"]:
        sc, sh = sc[:, :x.shape[1]], sh[:, :x.shape[1]]
    xp = staged(x, sc, sh, case_slope(c), transform_padding)
    if lose_lo:                                                       # the lo packets of x read as zero: hi x hi plus the one cross term lo(dy) x hi(x)
        xp = bf16_value(bf16_bits(xp.astype(np.float32)))
    if drop_last_plane:
        g = g.copy()
        g[:, :, -1] = 0.0
    if ring_reuse:                                                    # the z = -1 halo plane of a column holds the previous column's last plane
        xp = xp.copy()
        xp[:, :, 0, :, 17:] = xp[:, :, -2, :, 1:-16]
    dw = wgrad_padded(xp, g)
    if lose_last_block:
        dw[-16:] = 0.0
    co, ci = c["dw_cout"] or dw.shape[0], c["dw_cin"] or dw.shape[1]
    dw = dw[:co, :ci]
    if c["swapped"]:
        dw = swapped_form(dw, mirror)
    return dict(dw=dw, dy=dy, f=f)


# ---------------------------------------------------------------------------------------------------------------- restatements against the oracle
def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


SMALL = [(2, 16, 8, (3, 4, 5)), (1, 8, 16, (2, 5, 3))]                 # N, Cin, Cout, spatial


def _small(si, n, cin, cout, sp):
    x, dy = (draw(700 + 10 * si + t, *s).astype(np.float64) for t, s in enumerate([(n, cin) + sp, (n, cout) + sp]))
    gamma = draw(703 + 10 * si, cin).astype(np.float64) + np.where(np.arange(cin) % 2 == 0, 1.0, -1.0) * 1.5
    beta = draw(704 + 10 * si, cin).astype(np.float64) * 0.5 + 0.2
    return x, dy, gamma, beta


def _gn(x, gamma, beta):
    n, c = x.shape[:2]
    cpg = c // O.GN_GROUPS
    xg = x.reshape(n, O.GN_GROUPS, -1)
    mean, rstd = np.repeat(xg.mean(-1), cpg, 1), np.repeat(1.0 / np.sqrt(xg.var(-1) + O.GN_EPS), cpg, 1)
    return gamma[None] * rstd, beta[None] - gamma[None] * rstd * mean, mean, rstd


def test_weight_gradient_restatement_is_conv3d_weight():
    """plain: torch.nn.grad.conv3d_weight; transformed: autograd through GroupNorm -> LeakyReLU -> Conv3d, whose padding is Conv3d's own (after the activation)"""
    for si, (n, cin, cout, sp) in enumerate(SMALL):
        x, dy, gamma, beta = _small(si, n, cin, cout, sp)
        ref = torch.nn.grad.conv3d_weight(_t(x), (cout, cin, 3, 3, 3), _t(dy), padding=1).numpy()
        _close(wgrad_padded(staged(x), dy), ref)
        scale, shift, _, _ = _gn(x, gamma, beta)
        w = _t(draw(705 + si, cout, cin, 3, 3, 3), True)
        z = O.leaky_relu(O.group_norm(_t(x), _t(gamma), _t(beta)))
        (torch.nn.functional.conv3d(z, w, padding=1) * _t(dy)).sum().backward()
        _close(wgrad_padded(staged(x, scale, shift, O.LEAKY_SLOPE), dy), w.grad.numpy())
        _close(wgrad_padded(staged(x, scale, shift, O.LEAKY_SLOPE), dy)[:5, :3], w.grad.numpy()[:5, :3])


def test_swapped_restatement_is_the_weight_gradient_with_the_operands_exchanged():
    """kernel view x' = the convolution's output gradient, dy' = its input: the stored result is conv3d_weight(input = dy', grad_output = x')"""
    for si, (n, cin, cout, sp) in enumerate(SMALL):
        xin, dout, _, _ = _small(si, n, cin, cout, sp)
        ref = torch.nn.grad.conv3d_weight(_t(xin), (cout, cin, 3, 3, 3), _t(dout), padding=1).numpy()
        _close(swapped_form(wgrad_padded(staged(dout), xin)), ref)
        assert float(np.abs(swapped_form(wgrad_padded(staged(dout), xin), mirror=False) - ref).max()) > 1e-3


def test_apply_restatement_is_the_group_norm_backward():
    """z = leaky_relu(group_norm(a)): with (scale, shift) of the GroupNorm and the finalize coefficients cA = gamma rstd, cB = -rstd^2 S2 / m,
    cC = rstd (mean rstd S2 - S1) / m (S1 = sum gamma dh, S2 = sum gamma dh xhat over the group's m elements) the apply expression is autograd's gradient w.r.t. a"""
    for si, (n, c, _, sp) in enumerate(SMALL):
        a, _, gamma, beta = _small(si, n, c, c, sp)
        dz = draw(706 + si, n, c, *sp).astype(np.float64)
        ta = _t(a, True)
        (O.leaky_relu(O.group_norm(ta, _t(gamma), _t(beta))) * _t(dz)).sum().backward()
        scale, shift, mean, rstd = _gn(a, gamma, beta)
        b = lambda v: v[:, :, None, None, None]
        dh = np.where(a * b(scale) + b(shift) > 0, dz, dz * O.LEAKY_SLOPE)
        xhat = (a - b(mean)) * b(rstd)
        cpg, m = c // O.GN_GROUPS, (c // O.GN_GROUPS) * int(np.prod(sp))
        gsum = lambda v: np.repeat((v * gamma[None, :, None, None, None]).reshape(n, O.GN_GROUPS, -1).sum(-1), cpg, 1)
        s1, s2 = gsum(dh), gsum(dh * xhat)
        coef = np.stack([scale, -rstd * rstd * s2 / m, rstd * (mean * rstd * s2 - s1) / m], axis=2)      # dx = rstd (gamma dh - (S1 + xhat S2) / m)
        dy, _, margin = ref_apply(a, dz, scale, shift, coef, O.LEAKY_SLOPE)
        assert margin > 1e-7
        _close(dy, ta.grad.numpy(), 1e-10)


def test_bf16_and_e4m3_encoders_agree_with_torch():
    v = np.concatenate([draw(720, 4096) * s for s in (1e-3, 1.0, 100.0)] + [np.asarray([0.0, 448.0, 464.0, 1e4, -1e4, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -11, 0.0625 + 2.0 ** -8], np.float32)])
    t = torch.from_numpy(v)
    assert np.array_equal(bf16_bits(v), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    inr = np.abs(v) <= 448.0
    got = e4m3_encode(v.astype(np.float64))
    unsigned_zero = lambda b: np.where(b == 0x80, 0, b)
    assert np.array_equal(unsigned_zero(got[inr]), unsigned_zero(t[torch.from_numpy(inr)].to(torch.float8_e4m3fn).view(torch.uint8).numpy()))
    assert (got[~inr] & 0x7f == 0x7e).all()                           # saturating
    codes = np.arange(256, dtype=np.uint8)
    codes = codes[(codes & 0x7f) != 0x7f]
    assert np.array_equal(e4m3_encode(e4m3_decode(codes)), codes)     # every code is a fixed point
    assert np.array_equal(split_decode(split_encode(v[:4096 * 3].reshape(-1, 16))).ravel(), split_value(v[:4096 * 3]))


# ---------------------------------------------------------------------------------------------------------------- the exact family
EXACT_CASES = [c["name"] for c in CASES if c["exact"] and c["name"] not in TWINS]


def _units(a, what, bound=2.0 ** 23, unit=FINE):
    a = np.asarray(a, np.float64) / unit
    assert np.array_equal(a, np.round(a)), what
    assert float(np.abs(a).max(initial=0.0)) < bound, (what, float(np.abs(a).max()))


def _bf16_exact(a):
    return np.array_equal(bf16_value(bf16_bits(np.asarray(a, np.float32))), np.asarray(a, np.float64))


@pytest.mark.parametrize("name", EXACT_CASES)
def test_exact_family_is_exact(name):
    c = CASE_BY_NAME[name]
    i = make_inputs(c)
    f8 = lambda a: np.asarray(a, np.float64)
    for k, v in i.items():
        _units(v, (name, k), 2.0 ** 15)
    r = reference(c, i)
    sc, sh = (f8(i[k])[:, :i["x"].shape[1]] for k in ("scale", "shift")) if c["transform"] else (None, None)
    xa = staged(f8(i["x"]), sc, sh, case_slope(c))
    _units(xa, (name, "activated x"), 2.0 ** 15)
    if c["gb"]:
        b = lambda v: f8(v)[:, :, None, None, None]
        y, d = f8(i["gb_y"]), f8(i["gb_d"])
        u = y * b(i["gb_scale"]) + b(i["gb_shift"])
        assert (u == 0).any() and (d[u == 0] != 0).any(), name       # ties exist, so `>` against `>=` is visible
        dh = np.where(u > 0, d, d * case_slope(c))
        for what, v in (("y*scale", y * b(i["gb_scale"])), ("u", u), ("dh", dh), ("cA*dh", b(i["gb_coef"][:, :, 0]) * dh), ("cB*y", b(i["gb_coef"][:, :, 1]) * y),
                        ("cB*y + cC", b(i["gb_coef"][:, :, 1]) * y + b(i["gb_coef"][:, :, 2])), ("dy", r["dy"])):
            _units(v, (name, what), 2.0 ** 15)
        g = r["dy"]
    else:
        g = f8(i["dy"])
    assert np.array_equal(split_value(g.astype(np.float32)), g) and np.array_equal(split_value(xa.astype(np.float32)), xa), name        # hi + lo holds the value
    xe, ge = _bf16_exact(xa), _bf16_exact(g)
    assert xe or ge, name                                            # the dropped lo x lo product is zero
    assert c["products"] != 1 or (xe and ge), name                   # one product: operands are bf16 values
    assert fine_operand(c) is None or not (xe and ge), name          # ... and the fine cases do fill lo packets
    unit = FINE if fine_operand(c) else 1.0                          # (|hi| + |lo| <= (1 + 2^-8) |value|: the bound leaves a factor 2)
    _units(wgrad_padded(np.abs(xa), np.abs(g)), (name, "sum of |product|"), 2.0 ** 23, unit)
    _units(r["dw"], (name, "dw"), 2.0 ** 23, unit)
    assert float(np.abs(r["dw"]).max()) > 0


def test_real_family_draws_what_the_gpu_file_promises():
    for name in ("rag_gb_split_scale_real", "rag_gb_32_scale_real", "rag_16_16_scale_real"):
        c = CASE_BY_NAME[name]
        i = make_inputs(c)
        assert (i["scale"][:, 0] < 0).all() and (i["scale"][:, 1] == 0).all() and (i["shift"][:, 2] == 6).all() and float(np.abs(i["shift"]).min()) >= 0.1
        assert not np.array_equal(i["scale"][0], i["scale"][1])
        if c["gb"]:
            assert (i["gb_scale"][:, 0] < 0).all() and (i["gb_scale"][:, 1] == 0).all() and not np.array_equal(i["gb_coef"][0], i["gb_coef"][1])
            reference(c, i)                                           # asserts the margin


# ---------------------------------------------------------------------------------------------------------------- the encoders inside their bars
def test_encoders_meet_the_format_bars():
    for name in ("rag_gb_split_scale_real", "rag_gb_g16_scale_real", "rag_gb_32_scale_real"):
        c = CASE_BY_NAME[name]
        r = reference(c, make_inputs(c))
        ref, f = blocks(r["dy"]), blocks(r["f"])
        v32 = ref.astype(np.float32)
        for g16 in (False, True):
            ex = pub_excess((g16_encode if g16 else split_encode)(v32), v32.astype(np.float64), np.zeros_like(f), g16)
            print("  encoder %-8s on %-28s error / format bar %.3g" % ("g16" if g16 else "split", name, ex))
            assert ex <= 1.0
            assert pub_excess((g16_encode if g16 else split_encode)(v32), ref, f, g16) <= 1.0        # and against float64 with the rounding term


# ---------------------------------------------------------------------------------------------------------------- mutants
def test_mutants_exceed_every_bar():
    rows = []

    def dw_rows(what, names, **mutant):
        for name in names:
            c = CASE_BY_NAME[name]
            i = make_inputs(c)
            good, bad = reference(c, i)["dw"], reference(c, i, **mutant)["dw"]
            rows.append((what + ", " + name, exact_excess(bad, good) if c["exact"] else dw_excess(bad, good, c["products"] or 3)))

    dw_rows("transform applied to the halo", ("rag_16_16_scale_exact", "rag_16_16_scale_real", "rag_split_32_p1_scale_real"), transform_padding=True)
    dw_rows("last z plane dropped (odd D)", ("rag_16_16_scale_exact", "rag_16_16_scale_real", "rag_split_32_p1_scale_real"), drop_last_plane=True)
    dw_rows("first halo plane from the previous column", ("cols_64_d3_scale_exact", "cols_64_d3_scale_real", "cols_64_d7_real", "rag_split_32_p1_scale_real"), ring_reuse=True)
    dw_rows(">= at the apply threshold", ("rag_gb_split_scale_exact", "rag_gb_p1_scale_exact", "rag_gb_stem_exact"), ge=True)
    dw_rows("lo packets zeroed", ("rag_16_16_scale_real", "rag_gb_split_scale_real", "rag_xc4_real"), lose_lo=True)
    dw_rows("taps not mirrored", ("rag_head_swapped_exact", "rag_head_swapped_real"), mirror=False)
    dw_rows("last output block unwritten", ("rag_32_48_scale_exact", "rag_32_48_scale_real", "rag_16_48_real", "rag_32_80_scale_exact"), lose_last_block=True)
    # the published tensor
    for name in ("rag_gb_split_scale", "rag_gb_g16_scale"):
        g16 = name.endswith("g16_scale")
        enc = g16_encode if g16 else split_encode
        c = CASE_BY_NAME[name + "_exact"]
        i = make_inputs(c)
        good, bad = reference(c, i), reference(c, i, ge=True)
        rows.append((">= at the apply threshold, published bytes, " + c["name"],
                     exact_excess(canon(enc(blocks(bad["dy"]).astype(np.float32)), g16), canon(enc(blocks(good["dy"]).astype(np.float32)), g16))))
        if g16:
            v32 = blocks(good["dy"]).astype(np.float32)
            rows.append(("exponent from one channel half, published bytes, " + c["name"], exact_excess(canon(g16_encode(v32, per_half=True), True), canon(g16_encode(v32), True))))
        c = CASE_BY_NAME[name + "_real"]
        r = reference(c, make_inputs(c))
        v32 = blocks(r["dy"]).astype(np.float32)
        rows.append(("lo packets zeroed, published value, " + c["name"], pub_excess(enc(v32), blocks(r["dy"]), blocks(r["f"]), g16, zero_lo=True)))
        if g16:
            rows.append(("exponent from one channel half, published value, " + c["name"], pub_excess(g16_encode(v32, per_half=True), blocks(r["dy"]), blocks(r["f"]), True)))
    for what, ex in rows:
        print("  mutant %-92s error / bar %.3g" % (what, ex))
    for what, ex in rows:
        assert ex > 1.0, (what, ex)
