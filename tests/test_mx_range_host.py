"""The fp16 + MX-fp8 product scheme of the forward 3x3x3 convolutions (csrc/conv3_mx.hpp, conv3_wz32mx.hpp) and its gradient-operand form (conv3_mx_kernel<GRAD>)
as a MODEL on the CPU: what the operands convert to, bit for bit, and what that costs against float64 across operand magnitudes.  tests/test_mx_range.py holds
the kernels to this model on the device; nothing here needs a GPU, and nothing here is measured against a kernel.

Operand emulator (quantise / fwd_operands / wz_transform / grad_operands; float64 values of the codes, float64 accumulation):
  direct   f16(v) round-to-nearest-even with subnormals, saturating at 65504 (MODE.FP16_OVFL); lo = v - f16(v) with one float32 rounding (v_fma_mix_f32; exact
           wherever |v| <= 65504); activations e4m3(lo * 2^11), e4m3(v); weights e4m3(w * 2^8), e4m3(w_lo * 2^19); e4m3 round-to-nearest-even, subnormals down to
           2^-9, saturating at 448.  y = f16(x) f16(w) + 2^-19 [lo8(x) w8 + x8 lo8(w)]: the lo section of an activation packet meets the value weights and the
           value section the lo weights (k-group parity of the scaled MFMA), one E8M0 pair 2^-11 * 2^-8 for both.
  wz       the same conversions applied to the Winograd F(2,3)-in-z operands, formed in float32 in the order the code forms them: U0 = d0 - d2, U1 = d1 + d2,
           U2 = d2 - d1, U3 = d1 - d3 (wz_stage_waves), G0 = g0, G1 = 0.5 ((g0 + g2) + g1), G2 = 0.5 ((g0 + g2) - g1), G3 = g2 (wz32mx_pack_one); M_i = the 3x3
           (y, x) convolution of the converted U_i, G_i; plane 0 = M0 + (M1 + M2), plane 1 = M1 - (M2 + M3).
  grad     g16_encode of tests/test_wgrad3_fused_host.py (bf16 main term, e4m3(lo / 2^(e-8)), e4m3(g / 2^e), ONE exponent e per voxel recomputed by the reader
           from the voxel's 16 hi values) against bf16(w), e4m3(w * 2^8), e4m3((w - bf16(w)) * 2^16): y = hi bf16(w) + 2^(e-16) [lo8 w8 + g8 lo8(w)].
The conversions are checked against torch.float16 / torch.bfloat16 / torch.float8_e4m3fn where torch defines them, against the e4m3 / bf16 helpers of the
weight-gradient host file, and against hand-written tables at ties, subnormals and the saturation edge.

Range sweep (1 x 16 x 12^3 direct and grad, 1 x 32 x 12^3 Winograd-z; the distribution of the device tests: x = 1.3 lrelu(N(0,1)) + 0.1, w ~ N(0, 2 / (27 Cin))):
activations x 2^-24 .. 2^10, weights x 2^-16 .. 2^7, per-channel gains exp(s N(0,1)) on x compensated in w (s = 1.5, 3), heavy-tailed weights (1 % at 10 x);
grad: tensor scale 2^-60 .. 2^0 and a channel disparity of 1, 2^4, 2^8, 2^12 inside every voxel.  Error = max |y - float64| / RMS(float64) (grad: relative L2
and max / max |y|).  A point is IN RANGE when error <= 1.2e-4 and <= 4 x the emulated three-bf16-product error + 1e-6 (grad: 2.5e-4 relative L2 and 5e-4 of the
largest value).  MX_WINDOW holds the in-range run of powers of two around 1 per form and axis less one octave at each end (the reason stands at the constant), as
measured against float64; test_windows_are_what_the_sweep_measures asserts it, and brats2019_amd.model.MX_RANGE / the documents state the same numbers in absolute terms (max |x|, max |w|).  Outside the window the documented
degradation is asserted: finite, and no worse than ONE fp16 (grad: bf16) product plus the three-product error.

Exact tie family (tie_family): activations (1 + 2^-11) 2^j, (1 + 3 2^-11) 2^j (fp16 ties, residuals +-2^(j-11): exact in e4m3 after the 2^11 scale),
(1 + 19 2^-16) 2^j (the scaled residual 19 2^(j-5) ties in e4m3); a group in the e4m3 subnormal zone (j = -9 .. -7); a group at the saturation edge (448, 464,
480, and 1024 + 448 / 480 / 512 x 2^-11 whose residual codes are 448 and just beyond); weights: sparse signed powers of two (w = 2, 4 saturate e4m3(w * 2^8)) and a
few (1 + 2^-11) 2^i, whose lo operand is not zero, so that the value section of the activations is read.  test_tie_family_is_exact shows with integer arithmetic
(fractions) that every term of the emulated sum is an integer multiple of one power of two u and that the sum of their magnitudes stays below 2^24 u for every
output: every partial sum in ANY order is a float32, so a kernel that converts as modelled reproduces the emulated result bit for bit.

Mutants (test_mutants_are_caught): a scale exponent off by one, truncation instead of round-to-nearest-even, flushed e4m3 subnormals, no saturation, swapped lo /
value sections, for grad an exponent taken from one channel half -- each breaks equality on the tie family or exceeds a bar of the sweep.

`python tests/test_mx_range_host.py` writes profiles/mx_range.txt: the sweep, the windows and the seeded network's operand survey at 32^3."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

if __name__ == "__main__":                                            # run as a script (writes the profile): what tests/conftest.py does for pytest
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import resunet_oracle as O
from test_wgrad3_fused_host import bf16_bits, bf16_value, e4m3_decode, e4m3_encode, g16_encode, g16_exponent

SX, SWH, SWL = 11, 8, 19                      # conv3_mx_pack.hpp MX_SX, MX_SWH, MX_SWL
GSWH, GSWL = 8, 16                            # MXG_SWH, MXG_SWL
FMT = {"f16": (10, -14, 65504.0), "e4m3": (3, -6, 448.0), "bf16": (7, -126, float.fromhex("0x1.fep127"))}     # fraction bits, smallest normal exponent, largest value
BAR_RMS, BAR_X3, BAR_ABS = 1.2e-4, 4.0, 1e-6  # tests/test_hip_c16.py: test_conv3_mx_against_float64
BAR_G_L2, BAR_G_MAX = 2.5e-4, 5e-4            # test_conv3_gradient_operand_against_float64


class Mut(object):
    """the model's switches; the defaults are the model, every other value is a mutant"""

    def __init__(self, rne=True, subnormals=True, saturate=True, sx=0, swap=False, half=False):
        self.rne, self.subnormals, self.saturate, self.sx, self.swap, self.half = rne, subnormals, saturate, sx, swap, half


MODEL = Mut()
MUTANTS = {"scale exponent off by one": Mut(sx=1), "truncation instead of RNE": Mut(rne=False), "flushed e4m3 subnormals": Mut(subnormals=False),
           "no saturation": Mut(saturate=False), "swapped lo and value sections": Mut(swap=True)}
GRAD_MUTANTS = {"scale exponent off by one": Mut(sx=1), "swapped lo and value sections": Mut(swap=True), "exponent from one channel half": Mut(half=True),
                "truncated weight conversions": Mut(rne=False)}


# ---------------------------------------------------------------------------------------------------------------- formats
def quantise(v, fmt, m=MODEL):
    """the value a float conversion to `fmt` returns, in float64: round to nearest even on the format's grid (spacing 2^(e - fraction bits), e >= the smallest
    normal exponent: subnormals), saturating at the largest finite value.  Mutants: truncation, results below the smallest normal flushed (e4m3 only), no clamp."""
    mbits, emin, vmax = FMT[fmt]
    v = v.double()
    a = v.abs()
    # exponent and grid spacing by integer arithmetic on the float64 bits (torch.ldexp goes through a float32 pow, which is not exact on every device)
    e = (((a.view(torch.int64) >> 52) & 0x7ff) - 1023).clamp(min=emin)
    q = ((e - mbits + 1023) << 52).view(torch.float64)
    n = a / q                                                          # exact: a power-of-two quotient
    r = (torch.round(n) if m.rne else torch.floor(n)) * q              # torch.round: halves to even
    if fmt == "e4m3" and not m.subnormals:
        r = torch.where(r < 2.0 ** emin, torch.zeros_like(r), r)
    if m.saturate:
        r = r.clamp(max=vmax)
    return torch.copysign(r, v)


def f32(v):
    """one float32 rounding of a float64 value"""
    return v.float().double()


def fwd_operands(v32, side, m=MODEL):
    """float32 tensor -> (fp16 value, lo code, value code) of an activation ('x': mx_split8 / mx_split4) or a weight ('w': mx_pack_one / wz32mx_pack_one); the
    codes as the e4m3 values the matrix unit reads, scales not applied"""
    assert v32.dtype == torch.float32
    v = v32.double()
    h = quantise(v, "f16", m)
    lo = f32(v - h)
    if side == "x":
        return h, quantise(lo * 2.0 ** (SX + m.sx), "e4m3", m), quantise(v, "e4m3", m)
    return h, quantise(f32(lo * 2.0 ** SWL), "e4m3", m), quantise(f32(v * 2.0 ** SWH), "e4m3", m)


def conv_taps(x, w):
    """zero-padded 3^k-tap cross-correlation of [B, C, *spatial] with [O, C, 3, ...] in the tensors' dtype: one matmul per tap (the form the device file runs in
    float64; test_tap_form_is_conv3d)"""
    nd = x.dim() - 2
    xp = torch.nn.functional.pad(x, (1, 1) * nd).movedim(1, -1)
    y = None
    for tap in itertools.product(range(3), repeat=nd):
        sl = (slice(None),) + tuple(slice(t, t + s) for t, s in zip(tap, x.shape[2:]))
        t = xp[sl] @ w[(slice(None), slice(None)) + tap].t()
        y = t if y is None else y + t
    return y.movedim(-1, 1)


def _products(X, W, m, absolute):
    """main + 2^-19 (lo section x value weights + value section x lo weights) of converted operands (h, lo8, v8)"""
    if absolute:
        X, W = [t.abs() for t in X], [t.abs() for t in W]
    (xh, xl, xv), (wh, wl, wv) = X, W
    cross = conv_taps(xl, wl) + conv_taps(xv, wv) if m.swap else conv_taps(xl, wv) + conv_taps(xv, wl)
    return conv_taps(xh, wh) + cross * 2.0 ** -SWL


def emulate_direct(x, w, m=MODEL, absolute=False):
    """conv3_mx_kernel on float32 tensors [N, C, D, H, W], [O, C, 3, 3, 3] -> float64.  absolute: the sum of the magnitudes of the accumulated terms"""
    return _products(fwd_operands(x, "x", m), fwd_operands(w, "w", m), m, absolute)


def wz_transform(x, w):
    """float32 Winograd F(2,3)-in-z operands in the code's order: U [4][N * D/2, C, H, W], G [4][O, C, 3, 3]"""
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and x.shape[2] % 2 == 0
    n, c, d, h, wd = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 1, 1))
    dk = [xp[:, :, k:k + d:2] for k in range(4)]                       # planes z0 - 1 + k of the tile z0 = 2 t
    U = [dk[0] - dk[2], dk[1] + dk[2], dk[2] - dk[1], dk[1] - dk[3]]
    U = [u.permute(0, 2, 1, 3, 4).reshape(n * (d // 2), c, h, wd) for u in U]
    g = [w[:, :, i] for i in range(3)]
    G = [g[0], 0.5 * ((g[0] + g[2]) + g[1]), 0.5 * ((g[0] + g[2]) - g[1]), g[2]]
    return U, G


def wz_combine(M, n, absolute=False):
    """plane 0 = M0 + (M1 + M2), plane 1 = M1 - (M2 + M3) -> [N, O, D, H, W]"""
    y0 = M[0] + (M[1] + M[2])
    y1 = M[1] + (M[2] + M[3]) if absolute else M[1] - (M[2] + M[3])
    t, o, h, wd = y0.shape
    y = torch.stack([y0, y1], dim=1).reshape(n, t // n, 2, o, h, wd)
    return y.permute(0, 3, 1, 2, 4, 5).reshape(n, o, 2 * (t // n), h, wd)


def emulate_wz(x, w, m=MODEL, absolute=False):
    """conv3_wz32mx_kernel"""
    U, G = wz_transform(x, w)
    return wz_combine([_products(fwd_operands(U[i], "x", m), fwd_operands(G[i], "w", m), m, absolute) for i in range(4)], x.shape[0], absolute)


def grad_operands(g32, m=MODEL):
    """[N, 16, D, H, W] float32 -> (bf16 hi, lo code * 2^e, value code * 2^e) in float64, through the bytes of the gradient-operand form; the exponent is the one
    the READER recomputes from the voxel's 16 hi values.  Mutant half: the writer took it per channel half."""
    assert g32.shape[1] == 16
    v = np.ascontiguousarray(g32.permute(0, 2, 3, 4, 1).cpu().numpy(), np.float32)
    b = g16_encode(v, per_half=m.half)
    hi = bf16_value(np.ascontiguousarray(b[..., :32]).view(np.uint16))
    sc = np.ldexp(1.0, g16_exponent(hi) + m.sx)
    l8 = e4m3_decode(np.concatenate([b[..., 32:40], b[..., 48:56]], axis=-1)) * sc
    x8 = e4m3_decode(np.concatenate([b[..., 40:48], b[..., 56:64]], axis=-1)) * sc
    return [torch.from_numpy(np.ascontiguousarray(t)).permute(0, 4, 1, 2, 3).to(g32.device) for t in (hi, l8, x8)]


def grad_weight_operands(w32, m=MODEL):
    """the weight the convolution applies (for a data gradient: dgrad_weight of the forward weight) -> (bf16, e4m3(w * 2^8), e4m3((w - bf16(w)) * 2^16))"""
    w = w32.double()
    h = quantise(w, "bf16")
    return h, quantise(f32(f32(w - h) * 2.0 ** GSWL), "e4m3", m), quantise(f32(w * 2.0 ** GSWH), "e4m3", m)


def emulate_grad(g, w, m=MODEL, absolute=False):
    """conv3_mx_kernel<GRAD>"""
    X, W = grad_operands(g, m), grad_weight_operands(w, m)
    if absolute:
        X, W = [t.abs() for t in X], [t.abs() for t in W]
    (gh, gl, gv), (wh, wl, wv) = X, W
    cross = conv_taps(gl, wl) + conv_taps(gv, wv) if m.swap else conv_taps(gl, wv) + conv_taps(gv, wl)
    return conv_taps(gh, wh) + cross * 2.0 ** -GSWL


EMULATE = {"direct": emulate_direct, "wz": emulate_wz, "grad": emulate_grad}


def three_products(x, w):
    """the split-bf16 scheme: hi hi + lo hi + hi lo (float64 accumulation)"""
    xh, wh = quantise(x, "bf16"), quantise(w, "bf16")
    xl, wl = quantise(f32(x.double() - xh), "bf16"), quantise(f32(w.double() - wh), "bf16")
    return conv_taps(xh, wh) + conv_taps(xl, wh) + conv_taps(xh, wl)


def one_product(x, w, fmt, form="direct"):
    """ONE product of the main-term format: what is left of the scheme when both cross terms carry nothing (wz: of the transformed operands)"""
    if form == "wz":
        U, G = wz_transform(x, w)
        return wz_combine([conv_taps(quantise(U[i], fmt), quantise(G[i], fmt)) for i in range(4)], x.shape[0])
    return conv_taps(quantise(x, fmt), quantise(w, fmt))


def err_rms(y, ref):
    return float((y - ref).abs().max() / ref.pow(2).mean().sqrt())


def err_grad(y, ref):
    return float((y - ref).norm() / ref.norm()), float((y - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- the sweep
def draw_x(seed, n, c, *sp):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, *sp, generator=g)
    return torch.where(x > 0, x, 0.01 * x) * 1.3 + 0.1


def draw_w(seed, cout, cin):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, 3, 3, 3, generator=g) * float((2.0 / (cin * 27)) ** 0.5)


def gains(seed, c, spread):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(spread * torch.randn(c, generator=g))


def compensated(x, w, gain):
    return (x * gain.view(1, -1, 1, 1, 1)).float(), (w / gain.view(1, -1, 1, 1, 1)).float()


def heavy_tailed(w, seed, every=97, factor=10.0):
    """about 1 % of the weights at `factor` x their drawn value"""
    w = w.clone()
    flat = w.view(-1)
    flat[seed % every::every] *= factor
    return w


def draw_grad(seed, n, c, *sp):
    """tests/test_hip_c16.py: magnitudes around 1e-6 that change by decades from voxel to voxel and channel to channel"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(2.5 * torch.randn(n, 1, *sp, generator=g)) * 1e-6
    chan = torch.exp(1.5 * torch.randn(1, c, 1, 1, 1, generator=g))
    return (torch.randn(n, c, *sp, generator=g) * mag * chan).float()


def disparity(g, log2):
    """channel c of every voxel scaled by 2^-(log2 * c / 15): the voxel's one exponent serves channels `log2` octaves apart"""
    c = g.shape[1]
    return (g * torch.exp2(-log2 * torch.arange(c, dtype=torch.float32) / (c - 1)).view(1, -1, 1, 1, 1)).float()


SWEEP_SHAPE = {"direct": (1, 16, 16), "wz": (1, 32, 32), "grad": (1, 16, 16)}
X_LOG2, W_LOG2 = range(-24, 11), range(-16, 8)
G_LOG2, G_DISPARITY = range(-60, 1, 6), (0, 4, 8, 12)
GAIN_SPREADS = (1.5, 3.0)


def fwd_point(form, x, w):
    """-> dict of the errors of one operand point against float64: scheme, three products, one fp16 product; in_range by the bars"""
    x, w = x.float(), w.float()
    ref = conv_taps(x.double(), w.double())
    e = err_rms(EMULATE[form](x, w), ref)
    e3, e1 = err_rms(three_products(x, w), ref), err_rms(one_product(x, w, "f16", form), ref)
    finite = bool(np.isfinite(e))
    return dict(e=e, e3=e3, e1=e1, finite=finite, max_x=float(x.abs().max()), rms_x=float(x.pow(2).mean().sqrt()), max_w=float(w.abs().max()),
                in_range=finite and e <= BAR_RMS and e <= BAR_X3 * e3 + BAR_ABS, envelope=finite and e <= e1 + e3)


def grad_point(g, w):
    g, w = g.float(), w.float()
    ref = conv_taps(g.double(), w.double())
    (l2, mx), (l3, m3), (l1, m1) = err_grad(emulate_grad(g, w), ref), err_grad(three_products(g, w), ref), err_grad(one_product(g, w, "bf16"), ref)
    finite = bool(np.isfinite(l2) and np.isfinite(mx))
    return dict(e=l2, emax=mx, e3=l3, e1=l1, emax1=m1, emax3=m3, finite=finite, max_x=float(g.abs().max()), in_range=finite and l2 <= BAR_G_L2 and mx <= BAR_G_MAX,
                envelope=finite and l2 <= l1 + l3 and mx <= m1 + m3)


_SWEEP = {}


def sweep(form):
    """every point of a form's sweep, computed once per process: {(axis, key): point}"""
    if form in _SWEEP:
        return _SWEEP[form]
    n, cin, cout = SWEEP_SHAPE[form]
    pts = {}
    if form == "grad":
        g, w = draw_grad(41, n, cin, 12, 12, 12), draw_w(42, cout, cin)
        for k in G_LOG2:
            pts[("scale", k)] = grad_point(g * 2.0 ** k, w)
        for d in G_DISPARITY:
            pts[("disparity", d)] = grad_point(disparity(g, d), w)
    else:
        x, w = draw_x(21, n, cin, 12, 12, 12), draw_w(22, cout, cin)
        for k in X_LOG2:
            pts[("x", k)] = fwd_point(form, x * 2.0 ** k, w)
        for k in W_LOG2:
            pts[("w", k)] = fwd_point(form, x, w * 2.0 ** k)
        for s in GAIN_SPREADS:
            pts[("gain", s)] = fwd_point(form, *compensated(x, w, gains(23, cin, s)))
        pts[("heavy", 10)] = fwd_point(form, x, heavy_tailed(w, 24))
    _SWEEP[form] = pts
    return pts


def run_around_zero(pts, axis, keys):
    """the in-range run of consecutive keys around 0"""
    keys = list(keys)
    assert pts[(axis, 0)]["in_range"]
    lo = hi = 0
    while lo - 1 in keys and pts[(axis, lo - 1)]["in_range"]:
        lo -= 1
    while hi + 1 in keys and pts[(axis, hi + 1)]["in_range"]:
        hi += 1
    return lo, hi


# The in-range windows, measured against float64 by the sweep above (never against a kernel): log2 of the factor on the test distribution, and the same ends in
# absolute terms -- what brats2019_amd.model.MX_RANGE, INTEGRATION.md and DESIGN.md section 2 state.  A window is the in-range run of the sweep LESS ONE OCTAVE AT
# EACH END: the ends of the run sit on the flank of the error curve (the error doubles per octave there), and the error is a maximum over the outputs, which grows
# with their number -- the model on the device file's tensors (2 M outputs against 27 k here) measures 1.20e-4 at the direct kernel's weights x 2^3 and 9.9e-5 at the
# Winograd kernel's activations x 2^6, at or over the bar, and no more than 8.5e-5 one octave further in.
MARGIN_OCTAVES = 1
MX_WINDOW = {
    "direct": dict(x_log2=(-4, 5), w_log2=(-8, 2), x_rms=(0.0617, 31.6), x_max=(0.336, 172.0), w_max=(1.06e-3, 1.09)),
    "wz": dict(x_log2=(-4, 5), w_log2=(-7, 2), x_rms=(0.0617, 31.6), x_max=(0.382, 195.0), w_max=(1.50e-3, 0.769)),
}
GRAD_WINDOW = dict(scale_log2=(-60, 0), disparity_log2=(0, 12))      # flat: every point of the sweep is in range


def in_window(form, x, w):
    """whether an operand pair lies inside a form's window, in the absolute terms the documents state: RMS of x within x_rms, max |x| <= the upper x_max,
    max |w| within w_max (what model.mx_range_report applies to a layer)"""
    win = MX_WINDOW[form]
    rms, mx, mw = float(x.double().pow(2).mean().sqrt()), float(x.abs().max()), float(w.abs().max())
    return win["x_rms"][0] <= rms <= win["x_rms"][1] and mx <= win["x_max"][1] and win["w_max"][0] <= mw <= win["w_max"][1]


# ---------------------------------------------------------------------------------------------------------------- the exact tie family
TIE_GROUPS = ("tie", "sub", "sat")
TIE_SHAPE = {"direct": (1, 16, 16, (8, 12, 20)), "wz": (1, 32, 32, (8, 12, 20)), "grad": (1, 16, 16, (8, 12, 20))}


def _choice(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def tie_family(form, group, n, cin, cout, sp, seed=5):
    """float32 (x, w) of the exact family: half the activations zero, about four taps per output channel"""
    gen = torch.Generator().manual_seed(seed + 10 * TIE_GROUPS.index(group) + 100 * ("direct", "wz", "grad").index(form))
    sign = lambda shape: _choice(gen, [-1.0, 1.0], shape)
    # (wz: the transform adds and subtracts planes, which would turn the ties into other values and cost the family bits of its 24: activations sit on the planes
    # z = 1 mod 3 only, so that no two of a tile's four planes that the transform combines are both non-zero and every U is +- one activation; one octave)
    wz = form == "wz"
    wmask = (torch.randint(0, 8 * cin, (cout, cin, 3, 3, 3), generator=gen) == 0).double()
    if form == "grad":
        # bf16 ties (1 + 2^-8) 2^j -> 2^j, (1 + 3 2^-8) 2^j -> (1 + 2^-6) 2^j: residuals -+2^(j-8) = 128 2^-d after the voxel's scale; channel c of a voxel sits d(c) octaves
        # below its largest (d <= 4), in half the voxels the upper channel half two octaves below the lower; weights +-2^i, +-(1 + 2^-8) 2^i (lo != 0), +-19/16 2^i (e4m3 tie)
        base = _choice(gen, [1.0, 2.0], (n, 1) + sp)
        d = torch.randint(0, 3, (n, cin) + sp, generator=gen).double()
        d[:, 0] = 0
        d[:, cin // 2:] += 2.0 * torch.randint(0, 2, (n, 1) + sp, generator=gen).double()
        x = _choice(gen, [1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], (n, cin) + sp) * base * torch.exp2(-d) * sign((n, cin) + sp)
        x = x * (torch.randint(0, 2, (n, cin) + sp, generator=gen) == 0)
        x[:, 0] = torch.where(x[:, 0] == 0, base[:, 0], x[:, 0])      # every voxel keeps its largest channel
        w = _choice(gen, [0.5, 1.0, 2.0, 1 + 2.0 ** -8, 0.5 * (1 + 2.0 ** -8), 19.0 / 16], (cout, cin, 3, 3, 3)) * sign((cout, cin, 3, 3, 3)) * wmask
        return x.float(), w.float()
    if group == "sat":
        xv = [448.0, 464.0, 480.0, 1024.0, 1024 + 448 * 2.0 ** -11, 1024 + 480 * 2.0 ** -11, 1024 + 512 * 2.0 ** -11]
    else:
        js = ((0,) if wz else (0, 1)) if group == "tie" else ((-8,) if wz else (-9, -8, -7))
        xv = [f * 2.0 ** j for j in js for f in (1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 19 * 2.0 ** -16)]
    x = _choice(gen, xv, (n, cin) + sp) * sign((n, cin) + sp) * (torch.randint(0, 2, (n, cin) + sp, generator=gen) == 0)
    if wz:
        x = x * (torch.arange(sp[0]) % 3 == 1).double().view(1, 1, -1, 1, 1)
    wv = [1.0, 2.0, 4.0, 1 + 2.0 ** -11] if wz else [0.5, 1.0, 2.0, 4.0, 1 + 2.0 ** -11, 0.5 * (1 + 2.0 ** -11)]
    if group == "sat":
        wv.remove(4.0)
    w = _choice(gen, wv, (cout, cin, 3, 3, 3)) * sign((cout, cin, 3, 3, 3)) * wmask
    return x.float(), w.float()


def _lowbit(values):
    """the largest power of two (a Fraction) that divides every non-zero value of a float tensor, by integer arithmetic on its distinct values"""
    u = None
    for v in torch.unique(values.detach().cpu().double()).tolist():
        if v == 0.0:
            continue
        f = Fraction(abs(v))
        assert f.denominator & (f.denominator - 1) == 0
        b = Fraction(f.numerator & -f.numerator, f.denominator)
        u = b if u is None or b < u else u
    return u


def operand_classes(form, x, w, m=MODEL):
    """[(activation operand, weight operand, scale of the product)] of every matrix product of a form"""
    if form == "grad":
        X, W = grad_operands(x, m), grad_weight_operands(w, m)
        return [(X[0], W[0], 1.0), (X[1], W[2], 2.0 ** -GSWL), (X[2], W[1], 2.0 ** -GSWL)]
    pairs = [(x, w)] if form == "direct" else list(zip(*wz_transform(x, w)))
    out = []
    for a, b in pairs:
        X, W = fwd_operands(a, "x", m), fwd_operands(b, "w", m)
        out += [(X[0], W[0], 1.0), (X[1], W[2], 2.0 ** -SWL), (X[2], W[1], 2.0 ** -SWL)]
    return out


def exactness(form, x, w):
    """-> (emulated result, unit u, max over outputs of sum |terms| / (2^24 u)).  Every term of every matrix product is an integer multiple of u (each operand a
    multiple of its tensor's lowbit: Fractions); the float64 sums are exact (asserted: integers of u below 2^53).  A ratio < 1 makes every partial sum of the terms,
    in any order and grouping, an integer of u below 2^24: a float32."""
    u = min(_lowbit(a) * _lowbit(b) * Fraction(s) for a, b, s in operand_classes(form, x, w) if _lowbit(a) is not None and _lowbit(b) is not None)
    y, tot = EMULATE[form](x, w), EMULATE[form](x, w, absolute=True)
    for t in (y, tot):
        k = t / float(u)
        assert bool((k == k.round()).all()) and float(k.abs().max()) < 2.0 ** 53
    return y, u, float(tot.max()) / (2.0 ** 24 * float(u))


# ---------------------------------------------------------------------------------------------------------------- tests: the formats
def _log_uniform(seed, count, lo, hi):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(lo + (hi - lo) * torch.rand(count, generator=g))
    return (mag * torch.where(torch.rand(count, generator=g) < 0.5, -1.0, 1.0)).float()


def test_formats_against_torch_conversions():
    v = torch.cat([_log_uniform(1, 200000, -30, 17), _log_uniform(2, 100000, -12, 9.2), torch.tensor([0.0, -0.0, 65504.0, 448.0, -448.0, 2.0 ** -24, 2.0 ** -9])])
    ok = v.abs() < 65520
    assert torch.equal(quantise(v, "f16")[ok], v[ok].to(torch.float16).double())
    assert bool((quantise(v, "f16")[~ok].abs() == 65504.0).all())                          # torch: inf; MODE.FP16_OVFL: saturation
    assert torch.equal(quantise(v, "bf16"), v.to(torch.bfloat16).double())
    ok = v.abs() <= 448
    assert torch.equal(quantise(v, "e4m3")[ok], v[ok].to(torch.float8_e4m3fn).float().double())
    # the helpers the gradient-operand form is written with (tests/test_wgrad3_fused_host.py)
    assert np.array_equal(quantise(v, "e4m3").numpy(), e4m3_decode(e4m3_encode(v.double().numpy())))
    assert np.array_equal(quantise(v, "bf16").numpy(), bf16_value(bf16_bits(v.numpy())))


F16_TABLE = [(1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9), (1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -10), (2049.0, 2048.0), (2051.0, 2052.0),
             (2.0 ** -24, 2.0 ** -24), (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -25 * (1 + 2.0 ** -10), 2.0 ** -24), (1023.5 * 2.0 ** -24, 2.0 ** -14),
             (65504.0, 65504.0), (65519.0, 65504.0), (65520.0, 65504.0), (1e6, 65504.0), (-1e30, -65504.0)]
E4M3_TABLE = [(17.0, 16.0), (18.0, 18.0), (19.0, 20.0), (21.0, 20.0), (2.0 ** -9, 2.0 ** -9), (2.0 ** -10, 0.0), (3 * 2.0 ** -10, 2.0 ** -8), (2.0 ** -10 * (1 + 2.0 ** -20), 2.0 ** -9),
              (7 * 2.0 ** -9, 7 * 2.0 ** -9), (7.5 * 2.0 ** -9, 2.0 ** -6), (448.0, 448.0), (463.0, 448.0), (464.0, 448.0), (480.0, 448.0), (-3e4, -448.0), (0.0, 0.0)]


def test_formats_against_hand_written_tables():
    """ties (to even), subnormals (f16 spacing 2^-24, e4m3 spacing 2^-9), and the saturation edge (65504; 448 -- 464 would round to the NaN code's neighbour 480)"""
    for fmt, table in (("f16", F16_TABLE), ("e4m3", E4M3_TABLE)):
        got = quantise(torch.tensor([a for a, _ in table], dtype=torch.float64), fmt).tolist()
        assert got == [b for _, b in table], (fmt, got)
    t = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 19 * 2.0 ** -16, 2.0 ** -9 * (1 + 2.0 ** -11), 1024 + 480 * 2.0 ** -11], dtype=torch.float32)
    h, l8, v8 = fwd_operands(t, "x")
    assert h.tolist() == [1.0, 1 + 2.0 ** -9, 1.0, 2.0 ** -9, 1024.0] and l8.tolist() == [1.0, -1.0, 0.625, 2.0 ** -9, 448.0] and v8.tolist() == [1.0, 1.0, 1.0, 2.0 ** -9, 448.0]
    h, l8, v8 = fwd_operands(torch.tensor([1.0, 2.0, -(1 + 2.0 ** -11), 2.0 ** -12]), "w")
    assert h.tolist() == [1.0, 2.0, -1.0, 2.0 ** -12] and l8.tolist() == [0.0, 0.0, -256.0, 0.0] and v8.tolist() == [256.0, 448.0, -256.0, 2.0 ** -4]


def test_tap_form_is_conv3d_and_the_winograd_identity_holds():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 5, 6, 7, 9, generator=g, dtype=torch.float64), torch.randn(4, 5, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv3d(x, w, padding=1)
    assert float((conv_taps(x, w) - ref).abs().max()) <= 1e-12
    x2, w2 = x[:, :, 0], w[:, :, 0]
    assert float((conv_taps(x2, w2) - torch.nn.functional.conv2d(x2, w2, padding=1)).abs().max()) <= 1e-12
    # the transform in float64 (no conversion anywhere): F(2,3) in z is the convolution
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 1, 1))
    dk = [xp[:, :, k:k + 6:2] for k in range(4)]
    U = [(dk[0] - dk[2]), (dk[1] + dk[2]), (dk[2] - dk[1]), (dk[1] - dk[3])]
    U = [u.permute(0, 2, 1, 3, 4).reshape(6, 5, 7, 9) for u in U]
    G = [w[:, :, 0], 0.5 * (w[:, :, 0] + w[:, :, 2] + w[:, :, 1]), 0.5 * (w[:, :, 0] + w[:, :, 2] - w[:, :, 1]), w[:, :, 2]]
    assert float((wz_combine([conv_taps(U[i], G[i]) for i in range(4)], 2) - ref).abs().max()) <= 1e-12
    # and wz_transform forms the same operands to float32 rounding
    U32, G32 = wz_transform(x.float(), w.float())
    assert all(float((U32[i].double() - U[i]).abs().max()) <= 1e-5 and float((G32[i].double() - G[i]).abs().max()) <= 1e-6 for i in range(4))


# ---------------------------------------------------------------------------------------------------------------- tests: the windows
@pytest.mark.parametrize("form", ["direct", "wz"])
def test_windows_are_what_the_sweep_measures(form):
    pts, win = sweep(form), MX_WINDOW[form]
    for axis, keys in (("x", X_LOG2), ("w", W_LOG2)):
        lo, hi = run_around_zero(pts, axis, keys)
        assert [k for k in keys if pts[(axis, k)]["in_range"]] == list(range(lo, hi + 1))       # one run: nothing outside it is in range
        assert win[axis + "_log2"] == (lo + MARGIN_OCTAVES, hi - MARGIN_OCTAVES), (axis, lo, hi)
    near = lambda a, b: abs(a - b) <= 5e-3 * b
    for i in (0, 1):
        assert near(pts[("x", win["x_log2"][i])]["rms_x"], win["x_rms"][i]) and near(pts[("x", win["x_log2"][i])]["max_x"], win["x_max"][i])
        assert near(pts[("w", win["w_log2"][i])]["max_w"], win["w_max"][i])
    # the absolute form of the window agrees with the sweep on EVERY point, the compensated gains and the heavy-tailed weights included: inside implies in range
    # (the gains leave through max |w| and max |x|, the heavy tail through max |w|)
    for key, p in pts.items():
        t = 1 + 5e-3                                                  # (the constants are the ends to three digits)
        inside = win["x_rms"][0] <= p["rms_x"] * t and p["rms_x"] <= win["x_rms"][1] * t and p["max_x"] <= win["x_max"][1] * t and win["w_max"][0] <= p["max_w"] * t \
            and p["max_w"] <= win["w_max"][1] * t
        assert p["in_range"] or not inside, (key, p)
        if key[0] in "xw":
            assert inside == (win[key[0] + "_log2"][0] <= key[1] <= win[key[0] + "_log2"][1]), key
        else:
            assert not inside, key


def test_gradient_operand_form_is_flat_in_scale_and_holds_channel_disparity():
    pts = sweep("grad")
    base = pts[("scale", 0)]
    for k in G_LOG2:                                                   # one exponent per voxel: a power-of-two factor changes no code
        assert pts[("scale", k)]["in_range"] and abs(pts[("scale", k)]["e"] - base["e"]) <= 1e-9 * base["e"], (k, pts[("scale", k)])
    assert GRAD_WINDOW["scale_log2"] == (min(G_LOG2), max(G_LOG2)) and GRAD_WINDOW["disparity_log2"] == (min(G_DISPARITY), max(G_DISPARITY))
    assert all(pts[("disparity", d)]["in_range"] for d in G_DISPARITY)


@pytest.mark.parametrize("form", ["direct", "wz", "grad"])
def test_outside_the_window_the_scheme_degrades_to_one_product(form):
    """every point of the sweep, in range or not: finite, and no worse than ONE product of the main-term format plus the three-product error"""
    for key, p in sweep(form).items():
        assert p["finite"] and p["envelope"], (form, key, p)


def test_the_package_states_the_windows_the_sweep_measures():
    from brats2019_amd import model as M
    for form, kernel in (("direct", "conv3_mx"), ("wz", "conv3_wz32mx")):
        r = M.MX_RANGE[kernel]
        assert (r["x_rms"], r["x_max"], r["w_max"]) == (MX_WINDOW[form]["x_rms"], MX_WINDOW[form]["x_max"], MX_WINDOW[form]["w_max"])


# ---------------------------------------------------------------------------------------------------------------- tests: the tie family and the mutants
@pytest.mark.parametrize("form", ["direct", "wz", "grad"])
def test_tie_family_is_exact(form):
    n, cin, cout, sp = TIE_SHAPE[form]
    for group in (TIE_GROUPS if form != "grad" else ("tie",)):
        x, w = tie_family(form, group, n, cin, cout, sp)
        y, u, ratio = exactness(form, x, w)
        print("  %s %s: unit 2^%d, worst sum |terms| / (2^24 unit) %.3g, %d of %d outputs non-zero" % (form, group, round(np.log2(float(u))), ratio,
                                                                                                   int((y != 0).sum()), y.numel()))
        assert ratio < 1.0 and torch.equal(y.float().double(), y)
        assert int((y != 0).sum()) > y.numel() // 5
        if form != "grad":                                                # the family rounds where it says it does
            h, l8, v8 = fwd_operands(x, "x")
            assert bool((h != x.double()).any()) and bool((l8 != 0).any())
            if group == "sub":
                assert bool(((l8 != 0) & (l8.abs() < 2.0 ** -6)).any())
            if group == "sat":
                assert bool((l8.abs() == 448).any()) and bool((f32(x.double() - h) * 2.0 ** SX > 448).any()) and bool((x.abs() > 448).any())


@pytest.mark.parametrize("form", ["direct", "wz"])
def test_mutants_are_caught(form):
    n, cin, cout, sp = TIE_SHAPE[form]
    fam = {g: tie_family(form, g, n, cin, cout, sp) for g in TIE_GROUPS}
    model = {g: EMULATE[form](*fam[g]) for g in TIE_GROUPS}
    where = {"scale exponent off by one": "tie", "truncation instead of RNE": "tie", "flushed e4m3 subnormals": "sub", "no saturation": "sat",
             "swapped lo and value sections": "tie"}
    x, w = draw_x(21, *SWEEP_SHAPE[form][:2], 12, 12, 12), draw_w(22, SWEEP_SHAPE[form][2], SWEEP_SHAPE[form][1])
    ref = conv_taps(x.double(), w.double())
    for name, m in MUTANTS.items():
        g = where[name]
        differs = int((EMULATE[form](*fam[g], m=m) != model[g]).sum())
        e = err_rms(EMULATE[form](x, w, m=m), ref)
        print("  %s, %s: %d outputs of the %s group differ; sweep point 1 x 1: error / rms %.2e (bar %.1e)" % (form, name, differs, g, e, BAR_RMS))
        assert differs > 0, name


def test_gradient_mutants_are_caught():
    n, cin, cout, sp = TIE_SHAPE["grad"]
    x, w = tie_family("grad", "tie", n, cin, cout, sp)
    model = emulate_grad(x, w)
    for name, m in GRAD_MUTANTS.items():
        differs = int((emulate_grad(x, w, m=m) != model).sum())
        print("  grad, %s: %d outputs differ" % (name, differs))
        assert differs > 0, name


# ---------------------------------------------------------------------------------------------------------------- network level: parameter sets, report, survey
GN_KINDS = ("signs", "zeros", "tiny", "ties")
NETWORK_SETS = ["seeded"] + ["%s_x%s" % (k, f) for k in GN_KINDS for f in ("30", "0.01")] + ["w8"]
W8_BLOCK = "encoder_convs.0.1."                                       # a 32-channel Residual block: both of its 3x3x3 weights x 8
NETWORK_SEED = 31


def network_params(name, cfg=O.DEFAULT_CFG):
    """state dict (float32 numpy) of a network-level case: 'seeded' -- O.make_params; '<kind>_x<f>' -- every GroupNorm's (gamma, beta) = gn_param_set(kind) of
    tests/test_hip_ops.py times f; 'w8' -- the 3x3x3 weights of one Residual block times 8"""
    from test_hip_ops import gn_param_set
    p = O.make_params(NETWORK_SEED, **cfg)
    if name == "seeded":
        return p
    if name == "w8":
        for k in p:
            if k.startswith(W8_BLOCK) and p[k].ndim == 5 and p[k].shape[2:] == (3, 3, 3):
                p[k] = (p[k] * 8).astype(np.float32)
        return p
    kind, f = name.rsplit("_x", 1)
    rng = np.random.default_rng(7)
    for k in list(p):
        if p[k].ndim == 1 and k.endswith(".weight") and k[:-6] + "bias" in p:
            g, b = gn_param_set(kind, p[k].size, rng)
            p[k], p[k[:-6] + "bias"] = (g * float(f)).astype(np.float32), (b * float(f)).astype(np.float32)
    return p


def network_inside(name):
    """whether mx_range_report puts every layer of a parameter set inside the windows (what the device file's network test branches on)"""
    from brats2019_amd import model as M
    return all(r["inside"] for r in M.mx_range_report({k: torch.from_numpy(v) for k, v in network_params(name).items()}))


NETWORK_INSIDE = {n: n == "seeded" for n in NETWORK_SETS}            # x 30: max sqrt(gamma^2 + beta^2) = 47 > 31.6; x 0.01: 0.016 < 0.062; w8: max |w| 1.9 > 0.77


def test_range_report_on_the_network_parameter_sets():
    from brats2019_amd import model as M
    assert {n: network_inside(n) for n in NETWORK_SETS} == NETWORK_INSIDE
    rows = M.mx_range_report({k: torch.from_numpy(v) for k, v in network_params("seeded").items()})
    spec = dict(O.state_dict_spec(**O.DEFAULT_CFG))
    convs = [k for k, s in spec.items() if len(s) == 5 and tuple(s[2:]) == (3, 3, 3) and M.mx_kernel_of(s[1], s[0])]
    norms = [k for k, s in spec.items() if len(s) == 1 and k.endswith(".weight") and k[:-6] + "bias" in spec and k != "conv_output.weight"]
    assert [r["name"] for r in rows if r["kind"] == "weight"] == convs and [r["name"] for r in rows if r["kind"] == "activation"] == norms
    assert "conv_input.weight" not in convs and "conv_output.weight" not in convs           # 4 -> 16 and 16 -> 3: no fp16 + MX-fp8 kernel
    assert all(r["kernel"] == ("conv3_mx" if spec[r["name"]][-1 if r["kind"] == "activation" else 1] == 16 else "conv3_wz32mx") for r in rows)
    # the rows that leave the windows are the ones that were moved
    out = [r for r in M.mx_range_report({k: torch.from_numpy(v) for k, v in network_params("w8").items()}) if not r["inside"]]
    assert out and {r["name"] for r in out} <= {W8_BLOCK + "conv1.conv1.weight", W8_BLOCK + "conv2.conv1.weight"} and all(r["value"] > r["hi"] for r in out)
    n_w8 = len(out)
    out = [r for r in M.mx_range_report({k: torch.from_numpy(v) for k, v in network_params("signs_x0.01").items()}) if not r["inside"]]
    assert [r["name"] for r in out] == norms and all(r["value"] < r["lo"] for r in out)
    # a module works like its state dict
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in network_params("w8").items()})
    assert M.mx_range_report(net) == M.mx_range_report(net.state_dict())
    assert len([r for r in M.mx_range_report(net) if not r["inside"]]) == n_w8


def test_range_warning_is_given_once_and_names_the_switch():
    import warnings
    from brats2019_amd import model as M
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in network_params("seeded").items()})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert M.warn_mx_range(net) == []
    net.load_state_dict({k: torch.from_numpy(v) for k, v in network_params("w8").items()})
    with pytest.warns(RuntimeWarning, match="RU_MX=0") as rec:
        out = M.warn_mx_range(net)
    assert out and all(r["name"].startswith(W8_BLOCK) and r["name"] in str(rec[0].message) for r in out)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert M.warn_mx_range(net) == []                            # once per model and set of weights
    net.load_state_dict({k: torch.from_numpy(v) for k, v in network_params("w8").items()})
    os.environ["RU_MX"] = "0"
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert M.warn_mx_range(net) == []                        # the three-product kernels have no window
    finally:
        os.environ.pop("RU_MX", None)


def network_survey(size=32, seed=NETWORK_SEED):
    """the CPU oracle's forward at size^3 with the seeded parameters: per 3x3x3 convolution (name, Cin, Cout, max |x|, RMS x, max |w|, smallest non-zero |w|)"""
    p = O.to_torch(O.make_params(seed, **O.DEFAULT_CFG))
    names = {id(v): k for k, v in p.items()}
    rows, keep = [], O.conv3x3x3

    def probe(x, w, bias=None):
        nz = w.abs()[w != 0]
        rows.append((names[id(w)], int(w.shape[1]), int(w.shape[0]), float(x.abs().max()), float(x.pow(2).mean().sqrt()), float(w.abs().max()), float(nz.min())))
        return keep(x, w, bias)
    O.conv3x3x3 = probe
    try:
        with torch.no_grad():
            O.unet_forward(p, torch.from_numpy(O.make_input(1, size, size, size, seed=seed)), **O.DEFAULT_CFG)
    finally:
        O.conv3x3x3 = keep
    return rows


def test_seeded_network_sits_inside_the_windows():
    """the survey that profiles/mx_range.txt records: every 3x3x3 convolution input and weight of the seeded network at 32^3 against its kernel's window"""
    from brats2019_amd import model as M
    rows = network_survey()
    assert len(rows) == 2 + sum(1 for k, s in O.state_dict_spec(**O.DEFAULT_CFG) if len(s) == 5 and tuple(s[2:]) == (3, 3, 3) and k.startswith(("conv_first", "encoder", "decoder_convs.")) and not k.startswith("decoder_convs.3"))
    for name, cin, cout, mx, rms, mw, sw in rows:
        kernel = M.mx_kernel_of(cin, cout)
        if kernel:
            r = M.MX_RANGE[kernel]
            assert r["x_rms"][0] <= rms <= r["x_rms"][1] and mx <= r["x_max"][1] and r["w_max"][0] <= mw <= r["w_max"][1], (name, mx, rms, mw)


def write_profile(path):
    from brats2019_amd import model as M
    out = ["fp16 + MX-fp8 forward convolutions: error against float64 across operand magnitudes (CPU model of the operand conversions, float64 accumulation;",
           "tests/test_mx_range_host.py, which asserts the windows below).  error = max |y - float64| / RMS(float64); in range: error <= 1.2e-4 and <= 4 x three products + 1e-6.", ""]
    for form, title in (("direct", "conv3_mx_kernel, 1 x 16 -> 16 x 12^3"), ("wz", "conv3_wz32mx_kernel (Winograd F(2,3) in z), 1 x 32 -> 32 x 12^3")):
        pts = sweep(form)
        out += [title, "  %-14s %10s %10s %10s   %10s %12s %12s  %s" % ("point", "max|x|", "rms x", "max|w|", "fp16+MX", "3 products", "1 fp16 prod", "in range")]
        for (axis, k), p in pts.items():
            out.append("  %-14s %10.3g %10.3g %10.3g   %10.2e %12.2e %12.2e  %s" % ("%s %s" % (axis, ("2^%d" % k) if axis in "xw" else k), p["max_x"], p["rms_x"], p["max_w"], p["e"], p["e3"], p["e1"],
                                                                              "yes" if p["in_range"] else "no"))
        w = MX_WINDOW[form]
        out += ["  window (the in-range run less one octave at each end): activations x 2^%d .. 2^%d = RMS %.3g .. %.3g (max|x| %.3g .. %.3g); weights x 2^%d .. 2^%d = max|w| %.3g .. %.3g" % (
            w["x_log2"] + w["x_rms"] + w["x_max"] + w["w_log2"] + w["w_max"]), ""]
    pts = sweep("grad")
    out += ["conv3_mx_kernel<GRAD>, 1 x 16 -> 16 x 12^3: relative L2 (bar 2.5e-4) and max error / max |y| (bar 5e-4)",
            "  %-14s %10s   %10s %10s %12s %12s  %s" % ("point", "max|g|", "rel L2", "max/max", "3 products", "1 bf16 prod", "in range")]
    for (axis, k), p in pts.items():
        out.append("  %-14s %10.3g   %10.2e %10.2e %12.2e %12.2e  %s" % ("%s 2^%d" % (axis, k), p["max_x"], p["e"], p["emax"], p["e3"], p["e1"], "yes" if p["in_range"] else "no"))
    out += ["  window: every tensor scale 2^-60 .. 2^0 (one exponent per voxel: identical errors) and every channel disparity 1 .. 2^12 inside a voxel", ""]
    out += ["seeded network (oracle.make_params(%d), input 1 x 4 x 32^3) on the CPU oracle: every 3x3x3 convolution's input and weight" % NETWORK_SEED,
            "  %-36s %4s %4s %10s %10s %10s %12s  %s" % ("weight", "Cin", "Cout", "max|x|", "rms x", "max|w|", "min|w|>0", "kernel: margin to the window ends (x rms lo / hi, w max lo / hi)")]
    for name, cin, cout, mx, rms, mw, sw in network_survey():
        kernel = M.mx_kernel_of(cin, cout)
        tail = "-"
        if kernel:
            r = M.MX_RANGE[kernel]
            tail = "%s: %.0fx / %.0fx, %.0fx / %.1fx" % (kernel, rms / r["x_rms"][0], r["x_rms"][1] / rms, mw / r["w_max"][0], r["w_max"][1] / mw)
        out.append("  %-36s %4d %4d %10.3g %10.3g %10.3g %12.3g  %s" % (name, cin, cout, mx, rms, mw, sw, tail))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    write_profile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mx_range.txt"))
