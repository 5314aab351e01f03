"""The fp16 + MX-fp8 forward 3x3x3 kernels (conv3_mx_kernel, conv3_wz32mx_kernel) and the gradient-operand kernel (conv3_mx_kernel<GRAD>) against the CPU model
of tests/test_mx_range_host.py, across operand magnitudes: one launch at a time through ru_conv3_l (ops.conv3_fused), every case asserting the route it was written
for.  The host file proves the model's formats against torch's conversions and hand-written tables, derives the in-range windows against float64, proves the tie
family exact and shows every mutant of the model failing; here the KERNELS are held to the model.

Shapes (the smallest that take each kernel): conv3_mx 1 x 16 -> 16 at 32 x 64 x 64; conv3_wz32mx 1 x 32 -> 32 at 16 x 32 x 128 (every point), 64 -> 64 at
16 x 32 x 64 and 128 -> 128 at 16 x 32 x 32 (256 work items; three points each); GRAD 2 x 16 -> 16 at 30 x 30 x 60 (the mxg_* shape of tests/test_conv3_fused.py,
weight packed as a data gradient).
Operand points: both ends and the middle of each window (activations and weights), the fp16-subnormal zone (activations x 2^-20), the e4m3-underflow zone
(x 2^-9), saturation (activations x 2^9, weights x 2^6), per-channel gains exp(1.5 N), exp(3 N) on x compensated in w, heavy-tailed weights, and the three groups of
the exact tie family.  GRAD: tensor scale 2^0, 2^-30, 2^-60, channel disparity 2^12 inside every voxel, the tie family.
Per point:
  kernel against the model   bit for bit on the tie family (after the host file's integer-arithmetic proof on THIS shape's tensors: every partial sum is a float32);
                             elsewhere |y - model| <= T * 2^-24 * sum |terms| per output, float32 accumulation alone: sum |terms| is the model run on the
                             operands' magnitudes, T the terms one output accumulates, counted from the kernels as written -- conv3_mx: 14 fp16 MFMAs x K 32 + 7
                             scaled MFMAs x K 128 = 1344; conv3_wz32mx: three of the four M planes x (Cin / 16 chunks x (9 x 16 + 5 x 64)) + the 2 additions of the
                             output transform
  kernel against float64     inside the window the bars of tests/test_hip_c16.py (1.2e-4 of the output RMS and 4 x the three-product kernel's error + 1e-6;
                             GRAD 2.5e-4 relative L2, 5e-4 of the largest value); outside: finite and no worse than the model's ONE product of the main-term
                             format plus the model's three-product error
  bookkeeping                outputs pre-filled with NaN and fully written, every launch repeated once with identical bytes, no voxel excluded
Whether a point is inside comes from the host file's window constants in their absolute form (H.in_window: RMS and max of x, max of w -- float64 measurements),
never from the kernel.  The float64 reference and the model's convolutions run on the device as float64 matmuls per tap (conv_taps; the host file proves that form equal to conv3d), cached per module.

One network-level test: UNet at 1 x 4 x 32 x 64 x 256 (level 0 takes conv3_mx, level 1 conv3_wz32mx: both routes asserted at the op level on those shapes, and RU_MX=0
must change the bytes), default against RU_MX=0, on the host file's parameter sets: inside the windows (model.mx_range_report) the 2e-4 bar on the probabilities
of test_forward_convolution_kernels_agree_through_the_network; outside finiteness, the value printed.

Measured worst error / bar per group, first device run (MI355X; `pytest -s` prints every value and the running worst; no bar moves to fit a measurement):
  kernel against the model   exact tie family: 0 outputs of 2 097 152 (GRAD: 1 728 000) differ, in all nine cases -- conv3_mx and conv3_wz32mx on the tie, e4m3-subnormal and
                             saturation groups, 64 and 128 channels, GRAD; elsewhere conv3_mx 0.0065, conv3_wz32mx 0.0011, GRAD 0.014 of the accumulation bar.  (The
                             first run showed 0.4 and failed the family's proof on the device: the MODEL's grid spacing went through torch.ldexp, a float32 pow
                             that is inexact there -- quantise now builds it from the exponent bits, and a test holds the device's conversions to the host's.)
                             Nothing found in the kernels: they convert as modelled, ties, subnormals, saturation and section / scale pairing included.
  kernel against float64     inside the windows conv3_mx 0.63 (weights at the upper end), conv3_wz32mx 0.73 (weights at the lower end), GRAD 0.36; outside, against the
                             envelope: 1.00 in the fp16-subnormal zone, where the scheme IS one fp16 product (0.129 / 0.098 of the output RMS, model and kernel alike),
                             otherwise at most 0.60 (conv3_mx, saturating weights) / 0.54 (conv3_wz32mx)
  network                    seeded 0.40 (max |dp| 8.0e-5); outside the windows (finiteness only): GroupNorm parameters x 30 1.9e-3 .. 2.1e-3, x 0.01 1.9e-6 .. 2.4e-6,
                             one block's weights x 8 7.8e-5"""
import os

import pytest
import torch

import test_mx_range_host as H
from oracle import resunet_oracle as O
from test_conv3_fused_host import dgrad_weight

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
MEASURED = {}
_CACHE = {}

# name: (form, family, n, cin, cout, (d, h, w))
SHAPES = {"mx16": ("direct", "mx", 1, 16, 16, (32, 64, 64)), "wz32": ("wz", "wz32mx", 1, 32, 32, (16, 32, 128)), "wz64": ("wz", "wz32mx", 1, 64, 64, (16, 32, 64)),
          "wz128": ("wz", "wz32mx", 1, 128, 128, (16, 32, 32)), "grad": ("grad", "mx", 2, 16, 16, (30, 30, 60))}
FULL_POINTS = ["x_lo", "x_mid", "x_hi", "w_lo", "w_hi", "x_f16_subnormal", "x_e4m3_underflow", "x_saturation", "w_saturation", "gain_1.5", "gain_3", "heavy",
               "tie_tie", "tie_sub", "tie_sat"]
POINTS = {"mx16": FULL_POINTS, "wz32": FULL_POINTS, "wz64": ["x_mid", "x_saturation", "tie_tie"], "wz128": ["x_mid", "x_e4m3_underflow", "tie_sat"],
          "grad": ["g_2^0", "g_2^-30", "g_2^-60", "g_disparity_2^12", "tie_tie"]}
CASES = [(s, p) for s in SHAPES for p in POINTS[s]]


def terms_per_output(shape):
    form, _, _, cin, _, _ = SHAPES[shape]
    return 3 * (cin // 16) * (9 * 16 + 5 * 64) + 2 if form == "wz" else 14 * 32 + 7 * 128


def note(group, what, excess):
    MEASURED[group] = max(MEASURED.get(group, 0.0), excess)
    print("  %-28s %s: error / bar %.3g (worst of the group so far %.3g)" % (group, what, excess, MEASURED[group]))
    return excess


def operands(shape, point):
    """float32 device tensors (x, w) of a point and whether the host file's windows put it inside (None: the tie family)"""
    form, _, n, cin, cout, sp = SHAPES[shape]
    if point.startswith("tie_"):
        x, w = H.tie_family(form, point[4:], n, cin, cout, sp)
        return x.cuda(), w.cuda(), None
    if form == "grad":
        g, w = H.draw_grad(41, n, cin, *sp), H.draw_w(42, cout, cin)
        if point == "g_disparity_2^12":
            return H.disparity(g, 12).cuda(), w.cuda(), True
        k = int(point[4:])
        assert H.GRAD_WINDOW["scale_log2"][0] <= k <= H.GRAD_WINDOW["scale_log2"][1]
        return (g * 2.0 ** k).float().cuda(), w.cuda(), True
    win = H.MX_WINDOW[form]
    x, w = H.draw_x(21, n, cin, *sp), H.draw_w(22, cout, cin)
    rms, mx, mw = float(x.double().pow(2).mean().sqrt()), float(x.abs().max()), float(w.abs().max())
    # the ends of the window in its absolute form, a part in a thousand inside: these tensors are larger than the sweep's, so their maxima sit further out
    xk = {"x_lo": 1.001 * win["x_rms"][0] / rms, "x_mid": 1.0, "x_hi": 0.999 * min(win["x_rms"][1] / rms, win["x_max"][1] / mx), "x_f16_subnormal": 2.0 ** -20,
          "x_e4m3_underflow": 2.0 ** -9, "x_saturation": 2.0 ** 9}
    wk = {"w_lo": 1.001 * win["w_max"][0] / mw, "w_hi": 0.999 * win["w_max"][1] / mw, "w_saturation": 2.0 ** 6}
    if point in xk:
        x = (x * xk[point]).float()
    elif point in wk:
        w = (w * wk[point]).float()
    elif point.startswith("gain_"):
        x, w = H.compensated(x, w, H.gains(23, cin, float(point[5:])))
    else:
        assert point == "heavy"
        w = H.heavy_tailed(w, 24)
    inside = H.in_window(form, x, w)
    assert inside == (point in ("x_lo", "x_mid", "x_hi", "w_lo", "w_hi")), (point, inside)      # the window's absolute form sorts the points as their names say
    return x.cuda(), w.cuda(), inside


def shared(shape, point):
    """operands, float64 reference, the model's result and its sum of magnitudes, once per module"""
    key = (shape, point)
    if key not in _CACHE:
        form = SHAPES[shape][0]
        x, w, inside = operands(shape, point)
        wc = torch.from_numpy(dgrad_weight(w.cpu().numpy())).cuda() if form == "grad" else w      # GRAD: w is the forward weight, packed as its data gradient
        c = dict(x=x, w=w, inside=inside, ref=H.conv_taps(x.double(), wc.double()), emu=H.EMULATE[form](x, wc), tot=H.EMULATE[form](x, wc, absolute=True))
        if inside is None:
            _, c["unit"], c["ratio"] = H.exactness(form, x, wc)
        elif not inside:
            c["e1"], c["e3"] = H.one_product(x, wc, "f16", form), H.three_products(x, wc)
        _CACHE[key] = c
    return _CACHE[key]


def launch(shape, x, w, three_products=False):
    """-> (NCDHW output, route): output pre-filled with NaN, the launch repeated once.  three_products: the kernel the existing bars compare with
    (tests/test_hip_c16.py: the launch without the activation flag, with RU_WZ=0 at 32+ channels -- the direct three-product kernel)"""
    from brats2019_amd import ops
    form = SHAPES[shape][0]
    kw = dict(in_c16=True, out_c16=True)
    if not three_products:
        kw.update(gradient=True, weight_mode=1) if form == "grad" else kw.update(activations=True)
    elif form == "grad":
        kw.update(weight_mode=1)
    x16 = ops.to_c16(x)
    outs = []
    if three_products and form == "wz":
        os.environ["RU_WZ"] = "0"
    try:
        for _ in range(1 if three_products else 2):
            y = torch.full((x.shape[0], w.shape[1 if form == "grad" else 0] // 16) + tuple(x.shape[2:]) + (16,), float("nan"), dtype=torch.float32, device=x.device)
            res = ops.conv3_fused(x16, w, y=y, **kw)
            outs.append(res.y)
    finally:
        os.environ.pop("RU_WZ", None)
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches on the same operands differ"
    return ops.from_c16(outs[0]), ops.conv3_route(res.route)


def test_the_model_converts_on_the_device_as_on_the_host():
    """the model's conversions run on the device here: same values as on the CPU, where the host file checks them against torch and the hand-written tables"""
    v = torch.cat([H._log_uniform(1, 200000, -30, 17), torch.tensor([a for a, _ in H.F16_TABLE + H.E4M3_TABLE], dtype=torch.float32)])
    for fmt in ("f16", "e4m3", "bf16"):
        assert torch.equal(H.quantise(v.cuda(), fmt).cpu(), H.quantise(v, fmt)), fmt
    x, w = H.tie_family("wz", "tie", 1, 32, 32, (4, 8, 16))
    for a, b in zip(H.operand_classes("wz", x.cuda(), w.cuda()), H.operand_classes("wz", x, w)):
        assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1])


@pytest.mark.parametrize("shape,point", CASES, ids=["%s-%s" % c for c in CASES])
def test_kernel_against_the_model_and_float64(shape, point):
    form, family, n, cin, cout, sp = SHAPES[shape]
    c = shared(shape, point)
    y, route = launch(shape, c["x"], c["w"])
    assert route.family == family and route.grad == (form == "grad") and route.in16 and route.out16, route
    assert not bool(torch.isnan(y).any()), "a voxel was not written"
    assert bool(torch.isfinite(y).all())
    y = y.double()
    ref, emu, tot = c["ref"], c["emu"], c["tot"]
    group = "%s %s" % ("conv3_mx<GRAD>" if form == "grad" else "conv3_" + family, "")
    if c["inside"] is None:                                           # exact family: every partial sum is a float32 (proved on these tensors), so is the result
        assert c["ratio"] < 1.0, c["ratio"]
        wrong = int((y != emu).sum())
        print("  %s %s: unit %s, sum |terms| / (2^24 unit) %.3g, %d of %d outputs differ from the model" % (shape, point, c["unit"], c["ratio"], wrong, y.numel()))
        assert wrong == 0, "max |kernel - model| %g" % float((y - emu).abs().max())
        return
    acc = float(((y - emu).abs() / (terms_per_output(shape) * U24 * tot + 1e-300)).max())
    assert note(group + "against the model", "%s %s" % (shape, point), acc) <= 1.0
    if form == "grad":
        l2, mx = H.err_grad(y, ref)
        if c["inside"]:
            assert note(group + "against float64", "%s %s" % (shape, point), max(l2 / H.BAR_G_L2, mx / H.BAR_G_MAX)) <= 1.0
        return
    e = H.err_rms(y, ref)
    if c["inside"]:
        y3, r3 = launch(shape, c["x"], c["w"], three_products=True)
        assert r3.family in ("sb2", "sb"), r3
        e3 = H.err_rms(y3.double(), ref)
        assert note(group + "against float64", "%s %s (%.2e; three-product kernel %.2e)" % (shape, point, e, e3), max(e / H.BAR_RMS, e / (H.BAR_X3 * e3 + H.BAR_ABS))) <= 1.0
    else:
        e1, e3 = H.err_rms(c["e1"], ref), H.err_rms(c["e3"], ref)
        assert note(group + "outside: envelope", "%s %s (%.2e; one fp16 product %.2e)" % (shape, point, e, e1), e / (e1 + e3)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the network
NET_SHAPE = (1, 4, 32, 64, 256)


def test_network_shape_takes_both_kernels():
    """level 0 of NET_SHAPE is 1 x 16 x 32 x 64 x 256, level 1 is 1 x 32 x 16 x 32 x 128"""
    from brats2019_amd import ops
    for cin, sp, family in ((16, (32, 64, 256), "mx"), (32, (16, 32, 128), "wz32mx")):
        x = torch.zeros(1, cin // 16, *sp, 16, device="cuda")
        w = torch.zeros(cin, cin, 3, 3, 3, device="cuda")
        assert ops.conv3_route(ops.conv3_fused(x, w, in_c16=True, out_c16=True, activations=True).route).family == family


def _forward(params, x):
    from brats2019_amd import model as M
    net = M.UNet(**O.DEFAULT_CFG)
    net.set_precision("bf16x3")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net.cuda().eval()
    with torch.no_grad():
        return net([x])[0].clone()


@pytest.mark.parametrize("name", H.NETWORK_SETS)
def test_network_default_against_three_products(name):
    params = H.network_params(name)
    x = torch.from_numpy(O.make_input(*((NET_SHAPE[0],) + NET_SHAPE[2:]), seed=H.NETWORK_SEED)).cuda()
    p_mx = _forward(params, x)
    os.environ["RU_MX"] = "0"
    try:
        p_x3 = _forward(params, x)
    finally:
        os.environ.pop("RU_MX", None)
    assert bool(torch.isfinite(p_mx).all()) and bool(torch.isfinite(p_x3).all())
    assert not torch.equal(p_mx, p_x3), "RU_MX=0 did not change the bytes: the default forward took no fp16 + MX-fp8 kernel"
    dp = float((p_mx - p_x3).abs().max())
    inside = H.NETWORK_INSIDE[name]
    print("  network %-12s %s the windows: max |dp| against RU_MX=0 %.2e" % (name, "inside" if inside else "OUTSIDE", dp))
    if inside:
        assert note("network inside the windows", name, dp / 2e-4) <= 1.0
