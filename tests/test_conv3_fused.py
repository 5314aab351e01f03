"""The fused operands of the 3x3x3 convolution family, one launch at a time: every Conv3Args operand the engine fuses (in_scale / in_shift / in_slope, in_res /
in_sum_out, bias, add, sigmoid, stat_partials, bst_*, products, the data-gradient packing) driven through ru_conv3_l (ops.conv3_fused) against the float64
restatements of tests/test_conv3_fused_host.py, which proves them against the oracle's autograd, proves the exact family exact, and shows that every bar below can
fail.  Every case asserts the route it was written for (conv3_sb_route / conv3_f32c_route, the rule the launchers dispatch on), so a routing change cannot
silently empty a case.  Conv3Args::fin (the tail finalize) is held by tests/test_gn_c16.py on these cases.  Conv3Args::ksplit and the NCDHW exact-f32
conv3_f32_kernel are held by tests/test_ncdhw_convs.py.

Two input families per case (CASES of the host file):
  exact   small integers / powers of two, slope 0.5: stored outputs, in_sum_out and the float64 sum of the partials must EQUAL the float64 reference (a lost or
          doubled 16-voxel row, a transformed halo, statistics before `add`, `>=` for `>` on the ties u == thr all break equality); behind the sigmoid the stored
          output takes the real-valued bar (expf), in_sum_out stays exact
  real    seeded normal values: the convolution term at the bar the project states for the kernel class on plain launches -- three products 6e-5 of the RMS of
          the convolution term; fp16 + MX-fp8 forward 1.2e-4; conv3_mx_kernel<GRAD> relative L2 2.5e-4 and 5e-4 of the largest value; one product 2^-8
          relative L2; exact f32 1e-5 + 1e-5 |ref| -- plus 2^-23 |ref| per element for a fused add / bias; behind the sigmoid that bar / 4 plus 4 * 2^-24.
          Statistics are compared with float64 sums over the kernel's OWN stored output at L * 2^-24 * sum |term|, L = the terms one partial accumulates
          (tiles per workgroup run x voxels of a tile); bst operands keep |u - thr| >= 1e-3 (asserted), no voxel is excluded.
Measured worst error / bar per group, first device run (MI355X; every test prints its value and the running worst of its group, `pytest -s`; no bar moves to
fit a measurement):
  exact family   0 in every class -- three products (one-stage, persistent, 4-channel, Winograd-z), one product, exact f32, fp16 + MX-fp8 forward (direct and
                 Winograd-z) and the gradient-operand kernel all reproduce outputs, in_sum_out and summed partials exactly: no class needed the real-valued bar
  three products 0.62 (Winograd-z 0.62, persistent 0.50, one-stage 0.47, head behind the sigmoid 0.37)     fp16 + MX-fp8 forward 0.67
  gradient operand 0.34          one product 0.61          exact f32 0.21          in_sum_out 0.93
  statistics     0.0054 (one-stage and f32c (2,4) tiles, L = 128 / 512 terms; persistent kernels <= 0.0007)
  exact inputs behind the sigmoid (real-valued bar, expf only) 0.17"""
import numpy as np
import pytest
import torch

from test_conv3_fused_host import (CASES, R, case_terms, conv_excess, exact_excess, in_sum_excess, make_inputs, partial_length, reference, case_slope, sums_excess)

pytestmark = pytest.mark.gpu

MEASURED = {}
_REF = {}


def note(group, what, excess):
    MEASURED[group] = max(MEASURED.get(group, 0.0), excess)
    print("  %-12s %s: error / bar %.3g (worst of the group so far %.3g)" % (group, what, excess, MEASURED[group]))
    return excess


def shared(c):
    """inputs and float64 reference of a case, computed once per module"""
    if c["name"] not in _REF:
        i = make_inputs(c)
        _REF[c["name"]] = (i, reference(c, i))
    return _REF[c["name"]]


def dev(a, c16=False, split=False):
    from brats2019_amd import ops
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if c16:
        t = ops.to_c16(t)
    return ops.to_split_c16(t) if split else t


def host(t, c16):
    from brats2019_amd import ops
    return (ops.from_c16(t) if c16 else t).cpu().numpy()


def launch(c, i, **over):
    from brats2019_amd import ops
    kw = dict(bias=dev(i.get("bias")), in_c16=c["in16"], out_c16=c["out16"], few_channels=c["few"], in_split=c["split"], exact_f32=c["f32"], activations=c["act"],
              gradient=c["grad"], add=dev(i.get("add"), c["out16"]), in_scale=dev(i.get("scale")), in_shift=dev(i.get("shift")), in_slope=case_slope(c),
              in_res=dev(i.get("res"), True), in_sum_out=True if c["sum_out"] else None, sigmoid=c["sigmoid"], products=c["products"],
              bst_y=dev(i.get("bst_y"), c["out16"]), bst_k=dev(i.get("bst_k")), bst_slope=case_slope(c), stats=c["stats"] or c["bst"], weight_mode=c["wm"])
    kw.update(over)
    return ops.conv3_fused(dev(i["x"], c["in16"], c["split"]), dev(i["w"]), **kw)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fused_operands_against_float64(c):
    from brats2019_amd import ops
    i, ref = shared(c)
    res = launch(c, i)
    assert tuple(ops.conv3_route(res.route)) == c["route"], ops.conv3_route(res.route)
    got = host(res.y, c["out16"])
    fused = c["bias"] or c["add"]
    group = ("exact " if c["exact"] else "") + c["klass"]
    if c["exact"] and not c["sigmoid"]:
        assert note(group, c["name"] + " output", exact_excess(got, ref["y"])) == 0.0
    else:
        assert note(c["klass"], c["name"] + " output", conv_excess(got, ref, c["klass"], fused=fused, sigmoid=c["sigmoid"])) <= 1.0
    if c["sum_out"]:
        s = host(res.in_sum, True)
        assert not np.isnan(s).any()                                  # every voxel written (prefilled with NaN)
        if c["exact"]:
            assert note(group, c["name"] + " in_sum_out", exact_excess(s, ref["in_sum"])) == 0.0
        else:
            f8 = lambda a: np.asarray(a, np.float64)
            assert note("in_sum", c["name"], in_sum_excess(s, f8(i["x"]), f8(i["scale"]), f8(i["shift"]), case_slope(c), f8(i["res"]))) <= 1.0
    if c["stats"] or c["bst"]:
        assert res.nblk > 0 and res.partials.shape == (c["n"], c["cout"], res.nblk, 2)
        part = res.partials.double().cpu().numpy()
        assert not np.isnan(part).any()                               # every partial written (prefilled with NaN)
        if c["exact"]:
            assert note(group, c["name"] + " statistics", exact_excess(part.sum(2), case_terms(c, i, ref).sum(2))) == 0.0
        else:
            terms = case_terms(c, i, got.astype(np.float64))         # sums over the kernel's own stored output
            assert note("statistics", c["name"], sums_excess(part.sum(2), terms, partial_length(c, res.nblk))) <= 1.0


def _by_name(name):
    return next(c for c in CASES if c["name"] == name)


def test_add_on_the_forward_mx_shape_falls_back_to_the_persistent_kernel():
    """conv3_mx_kernel's forward form has no residual: the same launch with `add` takes conv3_sb2_kernel<..., ADD>"""
    from brats2019_amd import ops
    c = dict(_by_name("mx_scale_stats_real"), add=True)
    i, _ = shared(_by_name("mx_scale_stats_real"))
    i = dict(i, add=make_inputs(_by_name("sb2_16_add_stats_real"))["add"])
    res = launch(c, i)
    assert tuple(ops.conv3_route(res.route)) == R("sb2", 4, 8, True, True, add=True), ops.conv3_route(res.route)
    ref = reference(c, i)
    assert note("x3", "mx shape with add", conv_excess(host(res.y, True), ref, "x3", fused=True)) <= 1.0


def test_refusals_keep_their_messages():
    c = _by_name("head3_plain_real")
    i, _ = shared(c)
    with pytest.raises(RuntimeError, match="the fused sigmoid exists for NCDHW output only"):
        launch(dict(c, out16=True, cout=16), dict(i, w=make_inputs(_by_name("sb2_16_add_stats_real"))["w"], bias=None), bias=None)
    c = _by_name("dgrad_split_16_b1_a0_real")
    i, _ = shared(c)
    with pytest.raises(RuntimeError, match="fused GroupNorm-backward statistics need the persistent voxel-major kernel, a partial buffer"):
        launch(c, i, stats=False)
    c = _by_name("sb2_16_scale_stats_real")
    i, _ = shared(c)
    with pytest.raises(RuntimeError, match="a residual of the input is staged by the head-form kernel only"):
        launch(c, dict(i, res=i["x"]), stats=False)


def test_bst_on_the_four_channel_kernel_with_a_residual_is_refused():
    """sb2c4<true, true> exists for the head's data gradient, which has no skip gradient to join: bst + add + the 4-channel copy is refused"""
    c = _by_name("head_dgrad_c3_bst_real")
    i, _ = shared(c)
    with pytest.raises(RuntimeError, match="fused GroupNorm-backward statistics need the persistent voxel-major kernel"):
        launch(c, dict(i, add=make_inputs(_by_name("sb2_16_add_stats_real"))["add"]))


@pytest.mark.parametrize("cin, dhw, family", [(32, (16, 32, 128), "wz32mx"), (16, (32, 64, 64), "mx")], ids=["wz32mx_32", "mx_16"])
def test_a_pack_without_its_direct_fragments_refuses_the_direct_route(cin, dhw, family):
    """A pack says what it holds (csrc/conv3_pack_layout.hpp).  Flag bit 7 packs the weight as a training step does: a forward convolution on activations of this
    shape takes the Winograd-z (32 -> 32 at 1 x 16 x 32 x 128: 8 x 4 x 8 x 1 = 256 items, one per CU) / fp16 + MX-fp8 (16 -> 16 at 1 x 32 x 64 x 64: 256 (4,8,16)
    tiles, the smallest persistent-kernel shape) kernel, so the direct fragments are left out -- and the launch computes the bytes of the launch on a full pack.
    The same launch with a residual `add` routes to the direct persistent kernel, whose fragments that pack lacks: refused as an argument error on the host, the
    output untouched."""
    from brats2019_amd import ops
    g = torch.Generator().manual_seed(7 + cin)
    x = torch.randn(1, cin // 16, *dhw, 16, generator=g).cuda()
    w = (torch.randn(cin, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5).cuda()
    add = torch.randn(1, cin // 16, *dhw, 16, generator=g).cuda()
    kw = dict(in_c16=True, out_c16=True, activations=True)
    full, training = ops.conv3_fused(x, w, **kw), ops.conv3_fused(x, w, pack_training=True, **kw)
    assert ops.conv3_route(full.route).family == family and training.route == full.route, (ops.conv3_route(full.route), ops.conv3_route(training.route))
    assert torch.equal(full.y.view(torch.int32), training.y.view(torch.int32))
    with_add = ops.conv3_route(ops.conv3_fused(x, w, add=add, **kw).route)           # the full pack serves the direct route
    assert with_add.family == "sb2" and with_add.add, with_add
    y = torch.full_like(full.y, 12345.0)
    with pytest.raises(RuntimeError, match=r"\(-1\).*does not hold the direct fragments that route sb2"):
        ops.conv3_fused(x, w, add=add, pack_training=True, y=y, **kw)
    torch.cuda.synchronize()
    assert bool((y == 12345.0).all())
