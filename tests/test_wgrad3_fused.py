"""Every instantiation of the transpose-read 3x3x3 weight gradient, one launch at a time: wgrad3_tz_kernel<OT, XS, DS, NP> of csrc/wgrad_tr.hip with every operand of
Wgrad3Args the engine sets (in_scale / in_shift / in_slope on x with its zero halo, split-form dy, the 4-channel copies with the packed-tap stem form, the swapped
head form, one product, the fused GroupNorm-backward apply and the tensor it publishes in the split form or the gradient-operand form, dw_cin / dw_cout, the
deferred reduction) driven through ru_wgrad3_l (ops.wgrad3_fused) against the float64 restatements of tests/test_wgrad3_fused_host.py, which proves them against
the oracle's autograd, proves the exact family exact, derives the bars of the published forms from the formats and shows that every bar below can fail.  Every case
asserts the instantiation it was written for (wgrad3_tr_inst, the value the launcher switches on), so a routing change cannot silently empty a case.

Shapes (CASES of the host file): one (2, 8, 16) item; (N 2, D 5, H 11, W 19), ragged on every axis across a sample boundary; shapes with more columns than
workgroups at every channel count (264 columns on 256 workgroups at 16 channels with D = 3 and D = 7, whose column strides 6 and 10 wrap the 8-slot ring at
different phases; 144 on 128 at 32 channels; 36 on 32 at 64; 18 on 8 at 128), channel pairs with OT = 1, OT = 2, mixed, and odd output-block counts (32 -> 48,
16 -> 48, 32 -> 80), which take OT = 1 since wtr_choose counts the blocks.

Two input families per case:
  exact   small integers / powers of two, slope 0.5: dw must EQUAL the float64 reference and the published tensor the numpy encoder's bytes (a transformed
          halo, a lost plane, a reused ring slot, `>=` for `>` on the ties y*scale + shift == 0, a half's exponent, un-mirrored taps all break equality)
  real    seeded normal values, trained-like scale / shift (a negative and a zero scale, a large shift), |y*scale + shift| >= 1e-3 (asserted; no voxel
          excluded): dw at 2e-5 * max |ref| per element with three products (tests/test_hip_c16.py) and relative L2 2^-8 with one product; the decoded
          published tensor inside the bars the host file derives from the formats plus the float32 roundings of the apply expression
Measured worst error / bar per group, first device run (MI355X; every test prints its value and the running worst of its group, `pytest -s`; no bar moves to fit
a measurement):
  exact family            0 in every group: dw of all 16 instantiations (three products and one) equals the float64 reference, and the published bytes equal
                          the numpy encoders' in the split form and in the gradient-operand form
  real three products     0.40          real one product 0.62
  real published split    0.50          real published gradient operand 0.94 (the value code's half ulp, as the encoder itself on the CPU)
  ru_conv3d_bwd_weight_l at 16 -> 48 (garbage in dw[32:] before wtr_choose counted the blocks) 0.23"""
import numpy as np
import pytest
import torch

from test_wgrad3_fused_host import (CASES, CASE_BY_NAME, TWINS, blocks, canon, case_slope, dw_excess, exact_excess, g16_encode, make_inputs, pub_excess, reference,
                                    split_encode)

pytestmark = pytest.mark.gpu

MEASURED = {}
_REF = {}


def note(group, what, excess):
    MEASURED[group] = max(MEASURED.get(group, 0.0), excess)
    print("  %-22s %s: error / bar %.3g (worst of the group so far %.3g)" % (group, what, excess, MEASURED[group]))
    return excess


def shared(c):
    """inputs and float64 reference of a case, computed once per module (a deferred twin shares its sibling's)"""
    key = TWINS.get(c["name"], c["name"])
    if key not in _REF:
        i = make_inputs(CASE_BY_NAME[key])
        _REF[key] = (i, reference(CASE_BY_NAME[key], i))
    return _REF[key]


def dev(a, c16=False, split=False):
    from brats2019_amd import ops
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if c16:
        t = ops.to_c16(t)
    return ops.to_split_c16(t) if split else t


def launch(c, i, **over):
    from brats2019_amd import ops
    kw = dict(in_scale=dev(i.get("scale")), in_shift=dev(i.get("shift")), in_slope=case_slope(c), dy_split=c["dy_split"], x_c4=c["x_c4"], dy_c4=c["dy_c4"],
              swapped=c["swapped"], products=c["products"], gb_g16=c["gb"] == "g16", dw_cin=c["dw_cin"], dw_cout=c["dw_cout"], gb_y=dev(i.get("gb_y"), True),
              gb_d=dev(i.get("gb_d"), True), gb_scale=dev(i.get("gb_scale")), gb_shift=dev(i.get("gb_shift")), gb_coef=dev(i.get("gb_coef")), gb_slope=case_slope(c),
              gb_out=c["gb"] in ("split", "g16"), deferred=c["deferred"])
    kw.update(over)
    return ops.wgrad3_fused(dev(i["x"], not c["x_c4"]), dev(i.get("dy"), not c["dy_c4"], c["dy_split"]), **kw)


def pub_bytes(t):
    """the published tensor [N, C/16, D, H, W, 16] float32 on the device -> uint8 [N, C/16, D, H, W, 64]"""
    return t.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_instantiation_against_float64(c):
    from brats2019_amd import ops
    i, ref = shared(c)
    res = launch(c, i)
    assert ops.wgrad3_inst(res.inst) == c["inst"], ops.wgrad3_inst(res.inst)
    np3 = c["inst"][3]
    fam = "exact" if c["exact"] else "real"
    group = "%s %s" % (fam, "one product" if np3 == 1 else "three products")
    got = res.dw.cpu().numpy()
    assert not np.isnan(got).any()                                    # every element written (prefilled with NaN)
    if c["exact"]:
        assert note(group, c["name"] + " dw", exact_excess(got.astype(np.float64), ref["dw"])) == 0.0
    else:
        assert note(group, c["name"] + " dw", dw_excess(got, ref["dw"], np3)) <= 1.0
    if c["gb"] in ("split", "g16"):
        g16 = c["gb"] == "g16"
        b = pub_bytes(res.gb_out)
        assert not np.isnan(res.gb_out.cpu().numpy()).any()           # no voxel left unwritten (prefilled with NaN; neither form holds a NaN pattern)
        name = "published " + ("gradient operand" if g16 else "split")
        if c["exact"]:
            want = (g16_encode if g16 else split_encode)(blocks(ref["dy"]).astype(np.float32))
            assert note(fam + " " + name, c["name"], exact_excess(canon(b, g16), canon(want, g16))) == 0.0
        else:
            assert note(fam + " " + name, c["name"], pub_excess(b, blocks(ref["dy"]), blocks(ref["f"]), g16)) <= 1.0
    else:
        assert res.gb_out is None


@pytest.mark.parametrize("name", sorted(TWINS))
def test_deferred_reduction_is_bit_identical(name):
    """the batch kernel behind wgrad_reduce_flush against the immediate wgrad_reduce_kernel on the same partials"""
    c = CASE_BY_NAME[name]
    i, _ = shared(c)
    a, b = launch(c, i), launch(c, i, deferred=False)
    assert a.inst == b.inst
    assert np.array_equal(a.dw.cpu().numpy().view(np.uint32), b.dw.cpu().numpy().view(np.uint32))


def test_refusals_keep_their_messages():
    c = CASE_BY_NAME["rag_gb_split_scale_real"]
    i, _ = shared(c)
    with pytest.raises(RuntimeError, match="the fused GroupNorm-backward apply needs all of its operands"):
        launch(c, i, gb_out=False)
    with pytest.raises(RuntimeError, match="the fused GroupNorm-backward apply needs all of its operands"):
        launch(c, i, gb_coef=None)
    # gb_g16 where another kernel would publish the split form: one product, two output blocks, the stem
    with pytest.raises(RuntimeError, match="the gradient-operand form is published by the one-block, three-product kernel on a voxel-major x only"):
        launch(c, i, gb_g16=True, products=1)
    c32 = CASE_BY_NAME["rag_gb_32_scale_real"]
    with pytest.raises(RuntimeError, match="the gradient-operand form is published by the one-block, three-product kernel on a voxel-major x only"):
        launch(c32, shared(c32)[0], gb_g16=True)
    stem = CASE_BY_NAME["rag_gb_stem_real"]
    with pytest.raises(RuntimeError, match="the gradient-operand form is published by the one-block, three-product kernel on a voxel-major x only"):
        launch(stem, shared(stem)[0], gb_g16=True)
    # 4-channel copies
    p = CASE_BY_NAME["rag_32_32_real"]
    ip, _ = shared(p)
    with pytest.raises(RuntimeError, match="4-channel copies stand for ONE 16-channel block"):
        launch(dict(p, x_c4=True, dw_cin=3), dict(ip, x=ip["x"][:, :3]))
    xc = CASE_BY_NAME["rag_xc4_real"]
    ix, _ = shared(xc)
    with pytest.raises(RuntimeError, match="only one operand can be a 4-channel copy"):
        launch(dict(xc, dy_c4=True, dw_cout=3), dict(ix, dy=ix["dy"][:, :3]))
    # a 4-channel copy beside more than one block of its side where OT = 1: x with Cin = 32, dy with the odd block count Cout = 48
    with pytest.raises(RuntimeError, match="4-channel copies stand for ONE 16-channel block"):
        launch(xc, ix, cin=32)
    dc = CASE_BY_NAME["rag_dyc4_p1_real"]
    with pytest.raises(RuntimeError, match="4-channel copies stand for ONE 16-channel block"):
        launch(dc, shared(dc)[0], cout=48)
    with pytest.raises(RuntimeError, match="a 4-channel copy of x takes no fused transform"):
        launch(xc, dict(ix, scale=np.ones((xc["n"], 16), np.float32), shift=np.zeros((xc["n"], 16), np.float32)))
    i32 = {k: v for k, v in shared(c32)[0].items() if k.startswith("gb_")}
    with pytest.raises(RuntimeError, match="a 4-channel copy stands for ONE 16-channel block"):
        launch(stem, dict(i32, x=shared(stem)[0]["x"]))


def test_odd_output_block_count_through_the_plain_entry():
    """ru_conv3d_bwd_weight_l at Cout = 48 (three 16-channel blocks): wtr_choose gave the last block no workgroup and the reduction summed workspace nobody wrote;
    it now takes OT = 1 and the gradient is the reference's"""
    from brats2019_amd import ops
    c = CASE_BY_NAME["rag_16_48_real"]
    i, ref = shared(c)
    dw = ops.conv3d_bwd_weight_layout(dev(i["x"], True), dev(i["dy"], True), x_c16=True, dy_c16=True).cpu().numpy()
    assert note("real three products", "ru_conv3d_bwd_weight_l 16 -> 48", dw_excess(dw, ref["dw"], 3)) <= 1.0
