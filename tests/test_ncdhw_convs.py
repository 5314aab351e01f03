"""The NCDHW convolution family, one op at a time, against float64: conv3_f32_kernel<TZ, TY, KC, NT> in every instantiation of conv3_launch's dispatch table, forward
and data gradient (ops.conv3d / conv3d_bwd_data); its split-K form (Conv3Args::ksplit, sum_partials_kernel) through ru_conv3d_fwd_splitk (ops.conv3d_splitk);
wgrad3_f32_kernel in both instantiations with the persistent multi-tile walk, both sides of wgrad_reduce_kernel's switches and the bias gradient
(ops.conv3d_bwd_weight); wgrad3_sb_kernel on NCDHW tensors and on the two mixed layouts (ru_conv3d_bwd_weight_l); the three routes of conv1_launch with the
transposes and s2d_kernel / d2s_kernel, and wgrad1_f32_kernel's four NCDHW instantiations with its chunk walk, behind k = 1 and k = 2.  The float64 restatements,
the cases, the inputs and the bars are tests/test_ncdhw_convs_host.py's, which proves them on the CPU.

Every case asserts what it launches -- ops.ncdhw_conv3_inst / ncdhw_wgrad3_inst / ncdhw_conv1_route / ncdhw_wgrad1_inst, host functions of the arguments that
the launchers themselves switch on -- so a change of a choice rule cannot silently empty a case, and every walking case asserts ntile > nbx on the reported values.
Outputs are pre-filled with NaN (an unwritten element shows), every stored tensor is compared in full, and a second call must give the same bits.

wgrad3_sb_kernel<., true, true> has no case: wgrad3_launch hands two voxel-major tensors to the transpose-read kernel (tests/test_wgrad3_fused.py), so that
instantiation is unreachable through the library; the host file asserts the routing.

Two input families per case (host file):
  exact   small integers and halves: every stored tensor must EQUAL the float64 reference (a lost tile of a walk, a wrong half of an OT = 2 pair, a mis-summed
          partial, an un-mirrored tap all break equality); the split-bf16 weight gradient included, its operands being bf16 values
  real    seeded normal values: forward / data-gradient tensors at 1e-5 + 1e-5 |ref| per element, dw and db at 2e-4 max |ref|, three-product split-bf16 dw at
          2e-5 max |ref| per element
Measured worst error / bar per group, first device run (MI355X; every test prints its value and the running worst of its group, `pytest -s`; no bar moves to fit a
measurement).  Nothing was found: every case passed on that first run.
  exact family                 0 in every group: every y, dx, dw and db of all 49 exact cases equals the float64 reference
  real conv3_f32 fwd / dgrad   0.65 (48 -> 8 data gradient, six chunks)      real split-K            0.31 (64 -> 16, factor 2)
  real wgrad3_f32 dw / db      0.0017 (64 -> 64 walk)                        real wgrad3_sb dw       0.25 (16 -> 48, x voxel-major)
  real k = 1 fwd / dgrad       0.15      dw 0.0013                           real k = 2 fwd / dgrad  0.15      dw 0.0011"""
import numpy as np
import pytest
import torch

from test_ncdhw_convs_host import (CASES, CASE_BY_NAME, chosen, exact_excess, ksize, make_inputs, reduction_excess, reference, sb_excess, splitk_slices, tensor_excess,
                                   written_for)

pytestmark = pytest.mark.gpu

MEASURED = {}
_REF = {}


def note(group, what, excess):
    MEASURED[group] = max(MEASURED.get(group, 0.0), excess)
    print("  %-24s %s: error / bar %.3g (worst of the group so far %.3g)" % (group, what, excess, MEASURED[group]))
    return excess


def shared(c):
    """inputs and float64 reference of a case, computed once per module and never written to"""
    if c["name"] not in _REF:
        i = make_inputs(c)
        _REF[c["name"]] = (i, reference(c, i))
    return _REF[c["name"]]


def dev(a, c16=False):
    from brats2019_amd import ops
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.to_c16(t) if c16 else t


def nan_like(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def launch(c, i, precision=None):
    """every tensor the case stores, {name: device tensor}, outputs pre-filled with NaN"""
    from brats2019_amd import ops
    prec = precision or c["precision"]
    n, cin, cout, sp, k = c["n"], c["cin"], c["cout"], c["dhw"], ksize(c)
    so = i["dy"].shape[2:]
    x, w, b, dy = dev(i["x"], c["x_c16"]), dev(i["w"]), dev(i["b"]), dev(i["dy"], c["dy_c16"])
    out = {}
    if c["kind"] == "splitk":
        out["y"] = ops.conv3d_splitk(x, w, ksplit=0, out=nan_like(n, cout, *so))
        return out
    if c["kind"] in ("conv3", "k1", "k2"):
        out["y"] = ops.conv3d(x, w, b, precision=prec, out=nan_like(n, cout, *so))
        out["dx"] = ops.conv3d_bwd_data(dy, w, sp, precision=prec, out=nan_like(n, cin, *sp))
    if c["kind"] in ("k1", "k2"):
        out["dw"] = ops.conv3d_bwd_weight(x, dy, k, out=nan_like(cout, cin, k, k, k))
    elif c["kind"] == "wgrad3":
        r = ops.conv3d_bwd_weight(x, dy, 3, with_bias=bool(c.get("db")), precision=prec, out=nan_like(cout, cin, 3, 3, 3), out_db=nan_like(cout) if c.get("db") else None)
        out["dw"], out["db"] = r if c.get("db") else (r, None)
    elif c["kind"] == "wsb":
        if c["x_c16"] or c["dy_c16"]:
            out["dw"] = ops.conv3d_bwd_weight_layout(x, dy, x_c16=c["x_c16"], dy_c16=c["dy_c16"], out=nan_like(cout, cin, 3, 3, 3))
        else:
            out["dw"] = ops.conv3d_bwd_weight(x, dy, 3, precision="bf16x3", out=nan_like(cout, cin, 3, 3, 3))
    return {k_: v for k_, v in out.items() if v is not None}


GROUPS = {"conv3": "conv3_f32", "splitk": "split-K", "wgrad3": "wgrad3_f32", "wsb": "wgrad3_sb", "k1": "k = 1", "k2": "k = 2"}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_switch_against_float64(c):
    from brats2019_amd import ops
    assert chosen(c, ops) == written_for(c), chosen(c, ops)
    if c["walk"]:                                                         # more tiles (chunks) than workgroups, on the reported values themselves
        n, cin, cout, (d, h, w) = c["n"], c["cin"], c["cout"], c["dhw"]
        if c["kind"] == "k1":
            r = ops.ncdhw_wgrad1_inst(n, cin, cout, d * h * w)
            assert n * r.nchunk > r.nbx, r
        else:
            r = ops.ncdhw_wgrad3_inst(n, cin, cout, d, h, w, precision=c["precision"], x_c16=c["x_c16"], dy_c16=c["dy_c16"])
            assert r.ntile > r.nbx, r
    i, ref = shared(c)
    got, again = launch(c, i), launch(c, i)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    fam = "exact" if c["exact"] else "real"
    for name in sorted(ref):
        g = got[name].cpu().numpy()
        assert not np.isnan(g).any(), name                                # every element written (prefilled with NaN)
        assert np.array_equal(bits(got[name]), bits(again[name])), name   # the second call gives the same bits
        group = "%s %s %s" % (fam, GROUPS[c["kind"]], "fwd/dgrad" if name in ("y", "dx") else "dw/db")
        if c["exact"]:
            assert note(group, "%s %s" % (c["name"], name), exact_excess(g.astype(np.float64), ref[name])) == 0.0
        else:
            excess = tensor_excess if name in ("y", "dx") else (sb_excess if c["kind"] == "wsb" else reduction_excess)
            assert note(group, "%s %s" % (c["name"], name), excess(g, ref[name])) <= 1.0


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["kind"] == "splitk"])
def test_split_k_is_the_slice_order_sum_of_the_per_slice_launches(name):
    """sum_partials_kernel adds the partial tensors in slice order: the entry's bits are those of float32 additions, in that order, of the plain launches over each
    slice's channels (the same instantiation: the choice does not look at Cin beyond its padding), with the factor chosen and with the same factor given"""
    from brats2019_amd import ops
    c = CASE_BY_NAME[name]
    i, _ = shared(c)
    n, cin, cout, (d, h, w) = c["n"], c["cin"], c["cout"], c["dhw"]
    x, wt = dev(i["x"]), dev(i["w"])
    auto = ops.conv3d_splitk(x, wt, ksplit=0, out=nan_like(n, cout, d, h, w))
    given = ops.conv3d_splitk(x, wt, ksplit=c["ksplit"], out=nan_like(n, cout, d, h, w))
    assert np.array_equal(bits(auto), bits(given))
    acc = None
    for a, b in splitk_slices(cin, c["ksplit"]):
        assert tuple(ops.ncdhw_conv3_inst(n, b - a, cout, d, h, w)[:4]) == c["fwd"]
        part = ops.conv3d(x[:, a:b].contiguous(), wt[:, a:b].contiguous())
        acc = part if acc is None else acc + part
    assert np.array_equal(bits(auto), bits(acc))
    if c["ksplit"] == 1:                                                  # the entry degenerates to the plain launch, bias and all
        bias = dev(np.linspace(-1.0, 1.0, cout).astype(np.float32))
        assert np.array_equal(bits(ops.conv3d_splitk(x, wt, bias, ksplit=0)), bits(ops.conv3d(x, wt, bias)))


def test_split_k_refusals_keep_their_messages():
    from brats2019_amd import ops
    c = CASE_BY_NAME["sk_48_16_real"]
    i, _ = shared(c)
    x, w = dev(i["x"]), dev(i["w"])
    with pytest.raises(RuntimeError, match="split-K divides the input-channel chunks and has a plain epilogue"):
        ops.conv3d_splitk(x, w, ksplit=4)                                 # six chunks
    with pytest.raises(RuntimeError, match="split-K divides the input-channel chunks and has a plain epilogue"):
        ops.conv3d_splitk(x, w, dev(np.ones(16, np.float32)), ksplit=2)   # a bias beside a split


@pytest.mark.parametrize("name", ["c3_3_16_w18_real", "c3_8_16_real", "c3_16_3_bias_real", "w3_16_16_walk_real"])
def test_ragged_w_under_bf16x3_is_the_f32_kernel_bit_for_bit(name):
    """W % 4 != 0: precision="bf16x3" falls back to the exact-f32 kernels (conv3_effective_mode; wgrad3_launch), same instantiation, same bits"""
    c = CASE_BY_NAME[name]
    assert c["dhw"][2] % 4 != 0
    i, _ = shared(c)
    a, b = launch(c, i, precision="f32"), launch(c, i, precision="bf16x3")
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
