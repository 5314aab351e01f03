"""The trilinear x2 pair and the head of the backward pass on the device, one launch at a time through the op-level C-ABI, against the float64 restatements
of tests/test_up2_head_host.py -- its cases, its inputs, its bars (derived there from the roundings of each kernel as written), its exact families.

Trilinear (ops.upsample2x_c16 / upsample2x_bwd_c16 -> up2_fwd16_kernel / up2_bwd16_kernel; ops.upsample2x / upsample2x_bwd -> the NCDHW kernels, vector form for even W):
every case runs forward and adjoint on the real family (bars) and on the exact family (bit for bit, and the adjoint identity sum(up(x) dy) == sum(x upT(dy)) exactly in
float64).  Voxel-major cases: every axis clamped at both ends (1x1x1), N > 1 with CB > 1, D on both sides of the adjoint's z-march chunk of 8 (7: a short chunk; 8: one
chunk with k1 == D; 9: a second chunk of one plane; 16: a seam between two full chunks; 17: three chunks), the levels of the ragged 24 x 40 x 48 step, and one forward-only
exact case at 80^3 -- the smallest cube whose grid-stride loop wraps (81 * 81 * 160 * 4 threads > 16384 * 256), 262 MB of output, so the nontemporal stores as well --
with its float64 reference taken on the device two channels at a time.  NOT covered: the wrap of the adjoint's grid-stride loop, which needs a gradient of 0.5 GB or more
in a shape no network here produces.

Head (ops.head_grad -> ru_head_grad_l): the 4-channel pass with dp given and with the criterion formed on the way, and the generic route (flat sigmoid backward, then the
bias gradient), at one quad, exactly one 16384-voxel chunk, a second chunk of one quad, a last chunk one quad short, and 1, 2, 3, 4 channels.  Exact family bit for bit;
real family within the bars; the padding lanes of d4 are +0.0 by bit pattern; every output finite at the planted p in {0, 1}; the generic route's dlog and the 4-channel
pass's d4 bitwise equal; the criterion form bitwise equal to ru_criterion_grad followed by the dp form (the kernel's own claim); the refusals keep their messages.
Outputs are allocated filled with NaN; workspaces come from GuardedWorkspace and every head test ends with intact().  Each test prints its worst error / bar.

Measured on the MI355X, worst error / bar over the cases of a group (every exact-family comparison: 0, bit for bit): voxel-major forward 0.46, adjoint 0.19; NCDHW forward
0.46, adjoint 0.12; d on the 4-channel pass 0.93 (three roundings, all of them met), with the criterion 0.42, generic 0.85; db 0.008 / 0.026 / 0.004.  The criterion form
against the two-launch form: 0 words of 393 312 differ; before both kernels took the expression from crit_grad_value (csrc/pw_helpers.hpp) 2938 (weights 1/2, 1/2) and
3108 (1, 0) differed in the last bit, and 0 for (0, 1) -- the two kernels had contracted `kg*g + kp*p` into different fused multiply-adds."""
import numpy as np
import pytest
import torch

import test_up2_head_host as H
from op_cases import GuardedWorkspace
from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu

FAMILIES = ("real", "exact")


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def to_c16(x):
    """[N, C, D, H, W] -> voxel-major [N, C/16, D, H, W, 16] (torch indexing, not the library's converter)"""
    n, c, d, h, w = x.shape
    return x.reshape(n, c // 16, 16, d, h, w).permute(0, 1, 3, 4, 5, 2).contiguous()


def from_c16(y):
    n, cb, d, h, w, _ = y.shape
    return y.permute(0, 1, 5, 2, 3, 4).reshape(n, cb * 16, d, h, w)


def bits(t):
    return t.contiguous().view(torch.int32)


def report(what, ex):
    print("  %-60s worst error / bar %.3g" % (what, ex))
    return ex


# ---------------------------------------------------------------------------------------------------------------- trilinear
def _check_pair(case, family, fwd, bwd, r_f, r_b, slopes):
    x, dy = H.up_inputs(case, family)
    x64, dy64 = x.double(), dy.double()
    worst, y1 = 0.0, None
    for slope in slopes:
        y = fwd(x.cuda(), slope).cpu()
        ref = H.ref_up2(x64, slope)
        if family == "exact":
            assert H.same_bits(y, ref), (case, slope)
        ex = report("forward %s %s slope %g" % (H.case_id(case), family, slope), H.excess(y, ref, H.up_bar(x64, r_f)))
        assert ex <= 1.0, (case, slope, ex)
        worst = max(worst, ex)
        if slope == 1.0:
            y1 = y
    dx = bwd(dy.cuda()).cpu()
    ref = H.ref_up2_bwd(dy64)
    if family == "exact":
        assert H.same_bits(dx, ref), case
        assert float((y1.double() * dy64).sum()) == float((x64 * dx.double()).sum())          # the adjoint identity, exact in float64
    ex = report("adjoint %s %s" % (H.case_id(case), family), H.excess(dx, ref, H.up_bwd_bar(dy64, r_b)))
    assert ex <= 1.0, (case, ex)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", H.C16_CASES, ids=H.case_id)
def test_voxel_major_trilinear_pair(case, family):
    from brats2019_amd import ops
    n, c, d, h, w = case
    fwd = lambda x, slope: from_c16(ops.upsample2x_c16(to_c16(x), out_slope=slope, out=nan(n, c // 16, 2 * d, 2 * h, 2 * w, 16)))
    bwd = lambda dy: from_c16(ops.upsample2x_bwd_c16(to_c16(dy), out=nan(n, c // 16, d, h, w, 16)))
    _check_pair(case, family, fwd, bwd, H.R_UP_FWD16, H.R_UP_BWD, H.SLOPES[family])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", H.NCDHW_CASES, ids=H.case_id)
def test_ncdhw_trilinear_pair(case, family):
    from brats2019_amd import ops
    n, c, d, h, w = case
    fwd = lambda x, slope: ops.upsample2x(x, out=nan(n, c, 2 * d, 2 * h, 2 * w))
    bwd = lambda dy: ops.upsample2x_bwd(dy, out=nan(n, c, d, h, w))
    _check_pair(case, family, fwd, bwd, H.R_UP_FWD, H.R_UP_BWD, (1.0,))


def test_voxel_major_forward_where_the_grid_stride_loop_wraps():
    """80^3 coarse, exact family, slope 1/2: bit for bit against the float64 reference formed on the device, two channels at a time"""
    from brats2019_amd import ops
    n, c, d, h, w = H.WRAP_CASE
    g = torch.Generator().manual_seed(H._seed(H.WRAP_CASE, 2))
    x = torch.randint(-8, 9, (n, c, d, h, w), generator=g).float().cuda()
    y = ops.upsample2x_c16(to_c16(x), out_slope=0.5, out=nan(n, c // 16, 2 * d, 2 * h, 2 * w, 16))
    bad = []
    for c0 in range(0, c, 2):
        ref = H.ref_up2(x[:, c0:c0 + 2].double(), 0.5)
        got = y[:, 0, :, :, :, c0:c0 + 2].permute(0, 4, 1, 2, 3)
        if not torch.equal(got.double(), ref):
            bad.append(c0)
        del ref, got
    report("forward %s exact slope 0.5 (channel pairs that differ: %s)" % (H.case_id(H.WRAP_CASE), bad), 0.0 if not bad else float("inf"))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- head
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guard(monkeypatch, size_of=None):
    from brats2019_amd import _lib as L
    ws = GuardedWorkspace(size_of) if size_of else GuardedWorkspace()
    monkeypatch.setattr(L, "workspace", ws)
    return ws


def _check_head(tag, case, family, got, p, dp64, terms, r_d, r_sum):
    """got = (d4 or None, db, dlog or None) of the device against ref_head(p, dp64) at the bars of (terms, r_d, r_sum); -> the d4 / dlog tensors for bit comparisons"""
    n, c, v = case
    d, db, d4 = H.ref_head(p, dp64)
    bar_d, bar_db = H.head_bars(p, terms, r_d, r_sum)
    g4, gdb, gdlog = (None if t is None else t.cpu() for t in got)
    assert all(bool(torch.isfinite(t).all()) for t in (g4, gdb, gdlog) if t is not None), (tag, case)
    worst = 0.0
    if g4 is not None:
        assert g4.shape == (n, v, 4)
        assert not bool(bits(g4[:, :, c:]).any()), "the padding lanes are not +0.0"
        if family == "exact":
            assert H.same_bits(g4, d4), (tag, case)
        worst = max(worst, H.excess(g4[:, :, :c], d4[:, :, :c], bar_d.transpose(0, 2, 1)))
    if gdlog is not None:
        assert gdlog.shape == (n, c, v)
        if family == "exact":
            assert H.same_bits(gdlog, d), (tag, case)
        worst = max(worst, H.excess(gdlog, d, bar_d))
    if family == "exact":
        assert H.same_bits(gdb, db), (tag, case, gdb, db)
    ex_d, ex_db = report("%s d %s %s" % (tag, H.case_id(case), family), worst), report("%s db %s %s" % (tag, H.case_id(case), family), H.excess(gdb, db, bar_db))
    assert ex_d <= 1.0 and ex_db <= 1.0, (tag, case, ex_d, ex_db)
    return g4, gdlog


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", H.C4_CASES, ids=H.case_id)
def test_head_four_channel_pass(case, family, monkeypatch):
    from brats2019_amd import ops
    ws = _guard(monkeypatch)
    inp = H.head_inputs(case, family)
    p, dp = dev(inp["p"]), dev(inp["dp"])
    g4, gdlog = _check_head("c4", case, family, ops.head_grad(p, dp, with_dlog=True), inp["p"], inp["dp"].astype(np.float64), inp["dp"][None], H.R_D, H.R_SUM_C4)
    # the generic route on the same inputs: its dlog, the 4-channel pass's own dlog and d4[..., :C] are the same bits
    _, gdb, generic = ops.head_grad(p, dp, generic=True)
    c = case[1]
    assert torch.equal(bits(generic.cpu()), bits(gdlog)) and torch.equal(bits(generic.cpu().transpose(1, 2)), bits(g4[:, :, :c]))
    assert ws.intact()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", H.C4_CASES, ids=H.case_id)
def test_head_four_channel_pass_with_the_criterion(case, family, monkeypatch):
    from brats2019_amd import ops
    ws = _guard(monkeypatch)
    inp = H.head_inputs(case, family)
    c = case[1]
    dp64, terms = H.head_crit_reference(inp)
    if family == "real":                                          # the oracle's closed form itself (default weights); terms only carries the bar
        dp64 = O.np_criterion_grad(inp["p"], inp["g"], inp["sums"][:c], inp["sums"][c:2 * c], inp["count"], H.BGW)
    got = ops.head_grad(dev(inp["p"]), target=dev(inp["g"]), sums=dev(inp["sums"]), count=inp["count"], **inp["crit"])
    _check_head("crit", case, family, got, inp["p"], dp64, terms, H.R_D_CRIT, H.R_SUM_C4)
    assert ws.intact()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", H.GENERIC_CASES, ids=H.case_id)
def test_head_generic_route(case, family, monkeypatch):
    from brats2019_amd import ops
    ws = _guard(monkeypatch)
    inp = H.head_inputs(case, family)
    got = ops.head_grad(dev(inp["p"]), dev(inp["dp"]), generic=True)
    assert got[0] is None
    _check_head("generic", case, family, got, inp["p"], inp["dp"].astype(np.float64), inp["dp"][None], H.R_D, H.R_SUM_GEN)
    assert ws.intact()


@pytest.mark.parametrize("weights", [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)], ids=lambda w: "w%g_%g" % w)
@pytest.mark.parametrize("bgw", [1e-2, 1.0])
def test_criterion_form_is_criterion_grad_then_the_dp_form_bit_for_bit(bgw, weights, monkeypatch):
    """head_grad_c4_kernel<true> claims crit_grad_kernel's float operations in the same order: the same bits in d4 and db, with a global count that is not the shard's"""
    from brats2019_amd import ops
    ws = _guard(monkeypatch)
    inp = H.head_inputs((2, 3, 16388), "real")
    p, g = dev(inp["p"]), dev(inp["g"])
    assert inp["count"] != p.numel()
    sums = ops.criterion_sums(p, g, bg_weight=bgw)
    kw = dict(w_dice=weights[0], w_bce=weights[1], bg_weight=bgw, priority=1.0)
    fused = ops.head_grad(p, target=g, sums=sums, count=inp["count"], **kw)
    two = ops.head_grad(p, dp=ops.criterion_grad(p, g, sums, inp["count"], **kw))
    differ = int((bits(fused[0]) != bits(two[0])).sum())
    report("crit vs two launches bgw %g w %s: d4 words that differ %d" % (bgw, weights, differ), 0.0 if differ == 0 else float("inf"))
    assert differ == 0 and torch.equal(bits(fused[1]), bits(two[1]))
    assert bool(torch.isfinite(fused[0]).all()) and bool(torch.isfinite(fused[1]).all())
    assert ws.intact()


def test_refusals_keep_their_messages(monkeypatch):
    """each is refused on the host, by the launcher's own check or by the arena, before any launch"""
    from brats2019_amd import ops
    ws = _guard(monkeypatch)
    z = lambda *s: torch.full(s, 0.5, dtype=torch.float32, device="cuda")
    sums = torch.ones(7, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-1\): head_grad_c4: 1\.\.4 channels, V % 4 == 0"):
        ops.head_grad(z(1, 3, 6), z(1, 3, 6))
    with pytest.raises(RuntimeError, match=r"\(-1\): head_grad_c4_crit: 1\.\.4 channels, V % 4 == 0, target and sums"):
        ops.head_grad(z(1, 3, 6), target=z(1, 3, 6), sums=sums)
    with pytest.raises(RuntimeError, match=r"\(-1\): head_grad_c4: 1\.\.4 channels, V % 4 == 0"):
        ops.head_grad(z(1, 5, 8), z(1, 5, 8))
    with pytest.raises(RuntimeError, match=r"\(-1\): head_grad_c4_crit: 1\.\.4 channels, V % 4 == 0, target and sums"):
        ops.head_grad(z(1, 5, 8), target=z(1, 5, 8), sums=torch.ones(11, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match=r"\(-1\): head_grad_c4_crit: 1\.\.4 channels, V % 4 == 0, target and sums"):
        ops.head_grad(z(1, 3, 8), target=z(1, 3, 8))
    assert ws.intact()
    for kw in (dict(dp=z(2, 3, 16388)), dict(target=z(2, 3, 16388), sums=sums), dict(dp=z(2, 3, 16388), generic=True)):
        short = _guard(monkeypatch, lambda nbytes: nbytes - 4096 - 256)
        with pytest.raises(RuntimeError, match=r"\(-2\): .*workspace too small"):
            ops.head_grad(z(2, 3, 16388), **kw)
        assert short.intact()
