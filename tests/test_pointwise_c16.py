"""The voxel-major pointwise family, op by op: every conv1_16_kernel<COB, S2D, NSLOT, PAIR> instantiation a legal launch can select and every voxel-major
branch of wgrad1_launch, driven through ru_conv1_l / ru_wgrad1_l (ops.conv1x1_c16, ops.conv1x1_bwd_weight_c16) on seeded float32 inputs converted with
ops.to_c16, against the plain float64 restatements of tests/test_pointwise_c16_host.py (which checks them against the oracle's autograd, and shows that the
bars below can fail).  Every case asserts the instantiation it was written for (the entry points report what the launchers' dispatch functions chose), so a
routing change cannot silently empty a case.  Mask operands keep |value| >= 1e-3 and the statistics operands |u - thr| >= 1e-3 (asserted in float64): no
mask decision is a rounding lottery, and no voxel is excluded from any comparison.

Bars (this project's float32 contract, tests/test_hip_ops.py header: exact-f32 MFMA, only the summation order differs):
  stored outputs, fused dg_* outputs included    |d| <= 1e-5 + 1e-5 |ref|
  weight gradients                               max |d| <= 2e-4 max |ref|
  statistic sums over >= 1e3 voxels              max |d| <= 2e-4 max |ref|
  statistic sums over fewer voxels               |d| <= V x (1e-5 + 1e-5 max |summand|)   (V elementwise bars)
Measured worst error / bar per group (forward; scatter / plain with statistics; weight gradient; fused data gradient): NOT YET RECORDED -- these
cases have not run on a device.  Every test prints its error / bar and the running worst of its group (MEASURED, `pytest -s`); the first device run
belongs here, next to the bars, and no bar moves to fit it.

Case -> instantiation (COB, S2D, NSLOT, PAIR):
  PLAIN      Cout 16 -> (1,0,0,0); 32, 48 (last group half dead) -> (2,0,0,0); 64, 80 (last group mostly dead) -> (4,0,0,0); V = 1, 63, 65, 257, 3x5x7;
             concat (16,16), (16,48) with ldw > C0 + C1, (64,32); add; out_slope 0.01; mask without a split
  SPLIT      (Cout0, Cout) (16,32) -> (2,0,0,0); (32,64), (16,64) -> (4,0,0,0): y unmasked, y1 masked
  GATHER     fine 16 -> Cout 16 (1,1,0,0); 16 -> 32 (2,1,0,0); 32 -> 64, 64 -> 128 (4,1,0,0); coarse 1x1x1, 3x5x7, 2x3x8
  SCATTER    no statistics (4,2,0,0); statistics: fine blocks 1 / 2 with Wc = 8 / 16 and no mask -> (4,2,1,1) / (4,2,2,1) (paired stores, also over several
             workgroups with dead waves); Wc = 6 (Hc Wc = 24: 8 consecutive coarse voxels straddle a z-plane), Wc = 8 with a mask -> (4,2,1,0); Wc = 7 ->
             (4,2,2,0); fine blocks 4 -> (4,2,4,0)
  PLAIN_BST  Cout 16 / 32 / 64 -> (1,0,1,0) / (2,0,2,0) / (4,0,4,0) at V = 63, 257, 4099 (several workgroups per channel)
  non-temporal  1 x 16 -> 16 x 128^3: the output is exactly 128 MB -> (1,0,0,0) with non-temporal stores
  refusals   statistics in gather mode and with a split output are refused by design (RU_REQUIRE): the message is asserted
  (COB 2 / 1 in scatter mode exist for RU_C1_SCATTER_COB only, an A/B switch read once per process: not a legal-argument route.)
  WGRAD      (Cin, Cout) (16,16) -> <1,1>; (32,16) -> <1,2>; (16,32) -> <2,1>; (64,32), (128,64), (48,80: odd block counts on both sides) -> <2,2>;
             V = 1, 105, 4099; concat 16 + 32 and 48 + 16; ldw > Cin
  WGRAD_S2D  Cin 128 / 256 / 512, coarse 3x5x7 and 2x3x8: Cout 32 / 64 -> wgrad1_s2d_kernel; Cout 16 / 48 -> wgrad1_f32_kernel's gather branch;
             tap_split against the reference's [Cout][Cin][2][2][2]
  DGRAD      Cout 16 / 32, with and without x1, slope 0.01, dg_ldw > Cin once: dg_y0 and dg_y1 both compared"""
import numpy as np
import pytest
import torch

from test_pointwise_c16_host import (SLOPE, away_from_zero, bst_terms, draw, draw_bst, elementwise_excess, ref_conv1, ref_dgrad, ref_gather, ref_scatter,
                                     ref_wgrad1, ref_wgrad_s2d, relmax_excess, stats_excess)

pytestmark = pytest.mark.gpu

MEASURED = {"forward": 0.0, "statistics": 0.0, "wgrad": 0.0, "dgrad": 0.0}


def f8(a):
    return None if a is None else np.asarray(a, np.float64)


def c16(a):
    """float32 NCDHW numpy -> voxel-major device tensor"""
    from brats2019_amd import ops
    return None if a is None else ops.to_c16(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def ncdhw(t):
    from brats2019_amd import ops
    return None if t is None else ops.from_c16(t).cpu().numpy()


def note(group, what, excess):
    MEASURED[group] = max(MEASURED[group], excess)
    print("  %-10s %s: error / bar %.3f (worst of the group so far %.3f)" % (group, what, excess, MEASURED[group]))
    return excess


def check_stats(res, d_ref, by, bk, what):
    """partials [N, C, nblk, 2] summed over nblk in float64 against the sums of the float64 summands"""
    assert res.nblk > 0 and res.partials.shape[2] == res.nblk
    terms, margin = bst_terms(d_ref, f8(by), f8(bk), SLOPE)
    assert margin >= 1e-3, margin
    got = res.partials.double().sum(2).cpu().numpy()
    assert note("statistics", what, stats_excess(got, terms.sum(2), terms)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- plain mode
# N, C0, C1, Cout, spatial, extra pitch, add, out_slope, mask, (COB, S2D, NSLOT, PAIR)
PLAIN = [(1, 16, 0, 16, (1, 1, 1), 0, False, 1.0, False, (1, 0, 0, False)),
         (2, 16, 0, 32, (1, 1, 63), 0, False, 1.0, False, (2, 0, 0, False)),
         (1, 32, 0, 48, (1, 1, 65), 0, False, 1.0, False, (2, 0, 0, False)),
         (1, 16, 0, 64, (1, 1, 257), 0, False, 1.0, False, (4, 0, 0, False)),
         (2, 32, 0, 80, (3, 5, 7), 0, False, 1.0, False, (4, 0, 0, False)),
         (1, 16, 16, 32, (1, 1, 63), 0, True, 1.0, False, (2, 0, 0, False)),
         (1, 16, 48, 16, (1, 1, 65), 8, False, 1.0, False, (1, 0, 0, False)),
         (2, 64, 32, 64, (1, 1, 257), 0, False, 0.01, False, (4, 0, 0, False)),
         (1, 16, 0, 32, (1, 1, 63), 0, False, 1.0, True, (2, 0, 0, False)),
         (1, 32, 16, 80, (1, 1, 65), 4, True, 0.01, True, (4, 0, 0, False))]


@pytest.mark.parametrize("case", PLAIN, ids=["%dx%d+%d-%d_%s_p%d_a%d_s%g_m%d" % (c[:4] + ("x".join(map(str, c[4])),) + c[5:9]) for c in PLAIN])
def test_plain_against_float64(case):
    from brats2019_amd import ops
    n, c0, c1, cout, sp, pad, has_add, out_slope, has_mask, inst = case
    x0 = draw(1, n, c0, *sp)
    x1 = draw(2, n, c1, *sp) if c1 else None
    w = draw(3, cout, c0 + c1 + pad, scale=(c0 + c1) ** -0.5)
    add = draw(4, n, cout, *sp) if has_add else None
    mask = away_from_zero(draw(5, n, cout, *sp)) if has_mask else None
    assert mask is None or float(np.abs(f8(mask)).min()) >= 1e-3
    res = ops.conv1x1_c16(c16(x0), torch.from_numpy(w).cuda(), x1=c16(x1), add=c16(add), out_slope=out_slope, mask=c16(mask), mask_slope=SLOPE)
    assert ops.conv1_inst(res.inst) == inst, ops.conv1_inst(res.inst)
    ref = ref_conv1(f8(x0), f8(w), x1=f8(x1), out_slope=out_slope, mask=f8(mask), add=f8(add))
    assert note("forward", "plain %s" % (case[:9],), elementwise_excess(ncdhw(res.y), ref)) <= 1.0


SPLIT = [(1, 16, 16, 32, (1, 1, 63), (2, 0, 0, False)), (2, 32, 32, 64, (1, 1, 257), (4, 0, 0, False)), (1, 64, 16, 64, (1, 1, 65), (4, 0, 0, False))]


@pytest.mark.parametrize("case", SPLIT, ids=["%dx%d-%dof%d_%s" % (c[:4] + ("x".join(map(str, c[4])),)) for c in SPLIT])
def test_split_output_masks_the_second_tensor_only(case):
    from brats2019_amd import ops
    n, c0, cout0, cout, sp, inst = case
    x0, w = draw(11, n, c0, *sp), draw(12, cout, c0, scale=c0 ** -0.5)
    mask = away_from_zero(draw(13, n, cout - cout0, *sp))
    assert float(np.abs(f8(mask)).min()) >= 1e-3 and (mask < 0).any()
    res = ops.conv1x1_c16(c16(x0), torch.from_numpy(w).cuda(), mask=c16(mask), mask_slope=SLOPE, cout0=cout0)
    assert ops.conv1_inst(res.inst) == inst, ops.conv1_inst(res.inst)
    y, y1 = ref_conv1(f8(x0), f8(w), mask=f8(mask), cout0=cout0)
    assert note("forward", "split %s y" % (case[:5],), elementwise_excess(ncdhw(res.y), y)) <= 1.0
    assert note("forward", "split %s y1" % (case[:5],), elementwise_excess(ncdhw(res.y1), y1)) <= 1.0


# N, Cout, spatial, add, mask, (COB, S2D, NSLOT, PAIR)
PLAIN_BST = [(n, cout, (1, 1, v), (i + j) % 2 == 1, (i + j) % 3 == 2, (cob, 0, cob, False))
             for i, (cout, cob) in enumerate([(16, 1), (32, 2), (64, 4)]) for j, (n, v) in enumerate([(2, 63), (1, 257), (1, 4099)])]


@pytest.mark.parametrize("case", PLAIN_BST, ids=["%dx32-%d_%s_a%d_m%d" % (c[0], c[1], c[2][2], c[3], c[4]) for c in PLAIN_BST])
def test_plain_with_statistics_against_float64(case):
    from brats2019_amd import ops
    n, cout, sp, has_add, has_mask, inst = case
    x0, w = draw(21, n, 32, *sp), draw(22, cout, 32, scale=32 ** -0.5)
    add = draw(23, n, cout, *sp) if has_add else None
    mask = away_from_zero(draw(24, n, cout, *sp)) if has_mask else None
    by, bk = draw_bst(25, n, cout, sp)
    res = ops.conv1x1_c16(c16(x0), torch.from_numpy(w).cuda(), add=c16(add), mask=c16(mask), mask_slope=SLOPE,
                          bst_y=c16(by), bst_k=torch.from_numpy(bk).cuda(), bst_slope=SLOPE)
    assert ops.conv1_inst(res.inst) == inst, ops.conv1_inst(res.inst)
    assert res.nblk == (sp[2] + 255) // 256
    ref = ref_conv1(f8(x0), f8(w), mask=f8(mask), add=f8(add))
    assert note("forward", "plain + statistics %s" % (case[:5],), elementwise_excess(ncdhw(res.y), ref)) <= 1.0
    check_stats(res, ref, by, bk, "plain %s" % (case[:5],))


# ---------------------------------------------------------------------------------------------------------------- stride-2 modes
# N, fine channels, Cout, coarse extents, (COB, S2D, NSLOT, PAIR)
GATHER = [(1, 16, 32, (1, 1, 1), (2, 1, 0, False)), (2, 32, 64, (3, 5, 7), (4, 1, 0, False)), (1, 64, 128, (2, 3, 8), (4, 1, 0, False)),
          (2, 16, 16, (2, 3, 8), (1, 1, 0, False))]


@pytest.mark.parametrize("case", GATHER, ids=["%dx%d-%d_%s" % (c[:3] + ("x".join(map(str, c[3])),)) for c in GATHER])
def test_gather_against_float64(case):
    from brats2019_amd import ops
    n, cf, cout, (d, h, w), inst = case
    xf, w5 = draw(31, n, cf, 2 * d, 2 * h, 2 * w), draw(32, cout, cf, 2, 2, 2, scale=(8 * cf) ** -0.5)
    res = ops.conv1x1_c16(c16(xf), torch.from_numpy(w5).cuda(), s2d=1)
    assert ops.conv1_inst(res.inst) == inst, ops.conv1_inst(res.inst)
    assert note("forward", "gather %s" % (case[:4],), elementwise_excess(ncdhw(res.y), ref_gather(f8(xf), f8(w5)))) <= 1.0


# N, C0, fine channels (Cout = 8 x), coarse extents, add, mask, statistics, (COB, S2D, NSLOT, PAIR)
SCATTER = [(1, 32, 16, (2, 3, 8), False, False, True, (4, 2, 1, True)),
           (2, 32, 16, (3, 5, 7), True, False, False, (4, 2, 0, False)),
           (1, 64, 32, (2, 3, 8), False, False, False, (4, 2, 0, False)),
           (1, 128, 64, (1, 3, 8), False, True, False, (4, 2, 0, False)),
           (2, 64, 32, (2, 2, 16), True, False, True, (4, 2, 2, True)),
           (1, 32, 16, (5, 8, 8), True, False, True, (4, 2, 1, True)),
           (1, 128, 64, (1, 3, 8), False, False, True, (4, 2, 4, False)),
           (2, 32, 16, (3, 4, 6), True, False, True, (4, 2, 1, False)),
           (1, 64, 32, (2, 3, 7), False, False, True, (4, 2, 2, False)),
           (1, 32, 16, (2, 3, 8), False, True, True, (4, 2, 1, False))]


@pytest.mark.parametrize("case", SCATTER, ids=["%dx%d-8x%d_%s_a%d_m%d_s%d" % (c[:3] + ("x".join(map(str, c[3])),) + c[4:7]) for c in SCATTER])
def test_scatter_against_float64(case):
    from brats2019_amd import ops
    n, c0, cf, (d, h, w), has_add, has_mask, has_bst, inst = case
    fine = (2 * d, 2 * h, 2 * w)
    xc, w5 = draw(41, n, c0, d, h, w), draw(42, c0, cf, 2, 2, 2, scale=c0 ** -0.5)
    add = draw(43, n, cf, *fine) if has_add else None
    mask = away_from_zero(draw(44, n, cf, *fine)) if has_mask else None
    by, bk = draw_bst(45, n, cf, fine) if has_bst else (None, None)
    res = ops.conv1x1_c16(c16(xc), torch.from_numpy(w5).cuda(), add=c16(add), mask=c16(mask), mask_slope=SLOPE, s2d=2,
                          bst_y=c16(by), bst_k=None if bk is None else torch.from_numpy(bk).cuda(), bst_slope=SLOPE)
    assert ops.conv1_inst(res.inst) == inst, ops.conv1_inst(res.inst)
    ref = ref_scatter(f8(xc), f8(w5), mask=f8(mask), add=f8(add))
    assert note("forward", "scatter %s" % (case[:7],), elementwise_excess(ncdhw(res.y), ref)) <= 1.0
    if has_bst:
        assert res.nblk == ((d * h * w + 255) // 256) * (8 * cf // 64)
        check_stats(res, ref, by, bk, "scatter %s" % (case[:7],))


def test_statistics_are_refused_where_no_fused_form_exists():
    """by design (conv1_16_launch's RU_REQUIRE): the gather mode and the split output have no statistics epilogue"""
    from brats2019_amd import ops
    xf, w5 = draw(51, 1, 16, 2, 2, 2), draw(52, 32, 16, 2, 2, 2)
    by, bk = draw_bst(53, 1, 32, (1, 1, 1))
    with pytest.raises(RuntimeError, match="fused GroupNorm-backward statistics need the plain or scatter mode"):
        ops.conv1x1_c16(c16(xf), torch.from_numpy(w5).cuda(), s2d=1, bst_y=c16(by), bst_k=torch.from_numpy(bk).cuda())
    x0, w = draw(54, 1, 16, 1, 1, 5), draw(55, 32, 16)
    by, bk = draw_bst(56, 1, 32, (1, 1, 5))
    with pytest.raises(RuntimeError, match="fused GroupNorm-backward statistics need the plain or scatter mode"):
        ops.conv1x1_c16(c16(x0), torch.from_numpy(w).cuda(), cout0=16, bst_y=c16(by), bst_k=torch.from_numpy(bk).cuda())


def test_non_temporal_stores_at_128_megabytes():
    """1 x 16 -> 16 x 128^3: N Cout V 4 = 128 MB exactly, the threshold of conv1_16_kernel's non-temporal stores"""
    from brats2019_amd import ops
    v = 128
    assert 16 * v ** 3 * 4 == 128 << 20
    x = torch.randn(1, 16, v, v, v, generator=torch.Generator().manual_seed(61))
    w = draw(62, 16, 16, scale=0.25)
    res = ops.conv1x1_c16(ops.to_c16(x.cuda()), torch.from_numpy(w).cuda())
    assert ops.conv1_inst(res.inst) == (1, 0, 0, False)
    ref = (f8(w) @ x.numpy().astype(np.float64).reshape(16, -1)).reshape(1, 16, v, v, v)
    assert note("forward", "non-temporal 16-16 128^3", elementwise_excess(ncdhw(res.y), ref)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- weight gradient
# N, C0, C1, Cout, spatial, extra pitch, (OT, CT, stride-2 kernel, fused data gradient)
_W1 = [(16, 16, (1, 1)), (32, 16, (1, 2)), (16, 32, (2, 1)), (64, 32, (2, 2)), (128, 64, (2, 2)), (48, 80, (2, 2))]
WGRAD = [(n, cin, 0, cout, sp, 0, otct + (False, False)) for cin, cout, otct in _W1 for n, sp in [(1, (1, 1, 1)), (2, (3, 5, 7)), (1, (1, 1, 4099))]]
WGRAD += [(2, 16, 32, 16, (3, 5, 7), 0, (1, 2, False, False)), (1, 48, 16, 32, (1, 1, 4099), 8, (2, 2, False, False)), (1, 32, 0, 16, (1, 1, 257), 4, (1, 2, False, False))]


@pytest.mark.parametrize("case", WGRAD, ids=["%dx%d+%d-%d_%s_p%d" % (c[:4] + ("x".join(map(str, c[4])),) + c[5:6]) for c in WGRAD])
def test_weight_gradient_against_float64(case):
    from brats2019_amd import ops
    n, c0, c1, cout, sp, pad, inst = case
    x, dy = draw(71, n, c0, *sp), draw(72, n, cout, *sp)
    x1 = draw(73, n, c1, *sp) if c1 else None
    res = ops.conv1x1_bwd_weight_c16(c16(x), c16(dy), x1=c16(x1), ldw=c0 + c1 + pad)
    assert ops.wgrad1_inst(res.inst) == inst, ops.wgrad1_inst(res.inst)
    dw = res.dw.cpu().numpy()
    assert not dw[:, c0 + c1:].any()                                   # the pitch beyond Cin is not written
    assert note("wgrad", "1x1 %s" % (case[:6],), relmax_excess(dw[:, :c0 + c1], ref_wgrad1(f8(x), f8(dy), x1=f8(x1)))) <= 1.0


# N, fine channels (Cin = 8 x), Cout, coarse extents, tap_split, (OT, CT, stride-2 kernel, fused data gradient)
WGRAD_S2D = [(2, 16, 32, (3, 5, 7), True, (2, 2, True, False)), (1, 32, 64, (2, 3, 8), True, (2, 2, True, False)),
             (1, 64, 32, (2, 3, 8), False, (2, 2, True, False)), (2, 16, 16, (3, 5, 7), True, (1, 2, False, False)),
             (1, 32, 48, (2, 3, 8), True, (2, 2, False, False)), (1, 64, 16, (3, 5, 7), False, (1, 2, False, False))]


@pytest.mark.parametrize("case", WGRAD_S2D, ids=["%dx8x%d-%d_%s_t%d" % (c[:3] + ("x".join(map(str, c[3])),) + c[4:5]) for c in WGRAD_S2D])
def test_stride2_weight_gradient_against_float64(case):
    from brats2019_amd import ops
    n, cf, cout, (d, h, w), tap_split, inst = case
    xf, dy = draw(81, n, cf, 2 * d, 2 * h, 2 * w), draw(82, n, cout, d, h, w)
    res = ops.conv1x1_bwd_weight_c16(c16(xf), c16(dy), s2d=True, tap_split=tap_split)
    assert ops.wgrad1_inst(res.inst) == inst, ops.wgrad1_inst(res.inst)
    ref = ref_wgrad_s2d(f8(xf), f8(dy))                                # [Cout][Cin][2][2][2]
    if not tap_split:                                                  # the kernel's own order: [Cout][tap * Cin + c]
        ref = ref.reshape(cout, cf, 8).transpose(0, 2, 1).reshape(cout, 8 * cf)
    assert note("wgrad", "stride-2 %s" % (case[:5],), relmax_excess(res.dw.cpu().numpy(), ref)) <= 1.0


# N, C0, C1, Cout, spatial, extra pitch of dg_w, (OT, CT, stride-2 kernel, fused data gradient)
DGRAD = [(2, 16, 16, 16, (3, 5, 7), 0, (1, 2, False, True)), (1, 16, 48, 32, (1, 1, 257), 4, (2, 2, False, True)),
         (1, 16, 0, 16, (3, 5, 7), 0, (1, 1, False, True)), (2, 32, 0, 32, (1, 1, 257), 0, (2, 2, False, True)),
         (1, 16, 0, 32, (1, 1, 63), 0, (2, 1, False, True)), (1, 32, 32, 16, (1, 1, 4099), 0, (1, 2, False, True))]


@pytest.mark.parametrize("case", DGRAD, ids=["%dx%d+%d-%d_%s_p%d" % (c[:4] + ("x".join(map(str, c[4])),) + c[5:6]) for c in DGRAD])
def test_fused_data_gradient_against_float64(case):
    from brats2019_amd import ops
    n, c0, c1, cout, sp, pad, inst = case
    x, dy = draw(91, n, c0, *sp), draw(92, n, cout, *sp)
    x1 = away_from_zero(draw(93, n, c1, *sp)) if c1 else None
    assert x1 is None or (float(np.abs(f8(x1)).min()) >= 1e-3 and (x1 < 0).any())
    w = draw(94, cout, c0 + c1 + pad, scale=cout ** -0.5)
    res = ops.conv1x1_bwd_weight_c16(c16(x), c16(dy), x1=c16(x1), dg_w=torch.from_numpy(w).cuda(), dg_mask_slope=SLOPE)
    assert ops.wgrad1_inst(res.inst) == inst, ops.wgrad1_inst(res.inst)
    assert note("wgrad", "with fused data gradient %s" % (case[:6],), relmax_excess(res.dw.cpu().numpy(), ref_wgrad1(f8(x), f8(dy), x1=f8(x1)))) <= 1.0
    dx0, dx1 = ref_dgrad(f8(dy), f8(w), c0, x1=f8(x1), slope=SLOPE)
    assert note("dgrad", "dg_y0 %s" % (case[:6],), elementwise_excess(ncdhw(res.dx0), dx0)) <= 1.0
    assert (res.dx1 is None) == (c1 == 0)
    if c1:
        assert note("dgrad", "dg_y1 %s" % (case[:6],), elementwise_excess(ncdhw(res.dx1), dx1)) <= 1.0
