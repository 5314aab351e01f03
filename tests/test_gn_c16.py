"""The voxel-major GroupNorm chain of the shipped configuration, link by link, against the float64 reference of tests/test_gn_c16_host.py (which proves that reference
against the oracle and float64 autograd, and proves the exact family exact): the two finalizes on synthetic partials (ops.gn_finalize / ops.gn_bwd_finalize), the
constants the finalize writes fed into the kernels that consume them, the four stand-alone C16 kernels (ops.gn_apply_c16 / ops.gn_bwd_c16) at every path switch,
the in-launch tails of the reduction and of one launch per 3x3x3 route family, and the conditioning of the (sum, sumsq) statistics.

Path switches and the case on each side (V voxels per (sample, channel block); nblk = partials per (sample, channel)):
  gn16_chunk 512 -> 2048 at V = 2^15          V = 32767 (nblk 64) / 32768 (nblk 16)          gn16_chunk 2048 -> 8192 at V = 2^20     V = 2^20 - 1 (nblk 512) / 2^20 (nblk 128)
  gn_bwd_finalize_kernel<4 | 16 | 64>         nblk 4 / 5 (V = 2048 / 2049) and 32 / 33 (V = 16384 / 16385); synthetic partials nblk 1, 4, 5, 32, 33, 64, 65, 256, 257, 513
  fin_tail kind 2 lane groups 4 | 16 | 64     nblk 64 / 65 (V = 32767 / 131073) and 256 / 257 (exact V = 2^19 / real and exact V = 524289); nblk 512 (V = 2^20 - 1)
  fin_tail kind 1 lane groups 4 | 16 | 64     cnt = cpg * nblk: 64 (one-stage route case, nblk 32) / 80 (40 one-stage tiles); 512 and 1024 (the persistent, 4-channel, MX and
                                              Winograd-z route cases: nblk 256 at 16 and 32 channels) / 1056 (528 one-stage tiles: the outer loop of fin_sum_pairs<64> runs twice)
  fin_tail kind 2 inside a convolution        nblk 256 (persistent 16 -> 16, MX gradient operand, 4-channel head gradient) and 128 (32 -> 32): lane groups of 16
  apply grid cap 2048 workgroups              plain: V = 32768 (exactly 2048 * 64 float4) / 131073 (second grid-stride iteration); split: V = 131073 / 524289
  nontemporal apply at 128 MB                 N = 1, V = 2^20 (64 MB: plain loads and stores) / N = 2, V = 2^20 (RES 1 and RES 2, apply only)
  channel quad inside one group / across two  C = 32 (cpg 4) / C = 16 (cpg 2: every quad holds two groups) and C = 48 (cpg 6: the quad 4..7 holds channels of groups 0 and 1)
Not reachable at test size: gn_bwd_reduce16 with nblk > 1024 (V > 8.4 M voxels).

Bars: the project's own for the NCDHW kernels of the same arithmetic (tests/test_hip_ops.py, check_gn_case), unchanged -- y 3e-6 + 1e-5 |ref|; mean 1e-6; rstd 1e-5
relative; dx 1e-4 |ref| + 5e-6; dgamma, dbeta and each of the three coefficient planes 2e-4 of the plane's largest value.  scale, shift and bst_k carry the bars of the
mean and rstd they are formed from plus four float32 roundings (stat_bars).  The split output is held to those of dx plus the split form's own bar
(tests/test_wgrad3_fused_host.py: 2^-16 (|v| + F) + F) and must equal ops.to_split_c16 of the plain output bit for bit (pw_split8 is the converters' split_n).
Every check prints its error / bar before it asserts (`pytest -s`).

Measured on the first device run (MI355X), worst error / bar per group: y 0.17 (RES 2, C = 48), dx 0.003, summed partials / coefficients / dgamma / dbeta 0.002,
finalizes on real partials 0.0003, split output 0.07, chain (dw of the fused apply) 0.71; every tail, exact and real, wrote the bits of the separate launch.
Mutation check (by hand, one edit per build of the library, this file run against each; failed tests of 168):
  s2_sign flip dropped      gn_bwd_finalize_kernel 86 (exact and real finalizes, convolution tails against it, chain); fin_tail phase 1: 8 (the kind-2 convolution tails)
  gamma for |gamma| in thr  gn_finalize_kernel 93 (exact and real finalizes, bst_k constants, kind-1 tails against it, chain); fin_tail: 18 (kind-1 tails, one-stage tails)
  nblk - 1 pairs read       fin_sum_pairs 84 (every test with a tail)
  c4 / cpg for the quad     gn_bwd_reduce16_kernel 52 (every backward at C = 16 and 48; C = 32 passes, as it must)
  rscale / rshift swapped   gn_apply16_kernel<2> 43 (every RES = 2 apply, the 128 MB case included)"""
import numpy as np
import pytest
import torch

import test_gn_c16_host as H
from test_conv3_fused_host import CASE_BY_NAME
from test_hip_ops import GN_RATIOS, gn_fixture_ratio
from test_wgrad3_fused_host import dw_excess, split_decode

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
MEASURED = {}


@pytest.fixture(scope="module")
def ops():
    from brats2019_amd import ops as m
    return m


def note(group, what, excess):
    excess = float(excess)
    MEASURED[group] = max(MEASURED.get(group, 0.0), excess) if excess == excess else float("nan")
    print("  %-10s %s: error / bar %.3g (worst of the group so far %.3g)" % (group, what, excess, MEASURED[group]))
    return excess


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()                    # (a copy: the cached operands are read-only)


def gpu64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def excess_close(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|), on the device (ref: float64 numpy in got's layout); NaN where got has one"""
    r = gpu64(ref).reshape(got.shape)
    return float(((got.double() - r).abs() / (atol + rtol * r.abs())).max())


def excess_rel_max(got, ref, rel=2e-4):
    """close_rel_max of tests/test_hip_ops.py as error / bar"""
    r = gpu64(ref).reshape(got.shape)
    return float((got.double() - r).abs().max() / (rel * (r.abs().max() + 1e-30)))


def excess_coef(got, ref):
    return max(excess_rel_max(got[..., k], np.asarray(ref)[..., k]) for k in range(3))


def c16(a):
    return dev(H.blocks(a))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def stat_bars(st, gamma, beta):
    """bars of scale, shift, k1, k2 [N, C] from the bars of mean (1e-6) and rstd (1e-5 relative) they are formed from, plus four float32 roundings of the terms"""
    cpg = len(gamma) // H.G
    mu, rs = np.abs(H.per_channel(st["mean"], cpg)), H.per_channel(st["rstd"], cpg)
    ag, ab = np.abs(np.asarray(gamma, np.float64))[None], np.abs(np.asarray(beta, np.float64))[None]
    scale = ag * rs * (1e-5 + 4 * U24)
    return dict(scale=scale + 1e-300, shift=ag * rs * 1e-6 + mu * scale + 4 * U24 * (ab + mu * ag * rs) + 1e-300, k1=rs * (1e-5 + 4 * U24),
                k2=rs * 1e-6 + mu * rs * (1e-5 + 4 * U24) + 1e-300)


def check_stats(tag, r, want, gamma, beta, group="finalize"):
    """GnStats `r` against float64 statistics `want` at the bars above"""
    n = want["mean"].shape[0]
    b = stat_bars(want, gamma, beta)
    e = lambda got, ref, bar: float((np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref) / bar).max())
    worst = max(e(r.mean, want["mean"], 1e-6), e(r.rstd, want["rstd"], 1e-5 * want["rstd"]), e(r.scale, want["scale"], b["scale"]), e(r.shift, want["shift"], b["shift"]))
    if r.bst_k is not None:
        k = r.bst_k.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.where(gamma == 0, np.where(beta > 0, -np.inf, np.inf), -beta / np.abs(gamma)).astype(np.float32)     # one correctly rounded float32 division
        assert np.array_equal(k[:, 2], np.broadcast_to(thr, (n, len(gamma)))), tag
        worst = max(worst, e(r.bst_k[:, 0], want["bst_k"][:, 0], b["k1"]), e(r.bst_k[:, 1], want["bst_k"][:, 1], b["k2"]))
    assert note(group, tag, worst) <= 1.0


# ====================================================================================================================== a. finalize on synthetic partials
NBLKS = (1, 4, 5, 32, 33, 64, 65, 256, 257, 513)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [16, 32, 48])
@pytest.mark.parametrize("nblk", NBLKS)
def test_finalizes_on_exact_partials_equal_the_reference_bit_for_bit(ops, nblk, c, n):
    """ops.gn_finalize and ops.gn_bwd_finalize (s2_sign 0 and 1) on the exact family with the sign pattern and the zeros of gn_param_set: every output equals the host
    reference (a lost, doubled or stale pair moves a sum by at least one unit)"""
    for kind in ("signs", "zeros"):
        p, gamma, beta, V = H.exact_stat_partials(n, c, nblk, kind)
        r = ops.gn_finalize(dev(p), dev(gamma), dev(beta), V, want_k=True)
        want = H.ref_finalize_device(p, gamma, beta, V)
        for k in ("mean", "rstd", "scale", "shift", "bst_k"):
            got = getattr(r, k).cpu().numpy().reshape(want[k].shape)
            assert np.array_equal(got, want[k]), (kind, k, np.abs(got - want[k])[np.isfinite(want[k])].max())
        for s2_sign in (0, 1):
            p, gamma, mean, rstd, V = H.exact_bwd_partials(n, c, nblk, kind, s2_sign)
            r = ops.gn_bwd_finalize(dev(p), dev(gamma), dev(mean.ravel()), dev(rstd.ravel()), V, s2_sign)
            want = H.ref_bwd_finalize(p.astype(np.float64).sum(2), gamma, mean, rstd, V, s2_sign)
            for k in ("coef", "dgamma", "dbeta"):
                got = getattr(r, k).cpu().numpy().astype(np.float64)
                assert np.array_equal(got, want[k]), (kind, s2_sign, k, np.abs(got - want[k]).max())


def test_bst_k_constants_carry_the_sign_of_gamma_and_the_infinite_thresholds(ops):
    """gamma == 0 with beta > 0, < 0, == 0 (channels 0, 1, 2 of the `zeros` set): the third constant is -inf, +inf, +inf exactly; gamma < 0: the first two constants
    carry the sign (k1 = -rstd, k2 = +mean * rstd)"""
    p, gamma, beta, V = H.exact_stat_partials(3, 16, 5, "zeros")
    assert (gamma[:3] == 0).all() and beta[0] > 0 and beta[1] < 0 and beta[2] == 0 and (gamma < 0).any() and (gamma > 0).any()
    r = ops.gn_finalize(dev(p), dev(gamma), dev(beta), V, want_k=True)
    k, mean, rstd = r.bst_k.cpu().numpy(), r.mean.cpu().numpy().reshape(3, 8), r.rstd.cpu().numpy().reshape(3, 8)
    assert (k[:, 2, 0] == -np.inf).all() and (k[:, 2, 1] == np.inf).all() and (k[:, 2, 2] == np.inf).all()
    assert np.isfinite(k[:, 2, 3:]).all() and np.array_equal(k[:, 2, 3:], np.broadcast_to(-beta[3:] / np.abs(gamma[3:]), (3, 13)))
    assert (mean != 0).any()
    for j in range(16):
        sg = -1.0 if gamma[j] < 0 else 1.0
        assert np.array_equal(k[:, 0, j], sg * rstd[:, j // 2]) and np.array_equal(k[:, 1, j], -sg * mean[:, j // 2] * rstd[:, j // 2])
    assert (r.scale.cpu().numpy()[:, :3] == 0).all() and np.array_equal(r.shift.cpu().numpy()[:, :3], np.broadcast_to(beta[:3], (3, 3)))


@pytest.mark.parametrize("kind", ["signs", "zeros", "tiny", "ties"])
@pytest.mark.parametrize("c,nblk", [(16, 5), (32, 33), (48, 65), (16, 257)])
def test_finalizes_on_real_partials_against_float64(ops, c, nblk, kind):
    """float32 (sum, sumsq) partials of a seeded tensor with mean 0.5 and deviation 2, and float32 backward sums of seeded normal values: this file's bars"""
    a = H.real_case(2049, c, kind)
    p = H._chunk_partials(a["x"], nblk).astype(np.float32)
    r = ops.gn_finalize(dev(p), dev(a["gamma"]), dev(a["beta"]), 2049, want_k=True)
    check_stats("C=%d nblk=%d %s" % (c, nblk, kind), r, H.ref_finalize(p, a["gamma"], a["beta"], 2049), a["gamma"], a["beta"])
    rng = np.random.default_rng([c, nblk])
    S = rng.standard_normal((2, c, nblk, 2)).astype(np.float32) * 30
    st = H.stats32(H.stats_of(a["x"], a["gamma"], a["beta"]))
    for s2_sign in (0, 1):
        r = ops.gn_bwd_finalize(dev(S), dev(a["gamma"]), dev(st["mean"].ravel()), dev(st["rstd"].ravel()), 2049, s2_sign)
        want = H.ref_bwd_finalize(S.astype(np.float64).sum(2), a["gamma"], st["mean"], st["rstd"], 2049, s2_sign)
        worst = max(excess_coef(r.coef, want["coef"]), excess_rel_max(r.dgamma, want["dgamma"]), excess_rel_max(r.dbeta, want["dbeta"]))
        assert note("finalize", "backward C=%d nblk=%d %s s2_sign=%d" % (c, nblk, kind, s2_sign), worst) <= 1.0


def test_centred_finalize_on_real_partials_against_float64(ops):
    """the (sum, M2) pairs of the NCDHW statistics pass, three chunks with a ragged last one, at mean / deviation = 30"""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((2, 16, 1, 3, 5500)) + 30.0).astype(np.float32)
    gamma, beta = H.gn_param_set("signs", 16, rng)
    p = H._chunk_partials(x, 3, centred=True, chunk=H.GN_CHUNK).astype(np.float32)
    r = ops.gn_finalize(dev(p), dev(gamma), dev(beta), 16500, centred=True)
    check_stats("centred", r, H.ref_finalize(p, gamma, beta, 16500, centred=True), gamma, beta)


# ====================================================================================================================== c. the stand-alone kernels against float64
NBLK_OF = {105: 1, 2048: 4, 2049: 5, 16384: 32, 16385: 33, 32767: 64, 32768: 16, 131073: 65, 524289: 257, (1 << 20) - 1: 512, 1 << 20: 128}
_DEV = {}


def device_case(v, c, kind, n):
    """the operands of H.real_case on the device (voxel-major) and the float32 statistics of both GroupNorms, once per module"""
    key = (v, c, kind, n)
    if key not in _DEV:
        _DEV.clear()                                                                   # (one case resident at a time: the large ones are 64 MB per tensor)
        a = H.real_case(v, c, kind, n)
        st, st2 = H.stats_of(a["x"], a["gamma"], a["beta"]), H.stats_of(a["res"], a["gamma2"], a["beta2"])
        s32, s232 = H.stats32(st), H.stats32(st2)
        _DEV[key] = dict(a=a, st=st, st2=st2, x=c16(a["x"]), res=c16(a["res"]), dact=c16(a["dact"]), gamma=dev(a["gamma"]),
                         scale=dev(s32["scale"]), shift=dev(s32["shift"]), mean=dev(s32["mean"].ravel()), rstd=dev(s32["rstd"].ravel()),
                         rscale=dev(s232["scale"]), rshift=dev(s232["shift"]))
    return _DEV[key]


def check_apply(ops, d, slope, tag, forms=(0, 1, 2)):
    a, st, st2 = d["a"], d["st"], d["st2"]
    for res in forms:
        kw = {} if res == 0 else dict(res=d["res"]) if res == 1 else dict(res=d["res"], res_scale=d["rscale"], res_shift=d["rshift"], res_slope=0.01)
        y = ops.gn_apply_c16(d["x"], d["scale"], d["shift"], slope, **kw)
        ref = H.ref_apply(a["x"], st["scale"], st["shift"], slope, *((), (a["res"],), (a["res"], st2["scale"], st2["shift"], 0.01))[res])
        assert note("y", "%s RES=%d" % (tag, res), excess_close(y, H.blocks(ref), 1e-5, 3e-6)) <= 1.0


def check_backward(ops, d, slope, tag, v):
    a = d["a"]
    ref = H.ref_chain(a["x"], a["gamma"], a["beta"], a["dact"], slope)
    args = (d["x"], d["dact"], d["gamma"], d["scale"], d["shift"], d["mean"], d["rstd"], slope)
    dx64 = H.blocks(ref["dx"])
    runs = {(t, s): ops.gn_bwd_c16(*args, tail=t, split=s) for t in (False, True) for s in (False, True)}
    for (t, s), r in runs.items():
        what = "%s tail=%d split=%d" % (tag, t, s)
        assert r.partials.shape[2] == NBLK_OF[v], (what, r.partials.shape)
        assert note("sums", what, excess_rel_max(r.partials.double().sum(2), ref["S"])) <= 1.0
        assert note("coef", what, excess_coef(r.coef, ref["coef"])) <= 1.0
        assert note("dgamma", what, excess_rel_max(r.dgamma, ref["dgamma"])) <= 1.0
        assert note("dbeta", what, excess_rel_max(r.dbeta, ref["dbeta"])) <= 1.0
        if not s:
            assert note("dx", what, excess_close(r.dx, dx64, 1e-4, 5e-6)) <= 1.0
    plain, tailed = runs[(False, False)], runs[(True, False)]
    # the tail finalizes the same partials: within the coefficient bar of the separate launch (and the reduction does not depend on who finalizes)
    assert same([plain.partials], [tailed.partials])
    assert note("tail", tag + " tail against the separate finalize", max(excess_coef(tailed.coef, plain.coef.double().cpu().numpy()),
                                                                            excess_rel_max(tailed.dgamma, plain.dgamma.double().cpu().numpy()),
                                                                            excess_rel_max(tailed.dbeta, plain.dbeta.double().cpu().numpy()))) <= 1.0
    for t in (False, True):
        # split form: the packets of the plain output, bit for bit; decoded, within the bar of dx plus the split form's own
        assert same([runs[(t, True)].coef], [runs[(t, False)].coef])
        assert torch.equal(bits(runs[(t, True)].dx), bits(ops.to_split_c16(runs[(t, False)].dx))), "%s tail=%d: split output is not to_split_c16(plain output)" % (tag, t)
    if v <= 32768:                                                                     # (decoded on the host: the small cases carry this check)
        dec = split_decode(runs[(True, True)].dx.contiguous().view(torch.uint8).cpu().numpy().reshape(dx64.shape[:-1] + (64,)))
        f = H.blocks(H.ref_dx_rounding(a["x"], a["dact"], ref["scale"], ref["shift"], ref["coef"], slope))
        bar = 1e-4 * np.abs(dx64) + 5e-6 + 2.0 ** -16 * (np.abs(dx64) + f) + f
        assert note("split", tag, float((np.abs(dec - dx64) / bar).max())) <= 1.0
    stop = ops.gn_bwd_c16(*args, tail=True, stop_after_finalize=True)
    assert stop.dx is None and same(stop[1:], tailed[1:])


def check_case(ops, v, c, kind, n, slope):
    d = device_case(v, c, kind, n)
    tag = "V=%d C=%d N=%d %s slope=%g" % (v, c, n, kind, slope)
    check_apply(ops, d, slope, tag)
    check_backward(ops, d, slope, tag, v)


@pytest.mark.parametrize("slope", [1.0, 0.01])
@pytest.mark.parametrize("v,n", [(105, 2), (2048, 2), (2049, 2), (16384, 2), (16385, 2), (32767, 2), (32768, 2), (131073, 2), (524289, 1), ((1 << 20) - 1, 1), (1 << 20, 1)])
def test_c16_kernels_at_every_path_switch_against_float64(ops, v, n, slope):
    """gn_apply16 (RES 0, 1, 2), gn_bwd_reduce16 with and without its tail, both finalizes, gn_bwd_apply16 plain and split, on gammas of both signs"""
    check_case(ops, v, 16, "signs", n, slope)


@pytest.mark.parametrize("slope", [1.0, 0.01])
@pytest.mark.parametrize("c", [32, 48])
@pytest.mark.parametrize("v", [2049, 16385])
def test_c16_kernels_at_channel_counts_against_float64(ops, v, c, slope):
    """C = 32: cpg = 4, a thread's channel quad is one group; C = 48: cpg = 6, the quad 4..7 holds channels of two groups, unevenly (gn_bwd_reduce16_kernel looks the
    group up per channel; at C = 16 every quad holds two whole groups)"""
    check_case(ops, v, c, "signs", 2, slope)


@pytest.mark.parametrize("slope", [1.0, 0.01])
@pytest.mark.parametrize("v", [105, 2049])
@pytest.mark.parametrize("kind", ["zeros", "tiny", "ties"])
def test_c16_kernels_with_zero_tiny_and_tied_parameters_against_float64(ops, kind, v, slope):
    check_case(ops, v, 16, kind, 2, slope)


@pytest.mark.parametrize("slope", [0.01])
def test_apply_nontemporal_variants_at_128_mb(ops, slope):
    """N = 2, C = 16, V = 2^20: the tensor is exactly 128 MB, gn_apply16_kernel<1, true> and <2, true>.  The single large case of the file; the apply only."""
    d = device_case(1 << 20, 16, "signs", 2)
    assert d["x"].numel() * 4 == 128 << 20
    check_apply(ops, d, slope, "V=2^20 N=2 nontemporal", forms=(1, 2))
    _DEV.clear()


# ====================================================================================================================== d. tails
def exact_chain(v, c, kind, n):
    e = H.exact_chain_case(v, c, kind, n)
    args = (c16(e["x"]), c16(e["dact"]), dev(e["gamma"]), dev(e["scale"]), dev(e["shift"]), dev(e["mean"].ravel()), dev(e["rstd"].ravel()), H.EXACT_SLOPE)
    return e, args


@pytest.mark.parametrize("kind", ["signs", "zeros"])
@pytest.mark.parametrize("v,n,c", [(2048, 2, 16), (2048, 2, 32), (32768, 2, 16), (131072, 2, 16), (262144, 1, 16), (524288, 1, 16), (524289, 1, 16), ((1 << 20) - 1, 1, 16)])
def test_reduction_tail_on_exact_inputs_equals_the_separate_finalize_bit_for_bit(ops, v, n, c, kind):
    """nblk 4, 16, 64 (lane groups of 4), 128, 256 (16), 257, 512 (64).  The sums are exact, so dgamma, dbeta and the summed partials equal the float64 reference at every V;
    where V is a power of two the coefficients do too (their divisions are exact), elsewhere they meet the coefficient bar.  Called again on the SAME workspace without
    zeroing the ticket, the launch gives the same bits: the finisher reset it."""
    from brats2019_amd import _lib as L
    e, args = exact_chain(v, c, kind, n)
    sep, tail = ops.gn_bwd_c16(*args), ops.gn_bwd_c16(*args, tail=True)
    assert same(sep, tail)
    S = H.ref_bwd_sums(e["x"], e["dact"], e["scale"], e["shift"], e["mean"], e["rstd"], H.EXACT_SLOPE)
    fin = H.ref_bwd_finalize(S, e["gamma"], e["mean"], e["rstd"], v)
    for r in (sep, tail):
        assert np.array_equal(r.partials.double().sum(2).cpu().numpy(), S)
        assert np.array_equal(r.dgamma.double().cpu().numpy(), fin["dgamma"]) and np.array_equal(r.dbeta.double().cpu().numpy(), fin["dbeta"])
        if v & (v - 1) == 0:
            assert np.array_equal(r.coef.double().cpu().numpy(), fin["coef"])
        else:
            assert note("coef", "exact V=%d" % v, excess_coef(r.coef, fin["coef"])) <= 1.0
    ws = L.workspace(L.load().ru_gn_bwd_l_workspace_bytes(n, c, v), "cuda")
    ws.fill_(0xFF)
    first = ops.gn_bwd_c16(*args, tail=True, workspace=ws)
    second = ops.gn_bwd_c16(*args, tail=True, workspace=ws, keep_ticket=True)           # (dgamma / dbeta are new tensors full of NaN: a tail that never ran leaves them so)
    assert same(first, tail) and same(second, tail) and bool(torch.isfinite(second.dgamma).all())


def test_reduction_tail_refuses_what_exceeds_its_lds(ops):
    """N * C * 16 bytes of kind-2 scratch above the 64 KB of a workgroup: refused on the host with the launcher's message; the separate finalize takes the shape"""
    n, c = 8, 512
    x = torch.zeros(n, c // 16, 1, 1, 1, 16, device="cuda")
    v = torch.ones(n, c, device="cuda")
    g = torch.ones(n * 8, device="cuda")
    with pytest.raises(RuntimeError, match="batch x channels too large for the in-launch finalize"):
        ops.gn_bwd_c16(x, x, torch.ones(c, device="cuda"), v, v, g, g, 1.0, tail=True)
    assert bool(torch.isfinite(ops.gn_bwd_c16(x, x, torch.ones(c, device="cuda"), v, v, g, g, 1.0).dx).all())


# one launch per 3x3x3 route family that hosts a tail, at the cases of tests/test_conv3_fused_host.py (the `conv3_l_route_*` shapes of tests/op_cases.py):
# (case, kind, extra arguments, groups).  cnt = cpg * nblk pairs per item picks the lane-group width of kind 1; nblk that of kind 2.
CONV_TAILS = [("sb_24_scale_add_stats", 1, {}, 8), ("sb2_16_add_stats", 1, {}, 8), ("stem_c4_stats", 1, {}, 8), ("mx_scale_stats", 1, {}, 8), ("mxg_b0_a0", 1, dict(stats=True), 8),
              ("wz32_scale_stats", 1, {}, 8), ("wz32mx_scale_stats", 1, {}, 8), ("head3_plain", 1, dict(stats=True), 1),
              ("dgrad_split_16_b1_a0", 2, {}, 8), ("dgrad_split_32_b1_a0", 2, {}, 8), ("mxg_b1_a0", 2, {}, 8), ("head_dgrad_c3_bst", 2, {}, 8)]


def conv_tail_params(c, kind, groups, exact):
    rng = np.random.default_rng([sum(c["name"].encode()), kind, int(exact)])
    n, co = c["n"], c["cout"]
    if exact:
        gamma, beta = H.exact_params("signs", 16, rng)
        gamma, beta = np.resize(gamma, co), np.resize(beta, co)
        mean, rstd = rng.integers(-2, 3, n * groups).astype(np.float32), rng.choice([0.5, 1.0, 2.0], n * groups).astype(np.float32)
    else:
        gamma, beta = (np.resize(t, co) for t in H.gn_param_set("signs", 16, rng))
        mean, rstd = (rng.standard_normal(n * groups) * 0.3).astype(np.float32), rng.uniform(0.5, 1.5, n * groups).astype(np.float32)
    return gamma, beta, mean, rstd


def run_conv_tail(ops, name, kind, extra, groups, **more):
    import test_conv3_fused as TC
    c = CASE_BY_NAME[name]
    i, _ = TC.shared(c)
    gamma, beta, mean, rstd = conv_tail_params(c, kind, groups, c["exact"])
    kw = dict(tail=kind, tail_gamma=dev(gamma), tail_groups=groups)
    kw.update(dict(tail_beta=dev(beta), tail_want_k=True) if kind == 1 else dict(tail_mean=dev(mean), tail_rstd=dev(rstd), tail_s2_sign=1))
    kw.update(extra)
    kw.update(more)
    return c, (gamma, beta, mean, rstd), TC.launch(c, i, **kw)


@pytest.mark.parametrize("family", ["exact", "real"])
@pytest.mark.parametrize("name,kind,extra,groups", CONV_TAILS, ids=["%s_kind%d" % (t[0], t[1]) for t in CONV_TAILS])
def test_convolution_tails_equal_the_separate_finalize(ops, name, kind, extra, groups, family):
    """The tail of every 3x3x3 route family on the partials its own launch published, against the separate finalize launch on the same partials: exact inputs bit
    for bit; real inputs within one float32 ulp (mean, rstd, scale, shift) / the coefficient bar, and both within this file's bars of float64.  A second launch on the
    same workspace without zeroing the ticket gives the same bits."""
    c, (gamma, beta, mean, rstd), r = run_conv_tail(ops, name + "_" + family, kind, extra, groups)
    v = int(np.prod(c["dhw"]))
    fin, ws = r.fin
    p64 = r.partials.double().cpu().numpy()
    assert np.isfinite(p64).all()
    tag = "%s kind %d %s (%s, nblk %d)" % (name, kind, family, ops.conv3_route(r.route).family, r.nblk)
    if kind == 1:
        sep = ops.gn_finalize(r.partials, dev(gamma), dev(beta), v, want_k=True, groups=groups)
        if family == "exact":
            assert same(fin, sep), tag
        else:
            ulp = lambda a, b: float(((a.double() - b.double()).abs() / torch.from_numpy(np.spacing(np.abs(b.cpu().numpy()))).cuda().double()).max())
            assert note("tail", tag + " ulps", max(ulp(a, b) for a, b in zip(fin[:4], sep[:4]))) <= 1.0
            assert torch.equal(fin.bst_k[:, 2], sep.bst_k[:, 2])
        if groups == 8:
            want = H.ref_finalize(p64, gamma, beta, v)
            for got in (fin, sep):
                check_stats(tag, got, want, gamma, beta, group="tail")
    else:
        sep = ops.gn_bwd_finalize(r.partials, dev(gamma), dev(mean), dev(rstd), v, 1, groups=groups)
        if family == "exact":
            assert same(fin, sep), tag
        want = H.ref_bwd_finalize(p64.sum(2), gamma, mean.reshape(c["n"], groups), rstd.reshape(c["n"], groups), v, s2_sign=1)
        for got in (fin, sep):
            worst = max(excess_coef(got.coef, want["coef"]), excess_rel_max(got.dgamma, want["dgamma"]), excess_rel_max(got.dbeta, want["dbeta"]))
            assert note("tail", tag, worst) <= 1.0
    _, _, again = run_conv_tail(ops, name + "_" + family, kind, extra, groups, tail_workspace=ws, tail_keep_ticket=True)
    assert same(again.fin[0], fin) and same([again.y, again.partials], [r.y, r.partials]), tag


@pytest.mark.parametrize("sp,nblk", [((10, 16, 18), 40), ((66, 32, 18), 528)], ids=["cnt80", "cnt1056"])
def test_one_stage_tail_at_its_other_lane_group_widths(ops, sp, nblk):
    """1 x 16 -> 16 on one-stage (2, 4, 16) tiles, one partial per tile, cnt = cpg * nblk pairs per (sample, group).  10 x 16 x 18: 40 tiles, cnt = 80 -- lane groups of
    16 (the route cases have cnt 64, 512 and 1024: groups of 4 and 64).  66 x 32 x 18: 528 tiles, cnt = 1056 -- fin_sum_pairs<64> takes 1024 pairs per pass of its outer
    loop, so the second pass runs.  Exact integers: the tail equals the separate launch and the float64 reference bit for bit."""
    rng = np.random.default_rng(66)
    shape = (1, 16) + sp
    x = rng.integers(-2, 3, shape).astype(np.float32)
    w = (rng.choice([-1.0, 1.0], (16, 16, 3, 3, 3)) * (rng.integers(0, 256, (16, 16, 3, 3, 3)) == 0)).astype(np.float32)
    add = rng.integers(-3, 4, shape).astype(np.float32)
    gamma, beta = H.exact_params("signs", 16, rng)
    r = ops.conv3_fused(c16(x), dev(w), in_c16=True, out_c16=True, add=c16(add), stats=True, tail=1, tail_gamma=dev(gamma), tail_beta=dev(beta), tail_want_k=True)
    route = ops.conv3_route(r.route)
    assert route.family == "sb" and r.nblk == nblk, (route, r.nblk)
    fin, _ = r.fin
    v = int(np.prod(sp))
    assert same(fin, ops.gn_finalize(r.partials, dev(gamma), dev(beta), v, want_k=True))
    y = H.unblocks(r.y.cpu().numpy()).astype(np.float64)
    s = np.stack([y.reshape(1, 16, -1).sum(-1), (y * y).reshape(1, 16, -1).sum(-1)], axis=-1)
    assert np.array_equal(r.partials.double().sum(2).cpu().numpy(), s)
    want = H.ref_finalize(s[:, :, None, :], gamma, beta, v)
    assert np.array_equal(fin.mean.cpu().numpy().reshape(1, 8), want["mean"].astype(np.float32)) and np.array_equal(fin.rstd.cpu().numpy().reshape(1, 8), want["rstd"].astype(np.float32))


def test_mismatched_tail_descriptors_are_refused_with_the_launchers_messages(ops):
    """a wrong nblk / N / C is refused on the host before anything of the convolution is launched; conv3_f32c keeps refusing a tail"""
    for name, kind, groups, who in (("sb2_16_add_stats_real", 1, 8, "conv3_sb2"), ("sb_24_scale_add_stats_real", 1, 8, "conv3_sb"), ("mx_scale_stats_real", 1, 8, "conv3_mx"),
                                    ("wz32_scale_stats_real", 1, 8, "conv3_wz32"), ("wz32mx_scale_stats_real", 1, 8, "conv3_wz32mx"), ("stem_c4_stats_real", 1, 8, "conv3_sb2c4"),
                                    ("dgrad_split_16_b1_a0_real", 2, 8, "conv3_sb2")):
        c = CASE_BY_NAME[name]
        _, _, ok = run_conv_tail(ops, name, kind, {}, groups)
        for over in (dict(nblk=ok.nblk + 1), dict(N=c["n"] + 1), dict(C=c["cout"] + 16)):
            with pytest.raises(RuntimeError, match=who + ": tail descriptor does not match the launch"):
                run_conv_tail(ops, name, kind, {}, groups, tail_override=over)
    with pytest.raises(RuntimeError, match="conv3_sb: tail descriptor does not match the launch"):          # the one-stage kernel hosts kind 1 only
        run_conv_tail(ops, "sb_24_scale_add_stats_real", 2, {}, 8)
    with pytest.raises(RuntimeError, match=r"conv3_f32c: forward convolution only \(no residual / fused backward sums / split-form input / tail\)"):
        run_conv_tail(ops, "f32c_48_scale_stats_real", 1, {}, 8)
    with pytest.raises(RuntimeError, match="the tail finalizes the statistics of this launch"):
        run_conv_tail(ops, "sb2_16_add_stats_real", 1, dict(stats=False), 8)


# ====================================================================================================================== b. chain consistency
@pytest.mark.parametrize("tag", ["real", "exact"])
def test_constants_the_finalize_writes_are_the_ones_the_fused_kernels_expect(ops, tag):
    """Forward convolution with statistics -> ops.gn_finalize (mean / rstd / scale / shift / bst_k) -> the data-gradient convolution with the fused GroupNorm-backward
    sums (bst_y = the forward output, bst_k = what the finalize wrote) -> ops.gn_bwd_finalize(s2_sign = 1) -> the weight gradient with the fused apply (gb_coef =
    what that finalize wrote).  Every constant is the device's own; the end of the chain -- dgamma, dbeta, the published dy of the GroupNorm backward and the dw formed
    from it -- is compared with the float64 reference of the whole chain on the device's stored tensors: dgamma / dbeta at this file's bars, the published tensor at
    the split form's bar on top of the bar of dx, dw at the three-product bar of tests/test_wgrad3_fused_host.py (2e-5 of the largest value)."""
    import test_conv3_fused as TC
    fwd, bwd = CASE_BY_NAME["sb2_16_add_stats_" + tag], CASE_BY_NAME["dgrad_split_16_b1_a0_" + tag]
    fi, _ = TC.shared(fwd)
    bi, _ = TC.shared(bwd)
    slope = TC.case_slope(fwd)
    rng = np.random.default_rng(5)
    gamma, beta = H.exact_params("zeros", 16, rng) if tag == "exact" else H.gn_param_set("zeros", 16, rng)
    v = int(np.prod(fwd["dhw"]))
    f = TC.launch(fwd, fi)                                                             # y1 = conv(x) + add, statistics of y1
    y1 = TC.host(f.y, True)
    if tag == "real":                                                                  # stored values on the LeakyReLU kink of (gamma, beta) are moved off it through `add`
        fi = dict(fi, add=(fi["add"] + (H.gn_off_the_kink(y1, gamma, beta) - y1)).astype(np.float32))
        f = TC.launch(fwd, fi)
        y1 = TC.host(f.y, True)
    assert np.array_equal(H.gn_off_the_kink(y1, gamma, beta), y1)
    st = ops.gn_finalize(f.partials, dev(gamma), dev(beta), v, want_k=True)
    want = H.stats_of(y1, gamma, beta)
    if tag == "real":
        check_stats("chain forward statistics", st, want, gamma, beta, group="chain")
    # the data gradient of the NEXT convolution arrives at this GroupNorm's activation: d = conv_dgrad(g) with the fused sums over (y1, d)
    b = TC.launch(bwd, bi, bst_y=f.y, bst_k=st.bst_k, bst_slope=slope)
    assert ops.conv3_route(b.route).bst
    d = TC.host(b.y, True)
    co = ops.gn_bwd_finalize(b.partials, dev(gamma), st.mean, st.rstd, v, 1)
    ref = H.ref_chain(y1, gamma, beta, d, slope)
    x = c16(fi["x"])
    wg = ops.wgrad3_fused(x, None, gb_y=f.y, gb_d=b.y, gb_scale=st.scale, gb_shift=st.shift, gb_coef=co.coef, gb_slope=slope, gb_out=True)
    dy64 = H.blocks(ref["dx"])
    dec = split_decode(wg.gb_out.contiguous().view(torch.uint8).cpu().numpy().reshape(dy64.shape[:-1] + (64,)))
    from test_wgrad3_fused_host import pad0, wgrad_padded
    dw64 = wgrad_padded(pad0(np.asarray(fi["x"], np.float64)), ref["dx"])
    if tag == "exact":
        S = H.ref_bwd_sums(y1, d, want["scale"], want["shift"], want["mean"], want["rstd"], slope, gamma=gamma)
        # the fused sums use the device's float32 statistics (mean, rstd are not dyadic here): the sums of dh are exact, the others meet the bar
        assert np.array_equal(b.partials.double().sum(2).cpu().numpy()[..., 0], S[..., 0])
        assert np.array_equal(co.dbeta.double().cpu().numpy(), ref["dbeta"])
    worst = max(excess_rel_max(co.dgamma, ref["dgamma"]), excess_rel_max(co.dbeta, ref["dbeta"]), excess_coef(co.coef, ref["coef"]))
    assert note("chain", tag + " dgamma / dbeta / coef", worst) <= 1.0
    fr = H.blocks(H.ref_dx_rounding(y1, d, ref["scale"], ref["shift"], ref["coef"], slope))
    bar = 1e-4 * np.abs(dy64) + 5e-6 + 2.0 ** -16 * (np.abs(dy64) + fr) + fr
    assert note("chain", tag + " published dy", float((np.abs(dec - dy64) / bar).max())) <= 1.0
    assert note("chain", tag + " dw of the fused apply", dw_excess(wg.dw.cpu().numpy(), dw64, 3)) <= 1.0


# ====================================================================================================================== e. conditioning of the (sum, sumsq) form
def test_sum_sumsq_statistics_conditioning(golden, ops):
    """The C16 counterpart of test_group_norm_statistics_conditioning: a centre-tap identity 16 -> 16 weight with the constant mu joined in the store (`add`: the voxel-major
    split-bf16 kernels take no bias beside statistics) makes the persistent convolution of the shipped path store x + mu and publish the per-workgroup float32 (sum, sumsq)
    of what it stored; ops.gn_finalize combines them in float64.  Error of rstd and of the applied y against float64 beside float32
    torch.native_group_norm on the CPU, at mu / sigma of GN_RATIOS.  Rule (the existing test's): up to the asserted ratio ours stays within 4x the float32 CPU reference's
    plus 1e-6.  Measured on the first device run (profiles/gn_conditioning.txt): the rule holds at every listed ratio up to 10 R = 20.3 (0, 3, 10) and no longer at 30, where
    the float32 sumsq of a workgroup has lost the variance's low bits (rstd 6.4e-6 against 7.1e-8); DESIGN.md states the limit.  Larger ratios are printed only."""
    R = gn_fixture_ratio(golden)
    assert np.isfinite(R) and R > 0
    n, c, sp = 2, 16, (30, 30, 60)
    v = int(np.prod(sp))
    rng = np.random.default_rng(20)
    z = rng.standard_normal((n, c) + sp).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
    w = np.zeros((16, 16, 3, 3, 3), np.float32)
    w[np.arange(16), np.arange(16), 1, 1, 1] = 1.0
    limit = 10 * R
    print("\n  R = %.4f, asserted up to mu/sigma = %g\n  mu/sigma   rstd error (ours, f32 CPU)   y error (ours, f32 CPU)   asserted" % (R, limit))
    failures = []
    for ratio in GN_RATIOS:
        r = ops.conv3_fused(c16(z), dev(w), add=c16(np.full_like(z, ratio)), in_c16=True, out_c16=True, stats=True)
        assert ops.conv3_route(r.route).family == "sb2"
        x = H.unblocks(r.y.cpu().numpy())                                             # the statistics are those of the STORED tensor: it is the GroupNorm's input
        assert float(np.abs(x - (z + np.float32(ratio))).max()) <= 2.0 ** -14 * (4.5 + ratio)
        y64, _, rstd64 = H.O.np_group_norm(x, gamma, beta)
        yc, _, rc = torch.native_group_norm(torch.from_numpy(x), torch.from_numpy(gamma), torch.from_numpy(beta), n, c, v, H.G, H.O.GN_EPS)
        st = ops.gn_finalize(r.partials, dev(gamma), dev(beta), v)
        yh = H.unblocks(ops.gn_apply_c16(r.y, st.scale, st.shift, 1.0).cpu().numpy())
        e_r = lambda t: float(np.abs(t.cpu().numpy().astype(np.float64).ravel() - rstd64.ravel()).max() / rstd64.max())
        e_y = lambda y: float(np.abs(np.asarray(y, np.float64) - y64).max() / np.abs(y64).max())
        row = (e_r(st.rstd), e_r(rc), e_y(yh), e_y(yc.numpy()))
        asserted = ratio <= limit
        print("  %8g   %.2e  %.2e          %.2e  %.2e      %s" % ((ratio,) + row + ("yes" if asserted else "no",)))
        if asserted and not (row[0] <= 4 * row[1] + 1e-6 and row[2] <= 4 * row[3] + 1e-6):
            failures.append((ratio, row))
    assert not failures, failures

