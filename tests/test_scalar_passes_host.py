"""The float64 restatements that tests/test_scalar_passes.py holds the scalar-producing passes to -- the criterion's sums, value and gradient, the Dice counts and
their accumulation, the z-score and case moments -- and the flat, layout and merge passes beside them; that file's cases, inputs and bars; and the proof, on the CPU
alone, that (a) the restatements are the reference's operations, (b) the exact families are exact and (c) the bars and equalities can fail.

Kernels (csrc/pointwise.hip, csrc/inference.hip):
  crit_partial_kernel / crit_final_kernel    sums [2C + 1] = (sum p g, sum p^2 + g per class, sum g log(p + 1e-6f) + bgw (1 - g) log((1 + 1e-6)f - p)) = O.np_dice_bce_sums
  crit_value_kernel, ru_criterion_value      (w_dice dice + w_bce bce, dice, bce) from the sums = O.np_criterion_from_sums (float64, about ten operations: relative 1e-14)
  crit_grad_kernel                           d(w_dice Dice + w_bce BCE) / dp = O.np_criterion_grad
  dice_counts_kernel, dice_accumulate_kernel counts (#(p > .5 & g > .5), #(p > .5) + #(g > .5)) as integers; acc[c] += mean over n of the float32 ratio, NaN -> 1 = O.dice_metric
  zscore_partial / case_stats_partial (+ final)   per channel count(x > 0), sum x, sum x^2 over all voxels (of the box), float64 = the moments of O.zscore_positive
  ew_kernel<EW_SIGMOID / EW_LRELU / EW_LRELU_BWD>, layout_convert_kernel, tta_merge(_box)_kernel, compose_labels_kernel

Exact family (sums).  p in {1/4, 1/2, 3/4}, g in {0, 1}: p g is a multiple of 1/4 and p p + g of 1/16, and a tile of 8192 holds at most 8192 * 1.5625 = 12800 < 2^24 / 16:
every partial sum of a tile, in any order, with or without a fused multiply-add, is a float32 value (assert_exact checks the two premises), and the float64 sums of the
tiles are exact too.  inter and union must equal the float64 restatement bit for bit.  The BCE sum has no exact family; it is held by its bar on both.

Real family (sums, gradient).  p = sigmoid(12 z) in float32 (about 7 % of them exactly 1.0f), 0, 1, 2^-24, 1 - 2^-24 and 1/2 planted at the start of every row, p = 0 with
g = 1 in the last 256 voxels of every full 8192-voxel tile (the last of a thread's 32 strides: a dropped stride loses 256 from the union and 256 log(1e-6) from the BCE
sum), targets in {0, 1} with class 1 all zero and class 2 all one where C >= 3, a soft variant with g uniform in [0, 1] (distillation), bg_weight in {1e-2, 1, 0}.

Bars.  bar = r * 2^-24 * sum |term| of that output (+ r 2^-126); r = the float32 roundings on the longest path of crit_partial_kernel AS WRITTEN, a thread's serial sum over
its 32 strides (31: the first add is onto 0), block_sum (9: 6 shuffle levels and buf[0] + buf[1] + buf[2] + buf[3]) and 1 for crit_final_kernel's float64 combine:
  R_INTER = 42     the product (1) + 31 + 9 + 1
  R_UNION = 43     p p and + g (2) + 31 + 9 + 1
  R_BCE   = 46 + LOGF_UNITS   the longer term bgw (1 - g) log(b): the cast of bg_weight to float (1), 1 - g (1: inexact for a soft g < 1/2), the two products (2), the add of
                   the two terms (1), the error of logf (LOGF_UNITS), + 31 + 9 + 1.  The log arguments p + 1e-6f and (1 + 1e-6)f - p are NOT counted: the oracle forms them
                   in float32 too.
  LOGF_UNITS, EXPF_UNITS = 5, 3   the worst error of the device's logf / expf in units of 2^-24 |y| (half an ulp at the bottom of a binade, a whole one at its top),
                   measured against float64 log / exp by a stand-alone program built with the library's flags on every argument these tests hand the two functions
                   (853 364 and 7 931 419 distinct ones) -- logf 3.13 (2.14 ulp, at x = 0.018077), expf 1.39 (0.84 ulp) -- rounded up, plus one: a correctly rounded
                   reference against a faithfully rounded function.  Never taken from the kernels under test.
  gradient         R_D_CRIT = 10 of tests/test_up2_head_host.py and its expression |kg g| + |kp p| + cb (g / a + bgw (1 - g) / b), without the p (1 - p) factors
  sigmoid          (EXPF_UNITS + 2) 2^-24 |y| + 2^-126: expf, 1 + e and the division (|dy/de| e <= y)
  moments          (V / 256 + 12) 2^-53 sum |term|: a thread's serial sum, block_sum_d, the chunk sum; the count is exact.  The restatement's own sums are math.fsum's
                   (correctly rounded), so nothing of the bar is spent on the reference
Everything else is an equality: integers (counts, masks, labels), bit patterns (LeakyReLU against torch on the CPU, the layouts, the merge's float32 mean in the reference's
order), and the float32 restatement of dice_accumulate_kernel.

emulate_sums restates crit_partial_kernel's ORDER in numpy float32 (strides, shuffle tree, serial wave sums; numpy's float32 log, unfused): it is bit-equal to float64 on the
exact family and stays inside the bars on the real one (worst error / bar 0.044), so the bars are not tighter than the kernel as written can meet.

Mutants: test_mutants_exceed_the_bars_of_the_gpu_tests applies each listed error to the restatement on the GPU file's own inputs.  Nothing here needs a GPU."""
import math

import numpy as np
import pytest
import torch

import test_up2_head_host as HH
from oracle import resunet_oracle as O
from test_up2_head_host import PLANT, R_D_CRIT, TINY, U, assert_exact, case_id, excess

U64 = 2.0 ** -53
CR_CHUNK = 8192                                     # csrc/pointwise.hip: voxels per criterion partial (the moments' chunks, ZS_CHUNK and CS_CHUNK, are 16384)
LOGF_UNITS, EXPF_UNITS = 5, 3
R_INTER, R_UNION, R_BCE = 1 + 31 + 9 + 1, 2 + 31 + 9 + 1, 5 + LOGF_UNITS + 31 + 9 + 1
BGW = HH.BGW
COUNT_FACTOR = HH.COUNT_FACTOR
GUARD_WORDS = 1024                                  # what the GPU file keeps behind every layout output
NAN_BITS = 0x7FC00000                               # what it fills the output and the guard with

# ---------------------------------------------------------------------------------------------------------------- cases (tests/test_scalar_passes.py runs exactly these)
SUM_CASES = [(1, 1, 1), (1, 3, 255), (1, 3, 257), (2, 3, 8191), (2, 3, 8192), (2, 3, 8193), (3, 5, 2 * 8192 + 1), (1, 1, 3 * 8192)]
SUM_VARIANTS = [("hard", 1e-2), ("hard", 1.0), ("hard", 0.0), ("soft", 1e-2)]           # (targets, bg_weight)
GRAD_CASES = [(2, 5, 1001), (1, 3, 8193), (1, 1, 4096 * 256 + 5)]
VALUE_WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.5, 0.5)]
DICE_V = [1, 3, 4, 5, 1023, 1024, 8193, 524288 + 8192 + 4, 524288 + 8192 + 1]
DICE_ROWS = [(1, 1), (2, 3)]
ZS_CASES = [(c, v) for c in (1, 4) for v in (1, 16383, 16384, 16385, 3 * 16384 + 7)]
BOX_SMALL = (7, 9, 11)
BOXES_SMALL = [((0, 0, 0), (7, 9, 11)), ((0, 0, 0), (1, 1, 1)), ((6, 8, 10), (1, 1, 1)), ((1, 2, 3), (4, 1, 5)), ((3, 4, 5), (4, 5, 6))]
BOX_LARGE, BOXES_LARGE = (42, 41, 23), [((1, 1, 2), (40, 40, 21))]                    # 33600 voxels: three chunks of 16384
CASE_STATS_CASES = [(4, BOX_SMALL, lo, size) for lo, size in BOXES_SMALL] + [(1, BOX_SMALL) + BOXES_SMALL[0]] + [(4, BOX_LARGE, lo, size) for lo, size in BOXES_LARGE]
FLAT_N = [1, 1023, 1025, 8192 * 1024 + 1029]        # the last passes the 8192-workgroup cap of the flat launches
FLAT_PLANT = [0.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0, float("inf"), float("-inf"), float("nan")]
SLOPE = 0.01
LAYOUT_CASES = [(2, 32, v) for v in (1, 63, 64, 65)]
MERGE_SHAPE = (3, 5, 6, 7)
MERGE_FLIPS = {1: (7,), 2: (5, 2), 8: (0, 1, 2, 3, 4, 5, 6, 7)}       # per copy: bit 0 = D, bit 1 = H, bit 2 = W reversed; every combination occurs
MERGE_BOXES = [((4, 5, 6), (1, 1, 1)), ((2, 1, 3), (3, 5, 4))]
ET_MIN = 32


def _seed(case, salt):
    return HH._seed(tuple(int(v) for v in np.ravel(case)), salt)


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same_f64(got, ref):
    """a float64 device result is the float64 restatement, bit for bit (NaN never equals)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return got.shape == ref.shape and bool(np.array_equal(got, ref))


# ---------------------------------------------------------------------------------------------------------------- criterion: sums
def last_stride(v):
    """the voxels a thread reads in the last of its 32 strides of a tile: [7936, 8192) of every full tile"""
    idx = [np.arange(t + CR_CHUNK - 256, t + CR_CHUNK) for t in range(0, v, CR_CHUNK) if t + CR_CHUNK <= v]
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def crit_inputs(case, family, targets="hard"):
    """(p, g) [N, C, V] float32 numpy"""
    n, c, v = case
    rng = np.random.RandomState(_seed(case, (11 if family == "real" else 12) + (2 if targets == "soft" else 0)))
    g = (rng.rand(n, c, v) < 0.3).astype(np.float32)
    idx = last_stride(v)
    if family == "exact":
        assert targets == "hard"
        p = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=(n, c, v))
    else:
        p = torch.sigmoid(torch.from_numpy(rng.randn(n, c, v).astype(np.float32) * 12.0)).numpy()
        if targets == "soft":
            g = rng.rand(n, c, v).astype(np.float32)
        plant = np.array(PLANT, np.float32)
        for r in range(n * c):
            p[r // c, r % c, :min(v, 5)] = np.roll(plant, r)[:min(v, 5)]
        p[:, :, idx] = 0.0
    g[:, :, idx] = 1.0
    if targets == "hard" and c >= 3:
        g[:, 1], g[:, 2] = 0.0, 1.0
    return p, g


def sum_terms(p, g, bgw, mutant=None):
    """the elements of the three sums [3, N, C, V] float64, as O.np_dice_bce_sums forms them.  mutant: 'one_eps' (1 + 1e-6 taken in float64), 'bgw_fg' (bg_weight on
    the foreground term)"""
    p32 = np.asarray(p, np.float32)
    p64, g = p32.astype(np.float64), np.asarray(g, np.float64)
    a = (p32 + np.float32(1e-6)).astype(np.float64)
    b = (1.0 + 1e-6) - p64 if mutant == "one_eps" else (np.float32(1.0 + 1e-6) - p32).astype(np.float64)
    fg, bg = g * np.log(a), (1.0 - g) * np.log(b)
    return np.stack([p64 * g, p64 * p64 + g, bgw * fg + bg if mutant == "bgw_fg" else fg + bgw * bg])


def ref_sums(p, g, bgw, mutant=None):
    """[2C + 1] float64.  None: the oracle itself.  mutant: sum_terms', 'stride' (the last stride of every tile dropped), 'swap_nc' (crit_final_kernel reading the
    partial of (n, c) at (c N + n) instead of (n C + c))"""
    if mutant is None:
        inter, union, bce = O.np_dice_bce_sums(p, g, bgw)
        return np.concatenate([inter, union, [bce]])
    n, c, v = np.asarray(p).shape
    t = sum_terms(p, g, bgw, mutant)
    if mutant == "stride":
        t = np.delete(t, last_stride(v), axis=3)
    rows = t.sum(3).reshape(3, n * c)
    if mutant == "swap_nc":
        per = np.stack([rows[:, [cc * n + nn for nn in range(n)]].sum(1) for cc in range(c)], 1)
    else:
        per = rows.reshape(3, n, c).sum(1)
    return np.concatenate([per[0], per[1], [per[2].sum()]])


def sums_bars(p, g, bgw):
    p32 = np.asarray(p, np.float32)
    p64, g = p32.astype(np.float64), np.asarray(g, np.float64)
    a = (p32 + np.float32(1e-6)).astype(np.float64)
    b = (np.float32(1.0 + 1e-6) - p32).astype(np.float64)
    mag = [np.abs(p64 * g).sum((0, 2)), (p64 * p64 + g).sum((0, 2)), np.array([(np.abs(g * np.log(a)) + np.abs(bgw * (1.0 - g) * np.log(b))).sum()])]
    return np.concatenate([r * (U * m + TINY) for r, m in zip((R_INTER, R_UNION, R_BCE), mag)])


def _block_sum32(x):
    """pw_helpers.hpp's block_sum on [..., 256] float32: the xor-shuffle tree of each wave, then buf[0] + buf[1] + buf[2] + buf[3]"""
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., (lane & ~63) | ((lane & 63) ^ o)]
    return ((x[..., 0] + x[..., 64]) + x[..., 128]) + x[..., 192]


def emulate_sums(p, g, bgw):
    """crit_partial_kernel + crit_final_kernel in their own order, numpy float32 (unfused; numpy's float32 log)"""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    n, c, v = p.shape
    nblk = -(-v // CR_CHUNK)
    pad = nblk * CR_CHUNK - v
    pp, gg = (np.pad(t, ((0, 0), (0, 0), (0, pad))).reshape(n, c, nblk, 32, 256) for t in (p, g))
    live = np.pad(np.ones((n, c, v), bool), ((0, 0), (0, 0), (0, pad))).reshape(n, c, nblk, 32, 256)
    one_eps, w = np.float32(1.0 + 1e-6), np.float32(bgw)
    with np.errstate(divide="ignore", invalid="ignore"):
        tb = gg * np.log(pp + np.float32(1e-6)) + w * (np.float32(1.0) - gg) * np.log(one_eps - pp)
    part = []
    for t in (pp * gg, pp * pp + gg, tb):
        t = np.where(live, t, np.float32(0.0)).astype(np.float32)
        acc = t[..., 0, :]
        for s in range(1, 32):
            acc = acc + t[..., s, :]
        part.append(_block_sum32(acc).astype(np.float64))
    si, su, sb = (q.sum((0, 2)) for q in part)
    return np.concatenate([si, su, [sb.sum()]])


# ---------------------------------------------------------------------------------------------------------------- criterion: value
def value_cases():
    """dicts (name, shards [3, 2C + 1] -- the sums of three ranks --, sums = their sum, c, count, priority)"""
    out = []
    for c, priority in ((1, 1.0), (3, 1.0), (64, 1.0), (3, 1.5)):
        rng = np.random.RandomState(300 + c + int(10 * priority))
        union = rng.uniform(50.0, 500.0, size=(3, c))
        inter = union * rng.uniform(0.1, 0.4, size=(3, c))          # 2 I / U in [0.2, 0.8]: the Dice term is not a small difference
        shards = np.concatenate([inter, union, -rng.uniform(1e3, 1e4, size=(3, 1))], 1)
        out.append(dict(name="C%d_priority%g" % (c, priority), shards=shards, sums=shards.sum(0), c=c, count=12345.0 * c, priority=priority))
    out.append(dict(name="C3_zero", shards=np.zeros((3, 7)), sums=np.zeros(7), c=3, count=7.0, priority=1.0))
    return out


def ref_value(case, w_dice, w_bce, mutant=None):
    """(w_dice dice + w_bce bce, dice, bce) float64.  mutant 'eps_before': the epsilons added to every rank's sums before they are reduced"""
    c = case["c"]
    s = case["sums"]
    if mutant == "eps_before":
        k = len(case["shards"])
        s = s + np.concatenate([np.full(c, (k - 1) * 1e-6), np.full(c, (k - 1) * 2e-6), [0.0]])
    _, dice, bce = O.np_criterion_from_sums(s[:c], s[c:2 * c], s[2 * c], case["count"], case["priority"])
    return np.array([w_dice * dice + w_bce * bce, dice, bce])


def rel_excess(got, ref, tol=1e-14):
    """max |got - ref| / (tol |ref|); equal values (0 against 0) count as 0"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0.0, 0.0, d / (tol * np.abs(ref))).max())


# ---------------------------------------------------------------------------------------------------------------- criterion: gradient
def grad_inputs(case):
    """dict(p, g [N, C, V] float32, sums [2C + 1] float64, count): the real family, global count = 3 x the shard's elements"""
    p, g = crit_inputs(case, "real")
    return dict(p=p, g=g, sums=ref_sums(p, g, BGW), count=float(COUNT_FACTOR * p.size))


def ref_grad(inp, mutant=None):
    """(dp float64 -- the oracle's closed form --, bar)"""
    c = inp["p"].shape[1]
    terms = HH.crit_terms(inp["p"], inp["g"], inp["sums"], inp["count"], bgw=BGW, mutant=mutant)
    dp = O.np_criterion_grad(inp["p"], inp["g"], inp["sums"][:c], inp["sums"][c:2 * c], inp["count"], BGW) if mutant is None else terms.sum(0)
    return dp, R_D_CRIT * (U * np.abs(terms).sum(0) + TINY)


# ---------------------------------------------------------------------------------------------------------------- Dice metric
DICE_PLANT = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), np.nan, np.inf, -0.0], np.float32)
DICE_QUIET = np.array([0.5, np.nan, -0.0, 0.25, 0.5], np.float32)                      # the empty row's: nothing of it counts


def dice_inputs(rows, v):
    """(p, g) [N, C, V] float32: row 0 of density 0.3 with the planted values at both ends, 1 empty (0.5, NaN, -0.0, 0.25 only), 2 full, 3-5 of density 0.05, 0.9, 0.5"""
    n, c = rows
    rng = np.random.RandomState(_seed((n, c, v), 21))
    dens = [0.3, 0.0, 1.0, 0.05, 0.9, 0.5]
    p, g = np.empty((n * c, v), np.float32), np.empty((n * c, v), np.float32)
    for r in range(n * c):
        for t, salt in ((p, 0), (g, 2)):
            t[r] = np.where(rng.rand(v) < dens[r], 0.5 + 0.5 * rng.rand(v) + 1e-3, 0.5 * rng.rand(v)).astype(np.float32)
            plant = np.roll(DICE_QUIET if r == 1 else DICE_PLANT, r + salt)
            k = min(v, 5)
            t[r, :k] = plant[:k]
            if v >= 10:
                t[r, v - 5:] = plant[::-1]
    if n * c > 2:
        for t in (p, g):
            t[2] = np.where(np.isnan(t[2]) | (t[2] <= 0.5), np.float32(0.75), t[2])      # the full row: every voxel counts
    return p.reshape(n, c, v), g.reshape(n, c, v)


def ref_counts(p, g, mutant=None):
    """[N, C, 2] int64.  mutant: 'ge' (>= 0.5), 'nan' (NaN counted: !(x <= 0.5))"""
    with np.errstate(invalid="ignore"):
        if mutant == "ge":
            a, b = p >= 0.5, g >= 0.5
        elif mutant == "nan":
            a, b = ~(p <= 0.5), ~(g <= 0.5)
        else:
            a, b = p > 0.5, g > 0.5
    return np.stack([(a & b).sum(-1), a.sum(-1) + b.sum(-1)], -1).astype(np.int64)


def ref_accumulate(counts, acc, nacc, mutant=None):
    """dice_accumulate_kernel in numpy float32: (float)count, 2 num / den in float32, NaN -> 1, the mean over n and the add in float64; acc[nacc:] untouched.
    mutant 'den0': den = 0 -> 0"""
    counts = np.asarray(counts, np.int64)
    n = counts.shape[0]
    out = np.array(acc, np.float64)
    for c in range(nacc):
        s = 0.0
        for i in range(n):
            num, den = np.float32(counts[i, c, 0]), np.float32(counts[i, c, 1])
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.float32(2.0) * num / den
            if np.isnan(r):
                r = np.float32(0.0 if mutant == "den0" else 1.0)
            s += float(r)
        out[c] += s / n
    return out


def accumulate_cases():
    """dicts (name, counts [N, C, 2] int64, nacc): den = 0 in class 0, counts past 2^24 in class 2, nacc < C"""
    rng = np.random.RandomState(31)
    small = ref_counts(*[(rng.rand(3, 4, 50) < d).astype(np.float32) for d in (0.4, 0.6)])
    small[:, 0] = 0
    big = small.copy()
    big[0, 2], big[1, 2], big[2, 2] = (2 ** 24 + 1, 2 ** 25 + 2), (2 ** 24 + 3, 2 ** 26 + 4), (2 ** 24 + 1, 2 ** 25 + 6)
    return [dict(name="small", counts=small, nacc=3), dict(name="big", counts=big, nacc=3), dict(name="all", counts=small, nacc=4),
            dict(name="one_sample", counts=small[:1].copy(), nacc=1)]


def accumulate_start(c):
    """acc before the first call: distinct finite values, so that a touched entry past nacc shows by bit pattern"""
    return 0.125 + 0.25 * np.arange(c, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- moments
SUBNORMAL = np.float32(1e-45)
ZS_PLANT = np.array([SUBNORMAL, -0.0, 0.0, -3.5, 7.25], np.float32)


def zs_inputs(c, v):
    """[C, V] float32: 40 % zeros, 5 % negatives, the planted values at the start of every channel; of four channels, channel 1 has no positive voxel and channel 3
    is 1000 + N(0, 1)"""
    rng = np.random.RandomState(_seed((c, v), 41))
    x = np.where(rng.rand(c, v) < 0.4, 0.0, np.abs(rng.randn(c, v)) * 300.0 + 1.0)
    x = np.where(rng.rand(c, v) < 0.05, -np.abs(rng.randn(c, v)) * 20.0, x).astype(np.float32)
    for ch in range(c):
        x[ch, :min(v, 5)] = np.roll(ZS_PLANT, -ch)[:min(v, 5)]
    if c == 4:
        x[1] = -np.abs(x[1])
        x[3] = (1000.0 + rng.randn(v)).astype(np.float32)
    return x


def ref_moments(x, mutant=None):
    """x [C, V] float32 -> [C, 3] float64 = count(x > 0), sum x, sum x^2, each sum correctly rounded (math.fsum; x^2 is exact in float64).  mutant 'ge': count(x >= 0)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    x = x.reshape(x.shape[0], -1)
    cnt = (x >= 0).sum(1) if mutant == "ge" else (x > 0).sum(1)
    return np.stack([cnt.astype(np.float64), [math.fsum(r) for r in x], [math.fsum(r * r) for r in x]], 1)


def moments_bars(x):
    """[C, 3]: 0 for the count (exact), (V / 256 + 12) 2^-53 sum |term| for the two sums"""
    x = np.asarray(x, np.float32).astype(np.float64)
    x = x.reshape(x.shape[0], -1)
    r = x.shape[1] / 256.0 + 12.0
    return np.stack([np.zeros(x.shape[0]), r * U64 * np.abs(x).sum(1), r * U64 * (x * x).sum(1)], 1)


def moments_excess(got, ref, bar):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all() or not np.array_equal(got[:, 0], ref[:, 0]):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(got[:, 1:] - ref[:, 1:])
        return float(np.where(d == 0.0, 0.0, d / bar[:, 1:]).max())


def case_image(c, dims):
    return zs_inputs(c, int(np.prod(dims))).reshape((c,) + tuple(dims))


def crop(img, lo, size, mutant=None):
    """the box of img [C, D, H, W].  mutant 'origin': the x origin off by one (towards the inside of the volume; None where the box spans the axis)"""
    lo = list(lo)
    if mutant == "origin":
        if lo[2] + size[2] < img.shape[3]:
            lo[2] += 1
        elif lo[2] > 0:
            lo[2] -= 1
        else:
            return None
    return img[:, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]]


# ---------------------------------------------------------------------------------------------------------------- flat passes
def flat_inputs(n, salt=51):
    """[n] float32 of scale 6 with FLAT_PLANT at the start (and, reversed, at the end of the longer ones)"""
    rng = np.random.RandomState(_seed((n,), salt))
    x = (rng.randn(n) * 6.0).astype(np.float32)
    plant = np.roll(np.array(FLAT_PLANT, np.float32), salt - 51)
    x[:min(n, 10)] = plant[:min(n, 10)]
    if n >= 20:
        x[n - 10:] = plant[::-1]
    return x


def lrelu_inputs(n):
    """(y, dy) [n] float32 with +-0, NaN and +-inf planted in both, against each other"""
    y, dy = flat_inputs(n, 52), flat_inputs(n, 53)
    k = min(n, 3)
    y[:k], dy[:k] = np.array([-0.0, 0.0, -0.0], np.float32)[:k], np.array([0.0, -0.0, -3.0], np.float32)[:k]
    return y, dy


def ref_sigmoid(x, mutant=None):
    """(y float64, bar); NaN where x is.  mutant 'plus': 1 / (1 + exp(+x))"""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(x if mutant == "plus" else -x))
    return y, (EXPF_UNITS + 2) * U * np.abs(y) + TINY


def sigmoid_excess(got, x):
    """max |got - y| / bar over the numbers; inf unless got is NaN exactly where x is"""
    y, bar = ref_sigmoid(x)
    got = np.asarray(got, np.float64)
    nan = np.isnan(np.asarray(x, np.float32))
    if got.shape != y.shape or not np.array_equal(np.isnan(got), nan) or not np.isfinite(got[~nan]).all():
        return float("inf")
    return float((np.abs(got - y)[~nan] / bar[~nan]).max())


def ref_lrelu(x, slope=SLOPE):
    return torch.nn.functional.leaky_relu(torch.from_numpy(np.asarray(x, np.float32)), slope).numpy()


def ref_lrelu_bwd(y, dy, slope=SLOPE):
    y, dy = torch.from_numpy(np.asarray(y, np.float32)), torch.from_numpy(np.asarray(dy, np.float32))
    return torch.where(y > 0, dy, dy * slope).numpy()


# ---------------------------------------------------------------------------------------------------------------- layout
LAYOUT_PLANT = np.array([0x7FC12345, -0x003FFFFF, 0x7F800001, -0x80000000], np.int64).astype(np.int32)      # NaN payloads (quiet, negative, signalling) and -0.0


def layout_inputs(case):
    """[N, C, V] int32 bit patterns of seeded floats with LAYOUT_PLANT spread over them"""
    n, c, v = case
    rng = np.random.RandomState(_seed(case, 61))
    x = bits32(rng.randn(n, c, v)).copy().reshape(-1)
    x[::7][:4 * (x[::7].size // 4)] = np.tile(LAYOUT_PLANT, x[::7].size // 4)
    return x.reshape(n, c, v)


def ref_layout(src, case, to_c16, mutant=None):
    """layout_convert_kernel on bit patterns: src flat int32 (NCDHW [N, C, V] or voxel-major [N, C/16, V, 16]) -> the other layout, flat, followed by GUARD_WORDS
    of the fill.  mutant 'unclipped': the tile of 64 voxels not clipped at V (what it reads past the tensor is 0, what it writes lands where the buffer goes on)"""
    n, c, v = case
    src = np.concatenate([np.asarray(src, np.int32).reshape(-1), np.zeros(64 * 16, np.int32)])
    out = np.full(n * c * v + GUARD_WORDS, np.int32(NAN_BITS))
    ch = np.arange(16)[:, None]
    for nb in range(n * (c // 16)):
        for v0 in range(0, v, 64):
            vv = v0 + np.arange(64 if mutant == "unclipped" else min(64, v - v0))[None, :]
            plane, major = nb * 16 * v + ch * v + vv, nb * 16 * v + vv * 16 + ch
            rd, wr = (plane, major) if to_c16 else (major, plane)
            out[wr] = src[rd]
    return out


def torch_layout(x, case, to_c16):
    """the same permutation by torch indexing (int32)"""
    n, c, v = case
    x = torch.from_numpy(np.asarray(x, np.int32).reshape(-1).copy())
    if to_c16:
        return x.reshape(n, c // 16, 16, v).permute(0, 1, 3, 2).reshape(-1).numpy()
    return x.reshape(n, c // 16, v, 16).permute(0, 1, 3, 2).reshape(-1).numpy()


# ---------------------------------------------------------------------------------------------------------------- inference merge
def _axes(f):
    return tuple(ax for ax, bit in ((1, 1), (2, 2), (3, 4)) if f & bit)


def flips_word(flips):
    return sum(int(f) << (3 * k) for k, f in enumerate(flips))


def merge_inputs(k):
    """probs [K, C, D, H, W] float32: copy k is the prediction of the input flipped by MERGE_FLIPS[K][k]; un-flipped, voxel (c, 1, 2, 3) is 1/2 in every copy
    (mean exactly 1/2: off) and (c, 3, 2, 1) is nextafter(1/2, 1) in every copy (K = 1, 2, 8: the sum is exact, the mean is on)"""
    c, d, h, w = MERGE_SHAPE
    rng = np.random.RandomState(_seed((k,) + MERGE_SHAPE, 71))
    u = rng.rand(k, c, d, h, w).astype(np.float32)
    u[:, :, 1, 2, 3] = 0.5
    u[:, :, 3, 2, 1] = np.nextafter(np.float32(0.5), np.float32(1.0))
    return np.stack([np.ascontiguousarray(np.flip(u[i], _axes(f))) if f else u[i] for i, f in enumerate(MERGE_FLIPS[k])])


def ref_merge(probs, flips, mutant=None):
    """(mean float32 [C, D, H, W], mask uint8, counts int64 [C]): O.tta_merge's float32 left-to-right sum / K for any flips.  mutant: 'div4', 'flip_w' (the W bit
    ignored)"""
    probs = np.asarray(probs, np.float32)
    un = [np.flip(o, _axes(f & 3 if mutant == "flip_w" else f)) if f else o for o, f in zip(probs, flips)]
    acc = un[0]
    for o in un[1:]:
        acc = acc + o
    mean = (acc / np.float32(4 if mutant == "div4" else len(un))).astype(np.float32)
    mask = (mean > 0.5).astype(np.uint8)
    return mean, mask, mask.reshape(mask.shape[0], -1).sum(1).astype(np.int64)


def box_of(t, lo, size):
    return np.ascontiguousarray(t[:, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]])


def label_inputs(n_et):
    """mask uint8 [3, 5, 6, 7] with exactly n_et ET voxels (some outside TC and WT), counts int64 [3]"""
    rng = np.random.RandomState(81)
    v = int(np.prod(MERGE_SHAPE[1:]))
    mask = np.zeros((3, v), np.uint8)
    mask[0] = rng.rand(v) < 0.6
    mask[1] = (rng.rand(v) < 0.5) & (mask[0] > 0)
    mask[2, rng.permutation(v)[:n_et]] = 1
    return mask.reshape((3,) + MERGE_SHAPE[1:]), mask.sum(1).astype(np.int64)


def ref_labels(mask, et_min=ET_MIN, mutant=None):
    """O.compose_labels on the masks (its rule is `> 32`: et_min = 32).  mutant 'ge': the ET count compared with >="""
    if mutant is None and et_min == 32:
        return O.compose_labels(mask.astype(np.float32))[0]
    out = np.zeros(mask.shape[1:], np.uint8)
    out[mask[0] > 0] = 2
    out[mask[1] > 0] = 1
    n_et = int(mask[2].sum())
    if (n_et >= et_min) if mutant == "ge" else (n_et > et_min):
        out[mask[2] > 0] = 4
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) the restatements are the reference's operations
def test_sum_restatement_is_the_oracle_and_its_terms_add_up_to_it():
    for case in [(2, 3, 8193), (1, 1, 1)]:
        for targets, bgw in SUM_VARIANTS:
            p, g = crit_inputs(case, "real", targets)
            ref = ref_sums(p, g, bgw)
            t = sum_terms(p, g, bgw)
            c = case[1]
            mine = np.concatenate([t[0].sum((0, 2)), t[1].sum((0, 2)), [t[2].sum()]])
            assert np.isfinite(ref).all() and ref.shape == (2 * c + 1,)
            assert np.abs(mine - ref).max() <= 1e-13 * (1.0 + np.abs(ref).max())
            assert np.abs(ref_sums(p, g, bgw, "none") - ref).max() <= 1e-12 * (1.0 + np.abs(ref).max())      # the mutants' own summation, unmutated


def test_value_restatement_is_the_oracle_and_the_criterion_of_the_probabilities():
    p, g = crit_inputs((2, 3, 257), "real")
    s = ref_sums(p, g, BGW)
    case = dict(sums=s, shards=s[None], c=3, count=float(p.size), priority=1.0)
    total, dice, bce = ref_value(case, 0.5, 0.5)
    assert (total, dice, bce) == O.np_criterion_from_sums(s[:3], s[3:6], s[6], float(p.size))
    loss = float(O.criterion(torch.from_numpy(p.astype(np.float64)), torch.from_numpy(g.astype(np.float64)), BGW))
    assert abs(total - loss) <= 1e-4 * abs(loss)                 # (O.criterion forms the log arguments in float64: at p = 1.0f, log(1e-6) against log(9.54e-7))
    zero = [c for c in value_cases() if c["name"] == "C3_zero"][0]
    assert np.array_equal(ref_value(zero, 0.5, 0.5), np.zeros(3))      # 2 (0 + 1e-6) / (0 + 2e-6) == 1 exactly: Dice loss 0


def test_gradient_restatement_is_the_oracle_within_a_hundredth_of_its_bar():
    inp = grad_inputs((2, 5, 1001))
    dp, bar = ref_grad(inp)
    mine = HH.ref_crit_dp(inp["p"], inp["g"], inp["sums"], inp["count"], bgw=BGW)
    assert np.isfinite(dp).all() and inp["count"] == 3.0 * inp["p"].size
    assert excess(mine, dp, bar) < 1e-2
    assert all((inp["p"] == np.float32(v)).any() for v in PLANT) and (inp["p"] == 1.0).mean() > 0.03


def test_dice_restatements_are_the_metric_of_the_oracle():
    p, g = dice_inputs((2, 3), 1023)
    counts = ref_counts(p, g)
    got = ref_accumulate(counts, np.zeros(3), 3)
    assert np.array_equal(got, O.dice_metric(p, g))
    assert counts[0, 1, 1] == 0 and ref_accumulate(counts[:1], np.zeros(3), 3)[1] == 1.0          # the empty row: NaN -> 1
    assert np.array_equal(counts[0, 2], [1023, 2046])            # the full row
    for case in accumulate_cases():
        c, n = case["counts"], case["nacc"]
        if case["name"] != "big":
            with np.errstate(invalid="ignore", divide="ignore"):
                d = (2 * c[..., 0].astype(np.float32) / c[..., 1].astype(np.float32)).astype(np.float64)
            d[np.isnan(d)] = 1.0
            assert np.array_equal(ref_accumulate(c, np.zeros(4), n)[:n], d.mean(0)[:n])
    big = accumulate_cases()[1]["counts"]
    assert np.float32(big[0, 2, 0]) == 2.0 ** 24 and np.float32(big[1, 2, 0]) == 2.0 ** 24 + 4 and np.float32(big[1, 2, 1]) == 2.0 ** 26        # (float)count rounds to even
    exact = 2.0 * big[1, 2, 0] / big[1, 2, 1]
    assert float(np.float32(2.0) * np.float32(big[1, 2, 0]) / np.float32(big[1, 2, 1])) != float(np.float32(exact))


@pytest.mark.parametrize("case", [(4, 16385), (1, 1), (4, 1)], ids=case_id)
def test_moment_restatement_gives_the_mean_and_std_of_the_oracle(case):
    c, v = case
    x = zs_inputs(c, v)
    m = ref_moments(x)
    assert np.array_equal(m[:, 0], (x > 0).sum(1)) and (x[0] == SUBNORMAL).any() and m[0, 0] >= 1          # the subnormal counts
    with np.errstate(invalid="ignore", divide="ignore"):
        _, mean, std = O.zscore_positive(x.reshape(c, 1, 1, v).astype(np.float64))      # (on a float32 array numpy squares in float32; the kernels square in float64)
        mine_mean = m[:, 1] / m[:, 0]
        mine_std = np.sqrt(m[:, 2] / m[:, 0] - mine_mean ** 2)
    ok = m[:, 0] > 0
    assert ok[0] and (c == 1 or not ok[1])                       # channel 1 of four: no positive voxel
    np.testing.assert_allclose(mine_mean[ok], mean[ok], rtol=1e-12)
    if v > 1:
        np.testing.assert_allclose(mine_std[ok], std[ok], rtol=1e-8)                  # (the oracle's variance is a difference of two rounded means)
    if c == 4 and v > 1:
        assert abs(mine_mean[3] - 1000.0) < 1.0 and abs(mine_std[3] - 1.0) < 0.1


def test_flat_and_layout_restatements():
    y, dy = lrelu_inputs(1025)
    ty, tdy = torch.from_numpy(y), torch.from_numpy(dy)
    aten = torch.ops.aten.leaky_relu_backward(tdy, ty, SLOPE, False).numpy()
    assert np.array_equal(bits32(ref_lrelu_bwd(y, dy)), bits32(aten))
    assert np.signbit(ref_lrelu(np.array([-0.0], np.float32)))[0] and np.isnan(ref_lrelu(flat_inputs(1025))).sum() == 2
    x = flat_inputs(1025)
    yy, _ = ref_sigmoid(x)
    assert np.array_equal(np.isnan(yy), np.isnan(x)) and sigmoid_excess(torch.sigmoid(torch.from_numpy(x).double()).numpy(), x) < 1e-3
    for case in LAYOUT_CASES:
        src = layout_inputs(case)
        n = int(np.prod(case))
        assert all((src == b).any() for b in LAYOUT_PLANT) or n < 28
        for to_c16 in (1, 0):
            out = ref_layout(src, case, to_c16)
            assert np.array_equal(out[:n], torch_layout(src, case, to_c16)) and np.all(out[n:] == out[-1])
        assert np.array_equal(ref_layout(ref_layout(src, case, 1)[:n], case, 0)[:n], src.reshape(-1))


def test_merge_and_label_restatements_are_the_oracle():
    rng = np.random.RandomState(5)
    outs = [rng.rand(*MERGE_SHAPE).astype(np.float32) for _ in range(4)]
    mean, mask, counts = ref_merge(np.stack(outs), (0, 1, 2, 3))                      # O.TTA_FLIPS: (), (1,), (2,), (1, 2)
    assert np.array_equal(bits32(mean), bits32(O.tta_merge(outs)))
    for k in MERGE_FLIPS:
        probs = merge_inputs(k)
        mean, mask, counts = ref_merge(probs, MERGE_FLIPS[k])
        assert np.all(mean[:, 1, 2, 3] == 0.5) and not mask[:, 1, 2, 3].any() and mask[:, 3, 2, 1].all()
    assert set(f for fl in MERGE_FLIPS.values() for f in fl) == set(range(8))
    assert flips_word((0, 1, 2, 3)) == 0o3210 and box_of(mean, (4, 5, 6), (1, 1, 1)).shape == (3, 1, 1, 1)      # three bits per copy; the far corner
    for n_et in (ET_MIN, ET_MIN + 1):
        mask, counts = label_inputs(n_et)
        assert counts[2] == n_et
        lab = ref_labels(mask)
        assert np.array_equal(lab, ref_labels(mask, ET_MIN, "none")) and bool((lab == 4).any()) == (n_et > ET_MIN)
        assert set(np.unique(lab)) >= {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------- (b) the exact family is exact; the bars hold the kernel's order
@pytest.mark.parametrize("case", SUM_CASES, ids=case_id)
def test_sum_exact_family_is_exact_and_the_emulated_kernel_meets_the_bars(case):
    n, c, v = case
    p, g = crit_inputs(case, "exact")
    assert set(np.unique(p)) <= {0.25, 0.5, 0.75} and set(np.unique(g)) <= {0.0, 1.0}
    t = sum_terms(p, g, BGW)
    for k in (0, 1):
        tile = max(float(np.abs(t[k][:, :, v0:v0 + CR_CHUNK]).sum(2).max()) for v0 in range(0, v, CR_CHUNK))
        assert tile <= CR_CHUNK * 1.5625
        assert_exact(t[k], tile, 1.0 / 16)
        assert float(np.abs(t[k]).sum()) * 16 < 2.0 ** 53                              # the float64 combine
    ref, emu = ref_sums(p, g, BGW), emulate_sums(p, g, BGW)
    assert same_f64(emu[:2 * c], ref[:2 * c])
    assert excess(emu, ref, sums_bars(p, g, BGW)) <= 1.0
    worst = 0.0
    for targets, bgw in SUM_VARIANTS:
        p, g = crit_inputs(case, "real", targets)
        ref = ref_sums(p, g, bgw)
        assert np.isfinite(ref).all()
        worst = max(worst, excess(emulate_sums(p, g, bgw), ref, sums_bars(p, g, bgw)))
    print("  emulated sums %s worst error / bar %.3g" % (case_id(case), worst))
    assert worst <= 1.0


def test_real_sum_family_reaches_the_saturated_planted_and_constant_classes():
    p, g = crit_inputs((2, 3, 8193), "real")
    assert p.dtype == np.float32 and (p == 1.0).mean() > 0.03 and all((p == np.float32(v)).any() for v in PLANT)
    assert not g[:, 1].any() and g[:, 2].all() and set(np.unique(g)) == {0.0, 1.0}
    idx = last_stride(8193)
    assert idx.size == 256 and idx[0] == 7936 and not p[:, :, idx].any() and g[:, 0, idx].all()
    assert last_stride(8191).size == 0 and last_stride(3 * 8192).size == 768
    ps, gs = crit_inputs((2, 3, 8193), "real", "soft")
    assert 0.0 < gs.min() < 0.01 and 0.99 < gs.max() <= 1.0 and len(np.unique(gs)) > 1000


# ---------------------------------------------------------------------------------------------------------------- (c) the bars and equalities can fail
def test_mutants_exceed_the_bars_of_the_gpu_tests():
    """every listed error, on inputs and bars of tests/test_scalar_passes.py: the mutated restatement must exceed the bar of, or break the equality of (shown as inf),
    at least the cases named here.  The unmutated restatement has excess 0."""
    rows = []
    inf = float("inf")
    # criterion sums
    for mutant, case, family, variant in (("swap_nc", (2, 3, 8193), "real", ("hard", 1e-2)), ("swap_nc", (3, 5, 2 * 8192 + 1), "exact", ("hard", 1e-2)),
                                          ("swap_nc", (2, 3, 8191), "real", ("soft", 1e-2)),
                                          ("stride", (2, 3, 8192), "real", ("hard", 1e-2)), ("stride", (2, 3, 8193), "exact", ("hard", 1e-2)),
                                          ("stride", (1, 1, 3 * 8192), "real", ("hard", 0.0)), ("stride", (3, 5, 2 * 8192 + 1), "real", ("soft", 1e-2)),
                                          ("one_eps", (2, 3, 8193), "real", ("hard", 1e-2)), ("one_eps", (1, 3, 257), "real", ("hard", 1.0)),
                                          ("one_eps", (1, 1, 3 * 8192), "real", ("hard", 1e-2)),
                                          ("bgw_fg", (2, 3, 8193), "real", ("hard", 1e-2)), ("bgw_fg", (1, 1, 1), "real", ("hard", 0.0)),
                                          ("bgw_fg", (1, 3, 255), "real", ("soft", 1e-2))):
        p, g = crit_inputs(case, family, variant[0])
        ref, bad, c = ref_sums(p, g, variant[1]), ref_sums(p, g, variant[1], mutant), case[1]
        ex = excess(bad, ref, sums_bars(p, g, variant[1]))
        if family == "exact" and not same_f64(bad[:2 * c], ref[:2 * c]):
            ex = inf
        rows.append(("%s sums %s %s %s bgw %g" % (mutant, case_id(case), family, variant[0], variant[1]), ex))
    # criterion value
    for case in value_cases():
        if case["name"] != "C3_zero":
            for w in VALUE_WEIGHTS[::2]:
                rows.append(("eps_before value %s w %s" % (case["name"], w), rel_excess(ref_value(case, *w, mutant="eps_before")[:2], ref_value(case, *w)[:2])))
    # criterion gradient (the constants' mutants of tests/test_up2_head_host.py, here on the direct cases)
    for case in GRAD_CASES[:2]:
        inp = grad_inputs(case)
        dp, bar = ref_grad(inp)
        for mutant in ("count", "bgw", "kp"):
            rows.append(("%s gradient %s" % (mutant, case_id(case)), excess(ref_grad(inp, mutant)[0], dp, bar)))
    # Dice
    for rws in DICE_ROWS:
        for v in (1, 5, 1024, 8193):
            p, g = dice_inputs(rws, v)
            for mutant in ("ge", "nan"):
                hit = not np.array_equal(ref_counts(p, g, mutant), ref_counts(p, g))
                if v >= 5 or hit:                                # (one voxel holds one planted value: either 1/2 or NaN)
                    rows.append(("%s counts %dx%d V %d" % (mutant, rws[0], rws[1], v), inf if hit else 0.0))
    for case in accumulate_cases()[:3]:
        a0 = accumulate_start(4)
        hit = not np.array_equal(ref_accumulate(case["counts"], a0, case["nacc"], "den0"), ref_accumulate(case["counts"], a0, case["nacc"]))
        rows.append(("den0 accumulate %s" % case["name"], inf if hit else 0.0))
    # moments
    for c, v in ((1, 1), (4, 16385), (1, 3 * 16384 + 7)):
        x = zs_inputs(c, v)
        if v > 1:                                                # (V = 1 holds the subnormal alone)
            rows.append(("ge z-score %dx%d" % (c, v), moments_excess(ref_moments(x, "ge"), ref_moments(x), moments_bars(x))))
    for c, dims, lo, size in CASE_STATS_CASES:
        img = case_image(c, dims)
        good, bad = crop(img, lo, size), crop(img, lo, size, "origin")
        rows.append(("ge case stats %s %s" % (lo, size), moments_excess(ref_moments(good, "ge"), ref_moments(good), moments_bars(good))))
        if bad is not None:
            rows.append(("origin case stats %s %s" % (lo, size), moments_excess(ref_moments(bad), ref_moments(good), moments_bars(good))))
    # sigmoid, layout
    for n in FLAT_N[1:3]:                                        # (n = 1 holds the planted 0 alone)
        x = flat_inputs(n)
        with np.errstate(over="ignore"):
            rows.append(("plus sigmoid n %d" % n, sigmoid_excess(ref_sigmoid(x, "plus")[0], x)))
    for case in LAYOUT_CASES:
        for to_c16 in (1, 0):
            src = layout_inputs(case) if to_c16 else ref_layout(layout_inputs(case), case, 1)[:int(np.prod(case))]
            hit = not np.array_equal(ref_layout(src, case, to_c16, "unclipped"), ref_layout(src, case, to_c16))
            if case[2] % 64 or hit:
                rows.append(("unclipped layout %s to_c16 %d" % (case_id(case), to_c16), inf if hit else 0.0))
    # merge, labels
    for k in MERGE_FLIPS:
        probs, flips = merge_inputs(k), MERGE_FLIPS[k]
        good = ref_merge(probs, flips)
        for mutant in ("div4", "flip_w"):
            bad = ref_merge(probs, flips, mutant)
            hit = not (np.array_equal(bits32(bad[0]), bits32(good[0])) and np.array_equal(bad[2], good[2]))
            if hit or (mutant == "flip_w" and any(f & 4 for f in flips)):
                rows.append(("%s merge K %d" % (mutant, k), inf if hit else 0.0))
    mask, _ = label_inputs(ET_MIN)
    rows.append(("ge labels", inf if not np.array_equal(ref_labels(mask, ET_MIN, "ge"), ref_labels(mask)) else 0.0))
    for name, ex in rows:
        print("  mutant %-58s error / bar %.3g" % (name, ex))
    names = set(name.split()[0] + " " + name.split()[1] for name, _ in rows)
    assert names >= {"swap_nc sums", "stride sums", "one_eps sums", "bgw_fg sums", "eps_before value", "ge counts", "nan counts", "den0 accumulate", "ge z-score",
                     "origin case", "plus sigmoid", "unclipped layout", "div4 merge", "flip_w merge", "ge labels"}, names
    assert len(rows) > 60
    for name, ex in rows:
        assert ex > 1.0, (name, ex)
