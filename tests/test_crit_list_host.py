"""The float64 restatements that tests/test_crit_list.py holds the criterion-list passes of csrc/criteria.hip to -- ru_crit_moments, ru_crit_reduce, ru_crit_eval,
ru_crit_grad, and ru_tversky_eval (csrc/hardcrit.hip), whose table ru_crit_grad applies --, that file's cases, inputs and bars, and the proof, on the CPU alone, that
(a) the restatements are the reference's operations, (b) the exact family is exact and the bars hold the kernel's own order of summation, (c) the bars and equalities
can fail.

Restatements (numpy float64, written from loss.py:15-195, not from the kernels):
  moments64   the seven sums per row (n, c): sum pg, p^2, p, g, g log(p + 1e-6), (1 - g) log((1 + 1e-6) - p), (p - g)^2; the two log arguments are formed in float32, as
              the reference forms them on float32 tensors; without a log bit in the mask the two log moments are 0
  reduce64    per-channel totals over the samples, added in sample order (the order of crit_reduce_kernel: a float64 sum in a fixed order is reproduced exactly), and
              the Dice_loss_separate slot: sum over n and c >= 1 of (2 sum pg + 1) / (sum (p^2 + g) + 1)
  eval64      the value of every term, the weighted total and the [N, C, 5] table of d(total)/dp = a g + b p + c + d g / (p + 1e-6) + e (1 - g) / ((1 + 1e-6) - p),
              with the sum of the magnitudes of what each output is added up from
  apply64     dp from a table, a scale and with_logs
  tversky_table64   value and (a, c) per class of TverskyLoss, read off loss.tversky_host (tests/test_hardcrit_host.py holds that to float64 autograd): its gradient
              is a_c g + c_c, so two voxels of a class with different targets give both

Bars.  U = 2^-24, U64 = 2^-53, every bar is (roundings on the longest path of the kernel AS WRITTEN, unfused) * unit * (sum of the magnitudes of the partial terms);
a fused multiply-add only removes roundings.  None is measured on the kernels.
  moments   crit_moments_kernel: one lane adds 32 terms of a tile of 8192 (8 quads of 4, or 32 strides of 256), block_sum adds 9 levels (6 shuffles, then
            buf[0] + buf[1] + buf[2] + buf[3]), the float64 sum over the tiles adds nothing visible.  Per tile, hence per row (the factor is the same for every tile):
              R_PG = R_PP = 1 + 41 (the product)        R_P = R_G = 41        R_D2 = 3 + 41 (p - g rounds once and counts twice in the square, the square rounds)
              R_GLOGP = 1 + LOGF_UNITS + 41 (the product, logf)            R_QLOGQ = 2 + LOGF_UNITS + 41 (1 - g, the product, logf)
            and for the two log moments one unit of 2^-24 ABSOLUTE per term for the float32 rounding of the log argument (d log(a) = da / a <= 2^-24): + U sum g,
            + U sum (1 - g).  LOGF_UNITS = 5 is the committed figure of tests/test_scalar_passes_host.py (tools/libm_ulp.py), not taken from these kernels.
  reduce    totals: equality.  Separate-Dice slot: (4 + N (C - 1)) U64 sum |term| (2 s + 1 and the denominator: 3 roundings, the division, one add per term).
  evaluate  OPS = 12 C + 16 roundings of 2^-53 (at C = 4: 64, 7.1e-15 relative -- below the 1e-12 of test_sharded_moments_evaluate_to_the_whole_batch).  The longest
            path is GDL_joint's b coefficient 4 w pr w_c I / U^2: I = sum_c w_c (T_pg + 1) is 3 (C - 1) roundings, U = sum_c w_c (T_pp + T_g + 1) is 4 (C - 1) and
            counts twice, the quotient and its five factors 7, the eight terms of a list 8 more: 11 (C - 1) + 15 <= 12 C + 16.  Values and the float64 table within
            OPS U64 (sum of magnitudes); the float32 table within U |ref| + 2^-149 of that, element by element.
  apply     crit_apply_kernel, per element, against apply64 ON THE FLOAT32 TABLE ACTUALLY USED: R = 6 with the log terms (the longest path is e: e * scale, 1 - g,
            the division, the product, d.. + e.., r + ..), 4 without (x * scale, the product, + b p, + c); R U (|a g| + |b p| + |c| + |d g / pe| + |e (1 - g) / qe|).
            The denominators pe = p + 1e-6f and qe = (1 + 1e-6)f - p are float32 expressions on both sides.  (1 + 1e-6)f = 1 + 2^-20 is a multiple of 2^-23; p in
            [1/2, 1] is a multiple of 2^-24; their difference is a multiple of 2^-24 in [2^-20, 1/2 + 2^-20], below 1: 24 bits hold it, so qe is EXACT there and the
            saturated family's p = 1 and p = 1 - 2^-24 divide by exactly 2^-20 and 2^-20 + 2^-24 (test_saturated_family asserts it).
  Tversky   OPS_TV = 24 roundings (FP, FN 2; the denominator 5; TI 2; 1 - TI 1; pow 4; the mean C + 1; the priority 1; the coefficient's quotient 6), amplified by
            (1 + TI) / (1 - TI): the relative error of 1 - TI, which the power and the coefficients carry on.
Exact family: p in {0, 1/4, 1/2, 3/4, 1}, g in {0, 1/2, 1}: p g, p^2, p, g and (p - g)^2 are multiples of 1/16 no larger than 1, a tile of 8192 sums to at most
8192 < 2^24 / 16, so every partial sum, in any order, fused or not, is a float32 value: the five non-log moments, the totals and (with power-of-two coefficients and
scale, with_logs = 0) dp must equal the float64 restatement bit for bit.

emulate_moments restates crit_moments_kernel's ORDER in numpy float32 (lane stride of both forms, the shuffle tree, numpy's float32 log, unfused): bit-equal on the
exact family, and on the real family inside the bars with room to spare -- worst error / bar 0.060 over the 59 runs (the log moments 0.046; printed by the test), a factor 16.7: the bars are not tighter than
the kernel as written can meet, and a mutant that moves a sum by one part in 10^5 exceeds them.

NaN contract (include/resunet_hip.h): with a class absent from the batch GDL_joint's w_c is infinite; its value and the weighted total are NaN, the b coefficient of
every row c >= 1 is NaN (4 w pr w_c I / U^2 = inf / inf), the a coefficient is NaN in the rows of an absent class and -2 w pr w_c / inf = 0 in the rows of a present
one, so dp is NaN in every row c >= 1, as torch's is; rows c = 0 and every other kind stay finite.  NaN masks must be identical; no element is left out of a comparison.
Nothing here needs a GPU."""
import json

import numpy as np
import pytest
import torch

import hardcrit_inputs as I
from test_hardcrit_host import _operands
from test_scalar_passes_host import LOGF_UNITS, U64, _block_sum32
from test_up2_head_host import TINY, U, assert_exact

CM_CHUNK = 8192                                     # csrc/criteria.hip: voxels of one row per moments block
M_PG, M_PP, M_P, M_G, M_GLOGP, M_QLOGQ, M_D2 = range(7)
NONLOG = [M_PG, M_PP, M_P, M_G, M_D2]
KINDS = ["Dice_loss_joint", "BCE_Loss", "MSE_Loss", "CE_Loss", "Dice1D", "GDL_joint", "sens_loss_joint", "Dice_loss_separate"]       # in the order of RU_CRIT_*
LOG_KINDS = ("BCE_Loss", "CE_Loss")
R_MOMENT = np.array([1 + 41, 1 + 41, 41, 41, 1 + LOGF_UNITS + 41, 2 + LOGF_UNITS + 41, 3 + 41], np.float64)
R_APPLY = {True: 6, False: 4}
OPS_TV = 24
DENORM = 2.0 ** -149
EPS32, ONE_EPS32 = np.float32(1e-6), np.float32(1.0 + 1e-6)


def ops_eval(c):
    return 12 * c + 16


# ---------------------------------------------------------------------------------------------------------------- cases (tests/test_crit_list.py runs exactly these)
ROWS = [(1, 1), (2, 3), (3, 4)]
VS = [1, 3, 4, 5, 8191, 8192, 8193, 8196, 11951, 16388]
FAMILIES = ["real", "soft", "saturated", "absent1", "absent_all", "exact"]
# (N, C, V, family, logs): every V with the log moments and without, on the real, saturated and exact families, the rows rotating so that each (N, C) meets the
# multi-tile V (8193: 1 x 1, 8196: 2 x 3, 11951: 3 x 4, 16388: 1 x 1); soft targets, absent classes and the other rows at the multi-tile V beside them
CASES = [(ROWS[i % 3] + (v, family, logs)) for i, v in enumerate(VS) for family, logs in (("real", True), ("real", False), ("exact", False), ("saturated", True))]
CASES += [(2, 3, v, "soft", True) for v in (5, 8193, 16388)] + [(3, 4, 8193, "soft", False)]
CASES += [(n, c, v, family, True) for n, c, v in ((2, 3, 8196), (3, 4, 11951)) for family in ("absent1", "absent_all")]
CASES += [(2, 3, 8193, "real", True), (2, 3, 8193, "exact", True), (3, 4, 16388, "real", True), (2, 3, 11951, "real", False), (3, 4, 8196, "saturated", True)]
ALIGN_VS = [8196, 16388]
# element offsets of p, g, dp from a 16-byte boundary: all alike, all different, and g alone or dp alone off the boundary (a launcher that looks at p only)
ALIGN_OFFSETS = [(o, o, o) for o in (0, 1, 2, 3)] + [(1, 2, 3), (0, 1, 0), (0, 0, 1)]
TVERSKY_CASES = [(0.5, 0.5, 1.0, 1), (0.3, 0.7, 4.0 / 3.0, 1), (0.3, 0.7, 1.0, 2)]      # alpha, beta, gamma, priority: those of tests/test_hardcrit.py
TVERSKY_SHAPE = (2, 3, 11951)
WRAPPER_CASE = (2, 3, 8193)
WRAPPER_SCALE = 0.37


def case_id(case):
    return "x".join(str(v) for v in case[:3]) + "".join("_" + str(v) for v in case[3:])


def _terms():
    """name -> [(kind, weight, priority, bg_weight)]: each kind alone with weight 1 (priority 1 and 1.25 where it has one, bg_weight 1 and 1e-2 for BCE_Loss), the
    list of all eight with weights 1/8, the same list with eight distinct weights k/36 (a term that gets another term's weight shows), a list with unequal weights that mixes a log kind with the two kinds that skip channel 0, the same three without a log kind"""
    out = {}
    for k in KINDS:
        if k == "BCE_Loss":
            out["BCE_Loss_bg1"], out["BCE_Loss_bg0.01"] = [(k, 1.0, 1.0, 1.0)], [(k, 1.0, 1.0, 1e-2)]
        elif k in ("CE_Loss", "Dice1D"):
            out[k] = [(k, 1.0, 1.0, 1.0)]
        else:
            out[k + "_pr1"], out[k + "_pr1.25"] = [(k, 1.0, 1.0, 1.0)], [(k, 1.0, 1.25, 1.0)]
    pr = {"Dice_loss_joint": 1.25, "MSE_Loss": 0.5, "GDL_joint": 1.5, "sens_loss_joint": 2.0, "Dice_loss_separate": 3.0}
    out["all8"] = [(k, 1.0 / 8, pr.get(k, 1.0), 0.1) for k in KINDS]
    out["all8_unequal"] = [(k, (i + 1) / 36.0, pr.get(k, 1.0), 0.1) for i, k in enumerate(KINDS)]
    out["unequal_logs"] = [("BCE_Loss", 0.7, 1.0, 1e-2), ("GDL_joint", 0.2, 1.5, 1.0), ("Dice_loss_separate", 0.1, 1.0, 1.0)]
    out["unequal_no_logs"] = [("Dice1D", 0.7, 1.0, 1.0), ("GDL_joint", 0.2, 1.5, 1.0), ("Dice_loss_separate", 0.1, 1.0, 1.0), ("MSE_Loss", 0.05, 0.5, 1.0)]
    return out


TERM_LISTS = _terms()
APPLY_LISTS = {True: ["all8", "all8_unequal", "unequal_logs", "BCE_Loss_bg0.01"], False: ["unequal_no_logs", "Dice1D", "Dice_loss_separate_pr1"]}      # by with_logs


def has_logs(terms):
    return any(t[0] in LOG_KINDS for t in terms)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _seed(n, c, v, salt):
    return I.SEED + 7919 * salt + 100003 * n + 1009 * c + v


def inputs(n, c, v, family, salt=0):
    """(p, g) [N, C, V] float32, seeded.  real: hardcrit_inputs.make (p = sigmoid(N(0, 2.5)), g = Bernoulli(0.3)); soft: g uniform in [0, 1]; saturated: a tenth of p
    exactly 0, a tenth exactly 1, a fiftieth each 1 - 2^-24 and 1e-7, independent of g (the first eight voxels of every row hold the four values with g = 0 and
    g = 1 where the row is that long); absent1: the last class missing from the whole batch; absent_all: every class missing; exact: the module docstring's"""
    assert family in FAMILIES
    seed = _seed(n, c, v, salt + 10 * FAMILIES.index(family))
    p, g = I.make((n, c, v), seed=seed)
    rng = np.random.default_rng(seed + 1)
    if family == "soft":
        g = rng.random(size=(n, c, v)).astype(np.float32)
    elif family == "saturated":
        u = rng.random(size=(n, c, v))
        for lo, hi, val in ((0.0, 0.1, 0.0), (0.1, 0.2, 1.0), (0.2, 0.22, 1.0 - 2.0 ** -24), (0.22, 0.24, 1e-7)):
            p[(u >= lo) & (u < hi)] = np.float32(val)
        plant_p = np.array([0.0, 0.0, 1.0, 1.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-7, 1e-7], np.float32)
        plant_g = np.array([0.0, 1.0] * 4, np.float32)
        for r in range(n * c):                                       # (rolled by the row: the rows of a short V must not be copies of each other)
            p[r // c, r % c, :min(v, 8)], g[r // c, r % c, :min(v, 8)] = np.roll(plant_p, 2 * r)[:min(v, 8)], np.roll(plant_g, 2 * r + r // 4)[:min(v, 8)]
    elif family == "absent1":
        g[:, c - 1] = 0.0
    elif family == "absent_all":
        g[:] = 0.0
    elif family == "exact":
        p = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=(n, c, v))
        g = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(n, c, v))
    return np.ascontiguousarray(p), np.ascontiguousarray(g)


def exact_table(n, c):
    """(coef [N, C, 5] float32, scale): powers of two, signs and exponents varying with the row; d and e are set and must be ignored (with_logs = 0)"""
    r = np.arange(n * c)
    coef = np.stack([(-1.0) ** r * 2.0 ** (r % 3), -(-1.0) ** r * 2.0 ** -(r % 2), 2.0 ** -(1 + r % 4) * (-1.0) ** (r // 2), 64.0 + r, -32.0 - r], 1)
    return coef.reshape(n, c, 5).astype(np.float32), np.float32(0.25)


# ---------------------------------------------------------------------------------------------------------------- restatements
def log_args(p, args64=False, mutant=None):
    """(p + 1e-6, (1 + 1e-6) - p) as float64 values of the float32 expressions.  args64: formed in float64 (the reference run on float64 tensors).
    mutant 'one_eps64': (1 + 1e-6) taken in float64"""
    p32 = np.asarray(p, np.float32)
    p64 = p32.astype(np.float64)
    if args64:
        return p64 + 1e-6, (1.0 + 1e-6) - p64
    return (p32 + EPS32).astype(np.float64), ((1.0 + 1e-6) - p64 if mutant == "one_eps64" else (ONE_EPS32 - p32).astype(np.float64))


def moment_terms(p, g, args64=False, mutant=None):
    """[7, N, C, V] float64: the elements of the seven sums"""
    p64, g64 = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    pe, qe = log_args(p, args64, mutant)
    return np.stack([p64 * g64, p64 * p64, p64, g64, g64 * np.log(pe), (1.0 - g64) * np.log(qe), (p64 - g64) ** 2])


def moments64(p, g, logs=True, args64=False, mutant=None):
    """[N, C, 7] float64.  mutant: 'last_element' (the last element of a row dropped), 'last_quad' (the last quad of the final tile), 'tile_twice' (tile 0 counted
    twice where there is a second one), 'tile_boundary' (every tile but the first starts one element late), 'logs_unmasked' (the log moments computed although the mask
    has no log bit), 'one_eps64'"""
    t = moment_terms(p, g, args64, mutant)
    v = t.shape[3]
    keep = np.ones(v)
    if mutant == "last_element":
        keep[v - 1] = 0.0
    elif mutant == "last_quad":
        keep[max(v - 4, 0):] = 0.0
    elif mutant == "tile_twice" and v > CM_CHUNK:
        keep[:CM_CHUNK] = 2.0
    elif mutant == "tile_boundary":
        keep[CM_CHUNK::CM_CHUNK] = 0.0
    m = np.moveaxis((t * keep).sum(3), 0, 2)
    if not logs and mutant != "logs_unmasked":
        m[:, :, [M_GLOGP, M_QLOGQ]] = 0.0
    return np.ascontiguousarray(m)


def moments_bars(p, g, logs=True):
    """[N, C, 7]: R_m U sum |term| (+ U sum g and U sum (1 - g) for the log arguments); 0 for the log moments when they are masked out (they must be 0)"""
    t = np.abs(moment_terms(p, g))
    g64 = np.asarray(g, np.float64)
    bar = np.moveaxis(t.sum(3), 0, 2) * R_MOMENT * U + TINY
    bar[:, :, M_GLOGP] += U * np.abs(g64).sum(2)
    bar[:, :, M_QLOGQ] += U * np.abs(1.0 - g64).sum(2)
    if not logs:
        bar[:, :, [M_GLOGP, M_QLOGQ]] = 0.0
    return bar


def sep_terms(moments):
    """[N, C - 1]: Dice_loss_separate's per-sample term of the rows c >= 1 (loss.py:187-193)"""
    s = np.asarray(moments, np.float64)[:, 1:]
    return (2.0 * s[..., M_PG] + 1.0) / (s[..., M_PP] + s[..., M_G] + 1.0)


def reduce64(moments):
    """[7 C + 1] float64: the totals added in sample order from 0, then the separate-Dice slot"""
    m = np.asarray(moments, np.float64)
    n, c = m.shape[:2]
    tot = np.zeros(c * 7)
    for i in range(n):
        tot = tot + m[i].reshape(-1)
    return np.concatenate([tot, [sep_terms(m).sum()]])


def reduce_bar(moments):
    """the bar of the separate-Dice slot"""
    n, c = np.asarray(moments).shape[:2]
    return (4 + n * (c - 1)) * U64 * float(np.abs(sep_terms(moments)).sum())


def eval64(totals, moments, terms, count, n_global, mutant=None):
    """dict(values [1 + T], vmag [1 + T], coef [N, C, 5], cmag [N, C, 5]) float64, from loss.py's expressions: per class T_m = the totals, per row s_m = the moments.
    mutant: 'bgw_on_g', 'gdl_channel0', 'sens_skip0', 'sep_from_totals', 'n_global_local', 'weights_ignored', 'dice_eps_dropped', 'mse_factor2', 'dice1d_c_dropped',
    'row_mod_n' (a joint kind's row (n, c) reads the totals of class (n C + c) % N), 'weight_mod4' (term k takes the weight of term k % 4)"""
    moments = np.asarray(moments, np.float64)
    n, c = moments.shape[:2]
    count, n_global, cc = np.float64(count), np.float64(n if mutant == "n_global_local" else n_global), np.float64(c)
    t = np.asarray(totals, np.float64)[:c * 7].reshape(c, 7)
    sep_slot = np.float64(np.asarray(totals, np.float64)[c * 7])
    pg, pp, ps, gs, lp, lq, d2 = (t[:, m] for m in range(7))
    rows = np.arange(n * c).reshape(n, c)
    chan = rows % n if mutant == "row_mod_n" else rows % c
    values, vmag = [], []
    coef, cmag = np.zeros((n, c, 5)), np.zeros((n, c, 5))
    with np.errstate(divide="ignore", invalid="ignore"):
        weights = [np.float64(1.0 if mutant == "weights_ignored" else terms[i % 4 if mutant == "weight_mod4" else i][1]) for i in range(len(terms))]
        for (kind, _w, pr, bgw), w in zip(terms, weights):
            kc, kr = np.zeros((c, 5)), None                          # per class (the joint kinds) or per row (Dice_loss_separate)
            if kind == "Dice_loss_joint":                            # loss.py:114-122
                e1, e2 = (0.0, 0.0) if mutant == "dice_eps_dropped" else (1e-6, 2e-6)
                inter, union = pg + e1, pp + gs + e2
                dice = 2.0 * inter / union
                val, mag = pr * (1.0 - dice.sum() / cc), pr * (1.0 + np.abs(dice).sum() / cc)
                kc[:, 0], kc[:, 1] = -(2.0 * pr / cc) / union, 2.0 * (2.0 * pr / cc) * inter / union ** 2
            elif kind == "BCE_Loss":                                 # loss.py:76-79
                wf, wb = (bgw, 1.0) if mutant == "bgw_on_g" else (1.0, bgw)
                val, mag = -(wf * lp.sum() + wb * lq.sum()) / count, (wf * np.abs(lp).sum() + wb * np.abs(lq).sum()) / count
                kc[:, 3], kc[:, 4] = -wf / count, wb / count
            elif kind == "MSE_Loss":                                 # loss.py:27-29
                val = mag = pr * d2.sum() / count
                f = 1.0 if mutant == "mse_factor2" else 2.0
                kc[:, 0], kc[:, 1] = -f * pr / count, f * pr / count
            elif kind == "CE_Loss":                                  # loss.py:60-62
                val, mag = -lp.sum() / count, np.abs(lp).sum() / count
                kc[:, 3] = -1.0 / count
            elif kind == "Dice1D":                                   # loss.py:93-96
                inter, union = pg + 1.0, ps + gs + 2.0
                r = inter / union
                val, mag = 1.0 - 2.0 * (r.sum() / cc), 1.0 + 2.0 * (np.abs(r).sum() / cc)
                kc[:, 0] = -2.0 / (cc * union)
                if mutant != "dice1d_c_dropped":
                    kc[:, 2] = 2.0 * inter / (cc * union ** 2)
            elif kind == "GDL_joint":                                # loss.py:137-150: classes 1.., w_c = 1 / sum g
                first = 0 if mutant == "gdl_channel0" else 1
                wc = 1.0 / gs[first:]
                inter, union = (wc * (pg[first:] + 1.0)).sum(), (wc * (pp[first:] + gs[first:] + 1.0)).sum()
                val, mag = pr * (1.0 - 2.0 * inter / union), pr * (1.0 + np.abs(2.0 * inter / union))
                kc[first:, 0], kc[first:, 1] = -2.0 * pr * wc / union, 4.0 * pr * wc * inter / union ** 2
            elif kind == "sens_loss_joint":                          # loss.py:166-174: every class
                first = 1 if mutant == "sens_skip0" else 0
                r = (pg[first:] + 1.0) / (gs[first:] + 1.0)
                val, mag = pr * (1.0 - r.sum() / (cc - first)), pr * (1.0 + np.abs(r).sum() / (cc - first))
                kc[first:, 0] = -pr / ((cc - first) * (gs[first:] + 1.0))
            elif kind == "Dice_loss_separate":                       # loss.py:187-195: classes 1.., the mean over the GLOBAL batch, the priority unused
                k = 1.0 / (n_global * (cc - 1.0))
                kr = np.zeros((n, c, 5))
                if mutant == "sep_from_totals":
                    inter, union = pg[1:], pp[1:] + gs[1:] + 1.0
                    dice = ((2.0 * inter + 1.0) / union).sum() / (cc - 1.0)
                    kr[:, 1:, 0], kr[:, 1:, 1] = -2.0 / (cc - 1.0) / union, 2.0 / (cc - 1.0) * (2.0 * inter + 1.0) / union ** 2
                else:
                    inter, union = moments[:, 1:, M_PG], moments[:, 1:, M_PP] + moments[:, 1:, M_G] + 1.0
                    dice = sep_slot / (n_global * (cc - 1.0))
                    kr[:, 1:, 0], kr[:, 1:, 1] = -2.0 * k / union, 2.0 * k * (2.0 * inter + 1.0) / union ** 2
                val, mag = 1.0 - dice, 1.0 + np.abs(dice)
            else:
                raise ValueError(kind)
            if kr is None:
                kr = kc[chan]
                if kind == "GDL_joint" and mutant != "gdl_channel0":
                    kr = np.where((rows % c > 0)[..., None], kr, 0.0)          # (row_mod_n: the kernel's `c > 0` is still the row's own class)
            values.append(val)
            vmag.append(mag)
            coef += w * kr
            cmag += np.abs(w * kr)
        total = sum(w * v_ for w, v_ in zip(weights, values))
        tmag = sum(abs(w) * m_ for w, m_ in zip(weights, vmag))
    return dict(values=np.array([total] + values, np.float64), vmag=np.array([tmag] + vmag, np.float64), coef=coef, cmag=cmag)


def eval_bars(ev, c):
    """(values bar [1 + T], float64 table bar, float32 table bar [N, C, 5]); NaN where the magnitudes are"""
    k = ops_eval(c) * U64
    tb = k * ev["cmag"]
    return k * ev["vmag"], tb, tb + U * np.abs(ev["coef"]) + DENORM


def apply_terms(p, g, coef, scale, with_logs, mutant=None):
    """[5, N, C, V] float64: a g, b p, c, d g / pe, e (1 - g) / qe with the table times the scale.  mutant: 'scale_not_on_e', 'scale_twice', 'logs_applied' (d and e
    applied although with_logs = 0)"""
    p64, g64 = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    pe, qe = log_args(p)
    sc = np.full(5, 1.0 if scale is None else float(scale))
    if mutant == "scale_twice":
        sc = sc * sc
    elif mutant == "scale_not_on_e":
        sc[4] = 1.0
    k = (np.asarray(coef, np.float64) * sc)[..., None, :]
    t = np.stack([k[..., 0] * g64, k[..., 1] * p64, k[..., 2] + 0.0 * p64, k[..., 3] * (g64 / pe), k[..., 4] * ((1.0 - g64) / qe)])
    if not with_logs and mutant != "logs_applied":
        t[3:] = 0.0
    return t


def apply64(p, g, coef, scale, with_logs, mutant=None):
    """(dp, bar) [N, C, V] float64"""
    with np.errstate(invalid="ignore"):
        t = apply_terms(p, g, coef, scale, with_logs, mutant)
        return t.sum(0), R_APPLY[bool(with_logs)] * U * np.abs(t).sum(0) + TINY


def tversky_table64(p, g, alpha, beta, gamma, priority, smooth=1.0):
    """(value, coef [N, C, 5] float64, amp [C]) of TverskyLoss from loss.tversky_host: its gradient is a_c g + c_c, so in every class the voxel of sample 0 with the
    smallest target gives c_c (the target must be 0 there) and the one with the largest gives a_c.  amp = (1 + TI) / (1 - TI), for the bars"""
    from brats2019_amd import loss as L
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    n, c, v = p.shape
    value, dp = L.tversky_host(p, g, alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, priority=priority)
    coef = np.zeros((n, c, 5))
    for ch in range(c):
        lo, hi = int(np.argmin(g[0, ch])), int(np.argmax(g[0, ch]))
        assert g[0, ch, lo] == 0.0 and g[0, ch, hi] > 0.0
        coef[:, ch, 2] = dp[0, ch, lo]
        coef[:, ch, 0] = (dp[0, ch, hi] - dp[0, ch, lo]) / float(g[0, ch, hi])
    p64, g64 = p.astype(np.float64), g.astype(np.float64)
    tp = (p64 * g64).sum((0, 2))
    ti = (tp + smooth) / (tp + alpha * (p64.sum((0, 2)) - tp) + beta * (g64.sum((0, 2)) - tp) + smooth)
    return value, coef, (1.0 + ti) / (1.0 - ti)


def tversky_bars(value, coef, amp):
    """(value bar, float32 table bar [N, C, 5])"""
    k = OPS_TV * U64 * float(np.max(amp))
    return k * abs(value), 2.0 * k * np.abs(coef) + U * np.abs(coef) + DENORM


def ratio(got, ref, bar):
    """max |got - ref| / bar over the elements (0 where they are equal); inf unless got is NaN exactly where ref is and finite elsewhere"""
    got, ref, bar = (np.asarray(t, np.float64) for t in (got, ref, bar))
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan) or not np.isfinite(got[~nan]).all():
        return float("inf")
    d = np.abs(got - ref)[~nan]
    if d.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0.0, 0.0, d / bar[~nan]).max())


def same_bits(got, ref):
    """bit for bit as float64 values (a float32 result is widened: exact); NaN never equals"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return got.shape == ref.shape and bool(np.array_equal(got, ref))


# ---------------------------------------------------------------------------------------------------------------- the kernel's own order, float32
def emulate_moments(p, g, logs, vec):
    """crit_moments_kernel<logs, vec> + crit_moments_final_kernel in numpy float32, unfused: a lane adds its 32 terms of a tile in its own order (vec: quads 4 t + 1024 i,
    x y z w; else t + 256 i), block_sum, the tiles in float64"""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    n, c, v = p.shape
    assert not vec or v % 4 == 0
    nblk = -(-v // CM_CHUNK)
    one = np.float32(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = p - g
        t = [p * g, p * p, p, g, g * np.log(p + EPS32), (one - g) * np.log(ONE_EPS32 - p), d * d]
    out = np.zeros((n, c, 7))
    for m, x in enumerate(t):
        if m in (M_GLOGP, M_QLOGQ) and not logs:
            continue
        x = np.pad(x.astype(np.float32), ((0, 0), (0, 0), (0, nblk * CM_CHUNK - v)))
        x = x.reshape(n, c, nblk, 8, 256, 4).transpose(0, 1, 2, 3, 5, 4).reshape(n, c, nblk, 32, 256) if vec else x.reshape(n, c, nblk, 32, 256)
        acc = np.zeros((n, c, nblk, 256), np.float32)
        for s in range(32):
            acc = acc + x[..., s, :]
        out[:, :, m] = _block_sum32(acc).astype(np.float64).sum(2)
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) the restatements are the reference's operations
def torch_kind(kind, x, y, pe, qe, pr, bgw):
    """the criterion as loss.py writes it, on [N, C, V] float64 tensors (pe, qe: the two log arguments)"""
    if kind == "MSE_Loss":
        return torch.mean((x.reshape(-1) - y.reshape(-1)) ** 2) * pr
    if kind == "CE_Loss":
        return -torch.mean(y * torch.log(pe))
    if kind == "BCE_Loss":
        return -torch.mean(y * torch.log(pe) + bgw * (1. - y) * torch.log(qe))
    if kind == "Dice1D":
        return 1.0 - 2.0 * torch.mean(((x * y).sum(dim=(0, 2)) + 1) / ((x + y).sum(dim=(0, 2)) + 2))
    if kind == "Dice_loss_joint":
        return pr * (1.0 - torch.mean(2.0 * ((x * y).sum(dim=(0, 2)) + 1e-6) / ((x ** 2 + y).sum(dim=(0, 2)) + 2e-6)))
    if kind == "GDL_joint":
        xs, ys = x[:, 1:], y[:, 1:]
        w = 1 / ys.sum(dim=(0, 2))
        inter, union = w * ((xs * ys).sum(dim=(0, 2)) + 1), w * ((xs ** 2 + ys).sum(dim=(0, 2)) + 1)
        return pr * (1.0 - torch.mean(2.0 * inter.sum() / union.sum()))
    if kind == "sens_loss_joint":
        return pr * (1.0 - torch.mean(((x * y).sum(dim=(0, 2)) + 1) / (y.sum(dim=(0, 2)) + 1)))
    if kind == "Dice_loss_separate":
        xs, ys = x[:, 1:], y[:, 1:]
        return 1.0 - torch.mean((2.0 * (xs * ys).sum(dim=2) + 1) / ((xs ** 2 + ys).sum(dim=2) + 1))
    raise ValueError(kind)


def chain64(p, g, terms, logs=True, args64=False, scale=None):
    """the four restatements in a row on one shard: (eval64's dict, dp)"""
    m = moments64(p, g, logs, args64)
    ev = eval64(reduce64(m), m, terms, float(p.size), p.shape[0])
    with np.errstate(invalid="ignore"):
        t = apply_terms(p, g, ev["coef"], scale, logs)
        if args64:                                                   # the denominators in float64 too
            pe, qe = log_args(p, True)
            g64 = np.asarray(g, np.float64)
            t[3], t[4] = ev["coef"][..., None, 3] * (g64 / pe), ev["coef"][..., None, 4] * ((1.0 - g64) / qe)
        return ev, t.sum(0)


@pytest.mark.parametrize("name", sorted(TERM_LISTS))
def test_restatements_match_float64_autograd(name):
    """each kind alone and the three lists: value and d/dp against autograd of loss.py's expressions, within 1e-11 of the gradient's max"""
    terms = TERM_LISTS[name]
    for family in ("real", "soft"):
        p, g = inputs(2, 3, 257, family)
        x, pe, qe = _operands(p)
        y = torch.from_numpy(g.astype(np.float64))
        vals = [torch_kind(k, x, y, pe, qe, pr, bgw) for k, _w, pr, bgw in terms]
        total = sum(w * v for (_k, w, _pr, _bgw), v in zip(terms, vals))
        (dref,) = torch.autograd.grad(total, x)
        ev, dp = chain64(p, g, terms)
        ref = np.array([float(total.detach())] + [float(v.detach()) for v in vals])
        assert np.abs(ev["values"] - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), (name, ev["values"], ref)
        assert np.abs(dp - dref.numpy()).max() <= 1e-11 * np.abs(dref.numpy()).max(), name
        assert np.abs(dref.numpy()).max() > 0
    for full in ("all8", "all8_unequal"):
        assert [t[0] for t in TERM_LISTS[full]] == KINDS
    assert len({t[1] for t in TERM_LISTS["all8_unequal"]}) == 8 and abs(sum(t[1] for t in TERM_LISTS["all8_unequal"]) - 1.0) < 1e-15
    assert len({t[1] for t in TERM_LISTS["unequal_logs"]}) == 3 and "all8_unequal" in APPLY_LISTS[True]


@pytest.mark.parametrize("b", [0, 1, 2])
def test_restatements_match_the_committed_reference_runs(golden, b):
    """every run of tests/golden/criteria.npz (the reference's own classes on float64 tensors: the log arguments in float64): values at 1e-12, the gradient -- stored
    rounded to float32 -- at 2^-24 of each element, NaN exactly where the reference's is (batch 2: a class absent)"""
    gd = golden("criteria")
    runs = json.loads(str(gd["runs"]))
    p, g = gd["b%d_pred" % b].reshape(gd["b%d_pred" % b].shape[:2] + (-1,)), gd["b%d_gt" % b].reshape(gd["b%d_gt" % b].shape[:2] + (-1,))
    for name, members in runs.items():
        terms = [(cls, 1.0 / len(members), float(kw.get("priority", 1)), float(kw.get("bg_weight", 1))) for cls, kw in members]
        ev, dp = chain64(p, g, terms, True, args64=True)
        ref_v, ref_dp = gd["b%d_%s_values64" % (b, name)], gd["b%d_%s_dp" % (b, name)].reshape(p.shape).astype(np.float64)
        assert np.array_equal(np.isnan(ev["values"][1:]), np.isnan(ref_v)) and np.isnan(ev["values"][0]) == np.isnan(ref_v).any(), name
        ok = ~np.isnan(ref_v)
        assert np.abs(ev["values"][1:][ok] - ref_v[ok]).max(initial=0.0) <= 1e-12, name
        if ok.all():
            assert abs(ev["values"][0] - float(gd["b%d_%s_loss64" % (b, name)])) <= 1e-12, name
        assert np.array_equal(np.isnan(dp), np.isnan(ref_dp)), name
        fin = ~np.isnan(ref_dp)
        assert (np.abs(dp - ref_dp)[fin] <= 1.01 * U * np.abs(ref_dp)[fin] + DENORM).all(), name
    if b == 2:
        assert np.isnan(gd["b2_gdl_dp"][:, 1:]).all() and not np.isnan(gd["b2_gdl_dp"][:, 0]).any()


def test_tversky_table_is_the_gradient_of_the_host_restatement():
    from brats2019_amd import loss as L
    p, g = inputs(*TVERSKY_SHAPE, "exact")
    for alpha, beta, gamma, priority in TVERSKY_CASES:
        value, coef, amp = tversky_table64(p, g, alpha, beta, gamma, priority)
        _, ref = L.tversky_host(p, g, alpha=alpha, beta=beta, gamma=gamma, priority=priority)
        dp, _ = apply64(p, g, coef, None, False)
        assert np.abs(dp - ref).max() <= 1e-13 * np.abs(ref).max() and (amp > 1.0).all() and amp.max() < 100.0
        assert not coef[..., [1, 3, 4]].any() and coef[..., 0].all() and coef[..., 2].all()


# ---------------------------------------------------------------------------------------------------------------- the case list and the families
def test_case_list_covers_what_it_must():
    assert len(set(CASES)) == len(CASES)
    for v in VS:
        assert {logs for _n, _c, vv, _f, logs in CASES if vv == v} == {True, False}, v
        assert {f for _n, _c, vv, f, _l in CASES if vv == v} >= {"real", "exact", "saturated"}, v
    for rows in ROWS:
        assert any((n, c) == rows and v > CM_CHUNK for n, c, v, _f, _l in CASES), rows
    assert {f for _n, _c, _v, f, _l in CASES} == set(FAMILIES)
    assert max(n * c * v for n, c, v, _f, _l in CASES) <= 12 * 16388
    assert 11951 % 4 == 3 and all(v % 4 == 0 for v in ALIGN_VS) and WRAPPER_CASE[2] == CM_CHUNK + 1


def test_saturated_family_holds_the_planted_values_with_both_targets_and_exact_denominators():
    p, g = inputs(2, 3, 8193, "saturated")
    for val in (0.0, 1.0, 1.0 - 2.0 ** -24, 1e-7):
        hit = p == np.float32(val)
        assert hit.mean() > 0.01 and {0.0, 1.0} <= set(np.unique(g[hit])), val
    assert abs((p == 0).mean() - 0.1) < 0.01 and abs((p == 1).mean() - 0.1) < 0.01
    hi = p >= 0.5                                                    # (1 + 1e-6)f - p is exact in float32 for p in [1/2, 1]: the module docstring
    assert float(ONE_EPS32) == 1.0 + 2.0 ** -20
    assert np.array_equal((ONE_EPS32 - p[hi]).astype(np.float64), float(ONE_EPS32) - p[hi].astype(np.float64))
    _, qe = log_args(p)
    assert set(np.unique(qe[p == 1])) == {2.0 ** -20} and set(np.unique(qe[p == np.float32(1.0 - 2.0 ** -24)])) == {2.0 ** -20 + 2.0 ** -24}
    m = moments64(p, g)
    assert np.isfinite(m).all() and np.isfinite(apply64(p, g, np.ones((2, 3, 5), np.float32), 1.0, True)[0]).all()
    ps, gs = inputs(2, 3, 8193, "soft")
    assert 0.0 <= gs.min() < 0.01 and 0.99 < gs.max() <= 1.0 and len(np.unique(gs)) > 1000


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "exact"], ids=case_id)
def test_exact_family_is_exact(case):
    """the premises, on the inputs themselves; then float32 sums in the kernel's order (both forms) equal the float64 ones, and dp of the exact table too"""
    n, c, v, _f, logs = case
    p, g = inputs(n, c, v, "exact")
    assert set(np.unique(p)) <= {0.0, 0.25, 0.5, 0.75, 1.0} and set(np.unique(g)) <= {0.0, 0.5, 1.0}
    t = moment_terms(p, g)
    for m in NONLOG:
        tile = max(float(np.abs(t[m][:, :, v0:v0 + CM_CHUNK]).sum(2).max()) for v0 in range(0, v, CM_CHUNK))
        assert tile <= CM_CHUNK
        assert_exact(t[m], tile, 1.0 / 16)
        assert float(np.abs(t[m]).sum()) * 16 < 2.0 ** 53
    ref = moments64(p, g, logs)
    for vec in ([False, True] if v % 4 == 0 else [False]):
        assert same_bits(emulate_moments(p, g, logs, vec)[:, :, NONLOG], ref[:, :, NONLOG])
    coef, scale = exact_table(n, c)
    terms = apply_terms(p, g, coef, scale, False)
    assert not terms[3:].any()
    assert_exact(terms[:3], np.abs(terms[:3]).sum(0), 2.0 ** -8)
    dp, _ = apply64(p, g, coef, scale, False)
    assert np.array_equal(dp.astype(np.float32).astype(np.float64), dp) and (len(np.unique(dp)) > 8 or p.size < 64)


def test_emulated_kernel_order_sits_inside_the_moment_bars():
    """the real, soft and saturated families of CASES: crit_moments_kernel's order in float32, both forms, against the float64 restatement"""
    worst, worst_log, rows = 0.0, 0.0, 0
    for n, c, v, family, logs in CASES:
        if family == "exact":
            continue
        p, g = inputs(n, c, v, family)
        ref, bar = moments64(p, g, logs), moments_bars(p, g, logs)
        for vec in ([False, True] if v % 4 == 0 else [False]):
            emu = emulate_moments(p, g, logs, vec)
            worst = max(worst, ratio(emu[:, :, NONLOG], ref[:, :, NONLOG], bar[:, :, NONLOG]))
            worst_log = max(worst_log, ratio(emu[:, :, 4:6], ref[:, :, 4:6], bar[:, :, 4:6]))
            rows += 1
    print("  emulated moments over %d runs: worst error / bar %.3g (the log moments %.3g): the bars leave a factor %.1f" % (rows, worst, worst_log, 1.0 / max(worst, worst_log)))
    assert 1e-3 < max(worst, worst_log) <= 0.25


def test_reduce_and_evaluate_restatements_on_shards():
    """the sharded form: totals of two moments tensors added, each shard evaluated with n_global = 2 N -> the values of the whole batch, its rows of the table"""
    pa, ga = inputs(2, 3, 8193, "real")
    pb, gb = inputs(2, 3, 8193, "real", salt=1)
    ma, mb = moments64(pa, ga), moments64(pb, gb)
    mw = np.concatenate([ma, mb])
    terms = TERM_LISTS["all8"]
    whole = eval64(reduce64(mw), mw, terms, 2.0 * pa.size, 4)
    tot = reduce64(ma) + reduce64(mb)
    for half, sl in ((ma, slice(0, 2)), (mb, slice(2, 4))):
        ev = eval64(tot, half, terms, 2.0 * pa.size, 4)
        vb, tb, _ = eval_bars(whole, 3)
        assert ratio(ev["values"], whole["values"], vb) <= 1.0 and ratio(ev["coef"], whole["coef"][sl], tb[sl]) <= 1.0
    assert ops_eval(4) * U64 < 1e-12 and ops_eval(4) == 64


def test_nan_contract_of_an_absent_class():
    for n, c, v, family, logs in [k for k in CASES if k[3].startswith("absent")]:
        p, g = inputs(n, c, v, family)
        assert not g[:, c - 1].any() and (family == "absent_all") == (not g.any())
        m = moments64(p, g, logs)
        for name in ("all8", "all8_unequal", "unequal_logs", "GDL_joint_pr1.25"):
            terms = TERM_LISTS[name]
            ev = eval64(reduce64(m), m, terms, float(p.size), n)
            kinds = [t[0] for t in terms]
            nan = np.isnan(ev["values"])
            assert nan[0] and [k for k, bad in zip(kinds, nan[1:]) if bad] == ["GDL_joint"], (name, ev["values"])
            coef = ev["coef"]
            assert np.isfinite(coef[:, 0]).all() and np.isfinite(coef[:, :, 2:]).all()
            assert np.isnan(coef[:, 1:, 1]).all() and np.isnan(coef[:, c - 1, 0]).all()
            if family == "absent_all":
                assert np.isnan(coef[:, 1:, 0]).all()
            else:
                assert np.isfinite(coef[:, 1:c - 1, 0]).all()          # -2 w pr w_c / inf = 0 beside the other terms' shares
            dp, bar = apply64(p, g, coef.astype(np.float32), None, has_logs(terms))
            assert np.isnan(dp[:, 1:]).all() and np.isfinite(dp[:, 0]).all() and np.array_equal(np.isnan(bar), np.isnan(dp))
            assert ratio(dp, dp, bar) == 0.0 and ratio(np.nan_to_num(dp), dp, bar) == float("inf")


# ---------------------------------------------------------------------------------------------------------------- (c) the bars and equalities can fail
def test_mutants_exceed_the_bars():
    """every listed error, applied to the restatement on inputs and bars of tests/test_crit_list.py: it must exceed the bar, or break the equality (shown as inf), of
    every case named here.  The unmutated restatement has excess 0."""
    rows, inf = [], float("inf")

    def moments_row(mutant, case):
        n, c, v, family, logs = case
        p, g = inputs(n, c, v, family)
        ref, bad, bar = moments64(p, g, logs), moments64(p, g, logs, mutant=mutant), moments_bars(p, g, logs)
        ex = ratio(bad, ref, bar)
        if family == "exact" and not same_bits(bad[:, :, NONLOG], ref[:, :, NONLOG]):
            ex = inf
        rows.append(("%s moments %s" % (mutant, case_id(case)), ex))
    for case in CASES:
        n, c, v, family, logs = case
        if family in ("real", "exact", "saturated"):
            moments_row("last_element", case)
            if v % 4 == 0:
                moments_row("last_quad", case)
            if v > CM_CHUNK:
                moments_row("tile_twice", case)
                moments_row("tile_boundary", case)
        if family == "saturated" and v >= 3:                         # (p within 1e-3 of 1 is what shows it: a tenth of this family is exactly 1)
            moments_row("one_eps64", case)
        if not logs:                                                 # the mask test's equality: moments 4 and 5 exactly 0
            p, g = inputs(n, c, v, family)
            bad = moments64(p, g, False, mutant="logs_unmasked")
            rows.append(("logs_unmasked moments %s" % case_id(case), inf if bad[:, :, 4:6].any() else 0.0))

    def eval_row(mutant, name, case, shards=False, what="both"):
        n, c, v, family, logs = case
        p, g = inputs(n, c, v, family)
        m = moments64(p, g, logs)
        tot, ng, count = reduce64(m), n, float(p.size)
        if shards:
            p2, g2 = inputs(n, c, v, family, salt=1)
            tot, ng, count = tot + reduce64(moments64(p2, g2, logs)), 2 * n, 2.0 * p.size
        ref, bad = eval64(tot, m, TERM_LISTS[name], count, ng), eval64(tot, m, TERM_LISTS[name], count, ng, mutant=mutant)
        vb, _, tb32 = eval_bars(ref, c)
        ev, et = ratio(bad["values"], ref["values"], vb), ratio(bad["coef"].astype(np.float32), ref["coef"], tb32)
        rows.append(("%s evaluate %s %s%s" % (mutant, name, case_id(case), " sharded" if shards else ""), {"values": ev, "table": et, "both": min(ev, et), "any": max(ev, et)}[what]))
    big = [k for k in CASES if k[0] > 1 and k[3] in ("real", "soft", "saturated") and k[4]]
    assert len(big) >= 6
    for case in big:
        eval_row("bgw_on_g", "BCE_Loss_bg0.01", case)
        eval_row("bgw_on_g", "all8", case)
        eval_row("gdl_channel0", "GDL_joint_pr1.25", case)
        eval_row("gdl_channel0", "unequal_logs", case)
        eval_row("sens_skip0", "sens_loss_joint_pr1", case)
        eval_row("sens_skip0", "all8", case)
        eval_row("sep_from_totals", "Dice_loss_separate_pr1", case)
        eval_row("sep_from_totals", "unequal_logs", case)
        eval_row("n_global_local", "Dice_loss_separate_pr1", case, shards=True)
        eval_row("n_global_local", "all8", case, shards=True)
        eval_row("weights_ignored", "all8", case)
        eval_row("weights_ignored", "unequal_logs", case)
        eval_row("weights_ignored", "all8_unequal", case)
        eval_row("weight_mod4", "all8_unequal", case)
        eval_row("dice_eps_dropped", "Dice_loss_joint_pr1.25", case, what="values" if case[2] > 8 else "both")      # (1e-6 of a sum of thousands is below the float32 table's 2^-24)
        eval_row("mse_factor2", "MSE_Loss_pr1.25", case, what="table")          # (the value has no factor 2)
        eval_row("mse_factor2", "all8", case, what="table")
        eval_row("dice1d_c_dropped", "Dice1D", case, what="table")
        eval_row("dice1d_c_dropped", "all8", case, what="table")
        eval_row("row_mod_n", "all8", case, what="table")
        eval_row("row_mod_n", "Dice1D", case, what="table")

    def apply_row(mutant, case, with_logs, coef, scale):
        n, c, v, family, logs = case
        p, g = inputs(n, c, v, family)
        ref, bar = apply64(p, g, coef, scale, with_logs)
        bad, _ = apply64(p, g, coef, scale, with_logs, mutant=mutant)
        ex = ratio(bad, ref, bar)
        if family == "exact" and not same_bits(bad, ref):
            ex = inf
        rows.append(("%s apply %s" % (mutant, case_id(case)), ex))
    for case in CASES:
        n, c, v, family, logs = case
        if family.startswith("absent"):
            continue
        p, g = inputs(n, c, v, family)
        if family == "exact":
            coef, scale = exact_table(n, c)
            apply_row("scale_twice", case, False, coef, scale)
            apply_row("logs_applied", case, False, coef, scale)
            continue
        m = moments64(p, g, logs)
        coef = eval64(reduce64(m), m, TERM_LISTS["all8"], float(p.size), n)["coef"].astype(np.float32)
        if c == 1:
            coef = np.nan_to_num(coef)                               # (one class: GDL_joint and Dice_loss_separate have no class and are NaN)
        if logs:
            apply_row("scale_not_on_e", case, True, coef, np.float32(WRAPPER_SCALE))
        else:
            apply_row("logs_applied", case, False, coef, np.float32(WRAPPER_SCALE))
        apply_row("scale_twice", case, logs, coef, np.float32(WRAPPER_SCALE))
    for name, ex in rows:
        print("  mutant %-72s error / bar %.3g" % (name, ex))
    names = {name.split()[0] for name, _ in rows}
    assert names == {"last_element", "last_quad", "tile_twice", "tile_boundary", "logs_unmasked", "one_eps64", "bgw_on_g", "gdl_channel0", "sens_skip0", "sep_from_totals",
                     "n_global_local", "weights_ignored", "weight_mod4", "dice_eps_dropped", "mse_factor2", "dice1d_c_dropped", "row_mod_n", "scale_not_on_e", "scale_twice",
                     "logs_applied"}, names
    assert len(rows) > 300
    for name, ex in rows:
        assert ex > 1.0, (name, ex)
