"""The float64 restatements that tests/test_up2_head.py holds the trilinear pair and the head of the backward pass to, that file's cases, inputs and bars,
and the proof -- on the CPU alone -- that (a) the restatements are the reference's operations, (b) the exact families are exact and (c) the bars can fail.

Kernels (csrc/pointwise.hip, csrc/pointwise_c16.hip):
  up2_fwd_kernel / up2_fwd_vec_kernel / up2_fwd16_kernel     y = lrelu(Mz (My (Mx x)), out_slope), M = O.np_trilinear_matrix(n) per axis (model.py:12-14); only the
                                                             voxel-major kernel has the activation
  up2_bwd_kernel / up2_bwd_vec_kernel / up2_bwd16_kernel     dx = Mz^T (My^T (Mx^T dy))
  head_grad_c4_kernel<false>                                 d = dp * p * (1 - p) (model.py:431) -> d4 [N, V, 4] (+0 in lanes C..3) and, through bias_final_kernel,
                                                             db [C] = sum over n, v of d (model.py:348)
  head_grad_c4_kernel<true>                                  the same with dp = the criterion's gradient (crit_grad_kernel's expression) formed from (p, target, sums)
  ew_kernel<EW_SIGMOID_BWD>, bias_partial / bias_final       the generic route: d -> dlog [N, C, V], then db over the stored dlog

Exact families.  A sum of terms that are all whole multiples of one power of two q, with sum of |term| < 2^24 q, is a float32 value after ANY subset of the terms has
been added in ANY order, with or without fused multiply-adds: every partial sum is a whole multiple of q below 2^24 q.  assert_exact checks the two premises.
  trilinear  x (or dy) integers in [-8, 8]; per-axis coefficients in {1/4, 3/4, 1} (whole quarters), so a forward output is a sum of multiples of 1/64 (1/128 behind
             the activation of slope 1/2) with sum |term| <= 8, and an adjoint output a sum of multiples of 1/64 with sum |term| <= 8 * 2^3 (a column of M sums to <= 2)
  head       p in {1/4, 1/2, 3/4}, dp integers in [-8, 8]: dp * p is a multiple of 1/4, times (1 - p) a multiple of 1/16, |d| <= 2; db is a sum of N V such terms,
             exact while 32 N V < 2^24 (asserted for every case).  Criterion form: w_dice = 1, w_bce = 0, priority = C / 2 and sums solved so that U = 4 and I in {2, 4}
             exactly: the constants are kg = -1/4, kp in {1/4, 1/2}, cb = 0, so dp = kg g + kp p is a multiple of 1/16 with |dp| <= 1/2 (the BCE term is 0 * finite), d a
             multiple of 1/256 with |d| <= 1/8: again 32 units at most, the same inequality.
On these the device must reproduce the float64 restatement bit for bit; a lost, duplicated or misplaced term moves an output by at least one unit.

Real families.  Seeded normal data.  Head: p = sigmoid(12 z) in float32 (about 7 % of them are exactly 1.0f), 0, 1, 2^-24, 1 - 2^-24 and 1/2 planted at the start of every
row, targets in {0, 1}, and in the last quad of every 16384-voxel chunk p = 1/2 with dp = 2 (exact family: 8), so that a quad dropped there is never a quad of zeros.

Bars.  bar = r * 2^-24 * sum of |coefficient| * |operand| over the terms of that output (+ r * 2^-126, the smallest normal, for an underflowing product); r = the float32
roundings on the longest path of the kernel AS WRITTEN (an addition onto a zero accumulator and a product with 0 or 1 are exact but a product with 1/4 is counted with the
others; contraction into fused multiply-adds only removes roundings):
  R_UP_FWD16 = 7    three nested lerps `l0 * a + l1 * b`, each one rounded product and one rounded add on any path (6), and the activation's product (1)
  R_UP_FWD   = 6    the NCDHW kernels: the same three lerps, no activation
  R_UP_BWD   = 12   all three adjoint kernels: the x row sum of 4 products (1 product + 3 adds), the y accumulation `acc += wy * row` over 4 rows (1 product + 3 adds:
                    the first add is onto 0), and the z accumulation over the 4 fine planes that feed one coarse plane -- in up2_bwd16_kernel two as cC in one step of
                    the march and two as cP in the next -- (1 product + 3 adds)
  R_D        = 3    `1 - p` and the two products
  R_D_CRIT   = 10   R_D plus, for the criterion's gradient, the two constant casts on a path (cb and bgw; kg or kp on the Dice terms), the two divisions and the three
                    adds: an upper bound of every path (the longest, through bgw * (1 - g) / (1 + 1e-6 - p), has 6 + 3).  The log arguments p + 1e-6f and (1 + 1e-6)f - p
                    are NOT counted: the oracle forms them in float32 too.  The bar is taken on |kg g| + |kp p| + cb (g / a + bgw (1 - g) / b), because the terms cancel.
  R_SUM_C4   = 28   db on the 4-channel pass: (d0 + d1) + (d2 + d3) (2), the thread's serial sum over 16 quads (15: the first is onto 0), block_sum (9 as written:
                    6 shuffle levels and buf[0] + buf[1] + buf[2] + buf[3] -- not log2(256) = 8: the four wave sums are added serially), the store of the partial (0: it is a
                    float already), the float64 sum of the partials (1 covers its 2^-53 roundings) and the final cast (1).  bar = R_SUM * 2^-24 * sum |d| + sum of d's bars
  R_SUM_GEN  = 74   db on the generic route: a thread's serial sum over 64 voxels (63), block_sum (9), float64 sum (1), cast (1)

Mutants: test_mutants_exceed_the_bars_of_the_gpu_tests applies each listed error to the restatement on the GPU file's own inputs.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

U = 2.0 ** -24
TINY = 2.0 ** -126
R_UP_FWD16, R_UP_FWD, R_UP_BWD = 7, 6, 12
R_D, R_D_CRIT = 3, 10
R_SUM_C4, R_SUM_GEN = 2 + 15 + 9 + 0 + 1 + 1, 63 + 9 + 1 + 1
UP2B_ZC = 8                         # csrc/pointwise_c16.hip: coarse planes per step of the adjoint's z-march
BG_CHUNK = 16384                    # csrc/pointwise.hip: voxels per bias partial

# ---------------------------------------------------------------------------------------------------------------- cases (tests/test_up2_head.py runs exactly these)
C16_CASES = [(1, 16, 1, 1, 1), (1, 16, 1, 1, 4), (2, 32, 2, 3, 5)] + [(1, 16, d, 3, 4) for d in (7, 8, 9, 16, 17)] + [(1, 32, 3, 5, 6), (1, 16, 12, 20, 24)]
WRAP_CASE = (1, 16, 80, 80, 80)     # 81 * 81 * 160 * 4 threads > 16384 * 256: the forward's grid-stride loop wraps; 262 MB out: nontemporal stores
NCDHW_CASES = [(1, 2, 1, 1, 1), (2, 3, 2, 1, 2), (1, 4, 3, 2, 7), (2, 4, 9, 5, 12), (1, 3, 2, 3, 3)]
SLOPES = {"real": (1.0, 0.01), "exact": (1.0, 0.5)}
C4_CASES = [(1, 3, 4), (2, 3, 16384), (2, 3, 16388), (3, 3, 49148), (1, 1, 1028), (1, 2, 1028), (1, 4, 32772)]
GENERIC_CASES = [(2, 3, 16385), (1, 5, 1001)]
PLANT = [0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]
BGW = 1e-2
COUNT_FACTOR = 3                    # the criterion's global count is 3 x the shard's elements (a three-rank job)


def case_id(case):
    return "x".join(str(v) for v in case)


def _seed(case, salt):
    return 1000 * salt + sum((i + 1) * int(v) for i, v in enumerate(case)) % 997


# ---------------------------------------------------------------------------------------------------------------- trilinear: restatement (torch, any device)
def up_matrix(n, mutant=None):
    """O.np_trilinear_matrix(n) [2n, n]; mutant: 'unclamped' (i1 = i0 + 1 past the end reads zero), 'src' (src = o/2 - 1/4 not clamped at 0: the first output
    extrapolates), 'swapped' (l0 and l1 change places)"""
    m = O.np_trilinear_matrix(n)
    if mutant == "unclamped":
        m[2 * n - 1, n - 1] -= 0.25
    elif mutant == "src":
        m[0, :] = 0.0
        m[0, 0] += 1.25
        m[0, min(1, n - 1)] -= 0.25
    elif mutant == "swapped":
        m = np.zeros((2 * n, n))
        for k in range(n):
            m[2 * k, max(k - 1, 0)] += 0.75
            m[2 * k, k] += 0.25
            m[2 * k + 1, k] += 0.25
            m[2 * k + 1, min(k + 1, n - 1)] += 0.75
    else:
        assert mutant is None
    return m


def _apply(m, x, ax):
    m = torch.from_numpy(np.ascontiguousarray(m)).to(x.device)
    return torch.movedim(torch.tensordot(m, torch.movedim(x, ax, 0), dims=([1], [0])), 0, ax)


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def ref_up2(x, out_slope=1.0, mutant=None):
    """x [..., D, H, W] float64 -> [..., 2D, 2H, 2W], nesting z(y(x)) like the kernels.  mutant: one of up_matrix's on every axis, 'act_before_z' (the activation
    applied to the x/y-interpolated planes), 'sample0' (every sample reads the slabs of sample 0)"""
    assert x.dtype == torch.float64
    mm = mutant if mutant in ("unclamped", "src", "swapped") else None
    if mutant == "sample0":
        x = x[:1].expand_as(x)
    x = _apply(up_matrix(x.shape[-1], mm), x, -1)
    x = _apply(up_matrix(x.shape[-2], mm), x, -2)
    if mutant == "act_before_z":
        return _apply(up_matrix(x.shape[-3]), lrelu(x, out_slope), -3)
    return lrelu(_apply(up_matrix(x.shape[-3], mm), x, -3), out_slope)


def ref_up2_bwd(dy, mutant=None):
    """dy [..., 2D, 2H, 2W] float64 -> [..., D, H, W]: the transposed matrices.  mutant: up_matrix's, 'seam' (the fine planes 2 k0 - 1 and 2 k0 at a seam of the
    z-march counted for the chunk that starts at k0 only: coarse plane k0 - 1 loses them), 'last_plane' (the last chunk's final coarse plane not stored: NaN, what the
    output was filled with), 'sample0'"""
    assert dy.dtype == torch.float64
    mm = mutant if mutant in ("unclamped", "src", "swapped") else None
    if mutant == "sample0":
        dy = dy[:1].expand_as(dy)
    d = dy.shape[-3] // 2
    mz = up_matrix(d, mm).T.copy()
    if mutant == "seam":
        for k0 in range(UP2B_ZC, d, UP2B_ZC):
            mz[k0 - 1, 2 * k0 - 1] = 0.0
            mz[k0 - 1, 2 * k0] = 0.0
    dx = _apply(up_matrix(dy.shape[-1] // 2, mm).T, dy, -1)
    dx = _apply(up_matrix(dy.shape[-2] // 2, mm).T, dx, -2)
    dx = _apply(mz, dx, -3)
    if mutant == "last_plane":
        dx = dx.clone()
        dx[..., d - 1, :, :] = float("nan")
    return dx


def up_bar(x, r):
    """per output element: r 2^-24 sum |coefficient| |x| (the coefficients are positive: the same matrices on |x|)"""
    return r * (U * ref_up2(x.abs()) + TINY)


def up_bwd_bar(dy, r):
    return r * (U * ref_up2_bwd(dy.abs()) + TINY)


def up_inputs(case, family):
    """(x [N, C, D, H, W], dy [N, C, 2D, 2H, 2W]) float32 CPU tensors"""
    n, c, d, h, w = case
    g = torch.Generator().manual_seed(_seed(case, 1 if family == "real" else 2))
    if family == "exact":
        draw = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    return draw(n, c, d, h, w), draw(n, c, 2 * d, 2 * h, 2 * w)


def excess(got, ref, bar):
    """max over elements of |got - ref| / bar (<= 1 passes); a NaN or an infinity in `got` is +inf"""
    got, ref, bar = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).double() for t in (got, ref, bar))
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bar).max())


def same_bits(got, ref64):
    """exact family: the float32 tensor `got` is the float64 reference, which is a float32 value (NaN never equals)"""
    got, ref64 = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t) for t in (got, ref64))
    return got.shape == ref64.shape and bool(torch.equal(got.double(), ref64.double()))


def assert_exact(values, abs_sum, unit):
    """the premises of the module docstring: `values` whole multiples of `unit`, `abs_sum` (a bound on sum |term| of any output) below 2^24 units"""
    v = torch.as_tensor(values).double() / unit
    assert bool((v == v.round()).all()), "not a multiple of %g" % unit
    assert float(torch.as_tensor(abs_sum).double().max()) / unit < 2.0 ** 24, (float(torch.as_tensor(abs_sum).double().max()), unit)
    assert bool(torch.equal(torch.as_tensor(values).double().float().double(), torch.as_tensor(values).double()))


# ---------------------------------------------------------------------------------------------------------------- head: restatement (numpy float64)
def head_quads(v):
    """the voxels of the last quad of every chunk of BG_CHUNK (and of the row): where a chunk's loop ends"""
    ends = sorted(set(list(range(BG_CHUNK, v, BG_CHUNK)) + [v]))
    return np.unique(np.array([e - 4 + t for e in ends for t in range(4) if e - 4 + t >= 0], np.int64))


def ref_head(p, dp, mutant=None):
    """p, dp [N, C, V] -> (d [N, C, V], db [C], d4 [N, V, 4]) float64.  mutant: 'quad_sum' (the last quad of a chunk dropped from the sum), 'quad_d4' (dropped
    from d4: NaN, what the output was filled with), 'pad' (the padding lanes carry channel 0), 'sample0' (p (1 - p) of sample 0 for every sample), 'n0' (the
    bias partials of sample 0 only)"""
    p, dp = np.asarray(p, np.float64), np.asarray(dp, np.float64)
    n, c, v = p.shape
    q = np.broadcast_to(p[:1], p.shape) if mutant == "sample0" else p
    d = dp * q * (1.0 - q)
    summed = d[:1] if mutant == "n0" else d
    db = summed.sum((0, 2))
    if mutant == "quad_sum":
        db = db - summed[:, :, head_quads(v)].sum((0, 2))
    d4 = np.zeros((n, v, 4))
    d4[:, :, :min(c, 4)] = d.transpose(0, 2, 1)[:, :, :4]
    if mutant == "pad":
        d4[:, :, c:] = d[:, 0, :, None]
    if mutant == "quad_d4":
        d4[:, head_quads(v), :] = np.nan
    return d, db, d4


def crit_terms(p, g, sums, count, bgw=BGW, priority=1.0, w_dice=0.5, w_bce=0.5, mutant=None):
    """the four terms of d(w_dice Dice + w_bce BCE)/dp [4, N, C, V], float64, from the float32 p, the float32 target and float64 sums [2C + 1] (loss.py:70-79,
    105-122): kg g, kp p, -cb g / a, cb bgw (1 - g) / b with a = p + 1e-6f and b = (1 + 1e-6)f - p formed in float32 as loss.py forms them.
    mutant: 'bgw' (omitted), 'kp' (without its factor 2), 'count' (the shard's N C V instead of the global count)"""
    p32 = np.asarray(p, np.float32)
    p64, g = p32.astype(np.float64), np.asarray(g, np.float64)
    sums = np.asarray(sums, np.float64)
    c = p64.shape[1]
    sh = (1, c, 1)
    i_c, u_c = (sums[:c] + 1e-6).reshape(sh), (sums[c:2 * c] + 2e-6).reshape(sh)
    k = float(priority) * (2.0 / c) * float(w_dice)
    kg, kp = -k / u_c, (1.0 if mutant == "kp" else 2.0) * k * i_c / (u_c * u_c)
    cb = float(w_bce) / (float(p64.size) if mutant == "count" else float(count))
    a = (p32 + np.float32(1e-6)).astype(np.float64)
    b = (np.float32(1.0 + 1e-6) - p32).astype(np.float64)
    w = 1.0 if mutant == "bgw" else float(bgw)
    return np.stack([kg * g, kp * p64, -cb * (g / a), cb * (w * (1.0 - g) / b)])


def ref_crit_dp(p, g, sums, count, **kw):
    return crit_terms(p, g, sums, count, **kw).sum(0)


def head_bars(p, dp_terms, r_d, r_sum, n_only=None):
    """(bar of d [N, C, V], bar of db [C]).  dp_terms [T, N, C, V]: the terms of dp (one term on the 4-channel and generic routes)"""
    p = np.asarray(p, np.float64)
    mag = np.abs(np.asarray(dp_terms, np.float64)).sum(0) * p * np.abs(1.0 - p)
    bar_d = r_d * (U * mag + TINY)
    bar_db = r_sum * (U * mag.sum((0, 2)) + TINY) + bar_d.sum((0, 2))
    return bar_d, bar_db


def solve_sum(target, eps):
    """a float64 s with s + eps == target exactly (the kernels add the epsilons to the sums they are handed)"""
    s = target - eps
    for cand in (s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)):
        if cand + eps == target:
            return float(cand)
    raise AssertionError((target, eps))


def exact_crit(c):
    """the criterion of the exact family: dict(sums [2C + 1], w_dice, w_bce, priority, kg [C], kp [C]) with U = 4, I = 2, 4, 2, 4"""
    i_c = [2.0, 4.0, 2.0, 4.0][:c]
    sums = np.array([solve_sum(i, 1e-6) for i in i_c] + [solve_sum(4.0, 2e-6)] * c + [-1.0])
    return dict(sums=sums, w_dice=1.0, w_bce=0.0, priority=c / 2.0, kg=np.full(c, -0.25), kp=np.array(i_c) / 8.0)


def head_inputs(case, family):
    """dict(p, dp, g [N, C, V] float32, sums [2C + 1] float64, count, crit = keyword arguments of the criterion) -- numpy"""
    n, c, v = case
    rng = np.random.RandomState(_seed(case, 3 if family == "real" else 4))
    g = (rng.rand(n, c, v) < 0.3).astype(np.float32)
    quads = head_quads(v)
    if family == "exact":
        assert 32 * n * v < 2 ** 24, case
        p = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=(n, c, v))
        dp = rng.randint(-8, 9, size=(n, c, v)).astype(np.float32)
        p[:, :, quads], dp[:, :, quads], g[:, :, quads] = 0.5, 8.0, 0.0
        ec = exact_crit(min(c, 4))
        return dict(p=p, dp=dp, g=g, sums=ec["sums"], count=float(COUNT_FACTOR * p.size),
                    crit=dict(w_dice=ec["w_dice"], w_bce=ec["w_bce"], priority=ec["priority"], bg_weight=BGW))
    z = torch.from_numpy(rng.randn(n, c, v).astype(np.float32) * 12.0)
    p = torch.sigmoid(z).numpy()
    dp = rng.randn(n, c, v).astype(np.float32)
    p[:, :, quads], dp[:, :, quads] = 0.5, 2.0
    plant = np.array(PLANT, np.float32)
    for r in range(n * c):
        row = p[r // c, r % c]
        if v >= 12:
            row[:5] = np.roll(plant, r)
        else:
            row[1:4] = np.roll(plant, r)[:3]                     # one quad: 1/2 stays in its first voxel
    inter, union, bce = O.np_dice_bce_sums(p, g, BGW)
    return dict(p=p, dp=dp, g=g, sums=np.concatenate([inter, union, [bce]]), count=float(COUNT_FACTOR * p.size),
                crit=dict(w_dice=0.5, w_bce=0.5, priority=1.0, bg_weight=BGW))


def head_crit_reference(inp, mutant=None):
    """(dp [N, C, V] float64, its terms [4, N, C, V]) of the criterion route on head_inputs' dict"""
    k = inp["crit"]
    terms = crit_terms(inp["p"], inp["g"], inp["sums"], inp["count"], bgw=k["bg_weight"], priority=k["priority"], w_dice=k["w_dice"], w_bce=k["w_bce"], mutant=mutant)
    return terms.sum(0), terms


# ---------------------------------------------------------------------------------------------------------------- (a) the restatements are the reference's operations
def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


@pytest.mark.parametrize("case", [(2, 3, 1, 1, 1), (1, 2, 1, 1, 4), (2, 3, 2, 3, 5), (1, 2, 9, 3, 4)], ids=case_id)
def test_trilinear_restatement_is_the_reference_interpolation_and_its_autograd(case):
    x, dy = (t.double() for t in up_inputs(case, "real"))
    xr = x.clone().requires_grad_(True)
    y = O.trilinear_up2(xr)
    (dx,) = torch.autograd.grad(y, xr, dy)
    _close(ref_up2(x).numpy(), y.detach().numpy(), 1e-12)
    _close(ref_up2_bwd(dy).numpy(), dx.numpy(), 1e-12)
    _close(ref_up2(x).numpy(), O.np_trilinear_up2(x.numpy()), 1e-12)
    _close(ref_up2_bwd(dy).numpy(), O.np_trilinear_up2_bwd(dy.numpy()), 1e-12)
    _close(ref_up2(x, O.LEAKY_SLOPE).numpy(), O.leaky_relu(O.trilinear_up2(x)).numpy(), 1e-12)          # the fused activation: LeakyReLU of the interpolation


def test_head_restatement_is_the_autograd_of_the_criterion_through_a_float64_sigmoid():
    """p in [0.1, 0.9] as float32 values and count = N C V = 24576: the oracle's closed form builds the two log arguments in float32 (as loss.py does), float64 autograd
    does not; they differ by <= 2^-25 + |1e-6f - 1e-6| < 3.1e-8, which moves d by <= 0.5 * 3.1e-8 * (1 - p) / p / count <= 5.7e-12 here -- inside the 1e-11 asked for"""
    n, c, v = 2, 3, 4096
    rng = np.random.RandomState(5)
    p = torch.sigmoid(torch.from_numpy(np.clip(rng.randn(n, c, v) * 1.5, -2.19, 2.19).astype(np.float32))).numpy()
    assert p.dtype == np.float32 and 0.1 <= p.min() and p.max() <= 0.9
    g = (rng.rand(n, c, v) < 0.3).astype(np.float32)
    inter, union, bce = O.np_dice_bce_sums(p, g, BGW)
    sums = np.concatenate([inter, union, [bce]])
    dp = O.np_criterion_grad(p, g, inter, union, p.size, BGW)
    np.testing.assert_allclose(ref_crit_dp(p, g, sums, p.size), dp, rtol=1e-13, atol=1e-18)
    d, db, d4 = ref_head(p, dp)
    p64 = torch.from_numpy(p.astype(np.float64))
    z = torch.log(p64 / (1.0 - p64)).requires_grad_(True)
    loss = O.criterion(torch.sigmoid(z), torch.from_numpy(g.astype(np.float64)), BGW)
    (dz,) = torch.autograd.grad(loss, z)
    _close(d, dz.numpy(), 1e-11)
    # db is the plain sum of d: with the SAME dp on both sides it is the bias gradient of sigmoid(logits + bias) to 1e-11; against the float64 criterion the 2 * 4096
    # per-element differences above add up (they share a sign where p + 1e-6f rounds one way), so that comparison is held to their sum
    zb, bias = torch.log(p64 / (1.0 - p64)), torch.zeros(1, c, 1, dtype=torch.float64, requires_grad=True)
    (gb,) = torch.autograd.grad((torch.sigmoid(zb + bias) * torch.from_numpy(dp)).sum(), bias)
    _close(db, gb.reshape(-1).numpy(), 1e-11)
    assert float(np.abs(db - dz.sum((0, 2)).numpy()).max()) <= n * v * 5.7e-12
    assert np.array_equal(d4[:, :, :c], d.transpose(0, 2, 1)) and not d4[:, :, c:].any() and not np.signbit(d4[:, :, c:]).any()
    # other weights, bg_weight, priority and a global count: float64 autograd of the same two losses
    zz = torch.log(p64 / (1.0 - p64)).requires_grad_(True)
    pp, gg = torch.sigmoid(zz), torch.from_numpy(g.astype(np.float64))
    red = 0.7 * O.dice_loss_joint(pp, gg, 1.5) + 0.3 * O.bce_loss(pp, gg, 1.0) * (p.size / (3.0 * p.size))
    (dz2,) = torch.autograd.grad(red, zz)
    inter1, union1, bce1 = O.np_dice_bce_sums(p, g, 1.0)
    dp2 = ref_crit_dp(p, g, np.concatenate([inter1, union1, [bce1]]), 3.0 * p.size, bgw=1.0, priority=1.5, w_dice=0.7, w_bce=0.3)
    _close(ref_head(p, dp2)[0], dz2.numpy(), 1e-11)


# ---------------------------------------------------------------------------------------------------------------- (b) the exact families are exact
@pytest.mark.parametrize("case", C16_CASES + NCDHW_CASES, ids=case_id)
def test_trilinear_exact_family_is_exact(case):
    x, dy = (t.double() for t in up_inputs(case, "exact"))
    assert float(x.abs().max()) <= 8 and float(dy.abs().max()) <= 8 and bool((x == x.round()).all()) and bool((dy == dy.round()).all())
    for n in set(case[2:]):
        m = up_matrix(n)
        assert np.array_equal(4 * m, np.round(4 * m)) and m.min() >= 0 and np.allclose(m.sum(1), 1.0) and m.sum(0).max() <= 2.0
    for slope in SLOPES["exact"]:
        assert_exact(ref_up2(x, slope), ref_up2(x.abs()), (1.0 / 64) * min(slope, 1.0))
    assert float(ref_up2(x.abs()).max()) <= 8.0                 # (the x- and x/y-interpolated planes are bounded the same way: rows of M sum to 1)
    assert_exact(ref_up2_bwd(dy), ref_up2_bwd(dy.abs()), 1.0 / 64)
    assert float(ref_up2_bwd(dy.abs()).max()) <= 64.0
    # the adjoint identity, every product a multiple of 1/64 and the sums far below 2^53 units: exact in float64
    lhs, rhs = (ref_up2(x) * dy).sum(), (x * ref_up2_bwd(dy)).sum()
    assert float(lhs) == float(rhs) and float((ref_up2(x) * dy).abs().sum()) * 64 < 2.0 ** 53


def test_wrap_case_is_the_smallest_cube_whose_forward_grid_wraps_and_is_exact_by_the_same_bound():
    n, c, d, h, w = WRAP_CASE
    threads = lambda s: (s + 1) * (s + 1) * 2 * s * 4
    assert threads(d) == 4199040 > 16384 * 256 >= threads(d - 1)
    assert n * c * 8 * d * h * w * 4 >= 128 << 20                # the nontemporal-store rule of up2_fwd16_kernel
    assert n * c * 8 * d * h * w * 4 + 2 * n * c * d * h * w * 4 < 1 << 30


@pytest.mark.parametrize("case", C4_CASES + GENERIC_CASES, ids=case_id)
def test_head_exact_family_is_exact(case):
    n, c, v = case
    inp = head_inputs(case, "exact")
    assert 32 * n * v < 2 ** 24
    p, dp = inp["p"].astype(np.float64), inp["dp"].astype(np.float64)
    assert set(np.unique(p)) <= {0.25, 0.5, 0.75} and np.array_equal(dp, np.round(dp)) and np.abs(dp).max() <= 8
    d, db, d4 = ref_head(p, dp)
    assert_exact(dp * p, np.abs(dp * p), 0.25)
    assert_exact(d, np.abs(d), 1.0 / 16)
    assert_exact(db, np.abs(d).sum((0, 2)), 1.0 / 16)           # every partial sum of the n V terms of a channel, in any order
    assert np.abs(d).max() <= 2.0
    assert db[0] != ref_head(p, dp, "quad_sum")[1][0]            # the planted quads are not quads of zeros
    if c > 4:
        return
    # criterion form: the constants the kernels form in float64 and cast are the dyadic numbers of exact_crit
    ec = exact_crit(c)
    k = inp["crit"]
    kk = float(np.float32(k["priority"])) * (2.0 / c) * float(np.float32(k["w_dice"]))
    i_c, u_c = ec["sums"][:c] + 1e-6, ec["sums"][c:2 * c] + 2e-6
    assert kk == 1.0 and np.array_equal(u_c, np.full(c, 4.0)) and np.array_equal(i_c, ec["kp"] * 8.0)
    assert np.array_equal(np.float32(-kk / u_c), ec["kg"]) and np.array_equal(np.float32(2.0 * kk * i_c / (u_c * u_c)), ec["kp"])
    assert np.float32(float(np.float32(k["w_bce"])) / inp["count"]) == 0.0
    dpc, terms = head_crit_reference(inp)
    assert not terms[2:].any() and np.isfinite(terms).all()      # 0 * (a finite BCE term)
    assert np.array_equal(dpc, ec["kg"].reshape(1, c, 1) * inp["g"] + ec["kp"].reshape(1, c, 1) * p)
    dc, dbc, _ = ref_head(p, dpc)
    assert_exact(dpc, np.abs(terms).sum(0), 1.0 / 16)
    assert np.abs(dpc).max() <= 0.5
    assert_exact(dc, np.abs(terms).sum(0) * p * (1 - p), 1.0 / 256)
    assert_exact(dbc, (np.abs(terms).sum(0) * p * (1 - p)).sum((0, 2)), 1.0 / 256)
    assert np.abs(dc).max() <= 0.125 and 32 * n * v < 2 ** 24  # 32 units of 1/256 per term at most


def test_real_head_family_reaches_the_saturated_and_planted_values():
    inp = head_inputs((2, 3, 16388), "real")
    p = inp["p"]
    assert p.dtype == np.float32 and (p == 1.0).mean() > 0.03 and all((p == np.float32(v)).any() for v in PLANT)
    assert set(np.unique(inp["g"])) == {0.0, 1.0}
    assert np.array_equal(p[:, :, head_quads(16388)], np.full((2, 3, 8), 0.5, np.float32))
    assert inp["count"] != p.size
    d, db, _ = ref_head(p, head_crit_reference(inp)[0])
    assert np.isfinite(d).all() and np.isfinite(db).all()
    tiny = head_inputs((1, 3, 4), "real")["p"]
    assert (tiny == 0.0).any() and (tiny == 1.0).any() and (tiny[:, :, 0] == 0.5).all()


# ---------------------------------------------------------------------------------------------------------------- (c) the bars can fail
def _up_rows(case, family, slope, r_f, r_b, mutants_f, mutants_b):
    x, dy = (t.double() for t in up_inputs(case, family))
    good_y, good_dx = ref_up2(x, slope), ref_up2_bwd(dy)
    rows = []
    for m in mutants_f:
        bad = ref_up2(x, slope, m)
        rows.append(("%s forward %s %s" % (m, case_id(case), family), float("inf") if family == "exact" and not same_bits(bad.float(), good_y) else
                     excess(bad, good_y, up_bar(x, r_f))))
    for m in mutants_b:
        bad = ref_up2_bwd(dy, m)
        rows.append(("%s adjoint %s %s" % (m, case_id(case), family), float("inf") if family == "exact" and not same_bits(bad.float(), good_dx) else
                     excess(bad, good_dx, up_bwd_bar(dy, r_b))))
    return rows


def test_mutants_exceed_the_bars_of_the_gpu_tests():
    """every listed error, on inputs and bars of tests/test_up2_head.py (up_inputs / head_inputs of its cases): on the real family the mutated restatement must
    exceed the bar, on the exact family it must differ from the float64 reference (error / bar shown as inf).  The unmutated restatement has excess 0."""
    rows = []
    matrix = ["unclamped", "src", "swapped"]
    for family in ("real", "exact"):
        s = SLOPES[family][1]
        # the smallest case with more than one plane on every axis, N > 1 and CB > 1: border coefficients, sample / block addressing, the activation's place
        rows += _up_rows((2, 32, 2, 3, 5), family, s, R_UP_FWD16, R_UP_BWD, matrix + ["act_before_z", "sample0"], matrix + ["sample0"])
        rows += _up_rows((1, 16, 1, 1, 4), family, s, R_UP_FWD16, R_UP_BWD, matrix, matrix)
        # the z-march: the seam needs a second chunk (D = 9: a second chunk of one plane; D = 16: both full; D = 17: two seams); the last plane every D
        for d in (9, 16, 17):
            rows += _up_rows((1, 16, d, 3, 4), family, s, R_UP_FWD16, R_UP_BWD, [], ["seam", "last_plane"])
        for d in (7, 8):
            rows += _up_rows((1, 16, d, 3, 4), family, s, R_UP_FWD16, R_UP_BWD, [], ["last_plane"])
        # NCDHW kernels: scalar and vector forms at their smallest multi-voxel cases
        rows += _up_rows((1, 4, 3, 2, 7), family, 1.0, R_UP_FWD, R_UP_BWD, matrix, matrix)
        rows += _up_rows((2, 3, 2, 1, 2), family, 1.0, R_UP_FWD, R_UP_BWD, matrix + ["sample0"], matrix + ["sample0"])

        # head, 4-channel pass and criterion form at (2, 3, 16388): two chunks, the second of one quad, N > 1, a padding lane
        case = (2, 3, 16388)
        inp = head_inputs(case, family)
        p, c = inp["p"], case[1]
        dpc, terms = head_crit_reference(inp)
        for tag, dp, dp_terms, r_d in (("c4", inp["dp"], inp["dp"][None], R_D), ("crit", dpc, terms, R_D_CRIT)):
            d, db, d4 = ref_head(p, dp)
            bar_d, bar_db = head_bars(p, dp_terms, r_d, R_SUM_C4)
            bar4 = np.full(d4.shape, TINY)
            bar4[:, :, :c] = bar_d.transpose(0, 2, 1)
            bad = [(m, ref_head(p, dp, m)) for m in ("quad_sum", "quad_d4", "pad", "sample0", "n0")]
            if tag == "crit":                                                  # (w_bce = 0 on the exact family: the BCE mutants belong to the real one)
                bad += [(m, ref_head(p, head_crit_reference(inp, m)[0])) for m in (("bgw", "kp", "count") if family == "real" else ("kp",))]
            for m, (_, bdb, bd4) in bad:
                if family == "exact":
                    ex = 0.0 if same_bits(bd4.astype(np.float32), d4) and same_bits(bdb.astype(np.float32), db) else float("inf")
                elif m == "pad":
                    ex = float("inf") if bd4[:, :, c:].any() else 0.0          # the lanes are compared by bit pattern
                else:
                    ex = max(excess(bd4, d4, bar4), excess(bdb, db, bar_db))
                rows.append(("%s %s %s" % (m, tag, family), ex))
        # generic route at (2, 3, 16385): the sum over the stored dlog
        inp = head_inputs((2, 3, 16385), family)
        p = inp["p"]
        d, db, _ = ref_head(p, inp["dp"])
        bar_d, bar_db = head_bars(p, inp["dp"][None], R_D, R_SUM_GEN)
        for m in ("quad_sum", "sample0", "n0"):
            bd, bdb, _ = ref_head(p, inp["dp"], m)
            if family == "exact":
                ex = 0.0 if same_bits(bd.astype(np.float32), d) and same_bits(bdb.astype(np.float32), db) else float("inf")
            else:
                ex = max(excess(bd, d, bar_d), excess(bdb, db, bar_db))
            rows.append(("%s generic %s" % (m, family), ex))
    for name, ex in rows:
        print("  mutant %-46s error / bar %.3g" % (name, ex))
    assert len(rows) > 80
    for name, ex in rows:
        assert ex > 1.0, (name, ex)
