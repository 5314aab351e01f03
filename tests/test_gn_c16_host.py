"""The float64 reference of every link of the voxel-major GroupNorm chain that tests/test_gn_c16.py holds the device to, that file's input builders, and the
proof -- on the CPU alone -- that the reference is the reference's GroupNorm and that the exact family is exact.

Links (csrc/pointwise.hip, csrc/pointwise_c16.hip, csrc/fin_tail.hpp; NCDHW float64 here, 8 groups):
  finalize          partials [N, C, nblk, 2] of (sum, sumsq) -- or, centred, of (sum, M2 about the chunk's mean) -- -> mean, rstd [N, G]; scale = gamma * rstd,
                    shift = beta - mean * scale [N, C]; bst_k [N, 3, C] = (sign(gamma) * rstd, -sign(gamma) * mean * rstd, -beta / |gamma|), sign(0) = +1, and for
                    gamma == 0 the threshold is -inf where beta > 0 and +inf elsewhere (the mask `u > thr` is then the constant `beta > 0`)
  apply             y = res' + lrelu(x * scale + shift, slope), res' = nothing, res, or lrelu(res * rscale + rshift, rslope)
  backward sums     S1 = sum dh, S2 = sum dh * xhat per (n, c), dh = dact * lrelu'(x * scale + shift); the sign-carrying form has S2' = sign(gamma) * S2
  backward finalize m1 = sum_j gamma_j S1_j / m, m2 = sum_j gamma_j S2_j / m over the group (m = cpg * V); coef = (rstd * gamma, -rstd^2 * m2, rstd^2 * m2 * mean - rstd * m1);
                    dgamma = sum_n S2, dbeta = sum_n S1; s2_sign = 1 takes S2' and undoes the sign first
  backward apply    dx = cA * dh + cB * x + cC; the split form is ops.to_split_c16's: bf16 RNE hi, bf16 RNE of the float32 residual (csrc/pw_helpers.hpp: pw_split8 is
                    the same split_n the converters use), decoded and barred by tests/test_wgrad3_fused_host.py's split_decode / pub_bars
Each is compared with oracle.resunet_oracle.np_group_norm / np_group_norm_bwd and with float64 autograd of res' + leaky_relu(group_norm(x)).

Inputs.  Real family: gn_param_set / gn_off_the_kink of tests/test_hip_ops.py (imported), seeded normal tensors.  Exact family (exact_*): gamma = sign pattern of
gn_param_set(kind) on magnitudes {1/2, 1, 2} (its zeros kept), beta = its sign pattern on {1, 2, 3}; partials small non-zero integers, in every (sample, group) one
pair adjusted so that the group mean is 0 or +-2^k and the variance is 1, 5/4 or 3/2; the backward's mean a small integer and rstd a power of two; x, dact small integers
(dact even: slope 1/2).  V is a power of two and where cpg = 6 (C = 48) the sums are made divisible by 3, so every division is exact.  Then every sum, mean, variance and
backward coefficient is a dyadic rational of fewer than 24 bits: float32 and float64 arithmetic in ANY order and with or without fused multiply-adds give the same bits,
rstd is the one irrational number and is the correctly rounded value, and every output that depends on it is ONE rounding of an exact product.  A lost, duplicated
or stale partial moves a sum by at least one unit.  test_exact_family_is_exact proves all of this with `fractions`.  Nothing here needs a GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_hip_ops import gn_off_the_kink, gn_param_set
from test_wgrad3_fused_host import blocks, split_decode

G, EPS = O.GN_GROUPS, float(np.float32(O.GN_EPS))          # (the device holds eps as a float32)
GN_CHUNK = 8192                                             # csrc/pointwise.hip: the voxels of one centred pair
EXACT_SLOPE = 0.5
EXACT_V = 1 << 14


# ---------------------------------------------------------------------------------------------------------------- reference, float64
def lrelu(u, slope):
    return np.where(u > 0, u, u * slope)


def per_channel(a, cpg):
    """[N, G] -> [N, C]"""
    return np.repeat(a, cpg, axis=1)


def ref_finalize(partials, gamma, beta, V, eps=EPS, centred=False):
    """-> dict(mean [N, G], rstd [N, G], scale [N, C], shift [N, C], bst_k [N, 3, C]) in float64, in the operation order of gn_finalize_kernel"""
    p = np.asarray(partials, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    n, c, nblk, _ = p.shape
    cpg = c // G
    m = float(cpg) * float(V)
    s1 = p[..., 0].reshape(n, G, cpg * nblk).sum(-1)
    s2 = p[..., 1].reshape(n, G, cpg * nblk).sum(-1)
    mu = s1 / m
    if centred:
        cnt = np.minimum(GN_CHUNK, V - GN_CHUNK * np.arange(nblk)).astype(np.float64)
        dev = p[..., 0] / cnt - per_channel(mu, cpg)[:, :, None]
        var = (s2 + (cnt * dev * dev).reshape(n, G, cpg * nblk).sum(-1)) / m
    else:
        var = s2 / m - mu * mu
    var = np.maximum(var, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    return stats_from(mu, rstd, gamma, beta)


def stats_from(mu, rstd, gamma, beta):
    """what the finalize derives from (mean, rstd) [N, G]"""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    cpg = gamma.shape[0] // G
    muc, rsc = per_channel(mu, cpg), per_channel(rstd, cpg)
    scale = gamma[None] * rsc
    shift = beta[None] - muc * scale
    sg = np.where(gamma < 0, -1.0, 1.0)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = np.where(gamma == 0, np.where(beta > 0, -np.inf, np.inf), -beta / np.abs(gamma))
    bst_k = np.stack([sg * rsc, -sg * muc * rsc, np.broadcast_to(thr[None], muc.shape)], axis=1)
    return dict(mean=mu, rstd=rstd, scale=scale, shift=shift, bst_k=bst_k)


def ref_finalize_device(partials, gamma, beta, V, eps=EPS, centred=False):
    """what the device writes where its arithmetic is exact: mean and rstd rounded to float32 FIRST (the kernels form scale, shift and bst_k from the rounded pair),
    every output then one float32 rounding of the float64 value -> dict of float32 arrays"""
    st = ref_finalize(partials, gamma, beta, V, eps, centred)
    return stats32(stats_from(st["mean"].astype(np.float32).astype(np.float64), st["rstd"].astype(np.float32).astype(np.float64), gamma, beta))


def stats_of(x, gamma, beta):
    """the finalize outputs of the tensor x itself (float64 statistics)"""
    _, mu, rstd = O.np_group_norm(x, gamma, beta)
    return stats_from(mu, rstd, gamma, beta)


def stats32(st):
    """float64 statistics `st` as the float32 tensors a device kernel is handed (each rounded once)"""
    with np.errstate(over="ignore"):
        return {k: np.asarray(v, np.float32) for k, v in st.items()}


def bc(a):
    """[N, C] -> [N, C, 1, 1, 1]"""
    return np.asarray(a, np.float64)[:, :, None, None, None]


def ref_apply(x, scale, shift, slope, res=None, rscale=None, rshift=None, rslope=1.0):
    """the three residual forms of gn_apply16_kernel"""
    y = lrelu(np.asarray(x, np.float64) * bc(scale) + bc(shift), slope)
    if res is None:
        return y
    r = np.asarray(res, np.float64)
    if rscale is not None:
        r = lrelu(r * bc(rscale) + bc(rshift), rslope)
    return y + r


def ref_dh(x, dact, scale, shift, slope):
    return np.asarray(dact, np.float64) * np.where(np.asarray(x, np.float64) * bc(scale) + bc(shift) > 0, 1.0, slope)


def ref_bwd_sums(x, dact, scale, shift, mean, rstd, slope, gamma=None):
    """S [N, C, 2] = (sum dh, sum dh * xhat); with gamma the sign-carrying form (sum dh * sign(gamma) * xhat) the fused convolution statistics publish"""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    cpg = c // G
    dh = ref_dh(x, dact, scale, shift, slope)
    xh = (x - bc(per_channel(mean, cpg))) * bc(per_channel(rstd, cpg))
    s = np.stack([dh.reshape(n, c, -1).sum(-1), (dh * xh).reshape(n, c, -1).sum(-1)], axis=-1)
    if gamma is not None:
        s[..., 1] *= np.where(np.asarray(gamma) < 0, -1.0, 1.0)[None]
    return s


def ref_bwd_finalize(S, gamma, mean, rstd, V, s2_sign=0):
    """S [N, C, 2] (partials already summed) -> dict(coef [N, C, 3], dgamma [C], dbeta [C]), in the operation order of gn_bwd_finalize_kernel"""
    S = np.array(S, np.float64)
    gamma, mean, rstd = np.asarray(gamma, np.float64), np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    n, c, _ = S.shape
    cpg = c // G
    if s2_sign:
        S[..., 1] = np.where(gamma[None] < 0, -S[..., 1], S[..., 1])
    m = float(cpg) * float(V)
    m1 = (gamma[None] * S[..., 0]).reshape(n, G, cpg).sum(-1) / m
    m2 = (gamma[None] * S[..., 1]).reshape(n, G, cpg).sum(-1) / m
    cA = per_channel(rstd, cpg) * gamma[None]
    cB = per_channel(-rstd * rstd * m2, cpg)
    cC = per_channel(rstd * rstd * m2 * mean - rstd * m1, cpg)
    return dict(coef=np.stack([cA, cB, cC], axis=-1), dgamma=S[..., 1].sum(0), dbeta=S[..., 0].sum(0))


def ref_dx(x, dact, scale, shift, coef, slope):
    coef = np.asarray(coef, np.float64)
    return bc(coef[..., 0]) * ref_dh(x, dact, scale, shift, slope) + bc(coef[..., 1]) * np.asarray(x, np.float64) + bc(coef[..., 2])


def ref_dx_rounding(x, dact, scale, shift, coef, slope):
    """F of tests/test_wgrad3_fused_host.py's ref_apply: the float32 roundings of the device's expression cA*dh + (cB*x + cC)"""
    coef, x = np.asarray(coef, np.float64), np.asarray(x, np.float64)
    ca, cb, cc = (bc(coef[..., k]) for k in range(3))
    dh = ref_dh(x, dact, scale, shift, slope)
    lin = cb * x + cc
    return 2.0 ** -24 * (np.abs(ca * np.asarray(dact, np.float64) * slope) + np.abs(ca * dh) + np.abs(cb * x) + np.abs(lin) + np.abs(ca * dh + lin)) * (1 + 1e-6)


def split_of(v32):
    """the split form of a float32 NCDHW tensor as ops.to_split_c16 writes it: uint8 [N, C/16, D, H, W, 64]"""
    t = torch.from_numpy(blocks(np.asarray(v32, np.float32)))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.uint8).numpy()


def unblocks(t):
    """voxel-major [N, C/16, D, H, W, 16] -> NCDHW"""
    n, cb, d, h, w, _ = t.shape
    return np.ascontiguousarray(t.transpose(0, 1, 5, 2, 3, 4).reshape(n, cb * 16, d, h, w))


def ref_chain(x, gamma, beta, dact, slope):
    """the whole backward of lrelu(GN(x)) through the links above, every intermediate in float64 -> dict"""
    st = stats_of(x, gamma, beta)
    S = ref_bwd_sums(x, dact, st["scale"], st["shift"], st["mean"], st["rstd"], slope)
    V = int(np.prod(x.shape[2:]))
    fin = ref_bwd_finalize(S, gamma, st["mean"], st["rstd"], V)
    return dict(st, S=S, dx=ref_dx(x, dact, st["scale"], st["shift"], fin["coef"], slope), **fin)


# ---------------------------------------------------------------------------------------------------------------- input builders
def factor(v):
    """(D, H, W) with D * H * W = v (the kernels see only v)"""
    for w in (128, 64, 7, 5, 3):
        if v % w == 0 and v > w:
            for h in (64, 32, 5, 3):
                if (v // w) % h == 0 and v // w > h:
                    return (v // w // h, h, w)
            return (1, v // w, w)
    return (1, 1, v)


_real_cache = {}


def real_case(v, c, kind, n=2):
    """seeded float32 operands of the real family (cached and never written: the GPU tests share them): x off the LeakyReLU kink of (gamma, beta), a residual that is itself
    the raw input of a GroupNorm with parameters (gamma2, beta2) and lies off ITS kink, the upstream gradient dact"""
    key = (v, c, kind, n)
    if key not in _real_cache:
        rng = np.random.default_rng([v, c, n, sorted(("signs", "zeros", "tiny", "ties")).index(kind)])
        gamma, beta = gn_param_set(kind, c, rng)
        gamma2, beta2 = gn_param_set("signs", c, rng)
        shape = (n, c) + factor(v)
        x = gn_off_the_kink((rng.standard_normal(shape) * 2 + 0.5).astype(np.float32), gamma, beta)
        res = gn_off_the_kink((rng.standard_normal(shape) * 1.5 - 0.25).astype(np.float32), gamma2, beta2)
        dact = rng.standard_normal(shape).astype(np.float32)
        case = dict(x=x, res=res, dact=dact, gamma=gamma, beta=beta, gamma2=gamma2, beta2=beta2)
        for a in case.values():
            a.setflags(write=False)
        _real_cache[key] = case
    return _real_cache[key]


def exact_params(kind, c, rng):
    """gn_param_set's sign and zero pattern on powers of two / small integers"""
    g, b = gn_param_set(kind, c, rng)
    gamma = np.sign(g) * rng.choice([0.5, 1.0, 2.0], c)
    beta = np.sign(b) * rng.choice([1.0, 2.0, 3.0], c)
    return gamma.astype(np.float32), beta.astype(np.float32)


def _nonzero(rng, hi, shape):
    return (rng.integers(1, hi + 1, shape) * rng.choice([-1, 1], shape)).astype(np.int64)


def exact_stat_partials(n, c, nblk, kind, seed=0, V=EXACT_V):
    """-> (partials [N, C, nblk, 2] float32, gamma, beta, V): small non-zero integer pairs whose group means are 0 or +-2^k and whose variances are 1, 5/4 or 3/2"""
    rng = np.random.default_rng([n, c, nblk, seed, 1])
    gamma, beta = exact_params(kind, c, rng)
    cpg = c // G
    m = cpg * V
    p = np.stack([_nonzero(rng, 7, (n, c, nblk)), rng.integers(1, 16, (n, c, nblk))], axis=-1)
    flat = p.reshape(n, G, cpg * nblk, 2)                                             # (a view: the pairs of a group are contiguous)
    for i in range(n):
        for g in range(G):
            mu = Fraction(int(rng.choice([0, 1, -1, 2, -2, 4])), int(rng.choice([1, 2, 4])))
            var = Fraction(int(rng.choice([4, 5, 6])), 4)
            j = int(rng.integers(0, cpg * nblk))
            flat[i, g, j, 0] += int(mu * m) - int(flat[i, g, :, 0].sum())
            flat[i, g, j, 1] += int((var + mu * mu) * m) - int(flat[i, g, :, 1].sum())
            if flat[i, g, j, 0] == 0:                                                  # no pair is zero: move one unit between two pairs
                k = (j + 1) % (cpg * nblk)
                if k != j:
                    step = 1 if flat[i, g, k, 0] != 1 else -1
                    flat[i, g, j, 0] += step
                    flat[i, g, k, 0] -= step
    assert np.abs(p).max() < 2 ** 24
    return p.astype(np.float32), gamma, beta, V


def exact_bwd_partials(n, c, nblk, kind, s2_sign, seed=0, V=EXACT_V):
    """-> (partials [N, C, nblk, 2] float32, gamma, mean [N, G], rstd [N, G], V): small non-zero integers; where cpg has an odd factor (C = 48) one entry per sum and group
    is moved until sum_j gamma_j S_j divides by it"""
    rng = np.random.default_rng([n, c, nblk, seed, 2, s2_sign])
    gamma, _ = exact_params(kind, c, rng)
    cpg = c // G
    odd = cpg
    while odd % 2 == 0:
        odd //= 2
    p = _nonzero(rng, 7, (n, c, nblk, 2))
    w = np.rint(2 * gamma.astype(np.float64)).astype(np.int64)                       # 2 * gamma: integers
    for t in (0, 1):
        wt = np.where((gamma < 0) & bool(s2_sign and t == 1), -w, w)
        for i in range(n):
            for g in range(G):
                ch = [j for j in range(g * cpg, (g + 1) * cpg) if wt[j] != 0]
                if odd == 1 or not ch:
                    continue
                tot = lambda: int((wt[g * cpg:(g + 1) * cpg, None] * p[i, g * cpg:(g + 1) * cpg, :, t]).sum())
                j, b = ch[int(rng.integers(0, len(ch)))], int(rng.integers(0, nblk))
                step = 1 if p[i, j, b, t] > 0 else -1                                   # away from zero
                while tot() % odd:
                    p[i, j, b, t] += step
    mean = rng.integers(-2, 3, (n, G)).astype(np.float32)
    rstd = rng.choice([0.5, 1.0, 2.0], (n, G)).astype(np.float32)
    return p.astype(np.float32), gamma, mean, rstd, V


def exact_chain_case(v, c, kind, n=2, seed=0):
    """small-integer operands of the whole backward chain (v a power of two where c = 48 is not used): x in -3..3, dact even in -4..4, integer mean, power-of-two rstd,
    scale = gamma * rstd, shift = beta - mean * scale formed exactly"""
    rng = np.random.default_rng([v, c, n, seed, 3])
    gamma, beta = exact_params(kind, c, rng)
    cpg = c // G
    shape = (n, c) + factor(v)
    x = rng.integers(-3, 4, shape).astype(np.float32)
    dact = (2 * rng.integers(-2, 3, shape)).astype(np.float32)
    mean = rng.integers(-1, 2, (n, G)).astype(np.float32)
    rstd = rng.choice([0.5, 1.0, 2.0], (n, G)).astype(np.float32)
    scale = (gamma[None] * per_channel(rstd, cpg)).astype(np.float32)
    shift = (beta[None] - per_channel(mean, cpg) * scale).astype(np.float32)
    return dict(x=x, dact=dact, gamma=gamma, beta=beta, mean=mean, rstd=rstd, scale=scale, shift=shift)


# ---------------------------------------------------------------------------------------------------------------- the reference against the oracle and autograd
def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


SMALL = [(2, 16, (3, 5, 7), "signs"), (1, 48, (2, 3, 5), "signs"), (2, 32, (1, 4, 9), "zeros"), (2, 16, (2, 2, 3), "ties"), (1, 16, (3, 3, 3), "tiny")]


def _small(i):
    n, c, sp, kind = SMALL[i]
    rng = np.random.default_rng(100 + i)
    gamma, beta = gn_param_set(kind, c, rng)
    g2, b2 = gn_param_set("signs", c, rng)
    x = gn_off_the_kink((rng.standard_normal((n, c) + sp) * 2 + 0.5).astype(np.float32), gamma, beta)
    res = gn_off_the_kink(rng.standard_normal((n, c) + sp).astype(np.float32), g2, b2)
    return x, res, rng.standard_normal((n, c) + sp).astype(np.float32), gamma, beta, g2, b2


def _chunk_partials(x, nblk, centred=False, chunk=None):
    """(sum, sumsq) -- or (sum, M2) -- pairs of x [N, C, ...] over nblk consecutive chunks of its rows, float64"""
    n, c = x.shape[:2]
    rows = np.asarray(x, np.float64).reshape(n, c, -1)
    v = rows.shape[2]
    chunk = chunk or -(-v // nblk)
    out = np.zeros((n, c, nblk, 2))
    for b in range(nblk):
        part = rows[:, :, b * chunk:(b + 1) * chunk]
        out[:, :, b, 0] = part.sum(-1)
        out[:, :, b, 1] = ((part - part.mean(-1, keepdims=True)) ** 2).sum(-1) if centred else (part * part).sum(-1)
    return out


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_finalize_reference_is_the_oracles_group_norm(i):
    x, _, _, gamma, beta, _, _ = _small(i)
    v = int(np.prod(x.shape[2:]))
    _, mu, rstd = O.np_group_norm(x, gamma, beta, eps=EPS)
    for nblk in (1, 3):
        st = ref_finalize(_chunk_partials(x, nblk), gamma, beta, v)
        _close(st["mean"], mu)
        _close(st["rstd"], rstd, 1e-9)                                                # (sumsq / m - mean^2 cancels: 1e-9 of float64 statistics at these sizes)
    st = stats_of(x, gamma, beta)
    y, _, _ = O.np_group_norm(x, gamma, beta)
    _close(np.asarray(x, np.float64) * bc(st["scale"]) + bc(st["shift"]), y)
    # bst_k: u = x*k1 + k2 = sign(gamma) * xhat and `u > thr` is the mask of the pre-activation (where it is not a tie)
    k = st["bst_k"]
    u = np.asarray(x, np.float64) * bc(k[:, 0]) + bc(k[:, 1])
    cpg = x.shape[1] // G
    xh = (np.asarray(x, np.float64) - bc(per_channel(st["mean"], cpg))) * bc(per_channel(st["rstd"], cpg))
    _close(u, np.where(gamma < 0, -1.0, 1.0)[None, :, None, None, None] * xh)
    mask = u > bc(k[:, 2])
    assert np.array_equal(mask, y > 0)


def test_centred_finalize_reference_is_the_oracles_group_norm():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((2, 16, 1, 3, 5500)) + 30.0).astype(np.float32)         # V = 16500: three chunks of 8192, the last ragged
    gamma, beta = gn_param_set("signs", 16, rng)
    _, mu, rstd = O.np_group_norm(x, gamma, beta, eps=EPS)
    st = ref_finalize(_chunk_partials(x, 3, centred=True, chunk=GN_CHUNK), gamma, beta, 16500, centred=True)
    _close(st["mean"], mu)
    _close(st["rstd"], rstd)


@pytest.mark.parametrize("i", range(len(SMALL)))
@pytest.mark.parametrize("slope", [1.0, 0.01])
def test_chain_reference_is_autograd_of_res_plus_lrelu_group_norm(i, slope):
    x, res, dact, gamma, beta, g2, b2 = _small(i)
    gn = lambda t, g, b: torch.nn.functional.group_norm(t, G, g, b, O.GN_EPS)
    act = lambda t, s: torch.where(t > 0, t, t * s)
    st, st2 = stats_of(x, gamma, beta), stats_of(res, g2, b2)
    # forward, the three residual forms
    xt, gt, bt, rt, g2t, b2t = _t(x, True), _t(gamma, True), _t(beta, True), _t(res, True), _t(g2, True), _t(b2, True)
    y0 = act(gn(xt, gt, bt), slope)
    _close(ref_apply(x, st["scale"], st["shift"], slope), y0.detach().numpy())
    _close(ref_apply(x, st["scale"], st["shift"], slope, res), (rt + y0).detach().numpy())
    y2 = act(gn(rt, g2t, b2t), 0.01) + y0
    _close(ref_apply(x, st["scale"], st["shift"], slope, res, st2["scale"], st2["shift"], 0.01), y2.detach().numpy())
    # backward of the RES = 2 form: both GroupNorms get the upstream gradient, each through its own chain
    y2.backward(_t(dact))
    for inp, grad_x, g, b, gg, gb, sl in ((x, xt.grad, gamma, beta, gt.grad, bt.grad, slope), (res, rt.grad, g2, b2, g2t.grad, b2t.grad, 0.01)):
        ch = ref_chain(inp, g, b, dact, sl)
        _close(ch["dx"], grad_x.numpy(), 1e-10)
        _close(ch["dgamma"], gg.numpy(), 1e-10)
        _close(ch["dbeta"], gb.numpy(), 1e-10)
        dh = np.asarray(dact, np.float64) * np.where(O.np_group_norm(inp, g, b)[0] > 0, 1.0, sl)
        dx, dg, db = O.np_group_norm_bwd(inp, g, dh)
        _close(ch["dx"], dx, 1e-10)
        _close(ch["dgamma"], dg, 1e-10)
        _close(ch["dbeta"], db, 1e-10)
        # the sign-carrying sums with s2_sign = 1 finalize to the same
        S = ref_bwd_sums(inp, dact, ch["scale"], ch["shift"], ch["mean"], ch["rstd"], sl, gamma=g)
        fin = ref_bwd_finalize(S, g, ch["mean"], ch["rstd"], int(np.prod(inp.shape[2:])), s2_sign=1)
        _close(fin["coef"], ch["coef"])
        _close(fin["dgamma"], ch["dgamma"])


def test_split_reference_is_what_the_decoder_reads():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((1, 16, 2, 3, 5)) * 3).astype(np.float32)
    dec = split_decode(split_of(v))
    bound = 2.0 ** -16 * np.abs(blocks(v))                                            # two roundings to 8 significant bits
    assert (np.abs(dec - blocks(v).astype(np.float64)) <= bound).all()
    assert np.array_equal(unblocks(blocks(v)), v)


# ---------------------------------------------------------------------------------------------------------------- the exact family is exact
def f32_round(q):
    """a Fraction -> the nearest float32 (ties to even), by integer arithmetic"""
    if q == 0:
        return 0.0
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert -126 <= e <= 127                                                          # (no subnormals or overflow in this family)
    scaled = a / Fraction(2) ** (e - 23)                                              # in [2^23, 2^24)
    k = scaled.numerator // scaled.denominator
    r = scaled - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k % 2):
        k += 1
    return s * float(Fraction(k) * Fraction(2) ** (e - 23))


def _fr(a):
    return Fraction(float(a))


def _is_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


@pytest.mark.parametrize("kind", ["signs", "zeros"])
@pytest.mark.parametrize("n,c,nblk", [(1, 16, 1), (3, 16, 5), (1, 32, 33), (3, 48, 4), (1, 48, 65), (1, 16, 513)])
def test_exact_family_is_exact(n, c, nblk, kind):
    """rational arithmetic on the same inputs: every sum, mean, variance, threshold and backward coefficient equals the float64 reference and is a float32; rstd (and the
    outputs that carry it) are the correctly rounded float32 of the exact value"""
    cpg = c // G
    # ---- statistics
    p, gamma, beta, V = exact_stat_partials(n, c, nblk, kind)
    assert (p != 0).all() and np.array_equal(p, np.rint(p))
    st = ref_finalize(p, gamma, beta, V)
    dv = ref_finalize_device(p, gamma, beta, V)
    assert np.array_equal(dv["mean"], st["mean"]) and np.array_equal(dv["rstd"], st["rstd"].astype(np.float32))
    m = cpg * V
    eps = _fr(np.float32(O.GN_EPS))
    for i in range(n):
        for g in range(G):
            grp = p[i, g * cpg:(g + 1) * cpg]
            s1, s2 = sum(Fraction(int(t)) for t in grp[..., 0].ravel()), sum(Fraction(int(t)) for t in grp[..., 1].ravel())
            mu = s1 / m
            var = s2 / m - mu * mu
            assert _fr(st["mean"][i, g]) == mu and (mu == 0 or abs(mu).numerator == 1 and abs(mu).denominator & (abs(mu).denominator - 1) == 0 or abs(mu).denominator == 1
                                                    and abs(mu).numerator & (abs(mu).numerator - 1) == 0)
            assert var in (Fraction(1), Fraction(5, 4), Fraction(3, 2))
            r32 = np.float32(st["rstd"][i, g])                                        # the float32 the device writes; correctly rounded <=> 1 / (var + eps) lies between
            half = Fraction(float(np.spacing(r32))) / 2                               # the squares of its two rounding boundaries
            r = _fr(r32)
            assert (r - half) ** 2 * (var + eps) <= 1 <= (r + half) ** 2 * (var + eps)
            for j in range(g * cpg, (g + 1) * cpg):
                gm, bt = _fr(gamma[j]), _fr(beta[j])
                assert float(dv["scale"][i, j]) == f32_round(gm * r) == float(gm * r)              # a power of two times rstd: no second rounding
                assert float(dv["shift"][i, j]) == f32_round(bt - mu * gm * r)                     # ONE rounding of an exact product and difference
                sg = -1 if gm < 0 else 1
                assert float(dv["bst_k"][i, 0, j]) == float(sg * r)
                assert float(dv["bst_k"][i, 1, j]) == float(-sg * mu * r) and _is_f32(float(-sg * mu * r))
                thr = float(dv["bst_k"][i, 2, j])
                assert thr == ((-math.inf if bt > 0 else math.inf) if gm == 0 else float(-bt / abs(gm)))
    # ---- backward
    for s2_sign in (0, 1):
        p, gamma, mean, rstd, V = exact_bwd_partials(n, c, nblk, kind, s2_sign)
        assert (p != 0).all() and np.array_equal(p, np.rint(p)) and np.abs(p).max() <= 16
        fin = ref_bwd_finalize(p.astype(np.float64).sum(2), gamma, mean, rstd, V, s2_sign)
        dg, db = [Fraction(0)] * c, [Fraction(0)] * c
        for i in range(n):
            for g in range(G):
                m1 = m2 = Fraction(0)
                for j in range(g * cpg, (g + 1) * cpg):
                    S1 = sum(Fraction(int(t)) for t in p[i, j, :, 0])
                    S2 = sum(Fraction(int(t)) for t in p[i, j, :, 1]) * (-1 if (s2_sign and gamma[j] < 0) else 1)
                    m1 += _fr(gamma[j]) * S1
                    m2 += _fr(gamma[j]) * S2
                    dg[j] += S2
                    db[j] += S1
                m1, m2 = m1 / m, m2 / m
                assert m1.denominator & (m1.denominator - 1) == 0 and m2.denominator & (m2.denominator - 1) == 0        # dyadic: the division was exact
                rs, mu = _fr(rstd[i, g]), _fr(mean[i, g])
                for j in range(g * cpg, (g + 1) * cpg):
                    want = (rs * _fr(gamma[j]), -rs * rs * m2, rs * rs * m2 * mu - rs * m1)
                    assert tuple(_fr(t) for t in fin["coef"][i, j]) == want
        assert [_fr(t) for t in fin["dgamma"]] == dg and [_fr(t) for t in fin["dbeta"]] == db
        assert _is_f32(fin["coef"]) and _is_f32(fin["dgamma"]) and _is_f32(fin["dbeta"])


@pytest.mark.parametrize("c,v", [(16, 2048), (32, 4096)])
def test_exact_chain_sums_are_integers_below_2_24(c, v):
    """the reduction's sums on the exact chain operands: every summand a multiple of 1/4, every sum of |summand| below 2^22 units -- float32 in any order is exact"""
    e = exact_chain_case(v, c, "signs")
    cpg = c // G
    x = e["x"].astype(np.float64)
    assert np.array_equal(e["scale"].astype(np.float64), e["gamma"][None].astype(np.float64) * per_channel(e["rstd"], cpg))
    assert np.array_equal(e["shift"].astype(np.float64), e["beta"][None] - per_channel(e["mean"], cpg).astype(np.float64) * e["scale"])
    dh = ref_dh(x, e["dact"], e["scale"], e["shift"], EXACT_SLOPE)
    xh = (x - bc(per_channel(e["mean"], cpg))) * bc(per_channel(e["rstd"], cpg))
    for t in (dh, dh * xh):
        assert np.array_equal(t * 4, np.rint(t * 4))
        assert np.abs(t * 4).reshape(t.shape[0], c, -1).sum(-1).max() < 2 ** 22
    fin = ref_bwd_finalize(ref_bwd_sums(x, e["dact"], e["scale"], e["shift"], e["mean"], e["rstd"], EXACT_SLOPE), e["gamma"], e["mean"], e["rstd"], v)
    assert _is_f32(fin["coef"]) and _is_f32(fin["dgamma"]) and _is_f32(fin["dbeta"])


def test_real_family_is_off_the_kink_and_cached_read_only():
    a = real_case(105, 16, "zeros")
    assert real_case(105, 16, "zeros") is a and not a["x"].flags.writeable
    pre, _, _ = O.np_group_norm(a["x"], a["gamma"], a["beta"])
    nz = a["gamma"] != 0
    assert np.abs(pre[:, nz]).min() > 1e-6
    assert a["gamma"][0] == 0 and a["beta"][0] > 0 and a["beta"][1] < 0 and a["beta"][2] == 0
    for v in (105, 2049, 32767, 131073, 524289, (1 << 20) - 1, 1 << 20):
        assert int(np.prod(factor(v))) == v
