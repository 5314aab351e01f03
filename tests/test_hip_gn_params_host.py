"""GroupNorm parameters as training leaves them -- the tools of tests/test_hip_gn_params.py and the proof, on the CPU oracle alone, that its bars can fail.

make_params (oracle/resunet_oracle.py) draws gamma from U(.5, 1.5): every sign(gamma) is +1, no gamma is 0, and no pre-activation is exactly 0.  The engine
publishes sign(gamma) * rstd, -sign(gamma) * mean * rstd and the mask threshold -beta / |gamma| (gn_finalize_kernel, fin_tail.hpp) for its fused
GroupNorm-backward statistics; a dropped sign or a wrong inequality there is invisible with such parameters.  edit_gn_params rewrites every norm of a parameter
set into one of three sets; the mutants below are the three errors those sets exist to catch, each made on the oracle and held to 20x the bar the GPU test
computes for the same shape.  Nothing here needs a GPU."""
from collections import OrderedDict
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import resunet_oracle as O

KINDS = ("mixed", "zeros", "ties")
TINY = 1e-6
ZERO_BETAS = (0.3, -0.3, 0.0)


def norm_layers(params):
    """prefixes of every GroupNorm of a parameter set (norm_input included), in state-dict order"""
    return [k[:-len(".weight")] for k in params if ("norm" in k.split(".")[-2]) and k.endswith(".weight") and params[k].ndim == 1]


def special_channels(kind, c, rng):
    """zeros: the five channels of a layer that are not simply mixed-sign -- (three with gamma == 0, two with |gamma| == TINY)"""
    idx = rng.permutation(c)[:5]
    return idx[:3], idx[3:5]


def edit_gn_params(params, kind, seed=0):
    """-> (edited copy of `params`, {layer: dict(zero=, tiny=)} of the special channels).
    mixed: seeded signs on every gamma, exactly half of a layer's channels negative.
    zeros: per layer three channels with gamma = 0 and beta = +0.3, -0.3, 0, two channels with gamma = +1e-6, -1e-6, the rest mixed-sign.
    ties:  beta = 0 everywhere, mixed-sign gamma."""
    assert kind in KINDS, kind
    out = OrderedDict((k, v.copy()) for k, v in params.items())
    special = {}
    for li, layer in enumerate(norm_layers(params)):
        rng = np.random.default_rng([seed, KINDS.index(kind), li])
        gamma, beta = out[layer + ".weight"], out[layer + ".bias"]
        c = gamma.size
        gamma *= np.where(rng.permutation(c) < c // 2, -1.0, 1.0).astype(np.float32)
        special[layer] = dict(zero=np.zeros(0, np.int64), tiny=np.zeros(0, np.int64))
        if kind == "zeros":
            zero, tiny = special_channels(kind, c, rng)
            rest = np.setdiff1d(np.arange(c), np.concatenate([zero, tiny]))
            gamma[rest] = np.abs(gamma[rest]) * np.where(np.arange(rest.size) % 2 == 0, -1.0, 1.0).astype(np.float32)   # both signs among the rest
            gamma[zero] = 0.0
            beta[zero] = ZERO_BETAS
            gamma[tiny] = (TINY, -TINY)
            special[layer] = dict(zero=zero, tiny=tiny)
        elif kind == "ties":
            beta[:] = 0.0
    return out, special


def make_case_input(kind, n, dhw, seed):
    """ties: the LAST sample is all zeros (an all-background patch: the reference's inputs are skull-stripped, zero outside the brain).  No convolution of the
    trunk has a bias, so with beta == 0 every pre-activation of that sample is exactly 0 in float32 and float64 alike -- the only way `>` and `>=` can differ."""
    x = O.make_input(n, *dhw, seed=seed)
    if kind == "ties":
        x[-1] = 0.0
    return x, O.make_target(n, *dhw, seed=seed)


def grad_distance(grads, ref):
    """the metric of test_default_path_shape_sweep_against_the_oracle: max over parameters of max |g - ref| / max |ref|; -> (value, parameter)"""
    worst = (0.0, "")
    for k, r in ref.items():
        if r is None:
            continue
        r = np.asarray(r, np.float64)
        worst = max(worst, (float(np.abs(np.asarray(grads[k], np.float64) - r).max() / (np.abs(r).max() + 1e-12)), k))
    return worst


@functools.lru_cache(maxsize=None)
def oracle_case(cfgname, kind, n, dhw, seed):
    """The oracle's step on edited parameters, once per case: (params, special, x, g, probs, loss, grads, sens, bar).  sens / bar as in
    test_default_path_shape_sweep_against_the_oracle: the oracle runs again with every weight perturbed by 1e-5 relative (zeros stay zeros), bar = max(1e-3, 2 x
    the largest change of a gradient over its largest element)."""
    cfg = CONFIGS[cfgname]
    params, special = edit_gn_params(O.make_params(seed, **cfg), kind, seed)
    x, g = make_case_input(kind, n, dhw, seed)
    probs, loss, grads = O.forward_backward(params, x, g, **cfg)
    rng = np.random.default_rng(seed)
    pert = {k: (v * (1.0 + 1e-5 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in params.items()}
    _, _, pert_grads = O.forward_backward(pert, x, g, **cfg)
    sens = grad_distance(pert_grads, grads)[0]
    return dict(params=params, special=special, x=x, g=g, probs=probs, loss=loss, grads=grads, pert_grads=pert_grads, sens=sens, bar=max(1e-3, 2.0 * sens))


SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)     # tests/test_hip_unet.py
CONFIGS = {"default": O.DEFAULT_CFG, "small": SMALL}


# ---------------------------------------------------------------------------------------------------------------- the editor
def test_parameter_editor_counts_in_every_layer():
    for cfgname, nlayers in (("default", 27), ("small", 15)):
        base = O.make_params(3, **CONFIGS[cfgname])
        layers = norm_layers(base)
        assert len(layers) == nlayers and "norm_input" in layers, layers
        assert sorted(k for k in base if base[k].ndim == 1 and not k.startswith("conv_output")) == sorted(l + s for l in layers for s in (".weight", ".bias"))
        for kind in KINDS:
            p, special = edit_gn_params(base, kind, 3)
            assert list(p) == list(base)
            for k in base:                                   # nothing but the norms is touched, and |gamma| survives wherever it is not set
                if k.rsplit(".", 1)[0] not in layers:
                    assert np.array_equal(p[k], base[k]), k
            for layer in layers:
                gamma, beta, c = p[layer + ".weight"], p[layer + ".bias"], p[layer + ".weight"].size
                assert gamma.dtype == np.float32 and beta.dtype == np.float32
                if kind in ("mixed", "ties"):
                    assert int((gamma < 0).sum()) == c // 2 and int((gamma > 0).sum()) == c - c // 2, (layer, kind)
                    assert np.array_equal(np.abs(gamma), base[layer + ".weight"])
                    assert np.array_equal(beta, base[layer + ".bias"]) if kind == "mixed" else not beta.any()
                else:
                    zero, tiny = special[layer]["zero"], special[layer]["tiny"]
                    assert int((gamma == 0).sum()) == 3 and sorted(np.flatnonzero(gamma == 0)) == sorted(zero)
                    assert tuple(beta[zero]) == tuple(np.float32(b) for b in ZERO_BETAS)
                    assert int((np.abs(gamma) == np.float32(TINY)).sum()) == 2 and gamma[tiny[0]] == np.float32(TINY) and gamma[tiny[1]] == -np.float32(TINY)
                    rest = np.abs(gamma) > 0.4
                    assert int(rest.sum()) == c - 5 and int((gamma[rest] < 0).sum()) == (c - 5 + 1) // 2 and int((gamma[rest] > 0).sum()) == (c - 5) // 2
    # a seed gives the same parameters twice, another seed other signs
    a, _ = edit_gn_params(base, "mixed", 3)
    b, _ = edit_gn_params(base, "mixed", 3)
    c2, _ = edit_gn_params(base, "mixed", 4)
    assert all(np.array_equal(a[k], b[k]) for k in a) and any(not np.array_equal(a[k], c2[k]) for k in a)


def test_fixture_ratio_of_mean_to_std_is_finite_and_positive(golden):
    """R = max |mean| * rstd over every GroupNorm of the reference's own 32^3 step: the bar of test_group_norm_statistics_conditioning (tests/test_hip_ops.py)
    asserts up to 10 R; a fixture without statistics, or with zeros in them, would make that bar vacuous."""
    g = golden("unet32")
    keys = sorted(k for k in g if k.startswith("gnstat_"))
    assert len(keys) == 25
    per_layer = {k: float(np.abs(g[k][0].astype(np.float64) * g[k][1].astype(np.float64)).max()) for k in keys}
    R = max(per_layer.values())
    print("  R = %.4f (%s)" % (R, max(per_layer, key=per_layer.get)))
    assert all(np.isfinite(v) and v > 0 for v in per_layer.values())
    assert np.isfinite(R) and 1.0 < R < 100.0          # 2.03 (decoder_convs.0.0.norm1): ratios 0, 3 and 10 of the conditioning test are asserted


# ---------------------------------------------------------------------------------------------------------------- mutants
class _MaskedLeaky(torch.autograd.Function):
    """LeakyReLU whose BACKWARD takes a mask of the caller's choosing (the forward is the true one)"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return F.leaky_relu(x, O.LEAKY_SLOPE)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return torch.where(mask, dy, dy * O.LEAKY_SLOPE), None


def mutant_grads(case, cfg, mask_of):
    """the oracle's gradients with the LeakyReLU-after-GroupNorm mask of the backward replaced by mask_of(xhat, gamma, beta)"""
    pending = []
    true_gn, true_lrelu = O.group_norm, O.leaky_relu

    def gn(x, gamma, beta):
        xhat = F.group_norm(x.detach(), O.GN_GROUPS, None, None, O.GN_EPS)
        shape = (1, -1, 1, 1, 1)
        pending[:] = [mask_of(xhat, gamma.detach().reshape(shape), beta.detach().reshape(shape))]
        return true_gn(x, gamma, beta)

    def lrelu(x):
        if not pending:
            return true_lrelu(x)                 # the activation behind the up-sampling 1x1 (model.py:422): no GroupNorm in front of it
        return _MaskedLeaky.apply(x, pending.pop())

    O.group_norm, O.leaky_relu = gn, lrelu
    try:
        _, _, grads = O.forward_backward(case["params"], case["x"], case["g"], **cfg)
    finally:
        O.group_norm, O.leaky_relu = true_gn, true_lrelu
    return grads


MUTANT_SHAPE = (2, (16, 16, 16))
MUTANT_SEED = 1            # of seeds 1..12 the bar of the mixed set at this shape ranges 0.03 .. 0.21 (2 x 8 voxels per channel at the deepest level); 1, 7 and 12 leave the most room


def test_mutants_fall_far_outside_the_bar():
    """Three errors a fused GroupNorm-backward chain can make, produced on the CPU oracle at 2 x 16^3 (seed 1), each against the bar the GPU test computes for the
    same case (max(1e-3, 2 x sensitivity)); each must miss it by 20x or more.  Measured (seed 1): (i) 69x, (ii) 72x, (iii) beyond 1e30x -- with >= the all-zero
    sample passes its gradient through every GroupNorm (rstd = eps^-1/2 = 316 where the variance is 0) without the LeakyReLU slope of 0.01 in between.
    (i)   mixed: dgamma negated on the negative-gamma channels (the sign not undone in the reduce tail).
    (ii)  mixed: the mask taken as if gamma were |gamma| (u = xhat instead of sign(gamma) * xhat against the threshold -beta / |gamma|).
    (iii) ties: the mask taken with >= instead of > (exact zeros: the all-zero last sample, make_case_input).
    The identity mutant (the true mask, recomputed from xhat through the same patch) must stay inside the bar, or the patch itself would be what differs."""
    cfg = O.DEFAULT_CFG
    n, dhw = MUTANT_SHAPE
    mixed = oracle_case("default", "mixed", n, dhw, MUTANT_SEED)
    ties = oracle_case("default", "ties", n, dhw, MUTANT_SEED)
    same = mutant_grads(mixed, cfg, lambda xh, ga, be: ga * xh + be > 0)
    d0 = grad_distance(same, mixed["grads"])
    print("  identity mutant: distance %.3e (%s), bar %.3e" % (d0 + (mixed["bar"],)))
    assert d0[0] <= mixed["bar"], d0

    m1 = OrderedDict((k, None if v is None else v.copy()) for k, v in mixed["grads"].items())
    for layer in norm_layers(mixed["params"]):
        if m1[layer + ".weight"] is not None:
            neg = mixed["params"][layer + ".weight"] < 0
            m1[layer + ".weight"][neg] *= -1.0
    m2 = mutant_grads(mixed, cfg, lambda xh, ga, be: ga.abs() * xh + be > 0)
    m3 = mutant_grads(ties, cfg, lambda xh, ga, be: ga * xh + be >= 0)
    rows = [("(i) dgamma sign", grad_distance(m1, mixed["grads"]), mixed["bar"]), ("(ii) mask of |gamma|", grad_distance(m2, mixed["grads"]), mixed["bar"]),
            ("(iii) >= at ties", grad_distance(m3, ties["grads"]), ties["bar"])]
    for name, (dist, where), bar in rows:
        print("  mutant %-22s distance %.3e (%s)  bar %.3e  ratio %.0f" % (name, dist, where, bar, dist / bar))
    for name, (dist, where), bar in rows:
        assert dist >= 20 * bar, (name, dist, bar)
