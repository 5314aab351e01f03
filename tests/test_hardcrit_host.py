"""The float64 host restatements of the focal, Tversky and top-k losses (loss.focal_host, tversky_host, topk_host) against straightforward
float64 torch expressions and their autograd, the parameter checks, the declarations of the device entries, and the property of the
committed top-k inputs that tests/test_hardcrit.py and tests/test_flat_passes.py rely on.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import flat_sweep as F
import hardcrit_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
RTOL = 1e-12


def _operands(p):
    """x (float64, requires grad) and the two log arguments with the float32 rounding of p + 1e-6 and (1 + 1e-6) - p carried as constants"""
    x = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    pe32 = torch.from_numpy((p + np.float32(1e-6)).astype(np.float64))
    qe32 = torch.from_numpy((np.float32(1.0 + 1e-6) - p).astype(np.float64))
    pe = x + (pe32 - x.detach())
    qe = (qe32 + x.detach()) - x
    return x, pe, qe


def _bce_elements(p, g, bg_weight):
    x, pe, qe = _operands(p)
    y = torch.from_numpy(g.astype(np.float64))
    return x, -(y * torch.log(pe) + bg_weight * (1.0 - y) * torch.log(qe))


def _close(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= RTOL, (what, err)


@pytest.mark.parametrize("gamma", [0, 1, 2, 2.5])
@pytest.mark.parametrize("alpha", [None, 0.25])
@pytest.mark.parametrize("bg_weight", I.BG_WEIGHTS)
def test_focal_host_matches_float64_autograd(gamma, alpha, bg_weight):
    from brats2019_amd import loss as L
    p, g = I.make((2, 3, 5, 6, 7))
    x, pe, qe = _operands(p)
    y = torch.from_numpy(g.astype(np.float64))
    a1, a0 = (1.0, 1.0) if alpha is None else (alpha, 1.0 - alpha)
    ref = -(a1 * y * (1.0 - x) ** gamma * torch.log(pe) + a0 * bg_weight * (1.0 - y) * x ** gamma * torch.log(qe)).mean()
    (dref,) = torch.autograd.grad(ref, x)
    value, dp = L.focal_host(p, g, gamma=gamma, alpha=alpha, bg_weight=bg_weight)
    assert abs(value - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    _close(dp, dref.numpy(), "dp")
    assert dp.shape == p.shape and dp.dtype == np.float64


@pytest.mark.parametrize("bg_weight", I.BG_WEIGHTS)
def test_focal_gamma_0_and_topk_100_are_the_bce_expression(bg_weight):
    from brats2019_amd import loss as L
    p, g = I.make((2, 3, 5, 6, 7))
    x, l = _bce_elements(p, g, bg_weight)
    ref = l.mean()
    (dref,) = torch.autograd.grad(ref, x)
    for value, dp in (L.focal_host(p, g, gamma=0, alpha=None, bg_weight=bg_weight), L.topk_host(p, g, k=100, bg_weight=bg_weight)):
        assert abs(value - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
        _close(dp, dref.numpy(), "dp")


@pytest.mark.parametrize("alpha,beta,gamma,priority", [(0.5, 0.5, 1.0, 1), (0.3, 0.7, 4.0 / 3.0, 1), (0.3, 0.7, 1.0, 2)])
def test_tversky_host_matches_float64_autograd(alpha, beta, gamma, priority):
    from brats2019_amd import loss as L
    p, g = I.make((2, 3, 5, 6, 7))
    x = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    y = torch.from_numpy(g.astype(np.float64))
    tp = (x * y).sum(dim=(0, 2, 3, 4))
    fp, fn = x.sum(dim=(0, 2, 3, 4)) - tp, y.sum(dim=(0, 2, 3, 4)) - tp
    ti = (tp + 1.0) / (tp + alpha * fp + beta * fn + 1.0)
    ref = priority * ((1.0 - ti) ** (1.0 / gamma)).mean()
    (dref,) = torch.autograd.grad(ref, x)
    value, dp = L.tversky_host(p, g, alpha=alpha, beta=beta, gamma=gamma, smooth=1.0, priority=priority)
    assert abs(value - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    _close(dp, dref.numpy(), "dp")
    if (alpha, beta, gamma) == (0.5, 0.5, 1.0):                        # Tversky(1/2, 1/2) is the Dice of sum p + sum g
        dice = 1.0 - ((2 * tp + 2.0) / (x.sum(dim=(0, 2, 3, 4)) + y.sum(dim=(0, 2, 3, 4)) + 2.0)).mean()
        assert abs(value - float(dice.detach())) <= RTOL


@pytest.mark.parametrize("k", I.KS)
@pytest.mark.parametrize("bg_weight", I.BG_WEIGHTS)
def test_topk_host_matches_torch_topk(k, bg_weight):
    from brats2019_amd import loss as L
    p, g = I.make(I.ODD)
    x, l = _bce_elements(p, g, bg_weight)
    K = max(1, int(l.numel() * k / 100))
    ref = torch.topk(l.reshape(-1), K).values.mean()
    (dref,) = torch.autograd.grad(ref, x)
    value, dp = L.topk_host(p, g, k=k, bg_weight=bg_weight)
    assert abs(value - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    assert int((dp != 0).sum()) == K == int((dref != 0).sum())       # no float64 tie at the threshold in these inputs
    _close(dp, dref.numpy(), "dp")


def test_topk_host_shares_a_tie_symmetrically():
    from brats2019_amd import loss as L
    p, g = I.make_ties()
    l, K, t, n_gt, n_eq = L.topk_host_threshold(p, g, k=30, bg_weight=1)
    assert len(np.unique(l)) <= 6 and n_gt < K < n_gt + n_eq, "K must cut through a tie class"
    value, dp = L.topk_host(p, g, k=30, bg_weight=1)
    x, lt = _bce_elements(p, g, 1)
    ref = torch.topk(lt.reshape(-1), K).values.mean()                  # the value does not depend on which tied elements are taken
    assert abs(value - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    assert abs(value - (l[l > t].sum() + (K - n_gt) * t) / K) <= RTOL * value
    dl = (1.0 - g.astype(np.float64)) / (np.float32(1.0 + 1e-6) - p).astype(np.float64) - g.astype(np.float64) / (p + np.float32(1e-6)).astype(np.float64)
    tied = l == t
    np.testing.assert_allclose(dp[tied] / dl[tied], (K - n_gt) / (n_eq * K), rtol=RTOL)
    np.testing.assert_allclose(dp[l > t] / dl[l > t], 1.0 / K, rtol=RTOL)
    assert not dp[l < t].any()


def test_topk_host_ranks_nan_highest():
    from brats2019_amd import loss as L
    p, g = I.make((1, 1, 2, 3, 4))
    p = p.copy()
    p[0, 0, 0, 0, 0] = np.nan
    assert np.isnan(L.topk_host(p, g, k=10)[0]) and np.isnan(L.topk_host(p, g, k=100)[0])


def test_parameter_checks_raise():
    from brats2019_amd import loss as L
    p, g = I.make(I.TINY)
    for gamma in (0.5, -1.0, 0.999):
        with pytest.raises(ValueError):
            L.FocalLoss(gamma=gamma)
        with pytest.raises(ValueError):
            L.focal_host(p, g, gamma=gamma)
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(gamma=0.5), dict(smooth=0.0), dict(smooth=-1.0)):
        with pytest.raises(ValueError):
            L.TverskyLoss(**kw)
        with pytest.raises(ValueError):
            L.tversky_host(p, g, **kw)
    for k in (0.0, -1.0, 100.5):
        with pytest.raises(ValueError):
            L.TopKLoss(k=k)
        with pytest.raises(ValueError):
            L.topk_host(p, g, k=k)
    for cls in (L.FocalLoss, L.TverskyLoss, L.TopKLoss):
        assert cls().data_parallel is False and cls not in L._TERM_CLASSES
    assert L.fuse_criterion_list([L.Dice_loss_joint(), L.TopKLoss()]) is None      # a list with a new class is evaluated as written
    assert L.FocalLoss(gamma=0).gamma == 0 and L.FocalLoss(gamma=1).gamma == 1 and L.TverskyLoss(gamma=4 / 3).gamma == 4 / 3


def test_header_ctypes_table_and_sources_declare_the_entries():
    from brats2019_amd import _lib as L, build as B
    text = open(HEADER).read()
    for name in ("ru_focal_sum", "ru_focal_grad", "ru_tversky_eval", "ru_topk_select", "ru_topk_grad"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
    for name in ("ru_focal_workspace_bytes", "ru_topk_workspace_bytes"):
        assert re.search(r"\bsize_t %s\(size_t n\);" % name, text) and len(L.SIGNATURES[name][1]) == 1, name
    assert B.SOURCES[-1] == "hardcrit.hip" and os.path.exists(os.path.join(B.CSRC, "hardcrit.hip"))


def test_committed_topk_inputs_leave_few_elements_near_the_threshold():
    """tests/test_hardcrit.py leaves out of its gradient comparison the elements whose float64 l lies within t * (1 +- BAND): a float32 l may
    put those on either side of the threshold.  For the committed seed there are at most BAND_CAP of them, for every k and bg_weight."""
    from brats2019_amd import loss as L
    p, g = I.make(I.ODD)
    assert p.size == 71706
    for bg_weight in I.BG_WEIGHTS:
        for k in I.KS:
            l, K, t, n_gt, n_eq = L.topk_host_threshold(p, g, k=k, bg_weight=bg_weight)
            assert n_eq == 1 and n_gt == K - 1                        # no float64 tie at the threshold
            near = int((np.abs(l - t) <= I.BAND * abs(t)).sum())
            assert 1 <= near <= I.BAND_CAP, (bg_weight, k, near)


def test_sweep_topk_inputs_leave_few_elements_near_the_threshold():
    """the same property for the inputs of tests/test_flat_passes.py's top-k sweep up to 4099 elements (and its case with pointers at
    different offsets), where the gradient is compared element by element outside the band; K is max(1, n // 10) there"""
    from brats2019_amd import loss as L
    for n, off in [c for c in F.SWEEP if c[0] <= 4099] + [(F.MIXED_N, 4)]:
        p, g = F.probabilities(n, off)
        K, k, bg_weight = F.topk_case(n, off)
        l, K_h, t, n_gt, n_eq = L.topk_host_threshold(p, g, k=k, bg_weight=bg_weight)
        assert K_h == K and n_eq == 1 and n_gt == K - 1               # no float64 tie at the threshold
        near = int((np.abs(l - t) <= I.BAND * abs(t)).sum())
        assert 1 <= near <= I.BAND_CAP, (n, off, near)
