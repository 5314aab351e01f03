"""Intensity augmentation, host side (no GPU): the float64 restatements of brats2019_amd.dataloader against scipy, the noise generator, the
pointwise stages' invariants, the draws of `draw_intensity_params` and the reader option's promise to leave the global random streams alone."""
import random

import numpy as np
import pytest
from scipy import ndimage as ndi

from brats2019_amd import dataloader as DL

SHAPES = ((5, 6, 7), (16, 40, 24), (33, 20, 70))


def _channel(shape, seed=0):
    return np.random.default_rng(seed + sum(shape)).standard_normal(shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", (0.5, 1.0, 2.0))
def test_blur_matches_scipy(shape, sigma):
    """sigma 2.0 on (5, 6, 7): radius 8 exceeds every extent, the extension is periodic beyond one reflection"""
    x = _channel(shape)
    err = float(np.abs(DL.intensity_blur_host(x, sigma) - ndi.gaussian_filter(x, sigma, mode="reflect")).max())
    print("blur %s sigma %g (radius %d): max |restatement - scipy| = %.3e" % (shape, sigma, DL.elastic_radius(sigma), err))
    assert err <= 1e-12
    assert DL.elastic_radius(2.0) == 8 > max((5, 6, 7))


@pytest.mark.parametrize("shape,zoom", (((5, 6, 7), 0.5), ((16, 40, 24), 0.63), ((33, 20, 70), 0.77), ((9, 9, 9), 0.05)))
def test_lowres_matches_two_zooms(shape, zoom):
    x = _channel(shape, 1)
    nc = [max(1, int(np.floor(n * zoom + 0.5))) for n in shape]
    coarse = ndi.zoom(x, [a / b for a, b in zip(nc, shape)], order=0, mode="nearest", grid_mode=True)
    assert coarse.shape == tuple(nc)
    if zoom == 0.05:
        assert nc == [1, 1, 1]
    want = ndi.zoom(coarse, [b / a for a, b in zip(nc, shape)], order=1, mode="nearest", grid_mode=True)
    err = float(np.abs(DL.intensity_lowres_host(x, zoom) - want).max())
    print("low-res %s zoom %g (coarse %s): max |restatement - scipy| = %.3e" % (shape, zoom, nc, err))
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_lowres_zoom_one_is_the_identity(shape):
    x = _channel(shape, 2)
    assert np.array_equal(DL.intensity_lowres_host(x, 1.0), x)


def test_noise_generator():
    n = 64 ** 3
    a = DL.intensity_noise_host(11, 2, n)
    assert a.dtype == np.float64 and np.array_equal(a, DL.intensity_noise_host(11, 2, n))          # identical across calls
    assert np.array_equal(a[:5 * 6 * 7], DL.intensity_noise_host(11, 2, 5 * 6 * 7))                # common prefix across shapes
    assert not np.array_equal(a[:1000], DL.intensity_noise_host(12, 2, 1000))                      # seeds differ
    assert not np.array_equal(a[:1000], DL.intensity_noise_host(11, 3, 1000))                      # channels differ
    assert np.isfinite(a).all()
    mean, var = float(a.mean()), float(a.var())
    print("noise N = %d: mean %.3e (standard error %.3e), variance %.6f (standard error %.3e)" % (n, mean, n ** -0.5, var, (2.0 / n) ** 0.5))
    assert abs(mean) <= 6 * n ** -0.5
    assert abs(var - 1.0) <= 6 * (2.0 / n) ** 0.5
    big = (1 << 64) - 3                                              # the seed wraps in 64 bits
    assert np.array_equal(DL.intensity_noise_host(big, 0, 100), DL.intensity_noise_host(big - (1 << 64), 0, 100))
    x = np.zeros((1, 4, 5, 6))
    out = DL.intensity_augment_host(x, [dict(noise_variance=0.04, noise_seed=7)])
    assert np.array_equal(out[0].ravel(), 0.2 * DL.intensity_noise_host(7, 0, 120))                # linear voxel index, sqrt(variance)


def test_pointwise_stages():
    x = _channel((16, 40, 24), 3)
    assert np.abs(DL.intensity_contrast_host(x, 1.0) - x).max() <= 4e-15       # (x - mean) + mean: the identity up to float64 rounding
    for f in (0.75, 1.25):
        y = DL.intensity_contrast_host(x, f)
        assert y.min() >= x.min() and y.max() <= x.max()
    assert (DL.intensity_contrast_host(x, 1.25) == x.max()).sum() >= 1 and (DL.intensity_contrast_host(x, 1.25) == x.min()).sum() >= 1      # the clip binds
    rng = x.max() - x.min()
    for invert in (False, True):
        assert np.abs(DL.intensity_gamma_host(x, 1.0, invert) - x).max() <= 1e-6 * rng
        for g in (0.7, 1.5):
            y = DL.intensity_gamma_host(x, g, invert)
            assert y.min() >= x.min() - 1e-6 * rng and y.max() <= x.max() + 1e-6 * rng and not np.allclose(y, x)
            z = DL.intensity_gamma_host(x, g, invert, retain_stats=True)
            print("gamma %g invert %s retain-stats: mean %.3e -> %.3e, std %.6f -> %.6f" % (g, invert, x.mean(), z.mean(), x.std(), z.std()))
            assert abs(z.mean() - x.mean()) <= 1e-9 and abs(z.std() - x.std()) <= 1e-9
    brt = DL.intensity_augment_host(x[None], [dict(brightness=1.2)])[0]
    assert np.array_equal(brt, x * 1.2)
    assert np.array_equal(DL.intensity_augment_host(x[None].astype(np.float32), [dict()])[0], x.astype(np.float32).astype(np.float64))


def test_order_of_the_stages():
    """blur, low-res, noise, brightness, contrast, gamma: the whole call equals the single stages chained in that order"""
    x = _channel((9, 10, 12), 4)[None]
    q = dict(blur_sigma=0.8, lowres_zoom=0.7, noise_variance=0.05, noise_seed=5, brightness=1.1, contrast=1.2, gamma=0.8, gamma_invert=True, gamma_retain_stats=True)
    want = x
    for keys in (("blur_sigma",), ("lowres_zoom",), ("noise_variance", "noise_seed"), ("brightness",), ("contrast",), ("gamma", "gamma_invert", "gamma_retain_stats")):
        want = DL.intensity_augment_host(want, [{k: q[k] for k in keys}])
    assert np.array_equal(DL.intensity_augment_host(x, [q]), want)


def test_argument_checks():
    x = np.zeros((2, 4, 4, 4))
    for q, what in ((dict(blur_sigma=0.0), "sigma"), (dict(blur_sigma=float("nan")), "sigma"), (dict(blur_sigma=2.5), "radius"), (dict(lowres_zoom=0.0), "zoom"),
                    (dict(lowres_zoom=1.5), "zoom"), (dict(noise_variance=-0.1, noise_seed=1), "variance"), (dict(noise_variance=0.1), "noise_seed"),
                    (dict(gamma=0.0), "gamma"), (dict(gamma_invert=True), "gamma"), (dict(sharpen=1.0), "unknown")):
        with pytest.raises(ValueError, match=what):
            DL.intensity_augment_host(x, [q, {}])
    with pytest.raises(ValueError, match="per channel"):
        DL.intensity_augment_host(x, [{}])
    with pytest.raises(ValueError, match="channels"):
        DL.intensity_augment_host(np.zeros((9, 2, 2, 2)), [{}] * 9)


def test_draws_are_seeded_and_follow_the_configuration():
    cfg = DL.IntensityConfig()
    assert (cfg.p_blur, cfg.p_blur_channel, cfg.blur_sigma) == (0.2, 0.5, (0.5, 1.0)) and (cfg.p_lowres, cfg.p_lowres_channel, cfg.lowres_zoom) == (0.25, 0.5, (0.5, 1.0))
    assert (cfg.p_noise, cfg.noise_variance) == (0.1, (0.0, 0.1)) and (cfg.p_brightness, cfg.brightness) == (0.15, (0.75, 1.25))
    assert (cfg.p_contrast, cfg.contrast) == (0.15, (0.75, 1.25)) and (cfg.p_gamma_invert, cfg.p_gamma, cfg.gamma, cfg.gamma_retain_stats) == (0.1, 0.3, (0.7, 1.5), True)
    a = [DL.draw_intensity_params(4, r) for r in [random.Random(5)] for _ in range(50)]
    b = [DL.draw_intensity_params(4, r) for r in [random.Random(5)] for _ in range(50)]
    assert a == b and a != [DL.draw_intensity_params(4, r) for r in [random.Random(6)] for _ in range(50)]
    n = 4000
    rng = random.Random(1)
    draws = [DL.draw_intensity_params(4, rng) for _ in range(n)]
    first = [d[0] for d in draws]                                    # channel 0 of every draw: independent trials
    p_gamma_any = 1.0 - (1.0 - cfg.p_gamma_invert) * (1.0 - cfg.p_gamma)
    for what, hit, p in (("blur", lambda q: "blur_sigma" in q, cfg.p_blur * cfg.p_blur_channel), ("low-res", lambda q: "lowres_zoom" in q, cfg.p_lowres * cfg.p_lowres_channel),
                         ("noise", lambda q: "noise_variance" in q, cfg.p_noise), ("brightness", lambda q: "brightness" in q, cfg.p_brightness),
                         ("contrast", lambda q: "contrast" in q, cfg.p_contrast), ("gamma", lambda q: "gamma" in q, p_gamma_any),
                         ("inverted gamma", lambda q: bool(q.get("gamma_invert")), cfg.p_gamma_invert)):
        f = sum(1 for q in first if hit(q)) / n
        se = (p * (1.0 - p) / n) ** 0.5
        print("%-15s frequency %.4f, configured %.4f, standard error %.4f" % (what, f, p, se))
        assert abs(f - p) <= 5 * se
    for what, hit, p in (("blur", lambda d: any("blur_sigma" in q for q in d), cfg.p_blur * (1.0 - (1.0 - cfg.p_blur_channel) ** 4)),
                         ("low-res", lambda d: any("lowres_zoom" in q for q in d), cfg.p_lowres * (1.0 - (1.0 - cfg.p_lowres_channel) ** 4))):
        f = sum(1 for d in draws if hit(d)) / n                      # per patch: the per-patch draw fired and picked at least one of 4 channels
        assert abs(f - p) <= 5 * (p * (1.0 - p) / n) ** 0.5, what
    ranges = dict(blur_sigma=cfg.blur_sigma, lowres_zoom=cfg.lowres_zoom, noise_variance=cfg.noise_variance, brightness=cfg.brightness, contrast=cfg.contrast,
                  gamma=cfg.gamma)
    seen = set()
    for d in draws:
        assert len(d) == 4
        DL._check_intensity_params(d, 4)
        for q in d:
            for key, (lo, hi) in ranges.items():
                if key in q:
                    assert lo <= q[key] <= hi
                    seen.add(key)
            if "noise_variance" in q:
                assert 0 <= q["noise_seed"] < 1 << 63
            if "gamma" in q:
                assert q["gamma_retain_stats"] is True
            else:
                assert "gamma_invert" not in q and "gamma_retain_stats" not in q
    assert seen == set(ranges)
    assert len({q["noise_seed"] for d in draws for q in d if "noise_seed" in q}) > 100             # a seed per channel and patch
    one = DL.IntensityConfig(p_blur=1, p_blur_channel=1, p_lowres=1, p_lowres_channel=1, p_noise=1, p_brightness=1, p_contrast=1, p_gamma_invert=1, p_gamma=1)
    for q in DL.draw_intensity_params(3, random.Random(2), one):
        assert set(q) == set(DL.INTENSITY_KEYS) and q["gamma_invert"] is True                      # both gamma draws fired: the inverted one wins


def test_global_random_streams_are_not_touched(monkeypatch):
    """constructing the reader and drawing a patch's parameters consume the same global draws with and without the intensity option; no device needed"""
    counts = {}

    def counted(name, fn):
        def wrapper(*args, **kw):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kw)
        return wrapper

    monkeypatch.setattr(random, "random", counted("random.random", random.random))
    monkeypatch.setattr(np.random, "rand", counted("np.random.rand", np.random.rand))
    monkeypatch.setattr(np.random, "uniform", counted("np.random.uniform", np.random.uniform))
    bbox = np.array([[20.0, 20.0, 20.0], [40.0, 40.0, 40.0]])
    one = DL.IntensityConfig(p_blur=1, p_blur_channel=1, p_lowres=1, p_lowres_channel=1, p_noise=1, p_brightness=1, p_contrast=1, p_gamma_invert=1, p_gamma=1)
    seen, states, params = {}, {}, {}
    for name, kw in (("plain", {}), ("off", dict(intensity=False)), ("defaults", dict(intensity=True, intensity_seed=3)), ("all", dict(intensity=one, intensity_seed=3)),
                     ("elastic", dict(intensity=one, intensity_seed=3, elastic=True, elastic_seed=3))):
        counts.clear()
        random.seed(9)
        np.random.seed(9)
        rd = DL.SimpleReader([], (16, 16, 16), device="cpu", **kw)
        for _ in range(3):
            p = DL.draw_augment_params(bbox, rd.patch_size, 4, elastic=rd.elastic, elastic_rng=rd.elastic_rng)
            if rd.intensity is not None:
                q = DL.draw_intensity_params(4, rd.intensity_rng, rd.intensity)
        seen[name], states[name], params[name] = dict(counts), (random.getstate(), np.random.get_state()[1].copy()), p
        assert (rd.intensity is None) == (name in ("plain", "off"))
    assert seen["plain"] == {"random.random": 3 * 9, "np.random.rand": 3, "np.random.uniform": 6}
    for name in seen:
        assert seen[name] == seen["plain"], name
        assert states[name][0] == states["plain"][0] and np.array_equal(states[name][1], states["plain"][1]), name
        for key in ("crop_lo", "scale", "flips", "transpose", "gain", "bias"):
            assert np.array_equal(np.asarray(params[name][key]), np.asarray(params["plain"][key])), (name, key)
    assert all(set(c) == set(DL.INTENSITY_KEYS) for c in q)
