"""Intensity augmentation on the device (csrc/intensity.hip: `ru_intensity_augment` behind `dataloader.intensity_augment`) against the float64
restatement `dataloader.intensity_augment_host` on the same float32 input, stage by stage and all together; determinism; the refusals; the
reader option.  The device works in float32 and the oracle in float64: every bar below is 4x the largest error measured on an MI355X for that
stage over the cases of this file (measured value and bar side by side at BARS; also in profiles/intensity_time.txt), and none exceeds 1e-4
on these unit-variance inputs.  No voxel is left out of a comparison."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy

SHAPES = ((5, 6, 7), (16, 40, 24), (33, 20, 70))       # odd and smaller than the radius; 16-byte rows; rows that are no multiple of 4.  Each is ONE 32 x 128 tile per slice (cdiv(20, 32) * cdiv(70, 128) = 1): the tile rows and columns are tests/test_intensity_f64.py's

# stage: (largest |device - host| measured on an MI355X over this file's cases, bar = 4 x measured)
BARS = {
    "blur": (4.746e-07, 1.898e-06),
    "lowres": (4.318e-07, 1.727e-06),
    "noise": (1.126e-06, 4.504e-06),
    "brightness": (2.384e-07, 9.536e-07),
    "contrast": (2.648e-07, 1.059e-06),
    "gamma": (1.490e-06, 5.960e-06),
    "gamma_retain": (1.281e-06, 5.124e-06),
    "all": (5.421e-06, 2.168e-05),
}
assert all(bar <= 1e-4 for _, bar in BARS.values())


@functools.lru_cache(maxsize=None)
def _input(shape):
    """[4, *shape] float32, unit variance, one array per shape for every test (read-only)"""
    x = np.random.default_rng(sum(shape)).standard_normal((4,) + tuple(shape)).astype(np.float32)
    x.setflags(write=False)
    return x


def _check(shape, params, stage):
    """device against host on every voxel; stage-less channels bit for bit; a second call gives the same bytes"""
    from brats2019_amd import dataloader as DL
    x = _input(shape)
    dev = T(x.copy()).cuda()
    got_t = DL.intensity_augment(dev, params)
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == x.shape and got_t.data_ptr() != dev.data_ptr()
    assert torch.equal(dev.cpu(), T(x.copy()))                       # the input is not written
    got = got_t.cpu().numpy()
    want = DL.intensity_augment_host(x, params)
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    measured, bar = BARS[stage]
    print("%-12s %-12s %s: max |device - host| = %.3e (measured on MI355X %.3e, bar %.3e)" % (stage, shape, [sorted(q.items()) for q in params if q], err, measured, bar))
    for c, q in enumerate(params):
        if not q:
            assert got[c].tobytes() == x[c].tobytes(), "channel %d carries no stage and must be a bit-exact copy" % c
        else:
            assert not np.array_equal(got[c], x[c]), "channel %d: the stage did nothing" % c
    assert torch.equal(DL.intensity_augment(dev, params), got_t), "two calls must give identical bytes"
    assert err <= bar
    return got, want


def _only(channel, q):
    return [q if c == channel else {} for c in range(4)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", (0.5, 1.0, 2.0))
def test_blur(shape, sigma):
    """sigma 2.0: radius 8 > every extent of (5, 6, 7)"""
    _check(shape, _only(SHAPES.index(shape), dict(blur_sigma=sigma)), "blur")        # measured / bar: BARS["blur"]


@pytest.mark.parametrize("shape,zoom", (((5, 6, 7), 0.5), ((16, 40, 24), 0.63), ((33, 20, 70), 0.77), ((9, 9, 9), 0.05)))
def test_lowres(shape, zoom):
    got, _ = _check(shape, _only(3, dict(lowres_zoom=zoom)), "lowres")               # measured / bar: BARS["lowres"]
    if zoom == 0.05:
        assert np.unique(got[3]).size == 1                           # one coarse sample: the channel is constant


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", (1, (1 << 64) - 5))
def test_noise(shape, seed):
    got, _ = _check(shape, _only(1, dict(noise_variance=0.1, noise_seed=seed)), "noise")         # measured / bar: BARS["noise"]
    other, _ = _check(shape, _only(2, dict(noise_variance=0.1, noise_seed=seed)), "noise")
    x = _input(shape)
    assert not np.array_equal(got[1] - x[1], other[2] - x[2])        # the channel index enters the generator


@pytest.mark.parametrize("shape", SHAPES)
def test_brightness(shape):
    _check(shape, _only(0, dict(brightness=1.25)), "brightness")     # measured / bar: BARS["brightness"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("factor", (0.75, 1.25))
def test_contrast(shape, factor):
    got, _ = _check(shape, _only(2, dict(contrast=factor)), "contrast")              # measured / bar: BARS["contrast"]
    x = _input(shape)[2]
    assert got[2].min() >= x.min() and got[2].max() <= x.max()       # the clip bounds are the channel's exact min and max
    if factor > 1:
        assert (got[2] == x.max()).any() and (got[2] == x.min()).any()               # and the clip binds


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("retain", (False, True))
@pytest.mark.parametrize("invert", (False, True))
@pytest.mark.parametrize("g", (0.7, 1.5))
def test_gamma(shape, g, invert, retain):
    q = dict(gamma=g, gamma_invert=invert, gamma_retain_stats=retain)
    got, _ = _check(shape, _only(0, q), "gamma_retain" if retain else "gamma")       # measured / bar: BARS["gamma"], BARS["gamma_retain"]
    if retain:
        x = _input(shape)[0].astype(np.float64)
        assert abs(got[0].astype(np.float64).mean() - x.mean()) <= 1e-5 and abs(got[0].astype(np.float64).std() - x.std()) <= 1e-5


def _all_stages():
    return [dict(blur_sigma=0.5, lowres_zoom=0.9, noise_variance=0.02, noise_seed=3, brightness=0.8, contrast=1.25, gamma=0.7, gamma_invert=False, gamma_retain_stats=True),
            dict(blur_sigma=1.0, lowres_zoom=0.63, noise_variance=0.1, noise_seed=4, brightness=1.25, contrast=0.75, gamma=1.5, gamma_invert=True, gamma_retain_stats=True),
            dict(blur_sigma=2.0, lowres_zoom=0.5, noise_variance=0.05, noise_seed=5, brightness=1.1, contrast=1.1, gamma=1.2, gamma_invert=True, gamma_retain_stats=False),
            dict(blur_sigma=0.7, lowres_zoom=1.0, noise_variance=0.0, noise_seed=6, brightness=0.9, contrast=0.9, gamma=0.9, gamma_invert=False, gamma_retain_stats=False)]


@pytest.mark.parametrize("shape", SHAPES + ((64, 64, 64),))
def test_all_stages_on_all_channels(shape):
    """(64, 64, 64): 32 partials per channel and statistic, 16-byte accesses, two tiles per slice (along H only)"""
    _check(shape, _all_stages(), "all")                              # measured / bar: BARS["all"]


def test_mixed_channels():
    """blur only (written by the tile pass directly) next to a copy, a blurred channel with later stages and a pointwise-only channel"""
    _check((16, 40, 24), [dict(blur_sigma=1.0), {}, dict(blur_sigma=0.6, contrast=1.2), dict(lowres_zoom=0.7, gamma=0.8)], "all")
    _check((33, 20, 70), [dict(blur_sigma=1.0), {}, dict(blur_sigma=0.6, contrast=1.2), dict(lowres_zoom=0.7, gamma=0.8)], "all")


def test_refusals_come_before_any_launch():
    from brats2019_amd import dataloader as DL, _lib as L
    lib = L.load()
    shape = (16, 40, 24)
    x = T(_input(shape).copy()).cuda()
    out = torch.full_like(x, 7.0)
    ws_bytes = int(lib.ru_intensity_workspace_bytes(4, *shape))
    assert ws_bytes > 2 * x.numel() * 4
    ws = L.workspace(ws_bytes, x.device)

    def call(params, src=x, dst=out, c=4, nbytes=ws_bytes):
        blk = DL.intensity_param_block(params)
        rc = lib.ru_intensity_augment(L.f32(src), L.f32(dst), c, shape[0], shape[1], shape[2], C.byref(blk), L.ptr(ws), nbytes, L.stream())
        torch.cuda.synchronize()
        return rc

    bad = [dict(blur_sigma=0.0), dict(blur_sigma=float("nan")), dict(blur_sigma=2.5), dict(lowres_zoom=0.0), dict(lowres_zoom=1.5),
           dict(noise_variance=-0.01, noise_seed=1), dict(gamma=0.0), dict(gamma=float("nan"))]
    for q in bad:
        for channel in (0, 3):
            assert call(_only(channel, q)) != 0, q
            assert L.last_error()
            assert bool((out == 7.0).all()), q
        with pytest.raises(ValueError):
            DL.intensity_augment(x, _only(1, q))
    ok = _only(0, dict(blur_sigma=1.0))
    assert call(ok, dst=x) != 0 and "alias" in L.last_error()        # in == out
    assert call(ok, c=0) != 0 and call(ok, c=9) != 0
    assert call(ok, nbytes=ws_bytes - 1) != 0 and "workspace" in L.last_error()
    assert int(lib.ru_intensity_workspace_bytes(0, *shape)) == 0 and int(lib.ru_intensity_workspace_bytes(9, *shape)) == 0
    assert bool((out == 7.0).all()) and torch.equal(x.cpu(), T(_input(shape).copy()))
    for args in ((x, [{}] * 3), (x[0], [{}]), (x.cpu(), [{}] * 4), (x, _only(0, dict(noise_variance=0.1)))):
        with pytest.raises(ValueError):
            DL.intensity_augment(*args)
    assert call(ok) == 0 and not bool((out[0] == 7.0).any()) and torch.equal(out[1:], x[1:])     # and the same call with good arguments runs


def test_graph_capture():
    """the call only enqueues: captured once into a hipGraph and replayed once it gives the eager result bit for bit"""
    from brats2019_amd import dataloader as DL
    x = T(_input((16, 40, 24)).copy()).cuda()
    params = _all_stages()
    eager = DL.intensity_augment(x, params).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        DL.intensity_augment(x, params)                              # warm-up on the capture stream (allocator, workspace)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = DL.intensity_augment(x, params)
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def _items(image, label, patch, seeds, **kw):
    from brats2019_amd import dataloader as DL
    rd = DL.SimpleReader([(image, label)], patch, images_in_epoch=8, patches_from_single_image=100, **kw)
    out = []
    for seed in seeds:
        random.seed(seed)
        np.random.seed(seed)
        d, t = rd[0]
        out.append((d[0], t[0]))
    return out, (random.getstate(), np.random.get_state()[1].copy())


def test_reader_option():
    """`intensity=False` and no keyword: the plain reader's items.  With every probability 1: the same targets, data =
    intensity_augment(plain data, the private generator's draws), repeatable by `intensity_seed`; the same on top of `elastic=True`; the global
    random streams end where the plain reader leaves them."""
    from brats2019_amd import dataloader as DL
    image, label = O.make_dataloader_case(77)
    patch, seeds = (16, 20, 24), (21, 22)
    one = DL.IntensityConfig(p_blur=1, p_blur_channel=1, p_lowres=1, p_lowres_channel=1, p_noise=1, p_brightness=1, p_contrast=1, p_gamma_invert=1, p_gamma=1)
    for base in ({}, dict(elastic=True, elastic_seed=3)):
        plain, state = _items(image, label, patch, seeds, **base)
        off, state_off = _items(image, label, patch, seeds, intensity=False, **base)
        on, state_on = _items(image, label, patch, seeds, intensity=one, intensity_seed=3, **base)
        on2, _ = _items(image, label, patch, seeds, intensity=one, intensity_seed=3, **base)
        other, _ = _items(image, label, patch, seeds, intensity=one, intensity_seed=4, **base)
        defaults, state_def = _items(image, label, patch, seeds, intensity=True, intensity_seed=3, **base)
        rng = random.Random(3)
        for k in range(len(seeds)):
            assert torch.equal(off[k][0], plain[k][0]) and torch.equal(off[k][1], plain[k][1])
            assert torch.equal(on[k][1], plain[k][1]) and torch.equal(defaults[k][1], plain[k][1])           # targets untouched
            assert on[k][0].shape == plain[k][0].shape and not torch.equal(on[k][0], plain[k][0]) and bool(torch.isfinite(on[k][0]).all())
            assert torch.equal(on[k][0], on2[k][0]) and not torch.equal(on[k][0], other[k][0])
            assert torch.equal(on[k][0], DL.intensity_augment(plain[k][0], DL.draw_intensity_params(4, rng, one)))
        for st in (state_off, state_on, state_def):
            assert st[0] == state[0] and np.array_equal(st[1], state[1])
