"""Blended sliding window, host side: the tile geometry, the window profiles and `tiling.blend_host` -- the numpy float32 restatement of
csrc/blend.hip that the device tests compare against bit for bit -- against a float64 brute force written here; the declarations of the
two entries, their refusals, and the opt-in keywords and flags."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)

# the two geometries of the device tests: (volume, tile, starts at overlap 0.5)
GEOMETRIES = [((13, 19, 27), (8, 12, 16), ([0, 4, 5], [0, 6, 7], [0, 8, 11])),
              ((5, 12, 40), (8, 12, 16), ([0], [0], [0, 8, 16, 24]))]


def brute_profile(t, window, sigma_scale=0.125):
    if window == "constant":
        return [1.0] * t
    return [float(np.float32(math.exp(-0.5 * ((i - (t - 1) / 2.0) / (sigma_scale * t)) ** 2))) for i in range(t)]


def brute_blend(tiles, shape, tile, starts, window):
    """float64, tile by tile and voxel row by voxel row; shares nothing with brats2019_amd.tiling"""
    d, h, w = shape
    td, th, tw = tile
    gz, gy, gx = (brute_profile(t, window) for t in tile)
    ntiles = len(starts[0]) * len(starts[1]) * len(starts[2])
    n = tiles.shape[0] // ntiles
    s = np.zeros((n, tiles.shape[1], d, h, w), np.float64)
    wn = np.zeros((d, h, w), np.float64)
    t = 0
    for oz in starts[0]:
        for oy in starts[1]:
            for ox in starts[2]:
                for z in range(td):
                    for y in range(th):
                        if oz + z >= d or oy + y >= h:
                            continue
                        wzy = float(np.float32(gz[z] * gy[y]))
                        for x in range(tw):
                            if ox + x >= w:
                                continue
                            wt = float(np.float32(wzy * gx[x]))
                            s[:, :, oz + z, oy + y, ox + x] += wt * tiles[t * n:(t + 1) * n, :, z, y, x].astype(np.float64)
                            wn[oz + z, oy + y, ox + x] += wt
                t += 1
    return s / wn


def cut_tiles(vol, tile, starts):
    """zero-padded tiles of vol [N,C,D,H,W] in the layout of ru_tile_gather"""
    n, c, d, h, w = vol.shape
    out = []
    for oz in starts[0]:
        for oy in starts[1]:
            for ox in starts[2]:
                t = np.zeros((n, c) + tuple(tile), np.float32)
                ez, ey, ex = min(tile[0], d - oz), min(tile[1], h - oy), min(tile[2], w - ox)
                t[:, :, :ez, :ey, :ex] = vol[:, :, oz:oz + ez, oy:oy + ey, ox:ox + ex]
                out.append(t)
    return np.concatenate(out, axis=0)


def test_blend_starts_listed_values():
    from brats2019_amd import tiling
    for (n, t, ov), want in [((240, 128, 0.5), [0, 64, 112]), ((160, 128, 0.5), [0, 32]), ((155, 128, 0.5), [0, 27]), ((100, 128, 0.5), [0]),
                             ((128, 128, 0.5), [0])]:
        assert tiling.blend_starts(n, t, ov) == want, (n, t, ov)
    for shape, tile, starts in GEOMETRIES:
        assert tuple(tiling.blend_starts(n, t, 0.5) for n, t in zip(shape, tile)) == starts
    assert tiling.blend_origins(([0, 4], [0], [0, 8, 11]))[4] == (4, 0, 8)          # tile index = (iz*ny + iy)*nx + ix


def test_blend_starts_properties():
    from brats2019_amd import tiling
    for t in (8, 12, 16):
        for overlap in (0, 0.25, 0.5, 0.75):
            step = t - int(overlap * t)
            for n in range(1, 3 * t + 1):
                s = tiling.blend_starts(n, t, overlap)
                assert s[0] == 0 and all(b > a for a, b in zip(s, s[1:])), (n, t, overlap, s)
                assert all(b - a <= step for a, b in zip(s, s[1:])), (n, t, overlap, s)
                covered = np.zeros(n, bool)
                for a in s:
                    covered[a:a + t] = True
                assert covered.all(), (n, t, overlap, s)
                if n >= t:
                    assert s[-1] + t == n, (n, t, overlap, s)
                else:
                    assert s == [0]


@pytest.mark.parametrize("t", [7, 8, 12, 16, 128])
def test_blend_profile(t):
    from brats2019_amd import tiling
    g = tiling.blend_profile(t)
    assert g.dtype == np.float32 and g.shape == (t,)
    assert np.array_equal(g, g[::-1])
    assert g.max() == g[(t - 1) // 2] == g[t // 2]
    if t % 2:
        assert g[t // 2] == np.float32(1.0)
    assert np.all(np.diff(g[:(t + 1) // 2]) > 0)
    np.testing.assert_array_equal(g, np.array(brute_profile(t, "gaussian"), np.float32))
    half = tiling.blend_profile(t, sigma_scale=0.25)
    assert half[0] > g[0]
    c = tiling.blend_profile(t, "constant")
    assert c.dtype == np.float32 and np.array_equal(c, np.ones(t, np.float32))


@pytest.mark.parametrize("geometry", [0, 1])
@pytest.mark.parametrize("window", ["gaussian", "constant"])
def test_blend_host_equals_float64_brute_force(geometry, window):
    """the float32 chain has at most 27 terms here: relative error about (27 + 3) * 2^-24 = 1.8e-6 on each of S and Wn; p in [0, 1], so
    1e-5 absolute is about three times their sum"""
    from brats2019_amd import tiling
    shape, tile, starts = GEOMETRIES[geometry]
    rng = np.random.default_rng(100 + geometry)
    ntiles = len(starts[0]) * len(starts[1]) * len(starts[2])
    tiles = rng.random((ntiles * 2, 3) + tile).astype(np.float32)
    got = tiling.blend_host(tiles, shape, tile, starts, [tiling.blend_profile(t, window) for t in tile])
    assert got.dtype == np.float32 and got.shape == (2, 3) + shape
    want = brute_blend(tiles, shape, tile, starts, window)
    err = np.abs(got.astype(np.float64) - want).max()
    print("blend_host vs float64 brute force: max abs error %.3g" % err)
    assert err <= 1e-5
    assert np.array_equal(got, tiling.blend_host(tiles, (2, 3) + shape, tile, starts, [tiling.blend_profile(t, window) for t in tile]))


@pytest.mark.parametrize("window", ["gaussian", "constant"])
@pytest.mark.parametrize("overlap", [0.25, 0.5, 0.75])
def test_partition_of_unity(window, overlap):
    from brats2019_amd import tiling
    rng = np.random.default_rng(7)
    for shape, tile, _ in GEOMETRIES:
        vol = (rng.random((2, 3) + shape).astype(np.float32) + 0.5) * rng.choice([-1.0, 1.0], size=(2, 3) + shape).astype(np.float32)
        starts = [tiling.blend_starts(n, t, overlap) for n, t in zip(shape, tile)]
        got = tiling.blend_host(cut_tiles(vol, tile, starts), shape, tile, starts, [tiling.blend_profile(t, window) for t in tile])
        rel = np.abs(got.astype(np.float64) - vol) / np.abs(vol)
        assert rel.max() <= 1e-5, (shape, rel.max())


def test_header_ctypes_table_and_sources_declare_the_blend_entries():
    from brats2019_amd import _lib as L, build as B
    text = open(HEADER).read()
    for name in ("ru_blend_accumulate", "ru_blend_finalize"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
        assert hasattr(L.load(), name), name
    assert "blend.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "blend.hip"))


def test_entries_refuse_bad_arguments_before_any_launch():
    from brats2019_amd import _lib as L
    lib = L.load()
    ints = lambda *v: (C.c_int * len(v))(*v)
    one = C.c_void_p(64)                                  # any non-null pointer: never dereferenced by a failing check
    z, y, x = ints(0, 4, 5), ints(0, 6, 7), ints(0, 8, 11)

    def acc(tiles=one, acc_=one, prof=one, dims=(13, 19, 27), tile=(8, 12, 16), sz=z, nz=3, sy=y, ny=3, sx=x, nx=3, t0=0, t=27):
        return lib.ru_blend_accumulate(tiles, acc_, prof, 2, 3, *dims, *tile, sz, nz, sy, ny, sx, nx, t0, t, None)

    def fin(a=one, out=one, prof=one, dims=(13, 19, 27), tile=(8, 12, 16), sz=z, nz=3, sy=y, ny=3, sx=x, nx=3):
        return lib.ru_blend_finalize(a, out, prof, 2, 3, *dims, *tile, sz, nz, sy, ny, sx, nx, None)

    for call in (acc, fin):
        assert call(prof=None) < 0 and b"ru_blend_" in lib.ru_last_error()
        assert call(dims=(13, 0, 27)) < 0 and b"positive" in lib.ru_last_error()
        assert call(tile=(8, 12, 0)) < 0 and b"positive" in lib.ru_last_error()
        assert call(tile=(8, 12, 18)) < 0 and b"multiple of 4" in lib.ru_last_error()
        assert call(sz=ints(0, 5, 5)) < 0 and b"strictly increasing" in lib.ru_last_error()
        assert call(sz=ints(0, 5, 4)) < 0 and b"strictly increasing" in lib.ru_last_error()
        assert call(sz=ints(1, 4, 5)) < 0 and b"begin at 0" in lib.ru_last_error()
        assert call(sx=None) < 0
        assert call(ny=0) < 0
        assert call(sx=ints(0, 8, 10)) < 0 and b"volume's end" in lib.ru_last_error()
        assert call(dims=(30, 19, 27), sz=ints(0, 9, 22)) < 0 and b"gap" in lib.ru_last_error()
    assert acc(tiles=None) < 0 and acc(acc_=None) < 0 and fin(a=None) < 0 and fin(out=None) < 0
    assert acc(t0=20, t=8) < 0 and b"tile range" in lib.ru_last_error()
    assert acc(t=0) < 0 and acc(t0=-1) < 0


def test_keywords_and_flags_are_opt_in():
    from brats2019_amd import inference as I, test as entry, tiling, train as TR
    for fn in (I.predict_case, I.predict_case_device, I.predict_case_ensemble, I.predict_case_ensemble_device):
        p = inspect.signature(fn).parameters
        assert p["tile"].default is None and p["overlap"].default == 0.5 and p["window"].default == "gaussian", fn.__name__
    p = inspect.signature(TR.Trainer.predict_tiled).parameters
    assert p["blend"].default is None and p["overlap"].default == 0.5
    p = inspect.signature(tiling.predict_blended).parameters
    assert [p[k].default for k in ("overlap", "window", "sigma_scale", "batch_tiles")] == [0.5, "gaussian", 0.125, None]
    plain = entry.parser.parse_args([])
    assert not any(hasattr(plain, k) for k in ("tile", "overlap", "window"))
    got = entry.parser.parse_args(["--tile", "64", "96", "128", "--overlap", "0.25", "--window", "constant"])
    assert got.tile == [64, 96, 128] and got.overlap == 0.25 and got.window == "constant"
    with pytest.raises(SystemExit):
        entry.parser.parse_args(["--window", "hann"])
    with pytest.raises(SystemExit):
        entry.main(["--overlap", "0.25"])                 # needs --tile: refused before anything is loaded


def test_argument_checks_fire_before_the_library_is_loaded(monkeypatch, tmp_path):
    from brats2019_amd import _lib as L, inference as I, model as M, ops, tiling, train as TR

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(L, "load", no_load)
    monkeypatch.setattr(L, "require_gpu", no_load)
    net = M.UNet(**SMALL)
    x = torch.zeros((1, 4, 16, 16, 16))
    img = np.ones((4, 20, 20, 20), np.float32)
    stub = lambda xs: [xs[0]]
    for kw, what in [(dict(overlap=0.8), "overlap"), (dict(overlap=-0.1), "overlap"), (dict(window="hann"), "window"), (dict(sigma_scale=0.0), "sigma_scale")]:
        with pytest.raises(ValueError, match=what):
            tiling.predict_blended(stub, x, (8, 8, 8), **kw)
    with pytest.raises(ValueError, match="multiple of 4"):
        tiling.predict_blended(stub, x, (8, 8, 6))
    with pytest.raises(ValueError, match="divisible by 4"):
        tiling.predict_blended(net, x, (8, 10, 8))            # depth 3: two halvings
    with pytest.raises(ValueError, match="three positive"):
        tiling.predict_blended(stub, x, (8, 8))
    for fn, first in ((I.predict_case, net), (I.predict_case_device, net), (I.predict_case_ensemble, [net]), (I.predict_case_ensemble_device, [net])):
        arg = torch.from_numpy(img) if fn.__name__.endswith("_device") else img
        with pytest.raises(ValueError, match="overlap"):
            fn(first, arg, tile=(16, 16, 16), overlap=0.9)
        with pytest.raises(ValueError, match="window"):
            fn(first, arg, tile=(16, 16, 16), window="hann")
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(first, arg, tile=(16, 16, 18))
        with pytest.raises(ValueError, match="divisible by 4"):
            fn(first, arg, tile=(16, 18, 16))
    with pytest.raises(ValueError, match="window"):
        I.predict_case(net, img, uncertainty="std", tile=(16, 16, 16), window="hann")
    tr = TR.Trainer(name="t", models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    with pytest.raises(ValueError, match="window"):
        tr.predict_tiled([[x]], (1, 3, 16, 16, 16), (8, 8, 8), blend="hann")
    with pytest.raises(ValueError, match="overlap"):
        tr.predict_tiled([[x]], (1, 3, 16, 16, 16), (8, 8, 8), blend="gaussian", overlap=1.0)
    acc = torch.zeros((1, 3, 13, 19, 27))
    prof = torch.ones(8 + 12 + 16)
    starts = GEOMETRIES[0][2]
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.blend_accumulate(acc, torch.zeros((27, 3, 8, 12, 18)), starts, torch.ones(38))
    with pytest.raises(ValueError, match="do not cover"):
        ops.blend_accumulate(acc, torch.zeros((27, 3, 8, 12, 16)), ([0, 5, 4], starts[1], starts[2]), prof)
    with pytest.raises(ValueError, match="profiles"):
        ops.blend_accumulate(acc, torch.zeros((27, 3, 8, 12, 16)), starts, torch.ones(35))
    with pytest.raises(ValueError, match="tiles 20"):
        ops.blend_accumulate(acc, torch.zeros((8, 3, 8, 12, 16)), starts, prof, t0=20)
    with pytest.raises(ValueError, match="do not cover"):
        ops.blend_finalize(acc, (8, 12, 16), ([0, 4], starts[1], starts[2]), prof)
