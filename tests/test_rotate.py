"""Rotation augmentation on the device (csrc/rotate.hip: `ru_augment_patch_affine`, `augment_patch` with a `rotation` entry, `SimpleReader(rotation=...)`)
against the float64 host restatement `affine_patch_host` (held to scipy by tests/test_rotate_host.py), against the unchanged zoom pass where the two
must agree bit for bit, and with both thread mappings on every case.  Bars: image 2e-5 absolute on the z-scored data, targets 2e-6 -- the bars
tests/test_elastic.py holds the same 8-corner float32 arithmetic to."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_rotate_host import CASES, DIMS, LEAVING, case_transform, make_soft, make_volume

pytestmark = pytest.mark.gpu
T = torch.from_numpy
IMAGE_BAR, TARGET_BAR = 2e-5, 2e-6
MAPPINGS = ("row", "brick")
NOFLIP = (False, False, False)


@pytest.fixture(scope="module")
def volume():
    image, label = make_volume()
    return image, label, make_soft(label)


@pytest.fixture(scope="module")
def cases(volume):
    """the resident cases, hard and soft, built once; `patch_size` is given per call"""
    from brats2019_amd import dataloader as DL
    image, label, soft = volume
    return {False: DL.DeviceCase(image, label, (12, 10, 16)), True: DL.DeviceCase(image, label, (12, 10, 16), soft=soft)}


def params(lo, scale, flips=NOFLIP, transpose=False, gain=None, bias=None, **rotation):
    p = dict(crop_lo=np.asarray(lo), scale=np.asarray(scale, np.float64), flips=list(flips), transpose=transpose,
             gain=np.ones(4) if gain is None else gain, bias=np.zeros(4) if bias is None else bias)
    if rotation:
        p["rotation"] = rotation
    return p


def both_mappings(case, p, patch):
    """the affine pass with both thread mappings and once more: identical bytes; returns the default mapping's result"""
    from brats2019_amd import dataloader as DL
    d, t = DL.augment_patch(case, p, patch)
    for mapping in MAPPINGS:
        dm, tm = DL.augment_patch(case, dict(p, rotation=dict(p["rotation"], mapping=mapping)), patch)
        assert torch.equal(dm, d) and torch.equal(tm, t), mapping
    d2, t2 = DL.augment_patch(case, p, patch)
    assert torch.equal(d2, d) and torch.equal(t2, t)
    return d, t


def host(volume, case, soft, patch, matrix, offset, flips=NOFLIP, transpose=False, gain=None, bias=None):
    from brats2019_amd import dataloader as DL
    image, label, soft_map = volume
    return DL.affine_patch_host(image, soft_map if soft else label, case.mean, case.std, patch, matrix, offset, flips, transpose, gain, bias)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("patch,lo", [((12, 10, 16), (4, 7, 6)), ((5, 7, 9), (8, 8, 9)), ((20, 24, 28), (0, 0, 0))])
def test_identity_is_the_zoom_pass_at_scale_one(cases, patch, lo, soft):
    """angles 0, scale 1, a crop inside the volume: bit-identical to `augment_patch` without the entry, plain and with flips, transpose, gain and bias"""
    from brats2019_amd import dataloader as DL
    case = cases[soft]
    r = np.random.default_rng(3)
    for flips, transpose, gain, bias in ((NOFLIP, False, None, None), ((True, False, True), True, r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)),
                                         ((False, True, False), False, r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4))):
        plain = params(lo, (1.0, 1.0, 1.0), flips, transpose, gain, bias)
        d0, t0 = DL.augment_patch(case, plain, patch)
        d, t = both_mappings(case, dict(plain, rotation=dict(angles=(0.0, 0.0, 0.0))), patch)
        assert d.shape == d0.shape and torch.equal(d, d0) and torch.equal(t, t0)
        d, t = both_mappings(case, dict(plain, rotation=dict(matrix=np.eye(3), offset=np.asarray(lo, np.float64))), patch)
        assert torch.equal(d, d0) and torch.equal(t, t0)
    assert float(t0[2].sum()) > 0 or patch == (5, 7, 9)


@pytest.mark.parametrize("soft", [False, True])
def test_signed_permutations_are_exact(cases, soft):
    """a 90 degree turn about each axis as an explicit integer matrix and offset, on a cubic patch: weights are exactly 0 and 1, so the result is
    the identity result with its voxels rearranged"""
    case, n, lo = cases[soft], 8, np.array([5, 6, 7])
    patch = (n, n, n)
    d0, t0 = both_mappings(case, params(lo, (1, 1, 1), angles=(0.0, 0.0, 0.0)), patch)
    d0, t0 = d0.cpu().numpy(), t0.cpu().numpy()
    q = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"))
    turns = (np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]))
    for m in turns:
        inside = np.where(m.sum(1) < 0, n - 1, 0)                    # a row with a -1 counts down from the crop's far face
        d, t = both_mappings(case, params(lo, (1, 1, 1), matrix=m.astype(np.float64), offset=(lo + inside).astype(np.float64)), patch)
        s = np.tensordot(m, q, axes=(1, 0)) + inside.reshape(3, 1, 1, 1)
        assert s.min() == 0 and s.max() == n - 1
        assert np.array_equal(d.cpu().numpy(), d0[:, s[0], s[1], s[2]]) and np.array_equal(t.cpu().numpy(), t0[:, s[0], s[1], s[2]])
        assert not np.array_equal(d.cpu().numpy(), d0)


SETS = ("inside_small", "inside_mid", "inside_30deg")               # three angle / scale sets; the last is +-30 degrees on every axis, scales 0.7 .. 1.3
PATCHES = {(12, 10, 16): (4, 7, 6), (5, 7, 9): (8, 8, 9)}           # patch -> crop_lo; (5, 7, 9) is ragged against any brick shape
ALL_FLIPS = [tuple(bool(b >> ax & 1) for ax in range(3)) for b in range(8)]


@pytest.mark.parametrize("patch", sorted(PATCHES))
@pytest.mark.parametrize("name", SETS)
def test_oblique_matches_the_host(volume, cases, name, patch):
    """device against `affine_patch_host`: flips, transpose on and off, label and soft targets, gain and bias not 1 and 0"""
    _patch, _lo, angles, scale = CASES[name]
    lo = PATCHES[patch]
    half = (np.array(patch, np.float64) - 1.0) / 2.0
    from brats2019_amd import dataloader as DL
    matrix = DL.rotation_matrix(angles) * np.asarray(scale)[None, :]
    offset = (np.asarray(lo) + half) - matrix @ half
    r = np.random.default_rng(17)
    combos = [(f, bool(b & 1), bool(b & 2)) for b, f in enumerate(ALL_FLIPS)] if name == "inside_30deg" else \
        [(NOFLIP, False, False), ((True, False, True), True, True), ((False, True, False), True, False), ((True, True, True), False, True)]
    worst_d = worst_t = 0.0
    for flips, transpose, soft in combos:
        gain, bias = r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)
        d, t = both_mappings(cases[soft], params(lo, scale, flips, transpose, gain, bias, angles=angles), patch)
        want_d, want_t = host(volume, cases[soft], soft, patch, matrix, offset, flips, transpose, gain, bias)
        assert tuple(d.shape) == want_d.shape and tuple(t.shape) == want_t.shape and d.dtype == t.dtype == torch.float32
        err_d, err_t = float(np.abs(d.cpu().numpy() - want_d).max()), float(np.abs(t.cpu().numpy() - want_t).max())
        worst_d, worst_t = max(worst_d, err_d), max(worst_t, err_t)
        assert float(want_t.max()) > 0.5                             # the blob is in view
    print("%s patch %s: max |device - host| image %.3e (bar %.0e), targets %.3e (bar %.0e) over %d combinations"
          % (name, patch, worst_d, IMAGE_BAR, worst_t, TARGET_BAR, len(combos)))
    assert worst_d <= IMAGE_BAR and worst_t <= TARGET_BAR


@pytest.mark.parametrize("name", LEAVING)
def test_leaving_the_volume(volume, cases, name):
    """a crop that starts at a negative index, ones that run past the far faces, a patch longer than the volume: same bars, and where all eight
    corners are outside the data is the z-scored raw 0 -- ((0 - mean) istd) gain + bias, the last two as the one fused multiply-add the zoom
    pass's tail compiles to -- and the targets are 0, exactly"""
    patch, matrix, offset = case_transform(name)
    _patch, lo, angles, scale = CASES[name]
    r = np.random.default_rng(23)
    ones = np.ones((1,) + DIMS)
    for k, (flips, transpose, soft) in enumerate(((NOFLIP, False, False), ((True, False, True), True, True))):
        case = cases[soft]
        gain, bias = r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)
        d, t = both_mappings(case, params(lo, scale, flips, transpose, gain, bias, angles=angles), patch)
        want_d, want_t = host(volume, case, soft, patch, matrix, offset, flips, transpose, gain, bias)
        d, t = d.cpu().numpy(), t.cpu().numpy()
        err_d, err_t = float(np.abs(d - want_d).max()), float(np.abs(t - want_t).max())
        from brats2019_amd import dataloader as DL
        weight, _ = DL.affine_patch_host(ones, np.zeros(DIMS, np.uint8), [0.0], [1.0], patch, matrix, offset, flips, transpose)
        outside = weight[0] == 0.0                                   # no weight on any voxel of the volume
        print("%s (%d): max |device - host| image %.3e, targets %.3e; %d of %d voxels fully outside" % (name, k, err_d, err_t, outside.sum(), outside.size))
        assert err_d <= IMAGE_BAR and err_t <= TARGET_BAR
        assert 0 < outside.sum() < outside.size
        f32 = np.float32
        for c in range(4):
            z = (f32(0.0) - f32(case.mean[c])) * f32(1.0 / case.std[c])
            fill = f32(np.float64(z) * np.float64(f32(gain[c])) + np.float64(f32(bias[c])))
            assert np.array_equal(d[c][outside], np.full(int(outside.sum()), fill, f32)), c
        assert not t[:, outside].any()


@pytest.mark.parametrize("soft", [False, True])
def test_with_elastic(volume, cases, soft):
    """`rotation` and `elastic` (explicit noise) together == the device affine result without flips, gain or bias, pushed through the host field
    and warp.  Image 2e-5, targets exact (order 0 picks)."""
    from brats2019_amd import dataloader as DL
    case, patch, lo = cases[soft], (12, 10, 16), (4, 7, 6)
    _p, _lo, angles, scale = CASES["inside_mid"]
    r = np.random.default_rng(31 + int(soft))
    noise = r.uniform(-1, 1, (3,) + patch)
    flips, transpose, gain, bias = (True, False, True), True, r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)
    p = params(lo, scale, flips, transpose, gain, bias, angles=angles)
    p["elastic"] = dict(sigma=3.0, alpha=300.0, noise=noise)
    data, target = DL.augment_patch(case, p, patch)
    assert tuple(data.shape) == (4, 10, 12, 16) and tuple(target.shape) == (3, 10, 12, 16)
    d0, t0 = DL.augment_patch(case, params(lo, scale, angles=angles), patch)
    disp = DL.elastic_field_host(noise, 3.0, 300.0)
    assert np.abs(disp).max() > 1.0                                  # a real deformation
    want_d, want_t = DL.elastic_warp_host(d0.cpu().numpy(), t0.cpu().numpy(), disp, flips, transpose, gain, bias)
    err = float(np.abs(data.cpu().numpy() - want_d).max())
    wrong = int((target.cpu().numpy() != want_t).sum())
    print("soft %s: image max |device - host| = %.3e, target voxels that differ: %d" % (soft, err, wrong))
    assert err <= IMAGE_BAR and wrong == 0
    for mapping in MAPPINGS:
        dm, tm = DL.augment_patch(case, dict(p, rotation=dict(angles=angles, mapping=mapping)), patch)
        assert torch.equal(dm, data) and torch.equal(tm, target)


def test_reader(golden):
    """`p_rotation=0`: the plain reader's patches, bit for bit.  `p_rotation=1`: same crop, scale, flip, transpose, gain and bias draws (same global
    streams), a rotated patch, repeatable by `rotation_seed`; it composes with `elastic=`, `intensity=` and a soft case."""
    from brats2019_amd import dataloader as DL
    g = golden("dataloader")
    image, label = O.make_dataloader_case(77)
    patch = tuple(int(v) for v in g["patch"])
    always = DL.RotationConfig(p_rotation=1.0)
    soft = make_soft(np.where(label == 4, 3, label))
    kinds = (("plain", {}, False), ("never", dict(rotation=DL.RotationConfig(p_rotation=0.0), rotation_seed=1), False),
             ("on", dict(rotation=always, rotation_seed=3), False), ("on2", dict(rotation=always, rotation_seed=3), False),
             ("other", dict(rotation=always, rotation_seed=4), False), ("default", dict(rotation=True, rotation_seed=3), False),
             ("all", dict(rotation=always, rotation_seed=3, elastic=True, elastic_seed=5, intensity=True, intensity_seed=6), True))
    items, states = {}, {}
    for name, kw, with_soft in kinds:
        rd = DL.SimpleReader([(image, label, soft) if with_soft else (image, label)], patch, images_in_epoch=8, patches_from_single_image=100, **kw)
        out = []
        for k in range(2):
            random.seed(int(g["seed%d" % k]))
            np.random.seed(int(g["seed%d" % k]))
            d, t = rd[0]
            out.append((d[0], t[0]))
        items[name], states[name] = out, (random.getstate(), np.random.get_state()[1].copy())
    assert isinstance(DL.SimpleReader([(image, label)], patch, rotation=True).rotation, DL.RotationConfig)
    for k in range(2):
        np.testing.assert_allclose(items["plain"][k][0].cpu().numpy(), g["data%d" % k], rtol=0, atol=2e-5)
        assert torch.equal(items["never"][k][0], items["plain"][k][0]) and torch.equal(items["never"][k][1], items["plain"][k][1])
        assert items["on"][k][0].shape == items["plain"][k][0].shape and not torch.equal(items["on"][k][0], items["plain"][k][0])
        assert torch.equal(items["on"][k][0], items["on2"][k][0]) and torch.equal(items["on"][k][1], items["on2"][k][1])
        assert not torch.equal(items["on"][k][0], items["other"][k][0])
        for name in ("on", "other", "default", "all"):
            d, t = items[name][k]
            assert d.shape == items["plain"][k][0].shape and t.shape == items["plain"][k][1].shape
            assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0 + 1e-6 and bool(torch.isfinite(d).all()), name
    for name in states:
        assert states[name][0] == states["plain"][0] and np.array_equal(states[name][1], states["plain"][1]), name


def test_argument_errors_launch_nothing(cases):
    """the checks of the C ABI: an error code, `ru_last_error` set, the outputs untouched; the Python surface raises ValueError before any launch"""
    from brats2019_amd import _lib as L
    from brats2019_amd import dataloader as DL
    case, lib, patch = cases[False], L.load(), (5, 7, 9)
    data = torch.full((4,) + patch, 7.0, device="cuda")
    target = torch.full((3,) + patch, 7.0, device="cuda")
    arr = lambda ctype, values: (ctype * len(values))(*values)
    good = dict(image=L.f32(case.image), label=L.ptr(case.label), soft=None, mean=arr(C.c_float, [0.0] * 4), inv_std=arr(C.c_float, [1.0] * 4), C=4, D=DIMS[0],
                H=DIMS[1], W=DIMS[2], patch=arr(C.c_int, list(patch)), matrix=arr(C.c_double, list(np.eye(3).reshape(-1))), offset=arr(C.c_double, [3.0, 4.0, 5.0]),
                flags=0, gain=arr(C.c_float, [1.0] * 4), bias=arr(C.c_float, [0.0] * 4), mapping=0, data=L.f32(data), target=L.f32(target), stream=L.stream())
    singular = [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 1.0, 0.0]
    nan_m, inf_o = list(np.eye(3).reshape(-1)), [3.0, float("inf"), 5.0]
    nan_m[4] = float("nan")
    bad = [(dict(image=None), "null"), (dict(label=None), "null"), (dict(mean=None), "null"), (dict(inv_std=None), "null"), (dict(patch=None), "null"),
           (dict(matrix=None), "null"), (dict(offset=None), "null"), (dict(gain=None), "null"), (dict(bias=None), "null"), (dict(data=None), "null"),
           (dict(target=None), "null"), (dict(C=0), "channels"), (dict(C=9), "channels"), (dict(patch=arr(C.c_int, [5, 0, 9])), "positive"),
           (dict(patch=arr(C.c_int, [5, -7, 9])), "positive"), (dict(patch=arr(C.c_int, [2048, 2048, 512])), "32-bit"), (dict(D=0), "volume"),
           (dict(matrix=arr(C.c_double, nan_m)), "finite"), (dict(offset=arr(C.c_double, inf_o)), "finite"), (dict(matrix=arr(C.c_double, singular)), "det"),
           (dict(matrix=arr(C.c_double, [1e-3, 0, 0, 0, 1e-2, 0, 0, 0, 1e-2])), "det"), (dict(flags=16), "flags"), (dict(mapping=3), "mapping")]
    for change, what in bad:
        rc = lib.ru_augment_patch_affine(*dict(good, **change).values())
        assert rc != 0 and what in L.last_error(), (change, L.last_error())
    torch.cuda.synchronize()
    assert bool((data == 7.0).all()) and bool((target == 7.0).all())
    assert lib.ru_augment_patch_affine(*good.values()) == 0          # the unchanged arguments do run
    torch.cuda.synchronize()
    assert not bool((data == 7.0).any()) and not bool((target == 7.0).any())
    base = params((3, 4, 5), (1, 1, 1))
    for rot, what in ((dict(angles=(0, 0, 0), matrix=np.eye(3)), "not both"), (dict(matrix=np.reshape(singular, (3, 3))), "singular"), (dict(matrix=np.eye(2)), "3 x 3"),
                      (dict(angles=(0.0, float("nan"), 0.0)), "finite"), (dict(matrix=np.eye(3), offset=(1.0, 2.0)), "three"), (dict(), "needs")):
        with pytest.raises(ValueError, match=what):
            DL.augment_patch(case, dict(base, rotation=rot), patch)
    with pytest.raises(ValueError, match="singular"):
        DL.augment_patch(case, dict(base, scale=np.array([1.0, 0.0, 1.0]), rotation=dict(angles=(0.1, 0.2, 0.3))), patch)


def test_graph_capture(cases):
    """the affine pass only enqueues: captured once into a hipGraph and replayed once, it gives the eager result bit for bit (both mappings)"""
    from brats2019_amd import dataloader as DL
    _p, lo, angles, scale = CASES["negative"]
    patch = (12, 10, 16)
    r = np.random.default_rng(8)
    gain, bias = r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)

    def run():
        out = ()
        for mapping, soft in (("brick", False), ("row", True)):
            out += DL.augment_patch(cases[soft], params(lo, scale, (True, False, True), True, gain, bias, angles=angles, mapping=mapping), patch)
        return out

    eager = [t.clone() for t in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                        # warm-up on the capture stream (allocator)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, eager):
        assert torch.equal(got, want)
    assert float(outs[0].abs().max()) > 0.0
