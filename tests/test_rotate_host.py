"""Rotation augmentation on the host (no GPU): `affine_patch_host`, the float64 restatement of `ru_augment_patch_affine`, against
scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=0) per channel and per one-hot class; `rotation_matrix`; `draw_rotation_params`;
the argument errors.  The volume and the cases are shared with tests/test_rotate.py."""
import random

import numpy as np
import pytest
import scipy.ndimage as ndi

from brats2019_amd import dataloader as DL

DIMS = (20, 24, 28)


def make_volume():
    """(image [4,20,24,28] float32, label [20,24,28] uint8): an ellipsoid 'head' of positive intensities on a zero background and a small
    three-label blob (2 around 1 around 3) off its centre"""
    r = np.random.default_rng(2019)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in DIMS], indexing="ij")
    head = ((g[0] - 9.5) / 9.0) ** 2 + ((g[1] - 11.5) / 11.0) ** 2 + ((g[2] - 13.5) / 13.0) ** 2 <= 1.0
    image = np.where(head[None], 200.0 + 500.0 * r.random((4,) + DIMS), 0.0).astype(np.float32)
    d2 = (g[0] - 11.0) ** 2 + (g[1] - 10.0) ** 2 + ((g[2] - 15.0) / 1.5) ** 2
    label = np.zeros(DIMS, np.uint8)
    label[d2 <= 20.0] = 2
    label[d2 <= 9.0] = 1
    label[d2 <= 3.0] = 3
    return image, label


def make_soft(label):
    """[3,D,H,W] float32 teacher-like probabilities that follow the label's regions"""
    r = np.random.default_rng(7)
    lab = label.astype(np.int64)
    inside = np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3]).astype(np.float64)
    return (inside * (0.6 + 0.4 * r.random(inside.shape)) + (1.0 - inside) * 0.3 * r.random(inside.shape) ** 3).astype(np.float32)


# name -> (patch, crop_lo, angles in radians, scale).  `inside*` stay in the volume or graze it; `negative` starts at a negative index, `far` runs
# past the far faces, `larger` is longer than the volume along W.
CASES = {
    "inside_small": ((12, 10, 16), (4, 7, 6), (0.12, -0.2, 0.07), (1.0, 0.9, 1.1)),
    "inside_mid": ((12, 10, 16), (4, 7, 6), (-0.3, 0.25, 0.4), (0.8, 1.2, 0.9)),
    "inside_30deg": ((12, 10, 16), (4, 7, 6), (np.pi / 6, -np.pi / 6, np.pi / 6), (0.7, 1.3, 1.05)),
    "ragged_30deg": ((5, 7, 9), (8, 8, 9), (-np.pi / 6, np.pi / 6, -np.pi / 6), (1.3, 0.7, 1.2)),
    "ragged_mid": ((5, 7, 9), (7, 9, 10), (0.5, -0.5, 0.35), (1.1, 1.0, 0.75)),
    "negative": ((12, 10, 16), (-4, -3, -5), (0.3, -0.2, 0.5), (1.0, 1.1, 0.9)),
    "far": ((12, 10, 16), (12, 17, 16), (-0.5, 0.4, 0.25), (0.9, 1.0, 1.2)),
    "far_ragged": ((5, 7, 9), (16, 19, 21), (0.2, 0.5, -0.4), (1.2, 0.8, 1.0)),
    "larger": ((6, 8, 40), (7, 8, -6), (0.15, -0.1, 0.2), (1.0, 1.0, 1.0)),
}
LEAVING = ("negative", "far", "far_ragged", "larger")


def case_transform(name):
    """(patch, matrix, offset) of a case, by the rule of `augment_patch` for an `angles` entry"""
    patch, lo, angles, scale = CASES[name]
    matrix = DL.rotation_matrix(angles) * np.asarray(scale, np.float64)[None, :]
    half = (np.array(patch, np.float64) - 1.0) / 2.0
    return patch, matrix, (np.asarray(lo, np.float64) + half) - matrix @ half


def scipy_channel(vol, patch, matrix, offset):
    return ndi.affine_transform(np.asarray(vol, np.float64), matrix, offset, output_shape=patch, order=1, mode="grid-constant", cval=0.0)


def fill_share(patch, matrix, offset):
    """share of the patch's voxels with a corner of positive weight outside the volume"""
    return float((scipy_channel(np.ones(DIMS), patch, matrix, offset) < 1.0 - 1e-9).mean())


def finish(t, flips, transpose):
    for ax, f in enumerate(flips):
        if f:
            t = np.flip(t, axis=ax + 1)
    return np.ascontiguousarray(t.transpose((0, 2, 1, 3)) if transpose else t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_matches_scipy(name):
    """every image channel and every one-hot class within 1e-12 of scipy (float64 on both sides; raw intensities up to 700 divided by a std near 300)"""
    image, label = make_volume()
    patch, matrix, offset = case_transform(name)
    r = np.random.default_rng(len(name))
    mean, std = image.reshape(4, -1).mean(1).astype(np.float64), image.reshape(4, -1).std(1).astype(np.float64)
    gain, bias = r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)
    flips, transpose = [bool(v) for v in r.integers(0, 2, 3)], bool(r.integers(0, 2))
    data, target = DL.affine_patch_host(image, label, mean, std, patch, matrix, offset, flips, transpose, gain, bias)
    sh = (-1, 1, 1, 1)
    raw = np.stack([scipy_channel(image[c], patch, matrix, offset) for c in range(4)])
    want_d = finish(((raw - mean.reshape(sh)) / std.reshape(sh)) * gain.reshape(sh) + bias.reshape(sh), flips, transpose)
    cls = [scipy_channel(label == k, patch, matrix, offset) for k in (1, 2, 3)]
    want_t = finish(np.stack([cls[0] + cls[1] + cls[2], cls[0] + cls[2], cls[2]]), flips, transpose)
    assert data.dtype == target.dtype == np.float64 and data.shape == want_d.shape and target.shape == want_t.shape
    share = fill_share(patch, matrix, offset)
    err_d, err_t = float(np.abs(data - want_d).max()), float(np.abs(target - want_t).max())
    print("%s: fill share %.3f, max |host - scipy| image %.3e, targets %.3e" % (name, share, err_d, err_t))
    assert err_d <= 1e-12 and err_t <= 1e-12
    if name not in LEAVING:
        assert float(want_t[2].max()) > 0.5 and float(want_t[0].min()) == 0.0      # the blob is in view: every class is exercised
    else:
        assert 0.2 < share < 0.8                                     # the fill rule is exercised and the result is not all fill
    soft = make_soft(label)
    _d, tsoft = DL.affine_patch_host(image, soft, mean, std, patch, matrix, offset, flips, transpose, gain, bias)
    want_s = finish(np.stack([scipy_channel(soft[k], patch, matrix, offset) for k in range(3)]), flips, transpose)
    assert float(np.abs(tsoft - want_s).max()) <= 1e-12 and np.array_equal(_d, data)


def test_host_identity_is_the_crop_and_far_away_is_all_fill():
    image, label = make_volume()
    mean, std = np.full(4, 300.0), np.full(4, 250.0)
    data, target = DL.affine_patch_host(image, label, mean, std, (5, 7, 9), np.eye(3), (3, 4, 5))
    crop = (slice(3, 8), slice(4, 11), slice(5, 14))
    assert np.array_equal(data, (image[(slice(None),) + crop].astype(np.float64) - 300.0) * (1.0 / 250.0))
    lab = label[crop]
    assert np.array_equal(target, np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3]).astype(np.float64))
    big = np.array([[1e308, -1e308, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])         # inf - inf: a coordinate that is not a number
    for matrix, off in ((np.eye(3), (1e300, 0, 0)), (np.eye(3), (0, -1e300, 0)), (np.eye(3), (0, 0, 1e12)), (np.eye(3), (-40, 2, 2)), (big, (0, 0, 0)),
                        (np.eye(3), (3, 4, 28)), (np.eye(3), (3, 4, -10))):          # huge coordinates stay defined: all fill
        data, target = DL.affine_patch_host(image, label, mean, std, (5, 7, 9), matrix, off)
        assert np.array_equal(data, np.broadcast_to(np.float64(-300.0) * (1.0 / 250.0), data.shape)) and not target.any()


def test_rotation_matrix():
    r = np.random.default_rng(1)
    for angles in list(r.uniform(-np.pi, np.pi, (8, 3))) + [(0.5, 0.0, 0.0), (np.pi / 6,) * 3]:
        m = DL.rotation_matrix(angles)
        assert m.dtype == np.float64 and m.shape == (3, 3)
        assert float(np.abs(m @ m.T - np.eye(3)).max()) <= 1e-15 * 8 and abs(np.linalg.det(m) - 1.0) <= 1e-15 * 8
    a = 0.37
    c, s = np.cos(a), np.sin(a)
    assert np.array_equal(DL.rotation_matrix((a, 0, 0)), np.array([[1, 0, 0], [0, c, -s], [0, s, c]]))
    assert np.array_equal(DL.rotation_matrix((0, a, 0)), np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]))
    assert np.array_equal(DL.rotation_matrix((0, 0, a)), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
    eye = DL.rotation_matrix((0.0, 0.0, 0.0))
    assert np.array_equal(eye, np.eye(3)) and not np.signbit(eye).any()
    a0, a1, a2 = 0.2, -0.4, 0.9                                       # the order of the product: R0 @ R1 @ R2
    want = DL.rotation_matrix((a0, 0, 0)) @ DL.rotation_matrix((0, a1, 0)) @ DL.rotation_matrix((0, 0, a2))
    assert float(np.abs(DL.rotation_matrix((a0, a1, a2)) - want).max()) <= 1e-15


def test_draw_rotation_params():
    gs, ns = random.getstate(), np.random.get_state()[1].copy()
    cfg = DL.RotationConfig(p_rotation=0.5, max_angle=(0.1, 0.2, 0.3))
    a = [DL.draw_rotation_params(random.Random(11), cfg) for _ in range(2)]
    assert a[0] == a[1]                                              # reproducible by seed
    rng, rng2 = random.Random(5), random.Random(6)
    draws = [DL.draw_rotation_params(rng, cfg) for _ in range(400)]
    assert draws != [DL.draw_rotation_params(rng2, cfg) for _ in range(400)]
    fired = [d for d in draws if d is not None]
    assert 140 <= len(fired) <= 260                                  # p = 0.5 over 400 draws: +-6 sigma
    for d in fired:
        assert set(d) == {"angles"} and len(d["angles"]) == 3
        assert all(abs(v) <= m for v, m in zip(d["angles"], cfg.max_angle))
    assert max(abs(d["angles"][2]) for d in fired) > 0.2             # the third axis really uses its own range
    never, always = DL.RotationConfig(p_rotation=0.0), DL.RotationConfig(p_rotation=1.0)
    rng = random.Random(3)
    assert all(DL.draw_rotation_params(rng, never) is None for _ in range(200))
    assert all(DL.draw_rotation_params(rng, always) is not None for _ in range(200))
    default = DL.RotationConfig()
    assert default.p_rotation == 0.2 and np.allclose(default.max_angle, np.deg2rad(30.0))
    assert all(abs(v) <= np.deg2rad(30.0) for _ in range(50) for v in DL.draw_rotation_params(rng, always)["angles"])
    assert random.getstate() == gs and np.array_equal(np.random.get_state()[1], ns)      # the global streams are untouched


def test_argument_errors():
    image, label = make_volume()
    mean, std = np.full(4, 300.0), np.full(4, 250.0)
    ok = dict(image=image, label_or_soft=label, mean=mean, std=std, patch=(5, 7, 9), matrix=np.eye(3), offset=np.zeros(3))
    DL.affine_patch_host(**ok)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 0.0]])
    for change, what in ((dict(matrix=np.eye(4)), "3 x 3"), (dict(matrix=np.ones(9)), "3 x 3"), (dict(offset=np.zeros(2)), "three"),
                         (dict(matrix=np.diag([1.0, np.nan, 1.0])), "finite"), (dict(offset=(0.0, np.inf, 0.0)), "finite"),
                         (dict(matrix=singular), "singular"), (dict(matrix=np.eye(3) * 1e-3), "singular"), (dict(matrix=np.zeros((3, 3))), "singular"),
                         (dict(image=image[0]), "image"), (dict(label_or_soft=label[1:]), "label"), (dict(patch=(5, 0, 9)), "patch"),
                         (dict(patch=(5, 7)), "patch"), (dict(mean=np.zeros(3)), "per image channel"), (dict(gain=np.ones(5)), "per image channel")):
        with pytest.raises(ValueError, match=what):
            DL.affine_patch_host(**dict(ok, **change))
    for angles in ((0.1, 0.2), 0.3, (0.1, np.nan, 0.0), np.zeros((3, 3))):
        with pytest.raises(ValueError, match="angles"):
            DL.rotation_matrix(angles)
    # the `rotation` entry of augment_patch is checked by _rotation_transform, before any device is touched
    lo, scale, patch = (3, 4, 5), (1.0, 1.0, 1.0), (5, 7, 9)
    m, o, code = DL._rotation_transform(dict(angles=(0.0, 0.0, 0.0)), lo, scale, patch)
    assert np.array_equal(m, np.eye(3)) and np.array_equal(o, np.array(lo, np.float64)) and code == 0
    m, o, code = DL._rotation_transform(dict(matrix=np.eye(3) * 2.0, mapping="row"), lo, scale, patch)
    assert np.array_equal(o, np.array(lo) + np.array([2.0, 3.0, 4.0]) - 2.0 * np.array([2.0, 3.0, 4.0])) and code == 1
    for rot, what in ((dict(angles=(0, 0, 0), matrix=np.eye(3)), "not both"), (dict(angles=(0, 0, 0), offset=np.zeros(3)), "not both"),
                      (dict(), "needs angles or a matrix"), (dict(offset=np.zeros(3)), "needs angles or a matrix"), (dict(angle=(0, 0, 0)), "unknown keys"),
                      (dict(angles=(0, 0)), "angles"), (dict(angles=(0, np.inf, 0)), "finite"), (dict(matrix=singular), "singular"),
                      (dict(matrix=np.eye(2)), "3 x 3"), (dict(matrix=np.eye(3), offset=(1, 2)), "three"), (dict(matrix=np.eye(3), offset=(1, np.nan, 2)), "finite"),
                      (dict(matrix=np.eye(3), mapping="cube"), "mapping"), ((0.1, 0.2, 0.3), "entry must be")):
        with pytest.raises(ValueError, match=what):
            DL._rotation_transform(rot, lo, scale, patch)
    with pytest.raises(ValueError, match="singular"):                # a zero scale collapses the patch
        DL._rotation_transform(dict(angles=(0.1, 0.2, 0.3)), lo, (1.0, 0.0, 1.0), patch)
    with pytest.raises(ValueError, match="scale"):
        DL._rotation_transform(dict(angles=(0.1, 0.2, 0.3)), lo, (1.0, np.nan, 1.0), patch)
    with pytest.raises(ValueError, match="patch extents"):
        DL._rotation_transform(dict(angles=(0.1, 0.2, 0.3)), lo, scale, (2048, 2048, 512))
    for bad in (dict(p_rotation=1.5), dict(p_rotation=-0.1), dict(max_angle=(0.1, 0.2)), dict(max_angle=(0.1, -0.2, 0.3)), dict(max_angle=(0.1, np.nan, 0.3))):
        with pytest.raises(ValueError, match="rotation"):
            DL.RotationConfig(**bad)
