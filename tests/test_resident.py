"""The resident training set on the device (csrc/resident.hip, `ResidentCases`, `augment_batch`, `ResidentLoader`).  Every check is an equality of
bytes (`torch.equal`): a packed case unpacks to its input, and a patch cut from a packed case is the patch the unchanged entry points cut from the
same case held whole (`DeviceCase`) -- the kernels instantiate one per-voxel function (csrc/augment_voxel.hpp) on different sources."""
import random

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DIMS = (19, 23, 37)
BOX = ((9, 6, 11), (9, 11, 15))              # the tissue of the gather cases: D 9..17, H 6..16, W 11..25
PATCHES = ((8, 8, 10), (9, 9, 7))
SCALES = ((0.7, 0.7, 0.7), (1.0, 1.0, 1.0), (1.3, 1.3, 1.3), (0.7, 1.0, 1.3))


def make_case(dims, lo, size, seed, fractional=False, soft=False):
    """(image [4,D,H,W] float32, label [D,H,W] in {0,1,2,4}[, soft [3,D,H,W]]): integer intensities (or fractional ones) and nested labels inside the
    box [lo, lo + size), exact zeros around it"""
    r = np.random.default_rng(seed)
    image = np.zeros((4,) + tuple(dims), np.float32)
    label = np.zeros(dims, np.uint8)
    sl = tuple(slice(a, a + n) for a, n in zip(lo, size))
    vals = r.integers(0, 3000, size=(4,) + tuple(size)).astype(np.float32)
    vals[:, 0, 0, 0] = 1.0                                    # the box's two extreme corners are occupied: the box is [lo, lo + size) exactly
    vals[:, -1, -1, -1] = 65535.0
    image[(slice(None),) + sl] = vals * (0.37 if fractional else 1.0)
    inner = np.zeros(size, np.uint8)
    core = tuple(slice(max(1, n // 4), n - max(1, n // 4) + 1) for n in size)
    inner[core] = r.choice(np.array([0, 1, 2, 4], np.uint8), size=inner[core].shape)
    label[sl] = inner
    if not soft:
        return image, label
    sf = np.zeros((3,) + tuple(dims), np.float32)
    sf[(slice(None),) + sl] = r.random((3,) + tuple(size)).astype(np.float32) * (inner > 0)
    return image, label, sf


def trigger_case(value, seed):
    image, label = make_case(DIMS, (2, 3, 4), (6, 7, 9), seed)
    image[2, 4, 5, 6] = value
    return image, label


def roundtrip_cases():
    out = [("margin%d" % m, make_case(DIMS, (m, m, m), tuple(n - 2 * m for n in DIMS), 10 + m)) for m in (0, 1, 5)]
    one = (np.zeros((4,) + DIMS, np.float32), np.zeros(DIMS, np.uint8))
    one[0][3, 18, 0, 36] = 12.0
    out.append(("one-voxel", one))
    out.append(("all-zero", (np.zeros((4,) + DIMS, np.float32), np.zeros(DIMS, np.uint8))))
    for k, v in enumerate((0.5, -1.0, 65536.0, -0.0, float("nan"))):
        out.append(("trigger %r" % v, trigger_case(v, 20 + k)))
    out.append(("soft", make_case(DIMS, (4, 5, 6), (8, 9, 20), 30, soft=True)))
    wide = make_case(DIMS, (4, 5, 6), (8, 9, 20), 31, soft=True)
    wide[2][1, 1, 17, 2] = 0.25                               # a soft value outside the image's and the label's box widens it
    out.append(("soft-wide", wide))
    return out


def bits_equal(a, b):
    """equality of bytes of two float32 arrays (NaN and -0.0 included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_round_trip():
    from brats2019_amd import dataloader as DL
    named = roundtrip_cases()
    called = []

    def once(item):
        return lambda: (called.append(1), item)[1]
    store = DL.ResidentCases([once(item) for _, item in named], (8, 8, 10))
    assert len(store) == len(named) == len(called)            # callables are called once, at build
    total = 0
    for i, (name, item) in enumerate(named):
        image, label = item[0], item[1]
        soft = item[2] if len(item) > 2 else None
        view = store[i]
        lo, size, kind = DL.pack_case_host(image, label, soft)
        assert (view.box, view.kind) == ((lo, size), kind), name
        assert view.kind == ("float32" if name.startswith("trigger") else "uint16"), name
        assert view.shape == DIMS and view.channels == 4 and view.patch_size == (8, 8, 10), name
        assert tuple(view.image.shape) == (4,) + size and tuple(view.label.shape) == size, name
        assert view.image.dtype == (torch.uint16 if kind == "uint16" else torch.float32), name
        uimage, ulabel, usoft = store.unpack(i)
        assert bits_equal(uimage.cpu().numpy(), image), name
        assert np.array_equal(ulabel.cpu().numpy(), DL.remap_labels(label)), name
        assert (usoft is None) == (soft is None) and (soft is None or bits_equal(usoft.cpu().numpy(), soft)), name
        with np.errstate(all="ignore"):
            ref = DL.DeviceCase(image, label, (8, 8, 10), soft=soft)
        assert bits_equal(view.mean, ref.mean) and bits_equal(view.std, ref.std), name
        assert np.array_equal(view.bbox, ref.bbox), name
        total += view.nbytes
    assert store.nbytes == total
    assert store[3].box == ((18, 0, 36), (1, 1, 1)) and store[4].box == ((0, 0, 0), (1, 1, 1))
    assert store[11].box[0][0] == 1 and store[10].box[0][0] == 4
    again = DL.ResidentCases([item for _, item in named[:3]], (8, 8, 10))        # the probe is deterministic
    assert all(again[i].box == store[i].box and torch.equal(again[i].label, store[i].label) for i in range(3))


def test_dtype_and_max_bytes():
    from brats2019_amd import dataloader as DL
    exact = make_case(DIMS, (5, 5, 5), (9, 13, 27), 40)
    forced = DL.ResidentCases([exact], (8, 8, 10), dtype="float32")
    assert forced[0].kind == "float32" and forced[0].image.dtype == torch.float32
    assert bits_equal(forced.unpack(0)[0].cpu().numpy(), exact[0])
    voxels = 9 * 13 * 27
    assert forced.nbytes == voxels * (4 * 4 + 1) and DL.ResidentCases([exact], (8, 8, 10), dtype="uint16").nbytes == voxels * (4 * 2 + 1)
    with pytest.raises(ValueError, match="not exact"):
        DL.ResidentCases([exact, trigger_case(0.5, 41)], (8, 8, 10), dtype="uint16")
    need = voxels * 9
    assert DL.ResidentCases([exact], (8, 8, 10), max_bytes=need).nbytes == need
    with pytest.raises(ValueError, match="max_bytes"):
        DL.ResidentCases([exact], (8, 8, 10), max_bytes=need - 1)
    with pytest.raises(ValueError, match="case 1 .*max_bytes"):
        DL.ResidentCases([exact, exact], (8, 8, 10), max_bytes=2 * need - 1)


# ---------------------------------------------------------------------------------------------------------------- the gathers
@pytest.fixture(scope="module")
def pairs():
    """{(kind, soft): (view, DeviceCase)} of the same arrays, built once and left unchanged"""
    from brats2019_amd import dataloader as DL
    keys, items = [], []
    for kind in ("uint16", "float32"):
        for soft in (False, True):
            keys.append((kind, soft))
            items.append(make_case(DIMS, BOX[0], BOX[1], 50, fractional=kind == "float32", soft=soft))
    store = DL.ResidentCases(items, PATCHES[0])
    out = {}
    for i, (key, item) in enumerate(zip(keys, items)):
        assert store[i].kind == key[0] and store[i].box == BOX
        out[key] = (store[i], DL.DeviceCase(item[0], item[1], PATCHES[0], soft=item[2] if len(item) > 2 else None))
    return out


def params(lo, scale, flags=0, seed=0, **extra):
    r = np.random.default_rng(seed)
    p = dict(crop_lo=np.asarray(lo), scale=np.asarray(scale, np.float64), flips=[bool(flags & 1), bool(flags & 2), bool(flags & 4)], transpose=bool(flags & 8),
             gain=r.uniform(0.9, 1.1, 4), bias=r.uniform(-0.2, 0.2, 4))
    p.update(extra)
    return p


def zoom_crops(patch):
    """crops inside the volume: one centred on the tissue box, one across each of its six faces, one wholly outside it"""
    fit = lambda lo: tuple(int(min(max(v, 0), d - p)) for v, d, p in zip(lo, DIMS, patch))
    centre = [BOX[0][a] + BOX[1][a] // 2 - patch[a] // 2 for a in range(3)]
    crops = [fit(centre)]
    for a in range(3):
        for face in (BOX[0][a], BOX[0][a] + BOX[1][a]):
            lo = list(centre)
            lo[a] = face - patch[a] // 2
            crops.append(fit(lo))
            assert crops[-1][a] < face < crops[-1][a] + patch[a]
    crops.append(fit((0, centre[1], centre[2])))
    assert crops[-1][0] + patch[0] <= BOX[0][0]               # wholly outside the box along D
    return crops


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("kind", ["uint16", "float32"])
@pytest.mark.parametrize("patch", PATCHES)
def test_zoom_pass_equals_the_whole_case(pairs, patch, kind, soft):
    from brats2019_amd import dataloader as DL
    view, case = pairs[(kind, soft)]
    seen = 0.0
    for n, lo in enumerate(zoom_crops(patch)):
        for scale in SCALES[:3] if n else SCALES:
            for flags in range(16):
                p = params(lo, scale, flags, seed=flags)
                d, t = DL.augment_patch(view, p, patch)
                d0, t0 = DL.augment_patch(case, p, patch)
                assert d.shape == d0.shape and torch.equal(d, d0) and torch.equal(t, t0), (lo, scale, flags)
        seen += float(t0.abs().sum())
    assert seen > 0


@pytest.mark.parametrize("kind,soft", [("uint16", False), ("float32", True)])
def test_zoom_weights_where_a_fused_product_rounds_differently(pairs, kind, soft):
    """At scale 0.7 the double product 10 * 0.7 rounds up to exactly 7.0 while the exact product lies below 7: the weight (float)(x - floor(x)) is
    0 if the product is rounded before the subtraction and -4.4e-16 if the two are fused.  The standalone kernels fuse, so every instantiation
    must: indices 10 (scales 0.7, 0.9, 1.1, 1.3) and 5 (scale 1.2) need patch extents above 10, which the other patches of this file lack."""
    from brats2019_amd import dataloader as DL
    for scale, index in ((0.7, 10), (0.9, 10), (1.1, 10), (1.3, 10), (1.2, 5)):
        x = np.float64(index) * np.float64(scale)
        exact = np.longdouble(index) * np.longdouble(np.float64(scale)) - np.longdouble(np.floor(x))     # 4 + 53 bits: exact in the 64-bit mantissa
        if np.finfo(np.longdouble).nmant >= 63:
            assert np.float32(x - np.floor(x)) != np.float32(np.float64(exact)), (scale, index)
    view, case = pairs[(kind, soft)]
    patch = (11, 12, 21)
    for lo in ((4, 5, 8), (8, 11, 16), (0, 0, 0)):
        for scale in ((0.7, 0.7, 0.7), (1.3, 1.3, 1.3), (0.9, 1.1, 1.2), (1.2, 0.9, 1.1)):
            for flags in (0, 7, 8, 13):
                p = params(lo, scale, flags, seed=flags)
                d, t = DL.augment_patch(view, p, patch)
                d0, t0 = DL.augment_patch(case, p, patch)
                assert torch.equal(d, d0) and torch.equal(t, t0), (lo, scale, flags)


def affine_crops(patch):
    return [tuple(BOX[0][a] + BOX[1][a] // 2 - patch[a] // 2 for a in range(3)), (-3, 2, 5), (DIMS[0] - 5, DIMS[1] - 4, DIMS[2] - 6), (4, -2, 30)]


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("kind", ["uint16", "float32"])
@pytest.mark.parametrize("patch", PATCHES)
def test_affine_pass_equals_the_whole_case(pairs, patch, kind, soft):
    from brats2019_amd import dataloader as DL
    view, case = pairs[(kind, soft)]
    a30, a90 = np.pi / 6.0, np.pi / 2.0
    for lo in affine_crops(patch):
        for angles in ((a30, 0.0, 0.0), (0.0, a30, 0.0), (0.0, 0.0, a30), (a30, a30, a30), (a90, 0.0, 0.0), (0.0, 0.0, a90), (0.0, 0.0, 0.0)):
            for flags, scale in ((0, SCALES[1]), (5, SCALES[3]), (10, SCALES[0]), (15, SCALES[2])):
                base = params(lo, scale, flags, seed=flags)
                d0, t0 = DL.augment_patch(case, dict(base, rotation=dict(angles=angles)), patch)
                for mapping in (None, "row", "brick"):
                    d, t = DL.augment_patch(view, dict(base, rotation=dict(angles=angles, mapping=mapping)), patch)
                    assert torch.equal(d, d0) and torch.equal(t, t0), (lo, angles, flags, mapping)
    explicit = dict(matrix=np.array([[0.9, 0.2, 0.0], [-0.1, 1.1, 0.3], [0.0, -0.2, 0.8]]), offset=np.array([3.5, -1.25, 9.0]))
    d, t = DL.augment_patch(view, params((0, 0, 0), SCALES[1], 9, rotation=explicit), patch)
    d0, t0 = DL.augment_patch(case, params((0, 0, 0), SCALES[1], 9, rotation=explicit), patch)
    assert torch.equal(d, d0) and torch.equal(t, t0)


@pytest.mark.parametrize("kind,soft", [("uint16", False), ("float32", True)])
def test_elastic_through_a_view(pairs, kind, soft):
    from brats2019_amd import dataloader as DL
    view, case = pairs[(kind, soft)]
    lo = zoom_crops(PATCHES[0])[1]
    for flags, rot in ((0, None), (13, None), (6, dict(angles=(0.3, -0.2, 0.5)))):
        p = params(lo, SCALES[3], flags, seed=3, elastic=dict(sigma=11.0, alpha=900.0, seed=77))
        if rot is not None:
            p["rotation"] = rot
        d, t = DL.augment_patch(view, p)
        d0, t0 = DL.augment_patch(case, p)
        assert torch.equal(d, d0) and torch.equal(t, t0), (flags, rot)


def test_entry_point_refusals(pairs):
    from brats2019_amd import dataloader as DL
    view, _ = pairs[("uint16", False)]
    with pytest.raises(RuntimeError, match="crop must lie inside"):
        DL.augment_patch(view, params((DIMS[0] - 7, 0, 0), SCALES[1]), PATCHES[0])
    with pytest.raises(RuntimeError, match="scale must be positive"):
        DL.augment_patch(view, params((0, 0, 0), (1.0, 0.0, 1.0)), PATCHES[0])
    with pytest.raises(ValueError, match="singular"):
        DL.augment_patch(view, params((0, 0, 0), SCALES[1], rotation=dict(matrix=np.ones((3, 3)))), PATCHES[0])


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.fixture(scope="module")
def mixed():
    """a store of uint16 and float32, hard and soft cases of two shapes, for the 8 x 8 x 10 patch"""
    from brats2019_amd import dataloader as DL
    other = (21, 20, 25)
    items = [make_case(DIMS, BOX[0], BOX[1], 60), make_case(other, (3, 2, 4), (15, 16, 18), 61, fractional=True),
             make_case(other, (0, 0, 0), other, 62, soft=True), make_case(DIMS, (5, 4, 3), (10, 17, 30), 63, fractional=True, soft=True)]
    store = DL.ResidentCases(items, PATCHES[0])
    assert [v.kind for v in store] == ["uint16", "float32", "uint16", "float32"]
    return store


def batch_params(store, indices, seed):
    r = np.random.default_rng(seed)
    out = []
    for n, i in enumerate(indices):
        dims, patch = store[i].shape, store.patch_size
        lo = [int(r.integers(0, d - p + 1)) for d, p in zip(dims, patch)]
        p = params(lo, r.uniform(0.7, 1.3, 3), int(r.integers(0, 16)), seed=seed + n)
        if n % 2:
            p["rotation"] = dict(angles=tuple(r.uniform(-0.6, 0.6, 3)), mapping=(None, "row", "brick")[(n // 2) % 3])
        out.append(p)
    return out


def test_batch_equals_the_stack_of_singles(mixed):
    from brats2019_amd import dataloader as DL, _lib as L
    for count in (1, 3, L.AUG_BATCH_MAX + 1):
        indices = [(3 * n) % len(mixed) for n in range(count)]
        plist = batch_params(mixed, indices, 100 + count)
        singles = [DL.augment_patch(mixed[i], p) for i, p in zip(indices, plist)]
        data, target = DL.augment_batch(mixed, indices, plist)
        assert tuple(data.shape) == (count, 4) + PATCHES[0] and tuple(target.shape) == (count, 3) + PATCHES[0]
        assert torch.equal(data, torch.stack([d for d, _ in singles])) and torch.equal(target, torch.stack([t for _, t in singles])), count
        data2, target2 = DL.augment_batch(mixed, indices, plist)
        assert torch.equal(data2, data) and torch.equal(target2, target), count
        if count > 1:
            assert len({mixed[i].kind for i in indices}) == 2 and len({mixed[i].soft is None for i in indices}) == 2
            assert len({mixed[i].shape for i in indices}) == 2


def test_mixed_and_uniform_launches(mixed):
    """a launch whose samples share kind, target and mode runs a kernel that holds that one body; a launch that mixes them runs the one with all
    eight.  Both against the singles: every combination in one mixed launch, and each case twice in a launch of its own, zoom and affine."""
    from brats2019_amd import dataloader as DL
    r = np.random.default_rng(9)

    def sample(i, n, affine):
        lo = [int(r.integers(0, d - q + 1)) for d, q in zip(mixed[i].shape, PATCHES[0])]
        p = params(lo, (0.9, 1.1, 1.2), int(r.integers(0, 16)), seed=n)
        if affine:
            p["rotation"] = dict(angles=tuple(r.uniform(-0.6, 0.6, 3)))
        return p
    batches = [([0, 1, 2, 3, 0, 1, 2, 3], [False] * 4 + [True] * 4)]
    batches += [([i, i, i], [affine] * 3) for i in range(4) for affine in (False, True)]
    for indices, modes in batches:
        plist = [sample(i, n, affine) for n, (i, affine) in enumerate(zip(indices, modes))]
        singles = [DL.augment_patch(mixed[i], p) for i, p in zip(indices, plist)]
        data, target = DL.augment_batch(mixed, indices, plist)
        assert torch.equal(data, torch.stack([d for d, _ in singles])) and torch.equal(target, torch.stack([t for _, t in singles])), (indices, modes)


def test_batch_refusals_at_the_entry_point(mixed):
    """what the Python checks do not see is refused by the C entry point before any launch"""
    from brats2019_amd import dataloader as DL
    plist = batch_params(mixed, [0, 1], 7)
    plist[0].pop("rotation", None)
    plist[0]["crop_lo"] = np.array([DIMS[0], 0, 0])
    with pytest.raises(RuntimeError, match="sample 0: the crop must lie inside"):
        DL.augment_batch(mixed, [0, 1], plist)


# ---------------------------------------------------------------------------------------------------------------- reader, loader, training
RDIMS = (40, 44, 48)


@pytest.fixture(scope="module")
def reader_cases():
    return [make_case(RDIMS, (6, 5, 7), (28, 33, 35), 70), make_case(RDIMS, (2, 8, 4), (34, 30, 40), 71, soft=True),
            make_case(RDIMS, (5, 5, 5), (30, 34, 38), 72, fractional=True)]


def reseed(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def reader_options():
    from brats2019_amd import dataloader as DL
    busy = DL.IntensityConfig(p_blur=0.6, p_lowres=0.6, p_noise=0.6, p_brightness=0.6, p_contrast=0.6, p_gamma_invert=0.3, p_gamma=0.6)
    return dict(rotation=DL.RotationConfig(p_rotation=0.6), rotation_seed=5, intensity=busy, intensity_seed=6)


@pytest.mark.parametrize("per_image,augment", [(1, "none"), (2, "none"), (1, "all"), (2, "all"), (2, "no-elastic")])
def test_reader_items_equal_the_list_reader(reader_cases, per_image, augment):
    from brats2019_amd import dataloader as DL
    kw = dict(patches_from_single_image=per_image)
    if augment != "none":
        kw.update(reader_options())
    if augment == "all":
        kw.update(elastic=True, elastic_seed=4)
    patch = (16, 16, 16)
    order = [0, 1, 1, 2, 0, 2]
    reseed(11)
    ref = DL.SimpleReader(reader_cases, patch, **kw)
    want = [ref[i] for i in order]
    store = DL.ResidentCases(reader_cases, patch)
    reseed(11)
    reader = DL.SimpleReader(store, patch, **kw)
    for i, (data, target) in zip(order, want):
        got = reader[i]
        assert torch.equal(got[0][0], data[0]) and torch.equal(got[1][0], target[0]), i
    assert len(reader) == len(ref)


@pytest.mark.parametrize("elastic", [False, True])
def test_loader_batches_equal_the_dataloader(reader_cases, elastic):
    from brats2019_amd import dataloader as DL
    patch = (16, 16, 16)
    kw = dict(reader_options(), patches_from_single_image=1, images_in_epoch=10, elastic=elastic, elastic_seed=4)
    lists = [[0, 1, 2], [2, 2, 0], [1, 0, 1]]
    reseed(12)
    want = list(torch.utils.data.DataLoader(DL.SimpleReader(reader_cases, patch, **kw), batch_sampler=lists, num_workers=0))
    reseed(12)
    reader = DL.SimpleReader(DL.ResidentCases(reader_cases, patch), patch, **kw)
    loader = DL.ResidentLoader(reader, batch_sampler=lists)
    got = list(loader)
    assert len(loader) == len(got) == len(want) == 3
    for (gd, gt), (wd, wt) in zip(got, want):
        assert isinstance(gd, list) and isinstance(gt, list) and len(gd) == len(gt) == 1
        assert tuple(gd[0].shape) == (3, 4) + patch and torch.equal(gd[0], wd[0]) and torch.equal(gt[0], wt[0])
    assert len(DL.ResidentLoader(reader, batch_size=4)) == 2 and len(DL.ResidentLoader(reader, batch_size=4, drop_last=False)) == 3
    reseed(13)
    batches = list(DL.ResidentLoader(reader, batch_size=4))               # the default sampler draws a permutation of the epoch
    assert len(batches) == 2 and tuple(batches[0][0][0].shape) == (4, 4) + patch


def _train(loader, tmp_path, tag):
    from brats2019_amd import model as M, loss as L, train as TR, metrics as MT
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(41, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="r" + tag, models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    losses = []

    class Rec:
        def add_scalar(self, name, val, step):
            if name.startswith("loss/"):
                losses.append(float(val))
    tr.tb_writer = Rec()
    held = [([T(O.make_input(1, 32, 32, 32, seed=3))], [T(O.make_target(1, 32, 32, 32, seed=3))])]
    tr.train(criterion=[L.Dice_loss_joint(index=0, priority=1), L.BCE_Loss(index=0, bg_weight=1e-2)], optimizer=torch.optim.Adam,
             optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True), scheduler=None, scheduler_params=None, training_data_loader=loader,
             evaluation_data_loader=held, split_into_tiles=False, pretrained_weights=None, train_metrics=[MT.Dice(name="Dice")],
             val_metrics=[MT.Dice(name="Dice")], track_metric="Dice", epoches=1, default_val=np.zeros(3),
             comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b), eval_cpu=False, continue_form_pretraining=False)
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]), losses


def test_training_through_the_resident_loader(reader_cases, tmp_path):
    from brats2019_amd import dataloader as DL
    patch = (32, 32, 32)
    kw = dict(reader_options(), patches_from_single_image=1, images_in_epoch=4)
    lists = [[0, 1], [2, 0]]
    reseed(14)
    w_ref, l_ref = _train(torch.utils.data.DataLoader(DL.SimpleReader(reader_cases, patch, **kw), batch_sampler=lists, num_workers=0), tmp_path, "list")
    reseed(14)
    w_new, l_new = _train(DL.ResidentLoader(DL.SimpleReader(DL.ResidentCases(reader_cases, patch), patch, **kw), batch_sampler=lists), tmp_path, "store")
    assert len(l_ref) == 4 and l_new == l_ref
    assert torch.equal(w_new, w_ref)
