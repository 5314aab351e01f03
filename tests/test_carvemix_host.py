"""CarveMix without a GPU: the numpy restatement (`dataloader.carvemix_host`) against a direct statement with scipy's Euclidean distance transform,
R2 = floor(V^(2/3)) by exact integer cubes, the degenerate rules, the guard that no case of the device test passes on a trivial mask (checked
here for the exact list tests/test_carvemix.py walks), the new names in the header, the ctypes table and the build list, and the promise that
without the option every draw and both global generator streams are the parent's."""
import os
import random
import re

import numpy as np
import pytest

import carvemix_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = I.cases()


@pytest.fixture(scope="module")
def host_results():
    from brats2019_amd import dataloader as DL
    return {c["name"]: DL.carvemix_host(c["data"], c["target"], c["donor_data"], c["donor_target"], c["u"], c["side"], c["dst"]) for c in CASES}


def test_the_case_list_covers_what_it_must():
    shapes = {(c["data"].shape[0], c["data"].shape[1]) + c["data"].shape[2:] for c in CASES}
    assert {(2, 4) + I.SHAPE_A, (1, 4) + I.SHAPE_B, (1, 1) + I.SHAPE_C} <= shapes
    seen = {(kind, u, side) for c in CASES for kind, u, side in zip(c["kinds"], c["u"], c["side"])}
    for kind in ("ball", "two", "box", "single", "soft", "empty", "full"):
        for u, side in I.DRAWS:
            assert (kind, u, side) in seen, (kind, u, side)
    assert any(c["offset8"] for c in CASES)
    assert any(c["dst"] == [1] and c["data"].shape[0] == 2 for c in CASES) and any(c["dst"] == [1, 0] for c in CASES)
    for c in CASES:                                           # a NaN and a -0.0 in donor and receiver alike
        for key in ("data", "donor_data"):
            assert np.isnan(c[key]).any() and (np.signbit(c[key]) & (c[key] == 0)).any(), (c["name"], key)


def test_mask_equals_the_direct_statement_with_scipy(host_results):
    """M = rint(edt^2) compared with T, signs by side of the mask: scipy's transform is float64 and exact to rounding at these extents"""
    ndi = pytest.importorskip("scipy.ndimage")
    for c in CASES:
        _, _, mask, thr, vol = host_results[c["name"]]
        for k in range(len(c["kinds"])):
            g = c["donor_target"][k, 0] > np.float32(0.5)
            assert int(vol[k]) == int(g.sum())
            if g.any() and not g.all():
                s = np.where(g, -np.rint(ndi.distance_transform_edt(g) ** 2), np.rint(ndi.distance_transform_edt(~g) ** 2)).astype(np.int64)
            else:
                s = np.zeros(g.shape, np.int64)
            assert np.array_equal(mask[k].astype(bool), s <= int(thr[k])), (c["name"], k)


def test_r2_is_the_floor_of_the_two_thirds_power_by_integer_cubes():
    from brats2019_amd import dataloader as DL
    for v in list(range(0, 4097)) + [2 ** 27 - 1, 2 ** 27]:
        q = DL.carvemix_r2(v)
        assert q ** 3 <= v * v < (q + 1) ** 3, v
    assert DL.carvemix_r2(1) == 1 and DL.carvemix_r2(8) == 4 and DL.carvemix_r2(2 ** 27) == 2 ** 18


def test_threshold_rules():
    from brats2019_amd import dataloader as DL
    for u, side in I.DRAWS:
        assert DL.carvemix_threshold_host(0, 105, u, side) == -2 ** 31
        assert DL.carvemix_threshold_host(105, 105, u, side) == 2 ** 31 - 1
    assert DL.carvemix_threshold_host(1, 105, 0.0, "outer") == 0 and DL.carvemix_threshold_host(1, 105, 0.0, "inner") == 0
    assert DL.carvemix_threshold_host(1, 105, 0.75, "inner") == -1                       # -ceil(0.5625 * 0.25)
    assert DL.carvemix_threshold_host(1000, 10 ** 6, 1.0 - 2.0 ** -53, "outer") == 99    # R2 = 100, (u u) R2 just below it
    assert DL.carvemix_threshold_host(1000, 10 ** 6, 0.5, "outer") == 25 and DL.carvemix_threshold_host(1000, 10 ** 6, 0.5, "inner") == -7


def test_degenerate_donors(host_results):
    for c in CASES:
        data, target, mask, thr, vol = host_results[c["name"]]
        dst = c["dst"] if c["dst"] is not None else list(range(len(c["kinds"])))
        for k, kind in enumerate(c["kinds"]):
            if kind == "empty":                               # nothing is carved: the receiver is unchanged
                assert vol[k] == 0 and thr[k] == -2 ** 31 and not mask[k].any()
                assert np.array_equal(I.words(data[dst[k]]), I.words(c["data"][dst[k]])) and np.array_equal(I.words(target[dst[k]]), I.words(c["target"][dst[k]]))
            if kind == "full":                                # the output is the donor
                assert vol[k] == mask[k].size and thr[k] == 2 ** 31 - 1 and mask[k].all()
                assert np.array_equal(I.words(data[dst[k]]), I.words(c["donor_data"][k])) and np.array_equal(I.words(target[dst[k]]), I.words(c["donor_target"][k]))


def test_no_case_passes_on_a_trivial_mask(host_results):
    """every non-degenerate mask has selected and unselected voxels, inner masks lie inside G and outer masks contain it"""
    for c in CASES:
        _, _, mask, thr, _ = host_results[c["name"]]
        for k, kind in enumerate(c["kinds"]):
            if kind in I.DEGENERATE:
                continue
            m, g = mask[k].astype(bool), c["donor_target"][k, 0] > np.float32(0.5)
            assert m.any() and not m.all(), (c["name"], k)
            if c["side"][k] == "inner":
                assert not (m & ~g).any() and thr[k] <= 0, (c["name"], k)
            else:
                assert not (g & ~m).any() and thr[k] >= 0, (c["name"], k)


def test_receivers_outside_dst_and_inputs_are_untouched(host_results):
    for c in CASES:
        before = {key: c[key].copy() for key in ("data", "target", "donor_data", "donor_target")}
        data, target = host_results[c["name"]][:2]
        dst = c["dst"] if c["dst"] is not None else list(range(len(c["kinds"])))
        for n in range(c["data"].shape[0]):
            if n not in dst:
                assert np.array_equal(I.words(data[n]), I.words(c["data"][n])) and np.array_equal(I.words(target[n]), I.words(c["target"][n]))
        for key, val in before.items():                       # the restatement returns new arrays
            assert np.array_equal(I.words(val), I.words(c[key]))


def test_the_select_is_of_words(host_results):
    """where M the receiver holds the donor's bits, elsewhere its own: checked on every word of one case with NaN and -0.0 on both sides"""
    c = next(c for c in CASES if c["name"].startswith("A-ball-two-"))
    data, target, mask = host_results[c["name"]][:3]
    for k, n in enumerate(c["dst"]):
        m = mask[k].astype(bool)[None]
        assert np.array_equal(I.words(data[n]), np.where(m, I.words(c["donor_data"][k]), I.words(c["data"][n])))
        assert np.array_equal(I.words(target[n]), np.where(m, I.words(c["donor_target"][k]), I.words(c["target"][n])))


def test_argument_checks_come_before_the_device():
    import torch
    from brats2019_amd import dataloader as DL
    c = CASES[0]
    t = {key: torch.from_numpy(c[key]) for key in ("data", "target", "donor_data", "donor_target")}
    call = lambda **kw: DL.carvemix(**dict(dict(t, u=c["u"], side=c["side"], dst=c["dst"]), **kw))
    for kw in (dict(u=[0.5]), dict(u=[0.5, 1.0]), dict(u=[0.5, float("nan")]), dict(side=["outer", "middle"]), dict(dst=[1, 1]), dict(dst=[0, 2]),
               dict(dst=[0]), dict(target=t["target"][:, :2]), dict(donor_data=t["donor_data"][:, :, 1:]), dict(data=t["data"].double())):
        with pytest.raises(ValueError):
            call(**kw)
    big = torch.zeros((1, 1, 1, 1, 513))
    with pytest.raises(ValueError, match="512"):
        DL.carvemix(big, big.expand(1, 3, 1, 1, 513), big, big.expand(1, 3, 1, 1, 513), [0.5], ["outer"])
    with pytest.raises(ValueError, match="dst"):              # K < N without a dst list
        DL.carvemix(t["data"], t["target"], t["donor_data"][:1], t["donor_target"][:1], [0.5], "outer")
    with pytest.raises(ValueError, match="p_mix"):
        DL.CarveMixConfig(p_mix=1.5)


def test_new_names_in_header_ctypes_table_and_sources():
    from brats2019_amd import _lib as L, build as B
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "resunet_hip.h")).read(), flags=re.S)
    for name in ("ru_carvemix_workspace_bytes", "ru_carvemix_threshold", "ru_carvemix_mix"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    defines = dict(re.findall(r"#define\s+(RU_\w+)\s+(-?\d+)", src))
    assert (int(defines["RU_CARVE_OUTER"]), int(defines["RU_CARVE_INNER"])) == (L.CARVE_SIDES["outer"], L.CARVE_SIDES["inner"])
    assert int(defines["RU_CARVE_BATCH_MAX"]) == L.CARVE_BATCH_MAX >= 1
    assert "carvemix.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "carvemix.hip"))


# ---------------------------------------------------------------------------------------------------------------- the draws
def parent_draw(bbox, patch_size, channels=4):
    """`draw_augment_params` as it stood before the generator arguments: the global modules, in the reference's order"""
    center = np.random.rand(3)
    center = center * (bbox[1] - bbox[0]) + bbox[0]
    left_bottom = (center - np.array(patch_size) / 2.0).astype(np.int32)
    random.random()
    random.random()
    scale = [0.7 + random.random() * 0.6 for _ in range(3)]
    flips = [random.random() > 0.5 for _ in range(3)]
    transpose = random.random() > 0.5
    gain = np.random.uniform(0.9, 1.1, size=(channels, 1, 1, 1)).reshape(-1)
    bias = np.random.uniform(-0.2, 0.2, size=(channels, 1, 1, 1)).reshape(-1)
    return dict(crop_lo=left_bottom, scale=np.array(scale), flips=flips, transpose=transpose, gain=gain, bias=bias)


def _same_params(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def _states():
    return random.getstate(), np.random.get_state()


def _same_states(a, b):
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


BBOX = np.array([[9.0, 9.0, 9.0], [20.0, 24.0, 22.0]])


class _Case(object):
    """what `SimpleReader._draw` reads of a case"""
    bbox = BBOX
    image = np.zeros((4, 1, 1, 1), np.float32)


def _host_reader(**kw):
    """a reader whose case is in place already, so that `_draw` runs without a device"""
    from brats2019_amd import dataloader as DL
    reader = DL.SimpleReader([None, None, None], (16, 16, 16), patches_from_single_image=10 ** 6, **kw)
    reader.case, reader.patches_from_current_image = _Case(), 0
    return reader


def test_without_the_option_the_draws_and_the_global_streams_are_the_parents():
    from brats2019_amd import dataloader as DL
    random.seed(5)
    np.random.seed(5)
    want = [parent_draw(BBOX, (16, 16, 16)) for _ in range(6)]
    end = _states()
    for kw in (dict(), dict(carvemix=False), dict(carvemix=DL.CarveMixConfig(p_mix=0.0), carvemix_seed=3)):
        random.seed(5)
        np.random.seed(5)
        reader = _host_reader(**kw)
        for i, w in enumerate(want):
            _same_params(reader._draw(i), w)
        _same_states(_states(), end)
    random.seed(5)
    np.random.seed(5)
    for w in want:
        _same_params(DL.draw_augment_params(BBOX, (16, 16, 16)), w)
    _same_states(_states(), end)


def test_with_the_option_every_added_draw_is_private():
    """p_mix = 1: the receiver's draws and the global streams are still the parent's; the donor's draws are those of private generators and
    repeat under the same carvemix_seed"""
    from brats2019_amd import dataloader as DL
    random.seed(6)
    np.random.seed(6)
    want = [parent_draw(BBOX, (16, 16, 16)) for _ in range(5)]
    end = _states()
    runs = []
    for _ in range(2):
        random.seed(6)
        np.random.seed(6)
        reader = _host_reader(carvemix=DL.CarveMixConfig(p_mix=1.0), carvemix_seed=9)
        reader._donor_case = lambda index: _Case()
        got = [reader._draw(i) for i in range(5)]
        _same_states(_states(), end)
        record = []
        for g, w in zip(got, want):
            mix = g.pop("carvemix")
            _same_params(g, w)
            assert 0 <= mix["donor"] < 3 and 0.0 <= mix["u"] < 1.0 and mix["side"] in ("outer", "inner")
            assert set(mix["params"]) == set(w)               # the plain zoom path: no elastic field, no rotation
            record.append((mix["donor"], mix["u"], mix["side"], tuple(mix["params"]["crop_lo"]), tuple(mix["params"]["gain"])))
        runs.append(record)
    assert runs[0] == runs[1]
    rng = random.Random(1)
    state = _states()
    assert DL.draw_carvemix_params(rng, DL.CarveMixConfig(p_mix=0.0), 3) is None
    sides = {DL.draw_carvemix_params(rng, DL.CarveMixConfig(p_mix=1.0), 3)["side"] for _ in range(40)}
    assert sides == {"outer", "inner"}
    _same_states(_states(), state)


def test_the_donor_takes_the_receivers_transpose_when_the_patch_is_not_square():
    from brats2019_amd import dataloader as DL
    from brats2019_amd.dataloader import SimpleReader
    random.seed(7)
    np.random.seed(7)
    reader = SimpleReader([None, None], (16, 12, 16), patches_from_single_image=10 ** 6, carvemix=DL.CarveMixConfig(p_mix=1.0), carvemix_seed=2)
    reader.case, reader.patches_from_current_image = _Case(), 0
    reader._donor_case = lambda index: _Case()
    seen = set()
    for i in range(24):
        p = reader._draw(i)
        assert p["carvemix"]["params"]["transpose"] == p["transpose"]
        seen.add(p["transpose"])
    assert seen == {False, True}
