"""The eight-corner gathers on the device against their float64 restatements (tests/gather_inputs.py, tied to scipy in tests/test_gather_host.py):
ru_augment_patch / ru_augment_patch_soft, ru_augment_patch_affine with both thread mappings, ru_elastic_warp, and ru_augment_batch_packed -- held to
float64 itself, on uint16 and float32 boxes, one sample at a time, in one launch of more than RU_AUG_BATCH_MAX samples and in mixed launches.

Every call goes through the C ABI with the test's own mean and inv_std, writes into buffers with a guard region behind them, and is made twice:
the second call gives the first one's bytes and the guard is intact.  The exact family equals the float64 result bit for bit on every voxel; the
real family lies within the per-voxel bars derived in gather_inputs, no voxel left out; order-0 warp targets are exact.  The three two-pass cases
exceed the grid caps they are there for (4096 blocks of 256 for the zoom pass, the affine row mapping and a packed zoom-only launch; 8192 for the warp).

Worst error / bar on the MI355X, data / targets (test_report prints them with -s); the exact family and the order-0 targets were bit-equal:
  ru_augment_patch                          0.567 / 0.295        ru_augment_patch_soft                     0.578 / 0.356
  ru_augment_patch_affine, row mapping      0.583 / 0.407        brick and default mapping                 0.553 / 0.387
  ru_elastic_warp                           0.413 / exact
  ru_augment_batch_packed, one sample: zoom 0.578 / 0.356 (uint16 and float32 boxes), affine 0.553 / 0.387 (both boxes, all mappings)
  ru_augment_batch_packed, launches of nine samples (zoom-only uint16, mixed exact, mixed real)             0.567 / 0.342
The emulation of the same operation order in numpy (tests/test_gather_host.py) predicts 0.58, 0.55 and 0.41 for the three gathers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gather_inputs as G
from op_cases import GUARD, PATTERN

pytestmark = pytest.mark.gpu
WORST = {}                                   # entry point -> (worst error / bar, case): filled by the tests, printed by test_report
ids = lambda cases: [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------- plumbing
class Guarded:
    """`count` float32 values (stale: every byte 0xFF, a NaN) with GUARD bytes of PATTERN behind them"""

    def __init__(self, count):
        self.count = int(count)
        self.buf = torch.full((4 * self.count + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.buf[4 * self.count:] = PATTERN
        self.values = self.buf[:4 * self.count].view(torch.float32)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[4 * self.count:] == PATTERN).all())

    def untouched(self):
        return self.intact() and bool((self.buf[:4 * self.count] == 0xFF).all())

    def numpy(self, shape):
        return self.values.cpu().numpy().reshape(shape)


def arr(ctype, values):
    return (ctype * len(values))(*values)


def floats(a):
    return arr(C.c_float, [float(v) for v in a])


@functools.lru_cache(maxsize=None)
def device_volume(name):
    v = G.volume(name)
    return torch.from_numpy(v["image"].copy()).cuda(), torch.from_numpy(v["label"].copy()).cuda(), torch.from_numpy(v["soft"].copy()).cuda()


@functools.lru_cache(maxsize=None)
def packed_view(name, channels, soft, dtype="auto"):
    """the packed case of a volume's first `channels` channels, hard or soft: (ResidentCases, its only view)"""
    from brats2019_amd import dataloader as DL
    v = G.volume(name)
    item = (v["image"][:channels].copy(), v["label"].copy()) + ((v["soft"].copy(),) if soft else ())       # the shared arrays are read-only
    store = DL.ResidentCases([item], (1, 1, 1), dtype=dtype)
    view = store[0]
    assert view.box == v["box"] and view.kind == ("float32" if name == "frac" or dtype == "float32" else "uint16")
    return store, view


@functools.lru_cache(maxsize=None)
def reference(name):
    for case in G.all_cases() + G.two_pass_cases():
        if case["name"] == name:
            return G.run(case)
    raise KeyError(name)


def out_shape(case, k):
    p = case["patch"]
    return (k,) + ((p[1], p[0], p[2]) if case["flags"] & 8 else p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hold(entry, case, got, key):
    """the device result `got` of case[key] against the restatement: bit for bit in the exact family and wherever the bar is 0, else within the bar"""
    ref = reference(case["name"])
    want, bar = ref[key], ref["bar_" + key]
    assert got.shape == want.shape and got.dtype == np.float32, (entry, case["name"], key)
    if case["family"] == "exact" or (case["kind"] == "warp" and key == "target"):
        assert not bar.any()
        assert np.array_equal(want.astype(np.float32).astype(want.dtype), want)
        same = bits(got) == bits(want)
        assert same.all(), (entry, case["name"], key, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        return
    ratio, where = G.worst_ratio(got, want, bar)
    if ratio >= WORST.get((entry, key), (-1.0, ""))[0]:
        WORST[(entry, key)] = (ratio, case["name"])
    assert ratio <= 1.0, (entry, case["name"], key, ratio, where, float(got[where]), float(want[where]), float(bar[where]))


def twice(call, data, target):
    """run `call` twice into the guarded buffers: the same bytes both times, the guards intact"""
    from brats2019_amd import _lib as L
    L.check(call(), "first call")
    torch.cuda.synchronize()
    first = [b.buf.clone() for b in (data, target) if b is not None]
    for b in (data, target):
        if b is not None:
            b.buf[:4 * b.count] = 0x7F                                                       # other stale bytes: nothing of the first call is left to be found
    L.check(call(), "second call")
    torch.cuda.synchronize()
    for b, f in zip([b for b in (data, target) if b is not None], first):
        assert b.intact(), "the guard behind an output was written"
        assert torch.equal(b.buf, f), "two calls gave different bytes"


# ---------------------------------------------------------------------------------------------------------------- the entry points
def zoom_call(case, data, target):
    from brats2019_amd import _lib as L
    lib = L.load()
    v = G.volume(case["vol"])
    image, label, soft = device_volume(case["vol"])
    c = case["C"]
    tail = (floats(v["mean"][:c]), floats(v["istd"][:c]), c) + tuple(v["dims"]) + (arr(C.c_int, list(case["lo"])), arr(C.c_int, list(case["patch"])),
                                                                                  arr(C.c_double, list(case["scale"])), case["flags"], floats(case["gain"]),
                                                                                  floats(case["bias"]), data.ptr(), target.ptr(), L.stream())
    if case["soft"]:
        return lambda: lib.ru_augment_patch_soft(L.f32(image), None, L.f32(soft), *tail)     # `label` is not read with soft targets
    return lambda: lib.ru_augment_patch(L.f32(image), L.ptr(label), *tail)


def affine_call(case, mapping, data, target):
    from brats2019_amd import _lib as L
    lib = L.load()
    v = G.volume(case["vol"])
    image, label, soft = device_volume(case["vol"])
    c = case["C"]
    args = (L.f32(image), None if case["soft"] else L.ptr(label), L.f32(soft) if case["soft"] else None, floats(v["mean"][:c]), floats(v["istd"][:c]), c) + \
        tuple(v["dims"]) + (arr(C.c_int, list(case["patch"])), arr(C.c_double, [float(x) for x in case["matrix"].reshape(-1)]),
                            arr(C.c_double, [float(x) for x in case["offset"]]), case["flags"], floats(case["gain"]), floats(case["bias"]),
                            L.AFFINE_MAPPINGS[mapping], data.ptr(), target.ptr(), L.stream())
    return lambda: lib.ru_augment_patch_affine(*args)


def packed_call(cases, data, target, mappings=None, dtype="auto"):
    """one ru_augment_batch_packed call over `cases` (zoom and affine cases of one patch and channel count)"""
    from brats2019_amd import _lib as L
    lib = L.load()
    n = len(cases)
    cdesc, pdesc, keep = (L.CaseDesc * n)(), (L.PatchDesc * n)(), []
    for i, case in enumerate(cases):
        v = G.volume(case["vol"])
        store, view = packed_view(case["vol"], case["C"], case["soft"], dtype)
        keep.append(store)
        d, p, c = cdesc[i], pdesc[i], case["C"]
        d.image, d.label, d.soft = view.image.data_ptr(), view.label.data_ptr(), (view.soft.data_ptr() if case["soft"] else None)
        d.kind, d.C = L.PACK_KINDS[view.kind], c
        d.dims[:], d.box_lo[:], d.box_size[:] = v["dims"], view.box[0], view.box[1]
        d.mean[:c], d.inv_std[:c] = [float(x) for x in v["mean"][:c]], [float(x) for x in v["istd"][:c]]
        p.flags = case["flags"]
        p.gain[:c], p.bias[:c] = [float(x) for x in case["gain"]], [float(x) for x in case["bias"]]
        if case["kind"] == "zoom":
            p.mode = L.AUG_ZOOM
            p.crop_lo[:], p.scale[:] = list(case["lo"]), list(case["scale"])
        else:
            p.mode, p.mapping = L.AUG_AFFINE, L.AFFINE_MAPPINGS[(mappings[i] if mappings else None) or case.get("mapping") or "default"]
            p.matrix[:], p.offset[:] = [float(x) for x in case["matrix"].reshape(-1)], [float(x) for x in case["offset"]]
    patch = arr(C.c_int, list(cases[0]["patch"]))
    return lambda: (keep, lib.ru_augment_batch_packed(cdesc, pdesc, n, patch, data.ptr(), target.ptr(), L.stream()))[1]


def run_pair(entry, case, make_call):
    voxels = int(np.prod(case["patch"]))
    data, target = Guarded(case["C"] * voxels), Guarded(3 * voxels)
    twice(make_call(data, target), data, target)
    hold(entry, case, data.numpy(out_shape(case, case["C"])), "data")
    hold(entry, case, target.numpy(out_shape(case, 3)), "target")


ZOOM, AFFINE, WARP = G.zoom_cases(), G.affine_cases(), G.warp_cases()


@pytest.mark.parametrize("case", ZOOM, ids=ids(ZOOM))
def test_zoom(case):
    run_pair("ru_augment_patch_soft" if case["soft"] else "ru_augment_patch", case, lambda d, t: zoom_call(case, d, t))
    kind = "float32" if case["vol"] == "frac" else "uint16"
    run_pair("ru_augment_batch_packed zoom %s" % kind, case, lambda d, t: packed_call([case], d, t))
    if kind == "uint16":                                                                     # the same values in a float32 box
        run_pair("ru_augment_batch_packed zoom float32", case, lambda d, t: packed_call([case], d, t, dtype="float32"))


@pytest.mark.parametrize("case", AFFINE, ids=ids(AFFINE))
def test_affine(case):
    kind = "float32" if case["vol"] == "frac" else "uint16"
    for mapping in ("row", "brick", "default"):
        run_pair("ru_augment_patch_affine %s" % mapping, case, lambda d, t: affine_call(case, mapping, d, t))
        run_pair("ru_augment_batch_packed affine %s %s" % (kind, mapping), case, lambda d, t: packed_call([case], d, t, mappings=[mapping]))
    if kind == "uint16":
        run_pair("ru_augment_batch_packed affine float32 brick", case, lambda d, t: packed_call([case], d, t, mappings=["brick"], dtype="float32"))


def warp_run(case):
    from brats2019_amd import _lib as L
    lib = L.load()
    c, nt, p = case["C"], case["T"], case["patch"]
    voxels = int(np.prod(p))
    src = torch.from_numpy(case["data"].copy()).cuda() if c else None
    tgt = torch.from_numpy(case["target"].copy()).cuda() if nt else None
    disp = torch.from_numpy(case["disp"].copy()).cuda()
    data, target = (Guarded(c * voxels) if c else None), (Guarded(nt * voxels) if nt else None)
    gain, bias = (floats(case["gain"]), floats(case["bias"])) if c else (None, None)
    call = lambda: lib.ru_elastic_warp(L.f32(src) if c else None, c, L.f32(tgt) if nt else None, nt, L.ptr(disp), p[0], p[1], p[2], case["flags"], gain, bias,
                                       data.ptr() if c else None, target.ptr() if nt else None, L.stream())
    twice(call, data, target)
    if c:
        hold("ru_elastic_warp", case, data.numpy(out_shape(case, c)), "data")
    if nt:
        hold("ru_elastic_warp", case, target.numpy(out_shape(case, nt)), "target")


@pytest.mark.parametrize("case", WARP, ids=ids(WARP))
def test_warp(case):
    warp_run(case)


@pytest.mark.parametrize("name", sorted(G.BATCHES))
def test_packed_batch(name):
    """one call, every sample against its own float64 restatement"""
    from brats2019_amd import _lib as L
    cases = [G.by_name(n) for n in G.BATCHES[name]]
    n, c, patch = len(cases), cases[0]["C"], cases[0]["patch"]
    assert n > L.AUG_BATCH_MAX and all(k["C"] == c and k["patch"] == patch for k in cases)
    if "mixed" in name:                                                                      # the first launch of eight mixes every kind of sample
        first = cases[:L.AUG_BATCH_MAX]
        assert {k["kind"] for k in first} == {"zoom", "affine"} and {k["soft"] for k in first} == {False, True}
        assert "exact" in name or {k["vol"] for k in first} == {"brats", "frac"}
        assert {k.get("mapping") for k in first if k["kind"] == "affine"} >= {"row", "brick"}
    else:
        assert {k["kind"] for k in cases} == {"zoom"}
    voxels = int(np.prod(patch))
    data, target = Guarded(n * c * voxels), Guarded(n * 3 * voxels)
    twice(packed_call(cases, data, target), data, target)
    d, t = data.numpy((n, c * voxels)), target.numpy((n, 3 * voxels))
    for i, case in enumerate(cases):
        hold("ru_augment_batch_packed batch", case, d[i].reshape(out_shape(case, c)), "data")
        hold("ru_augment_batch_packed batch", case, t[i].reshape(out_shape(case, 3)), "target")


# ---------------------------------------------------------------------------------------------------------------- a second grid-stride pass
def test_two_pass_zoom_and_packed_zoom():
    case = G.two_pass_cases()[0]
    assert int(np.prod(case["patch"])) > G.CAP_ZOOM                                          # 4096 blocks of 256: voxels beyond come from a second pass
    run_pair("ru_augment_patch", case, lambda d, t: zoom_call(case, d, t))
    run_pair("ru_augment_batch_packed zoom uint16", case, lambda d, t: packed_call([case], d, t))


def test_two_pass_affine_row():
    case = G.two_pass_cases()[1]
    assert int(np.prod(case["patch"])) > G.CAP_ZOOM
    run_pair("ru_augment_patch_affine row", case, lambda d, t: affine_call(case, "row", d, t))


def test_two_pass_warp():
    case = G.two_pass_cases()[2]
    assert int(np.prod(case["patch"])) > G.CAP_WARP                                          # 8192 blocks of 256
    warp_run(case)


# ---------------------------------------------------------------------------------------------------------------- statistics and refusals
def test_zscore_stats_are_the_host_statistics():
    """the real family's mean and inv_std are those of `zscore_stats` (its float64 sums run in another order: 1e-12)"""
    from brats2019_amd import dataloader as DL
    for name in ("brats", "frac", "big"):
        v = G.volume(name)
        mean, std = DL.zscore_stats(device_volume(name)[0])
        m, s = G.zscore_host(v["image"])
        assert np.abs(mean - m).max() <= 1e-12 * np.abs(m).max() and np.abs(std - s).max() <= 1e-12 * np.abs(s).max()
        assert np.array_equal(m.astype(np.float32), v["mean"]) and np.array_equal((1.0 / s).astype(np.float32), v["istd"])


@pytest.mark.parametrize("axis,scale,patch,message", [(1, np.inf, 7, r"scale\[1\] is not finite"), (2, 2.0 ** 30 / 8.0, 9, r"scale\[2\] \* \(patch\[2\] - 1\)"),
                                                      (0, 1.0e300, 5, r"scale\[0\] \* \(patch\[0\] - 1\)")])
def test_library_refuses_a_scale_the_kernel_cannot_hold(axis, scale, patch, message):
    """RU_EINVAL before any launch from all three entries, the axis named, the outputs untouched; the largest accepted coordinate still runs"""
    import re
    from brats2019_amd import _lib as L
    base = G.by_name("zoom real 5x7x9 s0")
    assert base["patch"][axis] == patch
    for soft in (False, True):
        bad = dict(base, soft=soft, scale=tuple(scale if a == axis else s for a, s in enumerate(base["scale"])))
        voxels = int(np.prod(bad["patch"]))
        for make in (zoom_call, lambda k, d, t: packed_call([k], d, t)):
            data, target = Guarded(4 * voxels), Guarded(3 * voxels)
            assert make(bad, data, target)() == -1                                           # RU_EINVAL
            assert re.search(message, L.last_error()), L.last_error()
            assert data.untouched() and target.untouched()
    edge = dict(base, scale=tuple((2.0 ** 30 - 1.0) / (patch - 1) if a == axis else s for a, s in enumerate(base["scale"])))
    data, target = Guarded(4 * int(np.prod(edge["patch"]))), Guarded(3 * int(np.prod(edge["patch"])))
    L.check(zoom_call(edge, data, target)(), "the largest accepted scale")
    assert data.intact() and target.intact()
    ref = G.run(dict(edge, name="largest accepted scale"))
    ratio, _ = G.worst_ratio(data.numpy(out_shape(edge, 4)), ref["data"], ref["bar_data"])
    assert ratio <= 1.0, ratio


def test_report():
    """not a check of its own: prints what the tests above measured"""
    for key in sorted(WORST):
        print("worst error / bar  %-46s %-7s %.3f  (%s)" % (key[0], key[1], WORST[key][0], WORST[key][1]))
    assert all(r <= 1.0 for r, _ in WORST.values())
