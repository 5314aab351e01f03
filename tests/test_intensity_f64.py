"""The intensity augmentation kernels (csrc/intensity.hip) on the device against the float64 restatement of tests/intensity_inputs.py (tied to
`dataloader.intensity_augment_host` and scipy in tests/test_intensity_f64_host.py), under its per-voxel bars, on every case and every voxel.

Every case goes through the C ABI (`ru_intensity_augment`): the input sits in a buffer of its own at the case's pointer offset and is read back
unchanged; the output is pre-filled with NaN and has guard floats before and after it; the workspace is exactly `ru_intensity_workspace_bytes`
at a base one byte past a 256-byte boundary with a 0xA5 guard behind it; every call is made twice and gives the same bytes.  Then the exact
family (`intensity_inputs.exact_family`: copies, brightness, variance 0, zoom 1, one coarse sample, the clip bounds, constant channels, the two
routes on the same data) and the route through `dataloader.intensity_augment`.

Worst error / bar on the MI355X by the stage a channel's output leaves (test_report prints them with -s).  In that run the emulation of
tests/test_intensity_f64_host.py gave the same seven figures to three digits; that agreement is an observation and is not asserted -- numpy's log2 /
exp2 / log / cos are not the device's, and the bars allow for the difference:
  blur 0.296   low-res 0.912   noise 0.683 (u1 = 2^-53, the largest radius)   brightness 0.999 (one product just above a power of two, bit-equal)
  contrast 0.667   gamma 0.315   gamma with retain-stats 0.431
No case exposed a defect in the second tile column, the strided loop over more than 256 partials, the constant channel or the alignment-forced
scalar route; the noise was the defect (`noise_u1_float32` in intensity_inputs: logf(float32(u1)) alone), and csrc/intensity.hip no longer has it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import intensity_inputs as I
from op_cases import GUARD, PATTERN

pytestmark = pytest.mark.gpu
CASES = I.cases()
ids = [c["name"] for c in CASES]
FRONT = 64                                   # guard floats before the output: 256 bytes, so that the case's offset alone decides the alignment


@functools.lru_cache(maxsize=None)
def device_result(name):
    """the case through the C ABI, twice: float32 [C, *shape] (read-only)"""
    from brats2019_amd import dataloader as DL, _lib as L
    lib = L.load()
    case, x = I.by_name(name), I.input_of(name)
    n, (p0, p1, p2) = x.size, case["shape"]
    src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    assert src.data_ptr() % 256 == 0
    src_view = src[case["in_off"]:case["in_off"] + n]
    src_view.copy_(torch.from_numpy(x.reshape(-1).copy()))
    back = FRONT + case["out_off"]
    dst = torch.empty(back + n + FRONT, dtype=torch.float32, device="cuda")
    assert dst.data_ptr() % 256 == 0
    out_view = dst[back:back + n]
    assert (src_view.data_ptr() % 16 == 0) == (case["in_off"] % 4 == 0) and (out_view.data_ptr() % 16 == 0) == (case["out_off"] % 4 == 0)
    nbytes = int(lib.ru_intensity_workspace_bytes(case["C"], p0, p1, p2))
    assert nbytes > 0
    ws = torch.full((1 + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")       # stale workspace bytes read as NaN
    assert ws.data_ptr() % 256 == 0
    ws[1 + nbytes:] = PATTERN
    blk = DL.intensity_param_block(case["params"])
    runs = []
    for _ in range(2):
        dst.fill_(float("nan"))
        rc = lib.ru_intensity_augment(C.c_void_p(src_view.data_ptr()), C.c_void_p(out_view.data_ptr()), case["C"], p0, p1, p2, C.byref(blk),
                                      C.c_void_p(ws.data_ptr() + 1), nbytes, L.stream())
        L.check(rc, "ru_intensity_augment")
        torch.cuda.synchronize()
        host = dst.cpu().numpy()
        assert np.isnan(host[:back]).all() and np.isnan(host[back + n:]).all(), (name, "the guard floats around the output were written")
        assert bool((ws[1 + nbytes:] == PATTERN).all()), (name, "the guard behind the workspace was written")
        runs.append(host[back:back + n].copy())
    assert np.array_equal(src_view.cpu().numpy(), x.reshape(-1)) and not bool(src[:case["in_off"]].any()) and not bool(src[case["in_off"] + n:].any()), (name, "input written")
    assert runs[0].tobytes() == runs[1].tobytes(), (name, "two calls give different bytes")
    got = runs[0].reshape(x.shape)
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_against_float64(case):
    got, ref = device_result(case["name"]), I.reference(case["name"])
    assert got.dtype == np.float32 and got.shape == ref["out"].shape
    assert np.isfinite(got).all(), (case["name"], "a voxel was not written or is not finite", np.argwhere(~np.isfinite(got))[:4].tolist())
    bad = []
    for c, q in enumerate(case["params"]):
        ratio, where = I.worst_ratio(got[c], ref["out"][c], ref["bar"][c])
        stage = I.last_stage(q)
        print("%-28s channel %d leaves %-10s worst error / bar = %.3f at %s" % (case["name"], c, stage, ratio, tuple(int(v) for v in where)))
        if not ratio <= 1.0:
            bad.append((c, q, ratio, where, float(got[c][where]), float(ref["out"][c][where]), float(ref["bar"][c][where])))
    assert not bad, (case["name"], bad)


def test_exact_family():
    I.exact_family(device_result)


def test_pointer_offsets_take_the_scalar_route_and_change_no_byte():
    base = device_result("align base")
    for name in ("align in+1", "align out+1"):
        case = I.by_name(name)
        assert case["shape"][2] % 4 == 0 and (case["in_off"] + case["out_off"]) % 4 == 1
        assert device_result(name).tobytes() == base.tobytes(), name


@pytest.mark.parametrize("name", ("tiles float4", "tiles scalar", "ragged chunk", "grid 8x16x64 C8 unit", "grid 1x1x1 C1 unit", "constant gamma"))
def test_through_the_python_entry(name):
    """`dataloader.intensity_augment` (its own workspace and output allocation) gives the C-ABI call's bytes and leaves its input alone"""
    from brats2019_amd import dataloader as DL
    case, x = I.by_name(name), I.input_of(name)
    dev = torch.from_numpy(x.copy()).cuda()
    out = DL.intensity_augment(dev, case["params"])
    assert out.dtype == torch.float32 and tuple(out.shape) == x.shape and out.data_ptr() != dev.data_ptr()
    assert np.array_equal(dev.cpu().numpy(), x)
    assert out.cpu().numpy().tobytes() == device_result(name).tobytes()


def test_report():
    """the worst error / bar by the stage a channel leaves, over every case, from the cached device results (run with -s; the figures of the module
    docstring).  Nothing new is asserted here: test_against_float64 holds every voxel"""
    worst = {}
    for case in CASES:
        got, ref = device_result(case["name"]), I.reference(case["name"])
        for c, q in enumerate(case["params"]):
            ratio, _ = I.worst_ratio(got[c], ref["out"][c], ref["bar"][c])
            if ratio >= worst.get(I.last_stage(q), (-1.0,))[0]:
                worst[I.last_stage(q)] = (ratio, case["name"], c)
    for stage in ("copy",) + I.STAGES:
        if stage in worst:
            print("%-12s worst error / bar = %.3f   (%s, channel %d)" % ((stage,) + worst[stage]))
