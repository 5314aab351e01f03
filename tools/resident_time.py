#!/usr/bin/env python3
"""The resident training set (csrc/resident.hip, dataloader.ResidentCases / augment_batch) against the path it replaces, in one run on the MI355X,
at the BraTS case 4 x 240 x 240 x 155 and the benchmark's 128^3 patch.  The case is synthetic and seeded: an ellipsoid "brain" of integer
intensities filling a 140 x 170 x 140 box, exact zeros around it, nested-ball labels.

  (a) one reader item from a list of numpy cases (DeviceCase build + augment, as the reader does it; wall clock, synchronised) against one item of
      SimpleReader(ResidentCases);
  (b) the packed uint16 gather, the packed float32 gather and ru_augment_patch on the same case and parameters; the same three at 0 and 30 degrees
      against ru_augment_patch_affine; with the compulsory bytes of each (outputs once, the scaled crop of the stored source once);
  (c) a batch of 4: one ru_augment_batch_packed launch against four ru_augment_patch calls + torch.stack;
  (d) the store's bytes per case against the unpacked case;
  (e) the build time per case.

The legs of a comparison are timed in ALTERNATING rounds; a leg's figure is the median over the rounds and its spread is max - min over them.  Device
legs are timed as HIP events around back-to-back calls and, separately, as the median of calls timed alone after a 1 GB read that evicts the 256 MB
MALL.  Three conditions, each against the parent path measured in this run with that path's spread as the margin, back to back AND after a flush:
  1. the resident item is faster than the list item:           t_resident < t_list - spread_list
  2. the uint16 gather is not slower than ru_augment_patch:    t_u16 <= t_plain + spread_plain
  3. the batch launch is not slower than four calls + stack:   t_batch <= t_four + spread_four
The exit status is 1 if one is missed.  An optional text file (the compiler's kernel-resource-usage remarks) is appended as it is.

usage: resident_time.py [reps] [rounds] [resources.txt]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import dataloader as DL

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
resources = sys.argv[3] if len(sys.argv) > 3 else None
assert torch.cuda.is_available(), "resident_time.py measures on the GPU; there is nothing to time without one"

_flush = None


def flush():
    global _flush
    if _flush is None:
        _flush = (torch.ones(1 << 28, dtype=torch.float32, device="cuda"), torch.empty((), dtype=torch.float32, device="cuda"))
    torch.sum(_flush[0], dim=0, out=_flush[1])


def device_ms(fn, flushed):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a MALL flush (as tools/rotate_time.py)"""
    fn()
    torch.cuda.synchronize()
    if not flushed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    ts = []
    for _ in range(reps):
        flush()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def wall_ms(fn, flushed):
    """ms of one synchronised call on the wall clock (host work is part of what is measured)"""
    if flushed:
        flush()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(legs, timer):
    """{name: (median, spread)} for back to back and after a flush: every round times every leg once, in turn"""
    out = {}
    for flushed in (False, True):
        ts = {name: [] for name, _ in legs}
        for _ in range(rounds):
            for name, fn in legs:
                ts[name].append(timer(fn, flushed))
        out[flushed] = {name: (sorted(v)[len(v) // 2], max(v) - min(v)) for name, v in ts.items()}
    return out


def show(res, legs, mbytes=None, unit=1e3, unit_name="us"):
    for name, _ in legs:
        (t0, s0), (t1, s1) = res[False][name], res[True][name]
        rate = "" if mbytes is None else "  [%6.1f MB: %5.2f / %5.2f TB/s]" % (mbytes[name], mbytes[name] / t0 / 1e3, mbytes[name] / t1 / 1e3)
        print("    %-58s %9.1f %s (spread %7.1f) back to back, %9.1f %s (spread %7.1f) after a flush%s" % (name, t0 * unit, unit_name, s0 * unit, t1 * unit, unit_name, s1 * unit, rate))


verdicts = []


def condition(text, res, new, parent, strictly):
    ok = True
    parts = []
    for flushed in (False, True):
        (tn, _), (tp, sp) = res[flushed][new], res[flushed][parent]
        met = tn < tp - sp if strictly else tn <= tp + sp
        ok = ok and met
        parts.append("%s %.4f ms against %.4f ms, spread %.4f ms: %s" % ("after a flush" if flushed else "back to back", tn, tp, sp, "met" if met else "MISSED"))
    verdicts.append(ok)
    print("  CONDITION %s: %s -- %s" % (text, "MET" if ok else "MISSED", "; ".join(parts)))


# ------------------------------------------------------------------------------------------------------------------------ the case
shape, patch = (240, 240, 155), (128, 128, 128)
v = patch[0] * patch[1] * patch[2]
rs = np.random.default_rng(0)
zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij")
r2 = ((zz - 120) / 70.0) ** 2 + ((yy - 120) / 85.0) ** 2 + ((xx - 78) / 70.0) ** 2
brain = r2 <= 1.0
image = np.zeros((4,) + shape, np.float32)
for c in range(4):
    image[c][brain] = rs.integers(40, 1800 + 400 * c, size=int(brain.sum())).astype(np.float32)
ball = lambda rad: (zz - 125) ** 2 + (yy - 110) ** 2 + (xx - 80) ** 2 <= rad * rad
label = np.zeros(shape, np.uint8)
label[ball(30)] = 2
label[ball(20)] = 1
label[ball(10)] = 4
del zz, yy, xx, r2
full_bytes = image.nbytes + label.nbytes
print("case 4 x %s (%.1f MB float32 + uint8 label), patch %s; %d reps per timing, %d alternating rounds; times include the Python wrapper" % (shape, full_bytes / 1e6, patch, reps, rounds))

# ------------------------------------------------------------------------------------------------------------------------ (e), (d)
build = []
for _ in range(3):
    torch.cuda.synchronize()
    t = time.perf_counter()
    store = DL.ResidentCases([(image, label), (image, label)], patch)
    torch.cuda.synchronize()
    build.append((time.perf_counter() - t) * 1e3 / 2)
store32 = DL.ResidentCases([(image, label)], patch, dtype="float32")
view, view32 = store[0], store32[0]
print("(e) ResidentCases build: %.1f ms per case (median of 3 builds of 2 cases; upload, statistics, host label box, probe, pack)" % sorted(build)[1])
print("(d) store: kind %s, box lo %s size %s: %.1f MB per case = %.1f %% of the %.1f MB unpacked case (%.2fx smaller); forced float32: %.1f MB"
      % (view.kind, view.box[0], view.box[1], view.nbytes / 1e6, 100.0 * view.nbytes / full_bytes, full_bytes / 1e6, full_bytes / view.nbytes, view32.nbytes / 1e6))
ui, ul, _ = store.unpack(0)
print("    unpack(pack(case)) == case, byte for byte: %s" % (ui.cpu().numpy().tobytes() == image.tobytes() and np.array_equal(ul.cpu().numpy(), DL.remap_labels(label))))
del ui, ul

# ------------------------------------------------------------------------------------------------------------------------ (a)
import random


def item_legs():
    np.random.seed(1)
    random.seed(1)
    lst = DL.SimpleReader([(image, label), (image, label)], patch, patches_from_single_image=1)
    res = DL.SimpleReader(store, patch, patches_from_single_image=1)
    state = {"l": 0, "r": 0}

    def list_items():                                        # two items: the reader builds a DeviceCase for one of every two (its counter starts at 1)
        for _ in range(2):
            lst[state["l"]]
            state["l"] += 1

    def resident_items():
        for _ in range(2):
            res[state["r"]]
            state["r"] += 1
    return [("two items, SimpleReader over a list of numpy cases", list_items), ("two items, SimpleReader over ResidentCases", resident_items)]


legs = item_legs()
for _, fn in legs:
    fn()
res = alternate(legs, wall_ms)
print("(a) reader items, wall clock, synchronised (two consecutive items: the list reader builds one DeviceCase in them)")
show(res, legs, unit=1.0, unit_name="ms")
torch.cuda.synchronize()
t = time.perf_counter()
case = DL.DeviceCase(image, label, patch)
torch.cuda.synchronize()
print("    one DeviceCase build alone: %.1f ms" % ((time.perf_counter() - t) * 1e3))
condition("1 (the resident item is faster than the list item)", res, legs[1][0], legs[0][0], True)

# ------------------------------------------------------------------------------------------------------------------------ (b)
base = dict(crop_lo=np.array([40, 40, 10]), scale=np.array([0.9, 1.1, 1.2]), flips=[True, False, True], transpose=True, gain=np.full(4, 1.05), bias=np.full(4, 0.1))
out_mb = (4 + 3) * v * 4 / 1e6
src = v * 0.9 * 1.1 * 1.2 / 1e6                               # source voxels under the scaled crop, in millions
mb_plain, mb_u16, mb_f32 = out_mb + src * (4 * 4 + 1), out_mb + src * (4 * 2 + 1), out_mb + src * (4 * 4 + 1)
legs = [("ru_augment_patch (whole float32 case)", lambda: DL.augment_patch(case, base)),
        ("packed uint16 gather (ru_augment_batch_packed, N = 1)", lambda: DL.augment_patch(view, base)),
        ("packed float32 gather (ru_augment_batch_packed, N = 1)", lambda: DL.augment_patch(view32, base))]
res = alternate(legs, device_ms)
print("(b) zoom pass, the same case and parameters; bytes: outputs once + the scaled crop of the stored source once (the box clips the crop further)")
show(res, legs, dict(zip([n for n, _ in legs], (mb_plain, mb_u16, mb_f32))))
d0, t0 = DL.augment_patch(case, base)
d1, t1 = DL.augment_patch(view, base)
d2, t2 = DL.augment_patch(view32, base)
print("    the three give the same bytes: %s" % (torch.equal(d0, d1) and torch.equal(t0, t1) and torch.equal(d0, d2) and torch.equal(t0, t2)))
condition("2 (the uint16 gather is not slower than ru_augment_patch)", res, legs[1][0], legs[0][0], False)
for deg in (0, 30):
    p = dict(base, rotation=dict(angles=(np.deg2rad(deg),) * 3))
    legs = [("ru_augment_patch_affine, %2d degrees (whole float32 case)" % deg, lambda: DL.augment_patch(case, p)),
            ("packed uint16 gather, affine, %2d degrees" % deg, lambda: DL.augment_patch(view, p)),
            ("packed float32 gather, affine, %2d degrees" % deg, lambda: DL.augment_patch(view32, p))]
    res = alternate(legs, device_ms)
    print("    affine pass at %d degrees on all axes, brick mapping" % deg)
    show(res, legs, dict(zip([n for n, _ in legs], (mb_plain, mb_u16, mb_f32))))
    a, b = DL.augment_patch(case, p), DL.augment_patch(view, p)
    print("    whole case and packed case give the same bytes: %s" % (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))

# ------------------------------------------------------------------------------------------------------------------------ (c)
plist = [dict(base, transpose=False, crop_lo=np.array([40 + 8 * n, 50 - 4 * n, 10 + 3 * n]), flips=[bool(n & 1), bool(n & 2), True]) for n in range(4)]


def four_parent():
    items = [DL.augment_patch(case, q) for q in plist]
    return torch.stack([d for d, _ in items]), torch.stack([t for _, t in items])


def four_views():
    items = [DL.augment_patch(view, q) for q in plist]
    return torch.stack([d for d, _ in items]), torch.stack([t for _, t in items])


legs = [("four ru_augment_patch calls + torch.stack (whole case)", four_parent), ("four packed uint16 calls + torch.stack", four_views),
        ("one ru_augment_batch_packed launch, N = 4 (uint16)", lambda: DL.augment_batch(store, [0, 1, 0, 1], plist))]
res = alternate(legs, device_ms)
print("(c) a batch of 4 patches, written as [4,4,128,128,128] + [4,3,128,128,128]")
show(res, legs)
a, b = four_parent(), DL.augment_batch(store, [0, 1, 0, 1], plist)
print("    the batch launch gives the bytes of the stack: %s" % (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))
condition("3 (the batch launch is not slower than four calls + stack)", res, legs[2][0], legs[0][0], False)

if resources and os.path.exists(resources):
    print("kernel resources of the gather and pack kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    sys.stdout.write(open(resources).read())
print("conditions met: %d of %d" % (sum(verdicts), len(verdicts)))
sys.exit(0 if all(verdicts) else 1)
