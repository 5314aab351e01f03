#!/usr/bin/env python3
"""Rotation augmentation (csrc/rotate.hip, dataloader.augment_patch with a `rotation` entry) against the plain `ru_augment_patch` zoom pass and the
per-sample training step, at the BraTS case 4 x 240 x 240 x 155 and the benchmark's 128^3 patch, in one run:

  * `ru_augment_patch` alone: the existing zoom pass, the yardstick;
  * `ru_augment_patch_affine` with the same crop, scale, flips, transpose, gain and bias at angles 0, 15 and 30 degrees on all three axes,
    with both thread mappings (row: 256 consecutive output voxels along W per workgroup; brick: a compact 4 x 2 x 8 brick per wavefront).

Every row is timed as HIP events around back-to-back calls and as the median of calls timed alone after a MALL flush.  The bytes are the zoom
pass's compulsory traffic (the outputs once, the scaled crop of the four modalities and the label once), so the rate column compares rows; a
rotated gather touches more lines than that.  Times include the Python wrapper's output allocation.  The one condition: every rotated row must
cost less than the per-sample training step, or the exit status is 1.

usage: rotate_time.py [reps] [step_ms_per_sample]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import dataloader as DL

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
step_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 3.66          # 14.65 ms per batch-4 step / 4 (README, committed round-6 run)
assert torch.cuda.is_available(), "rotate_time.py measures on the GPU; there is nothing to time without one"

_flush = None


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the operands
    from the 256 MB MALL (as tools/intensity_time.py)"""
    global _flush
    for _ in range(warm):
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
    if _flush is None:
        _flush = (torch.ones(1 << 28, dtype=torch.float32, device="cuda"), torch.empty((), dtype=torch.float32, device="cuda"))
    ts = []
    for _ in range(reps):
        torch.sum(_flush[0], dim=0, out=_flush[1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def row(what, fn, mbytes):
    t0, t1 = timed(fn, False), timed(fn, True)
    print("  %-64s %8.1f us back to back (%5.2f TB/s), %8.1f us after a MALL flush (%5.2f TB/s)" % (what, t0 * 1e3, mbytes / t0 / 1e3, t1 * 1e3, mbytes / t1 / 1e3))
    return t0, t1


patch = (128, 128, 128)
v = patch[0] * patch[1] * patch[2]
rs = np.random.default_rng(0)
shape = (240, 240, 155)
image = (np.abs(rs.standard_normal((4,) + shape)) * 120 + 40).astype(np.float32)
label = np.zeros(shape, np.float32)
label[80:160, 80:160, 50:110] = 2
label[100:140, 100:140, 65:95] = 1
label[110:130, 110:130, 72:88] = 3
case = DL.DeviceCase(image, label, patch)
base = dict(crop_lo=np.array([40, 40, 10]), scale=np.array([0.9, 1.1, 1.2]), flips=[True, False, True], transpose=True, gain=np.full(4, 1.05), bias=np.full(4, 0.1))
mb = (4 + 3) * v * 4 / 1e6 + (4 * 4 + 1) * v * 1.1 * 0.9 * 1.2 / 1e6          # as tools/elastic_time.py

print("case 4 x %s, patch %s; %d reps; times include the output allocation of the Python wrapper; %.0f MB counted per call" % (shape, patch, reps, mb))
plain = row("ru_augment_patch alone (the zoom pass, the default path)", lambda: DL.augment_patch(case, base), mb)
results = {}
for deg in (0, 15, 30):
    for mapping in ("row", "brick"):
        p = dict(base, rotation=dict(angles=(np.deg2rad(deg),) * 3, mapping=mapping))
        results[deg, mapping] = row("ru_augment_patch_affine, %2d degrees on all axes, %s mapping" % (deg, mapping), lambda: DL.augment_patch(case, p), mb)

d_row, t_row = DL.augment_patch(case, dict(base, rotation=dict(angles=(np.deg2rad(30),) * 3, mapping="row")))
d_brk, t_brk = DL.augment_patch(case, dict(base, rotation=dict(angles=(np.deg2rad(30),) * 3, mapping="brick")))
print("  the two mappings give the same bytes at 30 degrees: %s" % (torch.equal(d_row, d_brk) and torch.equal(t_row, t_brk)))
for mapping in ("row", "brick"):
    print("  %-5s mapping / zoom pass, back to back (after a flush): %s" % (mapping, ", ".join(
        "%d deg %.2fx (%.2fx)" % (deg, results[deg, mapping][0] / plain[0], results[deg, mapping][1] / plain[1]) for deg in (0, 15, 30))))
worst = max(max(t) for t in results.values())
ok = worst < step_ms
print("  slowest rotated patch %.3f ms = %.1f %% of the %.2f ms per-sample training step: %s" % (worst, 100 * worst / step_ms, step_ms, "below it" if ok else "NOT below it"))
sys.exit(0 if ok else 1)
