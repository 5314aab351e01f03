#!/usr/bin/env python3
"""Elastic deformation (csrc/elastic.hip, dataloader.augment_patch with an `elastic` entry) against the plain `ru_augment_patch` pass, at the
benchmark's 4-channel 128^3 patch and at the reference's 144 x 144 x 128 patch, on a resident 4 x 240 x 240 x 155 case.

Per shape and per sigma (10, 20, 30: radius 40, 80, 120 -- the range `draw_augment_params` draws from): `ru_augment_patch` alone, then
`ru_elastic_noise`, `ru_elastic_field`, `ru_elastic_warp` and the whole elastic patch (zoom pass + noise + field + warp), each as HIP events around
back-to-back calls and as the median of calls timed alone after a MALL flush, with the bytes the pass must move (compulsory traffic: every
operand once) and the rate that gives.  The last line of each block compares the whole elastic patch with the per-sample training step.

usage: elastic_time.py [reps] [step_ms_per_sample]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import dataloader as DL, _lib as L

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
step_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 3.66          # 14.65 ms per batch-4 step / 4 (README, committed round-6 run)
assert torch.cuda.is_available(), "elastic_time.py measures on the GPU; there is nothing to time without one"

_flush = None


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the operands
    from the 256 MB MALL (as tools/ensemble_time.py)"""
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


rng = np.random.default_rng(0)
shape = (240, 240, 155)
image = (np.abs(rng.standard_normal((4,) + shape)) * 120 + 40).astype(np.float32)
label = np.zeros(shape, np.float32)
label[80:160, 80:160, 50:110] = 2
label[100:140, 100:140, 65:95] = 1
label[110:130, 110:130, 72:88] = 3

for patch in ((128, 128, 128), (144, 144, 128)):
    case = DL.DeviceCase(image, label, patch)
    v = patch[0] * patch[1] * patch[2]
    base = dict(crop_lo=np.array([40, 40, 10]), scale=np.array([0.9, 1.1, 1.2]), flips=[True, False, True], transpose=True,
                gain=np.full(4, 1.05), bias=np.full(4, 0.1))
    lib = L.load()
    ws = L.workspace(lib.ru_elastic_workspace_bytes(*patch), "cuda")
    noise = DL.elastic_noise(1, patch)
    disp = torch.empty_like(noise)
    d0, t0 = DL.augment_patch(case, dict(base, flips=[False] * 3, transpose=False))
    mb_aug = (4 + 3) * v * 4 / 1e6 + (4 * 4 + 1) * v * 1.1 * 0.9 * 1.2 / 1e6      # 7 float32 writes + the zoomed crop's reads (4 float32 + 1 byte per source voxel)
    mb_noise = 3 * v * 8 / 1e6                                                     # one float64 write per field
    mb_field = 3 * 2 * 3 * v * 8 / 1e6                                             # three passes, each one read and one write of [3][V] float64
    mb_warp = (3 * 8 + 2 * 7 * 4) * v / 1e6                                        # the field once, 7 float32 channels in and out
    print("patch %s, 4 image + 3 target channels, case %s; %d reps; times include the output allocation of the Python wrapper" % (patch, shape, reps))

    def row(what, fn, mbytes):
        t0_, t1_ = timed(fn, False), timed(fn, True)
        print("  %-58s %8.1f us back to back (%5.2f TB/s), %8.1f us after a MALL flush (%5.2f TB/s); %.0f MB"
              % (what, t0_ * 1e3, mbytes / t0_ / 1e3, t1_ * 1e3, mbytes / t1_ / 1e3, mbytes))
        return t0_, t1_

    plain = row("ru_augment_patch alone (the default path)", lambda: DL.augment_patch(case, base), mb_aug)
    row("ru_elastic_noise", lambda: DL.elastic_noise(1, patch), mb_noise)
    row("ru_elastic_warp (order 1 x 4, order 0 x 3, flips, transpose)", lambda: DL.elastic_warp(d0, t0, disp, base["flips"], True, base["gain"], base["bias"]), mb_warp)
    for sigma in (10.0, 20.0, 30.0):
        r = DL.elastic_radius(sigma)
        gfma = 3 * v * sum(min(2 * r + 1, n) for n in patch) / 1e9                # upper count: taps inside the volume, per voxel and axis
        tf = row("ru_elastic_field sigma %g (radius %d, <= %.1f G float64 FMA)" % (sigma, r, gfma), lambda: DL.elastic_field(noise, sigma, 2000.0, out=disp, ws=ws), mb_field)
        p = dict(base, elastic=dict(sigma=sigma, alpha=2000.0, seed=1))
        whole = row("whole elastic patch, sigma %g (zoom + noise + field + warp)" % sigma, lambda: DL.augment_patch(case, p), mb_aug + mb_noise + mb_field + mb_warp)
        print("    field = %.0f %% of the whole patch; whole / ru_augment_patch alone = %.1fx; whole patch %.3f ms vs %.2f ms per-sample training step: %s"
              % (100 * tf[0] / whole[0], whole[0] / plain[0], whole[0], step_ms, "UNDER the step" if whole[0] < step_ms else "OVER the step"))
    del case, noise, disp, ws, d0, t0
    torch.cuda.empty_cache()
