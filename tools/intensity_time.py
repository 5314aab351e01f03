#!/usr/bin/env python3
"""Intensity augmentation (csrc/intensity.hip, dataloader.intensity_augment) at the benchmark's 4-channel 128^3 patch, against the plain
`ru_augment_patch` pass and the per-sample training step, in one run:

  * each stage alone on all four channels, and the all-stages call;
  * a call with the default probabilities (`IntensityConfig()`), averaged over 64 seeded draws (a draw with no stage is the plain copy);
  * `ru_augment_patch` alone, on a resident 4 x 240 x 240 x 155 case.

Every row is timed as HIP events around back-to-back calls and as the median of calls timed alone after a MALL flush, with the bytes the call
must move (compulsory traffic: per channel one read or one write of V * 4 bytes per unit, the units of csrc/intensity.hip's header) and the rate
that gives.  Times include the Python wrapper's output and workspace allocation.

usage: intensity_time.py [reps] [step_ms_per_sample]"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import dataloader as DL

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
step_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 3.66          # 14.65 ms per batch-4 step / 4 (README, committed round-6 run)
assert torch.cuda.is_available(), "intensity_time.py measures on the GPU; there is nothing to time without one"

_flush = None


def timed(fn, flushed=False, warm=3, mean=False):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the operands
    from the 256 MB MALL (as tools/ensemble_time.py); `mean`: their mean instead, for calls that differ from one to the next"""
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
    return sum(ts) / len(ts) if mean else sorted(ts)[len(ts) // 2]


def units(q):
    """reads + writes of one channel, in units of V * 4 bytes, for a parameter dict (csrc/intensity.hip, 'Passes')"""
    stats = ("contrast" in q) + ("gamma" in q) + bool(q.get("gamma_retain_stats"))
    if set(q) == {"blur_sigma"}:
        return 4
    kept = 1 if stats and ("lowres_zoom" in q or "noise_variance" in q) else 0
    return (4 if "blur_sigma" in q else 0) + 2 + stats + kept


patch = (128, 128, 128)
v = patch[0] * patch[1] * patch[2]
data = torch.randn((4,) + patch, device="cuda")
mb_unit = v * 4 / 1e6


def row(what, fn, mbytes, passes=None, mean=False):
    t0, t1 = timed(fn, False, mean=mean), timed(fn, True, warm=0 if mean else 3, mean=mean)
    print("  %-64s %8.1f us back to back (%5.2f TB/s), %8.1f us after a MALL flush (%5.2f TB/s); %5.0f MB%s"
          % (what, t0 * 1e3, mbytes / t0 / 1e3, t1 * 1e3, mbytes / t1 / 1e3, mbytes, "" if passes is None else " = %d channel reads / writes" % passes))
    return t0, t1


print("patch %s, 4 channels; %d reps; times include the output and workspace allocation of the Python wrapper" % (patch, reps))
stages = (("copy (no stage on any channel)", {}),
          ("blur sigma 0.5 (radius 2)", dict(blur_sigma=0.5)), ("blur sigma 1.0 (radius 4)", dict(blur_sigma=1.0)), ("blur sigma 2.0 (radius 8)", dict(blur_sigma=2.0)),
          ("low-res zoom 0.5", dict(lowres_zoom=0.5)), ("low-res zoom 0.9", dict(lowres_zoom=0.9)),
          ("noise", dict(noise_variance=0.05, noise_seed=1)), ("brightness", dict(brightness=1.1)), ("contrast", dict(contrast=1.2)),
          ("gamma", dict(gamma=0.8)), ("gamma, inverted, retain-stats", dict(gamma=0.8, gamma_invert=True, gamma_retain_stats=True)),
          ("all stages", dict(blur_sigma=0.75, lowres_zoom=0.75, noise_variance=0.05, noise_seed=1, brightness=1.1, contrast=1.2, gamma=0.8, gamma_invert=True,
                              gamma_retain_stats=True)))
results = {}
for what, q in stages:
    params = [dict(q, noise_seed=c + 1) if "noise_seed" in q else dict(q) for c in range(4)]
    n = 4 * units(q)
    results[what] = row("intensity_augment: " + what, lambda: DL.intensity_augment(data, params), n * mb_unit, n)

rng = random.Random(0)
draws = [DL.draw_intensity_params(4, rng) for _ in range(64)]
n_mean = sum(units(q) for d in draws for q in d) / 64.0
busy = sum(1 for d in draws if any(d_c for d_c in d))
state = {"k": 0}


def default_call():
    state["k"] = (state["k"] + 1) % 64
    return DL.intensity_augment(data, draws[state["k"]])


reps_saved, reps = reps, max(reps, 64) // 64 * 64                   # whole cycles through the 64 draws
default = row("intensity_augment: default probabilities, mean of 64 seeded draws (%d with a stage)" % busy, default_call, n_mean * mb_unit, mean=True)
reps = reps_saved

rs = np.random.default_rng(0)
shape = (240, 240, 155)
image = (np.abs(rs.standard_normal((4,) + shape)) * 120 + 40).astype(np.float32)
label = np.zeros(shape, np.float32)
label[80:160, 80:160, 50:110] = 2
label[100:140, 100:140, 65:95] = 1
label[110:130, 110:130, 72:88] = 3
case = DL.DeviceCase(image, label, patch)
base = dict(crop_lo=np.array([40, 40, 10]), scale=np.array([0.9, 1.1, 1.2]), flips=[True, False, True], transpose=True, gain=np.full(4, 1.05), bias=np.full(4, 0.1))
mb_aug = (4 + 3) * v * 4 / 1e6 + (4 * 4 + 1) * v * 1.1 * 0.9 * 1.2 / 1e6      # as tools/elastic_time.py
plain = row("ru_augment_patch alone (the default path)", lambda: DL.augment_patch(case, base), mb_aug)

whole, dflt = results["all stages"][0], default[0]
print("  all stages %.3f ms = %.0f %% of the %.2f ms per-sample training step, %.1fx ru_augment_patch alone; default probabilities %.3f ms = %.1f %% of the step"
      % (whole, 100 * whole / step_ms, step_ms, whole / plain[0], dflt, 100 * dflt / step_ms))
