#!/usr/bin/env python3
"""Calibration scoring and the threshold search (csrc/calibration.hip) at 4 x 3 x 128^3 and on one 3 x 240 x 240 x 155 case.

  1. ru_calib_histogram on a uniform and on a saturated input (80 % exact zeros, 13 % tiny, 7 % near or at one; targets to match), at NB = 256
     and 1024, with float32 and with label targets; ru_calib_accumulate, ru_calib_summary, ru_threshold_regions; and beside them, on the
     same tensors in the same run, the two existing passes that read the same two float tensors: ru_label_confusion(RU_CONF_PROB) and
     ru_crit_moments (without the log moments).  Every leg is timed by HIP events back to back and alone after a MALL flush; the legs take
     turns in `rounds` rounds, and a row shows the median over the rounds and the leg's own spread (max - min).
  2. validate.score_calibration for one 240 x 240 x 155 case (upload, passes, copy back; host clock) beside the numpy restatement.

Two conditions, both against code timed in this run, printed as MET / MISSED:
  A. saturated input: the histogram pass <= 1.5 x the label confusion pass + that leg's spread (more means the hot bins serialise);
  B. the saturated input is no slower than the uniform input by more than the spread.

usage: calibration_time.py [rounds] [reps] [host_reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import _lib as L, metrics, ops, validate

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
host_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 1
assert torch.cuda.is_available(), "calibration_time.py measures on the GPU; there is nothing to time without one"

_flush = (torch.ones(1 << 28, dtype=torch.float32, device="cuda"), torch.empty((), dtype=torch.float32, device="cuda"))


def back_to_back(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def flushed(fn):
    """us of one call timed alone after a 1 GB read that evicts the operands from the 256 MB MALL; the median of 5"""
    ts = []
    for _ in range(5):
        torch.sum(_flush[0], dim=0, out=_flush[1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[2]


def saturated(shape, gen):
    u = torch.rand(shape, generator=gen, device="cuda")
    tiny = 2.0 ** -20
    p = torch.where(u < 0.80, torch.zeros_like(u), torch.where(u < 0.93, torch.full_like(u, tiny), torch.where(u < 0.97, torch.full_like(u, 1 - tiny), torch.ones_like(u))))
    g = (p > 0.5).float()
    flip = torch.rand(shape, generator=gen, device="cuda") < 0.01
    return p, torch.where(flip, 1 - g, g)


med = lambda v: sorted(v)[len(v) // 2]
gen = torch.Generator(device="cuda").manual_seed(0)
for n, shape in [(4, (128, 128, 128)), (1, (240, 240, 155))]:
    full = (n, 3) + shape
    pu = torch.rand(full, generator=gen, device="cuda")
    gu = (torch.rand(full, generator=gen, device="cuda") < pu).float()
    ps, gs = saturated(full, gen)
    lab = torch.where(gs[:, 0] > 0.5, torch.where(gs[:, 2] > 0.5, 4, torch.where(gs[:, 1] > 0.5, 1, 2)), 0).to(torch.uint8).contiguous()
    tables = ops.calib_histogram(pu, gu, 256)
    pool = ops.calib_pool(3, 256, "cuda")
    ops.calib_accumulate(*tables[:3], pool)
    legs = [
        ("calib_histogram, uniform, NB 256", lambda: ops.calib_histogram(pu, gu, 256)),
        ("calib_histogram, saturated, NB 256", lambda: ops.calib_histogram(ps, gs, 256)),
        ("calib_histogram, uniform, NB 1024", lambda: ops.calib_histogram(pu, gu, 1024)),
        ("calib_histogram, saturated, NB 1024", lambda: ops.calib_histogram(ps, gs, 1024)),
        ("calib_histogram, saturated, label target, NB 256", lambda: ops.calib_histogram(ps, lab, 256)),
        ("label_confusion (RU_CONF_PROB), uniform", lambda: ops.label_confusion(pu, gu)),
        ("label_confusion (RU_CONF_PROB), saturated", lambda: ops.label_confusion(ps, gs)),
        ("crit_moments without the logs, saturated", lambda: ops.crit_moments(ps, gs, L.CRIT_MASK_ALL & ~L.CRIT_MASK_LOGS)),
        ("threshold_regions, sample 0 (1 read, 1 byte written per voxel)", lambda: ops.threshold_regions(ps[0], (0.25, 0.5, 0.75))),
        ("calib_accumulate, N = %d, with curves" % n, lambda: ops.calib_accumulate(*tables[:3], pool, want_curves=True)),
        ("calib_summary, 16 bins", lambda: ops.calib_summary(*pool[:3], 16)),
    ]
    times = {what: ([], []) for what, _ in legs}
    for what, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for r in range(rounds):                                   # the legs take turns, so that drift of the machine hits all of them alike
        for what, fn in legs:
            times[what][0].append(back_to_back(fn))
            times[what][1].append(flushed(fn))
    mb = 2 * pu.numel() * 4 / 1e6
    print("%d x 3 x %s, %d alternating rounds of %d calls; the times include the output allocations of the ops wrappers; two float32 tensors = %.0f MB" %
          (n, "x".join(map(str, shape)), rounds, reps, mb))
    for what, _ in legs:
        b, f = times[what]
        rate = "  (%.2f / %.2f TB/s over the two tensors)" % (mb / med(b), mb / med(f)) if what.startswith(("calib_histogram, u", "calib_histogram, s", "label_conf", "crit_mom")) and "label target" not in what else ""
        print("  %-66s %8.1f us back to back (spread %6.1f), %8.1f us after a MALL flush (spread %6.1f)%s" % (what, med(b), max(b) - min(b), med(f), max(f) - min(f), rate))
    for col, name in ((0, "back to back"), (1, "after a MALL flush")):
        s, u = times["calib_histogram, saturated, NB 256"][col], times["calib_histogram, uniform, NB 256"][col]
        c = times["label_confusion (RU_CONF_PROB), saturated"][col]
        spread_c, spread = max(c) - min(c), max(max(s) - min(s), max(u) - min(u))
        print("  condition A, %-18s: histogram (saturated) %.1f us vs 1.5 x confusion %.1f us + spread %.1f = %.1f us: ratio %.2f: %s" %
              (name, med(s), med(c), spread_c, 1.5 * med(c) + spread_c, med(s) / med(c), "MET" if med(s) <= 1.5 * med(c) + spread_c else "MISSED"))
        print("  condition B, %-18s: saturated %.1f us vs uniform %.1f us + spread %.1f: %s" %
              (name, med(s), med(u), spread, "MET" if med(s) <= med(u) + spread else "MISSED"))
    del pu, gu, ps, gs, lab, tables, pool, legs
    torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. one case end to end, beside the numpy restatement
rng = np.random.default_rng(1)
label = rng.choice(np.array([0, 1, 2, 4], np.uint8), size=(240, 240, 155), p=[0.9, 0.03, 0.05, 0.02])
truth = np.stack([np.isin(label, m) for m in metrics.BRATS_REGION_LABELS])
probs = np.clip(np.where(truth, 0.8, 0.02) + rng.normal(0, 0.15, truth.shape), 0, 1).astype(np.float32)
probs[rng.random(probs.shape) < 0.8] = 0
case = [("case", label, probs)]
for _ in range(2):
    res = validate.score_calibration(case)
ts = []
for _ in range(max(rounds, 3)):
    t0 = time.perf_counter()
    res = validate.score_calibration(case)
    ts.append((time.perf_counter() - t0) * 1e3)
hs = []
for _ in range(host_reps):
    t0 = time.perf_counter()
    ref = validate.score_calibration(case, host=True)
    hs.append((time.perf_counter() - t0) * 1e3)
same = np.array_equal(res["best_bin"], ref["best_bin"]) and np.allclose(res["summary"], ref["summary"], rtol=1e-12, atol=0)
print("score_calibration, one 3 x 240 x 240 x 155 case, NB 256: device %.2f ms (upload + passes + one copy back, host clock; spread %.2f), numpy restatement %.0f ms; same thresholds and summary: %s"
      % (med(ts), max(ts) - min(ts), med(hs), same))
