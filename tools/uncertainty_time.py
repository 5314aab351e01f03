#!/usr/bin/env python3
"""Uncertainty maps and their score (csrc/uncertainty.hip) at the case tools/ensemble_time.py uses: a 240 x 240 x 155 case whose
150 x 185 x 148 crop pads to 160 x 192 x 160, four test-time flips, the full configuration.

  1. ru_unc_accumulate against ru_ens_accumulate, and ru_unc_accumulate_finalize (std, entropy) against ru_ens_accumulate_finalize, on
     one [4,3,160,192,160] prediction: HIP events, back to back and as the median of calls timed alone after a MALL flush, with the bytes
     each must move and the rate that gives.  Each pair is timed in alternating rounds, so the ratio and the spread of the existing pass
     (max - min over its rounds) come from the same run.  The second-moment pass moves (12 + 3 + 3 + 3 + 3) / (12 + 3 + 3) = 1.33 x the
     bytes of the existing one: the bar for the later-model pass is 1.33 x its time plus that spread;
  2. the histogram pass at 240 x 240 x 155 (five uint8 volumes read once), the score launch and the map paste;
  3. predict_case_ensemble_device with M models with and without uncertainty="std", alternating, each leg with its own spread.

usage: uncertainty_time.py [models] [rounds] [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from brats2019_amd import inference as INF, model as M, ops
from oracle import resunet_oracle as O        # configuration and seeded parameters only

nmodels = int(sys.argv[1]) if len(sys.argv) > 1 else 3
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
assert torch.cuda.is_available(), "uncertainty_time.py measures on the GPU; there is nothing to time without one"

_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the
    operands from the 256 MB MALL (as tools/ensemble_time.py)"""
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
    return med(ts)


def pair(what, base, base_mb, new, new_mb, bar=None):
    """`rounds` alternating rounds of (existing pass, new pass), both ways of timing; prints medians, rates, the ratio and the bar"""
    for flushed in (False, True):
        tb, tn = [], []
        for _ in range(rounds):
            tb.append(timed(base, flushed))
            tn.append(timed(new, flushed))
        mb_, mn = med(tb), med(tn)
        spread = max(tb) - min(tb)
        how = "after a MALL flush" if flushed else "back to back     "
        print("%s, %s: existing %7.1f us (%.2f TB/s, %3.0f MB; spread %.1f us)   new %7.1f us (%.2f TB/s, %3.0f MB; spread %.1f us)   ratio %.3f"
              % (what, how, mb_ * 1e3, base_mb / mb_ / 1e3, base_mb, spread * 1e3, mn * 1e3, new_mb / mn / 1e3, new_mb, (max(tn) - min(tn)) * 1e3, mn / mb_))
        if bar is not None:
            limit = bar * mb_ + spread
            print("    bar: %.2f x existing + its spread = %.1f us -> %s (new %.1f us)" % (bar, limit * 1e3, "met" if mn <= limit else "MISSED", mn * 1e3))


# ---------------------------------------------------------------- 1. the accumulate passes
padded, box = (160, 192, 160), (150, 185, 148)
left = tuple((p - b) // 2 for p, b in zip(padded, box))
gen = torch.Generator(device="cuda").manual_seed(0)
probs = torch.rand((4, 3) + padded, generator=gen, device="cuda")
vb = box[0] * box[1] * box[2]
mb = 3 * vb * 4 / 1e6                                   # one float32 copy of the box, three channels
acc = ops.ens_accumulate(probs, INF.TTA_FLIPS, None, left, box)
acc, acc2 = ops.unc_accumulate(probs, INF.TTA_FLIPS, None, None, left, box)
print("box %s of a padded %s prediction, 3 channels; the times include the output allocation of the ops wrapper; %d rounds x %d calls" % (box, padded, rounds, reps))
pair("accumulate, first model", lambda: ops.ens_accumulate(probs, INF.TTA_FLIPS, None, left, box), 5 * mb,
     lambda: ops.unc_accumulate(probs, INF.TTA_FLIPS, None, None, left, box), 6 * mb)
pair("accumulate, later model", lambda: ops.ens_accumulate(probs, INF.TTA_FLIPS, acc, left, box), 6 * mb,
     lambda: ops.unc_accumulate(probs, INF.TTA_FLIPS, acc, acc2, left, box), 8 * mb, bar=4.0 / 3.0)
pair("last accumulate + finalize, std", lambda: ops.ens_accumulate_finalize(probs, INF.TTA_FLIPS, acc, 3, left, box), 5.25 * mb,
     lambda: ops.unc_accumulate_finalize(probs, INF.TTA_FLIPS, acc, acc2, 3, "std", left, box), 6.5 * mb)
pair("last accumulate + finalize, entropy", lambda: ops.ens_accumulate_finalize(probs, INF.TTA_FLIPS, acc, 3, left, box), 5.25 * mb,
     lambda: ops.unc_accumulate_finalize(probs, INF.TTA_FLIPS, acc, None, 3, "entropy", left, box), 5.5 * mb)
pair("finalize from stored sums, std", lambda: ops.ens_finalize(acc, 3), 1.25 * mb, lambda: ops.unc_finalize(acc, acc2, 3, 4, "std"), 2.5 * mb)

# ---------------------------------------------------------------- 2. histogram, score, paste
full_shape = (240, 240, 155)
lo = tuple((s - b) // 2 for s, b in zip(full_shape, box))
v = full_shape[0] * full_shape[1] * full_shape[2]
zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in full_shape], indexing="ij")


def ball(c, r):
    return (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r


def labels(shift):
    lab = torch.zeros(full_shape, dtype=torch.uint8, device="cuda")
    for value, r in ((2, 50.0), (1, 32.0), (4, 20.0)):
        lab[ball((120 + shift, 118, 80), r)] = value
    return lab


pred, target = labels(0), labels(3)
maps = ops.paste_u8c(ops.unc_accumulate_finalize(probs, INF.TTA_FLIPS, acc, acc2, 3, "std", left, box)[3], full_shape, lo)
realistic = torch.zeros((3,) + full_shape, dtype=torch.uint8, device="cuda")        # a map that is zero away from the tumour's boundary
for r_, (ro, ri) in enumerate(((54.0, 46.0), (36.0, 28.0), (24.0, 16.0))):
    band = ball((120, 118, 80), ro) & ~ball((120, 118, 80), ri)
    realistic[r_][band] = torch.randint(0, 101, (int(band.sum()),), generator=gen, device="cuda", dtype=torch.uint8)
hmb = 5 * v / 1e6
for what, u in (("map zero away from the boundary bands", realistic), ("map non-zero on the whole crop (noise members)", maps)):
    fn = lambda u=u: ops.unc_histogram(pred, target, u)
    t0, t1 = timed(fn, False), timed(fn, True)
    print("histogram 240 x 240 x 155, %-48s %7.1f us back to back (%.2f TB/s), %7.1f us after a MALL flush (%.2f TB/s); %.0f MB"
          % (what, t0 * 1e3, hmb / t0 / 1e3, t1 * 1e3, hmb / t1 / 1e3, hmb))
hist, _ = ops.unc_histogram(pred, target, realistic)
total = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
t0 = timed(lambda: ops.unc_score(hist, (25, 50, 75, 100), acc=total), False)
print("score launch (4 thresholds)                                             %7.1f us back to back" % (t0 * 1e3))
small = ops.unc_accumulate_finalize(probs, INF.TTA_FLIPS, acc, acc2, 3, "std", left, box)[3]
pmb = (3 * vb + 3 * v) / 1e6
t0, t1 = timed(lambda: ops.paste_u8c(small, full_shape, lo), False), timed(lambda: ops.paste_u8c(small, full_shape, lo), True)
print("paste_u8c into 3 x 240 x 240 x 155 (1 read, full write)                 %7.1f us back to back (%.2f TB/s), %7.1f us after a MALL flush (%.2f TB/s); %.0f MB"
      % (t0 * 1e3, pmb / t0 / 1e3, t1 * 1e3, pmb / t1 / 1e3, pmb))
del probs, acc, acc2, maps, realistic, small, zz, yy, xx, _flush
_flush = None
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 3. end to end
cfg = O.DEFAULT_CFG
nets = []
for seed in range(nmodels):
    net = M.UNet(**cfg)
    net.load_state_dict({k: torch.from_numpy(v_) for k, v_ in O.make_params(100 + seed, **cfg).items()})
    nets.append(net.cuda().eval())
gcpu = torch.Generator(device="cpu").manual_seed(99)
img = torch.zeros((4,) + full_shape)
img[:, lo[0]:lo[0] + box[0], lo[1]:lo[1] + box[1], lo[2]:lo[2] + box[2]] = torch.rand((4,) + box, generator=gcpu) * 3.0 + 0.05
img = img.cuda()


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


legs = {"without uncertainty": lambda: INF.predict_case_ensemble_device(nets, img),
        'uncertainty="std"': lambda: INF.predict_case_ensemble_device(nets, img, uncertainty="std"),
        'uncertainty="entropy"': lambda: INF.predict_case_ensemble_device(nets, img, uncertainty="entropy")}
for _ in range(2):
    for fn in legs.values():
        fn()
times = {k: [] for k in legs}
for r in range(rounds):                                  # alternate, so that drift of the machine hits every leg alike
    for k, fn in legs.items():
        times[k].append(wall(fn))
print("%d models, full configuration, case %s -> padded crop %s, 4 flips, %d alternating rounds, host clock around a synchronise" % (nmodels, full_shape, padded, rounds))
for k, t in times.items():
    print("  predict_case_ensemble_device, %-22s: median %.2f ms, min %.2f, max %.2f (spread %.2f)  %s" % (k, med(t), min(t), max(t), max(t) - min(t), " ".join("%.1f" % x for x in t)))
base = med(times["without uncertainty"])
for k in list(legs)[1:]:
    print("  %s - without = %+.2f ms (%+.1f %%)" % (k, med(times[k]) - base, 100.0 * (med(times[k]) - base) / base))
