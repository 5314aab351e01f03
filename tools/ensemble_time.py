#!/usr/bin/env python3
"""Ensemble inference (csrc/ensemble.hip, inference.predict_case_ensemble_device) at the case bench.py's predict_case leg uses: a 240 x 240 x 155
case whose 150 x 185 x 148 crop pads to 160 x 192 x 160, four test-time flips, the full configuration.

  1. the merge passes alone on a [4,3,160,192,160] prediction: one accumulate pass (first / later model), the fused last accumulate + finalize,
     the separate finalize, the soft-label paste -- HIP events, back to back and as the median of calls timed alone after a MALL flush, with
     the bytes each must move and the rate that gives; beside them the criteria moments pass (tools/criteria_time.py's 4 x 3 x 128^3), the
     project's other pure read pass, as the rate to compare with;
  2. predict_case_ensemble_device with M models against M back-to-back predict_case_device calls of the same models, alternating in one
     process: per-round times, medians and each leg's own spread (max - min over the rounds);
  3. peak device memory with the M models resident (each UNet owns its engine workspace).

usage: ensemble_time.py [models] [rounds] [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from brats2019_amd import inference as INF, model as M, ops
from oracle import resunet_oracle as O        # configuration and seeded parameters only

nmodels = int(sys.argv[1]) if len(sys.argv) > 1 else 3
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
assert torch.cuda.is_available(), "ensemble_time.py measures on the GPU; there is nothing to time without one"

_flush = None


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the
    operands from the 256 MB MALL (as tools/criteria_time.py)"""
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


# ---------------------------------------------------------------- 1. the passes alone
padded, box = (160, 192, 160), (150, 185, 148)
left = tuple((p - b) // 2 for p, b in zip(padded, box))
gen = torch.Generator(device="cuda").manual_seed(0)
probs = torch.rand((4, 3) + padded, generator=gen, device="cuda")
vb = box[0] * box[1] * box[2]
mb = 3 * vb * 4 / 1e6                                   # one float32 copy of the box, three channels
acc = ops.ens_accumulate(probs, INF.TTA_FLIPS, None, left, box)
mean = ops.ens_finalize(acc, 3, want_mean=True)[2]
labels = (torch.rand(box, generator=gen, device="cuda") * 5).to(torch.uint8)
full_shape = (240, 240, 155)
lo = tuple((s - b) // 2 for s, b in zip(full_shape, box))
passes = [
    ("accumulate, first model (4 reads, 1 write)", lambda: ops.ens_accumulate(probs, INF.TTA_FLIPS, None, left, box), 5 * mb),
    ("accumulate, later model (5 reads, 1 write)", lambda: ops.ens_accumulate(probs, INF.TTA_FLIPS, acc, left, box), 6 * mb),
    ("last accumulate + finalize (5 reads, mask)", lambda: ops.ens_accumulate_finalize(probs, INF.TTA_FLIPS, acc, 3, left, box), 5.25 * mb),
    ("last accumulate + finalize + mean (5 reads, mask, 1 write)", lambda: ops.ens_accumulate_finalize(probs, INF.TTA_FLIPS, acc, 3, left, box, want_mean=True), 6.25 * mb),
    ("finalize (1 read, mask)", lambda: ops.ens_finalize(acc, 3), 1.25 * mb),
    ("finalize + mean (1 read, mask, 1 write)", lambda: ops.ens_finalize(acc, 3, want_mean=True), 2.25 * mb),
    ("paste_probs into 3 x 240 x 240 x 155 (1 read, full write)", lambda: ops.paste_probs(mean, full_shape, lo), mb + 3 * 240 * 240 * 155 * 4 / 1e6),
    ("tta_merge_box, one model at once (4 reads, mask) -- the existing pass", lambda: ops.tta_merge_box(probs, INF.TTA_FLIPS, left, box), 4.25 * mb),
    ("tta_merge on the whole padded volume (4 reads, mask)", lambda: ops.tta_merge(probs, INF.TTA_FLIPS), 4.25 * 3 * padded[0] * padded[1] * padded[2] * 4 / 1e6),
    ("paste_labels into 240 x 240 x 155 (1 read, full write)", lambda: ops.paste_labels(labels, full_shape, lo), (vb + 240 * 240 * 155) / 1e6),
]
print("box %s of a padded %s prediction, 3 channels; the times include the output allocation of the ops wrapper" % (box, padded))
for what, fn, mbytes in passes:
    t0, t1 = timed(fn, False), timed(fn, True)
    print("%-72s %7.1f us back to back (%.2f TB/s), %7.1f us after a MALL flush (%.2f TB/s); %.0f MB" % (what, t0 * 1e3, mbytes / t0 / 1e3, t1 * 1e3, mbytes / t1 / 1e3, mbytes))
p = torch.sigmoid(2.0 * torch.randn((4, 3, 128, 128, 128), generator=gen, device="cuda"))
g = (torch.rand(p.shape, generator=gen, device="cuda") < 0.2).float()
mbc = 2 * p.numel() * 4 / 1e6
t0, t1 = timed(lambda: ops.crit_moments(p, g), False), timed(lambda: ops.crit_moments(p, g), True)
print("%-72s %7.1f us back to back (%.2f TB/s), %7.1f us after a MALL flush (%.2f TB/s); %.0f MB" % ("criteria moments pass, 4 x 3 x 128^3 (2 reads) -- the comparison", t0 * 1e3, mbc / t0 / 1e3, t1 * 1e3, mbc / t1 / 1e3, mbc))
del probs, acc, mean, labels, p, g, _flush
_flush = None
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. + 3. end to end
torch.cuda.reset_peak_memory_stats()
free0 = torch.cuda.mem_get_info()[0]
cfg = O.DEFAULT_CFG
nets = []
for seed in range(nmodels):
    net = M.UNet(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(100 + seed, **cfg).items()})
    nets.append(net.cuda().eval())
gcpu = torch.Generator(device="cpu").manual_seed(99)
img = torch.zeros((4,) + full_shape)
img[:, lo[0]:lo[0] + box[0], lo[1]:lo[1] + box[1], lo[2]:lo[2] + box[2]] = torch.rand((4,) + box, generator=gcpu) * 3.0 + 0.05
img = img.cuda()


def leg_ensemble():
    return INF.predict_case_ensemble_device(nets, img)


def leg_separate():
    return [INF.predict_case_device(net, img) for net in nets]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


for _ in range(2):
    leg_separate()
    leg_ensemble()
te, ts = [], []
for r in range(rounds):                                  # alternate, so that drift of the machine hits both legs alike
    ts.append(wall(leg_separate))
    te.append(wall(leg_ensemble))
med = lambda v: sorted(v)[len(v) // 2]
print("%d models, full configuration, case %s -> padded crop %s, 4 flips, %d alternating rounds, host clock around a synchronise" % (nmodels, full_shape, padded, rounds))
print("  %d x predict_case_device      : median %.2f ms, min %.2f, max %.2f (spread %.2f)  %s" % (nmodels, med(ts), min(ts), max(ts), max(ts) - min(ts), " ".join("%.1f" % v for v in ts)))
print("  predict_case_ensemble_device : median %.2f ms, min %.2f, max %.2f (spread %.2f)  %s" % (med(te), min(te), max(te), max(te) - min(te), " ".join("%.1f" % v for v in te)))
print("  ensemble - separate = %+.2f ms (%+.1f %%)" % (med(te) - med(ts), 100.0 * (med(te) - med(ts)) / med(ts)))
soft_t = [wall(lambda: INF.predict_case_ensemble_device(nets, img, want_probs=True)) for _ in range(3)]
print("  with the pasted soft labels  : median %.2f ms" % med(soft_t))
torch.cuda.synchronize()
print("peak device memory with %d models resident: torch allocator %.2f GB allocated / %.2f GB reserved; free memory fell by %.2f GB of %.0f GB"
      % (nmodels, torch.cuda.max_memory_allocated() / 1e9, torch.cuda.max_memory_reserved() / 1e9, (free0 - torch.cuda.mem_get_info()[0]) / 1e9,
         torch.cuda.mem_get_info()[1] / 1e9))
