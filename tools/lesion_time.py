#!/usr/bin/env python3
"""Lesion-wise Dice and HD95 (csrc/lesion.hip) on one 240 x 240 x 155 uint8 label case, upload included, beside the region scorer
(`ops.surface_metrics`, what `validate --regions` runs) on the same case in the same run, in alternating rounds:

  realistic : 1 large and 8 small ground-truth lesions; the prediction shifts the large one, misses two small ones and adds three specks;
  noise     : the same ground truth against a prediction of Bernoulli(0.01) label noise (tens of thousands of predicted components).

Per leg: the median over the rounds of the median of `reps` warmed-up calls (HIP events around upload + call), the spread (max - min over
the rounds), and the ratio to the region scorer.  A third leg with `dilation=0` shows what the dilation and the larger components it
makes cost.  Last, the scipy oracle of tests/test_lesion_host.py on the host, once per case, with its counts compared to the device's.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/lesion_time.py 1 1 --no-host`.

usage: lesion_time.py [rounds] [reps] [--no-host]   (writes profiles/lesion_time.txt)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from brats2019_amd import ops

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 5
assert torch.cuda.is_available(), "lesion_time.py measures on the GPU; there is nothing to time without one"
med = lambda v: sorted(v)[len(v) // 2]
shape = (240, 240, 155)
zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
ball = lambda c, r: (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r


def case():
    lab, pre = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for value, r in ((2, 38.0), (1, 24.0), (4, 15.0)):                  # the large lesion; the prediction is shifted by 3 voxels
        lab[ball((120, 118, 80), r)] = value
        pre[ball((123, 118, 80), r)] = value
    rng = np.random.default_rng(0)
    centres = [(40, 50, 30), (40, 190, 40), (200, 60, 120), (190, 190, 100), (60, 120, 130), (180, 120, 20), (30, 30, 120), (210, 210, 30)]
    for i, c in enumerate(centres):                                     # 8 small lesions of radius 3..5; the last two are missed
        r = 3.0 + (i % 3)
        lab[ball(c, r)] = 4 if i % 2 else 1
        if i < 6:
            pre[ball((c[0] + 1, c[1], c[2]), r)] = 4 if i % 2 else 1
    for c in ((15, 200, 70), (225, 20, 75), (120, 15, 140)):            # three specks
        pre[ball(c, 1.5)] = 1
    noise = (rng.random(shape) < 0.01).astype(np.uint8) * rng.integers(1, 5, size=shape).astype(np.uint8)
    noise[noise == 3] = 4
    return lab, pre, noise


lab, pre, noise = case()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return med(ts)


def up(a):
    return torch.from_numpy(a).cuda()[None]


say("one %d x %d x %d uint8 label case, 3 regions, upload of both volumes included; %d alternating rounds x median of %d calls" % (shape + (rounds, reps)))
for what, p in (("realistic", pre), ("noise", noise)):
    legs = {"region scorer (ops.surface_metrics)": lambda p=p: ops.surface_metrics(up(p), up(lab)),
            "lesion-wise (ops.lesion_metrics)": lambda p=p: ops.lesion_metrics(up(p), up(lab)),
            "lesion-wise, dilation 0": lambda p=p: ops.lesion_metrics(up(p), up(lab), dilation=0)}
    summary, counts = ops.lesion_metrics(up(p), up(lab))
    say("%s prediction: LesionDice %s LesionHD95 %s; per region (n_gt, n_kept, n_tp, n_fn, n_fp) %s" % (
        what, np.round(summary[0, :, 0].cpu().numpy(), 4).tolist(), np.round(summary[0, :, 1].cpu().numpy(), 3).tolist(), counts[0, :, :5].cpu().tolist()))
    times = {k: [] for k in legs}
    for _ in range(rounds):                                             # alternate, so that drift of the machine hits every leg alike
        for k, fn in legs.items():
            times[k].append(timed(fn))
    base = med(times["region scorer (ops.surface_metrics)"])
    for k, t in times.items():
        say("  %-38s median %8.2f ms  min %8.2f  max %8.2f  (spread %.2f)  ratio to the region scorer %.2f" % (k, med(t), min(t), max(t), max(t) - min(t), med(t) / base))

if "--no-host" not in sys.argv:
    from test_lesion_host import oracle_lesions
    from test_surface_host import regions
    for what, p in (("realistic", pre), ("noise", noise)):
        t = time.perf_counter()
        res = [oracle_lesions(regions(p)[k], regions(lab)[k]) for k in range(3)]
        dt = time.perf_counter() - t
        got = ops.lesion_metrics(up(p), up(lab))
        same = [tuple(c) for c in got[1][0, :, :5].cpu().tolist()] == [r[1] for r in res]
        say("scipy oracle on the host, %s prediction, 3 regions: %.1f s; counts %s the device's; largest |LesionHD95 difference| %.2e" % (
            what, dt, "equal" if same else "DIFFER FROM", max(abs(got[0][0, k, 1].item() - res[k][0][1]) for k in range(3))))

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lesion_time.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
