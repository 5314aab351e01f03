#!/usr/bin/env python3
"""Dice_ITK + DiceWT update (the label confusion pass, twice: one per metric object) on the device against the same formulas as torch ops
on the GPU (argmax, compares, sums), at N x 3 x 128^3 (default 4) and on one 3-channel 240 x 240 x 155 case: median of `reps` warmed-up
updates by HIP events.  Also the confusion pass alone, and validate's scoring of one full 240 x 240 x 155 case (upload included) against
numpy on the host.  usage: overlap_time.py [reps] [host_reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import metrics, ops, validate

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3


def events(fn, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def torch_update(p, g, acc_itk, acc_wt, nacc):
    a, b = torch.argmax(p, dim=1), torch.argmax(g, dim=1)
    for i in range(1, nacc + 1):
        pi, gi = a == i, b == i
        inter = (pi & gi).sum(dim=(1, 2, 3)).double()
        s = pi.sum(dim=(1, 2, 3)).double() + gi.sum(dim=(1, 2, 3)).double()
        j = inter / (s - inter)
        acc_itk[i - 1] += (2 * j / (1 + j)).mean()
    pw, gw = (a > 0).float(), (b > 0).float()
    acc_wt += (2 * (pw * gw).sum(dim=(1, 2, 3)) / ((pw + gw).sum(dim=(1, 2, 3)) + 1e-6)).mean().double()


rng = np.random.default_rng(0)
for n, shape in [(4, (128, 128, 128)), (1, (240, 240, 155))]:
    lab = rng.integers(0, 4, size=(n,) + shape)
    g = torch.from_numpy(np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3], axis=1).astype(np.float32)).cuda()
    p = torch.from_numpy((rng.integers(0, 9, size=g.shape) / 8.0).astype(np.float32)).cuda()
    itk, wt = metrics.Dice_ITK(classes=4), metrics.DiceWT()

    def dev():
        itk.update([g], [p])
        wt.update([g], [p])
    acc_itk, acc_wt = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    for _ in range(3):
        dev()
        ops.label_confusion(p, g)
        torch_update(p, g, acc_itk, acc_wt, 3)
    torch.cuda.synchronize()
    t_dev = events(dev, reps)
    t_conf = events(lambda: ops.label_confusion(p, g), reps)
    t_torch = events(lambda: torch_update(p, g, acc_itk, acc_wt, 3), reps)
    mb = 2 * p.numel() * 4 / 1e6
    print("%d x 3 x %s: Dice_ITK + DiceWT update %.3f ms (torch ops %.3f ms); one confusion pass %.1f us = %.2f TB/s over %.0f MB"
          % (n, "x".join(map(str, shape)), t_dev, t_torch, t_conf * 1e3, mb / 1e6 / (t_conf * 1e-3), mb))

lab = rng.choice(np.array([0, 1, 2, 4], np.uint8), size=(240, 240, 155), p=[0.9, 0.03, 0.05, 0.02])
pred = np.where(rng.random(lab.shape) < 0.1, rng.choice(np.array([0, 1, 2, 4], np.uint8), size=lab.shape), lab)


def host_score():
    pr, la = pred.copy(), lab.copy()
    pr[pr == 4] = 3
    la[la == 4] = 3
    res = np.zeros(4)
    for i in range(1, 4):
        pp, gg = (pr == i).astype(np.float32), (la == i).astype(np.float32)
        res[i - 1] = 2 * (pp * gg).sum() / (pp + gg).sum()
    pp, gg = (pr > 0).astype(np.float32), (la > 0).astype(np.float32)
    res[3] = 2 * (pp * gg).sum() / (pp + gg).sum()
    return res


for _ in range(3):
    validate.score([("case", lab, pred)])
ts = []
for _ in range(reps):
    t0 = time.perf_counter()
    validate.score([("case", lab, pred)])
    ts.append(time.perf_counter() - t0)
hs = []
for _ in range(host_reps):
    t0 = time.perf_counter()
    host_score()
    hs.append(time.perf_counter() - t0)
print("validate one 240 x 240 x 155 case: device %.2f ms (upload + score + copy back, host clock), numpy host %.1f ms"
      % (np.median(ts) * 1e3, np.median(hs) * 1e3))
