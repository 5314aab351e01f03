#!/usr/bin/env python3
"""Hausdorff95.update (classes = 4: 3 channels) at N x 3 x 128^3 blobs (default N = 4) and `validate --regions`' scoring of one
240 x 240 x 155 uint8 label case on the device, against the scipy / numpy oracle on the host for the same masks (surfaces by
binary_erosion, distance_transform_edt both ways, np.percentile).  Device: median of `reps` warmed-up calls, each ended by a
synchronise (host clock), plus HIP events over the back-to-back loop.  Host: median of `host_reps`.
usage: hd95_time.py [reps] [host_reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage
from brats2019_amd import metrics, ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
STRUCT = ndimage.generate_binary_structure(3, 1)


def blobs(rng, shape, count):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    out = np.zeros((count,) + shape, dtype=bool)
    for m in out:
        for _ in range(4):
            c = [rng.uniform(0, s) for s in shape]
            r = rng.uniform(2.0, 0.2 * min(shape))
            m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return out


def host_hd95(a, b):
    if not (a.any() and b.any()):
        return 0.0
    sa, sb = a & ~ndimage.binary_erosion(a, STRUCT, border_value=0), b & ~ndimage.binary_erosion(b, STRUCT, border_value=0)
    return np.percentile(np.concatenate([ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]]), 95)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return np.median(ts) * 1e3, min(ts) * 1e3, e0.elapsed_time(e1) / reps


def host_time(fn):
    hs = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        fn()
        hs.append(time.perf_counter() - t0)
    return np.median(hs) * 1e3


rng = np.random.default_rng(0)
n, shape = 4, (128, 128, 128)
pm, gm = blobs(rng, shape, n * 3).reshape((n, 3) + shape), blobs(rng, shape, n * 3).reshape((n, 3) + shape)
p, g = torch.from_numpy(pm.astype(np.float32)).cuda(), torch.from_numpy(gm.astype(np.float32)).cuda()
m = metrics.Hausdorff95(classes=4)
med, mn, ev = timed(lambda: m.update([g], [p]))
host = host_time(lambda: [host_hd95(pm[i, k], gm[i, k]) for i in range(n) for k in range(3)])
print("Hausdorff95.update %d x 3 x %s: device median %.3f ms (min %.3f, events %.3f ms/update), scipy host median %.1f ms (%.0fx)"
      % (n, "x".join(map(str, shape)), med, mn, ev, host, host / med))

shape = (240, 240, 155)
wt, tc, et = blobs(rng, shape, 3)
lab = np.zeros(shape, np.uint8)
lab[wt] = 2
lab[wt & tc] = 1
lab[wt & tc & et] = 4
pre = lab.copy()
pre[100:130, 90:140, 60:90] = 3


def score_case():
    gl, pl = torch.from_numpy(lab).cuda(), torch.from_numpy(pre).cuda()       # the upload is part of scoring a case
    return ops.surface_metrics(pl[None], gl[None])


def host_case():
    for sel in ((1, 2, 3, 4), (1, 3, 4), (3, 4)):
        host_hd95(np.isin(pre, sel), np.isin(lab, sel))


med, mn, ev = timed(score_case)
host = host_time(host_case)
print("validate --regions, one 240 x 240 x 155 case (upload + 3 regions): device median %.3f ms (min %.3f, events %.3f ms/case), "
      "scipy host median %.1f ms (%.0fx)" % (med, mn, ev, host, host / med))
