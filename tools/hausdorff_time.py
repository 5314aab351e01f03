#!/usr/bin/env python3
"""Hausdorff_ITK.update (classes = 4: 3 channels) on the device against scipy on the host for the same masks: N x 3 x size^3 blobs
(default 4 x 128^3) and one 3-channel 240 x 240 x 155 case.  Device: median of `reps` warmed-up updates, each ended by a synchronise
(host clock), plus HIP events over the back-to-back loop.  Host: scipy.ndimage.distance_transform_edt per (sample, channel, direction),
as the reference's filter does it, median of `host_reps`.  usage: hausdorff_time.py [reps] [host_reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage
from brats2019_amd import metrics

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2


def blobs(rng, shape, count):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    out = np.zeros((count,) + shape, dtype=bool)
    for m in out:
        for _ in range(4):
            c = [rng.uniform(0, s) for s in shape]
            r = rng.uniform(2.0, 0.2 * min(shape))
            m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return out


def host_update(pm, gm):
    for n in range(pm.shape[0]):
        for i in range(pm.shape[1]):
            a, b = pm[n, i], gm[n, i]
            if a.any() and b.any():
                max(ndimage.distance_transform_edt(~b)[a].max(), ndimage.distance_transform_edt(~a)[b].max())


rng = np.random.default_rng(0)
for n, shape in [(4, (128, 128, 128)), (1, (240, 240, 155))]:
    pm, gm = blobs(rng, shape, n * 3).reshape((n, 3) + shape), blobs(rng, shape, n * 3).reshape((n, 3) + shape)
    p, g = torch.from_numpy(pm.astype(np.float32)).cuda(), torch.from_numpy(gm.astype(np.float32)).cuda()
    m = metrics.Hausdorff_ITK(classes=4)
    for _ in range(3):
        m.update([g], [p])
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.update([g], [p])
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        m.update([g], [p])
    e1.record()
    torch.cuda.synchronize()
    hs = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        host_update(pm, gm)
        hs.append(time.perf_counter() - t0)
    print("Hausdorff_ITK.update %d x 3 x %s: device median %.3f ms (min %.3f, events %.3f ms/update), scipy host median %.1f ms"
          % (n, "x".join(map(str, shape)), np.median(ts) * 1e3, min(ts) * 1e3, e0.elapsed_time(e1) / reps, np.median(hs) * 1e3))
