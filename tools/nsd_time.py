#!/usr/bin/env python3
"""ops.surface_distances with T = 8 tolerances (NSD x 8, ASSD, HD next to Dice, sensitivity, specificity, HD95) beside ops.surface_metrics,
timed in the same run, at the repository's two scoring workloads: 4 x 3 x 128^3 float32 blobs (tools/hd95_time.py's) and one
240 x 240 x 155 uint8 label case (3 regions; already on the device); and the float64 scipy form of the same numbers on the host
(metrics.surface_distances_host per pair: two distance_transform_edt, a histogram, the sums).

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/carvemix_time.py).  The two device legs run in alternating rounds; the spread is max - min over the rounds.  Reported, not gated: the
extra of surface_distances over surface_metrics with both spreads -- it is one more launch that rereads the histograms, and no bound
beyond that is derived here.  The ONE pass/fail condition: the device call is faster than the scipy form, in both legs, at both workloads.

usage: nsd_time.py [rounds] [reps] [--out FILE]     (FILE defaults to profiles/nsd_time.txt; exit status 1 if the condition is missed)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from brats2019_amd import metrics, ops

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "nsd_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 10
assert torch.cuda.is_available(), "nsd_time.py measures on the GPU; there is nothing to time without one"
TOL = (0.0, 0.5, 1.0, float(np.sqrt(2.0)), 2.0, 3.0, 5.0, float("inf"))

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_flush = None
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)


def timed(fn, flushed=False, warm=2):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read"""
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


def blobs(rng, shape, count):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    out = np.zeros((count,) + shape, dtype=bool)
    for m in out:
        for _ in range(4):
            c = [rng.uniform(0, s) for s in shape]
            r = rng.uniform(2.0, 0.2 * min(shape))
            m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return out


def regions(lab):
    return np.stack([(lab >= 1) & (lab <= 4), (lab == 1) | (lab == 3) | (lab == 4), (lab == 3) | (lab == 4)])


rng = np.random.default_rng(0)
n, shape = 4, (128, 128, 128)
pm, gm = blobs(rng, shape, n * 3).reshape((n, 3) + shape), blobs(rng, shape, n * 3).reshape((n, 3) + shape)
case_shape = (240, 240, 155)
wt, tc, et = blobs(rng, case_shape, 3)
lab = np.zeros(case_shape, np.uint8)
lab[wt] = 2
lab[wt & tc] = 1
lab[wt & tc & et] = 4
pre = lab.copy()
pre[100:130, 90:140, 60:90] = 3
workloads = [("4 x 3 x 128^3 float32", torch.from_numpy(pm.astype(np.float32)).cuda(), torch.from_numpy(gm.astype(np.float32)).cuda(),
              pm.reshape((-1,) + shape), gm.reshape((-1,) + shape)),
             ("1 x 240 x 240 x 155 uint8 labels, 3 regions", torch.from_numpy(pre)[None].cuda(), torch.from_numpy(lab)[None].cuda(), regions(pre), regions(lab))]

say("surface_distances with T = %d tolerances %s beside surface_metrics; %d rounds x %d calls" % (len(TOL), list(TOL), rounds, reps))
missed = []
for what, p, g, hp, hg in workloads:
    base = ops.surface_metrics(p, g)
    full = ops.surface_distances(p, g, TOL)
    assert torch.equal(base[0], full[0]) and torch.equal(base[1], full[1])
    t0 = time.perf_counter()
    host = np.array([metrics.surface_distances_host(a, b, TOL) for a, b in zip(hp, hg)])
    host_ms = (time.perf_counter() - t0) * 1e3
    dev = full[2].reshape(host.shape).cpu().numpy()
    assert np.array_equal(dev[:, :len(TOL)], host[:, :len(TOL)]) and np.array_equal(dev[:, -1], host[:, -1])
    worst = float(np.max(np.abs(dev[:, len(TOL)] - host[:, len(TOL)]) / np.maximum(host[:, len(TOL)], 1e-300)))
    say("=== %s: NSD and HD equal the host's bitwise; ASSD differs from the host restatement by at most %.3g relative" % (what, worst))
    say("scipy form on the host, one pass over the %d pairs: %.1f ms" % (len(hp), host_ms))
    legs = [("surface_metrics", lambda: ops.surface_metrics(p, g)), ("surface_distances, T = 8", lambda: ops.surface_distances(p, g, TOL))]
    for flushed in (False, True):
        how = "after a MALL flush" if flushed else "back to back"
        ts = [[] for _ in legs]
        for _ in range(rounds):                            # alternate, so that drift of the machine hits both legs alike
            for j, (_name, fn) in enumerate(legs):
                ts[j].append(timed(fn, flushed))
        m, sp = [med(v) for v in ts], [spread(v) for v in ts]
        say("--- %s" % how)
        for j, (name, _fn) in enumerate(legs):
            say("%-28s %9.1f us  (spread %.1f us)" % (name, m[j] * 1e3, sp[j] * 1e3))
        say("extra of surface_distances   %9.1f us  (spreads %.1f and %.1f us): reported, not gated" % ((m[1] - m[0]) * 1e3, sp[0] * 1e3, sp[1] * 1e3))
        ok = m[1] + sp[1] < host_ms
        say("device %.3f ms against the scipy form %.1f ms (%.0fx) -> %s" % (m[1], host_ms, host_ms / m[1], "met" if ok else "MISSED"))
        if not ok:
            missed.append("%s, %s" % (what, how))
say("condition (device faster than the scipy form): %s" % ("MET" if not missed else "MISSED: " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
