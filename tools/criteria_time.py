#!/usr/bin/env python3
"""The criterion-list kernels (csrc/criteria.hip) at 4 x 3 x 128^3: the fused device list [GDL_joint, BCE_Loss(bg_weight=1e-2)], forward
and backward to d(loss)/d(p), against the same formulas as float32 torch ops with autograd; then the moments pass (reads p and g) and
the gradient pass (reads p and g, writes dp) alone, with their effective bandwidth, back to back and after a MALL flush.  HIP events after
`warm` warm-up iterations.  Back to back gives the rate of consecutive calls, which for the fused list is bound by the host's launch work;
after a flush the call's launches queue up behind the flush read, so the events time the GPU work alone.
usage: criteria_time.py [reps] [warm]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from brats2019_amd import loss, ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5


_flush = None


def timed(fn, flushed=False):
    """ms per call: back to back over `reps` calls, or (flushed=True) the median of `reps` calls each timed alone after a 1 GB read
    that evicts p and g from the 256 MB MALL (201 MB of operands would otherwise partly stay there between back-to-back calls); a read,
    not a write, so that no dirty lines are written back during the timed call"""
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


def torch_list(x, y, bg_weight=1e-2):
    n, c = x.shape[:2]
    xp, yg = x.reshape(n, c, -1)[:, 1:], y.reshape(n, c, -1)[:, 1:]
    w = 1.0 / yg.sum(dim=(0, 2))
    gdl = 1.0 - 2.0 * (w * ((xp * yg).sum(dim=(0, 2)) + 1)).sum() / (w * ((xp * xp + yg).sum(dim=(0, 2)) + 1)).sum()
    bce = -torch.mean(y * torch.log(x + 1e-6) + bg_weight * (1.0 - y) * torch.log((1.0 + 1e-6) - x))
    return (gdl + bce) / 2


gen = torch.Generator(device="cuda").manual_seed(0)
shape = (4, 3, 128, 128, 128)
p = torch.sigmoid(2.0 * torch.randn(shape, generator=gen, device="cuda"))
g = (torch.rand(shape, generator=gen, device="cuda") < 0.2).float()
x = p.clone().requires_grad_(True)
fused = loss.fuse_criterion_list([loss.GDL_joint(), loss.BCE_Loss(bg_weight=1e-2)])


def dev():
    out, _vals = fused([x], [g])
    torch.autograd.grad(out, x)


def ref():
    torch.autograd.grad(torch_list(x, g), x)


for flushed in (False, True):
    t_dev, t_ref = timed(dev, flushed), timed(ref, flushed)
    print("[GDL_joint, BCE_Loss] 4 x 3 x 128^3, forward + backward to dp (%s): device %.3f ms, torch autograd %.3f ms (%.1fx)"
          % ("after a MALL flush, median" if flushed else "back to back", t_dev, t_ref, t_ref / t_dev))
m = ops.crit_moments(p, g)
tot = ops.crit_reduce(m)
_vals, coef = ops.crit_eval(tot, m, [("GDL_joint", 0.5, 1.0, 1.0), ("BCE_Loss", 0.5, 1.0, 1e-2)], float(p.numel()), 4)
mb = p.numel() * 4 / 1e6
for flushed in (False, True):
    t_mom = timed(lambda: ops.crit_moments(p, g), flushed)
    t_grad = timed(lambda: ops.crit_grad(p, g, coef), flushed)
    how = "after a MALL flush, median" if flushed else "back to back"
    print("moments pass  (%s): %.1f us  (%.0f MB read, %.2f TB/s)" % (how, t_mom * 1e3, 2 * mb, 2 * mb / t_mom / 1e3))
    print("gradient pass (%s): %.1f us  (%.0f MB read + %.0f MB written, %.2f TB/s)" % (how, t_grad * 1e3, 2 * mb, mb, 3 * mb / t_grad / 1e3))
