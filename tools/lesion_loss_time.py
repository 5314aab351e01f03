#!/usr/bin/env python3
"""The lesion-wise Dice loss (csrc/lesion_loss.hip) at 4 x 3 x 128^3 = 25,165,824 elements.

  targets: tools/boundary_time.py's nested balls plus 40 small satellite blobs per channel; predictions: the target moved by a few voxels
  through a sigmoid with noise.
  forward, pass by pass -- ru_lesion_loss_forward_upto stops after a given pass, and the differences are reported:
    pack + dilate     clears, G as bit rows, 3 dilation launches              reads g, writes 16 B + 4 B of state per voxel (the clears)
    label             cc_label<26> from the plane of Z into the labels          init, compress, merge, compress over 4 B / voxel
    sum               one pass over p, g and the labels                         12 B / voxel read, integer atomics per run
    evaluate          the roots' Dice and coefficients, the pair and batch sums 4 B / voxel read (the volume slots)
  gradient            ru_lesion_loss_grad                                       reads p g labels, writes dp: 16 B / voxel
  forward + backward to d(loss)/d(p) through LesionWiseDiceLoss, against the 14.65 ms training step.
  for comparison in the same run: ops.lesion_metrics on (target, target) as a whole (its labelling share cannot be isolated: one C call
  with a host synchronisation in it), ru_boundary_sum / ru_boundary_grad, and the same loss as float32 torch ops (index_add over the
  lesion slots) on labels made by scipy on the host in every call -- what a user has without this class, since precomputed labels do not
  survive augmentation.

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/boundary_time.py).  ONE pass/fail condition: forward + backward takes less time than the scipy + torch-op form in the same run, in
both legs (that form is timed with the wall clock: it runs for seconds).  Without scipy the condition is reported as not evaluated.

usage: lesion_loss_time.py [rounds] [reps] [--out FILE]     (FILE defaults to profiles/lesion_loss_time.txt; exit status 1 if the condition is missed)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from brats2019_amd import _lib as L, loss, ops

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "lesion_loss_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
assert torch.cuda.is_available(), "lesion_loss_time.py measures on the GPU; there is nothing to time without one"
STEP_MS = 14.65
DILATION = 3

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=2):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read (tools/hardcrit_time.py)"""
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# targets: per sample three nested balls (the BraTS regions are nested) and, per channel, 40 satellite balls of radius 1..3 at seeded
# centres; predictions: the target moved by a few voxels, through a sigmoid with noise
gen = torch.Generator(device="cuda").manual_seed(0)
shape = (4, 3, 128, 128, 128)
ax = torch.arange(128, device="cuda", dtype=torch.float32)
dd, hh, ww = torch.meshgrid(ax, ax, ax, indexing="ij")
g = torch.zeros(shape, device="cuda")
for n in range(4):
    c = 64 + 16 * (torch.rand(3, generator=gen, device="cuda") - 0.5)
    r = torch.sqrt((dd - c[0]) ** 2 + (hh - c[1]) ** 2 + (ww - c[2]) ** 2)
    for k, radius in enumerate((40.0, 26.0, 14.0)):
        m = r < radius + 2 * n
        for _ in range(40):
            sc = 4 + 120 * torch.rand(3, generator=gen, device="cuda")
            sr = 1 + 2 * torch.rand(1, generator=gen, device="cuda")
            m = m | ((dd - sc[0]) ** 2 + (hh - sc[1]) ** 2 + (ww - sc[2]) ** 2 < sr * sr)
        g[n, k] = m.float()
p = torch.sigmoid(4.0 * (torch.roll(g, (3, 2, 4), dims=(2, 3, 4)) - 0.5) + 1.5 * torch.randn(shape, generator=gen, device="cuda"))
x = p.clone().requires_grad_(True)
n = p.numel()
N, C, D, H, W = shape
totals, stats, labels, state = ops.lesion_loss_forward(p, g, DILATION, 0)
say("%d elements (4 x 3 x 128^3); %d rounds x %d calls; target foreground %.1f %%; lesions per (sample, channel) at dilation %d: %s"
    % (n, rounds, reps, 100.0 * float((g > 0.5).float().mean()), DILATION, stats[..., 0].cpu().numpy().reshape(-1).tolist()))

# ---------------------------------------------------------------- forward, pass by pass, and the gradient
lib = L.load()
ws = L.workspace(lib.ru_lesion_loss_workspace_bytes(N, C, D, H, W), p.device)


def forward_upto(k):
    L.check(lib.ru_lesion_loss_forward_upto(L.f32(p), L.f32(g), N, C, D, H, W, DILATION, 0, L.ptr(labels), L.ptr(state), L.ptr(totals), L.ptr(stats),
                                            L.ptr(ws), ws.numel(), k, L.stream()), "ru_lesion_loss_forward_upto")


s_g = ops.signed_sqdist(g)
names = ("pack + dilate", "label", "sum", "evaluate")
fwd_ms = {}
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- forward pass by pass (differences of calls that stop after a pass), gradient, and the boundary loss's passes, %s" % how)
    t = [[timed(lambda k=k: forward_upto(k), flushed) for k in (1, 2, 3, 4)] for _ in range(rounds)]
    cum = [med([row[k] for row in t]) for k in range(4)]
    for k in range(4):
        say("%-22s %8.1f us   (forward up to here %8.1f us, spread %.1f us)"
            % (names[k], (cum[k] - (cum[k - 1] if k else 0.0)) * 1e3, cum[k] * 1e3, (max(row[k] for row in t) - min(row[k] for row in t)) * 1e3))
    fwd_ms[flushed] = cum[3]
    forward_upto(4)
    for what, fn, bpe in (("gradient", lambda: ops.lesion_loss_grad(p, g, labels, state, totals, 1.0), 16),
                          ("ru_boundary_sum", lambda: ops.boundary_sum(p, s_g), 8), ("ru_boundary_grad", lambda: ops.boundary_grad(s_g, 1.0 / n), 8)):
        ts = [timed(fn, flushed) for _ in range(rounds)]
        say("%-22s %8.1f us  %5.0f MB  %5.2f TB/s  (spread %.1f us)" % (what, med(ts) * 1e3, n * bpe / 1e6, n * bpe / 1e6 / med(ts) / 1e3, (max(ts) - min(ts)) * 1e3))
ts = [wall(lambda: ops.lesion_metrics(g, g, dilation=DILATION, min_volume=0)) for _ in range(max(2, min(rounds, 3)))]
say("ops.lesion_metrics(target, target), the whole call (labelling, matching, per-lesion HD95, one host sync): %.1f ms wall (spread %.1f); its "
    "labelling share cannot be isolated" % (med(ts), max(ts) - min(ts)))

# ---------------------------------------------------------------- forward + backward, against the step and against scipy + torch ops
try:
    from scipy import ndimage as ndi
except ImportError:
    ndi = None


def torch_lesion_dice(xx, y):
    """the loss as float32 torch ops: scipy labels on the host, one index_add per sum over the lesion slots (0 = background)"""
    yh = y.detach().cpu().numpy()
    pair_losses = []
    for i in range(N):
        for c in range(C):
            lab, roots = loss.lesion_labels_host(yh[i, c], DILATION)
            if not len(roots):
                continue
            slot = torch.from_numpy(np.where(lab < 0, 0, np.searchsorted(roots, lab) + 1).reshape(-1)).cuda()
            pv, gv = xx[i, c].reshape(-1), y[i, c].reshape(-1)
            inter = torch.zeros(len(roots) + 1, device="cuda").index_add(0, slot, pv * gv)
            union = torch.zeros(len(roots) + 1, device="cuda").index_add(0, slot, pv * pv + gv)
            dice = 2 * (inter[0] + inter[1:] + 1e-6) / (union[0] + union[1:] + 2e-6)
            pair_losses.append(1 - dice.mean())
    return sum(pair_losses) / len(pair_losses)


module = loss.LesionWiseDiceLoss(dilation=DILATION)
missed = []
if ndi is not None:
    ts = [wall(lambda: torch.autograd.grad(torch_lesion_dice(x, g), x)) for _ in range(max(2, min(rounds, 3)))]
    ref_ms = (med(ts), max(ts) - min(ts))
    v_ref, v_dev = float(torch_lesion_dice(x, g).detach()), float(module([x], [g]).detach())
    say("scipy labels on the host + torch ops, forward + backward: %9.1f ms wall (%d calls, spread %.1f); value %.6f, device %.6f"
        % (ref_ms[0], len(ts), ref_ms[1], v_ref, v_dev))
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    td = [timed(lambda: torch.autograd.grad(module([x], [g]), x), flushed) for _ in range(rounds)]
    text = "LesionWiseDiceLoss(), forward + backward to dp, %s: %8.3f ms (spread %.3f)   %.3f of the %.2f ms step" % (how, med(td), max(td) - min(td), med(td) / STEP_MS, STEP_MS)
    if ndi is not None:
        ok = med(td) < ref_ms[0]
        if not ok:
            missed.append(how)
        text += "   scipy + torch ops %9.1f ms wall   %.0fx -> %s" % (ref_ms[0], ref_ms[0] / med(td), "met" if ok else "MISSED")
    say(text)
if ndi is None:
    say("condition (forward + backward faster than scipy labels + torch ops in the same run): not evaluated, scipy is not importable")
else:
    say("condition (forward + backward faster than scipy labels + torch ops in the same run): %s" % ("MET" if not missed else "MISSED " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
