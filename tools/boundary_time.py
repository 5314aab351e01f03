#!/usr/bin/env python3
"""The boundary and Hausdorff-DT losses (csrc/boundary.hip) at 4 x 3 x 128^3 = 25,165,824 elements.

  map pass, beside ops.hausdorff_sq on the same tensors in the same run -- the same three transform passes with surface-only queries and
  no map written; the ratio is reported without a bar:
    signed_sqdist     ru_signed_sqdist of the target     W pass (reads g, writes 2 x 4 B), H pass (reads and writes 2 x 4 B), D pass
                                                         (reads 2 x 4 B and g, writes the 4 B map)
    hausdorff_sq      ru_hausdorff_sq of (p, g)          two transforms as well (towards G, towards P), the D pass reduces to a maximum
  passes, beside ru_focal_sum from the same run, in bytes moved and TB/s:
    boundary sum      ru_boundary_sum                    reads p s_G                                        8 B / element
    boundary grad     ru_boundary_grad                   reads s_G, writes dp                               8 B / element
    hddt sum          ru_hddt_sum, alpha 2 and 2.5       reads p g s_P s_G                                 16 B / element
    hddt grad         ru_hddt_grad, alpha 2 and 2.5      reads p g s_P s_G, writes dp                      20 B / element
  losses, forward + backward to d(loss)/d(p), against the 14.65 ms training step, and against the same formulas as float32 torch ops on
  maps made by scipy's distance_transform_edt on the host in every call (which is what a user has without these classes, since
  precomputed maps do not survive augmentation), where scipy is importable.

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/hardcrit_time.py).  Each pair runs in alternating rounds; the spread is max - min over the rounds.  ONE pass/fail condition: each of
the two losses, forward + backward, takes less time than its scipy + torch-op form in the same run, in both legs (the scipy form is timed
with the wall clock, once per round: it runs for seconds).  Without scipy the condition is reported as not evaluated.

usage: boundary_time.py [rounds] [reps] [--out FILE]     (FILE defaults to profiles/boundary_time.txt; exit status 1 if the condition is missed)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from brats2019_amd import loss, ops

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "boundary_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
assert torch.cuda.is_available(), "boundary_time.py measures on the GPU; there is nothing to time without one"
STEP_MS = 14.65

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


# targets: per sample three nested balls (the BraTS regions are nested), centres and radii seeded; predictions: the target moved by a
# few voxels, through a sigmoid with noise, so P = p > 0.5 is a displaced copy with speckle at its rim
gen = torch.Generator(device="cuda").manual_seed(0)
shape = (4, 3, 128, 128, 128)
ax = torch.arange(128, device="cuda", dtype=torch.float32)
dd, hh, ww = torch.meshgrid(ax, ax, ax, indexing="ij")
g = torch.zeros(shape, device="cuda")
for n in range(4):
    c = 64 + 16 * (torch.rand(3, generator=gen, device="cuda") - 0.5)
    r = torch.sqrt((dd - c[0]) ** 2 + (hh - c[1]) ** 2 + (ww - c[2]) ** 2)
    for k, radius in enumerate((40.0, 26.0, 14.0)):
        g[n, k] = (r < radius + 2 * n).float()
p = torch.sigmoid(4.0 * (torch.roll(g, (3, 2, 4), dims=(2, 3, 4)) - 0.5) + 1.5 * torch.randn(shape, generator=gen, device="cuda"))
x = p.clone().requires_grad_(True)
n = p.numel()
s_p, s_g = ops.signed_sqdist(p), ops.signed_sqdist(g)
coef = 1.0 / n
say("%d elements (4 x 3 x 128^3); %d rounds x %d calls; target foreground %.1f %%, prediction foreground %.1f %%; largest |s| %d"
    % (n, rounds, reps, 100.0 * float((g > 0.5).float().mean()), 100.0 * float((p > 0.5).float().mean()), int(s_g.abs().max())))

# ---------------------------------------------------------------- the map pass beside the scorer's transform
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- map pass, %s" % how)
    ta, tb, tc = [], [], []
    for _ in range(rounds):
        ta.append(timed(lambda: ops.hausdorff_sq(p, g), flushed))
        tb.append(timed(lambda: ops.signed_sqdist(g), flushed))
        tc.append(timed(lambda: ops.signed_sqdist(p), flushed))
    say("%-34s %8.1f us  (spread %.1f us)" % ("hausdorff_sq(p, g)", med(ta) * 1e3, (max(ta) - min(ta)) * 1e3))
    say("%-34s %8.1f us  (spread %.1f us)   %.2f of hausdorff_sq" % ("signed_sqdist(g)", med(tb) * 1e3, (max(tb) - min(tb)) * 1e3, med(tb) / med(ta)))
    say("%-34s %8.1f us  (spread %.1f us)   %.2f of hausdorff_sq" % ("signed_sqdist(p), speckled", med(tc) * 1e3, (max(tc) - min(tc)) * 1e3, med(tc) / med(ta)))

# ---------------------------------------------------------------- the streaming passes beside ru_focal_sum
passes = [("boundary sum", lambda: ops.boundary_sum(p, s_g), 8),
          ("boundary grad", lambda: ops.boundary_grad(s_g, coef), 8),
          ("hddt sum, alpha 2", lambda: ops.hddt_sum(p, g, s_p, s_g, 2.0), 16),
          ("hddt sum, alpha 2.5", lambda: ops.hddt_sum(p, g, s_p, s_g, 2.5), 16),
          ("hddt grad, alpha 2", lambda: ops.hddt_grad(p, g, s_p, s_g, 2.0, coef), 20),
          ("hddt grad, alpha 2.5", lambda: ops.hddt_grad(p, g, s_p, s_g, 2.5, coef), 20)]
nb_name, nb_fn, nb_bpe = "ru_focal_sum", lambda: ops.focal_sum(p, g, 2.0, 1.0, 1.0), 8
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- passes, %s" % how)
    for what, fn, bpe in passes:
        ta, tn = [], []
        for _ in range(rounds):                            # alternate, so that drift of the machine hits both alike
            ta.append(timed(nb_fn, flushed))
            tn.append(timed(fn, flushed))
        ma, mn = med(ta), med(tn)
        mb_a, mb_n = n * nb_bpe / 1e6, n * bpe / 1e6
        say("%-22s %7.1f us  %5.0f MB  %5.2f TB/s  (spread %.1f us)   | %-14s %7.1f us  %5.0f MB  %5.2f TB/s  (spread %.1f us)"
            % (what, mn * 1e3, mb_n, mb_n / mn / 1e3, (max(tn) - min(tn)) * 1e3, nb_name, ma * 1e3, mb_a, mb_a / ma / 1e3, (max(ta) - min(ta)) * 1e3))

# ---------------------------------------------------------------- losses, forward + backward, against the step and against scipy + torch ops
try:
    from scipy import ndimage as ndi
except ImportError:
    ndi = None


def scipy_field(t, signed):
    """F (or phi) of every (sample, channel) mask of t by scipy on the host, back on the device as float32"""
    m = (t.detach() > 0.5).cpu().numpy()
    out = np.zeros(m.shape, dtype=np.float32)
    for i in np.ndindex(*m.shape[:2]):
        if m[i].any() and not m[i].all():
            outside, inside = ndi.distance_transform_edt(~m[i]), ndi.distance_transform_edt(m[i])
            out[i] = np.where(m[i], -(inside - 1.0), outside) if signed else outside + inside
    return torch.from_numpy(out).cuda()


def torch_boundary(xx, y):
    return (xx * scipy_field(y, True)).mean()


def torch_hddt(xx, y):
    return ((xx - y) ** 2 * (scipy_field(xx, False) ** 2 + scipy_field(y, False) ** 2)).mean()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


pairs = [("BoundaryLoss()", loss.BoundaryLoss(), torch_boundary), ("HausdorffDTLoss(alpha=2)", loss.HausdorffDTLoss(), torch_hddt)]
missed = []
ref_ms = {}
if ndi is not None:
    for what, _module, ref in pairs:
        ts = [wall(lambda: torch.autograd.grad(ref(x, g), x)) for _ in range(max(2, min(rounds, 3)))]
        ref_ms[what] = (med(ts), max(ts) - min(ts))
        say("%-26s scipy maps on the host + torch ops, forward + backward: %9.1f ms wall (%d calls, spread %.1f)" % (what, med(ts), len(ts), max(ts) - min(ts)))
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- losses, forward + backward to dp, %s" % how)
    for what, module, _ref in pairs:
        td = [timed(lambda: torch.autograd.grad(module([x], [g]), x), flushed) for _ in range(rounds)]
        text = "%-26s device %8.3f ms (spread %.3f)   %.3f of the %.2f ms step" % (what, med(td), max(td) - min(td), med(td) / STEP_MS, STEP_MS)
        if ndi is not None:
            tr, spread = ref_ms[what]
            ok = med(td) < tr
            if not ok:
                missed.append("%s, %s" % (what, how))
            text += "   scipy + torch ops %9.1f ms wall (spread %.1f)   %.0fx -> %s" % (tr, spread, tr / med(td), "met" if ok else "MISSED")
        say(text)
if ndi is None:
    say("condition (each loss, forward + backward, faster than scipy maps + torch ops in the same run): not evaluated, scipy is not importable")
else:
    say("condition (each loss, forward + backward, faster than scipy maps + torch ops in the same run): %s" % ("MET" if not missed else "MISSED by " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
