#!/usr/bin/env python3
"""CarveMix (csrc/carvemix.hip, dataloader.carvemix) at the repository's usual point: a batch of 4 patches of 4 x 128^3, every sample mixed
(K = N = 4), donor targets of nested balls as tools/boundary_time.py builds them.

  reported separately, in microseconds:
    donor augment_batch     dataloader.augment_batch of the 4 donor patches from a resident store of four 144 x 160 x 144 cases (one launch)
    signed_sqdist           ops.signed_sqdist of the 4 WT maps
    ru_carvemix_threshold   the count pass and the threshold launch
    ru_carvemix_mix         the one mix launch, with the bytes it really moves at this carve fraction and its TB/s: 4 B of map per voxel, and per
                            16-byte quad with a selected voxel 7 channels x (16 B donor + 16 B store), + 16 B receiver where the quad is selected in part
    ru_boundary_grad        of the same 4 maps, 8 B / element: the streaming pass the mix is held to
    carvemix                the whole call (WT copy, map, threshold, mix, allocations) as a share of the 14.65 ms training step

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/boundary_time.py).  The legs run in alternating rounds; the spread is max - min over the rounds.  TWO pass/fail conditions, both against
existing code timed in the same run, in both legs:
  (1) the mix pass moves its bytes no slower than ru_boundary_grad moves its own, within the leg's spread:
          t_mix <= r t_grad + (spread_mix + r spread_grad),  r = bytes_mix / bytes_grad
  (2) ru_carvemix_threshold + ru_carvemix_mix together take less than the signed_sqdist call they follow.

usage: carvemix_time.py [rounds] [reps] [--out FILE]     (FILE defaults to profiles/carvemix_time.txt; exit status 1 if a condition is missed)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from brats2019_amd import _lib as L, dataloader as DL, ops

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "carvemix_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
assert torch.cuda.is_available(), "carvemix_time.py measures on the GPU; there is nothing to time without one"
STEP_MS = 14.65

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_flush = None
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)


def timed(fn, flushed=False, warm=2):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read (tools/boundary_time.py)"""
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


# ---------------------------------------------------------------- operands
K = N = 4
CH, P = 4, 128
gen = torch.Generator(device="cuda").manual_seed(0)
ax = torch.arange(P, device="cuda", dtype=torch.float32)
dd, hh, ww = torch.meshgrid(ax, ax, ax, indexing="ij")
donor_target = torch.zeros((K, 3, P, P, P), device="cuda")
for n in range(K):                                         # tools/boundary_time.py's targets: three nested balls, centres seeded
    c = 64 + 16 * (torch.rand(3, generator=gen, device="cuda") - 0.5)
    r = torch.sqrt((dd - c[0]) ** 2 + (hh - c[1]) ** 2 + (ww - c[2]) ** 2)
    for k, radius in enumerate((40.0, 26.0, 14.0)):
        donor_target[n, k] = (r < radius + 2 * n).float()
donor_data = torch.randn((K, CH, P, P, P), generator=gen, device="cuda")
data0 = torch.randn((N, CH, P, P, P), generator=gen, device="cuda")
target0 = (torch.rand((N, 3, P, P, P), generator=gen, device="cuda") > 0.8).float()
u = [0.3, 0.75, 0.5, 0.9]
side = ["outer", "inner", "outer", "inner"]
data, target = data0.clone(), target0.clone()
_, _, mask, thr, vol = DL.carvemix(data, target, donor_data, donor_target, u, side, want_mask=True)
vox = P * P * P
quads = mask.reshape(-1, 4).to(torch.int32).sum(dim=1)
q_any, q_all = int((quads > 0).sum()), int((quads == 4).sum())
bytes_mix = 4 * K * vox + q_any * (CH + 3) * 32 + (q_any - q_all) * (CH + 3) * 16
bytes_grad = 8 * K * vox
say("batch %d of %d x %d^3, %d donors; %d rounds x %d calls; WT foreground %.1f %%, all three target channels %.1f %%"
    % (N, CH, P, K, rounds, reps, 100.0 * float((donor_target[:, 0] > 0.5).float().mean()), 100.0 * float((donor_target > 0.5).float().mean())))
say("u %s, side %s -> V %s, T %s; carved %.1f %% of the voxels, %.1f %% of the quads touched (%.1f %% whole)"
    % (u, side, [int(v) for v in vol], [int(v) for v in thr], 100.0 * float(mask.float().mean()), 100.0 * q_any / (K * vox / 4), 100.0 * q_all / (K * vox / 4)))

# the store of the donor gather: four cases of 144 x 160 x 144, integer intensities (packed as uint16), a labelled ball each
rs = np.random.default_rng(1)
dims = (144, 160, 144)
g3 = np.meshgrid(*[np.arange(v, dtype=np.float32) for v in dims], indexing="ij")
cases = []
for n in range(4):
    image = rs.integers(1, 3000, size=(CH,) + dims).astype(np.float32)
    dist = np.sqrt(sum((a - 0.5 * v) ** 2 for a, v in zip(g3, dims)))
    label = np.zeros(dims, np.uint8)
    label[dist < 40 + 2 * n] = 2
    label[dist < 26] = 1
    label[dist < 14] = 4
    cases.append((image, label))
store = DL.ResidentCases(cases, (P, P, P))
del cases
np.random.seed(2)
import random
random.seed(2)
params = [DL.draw_augment_params(store[n].bbox, (P, P, P), CH) for n in range(4)]
for q in params:
    q["transpose"] = False

# the two entry points alone, on preallocated operands
lib = L.load()
wt = donor_target[:, 0].contiguous()
s_map = ops.signed_sqdist(wt)
ws = L.workspace(lib.ru_carvemix_workspace_bytes(K, vox), wt.device)
t_out = torch.empty(K, dtype=torch.int32, device="cuda")
v_out = torch.empty(K, dtype=torch.int64, device="cuda")
u_arr = (C.c_double * K)(*u)
side_arr = (C.c_int * K)(*[L.CARVE_SIDES[v] for v in side])
dst_arr = (C.c_int * K)(*range(K))


def run_threshold():
    L.check(lib.ru_carvemix_threshold(L.f32(wt), K, vox, u_arr, side_arr, L.ptr(t_out), L.ptr(v_out), L.ptr(ws), ws.numel(), L.stream()), "ru_carvemix_threshold")


def run_mix():                                             # in place: from the second call on the same words are moved again
    L.check(lib.ru_carvemix_mix(L.f32(donor_data), L.f32(donor_target), L.ptr(s_map), L.ptr(t_out), K, dst_arr, N, CH, P, P, P, L.f32(data), L.f32(target),
                                None, L.stream()), "ru_carvemix_mix")


run_threshold()
assert torch.equal(t_out, thr) and torch.equal(v_out, vol)
legs = [("donor augment_batch", lambda: DL.augment_batch(store, [0, 1, 2, 3], params)),
        ("signed_sqdist (4 WT maps)", lambda: ops.signed_sqdist(wt)),
        ("ru_carvemix_threshold", run_threshold),
        ("ru_carvemix_mix", run_mix),
        ("ru_boundary_grad (4 maps)", lambda: ops.boundary_grad(s_map, 1.0 / (K * vox))),
        ("carvemix, the whole call", lambda: DL.carvemix(data, target, donor_data, donor_target, u, side))]
missed = []
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- %s" % how)
    ts = [[] for _ in legs]
    for _ in range(rounds):                                # alternate, so that drift of the machine hits every leg alike
        for j, (_what, fn) in enumerate(legs):
            ts[j].append(timed(fn, flushed))
    m = [med(v) for v in ts]
    sp = [spread(v) for v in ts]
    for j, (what, _fn) in enumerate(legs):
        text = "%-28s %8.1f us  (spread %.1f us)" % (what, m[j] * 1e3, sp[j] * 1e3)
        if what == "ru_carvemix_mix":
            text += "   %6.1f MB  %5.2f TB/s" % (bytes_mix / 1e6, bytes_mix / 1e6 / m[j] / 1e3)
        if what.startswith("ru_boundary_grad"):
            text += "   %6.1f MB  %5.2f TB/s" % (bytes_grad / 1e6, bytes_grad / 1e6 / m[j] / 1e3)
        if what.startswith("carvemix"):
            text += "   %.4f of the %.2f ms step" % (m[j] / STEP_MS, STEP_MS)
        say(text)
    ratio = bytes_mix / bytes_grad
    allowed = ratio * m[4] + (sp[3] + ratio * sp[4])
    ok1 = m[3] <= allowed
    say("(1) mix %.1f us against %.2f x boundary_grad + spreads = %.1f us -> %s" % (m[3] * 1e3, ratio, allowed * 1e3, "met" if ok1 else "MISSED"))
    ok2 = m[2] + m[3] < m[1]
    say("(2) threshold + mix %.1f us against signed_sqdist %.1f us -> %s" % ((m[2] + m[3]) * 1e3, m[1] * 1e3, "met" if ok2 else "MISSED"))
    if not ok1:
        missed.append("(1) %s" % how)
    if not ok2:
        missed.append("(2) %s" % how)
say("conditions: %s" % ("MET" if not missed else "MISSED: " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
