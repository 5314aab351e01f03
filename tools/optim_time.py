#!/usr/bin/env python3
"""The streaming passes of the optimisation recipe (csrc/optim.hip) on the network's three live runs -- the 4,509,939 floats of the shipped
configuration that have a gradient -- each timed beside ru_adam_step (amsgrad), the pass they sit next to.

  norm              ru_gradnorm_partial per run + ru_gradnorm_finalize          reads g                          4 B / float
  sgd               ru_sgd_step, Nesterov momentum, no coefficient              reads w g buf, writes w buf     20 B / float
  sgd + coef        the same with the device clipping coefficient               (one more dword per launch)     20 B / float
  adamw             ru_adamw_step, amsgrad, decoupled                           reads w g m v vmax, writes 4    36 B / float
  ema               ru_ema_update                                               reads ema w, writes ema         12 B / float
  scale             ru_scale_by                                                 reads g, writes g                8 B / float
  adam (existing)   ru_adam_step, amsgrad                                       reads w g m v vmax, writes 4    36 B / float

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/uncertainty_time.py).  Each pair runs in alternating rounds, so the existing pass's median and spread (max - min over its rounds)
come from the same run as the new pass's.  ONE pass/fail condition: every new pass's time per byte moved is at most ru_adam_step's time
per byte in the same leg plus that leg's spread -- the new kernels move 16 bytes per lane where the old one moves a dword, they must not be
slower per byte than their neighbour.  Also reported: norm + clipped SGD step as a fraction of the 14.65 ms training step.

usage: optim_time.py [rounds] [reps] [--out FILE]        (FILE defaults to profiles/optim_time.txt; exit status 1 if the condition is missed)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from brats2019_amd import _lib as L
from brats2019_amd.engine import ParamLayout
from oracle import resunet_oracle as O        # configuration only

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "optim_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 7
reps = int(args[1]) if len(args) > 1 else 30
assert torch.cuda.is_available(), "optim_time.py measures on the GPU; there is nothing to time without one"
STEP_MS = 14.65

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read (tools/uncertainty_time.py)"""
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


# ---------------------------------------------------------------- the live runs of the flat parameter buffer
lay = ParamLayout(**O.DEFAULT_CFG)
runs = []                                                 # [offset, numel] of consecutive parameters that have a gradient
for name, (shape, off, dead) in lay.entries.items():
    n = 1
    for s_ in shape:
        n *= int(s_)
    if dead or n == 0:
        continue
    if runs and runs[-1][0] + runs[-1][1] == off:
        runs[-1][1] += n
    else:
        runs.append([off, n])
live = sum(n for _, n in runs)
assert live == 4509939 and len(runs) == 3, (live, runs)
gen = torch.Generator(device="cuda").manual_seed(0)
buf = {k: torch.randn(lay.total, generator=gen, device="cuda") * s for k, s in (("w", 0.1), ("g", 1e-3), ("m", 1e-3), ("buf", 1e-3), ("ema", 0.1))}
buf["v"] = torch.rand(lay.total, generator=gen, device="cuda") * 1e-6
buf["vmax"] = buf["v"].clone()
lib, stream = L.load(), L.stream()
at = lambda k, off: C.c_void_p(buf[k].data_ptr() + 4 * off)
slots = [int(lib.ru_gradnorm_slots(n)) for _, n in runs]
ws = torch.empty(sum(slots), dtype=torch.float64, device="cuda")
norm = torch.empty((), dtype=torch.float64, device="cuda")
coef = torch.empty(1, dtype=torch.float32, device="cuda")
one = torch.ones(1, dtype=torch.float32, device="cuda")


def p_adam():
    for off, n in runs:
        L.check(lib.ru_adam_step(at("w", off), at("g", off), at("m", off), at("v", off), at("vmax", off), n, 2e-5, 0.9, 0.999, 1e-8, 1e-6, 10, stream), "ru_adam_step")


def p_norm():
    first = 0
    for (off, n), k in zip(runs, slots):
        L.check(lib.ru_gradnorm_partial(at("g", off), n, first, L.ptr(ws), ws.numel() * 8, stream), "ru_gradnorm_partial")
        first += k
    L.check(lib.ru_gradnorm_finalize(L.ptr(ws), first, 12.0, L.ptr(norm), L.ptr(coef), stream), "ru_gradnorm_finalize")


def p_sgd(c=None):
    for off, n in runs:
        L.check(lib.ru_sgd_step(at("w", off), at("g", off), at("buf", off), n, 1e-6, 0.99, 0.0, 3e-5, 1, 0, c, stream), "ru_sgd_step")


def p_adamw():
    for off, n in runs:
        L.check(lib.ru_adamw_step(at("w", off), at("g", off), at("m", off), at("v", off), at("vmax", off), n, 2e-5, 0.9, 0.999, 1e-8, 1e-2, 1, 10, None, stream), "ru_adamw_step")


def p_ema():
    for off, n in runs:
        L.check(lib.ru_ema_update(at("ema", off), at("w", off), n, 0.999, stream), "ru_ema_update")


def p_scale():
    for off, n in runs:
        L.check(lib.ru_scale_by(at("g", off), n, L.ptr(one), stream), "ru_scale_by")


def p_clipped_step():
    p_norm()
    p_sgd(L.ptr(coef))


passes = [("norm (3 partial + finalize)", p_norm, 4), ("sgd nesterov", p_sgd, 20), ("sgd nesterov + coefficient", lambda: p_sgd(L.ptr(coef)), 20),
          ("adamw amsgrad", p_adamw, 36), ("ema", p_ema, 12), ("scale_by", p_scale, 8)]
ADAM_B = 36
say("%d live floats in %d runs %s; %d rounds x %d calls; a pass = one launch per run" % (live, len(runs), [n for _, n in runs], rounds, reps))
p_norm()


def p_floor():
    for off, _ in runs:                                     # the same three launches on 4 floats each: what a pass costs before it moves a byte
        L.check(lib.ru_scale_by(at("g", off), 4, L.ptr(one), stream), "ru_scale_by")


missed = []
clip_ms = {}
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- %s" % how)
    for what, fn, bpf in passes:
        ta, tn = [], []
        for _ in range(rounds):                            # alternate, so that drift of the machine hits both alike
            ta.append(timed(p_adam, flushed))
            tn.append(timed(fn, flushed))
        ma, mn, spread = med(ta), med(tn), max(ta) - min(ta)
        mb_a, mb_n = live * ADAM_B / 1e6, live * bpf / 1e6
        limit = (ma + spread) / mb_a                      # ms per MB
        ok = mn / mb_n <= limit
        if not ok:
            missed.append("%s, %s" % (what, how))
        say("%-28s %7.1f us  %5.1f MB  %5.2f TB/s  (spread %.1f us)   | ru_adam_step %7.1f us  %5.1f MB  %5.2f TB/s  (spread %.1f us)   "
            "ns/KB %.3f vs limit %.3f -> %s" % (what, mn * 1e3, mb_n, mb_n / mn / 1e3, (max(tn) - min(tn)) * 1e3, ma * 1e3, mb_a, mb_a / ma / 1e3, spread * 1e3,
                                               mn / mb_n * 1e3, limit * 1e3, "met" if ok else "MISSED"))
    say("launch floor                 %7.1f us  (three launches of 4 floats: included in every pass above, whatever it moves)" % (med([timed(p_floor, flushed) for _ in range(rounds)]) * 1e3))
    t = [timed(p_clipped_step, flushed) for _ in range(rounds)]
    clip_ms[how] = med(t)
    say("norm + clipped sgd step      %7.1f us = %.3f %% of the %.2f ms training step" % (med(t) * 1e3, 100.0 * med(t) / STEP_MS, STEP_MS))
say("condition (every new pass no slower per byte than ru_adam_step in the same leg, plus that leg's spread): %s"
    % ("MET" if not missed else "MISSED by " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
