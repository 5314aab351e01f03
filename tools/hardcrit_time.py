#!/usr/bin/env python3
"""The focal, Tversky and top-k losses (csrc/hardcrit.hip) at 4 x 3 x 128^3 = 25,165,824 elements.

  passes, beside ru_crit_moments (logs on) and ru_crit_grad from the same run, in bytes moved and TB/s:
    focal sum         ru_focal_sum, gamma 2            reads p g                                          8 B / element
    focal grad        ru_focal_grad, gamma 2           reads p g, writes dp                              12 B / element
    topk select       ru_topk_select, k 10             key pass (reads p g, writes keys) + two histogram
                                                       passes + the value pass (read keys) + three scans  24 B / element
    topk select flat  the same on p = 0.5, g = 0       every key equal: all lanes add to one bin at every level
    topk grad         ru_topk_grad                     reads p g keys, writes dp                         16 B / element
    tversky eval      ru_tversky_eval                  one small launch
  losses, forward + backward to d(loss)/d(p), beside the same formulas written as float32 torch ops with autograd (for top-k:
  torch.topk on the per-element BCE), which is what a user has without these classes.

HIP events, back to back and as the median of calls timed alone after a 1 GB read that evicts the operands from the 256 MB MALL (as
tools/criteria_time.py).  Each pair runs in alternating rounds; the spread is max - min over the rounds.  ONE pass/fail condition: each of
the three losses, forward + backward, takes less time than its torch-op form in the same run, in both legs.  The rate of the radix passes
against the plain streaming passes is reported, not gated.

usage: hardcrit_time.py [rounds] [reps] [--out FILE]     (FILE defaults to profiles/hardcrit_time.txt; exit status 1 if the condition is missed)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from brats2019_amd import _lib as L, loss, ops

args = [a for a in sys.argv[1:]]
out_path = os.path.join(ROOT, "profiles", "hardcrit_time.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
rounds = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
assert torch.cuda.is_available(), "hardcrit_time.py measures on the GPU; there is nothing to time without one"

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=2):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read (tools/criteria_time.py)"""
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


gen = torch.Generator(device="cuda").manual_seed(0)
shape = (4, 3, 128, 128, 128)
p = torch.sigmoid(2.5 * torch.randn(shape, generator=gen, device="cuda"))
g = (torch.rand(shape, generator=gen, device="cuda") < 0.3).float()
p_flat, g_flat = torch.full(shape, 0.5, device="cuda"), torch.zeros(shape, device="cuda")
x = p.clone().requires_grad_(True)
n = p.numel()
K = loss._topk_count(n, 10.0)
EPS, ONE_EPS = 1e-6, 1.0 + 1e-6

# ---------------------------------------------------------------- passes
m = ops.crit_moments(p, g)
_vals, coef = ops.crit_eval(ops.crit_reduce(m), m, [("BCE_Loss", 1.0, 1.0, 1.0)], float(n), 4)
_out, state, keys = ops.topk_select(p, g, K)
totals = ops.crit_reduce(m)
passes = [("focal sum", lambda: ops.focal_sum(p, g, 2.0, 1.0, 1.0), 8, "moments"),
          ("focal grad", lambda: ops.focal_grad(p, g, 2.0, 1.0, 1.0, float(n)), 12, "grad"),
          ("topk select (4 passes)", lambda: ops.topk_select(p, g, K), 24, "moments"),
          ("topk select, all keys equal", lambda: ops.topk_select(p_flat, g_flat, K), 24, "moments"),
          ("topk grad", lambda: ops.topk_grad(p, g, keys, state, K), 16, "grad")]
neighbours = {"moments": ("ru_crit_moments (logs)", lambda: ops.crit_moments(p, g), 8), "grad": ("ru_crit_grad (logs)", lambda: ops.crit_grad(p, g, coef), 12)}
say("%d elements (4 x 3 x 128^3), K = %d; %d rounds x %d calls" % (n, K, rounds, reps))
rate = {}
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- passes, %s" % how)
    for what, fn, bpe, beside in passes:
        nb_name, nb_fn, nb_bpe = neighbours[beside]
        ta, tn = [], []
        for _ in range(rounds):                            # alternate, so that drift of the machine hits both alike
            ta.append(timed(nb_fn, flushed))
            tn.append(timed(fn, flushed))
        ma, mn = med(ta), med(tn)
        mb_a, mb_n = n * nb_bpe / 1e6, n * bpe / 1e6
        rate[(what, how)] = mb_n / mn / 1e3
        say("%-28s %7.1f us  %5.0f MB  %5.2f TB/s  (spread %.1f us)   | %-22s %7.1f us  %5.0f MB  %5.2f TB/s  (spread %.1f us)"
            % (what, mn * 1e3, mb_n, mb_n / mn / 1e3, (max(tn) - min(tn)) * 1e3, nb_name, ma * 1e3, mb_a, mb_a / ma / 1e3, (max(ta) - min(ta)) * 1e3))
    t = [timed(lambda: ops.tversky_eval(totals, 4, 3, 0.3, 0.7, 4.0 / 3.0, 1.0, 1.0), flushed) for _ in range(rounds)]
    say("%-28s %7.1f us  (one workgroup; spread %.1f us)" % ("tversky eval", med(t) * 1e3, (max(t) - min(t)) * 1e3))
    say("radix select against the plain passes: %.2f of focal sum's rate (all keys equal: %.2f)"
        % (rate[("topk select (4 passes)", how)] / rate[("focal sum", how)], rate[("topk select, all keys equal", how)] / rate[("focal sum", how)]))


# ---------------------------------------------------------------- losses, forward + backward, against torch ops
def torch_focal(xx, y):
    return -(y * (1.0 - xx) ** 2 * torch.log(xx + EPS) + (1.0 - y) * xx ** 2 * torch.log(ONE_EPS - xx)).mean()


def torch_tversky(xx, y, alpha=0.3, beta=0.7, gamma=4.0 / 3.0):
    tp = (xx * y).sum(dim=(0, 2, 3, 4))
    fp, fn = xx.sum(dim=(0, 2, 3, 4)) - tp, y.sum(dim=(0, 2, 3, 4)) - tp
    return ((1.0 - (tp + 1.0) / (tp + alpha * fp + beta * fn + 1.0)) ** (1.0 / gamma)).mean()


def torch_topk(xx, y):
    l = -(y * torch.log(xx + EPS) + (1.0 - y) * torch.log(ONE_EPS - xx))
    return torch.topk(l.reshape(-1), K, sorted=False).values.mean()


pairs = [("FocalLoss(gamma=2)", loss.FocalLoss(), torch_focal), ("TverskyLoss(gamma=4/3)", loss.TverskyLoss(gamma=4.0 / 3.0), torch_tversky),
         ("TopKLoss(k=10)", loss.TopKLoss(), torch_topk)]
missed = []
for flushed in (False, True):
    how = "after a MALL flush" if flushed else "back to back"
    say("--- losses, forward + backward to dp, %s" % how)
    for what, module, ref in pairs:
        dev_fn = lambda: torch.autograd.grad(module([x], [g]), x)
        ref_fn = lambda: torch.autograd.grad(ref(x, g), x)
        td, tr = [], []
        for _ in range(rounds):
            tr.append(timed(ref_fn, flushed))
            td.append(timed(dev_fn, flushed))
        ok = med(td) < med(tr)
        if not ok:
            missed.append("%s, %s" % (what, how))
        say("%-24s device %8.3f ms (spread %.3f)   torch ops %8.3f ms (spread %.3f)   %.1fx -> %s"
            % (what, med(td), max(td) - min(td), med(tr), max(tr) - min(tr), med(tr) / med(td), "met" if ok else "MISSED"))
say("condition (each loss, forward + backward, faster than its torch-op form in the same run): %s" % ("MET" if not missed else "MISSED by " + "; ".join(missed)))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if not missed else 1)
