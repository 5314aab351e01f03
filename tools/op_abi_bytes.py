#!/usr/bin/env python3
"""One SHA-256 per output of the entries of csrc/op_abi.hip on seeded inputs: every entry that takes a workspace at the cases of
tests/op_cases.py (each branch of its carve, the workspace exactly as large as its query says), and the forwarding entries at one small
shape each.  Two builds of the library compute the same bytes if and only if their listings are equal line for line: run it once per
library (RU_LIB_PATH selects another build), each in a process of its own, and compare.

usage: op_abi_bytes.py [--out FILE]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
from brats2019_amd import ops
from op_cases import _rand, cases

lines = []


def say(label, tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        text = "%s  %s[%d]" % (hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest(), label, i)
        print(text, flush=True)
        lines.append(text)


for name, _, run in cases():
    say(name, run())

x = _rand(1, 16, 3, 5, 6, seed=90)
y = _rand(1, 16, 3, 5, 6, seed=91)
p, g = torch.sigmoid(x), (y > 0).float()
say("leaky_relu", [ops.leaky_relu(x), ops.leaky_relu_bwd(x, y)])
say("upsample2x", [ops.upsample2x(x), ops.upsample2x_bwd(_rand(1, 16, 6, 10, 12, seed=92))])
say("sigmoid", [ops.sigmoid(x)])
say("criterion", [ops.criterion_sums(p, g), ops.criterion_grad(p, g, ops.criterion_sums(p, g), p.numel())])
xc = ops.to_c16(x)
say("layout", [xc, ops.from_c16(xc)])
say("upsample2x_c16", [ops.upsample2x_c16(xc, out_slope=0.01), ops.upsample2x_bwd_c16(ops.to_c16(_rand(1, 16, 6, 10, 12, seed=93)))])

if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
