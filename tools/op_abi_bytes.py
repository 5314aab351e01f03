#!/usr/bin/env python3
"""One SHA-256 per output of the entries of csrc/op_abi.hip on seeded inputs: every entry that takes a workspace at the cases of
tests/op_cases.py (each branch of its carve, the workspace exactly as large as its query says), and the forwarding entries at one small
shape each.  Two builds of the library compute the same bytes if and only if their listings are equal line for line: run it once per
library (RU_LIB_PATH selects another build), each in a process of its own, and compare.  Under RU_LIB_PATH a case whose entry the other build
does not have yet is listed as absent; the lines both listings have must be equal.

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
    try:
        say(name, run())
    except AttributeError as e:                # (an entry point added since that build: _lib.load leaves it out under RU_LIB_PATH)
        if not os.environ.get("RU_LIB_PATH"):
            raise
        print("absent  %s  (%s)" % (name, e), flush=True)

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

# one training step (loss, flat gradient) under the three sets of forward kernels: the smallest configuration of the suite on the NCDHW split-bf16 flow, and the
# shipped one at the smallest batch that reaches the fp16 + MX-fp8, Winograd-z and direct kernels in one step (2 x 64^3: levels 0 / 1 / 2-3)
from brats2019_amd import loss as loss_mod, model as model_mod
from oracle import resunet_oracle as O
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)       # tests/test_hip_unet.py
for cfg_name, cfg, n, size in (("small", SMALL, 1, 32), ("default", O.DEFAULT_CFG, 2, 64)):
    for env_name, env in (("default", {}), ("RU_MX=0", {"RU_MX": "0"}), ("RU_MX=0_RU_WZ=0", {"RU_MX": "0", "RU_WZ": "0"})):
        os.environ.update(env)
        try:
            net = model_mod.UNet(**cfg)
            net.set_precision("bf16x3")
            net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(41, **cfg).items()})
            net.cuda().train()
            out = net([torch.from_numpy(O.make_input(n, size, size, size, seed=41)).cuda()])
            loss = loss_mod.FusedCriterion()(out, [torch.from_numpy(O.make_target(n, size, size, size, seed=41)).cuda()])
            loss.backward()
            say("train_step_%s_%s" % (cfg_name, env_name),
                [loss.detach(), out[0].detach(), torch.cat([q.grad.reshape(-1) for _, q in net.named_parameters() if q.grad is not None])])
        finally:
            for k in env:
                os.environ.pop(k, None)
        del net

if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
