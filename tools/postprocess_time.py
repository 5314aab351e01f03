#!/usr/bin/env python3
"""Region-wise post-processing (csrc/postprocess.hip) at the 160 x 192 x 160 case of bench.py.

  1. ru_postprocess_regions on resident masks [3, 160, 192, 160] -- volume filtering only, with the confidence rule, and with all three
     regions hole-filled -- beside ru_cc_reject on the label volume composed from the same masks, in the same run: HIP events, back to back
     and as the median of calls timed alone after a MALL flush.  Two predictions, the extremes csrc/cc_unionfind.hpp names: blobs (a few
     large components) and noise (the prediction of a random-init network: one component that fills the volume, and specks).
     ru_cc_reject is ONE 26-connected labelling; the new call is three, plus up to three 6-connected labellings of the background: the
     ratio to ru_cc_reject is the figure to read.
  2. `predict_case_device` on a full-configuration model with and without `postprocess`, in alternating rounds, with each leg's spread.

usage: postprocess_time.py [rounds] [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import inference as I, model as M, ops
from oracle import resunet_oracle as O        # configuration and seeded parameters only

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
assert torch.cuda.is_available(), "postprocess_time.py measures on the GPU; there is nothing to time without one"

_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the
    operands from the 256 MB MALL (as tools/blend_time.py)"""
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


# ---------------------------------------------------------------- 1. the call alone
shape = (160, 192, 160)
gen = torch.Generator(device="cuda").manual_seed(0)
zz, yy, xx = torch.meshgrid(*(torch.arange(n, device="cuda", dtype=torch.float32) for n in shape), indexing="ij")


def ball(c, r):
    return (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r


wt = ball((80, 96, 80), 45) | ball((40, 60, 120), 12) | ball((130, 150, 30), 6)
tc = (ball((80, 96, 80), 28) & ~ball((80, 96, 80), 10)) | ball((40, 60, 120), 5)          # a shell: one enclosed hole
et = ball((70, 90, 75), 12) | ball((100, 110, 95), 3)
blobs = torch.stack([wt, tc, et]).to(torch.uint8).contiguous()
noise = (torch.rand((3,) + shape, generator=gen, device="cuda") > 0.5).to(torch.uint8).contiguous()
probs = torch.rand((3,) + shape, generator=gen, device="cuda")
del zz, yy, xx
lib_cc = lambda labels: ops.cc_reject(labels, 0.1)

print("masks 3 x %s = %.1f M voxels per region; %d reps per figure" % (shape, shape[0] * shape[1] * shape[2] / 1e6, reps))
for name, masks in (("blobs", blobs), ("noise", noise)):
    counts = masks.reshape(3, -1).sum(dim=1, dtype=torch.int64)
    labels = ops.compose_labels(masks, counts, et_min=32)
    scratch = labels.clone()

    def reject():
        scratch.copy_(labels)                                   # ru_cc_reject works in place: every call gets the same input (the copy is 5 MB)
        lib_cc(scratch)

    rows = [("ru_cc_reject (one labelling) + 5 MB copy", reject),
            ("ru_postprocess_regions, min_volume", lambda: ops.postprocess_regions(masks, min_volume=(50, 20, 10))),
            ("ru_postprocess_regions, + min_confidence", lambda: ops.postprocess_regions(masks, probs=probs, min_volume=(50, 20, 10), min_confidence=0.5)),
            ("ru_postprocess_regions, + fill_holes x 3", lambda: ops.postprocess_regions(masks, min_volume=(50, 20, 10), fill_holes=True)),
            ("ru_postprocess_regions, everything", lambda: ops.postprocess_regions(masks, probs=probs, min_volume=(50, 20, 10), min_confidence=0.5,
                                                                                   keep_largest=(True, False, False), fill_holes=True, nest=True))]
    base = None
    for what, fn in rows:
        t0, t1 = timed(fn, False), timed(fn, True)
        base = base or (t0, t1)
        print("%-6s %-44s %9.1f us back to back (x %.2f of ru_cc_reject), %9.1f us after a MALL flush (x %.2f)"
              % (name, what, t0 * 1e3, t0 / base[0], t1 * 1e3, t1 / base[1]))
    stats = ops.postprocess_regions(masks, probs=probs, min_volume=(50, 20, 10), min_confidence=0.5, fill_holes=True, want_stats=True)[2]
    print("%-6s statistics (found, by volume, by confidence, by largest, filled) per region: %s" % (name, stats.tolist()))
del blobs, noise, probs, _flush
_flush = None
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. the whole case
cfg = O.DEFAULT_CFG
net = M.UNet(**cfg)
net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(100, **cfg).items()})
net.cuda().eval()
net.freeze_params(True)
gcpu = torch.Generator(device="cpu").manual_seed(99)
img = torch.zeros((4, 176, 208, 176))
img[:, 8:168, 8:200, 8:168] = torch.rand((4,) + shape, generator=gcpu) + 0.05       # the crop box is the 160 x 192 x 160 case
img = img.cuda()
post = I.PostProcess(min_volume=(50, 20, 10), min_confidence=(0.0, 0.5, 0.5), fill_holes=True, nest=True)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


legs = {"predict_case_device": lambda: I.predict_case_device(net, img),
        "predict_case_device, postprocess=PostProcess()": lambda: I.predict_case_device(net, img, postprocess=I.PostProcess()),
        "predict_case_device, volume + confidence + holes + nest": lambda: I.predict_case_device(net, img, postprocess=post)}
for _ in range(2):
    for fn in legs.values():
        fn()
times = {k: [] for k in legs}
for r in range(rounds):
    for k, fn in legs.items():
        times[k].append(wall(fn))
print("full configuration, %s, case 4 x %s, %d alternating rounds, host clock around a synchronise" % (net._get_engine().precision, tuple(img.shape[1:]), rounds))
ref = med(times["predict_case_device"])
for k, t in times.items():
    print("  %-58s: median %.2f ms (%+.2f ms, %+.2f %%), min %.2f, max %.2f (spread %.2f)" % (k, med(t), med(t) - ref, 100.0 * (med(t) - ref) / ref, min(t), max(t), max(t) - min(t)))
