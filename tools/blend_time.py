#!/usr/bin/env python3
"""Blended sliding window (csrc/blend.hip) at a whole BraTS case: 240 x 240 x 155, padded to 240 x 240 x 160, one volume, three output
channels, tile 128^3, overlap 0.5 -> starts [0,64,112] x [0,64,112] x [0,32] = 18 tiles.

  1. ru_blend_accumulate (all 18 tiles in one launch, and in the launches of 8 + 8 + 2 tiles `predict_blended` makes at batch_tiles = 8) and
     ru_blend_finalize on random tile predictions, beside ru_tile_scatter in the 18-tile centre-paste geometry of `Trainer.predict_tiled`
     (centre 96, border 16) on the same volume: HIP events, back to back and as the median of calls timed alone after a MALL flush, with
     the bytes each must move (counted from the geometry) and the rate that gives;
  2. the whole call, full configuration, in two groups of alternating rounds with each leg's spread: on a resident volume the gather +
     forward loop alone (no paste of any kind), that loop with the centre paste (the body of `Trainer.predict_tiled`) and `predict_blended`;
     then `Trainer.predict_tiled` itself, upload and download included, with the centre paste and with blend="gaussian".  Both tilings run 18
     forwards of 128^3.  The blended call may cost the blend passes' stand-alone time on top of the centre-paste leg; the tool says for each
     group whether it stays within that plus the spread, and the forward-only leg shows what either paste adds.

usage: blend_time.py [rounds] [reps] [batch_tiles]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from brats2019_amd import model as M, ops, tiling, train as TR
from oracle import resunet_oracle as O        # configuration and seeded parameters only

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
batch_tiles = int(sys.argv[3]) if len(sys.argv) > 3 else 8
assert torch.cuda.is_available(), "blend_time.py measures on the GPU; there is nothing to time without one"

_flush = None
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, flushed=False, warm=3):
    """ms per call: back to back over `reps` calls, or the median of `reps` calls each timed alone after a 1 GB read that evicts the
    operands from the 256 MB MALL (as tools/ensemble_time.py)"""
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


# ---------------------------------------------------------------- 1. the passes alone
shape, tile, C = (240, 240, 160), (128, 128, 128), 3
starts = [tiling.blend_starts(n, t, 0.5) for n, t in zip(shape, tile)]
assert starts == [[0, 64, 112], [0, 64, 112], [0, 32]]
origins = tiling.blend_origins(starts)
ntiles = len(origins)
profiles = torch.from_numpy(np.concatenate([tiling.blend_profile(t) for t in tile])).cuda()
gen = torch.Generator(device="cuda").manual_seed(0)
preds = torch.rand((ntiles, C) + tile, generator=gen, device="cuda")
acc = torch.empty((1, C) + shape, device="cuda")
vol_mb = C * shape[0] * shape[1] * shape[2] * 4 / 1e6
tile_mb = C * tile[0] * tile[1] * tile[2] * 4 / 1e6


def launches(per):
    return [(t0, min(per, ntiles - t0)) for t0 in range(0, ntiles, per)]


def accumulate_mb(per):
    """bytes the launches of `per` tiles move: every tile voxel inside the volume read once, every voxel a launch touches written once,
    and read first where an earlier launch had reached it"""
    first = np.full(shape, ntiles, np.int32)                      # smallest covering tile index
    for t in range(ntiles - 1, -1, -1):
        z, y, x = origins[t]
        first[z:z + tile[0], y:y + tile[1], x:x + tile[2]] = t
    total = 0.0
    for t0, n in launches(per):
        touched = np.zeros(shape, bool)
        for z, y, x in origins[t0:t0 + n]:
            touched[z:z + tile[0], y:y + tile[1], x:x + tile[2]] = True
            total += tile_mb
        total += C * 4 * (int(touched.sum()) + int((touched & (first < t0)).sum())) / 1e6
    return total


def accumulate(per):
    for t0, n in launches(per):
        ops.blend_accumulate(acc, preds[t0:t0 + n], starts, profiles, t0=t0)


centre, border = (96, 96, 96), (16, 16, 16)
grid = tiling.grid_for(shape, centre)
los = [tiling.get_indices((i, j, k), centre, border)[0] for i in range(grid[0]) for j in range(grid[1]) for k in range(grid[2])]
assert len(los) == ntiles
pasted = torch.zeros((1, C) + shape, device="cuda")
print("volume 1 x %d x %s, tile %s, overlap 0.5, %d tiles; %d reps per figure" % (C, shape, tile, ntiles, reps))
rows = [("ru_blend_accumulate, 18 tiles in one launch", lambda: accumulate(ntiles), accumulate_mb(ntiles)),
        ("ru_blend_accumulate, launches of %d tiles" % batch_tiles, lambda: accumulate(batch_tiles), accumulate_mb(batch_tiles)),
        ("ru_blend_finalize, in place", lambda: ops.blend_finalize(acc, tile, starts, profiles), 2 * vol_mb),
        ("ru_tile_scatter, 18 centre blocks of 96^3", lambda: tiling.copy_back_tiles(pasted, preds, centre, los, border), 2 * vol_mb)]
alone = {}
for what, fn, mb in rows:
    t0, t1 = timed(fn, False), timed(fn, True)
    alone[what] = (t0, t1)
    print("%-48s %8.1f us back to back (%.2f TB/s), %8.1f us after a MALL flush (%.2f TB/s); %.0f MB" % (what, t0 * 1e3, mb / t0 / 1e3, t1 * 1e3, mb / t1 / 1e3, mb))
blend_alone = alone[rows[1][0]][1] + alone[rows[2][0]][1]
scatter_alone = alone[rows[3][0]][1]
print("blend passes of one call (launches of %d + finalize, after a flush): %.1f us; centre paste: %.1f us" % (batch_tiles, blend_alone * 1e3, scatter_alone * 1e3))
accumulate(ntiles)
one = ops.blend_finalize(acc, tile, starts, profiles).clone()
accumulate(batch_tiles)
assert torch.equal(one, ops.blend_finalize(acc, tile, starts, profiles)), "the result depends on the split into launches"
del preds, acc, pasted, one, _flush
_flush = None
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. the whole call
cfg = O.DEFAULT_CFG
net = M.UNet(**cfg)
net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(100, **cfg).items()})
net.cuda().eval()
tr = TR.Trainer(name="blend_time", models_root=tempfile.mkdtemp(), model=net, rewrite=True, connect_tb=False)
gcpu = torch.Generator(device="cpu").manual_seed(99)
vol = torch.randn((1, 4) + shape, generator=gcpu)
dev = vol.cuda()
out_shape = (1, C) + shape


def forward_only():
    with torch.no_grad():
        for t0, n in launches(batch_tiles):
            net([tiling.copy_tiles(dev, tile, origins[t0:t0 + n])])[0]


def centre_paste():                                      # the loop of Trainer.predict_tiled on the resident volume
    out = torch.zeros(out_shape, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        for t0, n in launches(batch_tiles):
            tiling.copy_back_tiles(out, net([tiling.copy_tiles(dev, tile, los[t0:t0 + n])])[0], centre, los[t0:t0 + n], border)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def compare(title, legs, paste_leg, blend_leg):
    """alternating rounds, so that drift of the machine hits every leg of a group alike; the groups run apart because a leg that ends in a
    download leaves the device idle, and the leg behind it pays for that"""
    for _ in range(2):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for r in range(rounds):
        for k, fn in legs.items():
            times[k].append(wall(fn))
    print(title)
    for k, t in times.items():
        print("  %-46s: median %.2f ms, min %.2f, max %.2f (spread %.2f)  %s" % (k, med(t), min(t), max(t), max(t) - min(t), " ".join("%.1f" % x for x in t)))
    paste, blend = times[paste_leg], times[blend_leg]
    extra = med(blend) - med(paste)
    spread = max(max(paste) - min(paste), max(blend) - min(blend))
    allowed = blend_alone + spread
    print("  blended - centre paste = %+.2f ms (%+.2f %%); blend passes alone %.2f ms + spread %.2f ms = %.2f ms -> %s"
          % (extra, 100.0 * extra / med(paste), blend_alone, spread, allowed, "within" if extra <= allowed else "EXCEEDS"))
    return times


net.freeze_params(True)                                  # as predict_tiled and predict_case do: weights packed once
print("full configuration, %s, volume 1 x 4 x %s, 18 forwards of %s in batches of %d, %d alternating rounds, host clock around a synchronise"
      % (net._get_engine().precision, shape, tile, batch_tiles, rounds))
resident = compare("volume resident, result left on the device:",
                   {"gather + forward alone": forward_only, "gather + forward + centre paste (96 + 2 x 16)": centre_paste,
                    "predict_blended": lambda: tiling.predict_blended(net, dev, tile, batch_tiles=batch_tiles)},
                   "gather + forward + centre paste (96 + 2 x 16)", "predict_blended")
print("  predict_blended - (gather + forward alone) = %+.2f ms; centre paste - (gather + forward alone) = %+.2f ms"
      % (med(resident["predict_blended"]) - med(resident["gather + forward alone"]),
         med(resident["gather + forward + centre paste (96 + 2 x 16)"]) - med(resident["gather + forward alone"])))
compare("Trainer.predict_tiled, volume uploaded and result downloaded in the call:",
        {"predict_tiled, centre paste (96 + 2 x 16)": lambda: tr.predict_tiled([[vol]], out_shape, tile, centre, border, batch_tiles=batch_tiles),
         'predict_tiled, blend="gaussian"': lambda: tr.predict_tiled([[vol]], out_shape, tile, blend="gaussian", batch_tiles=batch_tiles)},
        "predict_tiled, centre paste (96 + 2 x 16)", 'predict_tiled, blend="gaussian"')
