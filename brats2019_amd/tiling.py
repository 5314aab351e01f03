"""Sliding-window helpers with the semantics of loader_helper.py:34-97 (`get_indices`, `copy`, `copy_back`) as device kernels:
`copy_tiles` cuts T zero-padded tiles straight into the batch tensor of one forward (ru_tile_gather), `copy_back_tiles` pastes their
centre blocks (ru_tile_scatter) -- one launch each per batch of tiles, no host round trips (the reference does .cuda()/.cpu() per tile,
train.py:165-171) and no per-tile slice copies.  `copy` / `copy_back` keep the reference's single-tile signatures on top of them."""
from __future__ import annotations

import math

import torch

from . import ops


def get_indices(position, center_shape, border):
    """loader_helper.py:34-40: the tile is centre block `position` grown by `border` on every side."""
    lo = [p * c - b for p, c, b in zip(position, center_shape, border)]
    hi = [(p + 1) * c + b for p, c, b in zip(position, center_shape, border)]
    return lo, hi


def copy_tiles(data, tile_shape, index_mins):
    """T tiles of `data` [N,C,D,H,W] in one launch -> [T*N, C, *tile_shape] (rows t*N .. t*N+N-1 = tile t, i.e. torch.cat of the
    reference's per-tile `copy` results along the batch axis)."""
    return ops.tile_gather(data, tile_shape, [tuple(int(v) for v in lo) for lo in index_mins])


def copy_back_tiles(data, tiles, center_shape, index_mins, border):
    """paste the centre blocks of T tiles (layout of `copy_tiles`) into `data` in place, clipped at the volume end."""
    return ops.tile_scatter(data, tiles, [tuple(int(v) for v in lo) for lo in index_mins], border, center_shape)


def _device_kernels_apply(data, tile_shape):
    # ru_tile_gather / ru_tile_scatter move float4 pieces of device rows: a host tensor or a tile width that is not a multiple of 4
    # takes the index arithmetic of loader_helper.py:42-97 on torch slices instead (host-side helper use, e.g. a CPU label volume)
    return data.is_cuda and data.dtype == torch.float32 and int(tile_shape[-1]) % 4 == 0


def copy(data, tile_shape, index_min, index_max):
    """loader_helper.py:42-60: zero-padded extract data[:, :, min:max] -> [N,C,*tile_shape]."""
    assert all(int(b) - int(a) == int(t) for a, b, t in zip(index_min, index_max, tile_shape))
    if _device_kernels_apply(data, tile_shape):
        return copy_tiles(data, tile_shape, [index_min])
    # float32 whatever the volume's dtype, as loader_helper.py:43 allocates it (an integer label volume yields float tiles there too)
    out = torch.zeros(tuple(data.shape[:2]) + tuple(int(t) for t in tile_shape), dtype=torch.float32, device=data.device)
    src, dst = [slice(None), slice(None)], [slice(None), slice(None)]
    for a, b, n in zip(index_min, index_max, data.shape[2:]):
        lo, hi = max(int(a), 0), min(int(b), int(n))
        src.append(slice(lo, hi))
        dst.append(slice(lo - int(a), hi - int(a)))
    out[tuple(dst)] = data[tuple(src)]
    return out


def copy_back(data, tile, center_shape, index_min, index_max, border):
    """loader_helper.py:82-97: paste the tile's centre block into `data`, clipped at the volume end."""
    if _device_kernels_apply(data, tile.shape[2:]):
        copy_back_tiles(data, tile.to(data.device), center_shape, [index_min], border)
        return
    src, dst = [slice(None), slice(None)], [slice(None), slice(None)]
    for a, c, b, n in zip(index_min, center_shape, border, data.shape[2:]):
        first = int(a) + int(b)                              # first voxel of the centre block in the volume (negative: clamped, loader_helper.py:86)
        lo, hi = max(first, 0), min(first + int(c), int(n))
        dst.append(slice(lo, max(hi, lo)))
        src.append(slice(int(b) + lo - first, int(b) + lo - first + max(hi - lo, 0)))
    data[tuple(dst)] = tile.to(data.device)[tuple(src)].to(data.dtype)


def grid_for(shape, center_shape):
    """train.py:158: number of centre blocks per axis."""
    return [int(math.ceil(s / c)) for s, c in zip(shape, center_shape)]


def auto_batch_tiles(model, tile_shape, nvol, cap=8):
    """Tiles per forward: as many as fit in a third of the free device memory (the inference arena keeps every activation of a
    forward: ~5.7 GiB per 192^3 tile in bf16x3, 7.6 GiB in f32), at most `cap`; 1 for a callable without the engine."""
    net = model.module if hasattr(model, "module") else model
    if not (torch.cuda.is_available() and hasattr(net, "_get_engine")):
        return 1
    from . import _lib as L
    eng = net._get_engine()
    per = L.load().ru_unet_workspace_bytes(eng.h, int(nvol), int(tile_shape[0]), int(tile_shape[1]), int(tile_shape[2]), 0)
    if per == 0:
        return 1
    free, _total = torch.cuda.mem_get_info()
    return int(max(1, min(cap, (free // 3) // per)))


# ---------------------------------------------------------------------- overlap-and-blend sliding window (csrc/blend.hip)
# Tiles overlap, every predicted voxel is used and weighted by a window that falls off towards the tile's edge, where the network saw
# the least context (the sliding window of nnU-Net / MONAI; the reference pastes centre blocks only).  The arithmetic is fixed --
# INTEGRATION.md, "Blended sliding window" -- and `blend_host` restates it in numpy float32.
BLEND_WINDOWS = ("gaussian", "constant")
BLEND_MAX_OVERLAP = 0.75


def _check_blend(overlap, window, sigma_scale=0.125):
    if not (isinstance(overlap, (int, float)) and 0.0 <= float(overlap) <= BLEND_MAX_OVERLAP):
        raise ValueError("overlap=%r: a fraction in [0, %g]" % (overlap, BLEND_MAX_OVERLAP))
    if window not in BLEND_WINDOWS:
        raise ValueError("window=%r: one of %s" % (window, ", ".join(BLEND_WINDOWS)))
    if not float(sigma_scale) > 0.0:
        raise ValueError("sigma_scale=%r must be positive" % (sigma_scale,))


def blend_starts(n, tile, overlap=0.5):
    """Tile starts along an axis of `n` voxels: 0, step, 2*step, ... (step = tile - int(overlap*tile)) while the tile ends before the
    volume does, then n - tile, so the last tile ends at the volume's end; [0] when one tile holds the axis (it may stick out)."""
    _check_blend(overlap, "constant")
    n, tile = int(n), int(tile)
    if n < 1 or tile < 1:
        raise ValueError("blend_starts: extents must be positive, got n=%d tile=%d" % (n, tile))
    if n <= tile:
        return [0]
    step = tile - int(overlap * tile)
    starts, s = [], 0
    while s + tile < n:
        starts.append(s)
        s += step
    return starts + [n - tile]


def blend_profile(tile, window="gaussian", sigma_scale=0.125):
    """Window profile of one axis, float32 [tile]: exp(-0.5*((i - (tile-1)/2) / (sigma_scale*tile))^2) in float64, rounded; or ones."""
    _check_blend(0.0, window, sigma_scale)
    import numpy as np
    tile = int(tile)
    if window == "constant":
        return np.ones(tile, np.float32)
    i = np.arange(tile, dtype=np.float64)
    return np.exp(-0.5 * np.square((i - (tile - 1) / 2.0) / (float(sigma_scale) * tile))).astype(np.float32)


def blend_origins(starts):
    """The tiles of a call: the Cartesian product of the three start lists, tile index = (iz*ny + iy)*nx + ix."""
    return [(int(z), int(y), int(x)) for z in starts[0] for y in starts[1] for x in starts[2]]


def blend_host(tiles, shape, tile_shape, starts, profiles):
    """numpy float32 restatement of csrc/blend.hip: tiles [(t*N + n), C, td, th, tw] of a volume with the spatial extents shape[-3:]
    -> [N, C, D, H, W].  w = fl32(fl32(gz*gy)*gx); per voxel over its covering tiles in rising tile index S <- S + w*p, Wn <- Wn + w,
    every product and sum rounded to float32; result S / Wn.  What a tile holds outside the volume is dropped."""
    import numpy as np
    tiles = np.asarray(tiles, np.float32)
    d, h, w = (int(v) for v in tuple(shape)[-3:])
    td, th, tw = (int(v) for v in tile_shape)
    origins = blend_origins(starts)
    n = tiles.shape[0] // len(origins)
    if tiles.shape[0] != n * len(origins) or tuple(tiles.shape[2:]) != (td, th, tw):
        raise ValueError("blend_host: tiles %s do not match %d tiles of %s" % (tiles.shape, len(origins), (td, th, tw)))
    gz, gy, gx = (np.asarray(p, np.float32) for p in profiles)
    weight = (gz[:, None, None] * gy[None, :, None]) * gx[None, None, :]            # float32 throughout: two roundings
    total = np.zeros((n, tiles.shape[1], d, h, w), np.float32)
    norm = np.zeros((d, h, w), np.float32)
    for t, (oz, oy, ox) in enumerate(origins):
        ez, ey, ex = min(td, d - oz), min(th, h - oy), min(tw, w - ox)
        wt = weight[:ez, :ey, :ex]
        vol = (slice(oz, oz + ez), slice(oy, oy + ey), slice(ox, ox + ex))
        total[(slice(None), slice(None)) + vol] = total[(slice(None), slice(None)) + vol] + wt * tiles[t * n:(t + 1) * n, :, :ez, :ey, :ex]
        norm[vol] = norm[vol] + wt
    return total / norm


def _check_tile(model, tile_shape):
    tile = tuple(int(v) for v in tile_shape)
    if len(tile) != 3 or any(t <= 0 for t in tile):
        raise ValueError("tile=%r: three positive extents" % (tile_shape,))
    if tile[2] % 4:
        raise ValueError("tile=%r: the tile width must be a multiple of 4 (16-byte rows of the tile kernels)" % (tile,))
    net = model.module if hasattr(model, "module") else model
    depth = getattr(net, "depth", None)
    if isinstance(depth, int) and depth > 1 and any(t % (1 << (depth - 1)) for t in tile):
        raise ValueError("tile=%r: a network of depth %d takes extents divisible by %d" % (tile, depth, 1 << (depth - 1)))
    return tile


def predict_blended(model, x, tile_shape, overlap=0.5, window="gaussian", sigma_scale=0.125, batch_tiles=None):
    """Sliding-window forward of `model` (any callable with the `model([tiles])[0]` convention) over x [N,C,D,H,W] on the device with
    tiles that overlap by `overlap` and are blended with `window` -> [N,C_out,D,H,W] on the device.  Per batch of tiles: `copy_tiles`
    -> forward -> ops.blend_accumulate; then ops.blend_finalize in place.  The result does not depend on `batch_tiles` (None: sized
    from the free device memory, at most 8)."""
    _check_blend(overlap, window, sigma_scale)
    tile = _check_tile(model, tile_shape)
    if not (isinstance(x, torch.Tensor) and x.dim() == 5):
        raise ValueError("predict_blended: x must be an [N,C,D,H,W] tensor")
    if not x.is_cuda:
        raise RuntimeError("predict_blended: expected a ROCm device tensor, got a %s tensor (HIP-only path)" % x.device)
    import numpy as np
    x = x.contiguous().float()
    nvol = int(x.shape[0])
    starts = [blend_starts(n, t, overlap) for n, t in zip(x.shape[2:], tile)]
    origins = blend_origins(starts)
    profiles = torch.from_numpy(np.concatenate([blend_profile(t, window, sigma_scale) for t in tile])).to(x.device)
    per = max(1, int(batch_tiles if batch_tiles is not None else auto_batch_tiles(model, tile, nvol)))
    acc = None
    with torch.no_grad():
        for t0 in range(0, len(origins), per):
            out = model([copy_tiles(x, tile, origins[t0:t0 + per])])[0]
            if acc is None:                                                   # the first touch of a voxel is written: no memset
                acc = torch.empty((nvol, int(out.shape[1])) + tuple(int(v) for v in x.shape[2:]), dtype=torch.float32, device=x.device)
            ops.blend_accumulate(acc, out, starts, profiles, t0=t0)
            del out
    return ops.blend_finalize(acc, tile, starts, profiles)
