"""Device-side training input pipeline -- the part of the reference's `dataloader` module that feeds the hot path
(dataloader.py:67-216 `SimpleReader`, :218-286 `FullReader`): per-channel z-score, random crop around the lesion, affine
zoom 0.7-1.3 (scipy affine_transform order 1 / reflect, restated in the kernel), flips, D<->H transpose, intensity gain /
bias and the WT/TC/ET targets.  At > 100 volumes/s per GPU the reference's CPU path (scipy on 4 x 128^3 float64 per patch)
cannot keep 8 GPUs fed; here the raw case lives in HBM and ONE kernel (`ru_augment_patch`) produces a patch.

What stays on the host, on purpose: file IO (nibabel is not part of this path -- cases are handed over as arrays), the
bounding-box cache (dataloader.py:99-116, once per case) and the random draws, which reproduce the reference's order from
the same global generators (`numpy.random`, `random`), so equal seeds give equal patches (tests/test_dataloader.py).

Opt-in: elastic deformation (dataloader.py:24-48 `elastic_transform`, which the reference's reader draws parameters for and then leaves
commented out at :177 / :180 -- about 14 s of scipy per patch).  `SimpleReader(..., elastic=True)` or an `elastic` entry in the parameters
of `augment_patch` adds three more kernels after the zoom pass (csrc/elastic.hip: noise, float64 displacement field, warp); the default path
is the one above, unchanged.  `elastic_*_host` are the numpy restatements (tests/test_elastic_host.py holds them to the reference's outputs).
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import torch

from . import _lib as L


def _bbox3(mask):
    """loader_helper.py:105-129"""
    nz = np.nonzero(mask)
    if nz[0].size == 0:
        return np.array([[-1, -1, -1], [0, 0, 0]])
    return np.array([[a.min() for a in nz], [a.max() for a in nz]])


def label_bbox(label, patch_size):
    """dataloader.py:104-116: where patch centres may fall (lesion box +- 50 voxels, clipped so the patch fits)."""
    bbox = _bbox3(np.asarray(label) > 0).astype(np.float64)
    shape = np.array(np.asarray(label).shape)
    bbox[0] = np.maximum(bbox[0] - 50, np.array(patch_size) / 2.0 + 1)
    bbox[1] = np.minimum(bbox[1] + 50, shape - np.array(patch_size) / 2.0 - 1)
    return bbox


def zscore_stats(image):
    """(mean, std) float64 numpy per channel of a device tensor [C,D,H,W], dataloader.py:124-132: count over x > 0, sums over all."""
    L.require_gpu()
    if not image.is_cuda:
        raise RuntimeError("brats2019_amd.dataloader: expected a ROCm device tensor (HIP-only path)")
    image = image.contiguous().float()
    c = int(image.shape[0])
    v = image.numel() // c
    lib = L.load()
    stats = torch.empty((c, 3), dtype=torch.float64, device=image.device)
    ws = L.workspace(lib.ru_zscore_workspace_bytes(c, v), image.device)
    L.check(lib.ru_zscore_stats(L.f32(image), L.ptr(stats), c, v, L.ptr(ws), ws.numel(), L.stream()), "ru_zscore_stats")
    s = stats.cpu().numpy()
    mean = s[:, 1] / s[:, 0]
    std = np.sqrt(s[:, 2] / s[:, 0] - mean * mean)
    return mean, std


def remap_labels(label):
    """Label contract of the pipeline: {0, 1, 2, 3} with 3 = enhancing tumour.  The reference gets there in its reader
    (loader_helper.read_multimodal: `annotation[annotation == 4] = 3`, loader_helper.py:30) and `np.eye(4)[label]` fails loudly on a raw
    4 if that step is skipped; the device kernel only recognises 1, 2, 3, so raw BraTS labels {0, 1, 2, 4} are remapped HERE (4 -> 3)
    and anything else is refused instead of silently dropping every ET voxel from the WT / TC / ET targets."""
    lab = np.ascontiguousarray(label)
    bad = ~np.isin(lab, (0, 1, 2, 3, 4))
    if bad.any():
        raise ValueError("label volume holds values outside {0,1,2,3,4}: %s" % np.unique(lab[bad])[:8])
    lab = lab.astype(np.uint8)
    lab[lab == 4] = 3
    return lab


class DeviceCase(object):
    """One multimodal case resident in HBM: raw modalities [C,D,H,W] float32, label [D,H,W] uint8 in {0,1,2,3} (raw BraTS 4 is
    remapped to 3, see remap_labels), z-score constants, centre box.  `soft` (optional, keyword): [3,D,H,W] float32 WT/TC/ET
    probabilities of a teacher (`inference.predict_case_ensemble(..., want_probs=True)`) -- the targets of `augment_patch` are then
    interpolated from them instead of from the one-hot label; `label` still places the crops (`label_bbox`)."""

    def __init__(self, image, label, patch_size, device="cuda", soft=None):
        L.require_gpu()
        label = remap_labels(label)
        self.image = torch.as_tensor(np.ascontiguousarray(image, dtype=np.float32)).to(device)
        self.label = torch.as_tensor(label).to(device)
        self.soft = None
        if soft is not None:
            if isinstance(soft, torch.Tensor):
                self.soft = soft.detach().to(device=device, dtype=torch.float32).contiguous()
            else:
                self.soft = torch.as_tensor(np.ascontiguousarray(soft, dtype=np.float32)).to(device)
            if tuple(self.soft.shape) != (3,) + tuple(self.label.shape):
                raise ValueError("soft targets must be [3,D,H,W] = %s, got %s" % ((3,) + tuple(self.label.shape), tuple(self.soft.shape)))
        self.patch_size = tuple(int(p) for p in patch_size)
        self.mean, self.std = zscore_stats(self.image)
        self.bbox = label_bbox(label, self.patch_size)


_ELASTIC_RNG = random.Random()          # seeds of elastic fields when the caller brings no generator (the reference seeds from the wall clock, :166)


def draw_augment_params(bbox, patch_size, channels=4, elastic=False, elastic_rng=None):
    """The draws of SimpleReader.__getitem__ (dataloader.py:141-199), in its order, from the same global generators.  `elastic=True` keeps
    the two values the reference draws for its switched-off elastic transform (:167-168) and adds `elastic=dict(sigma, alpha, seed)`; the seed
    comes from `elastic_rng` (a private `random.Random`), never from the global generators, which advance exactly as with `elastic=False`."""
    center = np.random.rand(3)
    center = center * (bbox[1] - bbox[0]) + bbox[0]
    left_bottom = (center - np.array(patch_size) / 2.0).astype(np.int32)
    r_sigma = random.random()                            # sigma / alpha of the elastic transform (:167-168), drawn whether it runs or not
    r_alpha = random.random()
    scale = [0.7 + random.random() * 0.6 for _ in range(3)]
    flips = [random.random() > 0.5 for _ in range(3)]
    transpose = random.random() > 0.5
    gain = np.random.uniform(0.9, 1.1, size=(channels, 1, 1, 1)).reshape(-1)
    bias = np.random.uniform(-0.2, 0.2, size=(channels, 1, 1, 1)).reshape(-1)
    p = dict(crop_lo=left_bottom, scale=np.array(scale), flips=flips, transpose=transpose, gain=gain, bias=bias)
    if elastic:
        p["elastic"] = dict(sigma=r_sigma * 20 + 10, alpha=r_alpha * 4000 + 200, seed=(elastic_rng or _ELASTIC_RNG).getrandbits(63))
    return p


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _flags(flips, transpose):
    return sum(1 << i for i, f in enumerate(flips) if f) | (8 if transpose else 0)


def augment_patch(case, p, patch_size=None):
    """(data [C,Q0,Q1,P2], target [3,Q0,Q1,P2]) float32 device tensors for explicit parameters `p` (see draw_augment_params).  A case
    with soft targets takes the same pass with the teacher's three channels interpolated in place of the one-hot label
    (`ru_augment_patch_soft`: affine_transform(soft, (1, sx, sy, sz), order=1, mode='reflect'), dataloader.py:179 on float channels).

    With an `elastic` entry in `p` (dict(sigma, alpha, seed), or `noise` [3,P0,P1,P2] float64 in place of `seed`) the patch is deformed as
    the reference's commented lines :177 / :180 would: the zoom pass runs without flips, gain or bias, then `elastic_noise` ->
    `elastic_field` -> `elastic_warp` (order 1 on the image, order 0 on the targets) and the warp applies flips, transpose, gain and bias."""
    patch = tuple(int(v) for v in (patch_size or case.patch_size))
    c, d, h, w = (int(v) for v in case.image.shape)
    el = p.get("elastic")
    noise = None
    if el is not None:                                   # argument checks before any launch
        sigma, alpha = float(el["sigma"]), float(el["alpha"])
        _check_sigma(sigma)
        noise = el.get("noise")
        if noise is not None:
            noise = _noise_tensor(noise, patch, case.image.device)
    direct = el is None                                  # the one-pass path writes the final layout
    flags = _flags(p["flips"], p["transpose"]) if direct else 0
    out_sp = (patch[1], patch[0], patch[2]) if (p["transpose"] and direct) else patch
    data = torch.empty((c,) + out_sp, dtype=torch.float32, device=case.image.device)
    target = torch.empty((3,) + out_sp, dtype=torch.float32, device=case.image.device)
    lib = L.load()
    soft = getattr(case, "soft", None)
    gain = [float(v) for v in p["gain"]] if direct else [1.0] * c
    bias = [float(v) for v in p["bias"]] if direct else [0.0] * c
    tail = (_arr(C.c_float, [float(v) for v in case.mean]), _arr(C.c_float, [float(1.0 / v) for v in case.std]),
            c, d, h, w, _arr(C.c_int, [int(v) for v in p["crop_lo"]]), _arr(C.c_int, list(patch)),
            _arr(C.c_double, [float(v) for v in p["scale"]]), flags,
            _arr(C.c_float, gain), _arr(C.c_float, bias),
            L.f32(data), L.f32(target), L.stream())
    if soft is None:
        L.check(lib.ru_augment_patch(L.f32(case.image), L.ptr(case.label), *tail), "ru_augment_patch")
    else:
        L.check(lib.ru_augment_patch_soft(L.f32(case.image), L.ptr(case.label), L.f32(soft), *tail), "ru_augment_patch_soft")
    if direct:
        return data, target
    if noise is None:
        noise = elastic_noise(int(el["seed"]), patch, case.image.device)
    disp = elastic_field(noise, sigma, alpha)
    return elastic_warp(data, target, disp, p["flips"], p["transpose"], p["gain"], p["bias"])


# ---------------------------------------------------------------------------------------------------------------- elastic deformation
# dataloader.py:24-48 `elastic_transform` on the device (csrc/elastic.hip) and its numpy restatement for hosts without a GPU.
ELASTIC_MAX_RADIUS = 256
_M64 = (1 << 64) - 1
_GOLDEN, _MIX1, _MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def elastic_radius(sigma):
    """scipy.ndimage.gaussian_filter's kernel radius: int(truncate * sigma + 0.5), truncate = 4"""
    return int(4.0 * float(sigma) + 0.5)


def _check_sigma(sigma):
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError("elastic: sigma must be positive and finite, got %r" % (sigma,))
    if elastic_radius(sigma) > ELASTIC_MAX_RADIUS:
        raise ValueError("elastic: radius int(4 sigma + 0.5) = %d exceeds %d" % (elastic_radius(sigma), ELASTIC_MAX_RADIUS))


def _noise_tensor(noise, patch, device):
    """explicit noise [3,P0,P1,P2] (array or tensor) as a contiguous float64 device tensor; the shape is checked before any upload"""
    shape = tuple(int(v) for v in noise.shape)
    if shape != (3,) + tuple(patch):
        raise ValueError("elastic: noise must be [3,P0,P1,P2] = %s, got %s" % ((3,) + tuple(patch), shape))
    if isinstance(noise, torch.Tensor):
        return noise.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(noise, dtype=np.float64)).to(device)


def elastic_noise(seed, patch, device="cuda"):
    """[3,P0,P1,P2] float64 device tensor, uniform in [-1, 1): `ru_elastic_noise`, a pure function of (seed, field, linear voxel index)"""
    L.require_gpu()
    patch = tuple(int(v) for v in patch)
    out = torch.empty((3,) + patch, dtype=torch.float64, device=device)
    L.check(L.load().ru_elastic_noise(int(seed) & _M64, patch[0], patch[1], patch[2], L.ptr(out), L.stream()), "ru_elastic_noise")
    return out


def elastic_field(noise, sigma, alpha, out=None, ws=None):
    """[3,P0,P1,P2] float64 displacements in voxels from float64 noise of the same shape: `ru_elastic_field` = gaussian_filter(noise[f], sigma,
    mode="constant", cval=0) * (alpha, alpha, alpha / 2.5).  `out` / `ws` (optional) are reused instead of allocated."""
    L.require_gpu()
    sigma, alpha = float(sigma), float(alpha)
    _check_sigma(sigma)
    if noise.dtype != torch.float64 or noise.dim() != 4 or int(noise.shape[0]) != 3:
        raise ValueError("elastic: noise must be a float64 [3,P0,P1,P2] tensor, got %s %s" % (noise.dtype, tuple(noise.shape)))
    p0, p1, p2 = (int(v) for v in noise.shape[1:])
    noise = noise.contiguous()
    lib = L.load()
    disp = torch.empty_like(noise) if out is None else out
    if ws is None:
        ws = L.workspace(lib.ru_elastic_workspace_bytes(p0, p1, p2), noise.device)
    L.check(lib.ru_elastic_field(L.ptr(noise), sigma, alpha, p0, p1, p2, L.ptr(disp), L.ptr(ws), ws.numel(), L.stream()), "ru_elastic_field")
    return disp


def elastic_warp(data, target, disp, flips=(False, False, False), transpose=False, gain=None, bias=None, order=(1, 0)):
    """(data [C,Q0,Q1,P2], target [T,Q0,Q1,P2]) float32: `ru_elastic_warp` of data [C,P0,P1,P2] (order 1) and target [T,P0,P1,P2] (order 0) by
    disp [3,P0,P1,P2] float64, then flips, D <-> H transpose, per-channel gain and bias on the data.  Either of data / target may be None."""
    L.require_gpu()
    if tuple(order) != (1, 0):
        raise ValueError("elastic: only order 1 (image) and order 0 (targets) exist -- the reader's call sites; order 3 is not implemented")
    patch = tuple(int(v) for v in disp.shape[1:])
    if disp.dtype != torch.float64 or int(disp.shape[0]) != 3:
        raise ValueError("elastic: disp must be a float64 [3,P0,P1,P2] tensor")
    for t in (data, target):
        if t is not None and tuple(int(v) for v in t.shape[1:]) != patch:
            raise ValueError("elastic: channels %s do not match the displacement field %s" % (tuple(t.shape), tuple(disp.shape)))
    data = None if data is None else data.contiguous().float()       # strided views (a transposed one-hot volume) are laid out here
    target = None if target is None else target.contiguous().float()
    disp = disp.contiguous()
    c = 0 if data is None else int(data.shape[0])
    nt = 0 if target is None else int(target.shape[0])
    out_sp = (patch[1], patch[0], patch[2]) if transpose else patch
    data_out = None if data is None else torch.empty((c,) + out_sp, dtype=torch.float32, device=disp.device)
    target_out = None if target is None else torch.empty((nt,) + out_sp, dtype=torch.float32, device=disp.device)
    gain = [1.0] * c if gain is None else [float(v) for v in gain]
    bias = [0.0] * c if bias is None else [float(v) for v in bias]
    if len(gain) != c or len(bias) != c:
        raise ValueError("elastic: gain and bias need one value per image channel")
    L.check(L.load().ru_elastic_warp(None if data is None else L.f32(data), c, None if target is None else L.f32(target), nt, L.ptr(disp),
                                     patch[0], patch[1], patch[2], _flags(flips, transpose), _arr(C.c_float, gain), _arr(C.c_float, bias),
                                     None if data is None else L.f32(data_out), None if target is None else L.f32(target_out), L.stream()),
            "ru_elastic_warp")
    return data_out, target_out


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
    return z ^ (z >> np.uint64(31))


def elastic_noise_host(seed, patch):
    """numpy restatement of `ru_elastic_noise`, bit for bit: [3,P0,P1,P2] float64"""
    patch = tuple(int(v) for v in patch)
    v = np.arange(1, int(np.prod(patch)) + 1, dtype=np.uint64)
    out = np.empty((3,) + patch, np.float64)
    with np.errstate(over="ignore"):
        for f in range(3):
            key = _mix64(np.array([(int(seed) + (f + 1) * _GOLDEN) & _M64], dtype=np.uint64))
            z = _mix64(key + v * np.uint64(_GOLDEN))
            out[f] = ((z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0).reshape(patch)
    return out


def elastic_field_host(noise, sigma, alpha):
    """numpy restatement of `ru_elastic_field` (float64): per axis 0, 1, 2 the banded matrix G[i, j] = w[i - j], |i - j| <= radius, of
    scipy's normalised Gaussian weights -- zero outside the volume is the matrix simply ending -- then the scales alpha, alpha, alpha / 2.5."""
    sigma, alpha = float(sigma), float(alpha)
    _check_sigma(sigma)
    noise = np.asarray(noise, np.float64)
    if noise.ndim != 4 or noise.shape[0] != 3:
        raise ValueError("elastic: noise must be [3,P0,P1,P2], got %s" % (noise.shape,))
    r = elastic_radius(sigma)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w = w / w.sum()
    out = noise
    for ax in (1, 2, 3):
        n = out.shape[ax]
        d = np.arange(n)[:, None] - np.arange(n)[None, :]
        g = np.where(np.abs(d) <= r, w[np.clip(d + r, 0, 2 * r)], 0.0)
        out = np.moveaxis(np.tensordot(g, out, axes=([1], [ax])), 0, ax)
    return np.ascontiguousarray(out * np.array([alpha, alpha, alpha / 2.5]).reshape(3, 1, 1, 1))


def _reflect(i, n):
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def elastic_warp_host(data, target, disp, flips=(False, False, False), transpose=False, gain=None, bias=None, order=(1, 0)):
    """numpy restatement of `ru_elastic_warp`: data [C,P0,P1,P2] by map_coordinates(order=1, mode='reflect') in float64 (returned float64),
    target [T,P0,P1,P2] by order=0 (returned in its own dtype), then flips, transpose, gain and bias.  Either may be None."""
    if tuple(order) != (1, 0):
        raise ValueError("elastic: only order 1 (image) and order 0 (targets) exist -- the reader's call sites; order 3 is not implemented")
    disp = np.asarray(disp, np.float64)
    patch = disp.shape[1:]
    grid = np.meshgrid(*[np.arange(n) for n in patch], indexing="ij")
    lo, hi, wt, near = [], [], [], []
    for ax in range(3):
        c = grid[ax] + disp[ax]
        f = np.floor(c)
        lo.append(_reflect(f.astype(np.int64), patch[ax]))
        hi.append(_reflect(f.astype(np.int64) + 1, patch[ax]))
        wt.append(c - f)
        near.append(_reflect(np.floor(c + 0.5).astype(np.int64), patch[ax]))

    def finish(t):
        for ax, f in enumerate(flips):
            if f:
                t = np.flip(t, axis=ax + 1)
        return np.ascontiguousarray(t.transpose((0, 2, 1, 3)) if transpose else t)

    data_out = target_out = None
    if data is not None:
        src = np.asarray(data, np.float64)
        acc = np.zeros(src.shape, np.float64)
        for qa in range(2):
            for qb in range(2):
                for qc in range(2):
                    w = (wt[0] if qa else 1.0 - wt[0]) * (wt[1] if qb else 1.0 - wt[1]) * (wt[2] if qc else 1.0 - wt[2])
                    acc += w[None] * src[:, (hi[0] if qa else lo[0]), (hi[1] if qb else lo[1]), (hi[2] if qc else lo[2])]
        data_out = finish(acc)
        if gain is not None:
            data_out = data_out * np.asarray(gain, np.float64).reshape(-1, 1, 1, 1)
        if bias is not None:
            data_out = data_out + np.asarray(bias, np.float64).reshape(-1, 1, 1, 1)
    if target is not None:
        target_out = finish(np.asarray(target)[:, near[0], near[1], near[2]])
    return data_out, target_out


class SimpleReader(torch.utils.data.Dataset):
    """dataloader.py:67-216 over in-memory cases: `cases` is a list of (image [C,D,H,W], label [D,H,W]) arrays (or of callables
    returning such a pair -- the place for a NIfTI reader).  Items are ([data], [target]) like the reference's, on the device.
    A case may be (image, label, soft) with soft [3,D,H,W] float32 teacher probabilities: its targets are distilled from `soft`
    (see DeviceCase); the draws are the same.  `elastic=True` deforms every patch (see augment_patch) with the sigma and alpha the reference
    draws; the field seeds come from a private generator seeded with `elastic_seed`, so the global streams are those of `elastic=False`."""

    def __init__(self, cases, patch_size, images_in_epoch=4000, patches_from_single_image=1, device="cuda", elastic=False, elastic_seed=None):
        super(SimpleReader, self).__init__()
        self.cases = list(cases)
        self.patch_size = tuple(patch_size)
        self.images_in_epoch = images_in_epoch
        self.patches_from_single_image = patches_from_single_image
        self.device = device
        self.elastic = bool(elastic)
        self.elastic_rng = random.Random(elastic_seed)
        self.real_length = len(self.cases)
        self.patches_from_current_image = self.patches_from_single_image + 1     # first item loads (the reference's constructor + first item do)
        self.current_image_index = 0
        self.case = None

    def _load(self, index):
        if self.patches_from_current_image > self.patches_from_single_image or self.case is None:      # dataloader.py:119-121
            self.patches_from_current_image = 0
            self.current_image_index = index
            src = self.cases[index]
            item = src() if callable(src) else src
            image, label = item[0], item[1]
            self.case = DeviceCase(image, label, self.patch_size, self.device, soft=item[2] if len(item) > 2 else None)
        self.patches_from_current_image += 1

    def __getitem__(self, index):
        index = index % self.real_length
        self._load(index)
        p = draw_augment_params(self.case.bbox, self.patch_size, int(self.case.image.shape[0]), elastic=self.elastic, elastic_rng=self.elastic_rng)
        data, target = augment_patch(self.case, p)
        return [data], [target]

    def __len__(self):
        return int(self.images_in_epoch)


class FullReader(torch.utils.data.Dataset):
    """dataloader.py:218-286: whole case, zero-padded to multiples of 16, z-scored, hard WT/TC/ET targets."""

    def __init__(self, cases, device="cuda"):
        super(FullReader, self).__init__()
        self.cases = list(cases)
        self.device = device

    def __getitem__(self, index):
        src = self.cases[index]
        image, label = src() if callable(src) else src
        image, label = np.asarray(image), np.asarray(label)
        new_shape = tuple(int(np.ceil(s / 16.0) * 16) for s in image.shape[1:])      # loader_helper.closest_to_k
        img = np.zeros((image.shape[0],) + new_shape, np.float32)
        lab = np.zeros(new_shape, np.float32)
        img[(slice(None),) + tuple(slice(0, s) for s in image.shape[1:])] = image
        lab[tuple(slice(0, s) for s in label.shape)] = label
        case = DeviceCase(img, lab, new_shape, self.device)
        p = dict(crop_lo=(0, 0, 0), scale=(1.0, 1.0, 1.0), flips=(False, False, False), transpose=False,
                 gain=np.ones(img.shape[0]), bias=np.zeros(img.shape[0]))
        data, target = augment_patch(case, p, new_shape)
        return [data], [target]

    def __len__(self):
        return len(self.cases)
