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

Opt-in: intensity augmentation (csrc/intensity.hip), the transforms nnU-Net made standard and the reference does not have: Gaussian blur, simulated
low resolution, additive Gaussian noise, brightness, contrast and gamma, per channel, on the data tensor `augment_patch` returns.
`SimpleReader(..., intensity=True)` draws them from a private generator; `intensity_augment` takes explicit parameters and
`intensity_augment_host` is the float64 restatement.

Opt-in: rotation (csrc/rotate.hip), the spatial transform nnU-Net's recipes rely on most and the reference cannot afford.  A `rotation` entry in the
parameters of `augment_patch` replaces the zoom pass by `ru_augment_patch_affine`: the patch is gathered from the WHOLE resident volume through a
3 x 3 matrix and an offset (scipy's affine_transform convention, order 1, zero fill outside the volume), so a rotated patch shows real tissue in its
corners.  `SimpleReader(..., rotation=True)` draws the angles from a private generator; `affine_patch_host` is the float64 restatement.

Opt-in: the whole training set resident in HBM (csrc/resident.hip).  A list reader uploads a case (143 MB of float32 at BraTS size), runs numpy over its
label and waits for the device every time it changes case -- once per patch with the reference's settings.  `ResidentCases(cases, patch_size)` does that
work ONCE per case and keeps each case cropped to its non-zero box, as uint16 where that is exact (see `pack_case_host`); `SimpleReader(store, ...)`
then only selects a view, `augment_patch` takes the view (`ResidentCase`) in place of a `DeviceCase`, `augment_batch` cuts a whole batch in one launch
and `ResidentLoader` stands in for the `DataLoader`.  The per-voxel arithmetic is the one function of csrc/augment_voxel.hpp, so every patch equals the
list reader's bit for bit.

Opt-in: CarveMix (csrc/carvemix.hip), the lesion-aware mix of two cases (Zhang et al., MICCAI 2021; written from the paper, not checked against the
authors' code).  `carvemix(data, target, donor_data, donor_target, u, side)` carves the region s <= T around each donor's WT lesion -- s the exact
signed squared distance map of `ops.signed_sqdist`, T an integer threshold formed on the device from the lesion's volume and the draw u -- and
pastes its voxels and labels into the receivers in place; `carvemix_host` is the numpy restatement, bit for bit.  `SimpleReader(..., carvemix=True)`
draws everything the option adds from private generators; `ResidentLoader` mixes a batch with one extra gather and one mix launch.
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


def draw_augment_params(bbox, patch_size, channels=4, elastic=False, elastic_rng=None, rng=None, np_rng=None):
    """The draws of SimpleReader.__getitem__ (dataloader.py:141-199), in its order, from the same global generators.  `elastic=True` keeps
    the two values the reference draws for its switched-off elastic transform (:167-168) and adds `elastic=dict(sigma, alpha, seed)`; the seed
    comes from `elastic_rng` (a private `random.Random`), never from the global generators, which advance exactly as with `elastic=False`.
    `rng` (a `random.Random`) and `np_rng` (a `numpy.random.RandomState`) stand in for the global `random` / `numpy.random` modules, which are the
    defaults: the same draws in the same order from private streams (the CarveMix donor's)."""
    rng = random if rng is None else rng
    np_rng = np.random if np_rng is None else np_rng
    center = np_rng.rand(3)
    center = center * (bbox[1] - bbox[0]) + bbox[0]
    left_bottom = (center - np.array(patch_size) / 2.0).astype(np.int32)
    r_sigma = rng.random()                               # sigma / alpha of the elastic transform (:167-168), drawn whether it runs or not
    r_alpha = rng.random()
    scale = [0.7 + rng.random() * 0.6 for _ in range(3)]
    flips = [rng.random() > 0.5 for _ in range(3)]
    transpose = rng.random() > 0.5
    gain = np_rng.uniform(0.9, 1.1, size=(channels, 1, 1, 1)).reshape(-1)
    bias = np_rng.uniform(-0.2, 0.2, size=(channels, 1, 1, 1)).reshape(-1)
    p = dict(crop_lo=left_bottom, scale=np.array(scale), flips=flips, transpose=transpose, gain=gain, bias=bias)
    if elastic:
        p["elastic"] = dict(sigma=r_sigma * 20 + 10, alpha=r_alpha * 4000 + 200, seed=(elastic_rng or _ELASTIC_RNG).getrandbits(63))
    return p


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _flags(flips, transpose):
    return sum(1 << i for i, f in enumerate(flips) if f) | (8 if transpose else 0)


ZOOM_MAX_COORD = 2.0 ** 30


def _check_zoom_scale(scale, patch):
    """argument check of the zoom pass, ValueError before any launch: the kernel converts floor(scale * index) to a 32-bit integer, so every scale is
    finite and the largest source coordinate scale * (P - 1) stays below 2^30.  (A scale <= 0 is left to the entry point, which refuses it.)"""
    sc = np.asarray(scale, np.float64).reshape(-1)
    if sc.shape != (3,):
        raise ValueError("zoom: scale must hold three values, got %r" % (scale,))
    for ax in range(3):
        if sc[ax] == np.inf:                                 # NaN and -inf are not positive: the entry point's refusal
            raise ValueError("zoom: scale[%d] is not finite" % ax)
        if sc[ax] * float(int(patch[ax]) - 1) >= ZOOM_MAX_COORD:
            raise ValueError("zoom: scale[%d] * (patch[%d] - 1) = %g reaches 2^30" % (ax, ax, sc[ax] * float(int(patch[ax]) - 1)))


def augment_patch(case, p, patch_size=None):
    """(data [C,Q0,Q1,P2], target [3,Q0,Q1,P2]) float32 device tensors for explicit parameters `p` (see draw_augment_params).  A case
    with soft targets takes the same pass with the teacher's three channels interpolated in place of the one-hot label
    (`ru_augment_patch_soft`: affine_transform(soft, (1, sx, sy, sz), order=1, mode='reflect'), dataloader.py:179 on float channels).

    With an `elastic` entry in `p` (dict(sigma, alpha, seed), or `noise` [3,P0,P1,P2] float64 in place of `seed`) the patch is deformed as
    the reference's commented lines :177 / :180 would: the zoom pass runs without flips, gain or bias, then `elastic_noise` ->
    `elastic_field` -> `elastic_warp` (order 1 on the image, order 0 on the targets) and the warp applies flips, transpose, gain and bias.

    With a `rotation` entry in `p` the affine pass (`ru_augment_patch_affine`, see `affine_patch_host`) takes the place of the zoom pass, in the same
    slot: directly, or in front of the elastic warp with flags 0, gain 1 and bias 0.  The entry is dict(angles=(a0, a1, a2)) in radians -- the patch
    is rotated by `rotation_matrix(angles)` and zoomed by p["scale"] about its own centre: matrix = R diag(scale), offset = centre - matrix (P - 1) / 2
    with centre = crop_lo + (P - 1) / 2 -- or dict(matrix=3x3[, offset=3]) for an explicit transform (p["scale"] is not applied then; without
    `offset` the matrix acts about the patch centre as above).  The crop need not lie inside the volume: outside it the image is raw 0, the targets 0.
    An optional `mapping` ("row" / "brick") picks the kernel's thread mapping; the result does not depend on it."""
    patch = tuple(int(v) for v in (patch_size or case.patch_size))
    resident = isinstance(case, ResidentCase)            # a view of a ResidentCases store: the packed gather runs in the slot of the two passes
    c, d, h, w = ((case.channels,) + case.shape) if resident else (int(v) for v in case.image.shape)
    el = p.get("elastic")
    rot = p.get("rotation")
    affine = None if rot is None else _rotation_transform(rot, p["crop_lo"], p["scale"], patch)      # argument checks before any launch
    if affine is None:
        _check_zoom_scale(p["scale"], patch)
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
    if resident:
        _packed_gather([case], [_patch_desc(flags, gain, bias, crop_lo=p["crop_lo"], scale=p["scale"], affine=affine)], patch, data, target)
        if direct:
            return data, target
        if noise is None:
            noise = elastic_noise(int(el["seed"]), patch, case.image.device)
        return elastic_warp(data, target, elastic_field(noise, sigma, alpha), p["flips"], p["transpose"], p["gain"], p["bias"])
    if affine is not None:
        matrix, offset, mapping = affine
        L.check(lib.ru_augment_patch_affine(L.f32(case.image), L.ptr(case.label), None if soft is None else L.f32(soft),
                                            _arr(C.c_float, [float(v) for v in case.mean]), _arr(C.c_float, [float(1.0 / v) for v in case.std]),
                                            c, d, h, w, _arr(C.c_int, list(patch)), _arr(C.c_double, [float(v) for v in matrix.reshape(-1)]),
                                            _arr(C.c_double, [float(v) for v in offset]), flags, _arr(C.c_float, gain), _arr(C.c_float, bias),
                                            mapping, L.f32(data), L.f32(target), L.stream()), "ru_augment_patch_affine")
        if direct:
            return data, target
        if noise is None:
            noise = elastic_noise(int(el["seed"]), patch, case.image.device)
        return elastic_warp(data, target, elastic_field(noise, sigma, alpha), p["flips"], p["transpose"], p["gain"], p["bias"])
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


# ---------------------------------------------------------------------------------------------------------------- resident training set
# csrc/resident.hip: packed cases (`ru_case_probe` / `ru_case_pack` / `ru_case_unpack`) and the batched gather (`ru_augment_batch_packed`).
def pack_case_host(image, label, soft=None):
    """(box_lo, box_size, kind) of a case, the numpy restatement of `ru_case_probe`: the box bounds every voxel where the bit pattern of any image
    or soft channel is not that of +0.0f (so -0.0 and NaN are inside) or the label is not 0 -- (0,0,0) / (1,1,1) for an all-zero case -- and kind
    is "uint16" if every image value x (as float32) satisfies bits(float32(uint16(x))) == bits(x), else "float32": a negative, fractional,
    above-65535, -0.0 or NaN value anywhere makes the case float32."""
    x = np.ascontiguousarray(image, dtype=np.float32)
    if x.ndim != 4:
        raise ValueError("resident: image must be [C,D,H,W], got shape %s" % (x.shape,))
    lab = np.asarray(label)
    if lab.shape != x.shape[1:]:
        raise ValueError("resident: label must be [D,H,W] = %s, got %s" % (x.shape[1:], lab.shape))
    bits = x.view(np.uint32)
    occupied = (bits != 0).any(axis=0) | (lab != 0)
    if soft is not None:
        sf = np.ascontiguousarray(soft.detach().cpu().numpy() if isinstance(soft, torch.Tensor) else soft, dtype=np.float32)
        if sf.shape != (3,) + x.shape[1:]:
            raise ValueError("resident: soft targets must be [3,D,H,W] = %s, got %s" % ((3,) + x.shape[1:], sf.shape))
        occupied |= (sf.view(np.uint32) != 0).any(axis=0)
    box = _bbox3(occupied)
    if box[0][0] < 0:
        lo, size = (0, 0, 0), (1, 1, 1)
    else:
        lo, size = tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1] - box[0] + 1)
    with np.errstate(invalid="ignore"):
        ranged = (x >= 0) & (x <= 65535)
    back = np.where(ranged, x, 0).astype(np.uint16).astype(np.float32)
    exact = bool(ranged.all() and (back.view(np.uint32) == bits).all())
    return lo, size, ("uint16" if exact else "float32")


class ResidentCase(object):
    """One case of a `ResidentCases` store: a view, nothing is copied.  `image` / `label` / `soft` are the PACKED device tensors (the crop of the
    case to `box` = (lo, size); `image` uint16 or float32 by `kind`); `mean`, `std`, `bbox`, `patch_size` are `DeviceCase`'s, `channels` and
    `shape` = (D, H, W) those of the whole case.  `augment_patch` takes it in place of a `DeviceCase`."""

    def __init__(self, image, label, soft, kind, box, shape, mean, std, bbox, patch_size):
        self.image, self.label, self.soft = image, label, soft
        self.kind, self.box, self.shape = kind, box, tuple(int(v) for v in shape)
        self.channels = int(image.shape[0])
        self.mean, self.std, self.bbox, self.patch_size = mean, std, bbox, patch_size
        self.nbytes = sum(int(t.numel()) * t.element_size() for t in (image, label, soft) if t is not None)
        d = L.CaseDesc()
        d.image, d.label, d.soft = image.data_ptr(), label.data_ptr(), (None if soft is None else soft.data_ptr())
        d.kind, d.C = L.PACK_KINDS[kind], self.channels
        d.dims[:], d.box_lo[:], d.box_size[:] = self.shape, box[0], box[1]
        d.mean[:self.channels] = [float(v) for v in mean]                      # the values `augment_patch` hands to ru_augment_patch
        with np.errstate(all="ignore"):                                        # an all-zero case has no statistics, here as in a DeviceCase
            d.inv_std[:self.channels] = [float(1.0 / v) for v in std]
        self._desc = d


class ResidentCases(object):
    """The training set resident in HBM.  `cases` is what `SimpleReader` takes: (image [C,D,H,W], label [D,H,W][, soft [3,D,H,W]]) arrays or
    callables returning them, each called ONCE, here.  Per case, in order: the float32 upload to a transient buffer, `remap_labels`,
    `zscore_stats` on the full upload (so `mean` / `std` are `DeviceCase`'s bit for bit), `label_bbox` on the host, `ru_case_probe` and
    `ru_case_pack` (see `pack_case_host` for the rules); the transient buffer is then freed.  `dtype`: "auto" stores a case as uint16 where that is
    exact and as float32 otherwise, "float32" forces float32, "uint16" raises on a case that is not exact.  `max_bytes` (optional) bounds the
    store: the case that would exceed it raises before its allocation.  `store[i]` is a `ResidentCase`, `store.nbytes` the bytes held,
    `store.unpack(i)` the full (image, label, soft or None) device tensors back, byte for byte."""

    def __init__(self, cases, patch_size, device="cuda", dtype="auto", max_bytes=None):
        if dtype not in ("auto", "float32", "uint16"):
            raise ValueError("resident: dtype must be 'auto', 'float32' or 'uint16', got %r" % (dtype,))
        if max_bytes is not None and (isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 0):
            raise ValueError("resident: max_bytes must be a non-negative integer or None, got %r" % (max_bytes,))
        self.patch_size = tuple(int(p) for p in patch_size)
        if len(self.patch_size) != 3 or min(self.patch_size) < 1:
            raise ValueError("resident: patch_size must hold three positive extents, got %r" % (patch_size,))
        self.device, self.dtype, self.max_bytes = device, dtype, max_bytes
        self.nbytes = 0
        self._views = []
        cases = list(cases)
        if cases:
            L.require_gpu()
        for index, src in enumerate(cases):
            item = src() if callable(src) else src
            self._views.append(self._pack(index, item[0], item[1], item[2] if len(item) > 2 else None))
            self.nbytes += self._views[-1].nbytes

    def _pack(self, index, image, label, soft):
        lib = L.load()
        label = remap_labels(label)
        full = torch.as_tensor(np.ascontiguousarray(image, dtype=np.float32)).to(self.device)
        if full.dim() != 4 or tuple(full.shape[1:]) != tuple(label.shape):
            raise ValueError("resident: case %d: image must be [C,D,H,W] over the label's %s, got %s" % (index, tuple(label.shape), tuple(full.shape)))
        c, d, h, w = (int(v) for v in full.shape)
        lab = torch.as_tensor(label).to(self.device)
        sft = None
        if soft is not None:
            if isinstance(soft, torch.Tensor):
                sft = soft.detach().to(device=self.device, dtype=torch.float32).contiguous()
            else:
                sft = torch.as_tensor(np.ascontiguousarray(soft, dtype=np.float32)).to(self.device)
            if tuple(sft.shape) != (3, d, h, w):
                raise ValueError("soft targets must be [3,D,H,W] = %s, got %s" % ((3, d, h, w), tuple(sft.shape)))
        mean, std = zscore_stats(full)
        bbox = label_bbox(label, self.patch_size)
        probe = torch.empty(8, dtype=torch.int32, device=full.device)
        L.check(lib.ru_case_probe(L.f32(full), L.ptr(lab), None if sft is None else L.f32(sft), c, d, h, w, L.ptr(probe), L.stream()), "ru_case_probe")
        probe = [int(v) for v in probe.cpu()]
        lo, size, exact = tuple(probe[0:3]), tuple(probe[3:6]), bool(probe[6])
        if self.dtype == "uint16" and not exact:
            raise ValueError("resident: case %d is not exact in uint16 (a negative, fractional, above-65535, -0.0 or NaN value) and dtype='uint16'" % index)
        kind = "uint16" if (exact and self.dtype != "float32") else "float32"
        voxels = size[0] * size[1] * size[2]
        need = voxels * (c * (2 if kind == "uint16" else 4) + 1 + (12 if sft is not None else 0))
        if self.max_bytes is not None and self.nbytes + need > self.max_bytes:
            raise ValueError("resident: case %d needs %d bytes; with the %d already held that exceeds max_bytes = %d" % (index, need, self.nbytes, self.max_bytes))
        pimage = torch.empty((c,) + size, dtype=torch.uint16 if kind == "uint16" else torch.float32, device=full.device)
        plabel = torch.empty(size, dtype=torch.uint8, device=full.device)
        psoft = None if sft is None else torch.empty((3,) + size, dtype=torch.float32, device=full.device)
        L.check(lib.ru_case_pack(L.f32(full), L.ptr(lab), None if sft is None else L.f32(sft), c, d, h, w, _arr(C.c_int, list(lo)), _arr(C.c_int, list(size)),
                                 L.PACK_KINDS[kind], L.ptr(pimage), L.ptr(plabel), None if psoft is None else L.f32(psoft), L.stream()), "ru_case_pack")
        return ResidentCase(pimage, plabel, psoft, kind, (lo, size), (d, h, w), mean, std, bbox, self.patch_size)

    def __len__(self):
        return len(self._views)

    def __getitem__(self, index):
        return self._views[index]

    def unpack(self, index):
        """(image [C,D,H,W] float32, label [D,H,W] uint8, soft [3,D,H,W] float32 or None): `ru_case_unpack`, the arrays the case was built from"""
        v = self._views[index]
        d, h, w = v.shape
        image = torch.empty((v.channels, d, h, w), dtype=torch.float32, device=v.image.device)
        label = torch.empty((d, h, w), dtype=torch.uint8, device=v.image.device)
        soft = None if v.soft is None else torch.empty((3, d, h, w), dtype=torch.float32, device=v.image.device)
        L.check(L.load().ru_case_unpack(L.ptr(v.image), L.ptr(v.label), None if v.soft is None else L.f32(v.soft), L.PACK_KINDS[v.kind], v.channels, d, h, w,
                                        _arr(C.c_int, list(v.box[0])), _arr(C.c_int, list(v.box[1])), L.f32(image), L.ptr(label),
                                        None if soft is None else L.f32(soft), L.stream()), "ru_case_unpack")
        return image, label, soft


def _patch_desc(flags, gain, bias, crop_lo=None, scale=None, affine=None):
    """the `ru_patch_desc` (ctypes) of one sample: the affine pass for affine = (matrix, offset, mapping code), else the zoom pass"""
    q = L.PatchDesc()
    q.flags = int(flags)
    if affine is None:
        q.mode = L.AUG_ZOOM
        q.crop_lo[:] = [int(v) for v in crop_lo]
        q.scale[:] = [float(v) for v in scale]
    else:
        matrix, offset, mapping = affine
        q.mode, q.mapping = L.AUG_AFFINE, int(mapping)
        q.matrix[:] = [float(v) for v in matrix.reshape(-1)]
        q.offset[:] = [float(v) for v in offset]
    q.gain[:len(gain)] = [float(v) for v in gain]
    q.bias[:len(bias)] = [float(v) for v in bias]
    return q


def _packed_gather(views, descs, patch, data, target):
    """one `ru_augment_batch_packed` call: sample n = (views[n], descs[n]) into data[n] / target[n] (or into data / target for a single sample)"""
    n = len(views)
    L.check(L.load().ru_augment_batch_packed((L.CaseDesc * n)(*[v._desc for v in views]), (L.PatchDesc * n)(*descs), n, _arr(C.c_int, list(patch)),
                                             L.f32(data), L.f32(target), L.stream()), "ru_augment_batch_packed")


def _check_batch(patch, params_list):
    """argument checks of a batch, ValueError before any launch; returns the `ru_patch_desc` list"""
    descs = []
    for n, p in enumerate(params_list):
        if p.get("elastic") is not None:
            raise ValueError("resident: sample %d has an elastic entry: elastic deformation stays on the per-sample path (augment_patch)" % n)
        if p["transpose"] and len(params_list) > 1 and patch[0] != patch[1]:
            raise ValueError("resident: sample %d is transposed: a batch needs P0 == P1, got patch %s" % (n, tuple(patch)))
        rot = p.get("rotation")
        affine = None if rot is None else _rotation_transform(rot, p["crop_lo"], p["scale"], patch)
        if affine is None:
            _check_zoom_scale(p["scale"], patch)
        descs.append(_patch_desc(_flags(p["flips"], p["transpose"]), p["gain"], p["bias"], crop_lo=p["crop_lo"], scale=p["scale"], affine=affine))
    return descs


def _augment_views(views, params_list, patch, descs=None):
    descs = _check_batch(patch, params_list) if descs is None else descs
    n, c = len(views), views[0].channels
    out_sp = (patch[1], patch[0], patch[2]) if (n == 1 and params_list[0]["transpose"]) else patch
    data = torch.empty((n, c) + tuple(out_sp), dtype=torch.float32, device=views[0].image.device)
    target = torch.empty((n, 3) + tuple(out_sp), dtype=torch.float32, device=views[0].image.device)
    _packed_gather(views, descs, patch, data, target)
    return data, target


def augment_batch(store, indices, params_list):
    """(data [N,C,Q0,Q1,P2], target [N,3,Q0,Q1,P2]) float32 device tensors: sample n is `augment_patch(store[indices[n]], params_list[n])`, bit for
    bit, all N from ONE `ru_augment_batch_packed` call (chunks of `RU_AUG_BATCH_MAX` samples per launch) written straight into the batch: no
    per-sample tensors, no `torch.stack`.  Zoom and rotated samples, uint16 and float32 cases, hard and soft targets mix freely.  Refused
    (ValueError, before any launch): a sample with an `elastic` entry (elastic deformation stays on the per-sample path), a transposed sample in
    a batch of more than one unless P0 == P1, an index outside the store."""
    indices, params_list = [int(i) for i in indices], list(params_list)
    if len(indices) != len(params_list) or not indices:
        raise ValueError("resident: one parameter dict per index and at least one sample, got %d indices and %d dicts" % (len(indices), len(params_list)))
    for i in indices:
        if not 0 <= i < len(store):
            raise ValueError("resident: index %d outside the store of %d cases" % (i, len(store)))
    patch = tuple(int(v) for v in store.patch_size)
    descs = _check_batch(patch, params_list)
    L.require_gpu()
    return _augment_views([store[i] for i in indices], params_list, patch, descs)


# ---------------------------------------------------------------------------------------------------------------- rotation
# csrc/rotate.hip (`ru_augment_patch_affine`) and its float64 numpy restatement.  Array axes: 0 = D, 1 = H, 2 = W.
AFFINE_MIN_DET = 1e-6


def rotation_matrix(angles):
    """3 x 3 float64 R = R0(a0) @ R1(a1) @ R2(a2) for angles in radians about the array axes 0 = D, 1 = H, 2 = W.  With c = cos a, s = sin a:
    R0 = [[1,0,0],[0,c,-s],[0,s,c]], R1 = [[c,0,s],[0,1,0],[-s,0,c]], R2 = [[c,-s,0],[s,c,0],[0,0,1]]."""
    a = np.asarray(angles, np.float64)
    if a.shape != (3,):
        raise ValueError("rotation: angles must be three values (radians about D, H, W), got shape %s" % (a.shape,))
    if not np.isfinite(a).all():
        raise ValueError("rotation: angles must be finite, got %r" % (a,))
    (c0, c1, c2), (s0, s1, s2) = np.cos(a), np.sin(a)
    r0 = np.array([[1.0, 0.0, 0.0], [0.0, c0, -s0], [0.0, s0, c0]])
    r1 = np.array([[c1, 0.0, s1], [0.0, 1.0, 0.0], [-s1, 0.0, c1]])
    r2 = np.array([[c2, -s2, 0.0], [s2, c2, 0.0], [0.0, 0.0, 1.0]])
    return r0 @ r1 @ r2 + 0.0                            # + 0.0: no negative zeros


def _check_affine(matrix, offset):
    """argument checks of the affine pass: ValueError before any launch; returns (matrix [3,3], offset [3]) float64"""
    try:
        m, o = np.asarray(matrix, np.float64), np.asarray(offset, np.float64)
    except (TypeError, ValueError):
        raise ValueError("rotation: matrix and offset must be numeric arrays")
    if m.shape != (3, 3):
        raise ValueError("rotation: matrix must be 3 x 3, got shape %s" % (m.shape,))
    if o.shape != (3,):
        raise ValueError("rotation: offset must hold three values, got shape %s" % (o.shape,))
    if not (np.isfinite(m).all() and np.isfinite(o).all()):
        raise ValueError("rotation: matrix and offset must be finite")
    det = float(np.linalg.det(m))
    if not abs(det) >= AFFINE_MIN_DET:
        raise ValueError("rotation: the matrix is singular: |det| = %g is below %g (a collapsed patch)" % (abs(det), AFFINE_MIN_DET))
    return np.ascontiguousarray(m), np.ascontiguousarray(o)


def _rotation_transform(rot, crop_lo, scale, patch):
    """(matrix, offset, mapping code) of a `rotation` entry of `augment_patch` (see there); every argument error is a ValueError"""
    if not isinstance(rot, dict):
        raise ValueError("rotation: the entry must be dict(angles=...) or dict(matrix=...[, offset=...]), got %r" % (rot,))
    unknown = set(rot) - {"angles", "matrix", "offset", "mapping"}
    if unknown:
        raise ValueError("rotation: unknown keys %s" % sorted(unknown))
    mapping = rot.get("mapping") or "default"
    if mapping not in L.AFFINE_MAPPINGS:
        raise ValueError("rotation: mapping must be one of %s, got %r" % (sorted(L.AFFINE_MAPPINGS), mapping))
    if min(patch) < 1 or int(np.prod([int(v) for v in patch], dtype=object)) >= 2 ** 31 - 1:
        raise ValueError("rotation: the patch extents must be positive and hold fewer than 2^31 - 1 voxels, got %s" % (tuple(patch),))
    half = (np.array(patch, np.float64) - 1.0) / 2.0
    lo = np.asarray(crop_lo, np.float64)
    if lo.shape != (3,) or not np.isfinite(lo).all():
        raise ValueError("rotation: crop_lo must hold three finite values, got %r" % (crop_lo,))
    if "angles" in rot:
        if "matrix" in rot or "offset" in rot:
            raise ValueError("rotation: give either angles or a matrix (with an optional offset), not both")
        sc = np.asarray(scale, np.float64)
        if sc.shape != (3,) or not np.isfinite(sc).all():
            raise ValueError("rotation: scale must hold three finite values, got %r" % (scale,))
        matrix = rotation_matrix(rot["angles"]) * sc[None, :]             # R diag(scale)
        offset = None
    elif "matrix" in rot:
        matrix, offset = rot["matrix"], rot.get("offset")
    else:
        raise ValueError("rotation: the entry needs angles or a matrix")
    matrix, _ = _check_affine(matrix, np.zeros(3))
    if offset is None:
        offset = (lo + half) - matrix @ half
    matrix, offset = _check_affine(matrix, offset)
    return matrix, offset, L.AFFINE_MAPPINGS[mapping]


def affine_patch_host(image, label_or_soft, mean, std, patch, matrix, offset, flips=(False, False, False), transpose=False, gain=None, bias=None):
    """float64 numpy restatement of `ru_augment_patch_affine`, the oracle of the device path: (data [C,Q0,Q1,P2], target [3,Q0,Q1,P2]) float64 from
    plain arrays -- image [C,D,H,W] raw, label [D,H,W] in {0,1,2,3} or soft [3,D,H,W], mean / std per channel.

    For output index q = (i, j, k) of the patch, before flips and transpose, s = matrix q + offset (per axis ((m0 i + m1 j) + m2 k) + offset) in
    whole-volume voxel coordinates; f = floor(s), t = s - f; the eight corners f + {0,1}^3 are weighted by products of 1 - t and t and a corner
    outside the volume contributes 0: scipy.ndimage.affine_transform(volume, matrix, offset, output_shape=patch, order=1, mode='grid-constant',
    cval=0) of every image channel and of every one-hot class (or soft channel).  A coordinate that is not a number, below -2 or above the extent
    counts as -2 / the extent (all fill).  Then ((acc - mean) / std) gain + bias, WT = 1 + 2 + 3, TC = 1 + 3, ET = 3, flips, D <-> H transpose."""
    image = np.asarray(image, np.float64)
    if image.ndim != 4:
        raise ValueError("rotation: image must be [C,D,H,W], got shape %s" % (image.shape,))
    c, dims = image.shape[0], image.shape[1:]
    other = np.asarray(label_or_soft)
    if other.shape != tuple(dims) and other.shape != (3,) + tuple(dims):
        raise ValueError("rotation: label must be [D,H,W] or soft [3,D,H,W] of the image's extents %s, got %s" % (tuple(dims), other.shape))
    patch = tuple(int(v) for v in patch)
    if len(patch) != 3 or min(patch) < 1:
        raise ValueError("rotation: patch must hold three positive extents, got %s" % (patch,))
    m, o = _check_affine(matrix, offset)
    mean, std = np.asarray(mean, np.float64).reshape(-1), np.asarray(std, np.float64).reshape(-1)
    gain = np.ones(c) if gain is None else np.asarray(gain, np.float64).reshape(-1)
    bias = np.zeros(c) if bias is None else np.asarray(bias, np.float64).reshape(-1)
    if not (mean.size == std.size == gain.size == bias.size == c):
        raise ValueError("rotation: mean, std, gain and bias need one value per image channel (%d)" % c)
    q = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in patch], indexing="ij")
    idx, wt, inside = [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for ax in range(3):
            s = ((m[ax, 0] * q[0] + m[ax, 1] * q[1]) + m[ax, 2] * q[2]) + o[ax]
            s = np.where(s >= -2.0, s, -2.0)                                   # NaN too
            s = np.minimum(s, float(dims[ax]))
            f = np.floor(s)
            i0 = f.astype(np.int64)
            idx.append((i0, i0 + 1))
            wt.append((1.0 - (s - f), s - f))
            inside.append(((i0 >= 0) & (i0 < dims[ax]), (i0 + 1 >= 0) & (i0 + 1 < dims[ax])))
    if other.ndim == 3:
        lab = other.astype(np.int64)
        chans = np.stack([lab == 1, lab == 2, lab == 3]).astype(np.float64)
    else:
        chans = other.astype(np.float64)
    src = np.concatenate([image, chans])
    acc = np.zeros((c + 3,) + patch)
    for qa in range(2):
        for qb in range(2):
            for qc in range(2):
                w = wt[0][qa] * wt[1][qb] * wt[2][qc]
                ok = inside[0][qa] & inside[1][qb] & inside[2][qc]
                v = src[:, np.clip(idx[0][qa], 0, dims[0] - 1), np.clip(idx[1][qb], 0, dims[1] - 1), np.clip(idx[2][qc], 0, dims[2] - 1)]
                acc += w[None] * np.where(ok[None], v, 0.0)
    sh = (-1, 1, 1, 1)
    data = ((acc[:c] - mean.reshape(sh)) * (1.0 / std).reshape(sh)) * gain.reshape(sh) + bias.reshape(sh)
    cw = acc[c:]
    target = cw if other.ndim == 4 else np.stack([(cw[0] + cw[1]) + cw[2], cw[0] + cw[2], cw[2]])

    def finish(t):
        for ax, f in enumerate(flips):
            if f:
                t = np.flip(t, axis=ax + 1)
        return np.ascontiguousarray(t.transpose((0, 2, 1, 3)) if transpose else t)

    return finish(data), finish(target)


class RotationConfig(object):
    """Probability and range of `draw_rotation_params`; the defaults are nnU-Net's for 3-D patches: a patch is rotated with probability `p_rotation`,
    by angles uniform in +-max_angle[axis] (radians) about each of the axes D, H, W."""

    def __init__(self, p_rotation=0.2, max_angle=(np.pi / 6.0, np.pi / 6.0, np.pi / 6.0)):
        self.p_rotation = float(p_rotation)
        self.max_angle = tuple(float(v) for v in np.asarray(max_angle, np.float64).reshape(-1))
        if not 0.0 <= self.p_rotation <= 1.0:
            raise ValueError("rotation: p_rotation must lie in [0, 1], got %r" % (p_rotation,))
        if len(self.max_angle) != 3 or not all(np.isfinite(v) and v >= 0.0 for v in self.max_angle):
            raise ValueError("rotation: max_angle must hold three finite non-negative angles (radians), got %r" % (max_angle,))


def draw_rotation_params(rng, config=None):
    """None, or the `rotation` entry dict(angles=(a0, a1, a2)) of `augment_patch`, drawn from `rng` (a private `random.Random`) ONLY: the global
    `random` / `numpy.random` streams are not touched.  One draw decides (`p_rotation`); only if it fires, three angles follow in axis order."""
    cfg = config or RotationConfig()
    if not rng.random() < cfg.p_rotation:
        return None
    return dict(angles=tuple(rng.uniform(-m, m) for m in cfg.max_angle))


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


# ---------------------------------------------------------------------------------------------------------------- intensity augmentation
# csrc/intensity.hip (`ru_intensity_augment`) and its float64 numpy restatement.  Per channel, in this order: blur, low resolution, noise,
# brightness, contrast, gamma.  nnU-Net runs its noise before its blur; here the two spatial stages come first.
INTENSITY_KEYS = ("blur_sigma", "lowres_zoom", "noise_variance", "noise_seed", "brightness", "contrast", "gamma", "gamma_invert", "gamma_retain_stats")


def _check_intensity_params(params, channels):
    """argument checks of `intensity_augment` / `intensity_augment_host`: ValueError before any launch; returns the list of dicts"""
    params = list(params)
    if not 1 <= channels <= L.INT_MAXC:
        raise ValueError("intensity: 1..%d channels, got %d" % (L.INT_MAXC, channels))
    if len(params) != channels:
        raise ValueError("intensity: one parameter dict per channel (%d), got %d" % (channels, len(params)))
    for c, q in enumerate(params):
        unknown = set(q) - set(INTENSITY_KEYS)
        if unknown:
            raise ValueError("intensity: channel %d: unknown keys %s" % (c, sorted(unknown)))
        if "blur_sigma" in q:
            sigma = float(q["blur_sigma"])
            if not (sigma > 0.0 and np.isfinite(sigma)):
                raise ValueError("intensity: channel %d: blur sigma must be positive and finite, got %r" % (c, sigma))
            if elastic_radius(sigma) > L.INT_MAX_RADIUS:
                raise ValueError("intensity: channel %d: blur radius int(4 sigma + 0.5) = %d exceeds %d" % (c, elastic_radius(sigma), L.INT_MAX_RADIUS))
        if "lowres_zoom" in q and not 0.0 < float(q["lowres_zoom"]) <= 1.0:
            raise ValueError("intensity: channel %d: low-res zoom must lie in (0, 1], got %r" % (c, q["lowres_zoom"]))
        if "noise_variance" in q:
            var = float(q["noise_variance"])
            if not (var >= 0.0 and np.isfinite(var)):
                raise ValueError("intensity: channel %d: noise variance must be non-negative and finite, got %r" % (c, var))
            if "noise_seed" not in q:
                raise ValueError("intensity: channel %d: noise_variance needs a noise_seed" % c)
        elif "noise_seed" in q:
            raise ValueError("intensity: channel %d: noise_seed without noise_variance" % c)
        for key in ("brightness", "contrast"):
            if key in q and not np.isfinite(float(q[key])):
                raise ValueError("intensity: channel %d: %s must be finite, got %r" % (c, key, q[key]))
        if "gamma" in q:
            g = float(q["gamma"])
            if not (g > 0.0 and np.isfinite(g)):
                raise ValueError("intensity: channel %d: gamma must be positive and finite, got %r" % (c, g))
        elif "gamma_invert" in q or "gamma_retain_stats" in q:
            raise ValueError("intensity: channel %d: gamma_invert / gamma_retain_stats without gamma" % c)
    return params


def intensity_param_block(params):
    """the `ru_intensity_params` block (ctypes) of a checked list of per-channel dicts"""
    blk = L.IntensityParams()
    for c, q in enumerate(params):
        m = 0
        if "blur_sigma" in q:
            m |= L.INT_BLUR
            blk.blur_sigma[c] = float(q["blur_sigma"])
        if "lowres_zoom" in q:
            m |= L.INT_LOWRES
            blk.lowres_zoom[c] = float(q["lowres_zoom"])
        if "noise_variance" in q:
            m |= L.INT_NOISE
            blk.noise_variance[c] = float(q["noise_variance"])
            blk.noise_seed[c] = int(q["noise_seed"]) & _M64
        if "brightness" in q:
            m |= L.INT_BRIGHTNESS
            blk.brightness[c] = float(q["brightness"])
        if "contrast" in q:
            m |= L.INT_CONTRAST
            blk.contrast[c] = float(q["contrast"])
        if "gamma" in q:
            m |= L.INT_GAMMA | (L.INT_GAMMA_INVERT if q.get("gamma_invert") else 0) | (L.INT_GAMMA_RETAIN if q.get("gamma_retain_stats") else 0)
            blk.gamma[c] = float(q["gamma"])
        blk.mask[c] = m
    return blk


def intensity_augment(data, params):
    """A new float32 device tensor of `data`'s shape [C,P0,P1,P2]: `ru_intensity_augment`.  `params` holds one dict per channel with any of
    `blur_sigma`, `lowres_zoom`, `noise_variance` + `noise_seed`, `brightness`, `contrast`, `gamma` (+ `gamma_invert`, `gamma_retain_stats`); a
    missing key switches that stage off, an empty dict copies the channel bit for bit.  The stages and their order: include/resunet_hip.h,
    restated by `intensity_augment_host`.  Arguments are checked before any launch."""
    L.require_gpu()
    if not isinstance(data, torch.Tensor) or not data.is_cuda or data.dim() != 4:
        raise ValueError("intensity: data must be a [C,P0,P1,P2] device tensor")
    c, p0, p1, p2 = (int(v) for v in data.shape)
    params = _check_intensity_params(params, c)
    if min(p0, p1, p2) < 1:
        raise ValueError("intensity: the patch extents must be positive, got %s" % (tuple(data.shape),))
    data = data.contiguous().float()
    out = torch.empty_like(data)
    lib = L.load()
    ws = L.workspace(lib.ru_intensity_workspace_bytes(c, p0, p1, p2), data.device)
    blk = intensity_param_block(params)
    L.check(lib.ru_intensity_augment(L.f32(data), L.f32(out), c, p0, p1, p2, C.byref(blk), L.ptr(ws), ws.numel(), L.stream()), "ru_intensity_augment")
    return out


def intensity_noise_host(seed, channel, count):
    """The first `count` values n(seed, channel, v), v = 0 .. count-1, of `ru_intensity_augment`'s noise in float64 (the device rounds ln, sqrt and
    cos to float32, ln u1 with a relative error: logf(h) + (u1 - h) / h, h = float32(u1); tests/intensity_inputs.py holds n to its roundings): key = mix64(seed + (channel + 1) G); z1 = mix64(key + (2 v + 1) G), z2 = mix64(key + (2 v + 2) G); u1 = ((z1 >> 11) + 1) / 2^53
    in (0, 1], u2 = (z2 >> 11) / 2^53 in [0, 1); n = sqrt(-2 ln u1) cos(2 pi u2).  mix64 and G are `elastic_noise_host`'s."""
    v = np.arange(int(count), dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = _mix64(np.array([(int(seed) + (int(channel) + 1) * _GOLDEN) & _M64], dtype=np.uint64))
        z1 = _mix64(key + (np.uint64(2) * v + np.uint64(1)) * np.uint64(_GOLDEN))
        z2 = _mix64(key + (np.uint64(2) * v + np.uint64(2)) * np.uint64(_GOLDEN))
    u1 = ((z1 >> np.uint64(11)).astype(np.float64) + 1.0) / 9007199254740992.0
    u2 = (z2 >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def intensity_blur_host(x, sigma):
    """scipy.ndimage.gaussian_filter(x, sigma, mode='reflect') of one channel restated: radius int(4 sigma + 0.5), weights exp(-0.5 d^2 / sigma^2) / sum,
    axes 0, 1, 2 in turn on the half-sample-symmetric extension, periodic beyond one reflection (`_reflect`)"""
    x = np.asarray(x, np.float64)
    r = elastic_radius(sigma)
    d = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * d ** 2)
    w = w / w.sum()
    for ax in range(x.ndim):
        n = x.shape[ax]
        xp = np.take(x, _reflect(np.arange(-r, n + r), n), axis=ax)
        x = sum(w[k] * np.take(xp, np.arange(k, k + n), axis=ax) for k in range(2 * r + 1))
    return x


def lowres_axis_host(n, zoom):
    """(s0, s1, t) of one axis of the low-res stage: output voxel i = (1 - t[i]) x[s0[i]] + t[i] x[s1[i]].  n_c = max(1, floor(n zoom + 0.5)); coarse
    sample j is the source voxel min(floor((j + 0.5) n / n_c), n - 1); i sits at c = clamp((i + 0.5) n_c / n - 0.5, 0, n_c - 1) between coarse
    samples floor(c) and min(floor(c) + 1, n_c - 1).  The indices are formed in integers, as the kernel forms them."""
    n = int(n)
    nc = max(1, int(np.floor(n * float(zoom) + 0.5)))
    i = np.arange(n, dtype=np.int64)
    num = np.maximum((2 * i + 1) * nc - n, 0)
    j0 = num // (2 * n)
    t = (num % (2 * n)) / (2.0 * n)
    t = np.where(j0 >= nc - 1, 0.0, t)
    j0 = np.minimum(j0, nc - 1)
    j1 = np.minimum(j0 + 1, nc - 1)
    src = lambda j: np.minimum(((2 * j + 1) * n) // (2 * nc), n - 1)
    return src(j0), src(j1), t


def intensity_lowres_host(x, zoom):
    """the low-res stage of one channel: nearest-neighbour down to the coarse grid and linear interpolation back, axis by axis (`lowres_axis_host`)"""
    x = np.asarray(x, np.float64)
    for ax in range(x.ndim):
        s0, s1, t = lowres_axis_host(x.shape[ax], zoom)
        shape = [1] * x.ndim
        shape[ax] = -1
        t = t.reshape(shape)
        x = (1.0 - t) * np.take(x, s0, axis=ax) + t * np.take(x, s1, axis=ax)
    return x


def intensity_contrast_host(x, factor):
    x = np.asarray(x, np.float64)
    mean = x.mean()
    return np.clip((x - mean) * float(factor) + mean, x.min(), x.max())


def intensity_gamma_host(x, gamma, invert=False, retain_stats=False):
    x = np.asarray(x, np.float64)
    if invert:
        x = -x
    mean, std, mn = x.mean(), x.std(), x.min()
    rng = x.max() - mn
    y = np.power((x - mn) / (rng + 1e-7), float(gamma)) * rng + mn
    if retain_stats:
        sy = y.std()
        y = (y - y.mean()) * (std / (sy if sy >= 1e-8 else 1e-8)) + mean
    return -y if invert else y


def intensity_augment_host(data, params):
    """float64 numpy restatement of `ru_intensity_augment` on data [C,P0,P1,P2] (returned float64): the oracle of the device path.  Per channel, in
    order: blur (`intensity_blur_host`), low resolution (`intensity_lowres_host`), x + sqrt(noise_variance) n(noise_seed, channel, v)
    (`intensity_noise_host`, v the linear voxel index), x * brightness, clip((x - mean) contrast + mean, min, max), gamma
    (`intensity_gamma_host`); mean, std (population), min, max are the channel's as it enters the stage."""
    data = np.asarray(data.detach().cpu().numpy() if isinstance(data, torch.Tensor) else data, np.float64)
    if data.ndim != 4:
        raise ValueError("intensity: data must be [C,P0,P1,P2], got %s" % (data.shape,))
    params = _check_intensity_params(params, data.shape[0])
    out = np.empty_like(data)
    for c, q in enumerate(params):
        x = data[c]
        if "blur_sigma" in q:
            x = intensity_blur_host(x, q["blur_sigma"])
        if "lowres_zoom" in q:
            x = intensity_lowres_host(x, q["lowres_zoom"])
        if "noise_variance" in q:
            x = x + np.sqrt(float(q["noise_variance"])) * intensity_noise_host(q["noise_seed"], c, x.size).reshape(x.shape)
        if "brightness" in q:
            x = x * float(q["brightness"])
        if "contrast" in q:
            x = intensity_contrast_host(x, q["contrast"])
        if "gamma" in q:
            x = intensity_gamma_host(x, q["gamma"], bool(q.get("gamma_invert")), bool(q.get("gamma_retain_stats")))
        out[c] = x
    return out


class IntensityConfig(object):
    """Probabilities and ranges of `draw_intensity_params`; the defaults are nnU-Net's.  `p_*` is the chance per patch; blur and low-res then pick
    each channel with `p_*_channel`, the other transforms take every channel of a patch they fire on, each with a value of its own.  Ranges are
    (low, high) of a uniform draw.  One gamma stage exists per channel: the inverted draw (`p_gamma_invert`) and the plain one (`p_gamma`) are made
    independently, and where both fire the inverted one wins.  Both run with `gamma_retain_stats`."""

    def __init__(self, p_blur=0.2, p_blur_channel=0.5, blur_sigma=(0.5, 1.0), p_lowres=0.25, p_lowres_channel=0.5, lowres_zoom=(0.5, 1.0),
                 p_noise=0.1, noise_variance=(0.0, 0.1), p_brightness=0.15, brightness=(0.75, 1.25), p_contrast=0.15, contrast=(0.75, 1.25),
                 p_gamma_invert=0.1, p_gamma=0.3, gamma=(0.7, 1.5), gamma_retain_stats=True):
        self.p_blur, self.p_blur_channel, self.blur_sigma = float(p_blur), float(p_blur_channel), tuple(blur_sigma)
        self.p_lowres, self.p_lowres_channel, self.lowres_zoom = float(p_lowres), float(p_lowres_channel), tuple(lowres_zoom)
        self.p_noise, self.noise_variance = float(p_noise), tuple(noise_variance)
        self.p_brightness, self.brightness = float(p_brightness), tuple(brightness)
        self.p_contrast, self.contrast = float(p_contrast), tuple(contrast)
        self.p_gamma_invert, self.p_gamma, self.gamma = float(p_gamma_invert), float(p_gamma), tuple(gamma)
        self.gamma_retain_stats = bool(gamma_retain_stats)


def draw_intensity_params(channels, rng, config=None):
    """One dict per channel for `intensity_augment`, drawn from `rng` (a private `random.Random`) ONLY: the global `random` / `numpy.random` streams
    are not touched.  Order of the draws: blur, low-res, noise, brightness, contrast, inverted gamma, plain gamma; per transform the per-patch
    draw first, then (only if it fired) the channels in order.  See `IntensityConfig` for the probabilities and for the gamma rule."""
    cfg = config or IntensityConfig()
    params = [dict() for _ in range(int(channels))]
    if rng.random() < cfg.p_blur:
        for q in params:
            if rng.random() < cfg.p_blur_channel:
                q["blur_sigma"] = rng.uniform(*cfg.blur_sigma)
    if rng.random() < cfg.p_lowres:
        for q in params:
            if rng.random() < cfg.p_lowres_channel:
                q["lowres_zoom"] = rng.uniform(*cfg.lowres_zoom)
    if rng.random() < cfg.p_noise:
        for q in params:
            q["noise_variance"] = rng.uniform(*cfg.noise_variance)
            q["noise_seed"] = rng.getrandbits(63)
    if rng.random() < cfg.p_brightness:
        for q in params:
            q["brightness"] = rng.uniform(*cfg.brightness)
    if rng.random() < cfg.p_contrast:
        for q in params:
            q["contrast"] = rng.uniform(*cfg.contrast)
    inverted = rng.random() < cfg.p_gamma_invert
    inverted_values = [rng.uniform(*cfg.gamma) for _ in params] if inverted else None
    plain = rng.random() < cfg.p_gamma
    plain_values = [rng.uniform(*cfg.gamma) for _ in params] if plain else None
    if inverted or plain:
        for q, g in zip(params, inverted_values if inverted else plain_values):
            q["gamma"], q["gamma_invert"], q["gamma_retain_stats"] = g, inverted, cfg.gamma_retain_stats
    return params


# ---------------------------------------------------------------------------------------------------------------- CarveMix
# csrc/carvemix.hip (`ru_carvemix_threshold`, `ru_carvemix_mix`) around `ops.signed_sqdist`, and the numpy restatement.  Written from the paper
# (Zhang et al., MICCAI 2021; NeuroImage 2023), not checked against the authors' code; the definition is INTEGRATION.md's.
CARVE_SIDES = ("outer", "inner")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def carvemix_r2(volume):
    """the largest integer q with q^3 <= volume^2 (floor(volume^(2/3))), by integer search: the squared form of the paper's lambda_u = V^(1/3)"""
    v2 = int(volume) * int(volume)
    lo, hi = 0, 1 << 18
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if mid * mid * mid <= v2:
            lo = mid
        else:
            hi = mid - 1
    return lo


def carvemix_threshold_host(volume, voxels, u, side):
    """T of one donor: INT32_MIN for an empty lesion, INT32_MAX for a full one, else floor((u u) R2) (outer) or -ceil(((u u) R2) 0.25) (inner) in
    float64 from plain multiplies"""
    volume, voxels, u = int(volume), int(voxels), float(u)
    if volume == 0:
        return INT32_MIN
    if volume == voxels:
        return INT32_MAX
    a = (u * u) * float(carvemix_r2(volume))
    return int(np.floor(a)) if side == "outer" else -int(np.ceil(a * 0.25))


def _check_carvemix(data_shape, target_shape, donor_data_shape, donor_target_shape, u, side, dst):
    """argument checks of `carvemix` / `carvemix_host`: ValueError before any launch; returns (u list, side list, dst list)"""
    ds, ts, dds, dts = (tuple(int(v) for v in s) for s in (data_shape, target_shape, donor_data_shape, donor_target_shape))
    if len(ds) != 5 or len(ts) != 5 or len(dds) != 5 or len(dts) != 5:
        raise ValueError("carvemix: data / target must be [N,C,D,H,W] / [N,3,D,H,W] and the donors [K,C,D,H,W] / [K,3,D,H,W], got %s %s %s %s" % (ds, ts, dds, dts))
    n, c, sp = ds[0], ds[1], ds[2:]
    k = dds[0]
    if ts != (n, 3) + sp or dds != (k, c) + sp or dts != (k, 3) + sp:
        raise ValueError("carvemix: shapes do not agree: data %s, target %s, donor data %s, donor target %s" % (ds, ts, dds, dts))
    if not 1 <= c <= 8:
        raise ValueError("carvemix: 1..8 data channels, got %d" % c)
    if min(sp) < 1 or max(sp) > 512:
        raise ValueError("carvemix: every axis of the patch must be in [1, 512] (the limit of signed_sqdist), got %s" % (sp,))
    if not 1 <= k <= n:
        raise ValueError("carvemix: %d donors into %d receivers: 1 <= K <= N" % (k, n))
    try:
        u = [float(v) for v in np.asarray(u, np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError("carvemix: u must hold one number per donor")
    side = [side] * k if isinstance(side, str) else list(side)
    if len(u) != k or len(side) != k:
        raise ValueError("carvemix: one u and one side per donor (%d), got %d and %d" % (k, len(u), len(side)))
    for v in u:
        if not 0.0 <= v < 1.0:
            raise ValueError("carvemix: u must lie in [0, 1), got %r" % (v,))
    for sd in side:
        if sd not in CARVE_SIDES:
            raise ValueError("carvemix: side must be 'outer' or 'inner', got %r" % (sd,))
    if dst is None:
        if k != n:
            raise ValueError("carvemix: %d donors and %d receivers need a dst list" % (k, n))
        dst = list(range(k))
    dst = [int(v) for v in dst]
    if len(dst) != k or len(set(dst)) != k or not all(0 <= v < n for v in dst):
        raise ValueError("carvemix: dst must hold %d distinct indices in [0, %d), got %r" % (k, n, dst))
    return u, side, dst


def carvemix(data, target, donor_data, donor_target, u, side, dst=None, want_mask=False):
    """CarveMix on the device, IN PLACE on the receivers: data [N,C,D,H,W] / target [N,3,D,H,W] (contiguous float32 device tensors), donors
    donor_data [K,C,D,H,W] / donor_target [K,3,D,H,W], `u` [K] floats in [0, 1), `side` [K] of "outer" / "inner" (or one string).  Donor k goes into
    receiver dst[k] (distinct indices); with dst=None and N == K the donors pair up in order.  One `ops.signed_sqdist` of the K WT channels, one
    `ru_carvemix_threshold`, one `ru_carvemix_mix` launch; nothing waits for the host.  Returns (data, target), or with `want_mask`
    (data, target, mask uint8 [K,D,H,W], T int32 [K], V int64 [K]) as device tensors.  The definition: include/resunet_hip.h, restated by
    `carvemix_host`.  Arguments are checked before any launch (ValueError)."""
    from . import ops
    for t in (data, target, donor_data, donor_target):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("carvemix: expected float32 tensors")
    u, side, dst = _check_carvemix(data.shape, target.shape, donor_data.shape, donor_target.shape, u, side, dst)
    if not (data.is_contiguous() and target.is_contiguous()):
        raise ValueError("carvemix: the receivers are mixed in place and must be contiguous")
    L.require_gpu()
    n, c, d, h, w = (int(v) for v in data.shape)
    k, vox = int(donor_data.shape[0]), d * h * w
    donor_data, donor_target = donor_data.contiguous(), donor_target.contiguous()
    wt = donor_target[:, 0].contiguous()
    lib = L.load()
    s = ops.signed_sqdist(wt)
    thr = torch.empty(k, dtype=torch.int32, device=data.device)
    vol = torch.empty(k, dtype=torch.int64, device=data.device)
    ws = L.workspace(lib.ru_carvemix_workspace_bytes(k, vox), data.device)
    L.check(lib.ru_carvemix_threshold(L.f32(wt), k, vox, _arr(C.c_double, u), _arr(C.c_int, [L.CARVE_SIDES[sd] for sd in side]), L.ptr(thr), L.ptr(vol),
                                      L.ptr(ws), ws.numel(), L.stream()), "ru_carvemix_threshold")
    mask = torch.empty((k, d, h, w), dtype=torch.uint8, device=data.device) if want_mask else None
    L.check(lib.ru_carvemix_mix(L.f32(donor_data), L.f32(donor_target), L.ptr(s), L.ptr(thr), k, _arr(C.c_int, dst), n, c, d, h, w, L.f32(data), L.f32(target),
                                None if mask is None else L.ptr(mask), L.stream()), "ru_carvemix_mix")
    return (data, target, mask, thr, vol) if want_mask else (data, target)


def carvemix_host(data, target, donor_data, donor_target, u, side, dst=None):
    """numpy restatement of `carvemix`, the oracle of the device path, built on `loss.signed_sqdist_host`: returns NEW arrays
    (data, target, mask uint8 [K,D,H,W], T int32 [K], V int64 [K]).  Per donor: G = Ya[0] > 0.5f, V = |G|, s = signed_sqdist(Ya[0]),
    T = `carvemix_threshold_host`, M = s <= T, and the receiver takes the donor's 32-bit words where M."""
    from .loss import signed_sqdist_host
    arrs = [np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32) for t in (data, target, donor_data, donor_target)]
    data, target, donor_data, donor_target = arrs
    u, side, dst = _check_carvemix(data.shape, target.shape, donor_data.shape, donor_target.shape, u, side, dst)
    data, target = data.copy(), target.copy()
    k, vox = donor_data.shape[0], int(np.prod(data.shape[2:]))
    mask = np.zeros((k,) + data.shape[2:], np.uint8)
    thr, vol = np.zeros(k, np.int32), np.zeros(k, np.int64)
    for j in range(k):
        wt = donor_target[j, 0]
        vol[j] = int((wt > np.float32(0.5)).sum())
        thr[j] = carvemix_threshold_host(vol[j], vox, u[j], side[j])
        m = signed_sqdist_host(wt) <= thr[j]
        mask[j] = m
        xb, yb = data[dst[j]].view(np.uint32), target[dst[j]].view(np.uint32)       # words, not numbers: NaN and -0.0 pass through
        xb[:, m] = donor_data[j].view(np.uint32)[:, m]
        yb[:, m] = donor_target[j].view(np.uint32)[:, m]
    return data, target, mask, thr, vol


class CarveMixConfig(object):
    """`p_mix`: the probability per sample that `draw_carvemix_params` mixes a donor in.  0.5 is a placeholder, not a recommendation: a value would
    need trained weights to argue for."""

    def __init__(self, p_mix=0.5):
        self.p_mix = float(p_mix)
        if not 0.0 <= self.p_mix <= 1.0:
            raise ValueError("carvemix: p_mix must lie in [0, 1], got %r" % (p_mix,))


def draw_carvemix_params(rng, config, n_cases):
    """None, or dict(donor=case index, u=float in [0, 1), side="outer" / "inner"), drawn from `rng` (a private `random.Random`) ONLY.  One draw
    decides (`p_mix`); only if it fires follow the donor, uniform over the `n_cases` cases (it may be the receiver's own), u and the side (each
    with probability 1/2)."""
    cfg = config or CarveMixConfig()
    if not rng.random() < cfg.p_mix:
        return None
    donor = rng.randrange(int(n_cases))
    u = rng.random()
    return dict(donor=donor, u=u, side="inner" if rng.random() < 0.5 else "outer")


class SimpleReader(torch.utils.data.Dataset):
    """dataloader.py:67-216 over in-memory cases: `cases` is a list of (image [C,D,H,W], label [D,H,W]) arrays (or of callables
    returning such a pair -- the place for a NIfTI reader).  Items are ([data], [target]) like the reference's, on the device.
    A case may be (image, label, soft) with soft [3,D,H,W] float32 teacher probabilities: its targets are distilled from `soft`
    (see DeviceCase); the draws are the same.  `elastic=True` deforms every patch (see augment_patch) with the sigma and alpha the reference
    draws; the field seeds come from a private generator seeded with `elastic_seed`, so the global streams are those of `elastic=False`.
    `intensity=True` (nnU-Net's defaults) or an `IntensityConfig` runs `intensity_augment` on the data tensor of every patch, elastic or not, with
    parameters drawn from a private `random.Random(intensity_seed)`; targets and the global streams are those of `intensity=False`.
    `rotation=True` (nnU-Net's defaults) or a `RotationConfig` rotates a patch with probability `p_rotation` about its own centre (see augment_patch),
    the angles drawn from a private `random.Random(rotation_seed)`: a patch that draws no rotation takes the path above bit for bit, one that does
    keeps its crop, scale, flip, transpose, gain and bias draws, and the global streams are those of `rotation=False`.
    `cases` may be a `ResidentCases` store (built for the same `patch_size`): a change of case then selects a view -- no upload, no host numpy, no
    synchronisation -- and the draws, their order and the items are those of the list reader over the same cases, bit for bit.
    `carvemix=True` (`CarveMixConfig()`, whose p_mix is a placeholder) or a `CarveMixConfig` mixes a donor patch into a sample with probability
    `p_mix` (see `carvemix`).  Every draw the option adds -- the decision, the donor's case index, u, the side and the donor's OWN crop centre,
    zoom, flips, transpose, gain and bias -- comes from private generators seeded by `carvemix_seed`; the global streams are those of
    `carvemix=False`.  The donor is cut by the plain zoom path (no elastic field, no rotation); it takes its own transpose draw when P0 == P1 and
    the receiver's otherwise (the draw is made either way).  `intensity=` runs after the mix, on the mixed data.  Over a `ResidentCases` store the
    donor is a view; over a list it costs a `DeviceCase` build (upload, statistics, label box) per mixed sample."""

    def __init__(self, cases, patch_size, images_in_epoch=4000, patches_from_single_image=1, device="cuda", elastic=False, elastic_seed=None,
                 intensity=False, intensity_seed=None, rotation=False, rotation_seed=None, carvemix=False, carvemix_seed=None):
        super(SimpleReader, self).__init__()
        self.store = cases if isinstance(cases, ResidentCases) else None
        self.cases = cases if self.store is not None else list(cases)
        self.patch_size = tuple(patch_size)
        if self.store is not None and tuple(int(v) for v in self.patch_size) != self.store.patch_size:
            raise ValueError("SimpleReader: the store was built for patch %s, the reader asks for %s" % (self.store.patch_size, self.patch_size))
        self.images_in_epoch = images_in_epoch
        self.patches_from_single_image = patches_from_single_image
        self.device = device
        self.elastic = bool(elastic)
        self.elastic_rng = random.Random(elastic_seed)
        self.intensity = intensity if isinstance(intensity, IntensityConfig) else (IntensityConfig() if intensity else None)
        self.intensity_rng = random.Random(intensity_seed)
        self.rotation = rotation if isinstance(rotation, RotationConfig) else (RotationConfig() if rotation else None)
        self.rotation_rng = random.Random(rotation_seed)
        self.carvemix = carvemix if isinstance(carvemix, CarveMixConfig) else (CarveMixConfig() if carvemix else None)
        self.carvemix_rng = random.Random(carvemix_seed)
        self.carvemix_np_rng = np.random.RandomState(self.carvemix_rng.getrandbits(32))      # the donor's crop centre, gain and bias
        self.last_params = None                                                              # the draws of the latest item (see _draw)
        self.real_length = len(self.cases)
        self.patches_from_current_image = self.patches_from_single_image + 1     # first item loads (the reference's constructor + first item do)
        self.current_image_index = 0
        self.case = None

    def _load(self, index):
        if self.patches_from_current_image > self.patches_from_single_image or self.case is None:      # dataloader.py:119-121
            self.patches_from_current_image = 0
            self.current_image_index = index
            if self.store is not None:
                self.case = self.store[index]
            else:
                src = self.cases[index]
                item = src() if callable(src) else src
                image, label = item[0], item[1]
                self.case = DeviceCase(image, label, self.patch_size, self.device, soft=item[2] if len(item) > 2 else None)
        self.patches_from_current_image += 1

    def _draw(self, index):
        """selects the case of item `index` (`self.case`) and makes the item's draws, in the reference's order; returns the parameters"""
        index = index % self.real_length
        self._load(index)
        p = draw_augment_params(self.case.bbox, self.patch_size, int(self.case.image.shape[0]), elastic=self.elastic, elastic_rng=self.elastic_rng)
        if self.rotation is not None:
            rot = draw_rotation_params(self.rotation_rng, self.rotation)
            if rot is not None:
                p["rotation"] = rot
        if self.carvemix is not None:
            mix = draw_carvemix_params(self.carvemix_rng, self.carvemix, self.real_length)
            if mix is not None:
                mix["case"] = self._donor_case(mix["donor"])
                q = draw_augment_params(mix["case"].bbox, self.patch_size, int(self.case.image.shape[0]), rng=self.carvemix_rng, np_rng=self.carvemix_np_rng)
                if int(self.patch_size[0]) != int(self.patch_size[1]):
                    q["transpose"] = p["transpose"]              # the donor must land in the receiver's layout; its own draw was still made
                mix["params"] = q
                p["carvemix"] = mix
        self.last_params = p
        return p

    def _donor_case(self, index):
        """the donor's case: a view of the store, or a `DeviceCase` built for this sample (the receiver's own case is reused)"""
        if self.store is not None:
            return self.store[index]
        if index == self.current_image_index and self.case is not None:
            return self.case
        src = self.cases[index]
        item = src() if callable(src) else src
        return DeviceCase(item[0], item[1], self.patch_size, self.device, soft=item[2] if len(item) > 2 else None)

    def __getitem__(self, index):
        p = self._draw(index)
        data, target = augment_patch(self.case, p)
        mix = p.get("carvemix")
        if mix is not None:
            donor_data, donor_target = augment_patch(mix["case"], mix["params"])
            carvemix(data[None], target[None], donor_data[None], donor_target[None], [mix["u"]], [mix["side"]])
        if self.intensity is not None:
            data = intensity_augment(data, draw_intensity_params(int(data.shape[0]), self.intensity_rng, self.intensity))
        return [data], [target]

    def __len__(self):
        return int(self.images_in_epoch)


class ResidentLoader(object):
    """Stands in for `torch.utils.data.DataLoader` over a `SimpleReader` on a `ResidentCases` store (`Trainer.train` only iterates it and reads
    `len()`): for every index batch of `batch_sampler` -- default `BatchSampler(RandomSampler(reader), batch_size, drop_last)` -- the reader's draws
    are made sample by sample in `__getitem__`'s order, ONE `augment_batch` launch writes the batch (a batch with an elastic sample falls back to
    per-sample `augment_patch` calls and `torch.stack`), the K samples that drew a CarveMix donor get their donors from ONE more `augment_batch`
    launch and are mixed in place by one `carvemix` call, `intensity_augment` runs per sample, and ([data], [target]) is yielded: the batches of
    `DataLoader(reader, batch_sampler=..., num_workers=0)` under the same seeds, bit for bit, without the per-sample tensors and the stack."""

    def __init__(self, reader, batch_size=1, batch_sampler=None, drop_last=True):
        if not isinstance(reader, SimpleReader) or reader.store is None:
            raise ValueError("ResidentLoader: the reader must be a SimpleReader over a ResidentCases store")
        self.reader = reader
        if batch_sampler is None:
            batch_sampler = torch.utils.data.BatchSampler(torch.utils.data.RandomSampler(reader), int(batch_size), bool(drop_last))
        self.batch_sampler = batch_sampler

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        r = self.reader
        for batch in self.batch_sampler:
            views, params = [], []
            for index in batch:
                params.append(r._draw(index))
                views.append(r.case)
            if any(p.get("elastic") is not None for p in params):
                items = [augment_patch(v, p) for v, p in zip(views, params)]
                data, target = torch.stack([d for d, _ in items]), torch.stack([t for _, t in items])
            else:
                data, target = _augment_views(views, params, tuple(int(v) for v in r.patch_size))
            mixed = [n for n, p in enumerate(params) if p.get("carvemix") is not None]
            if mixed:                                        # the K donors of the batch: one more gather, one map, one threshold call, one mix launch
                mixes = [params[n]["carvemix"] for n in mixed]
                donor_data, donor_target = _augment_views([m["case"] for m in mixes], [m["params"] for m in mixes], tuple(int(v) for v in r.patch_size))
                carvemix(data, target, donor_data, donor_target, [m["u"] for m in mixes], [m["side"] for m in mixes], dst=mixed)
            if r.intensity is not None:
                data = torch.stack([intensity_augment(data[n], draw_intensity_params(int(data.shape[1]), r.intensity_rng, r.intensity))
                                    for n in range(int(data.shape[0]))])
            yield [data], [target]


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
