#!/usr/bin/env python3
"""Generate tests/golden/elastic.npz by running the REFERENCE's own `dataloader.elastic_transform` (dataloader.py:24-48).

    python tests/golden/make_elastic_golden.py

Needs the reference tree (see make_golden.py: it is imported unmodified, with blank stand-ins for the packages its module header names and this
path does not use).  For each parameter set the file holds sigma, alpha, seed and the shape; a sub-sampled copy ([::3] per axis) of the three
float64 displacement fields, recomputed here with the reference's three `gaussian_filter` lines from `np.random.RandomState(seed)`; the
function's output for a seeded float64 image at order 1 (same sub-sampling) and for the four channels of a seeded one-hot volume at order 0
(every voxel, bit-packed).  Inputs are not stored: `make_noise`, `make_image` and `make_onehot` below regenerate them, which is also how a test
feeds the reference's own random draws to the device.  Fixtures are data -- no reference source text is stored.

The order-0 comparison is exact, which is only fair if no source coordinate sits on a rounding boundary: `generate` asserts that none lies
within 1e-9 of a half-integer.  If a new set breaks that, change its seed."""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
from scipy.ndimage import gaussian_filter

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "elastic.npz")
REF = os.environ.get("BRATS_REFERENCE_DIR", "/root/reference")
SUB = 3
# shape, sigma, alpha, seed.  Set 1: displacements up to 7.7 voxels, 12.7 % of the axis-0 coordinates outside the volume (the reflect rule);
# set 2: radius 120, larger than every extent.
SETS = (((40, 36, 44), 10.0, 200.0, 7),
        ((40, 36, 44), 14.5, 4200.0, 11),
        ((32, 48, 24), 30.0, 2500.0, 3))


def reference_available():
    return os.path.exists(os.path.join(REF, "dataloader.py"))


def make_noise(seed, shape):
    """[3, *shape] float64: the three `random_state.rand(*shape) * 2 - 1` draws of elastic_transform, in its order (dx, dy, dz)"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.rand(*shape) * 2 - 1 for _ in range(3)])


def make_image(k, shape):
    """a z-score-like float64 volume"""
    return np.random.default_rng(100 + k).standard_normal(shape)


def make_onehot(k, shape):
    """[4, *shape] float64 one-hot channels of a blocky label volume {0, 1, 2, 3} (4-voxel blocks: boundaries everywhere)"""
    coarse = np.random.default_rng(200 + k).integers(0, 4, tuple((s + 3) // 4 for s in shape))
    lab = np.kron(coarse, np.ones((4, 4, 4), np.int64))[tuple(slice(0, s) for s in shape)]
    return np.eye(4)[lab].transpose((3, 0, 1, 2))


def reference_fields(seed, shape, sigma, alpha):
    """dataloader.py:38-40 of the reference: its three gaussian_filter lines, from its random draws"""
    n = make_noise(seed, shape)
    return np.stack([gaussian_filter(n[0], sigma, mode="constant", cval=0) * alpha,
                     gaussian_filter(n[1], sigma, mode="constant", cval=0) * alpha,
                     gaussian_filter(n[2], sigma, mode="constant", cval=0) * (alpha / 2.5)])


def _reference_function():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    for name in ("nibabel", "SimpleITK", "tensorboardX", "tqdm"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = types.ModuleType(name)
                if name == "tensorboardX":
                    m.SummaryWriter = object
                sys.modules[name] = m
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import dataloader as ref_dl
    return ref_dl.elastic_transform


def generate():
    elastic_transform = _reference_function()
    out = {"n": np.array(len(SETS), np.int32), "sub": np.array(SUB, np.int32)}
    sub = (slice(None, None, SUB),) * 3
    for k, (shape, sigma, alpha, seed) in enumerate(SETS):
        disp = reference_fields(seed, shape, sigma, alpha)
        coords = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")) + disp
        assert np.abs((coords - np.floor(coords)) - 0.5).min() > 1e-9, "set %d: a source coordinate within 1e-9 of a half-integer -- change the seed" % k
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            image_out = elastic_transform(make_image(k, shape), alpha, sigma, 1, np.random.RandomState(seed))
            onehot_out = np.stack([elastic_transform(ch, alpha, sigma, 0, np.random.RandomState(seed)) for ch in make_onehot(k, shape)])
        assert image_out.dtype == np.float64 and set(np.unique(onehot_out).tolist()) <= {0.0, 1.0}
        out["shape%d" % k] = np.array(shape, np.int32)
        out["sigma%d" % k] = np.array(sigma, np.float64)
        out["alpha%d" % k] = np.array(alpha, np.float64)
        out["seed%d" % k] = np.array(seed, np.int64)
        out["disp%d" % k] = np.ascontiguousarray(disp[(slice(None),) + sub])
        out["image_out%d" % k] = np.ascontiguousarray(image_out[sub])
        out["onehot_out_bits%d" % k] = np.packbits(onehot_out.astype(np.uint8))
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
