#!/usr/bin/env python3
"""Generate tests/golden/hausdorff.npz by running the REFERENCE's own `Hausdorff_ITK` / `Hausdorff_ITKWT` (metrics.py:188-271).

Runs only where a checkout of the reference exists:

    python tests/golden/make_hausdorff_golden.py <reference checkout>      # or BRATS_REF=<reference checkout>

It imports the reference's metrics.py unmodified and drives its two Hausdorff classes over seeded synthetic batches, storing the
inputs and the values `get()` returns after every `update`.  So the reference's bookkeeping -- thresholds, argmax, the 1e+6 of a
failed filter, its `result[n, i-1] = 0` index slip, the float64 batch mean and the accumulation -- is pinned by its own code.

SimpleITK is not installed here.  Only its distance filter is emulated, by a stand-in module placed in `sys.modules` that provides
`GetImageFromArray` and `HausdorffDistanceImageFilter`: max of the two directed distances, directed(A, B) = max over voxels of A of
the Euclidean distance from the voxel centre to the nearest voxel centre of B at unit spacing (scipy.ndimage.distance_transform_edt),
and a RuntimeError when either image has no foreground voxel.  That definition and that exception are ITK's documented behaviour for
HausdorffDistanceImageFilter on images made by GetImageFromArray (spacing 1); they were not checked against SimpleITK itself.
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BRATS_REF", "")
OUT = os.path.join(HERE, "hausdorff.npz")


# ---------------------------------------------------------------- stand-in SimpleITK: the distance filter only
class _Image(object):
    def __init__(self, arr):
        self.arr = np.asarray(arr)


class _HausdorffDistanceImageFilter(object):
    def __init__(self):
        self._hd = None

    def Execute(self, image1, image2):
        a, b = image1.arr != 0, image2.arr != 0
        if not a.any() or not b.any():
            raise RuntimeError("HausdorffDistanceImageFilter: an input image has no foreground voxel")
        d_ab = float(ndimage.distance_transform_edt(~b)[a].max())
        d_ba = float(ndimage.distance_transform_edt(~a)[b].max())
        self._hd = max(d_ab, d_ba)

    def GetHausdorffDistance(self):
        return self._hd


def _install_sitk():
    m = types.ModuleType("SimpleITK")
    m.GetImageFromArray = _Image
    m.HausdorffDistanceImageFilter = _HausdorffDistanceImageFilter
    sys.modules["SimpleITK"] = m


def _load_reference_metrics():
    if not os.path.isfile(os.path.join(REF, "metrics.py")):
        sys.exit("usage: make_hausdorff_golden.py <reference checkout>  (no metrics.py under %r)" % REF)
    _install_sitk()
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(REF, "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- seeded inputs
def blobs(rng, shape, nblobs):
    """Union of a few random balls in a (D, H, W) volume."""
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    m = np.zeros(shape, dtype=bool)
    for _ in range(nblobs):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(1.0, 0.35 * min(shape))
        m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return m


def soft(rng, mask):
    """Probabilities in multiples of 1/16 with `> 0.5` exactly where mask is set; some background voxels sit at exactly 0.5."""
    hi = 0.5 + rng.integers(1, 9, size=mask.shape) / 16.0
    lo = rng.integers(0, 9, size=mask.shape) / 16.0
    return np.where(mask, hi, lo).astype(np.float32)


def batch_blobs(seed, n, c, shape):
    rng = np.random.default_rng(seed)
    p = np.stack([np.stack([soft(rng, blobs(rng, shape, 3)) for _ in range(c)]) for _ in range(n)])
    g = np.stack([np.stack([soft(rng, blobs(rng, shape, 3)) for _ in range(c)]) for _ in range(n)])
    return p, g


def batch_special(seed):
    """N = 3, C = 3: sample 0 a perfect match; sample 1 channel 0 empty on both sides, channel 1 with an empty prediction;
    sample 2 channel 1 empty on both sides, channel 2 with an empty target.  The both-empty channels pin the reference's i-1 slip at
    i = 0 (writes the last column, later overwritten) and at i = 1 (zeroes channel 0's value)."""
    rng = np.random.default_rng(seed)
    shape = (12, 10, 9)
    pm = np.stack([np.stack([blobs(rng, shape, 2) for _ in range(3)]) for _ in range(3)])
    gm = np.stack([np.stack([blobs(rng, shape, 2) for _ in range(3)]) for _ in range(3)])
    pm[0] = gm[0]
    pm[0, 0, 0, 0, 0] = gm[0, 0, 0, 0, 0] = True              # never empty
    pm[1, 0] = gm[1, 0] = False
    pm[1, 1] = False
    gm[1, 1, 3, 4, 5] = True
    pm[2, 1] = gm[2, 1] = False
    gm[2, 2] = False
    pm[2, 2, 1, 1, 1] = True
    pm[2, 0, 6, 5, 4] = gm[2, 0, 0, 9, 8] = True
    return soft(rng, pm), soft(rng, gm)


def batch_corners():
    """N = 1, C = 3 on 9 x 7 x 5: channel 0 single voxels in opposite corners (HD = sqrt(8^2 + 6^2 + 4^2)), channel 1 a single voxel
    against a full volume, channel 2 empty on both sides (i-1 slip at the last channel)."""
    p = np.zeros((1, 3, 9, 7, 5), dtype=np.float32)
    g = np.zeros_like(p)
    p[0, 0, 0, 0, 0] = 1.0
    g[0, 0, 8, 6, 4] = 0.75
    p[0, 1] = 1.0
    g[0, 1, 4, 3, 2] = 1.0
    return p, g


def batch_ties(seed):
    """Argmax ties for the whole-tumour mask: channel values from {0, 0.25, 0.5} so that equal maxima are common (torch takes the
    first index: a tie with channel 0 is background).  Sample 1 has every maximum at channel 0 on both sides (both masks empty)."""
    rng = np.random.default_rng(seed)
    shape = (3, 4, 16, 13, 11)
    p = (rng.integers(0, 3, size=shape) / 4.0).astype(np.float32)
    g = (rng.integers(0, 3, size=shape) / 4.0).astype(np.float32)
    # sparse foreground: most voxels tie or lose against channel 0
    keep = rng.random(shape[:1] + shape[2:]) < 0.2
    p[:, 0] = np.where(keep, p[:, 0], 0.5)
    g[:, 0] = np.where(rng.random(keep.shape) < 0.2, g[:, 0], 0.5)
    p[1, 0] = 0.5
    g[1, 0] = 0.5
    return p, g


def main():
    import torch

    with contextlib.redirect_stdout(io.StringIO()):
        ref = _load_reference_metrics()
    batches = [batch_blobs(5, 3, 3, (24, 20, 17)), batch_special(6), batch_corners(), batch_ties(7)]
    runs = {
        # name: (constructor, batch order); reset() between the two passes over the same sequence
        "itk4": (lambda: ref.Hausdorff_ITK(name="Hausdorff_ITK", input_index=0, target_index=0, classes=4), [0, 1, 2]),
        "itk3": (lambda: ref.Hausdorff_ITK(classes=3), [1, 0]),
        "itk2": (lambda: ref.Hausdorff_ITK(classes=2), [1, 2]),
        "wt": (lambda: ref.Hausdorff_ITKWT(), [0, 1, 2, 3]),
    }
    out = {}
    for b, (p, g) in enumerate(batches):
        out["b%d_pred" % b] = p
        out["b%d_gr" % b] = g
    for name, (make, order) in runs.items():
        m = make()
        vals = []
        for rep in range(2):
            m.reset()
            for b in order:
                p, g = batches[b]
                with contextlib.redirect_stdout(io.StringIO()):
                    m.update([torch.from_numpy(g)], [torch.from_numpy(p)])
                vals.append(np.atleast_1d(np.asarray(m.get(), dtype=np.float64)))
        out["run_%s_order" % name] = np.asarray(order, dtype=np.int64)
        out["run_%s_values" % name] = np.stack(vals)
        out["run_%s_name" % name] = np.asarray(m.name)
        out["run_%s_classes" % name] = np.asarray(getattr(m, "classes", -1))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d KB)" % (OUT, os.path.getsize(OUT) // 1024))
    for name in runs:
        print(name, out["run_%s_values" % name][:len(runs[name][1])].tolist())


if __name__ == "__main__":
    main()
