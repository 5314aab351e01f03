#!/usr/bin/env python3
"""Generate tests/golden/overlap.npz by running the REFERENCE's own `Dice1D`, `RMSE`, `RMSE_masked`, `DiceWT`, `Dice_ITK` (metrics.py:22-185)
and its offline scorer validate.py.

Runs only where a checkout of the reference exists:

    python tests/golden/make_overlap_golden.py <reference checkout>      # or BRATS_REF=<reference checkout>

It imports the reference's metrics.py unmodified, drives each class over seeded batches with several `update`s, and stores the inputs,
every `get()` and the constructor surface (name, defaults).  validate.py runs unmodified through runpy on three synthetic cases.

SimpleITK is not installed here.  A stand-in module in `sys.modules` provides `GetImageFromArray`, `HausdorffDistanceImageFilter` (only
constructed: the reference builds one in its Hausdorff classes' __init__) and `LabelOverlapMeasuresImageFilter`: `Execute(g, p)` on two
binary images, `GetDiceCoefficient()` = ITK's mean overlap 2J/(1+J) from the union overlap J = I/(P+G-I) of the one non-zero label, in
float64.  When the label is absent from both images it returns BOTH_EMPTY = NaN.  That value was NOT checked against SimpleITK, whose
versions differ there; the formula is ITK's documented definition.
"""
import contextlib
import importlib.util
import io
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BRATS_REF", "")
OUT = os.path.join(HERE, "overlap.npz")
BOTH_EMPTY = float("nan")


# ---------------------------------------------------------------- stand-in SimpleITK
class _Image(object):
    def __init__(self, arr):
        self.arr = np.asarray(arr)


class _LabelOverlapMeasuresImageFilter(object):
    def __init__(self):
        self._dice = None

    def Execute(self, source, target):
        a, b = source.arr != 0, target.arr != 0
        inter, union = int((a & b).sum()), int((a | b).sum())
        if union == 0:
            self._dice = BOTH_EMPTY
            return
        j = float(inter) / float(union)
        self._dice = 2.0 * j / (1.0 + j)

    def GetDiceCoefficient(self):
        return self._dice


class _HausdorffDistanceImageFilter(object):
    def Execute(self, image1, image2):
        raise NotImplementedError("not used by this generator")


def _install_sitk():
    m = types.ModuleType("SimpleITK")
    m.GetImageFromArray = _Image
    m.LabelOverlapMeasuresImageFilter = _LabelOverlapMeasuresImageFilter
    m.HausdorffDistanceImageFilter = _HausdorffDistanceImageFilter
    sys.modules["SimpleITK"] = m


def _load_reference_metrics():
    if not os.path.isfile(os.path.join(REF, "metrics.py")):
        sys.exit("usage: make_overlap_golden.py <reference checkout>  (no metrics.py under %r)" % REF)
    _install_sitk()
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(REF, "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- seeded inputs
def label_volume(rng, shape, empty=()):
    """BraTS-like labels {0,1,2,3}: nested random balls, ED (2) around TC (1, 3), ET (3) inside; `empty` drops those labels."""
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    lab = np.zeros(shape, dtype=np.uint8)
    c = [rng.uniform(0.3 * s, 0.7 * s) for s in shape]
    r2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
    r = rng.uniform(0.25, 0.45) * min(shape)
    lab[r2 <= r * r] = 2
    lab[r2 <= (0.6 * r) ** 2] = 1
    lab[(r2 <= (0.35 * r) ** 2) | ((r2 <= (0.6 * r) ** 2) & (rng.random(shape) < 0.2))] = 3
    for e in empty:
        lab[lab == e] = 0
    return lab


def nested_target(lab):
    """The dataloader's targets from a label volume: WT (labels > 0) >= TC (1, 3) >= ET (3), as float32 one-hot regions."""
    return np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3]).astype(np.float32)


def quantised_prediction(rng, tgt, flip=0.15):
    """Probabilities in multiples of 1/8: exact ties between channels and values of exactly 0.5 occur often."""
    p = np.where(tgt > 0.5, rng.integers(3, 9, size=tgt.shape), rng.integers(0, 6, size=tgt.shape)) / 8.0
    noise = rng.random(tgt.shape) < flip
    p = np.where(noise, rng.integers(0, 9, size=tgt.shape) / 8.0, p)
    return p.astype(np.float32)


def batch(seed, n, shape, empties=()):
    rng = np.random.default_rng(seed)
    labs = [label_volume(rng, shape, empties[i] if i < len(empties) else ()) for i in range(n)]
    g = np.stack([nested_target(l) for l in labs])
    p = np.stack([quantised_prediction(rng, t) for t in g])
    return p, g


def batch_empty(seed):
    """N = 3 on 8 x 6 x 5: sample 0 prediction empty (argmax 0 everywhere: all ties), sample 1 target empty, sample 2 both empty."""
    rng = np.random.default_rng(seed)
    shape = (8, 6, 5)
    p, g = batch(seed, 3, shape)
    p[0] = 0.5                                                               # every channel ties: argmax 0, and nothing > 0.5
    g[1] = 0.0
    p[2] = (rng.integers(0, 5, size=p[2].shape) / 8.0).astype(np.float32)    # <= 0.5 everywhere
    p[2, 0] = 0.5                                                            # channel 0 wins or ties everywhere
    g[2] = 0.0
    return p, g


def batch_soft(seed, n, c, shape, nans=False):
    """Free (not nested) probabilities on both sides in multiples of 1/4, so that every label wins somewhere and equal maxima are
    common; `nans`: a sprinkling of NaN on both sides (torch's argmax takes the first NaN)."""
    rng = np.random.default_rng(seed)
    p = (rng.integers(0, 5, size=(n, c) + shape) / 4.0).astype(np.float32)
    g = (rng.integers(0, 5, size=(n, c) + shape) / 4.0).astype(np.float32)
    g[:, 0] = np.where(rng.random((n,) + shape) < 0.5, g[:, 0], 1.0)       # mostly background, as a segmentation is
    if nans:
        p[rng.random(p.shape) < 0.05] = np.nan
        g[rng.random(g.shape) < 0.05] = np.nan
    return p, g


def validate_cases(seed):
    """Three (label, prediction) pairs of uint8 {0,1,2,4}: one ragged, one without label 4 on either side (d3 = NaN -> 1), one with an
    empty prediction."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (shape, empty) in enumerate([((13, 11, 9), ()), ((10, 12, 8), (3,)), ((9, 9, 7), ())]):
        lab = label_volume(rng, shape, empty)
        pred = lab.copy()
        flip = rng.random(shape) < 0.2
        pred[flip] = rng.integers(0, 4 if 3 not in empty else 3, size=int(flip.sum()))
        if k == 2:
            pred[:] = 0
        lab[lab == 3] = 4
        pred[pred == 3] = 4
        out.append(("case%d" % k, lab, pred))
    return out


# ---------------------------------------------------------------- runs
def run_metric(make, batches, order, update):
    m = make()
    vals, raised = [], ""
    for _ in range(2):                                                       # reset() between two passes over the same sequence
        m.reset()
        for b in order:
            try:
                update(m, batches[b])
            except Exception as e:                                           # noqa: BLE001 -- recorded: the fixture pins that it raises
                raised = type(e).__name__
                return m, np.zeros((0,)), raised
            vals.append(np.atleast_1d(np.asarray(m.get(), dtype=np.float64)))
    return m, np.stack(vals), raised


def run_validate(cases):
    data = tempfile.mkdtemp()
    try:
        labels = {name: lab for name, lab, _ in cases}
        preds = {os.path.join(data, "pred", name + ".nii.gz"): pred for name, _, pred in cases}
        for name in labels:
            os.makedirs(os.path.join(data, "data", name))
        stub = types.ModuleType("loader_helper")

        def read_multimodal(data_path, series, annotation_path=None, read_annotation=True):
            lab = labels[series].copy()
            lab[lab == 4] = 3                                                # loader_helper.read_multimodal:30
            return None, lab, None

        stub.read_multimodal = read_multimodal
        stub.read_nii = lambda path: preds[path].copy()
        sys.modules["loader_helper"] = stub
        got = {"cases": [], "mean": None}

        def recorder(*args, **kw):
            # validate.py prints str(result) per case: take the array itself from the module's namespace
            g = sys._getframe(1).f_globals
            if len(args) == 2 and args[0] in labels:
                got["cases"].append((args[0], np.array(g["result"], dtype=np.float64)))
            elif len(args) == 1 and isinstance(args[0], np.ndarray):
                got["mean"] = np.array(args[0], dtype=np.float64)

        argv = sys.argv
        sys.argv = ["validate.py", "--data_path", os.path.join(data, "data"), "--predictions_path", os.path.join(data, "pred")]
        try:
            runpy.run_path(os.path.join(REF, "validate.py"), init_globals={"print": recorder}, run_name="__main__")
        finally:
            sys.argv = argv
    finally:
        shutil.rmtree(data)
    return got


def main():
    import torch

    with contextlib.redirect_stdout(io.StringIO()):
        ref = _load_reference_metrics()
    sys.modules["metrics"] = ref                                             # validate.py imports it as `metrics`
    batches = [batch(3, 2, (12, 10, 9)), batch(4, 3, (7, 5, 11), empties=[(3,), (1, 3), ()]), batch_empty(5),
               batch(6, 1, (16, 8, 8)), batch_soft(10, 2, 3, (9, 7, 5)), batch_soft(11, 3, 4, (5, 6, 7)),
               batch_soft(12, 2, 3, (6, 5, 4), nans=True)]
    rng = np.random.default_rng(9)
    masked = []                                                              # RMSE_masked's valid shape [1, 2, 2, H, H]
    for _ in range(2):
        p = (rng.integers(0, 9, size=(1, 2, 2, 6, 6)) / 8.0).astype(np.float32)
        g = (rng.random((1, 2, 2, 6, 6)) < 0.3).astype(np.float32)
        masked.append((p, g))
    masked[1][1][0, 1] = 0.0                                                 # a channel whose mask is empty

    def upd(m, pg):
        p, g = pg
        m.update([torch.from_numpy(g)], [torch.from_numpy(p)])

    runs = {
        # name: (constructor, batch list, order)
        "dice1d3": (lambda: ref.Dice1D(classes=3), batches, [0, 1, 2, 3, 4]),
        "dice1d2": (lambda: ref.Dice1D(name="Dice1D", classes=2), batches, [2, 0]),
        "dice1d4": (lambda: ref.Dice1D(), batches, [0]),                     # classes=4 against 3 channels: raises
        "rmse": (lambda: ref.RMSE(), batches, [0, 1, 2, 3, 4, 5]),
        "rmsemasked": (lambda: ref.RMSE_masked(), masked, [0, 1]),
        "rmsemaskedbad": (lambda: ref.RMSE_masked(), batches, [0]),          # a regular shape: the broadcast raises
        "wt": (lambda: ref.DiceWT(), batches, [0, 4, 1, 2, 5, 3]),
        "wtnan": (lambda: ref.DiceWT(), batches, [6, 4]),
        "itk5": (lambda: ref.Dice_ITK(), batches, [0, 4, 1, 3, 5]),
        "itk4": (lambda: ref.Dice_ITK(classes=4), batches, [1, 2, 0, 4]),
        "itk3": (lambda: ref.Dice_ITK(classes=3), batches, [2, 3, 4, 6]),
        "itk4c4": (lambda: ref.Dice_ITK(classes=4), batches, [5]),
    }
    out = {}
    for b, (p, g) in enumerate(batches):
        out["b%d_pred" % b], out["b%d_gr" % b] = p, g
    for b, (p, g) in enumerate(masked):
        out["m%d_pred" % b], out["m%d_gr" % b] = p, g
    for name, (make, data, order) in runs.items():
        with contextlib.redirect_stdout(io.StringIO()):
            m, vals, raised = run_metric(make, data, order, upd)
        out["run_%s_order" % name] = np.asarray(order, dtype=np.int64)
        out["run_%s_values" % name] = vals
        out["run_%s_raises" % name] = np.asarray(raised)
        out["run_%s_name" % name] = np.asarray(m.name)
        out["run_%s_classes" % name] = np.asarray(getattr(m, "classes", -1))
    # constructor surface: parameter names and defaults of every class, as the reference declares them
    import inspect
    for cls in ("Dice1D", "RMSE", "RMSE_masked", "DiceWT", "Dice_ITK"):
        params = list(inspect.signature(getattr(ref, cls).__init__).parameters.values())[1:]
        out["surface_%s_params" % cls] = np.asarray([p.name for p in params])
        out["surface_%s_defaults" % cls] = np.asarray([repr(p.default) for p in params])
        out["surface_%s_attrs" % cls] = np.asarray(sorted(vars(getattr(ref, cls)()).keys()))
    cases = validate_cases(8)
    got = run_validate(cases)
    for k, (name, lab, pred) in enumerate(cases):
        out["v%d_name" % k], out["v%d_label" % k], out["v%d_pred" % k] = np.asarray(name), lab, pred
    assert [n for n, _ in got["cases"]] == sorted(n for n, _, _ in cases)
    out["validate_results"] = np.stack([r for _, r in got["cases"]])
    out["validate_mean"] = got["mean"]
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d KB)" % (OUT, os.path.getsize(OUT) // 1024))
    for name in runs:
        print(name, out["run_%s_raises" % name], out["run_%s_values" % name][:len(runs[name][2])].tolist())
    print("validate", out["validate_results"].tolist(), out["validate_mean"].tolist())


if __name__ == "__main__":
    main()
