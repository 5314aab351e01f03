"""Host-side checks of the label-overlap metrics (no GPU needed): the C-ABI declares the new entry points and refuses bad arguments with
a message, the metric classes have the reference's surface (as recorded in tests/golden/overlap.npz), a numpy oracle -- np.bincount
confusion matrices and the formulas of include/resunet_hip.h -- reproduces every value of the fixture, which the reference's own
metrics.py and validate.py produced, and print_metrics logs like the reference's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
ENTRIES = ("ru_label_confusion", "ru_overlap_accumulate", "ru_dice1d_accumulate", "ru_rmse_accumulate")
CLASSES = ("Dice1D", "RMSE", "RMSE_masked", "DiceWT", "Dice_ITK")


# ---------------------------------------------------------------------- numpy oracle (shared with tests/test_overlap.py)
def conf_prob(pred, gr):
    """[N, C, C] int64: conf[n, a, b] = #voxels with argmax(pred) = a and argmax(gr) = b (numpy's argmax: first maximum, first NaN)."""
    n, c = pred.shape[:2]
    a = np.argmax(pred.reshape(n, c, -1), axis=1)
    b = np.argmax(gr.reshape(n, c, -1), axis=1)
    return np.stack([np.bincount(a[k] * c + b[k], minlength=c * c).reshape(c, c) for k in range(n)]).astype(np.int64)


def conf_label(pred, gr):
    """uint8 label volumes [N, ...]: 4 -> 3, L = 4; -> (conf [N, 4, 4], invalid [N])."""
    n = pred.shape[0]
    p, g = pred.reshape(n, -1).astype(np.int64), gr.reshape(n, -1).astype(np.int64)
    p, g = np.where(p == 4, 3, p), np.where(g == 4, 3, g)
    ok = (p <= 3) & (g <= 3)
    conf = np.stack([np.bincount(p[k][ok[k]] * 4 + g[k][ok[k]], minlength=16).reshape(4, 4) for k in range(n)]).astype(np.int64)
    return conf, (~ok).sum(axis=1).astype(np.int64)


def itk_result(conf, nacc):
    """[N, nacc] float64: label i = 1..nacc, J = I/(P+G-I), 2J/(1+J); NaN for a label absent from both images."""
    n, lab = conf.shape[:2]
    res = np.full((n, nacc), np.nan)
    for k in range(n):
        for i in range(1, nacc + 1):
            if i >= lab:
                continue
            inter, p, g = int(conf[k, i, i]), int(conf[k, i].sum()), int(conf[k, :, i].sum())
            if p + g == 0:
                continue
            j = float(inter) / float(p + g - inter)
            res[k, i - 1] = 2.0 * j / (1.0 + j)
    return res


def _f32_ratio(num, den, eps):
    num, den = np.float32(num), np.float32(den)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(2) * num / (den + np.float32(eps)) if eps else np.float32(2) * num / den


def wt_result(conf):
    """[N] float64 of float32 2*I / (S + 1e-6) over labels > 0."""
    return np.array([float(_f32_ratio(c[1:, 1:].sum(), c[1:].sum() + c[:, 1:].sum(), 1e-6)) for c in conf])


def validate_result(conf):
    """[N, 4] float64: d1, d2, d3, dWT in float32 from the float32-rounded counts, NaN -> 1."""
    out = np.zeros((conf.shape[0], 4))
    for k, c in enumerate(conf):
        pairs = [(c[i, i], c[i].sum() + c[:, i].sum()) for i in (1, 2, 3)] + [(c[1:, 1:].sum(), c[1:].sum() + c[:, 1:].sum())]
        for j, (num, den) in enumerate(pairs):
            r = _f32_ratio(num, den, 0)
            out[k, j] = 1.0 if np.isnan(r) else float(r)
    return out


def dice1d_result(pred, gr, classes):
    pm, gm = pred > 0.5, gr > 0.5
    n = pred.shape[0]
    res = np.zeros((n, classes))
    for c in range(classes):
        p, g = pm[:, c].reshape(n, -1), gm[:, c].reshape(n, -1)
        for k in range(n):
            res[k, c] = float(_f32_ratio((p[k] & g[k]).sum(), p[k].sum() + g[k].sum(), 1e-6))
    return res


def rmse_value(pred, gr):
    d = (pred - gr).astype(np.float64)                # float32 differences, as the device forms them
    return float(np.sqrt((d * d).sum() / d.size))


def rmse_masked_value(pred, gr, mask):
    m = (mask.sum(axis=(2, 3)) > 0).astype(np.float64)[:, :, :, None][:, :2]
    s = m * (pred - gr).astype(np.float64) ** 2       # the reference's broadcasting
    return float(np.sqrt(s.sum() / (m.sum() + 1e-8)))


def oracle_run(g, name):
    """The values get() returns over the fixture's run `name` (two passes with a reset between), from the numpy oracle."""
    order = g["run_%s_order" % name]
    classes = int(g["run_%s_classes" % name])
    vals = []
    for _ in range(2):
        acc, samples = 0.0, 0
        for b in order:
            if name == "rmsemasked":
                p, gr = g["m%d_pred" % b], g["m%d_gr" % b]
                acc = acc + rmse_masked_value(p, gr, gr)
            else:
                p, gr = g["b%d_pred" % b], g["b%d_gr" % b]
                if name.startswith("dice1d"):
                    acc = acc + dice1d_result(p, gr, classes).mean(axis=0)
                elif name == "rmse":
                    acc = acc + rmse_value(p, gr)
                elif name.startswith("wt"):
                    acc = acc + wt_result(conf_prob(p, gr)).mean()
                else:
                    acc = acc + itk_result(conf_prob(p, gr), classes - 1).mean(axis=0)
            samples += 1
            vals.append(np.atleast_1d(np.asarray(acc, dtype=np.float64) / samples))
    return np.stack(vals)


# float32 accumulations on the reference side (numpy 2 keeps `0.0 + np.float32` in float32): compared at float32 rounding
RTOL = {"dice1d": 1e-12, "itk": 0.0, "rmse": 1e-6, "rmsemasked": 1e-6, "wt": 1e-6}


def rtol_of(name):
    return RTOL[re.match(r"(dice1d|itk|rmsemasked|rmse|wt)", name).group(1)]


def run_names(g):
    return sorted(k[4:-7] for k in g if k.startswith("run_") and k.endswith("_values"))


# ---------------------------------------------------------------------- tests
def test_header_and_ctypes_table_declare_the_overlap_entries():
    from brats2019_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    for macro, val in (("RU_CONF_PROB", L.CONF_PROB), ("RU_CONF_LABEL", L.CONF_LABEL), ("RU_OVERLAP_MAX_LABELS", L.OVERLAP_MAX_LABELS),
                       ("RU_OVERLAP_ITK", L.OVERLAP_MODES["itk"]), ("RU_OVERLAP_WT", L.OVERLAP_MODES["wt"]),
                       ("RU_OVERLAP_VALIDATE", L.OVERLAP_MODES["validate"])):
        assert re.search(r"#define %s %d\b" % (macro, val), src), macro


@pytest.fixture(scope="module")
def lib():
    from brats2019_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from brats2019_amd import build
        build.build(verbose=False)
    return L.load()


def test_overlap_entry_points_reject_bad_arguments(lib):
    from brats2019_amd import _lib as L
    d = C.c_void_p(16)                           # never dereferenced: every call below fails its argument check first
    cases = [
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, d, 0, 1, 9, 100, d, None, None)),      # C > 8: counted on the host side
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, d, 0, 1, 0, 100, d, None, None)),
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, d, 0, 1, 3, 0, d, None, None)),
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, d, 2, 1, 3, 100, d, None, None)),
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, d, 1, 1, 1, 100, d, None, None)),      # labels need the invalid counter
        ("ru_label_confusion", lambda: lib.ru_label_confusion(d, None, 0, 1, 3, 100, d, None, None)),
        ("ru_overlap_accumulate", lambda: lib.ru_overlap_accumulate(d, 1, 3, 0, 0, d, None, None)),
        ("ru_overlap_accumulate", lambda: lib.ru_overlap_accumulate(d, 1, 3, 1, 2, d, None, None)),
        ("ru_overlap_accumulate", lambda: lib.ru_overlap_accumulate(d, 1, 3, 2, 4, d, d, None)),          # VALIDATE needs L = 4
        ("ru_overlap_accumulate", lambda: lib.ru_overlap_accumulate(d, 1, 4, 2, 4, d, None, None)),       # ... and an output
        ("ru_overlap_accumulate", lambda: lib.ru_overlap_accumulate(d, 1, 4, 7, 1, d, None, None)),
        ("ru_dice1d_accumulate", lambda: lib.ru_dice1d_accumulate(d, d, 1, 3, 4, None)),
        ("ru_dice1d_accumulate", lambda: lib.ru_dice1d_accumulate(None, d, 1, 3, 3, None)),
        ("ru_rmse_accumulate", lambda: lib.ru_rmse_accumulate(None, d, None)),
    ]
    for name, call in cases:
        rc = call()
        assert rc < 0, name
        assert name in L.last_error(), (name, L.last_error())


def test_metric_classes_have_the_reference_surface(golden):
    from brats2019_amd import metrics
    g = golden("overlap")
    for cls in CLASSES:
        ours = getattr(metrics, cls)
        assert issubclass(ours, metrics.Metrics)
        params = list(inspect.signature(ours.__init__).parameters.values())[1:]
        assert [p.name for p in params] == g["surface_%s_params" % cls].tolist(), cls
        assert [repr(p.default) for p in params] == g["surface_%s_defaults" % cls].tolist(), cls
        m = ours()
        # every attribute of the reference's instance but Dice_ITK's SimpleITK filter object
        want = set(g["surface_%s_attrs" % cls].tolist()) - {"overelap_measures_filter"}
        assert want <= set(vars(m)), (cls, want - set(vars(m)))
        assert m.accumulator == 0.0 and m.samples == 0.0
    assert metrics.RMSE().data_parallel is False
    for name in run_names(g):
        assert str(g["run_%s_name" % name]) in ("Dice1D", "RMSE", "RMSE_masked", "Dice_WT", "Dice_ITK"), name


def test_numpy_oracle_reproduces_the_reference_fixture(golden):
    g = golden("overlap")
    names = run_names(g)
    assert {"dice1d3", "dice1d2", "dice1d4", "rmse", "rmsemasked", "rmsemaskedbad", "wt", "wtnan", "itk5", "itk4", "itk3", "itk4c4"} <= set(names)
    for name in names:
        raised = str(g["run_%s_raises" % name])
        if raised:
            assert g["run_%s_values" % name].size == 0
            continue
        np.testing.assert_allclose(oracle_run(g, name), g["run_%s_values" % name], rtol=rtol_of(name), atol=0, err_msg=name)
    assert str(g["run_dice1d4_raises"]) == "IndexError"                   # Dice1D(classes=4) on 3 channels
    assert str(g["run_rmsemaskedbad_raises"]) == "RuntimeError"          # RMSE_masked on a regular shape
    assert np.isnan(g["run_itk5_values"][:, 2:]).all()                    # labels 3, 4 never occur with 3 channels
    # the nested targets tie everywhere: their argmax is 0, so the whole-tumour target is empty
    for b in range(4):
        assert (conf_prob(g["b%d_pred" % b], g["b%d_gr" % b])[:, :, 1:] == 0).all()


def test_numpy_oracle_reproduces_the_reference_validate(golden):
    g = golden("overlap")
    res = []
    for k in range(3):
        conf, invalid = conf_label(g["v%d_pred" % k][None], g["v%d_label" % k][None])
        assert invalid.tolist() == [0]
        res.append(validate_result(conf)[0])
    res = np.stack(res)
    np.testing.assert_array_equal(res, g["validate_results"])
    np.testing.assert_array_equal(res.sum(axis=0) / 3, g["validate_mean"])
    assert g["validate_results"][1, 2] == 1.0                             # label 4 absent on both sides: NaN -> 1


class _Writer(object):
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, float(value), step))


class _Fixed(object):
    def __init__(self, name, value):
        self.name, self.value = name, value

    def get(self):
        return self.value


def test_print_metrics_logs_like_the_reference(capsys):
    from brats2019_amd import metrics
    w = _Writer()
    metrics.print_metrics(w, _Fixed("Dice_ITK", np.array([0.25, 0.5, 0.75])), "val/", 3)
    assert w.calls == [("val/Dice_ITK0", 0.25, 3), ("val/Dice_ITK1", 0.5, 3), ("val/Dice_ITK2", 0.75, 3)]
    assert capsys.readouterr().out == "Epoch 3, val/ Dice_ITK %s\n" % np.array([0.25, 0.5, 0.75])
    w = _Writer()
    metrics.print_metrics(w, _Fixed("RMSE", np.float64(0.125)), "train/", 7)
    assert w.calls == [("train/RMSE", 0.125, 7)]
    assert capsys.readouterr().out == "Epoch 7, train/ RMSE 0.125\n"
