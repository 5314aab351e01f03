"""Ensemble inference, host side (no GPU): the numpy restatement kept in `brats2019_amd.inference` against the formula of the reference's
notebooks written out here (average_predicts.ipynb / emsemble_predicts.ipynb: `sum(data_files) / len(data_files)`, `np.argmax`, 3 -> 4)
and, for one model, against the oracle's `tta_merge`; the `ensemble` command line on `.npy` directories, host path, both rules."""
import numpy as np
import pytest

from oracle import resunet_oracle as O


def _model_outputs(rng, m, shape, shift=0.0):
    """m models x 4 flipped predictions [3, ...] in [0, 1]"""
    return [[np.clip(rng.random(shape).astype(np.float32) + np.float32(shift), 0, 1).astype(np.float32) for _ in range(4)] for _ in range(m)]


@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_host_restatement_is_the_notebook_formula(m):
    from brats2019_amd import inference as I
    rng = np.random.default_rng(100 + m)
    outs = _model_outputs(rng, m, (3, 8, 12, 16), shift=0.2)
    lo, size = (1, 2, 3), (6, 9, 11)
    sl = (slice(None),) + tuple(slice(a, a + s) for a, s in zip(lo, size))
    data_files = [O.tta_merge(o)[sl] for o in outs]                   # per model: test.py:134-140
    assert all(d.dtype == np.float32 for d in data_files)
    want = sum(data_files) / len(data_files)                          # the notebooks' line, verbatim
    assert want.dtype == np.float32
    mean, mask, counts = I.ensemble_merge_host(outs, lo, size)
    assert mean.dtype == np.float32 and np.array_equal(mean, want)
    assert np.array_equal(mask, want > 0.5) and counts == tuple(int(v) for v in (want > 0.5).sum(axis=(1, 2, 3)))
    assert np.array_equal(I.ensemble_mean_host(data_files), want)
    if m == 1:                                                        # the ensemble of one is today's merge
        full, _, _ = I.ensemble_merge_host(outs)
        assert np.array_equal(full, O.tta_merge(outs[0])) and np.array_equal(mean, O.tta_merge(outs[0])[sl])


def test_host_class_rule_is_the_notebook_formula():
    from brats2019_amd import inference as I
    rng = np.random.default_rng(7)
    data_files = [(rng.integers(0, 9, (4, 6, 7, 5)) / 8.0).astype(np.float32) for _ in range(3)]      # multiples of 1/8: ties occur
    prediction = sum(data_files) / len(data_files)
    labels = np.argmax(prediction, axis=0)
    assert ((prediction == prediction.max(axis=0)).sum(axis=0) > 1).mean() > 0.02
    labels[labels == 3] = 4
    got = I.ensemble_class_labels_host(data_files)
    assert got.dtype == np.uint8 and np.array_equal(got, labels) and set(np.unique(got).tolist()) == {0, 1, 2, 4}


def test_host_compose_labels_is_the_oracle_rule():
    from brats2019_amd import inference as I
    rng = np.random.default_rng(2)
    for et_scale in (1.0, 0.03):
        prob = rng.random((3, 9, 10, 11)).astype(np.float32) * np.array([1, 1, et_scale], np.float32).reshape(3, 1, 1, 1) + (0.3 if et_scale == 1.0 else 0.0)
        want, _ = O.compose_labels(prob)
        assert np.array_equal(I.compose_labels_host(prob), want)


@pytest.mark.parametrize("rule", ["class", "regions"])
def test_ensemble_command_line_host_path(tmp_path, rule):
    from brats2019_amd import ensemble as E, inference as I
    rng = np.random.default_rng(3)
    c = 4 if rule == "class" else 3
    dirs, cases = [], {"case_a": (10, 12, 9), "case_b": (7, 8, 11)}
    preds = {k: [] for k in cases}
    for m in range(3):
        d = tmp_path / ("model%d" % m)
        d.mkdir()
        dirs.append(str(d))
        for name, shape in cases.items():
            p = rng.random((c,) + shape).astype(np.float32)
            if rule == "regions":
                p[:, 2:6, 2:7, 3:8] += 0.4                            # a blob that survives the component rejection
            np.save(d / (name + ".npy"), p)
            preds[name].append(p)
    E.main(["--predictions"] + dirs + ["--output", str(tmp_path / "out"), "--rule", rule, "--host"])
    for name in cases:
        got = np.load(tmp_path / "out" / (name + ".npy"))
        mean = sum(preds[name]) / len(preds[name])
        if rule == "class":
            want = np.argmax(mean, axis=0).astype(np.uint8)
            want[want == 3] = 4
        else:
            want, _ = O.postprocess(mean)
        assert got.dtype == np.uint8 and got.shape == cases[name] and np.array_equal(got, want)
        assert len(np.unique(got)) > 1
    with pytest.raises(SystemExit):                                   # a class map handed to the region rule is refused, not reinterpreted
        E.main(["--predictions"] + dirs + ["--output", str(tmp_path / "bad"), "--rule", "regions" if rule == "class" else "class", "--host"])
