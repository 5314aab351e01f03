"""Host-side checks of the calibration scorer and the threshold search (no GPU needed): the numpy restatement
(metrics.calibration_host) against a direct sweep of `p > b / NB` masks and a plain float64 computation of ECE, MCE and Brier; the bin
function at its edges; the declarations of the four entry points; and `python -m brats2019_amd.validate --calibration --host` end to end.
The input families below are shared with tests/test_calibration.py, which holds the device to the restatement."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
ENTRIES = ("ru_calib_histogram", "ru_calib_accumulate", "ru_calib_summary", "ru_threshold_regions")
FAMILIES = ("uniform", "saturated", "edges", "invalid", "empty", "full")
TRIVIAL_OK = ("saturated", "empty", "full")         # declared exceptions of the three-bins-per-class rule: saturated in every channel, empty / full in channel 0


# ---------------------------------------------------------------------- input families (shared with tests/test_calibration.py)
def edge_values(nb):
    """k / nb and its float32 neighbours for several k, and the ends of the range"""
    ks = np.array([0, 1, 2, nb // 2 - 1, nb // 2, nb // 2 + 1, nb - 1, nb], np.float32) / np.float32(nb)
    vals = np.concatenate([ks, np.nextafter(ks, np.float32(2)), np.nextafter(ks, np.float32(-1))]).astype(np.float32)
    return np.concatenate([vals[(vals >= 0) & (vals <= 1)], np.array([0.0, -0.0, 1.0, 1e-40, 2.0 ** -24, 2.0 ** -25], np.float32)])


def make_case(family, shape, seed=0, nb=256):
    """(pred, target) float32 [N, C, V] of one family"""
    rng = np.random.default_rng(seed)
    n, c, v = shape
    pred = rng.random(shape, dtype=np.float32)
    target = (rng.random(shape, dtype=np.float32) < pred).astype(np.float32)              # a calibrated target
    if family == "saturated":
        tiny = np.float32(2.0 ** -20)
        u = rng.random(shape)
        pred = np.select([u < 0.80, u < 0.93, u < 0.97], [np.float32(0), tiny, np.float32(1) - tiny], np.float32(1)).astype(np.float32)
        target = (pred > 0.5).astype(np.float32)
        flip = rng.random(shape) < 0.01
        target[flip] = 1 - target[flip]
    elif family == "edges":
        e = edge_values(nb)
        idx = rng.choice(pred.size, size=min(pred.size // 2, 4 * len(e)), replace=False)
        pred.reshape(-1)[idx] = np.resize(e, len(idx))
    elif family == "invalid":
        bad = np.array([np.nan, -1e-30, -1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, np.inf, -np.inf], np.float32)
        idx = rng.choice(pred.size, size=min(pred.size // 3, 3 * len(bad)), replace=False)
        pred.reshape(-1)[idx] = np.resize(bad, len(idx))
        target.reshape(-1)[rng.choice(pred.size, size=max(1, pred.size // 50), replace=False)] = np.nan
        target.reshape(-1)[idx[:2]] = np.nan                                          # both tensors invalid at one voxel: counted once
    elif family == "empty":
        target[:, 0] = 0
    elif family == "full":
        target[:, 0] = 1
    return pred, target


def make_label_case(shape, seed=0):
    """(pred float32 [N, 3, V], uint8 label volume [N, V]) with the labels 0..4 and one invalid label"""
    rng = np.random.default_rng(seed)
    n, _, v = shape
    pred = rng.random((n, 3, v), dtype=np.float32)
    label = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4], np.uint8), size=(n, v))
    label[0, v // 2] = 7
    return pred, label


def distinct_bins(hist):
    """the smallest number of non-empty bins over (sample, channel, class)"""
    return int((np.asarray(hist) > 0).sum(axis=-2).min())


# ---------------------------------------------------------------------- a direct numpy sweep, written apart from the restatement
def sweep(pred, target, t):
    """Dice, Sens, Spec of the masks pred > t against target > 0.5 over the valid voxels of one (sample, channel) row"""
    with np.errstate(invalid="ignore"):
        ok = (pred >= 0) & (pred <= 1) & ~np.isnan(target)
    p, g = pred[ok] > np.float32(t), target[ok] > 0.5
    tp, fp, fn, tn = int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum()), int((~p & ~g).sum())
    d = 2 * tp + fp + fn
    return (np.float64(2 * tp) / np.float64(d) if d else 1.0, np.float64(tp) / np.float64(tp + fn) if tp + fn else 1.0,
            np.float64(tn) / np.float64(tn + fp) if tn + fp else 1.0)


def plain_summary(pred, target, m):
    """ECE, MCE, Brier in plain float64 numpy on p rounded down to r / 2^24, pooled over the samples of one channel"""
    pred, target = pred.reshape(-1).astype(np.float64), target.reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (pred >= 0) & (pred <= 1) & ~np.isnan(target)
    p, y = np.floor(pred[ok] * 2.0 ** 24) / 2.0 ** 24, (target[ok] > 0.5).astype(np.float64)
    q = pred[ok]                                                                       # the coarse bin comes from p itself: ceil(p * m) - 1, 0 for p = 0
    b = np.maximum(np.ceil(q * m).astype(np.int64), 1) - 1
    ece, mce = 0.0, 0.0
    for k in range(m):
        s = b == k
        if s.any():
            gap = abs(y[s].mean() - p[s].mean())
            ece += s.sum() / len(p) * gap
            mce = max(mce, gap)
    return ece, mce, float(np.mean((p - y) ** 2)) if len(p) else 0.0


# ---------------------------------------------------------------------- tests
@pytest.mark.parametrize("nb", [16, 256, 1024])
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_a_direct_sweep(family, nb):
    from brats2019_amd import metrics
    shape = (2, 3, 17 * 19 * 5)
    pred, target = make_case(family, shape, seed=3, nb=nb)
    h = metrics.calibration_host(pred, target, nb, 16)
    nbins = distinct_bins(h["hist"])
    print(family, nb, "distinct bins per class >=", nbins, "invalid", h["invalid"].tolist())
    assert nbins >= 3 or family in TRIVIAL_OK, "a trivial table would pass anything"
    if family in TRIVIAL_OK and family != "saturated":
        assert distinct_bins(h["hist"][:, 1:]) >= 3                                    # only channel 0 is the exception
    assert (h["hist"].sum(axis=(2, 3)) + h["invalid"] == shape[2]).all()
    assert (h["invalid"] > 0).all() == (family == "invalid")
    for b in sorted({0, 1, 2, nb // 4, nb // 2 - 1, nb // 2, nb // 2 + 1, 3 * nb // 4, nb - 2, nb - 1, nb, 5}):
        for n in range(shape[0]):
            for c in range(shape[1]):
                want = sweep(pred[n, c], target[n, c], b / nb)
                assert tuple(h["curves"][n, c, :, b]) == want, (family, nb, b, n, c)
    for c in range(shape[1]):
        ece, mce, brier = plain_summary(pred[:, c], target[:, c], 16)
        got = h["summary"][c]
        print(family, nb, c, "ECE", got[0], ece, "MCE", got[1], mce, "Brier", got[2], brier)
        assert abs(got[0] - ece) <= 1e-12 and abs(got[1] - mce) <= 1e-12 and abs(got[2] - brier) <= 1e-12
        assert got[5] == h["hist"][:, c].sum() and got[6] == (h["table"][c, :, 0] > 0).sum()


def test_label_targets_follow_the_regions():
    from brats2019_amd import metrics
    pred, label = make_label_case((2, 3, 4099), seed=5)
    h = metrics.calibration_host(pred, label, 256, 16)
    assert distinct_bins(h["hist"]) >= 3
    assert h["invalid"].tolist() == [[1, 1, 1], [0, 0, 0]]
    ok = label <= 4
    for c, members in enumerate(((1, 2, 3, 4), (1, 3, 4), (3, 4))):
        g = np.isin(label, members).astype(np.float32)
        g[~ok] = np.nan
        ref = metrics.calibration_host(pred[:, c:c + 1], g[:, None], 256, 16)
        for key in ("hist", "conf", "sq", "invalid"):
            assert np.array_equal(h[key][:, c:c + 1], ref[key]), (c, key)


def test_bin_function_at_the_edges():
    from brats2019_amd import metrics
    nb = 256
    f = lambda x: np.float32(x)
    up, down = lambda x: np.nextafter(f(x), f(2)), lambda x: np.nextafter(f(x), f(-1))
    cases = [(f(0.0), 0), (f(-0.0), 0), (f(1.0), nb), (f(1e-40), 1), (f(2.0 ** -149), 1), (down(1.0), nb), (up(0.0), 1)]
    for k in (1, 2, 127, 128, 129, 255):
        cases += [(f(k / nb), k), (up(k / nb), k + 1), (down(k / nb), k)]
    for x, k in cases:
        hist = metrics.calibration_tables_host(np.array([[[x]]], np.float32), np.ones((1, 1, 1), np.float32), nb)[0]
        assert hist[0, 0, k, 1] == 1 and hist.sum() == 1, (x, k, np.flatnonzero(hist[0, 0, :, 1]))
        # the mask rule the bins stand for: p > b / nb <=> k > b
        for b in (k - 1, k):
            if 0 <= b <= nb:
                assert (x > f(b / nb)) == (k > b), (x, b)
    for x in (np.nan, -1e-30, -1.0, up(1.0), np.inf, -np.inf):
        hist, conf, sq, inv = metrics.calibration_tables_host(np.array([[[x]]], np.float32), np.ones((1, 1, 1), np.float32), nb)
        assert hist.sum() == 0 and conf.sum() == 0 and sq.sum() == 0 and inv[0, 0] == 1, x
    # the fixed-point confidence: exact on [0.5, 1], truncated below
    conf = lambda x: int(metrics.calibration_tables_host(np.array([[[x]]], np.float32), np.ones((1, 1, 1), np.float32), nb)[1].sum())
    assert conf(f(1.0)) == 2 ** 24 and conf(f(0.5)) == 2 ** 23 and conf(down(1.0)) == 2 ** 24 - 1 and conf(f(2.0 ** -25)) == 0 and conf(f(0.3)) == int(np.floor(np.float64(f(0.3)) * 2 ** 24))


def test_threshold_choice_breaks_ties_towards_the_middle():
    from brats2019_amd.metrics import choose_threshold
    d = np.zeros(17)
    d[[0, 16]] = 9.0                                  # the ends are not candidates
    d[[3, 12]] = 0.5
    assert choose_threshold(d) == 12                  # |12 - 8| < |3 - 8|
    d[[6, 10]] = 0.5
    assert choose_threshold(d) == 6                   # equally close: the lower
    d[11] = 0.6
    assert choose_threshold(d) == 11
    assert choose_threshold(np.ones(17)) == 8


def test_header_ctypes_table_and_sources_declare_the_calibration_entries():
    from brats2019_amd import _lib as L, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    for macro, val in (("RU_CALIB_TARGET_REGIONS", L.CALIB_TARGET_REGIONS), ("RU_CALIB_TARGET_LABELS", L.CALIB_TARGET_LABELS), ("RU_CALIB_MIN_NB", L.CALIB_MIN_NB),
                       ("RU_CALIB_MAX_NB", L.CALIB_MAX_NB), ("RU_CALIB_DEFAULT_NB", L.CALIB_DEFAULT_NB), ("RU_CALIB_MAX_C", L.CALIB_MAX_C)):
        assert re.search(r"#define %s %d\b" % (macro, val), src), macro
    assert "calibration.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "calibration.hip"))


def test_validate_calibration_round_trip_on_the_host(tmp_path, capsys):
    from brats2019_amd import inference, metrics, validate
    rng = np.random.default_rng(11)
    labels_dir, probs_dir = tmp_path / "labels", tmp_path / "probs"
    labels_dir.mkdir()
    probs_dir.mkdir()
    cases = []
    for name in ("a", "b"):
        label = rng.choice(np.array([0, 0, 1, 2, 4], np.uint8), size=(6, 7, 9))
        truth = np.stack([np.isin(label, m) for m in metrics.BRATS_REGION_LABELS])
        probs = np.clip(np.where(truth, 0.62, 0.2) + rng.normal(0, 0.2, truth.shape), 0, 1).astype(np.float32) * np.float32(0.7)    # under-confident: the best threshold lies below 0.5
        np.save(labels_dir / (name + ".npy"), label)
        np.save(probs_dir / (name + ".npy"), probs)
        cases.append((name, label, probs))
    out = tmp_path / "thresholds.json"
    summary, thresholds = validate.main(["--data_path", str(labels_dir), "--probs_path", str(probs_dir), "--calibration", "--host", "--nb", "64", "--bins", "8",
                                         "--thresholds_output", str(out)])
    text = capsys.readouterr().out
    assert all(("%s ECE " % r) in text and ("%s bin  7" % r) in text for r in validate.REGION_NAMES)
    blob = json.loads(out.read_text())
    assert sorted(blob) == ["dice", "dice_at_half", "nb", "thresholds"] and blob["nb"] == 64 and blob["thresholds"] == list(thresholds)
    # the printed choice is the argmax of the mean of the per-case sweeps
    res = validate.score_calibration(cases, 64, 8, host=True)
    for c in range(3):
        mean = np.array([np.mean([sweep(p[c].reshape(-1), np.isin(l, metrics.BRATS_REGION_LABELS[c]).astype(np.float32).reshape(-1), b / 64)[0] for _, l, p in cases])
                         for b in range(65)])
        assert np.allclose(res["mean_curve"][c, 0], mean, rtol=0, atol=1e-15)
        assert res["best_bin"][c] == metrics.choose_threshold(mean) and blob["thresholds"][c] == res["best_bin"][c] / 64 < 0.5
        assert blob["dice"][c] >= blob["dice_at_half"][c] and blob["dice_at_half"][c] == res["mean_curve"][c, 0, 32]
    # the file is what the inference flags read
    import argparse
    parser = argparse.ArgumentParser()
    inference.add_threshold_arguments(parser)
    assert inference.thresholds_from_args(parser.parse_args(["--thresholds_file", str(out)])) == tuple(np.float32(t) for t in blob["thresholds"])
    assert inference.thresholds_from_args(parser.parse_args(["--thresholds", "0.25", "0.5", "0.75"])) == (0.25, 0.5, 0.75)
    assert inference.thresholds_from_args(parser.parse_args([])) is None
    with pytest.raises(ValueError):
        validate.score_calibration(cases, 48, 8, host=True)


def test_the_plain_validate_namespace_is_unchanged():
    from brats2019_amd import validate
    opt = validate.parser.parse_args(["--data_path", "x", "--predictions_path", "y"])
    assert vars(opt) == {"data_path": "x", "predictions_path": "y"}
