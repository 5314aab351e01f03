"""Host side of the uncertainty maps and the BraTS uncertainty score (csrc/uncertainty.hip): the numpy oracles the device tests
(tests/test_uncertainty.py) import, the `inference.uncertainty_*_host` helpers and the score's arithmetic held to them on small cases,
and the declarations.  The score oracle is brute force: per threshold it really filters the voxels and recounts; it never sees a
histogram."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
REGION_LABELS = ((1, 2, 3, 4), (1, 3, 4), (3, 4))          # WT, TC, ET, as validate --regions
FLIPS = ((), (1,), (2,), (1, 2))


# ---------------------------------------------------------------------- oracles
def oracle_mean(members):
    """members[m][k] float32 -> the library's float32 ensemble mean: (((o0+o1)+o2)+o3)/K per model, S_m = S_(m-1) + p_m, / (float)M"""
    total = None
    for copies in members:
        s = copies[0].astype(np.float32)
        for o in copies[1:]:
            s = s + o
        p = s / np.float32(len(copies))
        total = p if total is None else total + p
    assert total.dtype == np.float32
    return total / np.float32(len(members))


def oracle_second_moment(members):
    total = None
    for copies in members:
        q = copies[0] * copies[0]
        for o in copies[1:]:
            q = q + o * o                                   # numpy rounds the product, then the sum: no fma
        total = q if total is None else total + q
    assert total.dtype == np.float32
    return total


def oracle_std(members):
    m, k = len(members), len(members[0])
    e2 = oracle_second_moment(members).astype(np.float64) / np.float64(m * k)
    mu = oracle_mean(members).astype(np.float64)
    var = np.maximum(e2 - mu * mu, 0.0)
    return np.floor(np.minimum(200.0 * np.sqrt(var), 100.0) + 0.5).astype(np.uint8)


def oracle_entropy_real(mean):
    """100*H + 0.5 in float64, before the floor: the device tests need its distance to an integer"""
    mu = np.asarray(mean, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where((mu == 0.0) | (mu == 1.0), 0.0, mu * np.log2(mu))
        b = np.where((mu == 0.0) | (mu == 1.0), 0.0, (1.0 - mu) * np.log2(1.0 - mu))
    return 100.0 * -(a + b) + 0.5


def oracle_entropy(mean):
    return np.floor(oracle_entropy_real(mean)).astype(np.uint8)


def oracle_score(pred, target, maps, thresholds):
    """brute force: float64 [3, 4] = per region (score, AUC_Dice, AUC_FTP, AUC_FTN)"""
    out = np.zeros((3, 4))
    for r, labels in enumerate(REGION_LABELS):
        p, g, u = np.isin(pred, labels), np.isin(target, labels), maps[r]
        tp100, tn100 = int((p & g).sum()), int((~p & ~g).sum())
        dice, ftp, ftn = [], [], []
        for t in thresholds:
            keep = u <= t
            pk, gk = p[keep], g[keep]
            tp, fp, fn, tn = int((pk & gk).sum()), int((pk & ~gk).sum()), int((~pk & gk).sum()), int((~pk & ~gk).sum())
            den = 2 * tp + fp + fn
            dice.append(2 * tp / den if den else 1.0)
            ftp.append((tp100 - tp) / tp100 if tp100 else 0.0)
            ftn.append((tn100 - tn) / tn100 if tn100 else 0.0)
        aucs = []
        for curve in (dice, ftp, ftn):
            if len(thresholds) == 1:
                aucs.append(curve[0])
            else:
                area = sum((thresholds[i + 1] - thresholds[i]) * (curve[i] + curve[i + 1]) / 2.0 for i in range(len(thresholds) - 1))
                aucs.append(area / (thresholds[-1] - thresholds[0]))
        out[r] = ((aucs[0] + (1.0 - aucs[1]) + (1.0 - aucs[2])) / 3.0,) + tuple(aucs)
    return out


def oracle_histogram(pred, target, maps):
    """int64 [3, 101, 4] by bincount, classes TP, FP, FN, TN; inputs valid"""
    hist = np.zeros((3, 101, 4), np.int64)
    for r, labels in enumerate(REGION_LABELS):
        p, g = np.isin(pred, labels), np.isin(target, labels)
        cls = 3 - 2 * p.astype(np.int64) - g.astype(np.int64)
        hist[r] = np.bincount((maps[r].astype(np.int64) * 4 + cls).ravel(), minlength=404).reshape(101, 4)
    return hist


def score_from_histogram(hist, thresholds):
    """the arithmetic of unc_score_kernel on the host: cumulative sums over the map value, then the curves"""
    out = np.zeros((3, 4))
    for r in range(3):
        cum = np.cumsum(hist[r], axis=0)
        tp100, tn100 = int(cum[100, 0]), int(cum[100, 3])
        curves = [[], [], []]
        for t in thresholds:
            tp, fp, fn, tn = (int(v) for v in cum[t])
            den = 2 * tp + fp + fn
            curves[0].append(2 * tp / den if den else 1.0)
            curves[1].append((tp100 - tp) / tp100 if tp100 else 0.0)
            curves[2].append((tn100 - tn) / tn100 if tn100 else 0.0)
        aucs = []
        for c in curves:
            area = 0.0
            for i in range(1, len(thresholds)):
                area += (thresholds[i] - thresholds[i - 1]) * (c[i - 1] + c[i]) / 2.0
            aucs.append(area / (thresholds[-1] - thresholds[0]) if len(thresholds) > 1 else c[0])
        out[r] = ((aucs[0] + (1.0 - aucs[1]) + (1.0 - aucs[2])) / 3.0,) + tuple(aucs)
    return out


# ---------------------------------------------------------------------- inputs shared with the device tests
def random_members(rng, m, k, shape):
    """m x k un-flipped members: uniform float32 clipped to [0, 1]"""
    return [[np.clip(rng.random(shape).astype(np.float32) * np.float32(1.2) - np.float32(0.1), 0, 1).astype(np.float32) for _ in range(k)] for _ in range(m)]


def negative_variance_members(rng, m, k, shape):
    """all m x k members equal: the variance is 0, and where the float32 squares rounded down e2 - mu*mu comes out slightly negative.
    -> (members, bool array of those voxels)"""
    v = rng.random(shape).astype(np.float32)
    members = [[v] * k] * m
    mu = oracle_mean(members).astype(np.float64)
    return members, oracle_second_moment(members).astype(np.float64) / np.float64(m * k) - mu * mu < 0


def blob_labels(rng, shape, nblobs=3):
    """a label volume {0,1,2,4}: nested spheres of labels 2, 1, 4 around a few centres"""
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    lab = np.zeros(shape, np.uint8)
    centres = [[rng.uniform(0.2 * s, 0.8 * s) for s in shape] for _ in range(nblobs)]
    radii = rng.uniform(0.08, 0.2, size=nblobs) * min(shape)
    for value, scale in [(2, 2.5), (1, 1.6), (4, 1.0)]:
        for c, r in zip(centres, radii):
            lab[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= (scale * max(r, 1.0)) ** 2] = value
    return lab


def boundary_maps(rng, pred, every_level=False):
    """uint8 [3, ...] maps: zero away from the tumour, random 0..100 on a band around each region of `pred`"""
    from scipy import ndimage
    maps = np.zeros((3,) + pred.shape, np.uint8)
    for r, labels in enumerate(REGION_LABELS):
        p = np.isin(pred, labels)
        band = ndimage.binary_dilation(p, iterations=2) & ~ndimage.binary_erosion(p, iterations=2)
        maps[r][band] = rng.integers(0, 101, size=int(band.sum()), dtype=np.uint8)
    if every_level:
        flat = maps.reshape(3, -1)
        for r in range(3):
            flat[r, rng.choice(flat.shape[1], 101, replace=False)] = np.arange(101, dtype=np.uint8)
    return maps


def small_case(rng, shape=(9, 11, 13)):
    target = blob_labels(rng, shape)
    pred = np.roll(target, 1, axis=2)
    return pred, target, boundary_maps(rng, pred)


# ---------------------------------------------------------------------- tests
def test_host_helpers_equal_the_oracles():
    from brats2019_amd import inference as I
    rng = np.random.default_rng(1)
    for m, k in [(1, 4), (3, 4), (5, 1), (2, 3)]:
        members = random_members(rng, m, k, (3, 5, 6, 7))
        mean = oracle_mean(members)
        np.testing.assert_array_equal(I.second_moment_host(members), oracle_second_moment(members))
        np.testing.assert_array_equal(I.uncertainty_std_host(members), oracle_std(members))
        np.testing.assert_array_equal(I.uncertainty_std_host(members, mean), oracle_std(members))
        np.testing.assert_array_equal(I.uncertainty_entropy_host(mean), oracle_entropy(mean))
        assert I.uncertainty_std_host(members).dtype == np.uint8 and I.uncertainty_std_host(members).max() <= 100


def test_members_host_matches_ensemble_merge_host():
    """the helper's members are the arrays `ensemble_merge_host` averages: un-flipped, restricted to the box"""
    from brats2019_amd import inference as I
    rng = np.random.default_rng(2)
    outs = [[rng.random((3, 6, 8, 10)).astype(np.float32) for _ in FLIPS] for _ in range(3)]
    lo, size = (1, 2, 3), (4, 5, 6)
    members = I._members_host(outs, lo, size)
    mean, _, _ = I.ensemble_merge_host(outs, lo, size)
    np.testing.assert_array_equal(oracle_mean(members), mean)
    np.testing.assert_array_equal(members[1][3], np.flip(outs[1][3], axis=(1, 2))[:, 1:5, 2:7, 3:9])


def test_measures_at_exact_values():
    from brats2019_amd import inference as I
    same = [[np.full((2, 3), 0.3, np.float32)] * 4] * 3
    assert not I.uncertainty_std_host(same).any()
    split = [[np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32)] * 2] * 2
    assert (I.uncertainty_std_host(split) == 100).all()
    np.testing.assert_array_equal(I.uncertainty_entropy_host(np.array([0.0, 1.0, 0.5], np.float32)), [0, 0, 100])
    # float32 sums that make e2 - mu*mu slightly negative: clamped to 0, not NaN
    equal, negative = negative_variance_members(np.random.default_rng(7), 3, 4, (4096,))
    assert negative.sum() > 100 and not I.uncertainty_std_host(equal)[negative].any()


def test_score_arithmetic_equals_brute_force():
    rng = np.random.default_rng(3)
    for thresholds in [(25, 50, 75, 100), (0, 100), (10, 20, 30, 40, 50, 60, 70, 80, 90, 100), (5, 37, 99), (50,)]:
        pred, target, maps = small_case(rng)
        hist = oracle_histogram(pred, target, maps)
        assert hist.sum() == 3 * pred.size
        np.testing.assert_allclose(score_from_histogram(hist, thresholds), oracle_score(pred, target, maps, thresholds), rtol=1e-12, atol=0)


DEGENERATE = ["empty-gt", "empty-pred", "all-uncertain", "all-certain", "tp100-zero", "single-threshold"]


def degenerate_case(kind, rng):
    pred, target, maps = small_case(rng)
    thresholds = (25, 50, 75, 100)
    if kind == "empty-gt":
        target = np.zeros_like(target)
    elif kind == "empty-pred":
        pred = np.zeros_like(pred)
    elif kind == "all-uncertain":
        maps = np.full_like(maps, 100)
    elif kind == "all-certain":
        maps = np.zeros_like(maps)
    elif kind == "tp100-zero":
        target = np.where(pred > 0, 0, 2).astype(np.uint8)         # disjoint: no true positive anywhere
    elif kind == "single-threshold":
        thresholds = (75,)
    return pred, target, maps, thresholds


@pytest.mark.parametrize("kind", DEGENERATE)
def test_score_degenerate_cases(kind):
    pred, target, maps, thresholds = degenerate_case(kind, np.random.default_rng(4))
    want = oracle_score(pred, target, maps, thresholds)
    assert np.isfinite(want).all() and (want >= 0).all() and (want <= 1).all()
    np.testing.assert_allclose(score_from_histogram(oracle_histogram(pred, target, maps), thresholds), want, rtol=1e-12, atol=0)
    if kind == "all-certain":                                          # nothing is ever filtered: FTP = FTN = 0, the Dice is the plain one
        assert not want[:, 2:].any()
    if kind == "all-uncertain":                                        # everything is filtered below 100: Dice 1 there by the empty rule
        assert (want[:, 2] > 0.8).all() and (want[:, 3] > 0.8).all()
    if kind in ("tp100-zero", "empty-gt", "empty-pred"):
        assert not want[:, 2].any()                                    # FTP is 0 when nothing can be filtered


def test_header_and_ctypes_table_declare_the_uncertainty_entries():
    from brats2019_amd import _lib as L
    text = open(HEADER).read()
    for name in ("ru_unc_accumulate", "ru_unc_accumulate_finalize", "ru_unc_finalize", "ru_unc_histogram", "ru_unc_score", "ru_paste_u8c"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
        assert hasattr(L.load(), name), name
    assert re.search(r"#define RU_UNC_STD 0\b", text) and re.search(r"#define RU_UNC_ENTROPY 1\b", text)
    assert L.UNC_MEASURES == {"std": 0, "entropy": 1}


def test_keywords_and_flags_are_opt_in():
    import inspect
    from brats2019_amd import ensemble, inference as I, test as entry, validate
    for fn in (I.predict_case, I.predict_case_device, I.predict_case_ensemble, I.predict_case_ensemble_device, I.ensemble_merge):
        assert inspect.signature(fn).parameters["uncertainty"].default is None, fn.__name__
    with pytest.raises(ValueError, match="uncertainty"):
        I.ensemble_merge([None], (0, 0, 0), (1, 1, 1), uncertainty="variance")
    plain = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b"])
    assert not hasattr(plain, "uncertainty_path") and not hasattr(plain, "thresholds")
    got = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b", "--uncertainty_path", "c", "--thresholds", "10", "90"])
    assert got.uncertainty_path == "c" and got.thresholds == [10, 90]
    assert not hasattr(ensemble.parser.parse_args(["--predictions", "a", "--output", "b"]), "uncertainty_output")
    assert not hasattr(entry.parser.parse_args([]), "uncertainty") and not hasattr(entry.parser.parse_args([]), "uncertainty_output")
    assert I.UNCERTAINTY_STEMS == ("whole", "core", "enhance")


def test_score_uncertainty_reports_bad_input_before_any_upload():
    from brats2019_amd import validate
    lab = np.zeros((3, 4, 5), np.uint8)
    with pytest.raises(ValueError, match="case0"):
        validate.score_uncertainty([("case0", lab, lab, np.zeros((3, 3, 4, 6), np.uint8))])
    with pytest.raises(ValueError, match="case1"):
        validate.score_uncertainty([("case1", lab, lab, np.full((3, 3, 4, 5), 101, np.int32))])
    with pytest.raises(ValueError, match="thresholds"):
        validate.score_uncertainty([], thresholds=(50, 25))


def test_ensemble_host_route_writes_the_three_files(tmp_path):
    """`ensemble --host --uncertainty_output`: saved region probabilities are members with K = 1"""
    from brats2019_amd import ensemble, inference as I
    rng = np.random.default_rng(6)
    preds = [np.clip(rng.random((3, 6, 7, 8)).astype(np.float32), 0, 1) for _ in range(3)]
    for i, p in enumerate(preds):
        os.makedirs(tmp_path / ("run%d" % i))
        np.save(tmp_path / ("run%d" % i) / "caseA.npy", p)
    ensemble.main(["--predictions"] + [str(tmp_path / ("run%d" % i)) for i in range(3)] + ["--output", str(tmp_path / "out"), "--rule", "regions", "--host",
                                                                                          "--uncertainty_output", str(tmp_path / "unc")])
    want = oracle_std([[p] for p in preds])
    for r, stem in enumerate(I.UNCERTAINTY_STEMS):
        got = np.load(tmp_path / "unc" / ("caseA_unc_%s.npy" % stem))
        assert got.dtype == np.uint8 and got.shape == (6, 7, 8)
        np.testing.assert_array_equal(got, want[r])
    assert want.any()
