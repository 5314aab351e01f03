"""Lesion-wise Dice and HD95 (csrc/lesion.hip) without a GPU: the scipy oracle of the definition in INTEGRATION.md that
tests/test_lesion.py holds the device to; the facts about scipy's dilation and labelling that the device code relies on; hand-built cases
with values known in closed form; the C-ABI declarations; the metric classes' signatures; `validate --lesionwise`' argument handling.

Oracle: Dil = binary_dilation with the 18-neighbour structure; lesions = label(Dil(G)) with a 3 x 3 x 3 structure of ones, L_i = G & Z_i;
predicted components = label(P) likewise; M_i = the components that meet Z_i; HD95 as tests/test_surface_host.py computes it."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from test_surface_host import EMPTY, HEADER, oracle_hd95

S18 = ndimage.generate_binary_structure(3, 2)
S26 = np.ones((3, 3, 3), bool)


# ---------------------------------------------------------------------- oracle
def dilate(a, iterations):
    return a.copy() if iterations == 0 else ndimage.binary_dilation(a, S18, iterations=iterations)


def oracle_lesions(p, g, dilation=3, min_volume=50, empty_value=EMPTY):
    """one pair of masks -> ((LesionDice, LesionHD95), (n_gt, n_kept, n_tp, n_fn, n_fp), rows float64 [n_gt, 5] = (vol_i, |M_i|, tp_i,
    Dice_i, HD95_i)): steps 1-8 of the definition"""
    z, n = ndimage.label(dilate(g, dilation), S26)
    q, m = ndimage.label(p, S26)
    matched = np.zeros(m + 1, bool)
    rows = []
    for i in range(1, n + 1):
        zi = z == i
        li = g & zi
        js = np.unique(q[zi])
        js = js[js > 0]
        matched[js] = True
        mi = np.isin(q, js) & p
        vol, msz, tp = int(li.sum()), int(mi.sum()), int((mi & li).sum())
        assert vol > 0 and tp == int((p & li).sum())
        rows.append((vol, msz, tp, 2 * tp / (msz + vol), oracle_hd95(mi, li, empty_value)))
    n_fp = m - int(matched[1:].sum())
    kept = [r for r in rows if r[0] > min_volume]
    sd = sh = 0.0
    for r in kept:
        sd += r[3]
        sh += r[4]
    den = len(kept) + n_fp
    n_tp = sum(1 for r in kept if r[1] > 0)
    summary = (sd / den, (sh + n_fp * empty_value) / den) if den else (1.0, 0.0)
    return summary, (n, len(kept), n_tp, len(kept) - n_tp, n_fp), np.array(rows, dtype=np.float64).reshape(-1, 5)


def oracle_lesion_batch(pm, gm, **kw):
    """masks [N, K, D, H, W] -> (summary float64 [N, K, 2], counts int64 [N, K, 5], rows[n][k] float64 [n_gt, 5])"""
    n, k = pm.shape[:2]
    res = [[oracle_lesions(pm[i, j], gm[i, j], **kw) for j in range(k)] for i in range(n)]
    return (np.array([[r[0] for r in row] for row in res], dtype=np.float64), np.array([[r[1] for r in row] for row in res], dtype=np.int64),
            [[r[2] for r in row] for row in res])


def cube(shape, lo, size):
    a = np.zeros(shape, bool)
    a[tuple(slice(l, l + s) for l, s in zip(lo, size))] = True
    return a


# ---------------------------------------------------------------------- what the device code relies on
def test_a_component_of_the_dilated_mask_is_the_dilation_of_its_lesion():
    rng = np.random.default_rng(3)
    for shape, it in [((14, 15, 40), 3), ((9, 20, 21), 2), ((1, 30, 30), 3), ((12, 12, 12), 1)]:
        g = rng.random(shape) < 0.004
        g[0, 0, 0] = g[-1, -1, -1] = True
        z, n = ndimage.label(dilate(g, it), S26)
        assert n >= 2
        for i in range(1, n + 1):
            li = g & (z == i)
            assert li.any() and np.array_equal(z == i, dilate(li, it))


def test_label_numbers_components_by_ascending_smallest_index():
    rng = np.random.default_rng(4)
    a = rng.random((9, 17, 33)) < 0.03
    lab, n = ndimage.label(a, S26)
    firsts = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, n + 1)]
    assert n > 20 and firsts == sorted(firsts)
    # a U whose arms start before its base: the component that starts first is number 1 although it closes last
    u = np.zeros((1, 5, 7), bool)
    u[0, 0:5, 1] = u[0, 0:5, 5] = u[0, 4, 1:6] = True
    u[0, 0, 3] = True
    lab, n = ndimage.label(u, S26)
    assert n == 2 and lab[0, 0, 1] == lab[0, 0, 5] == 1 and lab[0, 0, 3] == 2


def test_three_iterations_of_the_18_structure_from_one_voxel():
    a = np.zeros((9, 9, 9), bool)
    a[4, 4, 4] = True
    d = dilate(a, 3)
    at = lambda o: bool(d[4 + o[0], 4 + o[1], 4 + o[2]])
    assert at((2, 2, 2)) and at((3, 3, 0)) and at((3, 2, 1)) and not at((3, 3, 3)) and not at((3, 2, 2))
    assert int(d.sum()) == 263
    assert int(S18.sum()) == 19 and S18[1, 1, 1] and not S18[0, 0, 0] and S18[0, 0, 1]
    assert np.array_equal(dilate(a, 0), a)
    corner = np.zeros((4, 4, 4), bool)
    corner[0, 0, 0] = True                                              # outside the grid is background: nothing wraps
    assert int(dilate(corner, 1).sum()) == 7


# ---------------------------------------------------------------------- closed-form cases
SHAPE = (12, 14, 40)


def two_cubes():
    return cube(SHAPE, (1, 1, 1), (4, 4, 4)), cube(SHAPE, (6, 8, 30), (4, 4, 4))              # 64 voxels each, far apart


def test_perfect_prediction():
    a, b = two_cubes()
    summary, counts, rows = oracle_lesions(a | b, a | b)
    assert summary == (1.0, 0.0) and counts == (2, 2, 2, 0, 0)
    assert rows.tolist() == [[64, 64, 64, 1.0, 0.0]] * 2


def test_one_missed_lesion():
    a, b = two_cubes()
    summary, counts, rows = oracle_lesions(a, a | b)
    assert summary == (0.5, EMPTY / 2) and counts == (2, 2, 1, 1, 0)
    assert rows[1].tolist() == [64, 0, 0, 0.0, EMPTY]


def test_one_distant_speck():
    a, b = two_cubes()
    p = a | b
    p[11, 0, 20] = True
    summary, counts, _ = oracle_lesions(p, a | b)
    assert summary == (2 / 3, EMPTY / 3) and counts == (2, 2, 2, 0, 1)
    p[11, 1, 21] = True                                                 # 26-adjacent: still one component
    assert oracle_lesions(p, a | b)[1] == (2, 2, 2, 0, 1)


def test_fifty_voxels_are_dropped_and_fifty_one_kept():
    small = cube(SHAPE, (1, 1, 1), (2, 5, 5))                          # exactly 50
    big = cube(SHAPE, (6, 8, 30), (2, 5, 5))
    big[8, 8, 30] = True                                                # exactly 51
    g = small | big
    summary, counts, rows = oracle_lesions(g, g)
    assert rows[:, 0].tolist() == [50, 51] and summary == (1.0, 0.0) and counts == (2, 1, 1, 0, 0)
    # a prediction of the dropped lesion alone: what it matched is no false positive, the kept lesion is missed
    summary, counts, rows = oracle_lesions(small, g)
    assert summary == (0.0, EMPTY) and counts == (2, 1, 0, 1, 0) and rows[0].tolist() == [50, 50, 50, 1.0, 0.0]
    assert oracle_lesions(g, g, min_volume=51)[1] == (2, 0, 0, 0, 0) and oracle_lesions(g, g, min_volume=51)[0] == (1.0, 0.0)
    assert oracle_lesions(g, g, min_volume=0)[1] == (2, 2, 2, 0, 0)


def test_both_masks_empty_and_an_empty_ground_truth_with_two_specks():
    z = np.zeros(SHAPE, bool)
    assert oracle_lesions(z, z) == ((1.0, 0.0), (0, 0, 0, 0, 0), pytest.approx(np.zeros((0, 5))))
    p = z.copy()
    p[2, 2, 2] = p[9, 9, 30] = True
    summary, counts, rows = oracle_lesions(p, z)
    assert summary == (0.0, EMPTY) and counts == (0, 0, 0, 0, 2) and rows.shape == (0, 5)
    assert oracle_lesions(p, z, empty_value=100.0)[0] == (0.0, 100.0)


def test_fragments_joined_by_the_dilation_are_one_lesion_and_a_bridge_is_counted_twice():
    g = np.zeros(SHAPE, bool)
    g[5, 5, 5:8] = g[5, 5, 14:17] = True                                # 6 voxels of background between: one lesion
    assert oracle_lesions(g, g, min_volume=0)[1][0] == 1
    g2 = np.zeros(SHAPE, bool)
    g2[5, 5, 5:8] = g2[5, 5, 15:18] = True                              # 7 between: two
    assert oracle_lesions(g2, g2, min_volume=0)[1][0] == 2
    p = np.zeros(SHAPE, bool)
    p[5, 5, 5:18] = True                                                # one component over both lesions: in both M_i
    summary, counts, rows = oracle_lesions(p, g2, min_volume=0)
    assert counts == (2, 2, 2, 0, 0) and rows[:, 1].tolist() == [13, 13] and rows[:, 3].tolist() == [6 / 16, 6 / 16]


# ---------------------------------------------------------------------- the interface, without a device
def test_header_and_ctypes_table_declare_the_lesion_entries():
    from brats2019_amd import _lib as L
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ru_lesion_workspace_bytes", "ru_lesion_metrics", "ru_lesion_accumulate"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    for macro, value in [("RU_LESION_DICE", L.LESION_COLUMNS["dice"]), ("RU_LESION_HD95", L.LESION_COLUMNS["hd95"]), ("RU_LESION_COUNTS", L.LESION_COUNTS),
                         ("RU_LESION_COLUMNS", L.LESION_TABLE_COLUMNS), ("RU_LESION_CHUNK", L.LESION_CHUNK)]:
        assert re.search(r"#define %s %d\b" % (macro, value), text), macro
    assert len(L.SIGNATURES["ru_lesion_metrics"][1]) == 18
    build = open(os.path.join(os.path.dirname(HEADER), "..", "brats2019_amd", "build.py")).read()
    assert '"lesion.hip"' in build


def test_workspace_query_refuses_bad_shapes_kinds_and_capacities():
    from brats2019_amd import _lib as L
    lib = L.load()
    small = lib.ru_lesion_workspace_bytes(L.SURFACE_PROB, 1, 3, 16, 16, 16, 64)
    assert small > 0
    # per-lesion state only: 52 B per lesion of max_lesions and (sample, region), nothing per voxel
    more = lib.ru_lesion_workspace_bytes(L.SURFACE_PROB, 1, 3, 16, 16, 16, 64 + 6400)
    assert 0 < more - small <= 3 * 6400 * 52 + 16 * 256
    assert lib.ru_lesion_workspace_bytes(L.SURFACE_LABEL, 1, 1, 240, 240, 155, 1024) > 0
    for args in [(L.SURFACE_PROB, 1, 1, 513, 4, 4, 8), (L.SURFACE_PROB, 1, 1, 4, 4, 513, 8), (L.SURFACE_PROB, 1, 1, 0, 4, 4, 8),
                 (L.SURFACE_LABEL, 1, 2, 4, 4, 4, 8), (2, 1, 1, 4, 4, 4, 8), (L.SURFACE_PROB, 0, 1, 4, 4, 4, 8), (L.SURFACE_PROB, 1, 1, 4, 4, 4, 0),
                 (L.SURFACE_PROB, 1, 1, 4, 4, 4, 65537)]:
        assert lib.ru_lesion_workspace_bytes(*args) == 0, args


def test_metric_classes_have_the_documented_surface():
    from brats2019_amd import metrics
    for cls, name in [(metrics.LesionWiseDice, "LesionWiseDice"), (metrics.LesionWiseHausdorff95, "LesionWiseHausdorff95")]:
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
            ("name", name), ("input_index", 0), ("target_index", 0), ("classes", 4), ("empty_value", 373.12866), ("dilation", 3), ("min_volume", 50)]
        assert issubclass(cls, metrics.Metrics)
        m = cls()
        assert m.name == name and m.accumulator == 0.0 and m.samples == 0.0 and (m.dilation, m.min_volume, m.empty_value) == (3, 50, EMPTY)
    from brats2019_amd import ops
    sig = inspect.signature(ops.lesion_metrics)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:6]] == [("dilation", 3), ("min_volume", 50), ("empty_value", ops.HD95_EMPTY),
                                                                                  ("want_table", False)]


def test_validate_lesionwise_flag_is_opt_in():
    from brats2019_amd import validate
    plain = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b"])
    assert str(plain) == "Namespace(data_path='a', predictions_path='b')"           # what the plain scorer prints, unchanged
    assert not hasattr(plain, "lesionwise") and not hasattr(plain, "dilation") and not hasattr(plain, "min_volume")
    opt = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b", "--lesionwise", "--dilation", "2", "--min_volume", "10"])
    assert opt.lesionwise is True and opt.dilation == 2 and opt.min_volume == 10
    with pytest.raises(SystemExit):
        validate.parser.parse_args(["--lesionwise=1"])
    row = validate._lesion_row(np.arange(6, dtype=np.float64).reshape(2, 3), np.arange(15).reshape(3, 5))
    assert row.split() == ["LesionDice", "WT", "0.0000", "TC", "1.0000", "ET", "2.0000", "LesionHD95", "WT", "3.0000", "TC", "4.0000", "ET", "5.0000",
                           "WT", "gt", "0", "kept", "1", "tp", "2", "fn", "3", "fp", "4", "TC", "gt", "5", "kept", "6", "tp", "7", "fn", "8", "fp", "9",
                           "ET", "gt", "10", "kept", "11", "tp", "12", "fn", "13", "fp", "14"]


def test_bad_shapes_and_parameters_are_refused_before_any_upload():
    import torch
    from brats2019_amd import ops, validate
    with pytest.raises(ValueError, match="case0"):
        validate.score_lesionwise([("case0", np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 5), np.uint8))])
    with pytest.raises(ValueError, match="case1"):
        validate.score_lesionwise([("case1", np.zeros((1, 4, 4, 4), np.uint8), np.zeros((1, 4, 4, 4), np.uint8))])
    with pytest.raises(ValueError, match="no cases"):
        validate.score_lesionwise([])
    with pytest.raises(ValueError, match="dilation"):
        validate.score_lesionwise([], dilation=-1)
    x = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="differ"):
        ops.lesion_metrics(x, torch.zeros((1, 1, 4, 4, 5)))
    with pytest.raises(ValueError, match="min_volume"):
        ops.lesion_metrics(x, x, min_volume=-1)
    with pytest.raises(ValueError, match=r"\[N, D, H, W\]"):
        ops.lesion_metrics(torch.zeros((4, 4, 4), dtype=torch.uint8), torch.zeros((4, 4, 4), dtype=torch.uint8))
