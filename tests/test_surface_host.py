"""The BraTS challenge metrics (Dice, sensitivity, specificity, HD95; csrc/surface.hip) without a GPU: the scipy / numpy oracle that
tests/test_surface.py holds the device to, on hand-worked cases; the empty rules; numpy's percentile interpolation as the select pass
restates it; the C-ABI declarations; the metric classes' signatures; and `validate --regions`' argument handling.

Oracle (the definitions of the feature): surface dA = A XOR binary_erosion(A, 6-connectivity, border_value=0); S = the squared
distances from dP to the nearest voxel of dG and from dG to dP, from distance_transform_edt's nearest-site indices so that they are
exact integers; HD95 = np.percentile(sqrt(S), 95)."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
EMPTY = 373.12866
STRUCT = ndimage.generate_binary_structure(3, 1)


# ---------------------------------------------------------------------- oracle
def surface(a):
    return a & ~ndimage.binary_erosion(a, STRUCT, border_value=0)


def sq_to(sites, query):
    """exact squared distance from each voxel of `query` to the nearest voxel of `sites` (non-empty), in np.argwhere order"""
    idx = ndimage.distance_transform_edt(~sites, return_distances=False, return_indices=True)
    d2 = ((idx - np.indices(sites.shape)).astype(np.int64) ** 2).sum(axis=0)
    return d2[query]


def surface_sq(p, g):
    sp, sg = surface(p), surface(g)
    return np.concatenate([sq_to(sg, sp), sq_to(sp, sg)])


def oracle_counts(p, g):
    """(|P|, |G|, TP, |dP|, |dG|)"""
    return (int(p.sum()), int(g.sum()), int((p & g).sum()), int(surface(p).sum()), int(surface(g).sum()))


def oracle_hd95(p, g, empty_value=EMPTY):
    if not p.any() and not g.any():
        return 0.0
    if not p.any() or not g.any():
        return empty_value
    return float(np.percentile(np.sqrt(surface_sq(p, g).astype(np.float64)), 95))


def oracle_values(p, g, empty_value=EMPTY):
    """(Dice, sensitivity, specificity, HD95) of one pair of masks, the definitions' float64 forms"""
    cp, cg, tp = int(p.sum()), int(g.sum()), int((p & g).sum())
    v = p.size
    dice = 1.0 if cp + cg == 0 else 2 * tp / (cp + cg)
    sens = 1.0 if cg == 0 else tp / cg
    spec = 1.0 if v == cg else (v - cp - cg + tp) / (v - cg)
    return dice, sens, spec, oracle_hd95(p, g, empty_value)


def oracle_batch(pm, gm, empty_value=EMPTY):
    """masks [N, K, D, H, W] -> (values float64 [N, K, 4], counts int64 [N, K, 5])"""
    n, k = pm.shape[:2]
    vals = np.array([[oracle_values(pm[i, j], gm[i, j], empty_value) for j in range(k)] for i in range(n)], dtype=np.float64)
    counts = np.array([[oracle_counts(pm[i, j], gm[i, j]) for j in range(k)] for i in range(n)], dtype=np.int64)
    return vals, counts


def regions(labels):
    """uint8 BraTS labels [..., D, H, W] -> masks [..., 3, D, H, W] of WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4}"""
    lab = np.asarray(labels)
    return np.stack([(lab >= 1) & (lab <= 4), (lab == 1) | (lab == 3) | (lab == 4), (lab == 3) | (lab == 4)], axis=-4)


def percentile_position(n):
    """numpy's linear method: (i, j, t) for the 95th percentile of n sorted values"""
    x = (n - 1) * 0.95
    i = int(np.floor(x))
    return i, min(i + 1, n - 1), x - i


def lerp_percentile(sq_sorted):
    """the select pass's arithmetic: numpy's _lerp of sqrt(s_(i)) and sqrt(s_(j)), two roundings, no fused multiply-add"""
    i, j, t = percentile_position(len(sq_sorted))
    a, b = np.sqrt(np.float64(sq_sorted[i])), np.sqrt(np.float64(sq_sorted[j]))
    return float(b - (b - a) * (1 - t)) if t >= 0.5 else float(a + (b - a) * t)


def blob_masks(rng, shape, count, nblobs=3):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    out = np.zeros((count,) + tuple(shape), dtype=bool)
    for m in out:
        for _ in range(nblobs):
            c = [rng.uniform(0, s) for s in shape]
            r = rng.uniform(1.0, max(1.5, 0.3 * max(shape)))
            m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return out


# ---------------------------------------------------------------------- the oracle on hand-worked cases
def test_single_voxel_against_single_voxel():
    p, g = np.zeros((4, 5, 6), bool), np.zeros((4, 5, 6), bool)
    p[0, 1, 1] = g[1, 3, 3] = True                                       # offset (1, 2, 2): distance 3 both ways
    assert surface_sq(p, g).tolist() == [9, 9]
    assert oracle_counts(p, g) == (1, 1, 0, 1, 1)
    assert oracle_values(p, g) == (0.0, 0.0, 118 / 119, 3.0)


def test_cube_against_the_same_cube_shifted_by_one():
    p, g = np.zeros((6, 6, 7), bool), np.zeros((6, 6, 7), bool)
    p[1:4, 1:4, 1:4] = True
    g[1:4, 1:4, 2:5] = True
    # 26 surface voxels each (all but the centre).  From dP: the 9 voxels of the layer w = 1 lie outside G (distance 1); P's voxel at
    # G's centre (2, 2, 3) is 1 from dG; the other 16 lie on dG.  The same the other way: 20 ones and 32 zeros in S.
    s = np.sort(surface_sq(p, g))
    assert oracle_counts(p, g) == (27, 27, 18, 26, 26)
    assert s.tolist() == [0] * 32 + [1] * 20
    assert percentile_position(52)[0] == 48 and oracle_hd95(p, g) == 1.0
    g2 = np.zeros_like(g)
    g2[1:4, 1:4, 3:6] = True                                            # shifted by two: the far layers are 2 apart
    assert oracle_hd95(p, g2) == np.percentile(np.sqrt(surface_sq(p, g2).astype(float)), 95) > 1.0


def test_masks_touching_the_grid_edge_have_their_edge_voxels_on_the_surface():
    full = np.ones((3, 3, 3), bool)
    assert surface(full).sum() == 26 and not surface(full)[1, 1, 1]      # erosion with a zero border: only the centre is interior
    assert surface(np.ones((2, 2, 2), bool)).all()
    p = np.zeros((5, 5, 5), bool)
    p[:, :, :2] = True                                                  # a slab on the face w = 0
    assert surface(p)[2, 2, 0] and surface(p)[2, 2, 1]
    assert oracle_counts(full, full) == (27, 27, 27, 26, 26) and oracle_values(full, full) == (1.0, 1.0, 1.0, 0.0)


def test_an_axis_of_extent_one_makes_every_voxel_surface():
    for shape in [(1, 4, 5), (4, 1, 5), (4, 5, 1)]:
        a = np.ones(shape, bool)
        assert surface(a).all()
    p, g = np.zeros((1, 1, 10), bool), np.zeros((1, 1, 10), bool)
    p[0, 0, :4] = True
    g[0, 0, 6:] = True
    # dP = 0..3 (distances to 6: 6, 5, 4, 3), dG = 6..9 (distances to 3: 3, 4, 5, 6): sorted sqrt 3 3 4 4 5 5 6 6; x = 6.65
    assert np.sort(surface_sq(p, g)).tolist() == [9, 9, 16, 16, 25, 25, 36, 36]
    assert oracle_hd95(p, g) == pytest.approx(6.0, abs=0) and lerp_percentile([9, 9, 16, 16, 25, 25, 36, 36]) == 6.0


# ---------------------------------------------------------------------- empty rules
def test_empty_rules():
    z, one = np.zeros((3, 4, 5), bool), np.zeros((3, 4, 5), bool)
    one[1, 2, 3] = True
    assert oracle_values(z, z) == (1.0, 1.0, 1.0, 0.0)
    assert oracle_values(one, z) == (0.0, 1.0, 59 / 60, EMPTY)           # G empty: sensitivity 1
    assert oracle_values(z, one) == (0.0, 0.0, 1.0, EMPTY)
    assert oracle_values(z, one, empty_value=-1.0)[3] == -1.0
    full = np.ones((3, 4, 5), bool)
    assert oracle_values(one, full)[2] == 1.0                            # G fills the volume: specificity 1
    assert EMPTY == pytest.approx(np.sqrt(240 ** 2 + 240 ** 2 + 155 ** 2), abs=5e-6)


# ---------------------------------------------------------------------- percentile arithmetic
def test_lerp_reproduces_numpy_percentile_exactly():
    rng = np.random.default_rng(5)
    seen = set()
    for n in list(range(2, 200)) + [401, 1001, 20001, 123457]:
        s = np.sort(rng.integers(0, 3 * 511 ** 2, size=n))
        if n % 3 == 0:
            s = np.sort(rng.integers(0, 4, size=n))                      # many ties
        want = float(np.percentile(np.sqrt(s.astype(np.float64)), 95))
        assert lerp_percentile(s) == want, n
        t = percentile_position(n)[2]
        seen.add("0" if t == 0 else ("lt" if t < 0.5 else "ge"))
    assert seen == {"0", "lt", "ge"}
    assert percentile_position(21) == (19, 20, 0.0)                    # 20 * 0.95 == 19.0 in float64


# ---------------------------------------------------------------------- the interface, without a device
def test_header_and_ctypes_table_declare_the_surface_entries():
    from brats2019_amd import _lib as L
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ru_surface_workspace_bytes", "ru_surface_metrics", "ru_surface_accumulate"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    for macro, value in [("RU_SURFACE_PROB", L.SURFACE_PROB), ("RU_SURFACE_LABEL", L.SURFACE_LABEL), ("RU_SURFACE_REGIONS", L.SURFACE_REGIONS),
                         ("RU_SURFACE_COUNTS", L.SURFACE_COUNTS), ("RU_SURFACE_DICE", L.SURFACE_COLUMNS["dice"]),
                         ("RU_SURFACE_SENS", L.SURFACE_COLUMNS["sensitivity"]), ("RU_SURFACE_SPEC", L.SURFACE_COLUMNS["specificity"]),
                         ("RU_SURFACE_HD95", L.SURFACE_COLUMNS["hd95"])]:
        assert re.search(r"#define %s %d\b" % (macro, value), text), macro


def test_workspace_query_refuses_bad_shapes_and_kinds():
    from brats2019_amd import _lib as L
    lib = L.load()
    ok = lib.ru_surface_workspace_bytes(L.SURFACE_PROB, 4, 3, 128, 128, 128)
    nk, v, words, bins = 12, 128 ** 3, 128 * 128 * 2, 3 * 127 ** 2 + 1
    assert ok == nk * (4 * words * 8 + 2 * v * 4 + bins * 4)
    assert lib.ru_surface_workspace_bytes(L.SURFACE_LABEL, 1, 1, 240, 240, 155) > 0
    for args in [(L.SURFACE_PROB, 1, 1, 513, 4, 4), (L.SURFACE_PROB, 1, 1, 4, 4, 513), (L.SURFACE_PROB, 1, 1, 0, 4, 4),
                 (L.SURFACE_LABEL, 1, 2, 4, 4, 4), (2, 1, 1, 4, 4, 4), (L.SURFACE_PROB, 0, 1, 4, 4, 4)]:
        assert lib.ru_surface_workspace_bytes(*args) == 0, args


def test_metric_classes_have_the_documented_surface():
    from brats2019_amd import metrics
    for cls, params in [(metrics.Hausdorff95, [("name", "Hausdorff95"), ("input_index", 0), ("target_index", 0), ("classes", 4),
                                               ("empty_value", 373.12866)]),
                        (metrics.Sensitivity, [("name", "Sensitivity"), ("input_index", 0), ("target_index", 0), ("classes", 4)]),
                        (metrics.Specificity, [("name", "Specificity"), ("input_index", 0), ("target_index", 0), ("classes", 4)])]:
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == params
        assert issubclass(cls, metrics.Metrics)
        m = cls()
        assert m.name == params[0][1] and m.accumulator == 0.0 and m.samples == 0.0


def test_validate_regions_flag_is_opt_in():
    from brats2019_amd import validate
    plain = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b"])
    assert str(plain) == "Namespace(data_path='a', predictions_path='b')"           # what the plain scorer prints, unchanged
    assert not hasattr(plain, "regions")
    opt = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b", "--regions"])
    assert opt.regions is True
    with pytest.raises(SystemExit):
        validate.parser.parse_args(["--regions=1"])
    r = np.arange(12, dtype=np.float64).reshape(4, 3)
    row = validate._region_row(r)
    assert row.split() == ["Dice", "WT", "0.0000", "TC", "1.0000", "ET", "2.0000", "Sens", "WT", "3.0000", "TC", "4.0000", "ET", "5.0000",
                           "Spec", "WT", "6.0000", "TC", "7.0000", "ET", "8.0000", "HD95", "WT", "9.0000", "TC", "10.0000", "ET", "11.0000"]


def test_validate_regions_reports_bad_shapes_before_any_upload():
    from brats2019_amd import validate
    with pytest.raises(ValueError, match="case0"):
        validate.score_regions([("case0", np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 5), np.uint8))])
    with pytest.raises(ValueError, match="no cases"):
        validate.score_regions([])


def test_oracle_regions_follow_the_label_sets():
    lab = np.arange(6, dtype=np.uint8).reshape(1, 1, 6)
    r = regions(lab)
    assert r.shape == (3, 1, 1, 6)
    assert r[0].ravel().tolist() == [False, True, True, True, True, False]
    assert r[1].ravel().tolist() == [False, True, False, True, True, False]
    assert r[2].ravel().tolist() == [False, False, False, True, True, False]
