"""The normalized surface Dice (NSD), the average symmetric surface distance (ASSD) and the Hausdorff distance from the histogram of
surface distances (csrc/surface.hip, ru_surface_distances; csrc/lesion.hip, ru_lesion_distances) without a GPU: `ops.tolerance_bins`
against a brute-force search; the float64 restatements of brats2019_amd/metrics.py, which tests/test_nsd.py holds the device to, on
cases with values known in closed form; the case set of that file and a guard that it is not trivial; the C-ABI declarations; the
argument errors that need no device; `validate --nsd`."""
import inspect
import re

import numpy as np
import pytest

from test_surface_host import EMPTY, HEADER

SQRT2 = np.sqrt(2.0)
BELOW_SQRT2 = np.nextafter(SQRT2, 0)
TOL8 = (0.0, 0.5, 1.0, SQRT2, BELOW_SQRT2, 2.0, 3.0, np.inf)        # the 8-list of tests/test_nsd.py
TOP = 2 ** 32 - 1


# ---------------------------------------------------------------------- the case set shared with tests/test_nsd.py
def ball(shape, centre, r):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    return (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 <= r * r


def mask_cases(shape, seed=0):
    """-> [(name, P, G)] bool [D, H, W]: both empty, one empty each way, the full grid, single voxels, identical masks, a box against its
    copy shifted by 2 in x, nested balls against a speckled displaced copy"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z = np.zeros(shape, bool)
    one, other = z.copy(), z.copy()
    one[0, 0, 0] = True
    other[min(1, d - 1), min(1, h - 1), 0] = True                                     # offset (1, 1, 0) where the grid has room
    box, shifted = z.copy(), z.copy()
    box[0:2, 1:h - 1, 1:w - 3] = True                                                 # 2 thick: every voxel is surface
    shifted[0:2, 1:h - 1, 3:w - 1] = True
    c = [(s - 1) / 2.0 for s in shape]
    r = max(1.0, 0.45 * min(max(shape), 2 * min(h, w)))
    nested = ball(shape, c, r) & ~ball(shape, c, 0.5 * r) | ball(shape, c, 0.25 * r)  # a shell around a core: inner surfaces too
    moved = np.roll(nested, (1, -1, 2), axis=(0, 1, 2)) ^ (rng.random(shape) < 0.03)
    return [("both empty", z, z), ("P empty", z, nested), ("G empty", nested, z), ("full grid", ~z, ~z), ("single voxels", one, other),
            ("identical", nested, nested), ("shifted box", box, shifted), ("nested balls", nested, moved), ("full against balls", ~z, moved)]


# ---------------------------------------------------------------------- tolerance_bins
def brute_bin(tau, limit=1 << 16):
    """the largest b < limit with numpy.sqrt(float64(b)) <= tau, by looking at every b"""
    ok = np.sqrt(np.arange(limit, dtype=np.float64)) <= np.float64(tau)
    assert ok[0] and not ok[-1]
    b = int(np.flatnonzero(ok)[-1])
    assert ok[:b + 1].all()                                                           # sqrt is monotone: the set is a prefix
    return b


def test_tolerance_bins_against_a_brute_force_search():
    from brats2019_amd import ops
    taus = [0.0, 0.5, 1.0, SQRT2, BELOW_SQRT2, 1.5, 2.0, 3.0]
    for b in range(200):
        s = np.sqrt(np.float64(b))
        taus += [s, np.nextafter(s, np.inf)] + ([np.nextafter(s, 0)] if b else [])
    for tau in taus:
        assert ops.tolerance_bins([tau]) == [brute_bin(tau)], repr(tau)
    for b in range(200):                                                              # an exact sqrt(b) includes bin b, the float below does not
        s = np.sqrt(np.float64(b))
        assert ops.tolerance_bins([s]) == [b]
        if b:
            assert ops.tolerance_bins([np.nextafter(s, 0)]) == [b - 1]
    assert ops.tolerance_bins([SQRT2, BELOW_SQRT2]) == [2, 1]
    # beyond every bin a uint32 names: sqrt(2**32 - 1) < 65536 <= tau, so the clamp is the answer
    assert np.sqrt(np.float64(TOP)) < 65536.0
    assert ops.tolerance_bins([1e9, np.inf, 65536.0]) == [TOP, TOP, TOP]
    assert ops.tolerance_bins([np.nextafter(65536.0, 0)]) == [TOP]                    # floor(tau^2) = 2^32 - 1 here: the corrections stop at the clamp
    assert ops.tolerance_bins([65535.0]) == [65535 ** 2]
    assert ops.tolerance_bins(TOL8) == [0, 0, 1, 2, 1, 4, 9, TOP] and ops.tolerance_bins(()) == []
    for bad in ([-1.0], [-0.5, 1.0], [float("nan")], [-np.inf], [1.0] * 9):
        with pytest.raises(ValueError):
            ops.tolerance_bins(bad)


# ---------------------------------------------------------------------- the restatement on hand-computable cases
def test_identical_masks():
    from brats2019_amd import metrics
    m = ball((9, 10, 11), (4, 4, 5), 3.2)
    assert metrics.surface_distances_host(m, m, TOL8).tolist() == [1.0] * 8 + [0.0, 0.0]
    assert metrics.surface_distances_host(m, m, ()).tolist() == [0.0, 0.0]


def test_a_box_and_its_copy_shifted_by_two():
    """boxes 2 x b x c, every voxel on the surface: of each box the 2b voxels of the first two x layers outside the other lie 2 and 1 from
    it, the rest inside it: S = 4b(c - 2) zeros, 4b ones, 4b fours"""
    from brats2019_amd import metrics
    b, c = 5, 7
    p, g = np.zeros((4, 8, 12), bool), np.zeros((4, 8, 12), bool)
    p[1:3, 1:1 + b, 1:1 + c] = True
    g[1:3, 1:1 + b, 3:3 + c] = True
    hist = metrics.surface_histogram_host(p, g)
    assert hist[[0, 1, 4]].tolist() == [4 * b * (c - 2), 4 * b, 4 * b] and hist.sum() == 4 * b * c and len(hist) == 9 + 49 + 121 + 1
    got = metrics.surface_distances_host(p, g, (0.0, 0.99, 1.0, 1.99, 2.0))
    assert got.tolist() == [(c - 2) / c, (c - 2) / c, (c - 1) / c, (c - 1) / c, 1.0, 3 / c, 2.0]


def test_single_voxels_at_offset_1_1_0():
    from brats2019_amd import metrics
    p, g = np.zeros((3, 4, 5), bool), np.zeros((3, 4, 5), bool)
    p[1, 1, 2] = g[2, 2, 2] = True
    got = metrics.surface_distances_host(p, g, (1.0, BELOW_SQRT2, SQRT2, 2.0))
    assert got.tolist() == [0.0, 0.0, 1.0, 1.0, SQRT2, SQRT2]


def test_empty_rules_and_the_grid_edge():
    from brats2019_amd import metrics
    z, m = np.zeros((3, 4, 5), bool), np.ones((3, 4, 5), bool)
    assert metrics.surface_distances_host(z, z, (1.0, 2.0)).tolist() == [1.0, 1.0, 0.0, 0.0]
    assert metrics.surface_distances_host(z, m, (1.0, np.inf)).tolist() == [0.0, 0.0, EMPTY, EMPTY]
    assert metrics.surface_distances_host(m, z, (1.0,), empty_value=-2.0).tolist() == [0.0, -2.0, -2.0]
    one = z.copy()
    one[1, 1, 2] = True
    # the full grid's surface is its boundary layer (outside counts as background): the centre voxel is 1 from it
    assert metrics._surface_host(m).sum() == 60 - 1 * 2 * 3
    got = metrics.surface_distances_host(m, one, (0.0, 1.0))
    n = 54 + 1
    assert got[0] == 0.0 and got[1] == 4 / n          # (0,1,2), (2,1,2), (1,0,2) lie on the boundary layer 1 away; and the voxel itself
    assert got[3] == np.sqrt(np.float64(1 + 4 + 4))                                   # the far corners of the 3 x 4 x 5 grid


def test_lesion_restatement_on_closed_form_cases():
    from brats2019_amd import metrics
    shape = (12, 14, 40)
    a, b = np.zeros(shape, bool), np.zeros(shape, bool)
    a[1:5, 1:5, 1:5] = True
    b[6:10, 8:12, 30:34] = True
    tol = (0.0, 1.0)
    s, rows, fp = metrics.lesion_distances_host(a | b, a | b, tol)
    assert s.tolist() == [1.0, 1.0, 0.0] and rows.tolist() == [[1.0, 1.0, 0.0, 0.0]] * 2 and fp == 0
    s, rows, fp = metrics.lesion_distances_host(a, a | b, tol)                        # one missed: NSD 0, ASSD and HD the penalty
    assert s.tolist() == [0.5, 0.5, EMPTY / 2] and rows[1].tolist() == [0.0, 0.0, EMPTY, EMPTY] and fp == 0
    speck = a | b
    speck[11, 0, 20] = True                                                           # one false positive: 0 and the penalty
    s, rows, fp = metrics.lesion_distances_host(speck, a | b, tol)
    assert s.tolist() == [2 / 3, 2 / 3, EMPTY / 3] and fp == 1
    z = np.zeros(shape, bool)
    assert metrics.lesion_distances_host(z, z, tol)[0].tolist() == [1.0, 1.0, 0.0]
    assert metrics.lesion_distances_host(speck, z, tol, empty_value=7.0)[0].tolist() == [0.0, 0.0, 7.0]
    small = np.zeros(shape, bool)
    small[1:3, 1:6, 1:6] = True                                                       # 50 voxels: dropped, and what it matched is no false positive
    s, rows, fp = metrics.lesion_distances_host(small, small | b, tol)
    assert s.tolist() == [0.0, 0.0, EMPTY] and rows[0].tolist() == [1.0, 1.0, 0.0, 0.0] and fp == 0


GRIDS = [(1, 2, (3, 5, 7)), (2, 3, (17, 19, 37)), (1, 3, (9, 64, 64)), (1, 2, (5, 6, 130))]      # (N, C, grid) of tests/test_nsd.py


def test_the_case_set_is_not_trivial():
    """over the grids of tests/test_nsd.py: for every tested tolerance in (0.5 .. 3) some case has 0 < NSD < 1, and some ASSD is no
    integer; at the grids beyond the smallest, each on its own"""
    from brats2019_amd import metrics
    seen = np.zeros(8, bool)
    for _, _, shape in GRIDS:
        cases = mask_cases(shape)
        assert len(cases) == 9
        vals = np.array([metrics.surface_distances_host(p, g, TOL8) for _, p, g in cases])
        between = ((vals[:, :8] > 0) & (vals[:, :8] < 1)).any(axis=0)
        seen |= between
        if max(shape) > 7:
            assert between[[1, 2, 3, 4, 5, 6]].all(), (shape, between)
        assert any(v != np.floor(v) for v in vals[:, 8]), shape
        names = [n for n, _, _ in cases]
        assert vals[names.index("both empty")].tolist() == [1.0] * 8 + [0.0, 0.0]
        assert vals[names.index("P empty")].tolist() == [0.0] * 8 + [EMPTY, EMPTY]
        assert vals[names.index("identical")].tolist() == [1.0] * 8 + [0.0, 0.0]
        # NSD rises with the tolerance; at infinity it is 1 for every pair of non-empty masks
        order = np.argsort(np.array(TOL8), kind="stable")
        assert (np.diff(vals[:, order], axis=1) >= 0).all() and (vals[3:, 7] == 1.0).all()
        if max(shape) > 7:
            assert (vals[:, 3] > vals[:, 4]).any()                                    # sqrt 2 against the float below it: bin 2 counts or not
    assert all(seen[t] for t, tau in enumerate(TOL8) if 0.5 <= tau <= 3)


# ---------------------------------------------------------------------- the interface, without a device
def test_header_and_ctypes_table_declare_the_distance_entries():
    from brats2019_amd import _lib as L
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in [("ru_surface_distances", 17), ("ru_surface_extras_accumulate", 8), ("ru_lesion_distances_workspace_bytes", 8),
                        ("ru_lesion_distances", 22)]:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs == len(decl.group(1).split(",")), name
    assert re.search(r"#define RU_SURFACE_MAX_TOL %d\b" % L.SURFACE_MAX_TOL, text) and L.SURFACE_MAX_TOL == 8
    assert L.surface_extras_columns(2) == {"nsd0": 0, "nsd1": 1, "assd": 2, "hd": 3} and L.surface_extras_columns(0) == {"assd": 0, "hd": 1}
    assert L.lesion_extras_columns(3) == {"nsd0": 0, "nsd1": 1, "nsd2": 2, "assd": 3}


def test_workspace_queries():
    from brats2019_amd import _lib as L
    lib = L.load()
    base = lib.ru_lesion_workspace_bytes(L.SURFACE_PROB, 1, 3, 16, 16, 16, 64)
    for t in (0, 1, 8):                                                               # 8 (T + 2) B per lesion and (n, k) more, rounded to 256
        more = lib.ru_lesion_distances_workspace_bytes(L.SURFACE_PROB, 1, 3, 16, 16, 16, 64, t)
        assert 0 <= more - base - 3 * 64 * 8 * (t + 2) < 256, t
    for args in [(L.SURFACE_PROB, 1, 3, 16, 16, 16, 64, 9), (L.SURFACE_PROB, 1, 3, 16, 16, 16, 64, -1), (L.SURFACE_PROB, 1, 3, 513, 16, 16, 64, 1),
                 (L.SURFACE_PROB, 1, 3, 16, 16, 16, 0, 1), (L.SURFACE_LABEL, 1, 2, 16, 16, 16, 64, 1)]:
        assert lib.ru_lesion_distances_workspace_bytes(*args) == 0, args


def test_metric_classes_have_the_documented_surface():
    from brats2019_amd import metrics, ops
    head = [("input_index", 0), ("target_index", 0), ("classes", 4)]
    for cls, name, tail in [(metrics.SurfaceDice, "SurfaceDice", [("tolerance", 1.0)]),
                            (metrics.AverageSurfaceDistance, "AverageSurfaceDistance", [("empty_value", 373.12866)]),
                            (metrics.LesionWiseSurfaceDice, "LesionWiseSurfaceDice", [("tolerance", 1.0), ("dilation", 3), ("min_volume", 50)])]:
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("name", name)] + head + tail
        assert issubclass(cls, metrics._ColumnMetric)
        m = cls()
        assert m.name == name and m.accumulator == 0.0 and m.samples == 0.0
    with pytest.raises(ValueError):
        metrics.SurfaceDice(tolerance=-1.0)
    with pytest.raises(ValueError):
        metrics.LesionWiseSurfaceDice(tolerance=float("nan"))
    sig = inspect.signature(ops.surface_distances)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [("tolerances", (1.0,)), ("empty_value", ops.HD95_EMPTY)]
    sig = inspect.signature(ops.lesion_distances)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("tolerances", (1.0,)), ("dilation", 3), ("min_volume", 50), ("empty_value", ops.HD95_EMPTY), ("want_table", False), ("max_lesions", ops.LESION_MAX)]


def test_argument_errors_need_no_device():
    import torch
    from brats2019_amd import ops
    x = torch.zeros((1, 1, 4, 4, 4))
    u = torch.zeros((4, 4, 4), dtype=torch.uint8)
    for fn in (ops.surface_distances, ops.lesion_distances):
        with pytest.raises(ValueError, match="differ"):
            fn(x, torch.zeros((1, 1, 4, 4, 5)))
        with pytest.raises(ValueError, match="differ"):
            fn(x, x.to(torch.float64))
        with pytest.raises(ValueError, match=">= 0"):
            fn(x, x, tolerances=(1.0, -1.0))
        with pytest.raises(ValueError, match=">= 0"):
            fn(x, x, tolerances=(float("nan"),))
        with pytest.raises(ValueError, match="at most 8"):
            fn(x, x, tolerances=(1.0,) * 9)
        with pytest.raises(ValueError, match=r"\[N, D, H, W\]"):
            fn(u, u)
    with pytest.raises(ValueError, match="min_volume"):
        ops.lesion_distances(x, x, min_volume=-1)
    with pytest.raises(ValueError, match="dilation"):
        ops.lesion_distances(x, x, dilation=-1)
    with pytest.raises(ValueError, match="max_lesions"):
        ops.lesion_distances(x, x, max_lesions=0)


def test_validate_nsd_flag_is_opt_in():
    from brats2019_amd import validate
    plain = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b"])
    assert str(plain) == "Namespace(data_path='a', predictions_path='b')"           # what the plain scorer prints, unchanged
    assert not hasattr(plain, "nsd")
    opt = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b", "--regions"])
    assert str(opt) == "Namespace(data_path='a', predictions_path='b', regions=True)" and not hasattr(opt, "nsd")
    opt = validate.parser.parse_args(["--data_path", "a", "--predictions_path", "b", "--regions", "--nsd", "1", "2.5"])
    assert opt.regions is True and opt.nsd == [1.0, 2.5]
    opt = validate.parser.parse_args(["--lesionwise", "--nsd", "2"])
    assert opt.lesionwise is True and opt.nsd == [2.0]
    with pytest.raises(SystemExit):
        validate.parser.parse_args(["--regions", "--nsd"])
    with pytest.raises(SystemExit):
        validate.parser.parse_args(["--regions", "--nsd", "near"])
    r = np.arange(21, dtype=np.float64).reshape(7, 3)
    assert validate._region_row(r[:4]) == validate._region_row(r[:4], ())            # without the flag the line is what it was
    assert validate._region_row(r[:4]).split()[-7:] == ["HD95", "WT", "9.0000", "TC", "10.0000", "ET", "11.0000"]
    assert validate._region_row(r, [1.0, 2.5]).split()[28:] == ["NSD@1", "WT", "12.0000", "TC", "13.0000", "ET", "14.0000", "NSD@2.5", "WT", "15.0000",
                                                                  "TC", "16.0000", "ET", "17.0000", "ASSD", "WT", "18.0000", "TC", "19.0000", "ET", "20.0000"]
    row = validate._lesion_row(np.arange(9, dtype=np.float64).reshape(3, 3), None, [1.0])
    assert row.split()[14:] == ["LesionNSD@1", "WT", "6.0000", "TC", "7.0000", "ET", "8.0000"]
    assert validate._lesion_row(np.arange(6, dtype=np.float64).reshape(2, 3)).split()[0] == "LesionDice"
    # bad lists and shapes are refused before any upload
    with pytest.raises(ValueError):
        validate.score_regions([], nsd=[-1.0])
    with pytest.raises(ValueError):
        validate.score_lesionwise([], nsd=[1.0] * 9)
    with pytest.raises(ValueError, match="case0"):
        validate.score_regions([("case0", np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 5), np.uint8))], nsd=[1.0])
    with pytest.raises(ValueError, match="no cases"):
        validate.score_lesionwise([], nsd=[1.0])
