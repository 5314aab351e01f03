"""The float64 restatements of the eight-corner gathers (tests/gather_inputs.py), without a GPU: what tests/test_gather.py holds the kernels to is
itself tied to scipy.ndimage, to `oracle.augment_patch` and to the host functions of brats2019_amd.dataloader on every committed case -- the crops
flush with the volume's faces, the patches of extent 1, the scales beyond two patch lengths and the border coordinates included -- the exact family
is shown to be exact, the kernels' float32 operation order is emulated and stays below the derived bars, and every mutant exceeds them.

The restatements take the interpolation weight t as the kernels define it: a float32 (see gather_inputs).  scipy, the oracle and the host functions
keep t in float64, so they differ from the restatement by at most 2^-25 per axis weight: 3 * 2^-25 per corner weight, 8 corners, on values of at
most max |x|: 12 * 2^-24 * max |x|, carried through |inv_std gain|; 1e-11 on top covers their own float64 roundings.  That is TIE below.  At a
product tie of the zoom pass (index 10 at scale 0.7) the restatement's weight is a negative number near -4.4e-16 where scipy's is 0, far inside
TIE; a hard target, a sum of such weights, can therefore be a negative number of that size where the reference gives 0.  That is by design: every
consumer in csrc/ thresholds targets at 0.5.

Emulated worst error / bar over the real family (this file prints them with -s): zoom data 0.58, zoom targets 0.36, affine data 0.55, affine
targets 0.39, warp fused 0.34, warp unfused 0.41.  The MI355X gives the same figures (tests/test_gather.py)."""
import types

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import gather_inputs as G
from oracle import resunet_oracle as O

ZOOM, AFFINE, WARP = G.zoom_cases(), G.affine_cases(), G.warp_cases()
ids = lambda cases: [c["name"] for c in cases]
pytestmark = pytest.mark.filterwarnings("ignore:The behavior of affine_transform with a 1-D array")     # the reference's own call form


def tie(case, xmax, scaled):
    """TIE of the module docstring: per channel through |inv_std gain| for the data (scaled), plain for the targets"""
    if not scaled:
        return 12.0 * G.U * xmax + 1e-11
    ig = np.abs(G.volume(case["vol"])["istd"][:case["C"]].astype(np.float64) * case["gain"].astype(np.float64))
    return (12.0 * G.U * xmax * ig + 1e-11).reshape(-1, 1, 1, 1)


def sources(case):
    v = G.volume(case["vol"])
    c = case["C"]
    other = v["soft"] if case["soft"] else v["label"]
    return v, v["image"][:c].astype(np.float64), other


def tail(case, acc, cw):
    """the float64 tail on interpolated raw channels acc [C, P...] and class / soft channels cw [3, P...], then the output layout"""
    v = G.volume(case["vol"])
    c, sh = case["C"], (-1, 1, 1, 1)
    f = lambda a: a.astype(np.float64).reshape(sh)
    data = ((acc - f(v["mean"][:c])) * f(v["istd"][:c])) * f(case["gain"]) + f(case["bias"])
    target = cw if case["soft"] else np.stack([(cw[0] + cw[1]) + cw[2], cw[0] + cw[2], cw[2]])
    return G.finish(data, case["flags"]), G.finish(target, case["flags"])


def channels(case):
    v, image, other = sources(case)
    cls = other.astype(np.float64) if case["soft"] else np.stack([other == 1, other == 2, other == 3]).astype(np.float64)
    return np.concatenate([image, cls])


def assert_tied(case, ref, data, target, xmax):
    assert data.shape == ref["data"].shape and target.shape == ref["target"].shape, case["name"]
    assert (np.abs(data - ref["data"]) <= tie(case, xmax, True)).all(), case["name"]
    assert (np.abs(target - ref["target"]) <= tie(case, 1.0, False)).all(), case["name"]


# ---------------------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("case", ZOOM, ids=ids(ZOOM))
def test_zoom_restatement_is_scipy_and_the_oracle(case):
    v, image, other = sources(case)
    ref = G.run(case)
    sl = tuple(slice(a, a + n) for a, n in zip(case["lo"], case["patch"]))
    crop = channels(case)[(slice(None),) + sl]
    got = np.stack([ndi.affine_transform(ch, case["scale"], order=1, mode="reflect") for ch in crop])
    xmax = float(np.abs(image).max())
    assert_tied(case, ref, *tail(case, got[:case["C"]], got[case["C"]:]), xmax)
    assert_tied(case, ref, *tail(case, *np.split(O.zoom_linear_reflect(crop, case["scale"]), [case["C"]])), xmax)
    if not case["soft"]:                                                                     # the oracle's whole pass: normalised first, one-hot label
        sh = (-1, 1, 1, 1)
        norm = (image - v["mean"][:case["C"]].astype(np.float64).reshape(sh)) * v["istd"][:case["C"]].astype(np.float64).reshape(sh)
        flips = [bool(case["flags"] & (1 << a)) for a in range(3)]
        d, t = O.augment_patch(norm, other, case["lo"], case["patch"], case["scale"], flips, bool(case["flags"] & 8), case["gain"].astype(np.float64),
                               case["bias"].astype(np.float64))
        assert d.dtype == np.float32 and np.abs(d - ref["data"]).max() <= float(tie(case, xmax, True).max()) + G.U * float(np.abs(ref["data"]).max())
        assert np.abs(t - ref["target"]).max() <= tie(case, 1.0, False) + G.U


@pytest.mark.parametrize("case", AFFINE, ids=ids(AFFINE))
def test_affine_restatement_is_scipy_and_the_host_function(case):
    from brats2019_amd import dataloader as DL
    v, image, other = sources(case)
    ref = G.run(case)
    xmax = float(np.abs(image).max())
    got = np.stack([ndi.affine_transform(ch, case["matrix"], case["offset"], output_shape=case["patch"], order=1, mode="grid-constant", cval=0.0)
                    for ch in channels(case)])
    assert_tied(case, ref, *tail(case, got[:case["C"]], got[case["C"]:]), xmax)
    flips = [bool(case["flags"] & (1 << a)) for a in range(3)]
    d, t = DL.affine_patch_host(v["image"][:case["C"]], other, v["mean"][:case["C"]], 1.0 / v["istd"][:case["C"]].astype(np.float64), case["patch"], case["matrix"],
                                case["offset"], flips, bool(case["flags"] & 8), case["gain"], case["bias"])
    assert_tied(case, ref, d, t, xmax)
    # cells and order of the coordinate arithmetic are the host function's: with t kept in float64 the two agree to float64 rounding
    assert case["family"] != "exact" or (np.array_equal(d, ref["data"]) and np.array_equal(t, ref["target"]))


def defined_disp(case):
    """the displacement with every entry the kernel reads as coordinate 0 (NaN, +-inf, |c| >= 1e9) replaced by the one that gives exactly 0"""
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in case["patch"]], indexing="ij")
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(np.stack(grid) + case["disp"]) < 1.0e9)
    return np.where(bad, -np.stack(grid), case["disp"]), int(bad.sum())


@pytest.mark.parametrize("case", WARP, ids=ids(WARP))
def test_warp_restatement_is_scipy_and_the_host_function(case):
    from brats2019_amd import dataloader as DL
    ref = G.run(case)
    disp, undefined = defined_disp(case)
    assert undefined > 0 or "edge" not in case["name"] or case["patch"] == (1, 1, 1)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in case["patch"]], indexing="ij")
    coords = np.stack(grid) + disp
    flips = [bool(case["flags"] & (1 << a)) for a in range(3)]
    data = case["data"] if case["C"] else None
    target = case["target"] if case["T"] else None
    d, t = DL.elastic_warp_host(data, target, disp, flips, bool(case["flags"] & 8), case["gain"].astype(np.float64), case["bias"].astype(np.float64))
    sh = (-1, 1, 1, 1)
    if case["C"]:
        xmax = float(np.abs(case["data"]).max())
        tol = (12.0 * G.U * xmax * np.abs(case["gain"].astype(np.float64)) + 1e-11).reshape(sh)
        assert (np.abs(d - ref["data"]) <= tol).all()
        got = np.stack([ndi.map_coordinates(ch.astype(np.float64), coords, order=1, mode="reflect") for ch in case["data"]])
        got = G.finish(got * case["gain"].astype(np.float64).reshape(sh) + case["bias"].astype(np.float64).reshape(sh), case["flags"])
        assert (np.abs(got - ref["data"]) <= tol).all()
    else:
        assert d is None and ref["data"] is None
    if case["T"]:
        assert t.dtype == np.float32 and np.array_equal(t, ref["target"])                    # floor(c + 0.5) on the extension, cell for cell
        # scipy reflects the coordinate before it rounds, the kernel rounds and then reflects: the two differ only on coordinates k + 0.5 exactly
        # outside [0, n - 1], which are left to the host function above
        n = np.array(case["patch"], np.float64).reshape(3, 1, 1, 1)
        skip = ((coords - np.floor(coords) == 0.5) & ((coords < 0.0) | (coords > n - 1.0))).any(axis=0)
        got = np.stack([ndi.map_coordinates(ch, coords, order=0, mode="reflect") for ch in case["target"]])
        keep = ~G.finish(skip[None], case["flags"])[0]
        assert np.array_equal(G.finish(got, case["flags"])[:, keep], ref["target"][:, keep])
    else:
        assert t is None and ref["target"] is None


def test_the_cases_reach_what_they_are_there_for():
    names = [c["name"] for c in G.all_cases()]
    assert len(set(names)) == len(names)
    for cases in (ZOOM, AFFINE):
        for fam in ("exact", "real"):
            mine = [c for c in cases if c["family"] == fam]
            assert {c["patch"] for c in mine} >= set(G.SHAPES)
            assert {c["flags"] for c in mine if c["patch"][0] != c["patch"][1]} == set(range(16))
            assert {c["C"] for c in mine} == {1, 2, 3, 4} and {c["soft"] for c in mine} == {False, True}
    for name in ("exact", "exact_full", "brats", "frac", "big"):
        assert set(np.unique(G.volume(name)["label"])) == {0, 1, 2, 3}
    far = tuple(d - p for d, p in zip(G.DIMS, G.SHAPES[3]))
    for fam in ("exact", "real"):
        los = [c["lo"] for c in ZOOM if c["family"] == fam and "flush" in c["name"]]
        assert all(any(lo[a] == 0 for lo in los) and any(lo[a] == far[a] for lo in los) for a in range(3))      # all six faces
    assert any(s * (p - 1) >= 2 * p for c in ZOOM for s, p in zip(c["scale"], c["patch"]) if p > 1)              # the periodic part of the reflection
    v = G.volume("brats")
    assert float(v["image"].max()) == 65535.0 and float(G.volume("frac")["image"].min()) < 0.0
    # the product ties: fl64(index * scale) is an integer, the exact product is not, and the float32 weight is what is left -- negative at 0.7
    signs = set()
    for scale, index in ((0.7, 10), (0.9, 10), (1.1, 10), (1.3, 10), (1.2, 5)):
        _, t = G.zoom_weight(np.array([index]), scale)
        x = np.float64(index) * np.float64(scale)
        assert x == np.floor(x) and 0.0 < abs(float(t[0])) < 1e-15, (scale, index)
        signs.add(float(t[0]) < 0.0)
    assert signs == {False, True} and float(G.zoom_weight(np.array([10]), 0.7)[1][0]) < 0.0
    tie_axes = {(s, c["patch"][a] > i) for c in ZOOM if "ties" in c["name"] for a, s in enumerate(c["scale"]) for i in (10 if s != 1.2 else 5,)}
    assert {(s, True) for s in (0.7, 0.9, 1.1, 1.3, 1.2)} <= tie_axes
    # the affine edge offsets put coordinates exactly on -2, -1, -0.5, 0, n - 1, n - 0.5, n and beyond both clamps
    seen = {a: set() for a in range(3)}
    for c in AFFINE:
        if "edge" in c["name"]:
            q = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in c["patch"]], indexing="ij")
            for a in range(3):
                s = ((c["matrix"][a, 0] * q[0] + c["matrix"][a, 1] * q[1]) + c["matrix"][a, 2] * q[2]) + c["offset"][a]
                seen[a] |= {("n", float(x) - G.DIMS[a]) if x > 5 else ("0", float(x)) for x in np.unique(s)}
    everywhere = set().union(*seen.values())
    assert {("0", -3.0), ("0", -2.0), ("0", -1.0), ("0", -0.5), ("0", 0.0), ("n", -1.0), ("n", -0.5), ("n", 0.0), ("n", 1.0)} <= everywhere
    # the warp's special displacements
    edge = [c for c in WARP if "edge" in c["name"] and c["patch"] != (1, 1, 1)]
    assert len(edge) == 8
    assert all(np.isnan(c["disp"]).any() and np.isinf(c["disp"]).any() and (np.abs(c["disp"]) == 1.0e9).any() for c in edge)
    big = [c for c in edge if c["patch"] == G.SHAPES[3]][0]
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in big["patch"]], indexing="ij"))
    with np.errstate(invalid="ignore"):
        c = grid + big["disp"]
        assert ((c - np.floor(c) == 0.5) & (np.abs(c) < 100)).any() and ((c < 0) & (c != np.floor(c)) & (c > -100)).any() and ((c > 2 * 9) & (c < 100)).any()
    assert {(c["C"] == 0, c["T"] == 0) for c in WARP} == {(False, False), (True, False), (False, True)}
    zoom, affine, warp = G.two_pass_cases()
    assert int(np.prod(zoom["patch"])) > G.CAP_ZOOM and int(np.prod(affine["patch"])) > G.CAP_ZOOM and int(np.prod(warp["patch"])) > G.CAP_WARP


def test_exact_family_is_exact():
    """the float64 result of every exact case is a float32, its bars are 0, and the emulated kernel order reproduces it bit for bit"""
    count = 0
    for case in G.all_cases():
        if case["family"] != "exact":
            continue
        ref, emu = G.run(case), G.run(case, "emu")
        for key in ("data", "target"):
            if ref[key] is None:
                continue
            assert np.array_equal(ref[key].astype(np.float32).astype(np.float64), ref[key]), (case["name"], key)
            assert not ref["bar_" + key].any(), (case["name"], key)
            assert np.array_equal(emu[key].astype(np.float64), ref[key]), (case["name"], key)
            count += 1
    assert count > 150


def test_emulated_kernel_order_stays_below_the_bars():
    worst = {}
    for case in G.all_cases():
        if case["family"] != "real":
            continue
        ref = G.run(case)
        runs = [("fused", G.run(case, "emu"))]
        if case["kind"] == "warp":
            runs.append(("unfused", G.run(case, "emu", fused=False)))
        for form, emu in runs:
            for key in ("data", "target"):
                if ref[key] is None:
                    continue
                ratio, _ = G.worst_ratio(emu[key], ref[key], ref["bar_" + key])
                k = (case["kind"], key, form)
                if ratio >= worst.get(k, (-1.0, ""))[0]:
                    worst[k] = (ratio, case["name"])
    for k in sorted(worst):
        print("emulated worst error / bar  %-24s %.3f  (%s)" % (" ".join(k), worst[k][0], worst[k][1]))
    assert len(worst) == 8 and all(r < 1.0 for r, _ in worst.values()), worst
    assert worst[("warp", "target", "fused")][0] == 0.0 and min(worst[k][0] for k in worst if k[1] == "data") > 0.05      # the bars are not slack by orders


# ---------------------------------------------------------------------------------------------------------------- mutants
MUTANT_CASES = (("whole_sample_reflect", "zoom real 5x7x9 s0", None), ("whole_sample_reflect", "warp real 5x7x9 smooth", None),
                ("reflect_no_period", "zoom real 5x7x9 s2", None), ("reflect_no_period", "warp real 5x7x9 far", None),
                ("swap_weights", "zoom real 5x7x9 s0", None), ("swap_weights", "affine real 5x7x9 rot3", None), ("swap_weights", "warp real 5x7x9 smooth", None),
                ("swap_q", "zoom real flags 8", None), ("swap_q", "affine real flags 13", None), ("swap_q", "warp real flags 9", None),
                ("flip_after_transpose", "zoom real flags 9", None), ("flip_after_transpose", "affine real flags 10", None),
                ("flip_after_transpose", "warp real flags 13", None),
                ("drop_crop_lo", "zoom real flush 1", None), ("tc_1_plus_2", "zoom real flags 0", None), ("tc_1_plus_2", "affine real flags 2", None),
                ("neighbour_gain", "zoom real C=3", None), ("neighbour_gain", "warp real 5x7x9 smooth", None),
                ("neighbour_bias", "affine real flags 4", None), ("neighbour_bias", "warp real flags 3", None),
                ("mean_before_fill", "affine real edge low", None), ("clamp_to_edge", "affine real edge high", None),
                ("trunc_not_floor", "affine real edge mixed", None), ("trunc_not_floor", "warp real 5x7x9 edge", None),
                ("round_half_even", "warp real 5x7x9 edge", None),
                ("second_pass_repeats", "zoom real 5x7x9 s1", 256), ("second_pass_repeats", "affine real 11x12x21 rot0", 2048),
                ("second_pass_repeats", "warp real 11x12x21 smooth", 2048),
                ("box_forgets_lo", "zoom real 5x7x9 s1", None), ("box_forgets_lo", "affine exact 5x7x9 perm0", None))


@pytest.mark.parametrize("mutant,name,cap", MUTANT_CASES, ids=["%s on %s" % (m, n) for m, n, _ in MUTANT_CASES])
def test_mutant_exceeds_its_bar(mutant, name, cap):
    case = G.by_name(name)
    ref, bad = G.run(case), G.run(case, mutant=mutant, cap=cap)
    ratios = [G.worst_ratio(bad[key], ref[key], ref["bar_" + key])[0] for key in ("data", "target") if ref[key] is not None]
    assert max(ratios) > 1.0, (mutant, name, ratios)
    if cap is not None:
        assert int(np.prod(case["patch"])) > cap


def test_every_mutant_is_caught():
    assert {m for m, _, _ in MUTANT_CASES} == set(G.MUTANTS)


# ---------------------------------------------------------------------------------------------------------------- the Python refusals
def fake_case(patch):
    return types.SimpleNamespace(image=torch.zeros((1, 4, 4, 4)), label=torch.zeros((4, 4, 4), dtype=torch.uint8), soft=None, mean=[0.0], std=[1.0],
                                 patch_size=patch)


def params(scale):
    return dict(crop_lo=np.zeros(3, np.int32), scale=np.asarray(scale, np.float64), flips=[False] * 3, transpose=False, gain=[1.0], bias=[0.0])


@pytest.mark.parametrize("scale,patch,message", [((1.0, np.inf, 1.0), (2, 2, 2), r"scale\[1\] is not finite"),
                                                 ((1.0, 1.0, 2.0 ** 30), (2, 2, 2), r"scale\[2\] \* \(patch\[2\] - 1\) = .* reaches 2\^30"),
                                                 ((2.0 ** 28, 1.0, 1.0), (5, 2, 2), r"scale\[0\] \* \(patch\[0\] - 1\)"),
                                                 ((1.0e300, 1.0, 1.0), (3, 1, 1), r"scale\[0\]")])
def test_python_wrappers_refuse_a_scale_the_kernel_cannot_hold(scale, patch, message):
    """before any launch, and before anything touches a device: the case here lives on the CPU"""
    from brats2019_amd import dataloader as DL
    with pytest.raises(ValueError, match=message):
        DL.augment_patch(fake_case(patch), params(scale), patch)
    with pytest.raises(ValueError, match=message):
        DL._check_batch(patch, [params((1.0, 1.0, 1.0)), params(scale)])
    DL._check_zoom_scale((2.0 ** 30 - 1.0, 1.0, 5.25), (2, 2, 2))                           # the largest coordinate below 2^30 passes
    DL._check_batch(patch, [dict(params(scale), rotation=dict(matrix=np.eye(3)))])          # the affine pass does not read `scale` with a matrix
