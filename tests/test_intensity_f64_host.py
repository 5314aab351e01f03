"""The CPU half of the float64 hold on the intensity augmentation (tests/intensity_inputs.py; the device half is tests/test_intensity_f64.py): the
restatement against `dataloader.intensity_augment_host` and scipy, the constructed noise draws, the emulation of the kernels' float32 order under
the per-voxel bars on every case and every voxel, the exact family on the emulation, and the mutants.

The restatement differs from `intensity_augment_host` only in the parameters it holds in float32, and each such rounding is bounded by a term the
bar already carries for the arithmetic rounding of the same product (a weight: 2^-24 S of the (2r + 1) 2^-24 S; t: rnd(t (x1 - x0)); sd: rnd(sd n);
brightness, the contrast factor: the product's rnd; gamma: t^g ln2 |g log2 t| 2^-24 of the (1 + ULP_LOG2) allowed; a statistic's float32 load: `_load`;
1e-7f - 1e-7 = 1.2e-15).  The tolerance of that comparison is built from exactly those terms (`against="host"` in intensity_inputs: each float32
parameter one 2^-24 of the product it enters, every arithmetic rounding 2^-52 for the two float64 sides), carried through the stages like the bars:
a radius-8 blur is tied to one 2^-24 S per axis, not to 17.  The emulation's worst error / bar over all cases is 0.9995 -- a lone float32 product just above a power of two, where one rounding
reaches 2^-24 of its value (brightness-only channels, bit-equal on the device)."""
import math

import numpy as np
import pytest
from scipy import ndimage as ndi

import intensity_inputs as I

CASES = I.cases()
ids = [c["name"] for c in CASES]


def test_case_list_reaches_every_branch():
    shapes = {c["shape"] for c in CASES}
    assert {(1, 1, 1), (1, 1, 4), (5, 6, 7), (17, 3, 8), (3, 34, 132), (2, 33, 131), (8, 16, 64), (3, 3, 911), (16, 40, 24), (130, 128, 128)} <= shapes
    assert {c["C"] for c in CASES} == {1, 4, 8} and {c["family"] for c in CASES} == set(I.FAMILIES)
    assert {(c["family"], c["C"]) for c in CASES} >= {(f, n) for f in I.FAMILIES for n in (1, 4, 8)}
    used = lambda key: {q[key] for c in CASES for q in c["params"] if key in q}
    assert used("gamma") >= set(I.GAMMAS) and used("contrast") >= set(I.CONTRASTS) and used("blur_sigma") >= set(I.SIGMAS) and used("lowres_zoom") >= set(I.ZOOMS)
    assert [I.radius(s) for s in I.SIGMAS] == [2, 2, 4, 8]
    combos = {(q["gamma"], bool(q.get("gamma_invert")), bool(q.get("gamma_retain_stats"))) for c in CASES for q in c["params"] if "gamma" in q}
    assert len(combos) == 20
    assert any(q.get("noise_seed", 0) >= 1 << 63 for c in CASES for q in c["params"])
    seen = {launch: 0 for launch in I.LAUNCHES}
    for c in CASES:                                            # every launch a case of several channels makes sees a channel that leaves at once beside one that works
        if c["C"] > 1:
            for launch in I.LAUNCHES:
                part = [I.takes_part(q, launch) for q in c["params"]]
                if any(part):                                  # (no channel: the entry does not launch it)
                    assert not all(part), (c["name"], launch)
                    seen[launch] += 1
    assert all(n >= 8 for n in seen.values()), seen
    kinds = {frozenset(q) for c in CASES if c["C"] > 1 for q in c["params"]}
    assert frozenset() in kinds and frozenset({"blur_sigma"}) in kinds and frozenset({"brightness"}) in kinds
    assert any("lowres_zoom" in k and "gamma" in k and "contrast" not in k for k in kinds) and any("noise_variance" in k and "contrast" in k and "gamma" not in k for k in kinds)
    # the branches by their arithmetic: tile rows / columns of 32 x 128, 16-output column blocks, chunks of 8192, 256 partials per round
    cdiv = lambda a, b: -(-a // b)
    assert cdiv(34, 32) == 2 and cdiv(132, 128) == 2 and 132 % 4 == 0 and 131 % 4 == 3 and cdiv(17, 16) == 2
    assert 8 * 16 * 64 == I.CHUNK and 3 * 3 * 911 == I.CHUNK + 7 and cdiv(130 * 128 * 128, I.CHUNK) == 260
    assert I.is_vec(I.by_name("tiles float4")) and not I.is_vec(I.by_name("tiles scalar")) and not I.is_vec(I.by_name("align in+1")) and not I.is_vec(I.by_name("align out+1"))


def test_mix64_inverts_and_the_constructed_seeds_give_their_draws():
    r = np.random.default_rng(5)
    for z in [0, 1, I.M64] + [int(v) for v in r.integers(0, 1 << 63, 64)]:
        assert I.unmix64(I.mix64(z)) == z and I.mix64(I.unmix64(z)) == z
    from brats2019_amd import dataloader as DL
    for name, (which, _, u) in I.NOISE_EDGES.items():
        for channel in range(4):
            seed = I.edge_seed(name, channel)
            u1, u2 = I.draws(seed, channel, 3)
            assert (u1[0] if which == 1 else u2[0]) == u, name
            n = DL.intensity_noise_host(seed, channel, 3)
            want = math.sqrt(-2.0 * math.log(u1[0])) * math.cos(2.0 * math.pi * u2[0])
            assert abs(n[0] - want) <= 1e-12, name
    assert float(np.float32(1.0 - 2.0 ** -30)) == 1.0 and float(np.float32(1.0 - 2.0 ** -24)) < 1.0
    u1, _ = I.draws(I.edge_seed("u1 = 2^-53", 2), 2, 1)
    assert abs(math.sqrt(-2.0 * math.log(u1[0])) - 8.5718) < 1e-3
    for name in ("u1 = 1 - 2^-30", "u1 = 1 - 2^-24", "u1 = 2^-53"):       # the u1 edges come with a cosine that shows them
        seed = I.edge_seed(name, 1)
        assert abs(math.cos(2.0 * math.pi * I.draws(seed, 1, 1)[1][0])) > 0.5


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_restatement_against_the_host_oracle(case):
    """|restatement - dataloader.intensity_augment_host| within the parameter roundings (module docstring), every case and every voxel"""
    from brats2019_amd import dataloader as DL
    ref = I.run(case, against="host")
    with np.errstate(all="ignore"):
        host = DL.intensity_augment_host(I.input_of(case["name"]), case["params"])
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["bar"]).all() and np.isfinite(host).all()
    assert np.array_equal(ref["out"], I.reference(case["name"])["out"])
    ratio, where = I.worst_ratio(host, ref["out"], ref["bar"])
    assert ratio <= 1.0, (case["name"], ratio, where, host[where], ref["out"][where], ref["bar"][where])


def test_the_host_tolerance_is_the_parameter_roundings():
    """far below the device bars wherever arithmetic dominates (a radius-8 blur: one 2^-24 S per axis against 17), and 0 where no parameter is rounded"""
    x = I.input_of("tiles float4")[0]
    _, bar = I.ref_channel(x, dict(blur_sigma=2.0), 0)
    _, tol = I.ref_channel(x, dict(blur_sigma=2.0), 0, against="host")
    assert (tol < bar / 10).all() and (tol > 0).all()
    _, tol = I.ref_channel(x, dict(brightness=1.25, contrast=0.75), 0, against="host")          # exact parameters: only the loaded statistics are rounded
    assert float(tol.max()) <= 8 * I.U * float(np.abs(x).max())


@pytest.mark.parametrize("sigma", I.SIGMAS)
def test_blur_restatement_against_scipy(sigma):
    for name in ("tiles float4", "tiles scalar", "grid 5x6x7 C4 offset"):
        x = I.input_of(name)[0]
        got, tol = I.ref_channel(x, dict(blur_sigma=sigma), 0, against="host")          # one 2^-24 S per axis for the float32 weights, 2^-52 per float64 rounding
        want = ndi.gaussian_filter(x.astype(np.float64), sigma, mode="reflect")
        ratio, where = I.worst_ratio(want, got, tol)
        assert ratio <= 1.0, (name, sigma, ratio, where)


@pytest.mark.parametrize("zoom", I.ZOOMS)
def test_lowres_restatement_against_scipy_zoom(zoom):
    """nearest-neighbour down and linear up as two scipy zooms (grid_mode), within rnd(t d) per lerp for the float32 t"""
    for name in ("tiles float4", "tiles scalar", "grid 5x6x7 C4 offset", "lowres scalar"):
        x = I.input_of(name)[0].astype(np.float64)
        nc = [I.lowres_axis(n, zoom)[3] for n in x.shape]
        coarse = ndi.zoom(x, [a / b for a, b in zip(nc, x.shape)], order=0, mode="nearest", grid_mode=True)
        assert coarse.shape == tuple(nc)
        want = ndi.zoom(coarse, [b / a for a, b in zip(nc, x.shape)], order=1, mode="nearest", grid_mode=True)
        got, tol = I.ref_channel(I.input_of(name)[0], dict(lowres_zoom=zoom), 0, against="host")
        # scipy forms its coordinate and weights in float64 with a few roundings of its own on a coordinate of up to 132: 2^-44 of the local difference scale
        ratio, where = I.worst_ratio(want, got, tol + 2.0 ** -44 * np.abs(x).max())
        assert ratio <= 1.0, (name, zoom, ratio, where)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_emulation_lies_under_the_bars(case):
    ref, emu = I.reference(case["name"]), I.run(case, "emu")
    assert emu.dtype == np.float32 and np.isfinite(emu).all() and np.isfinite(ref["bar"]).all()
    for c, q in enumerate(case["params"]):
        ratio, where = I.worst_ratio(emu[c], ref["out"][c], ref["bar"][c])
        assert ratio < 1.0, (case["name"], c, q, ratio, where, emu[c][where], ref["out"][c][where], ref["bar"][c][where])


def test_bars_are_roundings_not_tolerances():
    """on unit-variance data a single stage's bar is worth at most 64 float32 roundings of the channel's largest value at the median voxel (blur radius
    8: 3 x 17) and a chain up to contrast at most 256.  Gamma is left to its formula: t^g is not Lipschitz at 0, and retain-stats multiplies by std_x / std_y"""
    seen = 0
    for case in CASES:
        if case["family"] != "unit" or case["shape"] == (130, 128, 128) or int(np.prod(case["shape"])) < 100:      # (a range of 0 or of a few voxels: 1 / 1e-7)
            continue
        ref = I.reference(case["name"])
        for c, q in enumerate(case["params"]):
            stages = len(set(q) & {"blur_sigma", "lowres_zoom", "noise_variance", "brightness", "contrast", "gamma"})
            scale = max(float(np.abs(ref["out"][c]).max()), 1.0)
            units = float(np.median(ref["bar"][c])) / (I.U * scale)
            seen += stages == 1
            if "gamma" not in q:
                assert units <= (64 if stages <= 1 else 256), (case["name"], c, q, units)
    assert seen >= 10


def test_exact_family_on_the_emulation():
    cache = {}

    def result(name):
        if name not in cache:
            cache[name] = I.run(I.by_name(name), "emu")
        return cache[name]
    I.exact_family(result)


def test_the_two_routes_load_the_same_float32_statistics():
    """the premise of 'the 16-byte route and the scalar route give the same bytes': their float64 sums differ in order, not after the float32 load"""
    x = I.input_of("align base")
    for c in range(4):
        a, b = I.stats_emu(x[c], True), I.stats_emu(x[c], False)
        assert all(np.float32(u) == np.float32(v) for u, v in zip(a, b)) and a[2:] == b[2:]
        assert abs(a[0] - float(x[c].astype(np.float64).mean())) <= I.SUM64 * float(np.abs(x[c]).mean())


@pytest.mark.parametrize("mutant", sorted(I.MUTANTS))
def test_mutant_is_caught(mutant):
    name = I.MUTANTS[mutant]
    case, ref = I.by_name(name), I.reference(name)
    with np.errstate(all="ignore"):
        emu = I.run(case, "emu", mutant)
    ratio, where = I.worst_ratio(emu, ref["out"], ref["bar"])
    print("%-36s on %-24s worst error / bar = %.3g" % (mutant, name, ratio))
    assert ratio > 1.0 or not np.isfinite(emu).all(), (mutant, name, ratio)


def test_there_are_at_least_18_mutants():
    assert len(I.MUTANTS) >= 18 and all(I.by_name(n) for n in I.MUTANTS.values())
