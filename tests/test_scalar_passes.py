"""The scalar-producing passes of csrc/pointwise.hip and csrc/inference.hip on the device, one entry at a time through the op-level C-ABI, against the float64
restatements of tests/test_scalar_passes_host.py -- its cases, its inputs, its bars (derived there from the roundings of each kernel as written), its exact family.

Criterion: ru_criterion_sums at one voxel, on both sides of 256 and of the 8192-voxel tile, with N > 1, C > 1 and three tiles together, on the exact family (inter and
union bit for bit) and the real one (hard and soft targets, bg_weight 1e-2, 1, 0); ru_criterion_value and ru_criterion_value_device at relative 1e-14 for 1, 3 and 64
classes, zero sums, a priority and three weightings, 65 classes refused; ru_criterion_grad for five classes, odd V and the wrap of its grid-stride loop, finite everywhere.
Dice: ru_dice_counts equal to numpy's integers on both routes, past the 64-workgroup cap, with 1/2, nextafter(1/2), NaN, +inf and -0.0 planted; ru_dice_accumulate equal
to its float32 restatement by bit pattern, twice in a row, acc[nacc:] untouched.  Moments: ru_zscore_stats and ru_case_stats, count exact, sums within the bar.  Flat and
layout passes: ru_sigmoid_fwd within its bar (NaN in, NaN out), ru_leaky_relu_fwd / _bwd and ru_layout_convert by bit pattern.  Merge: ru_tta_merge, ru_tta_merge_box,
ru_compose_labels by bit pattern and integer.

Every entry is called through brats2019_amd._lib with outputs this file allocates: float outputs filled with NaN, integer outputs with 0xA5 bytes, one guard element in
front of and behind the small ones (GUARD_WORDS behind a layout output); workspaces come from GuardedWorkspace and every test that takes one ends with intact().  Each
test prints its worst error / bar.

The device's logf and expf, measured on the MI355X by a stand-alone program built with the library's flags on every distinct argument these tests hand them (853 364
and 7 931 419), against float64 log / exp: logf worst 3.13 units of 2^-24 |y| = 2.14 ulp (at x = 0.018077), expf worst 1.39 units = 0.84 ulp.  The bars carry each
rounded up, plus one: LOGF_UNITS = 5, EXPF_UNITS = 3.

Measured on the MI355X, worst error / bar over the cases of a group (every exact-family, integer and bit-pattern comparison: 0 differences): criterion sums 0.044 (the BCE
sum alone 0.040), value 0.022 (host form, 64 classes; the device form 0), gradient 0.28, z-score 0.11, case statistics 0.13, sigmoid 0.48."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_scalar_passes_host as H
from op_cases import PATTERN, GuardedWorkspace
from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from brats2019_amd import _lib as L
    L.require_gpu()
    return L.load()


def call(lib, name, *args):
    from brats2019_amd import _lib as L
    L.check(getattr(lib, name)(*args), name)


def stream():
    from brats2019_amd import _lib as L
    return L.stream()


def P(t, skip=0):
    return C.c_void_p(t.data_ptr() + skip * t.element_size())


_ALIVE = []


def dev(a):
    """a device copy that lives until the test ends: the entries get its address, not the tensor"""
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return _ALIVE[-1]


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def filled(n, dtype):
    """n + 2 elements: NaN (float) or 0xA5 bytes (integer); the entry gets the n in the middle"""
    if dtype.is_floating_point:
        return torch.full((n + 2,), NAN, dtype=dtype, device="cuda")
    return torch.full(((n + 2) * torch.empty(0, dtype=dtype).element_size(),), PATTERN, dtype=torch.uint8, device="cuda").view(dtype)


def inner(t):
    """the n elements the entry had, on the host; the two guards must be what they were"""
    h = t.cpu()
    raw = h.view(torch.uint8).reshape(h.numel(), -1)
    if t.dtype.is_floating_point:
        assert bool(torch.isnan(h[0])) and bool(torch.isnan(h[-1])), "guard element overwritten"
    else:
        assert bool((raw[0] == PATTERN).all()) and bool((raw[-1] == PATTERN).all()), "guard element overwritten"
    return h[1:-1].numpy()


def ints3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def report(what, ex):
    print("  %-64s worst error / bar %.3g" % (what, ex))
    return ex


# ---------------------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("case", H.SUM_CASES, ids=H.case_id)
def test_criterion_sums(case, lib):
    n, c, v = case
    ws = GuardedWorkspace()
    for family, targets, bgw in [("exact", "hard", H.BGW)] + [("real", t, b) for t, b in H.SUM_VARIANTS]:
        p, g = H.crit_inputs(case, family, targets)
        out = filled(2 * c + 1, torch.float64)
        buf = ws(lib.ru_criterion_workspace_bytes(n, c, v), "cuda")
        call(lib, "ru_criterion_sums", P(dev(p)), P(dev(g)), P(out, 1), n, c, v, bgw, P(buf), buf.numel(), stream())
        got, ref = inner(out), H.ref_sums(p, g, bgw)
        if family == "exact":
            assert H.same_f64(got[:2 * c], ref[:2 * c]), (case, got, ref)
        bar = H.sums_bars(p, g, bgw)
        ex = report("sums %s %s %s bgw %g" % (H.case_id(case), family, targets, bgw), H.excess(got, ref, bar))
        report("   of which the BCE sum", H.excess(got[2 * c:], ref[2 * c:], bar[2 * c:]))
        assert ex <= 1.0, (case, family, targets, bgw, got, ref, bar)
    assert ws.intact()


def test_criterion_value_host_and_device(lib):
    from brats2019_amd import _lib as L
    worst = 0.0
    for case in H.value_cases():
        c, s = case["c"], case["sums"]
        dice, bce = C.c_double(NAN), C.c_double(NAN)
        call(lib, "ru_criterion_value", (C.c_double * len(s))(*s), c, case["count"], case["priority"], C.byref(dice), C.byref(bce))
        worst = max(worst, report("value host %s" % case["name"], H.rel_excess([dice.value, bce.value], H.ref_value(case, 0.5, 0.5)[1:])))
        for w in H.VALUE_WEIGHTS:
            out = filled(3, torch.float64)
            call(lib, "ru_criterion_value_device", P(dev(s)), c, case["count"], case["priority"], w[0], w[1], P(out, 1), stream())
            got, ref = inner(out), H.ref_value(case, *w)
            if case["name"] == "C3_zero":
                assert got[1] == 0.0 and got[0] == 0.0
            worst = max(worst, report("value device %s w %s" % (case["name"], w), H.rel_excess(got, ref)))
    assert worst <= 1.0
    out = filled(3, torch.float64)
    rc = lib.ru_criterion_value_device(P(dev(np.ones(131))), 65, 1.0, 1.0, 0.5, 0.5, P(out, 1), stream())
    assert rc == -1 and "ru_criterion_value_device: bad argument" in L.last_error()
    assert np.isnan(inner(out)).all()


@pytest.mark.parametrize("case", H.GRAD_CASES, ids=H.case_id)
def test_criterion_grad(case, lib):
    n, c, v = case
    inp = H.grad_inputs(case)
    out = filled(n * c * v, torch.float32)
    call(lib, "ru_criterion_grad", P(dev(inp["p"])), P(dev(inp["g"])), P(dev(inp["sums"])), inp["count"], 0.5, 0.5, H.BGW, 1.0, P(out, 1), n, c, v, stream())
    got = inner(out).reshape(n, c, v)
    dp, bar = H.ref_grad(inp)
    assert np.isfinite(got).all()
    ex = report("gradient %s" % H.case_id(case), H.excess(got, dp, bar))
    assert ex <= 1.0, (case, ex)


# ---------------------------------------------------------------------------------------------------------------- Dice metric
@pytest.mark.parametrize("v", H.DICE_V)
def test_dice_counts(v, lib):
    for rows in H.DICE_ROWS:
        n, c = rows
        p, g = H.dice_inputs(rows, v)
        out = filled(n * c * 2, torch.int64)
        call(lib, "ru_dice_counts", P(dev(p)), P(dev(g)), P(out, 1), n, c, v, stream())
        got, ref = inner(out).reshape(n, c, 2), H.ref_counts(p, g)
        report("counts %dx%d V %d (rows that differ: %d)" % (n, c, v, int((got != ref).any(-1).sum())), 0.0 if np.array_equal(got, ref) else float("inf"))
        assert np.array_equal(got, ref), (rows, v, got, ref)
        if v == 1023 and rows == (2, 3):                          # below 2^24: the metric of the oracle, through the device's own accumulation
            acc = torch.zeros(3, dtype=torch.float64, device="cuda")
            call(lib, "ru_dice_accumulate", P(out, 1), P(acc), n, c, 3, stream())
            assert np.array_equal(acc.cpu().numpy(), O.dice_metric(p, g))


def test_dice_accumulate(lib):
    for case in H.accumulate_cases():
        counts, nacc = case["counts"], case["nacc"]
        n, c = counts.shape[:2]
        acc = filled(c, torch.float64)
        acc[1:-1] = dev(H.accumulate_start(c))
        ref = H.accumulate_start(c)
        for round_ in (1, 2):                                     # the second call adds onto the first
            call(lib, "ru_dice_accumulate", P(dev(counts)), P(acc, 1), n, c, nacc, stream())
            ref = H.ref_accumulate(counts, ref, nacc)
            got = inner(acc)
            same = np.array_equal(got.view(np.int64), ref.view(np.int64))
            report("accumulate %s call %d" % (case["name"], round_), 0.0 if same else float("inf"))
            assert same, (case["name"], round_, got, ref)
        assert np.array_equal(got[nacc:], H.accumulate_start(c)[nacc:])


# ---------------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("case", H.ZS_CASES, ids=H.case_id)
def test_zscore_stats(case, lib):
    c, v = case
    ws = GuardedWorkspace()
    x = H.zs_inputs(c, v)
    out = filled(c * 3, torch.float64)
    buf = ws(lib.ru_zscore_workspace_bytes(c, v), "cuda")
    call(lib, "ru_zscore_stats", P(dev(x)), P(out, 1), c, v, P(buf), buf.numel(), stream())
    got, ref = inner(out).reshape(c, 3), H.ref_moments(x)
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    ex = report("z-score %s" % H.case_id(case), H.moments_excess(got, ref, H.moments_bars(x)))
    assert ex <= 1.0, (case, got, ref)
    assert ws.intact()


@pytest.mark.parametrize("case", H.CASE_STATS_CASES, ids=lambda k: "C%d_%s_%s_%s" % (k[0], H.case_id(k[1]), H.case_id(k[2]), H.case_id(k[3])))
def test_case_stats(case, lib):
    c, dims, lo, size = case
    ws = GuardedWorkspace()
    img = H.case_image(c, dims)
    out = filled(c * 3, torch.float64)
    buf = ws(lib.ru_case_workspace_bytes(c, *dims), "cuda")
    call(lib, "ru_case_stats", P(dev(img)), P(out, 1), c, dims[0], dims[1], dims[2], ints3(lo), ints3(size), P(buf), buf.numel(), stream())
    box = H.crop(img, lo, size)
    got, ref = inner(out).reshape(c, 3), H.ref_moments(box)
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    ex = report("case stats %s %s in %s" % (lo, size, dims), H.moments_excess(got, ref, H.moments_bars(box)))
    assert ex <= 1.0, (case, got, ref)
    assert ws.intact()


# ---------------------------------------------------------------------------------------------------------------- flat and layout passes
@pytest.mark.parametrize("n", H.FLAT_N)
def test_sigmoid(n, lib):
    x = H.flat_inputs(n)
    out = filled(n, torch.float32)
    call(lib, "ru_sigmoid_fwd", P(dev(x)), P(out, 1), n, stream())
    got = inner(out)
    assert np.array_equal(np.isnan(got), np.isnan(x))
    ex = report("sigmoid n %d" % n, H.sigmoid_excess(got, x))
    assert ex <= 1.0, (n, ex)


@pytest.mark.parametrize("n", H.FLAT_N)
def test_leaky_relu_pair_is_torch_bit_for_bit(n, lib):
    y, dy = H.lrelu_inputs(n)
    out = filled(n, torch.float32)
    call(lib, "ru_leaky_relu_fwd", P(dev(y)), P(out, 1), n, H.SLOPE, stream())
    fwd = np.array_equal(H.bits32(inner(out)), H.bits32(H.ref_lrelu(y)))
    out = filled(n, torch.float32)
    call(lib, "ru_leaky_relu_bwd", P(dev(y)), P(dev(dy)), P(out, 1), n, H.SLOPE, stream())
    bwd = np.array_equal(H.bits32(inner(out)), H.bits32(H.ref_lrelu_bwd(y, dy)))
    report("LeakyReLU n %d forward %s backward %s" % (n, fwd, bwd), 0.0 if fwd and bwd else float("inf"))
    assert fwd and bwd


@pytest.mark.parametrize("case", H.LAYOUT_CASES, ids=H.case_id)
def test_layout_convert_is_a_permutation_of_bit_patterns(case, lib):
    n, c, v = case
    total = n * c * v
    src = H.layout_inputs(case).reshape(-1)
    for to_c16 in (1, 0):
        out = torch.full((total + H.GUARD_WORDS,), H.NAN_BITS, dtype=torch.int32, device="cuda")
        call(lib, "ru_layout_convert", P(dev(src)), P(out), n, c, v, to_c16, stream())
        got, ref = out.cpu().numpy(), H.ref_layout(src, case, to_c16)
        same = np.array_equal(got, ref)
        report("layout %s to_c16 %d (words that differ: %d)" % (H.case_id(case), to_c16, int((got != ref).sum())), 0.0 if same else float("inf"))
        assert same
        if to_c16:
            assert np.array_equal(got[:total], H.torch_layout(src, case, 1))
            src = got[:total].copy()                              # back again: what comes out is the input
    assert np.array_equal(got[:total], H.layout_inputs(case).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- inference merge
@pytest.mark.parametrize("k", sorted(H.MERGE_FLIPS))
def test_tta_merge_and_its_box_form(k, lib):
    c, d, h, w = H.MERGE_SHAPE
    probs, flips = H.merge_inputs(k), H.MERGE_FLIPS[k]
    word = H.flips_word(flips)
    mean, mask, counts = H.ref_merge(probs, flips)
    dprobs = dev(probs)
    for lo, size in [((0, 0, 0), (d, h, w))] + H.MERGE_BOXES + [(None, None)]:
        vb = d * h * w if lo is None else int(np.prod(size))
        om, ok, oc = filled(c * vb, torch.float32), filled(c * vb, torch.uint8), filled(c, torch.int64)
        if lo is None:
            call(lib, "ru_tta_merge", P(dprobs), k, word, P(om, 1), P(ok, 1), P(oc, 1), c, d, h, w, stream())
            rm, rk = mean, mask
        else:
            call(lib, "ru_tta_merge_box", P(dprobs), k, word, P(om, 1), P(ok, 1), P(oc, 1), c, d, h, w, ints3(lo), ints3(size), stream())
            rm, rk = H.box_of(mean, lo, size), H.box_of(mask, lo, size)
        rc = rk.reshape(c, -1).sum(1).astype(np.int64)
        same = (np.array_equal(H.bits32(inner(om)), H.bits32(rm).reshape(-1)), np.array_equal(inner(ok), rk.reshape(-1)), np.array_equal(inner(oc), rc))
        report("merge K %d box %s mean / mask / counts equal: %s" % (k, (lo, size) if lo else "none (ru_tta_merge)", same), 0.0 if all(same) else float("inf"))
        assert all(same), (k, lo, size, same)
    assert np.array_equal(rc, counts) and not mask[:, 1, 2, 3].any() and mask[:, 3, 2, 1].all()


def test_compose_labels_at_the_et_threshold(lib):
    for n_et in (H.ET_MIN, H.ET_MIN + 1):
        mask, counts = H.label_inputs(n_et)
        v = mask[0].size
        out = filled(v, torch.uint8)
        call(lib, "ru_compose_labels", P(dev(mask)), P(dev(counts)), H.ET_MIN, P(out, 1), v, stream())
        got, ref = inner(out), H.ref_labels(mask).reshape(-1)
        same = np.array_equal(got, ref)
        report("labels with %d ET voxels, et_min %d: label 4 %s" % (n_et, H.ET_MIN, bool((got == 4).any())), 0.0 if same else float("inf"))
        assert same and bool((got == 4).any()) == (n_et > H.ET_MIN)
