"""NSD, ASSD and the Hausdorff distance on the device (csrc/surface.hip, ru_surface_distances; csrc/lesion.hip, ru_lesion_distances)
against the float64 restatements of brats2019_amd/metrics.py, on the case set of tests/test_nsd_host.py at the grids where the finalize
kernel can go wrong: 57 bins (fewer than its 1024 threads), bins that are no multiple of the threads, rows that end on and just beyond a
64-bit word, and uint8 label volumes.

Held: `values` and `counts` are ops.surface_metrics' bytes (and the lesion-wise summary, counts and table ops.lesion_metrics');  NSD and
HD are bitwise the restatement's (integer counts, one division; one square root); ASSD is within ASSD_ROUNDINGS(bins) * 2^-53 of the
exact sum, relative: see `assd_roundings`.  The worst relative ASSD error each test meets is printed."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_surface import soft
from test_surface_host import EMPTY, regions
from test_nsd_host import GRIDS, SQRT2, TOL8, mask_cases

T = torch.from_numpy
TOLS = [(), (1.0,), TOL8]
U = Fraction(1, 2 ** 53)                                                              # float64 unit roundoff
THREADS = 1024                                                                        # the finalize kernel's workgroup


def assd_roundings(bins):
    """The float64 roundings between the exact sum of h_b sqrt(b) over n and the kernel's ASSD, counted from the kernel: a thread adds
    its ceil(bins / 1024) consecutive terms (chunk roundings at most; the first addition, to 0.0, is exact, which leaves one spare), the
    tree adds log2(1024) = 10 levels, each term carries the square root's and the product's rounding, and one division ends it.  Every
    term is >= 0, so each rounding moves the result by at most 2^-53 of it: the bound is relative to the sum.  The spare rounding covers
    the single rounding of math.fsum, the reference sum; the division is undone exactly, in rationals."""
    return -(-bins // THREADS) + 10 + 1 + 1 + 1


def assd_error(got, hist, what):
    """relative error of the device's ASSD against fsum of the restatement's terms over n, asserted within the derived bar"""
    from brats2019_amd import metrics
    ref = Fraction(math.fsum(metrics.assd_terms_host(hist)))
    n = int(hist.sum())
    err = abs(Fraction(float(got)) * n - ref)
    if ref == 0:
        assert err == 0, what
        return 0.0
    assert err <= assd_roundings(len(hist)) * U * ref, "%s: ASSD off by %.3g relative, bar %d * 2^-53" % (what, float(err / ref), assd_roundings(len(hist)))
    return float(err / ref)


def _batches(cases, n, c):
    """the case list cut into calls of n * c pairs (the last one filled from the start): [(names, P [n, c, D, H, W], G)]"""
    per = n * c
    cases = cases + cases[:(-len(cases)) % per]
    out = []
    for i in range(0, len(cases), per):
        cut = cases[i:i + per]
        shape = cut[0][1].shape
        out.append(([x[0] for x in cut], np.stack([x[1] for x in cut]).reshape((n, c) + shape), np.stack([x[2] for x in cut]).reshape((n, c) + shape)))
    return out


def _check_extras(extras, pm, gm, tol, what, empty_value=EMPTY):
    """extras [N, K, T + 2] of masks [N, K, D, H, W] against the restatement -> worst relative ASSD error"""
    from brats2019_amd import metrics
    t, worst = len(tol), 0.0
    assert extras.shape == pm.shape[:2] + (t + 2,) and extras.dtype == np.float64, what
    for i in range(pm.shape[0]):
        for j in range(pm.shape[1]):
            p, g, got = pm[i, j], gm[i, j], extras[i, j]
            want = metrics.surface_distances_host(p, g, tol, empty_value)
            tag = "%s (%d, %d) T=%d" % (what, i, j, t)
            assert got[:t].tobytes() == want[:t].tobytes(), "%s: NSD %s != %s" % (tag, got[:t].tolist(), want[:t].tolist())
            assert got[t + 1].tobytes() == want[t + 1].tobytes(), "%s: HD %r != %r" % (tag, got[t + 1], want[t + 1])
            if p.any() and g.any():
                worst = max(worst, assd_error(got[t], metrics.surface_histogram_host(p, g), tag))
            else:
                assert got[t] == want[t], tag
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,shape", GRIDS, ids=["3x5x7", "17x19x37", "9x64x64", "5x6x130"])
def test_extras_on_the_case_set(n, c, shape):
    from brats2019_amd import ops
    rng = np.random.default_rng(41)
    bins = sum((s - 1) ** 2 for s in shape) + 1
    assert (shape != (3, 5, 7) or bins == 57 < THREADS) and (shape != (17, 19, 37) or bins % THREADS)
    worst = 0.0
    for names, pm, gm in _batches(mask_cases(shape), n, c):
        pred, gr = T(soft(rng, pm)).cuda(), T(soft(rng, gm)).cuda()
        base = ops.surface_metrics(pred, gr)
        for tol in TOLS:
            got = ops.surface_distances(pred, gr, tol)
            again = ops.surface_distances(pred, gr, tol)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), names
            assert all(torch.equal(a, b) for a, b in zip(got, again)), names       # two calls: identical bytes
            assert got[2].is_cuda and got[2].dtype == torch.float64
            worst = max(worst, _check_extras(got[2].cpu().numpy(), pm, gm, tol, "%s %s" % (shape, names)))
        other = ops.surface_distances(pred, gr, (SQRT2,), empty_value=50.0)
        assert torch.equal(other[0], ops.surface_metrics(pred, gr, 50.0)[0])
        worst = max(worst, _check_extras(other[2].cpu().numpy(), pm, gm, (SQRT2,), "%s %s, empty_value 50" % (shape, names), 50.0))
    print("grid %s: %d bins, bar %d * 2^-53 = %.3g, worst relative ASSD error %.3g" % (shape, bins, assd_roundings(bins), assd_roundings(bins) * float(U), worst))


def _labels(rng, shape):
    lab = rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), size=shape, p=[0.6, 0.1, 0.15, 0.05, 0.1])
    lab[:, 2:9, 4:15, 10:50] = 2
    lab[:, 4:8, 6:12, 20:40] = 1
    lab[:, 5:7, 8:11, 25:33] = 4
    return lab


@pytest.mark.gpu
def test_uint8_label_volumes_and_tolerances_beyond_the_bins():
    from brats2019_amd import ops
    rng = np.random.default_rng(42)
    shape = (2, 12, 20, 70)
    lab = _labels(rng, shape)
    pre = lab.copy()
    flip = rng.random(shape) < 0.1
    pre[flip] = rng.integers(0, 5, size=int(flip.sum()))
    pre[1][regions(pre[1])[2]] = 2                                                    # sample 1 predicts no ET: one empty mask
    dp, dg = T(pre).cuda(), T(lab).cuda()
    base = ops.surface_metrics(dp, dg)
    worst = 0.0
    for tol in TOLS + [(1e9, 8.0, 1e-300)]:
        got = ops.surface_distances(dp, dg, tol)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and got[2].shape == (2, 3, len(tol) + 2)
        worst = max(worst, _check_extras(got[2].cpu().numpy(), regions(pre), regions(lab), tol, "labels"))
    ex = ops.surface_distances(dp, dg, (1.0,))[2].cpu().numpy()
    assert ex[1, 2].tolist() == [0.0, EMPTY, EMPTY] and 0 < ex[0, 0, 0] < 1
    print("labels: worst relative ASSD error %.3g" % worst)


@pytest.mark.gpu
def test_a_view_8_bytes_off_a_16_byte_boundary():
    from brats2019_amd import ops
    rng = np.random.default_rng(43)
    shape = (5, 6, 130)
    cases = mask_cases(shape)
    pm, gm = np.stack([cases[7][1], cases[6][1]])[None], np.stack([cases[7][2], cases[6][2]])[None]
    for arrs, off in [((soft(rng, pm), soft(rng, gm)), 2), ((pm[0].astype(np.uint8) * 4, gm[0].astype(np.uint8) * 4), 8)]:
        views, copies = [], []
        for a in arrs:
            buf = torch.empty(a.size + off, dtype=T(a).dtype, device="cuda")
            v = buf[off:].view(a.shape)
            v.copy_(T(a))
            assert v.is_contiguous() and v.data_ptr() % 16 == 8
            views.append(v)
            copies.append(T(a).cuda())
            assert copies[-1].data_ptr() % 16 == 0
        for tol in ((), TOL8):
            assert all(torch.equal(x, y) for x, y in zip(ops.surface_distances(*views, tol), ops.surface_distances(*copies, tol)))
        kw = dict(dilation=3, min_volume=0, want_table=True, max_lesions=256)        # the dilation joins the speckle: a handful of lesions
        a, b = ops.lesion_distances(*views, (1.0,), **kw), ops.lesion_distances(*copies, (1.0,), **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and 1 <= int(a[1][..., 0].max()) <= 24


# ---------------------------------------------------------------------- lesion-wise
def _lesion_masks(shape, rng):
    """K = 3 pairs on one grid: (0) a few lesions, one missed, one found with an offset, a false-positive component and a one-voxel
    lesion; (1) the empty pair; (2) blobs against a speckled copy (a dozen-odd lesions at dilation 0)"""
    d, h, w = shape
    g0, p0 = np.zeros(shape, bool), np.zeros(shape, bool)
    g0[1:4, 2:8, 3:11] = True                                                         # found, shifted by (0, 1, 2)
    p0[1:4, 3:9, 5:13] = True
    g0[d - 3:d, h - 6:h - 1, w - 9:w - 2] = True                                      # missed
    g0[0, h - 1, 0] = True                                                            # one voxel: dropped when min_volume >= 1
    p0[0, h - 1, 0] = True
    g0[d // 2, h // 2, w // 2 - 3:w // 2 + 3] = True                                  # found exactly
    p0[d // 2, h // 2, w // 2 - 3:w // 2 + 3] = True
    p0[d - 1, 0, w // 2:w // 2 + 2] = True                                            # a false-positive component
    z = np.zeros(shape, bool)
    g2 = np.zeros(shape, bool)
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    for _ in range(6):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(1.0, 0.2 * max(shape))
        g2 |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    p2 = np.roll(g2, (0, 1, -1), axis=(0, 1, 2)) ^ (rng.random(shape) < 0.0015)
    g2 |= rng.random(shape) < 0.0004
    return np.stack([p0, z, p2])[None], np.stack([g0, z, g2])[None]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 64, 64), (7, 19, 37)], ids=["9x64x64", "7x19x37"])
def test_lesionwise_against_the_restatement(shape):
    from brats2019_amd import metrics, ops
    rng = np.random.default_rng(44)
    pm, gm = _lesion_masks(shape, rng)
    pred, gr = T(soft(rng, pm)).cuda(), T(soft(rng, gm)).cuda()
    bins = sum((s - 1) ** 2 for s in shape) + 1
    worst = 0.0
    for dilation, min_volume in [(0, 0), (3, 0), (2, 1)]:
        kw = dict(dilation=dilation, min_volume=min_volume, want_table=True, max_lesions=64)
        base = ops.lesion_metrics(pred, gr, **kw)
        for tol in TOLS:
            t = len(tol)
            got = ops.lesion_distances(pred, gr, tol, **kw)
            assert len(got) == 5 and torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and torch.equal(got[3], base[2])
            assert all(torch.equal(a, b) for a, b in zip(got, ops.lesion_distances(pred, gr, tol, **kw)))
            short = ops.lesion_distances(pred, gr, tol, dilation=dilation, min_volume=min_volume, max_lesions=64)
            assert len(short) == 3 and all(torch.equal(a, b) for a, b in zip(short, got[:3]))
            summary_ex, table_ex, counts = got[2].cpu().numpy(), got[4].cpu().numpy(), got[1].cpu().numpy()
            assert summary_ex.shape == (1, 3, t + 1) and table_ex.shape == (1, 3, 64, t + 2)
            for k in range(3):
                tag = "%s region %d dilation %d min_volume %d T=%d" % (shape, k, dilation, min_volume, t)
                want, rows, n_fp = metrics.lesion_distances_host(pm[0, k], gm[0, k], tol, dilation, min_volume)
                n_gt, n_kept = int(counts[0, k, 0]), int(counts[0, k, 1])
                assert n_gt == len(rows) <= 24 and int(counts[0, k, 4]) == n_fp, tag
                assert table_ex[0, k, :n_gt].tobytes() == rows.tobytes(), "%s: per-lesion extras\n%s\n%s" % (tag, table_ex[0, k, :n_gt], rows)
                assert not table_ex[0, k, n_gt:].any(), tag
                assert summary_ex[0, k, :t].tobytes() == want[:t].tobytes(), "%s: LesionNSD %s != %s" % (tag, summary_ex[0, k, :t], want[:t])
                # LesionASSD: the exact value from the exact per-lesion sums; per lesion assd_roundings, then n_kept additions, the
                # false positives' product and its addition, one division -- all terms >= 0
                pairs, _ = metrics.lesion_pairs_host(pm[0, k], gm[0, k], dilation)
                exact = Fraction(n_fp) * Fraction(EMPTY)
                for mi, li in pairs:
                    if int(li.sum()) <= min_volume:
                        continue
                    if mi.any():
                        hist = metrics.surface_histogram_host(mi, li)
                        exact += Fraction(math.fsum(metrics.assd_terms_host(hist))) / int(hist.sum())
                    else:
                        exact += Fraction(EMPTY)
                den = n_kept + n_fp
                if den == 0:
                    assert summary_ex[0, k, t] == 0.0 and (summary_ex[0, k, :t] == 1.0).all(), tag
                    continue
                exact /= den
                err = abs(Fraction(float(summary_ex[0, k, t])) - exact)
                bar = (assd_roundings(bins) + n_kept + 3) * U * exact
                assert err <= bar, "%s: LesionASSD off by %.3g relative" % (tag, float(err / exact))
                worst = max(worst, float(err / exact) if exact else 0.0)
        if (dilation, min_volume) == (2, 1):
            c = counts[0, 0]
            assert c[0] > c[1] and c[3] >= 1 and c[4] >= 1, c                         # a dropped lesion, a missed one, a false positive
            assert counts[0, 1].tolist()[:5] == [0, 0, 0, 0, 0]
    print("lesion-wise %s: worst relative LesionASSD error %.3g" % (shape, worst))


# ---------------------------------------------------------------------- the metric classes and the scorer
def _mean_of_updates(per_update):
    """the accumulate launch restated: per update the batch sum in sample order over N, added to the accumulator; get() divides by the updates"""
    acc = np.zeros(per_update[0].shape[1], dtype=np.float64)
    for v in per_update:                                                              # v [N, nacc]
        s = np.zeros_like(acc)
        for row in v:
            s = s + row
        acc = acc + s / np.float64(len(v))
    return acc / np.float64(len(per_update))


@pytest.mark.gpu
def test_metric_classes_over_two_updates():
    from brats2019_amd import metrics
    rng = np.random.default_rng(45)
    shape = (6, 20, 37)
    bins = sum((s - 1) ** 2 for s in shape) + 1
    batches, masks = [], []
    for i in range(2):
        pm, gm = _lesion_masks(shape, rng)
        pm, gm = np.concatenate([pm, pm[:, ::-1]]), np.concatenate([gm, np.roll(gm[:, ::-1], 1, axis=4)])      # N = 2
        batches.append((soft(rng, pm), soft(rng, gm)))
        masks.append((pm, gm))

    def run(m):
        for b in batches:
            m.update([T(b[1]).cuda()], [T(b[0]).cuda()])
            assert isinstance(m.accumulator, torch.Tensor) and m.accumulator.is_cuda and m.accumulator.dtype == torch.float64
        assert m.samples == 2
        return np.asarray(m.get(), dtype=np.float64)

    for classes in (4, 3):
        k = classes - 1
        host = [np.array([[metrics.surface_distances_host(pm[n, j], gm[n, j], (2.0,), 50.0) for j in range(k)] for n in range(2)]) for pm, gm in masks]
        got = run(metrics.SurfaceDice(classes=classes, tolerance=2.0))
        assert got.shape == (k,) and got.tobytes() == _mean_of_updates([h[..., 0] for h in host]).tobytes()
        # ASSD: each value goes through its own roundings, then N batch additions, a division, two accumulator additions and get()'s division
        got = run(metrics.AverageSurfaceDistance(classes=classes, empty_value=50.0))
        want = _mean_of_updates([h[..., 1] for h in host])
        rtol = (assd_roundings(bins) + 2 + 4) * float(U)
        np.testing.assert_allclose(got, want, rtol=2 * rtol, atol=0)                  # both sides are within rtol of the exact mean
        host = [np.array([[metrics.lesion_distances_host(pm[n, j], gm[n, j], (2.0,), 2, 1)[0] for j in range(k)] for n in range(2)]) for pm, gm in masks]
        got = run(metrics.LesionWiseSurfaceDice(classes=classes, tolerance=2.0, dilation=2, min_volume=1))
        assert got.shape == (k,) and got.tobytes() == _mean_of_updates([h[..., 0] for h in host]).tobytes()
    m = metrics.SurfaceDice(classes=4)
    run(m)
    m.reset()
    assert m.accumulator == 0.0 and m.samples == 0.0
    with pytest.raises(IndexError):
        metrics.SurfaceDice(classes=5).update([T(batches[0][1])], [T(batches[0][0])])


@pytest.mark.gpu
def test_validate_nsd_scores_saved_cases(tmp_path, capsys):
    from brats2019_amd import metrics, validate
    rng = np.random.default_rng(46)
    shape = (12, 20, 45)
    (tmp_path / "data").mkdir()
    (tmp_path / "pred").mkdir()
    tol = [1.0, 2.5]
    want, want_les = [], []
    for i in range(2):
        lab = _labels(rng, (1,) + shape)[0]
        lab[lab > 0] *= (rng.random(shape) < 0.9)[lab > 0]
        pre = np.roll(lab, (0, 1, i), axis=(0, 1, 2))
        np.save(tmp_path / "data" / ("case%d.npy" % i), lab)
        np.save(tmp_path / "pred" / ("case%d.npy" % i), pre)
        pr, gr = regions(pre), regions(lab)
        want.append(np.array([metrics.surface_distances_host(pr[k], gr[k], tol)[:3] for k in range(3)]).T)       # [NSD, NSD, ASSD] x regions
        want_les.append(np.array([metrics.lesion_distances_host(pr[k], gr[k], tol, 1, 2)[0][:2] for k in range(3)]).T)
    args = ["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred")]
    plain, _ = validate.main(args + ["--regions"])
    res, mean = validate.main(args + ["--regions", "--nsd", "1", "2.5"])
    assert res.shape == (2, 7, 3) and mean.shape == (7, 3) and np.array_equal(res[:, :4], plain)
    assert res[:, 4:6].tobytes() == np.stack(want)[:, :2].tobytes()
    bins = sum((s - 1) ** 2 for s in shape) + 1
    np.testing.assert_allclose(res[:, 6], np.stack(want)[:, 2], rtol=2 * assd_roundings(bins) * float(U), atol=0)
    out = capsys.readouterr().out
    assert "case0 Dice WT" in out and "NSD@1 WT" in out and "NSD@2.5 WT" in out and "ASSD WT" in out and out.count("NSD@1 WT") == 3
    plain, _ = validate.main(args + ["--lesionwise", "--dilation", "1", "--min_volume", "2"])
    res, mean = validate.main(args + ["--lesionwise", "--dilation", "1", "--min_volume", "2", "--nsd", "1", "2.5"])
    assert res.shape == (2, 4, 3) and np.array_equal(res[:, :2], plain) and res[:, 2:].tobytes() == np.stack(want_les).tobytes()
    out = capsys.readouterr().out
    assert "LesionNSD@1 WT" in out and "LesionNSD@2.5 WT" in out
