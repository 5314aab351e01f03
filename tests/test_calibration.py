"""Calibration scoring and the threshold search on the device (csrc/calibration.hip) against the numpy restatement
(metrics.calibration_host, pinned to a direct sweep by tests/test_calibration_host.py): the integer tables byte for byte, the float64
curves and summary within bars counted from the kernels' roundings, the ties to metrics.Dice and ops.ens_finalize, the `thresholds=`
keyword of the inference pipeline and the metric classes."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_calibration_host import FAMILIES, TRIVIAL_OK, distinct_bins, make_case, make_label_case

pytestmark = pytest.mark.gpu

T = torch.from_numpy
U = 2.0 ** -53                                        # one float64 rounding, relative
SHAPES = ((2, 3, 17 * 19 * 37), (1, 3, 5), (1, 1, 4099), (1, 3, 9 * 64 * 64))
NBS = (16, 256, 1024)
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)

_HOST = {}


def host(family, shape, nb, seed=0):
    """(pred, target, restatement) of one case, computed once and shared; nobody writes them"""
    from brats2019_amd import metrics
    key = (family, shape, nb, seed)
    if key not in _HOST:
        pred, target = make_label_case(shape, seed) if family == "labels" else make_case(family, shape, seed, nb)
        _HOST[key] = (pred, target, metrics.calibration_host(pred, target, nb, 16))
    return _HOST[key]


def off_boundary(a, nbytes):
    """a device copy of `a` that starts `nbytes` bytes behind a 16-byte boundary"""
    k = nbytes // a.itemsize
    buf = torch.zeros(a.size + 16, dtype=T(a[:0].reshape(-1)).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + a.size].view(a.shape)
    view.copy_(T(a))
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    return view


def check_tables(pred, target, h, nb, what, dev=None):
    from brats2019_amd import ops
    p, g = dev if dev is not None else (T(pred).cuda(), T(target).cuda())
    got = ops.calib_histogram(p, g, nb)
    again = ops.calib_histogram(p, g, nb)
    for name, a, b in zip(("hist", "conf", "sq", "invalid"), got, again):
        assert a.dtype == torch.int64 and a.is_cuda
        assert torch.equal(a, b), "%s: two calls differ in %s" % (what, name)
        want = T(np.ascontiguousarray(h[name]))
        assert a.shape == want.shape and torch.equal(a.cpu(), want), "%s: %s differs in %d entries" % (what, name, int((a.cpu() != want).sum()))
    return got


# every family and every NB at the first shape; every other shape with every family at one NB each, in rotation
CASES = [(f, SHAPES[0], nb) for f in FAMILIES + ("labels",) for nb in NBS]
CASES += [(f, s, NBS[(i + j) % 3]) for i, s in enumerate(SHAPES[1:]) for j, f in enumerate(FAMILIES + ("labels",))]


@pytest.mark.parametrize("family,shape,nb", CASES)
def test_tables_equal_the_restatement(family, shape, nb):
    if family == "labels":
        shape = (shape[0], 3, shape[2])
    pred, target, h = host(family, shape, nb)
    if shape == SHAPES[0]:
        assert distinct_bins(h["hist"]) >= 3 or family in TRIVIAL_OK
    check_tables(pred, target, h, nb, "%s %s NB %d" % (family, shape, nb))


@pytest.mark.parametrize("family", ["uniform", "saturated", "invalid", "labels"])
def test_views_off_the_16_byte_boundary(family):
    shape, nb = (1, 3, 4099), 256
    pred, target, h = host(family, shape, nb, seed=2)
    shifts = ((8, 8), (8, 0), (4, 12)) if family != "labels" else ((8, 2), (12, 3), (8, 1), (0, 3))
    for sp, st in shifts:                              # alike offsets take the 16-byte walk with a head, unlike ones go one by one
        dev = (off_boundary(pred, sp), off_boundary(target, st))
        check_tables(pred, target, h, nb, "%s offsets %d / %d" % (family, sp, st), dev)


@pytest.mark.parametrize("nb", NBS)
def test_one_bin_takes_every_voxel(nb):
    """70001 voxels per channel in bin 0 with y = 0: a counter narrower than the chunk or a lost update under contention shows here"""
    from brats2019_amd import ops
    shape = (1, 3, 70001)
    got = ops.calib_histogram(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"), nb)
    want = torch.zeros((1, 3, nb + 1, 2), dtype=torch.int64)
    want[:, :, 0, 0] = 70001
    assert torch.equal(got[0].cpu(), want) and not got[1].any() and not got[2].any() and not got[3].any()
    # the same at the other end: bin NB with y = 1 carries the largest sums
    got = ops.calib_histogram(torch.ones(shape, device="cuda"), torch.ones(shape, device="cuda"), nb)
    assert (got[0][:, :, nb, 1] == 70001).all() and int(got[0].sum()) == 3 * 70001
    assert (got[1][:, :, nb, 1] == 70001 * 2 ** 24).all() and int(got[1].sum()) == 3 * 70001 * 2 ** 24
    assert (got[2][:, :, 1, 1] == 70001 * 2 ** 16).all() and int(got[2].sum()) == 3 * 70001 * 2 ** 16          # r * r = 2^48: the high words


@pytest.mark.parametrize("family,nb", [("uniform", 256), ("saturated", 16), ("invalid", 1024), ("empty", 256), ("full", 1024), ("labels", 256), ("edges", 16)])
def test_accumulate_and_summary(family, nb):
    from brats2019_amd import metrics, ops
    shape = SHAPES[0]
    pred, target, h = host(family, shape, nb)
    n, c = shape[:2]
    tables = check_tables(pred, target, h, nb, family)[:3]
    pool = ops.calib_pool(c, nb, "cuda")
    curves = ops.calib_accumulate(*tables, pool, want_curves=True)
    assert ops.calib_accumulate(*tables, pool) is None                                  # a second call: the pooled tables and the curve sums double
    assert torch.equal(pool[0].cpu(), T(2 * h["pool_hist"])) and torch.equal(pool[1].cpu(), T(2 * h["pool_conf"]))
    s2 = [[2 * v for v in row] for row in h["pool_s2"]]
    want_sq = np.array([[[v & 0xffffffff, v >> 32] for v in row] for row in s2], dtype=np.int64)
    assert torch.equal(pool[2].cpu(), T(want_sq)), "pool_sq is carried: low word < 2^32"
    # Curves: exact integers, conversions exact below 2^53, ONE division: 1 rounding, relative.  The restatement's division is correctly rounded too.
    got = curves.cpu().numpy()
    err = np.abs(got - h["curves"])
    print(family, nb, "curves: max error / bar", float((err / (U * np.abs(h["curves"]) + 1e-300)).max()))
    assert (err <= 1 * U * np.abs(h["curves"])).all()
    # curve_acc = 0 + (v_0 + v_1), then + (v_0 + v_1): N - 1 + 2 additions on top of the N values' roundings: (2N + 1) roundings relative to the sum
    acc = pool[3].cpu().numpy()
    assert (np.abs(acc - 2 * h["curve_sum"]) <= (2 * n + 1) * U * 2 * h["curve_sum"]).all()
    # Summary of the doubled pool = summary of the pool: every ratio is unchanged.
    for bins in (16, nb):
        out, table = (t.cpu().numpy() for t in ops.calib_summary(*pool[:3], bins))
        rows = [metrics.calibration_summary_host(2 * h["pool_hist"][j], 2 * h["pool_conf"][j], s2[j], bins) for j in range(c)]
        for j in range(c):
            want, wtab = rows[j]
            assert np.array_equal(table[j, :, 0], wtab[:, 0]) and out[j, 5] == want[5] and out[j, 6] == want[6], "counts are exact"
            # conf_m, freq_m: the sum of r is below 2^53 here, so its conversion is exact: one division each
            assert (np.abs(table[j, :, 1:] - wtab[:, 1:]) <= U * wtab[:, 1:]).all()
            w = wtab[:, 0] / max(want[5], 1.0)
            # ECE: per term conf_m, freq_m, their difference, the weight and the product round (5, relative to w_m * (freq_m + conf_m)); M - 1 additions
            bar_ece = (bins + 4) * U * float((w * (wtab[:, 1] + wtab[:, 2])).sum())
            # MCE: conf_m, freq_m and their difference round, relative to freq_m + conf_m <= 2
            bar_mce = 3 * U * 2.0
            # Brier: the numerator is an exact integer; its low word's conversion, the sum of the two words and the division round (3); the restatement rounds once
            bar_brier = 4 * U * want[2]
            print(family, nb, bins, j, "ECE", out[j, 0], want[0], bar_ece, "MCE", out[j, 1], want[1], "Brier", out[j, 2], want[2], bar_brier)
            assert abs(out[j, 0] - want[0]) <= bar_ece and abs(out[j, 1] - want[1]) <= bar_mce and abs(out[j, 2] - want[2]) <= bar_brier
            assert abs(out[j, 3] - want[3]) <= U * want[3] and abs(out[j, 4] - want[4]) <= U * want[4]
    if family == "uniform":
        assert (h["summary"][:, 0] < 0.05).all(), "a target drawn from the probabilities is calibrated"


def test_an_empty_channel_gives_zeros():
    from brats2019_amd import ops
    pred = torch.full((1, 2, 100), float("nan"), device="cuda")
    pred[0, 1] = 0.25
    tables = ops.calib_histogram(pred, torch.ones_like(pred), 16)
    assert tables[3].tolist() == [[100, 0]]
    pool = ops.calib_pool(2, 16, "cuda")
    curves = ops.calib_accumulate(*tables[:3], pool, want_curves=True)
    assert (curves[0, 0] == 1.0).all()                                                  # every denominator is empty
    out, table = ops.calib_summary(*pool[:3], 4)
    assert not out[0].any() and not table[0].any()
    assert out[1].tolist() == [0.75, 0.75, 0.5625, 0.25, 1.0, 100.0, 1.0]


def test_ties_to_dice_and_the_merge_family():
    from brats2019_amd import metrics, ops
    nb, shape = 256, (1, 3, 9 * 64 * 64)
    pred, target, h = host("edges", shape, nb)
    p, g = T(pred).cuda(), T(target).cuda()
    # the curve at NB / 2 is metrics.Dice: the same counts, its ratio formed in float32
    dice = metrics.Dice(classes=4)
    dice.update([g.view(1, 3, 9, 64, 64)], [p.view(1, 3, 9, 64, 64)])
    assert dice.get().tolist() == [float(np.float32(v)) for v in h["curves"][0, :, 0, nb // 2]]
    # at 0.5 the masks and counts are the merge family's, NaN and the value 0.5 itself included
    x = p[0].clone()
    x[0, :7] = T(np.array([np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.inf, -np.inf, -0.0, 1.0], np.float32)).cuda()
    mask, counts, mean = ops.ens_finalize(x, 1, want_mean=True)
    got = ops.threshold_regions(mean, 0.5)
    assert torch.equal(got[0], mask) and torch.equal(got[1], counts) and got[0].dtype == torch.uint8 and got[1].dtype == torch.int64
    again = ops.threshold_regions(mean, (0.5, 0.5, 0.5))
    assert torch.equal(again[0], mask) and torch.equal(again[1], counts)
    # the chosen threshold, then the existing Dice counts, reproduce the curve's value exactly; an odd size takes the bytewise path
    for pv, gv, hv in ((pred, target, h), host("uniform", SHAPES[0], nb)):
        bins = [metrics.choose_threshold(hv["curves"][0, c, 0]) for c in range(3)]
        m, cnt = ops.threshold_regions(T(pv[0]).cuda(), [b / nb for b in bins])
        dc = ops.dice_counts(m[None].float(), T(gv[:1]).cuda()).cpu().numpy()
        for c, b in enumerate(bins):
            assert np.float64(2 * dc[0, c, 0]) / np.float64(dc[0, c, 1]) == hv["curves"][0, c, 0, b], (c, b)
            assert int(cnt[c]) == int(hv["hist"][0, c, b + 1:].sum())
    with pytest.raises(ValueError):
        ops.threshold_regions(mean, (0.5, float("nan"), 0.5))
    with pytest.raises(ValueError):
        ops.threshold_regions(mean, (0.5, 0.5))
    with pytest.raises(ValueError):
        ops.calib_histogram(p, g, 100)
    with pytest.raises(ValueError):
        ops.calib_histogram(p, g[:, :2], 256)
    with pytest.raises(ValueError):
        ops.calib_summary(*ops.calib_pool(3, 256, "cuda")[:3], 24)


def _net(seed):
    from brats2019_amd import model as M
    net = M.UNet(**SMALL)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **SMALL).items()})
    return net.cuda()


def _case():
    rng = np.random.default_rng(45)
    img = np.zeros((4, 32, 32, 32), np.float32)
    img[:, 2:29, 3:31, 1:27] = rng.random((4, 27, 28, 26)).astype(np.float32) * 3 + 0.05
    return img


def test_the_thresholds_keyword():
    from brats2019_amd import inference as I
    net, img = _net(17), _case()
    plain = I.predict_case(net, img)
    half = I.predict_case(net, img, thresholds=(0.5, 0.5, 0.5))
    assert half[0].tobytes() == plain[0].tobytes() and half[1] == plain[1]
    assert I.predict_case(net, img, thresholds=0.5)[0].tobytes() == plain[0].tobytes()
    t = (0.25, 0.5, 0.75)
    labels, counts = I.predict_case(net, img, thresholds=t)
    ens = I.predict_case_ensemble([net], img, want_probs=True, uncertainty="std", thresholds=t)
    base = I.predict_case_ensemble([net], img, want_probs=True, uncertainty="std")
    assert ens[0].tobytes() == labels.tobytes() and ens[1] == counts
    assert np.array_equal(ens[2], base[2]) and np.array_equal(ens[3], base[3]), "soft labels and uncertainty maps are the merge's"
    # numpy: re-threshold the returned mean, then the host's label composition, rejection and paste
    mean = ens[2]
    mask = mean > np.asarray(t, np.float32).reshape(3, 1, 1, 1)
    want_counts = tuple(int(v) for v in mask.reshape(3, -1).sum(axis=1))
    print("counts at 0.5", plain[1], "at", t, want_counts)
    assert counts == want_counts and counts != plain[1]
    _, lo, size, _, _ = I.prepare_case_device(T(img).cuda())
    box = tuple(slice(int(l), int(l) + int(s)) for l, s in zip(lo, size))
    want = np.zeros(img.shape[1:], np.uint8)
    want[box] = I.postprocess_labels(I.compose_masks_host(mask[(slice(None),) + box], want_counts), 0.1)
    assert labels.dtype == np.uint8 and labels.tobytes() == want.tobytes()
    # before the post-processing: its region pass sees the re-thresholded masks
    post = I.PostProcess(min_volume=(8, 4, 2), nest=True, reject_ratio=None)
    got = I.predict_case(net, img, postprocess=post, thresholds=t)
    m, c = I.postprocess_regions_host(mask[(slice(None),) + box].astype(np.uint8), **post.regions())
    want[box] = I.compose_masks_host(m, c)
    assert got[0].tobytes() == want.tobytes() and got[1] == tuple(c.tolist())
    with pytest.raises(ValueError):
        I.predict_case(net, img, thresholds=(0.5, 0.5))


def test_metric_classes_pool_over_updates():
    from brats2019_amd import metrics
    nb = 256
    pa, ga, _ = host("uniform", SHAPES[0], nb)
    pb, gb, _ = host("saturated", SHAPES[0], nb)
    both = metrics.calibration_host(np.concatenate([pa, pb]), np.concatenate([ga, gb]), nb, 16)
    ece, brier = metrics.ExpectedCalibrationError(bins=16, nb=nb), metrics.BrierScore(nb=nb)
    dice, at = metrics.Dice(classes=4), metrics.DiceAtThreshold(0.5)
    shape5 = (2, 3, 17, 19, 37)
    for p, g in ((pa, ga), (pb, gb)):
        ground, predict = [T(g).cuda().view(shape5)], [T(p).cuda().view(shape5)]
        for m in (ece, brier, dice, at):
            m.update(ground, predict)                                                   # train.py:304: (ground, predict)
    want = both["summary"]
    w = both["table"][:, :, 0] / want[:, 5:6]
    bar = (16 + 4) * U * (w * (both["table"][:, :, 1] + both["table"][:, :, 2])).sum(axis=1)       # as in test_accumulate_and_summary
    print("ECE", ece.get(), want[:, 0], "Brier", brier.get(), want[:, 2])
    assert ece.get().shape == (3,) and (np.abs(ece.get() - want[:, 0]) <= bar).all()
    assert (np.abs(ece.max_error() - want[:, 1]) <= 6 * U).all() and np.array_equal(ece.reliability()[:, :, 0], both["table"][:, :, 0])
    assert (np.abs(brier.get() - want[:, 2]) <= 4 * U * want[:, 2]).all()
    assert np.array_equal(at.get(), dice.get())
    low = metrics.DiceAtThreshold((0.25, 0.5, 0.75))
    low.update([T(ga).cuda().view(shape5)], [T(pa).cuda().view(shape5)])
    ref = metrics.Dice(classes=4)
    t = np.asarray((0.25, 0.5, 0.75), np.float32).reshape(1, 3, 1)
    ref.update([T(ga).cuda().view(shape5)], [T((pa > t).astype(np.float32)).cuda().view(shape5)])
    assert np.array_equal(low.get(), ref.get())
    ece.reset()
    with pytest.raises(RuntimeError):
        ece.get()
