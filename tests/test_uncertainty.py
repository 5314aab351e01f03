"""Uncertainty maps and the BraTS uncertainty score on the device (csrc/uncertainty.hip) against the numpy oracles of
tests/test_uncertainty_host.py: the sums, mean, mask and counts bit for bit against the ru_ens_* passes, the std map exactly, the entropy
map up to the last place of log2, the histogram exactly, the score to rtol 1e-12; `predict_case_ensemble(..., uncertainty=...)`, the
command lines and graph capture."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_uncertainty_host import (DEGENERATE, FLIPS, blob_labels, boundary_maps, degenerate_case, negative_variance_members, oracle_entropy,
                                   oracle_entropy_real, oracle_histogram, oracle_mean, oracle_score, oracle_second_moment, oracle_std, random_members)

T = torch.from_numpy
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)
# (volume [3, D, H, W], box lo, box size): odd extents and offsets, W and the box width not multiples of 4, a box equal to the volume
BOXES = [((3, 8, 12, 16), (1, 2, 3), (6, 9, 11)), ((3, 8, 12, 16), (0, 0, 0), (8, 12, 16)), ((3, 5, 6, 7), (1, 1, 2), (3, 4, 5)),
         ((3, 5, 6, 7), (0, 0, 0), (5, 6, 7)), ((3, 6, 7, 18), (2, 0, 5), (3, 7, 9)), ((3, 4, 3, 3), (0, 1, 0), (4, 2, 3))]
BOX_IDS = ["box", "whole", "ragged-box", "ragged-whole", "odd-offset", "narrow"]


def _padded_outputs(rng, m, k, shape, lo, size, members=None):
    """-> (members[m][k] on the box, flipped padded predictions [m] of [k, 3, D, H, W] as a network would emit them)"""
    box = (slice(None),) + tuple(slice(l, l + s) for l, s in zip(lo, size))
    if members is None:
        members = random_members(rng, m, k, (3,) + tuple(size))
    outs = []
    for copies in members:
        flipped = []
        for o, ax in zip(copies, FLIPS):
            full = rng.random(shape).astype(np.float32)                  # the padding holds other values: it must not be read
            full[box] = o
            flipped.append(np.ascontiguousarray(np.flip(full, axis=ax)) if ax else full)
        outs.append(np.stack(flipped))
    return members, outs


def _entropy_check(got, mean, what):
    """equal to the oracle except where the oracle's 100*H + 0.5 lies within 1e-9 of an integer; there one step is allowed, on a share of
    the voxels of at most 1e-5, and the inputs keep the oracle inside that cap"""
    real = oracle_entropy_real(mean)
    band = np.abs(real - np.round(real)) < 1e-9
    want = oracle_entropy(mean)
    assert band.mean() <= 1e-5, what
    np.testing.assert_array_equal(got[~band], want[~band], err_msg=what)
    assert (np.abs(got[band].astype(int) - want[band].astype(int)) <= 1).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("shape,lo,size", BOXES, ids=BOX_IDS)
def test_passes_match_the_ensemble_passes_and_the_oracles(m, shape, lo, size):
    """All four flips.  acc / mean / mask / counts of the ru_unc_* passes equal the ru_ens_* passes' bit for bit, acc2 equals the float32
    second moment, the std map equals numpy exactly, on both routes (fused last member; stored sums + ru_unc_finalize)."""
    from brats2019_amd import inference as I, ops
    rng = np.random.default_rng(100 * m + shape[3])
    members, outs = _padded_outputs(rng, m, 4, shape, lo, size)
    probs = [T(o).cuda() for o in outs]
    acc_e, acc, acc2 = None, None, None
    for i, p in enumerate(probs):
        acc_e = ops.ens_accumulate(p, FLIPS, acc_e, lo, size)
        if i + 1 == m:
            fused = {meas: ops.unc_accumulate_finalize(p, FLIPS, acc, acc2, m, meas, lo, size, want_mean=True) for meas in ("std", "entropy")}
            fused["entropy, no acc2"] = ops.unc_accumulate_finalize(p, FLIPS, acc, None, m, "entropy", lo, size, want_mean=True)
        acc, acc2 = ops.unc_accumulate(p, FLIPS, acc, acc2, lo, size)
    np.testing.assert_array_equal(acc.cpu().numpy(), acc_e.cpu().numpy())
    np.testing.assert_array_equal(acc2.cpu().numpy(), oracle_second_moment(members))
    mask_e, counts_e, mean_e = ops.ens_finalize(acc_e, m, want_mean=True)
    mask_f, counts_f, mean_f = I.ensemble_merge(probs, lo, size, want_mean=True)
    assert torch.equal(mask_e, mask_f) and torch.equal(counts_e, counts_f) and torch.equal(mean_e, mean_f)
    mean_ref = oracle_mean(members)
    np.testing.assert_array_equal(mean_e.cpu().numpy(), mean_ref)
    routes = dict(fused)
    routes["stored std"] = ops.unc_finalize(acc, acc2, m, 4, "std", want_mean=True)
    routes["stored entropy"] = ops.unc_finalize(acc, None, m, 4, "entropy", want_mean=True)
    routes["ensemble_merge std"] = I.ensemble_merge(probs, lo, size, want_mean=True, uncertainty="std")
    for how, (mask, counts, mean, unc) in routes.items():
        np.testing.assert_array_equal(mean.cpu().numpy(), mean_e.cpu().numpy(), err_msg=how)
        np.testing.assert_array_equal(mask.cpu().numpy(), mask_e.cpu().numpy(), err_msg=how)
        np.testing.assert_array_equal(counts.cpu().numpy(), counts_e.cpu().numpy(), err_msg=how)
        assert unc.dtype == torch.uint8 and tuple(unc.shape) == (3,) + tuple(size), how
        if "std" in how:
            np.testing.assert_array_equal(unc.cpu().numpy(), oracle_std(members), err_msg=how)
        else:
            _entropy_check(unc.cpu().numpy(), mean_ref, how)
    assert oracle_std(members).max() > 20                              # the maps are not trivially zero
    no_mean = ops.unc_accumulate_finalize(probs[-1], FLIPS, *((None, None) if m == 1 else _sums(ops, probs[:-1], lo, size)), m, "std", lo, size)
    assert no_mean[2] is None and torch.equal(no_mean[3], routes["std"][3])


def _sums(ops, probs, lo, size):
    acc, acc2 = None, None
    for p in probs:
        acc, acc2 = ops.unc_accumulate(p, FLIPS, acc, acc2, lo, size)
    return acc, acc2


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3, 5])
def test_saved_predictions_are_members_with_one_copy(m):
    """K = 1: already merged [3, D, H, W] predictions, the box equal to the volume, as `ensemble --uncertainty_output` feeds them"""
    from brats2019_amd import ops
    rng = np.random.default_rng(40 + m)
    members = random_members(rng, m, 1, (3, 7, 9, 10))
    acc_e, acc, acc2 = None, None, None
    for copies in members:
        p = T(copies[0]).cuda()
        acc_e = ops.ens_accumulate(p, acc=acc_e)
        acc, acc2 = ops.unc_accumulate(p, acc=acc, acc2=acc2)
    assert torch.equal(acc, acc_e)
    mask_e, counts_e, mean_e = ops.ens_finalize(acc_e, m, want_mean=True)
    mask, counts, mean, unc = ops.unc_finalize(acc, acc2, m, 1, "std", want_mean=True)
    assert torch.equal(mask, mask_e) and torch.equal(counts, counts_e) and torch.equal(mean, mean_e)
    np.testing.assert_array_equal(unc.cpu().numpy(), oracle_std(members))
    _entropy_check(ops.unc_finalize(acc, None, m, 1, "entropy")[3].cpu().numpy(), oracle_mean(members), "K = 1")


@pytest.mark.gpu
def test_std_map_at_exact_and_awkward_values():
    from brats2019_amd import ops
    rng = np.random.default_rng(50)
    size = (4, 32, 32)

    def device(members):
        acc, acc2 = None, None
        for copies in members:
            acc, acc2 = ops.unc_accumulate(T(np.stack(copies)).cuda(), ((),) * len(copies), acc, acc2)
        return ops.unc_finalize(acc, acc2, len(members), len(members[0]), "std")[3].cpu().numpy()

    v = rng.random((3,) + size).astype(np.float32)
    assert not device([[v] * 4] * 3).any()                             # all members equal: no spread
    zero, one = np.zeros((3,) + size, np.float32), np.ones((3,) + size, np.float32)
    assert (device([[zero, one, zero, one], [one, zero, one, zero]]) == 100).all()      # an even 0 / 1 split: sigma = 0.5
    members, negative = negative_variance_members(rng, 3, 4, (3,) + size)
    assert negative.sum() > 100                                        # e2 - mu*mu < 0 there: clamped, not NaN
    got = device(members)
    np.testing.assert_array_equal(got, oracle_std(members))
    assert not got[negative].any()


@pytest.mark.gpu
def test_entropy_map_on_the_issue_inputs_and_at_exact_values():
    """3 x 4 members of 3 x 40 x 48 x 56 voxels, uniform float32 clipped to [0, 1]; p in {0, 1} -> 0 and p = 0.5 -> 100 exactly"""
    from brats2019_amd import ops
    rng = np.random.default_rng(60)
    members = random_members(rng, 3, 4, (3, 40, 48, 56))
    acc, acc2 = None, None
    for copies in members:
        acc, acc2 = ops.unc_accumulate(T(np.stack(copies)).cuda(), ((),) * 4, acc, acc2)
    mean = oracle_mean(members)
    real = oracle_entropy_real(mean)
    print("entropy: nearest 100*H + 0.5 to an integer %.2e" % float(np.abs(real - np.round(real)).min()))
    _entropy_check(ops.unc_finalize(acc, acc2, 3, 4, "entropy")[3].cpu().numpy(), mean, "issue inputs")
    exact = np.zeros((3, 2, 3, 8), np.float32)
    exact[1], exact[2] = 1.0, 0.5
    got = ops.unc_accumulate_finalize(T(exact).cuda(), ((),), None, None, 1, "entropy")[3].cpu().numpy()
    assert not got[0].any() and not got[1].any() and (got[2] == 100).all()


def _case():
    rng = np.random.default_rng(17)
    img = np.zeros((4, 40, 44, 36), np.float32)
    img[:, 4:33, 6:39, 3:30] = rng.random((4, 29, 33, 27)).astype(np.float32) * 3 + 0.05
    return img


def _net(seed):
    from brats2019_amd import model as M
    net = M.UNet(**SMALL)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **SMALL).items()})
    return net.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("measure", ["std", "entropy"])
def test_predict_case_ensemble_with_uncertainty(measure):
    """Three tiny networks.  Labels, counts and soft labels are the call's without the keyword; the map is the oracle's on the members
    predicted by separate forwards, zero outside the crop box; `predict_case(..., uncertainty=...)` is the ensemble of one."""
    from brats2019_amd import inference as I
    img = _case()
    nets = [_net(s) for s in (17, 18, 19)]
    plain = I.predict_case_ensemble(nets, img, want_probs=True)
    got = I.predict_case_ensemble(nets, img, want_probs=True, uncertainty=measure)
    assert len(got) == 4 and np.array_equal(got[0], plain[0]) and got[1] == plain[1] and np.array_equal(got[2], plain[2])
    short = I.predict_case_ensemble(nets, img, uncertainty=measure)
    assert len(short) == 3 and np.array_equal(short[0], plain[0]) and np.array_equal(short[2], got[3])
    batch, lo, size, left, _padded = I.prepare_case_device(T(img).cuda())
    outs = []
    for net in nets:
        net.eval()
        with torch.no_grad():
            outs.append(net([batch])[0].cpu().numpy())
    members = I._members_host(outs, left, size)
    box = (slice(None),) + tuple(slice(int(l), int(l) + int(s)) for l, s in zip(lo, size))
    maps = got[3]
    assert maps.dtype == np.uint8 and maps.shape == (3,) + img.shape[1:]
    if measure == "std":
        np.testing.assert_array_equal(maps[box], oracle_std(members))
    else:
        _entropy_check(maps[box], oracle_mean(members), "end to end")
    outside = np.ones(maps.shape, bool)
    outside[box] = False
    assert not maps[outside].any() and maps[box].any()
    one = I.predict_case(nets[0], img, uncertainty=measure)
    want = I.predict_case_ensemble([nets[0]], img, uncertainty=measure)
    base = I.predict_case(nets[0], img)
    assert len(one) == 3 and np.array_equal(one[0], base[0]) and one[1] == base[1] and np.array_equal(one[2], want[2])
    dev = I.predict_case_device(nets[0], T(img).cuda(), uncertainty=measure)
    assert np.array_equal(dev[2].cpu().numpy(), one[2])


@pytest.mark.gpu
def test_paste_u8c():
    from brats2019_amd import ops
    for full_shape, lo in [((5, 6, 7), (1, 2, 3)), ((5, 6, 8), (1, 2, 3)), ((2, 3, 4), (0, 0, 0))]:
        small = T((np.arange(3 * 2 * 3 * 4) % 101).astype(np.uint8).reshape(3, 2, 3, 4) + 1).cuda()
        want = np.zeros((3,) + full_shape, np.uint8)
        want[:, lo[0]:lo[0] + 2, lo[1]:lo[1] + 3, lo[2]:lo[2] + 4] = small.cpu().numpy()
        np.testing.assert_array_equal(ops.paste_u8c(small, full_shape, lo).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="box"):
        ops.paste_u8c(small, (5, 6, 7), (4, 2, 3))


def _histogram(pred, target, maps):
    from brats2019_amd import ops
    hist, invalid = ops.unc_histogram(T(pred).cuda(), T(target).cuda(), T(maps).cuda())
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (3, 101, 4)
    return hist.cpu().numpy(), int(invalid.cpu()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 11, 13), (17, 23, 29), (16, 24, 32), (240, 240, 155)], ids=lambda s: "x".join(map(str, s)))
def test_histogram_is_exact(shape):
    rng = np.random.default_rng(shape[0])
    target = blob_labels(rng, shape)
    pred = np.roll(target, 2, axis=1)
    maps = boundary_maps(rng, pred, every_level=True)
    want = oracle_histogram(pred, target, maps)
    assert (want.sum(axis=2) > 0).all()                                # every level 0..100 occurs in every region
    got, invalid = _histogram(pred, target, maps)
    np.testing.assert_array_equal(got, want)
    assert invalid == 0 and got.sum() == 3 * pred.size
    dense = rng.integers(0, 101, size=maps.shape, dtype=np.uint8)      # no voxel takes the register fast path's shortcut for long
    got, invalid = _histogram(pred, target, dense)
    np.testing.assert_array_equal(got, oracle_histogram(pred, target, dense))
    # all background, zero maps: one cell per region
    zero = np.zeros(shape, np.uint8)
    got, invalid = _histogram(zero, zero, np.zeros((3,) + shape, np.uint8))
    want = np.zeros((3, 101, 4), np.int64)
    want[:, 0, 3] = zero.size
    np.testing.assert_array_equal(got, want)
    # planted bad values are counted and stay out of every bin
    bad_pred, bad_target, bad_maps = pred.copy(), target.copy(), maps.copy()
    flat = rng.choice(pred.size, 9, replace=False)
    bad_pred.reshape(-1)[flat[:3]] = 5
    bad_target.reshape(-1)[flat[3:6]] = 255
    bad_maps.reshape(3, -1)[1, flat[6:]] = 101
    got, invalid = _histogram(bad_pred, bad_target, bad_maps)
    assert invalid == 9 and got.sum() == 3 * (pred.size - 9)
    keep = np.ones(pred.size, bool)
    keep[flat] = False
    np.testing.assert_array_equal(got, oracle_histogram(pred.reshape(-1)[keep], target.reshape(-1)[keep], maps.reshape(3, -1)[:, keep]))


@pytest.mark.gpu
@pytest.mark.parametrize("thresholds", [(25, 50, 75, 100), (0, 100), (10, 20, 30, 40, 50, 60, 70, 80, 90, 100), (5, 37, 99), (50,)], ids=str)
def test_score_uncertainty_equals_brute_force(thresholds):
    from brats2019_amd import validate
    rng = np.random.default_rng(70)
    cases = []
    for i, shape in enumerate([(17, 23, 29), (16, 24, 32), (9, 11, 13)]):
        target = blob_labels(rng, shape)
        pred = np.roll(target, 1 + i, axis=2)
        cases.append(("case%d" % i, target, pred, boundary_maps(rng, pred)))
    names, results, mean = validate.score_uncertainty(cases, thresholds)
    want = np.stack([oracle_score(p, g, u, thresholds) for _, g, p, u in cases])
    assert names == ["case0", "case1", "case2"] and results.shape == (3, 3, 4)
    np.testing.assert_allclose(results, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(mean, want.mean(axis=0), rtol=1e-12, atol=0)
    assert np.isfinite(want).all() and (want[:2, 0, 1] < 1).all()      # the rolled prediction does not match: a Dice curve below 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DEGENERATE)
def test_score_uncertainty_degenerate_cases(kind):
    from brats2019_amd import validate
    pred, target, maps, thresholds = degenerate_case(kind, np.random.default_rng(4))
    _, results, mean = validate.score_uncertainty([("c", target, pred, maps)], thresholds)
    np.testing.assert_allclose(results[0], oracle_score(pred, target, maps, thresholds), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(mean, results[0])


@pytest.mark.gpu
def test_score_uncertainty_names_the_case_with_bad_values():
    from brats2019_amd import validate
    rng = np.random.default_rng(71)
    target = blob_labels(rng, (9, 11, 13))
    maps = boundary_maps(rng, target)
    bad = maps.copy()
    bad[2, 4, 5, 6] = 101
    with pytest.raises(ValueError, match="second"):
        validate.score_uncertainty([("first", target, target, maps), ("second", target, target, bad)])


@pytest.mark.gpu
def test_command_lines_write_and_score_the_maps(tmp_path, capsys):
    """`ensemble --uncertainty_output` on saved region probabilities, then `validate --uncertainty_path` on what it wrote"""
    import os
    from brats2019_amd import ensemble, inference as I, validate
    rng = np.random.default_rng(80)
    shape = (20, 24, 28)
    target = blob_labels(rng, shape)
    regions = np.stack([np.isin(target, labels) for labels in ((1, 2, 3, 4), (1, 3, 4), (3, 4))]).astype(np.float32)
    preds = [np.clip(0.15 + 0.7 * regions + rng.normal(0, 0.25, regions.shape), 0, 1).astype(np.float32) for _ in range(3)]
    for i, p in enumerate(preds):
        os.makedirs(tmp_path / ("run%d" % i))
        np.save(tmp_path / ("run%d" % i) / "caseA.npy", p)
    os.makedirs(tmp_path / "gt")
    np.save(tmp_path / "gt" / "caseA.npy", target)
    runs = [str(tmp_path / ("run%d" % i)) for i in range(3)]
    ensemble.main(["--predictions"] + runs + ["--output", str(tmp_path / "plain"), "--rule", "regions"])
    for measure in ("std", "entropy"):
        out, unc = tmp_path / ("out_" + measure), tmp_path / ("unc_" + measure)
        ensemble.main(["--predictions"] + runs + ["--output", str(out), "--rule", "regions", "--uncertainty", measure, "--uncertainty_output", str(unc)])
        labels = np.load(out / "caseA.npy")
        assert np.array_equal(labels, np.load(tmp_path / "plain" / "caseA.npy"))
        maps = np.stack([np.load(unc / ("caseA_unc_%s.npy" % stem)) for stem in I.UNCERTAINTY_STEMS])
        assert maps.dtype == np.uint8 and maps.shape == (3,) + shape and maps.any()
        if measure == "std":
            np.testing.assert_array_equal(maps, oracle_std([[p] for p in preds]))
        else:
            _entropy_check(maps, oracle_mean([[p] for p in preds]), "ensemble CLI")
        capsys.readouterr()
        results, mean = validate.main(["--data_path", str(tmp_path / "gt"), "--predictions_path", str(out), "--uncertainty_path", str(unc),
                                       "--thresholds", "20", "60", "100"])
        printed = capsys.readouterr().out
        want = oracle_score(labels, target, maps, (20, 60, 100))
        np.testing.assert_allclose(results[0], want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(mean, want, rtol=1e-12, atol=0)
        rows = [line for line in printed.splitlines() if line.startswith(("caseA ", "mean "))]
        assert len(rows) == 2 and all("WT score %.4f" % want[0, 0] in r and "ET score %.4f" % want[2, 0] in r and "AUC_FTN" in r for r in rows)


@pytest.mark.gpu
def test_test_entry_point_writes_the_maps(tmp_path):
    """`test --uncertainty std --uncertainty_output DIR`: the three files equal the API's maps; the labels are those of the plain call"""
    import os, shutil, sys
    from brats2019_amd import test as entry, inference as I, train as TR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "tests", "golden", "ckpt", "tiny"), tmp_path / "tiny")
    rng = np.random.default_rng(5)
    img = np.zeros((4, 30, 28, 26), np.float32)
    img[:, 2:27, 3:25, 1:24] = rng.random((4, 25, 22, 23)).astype(np.float32) * 2 + 0.1
    np.save(tmp_path / "case.npy", img)
    common = ["--name", "tiny", "--models_path", str(tmp_path), "--input", str(tmp_path / "case.npy"), "--precision", "f32"]
    saved = {k: sys.modules.get(k) for k in ("model", "train", "loss")}
    try:
        entry.main(common + ["--output", str(tmp_path / "one.npy")])
        entry.main(common + ["--output", str(tmp_path / "two.npy"), "--uncertainty", "std", "--uncertainty_output", str(tmp_path / "unc")])
        with pytest.raises(SystemExit):
            entry.main(common + ["--uncertainty", "std"])
        tr = TR.Trainer(name="tiny", models_root=str(tmp_path), rewrite=False, connect_tb=False)
        tr.load_best()
        net = tr.model.module if hasattr(tr.model, "module") else tr.model
        net.set_precision("f32")
        net = net.cuda()
    finally:
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v
            else:
                sys.modules.pop(k, None)
    assert np.array_equal(np.load(tmp_path / "one.npy"), np.load(tmp_path / "two.npy"))
    want = I.predict_case(net, img, uncertainty="std")[2]
    for r, stem in enumerate(I.UNCERTAINTY_STEMS):
        got = np.load(tmp_path / "unc" / ("case_unc_%s.npy" % stem))
        assert got.dtype == np.uint8 and got.shape == img.shape[1:]
        np.testing.assert_array_equal(got, want[r])
    assert want.any()


@pytest.mark.gpu
def test_uncertainty_entries_capture_into_a_hip_graph():
    """No allocation outside the caching allocator and no synchronisation inside the calls: accumulate -> fused finalize -> paste ->
    histogram -> score capture into one hipGraph; each replay rewrites the same results and adds the same score to the running sum."""
    from brats2019_amd import ops
    rng = np.random.default_rng(90)
    shape, lo, size = (3, 16, 24, 32), (2, 3, 4), (12, 18, 25)
    members, outs = _padded_outputs(rng, 2, 4, shape, lo, size)
    probs = [T(o).cuda() for o in outs]
    target = blob_labels(rng, shape[1:])
    gt, pred = T(target).cuda(), T(np.roll(target, 1, axis=2)).cuda()
    total = torch.zeros((3, 4), dtype=torch.float64, device="cuda")

    def run():
        acc, acc2 = ops.unc_accumulate(probs[0], FLIPS, None, None, lo, size)
        mask, counts, mean, unc = ops.unc_accumulate_finalize(probs[1], FLIPS, acc, acc2, 2, "std", lo, size, want_mean=True)
        maps = ops.paste_u8c(unc, shape[1:], lo)
        hist, invalid = ops.unc_histogram(pred, gt, maps)
        return mask, counts, unc, hist, invalid, ops.unc_score(hist, (25, 50, 75, 100), acc=total)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # eager warm-up on the capture stream
        eager = run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    once = total.clone()
    np.testing.assert_array_equal(eager[2].cpu().numpy(), oracle_std(members))
    assert (once[:, 0] > 0).all() and int(eager[4].cpu()[0]) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))
        np.testing.assert_allclose(total.cpu().numpy(), (k + 2) * once.cpu().numpy(), rtol=1e-15)
