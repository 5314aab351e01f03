"""Lesion-wise Dice and HD95 on the device (csrc/lesion.hip, ru_lesion_metrics) against the scipy oracle of tests/test_lesion_host.py:
counts, vol_i, |M_i| and tp_i exactly, Dice_i and LesionDice to test_surface.py's RTOL_RATIO, HD95_i and LesionHD95 to its RTOL_HD; at
the smallest shapes at which each pass (packing and carries, the 18-neighbour dilation, labelling, matching, chunking) can go wrong."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_surface import RTOL_HD, RTOL_RATIO, soft
from test_surface_host import EMPTY, blob_masks, regions
from test_lesion_host import cube, oracle_lesion_batch

T = torch.from_numpy


def _compare(got, pm, gm, what, **kw):
    summary, counts, table = (t.cpu().numpy() for t in got)
    want_summary, want_counts, want_rows = oracle_lesion_batch(pm, gm, **kw)
    print(what, "counts", counts[..., :5].reshape(-1, 5).tolist(), "summary", summary.reshape(-1, 2).tolist())
    assert summary.dtype == np.float64 and summary.shape == want_summary.shape and counts.shape == want_counts.shape[:2] + (6,), what
    np.testing.assert_array_equal(counts[..., :5], want_counts, err_msg="%s: counts" % what)
    for n in range(pm.shape[0]):
        for k in range(pm.shape[1]):
            rows, m = want_rows[n][k], len(want_rows[n][k])
            np.testing.assert_array_equal(table[n, k, :m, :3], rows[:, :3], err_msg="%s: vol, |M|, tp of (%d, %d)" % (what, n, k))
            np.testing.assert_allclose(table[n, k, :m, 3], rows[:, 3], rtol=RTOL_RATIO, atol=0, err_msg="%s: Dice_i" % what)
            np.testing.assert_allclose(table[n, k, :m, 4], rows[:, 4], rtol=RTOL_HD, atol=0, err_msg="%s: HD95_i" % what)
            assert not table[n, k, m:].any(), what
    np.testing.assert_allclose(summary[..., 0], want_summary[..., 0], rtol=RTOL_RATIO, atol=0, err_msg="%s: LesionDice" % what)
    np.testing.assert_allclose(summary[..., 1], want_summary[..., 1], rtol=RTOL_HD, atol=0, err_msg="%s: LesionHD95" % what)
    return want_counts, want_rows


def _check(pm, gm, what, rng=None, max_lesions=256, **kw):
    """masks [N, K, D, H, W] -> the device (float32 probabilities) against the oracle; returns the oracle's (counts, rows)"""
    from brats2019_amd import ops
    rng = rng or np.random.default_rng(0)
    got = ops.lesion_metrics(T(soft(rng, pm)).cuda(), T(soft(rng, gm)).cuda(), want_table=True, max_lesions=max_lesions, **kw)
    assert got[0].is_cuda and got[1].dtype == torch.int64 and not got[1][..., 5].any()
    return _compare(got, pm, gm, what, **kw)


def _stack(masks):
    return np.stack(masks)[None]                                           # K masks -> [1, K, D, H, W]


@pytest.mark.gpu
def test_packing_and_carries_at_odd_widths():
    rng = np.random.default_rng(31)
    for shape in [(9, 10, 37), (5, 7, 70), (1, 12, 40)]:
        pm, gm = blob_masks(rng, shape, 4).reshape((2, 2) + shape), blob_masks(rng, shape, 4).reshape((2, 2) + shape)
        for m in (pm, gm):                                                 # every face of the grid is touched
            m[:, :, 0, 0, 0] = m[:, :, -1, -1, -1] = m[:, :, 0, -1, 0] = m[:, :, -1, 0, -1] = True
        _check(pm, gm, "blobs %s" % (shape,), rng, min_volume=0)
        _check(pm, gm, "blobs %s, default volume" % (shape,), rng)
    # only a carry joins the fragments: 62 grows to 65 through the word boundary, 69 down to 66; 65 grows down to 62, 58 up to 61
    shape = (5, 7, 70)
    up, down, both = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    up[2, 3, 62] = up[2, 3, 69] = True
    down[2, 3, 58] = down[2, 3, 65] = True
    both[4, 6, 63] = both[0, 0, 64] = both[0, 0, 57] = True               # set bits on both sides of the boundary
    gm = _stack([up, down, both])
    counts, _ = _check(gm.copy(), gm, "carries", rng, min_volume=0)
    assert counts[0, :2, 0].tolist() == [1, 1]
    apart = np.zeros(shape, bool)
    apart[2, 3, 61] = apart[2, 3, 69] = True                               # 7 between: the carry must not join more than it should
    counts, _ = _check(_stack([apart]), _stack([apart]), "carries, apart", rng, min_volume=0)
    assert counts[0, 0, 0] == 2


@pytest.mark.gpu
def test_the_dilation_uses_the_18_neighbour_structure():
    shape = (12, 12, 12)
    g3 = np.zeros(shape, bool)
    g3[2, 2, 2] = g3[5, 5, 2] = g3[5, 5, 5] = True                          # offsets (3, 3, 0) and (3, 3, 3) from the first
    far = np.zeros(shape, bool)
    far[1, 1, 1] = far[8, 8, 1] = far[8, 1, 1] = True                       # (7, 7, 0): joined by the 18-structure, not by the 6-structure
    counts, _ = _check(_stack([g3, far]), _stack([g3, far]), "structure", min_volume=0)
    # one voxel, dilation 3: (3, 3, 0) and (3, 2, 1) lie in Z, (3, 3, 3) and (3, 2, 2) do not -- specks there are false positives
    g = np.zeros(shape, bool)
    g[5, 5, 5] = True
    p = np.zeros(shape, bool)
    p[8, 8, 5] = p[2, 3, 4] = True                                          # +(3, 3, 0), -(3, 2, 1): matched
    p[8, 8, 8] = p[2, 3, 7] = True                                          # +(3, 3, 3), (-3, -2, +2): not reached
    counts, rows = _check(_stack([p]), _stack([g]), "structure, specks", min_volume=0)
    assert counts[0, 0].tolist() == [1, 1, 1, 0, 2] and rows[0][0][0, :3].tolist() == [1, 2, 0]
    # dilation 1 tells the structures apart: (1, 1, 0) is in Z for 18 and 26, (-1, -1, -1) only for 26
    p1 = np.zeros(shape, bool)
    p1[6, 6, 5] = p1[4, 4, 4] = True
    counts, _ = _check(_stack([p1]), _stack([g]), "structure, dilation 1", min_volume=0, dilation=1)
    assert counts[0, 0].tolist() == [1, 1, 1, 0, 1]


@pytest.mark.gpu
def test_the_gap_rule_along_each_axis():
    shape = (20, 20, 20)
    masks, want = [], []
    for axis in range(3):
        for gap in (6, 7):
            g = np.zeros(shape, bool)
            lo = [3, 3, 3]
            g[tuple(slice(l, l + 2) for l in lo)] = True
            lo[axis] += 2 + gap
            g[tuple(slice(l, l + 2) for l in lo)] = True
            masks.append(g)
            want.append(1 if gap == 6 else 2)
    gm = _stack(masks)
    counts, _ = _check(gm.copy(), gm, "gap rule", min_volume=0)
    assert counts[0, :, 0].tolist() == want


@pytest.mark.gpu
def test_matching_bridges_halo_components_and_dropped_lesions():
    shape = (12, 14, 40)
    g = np.zeros(shape, bool)
    g[5, 5, 5:8] = g[5, 5, 15:18] = True                                    # two lesions, 7 apart
    bridge = np.zeros(shape, bool)
    bridge[5, 5, 5:18] = True                                               # one component in both M_i
    counts, rows = _check(_stack([bridge]), _stack([g]), "bridge", min_volume=0)
    assert counts[0, 0].tolist() == [2, 2, 2, 0, 0] and rows[0][0][:, 1].tolist() == [13, 13]
    halo = np.zeros(shape, bool)
    halo[5, 7, 6] = True                                                    # in Z_1 \ L_1 only: matched, tp 0, finite HD95, no false positive
    counts, rows = _check(_stack([halo]), _stack([g]), "halo", min_volume=0)
    assert counts[0, 0].tolist() == [2, 2, 1, 1, 0] and rows[0][0][0, :4].tolist() == [3, 1, 0, 0.0] and rows[0][0][0, 4] < 3.0
    small, big = cube(shape, (1, 1, 1), (2, 5, 5)), cube(shape, (6, 8, 30), (2, 5, 5))
    big[8, 8, 30] = True                                                    # 50 and 51 voxels
    gm = _stack([small | big, small | big, small | big])
    pm = _stack([small | big, small, big])                                  # the second matches the dropped lesion only
    counts, _ = _check(pm, gm, "dropped")
    assert counts[0].tolist() == [[2, 1, 1, 0, 0], [2, 1, 0, 1, 0], [2, 1, 1, 0, 0]]


@pytest.mark.gpu
def test_many_predicted_components_and_a_serpentine():
    rng = np.random.default_rng(0)
    shape = (24, 24, 40)
    noise = rng.random(shape) < 0.02
    g = cube(shape, (2, 2, 2), (5, 5, 5)) | cube(shape, (14, 3, 20), (4, 6, 8)) | cube(shape, (2, 16, 32), (5, 5, 5))
    snake = np.zeros(shape, bool)                                           # one component folding back and forth through the grid
    for z in range(0, 24, 2):
        for y in range(0, 24, 2):
            snake[z, y, :] = True
            snake[z, min(y + 1, 23), 0 if (y // 2) % 2 else 39] = True
        snake[min(z + 1, 23), 22 if (z // 2) % 2 == 0 else 0, 39 if (z // 2) % 2 == 0 else 0] = True
    pm, gm = _stack([noise, snake, g, noise]), _stack([g, g, snake, noise])
    counts, rows = _check(pm, gm, "noise and serpentine", rng)
    assert counts[0, 0, 0] == 3 and counts[0, 0, 4] > 200                  # hundreds of false-positive specks
    assert counts[0, 1].tolist()[:1] == [3] and rows[0][1][0, 1] == snake.sum()


@pytest.mark.gpu
def test_more_lesions_than_one_hd95_chunk_and_the_capacity_error():
    from brats2019_amd import _lib as L, ops
    shape = (16, 40, 76)
    g = np.zeros(shape, bool)
    for z in range(0, 15, 9):
        for y in range(0, 39, 9):
            for x in range(0, 75, 9):
                g[z:z + 2, y:y + 2, x:x + 2] = True
    p = np.roll(g, 1, axis=2)
    p[:, :, 0:40] &= np.roll(g, 1, axis=1)[:, :, 0:40]                       # different overlaps left and right
    counts, rows = _check(_stack([p]), _stack([g]), "lattice", min_volume=0)
    n = int(counts[0, 0, 0])
    assert n == 2 * 5 * 9 and n > 2 * L.LESION_CHUNK
    rng = np.random.default_rng(1)
    dev = T(soft(rng, _stack([p]))).cuda(), T(soft(rng, _stack([g]))).cuda()
    exact = ops.lesion_metrics(*dev, min_volume=0, want_table=True, max_lesions=n)        # exactly the capacity: fits
    assert exact[1][0, 0, 0].item() == n and exact[2].shape == (1, 1, n, 5)
    with pytest.raises(RuntimeError, match="max_lesions"):
        ops.lesion_metrics(*dev, min_volume=0, want_table=True, max_lesions=n - 1)        # the error, not a truncated table
    again = ops.lesion_metrics(*dev, min_volume=0, want_table=True, max_lesions=n)        # the device still works
    assert all(torch.equal(a, b) for a, b in zip(exact, again))


@pytest.mark.gpu
def test_parameters_batches_and_label_volumes():
    from brats2019_amd import ops
    rng = np.random.default_rng(33)
    shape = (10, 18, 45)
    pm, gm = blob_masks(rng, shape, 6).reshape((2, 3) + shape), blob_masks(rng, shape, 6).reshape((2, 3) + shape)
    gm[1] |= rng.random((3,) + shape) < 0.003                               # the second sample has many more lesions
    pm[0, 2] = False
    gm[1, 2] = False
    for kw in [dict(dilation=0), dict(dilation=1), dict(min_volume=0), dict(empty_value=50.0), dict(dilation=2, min_volume=3, empty_value=1e6)]:
        counts, _ = _check(pm, gm, "parameters %s" % (kw,), rng, **kw)
    assert counts[0, :, 0].tolist() != counts[1, :, 0].tolist()
    # uint8 label volumes: the three regions; a label 7 is in no region and is counted
    lab = rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), size=(2,) + shape, p=[0.9, 0.03, 0.03, 0.02, 0.02])
    lab[:, 2:7, 3:12, 5:30] = 2
    lab[:, 3:6, 5:9, 10:20] = 4
    pre = lab.copy()
    pre[0, 2:7, 3:12, 5:12] = 0
    pre[1, 8, 15, 40] = 1
    got = ops.lesion_metrics(T(pre).cuda(), T(lab).cuda(), want_table=True, min_volume=5)
    assert got[0].shape == (2, 3, 2) and not got[1][..., 5].any()
    _compare(got, regions(pre), regions(lab), "labels", min_volume=5)
    bad_pre, bad_lab = pre.copy(), lab.copy()
    bad_pre[1, 4, 6, 12] = bad_lab[1, 4, 6, 12] = 7
    bad_lab[1, 0, 0, 0] = 7
    got = ops.lesion_metrics(T(bad_pre).cuda(), T(bad_lab).cuda(), want_table=True, min_volume=5)
    assert got[1][..., 5].cpu().tolist() == [[0, 0, 0], [2, 2, 2]]
    _compare(got, regions(bad_pre), regions(bad_lab), "labels with a 7", min_volume=5)


@pytest.mark.gpu
def test_refuses_extents_above_512_and_two_calls_give_identical_bytes():
    from brats2019_amd import ops
    x = torch.zeros((1, 1, 2, 3, 513), device="cuda")
    with pytest.raises(RuntimeError, match="extents"):
        ops.lesion_metrics(x, x)
    rng = np.random.default_rng(34)
    shape = (24, 24, 40)
    p = T(soft(rng, (rng.random((1, 3) + shape) < 0.03))).cuda()
    g = T(soft(rng, blob_masks(rng, shape, 3).reshape((1, 3) + shape))).cuda()
    a, b = ops.lesion_metrics(p, g, want_table=True, min_volume=0), ops.lesion_metrics(p, g, want_table=True, min_volume=0)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and a[1][0, 0, 4].item() > 100


def _run(m, batches):
    got = []
    for b in batches:
        m.update([T(b[1]).cuda()], [T(b[0]).cuda()])
        assert isinstance(m.accumulator, torch.Tensor) and m.accumulator.is_cuda and m.accumulator.dtype == torch.float64
        got.append(np.asarray(m.get(), dtype=np.float64))
    return np.stack(got)


@pytest.mark.gpu
def test_metric_classes_update_get_reset():
    from brats2019_amd import metrics
    rng = np.random.default_rng(36)
    shape = (12, 20, 33)
    batches, wants = [], []
    for i in range(2):
        pm, gm = blob_masks(rng, shape, 6).reshape((2, 3) + shape), blob_masks(rng, shape, 6).reshape((2, 3) + shape)
        pm |= rng.random(pm.shape) < 0.002
        batches.append((soft(rng, pm), soft(rng, gm)))
        wants.append(oracle_lesion_batch(pm, gm, dilation=2, min_volume=4, empty_value=50.0)[0])
    for cls, col in [(metrics.LesionWiseDice, 0), (metrics.LesionWiseHausdorff95, 1)]:
        for classes in (4, 3):
            m = cls(classes=classes, dilation=2, min_volume=4, empty_value=50.0)
            for _ in range(2):
                m.reset()
                got = _run(m, batches)
                want = np.cumsum([w[:, :classes - 1, col].mean(axis=0) for w in wants], axis=0) / np.arange(1, 3)[:, None]
                np.testing.assert_allclose(got, want, rtol=RTOL_HD, atol=0, err_msg=cls.__name__)
                assert m.get().shape == (classes - 1,) and m.samples == 2
        with pytest.raises(IndexError):
            cls(classes=5).update([T(batches[0][1])], [T(batches[0][0])])


@pytest.mark.gpu
def test_trainer_runs_with_the_lesionwise_metrics(tmp_path):
    from brats2019_amd import model as M, loss as L, train as TR, metrics
    seed, dhw = 43, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="lesionwise", models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    logged = {}

    class Rec:
        def add_scalar(self, name, val, step):
            logged[name] = float(val)
    tr.tb_writer = Rec()
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(O.make_target(2, *dhw, seed=seed + i))]) for i in range(2)]
    tr.train(criterion=[L.Dice_loss_joint(index=0, priority=1), L.BCE_Loss(index=0, bg_weight=1e-2)],
             optimizer=torch.optim.Adam, optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=16000, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=False, pretrained_weights=None,
             train_metrics=[metrics.Dice(name='Dice', input_index=0, target_index=0, classes=4), ],
             val_metrics=[metrics.Dice(name='Dice', input_index=0, target_index=0, classes=4),
                          metrics.LesionWiseDice(name='LesionWiseDice', input_index=0, target_index=0, classes=4),
                          metrics.LesionWiseHausdorff95(name='LesionWiseHausdorff95', input_index=0, target_index=0, classes=4),
                          ],
             track_metric='Dice', epoches=1, default_val=np.array([0, 0, 0, 0, 0]),
             comparator=lambda x, y: np.min(x) + np.mean(x) > np.min(y) + np.mean(y),
             eval_cpu=False, continue_form_pretraining=False)
    batch = loader[1]
    pred = tr.predict(batch)[0].detach().cpu().numpy()
    want = oracle_lesion_batch(pred > 0.5, batch[1][0].numpy() > 0.5)[0].mean(axis=0)        # [3 channels, 2]
    for name, col in [("LesionWiseDice", 0), ("LesionWiseHausdorff95", 1)]:
        got = np.array([logged["val/%s-%d" % (name, i)] for i in range(3)])
        assert tr.state.val_metric[name][0].shape == (3,)
        np.testing.assert_allclose(got, want[:, col], rtol=RTOL_HD, atol=0, err_msg=name)


@pytest.mark.gpu
def test_validate_lesionwise_scores_saved_cases(tmp_path, capsys):
    from brats2019_amd import validate
    rng = np.random.default_rng(38)
    shape = (20, 30, 45)
    (tmp_path / "data").mkdir()
    (tmp_path / "pred").mkdir()
    want, want_counts = [], []
    for i in range(3):
        lab = np.zeros(shape, np.uint8)
        lab[3:12, 4:16, 5:25] = 2
        lab[5:10, 6:12, 8:18] = 1
        lab[6:9, 7:10, 10:15] = 4
        lab[15:18, 22:27, 35:41] = 2 if i else 4                            # a second lesion: 90 voxels
        lab[1, 28, 2 + i] = 1                                               # a tiny one: dropped
        pre = lab.copy()
        if i == 1:
            pre[15:18, 22:27, 35:41] = 0                                    # missed
        if i == 2:
            pre[18, 1, 40] = 3                                              # a speck (3 counts as 4)
        np.save(tmp_path / "data" / ("case%d.npy" % i), lab)
        np.save(tmp_path / "pred" / ("case%d.npy" % i), pre)
        s, c, _ = oracle_lesion_batch(regions(pre)[None], regions(lab)[None])
        want.append(s[0].T)                                                 # [2 metrics, 3 regions]
        want_counts.append(c[0])
    want = np.stack(want)
    args = ["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred"), "--lesionwise"]
    res, mean = validate.main(args)
    assert res.shape == (3, 2, 3) and mean.shape == (2, 3) and res.dtype == np.float64
    np.testing.assert_allclose(res[:, 0], want[:, 0], rtol=RTOL_RATIO, atol=0)
    np.testing.assert_allclose(res[:, 1], want[:, 1], rtol=RTOL_HD, atol=0)
    np.testing.assert_allclose(mean, want.mean(axis=0), rtol=RTOL_HD, atol=0)
    out = capsys.readouterr().out
    assert "case0 LesionDice WT" in out and "mean LesionDice WT" in out
    assert "WT gt %d kept %d tp %d fn %d fp %d" % tuple(want_counts[1][0]) in out.split("case1 ")[1].split("\n")[0]
    names, _, _, counts = validate.score_lesionwise(
        (("case%d" % i, np.load(tmp_path / "data" / ("case%d.npy" % i)), np.load(tmp_path / "pred" / ("case%d.npy" % i))) for i in range(3)))
    np.testing.assert_array_equal(counts, np.stack(want_counts))
    res0, _ = validate.main(args + ["--dilation", "0", "--min_volume", "0"])
    s0 = oracle_lesion_batch(regions(np.load(tmp_path / "pred" / "case2.npy"))[None], regions(np.load(tmp_path / "data" / "case2.npy"))[None],
                             dilation=0, min_volume=0)[0]
    np.testing.assert_allclose(res0[2], s0[0].T, rtol=RTOL_HD, atol=0)
    bad = np.load(tmp_path / "pred" / "case1.npy")
    bad[0, 0, 0] = 5
    np.save(tmp_path / "pred" / "case1.npy", bad)
    with pytest.raises(ValueError, match="case1"):
        validate.main(args)
