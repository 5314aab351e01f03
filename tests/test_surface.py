"""Dice, sensitivity, specificity and HD95 of the BraTS challenge on the device (csrc/surface.hip, ru_surface_metrics): counts and
surfaces exactly, HD95 to rtol 1e-12 against the scipy / numpy oracle of tests/test_surface_host.py; the metric classes, Trainer.train
with them as validation metrics, graph capture, and `validate --regions` on full-size BraTS cases."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_surface_host import (EMPTY, blob_masks, oracle_batch, oracle_values, percentile_position, regions)

T = torch.from_numpy
RTOL_HD = 1e-12
RTOL_RATIO = 1e-15


def soft(rng, mask):
    """float32 values > 0.5 exactly on the mask"""
    return np.where(mask, 0.5 + rng.integers(1, 9, size=mask.shape) / 16.0, rng.integers(0, 9, size=mask.shape) / 16.0).astype(np.float32)


def _device(pred, gr, **kw):
    from brats2019_amd import ops
    vals, counts = ops.surface_metrics(T(np.ascontiguousarray(pred)).cuda(), T(np.ascontiguousarray(gr)).cuda(), **kw)
    assert vals.is_cuda and vals.dtype == torch.float64 and counts.dtype == torch.int64
    return vals.cpu().numpy(), counts.cpu().numpy()


def _check(pm, gm, what, rng, empty_value=EMPTY):
    """masks [N, K, D, H, W] -> checks the device against the oracle; returns the percentile positions t of the non-empty pairs"""
    kw = {} if empty_value == EMPTY else {"empty_value": empty_value}
    vals, counts = _device(soft(rng, pm), soft(rng, gm), **kw)
    want_vals, want_counts = oracle_batch(pm, gm, empty_value)
    assert vals.shape == want_vals.shape and counts.shape == want_counts.shape[:2] + (6,), what
    np.testing.assert_array_equal(counts[..., :5], want_counts, err_msg="%s: counts" % what)
    assert not counts[..., 5].any(), what
    np.testing.assert_allclose(vals[..., :3], want_vals[..., :3], rtol=RTOL_RATIO, atol=0, err_msg="%s: ratios" % what)
    np.testing.assert_allclose(vals[..., 3], want_vals[..., 3], rtol=RTOL_HD, atol=0, err_msg="%s: HD95" % what)
    both = (want_counts[..., 0] > 0) & (want_counts[..., 1] > 0)
    return [percentile_position(int(n))[2] for n in (want_counts[..., 3] + want_counts[..., 4])[both]]


@pytest.mark.gpu
def test_counts_surfaces_and_hd95_on_blobs_at_odd_extents():
    rng = np.random.default_rng(21)
    ts = []
    for n, c, shape in [(2, 3, (5, 37, 129)), (1, 2, (64, 1, 300)), (1, 2, (3, 4, 500)), (2, 2, (7, 9, 449)), (1, 3, (1, 1, 65))]:
        pm, gm = blob_masks(rng, shape, n * c).reshape((n, c) + shape), blob_masks(rng, shape, n * c).reshape((n, c) + shape)
        ts += _check(pm, gm, "blobs %s" % (shape,), rng)
    # sparse speckle: long gaps in every pass
    for shape in [(37, 41, 29), (6, 70, 130)]:
        pm, gm = rng.random((2, 2) + shape) < 0.004, rng.random((2, 2) + shape) < 0.004
        pm[:, :, 0, 0, 0] = gm[:, :, -1, -1, -1] = True
        ts += _check(pm, gm, "speckle %s" % (shape,), rng)
    assert any(0 < t < 0.5 for t in ts) and any(t >= 0.5 for t in ts)


@pytest.mark.gpu
def test_counts_surfaces_and_hd95_at_128_cubed():
    rng = np.random.default_rng(22)
    shape = (128, 128, 128)
    pm = blob_masks(rng, shape, 12, nblobs=4).reshape((4, 3) + shape)
    gm = blob_masks(rng, shape, 12, nblobs=4).reshape((4, 3) + shape)
    gm[1, 2] = pm[1, 2]                                                   # identical masks: HD95 0
    _check(pm, gm, "128^3", rng)


@pytest.mark.gpu
def test_special_masks_and_empty_rules():
    rng = np.random.default_rng(23)
    shape = (9, 7, 70)
    pm, gm = np.zeros((1, 6) + shape, bool), np.zeros((1, 6) + shape, bool)
    pm[0, 0, 0, 0, 0] = gm[0, 0, 8, 6, 69] = True                          # single voxels in opposite corners
    pm[0, 1] = gm[0, 1] = True                                             # the whole grid on both sides
    pm[0, 2, 2:5, 1:6, 10:60] = True                                       # identical boxes
    gm[0, 2] = pm[0, 2]
    pm[0, 3, 4, 3, 5] = True                                               # G empty
    gm[0, 4, 1:3, 1:3, 1:3] = True                                         # P empty
    _check(pm, gm, "special", rng)                                         # channel 5: both empty
    vals, counts = _device(soft(rng, pm), soft(rng, gm))
    assert vals[0, 0, 3] == np.sqrt(8 ** 2 + 6 ** 2 + 69 ** 2)
    assert vals[0, 1].tolist() == [1.0, 1.0, 1.0, 0.0] and vals[0, 2, 3] == 0.0
    v = 9 * 7 * 70
    assert vals[0, 3].tolist() == [0.0, 1.0, (v - 1) / v, EMPTY]
    assert vals[0, 4, 3] == EMPTY and vals[0, 4, 1] == 0.0 and vals[0, 5].tolist() == [1.0, 1.0, 1.0, 0.0]
    assert counts[0, 1, 3] == 2 * (9 * 7 + 9 * 70 + 7 * 70) - 4 * (9 + 7 + 70) + 8    # the box's boundary layer
    _check(pm, gm, "special, empty_value 1e6", rng, empty_value=1e6)


@pytest.mark.gpu
def test_percentile_positions_t_zero_below_and_above_one_half():
    rng = np.random.default_rng(24)
    shape = (1, 3, 40)
    pm, gm = np.zeros((1, 3) + shape, bool), np.zeros((1, 3) + shape, bool)
    pm[0, 0, 0, 1, 0:20] = True                                            # |dP| = 20 + |dG| = 1: n = 21, x = 19.0, t = 0
    gm[0, 0, 0, 1, 39] = True
    pm[0, 1, 0, 0, 0:12] = True                                            # n = 12 + 3 = 15: x = 13.3, t < 0.5
    gm[0, 1, 0, 2, 30:33] = True
    pm[0, 2, 0, 0, 5:11] = True                                            # n = 6 + 2 = 8: x = 6.65, t >= 0.5
    gm[0, 2, 0, 2, 20:22] = True
    ts = _check(pm, gm, "positions", rng)
    assert ts[0] == 0.0 and 0 < ts[1] < 0.5 and ts[2] >= 0.5


@pytest.mark.gpu
def test_uint8_label_volumes_score_the_three_regions():
    from brats2019_amd import ops
    rng = np.random.default_rng(25)
    shape = (2, 11, 37, 70)
    lab = rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), size=shape, p=[0.5, 0.15, 0.15, 0.1, 0.1])
    pre = lab.copy()
    flip = rng.random(shape) < 0.2
    pre[flip] = rng.integers(0, 5, size=int(flip.sum()))
    vals, counts = ops.surface_metrics(T(pre).cuda(), T(lab).cuda())
    vals, counts = vals.cpu().numpy(), counts.cpu().numpy()
    want_vals, want_counts = oracle_batch(regions(pre), regions(lab))
    assert vals.shape == (2, 3, 4)
    np.testing.assert_array_equal(counts[..., :5], want_counts)
    assert not counts[..., 5].any()
    np.testing.assert_allclose(vals[..., :3], want_vals[..., :3], rtol=RTOL_RATIO, atol=0)
    np.testing.assert_allclose(vals[..., 3], want_vals[..., 3], rtol=RTOL_HD, atol=0)
    bad = pre.copy()
    bad[1, 3, 4, 5] = 5
    bad[1, 0, 0, 0] = 200
    counts = ops.surface_metrics(T(bad).cuda(), T(lab).cuda())[1].cpu().numpy()
    assert counts[0, :, 5].tolist() == [0, 0, 0] and counts[1, :, 5].tolist() == [2, 2, 2]


@pytest.mark.gpu
def test_refuses_extents_above_512():
    from brats2019_amd import ops
    for shape in [(1, 1, 2, 3, 513), (1, 1, 513, 2, 3)]:
        x = torch.zeros(shape, device="cuda")
        with pytest.raises(RuntimeError, match="extents"):
            ops.surface_metrics(x, x)
    p = torch.zeros((1, 1, 4, 4, 4), device="cuda")
    p[0, 0, 0, 0, 0] = 1.0
    q = torch.zeros_like(p)
    q[0, 0, 3, 3, 3] = 1.0
    vals, counts = ops.surface_metrics(p, q)                               # nothing was launched: the device still works
    assert counts.cpu().tolist() == [[[1, 1, 0, 1, 1, 0]]] and vals[0, 0, 3].item() == np.sqrt(27.0)


def _run(m, batches, on_device=True):
    got = []
    for b in batches:
        gr, p = T(b[1]), T(b[0])
        if on_device:
            gr, p = gr.cuda(), p.cuda()
        m.update([gr], [p])
        assert isinstance(m.accumulator, torch.Tensor) and m.accumulator.is_cuda and m.accumulator.dtype == torch.float64
        got.append(np.asarray(m.get(), dtype=np.float64))
    return np.stack(got)


@pytest.mark.gpu
def test_metric_classes_update_get_reset():
    from brats2019_amd import metrics
    rng = np.random.default_rng(26)
    shape = (12, 20, 33)
    batches, wants = [], []
    for i in range(3):
        pm, gm = blob_masks(rng, shape, 6).reshape((2, 3) + shape), blob_masks(rng, shape, 6).reshape((2, 3) + shape)
        if i == 1:
            pm[0, 1] = False                                               # one empty mask: empty_value
        batches.append((soft(rng, pm), soft(rng, gm)))
        wants.append(oracle_batch(pm, gm, 50.0)[0])
    for cls, col, kw in [(metrics.Hausdorff95, 3, {"empty_value": 50.0}), (metrics.Sensitivity, 1, {}), (metrics.Specificity, 2, {})]:
        for classes in (4, 3):
            m = cls(classes=classes, **kw)
            for on_device in (False, True):
                m.reset()
                got = _run(m, batches, on_device)
                want = np.cumsum([w[:, :classes - 1, col].mean(axis=0) for w in wants], axis=0) / np.arange(1, 4)[:, None]
                np.testing.assert_allclose(got, want, rtol=RTOL_HD, atol=0, err_msg=cls.__name__)
                assert m.get().shape == (classes - 1,) and m.samples == 3
        with pytest.raises(IndexError):
            cls(classes=5).update([T(batches[0][1])], [T(batches[0][0])])


@pytest.mark.gpu
def test_trainer_runs_with_the_challenge_metrics(tmp_path):
    from brats2019_amd import model as M, loss as L, train as TR, metrics
    seed, dhw = 43, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="hd95", models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
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
                          metrics.Hausdorff95(name='Hausdorff95', input_index=0, target_index=0, classes=4),
                          metrics.Sensitivity(name='Sensitivity', input_index=0, target_index=0, classes=4),
                          metrics.Specificity(name='Specificity', input_index=0, target_index=0, classes=4),
                          ],
             track_metric='Dice', epoches=1, default_val=np.array([0, 0, 0, 0, 0]),
             comparator=lambda x, y: np.min(x) + np.mean(x) > np.min(y) + np.mean(y),
             eval_cpu=False, continue_form_pretraining=False)
    batch = loader[1]
    pred = tr.predict(batch)[0].detach().cpu().numpy()
    want = oracle_batch(pred > 0.5, batch[1][0].numpy() > 0.5)[0].mean(axis=0)         # [3 channels, 4]
    for name, col in [("Hausdorff95", 3), ("Sensitivity", 1), ("Specificity", 2)]:
        got = np.array([logged["val/%s-%d" % (name, i)] for i in range(3)])
        assert tr.state.val_metric[name][0].shape == (3,)
        np.testing.assert_allclose(got, want[:, col], rtol=RTOL_HD, atol=0, err_msg=name)


@pytest.mark.gpu
def test_surface_entries_capture_into_a_hip_graph():
    """No allocation and no synchronisation inside the calls: `surface_metrics` + `surface_accumulate` capture into one hipGraph, and
    each replay adds the same batch mean again."""
    from brats2019_amd import ops
    rng = np.random.default_rng(27)
    shape = (16, 12, 70)
    pred = T(soft(rng, blob_masks(rng, shape, 6)).reshape((2, 3) + shape)).cuda()
    gr = T(soft(rng, blob_masks(rng, shape, 6)).reshape((2, 3) + shape)).cuda()
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # eager warm-up on the capture stream
        vals_e, counts_e = ops.surface_metrics(pred, gr)
        ops.surface_accumulate(vals_e, acc, 3, "hd95")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    once = acc.clone()
    assert (once > 0).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vals_c, counts_c = ops.surface_metrics(pred, gr)
        ops.surface_accumulate(vals_c, acc, 3, "hd95")
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(vals_c, vals_e) and torch.equal(counts_c, counts_e)
        np.testing.assert_allclose(acc.cpu().numpy(), (k + 2) * once.cpu().numpy(), rtol=1e-15)


def _brats_labels(rng, shape):
    """a synthetic case: spheres of label 2, then 1, then 4 drawn over each other around three centres"""
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    lab = np.zeros(shape, np.uint8)
    spheres = []
    for _ in range(3):
        c, r = [rng.uniform(0.2 * s, 0.8 * s) for s in shape], rng.uniform(5.0, 20.0)
        spheres.append((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2)
    for value, scale in [(2, 2.5), (1, 1.6), (4, 1.0)]:
        for d2, r in zip(spheres, rng.uniform(5.0, 20.0, size=3)):
            lab[d2 <= (scale * r) ** 2] = value
    return lab


@pytest.mark.gpu
def test_validate_regions_scores_full_brats_cases(tmp_path, capsys):
    from brats2019_amd import validate
    rng = np.random.default_rng(28)
    shape = (240, 240, 155)
    (tmp_path / "data").mkdir()
    (tmp_path / "pred").mkdir()
    want = []
    for i in range(2):
        lab = _brats_labels(rng, shape)
        pre = lab.copy()
        pre[100 + 10 * i:130, 90:140, 60:90] = 3 if i else 2               # a block of changed labels (3 counts as 4)
        np.save(tmp_path / "data" / ("case%d.npy" % i), lab)
        np.save(tmp_path / "pred" / ("case%d.npy" % i), pre)
        pr, gr = regions(pre), regions(lab)
        want.append(np.array([oracle_values(pr[k], gr[k]) for k in range(3)]).T)           # [4 metrics, 3 regions]
    want = np.stack(want)
    res, mean = validate.main(["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred"), "--regions"])
    assert res.shape == (2, 4, 3) and mean.shape == (4, 3) and res.dtype == np.float64
    np.testing.assert_allclose(res[:, :3], want[:, :3], rtol=RTOL_RATIO, atol=0)
    np.testing.assert_allclose(res[:, 3], want[:, 3], rtol=RTOL_HD, atol=0)
    np.testing.assert_allclose(mean, want.mean(axis=0), rtol=RTOL_HD, atol=0)
    out = capsys.readouterr().out
    assert "case0 Dice WT" in out and "case1 Dice WT" in out and "mean Dice WT" in out
    bad = np.load(tmp_path / "pred" / "case1.npy")
    bad[0, 0, 0] = 5
    np.save(tmp_path / "pred" / "case1.npy", bad)
    with pytest.raises(ValueError, match="case1"):
        validate.main(["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred"), "--regions"])
