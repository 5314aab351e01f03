"""Dice1D, RMSE, RMSE_masked, DiceWT, Dice_ITK (metrics.py:22-185) and validate.py on the device: the label confusion pass
(ru_label_confusion) exactly against np.bincount, the metric classes and brats2019_amd.validate against tests/golden/overlap.npz (the
reference's own classes and script), graph capture of the new entry points, the torch path for more than 8 channels, and
Trainer.train with the new metrics in its train and validation lists."""
import os

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_overlap_host import (conf_label, conf_prob, oracle_run, rmse_value, rtol_of, run_names, validate_result)

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def nested(rng, n, shape):
    """Targets as the dataloader builds them: WT >= TC >= ET one-hot regions of a label volume."""
    lab = rng.integers(0, 4, size=(n,) + shape)
    return np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3], axis=1).astype(np.float32)


def _conf(pred, gr):
    from brats2019_amd import ops
    conf, invalid = ops.label_confusion(T(np.ascontiguousarray(pred)).cuda(), T(np.ascontiguousarray(gr)).cuda())
    assert conf.is_cuda and conf.dtype == torch.int64
    return conf.cpu().numpy(), None if invalid is None else invalid.cpu().numpy()


def test_label_confusion_is_exact_for_every_channel_count_and_ragged_sizes():
    rng = np.random.default_rng(21)
    for c in range(1, 9):
        for v in (1, 7, 130, 4096 + 3, 64 * 1024):
            n = 1 if v == 1 else 3
            pred = (rng.integers(0, 4, size=(n, c, v)) / 4.0).astype(np.float32)     # ties everywhere
            gr = (rng.integers(0, 3, size=(n, c, v)) / 2.0).astype(np.float32)
            got, _ = _conf(pred, gr)
            np.testing.assert_array_equal(got, conf_prob(pred, gr), err_msg="C=%d V=%d" % (c, v))
            assert got.sum() == n * v
    for v in (1, 7, 130, 1001, 4096):
        pred = rng.integers(0, 5, size=(2, v)).astype(np.uint8)
        gr = rng.integers(0, 5, size=(2, v)).astype(np.uint8)
        got, inv = _conf(pred, gr)
        want, winv = conf_label(pred, gr)
        np.testing.assert_array_equal(got, want, err_msg="labels V=%d" % v)
        np.testing.assert_array_equal(inv, winv)


def test_label_confusion_on_nested_targets_ties_nans_and_invalid_labels():
    rng = np.random.default_rng(22)
    g = nested(rng, 2, (9, 7, 5))
    p = (rng.integers(0, 9, size=g.shape) / 8.0).astype(np.float32)
    got, _ = _conf(p, g)
    np.testing.assert_array_equal(got, conf_prob(p, g))
    assert (got[:, :, 1:] == 0).all()                                     # a nested target's argmax is 0 everywhere
    ties = np.full((2, 3, 130), 0.5, np.float32)
    np.testing.assert_array_equal(_conf(ties, ties)[0][:, 0, 0], [130, 130])
    nan = (rng.integers(0, 3, size=(2, 4, 333)) / 2.0).astype(np.float32)
    nan[rng.random(nan.shape) < 0.2] = np.nan
    gn = nan[:, ::-1].copy()
    np.testing.assert_array_equal(_conf(nan, gn)[0], conf_prob(nan, gn))
    lab = rng.integers(0, 5, size=(3, 17, 9, 6)).astype(np.uint8)
    pl = lab.copy()
    pl[0, 0, 0, :3] = [5, 200, 255]
    lab[1, 3, 3, 3] = 7
    pl[1, 3, 3, 3] = 9                                                    # both invalid: counted once
    got, inv = _conf(pl, lab)
    want, winv = conf_label(pl, lab)
    np.testing.assert_array_equal(got, want)
    assert inv.tolist() == winv.tolist() == [3, 1, 0]


def test_label_confusion_is_exact_at_training_and_full_case_sizes():
    rng = np.random.default_rng(23)
    for n, shape in [(4, (128, 128, 128)), (1, (240, 240, 155))]:
        g = nested(rng, n, shape)
        if n == 1:                                                        # free probabilities: every label pair occurs
            g = (rng.integers(0, 5, size=g.shape) / 4.0).astype(np.float32)
        p = (rng.integers(0, 9, size=g.shape) / 8.0).astype(np.float32)
        np.testing.assert_array_equal(_conf(p, g)[0], conf_prob(p, g), err_msg=str(shape))
    lab = rng.integers(0, 5, size=(1, 240, 240, 155)).astype(np.uint8)
    pl = rng.integers(0, 5, size=lab.shape).astype(np.uint8)
    got, inv = _conf(pl, lab)
    np.testing.assert_array_equal(got, conf_label(pl, lab)[0])
    assert inv.tolist() == [0]


def test_label_confusion_refuses_more_than_8_channels_and_the_torch_path_agrees():
    from brats2019_amd import metrics, ops
    x = torch.zeros((1, 9, 10), device="cuda")
    with pytest.raises(ValueError):
        ops.label_confusion(x, x)
    rng = np.random.default_rng(24)
    for c in (8, 9, 12):
        p = T((rng.integers(0, 4, size=(3, c, 5, 6, 7)) / 4.0).astype(np.float32)).cuda()
        g = T((rng.integers(0, 4, size=(3, c, 5, 6, 7)) / 4.0).astype(np.float32)).cuda()
        want = conf_prob(p.cpu().numpy(), g.cpu().numpy())
        np.testing.assert_array_equal(metrics.confusion_torch(p, g).cpu().numpy(), want)
        if c == 8:
            np.testing.assert_array_equal(ops.label_confusion(p, g)[0].cpu().numpy(), want)
        m_dev, m_any = metrics.Dice_ITK(classes=c), metrics.DiceWT()
        m_dev.update([g], [p])
        m_any.update([g], [p])
        assert np.isfinite(m_any.get())


def _make(g, name):
    from brats2019_amd import metrics
    cls = {"dice1d": metrics.Dice1D, "rmsemasked": metrics.RMSE_masked, "rmse": metrics.RMSE, "wt": metrics.DiceWT, "itk": metrics.Dice_ITK}
    for k in ("dice1d", "rmsemasked", "rmse", "wt", "itk"):
        if name.startswith(k):
            c = cls[k]
            break
    classes = int(g["run_%s_classes" % name])
    return c(name=str(g["run_%s_name" % name]), classes=classes) if classes >= 0 else c(name=str(g["run_%s_name" % name]))


def _run(m, g, name, on_device):
    pre = "m" if name == "rmsemasked" else "b"                                 # rmsemaskedbad runs on a regular batch
    vals = []
    for _ in range(2):
        m.reset()
        for b in g["run_%s_order" % name]:
            p, gr = T(g["%s%d_pred" % (pre, b)]), T(g["%s%d_gr" % (pre, b)])
            if on_device:
                p, gr = p.cuda(), gr.cuda()
            m.update([gr], [p])
            assert isinstance(m.accumulator, torch.Tensor) and m.accumulator.is_cuda and m.accumulator.dtype == torch.float64
            vals.append(np.atleast_1d(np.asarray(m.get(), dtype=np.float64)))
    return np.stack(vals)


def test_metric_classes_match_the_reference_fixture(golden):
    g = golden("overlap")
    for name in run_names(g):
        raised = str(g["run_%s_raises" % name])
        for on_device in (False, True):
            m = _make(g, name)
            if raised:
                with pytest.raises({"IndexError": IndexError, "RuntimeError": RuntimeError}[raised]):
                    _run(m, g, name, on_device)
                continue
            got = _run(m, g, name, on_device)
            want = g["run_%s_values" % name]
            np.testing.assert_allclose(got, want, rtol=rtol_of(name), atol=0, err_msg=name)
            if name.startswith("itk"):
                np.testing.assert_array_equal(got, want, err_msg=name)            # bit-exact: integer counts, float64 formulas
                np.testing.assert_array_equal(got, oracle_run(g, name))
            if name.startswith(("rmse", "wt")):
                assert np.ndim(m.get()) == 0 and not isinstance(m.get(), np.ndarray)
            else:
                assert isinstance(m.get(), np.ndarray) and m.get().shape == want.shape[1:]


def test_rmse_is_exact_at_training_size():
    from brats2019_amd import metrics
    rng = np.random.default_rng(25)
    g = nested(rng, 4, (128, 128, 128))
    p = rng.random(g.shape, dtype=np.float32)
    m = metrics.RMSE()
    m.update([T(g).cuda()], [T(p).cuda()])
    np.testing.assert_allclose(m.get(), rmse_value(p, g), rtol=1e-9)


def test_validate_main_reproduces_the_reference_script(golden, tmp_path, capsys):
    from brats2019_amd import validate
    g = golden("overlap")
    (tmp_path / "data").mkdir()
    (tmp_path / "pred").mkdir()
    for k in range(3):
        name = str(g["v%d_name" % k])
        np.save(str(tmp_path / "data" / (name + ".npy")), g["v%d_label" % k])
        np.save(str(tmp_path / "pred" / (name + ".npy")), g["v%d_pred" % k])
    res, mean = validate.main(["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred")])
    np.testing.assert_array_equal(res, g["validate_results"])
    np.testing.assert_array_equal(mean, g["validate_mean"])
    out = capsys.readouterr().out
    assert "case1 %s" % str(res[1]) in out
    # a volume with a value outside {0,1,2,3,4}, and mismatched shapes, are refused
    bad = g["v0_pred"].copy()
    bad[0, 0, 0] = 5
    np.save(str(tmp_path / "pred" / "case0.npy"), bad)
    with pytest.raises(ValueError, match="case0"):
        validate.main(["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred")])
    np.save(str(tmp_path / "pred" / "case0.npy"), g["v0_pred"][:-1])
    with pytest.raises(ValueError, match="shape"):
        validate.main(["--data_path", str(tmp_path / "data"), "--predictions_path", str(tmp_path / "pred")])


def test_validate_score_of_a_full_case():
    from brats2019_amd import validate
    rng = np.random.default_rng(26)
    lab = rng.choice(np.array([0, 1, 2, 4], np.uint8), size=(240, 240, 155), p=[0.9, 0.03, 0.05, 0.02])
    pred = np.where(rng.random(lab.shape) < 0.1, rng.choice(np.array([0, 1, 2, 4], np.uint8), size=lab.shape), lab)
    names, res, mean = validate.score([("a", lab, pred)])
    want = validate_result(conf_label(pred[None], lab[None])[0])
    np.testing.assert_array_equal(res, want)
    np.testing.assert_array_equal(mean, want[0])


def test_new_entries_capture_into_a_hip_graph():
    """No allocation, host sync or memset inside the calls: label_confusion + the three accumulates capture into one hipGraph, and each
    replay adds the same values again."""
    from brats2019_amd import ops
    rng = np.random.default_rng(27)
    g = T((rng.integers(0, 5, size=(2, 3, 16, 12, 20)) / 4.0).astype(np.float32)).cuda()
    p = T((rng.integers(0, 9, size=(2, 3, 16, 12, 20)) / 8.0).astype(np.float32)).cuda()
    lab = T(rng.integers(0, 5, size=(1, 3001)).astype(np.uint8)).cuda()
    plab = T(rng.integers(0, 5, size=(1, 3001)).astype(np.uint8)).cuda()
    counts = ops.dice_counts(p, g)
    sums = ops.rmse_sums(p, g)
    acc = {k: torch.zeros(n, dtype=torch.float64, device="cuda") for k, n in (("itk", 2), ("wt", 1), ("val", 4), ("d1", 3), ("rmse", 1))}
    out = torch.zeros(4, dtype=torch.float64, device="cuda")

    def step():
        conf, _ = ops.label_confusion(p, g)
        ops.overlap_accumulate(conf, acc["itk"], 2, "itk")
        ops.overlap_accumulate(conf, acc["wt"], 1, "wt")
        cl, inv = ops.label_confusion(plab, lab)
        ops.overlap_accumulate(cl, acc["val"], 4, "validate", out=out)
        ops.dice1d_accumulate(counts, acc["d1"], 3)
        ops.rmse_accumulate(sums, acc["rmse"])
        return conf, cl, inv
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # eager warm-up on the capture stream
        conf_e, cl_e, inv_e = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    once = {k: v.clone() for k, v in acc.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        conf_c, cl_c, inv_c = step()
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(conf_c, conf_e) and torch.equal(cl_c, cl_e) and torch.equal(inv_c, inv_e)
        for key in acc:
            np.testing.assert_allclose(acc[key].cpu().numpy(), (k + 2) * once[key].cpu().numpy(), rtol=1e-14, err_msg=key)
    np.testing.assert_array_equal(conf_e.cpu().numpy(), conf_prob(p.cpu().numpy(), g.cpu().numpy()))


@pytest.mark.parametrize("tiles", [False, True])
def test_trainer_runs_with_the_new_metrics(tmp_path, tiles):
    from brats2019_amd import model as M, loss as L, train as TR, metrics
    seed, dhw = 51, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="ov%d" % tiles, models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    tr.tile_shape, tr.center_shape, tr.border = (64, 64, 64), (32, 32, 32), (16, 16, 16)
    logged = {}

    class Rec:
        def add_scalar(self, name, val, step):
            logged[name] = float(val)
    tr.tb_writer = Rec()
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(O.make_target(2, *dhw, seed=seed + i))]) for i in range(2)]
    tr.train(criterion=[L.Dice_loss_joint(index=0, priority=1), L.BCE_Loss(index=0, bg_weight=1e-2)],
             optimizer=torch.optim.Adam, optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=16000, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=tiles, pretrained_weights=None,
             train_metrics=[metrics.Dice1D(classes=3), metrics.RMSE()],
             val_metrics=[metrics.Dice(), metrics.DiceWT(), metrics.Dice_ITK(classes=4), metrics.Hausdorff_ITK(classes=4)],
             track_metric='Dice', epoches=1, default_val=np.array([0, 0, 0, 0, 0]),
             comparator=lambda x, y: np.min(x) + np.mean(x) > np.min(y) + np.mean(y),
             eval_cpu=False, continue_form_pretraining=False)
    for key in ["train/Dice1D-%d" % i for i in range(3)] + ["train/RMSE-0", "val/Dice_WT-0"] + ["val/Hausdorff_ITK-%d" % i for i in range(3)]:
        assert np.isfinite(logged[key]), key
    # Dice_ITK against the oracle on the model's own output: the nested targets never have labels 1, 2, so those columns are NaN
    # when the prediction has no such label either, and finite (0) when it has
    batch = loader[1]
    out = tr.predict_tiled(batch, tuple(batch[1][0].shape)) if tiles else tr.predict(batch)
    pred = out[0].detach().cpu().numpy()
    conf = conf_prob(pred, batch[1][0].numpy())
    from test_overlap_host import itk_result, wt_result
    want = itk_result(conf, 3).mean(axis=0)
    got = np.array([logged["val/Dice_ITK-%d" % i] for i in range(3)])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12)
    np.testing.assert_allclose(logged["val/Dice_WT-0"], wt_result(conf).mean(), rtol=1e-6)
    assert tr.state.val_metric["Dice_ITK"][0].shape == (3,)
