"""Hausdorff_ITK / Hausdorff_ITKWT (metrics.py:188-271), the second validation metric of main.py:149-151: the device distance transform
(ru_hausdorff_sq) against a local scipy oracle, exactly, as integers; the device bookkeeping (ru_hausdorff_accumulate) and the metric
classes against tests/golden/hausdorff.npz, which the reference's own classes produced; and Trainer.train with main.py's val_metrics.

Oracle: directed(A, B) = max over voxels of A of the Euclidean distance to the nearest voxel of B at unit spacing, taken from
scipy.ndimage.distance_transform_edt's nearest-site indices so that squared distances stay exact integers."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle import resunet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "resunet_hip.h")
T = torch.from_numpy


# ---------------------------------------------------------------------- oracle
def directed_sq(a, b):
    """max over a of the squared distance to the nearest voxel of b (exact integer); both masks non-empty."""
    idx = ndimage.distance_transform_edt(~b, return_distances=False, return_indices=True)
    grid = np.indices(a.shape)
    d2 = ((idx - grid).astype(np.int64) ** 2).sum(axis=0)
    return int(d2[a].max())


def oracle_sq(pm, gm):
    """(max over P of d^2 to G, max over G of d^2 to P, #P, #G); the maxima are 0 when either mask is empty."""
    cp, cg = int(pm.sum()), int(gm.sum())
    if cp == 0 or cg == 0:
        return 0, 0, cp, cg
    return directed_sq(pm, gm), directed_sq(gm, pm), cp, cg


def oracle_batch_sq(pred, gr, mode):
    """[N, K, 4] int64 for numpy inputs [N, C, D, H, W]: mode 0 per channel > 0.5, mode 1 argmax over C > 0."""
    if mode == 0:
        pm, gm = pred > 0.5, gr > 0.5
    else:
        pm, gm = (np.argmax(pred, axis=1) > 0)[:, None], (np.argmax(gr, axis=1) > 0)[:, None]
    return np.array([[oracle_sq(pm[n, k], gm[n, k]) for k in range(pm.shape[1])] for n in range(pm.shape[0])], dtype=np.int64)


def oracle_result(sq, nacc, mode):
    """The reference's result array (metrics.py:208-228 / 248-263) from the squared maxima and counts, its loop as written."""
    def hd(q):
        return 1e6 if q[2] == 0 or q[3] == 0 else float(np.sqrt(float(max(q[0], q[1]))))
    if mode == 1:
        return np.array([hd(sq[n, 0]) for n in range(sq.shape[0])])
    res = np.zeros((sq.shape[0], nacc))
    for n in range(sq.shape[0]):
        for i in range(nacc):
            if sq[n, i, 2] == 0 and sq[n, i, 3] == 0:
                res[n, i - 1] = 0                              # the reference's index slip, kept
                continue
            res[n, i] = hd(sq[n, i])
    return res


def brute_directed_sq(a, b):
    pa, pb = np.argwhere(a), np.argwhere(b)
    return int((((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)).min(axis=1).max())


def blob_masks(rng, shape, count, nblobs=3):
    zz, yy, xx = np.ogrid[tuple(slice(0, s) for s in shape)]
    out = np.zeros((count,) + tuple(shape), dtype=bool)
    for m in out:
        for _ in range(nblobs):
            c = [rng.uniform(0, s) for s in shape]
            r = rng.uniform(1.0, max(1.5, 0.3 * min(shape)))                     # (1.5: shapes with an axis of 1)
            m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return out


def soft(rng, mask):
    return np.where(mask, 0.5 + rng.integers(1, 9, size=mask.shape) / 16.0, rng.integers(0, 9, size=mask.shape) / 16.0).astype(np.float32)


# ---------------------------------------------------------------------- CPU
def test_oracle_matches_brute_force_pairwise_distances():
    rng = np.random.default_rng(3)
    for shape in [(1, 1, 7), (3, 4, 5), (6, 2, 5), (5, 6, 7)]:
        for dens in (0.05, 0.3, 0.8):
            a, b = rng.random(shape) < dens, rng.random(shape) < dens
            a.flat[rng.integers(a.size)] = True
            b.flat[rng.integers(b.size)] = True
            assert directed_sq(a, b) == brute_directed_sq(a, b)
            assert directed_sq(b, a) == brute_directed_sq(b, a)
            hd = ndimage.distance_transform_edt(~b)[a].max()
            assert hd == np.sqrt(float(directed_sq(a, b)))                  # the float form the fixture's filter used


def _golden_runs(g):
    names = sorted({k.split("_")[1] for k in g if k.startswith("run_")})
    assert names == ["itk2", "itk3", "itk4", "wt"]
    return names


def test_oracle_and_semantics_reproduce_the_reference_fixture(golden):
    g = golden("hausdorff")
    for name in _golden_runs(g):
        order, want = g["run_%s_order" % name], g["run_%s_values" % name]
        mode = 1 if name == "wt" else 0
        nacc = 1 if mode else int(g["run_%s_classes" % name]) - 1
        vals = []
        for _ in range(2):                                                    # the fixture resets between two passes
            acc, samples = 0.0, 0
            for b in order:
                sq = oracle_batch_sq(g["b%d_pred" % b], g["b%d_gr" % b], mode)
                acc = acc + oracle_result(sq, nacc, mode).mean(axis=0)
                samples += 1
                vals.append(np.atleast_1d(acc / samples))
        np.testing.assert_allclose(np.stack(vals), want, rtol=1e-12, atol=0, err_msg=name)
    # the fixture pins the cases it claims
    assert g["run_itk3_values"][0][0] == 0.0                                  # both-empty channel 1 zeroes channel 0 (i-1 slip at i = 1)
    corners = oracle_batch_sq(g["b2_pred"], g["b2_gr"], 0)
    assert corners[0, 0, 0] == 8 ** 2 + 6 ** 2 + 4 ** 2 and corners[0, 2, 2] == corners[0, 2, 3] == 0


def test_metric_classes_have_the_reference_surface():
    from brats2019_amd import metrics
    for cls, params in [(metrics.Hausdorff_ITK, [("name", "Hausdorff_ITK"), ("input_index", 0), ("target_index", 0), ("classes", 5)]),
                        (metrics.Hausdorff_ITKWT, [("name", "Hausdorff_ITKWT"), ("input_index", 0), ("target_index", 0)])]:
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == params
        assert issubclass(cls, metrics.Metrics)
        m = cls()
        assert m.name == params[0][1] and m.accumulator == 0.0 and m.samples == 0.0
    m = metrics.Hausdorff_ITK(name="Hausdorff_ITK", input_index=0, target_index=0, classes=4)       # main.py:150, verbatim
    assert m.classes == 4


def test_header_and_ctypes_table_declare_the_hausdorff_entries():
    from brats2019_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ru_hausdorff_workspace_bytes", "ru_hausdorff_sq", "ru_hausdorff_accumulate"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name


# ---------------------------------------------------------------------- GPU
def _device_sq(pred, gr, mode):
    from brats2019_amd import ops
    out = ops.hausdorff_sq(T(np.ascontiguousarray(pred)).cuda(), T(np.ascontiguousarray(gr)).cuda(), mode=mode)
    assert out.is_cuda and out.dtype == torch.int64
    return out.cpu().numpy()


def _check_exact(pred, gr, mode, what):
    got, want = _device_sq(pred, gr, mode), oracle_batch_sq(pred, gr, mode)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got[..., 2:], want[..., 2:], err_msg="%s: counts" % what)
    both = (want[..., 2] > 0) & (want[..., 3] > 0)                            # a directed maximum is defined only for two non-empty masks
    np.testing.assert_array_equal(got[..., :2][both], want[..., :2][both], err_msg="%s: squared maxima" % what)


@pytest.mark.gpu
def test_hausdorff_sq_is_exact_on_blobs_and_ragged_shapes():
    rng = np.random.default_rng(11)
    wide = [(5, 37, 129), (1, 1, 65), (3, 4, 500), (64, 1, 300)]              # rows of more than one 64-voxel word, D = 1, H = 1
    for n, c, shape in [(2, 3, (128, 128, 128)), (2, 2, (5, 6, 7)), (1, 3, (37, 41, 29))] + [(1, 2, shape) for shape in wide]:
        pm, gm = blob_masks(rng, shape, n * c), blob_masks(rng, shape, n * c)
        pred = soft(rng, pm).reshape((n, c) + shape)
        gr = soft(rng, gm).reshape((n, c) + shape)
        _check_exact(pred, gr, 0, "blobs %s" % (shape,))
        _check_exact(pred, gr, 1, "blobs %s WT" % (shape,))
    # sparse speckle: long gaps in every pass
    for shape in [(37, 41, 29), (5, 6, 7)] + wide:
        pred = (rng.random((2, 2) + shape) < 0.004).astype(np.float32)
        gr = (rng.random((2, 2) + shape) < 0.004).astype(np.float32)
        pred[:, :, 0, 0, 0] = gr[:, :, -1, -1, -1] = 1.0
        _check_exact(pred, gr, 0, "speckle %s" % (shape,))


@pytest.mark.gpu
def test_hausdorff_sq_is_exact_on_lines_of_300_along_each_axis():
    rng = np.random.default_rng(12)
    for axis in range(3):
        shape = [3, 2, 5]
        shape[axis] = 300
        pred = np.zeros((1, 2) + tuple(shape), dtype=np.float32)
        gr = np.zeros_like(pred)
        line = [1, 1, 2]
        # channel 0: a single voxel at each end of the line
        sl = [0, 0] + line
        sl[2 + axis] = 0
        pred[tuple(sl)] = 1.0
        sl[2 + axis] = 299
        gr[tuple(sl)] = 1.0
        # channel 1: sparse sites along the whole line
        sl = [0, 1] + line
        sl[2 + axis] = slice(None)
        pred[tuple(sl)] = (rng.random(300) < 0.03).astype(np.float32)
        gr[tuple(sl)] = (rng.random(300) < 0.03).astype(np.float32)
        pred[0, 1, 0, 0, 0] = gr[0, 1, -1, -1, -1] = 1.0
        got = _device_sq(pred, gr, 0)
        assert got[0, 0, 0] == got[0, 0, 1] == 299 ** 2
        _check_exact(pred, gr, 0, "line along axis %d" % axis)


@pytest.mark.gpu
def test_hausdorff_sq_is_exact_on_a_full_brats_case():
    rng = np.random.default_rng(13)
    shape = (240, 240, 155)
    pm, gm = blob_masks(rng, shape, 1, nblobs=4), blob_masks(rng, shape, 1, nblobs=4)
    _check_exact(soft(rng, pm)[None], soft(rng, gm)[None], 0, "240 x 240 x 155")


@pytest.mark.gpu
def test_hausdorff_sq_special_masks():
    shape = (9, 7, 5)
    pred = np.zeros((1, 5) + shape, dtype=np.float32)
    gr = np.zeros_like(pred)
    pred[0, 0, 0, 0, 0] = gr[0, 0, 8, 6, 4] = 1.0                   # single voxels in opposite corners
    pred[0, 1] = gr[0, 1] = 1.0                                      # all foreground on both sides
    pred[0, 2] = 1.0                                                 # all foreground against a single voxel
    gr[0, 2, 4, 3, 2] = 1.0
    pred[0, 3, 2, 2, 2] = 1.0                                        # one empty
    got = _device_sq(pred, gr, 0)                                    # channel 4 empty on both sides
    assert got[0, 0].tolist() == [116, 116, 1, 1]
    assert got[0, 1].tolist() == [0, 0, 315, 315]
    assert got[0, 2].tolist() == [16 + 9 + 4, 0, 315, 1]
    assert got[0, 3, 2:].tolist() == [1, 0] and got[0, 4, 2:].tolist() == [0, 0]
    _check_exact(pred, gr, 0, "special")
    _check_exact(pred, gr, 1, "special WT")


@pytest.mark.gpu
def test_hausdorff_sq_refuses_extents_above_512():
    from brats2019_amd import ops
    x = torch.zeros((1, 1, 2, 3, 513), device="cuda")
    with pytest.raises(RuntimeError, match="extents"):
        ops.hausdorff_sq(x, x)
    y = torch.zeros((1, 1, 513, 2, 3), device="cuda")
    with pytest.raises(RuntimeError, match="extents"):
        ops.hausdorff_sq(y, y, mode=1)
    # nothing was launched: the device still works
    p = torch.zeros((1, 1, 4, 4, 4), device="cuda")
    p[0, 0, 0, 0, 0] = 1.0
    q = torch.zeros_like(p)
    q[0, 0, 3, 3, 3] = 1.0
    assert ops.hausdorff_sq(p, q).cpu().tolist() == [[[27, 27, 1, 1]]]


def _run_metric(m, g, name, on_device):
    order = g["run_%s_order" % name]
    vals = []
    for _ in range(2):
        m.reset()
        for b in order:
            p, gr = T(g["b%d_pred" % b]), T(g["b%d_gr" % b])
            if on_device:
                p, gr = p.cuda(), gr.cuda()
            m.update([gr], [p])
            assert isinstance(m.accumulator, torch.Tensor) and m.accumulator.is_cuda and m.accumulator.dtype == torch.float64
            vals.append(np.atleast_1d(np.asarray(m.get(), dtype=np.float64)))
    return np.stack(vals)


@pytest.mark.gpu
def test_metric_classes_match_the_reference_fixture(golden):
    from brats2019_amd import metrics
    g = golden("hausdorff")
    for name in _golden_runs(g):
        for on_device in (False, True):
            if name == "wt":
                m = metrics.Hausdorff_ITKWT()
            else:
                m = metrics.Hausdorff_ITK(name=str(g["run_%s_name" % name]), classes=int(g["run_%s_classes" % name]))
            got = _run_metric(m, g, name, on_device)
            np.testing.assert_allclose(got, g["run_%s_values" % name], rtol=1e-12, atol=0, err_msg=name)
            if name == "wt":
                assert np.ndim(m.get()) == 0                                  # a scalar, like the reference's result.mean()
            else:
                assert m.get().shape == (int(g["run_%s_classes" % name]) - 1,)
    m = metrics.Hausdorff_ITK(classes=5)                                      # classes - 1 > C: the reference's indexing raises
    with pytest.raises(IndexError):
        m.update([T(g["b0_gr"])], [T(g["b0_pred"])])


@pytest.mark.parametrize("tiles", [False, True])
@pytest.mark.gpu
def test_trainer_runs_with_the_validation_metrics_of_main(tmp_path, tiles):
    from brats2019_amd import model as M, loss as L, train as TR, metrics
    seed, dhw = 41, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="hd%d" % tiles, models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
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
             train_metrics=[metrics.Dice(name='Dice', input_index=0, target_index=0, classes=4), ],
             val_metrics=[metrics.Dice(name='Dice', input_index=0, target_index=0, classes=4),
                          metrics.Hausdorff_ITK(name='Hausdorff_ITK', input_index=0, target_index=0, classes=4),
                          ],
             track_metric='Dice', epoches=1, default_val=np.array([0, 0, 0, 0, 0]),
             comparator=lambda x, y: np.min(x) + np.mean(x) > np.min(y) + np.mean(y),
             eval_cpu=False, continue_form_pretraining=False)
    got = np.array([logged["val/Hausdorff_ITK-%d" % i] for i in range(3)])
    assert tr.state.val_metric["Hausdorff_ITK"][0].shape == (3,)
    batch = loader[1]
    out = tr.predict_tiled(batch, tuple(batch[1][0].shape)) if tiles else tr.predict(batch)
    pred = out[0].detach().cpu().numpy()
    sq = oracle_batch_sq(pred, batch[1][0].numpy(), 0)
    want = oracle_result(sq, 3, 0).mean(axis=0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_hausdorff_entries_capture_into_a_hip_graph():
    """The convention of include/resunet_hip.h: no allocation and no synchronisation inside the calls, so `hausdorff_sq` +
    `hausdorff_accumulate` capture into one hipGraph; each replay adds the same batch mean again."""
    from brats2019_amd import ops
    rng = np.random.default_rng(14)
    shape = (16, 12, 20)
    pred = T(soft(rng, blob_masks(rng, shape, 3)).reshape((1, 3) + shape)).cuda()
    gr = T(soft(rng, blob_masks(rng, shape, 3)).reshape((1, 3) + shape)).cuda()
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # eager warm-up on the capture stream
        sq_e = ops.hausdorff_sq(pred, gr)
        ops.hausdorff_accumulate(sq_e, acc, 3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    once = acc.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sq_c = ops.hausdorff_sq(pred, gr)
        ops.hausdorff_accumulate(sq_c, acc, 3)
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sq_c, sq_e)
        np.testing.assert_allclose(acc.cpu().numpy(), (k + 2) * once.cpu().numpy(), rtol=1e-15)
