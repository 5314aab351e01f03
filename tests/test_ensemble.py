"""Ensemble inference on the device (csrc/ensemble.hip): the merge kernels bit for bit against the numpy restatement
(`inference.ensemble_merge_host`, pinned to the notebooks' formula by tests/test_ensemble_host.py), the class rule against `np.argmax`,
the ensemble of one against `predict_case_device`, three networks end to end against the oracle pipeline, the pasted soft labels and the
`test --ensemble` entry point."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

T = torch.from_numpy
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)
SEEDS = (17, 18, 19)


def _outputs(rng, m, shape, few_et):
    """m models x 4 flipped predictions [3, ...].  Uniform noise shifted per channel by +0.02 / -0.02 / 0, so that the means of 4 m values
    crowd around the 0.5 threshold (the closer the more models); few_et: the ET channel stays below 0.02 except at 10 voxels near the
    volume's centre that every copy (un-flipped) puts at 0.9 -- fewer than 33 ET voxels, the rule of test.py:157."""
    shift = np.array([0.02, -0.02, 0.0], np.float32).reshape(3, 1, 1, 1)
    centre = tuple(s // 2 for s in shape[1:])
    models = []
    for _ in range(m):
        copies = []
        for ax in O.TTA_FLIPS:
            u = np.clip(rng.random(shape).astype(np.float32) + shift, 0, 1).astype(np.float32)
            if few_et:
                u[2] *= np.float32(0.02)
                u[2, centre[0], centre[1] - 1:centre[1] + 1, centre[2] - 2:centre[2] + 3] = 0.9
            copies.append(np.ascontiguousarray(np.flip(u, axis=ax)) if ax else u)
        models.append(copies)
    return models


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("shape,lo,size,few_et", [((3, 8, 12, 16), (1, 2, 3), (6, 9, 11), False), ((3, 8, 12, 16), (0, 0, 0), (8, 12, 16), False),
                                                 ((3, 5, 6, 7), (1, 1, 2), (3, 4, 5), False), ((3, 5, 6, 7), (0, 0, 0), (5, 6, 7), True)],
                         ids=["box", "whole", "ragged-box", "ragged-whole-few-et"])
def test_merge_kernels_bit_exact_vs_host_restatement(m, shape, lo, size, few_et):
    """M = 5 is 20 flipped copies: more than the flip word of ru_tta_merge_box can describe.  Both routes are held to the restatement: every
    model through ru_ens_accumulate then ru_ens_finalize, and `ensemble_merge` (last model fused with the finalize)."""
    from brats2019_amd import inference as I, ops
    rng = np.random.default_rng(1000 * m + shape[1])
    outs = _outputs(rng, m, shape, few_et)
    mean_ref, mask_ref, counts_ref = I.ensemble_merge_host(outs, lo, size)
    near = float((np.abs(mean_ref[:2] - 0.5) < 0.05).mean())
    assert near > 0.2, near                                           # a large share of the means sits near the threshold
    assert all(0 < c < mask_ref[0].size for c in counts_ref[:2])
    labels_ref, vols = O.compose_labels(mean_ref)
    assert vols == counts_ref
    if few_et:
        assert 0 < counts_ref[2] <= 32 and not (labels_ref == 4).any()
    probs = [torch.stack([T(o) for o in model]).cuda() for model in outs]
    acc = None
    for p in probs:
        acc = ops.ens_accumulate(p, O.TTA_FLIPS, acc, lo, size)
    routes = {"accumulate + finalize": ops.ens_finalize(acc, m, want_mean=True), "fused last model": I.ensemble_merge(probs, lo, size, want_mean=True)}
    for how, (mask, counts, mean) in routes.items():
        assert tuple(mean.shape) == (3,) + tuple(size), how
        assert np.array_equal(mean.cpu().numpy(), mean_ref), how
        assert np.array_equal(mask.cpu().numpy().astype(bool), mask_ref), how
        assert tuple(counts.cpu().tolist()) == counts_ref, how
        assert np.array_equal(ops.compose_labels(mask, counts, et_min=32).cpu().numpy(), labels_ref), how
    mask, counts, mean = I.ensemble_merge(probs, lo, size)            # without the mean: same mask and counts
    assert mean is None and np.array_equal(mask.cpu().numpy().astype(bool), mask_ref) and tuple(counts.cpu().tolist()) == counts_ref
    if m == 1:                                                        # the ensemble of one is ru_tta_merge_box
        mb, cb, meanb = ops.tta_merge_box(probs[0], O.TTA_FLIPS, lo, size, want_mean=True)
        assert torch.equal(mb, mask) and torch.equal(cb, counts) and np.array_equal(meanb.cpu().numpy(), mean_ref)


@pytest.mark.gpu
def test_finalize_vector_and_scalar_forms_agree_with_numpy():
    """ru_ens_finalize reads 4 voxels per lane when the channel pitch is a multiple of 4, else one: both against numpy's float32 division"""
    from brats2019_amd import ops
    rng = np.random.default_rng(5)
    for shape in ((3, 16, 20, 24), (3, 7, 9, 11), (4, 1, 1, 5)):
        acc = (rng.random(shape) * 3).astype(np.float32)
        mask, counts, mean = ops.ens_finalize(T(acc).cuda(), 3, want_mean=True)
        want = acc / np.float32(3)
        assert np.array_equal(mean.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy().astype(bool), want > 0.5)
        assert counts.cpu().tolist() == (want > 0.5).sum(axis=(1, 2, 3)).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3])
def test_argmax_rule_vs_numpy_with_ties(m):
    from brats2019_amd import inference as I, ops
    rng = np.random.default_rng(9 + m)
    shape = (4, 9, 10, 13)
    preds = [(rng.integers(0, 9, shape) / 8.0).astype(np.float32) for _ in range(m)]      # multiples of 1/8: sums and maxima tie exactly
    mean = sum(preds) / len(preds)
    tied = ((mean == mean.max(axis=0)).sum(axis=0) > 1).mean()
    assert tied > 0.02, tied                                          # ties occur in a sizeable share of voxels
    want = np.argmax(mean, axis=0).astype(np.uint8)
    want[want == 3] = 4
    assert np.array_equal(I.ensemble_class_labels_host(preds), want)
    acc = None
    for p in preds:
        acc = ops.ens_accumulate(T(p).cuda(), acc=acc)                # saved class maps: one copy, no flips, the whole volume
    got = ops.ens_argmax(acc, m)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want) and set(np.unique(want).tolist()) == {0, 1, 2, 4}


def _case():
    rng = np.random.default_rng(17)                                   # the image of test_predict_case_matches_oracle_pipeline
    img = np.zeros((4, 40, 44, 36), np.float32)
    img[:, 4:33, 6:39, 3:30] = rng.random((4, 29, 33, 27)).astype(np.float32) * 3 + 0.05
    return img


def _net(seed):
    from brats2019_amd import model as M
    params = O.make_params(seed, **SMALL)
    net = M.UNet(**SMALL)
    net.load_state_dict({k: T(v) for k, v in params.items()})
    return net.cuda(), params


@pytest.mark.gpu
def test_ensemble_of_one_is_predict_case_device():
    from brats2019_amd import inference as I
    net, _ = _net(17)
    img = T(_case()).cuda()
    full, counts = I.predict_case_device(net, img)
    got, got_counts = I.predict_case_ensemble_device([net], img)
    assert torch.equal(got, full) and torch.equal(got_counts, counts) and got.dtype == torch.uint8
    lab, vols, soft = I.predict_case_ensemble([net], img.cpu().numpy(), want_probs=True)
    assert np.array_equal(lab, full.cpu().numpy()) and vols == tuple(counts.cpu().tolist()) and soft.shape == (3, 40, 44, 36)


@pytest.mark.gpu
def test_models_must_agree():
    from brats2019_amd import inference as I, model as M
    net, _ = _net(17)
    other = M.UNet(**dict(SMALL, number_of_outputs=4)).cuda()
    with pytest.raises(ValueError, match="agree"):
        I.predict_case_ensemble_device([net, other], T(_case()).cuda())
    with pytest.raises(ValueError):
        I.predict_case_ensemble_device([], T(_case()).cuda())


@pytest.mark.gpu
def test_three_models_match_oracle_pipeline_and_soft_labels():
    """Three SMALL networks (seeds 17, 18, 19) on one case.  (a) `ensemble_merge` fed the probabilities each model produced here equals the
    host restatement exactly; (b) the end-to-end labels against the oracle pipeline -- per-model `O.unet_forward` over `O.tta_inputs`,
    `O.tta_merge`, the float32 model sum / 3, `O.postprocess` -- under the bars test_predict_case_matches_oracle_pipeline holds one model to
    (labels differ on < 1e-3 of the voxels, counts within 3); (c) the soft labels: the merge's mean inside the crop box, zero outside.
    The oracle's ensemble labels for these seeds are not degenerate: on the CPU they hold 3590 background, 3109 label-1, 5323 label-2 and
    11274 label-4 voxels of the 23296 in the crop (asserted below: background, 1 and 2 present)."""
    from brats2019_amd import inference as I
    img = _case()
    nets, params = zip(*[_net(s) for s in SEEDS])
    dev = T(img).cuda()
    # (a) the merge alone, from the device's own probabilities
    batch, lo, size, left, _padded = I.prepare_case_device(dev)
    probs = []
    for net in nets:
        net.eval()
        with torch.no_grad():
            probs.append(net([batch])[0])
    mask, counts, mean = I.ensemble_merge(probs, left, size, want_mean=True)
    mean_ref, mask_ref, counts_ref = I.ensemble_merge_host([p.cpu().numpy() for p in probs], left, size)
    assert np.array_equal(mean.cpu().numpy(), mean_ref) and np.array_equal(mask.cpu().numpy().astype(bool), mask_ref)
    assert tuple(counts.cpu().tolist()) == counts_ref
    # (b) end to end against the oracle
    got, vols, soft = I.predict_case_ensemble(list(nets), img, want_probs=True)
    bbox = O.get_bbox(img)
    crop = img[:, bbox[0, 0]:bbox[1, 0], bbox[0, 1]:bbox[1, 1], bbox[0, 2]:bbox[1, 2]]
    padded, pl, pr = O.pad_to_multiple(crop, 16)
    x = O.zscore_nonzero(padded).astype(np.float32)
    per_model = []
    with torch.no_grad():
        for prm in params:
            p = O.to_torch(prm)
            outs = [O.unet_forward(p, T(np.ascontiguousarray(xi))[None], **SMALL)[0].numpy() for xi in O.tta_inputs(x)]
            m = O.tta_merge(outs)
            d, h, w = m.shape[1:]
            per_model.append(m[:, pl[0]:d - pr[0], pl[1]:h - pr[1], pl[2]:w - pr[2]])
    omean = sum(per_model) / len(per_model)
    assert omean.dtype == np.float32
    want, want_vols = O.postprocess(omean)
    assert {0, 1, 2} <= set(np.unique(want).tolist())                 # not degenerate
    dv = max(abs(a - b) for a, b in zip(vols, want_vols))
    full = np.zeros(img.shape[1:], np.uint8)
    full[bbox[0, 0]:bbox[1, 0], bbox[0, 1]:bbox[1, 1], bbox[0, 2]:bbox[1, 2]] = want
    diff = got != full
    print("three-model ensemble: counts %s vs oracle %s, %d / %d labels differ, max |mean - oracle| %.2e"
          % (vols, want_vols, int(diff.sum()), diff.size, float(np.abs(mean_ref - omean).max())))
    assert dv <= 3
    assert diff.mean() < 1e-3, "labels differ on %d voxels" % diff.sum()
    assert set(np.unique(got).tolist()) <= {0, 1, 2, 4}
    # (c) soft labels
    assert soft.shape == (3,) + img.shape[1:] and soft.dtype == np.float32
    box = (slice(None), slice(bbox[0, 0], bbox[1, 0]), slice(bbox[0, 1], bbox[1, 1]), slice(bbox[0, 2], bbox[1, 2]))
    assert np.array_equal(soft[box], mean_ref)
    outside = np.ones(soft.shape, bool)
    outside[box] = False
    assert not soft[outside].any() and (mean_ref > 0).all()
    assert vols == counts_ref


@pytest.mark.gpu
def test_paste_probs():
    from brats2019_amd import ops
    small = T(np.arange(3 * 2 * 3 * 4, dtype=np.float32).reshape(3, 2, 3, 4) + 1).cuda()
    full = ops.paste_probs(small, (5, 6, 7), (1, 2, 3)).cpu().numpy()
    want = np.zeros((3, 5, 6, 7), np.float32)
    want[:, 1:3, 2:5, 3:7] = small.cpu().numpy()
    assert np.array_equal(full, want)
    with pytest.raises(RuntimeError, match="box"):
        ops.paste_probs(small, (5, 6, 7), (4, 2, 3))                  # refused before any launch


@pytest.mark.gpu
def test_entry_point_ensemble(tmp_path):
    """`test --ensemble`: two tiny checkpoints under tmp_path (written as test_entry_point_loads_reference_checkpoint_and_segments has its
    one: the reference-written tests/golden/ckpt/tiny, and a second experiment saved by Trainer._save from other weights).  With
    --ensemble the labels and the soft labels equal the API's; without it the output is `predict_case`'s, as before."""
    import os, shutil, sys
    from brats2019_amd import test as entry, inference as I, model as M, train as TR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "tests", "golden", "ckpt", "tiny"), tmp_path / "tiny")
    cfg = dict(depth=2, encoder_layers=[1, 1], decoder_layers=[1, 1], number_of_channels=[8, 16], number_of_outputs=3)
    net_b = M.UNet(**cfg)
    net_b.load_state_dict({k: T(v) for k, v in O.make_params(41, **cfg).items()})
    TR.Trainer(name="tiny_b", models_root=str(tmp_path), model=net_b, rewrite=True, connect_tb=False)._save(suffix="best_model")
    rng = np.random.default_rng(5)
    img = np.zeros((4, 30, 28, 26), np.float32)
    img[:, 2:27, 3:25, 1:24] = rng.random((4, 25, 22, 23)).astype(np.float32) * 2 + 0.1
    np.save(tmp_path / "case.npy", img)
    common = ["--name", "tiny", "--models_path", str(tmp_path), "--input", str(tmp_path / "case.npy"), "--precision", "f32"]
    saved = {k: sys.modules.get(k) for k in ("model", "train", "loss")}
    try:
        entry.main(common + ["--output", str(tmp_path / "one.npy")])
        entry.main(common + ["--output", str(tmp_path / "two.npy"), "--ensemble", "tiny_b", "--probs_output", str(tmp_path / "soft")])
        nets = []
        for name in ("tiny", "tiny_b"):
            tr = TR.Trainer(name=name, models_root=str(tmp_path), rewrite=False, connect_tb=False)
            tr.load_best()
            net = tr.model.module if hasattr(tr.model, "module") else tr.model
            net.set_precision("f32")
            nets.append(net.cuda())
    finally:
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v
            else:
                sys.modules.pop(k, None)
    one, two, soft = np.load(tmp_path / "one.npy"), np.load(tmp_path / "two.npy"), np.load(tmp_path / "soft" / "case.npy")
    want_one, _ = I.predict_case(nets[0], img)
    want_two, _, want_soft = I.predict_case_ensemble(nets, img, want_probs=True)
    assert np.array_equal(one, want_one)
    assert np.array_equal(two, want_two) and np.array_equal(soft, want_soft)
    assert two.dtype == np.uint8 and soft.dtype == np.float32 and soft.shape == (3,) + img.shape[1:]
    assert (one != two).any()                                         # the second model had a say
