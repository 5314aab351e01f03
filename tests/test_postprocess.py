"""Region-wise post-processing on the device (csrc/postprocess.hip, ru_postprocess_regions) against the numpy / scipy restatement
(inference.postprocess_regions_host, pinned to hand-built cases by tests/test_postprocess_host.py): masks or labels, counts and statistics
byte for byte -- there is no tolerance in this feature -- at the smallest shapes at which each pass can go wrong."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_surface_host import blob_masks
from test_postprocess_host import shell

T = torch.from_numpy
SMALL = dict(depth=3, encoder_layers=[1, 1, 2], decoder_layers=[1, 1, 1], number_of_channels=[8, 16, 32], number_of_outputs=3)


def _check(x, probs=None, what="", **kw):
    """device == host for (output, counts, statistics); the input is not written; returns the host's three"""
    from brats2019_amd import inference as I, ops
    x = np.ascontiguousarray(x)
    dev = T(x.copy()).cuda()
    got = ops.postprocess_regions(dev, probs=None if probs is None else T(probs).cuda(), want_stats=True, **kw)
    want = I.postprocess_regions_host(x, probs=probs, want_stats=True, **kw)
    assert got[0].is_cuda and got[0].dtype == torch.uint8 and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
    out, counts, stats = (t.cpu().numpy() for t in got)
    print(what, kw, "counts", counts.tolist(), "stats", stats.tolist())
    assert out.shape == want[0].shape and stats.shape == want[2].shape, what
    np.testing.assert_array_equal(stats, want[2], err_msg="%s %s: statistics" % (what, kw))
    np.testing.assert_array_equal(counts, want[1], err_msg="%s %s: counts" % (what, kw))
    assert out.tobytes() == want[0].tobytes(), "%s %s: %d voxels differ" % (what, kw, int((out != want[0]).sum()))
    assert np.array_equal(dev.cpu().numpy(), x), "%s: the input was written" % what
    short = ops.postprocess_regions(dev, probs=None if probs is None else T(probs).cuda(), **kw)
    assert len(short) == 2 and torch.equal(short[0], got[0]) and torch.equal(short[1], got[1])
    return want


def _blobs(rng, shape):
    """three blob masks with specks, punched holes and every face and corner of the grid touched"""
    m = blob_masks(rng, shape, 3)
    m &= rng.random(m.shape) > 0.04                                     # cavities, tunnels and ragged borders
    m |= rng.random(m.shape) < 0.01                                     # specks
    m[:, 0, 0, 0] = m[:, -1, -1, -1] = m[:, 0, -1, 0] = m[:, -1, 0, -1] = True
    return m.astype(np.uint8)


ALONE = [dict(), dict(min_volume=(5, 3, 2)), dict(keep_largest=True), dict(keep_largest=(False, True, False)), dict(fill_holes=True),
         dict(fill_holes=(False, False, True)), dict(nest=True)]
TOGETHER = dict(min_volume=(6, 4, 2), keep_largest=(False, False, True), fill_holes=(True, True, False), nest=True)
CONFIDENCE = (0.5, 0.45, 0.55)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 10, 37), (5, 7, 70), (1, 12, 40)])
def test_odd_widths(shape):
    rng = np.random.default_rng(41)
    m = _blobs(rng, shape)
    probs = rng.random(m.shape, dtype=np.float32)
    changed = 0
    for kw in ALONE + [TOGETHER]:
        want = _check(m, what="blobs %s" % (shape,), **kw)
        changed += int(want[2][:, 1:].sum())
        _check(m, probs=probs, what="blobs %s with probabilities" % (shape,), **kw)          # probabilities alone change nothing
    assert changed > 0
    for kw in [dict(min_confidence=CONFIDENCE), dict(min_confidence=(0.0, 0.0, 0.52)), dict(min_confidence=CONFIDENCE, **TOGETHER)]:
        want = _check(m, probs=probs, what="blobs %s" % (shape,), **kw)
    assert want[2][:, 2].sum() > 0
    lab = rng.choice(np.array([0, 1, 2, 3, 4, 9], np.uint8), size=shape, p=[0.55, 0.1, 0.2, 0.05, 0.08, 0.02])
    for kw in ALONE + [TOGETHER]:
        want = _check(lab, what="labels %s" % (shape,), **kw)
    assert want[2].shape == (3, 6) and want[2][0, 5] == (lab == 9).sum() > 0


def _snake(shape):
    """one component folding back and forth through the whole grid (tests/test_lesion.py)"""
    d, h, w = shape
    s = np.zeros(shape, bool)
    for z in range(0, d, 2):
        for y in range(0, h, 2):
            s[z, y, :] = True
            s[z, min(y + 1, h - 1), 0 if (y // 2) % 2 else w - 1] = True
        s[min(z + 1, d - 1), h - 2 if (z // 2) % 2 == 0 else 0, w - 1 if (z // 2) % 2 == 0 else 0] = True
    return s


@pytest.mark.gpu
def test_several_workgroups():
    shape = (40, 48, 70)                                                # 134 400 voxels: 132 workgroups per region
    rng = np.random.default_rng(42)
    snake = _snake(shape)
    shells = shell(shape, (2, 3, 4), (38, 45, 66)) | shell(shape, (10, 12, 14), (30, 36, 56))      # a shell in the cavity of a shell
    shells[20, 24, 30] = True                                           # and a speck in the innermost cavity
    noise = rng.random(shape) < 0.3
    m = np.stack([shells, snake, noise]).astype(np.uint8)
    probs = rng.random(m.shape, dtype=np.float32)
    want = _check(m, what="several workgroups")
    assert want[2][:, 0].tolist()[:2] == [3, 1]
    want = _check(m, what="several workgroups", fill_holes=True)
    assert want[1][0] == 36 * 42 * 62 and want[2][0, 4] == 36 * 42 * 62 - shells.sum()
    assert want[2][1, 4] == 0 and want[2][2, 4] > 0                     # the snake's gaps all reach a face
    want = _check(m, what="several workgroups", min_volume=(2000, 0, 3), fill_holes=(True, False, True), keep_largest=(False, True, True), nest=True)
    assert want[2][0, 1] == 1                                           # the speck goes, then its cavity is filled
    want = _check(m, probs=probs, what="several workgroups", min_confidence=(0.5, 0.5, 0.5), keep_largest=(True, False, False), fill_holes=True)
    # the outer shell keeps its cavity open to the faces
    open_shell = shells.copy()
    open_shell[2, 20, 30] = False
    want = _check(np.stack([open_shell, snake & noise, ~snake]).astype(np.uint8), what="open shell", fill_holes=True, min_volume=(0, 2, 0))
    assert want[2][0, 4] == 18 * 22 * 40 - 1                            # only the inner shell's cavity (less its speck) is enclosed now
    lab = np.zeros(shape, np.uint8)
    lab[shells] = 2
    lab[snake & ~shells & (rng.random(shape) < 0.5)] = 1
    lab[noise & (rng.random(shape) < 0.05)] = 4
    _check(lab, what="labels, several workgroups", min_volume=(10, 5, 2), fill_holes=(True, False, False), nest=True)


@pytest.mark.gpu
def test_degenerate_masks():
    shape = (5, 7, 70)
    full, empty, last = np.ones(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    last[-1, -1, -1] = True
    m = np.stack([full, empty, last]).astype(np.uint8)
    probs = np.full(m.shape, 0.5, np.float32)
    for kw in ALONE + [TOGETHER, dict(min_volume=1), dict(min_volume=2), dict(min_volume=5 * 7 * 70 + 1)]:
        _check(m, what="degenerate", **kw)
    want = _check(m, probs=probs, what="degenerate", min_confidence=0.5)
    assert want[1].tolist() == [5 * 7 * 70, 0, 1]
    want = _check(m, probs=probs, what="degenerate", min_confidence=(0.5 + 2.0 ** -16, 0.5, 0.5), keep_largest=True)
    assert want[1].tolist() == [0, 0, 1]
    _check(np.stack([last, full, empty]).astype(np.uint8), what="degenerate, permuted", fill_holes=True, nest=True, keep_largest=True)
    _check(np.full(shape, 4, np.uint8), what="labels, all ET", keep_largest=True, fill_holes=True)
    _check(np.zeros(shape, np.uint8), what="labels, empty", keep_largest=True, fill_holes=True)


@pytest.mark.gpu
def test_fixed_point_confidence():
    rng = np.random.default_rng(43)
    shape = (9, 10, 37)
    m = _blobs(rng, shape)
    levels = np.array([0.0, 2.0 ** -16, 0.5, 1.0 - 2.0 ** -16, 1.0], np.float32)
    probs = rng.choice(levels, size=m.shape)
    for c in (0.5, 2.0 ** -16, 1.0, (0.25, 0.5, 0.75)):
        _check(m, probs=probs, what="levels", min_confidence=c)
    wild = (rng.standard_normal(m.shape) * 0.8 + 0.5).astype(np.float32)                   # a third of the values outside [0, 1]: clamped
    assert (wild < 0).any() and (wild > 1).any()
    for c in (0.5, (0.3, 0.6, 0.45)):
        _check(m, probs=wild, what="random float32", min_confidence=c, min_volume=2)
    # the equality threshold: conf == T * vol stays, one q less goes -- in components spread over several waves
    a = np.zeros((3,) + shape, np.uint8)
    a[:, 1:4, 1:9, 2:30] = 1                                            # 672 voxels
    a[:, 6:8, 1:9, 2:30] = 1                                            # 448 voxels
    p = np.full(a.shape, np.float32(0.7), np.float32)
    p[0, 6, 3, 17] = np.float32(45874 / 65536.0)                        # region 0: the second component is one q short
    p[1, 2, 5, 29] = np.float32(0.7) + np.float32(2.0 ** -16)           # region 1: one q above changes nothing
    p[2, 1:4, 1:9, 2:30] = np.float32(0.7) - np.float32(2.0 ** -16)     # region 2: every voxel of the first is one q short
    want = _check(a, probs=p, what="equality", min_confidence=45875 / 65536.0)
    assert want[1].tolist() == [672, 1120, 448] and want[2][:, 2].tolist() == [1, 0, 1]


@pytest.mark.gpu
def test_two_calls_give_identical_bytes_and_bad_arguments_raise():
    from brats2019_amd import ops
    rng = np.random.default_rng(44)
    shape = (24, 24, 40)
    m = T(np.stack([_blobs(rng, shape)[0], rng.random(shape) < 0.03, rng.random(shape) < 0.4]).astype(np.uint8)).cuda()
    probs = T(rng.random((3,) + shape, dtype=np.float32)).cuda()
    before = m.clone()
    kw = dict(probs=probs, min_volume=(3, 2, 2), min_confidence=0.4, keep_largest=(True, False, False), fill_holes=True, nest=True, want_stats=True)
    a, b = ops.postprocess_regions(m, **kw), ops.postprocess_regions(m, **kw)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(m, before)
    assert a[2][:, 0].min().item() > 0 and a[2][1, 1].item() > 100
    with pytest.raises(ValueError):
        ops.postprocess_regions(m, min_confidence=0.5)
    with pytest.raises(ValueError):
        ops.postprocess_regions(m[0], probs=probs)
    with pytest.raises(ValueError):
        ops.postprocess_regions(m.float())
    again = ops.postprocess_regions(m, **kw)
    assert all(torch.equal(u, v) for u, v in zip(a, again))


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


@pytest.mark.gpu
def test_pipeline_with_a_postprocess():
    from brats2019_amd import inference as I, ops
    net, img = _net(17), T(_case()).cuda()
    post = I.PostProcess(min_volume=(8, 4, 2), fill_holes=True, nest=True)
    full, counts = I.predict_case_device(net, img, postprocess=post)
    # the merge as the pipeline runs it, then the host restatement, the reference's compose, rejection and paste
    batch, lo, size, left, _ = I.prepare_case_device(img)
    with torch.no_grad():
        probs = net([batch])[0]
    mask, raw_counts, mean = ops.tta_merge_box(probs, I.TTA_FLIPS, left, size, want_mean=True)
    m, c, stats = I.postprocess_regions_host(mask.cpu().numpy(), probs=mean.cpu().numpy(), want_stats=True, **post.regions())
    print("raw counts", raw_counts.tolist(), "post-processed", c.tolist(), "stats", stats.tolist())
    labels = I.postprocess_labels(I.compose_masks_host(m, c), 0.1)
    want = np.zeros(img.shape[1:], np.uint8)
    want[tuple(slice(int(l), int(l) + int(s)) for l, s in zip(lo, size))] = labels
    assert counts.cpu().tolist() == c.tolist()
    assert full.dtype == torch.uint8 and full.cpu().numpy().tobytes() == want.tobytes()
    # with a confidence rule the mean comes along; the numpy entry gives the same
    post = I.PostProcess(min_volume=(8, 4, 2), min_confidence=(0.0, 0.55, 0.6), keep_largest=(True, False, False), reject_ratio=None)
    full, counts = I.predict_case_device(net, img, postprocess=post)
    m, c = I.postprocess_regions_host(mask.cpu().numpy(), probs=mean.cpu().numpy(), **post.regions())
    want[tuple(slice(int(l), int(l) + int(s)) for l, s in zip(lo, size))] = I.compose_masks_host(m, c)
    assert counts.cpu().tolist() == c.tolist() and full.cpu().numpy().tobytes() == want.tobytes()
    lab, vols = I.predict_case(net, img.cpu().numpy(), postprocess=post)
    assert lab.tobytes() == want.tobytes() and vols == tuple(c.tolist())
    with pytest.raises(ValueError):
        I.predict_case_device(net, img, postprocess=dict(min_volume=3))


@pytest.mark.gpu
def test_pipeline_with_the_default_postprocess_is_the_pipeline():
    from brats2019_amd import inference as I
    nets, img = [_net(17), _net(18)], T(_case()).cuda()
    plain, post = I.predict_case_device(nets[0], img), I.predict_case_device(nets[0], img, postprocess=I.PostProcess())
    assert all(torch.equal(a, b) for a, b in zip(plain, post)) and len(post) == 2
    plain = I.predict_case_ensemble_device(nets, img, want_probs=True, uncertainty="std")
    post = I.predict_case_ensemble_device(nets, img, want_probs=True, uncertainty="std", postprocess=I.PostProcess())
    assert len(post) == 4 and all(torch.equal(a, b) for a, b in zip(plain, post))
    # soft labels and uncertainty maps are those of the merge whatever the post-processing
    hard = I.predict_case_ensemble_device(nets, img, want_probs=True, uncertainty="std",
                                          postprocess=I.PostProcess(min_volume=50, min_confidence=0.6, keep_largest=True, nest=True))
    assert torch.equal(hard[2], plain[2]) and torch.equal(hard[3], plain[3])
