"""Elastic deformation on the device (csrc/elastic.hip: ru_elastic_noise / ru_elastic_field / ru_elastic_warp and `augment_patch` with an
`elastic` entry) against the reference's own outputs (tests/golden/elastic.npz), against the host restatements, and the unchanged default path
against tests/golden/dataloader.npz."""
import random

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_elastic_host import fixture_set, generator, unpack_onehot

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def test_hip_noise_is_a_function_of_seed_field_and_index():
    """identical bits across calls and across shapes (common prefix of linear indices), equal to the host restatement; different seeds and
    fields differ; values in [-1, 1); mean within 6 / sqrt(3 N) of 0 and variance within 6 standard errors of 1/3 for N = 128^3"""
    from brats2019_amd import dataloader as DL
    a = DL.elastic_noise(5, (128, 128, 128))
    assert a.is_cuda and a.dtype == torch.float64 and tuple(a.shape) == (3, 128, 128, 128)
    assert torch.equal(a, DL.elastic_noise(5, (128, 128, 128)))
    b = DL.elastic_noise(5, (16, 40, 24))
    assert torch.equal(b.reshape(3, -1), a.reshape(3, -1)[:, :16 * 40 * 24])
    assert np.array_equal(b.cpu().numpy(), DL.elastic_noise_host(5, (16, 40, 24)))
    big = (1 << 63) + 12345                                          # a seed above 2^63 travels whole
    assert np.array_equal(DL.elastic_noise(big, (5, 6, 7)).cpu().numpy(), DL.elastic_noise_host(big, (5, 6, 7)))
    assert not torch.equal(b, DL.elastic_noise(6, (16, 40, 24)))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    assert float(a.min()) >= -1.0 and float(a.max()) < 1.0
    n = 128 ** 3
    for f in range(3):
        mean, m2 = float(a[f].mean()), float((a[f] * a[f]).mean())
        print("field %d: mean %.3e (bound %.3e), mean square - 1/3 = %.3e (bound %.3e)"
              % (f, mean, 6.0 / np.sqrt(3.0 * n), m2 - 1.0 / 3.0, 6.0 * np.sqrt((1.0 / 5.0 - 1.0 / 9.0) / n)))
        assert abs(mean) <= 6.0 / np.sqrt(3.0 * n)
        assert abs(m2 - 1.0 / 3.0) <= 6.0 * np.sqrt((1.0 / 5.0 - 1.0 / 9.0) / n)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_hip_field_matches_the_reference(golden, k):
    """the reference's own random draws uploaded as noise; absolute 1e-9 voxels (float64 on both sides, see test_elastic_host)"""
    from brats2019_amd import dataloader as DL
    g, gen = golden("elastic"), generator()
    shape, sigma, alpha, seed = fixture_set(g, k)
    s = int(g["sub"])
    noise = T(gen.make_noise(seed, shape)).cuda()
    disp = DL.elastic_field(noise, sigma, alpha)
    assert disp.dtype == torch.float64 and tuple(disp.shape) == (3,) + shape
    got = disp.cpu().numpy()
    err = float(np.abs(got[:, ::s, ::s, ::s] - g["disp%d" % k]).max())
    err_host = float(np.abs(got - DL.elastic_field_host(noise.cpu().numpy(), sigma, alpha)).max())
    print("set %d: max |device field - reference| = %.3e voxels (sub-sampled), vs the host restatement on every voxel %.3e" % (k, err, err_host))
    assert err <= 1e-9 and err_host <= 1e-9


@pytest.mark.parametrize("k", [0, 1, 2])
def test_hip_warp_matches_the_reference(golden, k):
    """noise -> device field -> device warp against elastic_transform's outputs: order 0 exact on every voxel, order 1 to 2e-5 (float32 on the
    device, float64 in the reference -- the bar test_hip_augment_matches_reference holds the same interpolation to)"""
    from brats2019_amd import dataloader as DL
    g, gen = golden("elastic"), generator()
    shape, sigma, alpha, seed = fixture_set(g, k)
    s = int(g["sub"])
    disp = DL.elastic_field(T(gen.make_noise(seed, shape)).cuda(), sigma, alpha)
    image = T(gen.make_image(k, shape)[None].astype(np.float32)).cuda()
    onehot = T(gen.make_onehot(k, shape).astype(np.float32)).cuda()
    data, target = DL.elastic_warp(image, onehot, disp)
    assert data.dtype == torch.float32 and tuple(data.shape) == (1,) + shape and tuple(target.shape) == (4,) + shape
    want = unpack_onehot(g, k, shape)
    wrong = int((target.cpu().numpy() != want).sum())
    err = float(np.abs(data.cpu().numpy()[0, ::s, ::s, ::s] - g["image_out%d" % k]).max())
    print("set %d: order 0 voxels that differ: %d of %d; order 1 max |device - reference| = %.3e" % (k, wrong, want.size, err))
    assert wrong == 0
    assert err <= 2e-5
    d_only, none = DL.elastic_warp(image, None, disp)                # either group alone gives the same numbers
    none2, t_only = DL.elastic_warp(None, onehot, disp)
    assert none is None and none2 is None and torch.equal(d_only, data) and torch.equal(t_only, target)


def _pipeline_case(patch, soft):
    from brats2019_amd import dataloader as DL
    image, label = O.make_dataloader_case(77)
    if soft:
        lab = label.astype(np.int64)
        r = np.random.default_rng(5)
        inside = np.stack([lab > 0, (lab == 1) | (lab == 3), lab == 3]).astype(np.float64)
        soft_map = (inside * (0.6 + 0.4 * r.random(inside.shape)) + (1.0 - inside) * 0.3 * r.random(inside.shape) ** 3).astype(np.float32)
        return DL.DeviceCase(image, label, patch, soft=soft_map)
    return DL.DeviceCase(image, label, patch)


@pytest.mark.parametrize("patch,flips,transpose,soft", [
    ((24, 24, 24), (False, False, False), True, False),              # transposed
    ((24, 24, 24), (True, False, True), False, False),               # flipped
    ((16, 20, 24), (False, True, True), True, False),                # rectangular, flipped and transposed
    ((16, 20, 24), (True, True, False), True, True),                 # soft targets
])
def test_hip_whole_pipeline(patch, flips, transpose, soft):
    """`augment_patch` with an `elastic` entry carrying explicit noise == `ru_augment_patch` without flips, gain or bias, downloaded and pushed
    through the host field and warp plus numpy flips, transpose, gain and bias.  Image 2e-5, targets exact."""
    from brats2019_amd import dataloader as DL
    case = _pipeline_case(patch, soft)
    r = np.random.default_rng(sum(patch) + 2 * int(transpose) + int(soft))
    lo = np.array([r.integers(16, 24), r.integers(15, 23), r.integers(5, 15)])      # the lesion's centre (26, 25, 21) lies in the first 0.7 of every crop
    noise = r.uniform(-1, 1, (3,) + patch)
    p = dict(crop_lo=lo, scale=r.uniform(0.7, 1.3, 3), flips=list(flips), transpose=transpose, gain=r.uniform(0.9, 1.1, 4), bias=r.uniform(-0.2, 0.2, 4),
             elastic=dict(sigma=5.0, alpha=700.0, noise=noise))
    data, target = DL.augment_patch(case, p)
    out_sp = (patch[1], patch[0], patch[2]) if transpose else patch
    assert tuple(data.shape) == (4,) + out_sp and tuple(target.shape) == (3,) + out_sp and data.dtype == target.dtype == torch.float32
    plain = dict(p, flips=[False] * 3, transpose=False, gain=np.ones(4), bias=np.zeros(4))
    del plain["elastic"]
    d0, t0 = DL.augment_patch(case, plain)
    disp = DL.elastic_field_host(noise, 5.0, 700.0)
    assert np.abs(disp).max() > 1.0                                  # a real deformation
    want_d, want_t = DL.elastic_warp_host(d0.cpu().numpy(), t0.cpu().numpy(), disp, flips, transpose, p["gain"], p["bias"])
    err = float(np.abs(data.cpu().numpy() - want_d).max())
    wrong = int((target.cpu().numpy() != want_t).sum())
    print("patch %s flips %s transpose %s soft %s: image max |device - host| = %.3e, target voxels that differ: %d" % (patch, flips, transpose, soft, err, wrong))
    assert err <= 2e-5
    assert wrong == 0
    assert float(t0[2].sum()) > 0 and not np.array_equal(want_t, DL.elastic_warp_host(None, t0.cpu().numpy(), np.zeros_like(disp), flips, transpose)[1])
    # a seed in place of the noise: the device generator's field, same result as handing its noise over
    ps = dict(p, elastic=dict(sigma=5.0, alpha=700.0, seed=1234))
    pn = dict(p, elastic=dict(sigma=5.0, alpha=700.0, noise=DL.elastic_noise(1234, patch)))
    (ds, ts), (dn, tn) = DL.augment_patch(case, ps), DL.augment_patch(case, pn)
    assert torch.equal(ds, dn) and torch.equal(ts, tn) and not torch.equal(ds, data)


def test_default_path_is_unchanged_and_reader_options(golden):
    """`elastic=False` (the default): SimpleReader yields the reference's patches of tests/golden/dataloader.npz.  `elastic=True`: the crop, zoom,
    flips, transpose, gain and bias are the same draws (same global streams), the patch is deformed, and `elastic_seed` makes it repeatable."""
    from brats2019_amd import dataloader as DL
    g = golden("dataloader")
    image, label = O.make_dataloader_case(77)
    patch = tuple(int(v) for v in g["patch"])
    items, states = {}, {}
    for name, kw in (("plain", {}), ("off", dict(elastic=False)), ("on", dict(elastic=True, elastic_seed=3)), ("on2", dict(elastic=True, elastic_seed=3)),
                     ("other", dict(elastic=True, elastic_seed=4))):
        rd = DL.SimpleReader([(image, label)], patch, images_in_epoch=8, patches_from_single_image=100, **kw)
        out = []
        for k in range(2):
            random.seed(int(g["seed%d" % k]))
            np.random.seed(int(g["seed%d" % k]))
            d, t = rd[0]
            out.append((d[0], t[0]))
        items[name], states[name] = out, (random.getstate(), np.random.get_state()[1].copy())
    for k in range(2):
        np.testing.assert_allclose(items["plain"][k][0].cpu().numpy(), g["data%d" % k], rtol=0, atol=2e-5)
        np.testing.assert_allclose(items["plain"][k][1].cpu().numpy(), g["target%d" % k], rtol=0, atol=2e-6)
        assert torch.equal(items["off"][k][0], items["plain"][k][0]) and torch.equal(items["off"][k][1], items["plain"][k][1])
        assert items["on"][k][0].shape == items["plain"][k][0].shape and not torch.equal(items["on"][k][0], items["plain"][k][0])
        assert torch.equal(items["on"][k][0], items["on2"][k][0]) and torch.equal(items["on"][k][1], items["on2"][k][1])
        assert not torch.equal(items["on"][k][0], items["other"][k][0])
        tv = items["on"][k][1]
        assert float(tv.min()) >= 0.0 and float(tv.max()) <= 1.0 + 1e-6 and bool(torch.isfinite(items["on"][k][0]).all())
    for name in states:
        assert states[name][0] == states["plain"][0] and np.array_equal(states[name][1], states["plain"][1]), name


def test_hip_argument_checks_fail_before_any_launch():
    from brats2019_amd import dataloader as DL
    case = _pipeline_case((16, 20, 24), False)
    base = dict(crop_lo=np.array([14, 12, 5]), scale=np.ones(3), flips=[False] * 3, transpose=False, gain=np.ones(4), bias=np.zeros(4))
    noise = torch.zeros((3, 16, 20, 24), dtype=torch.float64, device="cuda")
    for el, what in ((dict(sigma=0.0, alpha=100.0, seed=1), "positive"), (dict(sigma=float("nan"), alpha=100.0, seed=1), "positive"),
                     (dict(sigma=64.2, alpha=100.0, seed=1), "radius"), (dict(sigma=10.0, alpha=100.0, noise=np.zeros((3, 16, 20, 25))), "noise"),
                     (dict(sigma=10.0, alpha=100.0, noise=torch.zeros((3, 20, 16, 24), dtype=torch.float64, device="cuda")), "noise")):
        with pytest.raises(ValueError, match=what):
            DL.augment_patch(case, dict(base, elastic=el))
    with pytest.raises(ValueError, match="radius"):
        DL.elastic_field(noise, 64.2, 100.0)
    with pytest.raises(ValueError, match="float64"):
        DL.elastic_field(noise.float(), 10.0, 100.0)
    with pytest.raises(ValueError, match="order"):
        DL.elastic_warp(torch.zeros((1, 16, 20, 24), device="cuda"), None, noise, order=(3, 0))
    with pytest.raises(ValueError, match="match"):
        DL.elastic_warp(torch.zeros((1, 16, 20, 25), device="cuda"), None, noise)
    d, t = DL.augment_patch(case, dict(base, elastic=dict(sigma=64.1, alpha=100.0, noise=noise)))      # radius 256 is allowed; zero noise: no deformation
    d0, t0 = DL.augment_patch(case, base)
    assert torch.equal(d, d0) and torch.equal(t, t0)                 # order 0 picks the voxel itself; order 1 with weights (1, 0) is exact


def test_hip_graph_capture():
    """noise, field and warp only enqueue: captured once into a hipGraph and replayed once, they give the eager result bit for bit"""
    from brats2019_amd import dataloader as DL
    patch = (24, 20, 32)
    r = np.random.default_rng(8)
    image = T(r.standard_normal((4,) + patch).astype(np.float32)).cuda()
    target = T((r.random((3,) + patch) < 0.3).astype(np.float32)).cuda()
    flips, transpose, gain, bias = (True, False, True), True, r.uniform(0.9, 1.1, 4), r.uniform(-0.2, 0.2, 4)

    def run():
        noise = DL.elastic_noise(77, patch)
        disp = DL.elastic_field(noise, 6.0, 900.0)
        return (noise, disp) + DL.elastic_warp(image, target, disp, flips, transpose, gain, bias)

    eager = [t.clone() for t in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                        # warm-up on the capture stream (allocator, workspace)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, eager):
        assert torch.equal(got, want)
    assert float(outs[1].abs().max()) > 1.0
