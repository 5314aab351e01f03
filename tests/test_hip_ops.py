"""GPU parity, op level: every entry point of libresunet_hip.so is called through the C-ABI (brats2019_amd.ops
-> ctypes) and compared (a) with the reference's own outputs in tests/golden/ops.npz and (b) with the CPU
oracle on further seeded shapes (ragged extents, channel counts of every network level).

Tolerances (float32 path, exact-f32 MFMA; only the summation ORDER differs from the CPU):
forward tensors  |d| <= 1e-5 + 1e-5*|ref|   (K <= 3456 products per output)
reductions over >= 1e3 voxels (weight grads, GN parameter grads) relative 2e-4 of the tensor's max.

The shapes here are chosen for channel pairs.  The launchers' switches -- every conv3_f32_kernel instantiation, split-K, the persistent walks of the weight
gradients, the routes of conv1_launch, the reduction's forms -- are reached, asserted and held to float64 at these same bars by tests/test_ncdhw_convs.py."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def dev(a):
    return T(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def close(got, ref, rtol=1e-5, atol=1e-5, name=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = atol + rtol * np.abs(ref)
    bad = err > tol
    assert not bad.any(), "%s: %d/%d mismatches, max err %.3e (ref %.3e) at %s" % (
        name, bad.sum(), bad.size, err.max(), np.abs(ref).max(), np.unravel_index(err.argmax(), err.shape))


def close_rel_max(got, ref, rel=2e-4, name=""):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = np.abs(ref).max() + 1e-30
    err = np.abs(got - ref).max()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


@pytest.fixture(scope="module")
def ops():
    from brats2019_amd import ops as m
    return m


@pytest.mark.parametrize("tag,bias", [("c3_4_16", False), ("c3_16_16", False), ("c3_32_32", False), ("c3_16_3b", True)])
def test_conv3_golden(golden, ops, tag, bias):
    g = golden("ops")
    x, w, dy = dev(g[tag + "_x"]), dev(g[tag + "_w"]), dev(g[tag + "_dy"])
    b = dev(g[tag + "_b"]) if bias else None
    close(ops.conv3d(x, w, b), g[tag + "_y"], name=tag + " fwd")
    close(ops.conv3d_bwd_data(dy, w, x.shape[2:]), g[tag + "_dx"], name=tag + " dgrad")
    if bias:
        dw, db = ops.conv3d_bwd_weight(x, dy, 3, with_bias=True)
        close_rel_max(db, g[tag + "_db"], name=tag + " db")
    else:
        dw = ops.conv3d_bwd_weight(x, dy, 3)
    close_rel_max(dw, g[tag + "_dw"], name=tag + " wgrad")


@pytest.mark.parametrize("tag,k", [("c2s2_16_32", 2), ("c1_32_16", 1), ("c1_128_64", 1)])
def test_small_convs_golden(golden, ops, tag, k):
    g = golden("ops")
    x, w, dy = dev(g[tag + "_x"]), dev(g[tag + "_w"]), dev(g[tag + "_dy"])
    close(ops.conv3d(x, w), g[tag + "_y"], name=tag + " fwd")
    close(ops.conv3d_bwd_data(dy, w, x.shape[2:]), g[tag + "_dx"], name=tag + " dgrad")
    close_rel_max(ops.conv3d_bwd_weight(x, dy, k), g[tag + "_dw"], name=tag + " wgrad")


CONV3_CASES = [  # (N, Cin, Cout, D, H, W): every level's channel pair, ragged / non-multiple-of-tile extents, W % 4 != 0
    (1, 4, 16, 12, 20, 36), (2, 16, 16, 9, 17, 33), (1, 32, 32, 8, 16, 32), (1, 64, 64, 8, 8, 16),
    (1, 128, 128, 4, 8, 16), (1, 16, 3, 7, 9, 18), (1, 8, 8, 6, 6, 6), (2, 3, 16, 5, 8, 16), (1, 16, 32, 4, 4, 4),
    (1, 32, 32, 32, 32, 32),
]


@pytest.mark.parametrize("case", CONV3_CASES)
def test_conv3_vs_oracle(ops, case):
    n, cin, cout, d, h, w = case
    rng = np.random.default_rng(sum(case))
    x = rng.standard_normal((n, cin, d, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)
    dy = rng.standard_normal((n, cout, d, h, w)).astype(np.float32)
    xt, wtt = T(x).requires_grad_(True), T(wt).requires_grad_(True)
    y = O.conv3x3x3(xt, wtt)
    y.backward(T(dy))
    close(ops.conv3d(dev(x), dev(wt)), y, name="fwd %s" % (case,))
    close(ops.conv3d_bwd_data(dev(dy), dev(wt), (d, h, w)), xt.grad, atol=2e-5, name="dgrad %s" % (case,))
    close_rel_max(ops.conv3d_bwd_weight(dev(x), dev(dy), 3), wtt.grad.numpy(), name="wgrad %s" % (case,))


@pytest.mark.parametrize("case", [(2, 16, 32, 8, 12, 16, 2), (1, 64, 128, 4, 4, 8, 2), (1, 8, 16, 2, 6, 6, 2),
                                  (1, 64, 32, 5, 7, 9, 1), (2, 32, 16, 8, 8, 8, 1), (1, 16, 8, 3, 3, 3, 1)])
def test_small_convs_vs_oracle(ops, case):
    n, cin, cout, d, h, w, k = case
    rng = np.random.default_rng(sum(case))
    x = rng.standard_normal((n, cin, d, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k, k)) / np.sqrt(k ** 3 * cin)).astype(np.float32)
    xt, wtt = T(x).requires_grad_(True), T(wt).requires_grad_(True)
    y = O.conv2x2x2_s2(xt, wtt) if k == 2 else O.conv1x1x1(xt, wtt)
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(T(dy))
    close(ops.conv3d(dev(x), dev(wt)), y, name="fwd %s" % (case,))
    close(ops.conv3d_bwd_data(dev(dy), dev(wt), (d, h, w)), xt.grad, atol=2e-5, name="dgrad %s" % (case,))
    close_rel_max(ops.conv3d_bwd_weight(dev(x), dev(dy), k), wtt.grad.numpy(), name="wgrad %s" % (case,))


@pytest.mark.parametrize("tag", ["gn16", "gn128"])
def test_group_norm_golden(golden, ops, tag):
    g = golden("ops")
    x, gamma, beta, dy = dev(g[tag + "_x"]), dev(g[tag + "_gamma"]), dev(g[tag + "_beta"]), dev(g[tag + "_dy"])
    y, mean, rstd = ops.group_norm(x, gamma, beta, slope=1.0)
    close(y, g[tag + "_y"], atol=2e-6, name=tag + " y")
    close(mean, g[tag + "_mean"].ravel(), atol=1e-6, name=tag + " mean")
    close(rstd, g[tag + "_rstd"].ravel(), rtol=1e-5, name=tag + " rstd")
    dx, dgam, dbet = ops.group_norm_bwd(x, gamma, beta, mean, rstd, dy, slope=1.0)
    close(dx, g[tag + "_dx"], rtol=1e-4, atol=5e-6, name=tag + " dx")
    close_rel_max(dgam, g[tag + "_dgamma"], name=tag + " dgamma")
    close_rel_max(dbet, g[tag + "_dbeta"], name=tag + " dbeta")


def test_group_norm_act_residual_vs_oracle(ops):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 32, 6, 10, 14)) * 2 + 0.5).astype(np.float32)
    res = rng.standard_normal(x.shape).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.uniform(-0.5, 0.5, 32).astype(np.float32)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    xt, gt, bt, rt = (T(a).requires_grad_(True) for a in (x, gamma, beta, res))
    y = rt + O.leaky_relu(O.group_norm(xt, gt, bt))
    y.backward(T(dy))
    yh, mean, rstd = ops.group_norm(dev(x), dev(gamma), dev(beta), slope=0.01, residual=dev(res))
    close(yh, y, atol=3e-6, name="gn+lrelu+res")
    dx, dgam, dbet = ops.group_norm_bwd(dev(x), dev(gamma), dev(beta), mean, rstd, dev(dy), slope=0.01)
    close(dx, xt.grad, rtol=1e-4, atol=5e-6, name="dx")
    close_rel_max(dgam, gt.grad.numpy(), name="dgamma")
    close_rel_max(dbet, bt.grad.numpy(), name="dbeta")


def test_leaky_relu_sigmoid_golden(golden, ops):
    g = golden("ops")
    y = ops.leaky_relu(dev(g["lrelu_x"]))
    assert np.array_equal(y.cpu().numpy(), g["lrelu_y"])                       # bit-exact elementwise
    assert np.array_equal(ops.leaky_relu_bwd(y, dev(g["lrelu_dy"])).cpu().numpy(), g["lrelu_dx"])
    close(ops.sigmoid(dev(g["sig_x"])), g["sig_y"], rtol=1e-6, atol=1e-7, name="sigmoid")


def test_trilinear_golden_and_ragged(golden, ops):
    g = golden("ops")
    close(ops.upsample2x(dev(g["up_x"])), g["up_y"], atol=1e-6, name="up fwd")
    close(ops.upsample2x_bwd(dev(g["up_dy"])), g["up_dx"], atol=1e-5, name="up bwd")
    rng = np.random.default_rng(9)
    for shape in [(1, 2, 1, 1, 1), (1, 3, 2, 1, 5), (2, 4, 8, 8, 8)]:
        x = rng.standard_normal(shape).astype(np.float32)
        xt = T(x).requires_grad_(True)
        y = O.trilinear_up2(xt)
        dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
        y.backward(T(dy))
        close(ops.upsample2x(dev(x)), y, atol=1e-6, name="up fwd %s" % (shape,))
        close(ops.upsample2x_bwd(dev(dy)), xt.grad, atol=1e-5, name="up bwd %s" % (shape,))


def test_criterion_golden(golden, ops):
    g = golden("loss")
    p, gt = dev(g["p"]), dev(g["g"])
    count = float(p.numel())
    for tag, wd, wb, bgw in (("dice", 1.0, 0.0, 1.0), ("bce", 0.0, 1.0, 1e-2), ("bce_w1", 0.0, 1.0, 1.0), ("crit", 0.5, 0.5, 1e-2)):
        sums = ops.criterion_sums(p, gt, bgw)
        dice, bce = ops.criterion_value(sums, count)
        loss = float(wd * dice + wb * bce)
        assert abs(loss - float(g[tag + "_loss"])) < 2e-6, (tag, loss, float(g[tag + "_loss"]))
        dp = ops.criterion_grad(p, gt, sums, count, wd, wb, bgw, 1.0)
        close(dp, g[tag + "_dp"], rtol=2e-5, atol=1e-9, name=tag + " dp")
    # closed-form sums vs oracle
    inter, union, bce = O.np_dice_bce_sums(g["p"], g["g"], 1e-2)
    s = ops.criterion_sums(p, gt, 1e-2).cpu().numpy()
    np.testing.assert_allclose(s[:3], inter, rtol=1e-6)
    np.testing.assert_allclose(s[3:6], union, rtol=1e-6)
    np.testing.assert_allclose(s[6], bce, rtol=1e-5)


def test_loss_modules_autograd(golden):
    from brats2019_amd import loss as L
    g = golden("loss")
    for tag, crit in (("dice", [L.Dice_loss_joint(index=0, priority=1)]), ("bce", [L.BCE_Loss(index=0, bg_weight=1e-2)]),
                      ("crit", [L.Dice_loss_joint(), L.BCE_Loss(bg_weight=1e-2)]), ("crit", [L.FusedCriterion()])):
        p = dev(g["p"]).requires_grad_(True)
        vals = [c([p], [dev(g["g"])]) for c in crit]
        lv = sum(vals) / len(vals)                       # train.py:203-205
        lv.backward()
        assert abs(float(lv) - float(g[tag + "_loss"])) < 2e-6
        close(p.grad, g[tag + "_dp"], rtol=2e-5, atol=1e-9, name=tag + " module dp")


def test_adam_golden(golden, ops):
    g = golden("adam")
    w = dev(g["w0"])
    m, v, vmax = torch.zeros_like(w), torch.zeros_like(w), torch.zeros_like(w)
    for i in range(g["grads"].shape[0]):
        ops.adam_amsgrad_step(w, dev(g["grads"][i]), m, v, vmax, i + 1, float(g["lrs"][i]), weight_decay=1e-6)
        close(w, g["traj"][i], rtol=1e-6, atol=1e-7, name="adam step %d" % i)


@pytest.mark.parametrize("tag", ["res16", "res32d"])
def test_residual_module_golden(golden, tag):
    """model.Residual built from the per-op autograd functions (stand-alone use of the building blocks)."""
    from brats2019_amd import model as M
    g = golden("residual")
    params = {k[len(tag) + 3:]: v for k, v in g.items() if k.startswith(tag + "_p_")}
    down = None
    c = params["conv1.conv1.weight"].shape[0]
    if "downsample.0.weight" in params:
        cin = params["downsample.0.weight"].shape[1]
        down = torch.nn.Sequential(torch.nn.Conv3d(cin, c, kernel_size=2, stride=2, bias=False))
    blk = M.Residual(in_channels=c, out_channels=c, stride=1, downsample=down)
    blk.load_state_dict({k: T(v) for k, v in params.items()})
    blk.cuda()
    x = dev(g[tag + "_x"]).requires_grad_(True)
    y = blk(x)
    y.backward(dev(g[tag + "_dy"]))
    close(y, g[tag + "_y"], atol=2e-5, name=tag + " y")
    close(x.grad, g[tag + "_dx"], rtol=1e-4, atol=2e-5, name=tag + " dx")
    for k, p in blk.named_parameters():
        close_rel_max(p.grad, g["%s_g_%s" % (tag, k)], rel=3e-4, name="%s grad %s" % (tag, k))


# ---------------------------------------------------------------- split-bf16 (bf16x3) convolution path
# hi+lo operands carry 16 mantissa bits -> each product is accurate to ~2^-16; over K <= 3456 products of random sign the
# output error is ~2^-16 * sqrt(K) * rms(x) * rms(w): we hold max|err| <= 1e-4 * max|ref| (plain bf16 operands: ~5e-3).
@pytest.mark.parametrize("case", [(1, 4, 16, 12, 20, 32), (2, 16, 16, 9, 17, 32), (1, 32, 32, 8, 16, 32), (1, 64, 64, 8, 8, 16),
                                  (1, 128, 128, 4, 8, 16), (1, 16, 3, 7, 9, 20), (1, 8, 8, 6, 6, 8), (2, 3, 16, 5, 8, 16),
                                  (1, 16, 16, 32, 32, 32), (1, 24, 40, 6, 10, 12)])
def test_conv3_bf16x3_vs_oracle(ops, case):
    n, cin, cout, d, h, w = case
    rng = np.random.default_rng(sum(case) + 1)
    x = rng.standard_normal((n, cin, d, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    dy = rng.standard_normal((n, cout, d, h, w)).astype(np.float32)
    xt, wtt = T(x).requires_grad_(True), T(wt)
    y = O.conv3x3x3(xt, wtt, T(b))
    y.backward(T(dy))
    close_rel_max(ops.conv3d(dev(x), dev(wt), dev(b), precision="bf16x3"), y.detach().numpy(), rel=1e-4, name="bf16x3 fwd %s" % (case,))
    close_rel_max(ops.conv3d_bwd_data(dev(dy), dev(wt), (d, h, w), precision="bf16x3"), xt.grad.numpy(), rel=1e-4, name="bf16x3 dgrad %s" % (case,))
    wtt2 = T(wt).requires_grad_(True)
    O.conv3x3x3(T(x), wtt2).backward(T(dy))
    close_rel_max(ops.conv3d_bwd_weight(dev(x), dev(dy), 3, precision="bf16x3"), wtt2.grad.numpy(), rel=2e-4, name="bf16x3 wgrad %s" % (case,))


def test_conv3_bf16x3_is_not_plain_bf16(ops):
    """The lo terms matter: the result must be far closer to fp32 than single-bf16 operands could be."""
    rng = np.random.default_rng(77)
    x = rng.standard_normal((1, 16, 8, 16, 32)).astype(np.float32)
    wt = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(432)).astype(np.float32)
    ref = O.conv3x3x3(T(x), T(wt)).numpy().astype(np.float64)
    got = ops.conv3d(dev(x), dev(wt), precision="bf16x3").cpu().numpy()
    plain = O.conv3x3x3(T(x).bfloat16().float(), T(wt).bfloat16().float()).numpy()
    e_split, e_plain = np.abs(got - ref).max(), np.abs(plain - ref).max()
    assert e_split < e_plain / 50, (e_split, e_plain)


def test_conv3_bf16x3_ragged_w_falls_back_to_f32(ops):
    rng = np.random.default_rng(78)
    x = rng.standard_normal((1, 16, 4, 6, 18)).astype(np.float32)        # W % 4 != 0
    wt = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(432)).astype(np.float32)
    close(ops.conv3d(dev(x), dev(wt), precision="bf16x3"), O.conv3x3x3(T(x), T(wt)), name="fallback")


def test_dice_metric_matches_reference(golden):
    """metrics.Dice (metrics.py:101-133) vs the value the reference's own class produced (tests/golden/loss.npz)."""
    from brats2019_amd import metrics as MT
    g = golden("loss")
    m = MT.Dice(classes=4)
    m.update([dev(g["g"])], [dev(g["p"])])
    np.testing.assert_array_equal(m.get(), g["metric_dice"])
    m.update([dev(g["g"])], [dev(g["g"])])                 # perfect prediction -> 1 in every class; mean of the two updates
    np.testing.assert_allclose(m.get(), (g["metric_dice"] + 1.0) / 2, rtol=0, atol=1e-12)
    empty = torch.zeros(1, 3, 4, 4, 4).cuda()
    m.reset()
    m.update([empty], [empty])                              # 0/0 -> NaN -> 1 (metrics.py:128)
    assert np.array_equal(m.get(), np.ones(3))


# ---------------------------------------------------------------- GroupNorm with trained-like parameters, against float64
# Row lengths V = D*H*W around GN_CHUNK = 8192 (pointwise.hip): one, two and three chunks, a ragged last chunk, the float4 path (V % 4 == 0) and the scalar one;
# every W is odd.  8191 is prime and 8192 = 2^13, so those two are single rows / W = 1.
GN_SHAPES = {8191: (1, 1, 8191), 8192: (32, 256, 1), 8193: (1, 3, 2731), 16385: (5, 29, 113), 105: (3, 5, 7)}
_EPS32 = float(np.finfo(np.float32).eps)


def gn_param_set(kind, c, rng):
    """gamma / beta as Adam leaves them (module docstring of tests/test_hip_gn_params.py), 8 groups of c/8 channels:
    signs -- seeded +-1 on U(.5, 1.5); group 0 is forced to hold both signs.   zeros -- gamma == 0 with beta > 0, < 0 and == 0 (channels 0, 1, 2).
    tiny -- |gamma| = 1e-6 of both signs (channels 0, 1, with beta != 0; channels 2, 3 with beta == 0).   ties -- beta == 0 everywhere, gamma != 0."""
    gamma = rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)
    beta = rng.uniform(-0.5, 0.5, c)
    gamma[0], gamma[1] = abs(gamma[0]), -abs(gamma[1])
    if kind == "zeros":
        gamma[:3] = 0.0
        beta[:3] = (0.3, -0.3, 0.0)
    elif kind == "tiny":
        gamma[:4] = (1e-6, -1e-6, 1e-6, -1e-6)
        beta[:4] = (0.2, -0.2, 0.0, 0.0)
    elif kind == "ties":
        beta[:] = 0.0
    else:
        assert kind == "signs"
    return gamma.astype(np.float32), beta.astype(np.float32)


def gn_off_the_kink(x, gamma, beta):
    """LeakyReLU is discontinuous in its derivative: where the float64 pre-activation lies within float32 rounding of zero, no float32 implementation has a defined
    mask, and one flipped element moves dx, dgamma and dbeta by O(1).  Such elements (a few per million) are moved off the kink by 1e-3 in x; the band is 64 ulp of the
    terms that form the pre-activation.  Exact ties survive on purpose: gamma == 0 gives pre == beta in float32 and float64 alike (beta == 0: the `>` branch)."""
    x = x.copy()
    bshape = (1, -1, 1, 1, 1)
    g64, b64 = gamma.astype(np.float64).reshape(bshape), beta.astype(np.float64).reshape(bshape)
    for _ in range(8):
        pre, mu, rstd = O.np_group_norm(x, gamma, beta)
        cpg = x.shape[1] // O.GN_GROUPS
        a = np.abs(g64) * np.repeat(rstd, cpg, axis=1).reshape(x.shape[0], -1, 1, 1, 1)
        m = np.abs(np.repeat(mu, cpg, axis=1)).reshape(x.shape[0], -1, 1, 1, 1)
        band = 64 * _EPS32 * (a * (np.abs(x) + m + np.abs(x).max()) + np.abs(b64))
        amb = (np.abs(pre) < band) & (g64 != 0)
        if not amb.any():
            return x
        x[amb] += np.float32(1e-3) * np.where(x[amb] >= 0, 1, -1).astype(np.float32)
    raise AssertionError("could not move the inputs off the LeakyReLU kink")


def gn_reference64(x, gamma, beta, dy, slope, res):
    """float64: y = res + lrelu(GN(x)), and the backward of lrelu(GN(x)) for an upstream dy (the residual passes dy on unchanged: no part of group_norm_bwd)"""
    pre, mu, rstd = O.np_group_norm(x, gamma, beta)
    y = np.where(pre > 0, pre, pre * slope) + (0.0 if res is None else res.astype(np.float64))
    dh = dy.astype(np.float64) * np.where(pre > 0, 1.0, slope)
    dx, dgamma, dbeta = O.np_group_norm_bwd(x, gamma, dh)
    return y, mu, rstd, dx, dgamma, dbeta


def check_gn_case(ops, v, c, slope, with_res, kind):
    n = 2
    seed = [v, c, int(slope * 100), int(with_res), sorted(("signs", "zeros", "tiny", "ties")).index(kind)]
    rng = np.random.default_rng(seed)
    gamma, beta = gn_param_set(kind, c, rng)
    shape = (n, c) + GN_SHAPES[v]
    x = gn_off_the_kink((rng.standard_normal(shape) * 2 + 0.5).astype(np.float32), gamma, beta)
    res = rng.standard_normal(shape).astype(np.float32) if with_res else None
    dy = rng.standard_normal(shape).astype(np.float32)
    y64, mu64, rstd64, dx64, dg64, db64 = gn_reference64(x, gamma, beta, dy, slope, res)
    tag = "V=%d C=%d slope=%g res=%d %s" % (v, c, slope, with_res, kind)
    yh, mean, rstd = ops.group_norm(dev(x), dev(gamma), dev(beta), slope=slope, residual=None if res is None else dev(res))
    dx, dgam, dbet = ops.group_norm_bwd(dev(x), dev(gamma), dev(beta), mean, rstd, dev(dy), slope=slope)
    err = lambda got, ref: float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print("  %s: max error  y %.2e  mean %.2e  rstd %.2e  dx %.2e  dgamma %.2e / %.2e  dbeta %.2e / %.2e" % (
        tag, err(yh, y64), err(mean, mu64.ravel()), err(rstd, rstd64.ravel()), err(dx, dx64), err(dgam, dg64), np.abs(dg64).max(), err(dbet, db64), np.abs(db64).max()))
    close(yh, y64, atol=3e-6, name=tag + " y")
    close(mean, mu64.ravel(), atol=1e-6, name=tag + " mean")
    close(rstd, rstd64.ravel(), rtol=1e-5, name=tag + " rstd")
    close(dx, dx64, rtol=1e-4, atol=5e-6, name=tag + " dx")
    close_rel_max(dgam, dg64, name=tag + " dgamma")
    close_rel_max(dbet, db64, name=tag + " dbeta")


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("slope", [1.0, 0.01])
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("v", sorted(GN_SHAPES))
def test_group_norm_row_lengths_mixed_sign_gamma_vs_float64(ops, v, c, slope, with_res):
    """ops.group_norm / ops.group_norm_bwd (model.py:95-96 + the LeakyReLU of model.py:93-94 + the residual add of model.py:115) against float64 at row lengths on
    both sides of every path switch of gn_stats / gn_apply / gn_bwd_reduce / gn_bwd_apply, with gammas of both signs (one group holds both) -- this file's
    tolerances for y, dx (close) and dgamma, dbeta (close_rel_max), unchanged."""
    check_gn_case(ops, v, c, slope, with_res, "signs")


@pytest.mark.parametrize("slope", [1.0, 0.01])
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("v", [105, 8193])
@pytest.mark.parametrize("kind", ["zeros", "tiny", "ties"])
def test_group_norm_zero_tiny_and_tied_parameters_vs_float64(ops, kind, v, c, slope):
    """gamma == 0 with beta > 0, < 0, == 0 (the pre-activation is the constant beta: mask all, none, none); |gamma| = 1e-6 of both signs; beta == 0 with gamma != 0
    (the mask is the sign of gamma * xhat).  Same tolerances; the residual is on."""
    check_gn_case(ops, v, c, slope, True, kind)


def gn_fixture_ratio(golden):
    """R = max |mean| * rstd over every GroupNorm layer of the reference's own 32^3 step (tests/golden/unet32.npz, gnstat_*: [2][1][8] = mean, rstd per group)"""
    g = golden("unet32")
    keys = sorted(k for k in g if k.startswith("gnstat_"))
    assert len(keys) == 25, keys
    return max(float(np.abs(g[k][0].astype(np.float64) * g[k][1].astype(np.float64)).max()) for k in keys)


GN_RATIOS = (0, 3, 10, 30, 100, 300, 1000)


def test_group_norm_statistics_conditioning(golden, ops):
    """Variance of x = mu + z (z ~ N(0, 1) seeded, V = 16385, C = 16, N = 2) at mu / sigma from 0 to 1000: error of rstd and of y (max |y - y64| / max |y64|) for
    ops.group_norm and for float32 F.group_norm on the CPU (what the reference runs), both against float64.  Bar: up to 10 R -- R = the largest |mean| * rstd the
    reference's own step reaches (gn_fixture_ratio; tests/test_hip_gn_params_host.py holds R finite and positive), ten-fold headroom for training drift -- our error
    stays within 4x the float32 reference's plus 1e-6.  Larger ratios are printed only.  profiles/gn_conditioning.txt holds the measured table."""
    R = gn_fixture_ratio(golden)
    assert np.isfinite(R) and R > 0
    n, c, v = 2, 16, 16385
    rng = np.random.default_rng(20)
    z = rng.standard_normal((n, c) + GN_SHAPES[v])
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
    print("\n  R = %.4f, asserted up to mu/sigma = %.2f\n  mu/sigma   rstd error (ours, f32 CPU)   y error (ours, f32 CPU)   asserted" % (R, 10 * R))
    failures = []
    for ratio in GN_RATIOS:
        x = (ratio + z).astype(np.float32)
        y64, _, rstd64 = O.np_group_norm(x, gamma, beta)
        yc, _, rc = torch.native_group_norm(T(x), T(gamma), T(beta), n, c, v, O.GN_GROUPS, O.GN_EPS)
        yh, _, rh = ops.group_norm(dev(x), dev(gamma), dev(beta), slope=1.0)
        e_r = lambda r: float(np.abs(r.cpu().numpy().astype(np.float64).ravel() - rstd64.ravel()).max() / rstd64.max())
        e_y = lambda y: float(np.abs(y.cpu().numpy().astype(np.float64) - y64).max() / np.abs(y64).max())
        row = (e_r(rh), e_r(rc), e_y(yh), e_y(yc))
        asserted = ratio <= 10 * R
        print("  %8g   %.2e  %.2e          %.2e  %.2e      %s" % ((ratio,) + row + ("yes" if asserted else "no",)))
        if asserted and not (row[0] <= 4 * row[1] + 1e-6 and row[2] <= 4 * row[3] + 1e-6):
            failures.append((ratio, row))
    assert not failures, failures
