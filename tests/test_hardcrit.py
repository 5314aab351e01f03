"""Focal, Tversky / focal-Tversky and top-k losses on the device (csrc/hardcrit.hip; loss.FocalLoss, TverskyLoss, TopKLoss) against their
float64 host restatements (loss.focal_host, tversky_host, topk_host; tests/test_hardcrit_host.py holds those to float64 autograd), against
BCE_Loss where they coincide, sharded against whole, inside the network's backward and inside Trainer.train.

Bars.  Every bar below is 4x the worst figure measured on the MI355X against the float64 restatement (the convention of
tests/test_intensity.py); each test prints its figure before it asserts.  Gradient error is max |dp - ref| / (|ref| + 1e-4 max |ref|),
value error is relative.  Measured worst cases are written beside each bar."""
import functools

import numpy as np
import pytest
import torch

import hardcrit_inputs as I
from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy

FOCAL_VALUE_BAR = 4 * 6.8e-8        # measured 6.8e-8 (the float32 rounding of the returned scalar, 2^-24)
FOCAL_GRAD_BAR = 4 * 2.3e-7         # measured 2.3e-7 (gamma = 2.5 at the two-trip shape)
TVERSKY_VALUE_BAR = 4 * 3.6e-8      # measured 3.6e-8
TVERSKY_GRAD_BAR = 4 * 7.6e-8       # measured 7.6e-8
TOPK_VALUE_BAR = 4 * 7.8e-8         # measured 7.8e-8 (K = 1: one float32 l against the float64 one)
GRAD_CEILING = 2e-5                 # tests/test_criteria.py holds ru_crit_grad to this: a measured gradient error above it is a defect

FOCAL_CASES = [(2.0, None, 1), (0, None, 1e-2), (1, 0.25, 1), (2.5, 0.25, 1e-2)]                 # gamma, alpha, bg_weight
TVERSKY_CASES = [(0.5, 0.5, 1.0, 1), (0.3, 0.7, 4.0 / 3.0, 1), (0.3, 0.7, 1.0, 2)]               # alpha, beta, gamma, priority
SHAPES = [I.ODD, I.TINY, I.TWO_TRIPS]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    p, g = I.make(shape)
    return p, g, T(p).cuda(), T(g).cuda()


def _grad_err(dp, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(np.asarray(dp, dtype=np.float64) - ref) / (np.abs(ref) + 1e-4 * np.abs(ref).max())).max())


def _run(module, pd, gd):
    x = pd.clone().requires_grad_(True)
    loss = module([x], [gd])
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (dp,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), dp.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=["odd", "tiny", "two_trips"])
def test_focal_matches_the_host_restatement(shape):
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(shape)
    worst_v = worst_g = 0.0
    for gamma, alpha, bg in FOCAL_CASES:
        value, dp = _run(L.FocalLoss(gamma=gamma, alpha=alpha, bg_weight=bg), pd, gd)
        ref_v, ref_dp = L.focal_host(p, g, gamma=gamma, alpha=alpha, bg_weight=bg)
        ev, eg = abs(value - ref_v) / abs(ref_v), _grad_err(dp, ref_dp)
        print("focal %s gamma=%s alpha=%s bg=%s: value err %.3e, gradient err %.3e" % (shape, gamma, alpha, bg, ev, eg))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    assert FOCAL_GRAD_BAR < GRAD_CEILING
    assert worst_v <= FOCAL_VALUE_BAR and worst_g <= FOCAL_GRAD_BAR, (worst_v, worst_g)


@pytest.mark.parametrize("shape", SHAPES, ids=["odd", "tiny", "two_trips"])
def test_tversky_matches_the_host_restatement(shape):
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(shape)
    worst_v = worst_g = 0.0
    for alpha, beta, gamma, priority in TVERSKY_CASES:
        value, dp = _run(L.TverskyLoss(alpha=alpha, beta=beta, gamma=gamma, priority=priority), pd, gd)
        ref_v, ref_dp = L.tversky_host(p, g, alpha=alpha, beta=beta, gamma=gamma, priority=priority)
        ev, eg = abs(value - ref_v) / abs(ref_v), _grad_err(dp, ref_dp)
        print("tversky %s alpha=%s beta=%s gamma=%.4f priority=%s: value err %.3e, gradient err %.3e" % (shape, alpha, beta, gamma, priority, ev, eg))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    assert TVERSKY_GRAD_BAR < GRAD_CEILING
    assert worst_v <= TVERSKY_VALUE_BAR and worst_g <= TVERSKY_GRAD_BAR, (worst_v, worst_g)


@pytest.mark.parametrize("bg", I.BG_WEIGHTS)
def test_focal_gamma_0_and_topk_100_are_bce_loss(bg):
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(I.ODD)
    bce_v, bce_dp = _run(L.BCE_Loss(bg_weight=bg), pd, gd)
    for name, module in (("focal", L.FocalLoss(gamma=0, alpha=None, bg_weight=bg)), ("topk", L.TopKLoss(k=100, bg_weight=bg))):
        value, dp = _run(module, pd, gd)
        ev, eg = abs(value - bce_v) / abs(bce_v), _grad_err(dp, bce_dp)
        print("%s vs BCE_Loss bg=%s: value err %.3e, gradient err %.3e" % (name, bg, ev, eg))
        assert ev <= max(FOCAL_VALUE_BAR, TOPK_VALUE_BAR) and eg <= FOCAL_GRAD_BAR, (name, ev, eg)
        assert int((dp != 0).sum()) == dp.size


@pytest.mark.parametrize("gamma", [0, 1, 2])
def test_focal_is_finite_at_saturated_probabilities(gamma):
    from brats2019_amd import loss as L
    p, g = I.make((1, 2, 3, 5, 7))
    p = p.copy()
    p.reshape(-1)[::3] = 0.0
    p.reshape(-1)[1::3] = 1.0
    for alpha in (None, 0.25):
        value, dp = _run(L.FocalLoss(gamma=gamma, alpha=alpha), T(p).cuda(), T(g).cuda())
        ref_v, ref_dp = L.focal_host(p, g, gamma=gamma, alpha=alpha)
        print("focal saturated gamma=%s alpha=%s: value err %.3e, gradient err %.3e" % (gamma, alpha, abs(value - ref_v) / abs(ref_v), _grad_err(dp, ref_dp)))
        assert np.isfinite(value) and np.isfinite(dp).all() and np.isfinite(ref_v) and np.isfinite(ref_dp).all()
        assert abs(value - ref_v) <= FOCAL_VALUE_BAR * abs(ref_v) and _grad_err(dp, ref_dp) <= FOCAL_GRAD_BAR


def _select(pd, gd, k, bg):
    from brats2019_amd import loss as L, ops
    K = L._topk_count(pd.numel(), k)
    out, state, keys = ops.topk_select(pd, gd, K, bg)
    dp = ops.topk_grad(pd, gd, keys, state, K, bg)
    return K, out, state, keys, dp


@pytest.mark.parametrize("bg", I.BG_WEIGHTS)
def test_topk_value_and_threshold_match_the_host_restatement(bg):
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(I.ODD)
    worst_v = worst_g = 0.0
    for k in I.KS:
        K, out, state, keys, dp = _select(pd, gd, k, bg)
        value, t = [float(v) for v in out.cpu()]
        _key, rest, n_gt, n_eq = [int(v) for v in state.cpu()]
        dp = dp.cpu().numpy()
        l, K_h, t_h, n_gt_h, n_eq_h = L.topk_host_threshold(p, g, k=k, bg_weight=bg)
        ref_v, ref_dp = L.topk_host(p, g, k=k, bg_weight=bg)
        ev = abs(value - ref_v) / abs(ref_v)
        outside = np.abs(l - t_h) > I.BAND * abs(t_h)
        eg = float((np.abs(dp - ref_dp)[outside] / (np.abs(ref_dp)[outside] + 1e-4 * np.abs(ref_dp).max())).max()) if outside.any() else 0.0
        print("topk bg=%s k=%s: K %d, t %.9g (host %.9g), n_gt %d, n_eq %d, value err %.3e, gradient err outside the band %.3e, %d in the band"
              % (bg, k, K, t, t_h, n_gt, n_eq, ev, eg, int((~outside).sum())))
        assert K == K_h and rest == K - n_gt and n_gt < K <= n_gt + n_eq
        assert int((dp != 0).sum()) == K                            # no float32 tie at the threshold: exactly K elements carry gradient
        assert abs(t - t_h) <= I.BAND * abs(t_h)
        assert int((~outside).sum()) <= I.BAND_CAP
        value_mod, _ = _run(L.TopKLoss(k=k, bg_weight=bg), pd, gd)
        assert value_mod == float(np.float32(value))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    assert worst_v <= TOPK_VALUE_BAR and worst_g <= FOCAL_GRAD_BAR, (worst_v, worst_g)


@pytest.mark.parametrize("shape,k", [(I.TINY, 10), (I.TWO_TRIPS, 10), (I.TWO_TRIPS, 0.001)], ids=["tiny", "two_trips_10", "two_trips_0.001"])
def test_topk_value_at_the_other_shapes(shape, k):
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(shape)
    K, out, state, keys, dp = _select(pd, gd, k, 1)
    ref_v, ref_dp = L.topk_host(p, g, k=k)
    ev = abs(float(out[0]) - ref_v) / abs(ref_v)
    print("topk %s k=%s: K %d, value err %.3e" % (shape, k, K, ev))
    assert ev <= TOPK_VALUE_BAR
    n_gt, n_eq = int(state[2]), int(state[3])
    assert int((dp != 0).sum()) == n_gt + n_eq and n_gt < K <= n_gt + n_eq


def test_topk_k_1_puts_the_gradient_at_the_arg_max():
    from brats2019_amd import loss as L
    for shape in (I.TINY, I.ODD):
        p, g, pd, gd = _inputs(shape)
        assert L._topk_count(p.size, 0.001) == 1
        l, K, t, n_gt, n_eq = L.topk_host_threshold(p, g, k=0.001)
        value, dp = _run(L.TopKLoss(k=0.001), pd, gd)
        (nz,) = np.nonzero(dp.reshape(-1))
        assert nz.tolist() == [int(np.argmax(l))]
        assert abs(value - t) <= TOPK_VALUE_BAR * t
        ref_dp = L.topk_host(p, g, k=0.001)[1].reshape(-1)
        assert abs(dp.reshape(-1)[nz[0]] - ref_dp[nz[0]]) <= FOCAL_GRAD_BAR * abs(ref_dp[nz[0]])


def test_topk_shares_a_tie_symmetrically():
    from brats2019_amd import loss as L
    p, g = I.make_ties()
    bg, k = 0.5, 30
    pd, gd = T(p).cuda(), T(g).cuda()
    l, K_h, t_h, n_gt_h, n_eq_h = L.topk_host_threshold(p, g, k=k, bg_weight=bg)
    assert len(np.unique(l)) == 6 and n_gt_h < K_h < n_gt_h + n_eq_h, "K must cut through a tie class"
    K, out, state, keys, dp = _select(pd, gd, k, bg)
    value, t = [float(v) for v in out.cpu()]
    _key, rest, n_gt, n_eq = [int(v) for v in state.cpu()]
    dp = dp.cpu().numpy()
    assert (K, n_gt, n_eq) == (K_h, n_gt_h, n_eq_h)
    assert abs(t - t_h) <= 1e-6 * t_h
    ref_v = (l[l > t_h].sum() + (K - n_gt) * t_h) / K
    assert abs(value - ref_v) <= TOPK_VALUE_BAR * ref_v
    dl = bg * (1.0 - g.astype(np.float64)) / (np.float32(1.0 + 1e-6) - p).astype(np.float64) - g.astype(np.float64) / (p + np.float32(1e-6)).astype(np.float64)
    tied, above = l == t_h, l > t_h
    np.testing.assert_allclose(dp[tied] / dl[tied], (K - n_gt) / (n_eq * K), rtol=FOCAL_GRAD_BAR)
    np.testing.assert_allclose(dp[above] / dl[above], 1.0 / K, rtol=FOCAL_GRAD_BAR)
    assert not dp[l < t_h].any()
    assert _grad_err(dp, L.topk_host(p, g, k=k, bg_weight=bg)[1]) <= FOCAL_GRAD_BAR


def test_topk_nan_gives_a_nan_value():
    from brats2019_amd import loss as L
    p, g = I.make((1, 2, 3, 5, 7))
    p = p.copy()
    p[0, 1, 2, 3, 4] = np.nan
    for k in (1, 100):
        value, _ = _run(L.TopKLoss(k=k), T(p).cuda(), T(g).cuda())
        assert np.isnan(value)


def test_two_calls_give_identical_bytes():
    from brats2019_amd import ops
    p, g, pd, gd = _inputs(I.TWO_TRIPS)
    runs = []
    for _ in range(2):
        K, out, state, keys, dp = _select(pd, gd, 10, 1)
        fs = ops.focal_sum(pd, gd, 2.0, 1.0, 1.0)
        fg = ops.focal_grad(pd, gd, 2.0, 1.0, 1.0, float(pd.numel()))
        runs.append([v.cpu().numpy().tobytes() for v in (out, state, keys, dp, fs, fg)])
    assert runs[0] == runs[1]


def test_sharded_sums_evaluate_to_the_whole_batch():
    """two half-batches: focal sums added and Tversky totals added (what the all-reduce does), evaluated per half -> the whole batch.  The
    second half starts 4 bytes past a 16-byte boundary."""
    from brats2019_amd import ops, _lib
    p, g, pd, gd = _inputs(I.ODD)
    halves = [(pd[:1], gd[:1]), (pd[1:], gd[1:])]
    assert halves[1][0].is_contiguous() and halves[1][0].data_ptr() % 16 == 4
    count = float(pd.numel())
    fp = (2.0, 0.25, 0.75 * 1e-2)
    s_all = ops.focal_sum(pd, gd, *fp)
    s_half = sum(ops.focal_sum(a, b, *fp) for a, b in halves)
    np.testing.assert_allclose(s_half.cpu().numpy(), s_all.cpu().numpy(), rtol=1e-12, atol=0)
    ref = ops.focal_grad(pd, gd, *fp, count).cpu().numpy()
    got = torch.cat([ops.focal_grad(a, b, *fp, count) for a, b in halves]).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())
    mask = _lib.CRIT_MASK_ALL & ~_lib.CRIT_MASK_LOGS
    tv = (0.3, 0.7, 4.0 / 3.0, 1.0, 1.0)
    v_all, coef = ops.tversky_eval(ops.crit_reduce(ops.crit_moments(pd, gd, mask)), 2, 3, *tv)
    ref = ops.crit_grad(pd, gd, coef, None, False).cpu().numpy()
    totals = sum(ops.crit_reduce(ops.crit_moments(a, b, mask)) for a, b in halves)
    outs = [ops.tversky_eval(totals, 1, 3, *tv) for _ in halves]
    for v, _c in outs:
        np.testing.assert_allclose(v.cpu().numpy(), v_all.cpu().numpy(), rtol=1e-12, atol=0)
    got = torch.cat([ops.crit_grad(a, b, c, None, False) for (a, b), (_v, c) in zip(halves, outs)]).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("members", [("Dice_loss_joint", "TopKLoss"), ("TverskyLoss", "FocalLoss")], ids=lambda m: "+".join(m))
def test_lists_inside_hand_over_give_the_same_parameter_gradients(members):
    """evaluated as written: inside hand_over_to_network() Dice_loss_joint describes its gradient to the network's node while the new
    classes write theirs -- the bars of test_dice_joint_with_separate_inside_hand_over_gives_the_same_parameter_gradients"""
    from brats2019_amd import model as M, loss as L
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(23, **O.DEFAULT_CFG).items()})
    net.cuda().train()
    x = T(O.make_input(2, 32, 32, 32, seed=23)).cuda()
    y = T(O.make_target(2, 32, 32, 32, seed=23)).cuda()
    assert L.fuse_criterion_list([getattr(L, m)() for m in members]) is None

    def grads(inside):
        for q in net.parameters():
            q.grad = None
        out = net([x])
        vals = [getattr(L, m)()(out, [y]) for m in members]
        loss = sum(vals) / len(vals)
        if inside:
            with L.hand_over_to_network():
                loss.backward()
        else:
            loss.backward()
        return torch.cat([q.grad.reshape(-1) for q in net.parameters() if q.grad is not None]).cpu().numpy(), float(loss.detach())
    g_out, l_out = grads(False)
    g_in, l_in = grads(True)
    assert l_in == l_out and g_in.shape == g_out.shape and np.abs(g_out).max() > 0
    np.testing.assert_allclose(g_in, g_out, rtol=1e-4, atol=1e-6 * np.abs(g_out).max())
    assert np.linalg.norm(g_in - g_out) <= 1e-5 * np.linalg.norm(g_out)


def test_trainer_runs_with_the_new_criteria(tmp_path):
    from brats2019_amd import model as M, train as TR, metrics as MT, loss as L
    seed, dhw = 41, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    w0 = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).clone()
    tr = TR.Trainer(name="hardcrit", models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    losses = []

    class Rec:
        def add_scalar(self, name, val, step):
            if name.startswith("loss/"):
                losses.append(float(val))
    tr.tb_writer = Rec()
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(O.make_target(2, *dhw, seed=seed + i))]) for i in range(2)]
    tr.train(criterion=[L.Dice_loss_joint(), L.FocalLoss(), L.TverskyLoss(gamma=4.0 / 3.0), L.TopKLoss()],
             optimizer=torch.optim.Adam, optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=False, pretrained_weights=None,
             train_metrics=[MT.Dice(name="Dice")], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice", epoches=1,
             default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    w1 = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).cpu()
    losses = np.asarray(losses)
    assert losses.shape == (8,) and np.isfinite(losses).all() and (losses > 0).all()      # four criteria x two steps
    assert torch.isfinite(w1).all() and not torch.equal(w1, w0.cpu())
