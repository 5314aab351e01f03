"""The reference's remaining training criteria on the device (loss.py:15-195; csrc/criteria.hip): MSE_Loss, CE_Loss, Dice1D, GDL_joint,
sens_loss_joint and Dice_loss_separate, one at a time and in fused lists, against the reference's own classes (tests/golden/criteria.npz,
tests/golden/make_criteria_golden.py), against float64 torch at 4 x 3 x 128^3, sharded against whole, and inside Trainer.train."""
import json

import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
KINDS = ["MSE_Loss", "CE_Loss", "Dice1D", "GDL_joint", "sens_loss_joint", "Dice_loss_separate", "Dice_loss_joint", "BCE_Loss"]


def _make(members):
    from brats2019_amd import loss as L
    return [getattr(L, cls)(**kw) for cls, kw in members]


@pytest.mark.parametrize("b", [0, 1, 2])
def test_criteria_golden(golden, b):
    """every class alone and every list, fused, against the reference's classes: values within 2e-6, dp within rtol 2e-5 / atol 1e-9
    of the float64 run (the bars of test_hip_ops.py::test_criterion_golden); batch 2 has a class absent (GDL_joint NaN where torch's is)"""
    from brats2019_amd import loss as L
    g = golden("criteria")
    runs = json.loads(str(g["runs"]))
    assert sorted({cls for m in runs.values() for cls, _ in m}) == sorted(KINDS)
    p = T(g["b%d_pred" % b]).cuda()
    y = T(g["b%d_gt" % b]).cuda()
    errors = []
    for name, members in runs.items():
        x = p.clone().requires_grad_(True)
        mods = _make(members)
        if len(mods) == 1:
            loss = mods[0]([x], [y])
            vals = [loss]
        else:
            fused = L.fuse_criterion_list(mods)
            assert fused is not None, name
            loss, vals = fused([x], [y])
        assert loss.dim() == 0 and loss.dtype == torch.float32 and len(vals) == len(members)
        (dp,) = torch.autograd.grad(loss, x)
        got = np.asarray([float(v.detach()) for v in vals])
        dp = dp.cpu().numpy()
        ref64 = g["b%d_%s_dp" % (b, name)]
        checks = [(got, g["b%d_%s_values%s" % (b, name, tag)], 0, 2e-6, "values" + tag) for tag in ("64", "32")]
        checks.append((float(loss.detach()), float(g["b%d_%s_loss64" % (b, name)]), 0, 2e-6, "loss"))
        key32 = "b%d_%s_dp32" % (b, name)
        if key32 in g:
            # BCE: the reference's (1 + 1e-6) - p is a float32 expression; where the float64 run moves it by more than the bar (p within
            # ~1e-3 of 1) the float32 run is the reference's number, elsewhere both must hold
            ref32 = g[key32]
            same = (np.abs(ref32 - ref64) <= 1e-5 * np.abs(ref64) + 1e-9) | (np.isnan(ref32) & np.isnan(ref64))
            assert same.mean() > 0.99
            checks += [(dp, ref32, 2e-5, 1e-9, "dp vs float32 run"), (dp[same], ref64[same], 2e-5, 1e-9, "dp vs float64 run")]
        else:
            checks.append((dp, ref64, 2e-5, 1e-9, "dp vs float64 run"))
        for a, r, rtol, atol, what in checks:
            try:
                np.testing.assert_allclose(a, r, rtol=rtol, atol=atol, equal_nan=True)
            except AssertionError as e:
                errors.append("%s %s: %s" % (name, what, str(e)[:600]))
    assert not errors, "\n".join(errors)
    if b == 2:
        assert np.isnan(g["b2_gdl_values64"][0]) and np.isnan(g["b2_gdl_dp"][:, 1:]).all() and not np.isnan(g["b2_gdl_dp"][:, 0]).any()


def _batch128(seed=7):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    shape = (4, 3, 128, 128, 128)
    p = torch.sigmoid(2.0 * torch.randn(shape, generator=gen, device="cuda"))
    g = (torch.rand(shape, generator=gen, device="cuda") < 0.2).float()
    return p, g


def _moments64(p, g):
    """the seven moments per (n, c) in float64, with the float32 constants of the reference's expressions"""
    eps, one_eps = float(np.float32(1e-6)), float(np.float32(1.0 + 1e-6))
    pd, gd = p.double().flatten(2), g.double().flatten(2)
    lp = torch.log((p + eps).double()).flatten(2)            # p + 1e-6 is formed in float32 (loss.py:59,77)
    lq = torch.log((one_eps - p).double()).flatten(2)
    return torch.stack([(pd * gd).sum(2), (pd * pd).sum(2), pd.sum(2), gd.sum(2), (gd * lp).sum(2), ((1 - gd) * lq).sum(2),
                        ((pd - gd) ** 2).sum(2)], dim=2)


def test_moments_at_128_cubed_match_float64_sums():
    from brats2019_amd import ops
    p, g = _batch128()
    m = ops.crit_moments(p, g)
    ref = _moments64(p, g)
    assert m.shape == (4, 3, 7) and m.dtype == torch.float64
    np.testing.assert_allclose(m.cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=0)
    m2 = ops.crit_moments(p, g, mask=0)                      # no CE / BCE term: the log moments are skipped
    np.testing.assert_array_equal(m2[..., 4:6].cpu().numpy(), 0.0)
    np.testing.assert_array_equal(m2[..., [0, 1, 2, 3, 6]].cpu().numpy(), m[..., [0, 1, 2, 3, 6]].cpu().numpy())
    # odd extent: no V % 4 assumption
    po, go = p[:, :, :127, :127, :127].contiguous(), g[:, :, :127, :127, :127].contiguous()
    np.testing.assert_allclose(ops.crit_moments(po, go).cpu().numpy(), _moments64(po, go).cpu().numpy(), rtol=1e-6, atol=0)


def _torch_losses(x, y, bg_weight):
    """GDL_joint() and BCE_Loss(bg_weight) of loss.py:64-79,125-150 as float64 torch expressions.  The reference forms (1 + 1e-6) - p in
    float32, so the constant here is its float32 value: with the float64 one, p within ~1e-3 of 1 moves the BCE gradient by more than
    the bar."""
    n, c = x.shape[:2]
    xp, yg = x.reshape(n, c, -1)[:, 1:], y.reshape(n, c, -1)[:, 1:]
    w = 1.0 / yg.sum(dim=(0, 2))
    num = (w * ((xp * yg).sum(dim=(0, 2)) + 1)).sum()
    den = (w * ((xp * xp + yg).sum(dim=(0, 2)) + 1)).sum()
    gdl = 1.0 - 2.0 * num / den
    bce = -torch.mean(y * torch.log(x + 1e-6) + bg_weight * (1.0 - y) * torch.log(float(np.float32(1.0 + 1e-6)) - x))
    return gdl, bce


def test_fused_list_at_128_cubed_matches_float64_autograd():
    from brats2019_amd import loss as L
    p, g = _batch128(11)
    x = p.clone().requires_grad_(True)
    fused = L.fuse_criterion_list([L.GDL_joint(), L.BCE_Loss(bg_weight=1e-2)])
    loss, vals = fused([x], [g])
    (dp,) = torch.autograd.grad(loss, x)
    xd = p.double().requires_grad_(True)
    gdl, bce = _torch_losses(xd, g.double(), 1e-2)
    ref = (gdl + bce) / 2
    (dpd,) = torch.autograd.grad(ref, xd)
    np.testing.assert_allclose([float(v.detach()) for v in vals], [float(gdl.detach()), float(bce.detach())], rtol=0, atol=2e-6)
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-6
    np.testing.assert_allclose(dp.cpu().numpy(), dpd.float().cpu().numpy(), rtol=2e-5, atol=1e-9)


def test_sharded_moments_evaluate_to_the_whole_batch():
    """two half-batches: moments, totals summed (what the all-reduce does), evaluated per half -> the whole batch's values and dp"""
    from brats2019_amd import ops
    p, g = _batch128(13)
    terms = [(k, 1.0 / len(KINDS), 1.25, 0.1) for k in KINDS]
    count = float(p.numel())

    def run(pp, gg, totals=None):
        m = ops.crit_moments(pp, gg)
        tot = ops.crit_reduce(m) if totals is None else totals
        vals, coef = ops.crit_eval(tot, m, terms, count, 4)
        return m, vals, ops.crit_grad(pp, gg, coef)
    _, v_all, dp_all = run(p, g)
    halves = [(p[:2].contiguous(), g[:2].contiguous()), (p[2:].contiguous(), g[2:].contiguous())]
    totals = sum(ops.crit_reduce(ops.crit_moments(pp, gg)) for pp, gg in halves)
    outs = [run(pp, gg, totals) for pp, gg in halves]
    for _m, v, _dp in outs:
        np.testing.assert_allclose(v.cpu().numpy(), v_all.cpu().numpy(), rtol=1e-12, atol=0)
    dp_half = torch.cat([o[2] for o in outs])
    ref = dp_all.cpu().numpy()
    np.testing.assert_allclose(dp_half.cpu().numpy(), ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())
    assert torch.isfinite(dp_all).all()


def _train_two_steps(criterion, fuse, tmp_path, tag):
    from brats2019_amd import model as M, train as TR, metrics as MT
    seed, dhw = 41, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    tr = TR.Trainer(name="c" + tag, models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    tr.fuse_criteria = fuse
    losses = []

    class Rec:
        def add_scalar(self, name, val, step):
            if name.startswith("loss/"):
                losses.append(float(val))
    tr.tb_writer = Rec()
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(O.make_target(2, *dhw, seed=seed + i))]) for i in range(2)]
    tr.train(criterion=criterion, optimizer=torch.optim.Adam, optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=False, pretrained_weights=None,
             train_metrics=[MT.Dice(name="Dice")], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice", epoches=1,
             default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    w = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()
    return w, np.asarray(losses)


def test_trainer_fused_gdl_bce_equals_the_list_as_written(tmp_path):
    from brats2019_amd import loss as L
    mk = lambda: [L.GDL_joint(), L.BCE_Loss(bg_weight=1e-2)]
    w_ref, l_ref = _train_two_steps(mk(), False, tmp_path, "ref")
    w_new, l_new = _train_two_steps(mk(), True, tmp_path, "new")
    assert l_ref.shape == l_new.shape == (4,) and np.isfinite(l_new).all()
    np.testing.assert_allclose(l_new, l_ref, rtol=0, atol=2e-6)
    dw = np.abs(w_new - w_ref)
    assert dw.max() <= 2 * (1e-3 + 5e-4) + 1e-6 and dw.mean() < 1e-7, (dw.max(), dw.mean())


def test_dice_joint_with_separate_inside_hand_over_gives_the_same_parameter_gradients():
    """[Dice_loss_joint, Dice_loss_separate] evaluated as written: inside hand_over_to_network() Dice_loss_joint describes its gradient to the
    network's node while Dice_loss_separate writes its own -- the node's "somebody else also used the probabilities" branch"""
    from brats2019_amd import model as M, loss as L
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(23, **O.DEFAULT_CFG).items()})
    net.cuda().train()
    x = T(O.make_input(2, 32, 32, 32, seed=23)).cuda()
    y = T(O.make_target(2, 32, 32, 32, seed=23)).cuda()

    def grads(inside):
        for q in net.parameters():
            q.grad = None
        out = net([x])
        vals = [c(out, [y]) for c in (L.Dice_loss_joint(), L.Dice_loss_separate())]
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
