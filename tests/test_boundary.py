"""The boundary and Hausdorff-DT losses on the device (csrc/boundary.hip; ops.signed_sqdist, loss.BoundaryLoss, loss.HausdorffDTLoss)
against their host restatements (loss.signed_sqdist_host, boundary_host, hddt_host; tests/test_boundary_host.py holds those to scipy
and to float64 autograd): the maps exactly, values and gradients at bars derived from the arithmetic, sharded against whole, inside
the network's backward and inside Trainer.train.

Bars.  The map is an exact integer compare.  The device forms phi and F^alpha in float32 from the exact integer (sqrtf and powf, a
fraction of 2^-24 = 6.0e-8 each), multiplies in float64 and adds in float64; the value is returned as float32.  That bounds the value
error by a few 2^-24 of sum |term| / count and the gradient error by a few float32 ulp per element.  Every bar below is 4x the worst
figure measured on the MI355X against the float64 restatement (the convention of tests/test_hardcrit.py); each test prints its figure
before it asserts.  Gradient error is max |dp - ref| / (|ref| + 1e-4 max |ref|); value error is |value - ref| / (sum |term| / count).
A figure above about 1e-6 would be something other than rounding.  Measured worst cases are written beside each bar."""
import functools

import numpy as np
import pytest
import torch

import boundary_inputs as I
from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy

BOUNDARY_VALUE_BAR = 4 * 4.9e-8     # measured 4.9e-8 (shape C; below the float32 rounding of the returned scalar, 2^-24)
BOUNDARY_GRAD_BAR = 4 * 1.5e-7      # measured 1.5e-7 (shape A, priority 0.01: sqrtf, 1 - F and the product with float32(priority / count))
HDDT_VALUE_BAR = 4 * 5.8e-8         # measured 5.8e-8 (shape C, alpha 1)
HDDT_GRAD_BAR = 4 * 2.6e-7          # measured 2.6e-7 (shape A, alpha 2.5, priority 0.01: two powf, their sum, p - g and two products)
TRAINER_BAR = 4 * 1.5e-8            # measured 1.5e-8 of the parameters (1.2e-4 of their movement over the two steps)
ROUNDING_CEILING = 1e-6             # a measured figure above this is not rounding: a defect to find, not a bar to raise

SHAPES = [I.A, I.B, I.C]
IDS = ["A", "B", "C"]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    p, g, _names = I.make(shape)
    return p, g, T(p).cuda(), T(g).cuda()


@functools.lru_cache(maxsize=None)
def _host_maps(shape):
    from brats2019_amd import loss as L
    p, g, _pd, _gd = _inputs(shape)
    return L.signed_sqdist_host(p), L.signed_sqdist_host(g)


def _grad_err(dp, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(np.asarray(dp, dtype=np.float64) - ref) / (np.abs(ref) + 1e-4 * np.abs(ref).max())).max())


def _run(module, pd, gd):
    x = pd.clone().requires_grad_(True)
    loss = module([x], [gd])
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return float(loss.detach()), x.grad.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_signed_sqdist_is_exact(shape):
    from brats2019_amd import ops
    _p, _g, pd, gd = _inputs(shape)
    for x, ref in zip((pd, gd), _host_maps(shape)):
        got = ops.signed_sqdist(x)
        assert got.dtype == torch.int32 and got.shape == x.shape
        np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_signed_sqdist_of_a_slice_off_the_16_byte_boundary():
    from brats2019_amd import ops
    _p, _g, pd, gd = _inputs(I.A)
    for x, ref in zip((pd, gd), _host_maps(I.A)):
        part = x[1:]
        assert part.is_contiguous() and part.data_ptr() % 16 != 0
        np.testing.assert_array_equal(ops.signed_sqdist(part).cpu().numpy(), ref[1:])
        np.testing.assert_array_equal(ops.signed_sqdist(x[1, 2]).cpu().numpy(), ref[1, 2])      # a bare [D, H, W] volume


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_boundary_loss_matches_the_host_restatement(shape):
    """measured on the MI355X, worst over the priorities, value / gradient: A 2.8e-8 / 1.5e-7, B 2.5e-8 / 1.1e-7, C 4.9e-8 / 9.6e-8"""
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(shape)
    worst_v = worst_g = 0.0
    for priority in (1, 0.01):
        value, dp = _run(L.BoundaryLoss(priority=priority), pd, gd)
        ref_v, ref_dp = L.boundary_host(p, g, priority)
        scale = float((np.abs(p.astype(np.float64)) * np.abs(ref_dp)).sum())            # sum |term| / count
        ev, eg = abs(value - ref_v) / scale, _grad_err(dp, ref_dp)
        print("boundary %s priority=%s: value %.9g (host %.9g), value err %.3e, gradient err %.3e" % (shape, priority, value, ref_v, ev, eg))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    assert max(BOUNDARY_VALUE_BAR, BOUNDARY_GRAD_BAR) < 4 * ROUNDING_CEILING
    assert worst_v <= BOUNDARY_VALUE_BAR and worst_g <= BOUNDARY_GRAD_BAR, (worst_v, worst_g)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_hausdorff_dt_loss_matches_the_host_restatement(shape):
    """measured on the MI355X, worst over alpha in (1, 2, 2.5) and the priorities, value / gradient: A 3.1e-8 / 2.6e-7, B 3.9e-8 / 1.6e-7,
    C 5.8e-8 / 2.3e-7"""
    from brats2019_amd import loss as L
    p, g, pd, gd = _inputs(shape)
    worst_v = worst_g = 0.0
    for alpha in I.ALPHAS:
        for priority in (1, 0.01):
            value, dp = _run(L.HausdorffDTLoss(alpha=alpha, priority=priority), pd, gd)
            ref_v, ref_dp = L.hddt_host(p, g, alpha, priority)
            ev, eg = abs(value - ref_v) / abs(ref_v), _grad_err(dp, ref_dp)                 # every term has the value's sign
            print("hddt %s alpha=%s priority=%s: value %.9g (host %.9g), value err %.3e, gradient err %.3e" % (shape, alpha, priority, value, ref_v, ev, eg))
            worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    assert max(HDDT_VALUE_BAR, HDDT_GRAD_BAR) < 4 * ROUNDING_CEILING
    assert worst_v <= HDDT_VALUE_BAR and worst_g <= HDDT_GRAD_BAR, (worst_v, worst_g)


def test_boundary_loss_has_the_sign_of_the_side():
    from brats2019_amd import loss as L
    for shape in SHAPES:
        _p, g, _pd, _gd = _inputs(shape)
        gh = T(I.hard(g)).cuda()
        on, _ = _run(L.BoundaryLoss(), gh, gh)
        off, _ = _run(L.BoundaryLoss(), 1.0 - gh, gh)
        print("boundary %s: p = g gives %.6g, p = 1 - g gives %.6g" % (shape, on, off))
        assert on <= 0 < off
        if shape == I.A:
            assert on < 0


def test_hausdorff_dt_loss_of_the_target_is_exactly_zero():
    from brats2019_amd import loss as L
    for shape in SHAPES:
        _p, g, _pd, _gd = _inputs(shape)
        gh = T(I.hard(g)).cuda()
        for alpha in I.ALPHAS:
            value, dp = _run(L.HausdorffDTLoss(alpha=alpha), gh, gh)
            assert value == 0.0 and not dp.any()


def test_two_calls_give_identical_bytes():
    from brats2019_amd import ops
    _p, _g, pd, gd = _inputs(I.A)
    runs = []
    for _ in range(2):
        s_p, s_g = ops.signed_sqdist(pd), ops.signed_sqdist(gd)
        out = [s_p, s_g, ops.boundary_sum(pd, s_g), ops.boundary_grad(s_g, 0.25 / pd.numel())]
        for alpha in I.ALPHAS:
            out += [ops.hddt_sum(pd, gd, s_p, s_g, alpha), ops.hddt_grad(pd, gd, s_p, s_g, alpha, 0.25 / pd.numel())]
        runs.append([v.cpu().numpy().tobytes() for v in out])
    assert runs[0] == runs[1]


def test_sharded_sums_evaluate_to_the_whole_batch():
    """two half-batches: the sums added (what the all-reduce does) and the gradients per half with the global count -> the whole batch.
    The maps are per sample, so a half's map is the whole's slice.  The second half starts 8 bytes past a 16-byte boundary: with freshly
    made maps the pointers of a pass disagree (everything one by one), with slices of the whole's maps they agree (a head of two)."""
    from brats2019_amd import ops
    _p, _g, pd, gd = _inputs(I.A)
    s_p, s_g = ops.signed_sqdist(pd), ops.signed_sqdist(gd)
    assert pd[1:].is_contiguous() and pd[1:].data_ptr() % 16 == 8
    coef = 0.7 / pd.numel()
    for fresh in (True, False):
        halves = []
        for a in (slice(0, 1), slice(1, 2)):
            hp, hg = (ops.signed_sqdist(pd[a]), ops.signed_sqdist(gd[a])) if fresh else (s_p[a], s_g[a])
            assert torch.equal(hp, s_p[a]) and torch.equal(hg, s_g[a])
            if a.start == 1:
                assert fresh == (hp.data_ptr() % 16 != pd[a].data_ptr() % 16)
            halves.append((pd[a], gd[a], hp, hg))
        whole = ops.boundary_sum(pd, s_g).cpu().numpy()
        parts = sum(ops.boundary_sum(a, d) for a, _b, _c, d in halves).cpu().numpy()
        scale = float((pd.double() * ops.boundary_grad(s_g, 1.0).double()).abs().sum())
        assert abs(parts[0] - whole[0]) <= 1e-12 * scale
        ref = ops.boundary_grad(s_g, coef).cpu().numpy()
        got = torch.cat([ops.boundary_grad(d, coef) for _a, _b, _c, d in halves]).cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())
        for alpha in I.ALPHAS:
            whole = ops.hddt_sum(pd, gd, s_p, s_g, alpha).cpu().numpy()
            parts = sum(ops.hddt_sum(a, b, c, d, alpha) for a, b, c, d in halves).cpu().numpy()
            np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0)
            ref = ops.hddt_grad(pd, gd, s_p, s_g, alpha, coef).cpu().numpy()
            got = torch.cat([ops.hddt_grad(a, b, c, d, alpha, coef) for a, b, c, d in halves]).cpu().numpy()
            np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0


@pytest.mark.parametrize("members", [("Dice_loss_joint", "BoundaryLoss"), ("HausdorffDTLoss", "FocalLoss")], ids=lambda m: "+".join(m))
def test_lists_inside_hand_over_give_the_same_parameter_gradients(members):
    """evaluated as written: inside hand_over_to_network() Dice_loss_joint describes its gradient to the network's node while the new
    classes write theirs -- the bars of tests/test_hardcrit.py's test of the same name"""
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


class _TorchBoundary(torch.nn.Module):
    """BoundaryLoss as float32 torch ops with autograd on ops.signed_sqdist's map: the reference of the Trainer comparison"""

    def __init__(self, priority):
        super().__init__()
        self.priority = priority

    def forward(self, x, y):
        from brats2019_amd import ops
        s = ops.signed_sqdist(y[0])
        F = s.abs().float().sqrt()
        phi = torch.where(s > 0, F, torch.where(s < 0, 1.0 - F, torch.zeros_like(F)))
        return self.priority * (x[0] * phi).mean()


class _TorchHausdorffDT(torch.nn.Module):
    """HausdorffDTLoss(alpha=2) as float32 torch ops with autograd on ops.signed_sqdist's maps"""

    def __init__(self, priority):
        super().__init__()
        self.priority = priority

    def forward(self, x, y):
        from brats2019_amd import ops
        w = ops.signed_sqdist(x[0].detach()).abs().float() + ops.signed_sqdist(y[0]).abs().float()
        return self.priority * ((x[0] - y[0]) ** 2 * w).mean()


def _train(tmp_path, name, criterion):
    from brats2019_amd import model as M, train as TR, metrics as MT
    seed, dhw = 43, (32, 32, 32)
    net = M.UNet(**O.DEFAULT_CFG)
    net.load_state_dict({k: T(v) for k, v in O.make_params(seed, **O.DEFAULT_CFG).items()})
    w0 = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).clone()
    tr = TR.Trainer(name=name, models_root=str(tmp_path), model=net, rewrite=True, connect_tb=False)
    losses = []

    class Rec:
        def add_scalar(self, name, val, step):
            if name.startswith("loss/"):
                losses.append(float(val))
    tr.tb_writer = Rec()
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(O.make_target(2, *dhw, seed=seed + i))]) for i in range(2)]
    tr.train(criterion=criterion, optimizer=torch.optim.SGD, optimizer_params=dict(lr=1e-2),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=False, pretrained_weights=None,
             train_metrics=[MT.Dice(name="Dice")], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice", epoches=1,
             default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    w1 = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).cpu().double().numpy()
    return w0.cpu().double().numpy(), w1, np.asarray(losses)


def test_trainer_runs_with_the_new_criteria_and_matches_torch_ops(tmp_path):
    """One epoch of two SGD steps with [Dice_loss_joint(), BoundaryLoss(0.01), HausdorffDTLoss(0.01)], and the same with the two new
    criteria replaced by torch-op modules on the same maps.  Measured on the MI355X: relative L2 of the final parameters between the
    two runs 1.5e-8, of the parameters' movement 1.2e-4; the bar is 4x the former."""
    from brats2019_amd import loss as L
    w0, w_dev, l_dev = _train(tmp_path, "boundary", [L.Dice_loss_joint(), L.BoundaryLoss(priority=0.01), L.HausdorffDTLoss(priority=0.01)])
    assert l_dev.shape == (6,) and np.isfinite(l_dev).all()                               # three criteria x two steps
    assert np.isfinite(w_dev).all() and not np.array_equal(w_dev, w0)
    _w0, w_ref, l_ref = _train(tmp_path, "boundary_torch", [L.Dice_loss_joint(), _TorchBoundary(0.01), _TorchHausdorffDT(0.01)])
    rel = float(np.linalg.norm(w_dev - w_ref) / np.linalg.norm(w_ref))
    moved = float(np.linalg.norm(w_dev - w_ref) / np.linalg.norm(w_ref - w0))
    print("trainer: losses %s (torch ops %s); relative L2 of the parameters %.3e, of their movement %.3e" % (l_dev, l_ref, rel, moved))
    assert np.linalg.norm(w_ref - w0) > 0
    assert rel <= TRAINER_BAR, rel
