"""The lesion-wise Dice loss on the device (csrc/lesion_loss.hip; ops.lesion_loss_forward / _grad / _table, loss.LesionWiseDiceLoss)
against its host restatement (loss.lesion_dice_host, which tests/test_lesion_loss_host.py holds to float64 autograd on scipy's labels):
the labelling, the per-lesion volumes and the 64-bit fixed-point sums EXACTLY, the value and the gradient at bars derived from the
arithmetic, through autograd, and inside Trainer.train.

Bars.  The integers are compared with assert_array_equal.  Value: both sides do the same float64 arithmetic on the same integers; only
the order of the float64 additions over the lesions differs (the device adds lane by lane, the host in ascending root order), a few
2^-53 per lesion: 1e-12 relative (measured on the MI355X: 0 in all twelve cases, every value bit for bit the host's).  Gradient: float64
arithmetic rounded once to float32, so max |dp - ref| / (|ref| + 1e-4 max |ref|) is bounded by half an ulp, 2^-24 = 5.96e-8; measured
5.25e-8 .. 5.91e-8 over the twelve cases.  The bar is 4x the worst measured figure (the convention of tests/test_boundary.py).  Each
test prints its figure before it asserts."""
import functools

import numpy as np
import pytest
import torch

import lesion_loss_inputs as I
from oracle import resunet_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy

VALUE_BAR = 1e-12                   # measured 0 (all cases)
GRAD_BAR = 4 * 5.91e-8              # measured 5.91e-8 (shapes A and C): the one rounding to float32
TRAINER_BAR = 4 * 1.2e-9            # measured 1.2e-9 of the parameters (7.4e-5 of their movement over the two steps)
ROUNDING_CEILING = 1e-6             # a measured figure above this is not rounding: a defect to find, not a bar to raise

CASES = [(s, d, m) for s in "ABCD" for d, m in ((0, 0), (3, 0), (2, 1))]
IDS = ["%s-dil%d-min%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(shape_id):
    p, g, names = I.make(I.SHAPES[shape_id])
    return p, g, T(p).cuda(), T(g).cuda(), names


@functools.lru_cache(maxsize=None)
def _host(shape_id, dilation, min_volume, priority=0.7):
    from brats2019_amd import loss as L
    p, g = _inputs(shape_id)[:2]
    return L.lesion_dice_host(p, g, priority, dilation, min_volume, quantised=True)


@functools.lru_cache(maxsize=None)
def _device(shape_id, dilation, min_volume, priority=0.7):
    from brats2019_amd import ops
    _p, _g, pd, gd, _ = _inputs(shape_id)
    totals, stats, labels, state = ops.lesion_loss_forward(pd, gd, dilation, min_volume)
    dp = ops.lesion_loss_grad(pd, gd, labels, state, totals, priority)
    return totals, stats, labels, state, dp


def _grad_err(dp, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(np.asarray(dp, dtype=np.float64) - ref) / (np.abs(ref) + 1e-4 * np.abs(ref).max())).max())


def _value(totals, priority):
    t = totals.cpu().numpy()
    return priority * (t[0] / t[1]) if t[1] else 0.0


def test_inputs_hold_the_constructed_lesions():
    from brats2019_amd import loss as L
    g = I.make(I.D)[1]
    for dilation, n in ((0, 3), (2, 3), (3, 2)):                      # straddle + corner: the two boxes join at dilation 3 only
        assert len(L.lesion_labels_host(g[0, 0], dilation)[1]) == n
    g = I.make(I.B)[1]
    assert len(L.lesion_labels_host(g[0, 0], 0)[1]) == 2              # the corner voxel, and the two voxels that touch at a corner
    g = I.make(I.A)[1]
    assert len(L.lesion_labels_host(g[0, 1], 0)[1]) > 100 and not (g[0, 2] > 0.5).any() and (g[1, 0] > 0.5).all()
    assert ((g[1, 2] > 0) & (g[1, 2] < 1)).any()                      # a soft channel


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_volumes_and_integer_sums_are_exact(case):
    from brats2019_amd import ops
    _v, _grad, table = _host(*case)
    totals, stats, labels, state, _dp = _device(*case)
    dev = ops.lesion_loss_table(labels, state)
    lab = labels.cpu().numpy()
    st = stats.cpu().numpy()
    g = _inputs(case[0])[1]
    for n, row in enumerate(table):
        for c, h in enumerate(row):
            d = dev[n][c]
            np.testing.assert_array_equal(lab[n, c], h["labels"])     # the partition, the roots, and -1 exactly outside G
            assert ((lab[n, c] == -1) == ~(g[n, c] > np.float32(0.5))).all()
            for key in ("root", "vol", "qI", "qU"):
                assert d[key].dtype == np.int64
                np.testing.assert_array_equal(d[key], h[key], err_msg="%s of (%d, %d)" % (key, n, c))
            assert (d["qI0"], d["qU0"]) == (h["qI0"], h["qU0"])
            assert list(st[n, c]) == [len(h["root"]), int(h["kept"].sum())]
    kept_pairs = sum(1 for row in table for h in row if h["kept"].any())
    assert totals.cpu().numpy()[1] == kept_pairs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_value_and_gradient_match_the_host_restatement(case):
    v, grad, table = _host(*case)
    totals, _stats, _labels, _state, dp = _device(*case)
    dv = _value(totals, 0.7)
    verr = abs(dv - v) / abs(v)
    gerr = _grad_err(dp.cpu().numpy(), grad)
    print("%s: value %.17g (host %.17g), relative error %.3e; gradient error %.3e" % (IDS[CASES.index(case)], dv, v, verr, gerr))
    assert np.isfinite(dp.cpu().numpy()).all() and np.abs(grad).max() > 0
    assert verr <= VALUE_BAR, verr
    assert gerr <= ROUNDING_CEILING, gerr
    assert gerr <= GRAD_BAR, gerr
    for n, row in enumerate(table):                                   # the voxels of a dropped lesion: exact zeros
        for c, h in enumerate(row):
            for root in h["root"][~h["kept"]]:
                assert not dp[n, c].cpu().numpy()[h["labels"] == root].any()


def test_two_calls_give_identical_bytes():
    from brats2019_amd import ops
    _p, _g, pd, gd, _ = _inputs("A")
    outs = []
    for _ in range(2):
        totals, stats, labels, state = ops.lesion_loss_forward(pd, gd, 3, 1)
        dp = ops.lesion_loss_grad(pd, gd, labels, state, totals, 0.7)
        outs.append([t.cpu().numpy().copy() for t in (totals, stats, labels, dp)])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape_id", ["A", "D"])
def test_through_autograd(shape_id):
    """LesionWiseDiceLoss(...)([p], [g]).backward() is the op's dp times gout, for a unit and a non-unit gout and for a prediction that is
    a slice starting 8 bytes off a 16-byte boundary (then every element goes one by one)."""
    from brats2019_amd import loss as L, ops
    _p, _g, pd, gd, _ = _inputs(shape_id)
    totals, _stats, labels, state, dp = _device(shape_id, 3, 0)
    module = L.LesionWiseDiceLoss(priority=0.7)
    x = pd.clone().requires_grad_(True)
    out = module([x], [gd])
    assert out.dim() == 0 and out.dtype == torch.float32
    assert float(out.detach()) == float(np.float32(_value(totals, 0.7)))
    out.backward()
    assert x.grad.cpu().numpy().tobytes() == dp.cpu().numpy().tobytes()
    x3 = pd.clone().requires_grad_(True)
    (module([x3], [gd]) * 3).backward()
    three = torch.tensor(3.0, device="cuda")
    np.testing.assert_array_equal(x3.grad.cpu().numpy(), ops.lesion_loss_grad(pd, gd, labels, state, totals, 0.7, three).cpu().numpy())
    np.testing.assert_allclose(x3.grad.cpu().numpy(), 3 * dp.cpu().numpy(), rtol=2.0 ** -22, atol=0)
    buf = torch.zeros(pd.numel() + 6, dtype=torch.float32, device="cuda")
    off = (-buf.data_ptr() // 4) % 4 + 2                              # elements to the next 16-byte boundary, plus 8 bytes
    xs = buf[off:off + pd.numel()].view(pd.shape)
    xs.copy_(pd)
    assert xs.data_ptr() % 16 == 8 and xs.is_contiguous()
    xs.requires_grad_(True)
    module([xs], [gd]).backward()
    assert xs.grad.cpu().numpy().tobytes() == dp.cpu().numpy().tobytes()


def test_no_lesion_is_exactly_zero():
    from brats2019_amd import loss as L
    rng = np.random.default_rng(3)
    g = (0.45 * rng.random((2, 2, 5, 6, 70))).astype(np.float32)
    g[1, 1, 2, 3, 60:66] = 1.0                                        # one lesion of 6 voxels ...
    x = T(I.predict(g, rng)).cuda().requires_grad_(True)
    out = L.LesionWiseDiceLoss(min_volume=6)([x], [T(g).cuda()])       # ... which is dropped
    out.backward()
    assert float(out) == 0.0 and not x.grad.cpu().numpy().any()
    g[:] = 0
    x.grad = None
    out = L.LesionWiseDiceLoss()([x], [T(g).cuda()])
    out.backward()
    assert float(out) == 0.0 and not x.grad.cpu().numpy().any()


def test_one_lesion_agrees_with_dice_loss_joint():
    """N = C = 1 and one lesion: the domain is the whole volume, so the loss is Dice_loss_joint's -- within the float32 of that
    criterion's returned value and written gradient (its sums are float64 as well)."""
    from brats2019_amd import loss as L
    rng = np.random.default_rng(4)
    g = np.zeros((1, 1, 9, 10, 70), dtype=np.float32)
    g[0, 0, 2:6, 3:8, 50:68] = 1.0
    p = I.predict(g, rng)
    outs = []
    for module in (L.LesionWiseDiceLoss(priority=1), L.Dice_loss_joint(priority=1)):
        x = T(p).cuda().requires_grad_(True)
        out = module([x], [T(g).cuda()])
        out.backward()
        outs.append((float(out), x.grad.cpu().numpy()))
    (v, dv), (r, dr) = outs
    print("one lesion: %.9g, Dice_loss_joint %.9g; gradient error %.3e" % (v, r, _grad_err(dv, dr)))
    assert abs(v - r) <= 2.0 ** -23 * abs(r)
    assert _grad_err(dv, dr) <= 1e-6


class _TorchLesionDice(torch.nn.Module):
    """LesionWiseDiceLoss as float32 torch ops with autograd on loss.lesion_dice_host's labelling: the reference of the Trainer comparison"""

    def __init__(self, priority, dilation, min_volume=0):
        super().__init__()
        self.priority, self.dilation, self.min_volume = priority, dilation, min_volume

    def forward(self, x, y):
        from brats2019_amd import loss as L
        p, g = x[0], y[0]
        gh = g.detach().cpu().numpy()
        pair_losses = []
        for n in range(p.shape[0]):
            for c in range(p.shape[1]):
                labels, roots = L.lesion_labels_host(gh[n, c], self.dilation)
                lab = T(labels).to(p.device)
                dices = []
                for root in roots:
                    if int((labels == root).sum()) <= self.min_volume:
                        continue
                    mask = ((lab == -1) | (lab == int(root))).to(p.dtype)
                    inter, union = (p[n, c] * g[n, c] * mask).sum(), ((p[n, c] ** 2 + g[n, c]) * mask).sum()
                    dices.append(2 * (inter + 1e-6) / (union + 2e-6))
                if dices:
                    pair_losses.append(1 - sum(dices) / len(dices))
        if not pair_losses:
            return p.sum() * 0
        return self.priority * sum(pair_losses) / len(pair_losses)


def _train(tmp_path, name, criterion):
    from brats2019_amd import model as M, train as TR, metrics as MT
    seed, dhw = 47, (32, 32, 32)
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
    loader = [([T(O.make_input(2, *dhw, seed=seed + i))], [T(I.blob_targets(2, dhw, seed + i))]) for i in range(2)]
    tr.train(criterion=criterion, optimizer=torch.optim.SGD, optimizer_params=dict(lr=1e-2),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[loader[1]], split_into_tiles=False, pretrained_weights=None,
             train_metrics=[MT.Dice(name="Dice")], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice", epoches=1,
             default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    w1 = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).cpu().double().numpy()
    return w0.cpu().double().numpy(), w1, np.asarray(losses)


def test_trainer_matches_torch_ops_on_the_host_labelling(tmp_path):
    """One epoch of two SGD steps at 32^3, batch 2, with [Dice_loss_joint(), LesionWiseDiceLoss(priority=0.5, dilation=1)], every target
    channel holding four separate boxes, and the same with the second criterion written as float32 torch ops on lesion_dice_host's
    labelling.  Measured on the MI355X: relative L2 of the final parameters between the two runs 1.2e-9, of the parameters' movement
    7.4e-5 (BoundaryLoss's entry: 1.5e-8 and 1.2e-4); the bar is 4x the former."""
    from brats2019_amd import loss as L
    for i in range(2):
        g = I.blob_targets(2, (32, 32, 32), 47 + i)
        assert all(len(L.lesion_labels_host(g[n, c], 1)[1]) >= 3 for n in range(2) for c in range(3))
    w0, w_dev, l_dev = _train(tmp_path, "lesion", [L.Dice_loss_joint(), L.LesionWiseDiceLoss(priority=0.5, dilation=1)])
    assert l_dev.shape == (4,) and np.isfinite(l_dev).all()                               # two criteria x two steps
    assert np.isfinite(w_dev).all() and not np.array_equal(w_dev, w0)
    _w0, w_ref, l_ref = _train(tmp_path, "lesion_torch", [L.Dice_loss_joint(), _TorchLesionDice(0.5, 1)])
    rel = float(np.linalg.norm(w_dev - w_ref) / np.linalg.norm(w_ref))
    moved = float(np.linalg.norm(w_dev - w_ref) / np.linalg.norm(w_ref - w0))
    print("trainer: losses %s (torch ops %s); relative L2 of the parameters %.3e, of their movement %.3e" % (l_dev, l_ref, rel, moved))
    assert np.linalg.norm(w_ref - w0) > 0
    np.testing.assert_allclose(l_dev, l_ref, rtol=1e-5)
    assert rel <= TRAINER_BAR, rel
