"""CPU-side checks of the optimisation recipe (brats2019_amd/optim.py, csrc/optim.hip): the float64 numpy restatements of the kernels' formulas
against torch's own CPU optimizers and clip_grad_norm_, PolyLR against its closed form, state_dict interchange with the torch classes, and
the argument checks of the classes and of the C entries (none of which touches a GPU)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from brats2019_amd import optim

SHAPES = [(5, 3), (7,), (2, 3, 4)]


def _tensors(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [scale * rng.standard_normal(s) for s in SHAPES]


SGD_VARIANTS = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "dampening": dict(momentum=0.9, dampening=0.3),
    "nesterov": dict(momentum=0.99, nesterov=True),
    "weight_decay": dict(momentum=0.9, weight_decay=0.05),
    "weight_decay_plain": dict(weight_decay=0.05),
}


@pytest.mark.parametrize("variant", sorted(SGD_VARIANTS))
def test_sgd_restatement_equals_torch_sgd_in_float64(variant):
    kw = SGD_VARIANTS[variant]
    ws = _tensors(1)
    params = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in ws]
    opt = torch.optim.SGD(params, lr=0.1, **kw)
    bufs = [None] * len(ws)
    for step in range(3):
        gs = _tensors(10 + step)
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, g in enumerate(gs):
            ws[i], bufs[i] = optim.sgd_step_host(ws[i], g, bufs[i], 0.1, **kw)
            np.testing.assert_allclose(ws[i], params[i].detach().numpy(), rtol=1e-12, atol=1e-12)
            if kw.get("momentum"):
                np.testing.assert_allclose(bufs[i], opt.state[params[i]]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-12)
            else:
                assert bufs[i] is None


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("decoupled", [True, False])
def test_adamw_restatement_equals_torch_in_float64(amsgrad, decoupled):
    """decoupled: torch.optim.AdamW; not decoupled: torch.optim.Adam (L2 decay added to the gradient)"""
    hp = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1)
    ws = _tensors(2)
    params = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in ws]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(params, amsgrad=amsgrad, **hp)
    ms, vs = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
    vms = [np.zeros_like(w) if amsgrad else None for w in ws]
    for step in range(1, 4):
        gs = _tensors(20 + step)
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, g in enumerate(gs):
            ws[i], ms[i], vs[i], vms[i] = optim.adamw_step_host(ws[i], g, ms[i], vs[i], vms[i], hp["lr"], 0.9, 0.99, hp["eps"], hp["weight_decay"], decoupled, step)
            st = opt.state[params[i]]
            np.testing.assert_allclose(ws[i], params[i].detach().numpy(), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(ms[i], st["exp_avg"].numpy(), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(vs[i], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-12)
            if amsgrad:
                np.testing.assert_allclose(vms[i], st["max_exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("max_norm", [0.5, 12.0, 1e6])
def test_clip_restatement_equals_torch_clip_grad_norm_in_float64(max_norm):
    gs = _tensors(3, scale=2.0)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy())
    params.append(torch.nn.Parameter(torch.zeros(3, dtype=torch.float64)))          # a parameter without a gradient is skipped
    want = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef = optim.clip_coef_host(gs, max_norm)
    assert abs(norm - want) <= 1e-12 * want
    assert (coef < 1.0) == (max_norm < want)
    for p, g in zip(params, gs):
        np.testing.assert_allclose(coef * g, p.grad.numpy(), rtol=1e-12, atol=1e-12)
    # the coefficient folded into the step equals a step on the clipped gradients
    w = _tensors(4)[0]
    a, _ = optim.sgd_step_host(w, gs[0], None, 0.1, momentum=0.9, nesterov=True, coef=coef)
    b, _ = optim.sgd_step_host(w, coef * gs[0], None, 0.1, momentum=0.9, nesterov=True)
    np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)
    nan_norm, nan_coef = optim.clip_coef_host([np.array([1.0, np.nan])], max_norm)
    assert np.isnan(nan_norm) and np.isnan(nan_coef)                                   # no skip policy: as torch with error_if_nonfinite=False


def test_ema_restatement():
    e, w = _tensors(5)[0], _tensors(6)[0]
    np.testing.assert_array_equal(optim.ema_host(e, w, 0.0), w)
    np.testing.assert_array_equal(optim.ema_host(e, w, 1.0), e)
    np.testing.assert_allclose(optim.ema_host(e, w, 0.9), 0.9 * e + 0.1 * w, rtol=1e-15)


def test_polylr_follows_the_closed_form_and_clamps_at_zero():
    p = [torch.nn.Parameter(torch.zeros(2))]
    opt = torch.optim.SGD([dict(params=p, lr=0.01), dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=0.5)], lr=0.01)
    sch = optim.PolyLR(opt, max_steps=10, exponent=0.9)
    assert isinstance(sch, torch.optim.lr_scheduler.LRScheduler)
    for step in range(14):
        frac = max(0.0, 1.0 - step / 10)
        for g, base in zip(opt.param_groups, (0.01, 0.5)):
            assert g["lr"] == pytest.approx(base * frac ** 0.9, rel=1e-15, abs=0), step
        assert (opt.param_groups[0]["lr"] == 0.0) == (step >= 10)
        opt.step()
        sch.step()
    sch.resume_at(4)                                        # a closed form of the count: continuing at a step is setting the count
    assert sch.last_epoch == 4 and opt.param_groups[1]["lr"] == pytest.approx(0.5 * 0.6 ** 0.9, rel=1e-15)
    assert sch.get_last_lr() == [g["lr"] for g in opt.param_groups]
    with pytest.raises(ValueError):
        optim.PolyLR(opt, max_steps=0)


def _same_state(a, b):
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys()
        for name, v in a["state"][k].items():
            w = b["state"][k][name]
            assert (v is None and w is None) or torch.equal(torch.as_tensor(v), torch.as_tensor(w)), (k, name)


@pytest.mark.parametrize("kind", ["sgd", "sgd_plain", "adamw", "adamw_amsgrad"])
def test_state_dict_interchanges_with_the_torch_classes(kind):
    """torch -> ours -> torch: the state loads into this module's class, comes out of its state_dict() unchanged (torch's layout: momentum_buffer;
    step, exp_avg, exp_avg_sq[, max_exp_avg_sq]) and continues under a fresh torch optimizer exactly as the one that never stopped."""
    if kind.startswith("sgd"):
        kw = dict(lr=0.1, momentum=0.9, nesterov=True) if kind == "sgd" else dict(lr=0.1)
        tcls, ocls = torch.optim.SGD, optim.SGD
    else:
        kw = dict(lr=1e-2, weight_decay=0.1, amsgrad=kind.endswith("amsgrad"))
        tcls, ocls = torch.optim.AdamW, optim.AdamW

    def make():
        return [torch.nn.Parameter(torch.from_numpy(w.astype(np.float32))) for w in _tensors(7)]

    def give(params, step):
        for p, g in zip(params, _tensors(30 + step)):
            p.grad = torch.from_numpy(g.astype(np.float32))
    pa = make()
    a = tcls(pa, **kw)
    for step in range(2):
        give(pa, step)
        a.step()
    po = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ours = ocls(po, **kw)
    ours.load_state_dict(copy.deepcopy(a.state_dict()))       # (load_state_dict keeps tensors that need no cast: a copy, so that `a` can go on alone)
    _same_state(ours.state_dict(), a.state_dict())
    if kind == "sgd":
        assert all(set(v) == {"momentum_buffer"} for v in ours.state_dict()["state"].values())
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    b = tcls(pb, **kw)
    b.load_state_dict(copy.deepcopy(ours.state_dict()))
    give(pa, 2), give(pb, 2)
    a.step(), b.step()
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    # a CPU step of this module's class is refused, it does not fall back
    give(po, 2)
    with pytest.raises(RuntimeError):
        ours.step()


def test_argument_checks_of_the_classes():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1.0), dict(lr=0.1, nesterov=True),
                dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            optim.SGD(p, **bad)
        with pytest.raises(ValueError):
            torch.optim.SGD(p, **bad)                       # torch's validation refuses the same
    with pytest.raises(NotImplementedError):
        optim.SGD(p, lr=0.1, maximize=True)
    optim.SGD(p, lr=0.1, maximize=False, foreach=None, fused=None)
    with pytest.raises(NotImplementedError):
        optim.AdamW(p, maximize=True)
    with pytest.raises(NotImplementedError):
        optim.Adam(p, decoupled_weight_decay=True)             # that is optim.AdamW
    with pytest.raises(ValueError):
        optim.AdamW(p, betas=(1.0, 0.9))
    assert optim.AdamW(p).defaults["weight_decay"] == 1e-2 and isinstance(optim.AdamW(p), optim.Adam)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(p, -1.0)
    assert float(optim.clip_grad_norm_(p, 1.0)) == 0.0        # no gradient at all: torch returns 0 too
    p[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        optim.clip_grad_norm_(p, 1.0)
    with pytest.raises(ValueError):
        optim.EMA(torch.nn.Linear(2, 2), 1.5)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        optim.EMA(torch.nn.Linear(2, 2), 0.9)


@pytest.fixture(scope="module")
def lib():
    from brats2019_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from brats2019_amd import build
        build.build(verbose=False)
    return L.load()


def test_argument_errors_of_the_entries_are_reported_before_any_launch(lib):
    one, two, three = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(2 << 20)      # never dereferenced by a failing check
    err = lambda: lib.ru_last_error()
    assert lib.ru_sgd_step(None, None, None, 4, 0.1, 0.0, 0.0, 0.0, 0, 0, None, None) < 0 and b"ru_sgd_step" in err()
    assert lib.ru_sgd_step(one, two, None, 4, 0.1, 0.9, 0.0, 0.0, 0, 0, None, None) < 0 and b"momentum buffer" in err()
    assert lib.ru_sgd_step(one, two, three, 4, 0.1, 0.0, 0.0, 0.0, 0, 0, None, None) < 0 and b"momentum buffer" in err()
    assert lib.ru_sgd_step(one, two, three, 4, 0.1, 0.9, 0.1, 0.0, 1, 0, None, None) < 0 and b"Nesterov" in err()
    assert lib.ru_sgd_step(one, C.c_void_p(4096 + 8), None, 4, 0.1, 0.0, 0.0, 0.0, 0, 0, None, None) < 0 and b"overlap" in err()
    assert lib.ru_sgd_step(C.c_void_p(4097), two, None, 4, 0.1, 0.0, 0.0, 0.0, 0, 0, None, None) < 0 and b"misaligned" in err()
    assert lib.ru_adamw_step(one, two, three, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, None) < 0 and b"ru_adamw_step" in err()
    assert lib.ru_adamw_step(one, two, three, C.c_void_p(3 << 20), None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, None, None) < 0 and b"1-based" in err()
    assert lib.ru_adamw_step(one, two, three, three, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, None) < 0 and b"overlap" in err()
    assert lib.ru_ema_update(one, two, 4, 1.5, None) < 0 and b"[0, 1]" in err()
    assert lib.ru_ema_update(one, one, 4, 0.5, None) < 0 and b"overlap" in err()
    assert lib.ru_swap_f32(one, None, 4, None) < 0 and lib.ru_swap_f32(one, C.c_void_p(4096 + 12), 4, None) < 0 and b"overlap" in err()
    assert lib.ru_scale_by(one, 4, None, None) < 0 and b"ru_scale_by" in err()
    assert lib.ru_gradnorm_partial(one, 4, 0, None, 0, None) < 0
    assert lib.ru_gradnorm_partial(one, 4, 3, two, 3 * 8, None) < 0 and b"workspace too small" in err()
    assert lib.ru_gradnorm_finalize(two, 1, -1.0, one, three, None) < 0 and b"max_norm" in err()
    assert lib.ru_gradnorm_finalize(two, 1, 1.0, None, three, None) < 0
    # empty runs are accepted and launch nothing
    assert lib.ru_sgd_step(one, two, None, 0, 0.1, 0.0, 0.0, 0.0, 0, 0, None, None) == 0 and lib.ru_swap_f32(one, two, 0, None) == 0
    assert lib.ru_gradnorm_partial(one, 0, 0, two, 0, None) == 0


def test_gradnorm_slot_bookkeeping(lib):
    """one float64 slot per workgroup: the count is a function of the run's length alone, capped by the grid cap, and the workspace bound covers
    every split of the network's 4,509,939 live floats into runs"""
    slots = lambda n: int(lib.ru_gradnorm_slots(n))
    assert slots(0) == 0 and slots(1) == 1 and slots(1024) == 2 and slots(1 << 40) == slots(1 << 30)
    cap = slots(1 << 30)
    assert cap == 2048 and slots((1 << 21) + 4099) == cap                  # tests/test_optim_recipe.py's longest run is past one sweep of the capped grid
    assert all(slots(n) <= slots(n + 1) for n in (1, 3, 1011, 1012, 1013, 4099, 1 << 21))
    rng = np.random.default_rng(0)
    for runs in (1, 3, 86, 1000):
        cuts = np.sort(rng.integers(1, 4509939, runs - 1))
        lens = np.diff(np.concatenate([[0], cuts, [4509939]]))
        lens = lens[lens > 0]
        assert 8 * sum(slots(int(n)) for n in lens) <= int(lib.ru_gradnorm_workspace_bytes(4509939, len(lens)))
    assert 8 * 7 * slots(1) <= int(lib.ru_gradnorm_workspace_bytes(7, 7))


def test_trainer_maps_adamw_and_keeps_the_options_off_by_default(tmp_path):
    from brats2019_amd import train as TR, model as M
    cfg = dict(depth=2, encoder_layers=[1, 1], decoder_layers=[1, 1], number_of_channels=[8, 16], number_of_outputs=3)
    tr = TR.Trainer(name="o", models_root=str(tmp_path), model=M.UNet(**cfg), rewrite=True, connect_tb=False)
    assert tr.clip_grad_norm is None and tr.ema_decay is None and not hasattr(tr.state, "ema_state")
    opt, sch = tr._make_optimizer(torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.05), optim.PolyLR, dict(max_steps=100))
    assert type(opt) is optim.AdamW and isinstance(sch, optim.PolyLR)
    opt, _ = tr._make_optimizer(torch.optim.Adam, dict(lr=1e-3), None, None)
    assert type(opt) is optim.Adam
    opt, _ = tr._make_optimizer(optim.SGD, dict(lr=1e-2, momentum=0.99, nesterov=True), None, None)
    assert type(opt) is optim.SGD
    tr.hip_optimizer = False
    opt, _ = tr._make_optimizer(torch.optim.AdamW, dict(lr=1e-3), None, None)
    assert type(opt) is torch.optim.AdamW
