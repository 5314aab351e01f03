"""GPU parity, whole network, with GroupNorm parameters as training leaves them: gammas of both signs, exact zeros, |gamma| = 1e-6, beta == 0
(tests/test_hip_gn_params_host.py: edit_gn_params and why).  Every route of the GroupNorm backward -- the separate reduce / finalize / apply passes of the NCDHW
engine, the fused statistics of the data-gradient and 1x1 epilogues, the apply fused into the 16-channel weight gradient, the one-product gradient kernels and
ru_unet_backward_criterion -- runs the same edited parameters as the CPU oracle (model.py:407-433 + loss.py through autograd).
Bars, as in test_default_path_shape_sweep_against_the_oracle: probabilities 2e-4, loss 2e-5, every parameter gradient within max(1e-3, 2 x the change a 1e-5
relative weight perturbation causes in the oracle's own gradients) of its largest element."""
import numpy as np
import pytest
import torch

from oracle import resunet_oracle as O
from test_hip_gn_params_host import CONFIGS, KINDS, grad_distance, oracle_case

pytestmark = pytest.mark.gpu

T = torch.from_numpy
PERSISTENT = (2, (16, 128, 128))           # tests/test_hip_c16.py: the first level takes the persistent kernels, statistics partials across a sample boundary
FUSIONS = {"fused": (True, True), "no-bst": (False, True), "no-gba": (True, False), "unfused": (False, False)}


def run_step(case, cfgname, precision, fusion=None, grad_precision=None, probe=False):
    """run_train_step of tests/test_hip_unet.py on the case's parameters -> (probs, loss, {name: gradient or None}, probe counts)"""
    from brats2019_amd import model as M, loss as L
    net = M.UNet(**CONFIGS[cfgname])
    net.set_precision(precision)
    net.load_state_dict({k: T(v) for k, v in case["params"].items()})
    net.cuda().train()
    eng = net._get_engine()
    if fusion is not None:
        eng.set_fusion(*fusion)
    if grad_precision is not None:
        net.set_grad_precision(grad_precision)
    if probe:
        eng.probe(2)
    out = net([T(case["x"]).cuda()])
    g = T(case["g"]).cuda()
    vals = [c(out, [g]) for c in (L.Dice_loss_joint(index=0, priority=1), L.BCE_Loss(index=0, bg_weight=1e-2))]
    loss = sum(vals) / len(vals)
    loss.backward()
    counts = None
    if probe:
        fam, inst = eng.probe_read_families(instances=True)
        counts = {k: v[1] for k, v in list(fam.items()) + list(inst.items())}
        eng.probe(False)
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in net.named_parameters()}
    return out[0].detach().cpu().numpy(), float(loss), grads, counts


def check_step(case, probs, loss, grads, tag):
    dp = float(np.abs(probs - case["probs"]).max())
    for k, r in case["grads"].items():
        assert (grads[k] is None) == (r is None), k
    worst = grad_distance(grads, case["grads"])
    print("  %s: max |dp| %.1e, loss error %.1e, worst gradient error / max |ref| %.1e (%s); sensitivity %.1e -> bar %.1e"
          % (tag, dp, abs(loss - case["loss"]), worst[0], worst[1], case["sens"], case["bar"]))
    assert dp <= 2e-4, dp
    assert abs(loss - case["loss"]) < 2e-5
    assert worst[0] <= case["bar"], (worst, case["sens"])
    # zero-gamma channels: their gamma / beta gradients absolutely (a bar relative to the channel's own value would mean nothing: the oracle's value may be 0)
    for layer, sp in case["special"].items():
        for suffix in (".weight", ".bias"):
            ref = case["grads"][layer + suffix]
            if ref is None or not sp["zero"].size:
                continue
            atol = case["bar"] * float(np.abs(ref).max())
            err = np.abs(grads[layer + suffix].astype(np.float64) - ref.astype(np.float64))[sp["zero"]]
            assert (err <= atol).all(), (layer + suffix, sp["zero"], err, atol)


STEP_CASES = [("default", 2, (16, 16, 16)), ("default", 2, (32, 48, 24)), ("small", 2, (16, 24, 16))]


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("cfgname,n,dhw", STEP_CASES, ids=["%s-%dx%dx%dx%d" % ((c, n) + d) for c, n, d in STEP_CASES])
@pytest.mark.parametrize("kind", KINDS)
def test_edited_parameters_train_step_against_the_oracle(kind, cfgname, n, dhw, precision):
    case = oracle_case(cfgname, kind, n, dhw, 100 + n + dhw[1])
    probs, loss, grads, _ = run_step(case, cfgname, precision)
    check_step(case, probs, loss, grads, "%s %s %d x %s %s" % (kind, cfgname, n, dhw, precision))


_persistent = {}


def persistent_step(kind, route):
    if (kind, route) not in _persistent:
        case = oracle_case("default", kind, PERSISTENT[0], PERSISTENT[1], 128)
        _persistent[(kind, route)] = run_step(case, "default", "bf16x3", fusion=FUSIONS[route], probe=True)
    return _persistent[(kind, route)]


@pytest.mark.parametrize("route", list(FUSIONS))
@pytest.mark.parametrize("kind", ["mixed", "zeros"])
def test_persistent_shape_every_fusion_route_against_the_oracle(kind, route):
    """2 x 16 x 128 x 128: persistent first-level kernels, fused statistics across the sample boundary, each ru_unet_set_fusion combination of
    test_unet128_train_step_bf16x3_matches_reference_fixture.  The probe (ru_unet_probe_read_families) must show that the route really ran: the 16-channel
    data-gradient convolutions (whose epilogue takes the fused statistics), and the weight gradient with / without the fused apply."""
    case = oracle_case("default", kind, PERSISTENT[0], PERSISTENT[1], 128)
    probs, loss, grads, counts = persistent_step(kind, route)
    print("  probe launches (%s): %s" % (route, counts))
    bst, gba = FUSIONS[route]
    assert counts["conv16_fwd"] > 0 and counts["conv16_dgrad"] > 0
    assert (counts["wgrad16_fused_apply"] > 0) == gba and (counts["wgrad16_plain"] > 0) == (not gba), counts
    check_step(case, probs, loss, grads, "%s persistent %s" % (kind, route))


@pytest.mark.parametrize("kind", ["mixed", "zeros"])
def test_persistent_shape_fused_and_unfused_agree(kind):
    """same parameters, fusions on against off, at the bars of test_fused_and_unfused_backward_agree_tightly (relative L2: 1e-3 convolution weights, 2e-3 vectors);
    the fused statistics replace GroupNorm reduce launches, so the groupnorm family must have fewer launches with them on"""
    res = {r: persistent_step(kind, r) for r in FUSIONS}
    assert res["fused"][3]["groupnorm"] < res["no-bst"][3]["groupnorm"], (res["fused"][3], res["no-bst"][3])
    assert res["no-gba"][3]["groupnorm"] < res["unfused"][3]["groupnorm"], (res["no-gba"][3], res["unfused"][3])
    assert np.array_equal(res["fused"][0], res["unfused"][0])                      # the forward does not depend on the switch
    ga, gb = res["fused"][2], res["unfused"][2]
    rel = {k: float(np.linalg.norm(ga[k].astype(np.float64) - gb[k]) / (np.linalg.norm(gb[k].astype(np.float64)) + 1e-30)) for k in ga if ga[k] is not None}
    worst_w = max((v, k) for k, v in rel.items() if ga[k].ndim == 5)
    worst_v = max((v, k) for k, v in rel.items() if ga[k].ndim != 5)
    print("  %s fused vs unfused: worst relative L2 %.2e (%s) on conv weights, %.2e (%s) on vectors" % ((kind,) + worst_w + worst_v))
    assert any(not np.array_equal(ga[k], gb[k]) for k in rel)
    assert worst_w[0] < 1e-3, worst_w
    assert worst_v[0] < 2e-3, worst_v


@pytest.mark.parametrize("kind", ["mixed", "zeros"])
def test_edited_parameters_bf16_gradient_precision(kind):
    """grad_precision="bf16" (one-product gradient kernels) on the edited parameters, same bars"""
    n, dhw = 2, (32, 48, 24)
    case = oracle_case("default", kind, n, dhw, 100 + n + dhw[1])
    probs, loss, grads, _ = run_step(case, "default", "bf16x3", grad_precision="bf16")
    check_step(case, probs, loss, grads, "%s bf16 gradients" % kind)


@pytest.mark.parametrize("fused", [True, False], ids=["criterion-fused", "criterion-separate"])
@pytest.mark.parametrize("kind", ["mixed", "zeros"])
def test_edited_parameters_backward_criterion(kind, fused):
    """parallel.DataParallelStep (ru_unet_backward_criterion with fuse_criterion_grad on, ru_criterion_grad + ru_unet_backward with it off)"""
    from brats2019_amd import parallel as P
    n, dhw = 2, (32, 48, 24)
    case = oracle_case("default", kind, n, dhw, 100 + n + dhw[1])
    be = P.HipBackend(cfg=O.DEFAULT_CFG)
    assert be.engine.precision == "bf16x3"
    flat = be.new_flat()
    for k, v in be.engine.layout.views(flat).items():
        v.copy_(T(case["params"][k]))
    st = P.DataParallelStep(be, flat)
    st.fuse_criterion_grad = fused
    loss, _, _ = st.loss_and_grads(T(case["x"]).cuda(), T(case["g"]).cuda())
    grads = {k: (None if case["grads"][k] is None else v.detach().cpu().numpy()) for k, v in be.engine.layout.views(st.grads).items()}
    check_step(case, st.last_probs.detach().cpu().numpy(), float(loss), grads, "%s backward_criterion fused=%s" % (kind, fused))
