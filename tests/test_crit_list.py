"""The criterion-list passes of csrc/criteria.hip on the device, one entry at a time through the C-ABI -- ru_crit_moments, ru_crit_reduce, ru_crit_eval, ru_crit_grad, and
ru_tversky_eval (csrc/hardcrit.hip), whose table ru_crit_grad applies -- against the float64 restatements of tests/test_crit_list_host.py: its cases, its inputs, its
bars (derived there from the roundings of each kernel as written), its exact family, its NaN contract.

Every entry gets the inputs its restatement gets: ru_crit_reduce the moments the device made, ru_crit_eval the totals and moments the device made (and, sharded, the sum
of two shards' totals with n_global = 2 N), ru_crit_grad the float32 table read back from the device.  p, g and dp are flat_sweep.Slab runs between guard elements (dp
pre-filled with NaN); moments, totals, values and table are NaN-filled with a guard element on either side; the workspace is op_cases.GuardedWorkspace at exactly the
queried size, filled with 0xFF; guards are checked after every call.  NaN masks must equal the restatement's; no element is left out of a comparison.

Alignment: at V = 8196 and 16388 p, g and dp sit 0, 1, 2 and 3 elements past a 16-byte boundary (and at 1, 2, 3; g alone and dp alone off it): moments and dp stay within the bars and dp keeps
the bytes of the aligned call (the arithmetic is per element; only the instantiation changes).

Measured on the MI355X, worst error / bar per entry over the cases of a family (every exact-family, totals, mask, repeatability and alignment comparison: 0 differences):

  family       moments   log moments   evaluate   table   apply
  real         0.060     0.046         0.023      0.99    0.52
  soft         0.058     0.035         0.011      0.97    0.59
  saturated    0.049     0.054         0.026      1.00    0.50
  absent1      0.033     0.040         0          0.98    0.47
  absent_all   0.042     0.039         0          0.92    0.51
  exact        0         0.079         0.013      0.99    0.40
  alignment    0.048     (with them)   -          -       0.63
separate-Dice slot 0.080; the autograd wrapper's gradient 0.40; Tversky: value 0.023, table 0.59, its table applied 0.31.  The table's figure is the float32 rounding of
a float64 coefficient: half an ulp is 2^-24 |ref| at the bottom of a binade, so a figure just below 1 is what a correctly rounded table gives and a wrong digit in
float64 would pass 1 by orders of magnitude (the mutants of the host file: 10^6 and more).  The figures are measurements against the derived bars, never inputs to them."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_crit_list_host as H
from flat_sweep import Slab
from op_cases import GuardedWorkspace
from test_scalar_passes import P, _release, call, dev, filled, inner, lib, report, stream      # noqa: F401 (lib and _release are fixtures)

pytestmark = pytest.mark.gpu
NAN = float("nan")
MASK_ALL, MASK_LOGS = 0x7F, (1 << 4) | (1 << 5)


def slab(a, off=0):
    return Slab(np.ascontiguousarray(a, dtype=np.float32).reshape(-1), off)


def nan_slab(n, off=0):
    return Slab(np.full(n, NAN, np.float32), off)


def run_moments(lib, ps, gs, n, c, v, mask, ws):
    """ru_crit_moments on two slabs -> (the guarded device buffer, [N, C, 7] float64 on the host)"""
    out = filled(n * c * 7, torch.float64)
    buf = ws(lib.ru_crit_moments_workspace_bytes(n, c, v), "cuda")
    assert buf.numel() == n * c * (-(-v // H.CM_CHUNK)) * 7 * 4
    call(lib, "ru_crit_moments", ps.ptr, gs.ptr, n, c, v, mask, P(out, 1), P(buf), buf.numel(), stream())
    got = inner(out).reshape(n, c, 7).copy()
    ps.get(), gs.get()
    return out, got


def run_reduce(lib, moments_dev, n, c):
    out = filled(c * 7 + 1, torch.float64)
    call(lib, "ru_crit_reduce", P(moments_dev, 1), n, c, P(out, 1), stream())
    return out, inner(out).copy()


def term_array(terms):
    from brats2019_amd import _lib as L
    return (L.CritTerm * len(terms))(*[L.CritTerm(L.CRIT_KINDS[k], float(w), float(pr), float(bg)) for k, w, pr, bg in terms])


def run_eval(lib, totals_dev, moments_dev, n, c, terms, count, n_global):
    values, coef = filled(1 + len(terms), torch.float64), filled(n * c * 5, torch.float32)
    arr = term_array(terms)
    call(lib, "ru_crit_eval", P(totals_dev, 1), P(moments_dev, 1), n, c, float(count), float(n_global), C.cast(arr, C.c_void_p), len(terms), P(values, 1), P(coef, 1),
         stream())
    return inner(values).copy(), inner(coef).reshape(n, c, 5).copy()


def run_grad(lib, ps, gs, coef, scale, n, c, v, with_logs, off=0):
    """ru_crit_grad with the table and the scale given -> dp [N, C, V] float32"""
    table = filled(n * c * 5, torch.float32)
    table[1:-1] = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float32).reshape(-1)).cuda()
    sc = None if scale is None else dev(np.array([scale], np.float32))
    out = nan_slab(n * c * v, off)
    call(lib, "ru_crit_grad", ps.ptr, gs.ptr, P(table, 1), None if sc is None else P(sc), n, c, v, int(with_logs), out.ptr, stream())
    got = out.get().reshape(n, c, v)
    inner(table), ps.get(), gs.get()
    return got


WORST = {}


def note(entry, family, ex):
    key = "%s %s" % (entry, family)
    WORST[key] = max(WORST.get(key, 0.0), ex)
    return ex


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    for key in sorted(WORST):
        print("  worst error / bar  %-28s %.3g" % (key, WORST[key]))


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_case(case, lib):
    """moments -> reduce -> evaluate (every term list; the sharded form for two of them) -> apply (three lists), each against its restatement on the same inputs"""
    n, c, v, family, logs = case
    p, g = H.inputs(n, c, v, family)
    ws = GuardedWorkspace()
    ps, gs = slab(p), slab(g)
    mask = MASK_ALL if logs else MASK_ALL & ~MASK_LOGS
    # ---- moments
    m_dev, m = run_moments(lib, ps, gs, n, c, v, mask, ws)
    ref, bar = H.moments64(p, g, logs), H.moments_bars(p, g, logs)
    if family == "exact":
        assert H.same_bits(m[:, :, H.NONLOG], ref[:, :, H.NONLOG]), (case, m, ref)
    if not logs:
        assert not m[:, :, 4:6].any() and not np.signbit(m[:, :, 4:6]).any()
    ex = report("moments %s" % H.case_id(case), note("moments", family, H.ratio(m[:, :, H.NONLOG], ref[:, :, H.NONLOG], bar[:, :, H.NONLOG])))
    exl = report("   the log moments", note("log moments", family, H.ratio(m[:, :, 4:6], ref[:, :, 4:6], bar[:, :, 4:6])))
    assert ex <= 1.0 and exl <= 1.0, (case, ex, exl)
    # ---- reduce, on the device's moments
    t_dev, tot = run_reduce(lib, m_dev, n, c)
    tref = H.reduce64(m)
    assert H.same_bits(tot[:-1], tref[:-1]), (case, tot, tref)
    exr = report("   the separate-Dice slot", note("reduce slot", family, H.ratio(tot[-1:], tref[-1:], np.array([H.reduce_bar(m)]))))
    assert exr <= 1.0
    # ---- evaluate, on the device's totals and moments
    count = float(p.size)
    tables = {}
    for name, terms in H.TERM_LISTS.items():
        values, coef = run_eval(lib, t_dev, m_dev, n, c, terms, count, n)
        ev = H.eval64(tot, m, terms, count, n)
        vb, _, tb = H.eval_bars(ev, c)
        exv, ext = note("evaluate", family, H.ratio(values, ev["values"], vb)), note("table", family, H.ratio(coef, ev["coef"], tb))
        assert exv <= 1.0 and ext <= 1.0, (case, name, exv, ext, values, ev["values"])
        tables[name] = coef
    report("   evaluate, %d term lists" % len(H.TERM_LISTS), max(WORST["evaluate " + family], WORST["table " + family]))
    if v > 8 or n > 1:                                               # the sharded form: a second shard's totals added, n_global = 2 N
        p2, g2 = H.inputs(n, c, v, family, salt=1)
        m2_dev, m2 = run_moments(lib, slab(p2), slab(g2), n, c, v, mask, ws)
        _, tot2 = run_reduce(lib, m2_dev, n, c)
        both = tot + tot2
        both_dev = filled(c * 7 + 1, torch.float64)
        both_dev[1:-1] = dev(both)
        for name in ("all8", "Dice_loss_separate_pr1"):
            for md, mh in ((m_dev, m), (m2_dev, m2)):
                values, coef = run_eval(lib, both_dev, md, n, c, H.TERM_LISTS[name], 2.0 * count, 2 * n)
                ev = H.eval64(both, mh, H.TERM_LISTS[name], 2.0 * count, 2 * n)
                vb, _, tb = H.eval_bars(ev, c)
                exv, ext = note("evaluate", family, H.ratio(values, ev["values"], vb)), note("table", family, H.ratio(coef, ev["coef"], tb))
                assert exv <= 1.0 and ext <= 1.0, (case, name, "sharded", exv, ext)
    # ---- apply, on the float32 table the device wrote
    if family == "exact":
        coef, scale = H.exact_table(n, c)
        dp = run_grad(lib, ps, gs, coef, scale, n, c, v, 0)
        dref, _ = H.apply64(p, g, coef, scale, False)
        assert H.same_bits(dp, dref), case
    for name in H.APPLY_LISTS[logs]:
        for scale in (None, H.WRAPPER_SCALE):
            dp = run_grad(lib, ps, gs, tables[name], scale, n, c, v, int(logs))
            dref, dbar = H.apply64(p, g, tables[name], None if scale is None else np.float32(scale), logs)
            exa = note("apply", family, H.ratio(dp, dref, dbar))
            assert exa <= 1.0, (case, name, scale, exa)
            if family.startswith("absent") and "GDL_joint" in [t[0] for t in H.TERM_LISTS[name]]:
                assert np.isnan(dp[:, 1:]).all() and np.isfinite(dp[:, 0]).all()
    report("   apply", WORST["apply " + family])
    assert ws.intact()


@pytest.mark.parametrize("v", H.ALIGN_VS)
def test_alignment(v, lib):
    n, c = 2, 3
    p, g = H.inputs(n, c, v, "real")
    ws = GuardedWorkspace()
    scale = np.float32(H.WRAPPER_SCALE)
    m0 = H.moments64(p, g)
    coef = H.eval64(H.reduce64(m0), m0, H.TERM_LISTS["all8_unequal"], float(p.size), n)["coef"].astype(np.float32)
    refs = {logs: (H.moments64(p, g, logs), H.moments_bars(p, g, logs)) + H.apply64(p, g, coef, scale, logs) for logs in (True, False)}
    first = {}
    for po, go, do in H.ALIGN_OFFSETS:
        ps, gs = slab(p, po), slab(g, go)
        assert ps.ptr.value % 16 == 4 * po and gs.ptr.value % 16 == 4 * go
        for logs in (True, False):
            mref, mbar, dref, dbar = refs[logs]
            _, m = run_moments(lib, ps, gs, n, c, v, MASK_ALL if logs else MASK_ALL & ~MASK_LOGS, ws)
            ex = report("moments V %d offsets %d %d logs %d" % (v, po, go, logs), note("moments", "aligned", H.ratio(m, mref, mbar)))
            assert ex <= 1.0
            dp = run_grad(lib, ps, gs, coef, scale, n, c, v, int(logs), do)
            exa = report("   apply, dp offset %d" % do, note("apply", "aligned", H.ratio(dp, dref, dbar)))
            assert exa <= 1.0
            if logs not in first:
                assert (po, go, do) == (0, 0, 0)
                first[logs] = dp.tobytes()
            assert dp.tobytes() == first[logs], "dp changed with the alignment: offsets %d %d %d, logs %d" % (po, go, do, logs)
    assert ws.intact()


def test_two_calls_give_identical_bytes(lib):
    n, c, v = 2, 3, 11951
    p, g = H.inputs(n, c, v, "real")
    runs = []
    for _ in range(2):
        ws = GuardedWorkspace()
        ps, gs = slab(p), slab(g)
        m_dev, m = run_moments(lib, ps, gs, n, c, v, MASK_ALL, ws)
        t_dev, tot = run_reduce(lib, m_dev, n, c)
        values, coef = run_eval(lib, t_dev, m_dev, n, c, H.TERM_LISTS["all8"], float(p.size), n)
        dp = run_grad(lib, ps, gs, coef, H.WRAPPER_SCALE, n, c, v, 1)
        tv = filled(1, torch.float64), filled(n * c * 5, torch.float32)
        call(lib, "ru_tversky_eval", P(t_dev, 1), n, c, 0.3, 0.7, 4.0 / 3.0, 1.0, 1.0, P(tv[0], 1), P(tv[1], 1), stream())
        runs.append([a.tobytes() for a in (m, tot, values, coef, dp, inner(tv[0]), inner(tv[1]))])
        assert ws.intact()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("v", [5, 8196, 11951])
def test_mask(v, lib):
    """no log bit: moments 4 and 5 exactly 0, the other five bit-equal to the full-mask call; either single log bit: both written"""
    n, c = 2, 3
    p, g = H.inputs(n, c, v, "real")
    ws = GuardedWorkspace()
    ps, gs = slab(p), slab(g)
    _, full = run_moments(lib, ps, gs, n, c, v, MASK_ALL, ws)
    _, none = run_moments(lib, ps, gs, n, c, v, MASK_ALL & ~MASK_LOGS, ws)
    _, zero = run_moments(lib, ps, gs, n, c, v, 0, ws)
    assert full[:, :, 4:6].all()
    for got in (none, zero):
        assert not got[:, :, 4:6].any() and got[:, :, H.NONLOG].tobytes() == full[:, :, H.NONLOG].tobytes()
    for bit in (4, 5):
        _, one = run_moments(lib, ps, gs, n, c, v, 1 << bit, ws)
        assert one.tobytes() == full.tobytes(), bit
    assert ws.intact()


@pytest.mark.parametrize("which", ["GDL_joint", "all8"])
def test_autograd_wrapper_scales_the_gradient(which, lib):
    """loss._TermsFn through the public classes at 2 x 3 x 8193: backward of 0.37 * loss = apply64 of the table the forward saved, with that scale"""
    from brats2019_amd import loss as L
    n, c, v = H.WRAPPER_CASE
    p, g = H.inputs(n, c, v, "real")
    x = torch.from_numpy(p.reshape(n, c, 1, 1, v)).cuda().requires_grad_(True)
    y = torch.from_numpy(g.reshape(n, c, 1, 1, v)).cuda()
    if which == "GDL_joint":
        terms = [("GDL_joint", 1.0, 1.5, 1.0)]
        loss = L.GDL_joint(priority=1.5)([x], [y])
    else:
        terms = [(k, 1.0 / 8, pr, bg) for k, _w, pr, bg in H.TERM_LISTS["all8"]]
        mods = [L.Dice_loss_joint(priority=1.25), L.BCE_Loss(bg_weight=0.1), L.MSE_Loss(priority=0.5), L.CE_Loss(), L.Dice1D(), L.GDL_joint(priority=1.5),
                L.sens_loss_joint(priority=2.0), L.Dice_loss_separate(priority=3.0)]
        assert [type(m).__name__ for m in mods] == [t[0] for t in terms]
        loss, vals = L.fuse_criterion_list(mods)([x], [y])
    node = loss.grad_fn
    logs = H.has_logs(terms)
    assert node.logs is logs
    coef = node.saved_tensors[2].cpu().numpy()
    m = H.moments64(p, g, logs)
    ev = H.eval64(H.reduce64(m), m, terms, float(p.size), n)
    # (a sanity check of what the forward returned, not a bar of an entry: the moments are off by up to R_MOMENT U each, a quotient of two carries both, U^2 both twice)
    loose = float(H.R_MOMENT.max()) * H.U
    assert abs(float(loss.detach()) - ev["values"][0]) <= H.U * abs(ev["values"][0]) + 4.0 * loose * ev["vmag"][0]
    assert H.ratio(coef, ev["coef"], 6.0 * loose * ev["cmag"] + H.U * np.abs(ev["coef"]) + H.DENORM) <= 1.0
    (loss * H.WRAPPER_SCALE).backward()
    dref, dbar = H.apply64(p, g, coef, np.float32(H.WRAPPER_SCALE), logs)
    ex = report("wrapper %s, incoming gradient %g" % (which, H.WRAPPER_SCALE), note("apply", "wrapper", H.ratio(x.grad.cpu().numpy().reshape(n, c, v), dref, dbar)))
    assert ex <= 1.0


def test_tversky_eval_and_its_table_applied(lib):
    """ru_tversky_eval on the exact family's totals (the float64 sums exactly: what loss.tversky_host sums) against the host restatement, then its table applied to the
    real family at V = 11951 with with_logs = 0"""
    n, c, v = H.TVERSKY_SHAPE
    pe, ge = H.inputs(n, c, v, "exact")
    pr, gr = H.inputs(n, c, v, "real")
    tot = H.reduce64(H.moments64(pe, ge, False))
    t_dev = filled(c * 7 + 1, torch.float64)
    t_dev[1:-1] = dev(tot)
    ps, gs = slab(pr), slab(gr)
    for alpha, beta, gamma, priority in H.TVERSKY_CASES:
        value, coef = filled(1, torch.float64), filled(n * c * 5, torch.float32)
        call(lib, "ru_tversky_eval", P(t_dev, 1), n, c, alpha, beta, gamma, 1.0, float(priority), P(value, 1), P(coef, 1), stream())
        got_v, got_c = inner(value).copy(), inner(coef).reshape(n, c, 5).copy()
        ref_v, ref_c, amp = H.tversky_table64(pe, ge, alpha, beta, gamma, priority)
        vb, tb = H.tversky_bars(ref_v, ref_c, amp)
        exv = report("tversky value alpha %g beta %g gamma %.4f priority %g" % (alpha, beta, gamma, priority), note("tversky", "value", H.ratio(got_v, [ref_v], [vb])))
        ext = report("   table", note("tversky", "table", H.ratio(got_c, ref_c, tb)))
        assert exv <= 1.0 and ext <= 1.0, (got_v, ref_v, got_c[0], ref_c[0])
        dp = run_grad(lib, ps, gs, got_c, H.WRAPPER_SCALE, n, c, v, 0)
        dref, dbar = H.apply64(pr, gr, got_c, np.float32(H.WRAPPER_SCALE), False)
        exa = report("   applied", note("tversky", "applied", H.ratio(dp, dref, dbar)))
        assert exa <= 1.0
    inner(t_dev)
