"""The flat streaming passes of csrc/hardcrit.hip and csrc/boundary.hip (focal, top-k, boundary, Hausdorff-DT; sums and gradients) through
the C ABI at every length and alignment of the sweep tests/test_optim_recipe.py gives the optimizer passes, with every input and output
between guard elements: nothing outside a run is written, no input changes, and values and gradients meet the float64 restatements of
loss.py at the bars of tests/test_hardcrit.py and tests/test_boundary.py.  The distance maps are seeded integers: the passes only read
them.  Each case prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import hardcrit_inputs as I
from flat_sweep import MIXED_N, SWEEP, Slab, distance_maps, probabilities, topk_case
from test_boundary import BOUNDARY_GRAD_BAR, BOUNDARY_VALUE_BAR, HDDT_GRAD_BAR, HDDT_VALUE_BAR
from test_hardcrit import FOCAL_CASES, FOCAL_GRAD_BAR, FOCAL_VALUE_BAR, TOPK_VALUE_BAR

pytestmark = pytest.mark.gpu

IDS = ["%d+%d" % c for c in SWEEP]
ALIKE = lambda off: dict.fromkeys(("p", "g", "sp", "sg", "dp", "keys"), off)
MIXED = dict(p=1, g=2, sp=3, sg=0, dp=1, keys=3)             # in every pass two operands disagree about the 16-byte boundary: all goes one by one
MIXED_KEY = (MIXED_N, 4)                                     # the inputs of the mixed case: a seed of their own
GAMMAS = (0, 1, 2, 2.5)
ALPHAS = (1, 2, 2.5)
TINY = 1e-300


@pytest.fixture(scope="module")
def lib():
    from brats2019_amd import _lib as L
    L.require_gpu()
    return L.load()


def _stream():
    from brats2019_amd import _lib as L
    return L.stream()


class Doubles:
    """`count` float64 (or 64-bit integer) values on the device with one guard value on either side"""

    def __init__(self, count, dtype=torch.float64):
        self.t = torch.full((count + 2,), -7, dtype=dtype, device="cuda")
        self.ptr, self.bytes = C.c_void_p(self.t.data_ptr() + 8), 8 * count

    def get(self):
        h = self.t.cpu().numpy()
        assert h[0] == -7 and h[-1] == -7, "a kernel wrote outside its buffer"
        return h[1:-1]


def _scale(off):
    """the incoming gradient of the odd offsets: a power of two, so that it adds no rounding; the even offsets pass none"""
    return (torch.tensor([0.5], dtype=torch.float32, device="cuda"), 0.5) if off % 2 else (None, 1.0)


def _grad_err(dp, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(dp.astype(np.float64) - ref) / (np.abs(ref) + 1e-4 * np.abs(ref).max() + TINY)).max())


def _unchanged(slabs, values):
    for s, v in zip(slabs, values):
        assert np.array_equal(s.get().view(np.uint32), v.view(np.uint32)), "a pass changed an input"


def _focal(lib, key, at):
    from brats2019_amd import loss as L
    (n, off), (p0, g0) = key, probabilities(*key)
    p, g = Slab(p0, at["p"]), Slab(g0, at["g"])
    sdev, sc = _scale(off)
    for gamma, (_gamma, alpha, bg) in zip(GAMMAS, sorted(FOCAL_CASES, key=lambda c: c[0])):
        assert gamma == _gamma
        a1, a0w = (1.0, float(bg)) if alpha is None else (alpha, (1.0 - alpha) * bg)
        out, ws, dp = Doubles(1), Doubles(lib.ru_focal_workspace_bytes(n) // 8), Slab(np.zeros(n, np.float32), at["dp"])
        assert lib.ru_focal_sum(p.ptr, g.ptr, n, float(gamma), a1, a0w, out.ptr, ws.ptr, ws.bytes, _stream()) == 0, lib.ru_last_error()
        assert lib.ru_focal_grad(p.ptr, g.ptr, n, float(gamma), a1, a0w, float(n), None if sdev is None else C.c_void_p(sdev.data_ptr()), dp.ptr,
                                 _stream()) == 0, lib.ru_last_error()
        ref_v, ref_dp = L.focal_host(p0, g0, gamma=gamma, alpha=alpha, bg_weight=bg)
        ws.get()
        ev, eg = abs(out.get()[0] / n - ref_v) / abs(ref_v), _grad_err(dp.get(), sc * ref_dp)
        print("focal n=%d at %s gamma=%s: value err %.3e, gradient err %.3e" % (n, at, gamma, ev, eg))
        assert ev <= FOCAL_VALUE_BAR and eg <= FOCAL_GRAD_BAR, (gamma, ev, eg)
    _unchanged((p, g), (p0, g0))


def _topk(lib, key, at):
    from brats2019_amd import loss as L
    (n, off), (p0, g0) = key, probabilities(*key)
    K, k, bg = topk_case(n, off)
    p, g, keys, dp = Slab(p0, at["p"]), Slab(g0, at["g"]), Slab(np.zeros(n, np.uint32), at["keys"]), Slab(np.zeros(n, np.float32), at["dp"])
    state, out, ws = Doubles(4, torch.int64), Doubles(2), Doubles(lib.ru_topk_workspace_bytes(n) // 8)
    sdev, sc = _scale(off)
    assert lib.ru_topk_select(p.ptr, g.ptr, n, K, float(bg), keys.ptr, state.ptr, out.ptr, ws.ptr, ws.bytes, _stream()) == 0, lib.ru_last_error()
    assert lib.ru_topk_grad(p.ptr, g.ptr, keys.ptr, state.ptr, n, K, float(bg), 1.0, None if sdev is None else C.c_void_p(sdev.data_ptr()), dp.ptr,
                            _stream()) == 0, lib.ru_last_error()
    ws.get()
    (value, t), (_key, rest, n_gt, n_eq), got = out.get(), [int(v) for v in state.get()], dp.get()
    l, K_h, t_h, _n_gt_h, _n_eq_h = L.topk_host_threshold(p0, g0, k=k, bg_weight=bg)
    ref_v, ref_dp = L.topk_host(p0, g0, k=k, bg_weight=bg)
    ev = abs(value - ref_v) / abs(ref_v)
    outside = np.abs(l - t_h) > I.BAND * abs(t_h)
    print("topk n=%d at %s bg=%s: K %d, t %.9g (host %.9g), n_gt %d, n_eq %d, value err %.3e, %d in the band"
          % (n, at, bg, K, t, t_h, n_gt, n_eq, ev, int((~outside).sum())))
    assert K == K_h and rest == K - n_gt and n_gt < K <= n_gt + n_eq
    assert int(np.count_nonzero(got)) == n_gt + n_eq
    assert ev <= TOPK_VALUE_BAR and abs(t - t_h) <= I.BAND * abs(t_h)
    if n <= 4099:
        assert int((~outside).sum()) <= I.BAND_CAP                  # tests/test_hardcrit_host.py holds the seeds to this
        ref = sc * ref_dp
        eg = float((np.abs(got - ref)[outside] / (np.abs(ref)[outside] + 1e-4 * np.abs(ref).max())).max()) if outside.any() else 0.0
        print("topk n=%d at %s: gradient err outside the band %.3e" % (n, at, eg))
        assert eg <= FOCAL_GRAD_BAR, eg
    _unchanged((p, g), (p0, g0))
    assert len(keys.get()) == n


def _boundary(lib, key, at):
    from brats2019_amd import loss as L
    (n, off), (p0, _g0), (_s_p, s0) = key, probabilities(*key), distance_maps(*key)
    p, s, dp = Slab(p0, at["p"]), Slab(s0, at["sg"]), Slab(np.zeros(n, np.float32), at["dp"])
    out, ws = Doubles(1), Doubles(lib.ru_boundary_workspace_bytes(n) // 8)
    sdev, sc = _scale(off)
    coef = float(np.float32(0.7 / n))
    assert lib.ru_boundary_sum(p.ptr, s.ptr, n, out.ptr, ws.ptr, ws.bytes, _stream()) == 0, lib.ru_last_error()
    assert lib.ru_boundary_grad(s.ptr, n, coef, None if sdev is None else C.c_void_p(sdev.data_ptr()), dp.ptr, _stream()) == 0, lib.ru_last_error()
    ws.get()
    phi = L._phi_host(s0)
    terms = p0.astype(np.float64) * phi
    ev, eg = abs(out.get()[0] - terms.sum()) / (np.abs(terms).sum() + TINY), _grad_err(dp.get(), sc * coef * phi)
    print("boundary n=%d at %s: value err %.3e of sum |term|, gradient err %.3e" % (n, at, ev, eg))
    assert ev <= BOUNDARY_VALUE_BAR and eg <= BOUNDARY_GRAD_BAR, (ev, eg)
    _unchanged((p, s), (p0, s0))


def _hddt(lib, key, at):
    (n, off), (p0, g0), (sp0, sg0) = key, probabilities(*key), distance_maps(*key)
    p, g, sp, sg = Slab(p0, at["p"]), Slab(g0, at["g"]), Slab(sp0, at["sp"]), Slab(sg0, at["sg"])
    sdev, sc = _scale(off)
    coef = float(np.float32(0.7 / n))
    d = p0.astype(np.float64) - g0.astype(np.float64)
    for alpha in ALPHAS:
        out, ws, dp = Doubles(1), Doubles(lib.ru_boundary_workspace_bytes(n) // 8), Slab(np.zeros(n, np.float32), at["dp"])
        assert lib.ru_hddt_sum(p.ptr, g.ptr, sp.ptr, sg.ptr, n, float(alpha), out.ptr, ws.ptr, ws.bytes, _stream()) == 0, lib.ru_last_error()
        assert lib.ru_hddt_grad(p.ptr, g.ptr, sp.ptr, sg.ptr, n, float(alpha), coef, None if sdev is None else C.c_void_p(sdev.data_ptr()), dp.ptr,
                                _stream()) == 0, lib.ru_last_error()
        ws.get()
        w = np.abs(sp0).astype(np.float64) ** (alpha / 2.0) + np.abs(sg0).astype(np.float64) ** (alpha / 2.0)       # loss.hddt_host's |s|^(alpha/2) form
        ref_v = float((d * d * w).sum())
        ev, eg = abs(out.get()[0] - ref_v) / (abs(ref_v) + TINY), _grad_err(dp.get(), sc * coef * 2.0 * d * w)
        print("hddt n=%d at %s alpha=%s: value err %.3e, gradient err %.3e" % (n, at, alpha, ev, eg))
        assert ev <= HDDT_VALUE_BAR and eg <= HDDT_GRAD_BAR, (alpha, ev, eg)
    _unchanged((p, g, sp, sg), (p0, g0, sp0, sg0))


ENTRIES = {"focal": _focal, "topk": _topk, "boundary": _boundary, "hddt": _hddt}


@pytest.mark.parametrize("case", SWEEP, ids=IDS)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_entry_at_every_length_and_alignment(lib, entry, case):
    """all operands of a pass `off` elements past a 16-byte boundary: a head of (4 - off) % 4 elements, quads, a tail"""
    ENTRIES[entry](lib, case, ALIKE(case[1]))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_pointers_at_different_offsets_take_the_scalar_path(lib, entry):
    ENTRIES[entry](lib, MIXED_KEY, MIXED)
