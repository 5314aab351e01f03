#!/usr/bin/env python3
"""One SHA-256 per output of every entry of csrc/optim.hip, csrc/hardcrit.hip and csrc/boundary.hip on seeded inputs, at the lengths and
alignments of the tests' sweep (tests/flat_sweep.py) plus one case per length class with the operands at different offsets from a 16-byte
boundary.  Two builds of the library compute the same bytes if and only if their listings are equal line for line: run it once per
library (RU_LIB_PATH selects another build), each in a process of its own, and compare.

usage: flat_passes_bytes.py [--out FILE]"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from brats2019_amd import _lib as L

NS = [1, 3, 4, 5, 255, 1027, 4099, (1 << 21) + 4099]
lines = []


def say(label, t):
    torch.cuda.synchronize()
    text = "%s  %s" % (hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(), label)
    print(text, flush=True)
    lines.append(text)


class Run:
    """n 32-bit elements on the device, `off` elements past a 16-byte boundary"""

    def __init__(self, values, off):
        values = np.ascontiguousarray(values)
        self.t = torch.zeros(len(values) + 8, dtype=torch.int32, device="cuda")
        self.v = self.t[off:off + len(values)]
        self.v.copy_(torch.from_numpy(values.view(np.int32)))
        self.ptr = C.c_void_p(self.v.data_ptr())
        assert self.t.data_ptr() % 16 == 0


def dev(count, dtype):
    t = torch.zeros(count, dtype=dtype, device="cuda")
    return t, C.c_void_p(t.data_ptr())


def ok(rc, lib):
    assert rc == 0, lib.ru_last_error()


def case(lib, n, at, tag):
    rng = np.random.default_rng(7000 + 10 * n + sum(at.values()))
    f32 = lambda scale=1.0: (rng.standard_normal(n) * scale).astype(np.float32)
    st = L.stream()
    R = lambda values, name: Run(values, at[name])
    w0, g0, m0, e0, v0 = f32(), f32(), f32(), f32(), np.abs(f32())
    p0 = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.5, size=n)))).astype(np.float32)
    t0 = (rng.random(size=n) < 0.3).astype(np.float32)
    maps = rng.integers(-(1 << 18), (1 << 18) + 1, size=(2, n)).astype(np.int32)
    maps[rng.random(size=(2, n)) < 0.1] = 0
    coef, cptr = dev(1, torch.float32)
    coef.fill_(0.37)
    zeros = np.zeros(n, np.float32)
    # ---- optim.hip
    g = R(g0, "g")
    slots = int(lib.ru_gradnorm_slots(n))
    ws, wsp = dev(slots, torch.float64)
    norm, normp = dev(1, torch.float64)
    c2, c2p = dev(1, torch.float32)
    ok(lib.ru_gradnorm_partial(g.ptr, n, 0, wsp, slots * 8, st), lib)
    ok(lib.ru_gradnorm_finalize(wsp, slots, 0.5, normp, c2p, st), lib)
    say("%s gradnorm slots" % tag, ws), say("%s gradnorm norm" % tag, norm), say("%s gradnorm coef" % tag, c2)
    ok(lib.ru_scale_by(g.ptr, n, cptr, st), lib)
    say("%s scale_by g" % tag, g.v)
    for name, (mom, damp, wd, nest, first, cp) in {"nesterov": (0.99, 0.0, 0.01, 1, 0, cptr), "first": (0.9, 0.3, 0.05, 0, 1, None), "plain": (0.0, 0.0, 0.0, 0, 0, None)}.items():
        w, g, b = R(w0, "p"), R(g0, "g"), R(m0, "sp")
        ok(lib.ru_sgd_step(w.ptr, g.ptr, b.ptr if mom else None, n, 0.1, mom, damp, wd, nest, first, cp, st), lib)
        say("%s sgd %s w" % (tag, name), w.v), say("%s sgd %s buf" % (tag, name), b.v)
    for ams in (1, 0):
        for dec in (1, 0):
            w, g, m, v, vm = R(w0, "p"), R(g0, "g"), R(m0, "sp"), R(v0, "sg"), R(0.5 * v0, "dp")
            ok(lib.ru_adamw_step(w.ptr, g.ptr, m.ptr, v.ptr, vm.ptr if ams else None, n, 1e-2, 0.9, 0.99, 1e-8, 0.1, dec, 3, cptr if dec else None, st), lib)
            for what, r in (("w", w), ("m", m), ("v", v), ("vmax", vm)):
                say("%s adamw ams=%d dec=%d %s" % (tag, ams, dec, what), r.v)
    e, w = R(e0, "p"), R(w0, "g")
    ok(lib.ru_ema_update(e.ptr, w.ptr, n, 0.9, st), lib)
    say("%s ema" % tag, e.v)
    ok(lib.ru_swap_f32(e.ptr, w.ptr, n, st), lib)
    say("%s swap a" % tag, e.v), say("%s swap b" % tag, w.v)
    # ---- hardcrit.hip
    p, t = R(p0, "p"), R(t0, "g")
    out, outp = dev(2, torch.float64)
    half, halfp = dev(1, torch.float32)
    half.fill_(0.5)
    for gamma, a1, a0w in ((0.0, 1.0, 1e-2), (1.0, 0.25, 0.75), (2.0, 1.0, 1.0), (2.5, 0.25, 0.75e-2)):
        ws, wsp = dev(int(lib.ru_focal_workspace_bytes(n)) // 8, torch.float64)
        dp = R(zeros, "dp")
        ok(lib.ru_focal_sum(p.ptr, t.ptr, n, gamma, a1, a0w, outp, wsp, ws.numel() * 8, st), lib)
        ok(lib.ru_focal_grad(p.ptr, t.ptr, n, gamma, a1, a0w, float(n), halfp if gamma == 1.0 else None, dp.ptr, st), lib)
        say("%s focal gamma=%s slots" % (tag, gamma), ws), say("%s focal gamma=%s sum" % (tag, gamma), out[:1]), say("%s focal gamma=%s dp" % (tag, gamma), dp.v)
    for K, bg, sc in ((max(1, n // 10), 1.0, None), (max(1, n // 2), 1e-2, halfp)):
        keys, dp = R(np.zeros(n, np.int32), "keys"), R(zeros, "dp")
        state, statep = dev(4, torch.int64)
        ws, wsp = dev(int(lib.ru_topk_workspace_bytes(n)) // 8, torch.float64)
        ok(lib.ru_topk_select(p.ptr, t.ptr, n, K, bg, keys.ptr, statep, outp, wsp, ws.numel() * 8, st), lib)
        ok(lib.ru_topk_grad(p.ptr, t.ptr, keys.ptr, statep, n, K, bg, 1.0, sc, dp.ptr, st), lib)
        for what, r in (("workspace", ws), ("keys", keys.v), ("state", state), ("value and threshold", out), ("dp", dp.v)):
            say("%s topk K=%d %s" % (tag, K, what), r)
    # ---- boundary.hip
    sp, sg = R(maps[0], "sp"), R(maps[1], "sg")
    ws, wsp = dev(int(lib.ru_boundary_workspace_bytes(n)) // 8, torch.float64)
    dp = R(zeros, "dp")
    ok(lib.ru_boundary_sum(p.ptr, sg.ptr, n, outp, wsp, ws.numel() * 8, st), lib)
    ok(lib.ru_boundary_grad(sg.ptr, n, 0.7 / n, halfp, dp.ptr, st), lib)
    say("%s boundary slots" % tag, ws), say("%s boundary sum" % tag, out[:1]), say("%s boundary dp" % tag, dp.v)
    for alpha, sc in ((1.0, None), (2.0, halfp), (2.5, None)):
        dp = R(zeros, "dp")
        ok(lib.ru_hddt_sum(p.ptr, t.ptr, sp.ptr, sg.ptr, n, alpha, outp, wsp, ws.numel() * 8, st), lib)
        ok(lib.ru_hddt_grad(p.ptr, t.ptr, sp.ptr, sg.ptr, n, alpha, 0.7 / n, sc, dp.ptr, st), lib)
        say("%s hddt alpha=%s slots" % (tag, alpha), ws), say("%s hddt alpha=%s sum" % (tag, alpha), out[:1]), say("%s hddt alpha=%s dp" % (tag, alpha), dp.v)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    L.require_gpu()
    lib = L.load()
    names = ("p", "g", "sp", "sg", "dp", "keys")
    for n in NS:
        for off in ((0, 3) if n > (1 << 21) else (0, 1, 2, 3)):
            case(lib, n, dict.fromkeys(names, off), "n=%d off=%d" % (n, off))
    for n in (5, 4099):
        case(lib, n, dict(p=1, g=2, sp=3, sg=0, dp=1, keys=3), "n=%d mixed offsets" % n)
    # the map of boundary.hip is not a flat pass; one small volume shows that the unit as a whole still computes the same
    x = torch.from_numpy((np.random.default_rng(3).random((2, 19, 37, 65)) < 0.4).astype(np.float32)).cuda()
    sd, sdp = dev(x.numel(), torch.int32)
    ws, wsp = dev(int(lib.ru_signed_sqdist_workspace_bytes(2, 19, 37, 65)), torch.uint8)
    ok(lib.ru_signed_sqdist(C.c_void_p(x.data_ptr()), 2, 19, 37, 65, sdp, wsp, ws.numel(), L.stream()), lib)
    say("signed_sqdist 2 x 19x37x65", sd)
    from brats2019_amd import ops
    rng = np.random.default_rng(4)
    pd = torch.from_numpy((1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.5, size=(2, 3, 5, 6, 7))))).astype(np.float32)).cuda()
    gd = torch.from_numpy((rng.random(size=(2, 3, 5, 6, 7)) < 0.3).astype(np.float32)).cuda()
    tot = ops.crit_reduce(ops.crit_moments(pd, gd, L.CRIT_MASK_ALL & ~L.CRIT_MASK_LOGS))
    totp = C.c_void_p(tot.data_ptr())
    val, valp = dev(1, torch.float64)
    coef, coefp = dev(2 * 3 * 5, torch.float32)
    ok(lib.ru_tversky_eval(totp, 2, 3, 0.3, 0.7, 4.0 / 3.0, 1.0, 1.0, valp, coefp, L.stream()), lib)
    say("tversky_eval value", val), say("tversky_eval coef", coef)
    print("%d outputs, library %s" % (len(lines), os.path.basename(L.LIB_PATH)))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
