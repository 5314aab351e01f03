#!/usr/bin/env python3
"""Worst error of the device's logf / expf against float64 log / exp on every distinct argument tests/test_scalar_passes.py hands them (the log arguments
p + 1e-6f and (1 + 1e-6)f - p of every criterion case, -x of every sigmoid case), in units of 2^-24 |y| and in ulp.  Builds tools/libm_ulp_probe.hip with the
library's flags into a temporary directory and runs it once per function, each in a process of its own.  LOGF_UNITS / EXPF_UNITS of
tests/test_scalar_passes_host.py are these figures rounded up, plus one.

With `intensity`: the same for the functions of csrc/intensity.hip on every distinct argument the cases of tests/intensity_inputs.py hand them -- v_log_f32 on t and
v_exp_f32 on g log2 t (gamma), logf on the noise's float32(u1), cosf on its angles, the constructed edge draws among them; ULP_LOG2, ULP_EXP2, ULP_LOGF
and ULP_COS there are these figures rounded up, plus one.  A subnormal argument of v_log_f32 is left out (the bars count it as 0).

usage: libm_ulp.py [intensity] [--probe BUILT_PROBE]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_scalar_passes_host as H  # noqa: E402
from brats2019_amd import build as B  # noqa: E402


def log_args():
    vals = []
    for case in H.SUM_CASES:
        for family, targets in (("real", "hard"), ("real", "soft"), ("exact", "hard")):
            p, _ = H.crit_inputs(case, family, targets)
            vals += [(p + np.float32(1e-6)).ravel(), (np.float32(1.0 + 1e-6) - p).ravel()]
    return np.unique(np.concatenate(vals).astype(np.float32))


def exp_args():
    v = np.unique(np.concatenate([-H.flat_inputs(n) for n in H.FLAT_N]).astype(np.float32))
    return v[np.isfinite(v)]


def intensity_args():
    import intensity_inputs as I
    tap = {"log2": [], "exp2": [], "log": [], "cos": []}
    for case in I.cases():
        I.run(case, "emu", tap=tap)
    out = {k: np.unique(np.concatenate([np.asarray(a, np.float32).ravel() for a in v])) for k, v in tap.items()}
    out["log2"] = out["log2"][out["log2"] >= np.float32(2.0 ** -126)]
    out["exp2"] = out["exp2"][~np.isnan(out["exp2"])]
    return out


def measure(probe, tmp, op, x, f64):
    a, b = os.path.join(tmp, op + "_in.bin"), os.path.join(tmp, op + "_out.bin")
    x.tofile(a)
    subprocess.run([probe, op, a, b], check=True, timeout=120)
    got = np.fromfile(b, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        ref = f64(x.astype(np.float64))
        ref32 = ref.astype(np.float32)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0), "a zero result is not zero"
    ok = np.isfinite(ref32) & (np.abs(ref) >= 2.0 ** -126) & ~zero          # results in the normal range
    d, r = np.abs(got - ref)[ok], np.abs(ref)[ok]
    units = d / (2.0 ** -24 * r)
    ulps = d / np.spacing(np.abs(ref32[ok])).astype(np.float64)
    print("%sf: %d arguments, %d compared: worst %.4f units of 2^-24 |y| (at x = %r), worst %.4f ulp"
          % (op, x.size, units.size, units.max(), float(x[ok][int(np.argmax(units))]), ulps.max()), flush=True)


with tempfile.TemporaryDirectory() as tmp:
    if "--probe" in sys.argv:
        probe = os.path.abspath(sys.argv[sys.argv.index("--probe") + 1])
    else:
        probe = os.path.join(tmp, "libm_ulp_probe")
        flags = [f for f in B.FLAGS if f not in ("-fPIC", "-fno-gpu-rdc")]
        subprocess.run([B._hipcc()] + flags + [os.path.join(ROOT, "tools", "libm_ulp_probe.hip"), "-o", probe], check=True)
    if "intensity" in sys.argv:
        args = intensity_args()
        for op, f64 in (("log2", np.log2), ("exp2", np.exp2), ("log", np.log), ("cos", np.cos)):
            measure(probe, tmp, op, args[op], f64)
    else:
        measure(probe, tmp, "log", log_args(), np.log)
        measure(probe, tmp, "exp", exp_args(), np.exp)
