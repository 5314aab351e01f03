#!/usr/bin/env python3
"""Generate tests/golden/criteria.npz by running the REFERENCE's own criteria (loss.py:15-195).

Runs only where a checkout of the reference exists:

    python tests/golden/make_criteria_golden.py <reference checkout>      # or BRATS_REF=<reference checkout>

It imports the reference's loss.py unmodified and evaluates MSE_Loss, CE_Loss, Dice1D, GDL_joint, sens_loss_joint,
Dice_loss_separate, Dice_loss_joint and BCE_Loss, one at a time and as lists averaged as train.py:203-205 does
(`sum(values) / len(list)`), on seeded batches.  For each run it stores the values and d(loss)/d(pred) from torch autograd, with the
inputs in float32 and again cast to float64.  The float64 gradient is stored rounded to float32 (the tests' bar is rtol 2e-5), which
keeps the file small.  Runs with a BCE_Loss also keep the float32 run's gradient: its (1 + 1e-6) - p is formed in float32, and where
p is within ~1e-3 of 1 that differs from the float64 run by more than the bar.

Batches: (2,3,8,8,8) with binary targets, (3,4,5,7,6) with soft targets, and (2,3,8,8,8) binary with class 2 absent from the whole
batch (GDL_joint's weight 1 / sum g is then infinite, so its value and gradient are NaN).
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BRATS_REF", "")
OUT = os.path.join(HERE, "criteria.npz")

# run name -> list of (class, constructor kwargs)
RUNS = {
    "mse": [("MSE_Loss", {"index": 0, "priority": 0.7})],
    "ce": [("CE_Loss", {"index": 0})],
    "dice1d": [("Dice1D", {"label_index": 0})],
    "gdl": [("GDL_joint", {"index": 0, "priority": 1.5})],
    "sens": [("sens_loss_joint", {"index": 0, "priority": 0.8})],
    "sep": [("Dice_loss_separate", {"index": 0, "priority": 3})],
    "dice": [("Dice_loss_joint", {"index": 0, "priority": 1.2})],
    "bce": [("BCE_Loss", {"index": 0, "bg_weight": 1e-2})],
    "gdl_bce": [("GDL_joint", {}), ("BCE_Loss", {"bg_weight": 1e-2})],
    "sep_gdl_mse": [("Dice_loss_separate", {}), ("GDL_joint", {}), ("MSE_Loss", {})],
    "mixed4": [("Dice_loss_joint", {"priority": 2}), ("sens_loss_joint", {}), ("CE_Loss", {}), ("Dice1D", {})],
    "all8": [("MSE_Loss", {"priority": 0.5}), ("CE_Loss", {}), ("Dice1D", {}), ("GDL_joint", {"priority": 1.5}),
             ("sens_loss_joint", {"priority": 2}), ("Dice_loss_separate", {}), ("Dice_loss_joint", {}), ("BCE_Loss", {"bg_weight": 0.1})],
}


def _load_reference_loss():
    if not os.path.isfile(os.path.join(REF, "loss.py")):
        sys.exit("usage: make_criteria_golden.py <reference checkout>  (no loss.py under %r)" % REF)
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def batches():
    rng = np.random.default_rng(2019)
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    p0 = sig(rng.normal(0, 2, (2, 3, 8, 8, 8))).astype(np.float32)
    g0 = (rng.random((2, 3, 8, 8, 8)) < 0.3).astype(np.float32)
    p1 = sig(rng.normal(0, 1.5, (3, 4, 5, 7, 6))).astype(np.float32)
    g1 = rng.random((3, 4, 5, 7, 6)).astype(np.float32)
    p2 = sig(rng.normal(0, 2, (2, 3, 8, 8, 8))).astype(np.float32)
    g2 = (rng.random((2, 3, 8, 8, 8)) < 0.3).astype(np.float32)
    g2[:, 2] = 0.0
    return [(p0, g0), (p1, g1), (p2, g2)]


def main():
    import torch

    ref = _load_reference_loss()
    out = {"runs": np.asarray(json.dumps(RUNS))}
    for b, (p, g) in enumerate(batches()):
        out["b%d_pred" % b], out["b%d_gt" % b] = p, g
        for name, members in RUNS.items():
            for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
                x = torch.from_numpy(p).to(dt).requires_grad_(True)
                y = torch.from_numpy(g).to(dt)
                vals = [getattr(ref, cls)(**kw)([x], [y]) for cls, kw in members]
                loss = sum(vals) / len(vals)                    # train.py:203-205
                loss.backward()
                out["b%d_%s_values%s" % (b, name, tag)] = np.asarray([float(v.detach()) for v in vals], dtype=np.float64)
                out["b%d_%s_loss%s" % (b, name, tag)] = np.asarray(float(loss.detach()), dtype=np.float64)
                if tag == "64":
                    out["b%d_%s_dp" % (b, name)] = x.grad.numpy().astype(np.float32)
                elif any(cls == "BCE_Loss" for cls, _ in members):
                    out["b%d_%s_dp32" % (b, name)] = x.grad.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d KB)" % (OUT, os.path.getsize(OUT) // 1024))
    for b in range(3):
        print(b, {n: out["b%d_%s_values64" % (b, n)].round(6).tolist() for n in RUNS})


if __name__ == "__main__":
    main()
