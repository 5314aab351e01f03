"""Entry point with the reference's `test.py --name --models_path` contract (test.py:17-19,64-176): load the best checkpoint
of <models_path>/<name>/ and segment cases.  The reference hard-codes its NIfTI input/output directories (test.py:68-69)
and needs nibabel / skimage, which this image lacks; here a case is a `.npy` array [4,D,H,W] (t1, t1ce, t2, flair stacked as
loader_helper.read_multimodal does) and the result a uint8 `.npy` label volume {0,1,2,4}.

    python -m brats2019_amd.test --name brain-tumor-segmentation-0002 --models_path ./models --input case.npy --output seg.npy

`--ensemble B C ...` adds the best checkpoints of further experiments under the same `--models_path`: every case is segmented by the
mean of all models' probabilities (`inference.predict_case_ensemble`).  `--probs_output DIR` also saves that mean -- the soft labels a
student network is distilled from -- as float32 `NAME.npy` [3,D,H,W].

`--uncertainty std|entropy --uncertainty_output DIR` also writes the BraTS uncertainty task's three maps per case, uint8 [D,H,W] with
values 0 (certain) .. 100 (uncertain): `NAME_unc_whole.npy`, `NAME_unc_core.npy`, `NAME_unc_enhance.npy`, made from the models x flips
predictions in the passes that merge them (`inference.predict_case_ensemble(..., uncertainty=...)`, csrc/uncertainty.hip).

`--tile D H W [--overlap F] [--window gaussian|constant]` runs every forward as a sliding window over the padded crop: tiles of D x H x W
overlapping by the fraction F (default 0.5), every predicted voxel used and weighted by the window (`tiling.predict_blended`,
csrc/blend.hip) -- for a case whose padded crop does not fit the device whole.

`--min_volume WT TC ET`, `--min_confidence WT TC ET`, `--keep_largest wt|tc|et ...`, `--fill_holes wt|tc|et ...`, `--nest`, `--no_reject`
post-process the merged masks per region on the device before the labels are composed (`inference.PostProcess`, csrc/postprocess.hip;
INTEGRATION.md states the definition); `--no_reject` drops the reference's rejection on the union of all labels.

`--thresholds WT TC ET` or `--thresholds_file FILE` (the JSON `python -m brats2019_amd.validate --calibration --thresholds_output` writes) make the
region masks `mean probability > threshold` instead of `> 0.5`, before the post-processing and the label composition (csrc/calibration.hip).
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import inference, train

parser = argparse.ArgumentParser(description="PyTorch BraTS2019 (MI355X HIP engine)")
parser.add_argument("--name", default="test", type=str, help="Name of the experiment")
parser.add_argument("--models_path", default="/models", type=str, help="Path to models folder")
parser.add_argument("--input", default=None, type=str, nargs="+", help=".npy case(s) [4,D,H,W]; default: a synthetic 128^3 case")
parser.add_argument("--output", default=None, type=str, help="output .npy (single case) or directory")
parser.add_argument("--precision", default="bf16x3", choices=["bf16x3", "f32"])
parser.add_argument("--ensemble", default=None, type=str, nargs="+", help="further experiment names under --models_path: segment with the mean of all models")
parser.add_argument("--probs_output", default=None, type=str, help="directory for the mean region probabilities (soft labels), float32 NAME.npy [3,D,H,W]")
# SUPPRESS: without these flags the namespace -- and so the printed output -- does not change
parser.add_argument("--uncertainty", default=argparse.SUPPRESS, choices=["std", "entropy"], help="uncertainty measure of the maps (with --uncertainty_output)")
parser.add_argument("--uncertainty_output", default=argparse.SUPPRESS, type=str,
                    help="directory for the uint8 uncertainty maps NAME_unc_whole.npy, NAME_unc_core.npy, NAME_unc_enhance.npy")
parser.add_argument("--tile", default=argparse.SUPPRESS, type=int, nargs=3, metavar=("D", "H", "W"), help="blended sliding-window forward with tiles of this size")
parser.add_argument("--overlap", default=argparse.SUPPRESS, type=float, help="overlap of neighbouring tiles as a fraction of the tile, 0 .. 0.75 (with --tile; default 0.5)")
parser.add_argument("--window", default=argparse.SUPPRESS, choices=["gaussian", "constant"], help="blend window (with --tile; default gaussian)")
inference.add_postprocess_arguments(parser)
inference.add_threshold_arguments(parser)


def _load_net(name, opt):
    trainer = train.Trainer(name=name, models_root=opt.models_path, rewrite=False, connect_tb=False)
    trainer.load_best()
    trainer.state.cuda = True
    net = trainer.model.module if hasattr(trainer.model, "module") else trainer.model
    net.set_precision(opt.precision)
    net.cuda()
    return net


def main(argv=None):
    opt = parser.parse_args(argv)
    measure, unc_dir = getattr(opt, "uncertainty", None), getattr(opt, "uncertainty_output", None)
    if (measure is None) != (unc_dir is None):
        parser.error("--uncertainty and --uncertainty_output go together")
    if not hasattr(opt, "tile") and (hasattr(opt, "overlap") or hasattr(opt, "window")):
        parser.error("--overlap and --window need --tile")
    tiled = dict(tile=tuple(opt.tile), overlap=getattr(opt, "overlap", 0.5), window=getattr(opt, "window", "gaussian")) if hasattr(opt, "tile") else {}
    post = inference.postprocess_from_args(opt)
    if post is not None:
        tiled["postprocess"] = post
    thresholds = inference.thresholds_from_args(opt)
    if thresholds is not None:
        tiled["thresholds"] = thresholds
    print(torch.__version__)
    print(opt)
    net = _load_net(opt.name, opt)
    others = [_load_net(name, opt) for name in (opt.ensemble or [])]
    cases = opt.input
    if not cases:
        rng = np.random.default_rng(0)
        img = np.zeros((4, 128, 128, 128), np.float32)
        img[:, 8:120, 8:120, 8:120] = rng.random((4, 112, 112, 112)).astype(np.float32) + 0.05
        cases = [("synthetic", img)]
    else:
        cases = [(os.path.splitext(os.path.basename(c))[0], np.load(c)) for c in cases]
    for name, image in cases:
        if others or opt.probs_output or measure:
            out = inference.predict_case_ensemble([net] + others, image, want_probs=bool(opt.probs_output), uncertainty=measure, **tiled)
            labels, (wt, tc, et) = out[0], out[1]
            if opt.probs_output:
                os.makedirs(opt.probs_output, exist_ok=True)
                np.save(os.path.join(opt.probs_output, name + ".npy"), out[2])
            if measure:
                inference.save_uncertainty(unc_dir, name, out[-1])
        else:
            labels, (wt, tc, et) = inference.predict_case(net, image, **tiled)
        if opt.output:
            dst = opt.output if opt.output.endswith(".npy") and len(cases) == 1 else os.path.join(opt.output, name + ".npy")
            os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
            np.save(dst, labels)
        print(name, labels.shape, labels.dtype, wt, tc, et)


if __name__ == "__main__":
    main()
