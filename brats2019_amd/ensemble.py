"""Ensemble of saved predictions: the reference's average_predicts.ipynb / emsemble_predicts.ipynb (`sum(data_files) / len(data_files)`,
argmax, 3 -> 4) for `.npy` predictions.  Every `--predictions` directory holds one model's outputs under the same file names; the files
found in the first directory are merged across all of them.

    python -m brats2019_amd.ensemble --predictions runA runB runC --output merged [--rule class|regions]

  --rule class    (default, the notebooks') [4,D,H,W] class probabilities -> uint8 labels {0,1,2,4}: argmax over the channels of the mean
                  (first maximum wins), class 3 stored as 4;
  --rule regions  [3,D,H,W] WT/TC/ET probabilities, e.g. what `python -m brats2019_amd.test --probs_output DIR` writes -> mean, 0.5
                  threshold, label composition with the ET > 32 rule and 26-connected component rejection (test.py:144-164).

The sums, the division, the threshold / argmax and the post-processing run on the device (csrc/ensemble.hip, csrc/inference.hip) with one
upload per file and one download per case.  With `--rule regions`, `--uncertainty_output DIR [--uncertainty std|entropy]` also writes the
BraTS uncertainty maps of the saved predictions, taken as members with one copy each (K = 1): uint8 `NAME_unc_whole.npy`, `NAME_unc_core.npy`,
`NAME_unc_enhance.npy`, values 0 (certain) .. 100 (uncertain) (csrc/uncertainty.hip; `inference.uncertainty_*_host` with `--host`).  With `--rule regions`, the flags `--min_volume`, `--min_confidence`, `--keep_largest`,
`--fill_holes`, `--nest`, `--no_reject` of `python -m brats2019_amd.test` post-process the masks of the mean per region before the labels are
composed (csrc/postprocess.hip; `inference.postprocess_regions_host` with `--host`), and `--thresholds WT TC ET` / `--thresholds_file FILE` threshold the mean at these values
instead of 0.5 (csrc/calibration.hip).  `--host` computes the same with numpy and scipy (`inference.ensemble_mean_host`, no GPU).
NIfTI input is out of scope (no nibabel): predictions are arrays.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import inference

parser = argparse.ArgumentParser(description="Average saved predictions of several models (MI355X HIP engine)")
parser.add_argument("--predictions", required=True, type=str, nargs="+", help="one directory of .npy predictions per model")
parser.add_argument("--output", required=True, type=str, help="directory for the merged uint8 label volumes")
parser.add_argument("--rule", default="class", choices=["class", "regions"])
parser.add_argument("--host", action="store_true", help="numpy / scipy instead of the device kernels")
# SUPPRESS: without these flags the namespace does not change
parser.add_argument("--uncertainty", default=argparse.SUPPRESS, choices=["std", "entropy"], help="uncertainty measure of the maps (default std)")
parser.add_argument("--uncertainty_output", default=argparse.SUPPRESS, type=str,
                    help="--rule regions: directory for the uint8 uncertainty maps NAME_unc_whole.npy, NAME_unc_core.npy, NAME_unc_enhance.npy")
inference.add_postprocess_arguments(parser)
inference.add_threshold_arguments(parser)

CHANNELS = {"class": 4, "regions": 3}


def merge_host(preds, rule, postprocess=None, thresholds=None):
    if rule == "class":
        return inference.ensemble_class_labels_host(preds)
    if postprocess is None and thresholds is None:
        return inference.postprocess_labels(inference.compose_labels_host(inference.ensemble_mean_host(preds)))
    mean = inference.ensemble_mean_host(preds)
    t = np.asarray(thresholds if thresholds is not None else (0.5, 0.5, 0.5), dtype=np.float32).reshape(3, 1, 1, 1)
    mask = mean > t
    if postprocess is None:
        return inference.postprocess_labels(inference.compose_masks_host(mask, mask.reshape(3, -1).sum(axis=1)))
    mask, counts = inference.postprocess_regions_host(mask, probs=mean if postprocess.needs_probs else None, **postprocess.regions())
    labels = inference.compose_masks_host(mask, counts)
    return labels if postprocess.reject_ratio is None else inference.postprocess_labels(labels, postprocess.reject_ratio)


def uncertainty_host(preds, measure):
    mean = inference.ensemble_mean_host(preds)
    return inference.uncertainty_std_host([[p] for p in preds], mean) if measure == "std" else inference.uncertainty_entropy_host(mean)


def merge_device(preds, rule, uncertainty=None, postprocess=None, thresholds=None):
    """-> labels, or (labels, uint8 maps [3,D,H,W]) with `uncertainty` (rule "regions")"""
    import torch
    from . import ops
    want_mean = thresholds is not None or (postprocess is not None and postprocess.needs_probs)
    if uncertainty is not None:
        acc, acc2 = None, None
        for p in preds:
            acc, acc2 = ops.unc_accumulate(torch.as_tensor(p, dtype=torch.float32).cuda(), acc=acc, acc2=acc2)
        mask, counts, mean, unc = ops.unc_finalize(acc, acc2, len(preds), 1, uncertainty, want_mean=want_mean)
        return inference._labels_from_masks(mask, counts, mean, postprocess, thresholds)[0].cpu().numpy(), unc.cpu().numpy()
    acc = None
    for p in preds:                                               # one upload at a time: a prediction is folded in before the next arrives
        acc = ops.ens_accumulate(torch.as_tensor(p, dtype=torch.float32).cuda(), acc=acc)
    if rule == "class":
        return ops.ens_argmax(acc, len(preds)).cpu().numpy()
    mask, counts, mean = ops.ens_finalize(acc, len(preds), want_mean=want_mean)
    return inference._labels_from_masks(mask, counts, mean, postprocess, thresholds)[0].cpu().numpy()


def main(argv=None):
    opt = parser.parse_args(argv)
    unc_dir = getattr(opt, "uncertainty_output", None)
    measure = getattr(opt, "uncertainty", "std") if unc_dir else None
    if unc_dir and opt.rule != "regions":
        parser.error("--uncertainty_output needs --rule regions: the maps are per region")
    post = inference.postprocess_from_args(opt)
    if post is not None and opt.rule != "regions":
        parser.error("the post-processing flags need --rule regions: they are per region")
    thr = inference.thresholds_from_args(opt)
    if thr is not None and opt.rule != "regions":
        parser.error("--thresholds and --thresholds_file need --rule regions: they are per region")
    names = sorted(f for f in os.listdir(opt.predictions[0]) if f.endswith(".npy"))
    if not names:
        raise SystemExit("no .npy predictions in %s" % opt.predictions[0])
    os.makedirs(opt.output, exist_ok=True)
    for name in names:
        preds = []
        for d in opt.predictions:
            path = os.path.join(d, name)
            if not os.path.exists(path):
                raise SystemExit("%s is missing from %s" % (name, d))
            p = np.load(path)
            if p.ndim != 4 or p.shape[0] != CHANNELS[opt.rule] or (preds and p.shape != preds[0].shape):
                raise SystemExit("%s: expected [%d,D,H,W] arrays of one shape for --rule %s, got %s" % (path, CHANNELS[opt.rule], opt.rule, p.shape))
            preds.append(p.astype(np.float32, copy=False))
        if measure:
            labels, maps = (merge_host(preds, opt.rule, post, thr), uncertainty_host(preds, measure)) if opt.host else merge_device(preds, opt.rule, measure, post, thr)
            inference.save_uncertainty(unc_dir, name[:-4], maps)
        else:
            labels = merge_host(preds, opt.rule, post, thr) if opt.host else merge_device(preds, opt.rule, postprocess=post, thresholds=thr)
        np.save(os.path.join(opt.output, name), labels)
        print(name, labels.shape, labels.dtype, len(preds), "models", {int(k): int(v) for k, v in zip(*np.unique(labels, return_counts=True))})


if __name__ == "__main__":
    main()
