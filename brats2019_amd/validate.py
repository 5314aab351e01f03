"""Offline scorer with the reference's `validate.py --data_path --predictions_path` contract (validate.py:7-9,51-101): per case the
Dice of labels 1, 2, 3 and of the whole tumour (labels > 0), label 4 counting as 3, and the mean over the cases.  The reference reads
NIfTI through nibabel, which this image lacks; here a case is `<case>.npy` in `data_path` (uint8 ground-truth labels {0,1,2,4},
[D,H,W]) and its prediction `<case>.npy` in `predictions_path`, as `python -m brats2019_amd.test --output DIR` writes it.

Each case is uploaded as uint8 and scored on the device: one label confusion pass and one small launch (ru_label_confusion,
ru_overlap_accumulate), the ratio of the float32-rounded counts in float32 (NaN -> 1) as validate.py forms it from float32 sums.

    python -m brats2019_amd.validate --data_path ./labels --predictions_path ./predictions

`--regions` scores the BraTS challenge's way instead: per case the Dice, sensitivity, specificity and HD95 of the regions WT = {1,2,3,4},
TC = {1,3,4} and ET = {3,4} (3 counts as 4), from one pass sequence of ru_surface_metrics per case (metrics.Hausdorff95 states HD95).

`--lesionwise [--dilation 3] [--min_volume 50]` scores the challenge's lesion-wise ranking numbers instead: per case and region the
lesion-wise Dice and HD95 and the counts of ground-truth, kept, found, missed and false-positive lesions (ru_lesion_metrics; INTEGRATION.md
states the definition).  Not checked against the challenge's own evaluator.

`--nsd TOL [TOL ...]` (with `--regions` or `--lesionwise`) adds the normalized surface Dice at each tolerance (voxels, at most 8): with
`--regions` one NSD row per tolerance and the average symmetric surface distance ASSD, with `--lesionwise` one LesionNSD row per
tolerance, from the same passes (ru_surface_distances, ru_lesion_distances).  The voxel-surface form of NSD; not compared with MONAI's
code or any official evaluator.

`--uncertainty_path DIR [--thresholds 25 50 75 100]` scores the BraTS uncertainty task instead: DIR holds `<case>_unc_whole.npy`,
`<case>_unc_core.npy`, `<case>_unc_enhance.npy` (uint8 [D,H,W], 0 certain .. 100 uncertain) as `python -m brats2019_amd.test
--uncertainty_output DIR` writes them.  At a threshold t the voxels with a map value above t are filtered out and TP, FP, FN, TN of the
region are counted on the rest: Dice_t = 2TP/(2TP+FP+FN) (1 for an empty denominator), FTP_t = (TP_100 - TP_t)/TP_100 (0 for TP_100 = 0),
FTN_t likewise; the AUCs are trapezoid sums over the thresholds divided by their span, score = (AUC_Dice + (1 - AUC_FTP) + (1 - AUC_FTN)) / 3.
One histogram pass and one small launch per case (ru_unc_histogram, ru_unc_score).  Neither the default thresholds nor the
empty-denominator values have been checked against the challenge's own evaluator.

`--calibration --probs_path DIR [--bins 16] [--nb 256] [--thresholds_output FILE] [--host]` scores the calibration of the region probabilities
instead: DIR holds `<case>.npy` float32 [3,D,H,W] (WT, TC, ET) as `python -m brats2019_amd.test --probs_output DIR` writes them.  Per region it
prints ECE, MCE and the Brier score over all cases' voxels, the mean Dice over the cases at 0.5, the threshold b / nb with the best mean Dice
and that Dice, and the reliability table; `--thresholds_output` writes the thresholds as the JSON `test --thresholds_file` reads.  One
histogram pass and one small launch per case, one summary launch (ru_calib_histogram, ru_calib_accumulate, ru_calib_summary; INTEGRATION.md
states the definitions); `--host` computes the same with numpy.  The conventions are this library's own, not checked against another package.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import ops

parser = argparse.ArgumentParser(description="PyTorch BraTS2019 Validate (MI355X HIP engine)")
parser.add_argument("--data_path", default="", type=str, help="directory of <case>.npy ground-truth label volumes")
parser.add_argument("--predictions_path", default="", type=str, help="directory of <case>.npy predicted label volumes")
# SUPPRESS: without the flag the namespace -- and so the printed output -- is the plain scorer's
parser.add_argument("--regions", action="store_true", default=argparse.SUPPRESS,
                    help="score Dice, sensitivity, specificity and HD95 of the regions WT, TC, ET")
parser.add_argument("--uncertainty_path", default=argparse.SUPPRESS, type=str,
                    help="directory of <case>_unc_whole.npy, _unc_core.npy, _unc_enhance.npy: score the uncertainty maps")
parser.add_argument("--thresholds", default=argparse.SUPPRESS, type=int, nargs="+", help="uncertainty thresholds, rising, inside 0..100 (default 25 50 75 100)")
parser.add_argument("--lesionwise", action="store_true", default=argparse.SUPPRESS,
                    help="score the lesion-wise Dice and HD95 of the regions WT, TC, ET")
parser.add_argument("--dilation", default=argparse.SUPPRESS, type=int, help="lesion-wise: dilation iterations that join ground-truth fragments (default 3)")
parser.add_argument("--min_volume", default=argparse.SUPPRESS, type=int, help="lesion-wise: ground-truth lesions of at most this many voxels are not scored (default 50)")
parser.add_argument("--nsd", default=argparse.SUPPRESS, type=float, nargs="+", metavar="TOL",
                    help="with --regions or --lesionwise: add the surface Dice at these tolerances in voxels (and ASSD with --regions)")
parser.add_argument("--calibration", action="store_true", default=argparse.SUPPRESS,
                    help="score the calibration of the region probabilities in --probs_path and search the best threshold per region")
parser.add_argument("--probs_path", default=argparse.SUPPRESS, type=str, help="directory of <case>.npy float32 [3,D,H,W] region probabilities (test.py --probs_output)")
parser.add_argument("--bins", default=argparse.SUPPRESS, type=int, help="calibration: coarse confidence bins, a divisor of --nb (default 16)")
parser.add_argument("--nb", default=argparse.SUPPRESS, type=int, help="calibration: fine bins = candidate thresholds b / nb, a power of two in 16..1024 (default 256)")
parser.add_argument("--thresholds_output", default=argparse.SUPPRESS, type=str, help="calibration: write the chosen thresholds to this JSON file")
parser.add_argument("--host", action="store_true", default=argparse.SUPPRESS, help="calibration: compute with the numpy restatement instead of the device")

UNCERTAINTY_THRESHOLDS = (25, 50, 75, 100)
UNCERTAINTY_COLUMNS = ("score", "AUC_Dice", "AUC_FTP", "AUC_FTN")

REGION_NAMES = ("WT", "TC", "ET")
REGION_METRICS = ("Dice", "Sens", "Spec", "HD95")
LESION_METRICS = ("LesionDice", "LesionHD95")
LESION_COUNTS = ("gt", "kept", "tp", "fn", "fp")

VALID_LABELS = (0, 1, 2, 3, 4)


def _upload(arr, what):
    arr = np.ascontiguousarray(arr)
    if arr.dtype != np.uint8:
        # the kernel counts values outside 0..4 of a uint8 volume; a wider type is checked here, before the cast could hide them
        if arr.size and (arr.min() < 0 or arr.max() > 4 or not np.array_equal(arr, np.round(arr))):
            raise ValueError("%s: labels outside {0,1,2,3,4}" % what)
        arr = arr.astype(np.uint8)
    return torch.from_numpy(arr).cuda()


def score(cases):
    """cases: iterable of (name, ground-truth labels, predicted labels), read one at a time.  -> (names, results float64 [cases, 4],
    mean float64 [4]).  The values stay on the device until the end: one host copy for all cases."""
    names, rows, invalid = [], [], []
    total = torch.zeros(4, dtype=torch.float64, device="cuda")
    for name, label, predict in cases:
        if tuple(label.shape) != tuple(predict.shape):
            raise ValueError("%s: prediction shape %s differs from the label shape %s" % (name, tuple(predict.shape), tuple(label.shape)))
        g, p = _upload(label, name + " (labels)"), _upload(predict, name + " (prediction)")
        conf, inv = ops.label_confusion(p.reshape(1, -1), g.reshape(1, -1))
        row = torch.empty(4, dtype=torch.float64, device="cuda")
        ops.overlap_accumulate(conf, total, 4, "validate", out=row)
        names.append(name)
        rows.append(row)
        invalid.append(inv)
    if not names:
        raise ValueError("validate: no cases")
    bad = torch.cat(invalid).cpu().numpy()
    if bad.any():
        k = int(np.argmax(bad > 0))
        raise ValueError("%s: labels outside {0,1,2,3,4} in %d voxels" % (names[k], int(bad[k])))
    return names, torch.stack(rows).cpu().numpy(), total.cpu().numpy() / len(names)


def _nsd_names(prefix, nsd):
    return tuple("%s@%g" % (prefix, t) for t in nsd)


def score_regions(cases, nsd=None):
    """cases: iterable of (name, ground-truth labels, predicted labels), read one at a time.  -> (names, results float64 [cases, 4, 3],
    mean float64 [4, 3]): rows Dice, sensitivity, specificity, HD95; columns WT, TC, ET.  The values stay on the device until the end:
    one host copy for all cases.  With `nsd` (T tolerances in voxels): results [cases, 4 + T + 1, 3], the further rows NSD per
    tolerance and ASSD."""
    if nsd is not None:
        nsd = [float(t) for t in nsd]
        ops.tolerance_bins(nsd)                                                       # a bad list fails before any upload
    nex = 0 if nsd is None else len(nsd) + 1
    names, rows = [], []
    for name, label, predict in cases:
        if tuple(label.shape) != tuple(predict.shape) or np.ndim(label) != 3:
            raise ValueError("%s: prediction shape %s and label shape %s must be one [D, H, W]" % (name, tuple(predict.shape), tuple(label.shape)))
        g, p = _upload(label, name + " (labels)"), _upload(predict, name + " (prediction)")
        if nsd is None:
            values, counts = ops.surface_metrics(p[None], g[None])              # [1, 3, 4], [1, 3, 6]
        else:
            values, counts, extras = ops.surface_distances(p[None], g[None], nsd)           # and [1, 3, T + 2]
            values = torch.cat([values, extras[..., :nex]], dim=2)
        names.append(name)
        rows.append(torch.cat([values.reshape(-1), counts[0, 0, 5:].to(torch.float64)]))
    if not names:
        raise ValueError("validate: no cases")
    host = torch.stack(rows).cpu().numpy()
    bad = host[:, -1]
    if bad.any():
        k = int(np.argmax(bad > 0))
        raise ValueError("%s: labels outside {0,1,2,3,4} in %d voxels" % (names[k], int(bad[k])))
    results = np.ascontiguousarray(host[:, :-1].reshape(len(names), 3, 4 + nex).transpose(0, 2, 1))
    return names, results, results.mean(axis=0)


def score_lesionwise(cases, dilation=3, min_volume=50, nsd=None):
    """cases: iterable of (name, ground-truth labels, predicted labels), read one at a time.  -> (names, results float64 [cases, 2, 3],
    mean float64 [2, 3], counts int64 [cases, 3, 5]): rows lesion-wise Dice and HD95; columns WT, TC, ET; counts n_gt, n_kept, n_tp, n_fn,
    n_fp per region.  The values stay on the device until the end: one host copy for all cases.  With `nsd` (T tolerances in voxels):
    results [cases, 2 + T, 3], the further rows LesionNSD per tolerance."""
    if int(dilation) < 0 or int(min_volume) < 0:
        raise ValueError("validate: dilation %s and min_volume %s must be >= 0" % (dilation, min_volume))
    if nsd is not None:
        nsd = [float(t) for t in nsd]
        ops.tolerance_bins(nsd)
    nex = 0 if nsd is None else len(nsd)
    names, rows = [], []
    for name, label, predict in cases:
        if tuple(label.shape) != tuple(predict.shape) or np.ndim(label) != 3:
            raise ValueError("%s: prediction shape %s and label shape %s must be one [D, H, W]" % (name, tuple(predict.shape), tuple(label.shape)))
        g, p = _upload(label, name + " (labels)"), _upload(predict, name + " (prediction)")
        if nsd is None:
            summary, counts = ops.lesion_metrics(p[None], g[None], dilation=dilation, min_volume=min_volume)     # [1, 3, 2], [1, 3, 6]
        else:
            summary, counts, ex = ops.lesion_distances(p[None], g[None], nsd, dilation=dilation, min_volume=min_volume)     # and [1, 3, T + 1]
            summary = torch.cat([summary, ex[..., :nex]], dim=2)
        names.append(name)
        rows.append(torch.cat([summary.reshape(-1), counts.reshape(-1).to(torch.float64)]))
    if not names:
        raise ValueError("validate: no cases")
    host = torch.stack(rows).cpu().numpy()
    nv = 3 * (2 + nex)
    counts = host[:, nv:].reshape(len(names), 3, 6).astype(np.int64)
    bad = counts[:, 0, 5]
    if bad.any():
        k = int(np.argmax(bad > 0))
        raise ValueError("%s: labels outside {0,1,2,3,4} in %d voxels" % (names[k], int(bad[k])))
    results = np.ascontiguousarray(host[:, :nv].reshape(len(names), 3, 2 + nex).transpose(0, 2, 1))
    return names, results, results.mean(axis=0), np.ascontiguousarray(counts[:, :, :5])


def score_uncertainty(cases, thresholds=UNCERTAINTY_THRESHOLDS):
    """cases: iterable of (name, ground-truth labels [D,H,W], predicted labels [D,H,W], uncertainty maps uint8 [3,D,H,W] in the order WT,
    TC, ET), read one at a time.  -> (names, results float64 [cases, 3, 4], mean float64 [3, 4]): rows WT, TC, ET; columns score,
    AUC_Dice, AUC_FTP, AUC_FTN over the rising integer `thresholds`.  The values stay on the device until the end: one host copy for
    all cases."""
    thresholds = [int(t) for t in thresholds]
    if not thresholds or thresholds[0] < 0 or thresholds[-1] > 100 or any(b <= a for a, b in zip(thresholds, thresholds[1:])):
        raise ValueError("validate: the thresholds must rise strictly inside 0..100, got %s" % (thresholds,))
    names, rows, total = [], [], None
    for name, label, predict, maps in cases:
        if np.ndim(label) != 3 or tuple(predict.shape) != tuple(label.shape) or tuple(np.shape(maps)) != (3,) + tuple(label.shape):
            raise ValueError("%s: label shape %s, prediction shape %s and uncertainty shape %s must be [D,H,W], [D,H,W], [3,D,H,W]"
                             % (name, tuple(label.shape), tuple(predict.shape), tuple(np.shape(maps))))
        maps = np.ascontiguousarray(maps)
        if maps.dtype != np.uint8:
            # the kernel counts values above 100 of a uint8 map; a wider type is checked here, before the cast could hide them
            if maps.size and (maps.min() < 0 or maps.max() > 100 or not np.array_equal(maps, np.round(maps))):
                raise ValueError("%s: uncertainty values outside the integers 0..100" % name)
            maps = maps.astype(np.uint8)
        g, p = _upload(label, name + " (labels)"), _upload(predict, name + " (prediction)")
        if total is None:
            total = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
        hist, inv = ops.unc_histogram(p, g, torch.from_numpy(maps).cuda())
        row = torch.empty(13, dtype=torch.float64, device="cuda")
        ops.unc_score(hist, thresholds, acc=total, out=row[:12])
        row[12:] = inv
        names.append(name)
        rows.append(row)
    if not names:
        raise ValueError("validate: no cases")
    rows.append(torch.cat([total.reshape(-1), total.new_zeros(1)]))                   # the sums travel with the rows: one copy
    host = torch.stack(rows).cpu().numpy()
    bad = host[:-1, 12]
    if bad.any():
        k = int(np.argmax(bad > 0))
        raise ValueError("%s: labels outside {0,1,2,3,4} or uncertainty values above 100 in %d voxels" % (names[k], int(bad[k])))
    return names, np.ascontiguousarray(host[:-1, :12].reshape(len(names), 3, 4)), host[-1, :12].reshape(3, 4) / len(names)


CALIBRATION_COLUMNS = ("ECE", "MCE", "Brier", "mean_conf", "prevalence", "n", "bins_used")


def score_calibration(cases, nb=256, bins=16, host=False):
    """cases: iterable of (name, ground-truth labels uint8 [D,H,W], region probabilities float32 [3,D,H,W] in the order WT, TC, ET), read
    one at a time.  One histogram pass and one small launch per case (ru_calib_histogram, ru_calib_accumulate), one summary launch and
    one host copy at the end.  -> dict: `names`; `curves` float64 [cases,3,3,nb+1] (region; Dice, Sens, Spec; threshold b / nb);
    `mean_curve` [3,3,nb+1]; `summary` [3,7] (CALIBRATION_COLUMNS) and `table` [3,bins,3] (n_m, conf_m, freq_m) over all cases' voxels;
    `best_bin` [3], `thresholds` [3] = best_bin / nb (metrics.choose_threshold on the mean Dice curve), `dice` [3] there and
    `dice_at_half` [3] at 0.5.  host=True computes the same with the numpy restatement (metrics.calibration_host), without a GPU."""
    from . import metrics
    nb, bins = int(nb), int(bins)
    if not (16 <= nb <= 1024 and nb & (nb - 1) == 0) or bins < 1 or nb % bins:
        raise ValueError("validate: nb = %d must be a power of two in 16..1024 and bins = %d must divide it" % (nb, bins))
    names, curves, invalid, pool = [], [], [], None
    for name, label, probs in cases:
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        if np.ndim(label) != 3 or tuple(probs.shape) != (3,) + tuple(label.shape):
            raise ValueError("%s: label shape %s and probability shape %s must be [D,H,W] and [3,D,H,W]" % (name, tuple(label.shape), tuple(probs.shape)))
        label = np.ascontiguousarray(label)
        if label.dtype != np.uint8:
            if label.size and (label.min() < 0 or label.max() > 4 or not np.array_equal(label, np.round(label))):
                raise ValueError("%s (labels): labels outside {0,1,2,3,4}" % name)
            label = label.astype(np.uint8)
        if host:
            h = metrics.calibration_host(probs[None], label[None], nb, bins)
            if pool is None:
                pool = [np.zeros_like(h["pool_hist"]), np.zeros_like(h["pool_conf"]), [[0, 0] for _ in range(3)], np.zeros_like(h["curve_sum"])]
            pool[0] += h["pool_hist"]
            pool[1] += h["pool_conf"]
            pool[2] = [[a + b for a, b in zip(x, y)] for x, y in zip(pool[2], h["pool_s2"])]
            pool[3] = pool[3] + h["curve_sum"]
            curves.append(h["curves"][0])
            invalid.append(h["invalid"][0])
        else:
            p, g = torch.from_numpy(probs).cuda(), torch.from_numpy(label).cuda()
            hist, conf, sq, inv = ops.calib_histogram(p[None], g[None], nb)
            if pool is None:
                pool = ops.calib_pool(3, nb, p.device)
            curves.append(ops.calib_accumulate(hist, conf, sq, pool, want_curves=True)[0])
            invalid.append(inv[0])
        names.append(name)
    if not names:
        raise ValueError("validate: no cases")
    if host:
        rows = [metrics.calibration_summary_host(pool[0][c], pool[1][c], pool[2][c], bins) for c in range(3)]
        summary, table = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        curves, bad, curve_sum = np.stack(curves), np.stack(invalid), pool[3]
    else:
        out, tab = ops.calib_summary(pool[0], pool[1], pool[2], bins)
        flat = torch.cat([torch.stack(curves).reshape(-1), pool[3].reshape(-1), out.reshape(-1), tab.reshape(-1),
                          torch.stack(invalid).reshape(-1).to(torch.float64)]).cpu().numpy()          # the one host copy
        k = 9 * (nb + 1)
        cuts = np.cumsum([len(names) * k, k, 21, 9 * bins])
        curves, curve_sum, summary, table, bad = np.split(flat, cuts)
        curves, curve_sum = curves.reshape(len(names), 3, 3, nb + 1), curve_sum.reshape(3, 3, nb + 1)
        summary, table, bad = summary.reshape(3, 7), table.reshape(3, bins, 3), bad.reshape(len(names), 3)
    if bad.any():
        k = int(np.argmax(bad.sum(axis=1) > 0))
        raise ValueError("%s: %d voxels with a label outside {0,1,2,3,4} or a probability outside [0, 1]" % (names[k], int(bad[k].max())))
    mean_curve = curve_sum / len(names)
    best = [metrics.choose_threshold(mean_curve[c, 0]) for c in range(3)]
    return {"names": names, "curves": curves, "mean_curve": mean_curve, "summary": summary, "table": table, "best_bin": best, "nb": nb,
            "thresholds": [b / nb for b in best], "dice": [float(mean_curve[c, 0, best[c]]) for c in range(3)],
            "dice_at_half": [float(mean_curve[c, 0, nb // 2]) for c in range(3)]}


def write_thresholds(path, res):
    """the small JSON `python -m brats2019_amd.test --thresholds_file` and `ensemble --thresholds_file` read"""
    import json
    with open(path, "w") as f:
        json.dump({"thresholds": [float(t) for t in res["thresholds"]], "nb": int(res["nb"]), "dice": [float(v) for v in res["dice"]],
                   "dice_at_half": [float(v) for v in res["dice_at_half"]]}, f)
        f.write("\n")


def _calibration_lines(res):
    lines = []
    for c, region in enumerate(REGION_NAMES):
        s = res["summary"][c]
        lines.append("%s ECE %.6f MCE %.6f Brier %.6f Dice@0.5 %.4f best_threshold %.6f Dice@best %.4f" %
                     (region, s[0], s[1], s[2], res["dice_at_half"][c], res["thresholds"][c], res["dice"][c]))
        m = len(res["table"][c])
        for b, (n, cf, fr) in enumerate(res["table"][c]):
            lines.append("%s bin %2d (%.4f, %.4f] n %d conf %.6f freq %.6f" % (region, b, b / m, (b + 1) / m, int(n), cf, fr))
    return lines


def _uncertainty_row(r):
    return "  ".join("%s %s" % (n, " ".join("%s %.4f" % (k, v) for k, v in zip(UNCERTAINTY_COLUMNS, row))) for n, row in zip(REGION_NAMES, r))


def _uncertainty_cases(opt, series):
    from .inference import UNCERTAINTY_STEMS
    for f in series:
        maps = [np.load(os.path.join(opt.uncertainty_path, "%s_unc_%s.npy" % (f, stem))) for stem in UNCERTAINTY_STEMS]
        if any(m.shape != maps[0].shape for m in maps):
            raise ValueError("%s: the three uncertainty maps have different shapes %s" % (f, [m.shape for m in maps]))
        yield f, np.load(os.path.join(opt.data_path, f + ".npy")), np.load(os.path.join(opt.predictions_path, f + ".npy")), np.stack(maps)


def _region_row(r, nsd=()):
    metrics = REGION_METRICS + ((_nsd_names("NSD", nsd) + ("ASSD",)) if len(r) > len(REGION_METRICS) else ())
    return "  ".join("%s %s" % (m, " ".join("%s %.4f" % (k, v) for k, v in zip(REGION_NAMES, row))) for m, row in zip(metrics, r))


def _lesion_row(r, counts=None, nsd=()):
    metrics = LESION_METRICS + _nsd_names("LesionNSD", nsd)
    row = "  ".join("%s %s" % (m, " ".join("%s %.4f" % (k, v) for k, v in zip(REGION_NAMES, vals))) for m, vals in zip(metrics, r))
    if counts is None:
        return row
    return row + "  " + "  ".join("%s %s" % (n, " ".join("%s %d" % (k, v) for k, v in zip(LESION_COUNTS, c))) for n, c in zip(REGION_NAMES, counts))


def main(argv=None):
    """-> (per-case results float64 [cases, 4] = [d1, d2, d3, dWT], their mean).  With --regions: (results float64 [cases, 4, 3], their
    mean [4, 3]), rows Dice, sensitivity, specificity, HD95 and columns WT, TC, ET.  With --uncertainty_path: (results float64 [cases, 3, 4],
    their mean [3, 4]), rows WT, TC, ET and columns score, AUC_Dice, AUC_FTP, AUC_FTN.  With --lesionwise: (results float64 [cases, 2, 3],
    their mean [2, 3]), rows lesion-wise Dice and HD95 and columns WT, TC, ET.  --nsd adds rows to the last two (score_regions,
    score_lesionwise)."""
    opt = parser.parse_args(argv)
    print(torch.__version__)
    print(opt)
    series = sorted(f[:-4] for f in os.listdir(opt.data_path) if f.endswith(".npy") and os.path.isfile(os.path.join(opt.data_path, f)))
    if getattr(opt, "calibration", False):
        if not getattr(opt, "probs_path", None):
            raise ValueError("validate: --calibration needs --probs_path")
        cases = ((f, np.load(os.path.join(opt.data_path, f + ".npy")), np.load(os.path.join(opt.probs_path, f + ".npy"))) for f in series)
        res = score_calibration(cases, getattr(opt, "nb", 256), getattr(opt, "bins", 16), getattr(opt, "host", False))
        for line in _calibration_lines(res):
            print(line)
        if getattr(opt, "thresholds_output", None):
            write_thresholds(opt.thresholds_output, res)
        return res["summary"], res["thresholds"]
    if getattr(opt, "uncertainty_path", None):
        series, results, mean = score_uncertainty(_uncertainty_cases(opt, series), getattr(opt, "thresholds", UNCERTAINTY_THRESHOLDS))
        for f, r in zip(series, results):
            print(f, _uncertainty_row(r))
        print("mean", _uncertainty_row(mean))
        return results, mean
    cases = ((f, np.load(os.path.join(opt.data_path, f + ".npy")), np.load(os.path.join(opt.predictions_path, f + ".npy"))) for f in series)
    nsd = getattr(opt, "nsd", None)
    if getattr(opt, "lesionwise", False):
        series, results, mean, counts = score_lesionwise(cases, getattr(opt, "dilation", 3), getattr(opt, "min_volume", 50), nsd)
        for f, r, c in zip(series, results, counts):
            print(f, _lesion_row(r, c, nsd or ()))
        print("mean", _lesion_row(mean, None, nsd or ()))
        return results, mean
    if getattr(opt, "regions", False):
        series, results, mean = score_regions(cases, nsd)
        for f, r in zip(series, results):
            print(f, _region_row(r, nsd or ()))
        print("mean", _region_row(mean, nsd or ()))
        return results, mean
    series, results, mean = score(cases)
    for f, r in zip(series, results):
        print(f, str(r))
    print(mean)
    return results, mean


if __name__ == "__main__":
    main()
