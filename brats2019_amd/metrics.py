"""Drop-in for the part of the reference's `metrics` module that the hot path's Trainer uses: the `Metrics` accumulator
protocol (metrics.py:6-20: name / update / get / reset), `Dice` (metrics.py:101-133) -- threshold 0.5, per sample and
channel 2*sum(p*g)/sum(p+g) (NaN -> 1), mean over the batch, accumulated over update() calls -- and the Hausdorff distances
`Hausdorff_ITK` / `Hausdorff_ITKWT` (metrics.py:188-271) that main.py:149-151 validates with, in SimpleITK's definition (unit
spacing, voxel centres) without SimpleITK: an exact squared distance transform on the device (ru_hausdorff_sq), then the
reference's bookkeeping -- 1e6 for an empty mask, its i-1 index slip, the float64 batch mean -- in one more launch.  The counting runs on
the device (ru_dice_counts, ru_hausdorff_sq) and the running sums stay there: `update` never synchronises, `get()` copies a few numbers
to the host.  `update(ground, predict)` keeps the reference's argument order (train.py:304).

The rest of the reference's metrics.py: `Dice1D`, `RMSE`, `RMSE_masked`, `DiceWT`, `Dice_ITK` (metrics.py:22-185) and `print_metrics`
(metrics.py:273-280).  DiceWT and Dice_ITK read one per-sample label confusion matrix (ru_label_confusion), Dice1D the Dice counts,
RMSE the squared-difference moment; a small launch turns each into the batch mean on the device (ru_overlap_accumulate,
ru_dice1d_accumulate, ru_rmse_accumulate).

Beyond the reference: the BraTS challenge's `Hausdorff95`, `Sensitivity` and `Specificity`, per channel on the `> 0.5` masks, from one
pass sequence on the device (ru_surface_metrics: bit-packed masks and surfaces, an exact squared distance transform that fills a
histogram of surface distances, an exact order statistic) and its accumulate launch (ru_surface_accumulate); and the challenge's
lesion-wise ranking numbers `LesionWiseDice` and `LesionWiseHausdorff95` (ru_lesion_metrics, ru_lesion_accumulate).  From the same
histogram of surface distances: `SurfaceDice` (NSD at a tolerance), `AverageSurfaceDistance` (ASSD) and `LesionWiseSurfaceDice`
(ru_surface_distances, ru_lesion_distances, ru_surface_extras_accumulate), and their float64 numpy / scipy restatements
`surface_distances_host` and `lesion_distances_host`, which the tests hold the device to.

Calibration and the operating point: `ExpectedCalibrationError`, `BrierScore` and `DiceAtThreshold` pool the integer tables of one binning
pass over (probability, target) on the device (ru_calib_histogram, ru_calib_accumulate, ru_calib_summary, ru_threshold_regions);
`calibration_host` restates tables, curves and summary in numpy from the definitions in INTEGRATION.md, and `choose_threshold` picks the
threshold from a mean Dice curve."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


class Metrics(object):
    def __init__(self, name):
        self.name = name
        self.accumulator = 0.0
        self.samples = 0.0

    def update(self, ground, predict):
        self.samples = self.samples + 1

    def get(self):
        return self.accumulator / self.samples

    def reset(self):
        self.accumulator = 0.0
        self.samples = 0.0


class Dice(Metrics):
    def __init__(self, name="Dice", input_index=0, target_index=0, classes=4):
        super(Dice, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.classes = classes

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        counts = ops.dice_counts(pred.cuda(), gr.cuda())                        # [N,C,2] int64, stays on the device: no host sync per update
        nacc = self.classes - 1
        if nacc <= int(counts.shape[1]) and nacc <= 64:
            # ratio (float32, 0/0 -> NaN -> 1), batch mean and accumulation (float64) in one tiny launch: metrics.py:124-130 without a
            # dozen ATen passes over 12 numbers per training step
            if not isinstance(self.accumulator, torch.Tensor):
                self.accumulator = torch.full((nacc,), float(self.accumulator), dtype=torch.float64, device=counts.device)
            ops.dice_accumulate(counts, self.accumulator, nacc)
        else:
            cf = counts.to(torch.float32)
            r = ((2 * cf[..., 0]) / cf[..., 1]).to(torch.float64)               # float32 division like metrics.py:126 (0/0 -> NaN)
            r = torch.where(torch.isnan(r), torch.ones_like(r), r)              # metrics.py:127
            self.accumulator = self.accumulator + r[:, :nacc].mean(dim=0)
        self.samples += 1

    def get(self):
        acc = self.accumulator
        if isinstance(acc, torch.Tensor):
            acc = acc.cpu().numpy()                                             # the one device -> host copy, when the value is asked for
        return acc / self.samples


class Hausdorff_ITK(Metrics):
    """metrics.py:188-230: per sample and channel i < classes-1 the symmetric Hausdorff distance of `pred > 0.5` and `gr > 0.5`; 1e6 when
    one mask is empty (ITK raises; the reference's message print is left out, it would need a host sync); when both are empty the reference
    zeroes column i-1 instead of i -- reproduced, see ru_hausdorff_accumulate.  get(): float64 array [classes-1]."""

    def __init__(self, name="Hausdorff_ITK", input_index=0, target_index=0, classes=5):
        super(Hausdorff_ITK, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.classes = classes

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        nacc = self.classes - 1
        if nacc < 1 or nacc > int(pred.shape[1]) or nacc > 64:
            raise IndexError("Hausdorff_ITK: classes=%d needs 1 <= classes-1 <= %d channels" % (self.classes, min(int(pred.shape[1]), 64)))
        sq = ops.hausdorff_sq(pred.cuda(), gr.cuda(), mode=0)                 # [N,C,4] int64, stays on the device
        if not isinstance(self.accumulator, torch.Tensor):
            self.accumulator = torch.full((nacc,), float(self.accumulator), dtype=torch.float64, device=sq.device)
        ops.hausdorff_accumulate(sq, self.accumulator, nacc, mode=0)
        self.samples += 1

    def get(self):
        acc = self.accumulator
        if isinstance(acc, torch.Tensor):
            acc = acc.cpu().numpy()                                             # the one device -> host copy
        return acc / self.samples


class Hausdorff_ITKWT(Metrics):
    """metrics.py:232-265: the whole-tumour mask `argmax over dim 1 > 0` per sample; 1e6 when either mask is empty (both included, ITK
    raises then too).  get(): a float64 scalar."""

    def __init__(self, name="Hausdorff_ITKWT", input_index=0, target_index=0):
        super(Hausdorff_ITKWT, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        sq = ops.hausdorff_sq(pred.cuda(), gr.cuda(), mode=1)                 # [N,1,4] int64, stays on the device
        if not isinstance(self.accumulator, torch.Tensor):
            self.accumulator = torch.full((1,), float(self.accumulator), dtype=torch.float64, device=sq.device)
        ops.hausdorff_accumulate(sq, self.accumulator, 1, mode=1)
        self.samples += 1

    def get(self):
        acc = self.accumulator
        if isinstance(acc, torch.Tensor):
            acc = acc.cpu().numpy()                                             # the one device -> host copy
        if isinstance(acc, np.ndarray):
            acc = acc.reshape(-1)[0]                                            # a scalar, like the reference's result.mean()
        return acc / self.samples


def _acc(m, n, device):
    if not isinstance(m.accumulator, torch.Tensor):
        m.accumulator = torch.full((n,), float(m.accumulator), dtype=torch.float64, device=device)
    return m.accumulator


def _get_array(m):
    acc = m.accumulator
    if isinstance(acc, torch.Tensor):
        acc = acc.cpu().numpy()                                                 # the one device -> host copy
    return acc / m.samples


def _get_scalar(m):
    acc = _get_array(m)
    return acc.reshape(-1)[0] if isinstance(acc, np.ndarray) else acc       # a scalar, like the reference's


def confusion_torch(pred, gr):
    """label_confusion's kind-0 counts with torch ops on the device (argmax, bincount): the path for more channels than the kernel counts."""
    n, c = int(pred.shape[0]), int(pred.shape[1])
    a = torch.argmax(pred.reshape(n, c, -1), dim=1)
    b = torch.argmax(gr.reshape(n, c, -1), dim=1)
    idx = (torch.arange(n, device=pred.device).view(n, 1) * c + a) * c + b
    return torch.bincount(idx.reshape(-1), minlength=n * c * c).view(n, c, c)


def _confusion(pred, gr):
    if int(pred.shape[1]) > _lib.OVERLAP_MAX_LABELS:
        return confusion_torch(pred.float(), gr.float())
    return ops.label_confusion(pred, gr)[0]


class Dice1D(Metrics):
    """metrics.py:22-52: per sample and channel c < classes, r = 2*sum(p*g) / (sum(p+g) + 1e-6) on the `> 0.5` masks in float32; the batch
    mean and the accumulator in float64.  classes > C raises IndexError (the reference's pred[:, i] does; the default classes=4 against
    the model's 3 outputs does so).  get(): float64 array [classes]."""

    def __init__(self, name="Dice1D", input_index=0, target_index=0, classes=4):
        super(Dice1D, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.classes = classes

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        if self.classes > int(pred.shape[1]) or self.classes > 64:
            raise IndexError("Dice1D: classes=%d, but the tensors have %d channels" % (self.classes, int(pred.shape[1])))
        counts = ops.dice_counts(pred.cuda(), gr.cuda())                        # [N,C,2] int64 on the device
        ops.dice1d_accumulate(counts, _acc(self, self.classes, counts.device), self.classes)
        self.samples += 1

    def get(self):
        return _get_array(self)


class RMSE(Metrics):
    """metrics.py:54-73: sqrt(mean((pred - gr)^2)) over the whole tensor.  `data_parallel` (default False): Trainer.train sets it on its
    train metrics when world > 1, and update() then all-reduces the two sums before the square root, so the value is the global batch's,
    as the reference computes it on the gathered batch.  get(): a float64 scalar."""

    def __init__(self, name="RMSE", input_index=0, target_index=0):
        super(RMSE, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.data_parallel = False

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        sums = ops.rmse_sums(pred.cuda(), gr.cuda())                            # [sum d^2, count] float64 on the device
        if self.data_parallel:
            from .loss import _all_reduce_sums
            _all_reduce_sums(sums, self.data_parallel)
        ops.rmse_accumulate(sums, _acc(self, 1, sums.device))
        self.samples += 1

    def get(self):
        return _get_scalar(self)


class RMSE_masked(Metrics):
    """metrics.py:75-99 with plain torch ops on the device and the reference's broadcasting: the mask sum(mask, dim=(2, 3)) > 0 has the
    shape [N, min(C, 2), W, 1] and is broadcast against [N, C, D, H, W], so the metric is defined only for degenerate shapes such as
    [1, 2, 2, H, H] and raises (RuntimeError) where the reference raises.  get(): a float64 scalar."""

    def __init__(self, name="RMSE_masked", input_index=0, target_index=0, target_index_mask=0):
        super(RMSE_masked, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.target_index_mask = target_index_mask

    def update(self, ground, predict):
        pred = predict[self.input_index].detach().cuda()
        gr = ground[self.target_index].detach().cuda()
        mask = ground[self.target_index_mask].detach().cuda()
        assert gr.shape == pred.shape
        mask = torch.unsqueeze((torch.sum(mask, dim=(2, 3)) > 0).float(), dim=3)[:, :2]
        mse = torch.sum(mask * (pred - gr) ** 2) / (torch.sum(mask) + 1e-8)
        _acc(self, 1, pred.device).add_(torch.sqrt(mse.mean()).to(torch.float64))
        self.samples += 1

    def get(self):
        return _get_scalar(self)


class DiceWT(Metrics):
    """metrics.py:135-155: whole-tumour Dice of `argmax over dim 1 > 0` per sample, 2*I / (|P| + |G| + 1e-6) in float32 (both empty: 0),
    the batch mean accumulated (float64 here; the reference's accumulator ends float32).  get(): a float64 scalar."""

    def __init__(self, name="Dice_WT", input_index=0, target_index=0):
        super(DiceWT, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        conf = _confusion(pred.cuda(), gr.cuda())                               # [N,C,C] int64 on the device
        ops.overlap_accumulate(conf, _acc(self, 1, conf.device), 1, "wt")
        self.samples += 1

    def get(self):
        return _get_scalar(self)


class Dice_ITK(Metrics):
    """metrics.py:157-185: per sample and label i = 1..classes-1 of `argmax over dim 1`, the Dice of SimpleITK's
    LabelOverlapMeasuresImageFilter on the two binary images (pred == i, gr == i): J = I/(P+G-I), 2J/(1+J) in float64, without
    SimpleITK.  A label absent from both images -- always so for i >= C, e.g. columns 3 and 4 of the default classes=5 against 3
    channels -- gives ops.OVERLAP_BOTH_EMPTY (NaN), and the column's mean with it.  That value was not checked against SimpleITK, whose
    versions differ there.  get(): float64 array [classes-1]."""

    def __init__(self, name="Dice_ITK", input_index=0, target_index=0, classes=5):
        super(Dice_ITK, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.classes = classes

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        nacc = self.classes - 1
        if nacc < 1 or nacc > 64:
            raise ValueError("Dice_ITK: classes=%d, 2..65" % self.classes)
        conf = _confusion(pred.cuda(), gr.cuda())                               # [N,C,C] int64 on the device
        ops.overlap_accumulate(conf, _acc(self, nacc, conf.device), nacc, "itk")
        self.samples += 1

    def get(self):
        return _get_array(self)


class _ColumnMetric(Metrics):
    """One column of a per-(sample, channel) device scorer on `pred > 0.5` and `gr > 0.5`, channels i < classes-1; update() adds the batch
    mean to the float64 device accumulator and never reads it back.  A subclass supplies _score (the op: a float64 device tensor
    [N,C,columns]) and _accumulate (its column-mean op).  get(): float64 array [classes-1]."""
    column = None

    def __init__(self, name, input_index, target_index, classes):
        super(_ColumnMetric, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.classes = classes

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        nacc = self.classes - 1
        if nacc < 1 or nacc > int(pred.shape[1]) or nacc > 64:
            raise IndexError("%s: classes=%d needs 1 <= classes-1 <= %d channels" % (self.name, self.classes, min(int(pred.shape[1]), 64)))
        values = self._score(pred.cuda(), gr.cuda())                                   # stays on the device
        self._accumulate(values, _acc(self, nacc, values.device), nacc, self.column)
        self.samples += 1

    def get(self):
        return _get_array(self)


class _SurfaceMetric(_ColumnMetric):
    """A column of ops.surface_metrics ([N,C,4])."""
    empty_value = ops.HD95_EMPTY                                                   # HD95's value for one empty mask; not read by the others
    _accumulate = staticmethod(ops.surface_accumulate)

    def _score(self, pred, gr):
        return ops.surface_metrics(pred, gr, self.empty_value)[0]


class Hausdorff95(_SurfaceMetric):
    """The 95th-percentile symmetric surface distance (HD95) of the BraTS challenge, in voxels at unit spacing: the surfaces are the
    mask voxels with a face neighbour outside the mask or the grid, and the value is numpy.percentile of the distances from each surface
    voxel to the other surface, both directions pooled (medpy.metric.binary.hd95 with connectivity=1; medpy itself was not run here).
    Both masks empty: 0.  Exactly one empty: `empty_value`, by default 373.12866 = sqrt(240^2 + 240^2 + 155^2), the diagonal of a BraTS
    volume -- a convention commonly used for BraTS leaderboards that was NOT checked against the official evaluation."""
    column = "hd95"

    def __init__(self, name="Hausdorff95", input_index=0, target_index=0, classes=4, empty_value=ops.HD95_EMPTY):
        super(Hausdorff95, self).__init__(name, input_index, target_index, classes)
        self.empty_value = empty_value


class Sensitivity(_SurfaceMetric):
    """TP / |G| per sample and channel (1 when G is empty), from exact voxel counts in float64."""
    column = "sensitivity"

    def __init__(self, name="Sensitivity", input_index=0, target_index=0, classes=4):
        super(Sensitivity, self).__init__(name, input_index, target_index, classes)


class Specificity(_SurfaceMetric):
    """TN / (V - |G|) per sample and channel (1 when G fills the volume), from exact voxel counts in float64."""
    column = "specificity"

    def __init__(self, name="Specificity", input_index=0, target_index=0, classes=4):
        super(Specificity, self).__init__(name, input_index, target_index, classes)


class _LesionMetric(_ColumnMetric):
    """A column of ops.lesion_metrics' summary ([N,C,2]); this op reads the lesion counts back, so update() synchronises."""
    _accumulate = staticmethod(ops.lesion_accumulate)

    def __init__(self, name, input_index, target_index, classes, empty_value, dilation, min_volume):
        super(_LesionMetric, self).__init__(name, input_index, target_index, classes)
        self.empty_value = empty_value
        self.dilation = dilation
        self.min_volume = min_volume

    def _score(self, pred, gr):
        return ops.lesion_metrics(pred, gr, self.dilation, self.min_volume, self.empty_value)[0]


class LesionWiseDice(_LesionMetric):
    """The BraTS challenge's lesion-wise Dice (its ranking number since 2023): the ground-truth lesions are the 26-connected components of
    the mask dilated `dilation` times (18-neighbour structure), each is scored against the union of the predicted components that meet
    its dilated component, every predicted component that meets none counts as a lesion of Dice 0, and lesions of at most `min_volume`
    voxels are not scored (include/resunet_hip.h, ru_lesion_metrics).  NOT checked against the official evaluator."""
    column = "dice"

    def __init__(self, name="LesionWiseDice", input_index=0, target_index=0, classes=4, empty_value=ops.HD95_EMPTY, dilation=3, min_volume=50):
        super(LesionWiseDice, self).__init__(name, input_index, target_index, classes, empty_value, dilation, min_volume)


class LesionWiseHausdorff95(_LesionMetric):
    """The lesion-wise HD95 of the same matching: Hausdorff95's value per lesion, `empty_value` for a missed lesion and for every false
    positive component.  NOT checked against the official evaluator (its penalty is a constant near 374)."""
    column = "hd95"

    def __init__(self, name="LesionWiseHausdorff95", input_index=0, target_index=0, classes=4, empty_value=ops.HD95_EMPTY, dilation=3, min_volume=50):
        super(LesionWiseHausdorff95, self).__init__(name, input_index, target_index, classes, empty_value, dilation, min_volume)


class _ExtrasMetric(_ColumnMetric):
    """A column (an index) of ops.surface_distances' extras or ops.lesion_distances' summary_ex, rows of any width."""
    _accumulate = staticmethod(ops.surface_extras_accumulate)


class SurfaceDice(_ExtrasMetric):
    """The normalized surface Dice (NSD, "surface Dice at tolerance tau") per channel on the `> 0.5` masks: the share of the surface voxels
    of both masks, pooled, that lie within `tolerance` voxels (unit spacing) of the other mask's surface; surfaces and distances as
    Hausdorff95's.  This is the voxel-surface form (MONAI's SurfaceDiceMetric counts the same way); it is NOT DeepMind's
    surface-element-area form, and it was NOT compared with MONAI's code or any official evaluator.  Both masks empty: 1; one empty: 0.
    update() never synchronises."""
    column = 0

    def __init__(self, name="SurfaceDice", input_index=0, target_index=0, classes=4, tolerance=1.0):
        super(SurfaceDice, self).__init__(name, input_index, target_index, classes)
        ops.tolerance_bins([tolerance])                                               # a bad tolerance fails here, not in the first update
        self.tolerance = tolerance

    def _score(self, pred, gr):
        return ops.surface_distances(pred, gr, (self.tolerance,))[2]


class AverageSurfaceDistance(_ExtrasMetric):
    """The average symmetric surface distance (ASSD) per channel, in voxels at unit spacing: the mean over the surface voxels of both
    masks, pooled, of the distance to the other mask's surface.  Both masks empty: 0; one empty: `empty_value`, Hausdorff95's convention,
    NOT checked against any official evaluator.  update() never synchronises."""
    column = 0

    def __init__(self, name="AverageSurfaceDistance", input_index=0, target_index=0, classes=4, empty_value=ops.HD95_EMPTY):
        super(AverageSurfaceDistance, self).__init__(name, input_index, target_index, classes)
        self.empty_value = empty_value

    def _score(self, pred, gr):
        return ops.surface_distances(pred, gr, (), self.empty_value)[2]


class LesionWiseSurfaceDice(_ExtrasMetric):
    """The lesion-wise NSD of LesionWiseDice's matching: SurfaceDice's value per kept lesion against what it matched, 0 for a missed lesion
    and for every false-positive component, divided by their number (1 when there is none).  NOT checked against the official evaluator.
    update() synchronises once, as the other lesion-wise metrics do."""
    column = 0

    def __init__(self, name="LesionWiseSurfaceDice", input_index=0, target_index=0, classes=4, tolerance=1.0, dilation=3, min_volume=50):
        super(LesionWiseSurfaceDice, self).__init__(name, input_index, target_index, classes)
        ops.tolerance_bins([tolerance])
        self.tolerance = tolerance
        self.dilation = dilation
        self.min_volume = min_volume

    def _score(self, pred, gr):
        return ops.lesion_distances(pred, gr, (self.tolerance,), self.dilation, self.min_volume)[2]


# ---------------------------------------------------------------------- the definitions restated in float64 numpy / scipy (host)
_RESTATE_THREADS = 1024                                                               # the finalize kernel's workgroup


def _surface_host(a):
    """the voxels of `a` with a face neighbour outside `a` or outside the grid"""
    p = np.pad(a, 1)
    inner = p[1:-1, 1:-1, 1:-1].copy()
    for ax in range(3):
        for sh in (1, -1):
            inner &= np.roll(p, sh, axis=ax)[1:-1, 1:-1, 1:-1]
    return a & ~inner


def surface_histogram_host(p, g):
    """bool masks [D, H, W], both non-empty -> int64 histogram of the |dP| + |dG| exact squared surface distances, (D-1)^2 + (H-1)^2 +
    (W-1)^2 + 1 bins"""
    from scipy import ndimage
    sp, sg = _surface_host(p), _surface_host(g)
    to_g = np.rint(ndimage.distance_transform_edt(~sg) ** 2).astype(np.int64)
    to_p = np.rint(ndimage.distance_transform_edt(~sp) ** 2).astype(np.int64)
    bins = sum((s - 1) ** 2 for s in p.shape) + 1
    return np.bincount(np.concatenate([to_g[sp], to_p[sg]]), minlength=bins)


def assd_terms_host(hist):
    """the float64 terms h_b * sqrt(b) of the ASSD sum (one rounding in the square root, one in the product)"""
    return hist.astype(np.float64) * np.sqrt(np.arange(len(hist), dtype=np.float64))


def surface_distances_host(p, g, tolerances=(1.0,), empty_value=ops.HD95_EMPTY):
    """ops.surface_distances' extras of one pair of bool masks [D, H, W], restated: -> float64 [T + 2] = (NSD per tolerance, ASSD, HD).
    NSD: an integer count over one float64 division.  ASSD: the kernel's order -- position i of 1024 adds its ceil(bins / 1024)
    consecutive terms in ascending bin order, then the tree i += i + 512, + 256, ... + 1 -- and one division.  HD: sqrt of the last
    non-empty bin."""
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    tb = ops.tolerance_bins(tolerances)
    t = len(tb)
    out = np.zeros(t + 2, dtype=np.float64)
    if not p.any() or not g.any():
        both = not p.any() and not g.any()
        out[:t] = 1.0 if both else 0.0
        out[t:] = 0.0 if both else empty_value
        return out
    hist = surface_histogram_host(p, g)
    n = np.float64(hist.sum())
    cum = np.cumsum(hist)
    for i, b in enumerate(tb):
        out[i] = np.float64(cum[min(b, len(hist) - 1)]) / n
    chunk = -(-len(hist) // _RESTATE_THREADS)
    terms = np.zeros(chunk * _RESTATE_THREADS, dtype=np.float64)
    terms[:len(hist)] = assd_terms_host(hist)
    terms = terms.reshape(_RESTATE_THREADS, chunk)
    part = np.zeros(_RESTATE_THREADS, dtype=np.float64)
    for j in range(chunk):
        part = part + terms[:, j]
    s = _RESTATE_THREADS // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    out[t] = part[0] / n
    out[t + 1] = np.sqrt(np.float64(np.flatnonzero(hist)[-1]))
    return out


def lesion_pairs_host(p, g, dilation=3):
    """the matching of the lesion-wise scorers with scipy's dilation and labelling (INTEGRATION.md states it): -> (pairs [(M_i, L_i)] in
    lesion order, n_fp)"""
    from scipy import ndimage
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    s18, s26 = ndimage.generate_binary_structure(3, 2), np.ones((3, 3, 3), bool)
    z, n = ndimage.label(ndimage.binary_dilation(g, s18, iterations=dilation) if dilation else g, s26)
    q, m = ndimage.label(p, s26)
    matched = np.zeros(m + 1, bool)
    pairs = []
    for i in range(1, n + 1):
        zi = z == i
        js = np.unique(q[zi])
        js = js[js > 0]
        matched[js] = True
        pairs.append((np.isin(q, js) & p, g & zi))
    return pairs, m - int(matched[1:].sum())


def lesion_distances_host(p, g, tolerances=(1.0,), dilation=3, min_volume=50, empty_value=ops.HD95_EMPTY):
    """ops.lesion_distances' extras of one pair of bool masks [D, H, W], restated: -> (summary_ex float64 [T + 1] = (LesionNSD per
    tolerance, LesionASSD), rows float64 [n_gt, T + 2] = surface_distances_host of every pair (M_i, L_i), n_fp).  The sums run over the
    kept lesions in ascending order."""
    t = len(ops.tolerance_bins(tolerances))
    pairs, n_fp = lesion_pairs_host(p, g, dilation)
    rows, kept = np.zeros((len(pairs), t + 2), dtype=np.float64), 0
    sums = np.zeros(t + 1, dtype=np.float64)
    for i, (mi, li) in enumerate(pairs):
        rows[i] = surface_distances_host(mi, li, tolerances, empty_value)
        if int(li.sum()) > min_volume:
            kept += 1
            sums = sums + rows[i, :t + 1]
    den = kept + n_fp
    out = np.zeros(t + 1, dtype=np.float64)
    out[:t] = sums[:t] / np.float64(den) if den else 1.0
    out[t] = (sums[t] + np.float64(n_fp) * np.float64(empty_value)) / np.float64(den) if den else 0.0
    return out, rows, n_fp


# ---------------------------------------------------------------------- calibration and the threshold search ("Calibration")
BRATS_REGION_LABELS = ((1, 2, 3, 4), (1, 3, 4), (3, 4))                               # WT, TC, ET


def _bin_sums(key, weight, size):
    """exact int64 sums of the non-negative int64 `weight` (< 2^25) per key: two bincounts over 13-bit halves, each below 2^53 in float64"""
    hi = np.bincount(key, weights=(weight >> 13).astype(np.float64), minlength=size).astype(np.int64)
    lo = np.bincount(key, weights=(weight & 8191).astype(np.float64), minlength=size).astype(np.int64)
    return (hi << 13) + lo


def calibration_tables_host(pred, target, nb=256):
    """The integer tables of ops.calib_histogram restated from the definitions: pred float32 [N,C,...]; target float32 of the same shape
    or a uint8 label volume [N,...] (C = 3) -> (hist, conf, sq, invalid) as int64 arrays [N,C,nb+1,2], [N,C,nb+1,2], [N,C,2,2], [N,C]."""
    p = np.asarray(pred, dtype=np.float32)
    n, c = p.shape[:2]
    p = p.reshape(n, c, -1)
    t = np.asarray(target)
    labels = t.dtype == np.uint8
    t = t.reshape(n, -1) if labels else t.astype(np.float32).reshape(n, c, -1)
    k1 = nb + 1
    hist, conf = np.zeros((n, c, k1, 2), np.int64), np.zeros((n, c, k1, 2), np.int64)
    sq, invalid = np.zeros((n, c, 2, 2), np.int64), np.zeros((n, c), np.int64)
    for i in range(n):
        for j in range(c):
            x = p[i, j].astype(np.float64)
            with np.errstate(invalid="ignore"):
                ok = (x >= 0.0) & (x <= 1.0)
                if labels:
                    ok &= t[i] <= 4
                    y = np.isin(t[i], BRATS_REGION_LABELS[j])
                else:
                    ok &= ~np.isnan(t[i, j])
                    y = t[i, j] > np.float32(0.5)
            x, y = x[ok], y[ok].astype(np.int64)
            k = np.ceil(x * nb).astype(np.int64)
            r = np.floor(x * 16777216.0).astype(np.int64)
            key = 2 * k + y
            invalid[i, j] = ok.size - int(ok.sum())
            hist[i, j] = np.bincount(key, minlength=2 * k1).reshape(k1, 2)
            conf[i, j] = _bin_sums(key, r, 2 * k1).reshape(k1, 2)
            r2 = r.astype(np.uint64) * r.astype(np.uint64)
            for cls in (0, 1):
                sel = r2[y == cls]
                sq[i, j, cls, 0] = int((sel & np.uint64(0xffffffff)).sum(dtype=np.uint64))
                sq[i, j, cls, 1] = int((sel >> np.uint64(32)).sum(dtype=np.uint64))
    return hist, conf, sq, invalid


def calibration_curves_host(hist):
    """hist int64 [..., nb+1, 2] -> float64 [..., 3, nb+1]: Dice_b, Sens_b, Spec_b of the mask k > b, from exact integers, one division each,
    1 for a zero denominator"""
    h = np.asarray(hist, dtype=np.int64)
    tot = h.sum(axis=-2, keepdims=True)
    above = tot - np.cumsum(h, axis=-2)                                               # sums over k > b
    fp, tp = above[..., 0], above[..., 1]
    fn, tn = tot[..., 1] - tp, tot[..., 0] - fp

    def ratio(num, den):
        return np.where(den > 0, num.astype(np.float64) / np.maximum(den, 1).astype(np.float64), 1.0)
    return np.stack([ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, tp + fn), ratio(tn, tn + fp)], axis=-2)


def calibration_summary_host(pool_hist, pool_conf, pool_s2, m=16):
    """Pooled tables of ONE channel (hist, conf int64 [nb+1,2]; pool_s2 = the exact Python ints (S2(y=0), S2(y=1))) -> (summary float64 [7] =
    ECE, MCE, Brier, mean confidence, prevalence, n, non-empty coarse bins; table float64 [m,3] = n_m, conf_m, freq_m).  Every ratio is one
    correctly rounded division of exact Python integers; ECE adds its rounded products in order of the coarse bin."""
    h, s = np.asarray(pool_hist, dtype=np.int64), np.asarray(pool_conf, dtype=np.int64)
    nb = h.shape[0] - 1
    assert nb % m == 0
    width = nb // m
    coarse = (np.maximum(np.arange(nb + 1), 1) - 1) // width
    table, out = np.zeros((m, 3), np.float64), np.zeros(7, np.float64)
    n, n1 = int(h.sum()), int(h[:, 1].sum())
    if n == 0:
        return out, table
    ece, mce, used = 0.0, 0.0, 0
    for b in range(m):
        sel = coarse == b
        nm, nm1, rm = int(h[sel].sum()), int(h[sel, 1].sum()), int(s[sel].sum())
        if nm == 0:
            continue
        cf, fr = rm / (nm * (1 << 24)), nm1 / nm
        gap = abs(fr - cf)
        ece = ece + (nm / n) * gap
        mce = max(mce, gap)
        used += 1
        table[b] = (nm, cf, fr)
    r, r1 = int(s.sum()), int(s[:, 1].sum())
    num = int(pool_s2[0]) + n1 * (1 << 48) - (1 << 25) * r1 + int(pool_s2[1])
    out[:] = (ece, mce, num / (n * (1 << 48)), r / (n * (1 << 24)), n1 / n, n, used)
    return out, table


def choose_threshold(dice_curve):
    """The bin b in 1..nb-1 with the largest value of the (mean) Dice curve [nb+1]; ties go to the b closest to nb / 2, then to the lower b.
    The threshold is b / nb."""
    d = np.asarray(dice_curve, dtype=np.float64)
    nb = d.shape[0] - 1
    best = max(d[1:nb])
    return min((b for b in range(1, nb) if d[b] == best), key=lambda b: (abs(b - nb // 2), b))


def calibration_host(pred, target, nb=256, m=16):
    """The numpy restatement of the calibration scorer, written from the definitions and independent of the kernels: a dict with the
    per-sample tables `hist`, `conf`, `sq`, `invalid` (int64), `s2` (Python ints [N][C][2]), `curves` float64 [N,C,3,nb+1]; the pooled
    `pool_hist`, `pool_conf` (int64 [C,nb+1,2]), `pool_s2` (Python ints [C][2]), `pool_sq` (int64 [C,2,2], carried: low word < 2^32),
    `curve_sum` float64 [C,3,nb+1] (the samples added in order); and `summary` float64 [C,7], `table` float64 [C,m,3]."""
    hist, conf, sq, invalid = calibration_tables_host(pred, target, nb)
    n, c = hist.shape[:2]
    s2 = [[[int(sq[i, j, y, 1]) * (1 << 32) + int(sq[i, j, y, 0]) for y in (0, 1)] for j in range(c)] for i in range(n)]
    pool_s2 = [[sum(s2[i][j][y] for i in range(n)) for y in (0, 1)] for j in range(c)]
    pool_sq = np.array([[[v & 0xffffffff, v >> 32] for v in pool_s2[j]] for j in range(c)], dtype=np.int64)
    curves = calibration_curves_host(hist)
    curve_sum = curves[0].copy()
    for i in range(1, n):
        curve_sum = curve_sum + curves[i]
    pool_hist, pool_conf = hist.sum(axis=0), conf.sum(axis=0)
    rows = [calibration_summary_host(pool_hist[j], pool_conf[j], pool_s2[j], m) for j in range(c)]
    return {"hist": hist, "conf": conf, "sq": sq, "invalid": invalid, "s2": s2, "curves": curves, "curve_sum": curve_sum, "pool_hist": pool_hist,
            "pool_conf": pool_conf, "pool_s2": pool_s2, "pool_sq": pool_sq, "summary": np.stack([r[0] for r in rows]),
            "table": np.stack([r[1] for r in rows])}


class _CalibrationMetric(Metrics):
    """Pools ops.calib_histogram's integer tables over the update() calls on the device (no host sync); get() runs ops.calib_summary on
    them and returns column `_column` per channel as a float64 array [C].  `data_parallel` (Trainer.train sets it on train metrics when
    world > 1): get() all-reduces (SUM) a copy of the pooled integer tables before the summary, as RMSE does with its sums."""
    _column = 0

    def __init__(self, name, input_index, target_index, bins, nb):
        super(_CalibrationMetric, self).__init__(name)
        self.input_index = input_index
        self.target_index = target_index
        self.bins, self.nb = int(bins), int(nb)
        self.data_parallel = False
        self.pool = None

    def reset(self):
        super(_CalibrationMetric, self).reset()
        self.pool = None

    def update(self, ground, predict):
        pred = predict[self.input_index].detach()
        gr = ground[self.target_index].detach()
        assert gr.shape == pred.shape
        pred, gr = pred.cuda().float(), gr.cuda().float()
        hist, conf, sq, _ = ops.calib_histogram(pred, gr, self.nb)
        if self.pool is None:
            self.pool = ops.calib_pool(int(pred.shape[1]), self.nb, pred.device)
        ops.calib_accumulate(hist, conf, sq, self.pool)
        self.samples += 1

    def summary(self):
        """(out float64 [C,7], table float64 [C,bins,3]) device tensors of the pooled tables so far"""
        if self.pool is None:
            raise RuntimeError("%s: no update() yet" % self.name)
        tables = self.pool[:3]
        if self.data_parallel:
            from .loss import _all_reduce_sums
            tables = [t.clone() for t in tables]
            # pool_sq's carried {low, high} words add up to the same S2; the summary reads them as such
            for t in tables:
                _all_reduce_sums(t, self.data_parallel)
        return ops.calib_summary(tables[0], tables[1], tables[2], self.bins)

    def get(self):
        return self.summary()[0][:, self._column].cpu().numpy()


class ExpectedCalibrationError(_CalibrationMetric):
    """ECE per channel over everything seen since reset(): `bins` equal-width confidence bins over `nb` fine bins (include/resunet_hip.h,
    ru_calib_summary).  `max_error()` is the MCE, `reliability()` the table [C,bins,3] = (n_m, conf_m, freq_m)."""

    def __init__(self, name="ECE", input_index=0, target_index=0, bins=16, nb=256):
        super(ExpectedCalibrationError, self).__init__(name, input_index, target_index, bins, nb)

    def max_error(self):
        return self.summary()[0][:, 1].cpu().numpy()

    def reliability(self):
        return self.summary()[1].cpu().numpy()


class BrierScore(_CalibrationMetric):
    """Brier score per channel over everything seen since reset(), on the probabilities truncated to 24 fractional bits."""
    _column = 2

    def __init__(self, name="Brier", input_index=0, target_index=0, nb=256):
        super(BrierScore, self).__init__(name, input_index, target_index, 16, nb)


class DiceAtThreshold(Metrics):
    """metrics.Dice with the masks `p > threshold` (a scalar or one value per channel) in place of `p > 0.5`: ops.threshold_regions per
    sample, then Dice's own counts and accumulate launches.  get(): float64 array [C]."""

    def __init__(self, threshold, name="DiceAtThreshold", input_index=0, target_index=0):
        super(DiceAtThreshold, self).__init__(name)
        self.threshold = threshold
        self.input_index = input_index
        self.target_index = target_index

    def update(self, ground, predict):
        pred = predict[self.input_index].detach().cuda().float().contiguous()
        gr = ground[self.target_index].detach().cuda()
        assert gr.shape == pred.shape
        masks = torch.stack([ops.threshold_regions(pred[i], self.threshold)[0] for i in range(int(pred.shape[0]))]).float()
        counts = ops.dice_counts(masks, gr)
        c = int(counts.shape[1])
        ops.dice_accumulate(counts, _acc(self, c, counts.device), c)
        self.samples += 1

    def get(self):
        return _get_array(self)


def print_metrics(writer, metric, prefix, epoch):
    """metrics.py:273-280: an array value is logged as one scalar per entry, tagged prefix + name + index; any other value as one scalar
    tagged prefix + name.  Then the line `Epoch <epoch>, <prefix> <name> <value>`."""
    value = metric.get()
    if isinstance(value, np.ndarray):
        for i, v in enumerate(value):
            writer.add_scalar("%s%s%d" % (prefix, metric.name, i), v, epoch)
    else:
        writer.add_scalar(prefix + metric.name, value, epoch)
    print("Epoch %d, %s %s %s" % (epoch, prefix, metric.name, value))
