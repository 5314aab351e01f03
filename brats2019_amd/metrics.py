"""Drop-in for the part of the reference's `metrics` module that the hot path's Trainer uses: the `Metrics` accumulator
protocol (metrics.py:6-20: name / update / get / reset), `Dice` (metrics.py:101-133) -- threshold 0.5, per sample and
channel 2*sum(p*g)/sum(p+g) (NaN -> 1), mean over the batch, accumulated over update() calls -- and the Hausdorff distances
`Hausdorff_ITK` / `Hausdorff_ITKWT` (metrics.py:188-271) that main.py:149-151 validates with, in SimpleITK's definition (unit
spacing, voxel centres) without SimpleITK: an exact squared distance transform on the device (ru_hausdorff_sq), then the
reference's bookkeeping -- 1e6 for an empty mask, its i-1 index slip, the float64 batch mean -- in one more launch.  The counting runs on
the device (ru_dice_counts, ru_hausdorff_sq) and the running sums stay there: `update` never synchronises, `get()` copies a few numbers
to the host.  `update(ground, predict)` keeps the reference's argument order (train.py:304)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


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
