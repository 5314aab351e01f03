"""Inference driver around the forward pass: the per-case pipeline of the reference's test.py (:82-164), on the device from the upload
of the case to the download of its label volume (kernels in csrc/inference.hip, the merge and the paste in the one family of csrc/ensemble.hip) --

  ru_case_bbox      bounding box of the non-zero voxels (test.py:47-49,85-87); its 6 integers are the only values that visit the host
                    in between: they fix the tensor shapes of everything downstream;
  ru_case_stats     non-zero z-score moments of the crop (test.py:103-111), float64;
  ru_case_prepare   crop + zero-pad to x16 (test.py:92-99) + z-score (:113) + the FOUR test-time flips (:115-120) written as ONE batch;
  model             one batch-4 forward instead of four forward calls with host round trips (:124-132);
  ru_tta_merge_box  un-flip + average + un-pad + threshold + per-class counts (:134-144); ru_compose_labels (:146-159);
  ru_postprocess_regions  opt-in (`postprocess=PostProcess(...)`): per region, components below a volume or a mean probability go, only the
                    largest stays, holes are filled, the regions are nested -- between the merge and the label composition (csrc/postprocess.hip);
  ru_cc_reject      26-connected components (skimage.morphology.label) + rejection of regions below ratio 0.1 (:51-62,162-164);
  ru_paste_labels   paste into the full volume (:167-168).

Ensembles (README.md:1-5 of the reference: an ensemble annotates the cases the small network is distilled from; average_predicts.ipynb /
emsemble_predicts.ipynb average saved predictions on the host): `predict_case_ensemble*` prepares the case ONCE, runs each model on the
shared batch and folds its prediction into a running float32 sum at once (csrc/ensemble.hip), so at most one model's output is alive;
the mean probabilities -- the soft labels a student is trained on -- come back pasted into the case's frame when asked for.
`ensemble_merge_host` / `ensemble_class_labels_host` restate the arithmetic in numpy.

The numpy functions below (`get_bbox`, `prepare_case`, `reject_small_regions`, `postprocess_labels`) are the host restatement the
device pipeline is tested against; `predict_case` does not call them.  NIfTI reading/writing (nibabel) is out of scope; `predict_case`
takes and returns arrays.
"""
from __future__ import annotations

import collections
import os

import numpy as np
import torch

from . import ops, tiling

TTA_FLIPS = ((), (1,), (2,), (1, 2))          # test.py:117-120, axes of the [C,D,H,W] volume


def closest_to_k(n, k=16):
    """loader_helper.py:99-103."""
    return n if n % k == 0 else (n // k + 1) * k


def get_bbox(image):
    """test.py:47-49 / loader_helper.py:105-129: union bounding box of the non-zero voxels of every modality."""
    lo, hi = [], []
    for d in image:
        nz = np.nonzero(d)
        if nz[0].size == 0:
            lo.append([-1, -1, -1]); hi.append([0, 0, 0])
        else:
            lo.append([a.min() for a in nz]); hi.append([a.max() for a in nz])
    return np.stack([np.min(lo, axis=0), np.max(hi, axis=0)], axis=0)


def prepare_case(image):
    """test.py:85-113 -> (normalised padded crop [C,D,H,W] float32, bbox, pad_left, pad_right)."""
    bbox = get_bbox(image)
    crop = image[:, bbox[0, 0]:bbox[1, 0], bbox[0, 1]:bbox[1, 1], bbox[0, 2]:bbox[1, 2]]
    old = np.array(crop.shape[1:])
    new = np.array([closest_to_k(int(i), 16) for i in old])
    diff = new - old
    left = diff // 2
    right = diff - left
    x = np.pad(crop, ((0, 0),) + tuple((int(left[i]), int(right[i])) for i in range(3)), mode="constant", constant_values=0)
    n = (x > 0).sum(axis=(1, 2, 3))
    mean = np.sum(x / n[:, None, None, None], axis=(1, 2, 3))
    mean2 = np.sum(np.square(x) / n[:, None, None, None], axis=(1, 2, 3))
    std = np.sqrt(mean2 - mean * mean)
    x = (x - mean.reshape(-1, 1, 1, 1)) / std.reshape(-1, 1, 1, 1)
    return x.astype(np.float32), bbox, left, right


def reject_small_regions(connectivity, ratio=0.25):
    """test.py:51-62."""
    out = connectivity.copy()
    unique, counts = np.unique(connectivity, return_counts=True)
    nonzero = connectivity.size - counts.max()
    for u, c in zip(unique, counts):
        if c < ratio * nonzero:
            out[out == u] = 0
    return out


def predict_tta(model, x, pad_left=(0, 0, 0), pad_right=(0, 0, 0), want_mean=False):
    """x: [C,D,H,W] float32 (numpy or tensor), extents divisible by 8.  One batch-4 forward over the four flips, then the
    device-side merge; the padding is removed BEFORE the labels are composed (test.py:140-159: the ET > 32 rule counts
    un-padded voxels).  Returns (labels uint8 [d,h,w] device tensor, counts [3] device tensor, mean probs or None)."""
    xt = torch.as_tensor(x, dtype=torch.float32).cuda()
    batch = torch.stack([torch.flip(xt, dims=list(ax)) if ax else xt for ax in TTA_FLIPS], dim=0).contiguous()
    model.eval()
    if hasattr(model, "freeze_params"):
        model.freeze_params(True)                       # constant weights: packed once, reused by every later forward (dropped by .train() / load_state_dict)
    with torch.no_grad():
        probs = model([batch])[0]                       # [4,3,D,H,W]
    mask, counts, mean = ops.tta_merge(probs, TTA_FLIPS, want_mean=want_mean)
    d, h, w = [int(v) for v in mask.shape[1:]]
    if any(int(v) for v in pad_left) or any(int(v) for v in pad_right):
        mask = mask[:, int(pad_left[0]):d - int(pad_right[0]), int(pad_left[1]):h - int(pad_right[1]),
                    int(pad_left[2]):w - int(pad_right[2])].contiguous()
        counts = mask.sum(dim=(1, 2, 3), dtype=torch.int64)
        if mean is not None:
            mean = mean[:, int(pad_left[0]):d - int(pad_right[0]), int(pad_left[1]):h - int(pad_right[1]), int(pad_left[2]):w - int(pad_right[2])]
    labels = ops.compose_labels(mask, counts, et_min=32)
    return labels, counts, mean


def postprocess_labels(labels, ratio=0.1):
    """test.py:162-164 on the host (26-connected components, ratio 0.1)."""
    import scipy.ndimage as ndi
    comp, _ = ndi.label(labels > 0, structure=np.ones((3, 3, 3), dtype=bool))
    clusters = reject_small_regions(comp, ratio)
    labels = labels.copy()
    labels[clusters == 0] = 0
    return labels


# ---------------------------------------------------------------------- region-wise post-processing (csrc/postprocess.hip)
class PostProcess(collections.namedtuple("PostProcess", "min_volume min_confidence keep_largest fill_holes nest reject_ratio")):
    """The post-processing of one case, the `postprocess=` keyword of `predict_case*`: the parameters of `ops.postprocess_regions` (a scalar
    or a triple WT, TC, ET each; INTEGRATION.md states the definition) and `reject_ratio`, the reference's own step on the union of all
    labels (test.py:162-164, `ops.cc_reject`), which stays by default; None switches it off.  `PostProcess()` changes nothing."""
    __slots__ = ()

    def __new__(cls, min_volume=0, min_confidence=0.0, keep_largest=False, fill_holes=False, nest=False, reject_ratio=0.1):
        mv, _, kl, fh = ops.postprocess_params(min_volume, min_confidence, keep_largest, fill_holes)           # (raises on a bad value)
        if reject_ratio is not None and not float(reject_ratio) >= 0.0:
            raise ValueError("PostProcess: reject_ratio %r: a ratio >= 0 or None" % (reject_ratio,))
        mc = tuple(float(c) for c in min_confidence) if hasattr(min_confidence, "__len__") else (float(min_confidence),) * 3
        return super().__new__(cls, tuple(mv), mc, tuple(bool((kl >> k) & 1) for k in range(3)), tuple(bool((fh >> k) & 1) for k in range(3)), bool(nest),
                               None if reject_ratio is None else float(reject_ratio))        # every per-region field is stored as a triple WT, TC, ET

    @property
    def needs_probs(self):
        """the confidence rule of some region is on: the merge passes must return the mean probabilities"""
        return any(ops.postprocess_params(self.min_volume, self.min_confidence)[1])

    def regions(self):
        """the keywords of `ops.postprocess_regions` / `postprocess_regions_host`"""
        return dict(min_volume=self.min_volume, min_confidence=self.min_confidence, keep_largest=self.keep_largest, fill_holes=self.fill_holes,
                    nest=self.nest)


def _check_postprocess(postprocess):
    if postprocess is not None and not isinstance(postprocess, PostProcess):
        raise ValueError("postprocess=%r: None or an inference.PostProcess" % (postprocess,))
    return postprocess


def postprocess_regions_host(x, probs=None, min_volume=0, min_confidence=0.0, keep_largest=False, fill_holes=False, nest=False, want_stats=False):
    """`ops.postprocess_regions` restated with numpy and scipy (INTEGRATION.md states the definition): the oracle of the device tests and the
    `--host` path of `python -m brats2019_amd.postprocess`.  x: masks [3, D, H, W] (non-zero = foreground) -> (uint8 masks, int64 counts
    [3]), or a uint8 label volume [D, H, W] -> (uint8 labels, counts); want_stats appends the int64 statistics [3, 5] / [3, 6]."""
    import scipy.ndimage as ndi
    mv, thr, kl, fh = ops.postprocess_params(min_volume, min_confidence, keep_largest, fill_holes)
    x = np.asarray(x)
    labels_in = x.ndim == 3
    if not (labels_in or (x.ndim == 4 and x.shape[0] == 3)):
        raise ValueError("postprocess_regions_host: masks [3, D, H, W] or a label volume [D, H, W], got %s" % (x.shape,))
    if any(thr) and probs is None:
        raise ValueError("postprocess_regions_host: min_confidence > 0 needs the probabilities")
    if probs is not None and (labels_in or tuple(np.shape(probs)) != x.shape):
        raise ValueError("postprocess_regions_host: probabilities go with masks and have their shape")
    if labels_in:
        regions = [(x >= 1) & (x <= 4), (x == 1) | (x == 3) | (x == 4), (x == 3) | (x == 4)]
    else:
        regions = [x[k] != 0 for k in range(3)]
    q = None
    if any(thr):                                                     # q(p): an exact float32 product by 2^16, truncated
        q = np.floor(np.clip(np.asarray(probs, np.float32), np.float32(0), np.float32(1)) * np.float32(65536.0)).astype(np.int64)
    stats = np.zeros((3, 6 if labels_in else 5), np.int64)
    out = []
    for k, r in enumerate(regions):
        comp, n = ndi.label(r, structure=np.ones((3, 3, 3), dtype=bool))          # numbered by ascending smallest linear index
        vol = np.bincount(comp.ravel(), minlength=n + 1).astype(np.int64)
        keep = np.ones(n + 1, bool)
        keep[0] = False
        small = keep & (vol < mv[k])
        keep &= ~small
        stats[k, 0], stats[k, 1] = n, small.sum()
        if thr[k] > 0:
            conf = np.bincount(comp.ravel(), weights=q[k].ravel(), minlength=n + 1).astype(np.int64)    # (sums below 2^53: exact in float64)
            low = keep & (conf < thr[k] * vol)
            keep &= ~low
            stats[k, 2] = low.sum()
        if (kl >> k) & 1 and keep.any():
            alive = np.flatnonzero(keep)
            best = alive[np.argmax(vol[alive])]                      # the first maximum: the smallest label, the smallest linear index
            stats[k, 3] = alive.size - 1
            keep[:] = False
            keep[best] = True
        r = keep[comp]
        if (fh >> k) & 1:
            filled = ndi.binary_fill_holes(r)
            stats[k, 4] = int(filled.sum()) - int(r.sum())
            r = filled
        out.append(r)
    if nest:
        out[1] = out[1] & out[0]
        out[2] = out[2] & out[1]
    counts = np.array([int(r.sum()) for r in out], np.int64)
    if labels_in:
        stats[:, 5] = int((x > 4).sum())
        res = np.zeros(x.shape, np.uint8)
        res[out[0]] = 2
        res[out[1]] = 1
        res[out[2]] = 4
    else:
        res = np.stack(out).astype(np.uint8)
    return (res, counts, stats) if want_stats else (res, counts)


def compose_masks_host(mask, counts, et_min=32):
    """test.py:153-159 from the three masks and their counts (`ops.compose_labels`): ET only with more than `et_min` ET voxels."""
    m = np.asarray(mask) != 0
    out = np.zeros(m.shape[1:], np.uint8)
    out[m[0]] = 2
    out[m[1]] = 1
    if int(counts[2]) > et_min:
        out[m[2]] = 4
    return out


def _check_thresholds(thresholds):
    """thresholds=None | a scalar | (wt, tc, et): the region masks are `mean > t` instead of the merge's `mean > 0.5`"""
    return None if thresholds is None else tuple(ops.region_thresholds(thresholds, 3))


def _labels_from_masks(mask, counts, mean, postprocess, thresholds=None):
    """masks of the merge -> (label volume in the crop frame, counts): with `thresholds` the masks and counts rewritten from the mean
    (`ops.threshold_regions`), the region pass of `postprocess` (if any), test.py:153-159, and the reference's rejection on the union of
    all labels unless `postprocess` switches it off"""
    ratio = 0.1
    if thresholds is not None:
        mask, counts = ops.threshold_regions(mean, thresholds)
    if postprocess is not None:
        mask, counts = ops.postprocess_regions(mask, probs=mean if postprocess.needs_probs else None, **postprocess.regions())
        ratio = postprocess.reject_ratio
    labels = ops.compose_labels(mask, counts, et_min=32)
    if ratio is not None:
        ops.cc_reject(labels, ratio)
    return labels, counts


def prepare_case_device(image):
    """test.py:85-120 on the device.  image: [C,D,H,W] float32 device tensor.  Returns (batch [4,C,Dp,Hp,Wp] = the four test-time flips
    of the padded, normalised crop; lo, size = the crop box; pad_left; padded extents)."""
    boxes = ops.case_bbox(image)                                     # [C,6] on the host: the only device -> host copy before the labels
    lo = boxes[:, :3].min(axis=0)
    hi = boxes[:, 3:].max(axis=0)                                    # test.py:87 uses the max INDEX as an exclusive slice end
    size = hi - lo
    if (lo < 0).any() or (size <= 0).any():
        raise ValueError("predict_case: a modality without non-zero voxels (or a one-voxel-thick box) gives an empty crop (test.py:85-87)")
    padded = np.array([closest_to_k(int(v), 16) for v in size])
    left = (padded - size) // 2
    stats = ops.case_stats(image, lo, size)
    batch = ops.case_prepare(image, stats, lo, size, left, padded, TTA_FLIPS)
    return batch, lo, size, left, padded


def _forward(model, batch, tile, overlap, window):
    """The forward of the batch of flips: whole, or with `tile` set through overlapping tiles blended with `window` (tiling.predict_blended)."""
    from .model import warn_mx_range
    warn_mx_range(model)                                         # once per model: parameters outside the fp16 + MX-fp8 operand range (model.MX_RANGE)
    if tile is None:
        return model([batch])[0]
    return tiling.predict_blended(model, batch, tile, overlap=overlap, window=window)


def _check_tiled(model, tile, overlap, window):
    if tile is not None:
        tiling._check_blend(overlap, window)
        tiling._check_tile(model, tile)


def predict_case_device(model, image, uncertainty=None, tile=None, overlap=0.5, window="gaussian", postprocess=None, thresholds=None):
    """The per-case pipeline of test.py:82-168 with every array on the device: image [4,D,H,W] device tensor -> (uint8 device label volume
    [D,H,W] with values {0,1,2,4}, int64 device tensor of the (wt, tc, et) voxel counts).  uncertainty="std" | "entropy": the model is
    served as an ensemble of one and the uint8 [3,D,H,W] uncertainty maps of its four flips are appended.  tile=(td, th, tw): the padded
    crop does not go through the network whole but in tiles overlapping by `overlap`, blended with `window` ("gaussian" | "constant");
    everything behind the forward is the same.  postprocess=PostProcess(...): the region pass (`ops.postprocess_regions`) runs on the merged
    masks in the crop frame before the labels are composed, so the ET > 32 rule and the returned counts are those of the post-processed
    masks; the uncertainty maps are not touched.  thresholds=(wt, tc, et) or a scalar (e.g. from `validate --calibration`): the merge is
    asked for its mean and the region masks and counts are `mean > t` (`ops.threshold_regions`) before `postprocess`, the ET > 32 rule and
    the label composition; None: the merge's own `mean > 0.5`, no further launch; 0.5 gives the same labels byte for byte."""
    _check_postprocess(postprocess)
    thresholds = _check_thresholds(thresholds)
    if uncertainty is not None:
        return predict_case_ensemble_device([model], image, uncertainty=uncertainty, tile=tile, overlap=overlap, window=window, postprocess=postprocess,
                                            thresholds=thresholds)
    _check_tiled(model, tile, overlap, window)
    image = image.contiguous().float()
    batch, lo, size, left, _padded = prepare_case_device(image)
    model.eval()
    if hasattr(model, "freeze_params"):
        model.freeze_params(True)
    with torch.no_grad():
        probs = _forward(model, batch, tile, overlap, window)        # [4,3,Dp,Hp,Wp]
    mask, counts, mean = ops.tta_merge_box(probs, TTA_FLIPS, left, size, want_mean=thresholds is not None or (postprocess is not None and postprocess.needs_probs))
    labels, counts = _labels_from_masks(mask, counts, mean, postprocess, thresholds)
    return ops.paste_labels(labels, image.shape[1:], lo), counts


def predict_case(model, image, uncertainty=None, tile=None, overlap=0.5, window="gaussian", postprocess=None, thresholds=None):
    """Full per-case pipeline of test.py:82-168 for one multimodal volume `image` [4,D,H,W] (numpy or tensor): one upload, the device
    pipeline above, one download.  Returns (uint8 label volume [D,H,W] with values {0,1,2,4}, (wt, tc, et) voxel counts) and, with
    uncertainty="std" | "entropy", the uint8 [3,D,H,W] uncertainty maps.  `tile`, `overlap`, `window`, `postprocess`, `thresholds`: as
    `predict_case_device`."""
    _check_postprocess(postprocess)
    thresholds = _check_thresholds(thresholds)
    if uncertainty is not None:
        return predict_case_ensemble([model], image, uncertainty=uncertainty, tile=tile, overlap=overlap, window=window, postprocess=postprocess,
                                     thresholds=thresholds)
    _check_tiled(model, tile, overlap, window)
    img = torch.as_tensor(np.asarray(image) if not isinstance(image, torch.Tensor) else image, dtype=torch.float32).cuda()
    full, counts = predict_case_device(model, img, tile=tile, overlap=overlap, window=window, postprocess=postprocess, thresholds=thresholds)
    return full.cpu().numpy(), tuple(int(v) for v in counts.cpu().tolist())


# ---------------------------------------------------------------------- ensembles of models and soft labels (csrc/ensemble.hip)
def ensemble_mean_host(preds):
    """`sum(data_files) / len(data_files)` of the reference's notebooks on float32 arrays: S_1 = p_1, S_m = S_(m-1) + p_m in list order,
    one true division by the number of models."""
    acc = np.asarray(preds[0], np.float32)
    for p in preds[1:]:
        acc = acc + np.asarray(p, np.float32)
    return acc / np.float32(len(preds))


def ensemble_merge_host(outs_list, pad_left=(0, 0, 0), size=None):
    """Host restatement of `ensemble_merge`: outs_list[m] = the K = 4 flipped predictions [K,3,Dp,Hp,Wp] of model m.  Per model the
    un-flipped float32 mean (((o0 + o1) + o2) + o3) / K of test.py:134-138 on the un-padded box, then `ensemble_mean_host` over the models,
    the 0.5 threshold and the per-region counts (test.py:144).  Returns (mean float32 [3,*size], mask bool, (wt, tc, et))."""
    per_model = []
    for copies in _members_host(outs_list, pad_left, size):
        acc = copies[0]
        for o in copies[1:]:
            acc = acc + o
        per_model.append(acc / np.float32(len(copies)))
    mean = ensemble_mean_host(per_model)
    mask = mean > 0.5
    return mean, mask, tuple(int(v) for v in mask.sum(axis=(1, 2, 3)))


def ensemble_class_labels_host(preds):
    """The notebooks' rule for saved class maps [4,D,H,W]: argmax over the channels of the mean, class 3 stored as 4."""
    lab = np.argmax(ensemble_mean_host(preds), axis=0).astype(np.uint8)
    lab[lab == 3] = 4
    return lab


def compose_labels_host(mean):
    """test.py:144-159: labels {0,1,2,4} from region probabilities [3,D,H,W]; ET only with more than 32 ET voxels."""
    m = np.asarray(mean) > 0.5
    out = np.zeros(m.shape[1:], np.uint8)
    out[m[0]] = 2
    out[m[1]] = 1
    if m[2].sum() > 32:
        out[m[2]] = 4
    return out


def _members_host(outs_list, pad_left=(0, 0, 0), size=None):
    """The M x K un-flipped float32 members of an ensemble on the un-padded box: outs_list[m] = [K,3,Dp,Hp,Wp] as in `ensemble_merge_host`."""
    members = []
    for outs in outs_list:
        un = [np.flip(np.asarray(o, np.float32), axis=ax) if ax else np.asarray(o, np.float32) for o, ax in zip(outs, TTA_FLIPS)]
        sz = un[0].shape[1:] if size is None else size
        members.append([o[:, int(pad_left[0]):int(pad_left[0]) + int(sz[0]), int(pad_left[1]):int(pad_left[1]) + int(sz[1]),
                          int(pad_left[2]):int(pad_left[2]) + int(sz[2])] for o in un])
    return members


def second_moment_host(members):
    """T_M of csrc/uncertainty.hip: members[m][k] float32 arrays; per model q_m = ((o0*o0 + o1*o1) + o2*o2) + o3*o3, every product and
    sum rounded to float32, then T_1 = q_1, T_m = T_(m-1) + q_m in list order."""
    total = None
    for copies in members:
        q = None
        for o in copies:
            o = np.asarray(o, np.float32)
            q = o * o if q is None else q + o * o
        total = q if total is None else total + q
    return total


def uncertainty_std_host(members, mean=None):
    """The "std" map: members[m][k] = the M x K un-flipped float32 predictions of one shape, `mean` their float32 ensemble mean (formed as
    `ensemble_merge_host` forms it when not given).  e2 = T_M / (M*K), var = max(e2 - mean^2, 0) and u = floor(min(200*sqrt(var), 100) +
    0.5) in float64; uint8 in 0..100."""
    m, k = len(members), len(members[0])
    if mean is None:
        per_model = []
        for copies in members:
            acc = np.asarray(copies[0], np.float32)
            for o in copies[1:]:
                acc = acc + np.asarray(o, np.float32)
            per_model.append(acc / np.float32(k))
        mean = ensemble_mean_host(per_model)
    e2 = second_moment_host(members).astype(np.float64) / np.float64(m * k)
    mu = np.asarray(mean, np.float32).astype(np.float64)
    var = np.maximum(e2 - mu * mu, 0.0)
    return np.floor(np.minimum(200.0 * np.sqrt(var), 100.0) + 0.5).astype(np.uint8)


def uncertainty_entropy_host(mean):
    """The "entropy" map of the float32 ensemble mean: H = -(mu*log2(mu) + (1-mu)*log2(1-mu)) in float64, a term being 0 unless its
    argument lies inside (0, 1); u = floor(100*H + 0.5), uint8 in 0..100."""
    mu = np.asarray(mean, np.float32).astype(np.float64)
    nu = 1.0 - mu

    def term(a):
        inside = (a > 0.0) & (a < 1.0)
        return np.where(inside, a * np.log2(np.where(inside, a, 0.5)), 0.0)

    h = -(term(mu) + term(nu))
    return np.minimum(np.floor(100.0 * h + 0.5), 100.0).astype(np.uint8)


UNCERTAINTY_STEMS = ("whole", "core", "enhance")     # NAME_unc_<stem>: the challenge's file stems of the WT, TC and ET maps


def save_uncertainty(directory, name, maps):
    """The three files of one case, NAME_unc_whole.npy / _core / _enhance: maps uint8 [3,D,H,W] in the order WT, TC, ET."""
    os.makedirs(directory, exist_ok=True)
    for stem, m in zip(UNCERTAINTY_STEMS, maps):
        np.save(os.path.join(directory, "%s_unc_%s.npy" % (name, stem)), np.ascontiguousarray(m, dtype=np.uint8))


def _check_uncertainty(uncertainty):
    if uncertainty not in (None, "std", "entropy"):
        raise ValueError("uncertainty=%r: None, \"std\" or \"entropy\"" % (uncertainty,))
    return uncertainty


def _merge_step(acc, probs, index, count, lo, size, want_mean, uncertainty=None):
    """Fold model `index` of `count` into the running sum; the last one is fused with the finalize.  -> (acc, result or None).  With
    `uncertainty`, acc is the pair (sum, second-moment sum) of csrc/uncertainty.hip and the result gains the uint8 map."""
    if uncertainty is None:
        if index + 1 < count:
            return ops.ens_accumulate(probs, TTA_FLIPS, acc, lo, size), None
        return acc, ops.ens_accumulate_finalize(probs, TTA_FLIPS, acc, count, lo, size, want_mean=want_mean)
    s1, s2 = acc if acc is not None else (None, None)
    if index + 1 < count:
        return ops.unc_accumulate(probs, TTA_FLIPS, s1, s2, lo, size), None
    return acc, ops.unc_accumulate_finalize(probs, TTA_FLIPS, s1, s2, count, uncertainty, lo, size, want_mean=want_mean)


def ensemble_merge(probs_list, pad_left, size, want_mean=False, uncertainty=None):
    """The merge of an ensemble alone: probs_list[m] = [4,3,Dp,Hp,Wp] device tensor, the four test-time flips predicted by model m.
    Returns what `ops.tta_merge_box` returns for one model -- (mask uint8 [3,*size], counts int64 [3], mean float32 or None) -- for the
    float32 mean over the models of their un-flipped, un-padded means.  uncertainty="std" | "entropy": the same three, bit for bit, plus
    the uint8 [3,*size] uncertainty map of the M x 4 members (csrc/uncertainty.hip)."""
    _check_uncertainty(uncertainty)
    if not len(probs_list):
        raise ValueError("ensemble_merge: empty list")
    if any(tuple(p.shape) != tuple(probs_list[0].shape) for p in probs_list):
        raise ValueError("ensemble_merge: predictions of different shapes: %s" % [tuple(p.shape) for p in probs_list])
    acc, out = None, None
    for i, p in enumerate(probs_list):
        acc, out = _merge_step(acc, p, i, len(probs_list), pad_left, size, want_mean, uncertainty)
    return out


def _check_ensemble(models):
    models = list(models)
    if not models:
        raise ValueError("predict_case_ensemble: no model given")
    sig = [(int(m.conv_input.in_channels), int(m.number_of_outputs)) for m in models]
    if any(s != sig[0] for s in sig):
        raise ValueError("predict_case_ensemble: the models must agree on input channels and outputs, got (inputs, outputs) = %s" % sig)
    return models


def predict_case_ensemble_device(models, image, want_probs=False, uncertainty=None, tile=None, overlap=0.5, window="gaussian", postprocess=None,
                                 thresholds=None):
    """`predict_case_device` for a list of models: the case is prepared once, every model runs on the same batch of four flips and its
    prediction enters the running sum before the next forward starts; then labels, component rejection and paste as for one model.
    Returns (labels, counts) and, with want_probs, the float32 [3,D,H,W] mean probabilities pasted into the case's frame (zero outside
    the crop box).  An ensemble of one is `predict_case_device`.  uncertainty="std" | "entropy" appends the uint8 [3,D,H,W] uncertainty
    maps (WT, TC, ET; 0 certain .. 100 uncertain, zero outside the crop box) of the models x flips members, made in the same passes; the
    other results do not change.  `tile`, `overlap`, `window`: every model's forward runs as in `predict_case_device`.  `postprocess`: as
    there, on the masks of the ensemble mean; the soft labels and the uncertainty maps are those of the merge, not post-processed.
    `thresholds`: as there, on the ensemble mean; the soft labels and the uncertainty maps do not change."""
    _check_uncertainty(uncertainty)
    _check_postprocess(postprocess)
    thresholds = _check_thresholds(thresholds)
    models = _check_ensemble(models)
    for model in models:
        _check_tiled(model, tile, overlap, window)
    image = image.contiguous().float()
    if int(image.shape[0]) != int(models[0].conv_input.in_channels):
        raise ValueError("predict_case_ensemble: the case has %d modalities, the models take %d" % (int(image.shape[0]), int(models[0].conv_input.in_channels)))
    batch, lo, size, left, _padded = prepare_case_device(image)
    acc, out = None, None
    for i, model in enumerate(models):
        model.eval()
        if hasattr(model, "freeze_params"):
            model.freeze_params(True)
        with torch.no_grad():
            probs = _forward(model, batch, tile, overlap, window)    # [4,3,Dp,Hp,Wp]; merged below, released before the next forward
        acc, out = _merge_step(acc, probs, i, len(models), left, size,
                               want_probs or thresholds is not None or (postprocess is not None and postprocess.needs_probs), uncertainty)
        del probs
    mask, counts, mean = out[:3]
    labels, counts = _labels_from_masks(mask, counts, mean, postprocess, thresholds)
    res = (ops.paste_labels(labels, image.shape[1:], lo), counts)
    if want_probs:
        res += (ops.paste_probs(mean, image.shape[1:], lo),)
    if uncertainty is not None:
        res += (ops.paste_u8c(out[3], image.shape[1:], lo),)
    return res


def predict_case_ensemble(models, image, want_probs=False, uncertainty=None, tile=None, overlap=0.5, window="gaussian", postprocess=None, thresholds=None):
    """`predict_case` for a list of models (numpy or tensor in, numpy out): one upload, `predict_case_ensemble_device`, one download.
    Returns (labels, counts), then the mean probabilities with want_probs, then the uncertainty maps with `uncertainty`."""
    _check_uncertainty(uncertainty)
    _check_postprocess(postprocess)
    thresholds = _check_thresholds(thresholds)
    models = _check_ensemble(models)
    for model in models:
        _check_tiled(model, tile, overlap, window)
    img = torch.as_tensor(np.asarray(image) if not isinstance(image, torch.Tensor) else image, dtype=torch.float32).cuda()
    out = predict_case_ensemble_device(models, img, want_probs=want_probs, uncertainty=uncertainty, tile=tile, overlap=overlap, window=window,
                                       postprocess=postprocess, thresholds=thresholds)
    return (out[0].cpu().numpy(), tuple(int(v) for v in out[1].cpu().tolist())) + tuple(t.cpu().numpy() for t in out[2:])


# ---------------------------------------------------------------------- the post-processing flags of test, ensemble and postprocess
def add_postprocess_arguments(parser):
    """--min_volume, --min_confidence, --keep_largest, --fill_holes, --nest, --no_reject.  SUPPRESS: without them the namespace does not change."""
    import argparse
    names = list(ops.REGION_NAMES)
    parser.add_argument("--min_volume", default=argparse.SUPPRESS, type=int, nargs=3, metavar=("WT", "TC", "ET"),
                        help="drop the 26-connected components of a region with fewer voxels")
    parser.add_argument("--min_confidence", default=argparse.SUPPRESS, type=float, nargs=3, metavar=("WT", "TC", "ET"),
                        help="drop the components of a region whose mean probability is lower (0 .. 1)")
    parser.add_argument("--keep_largest", default=argparse.SUPPRESS, nargs="+", choices=names, help="regions of which only the largest component stays")
    parser.add_argument("--fill_holes", default=argparse.SUPPRESS, nargs="+", choices=names, help="regions whose enclosed holes are filled")
    parser.add_argument("--nest", default=argparse.SUPPRESS, action="store_true", help="cut TC to WT and ET to TC")
    parser.add_argument("--no_reject", default=argparse.SUPPRESS, action="store_true",
                        help="without the reference's rejection of small components of the union of all labels (ratio 0.1)")


def postprocess_from_args(opt):
    """The `PostProcess` of a parsed namespace; None when none of the flags of `add_postprocess_arguments` was given."""
    flags = ("min_volume", "min_confidence", "keep_largest", "fill_holes", "nest", "no_reject")
    if not any(hasattr(opt, f) for f in flags):
        return None
    which = lambda f: tuple(n in getattr(opt, f, ()) for n in ops.REGION_NAMES)
    return PostProcess(min_volume=tuple(getattr(opt, "min_volume", (0, 0, 0))), min_confidence=tuple(getattr(opt, "min_confidence", (0.0, 0.0, 0.0))),
                       keep_largest=which("keep_largest"), fill_holes=which("fill_holes"), nest=getattr(opt, "nest", False),
                       reject_ratio=None if getattr(opt, "no_reject", False) else 0.1)


# ---------------------------------------------------------------------- the threshold flags of test and ensemble
def add_threshold_arguments(parser):
    """--thresholds WT TC ET, --thresholds_file FILE.  SUPPRESS: without them the namespace does not change."""
    import argparse
    parser.add_argument("--thresholds", default=argparse.SUPPRESS, type=float, nargs=3, metavar=("WT", "TC", "ET"),
                        help="region masks are `probability > threshold` instead of `> 0.5`")
    parser.add_argument("--thresholds_file", default=argparse.SUPPRESS, type=str,
                        help="the JSON `python -m brats2019_amd.validate --calibration --thresholds_output` writes")


def thresholds_from_args(opt):
    """The `thresholds=` of a parsed namespace; None when neither flag of `add_threshold_arguments` was given."""
    if hasattr(opt, "thresholds") and hasattr(opt, "thresholds_file"):
        raise ValueError("--thresholds and --thresholds_file exclude each other")
    if hasattr(opt, "thresholds_file"):
        import json
        with open(opt.thresholds_file) as f:
            return _check_thresholds(json.load(f)["thresholds"])
    return _check_thresholds(getattr(opt, "thresholds", None))
