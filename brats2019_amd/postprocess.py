"""Region-wise post-processing of saved predictions: every uint8 `.npy` label volume [D,H,W] with values {0,1,2,4} of a directory goes
through `ops.postprocess_regions` (csrc/postprocess.hip; INTEGRATION.md states the definition) and is written under the same name.

    python -m brats2019_amd.postprocess --predictions DIR --output DIR [--min_volume WT TC ET] [--keep_largest wt|tc|et ...]
                                        [--fill_holes wt|tc|et ...] [--nest] [--no_reject] [--host]

The regions are WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4} (3 is read as 4); a label above 4 is background and is counted as invalid.  The
result is composed as the reference composes it -- 2 where WT, 1 where TC, 4 where ET -- without the ET > 32 rule.  Then the reference's
rejection of small components of the union of all labels (test.py:162-164, ratio 0.1) runs, as `inference.PostProcess` keeps it by
default; `--no_reject` leaves the region pass alone.  A saved label volume carries no probabilities: `--min_confidence` is refused.
One line of statistics per case: per region the components found, those removed by volume and by `--keep_largest`, and the voxels filled.
`python -m brats2019_amd.validate --lesionwise` scores the directory before and after.  `--host` computes the same with numpy and scipy
(`inference.postprocess_regions_host`, no GPU)."""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import inference

parser = argparse.ArgumentParser(description="Region-wise post-processing of saved label volumes (MI355X HIP engine)")
parser.add_argument("--predictions", required=True, type=str, help="directory of uint8 .npy label volumes [D,H,W]")
parser.add_argument("--output", required=True, type=str, help="directory for the post-processed label volumes")
parser.add_argument("--host", action="store_true", help="numpy / scipy instead of the device kernels")
inference.add_postprocess_arguments(parser)


def run_host(labels, post):
    out, counts, stats = inference.postprocess_regions_host(labels, want_stats=True, **post.regions())
    if post.reject_ratio is not None:
        out = inference.postprocess_labels(out, post.reject_ratio)
    return out, counts, stats


def run_device(labels, post):
    import torch
    from . import ops
    out, counts, stats = ops.postprocess_regions(torch.as_tensor(labels).cuda(), want_stats=True, **post.regions())
    if post.reject_ratio is not None:
        ops.cc_reject(out, post.reject_ratio)
    return out.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy()


def main(argv=None):
    opt = parser.parse_args(argv)
    post = inference.postprocess_from_args(opt) or inference.PostProcess()
    if post.needs_probs:
        parser.error("--min_confidence needs probabilities: a saved label volume has none (use it with brats2019_amd.test or ensemble --rule regions)")
    names = sorted(f for f in os.listdir(opt.predictions) if f.endswith(".npy"))
    if not names:
        raise SystemExit("no .npy predictions in %s" % opt.predictions)
    os.makedirs(opt.output, exist_ok=True)
    results = []
    for name in names:
        labels = np.load(os.path.join(opt.predictions, name))
        if labels.ndim != 3 or labels.dtype != np.uint8:
            raise SystemExit("%s: expected a uint8 label volume [D,H,W], got %s %s" % (os.path.join(opt.predictions, name), labels.dtype, labels.shape))
        out, counts, stats = (run_host if opt.host else run_device)(np.ascontiguousarray(labels), post)
        np.save(os.path.join(opt.output, name), out)
        print(name[:-4], out.shape, " ".join("%s found %d volume %d largest %d filled %d voxels %d" % (r.upper(), s[0], s[1], s[3], s[4], c)
                                               for r, s, c in zip(inference.ops.REGION_NAMES, stats.tolist(), counts.tolist())), "invalid %d" % stats[0, 5])
        results.append((name[:-4], counts, stats))
    return results


if __name__ == "__main__":
    main()
