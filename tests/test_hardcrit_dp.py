"""Data-parallel training with the focal, Tversky and top-k losses: two gloo ranks as fresh child processes share cuda:0.  With
criterion=[FocalLoss(), TverskyLoss()] both must reproduce the single-process global-batch run (the bars of tests/test_criteria_dp.py).
TopKLoss selects within each rank's shard, which is not the single-process global-batch loss: with it in the list the replicas must stay
identical and log the mean of the two per-rank values.

The optimizer is plain SGD(lr=1e-2), not the Adam of tests/test_criteria_dp.py.  An SGD step is linear in the gradient: a wrong factor such as
a missing 1/world moves the weights and the second step's losses at once, and rounding differences stay rounding differences.  Adam's first
step is lr * g / (|g| + eps), which hides any common factor and turns the rounding noise of near-zero gradients (two ranks add per-sample
gradients in another order than one process does) into weight differences of +-lr.  Measured on the MI355X with that test's Adam settings, the
second step's loss moved, two ranks against one process, by 1.0e-4 relative for FocalLoss (2.2e-4 of 2.12) and by 1.3e-4 relative for the
existing CE_Loss (4.7e-6 of 0.036): the same sensitivity, and only the size of the focal value puts it past an absolute 5e-5.  With SGD the
largest difference is 3.8e-6 for [FocalLoss(), TverskyLoss()].  The bars below are those of tests/test_criteria_dp.py, unchanged."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "hardcrit_dp_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(out_dir, world):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, str(out_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode("utf-8", "replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-4000:])
    return [dict(np.load(os.path.join(str(out_dir), "hardcrit_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.mark.timeout(1800)
def test_trainer_with_focal_tversky_and_topk_is_data_parallel(tmp_path):
    (ref,) = _launch(tmp_path, 1)
    r0, r1 = _launch(tmp_path, 2)
    assert int(r0["global_step"]) == int(ref["global_step"]) == 2
    assert ref["losses"].shape == (4,) and np.isfinite(ref["losses"]).all()        # 2 criteria x 2 steps
    np.testing.assert_array_equal(r0["weights"], r1["weights"])                     # replicas stay identical
    np.testing.assert_array_equal(r0["losses"], r1["losses"])
    np.testing.assert_allclose(r0["losses"], ref["losses"], rtol=0, atol=5e-5)
    dw = np.abs(r0["weights"] - ref["weights"])
    assert dw.max() <= 2 * (1e-3 + 5e-4) + 1e-6 and dw.mean() < 2e-5, (dw.max(), dw.mean())
    # [Dice_loss_joint(), TopKLoss()]: identical replicas; the logged top-k value of the first step is the mean of the ranks' own
    np.testing.assert_array_equal(r0["topk_weights"], r1["topk_weights"])
    np.testing.assert_array_equal(r0["topk_losses"], r1["topk_losses"])
    assert r0["topk_losses"].shape == (4,) and np.isfinite(r0["topk_losses"]).all()
    assert not np.array_equal(r0["topk_weights"], r0["weights"])
    local = [float(r0["topk_local"]), float(r1["topk_local"])]
    assert local[0] != local[1]
    np.testing.assert_allclose(r0["topk_losses"][1], 0.5 * (local[0] + local[1]), rtol=1e-6, atol=0)
