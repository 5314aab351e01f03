"""Data-parallel training with the lesion-wise Dice loss: two gloo ranks as fresh child processes share cuda:0.  With
criterion=[Dice_loss_joint(), LesionWiseDiceLoss(priority=0.5)] the replicas must stay identical and reproduce the single-process
global-batch run: the lesions are per sample, so the sum of the pair losses and the number of pairs that hold a lesion are all that
cross the ranks.  Rank 1's shard has an empty channel, so the ranks' own pair counts differ (3 and 2) and the loss is right only with
the all-reduced count (5).  Plain SGD and the bars of tests/test_boundary_dp.py (which are those of tests/test_criteria_dp.py), for the
reasons given there."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "lesion_loss_dp_worker.py")


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
    return [dict(np.load(os.path.join(str(out_dir), "lesion_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.mark.timeout(1800)
def test_trainer_with_the_lesion_wise_dice_loss_is_data_parallel(tmp_path):
    (ref,) = _launch(tmp_path, 1)
    r0, r1 = _launch(tmp_path, 2)
    assert int(r0["global_step"]) == int(ref["global_step"]) == 2
    assert ref["losses"].shape == (4,) and np.isfinite(ref["losses"]).all()        # 2 criteria x 2 steps
    assert (float(ref["local_pairs"]), float(r0["local_pairs"]), float(r1["local_pairs"])) == (5.0, 3.0, 2.0)       # M differs between the ranks
    assert not ref["data_parallel"].any() and r0["data_parallel"].all() and r1["data_parallel"].all()
    np.testing.assert_array_equal(r0["weights"], r1["weights"])                     # replicas stay identical
    np.testing.assert_array_equal(r0["losses"], r1["losses"])
    print("losses: two ranks %s, one process %s" % (r0["losses"], ref["losses"]))
    np.testing.assert_allclose(r0["losses"], ref["losses"], rtol=0, atol=5e-5)
    dw = np.abs(r0["weights"] - ref["weights"])
    print("weights: max difference %.3e, mean %.3e" % (dw.max(), dw.mean()))
    assert dw.max() <= 2 * (1e-3 + 5e-4) + 1e-6 and dw.mean() < 2e-5, (dw.max(), dw.mean())
