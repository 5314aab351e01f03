"""Data-parallel training with the boundary and Hausdorff-DT losses: two gloo ranks as fresh child processes share cuda:0.  With
criterion=[BoundaryLoss(priority=0.01), HausdorffDTLoss(priority=0.01)] the replicas must stay identical and reproduce the
single-process global-batch run: the distance maps are per sample, so the one float64 sum of each loss is all that crosses the ranks.
Plain SGD and the bars of tests/test_hardcrit_dp.py (which are those of tests/test_criteria_dp.py), for the reasons given there."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "boundary_dp_worker.py")


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
    return [dict(np.load(os.path.join(str(out_dir), "boundary_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.mark.timeout(1800)
def test_trainer_with_boundary_and_hausdorff_dt_is_data_parallel(tmp_path):
    (ref,) = _launch(tmp_path, 1)
    r0, r1 = _launch(tmp_path, 2)
    assert int(r0["global_step"]) == int(ref["global_step"]) == 2
    assert ref["losses"].shape == (4,) and np.isfinite(ref["losses"]).all()        # 2 criteria x 2 steps
    assert not ref["data_parallel"].any() and r0["data_parallel"].all() and r1["data_parallel"].all()
    np.testing.assert_array_equal(r0["weights"], r1["weights"])                     # replicas stay identical
    np.testing.assert_array_equal(r0["losses"], r1["losses"])
    print("losses: two ranks %s, one process %s" % (r0["losses"], ref["losses"]))
    np.testing.assert_allclose(r0["losses"], ref["losses"], rtol=0, atol=5e-5)
    dw = np.abs(r0["weights"] - ref["weights"])
    print("weights: max difference %.3e, mean %.3e" % (dw.max(), dw.mean()))
    assert dw.max() <= 2 * (1e-3 + 5e-4) + 1e-6 and dw.mean() < 2e-5, (dw.max(), dw.mean())
