"""Data-parallel metrics.RMSE: two gloo ranks as fresh child processes share cuda:0 and train with train_metrics=[RMSE()].  Trainer.train
sets RMSE.data_parallel, update() all-reduces the two sums before the square root, and the epoch's value is the reference's: the RMSE of
the gathered global batch, not the mean of the ranks' shard values."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "overlap_dp_worker.py")


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
    return [dict(np.load(os.path.join(str(out_dir), "rmse_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.mark.timeout(1800)
def test_rmse_is_the_global_batch_value_under_data_parallelism(tmp_path):
    (ref,) = _launch(tmp_path, 1)
    r0, r1 = _launch(tmp_path, 2)
    assert not bool(ref["data_parallel"]) and bool(r0["data_parallel"]) and bool(r1["data_parallel"])
    # single process: RMSE is the global-batch value by construction
    np.testing.assert_allclose(float(ref["rmse"]), float(ref["probe"][0]), rtol=1e-6)
    for r in (r0, r1):
        glob, shard_mean = float(r["probe"][0]), float(r["probe"][1])
        np.testing.assert_allclose(float(r["rmse"]), glob, rtol=1e-6)
        assert abs(shard_mean - glob) > 1e-4 * glob                     # the mean of the shards' roots is 100 tolerances away
    np.testing.assert_allclose(float(r0["rmse"]), float(ref["rmse"]), rtol=1e-4)   # and it is the single-process run's value
