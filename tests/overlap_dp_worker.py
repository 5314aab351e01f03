#!/usr/bin/env python3
"""One data-parallel rank on cuda:0 training with metrics.RMSE in train_metrics (child process of tests/test_overlap_dp.py).

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/overlap_dp_worker.py <outdir>

train.Trainer.train for one epoch of 2 global batches of 2 at 32^3.  Next to RMSE a probe metric gathers every rank's output and target
and forms the reference's value on the global batch in float64 (sqrt of the mean over the gathered tensors), and the mean of the
per-shard roots that an unreduced RMSE would give.  Writes <outdir>/rmse_w<W>_r<rank>.npz: the logged RMSE, the probe's two values.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

from oracle import resunet_oracle as O       # seeded inputs / weights only (data, not arithmetic)

CFG = O.DEFAULT_CFG
DHW = (32, 32, 32)
SEED = 47


class GlobalRMSEProbe(object):
    """Metrics protocol; no `data_parallel` attribute, so Trainer leaves it alone.  accumulator = [global-batch RMSE, shard RMSE]."""

    def __init__(self):
        self.name = "probe"
        self.reset()

    def reset(self):
        self.accumulator = np.zeros(2)
        self.samples = 0.0

    def update(self, ground, predict):
        p = predict[0].detach().double().cpu()
        g = ground[0].detach().double().cpu()
        shard = float(torch.sqrt(((p - g) ** 2).mean()))
        if dist.is_initialized():
            ps, gs = [torch.empty_like(p) for _ in range(dist.get_world_size())], [torch.empty_like(g) for _ in range(dist.get_world_size())]
            dist.all_gather(ps, p)
            dist.all_gather(gs, g)
            p, g = torch.cat(ps), torch.cat(gs)
        self.accumulator = self.accumulator + np.array([float(torch.sqrt(((p - g) ** 2).mean())), shard])
        self.samples += 1

    def get(self):
        return self.accumulator / self.samples


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from brats2019_amd import model as M, loss as L, train as TR, metrics as MT
    net = M.UNet(**CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(SEED, **CFG).items()})
    tr = TR.Trainer(name="rmse", models_root=os.path.join(out_dir, "models_w%d" % world), model=net, rewrite=True, connect_tb=False)
    logged = {}

    class Rec:
        def add_scalar(self, tag, val, step):
            logged[tag] = float(val)
    tr.tb_writer = Rec()
    targets = [O.make_target(2, *DHW, seed=SEED + i) for i in range(2)]
    for t in targets:
        t[1] = 0.0                         # the second sample (rank 1's shard) has no tumour: the shards' RMSEs differ widely
    loader = [([torch.from_numpy(O.make_input(2, *DHW, seed=SEED + i))], [torch.from_numpy(targets[i])]) for i in range(2)]
    rmse, probe = MT.RMSE(), GlobalRMSEProbe()
    tr.train(criterion=[L.Dice_loss_joint(index=0, priority=1), L.BCE_Loss(index=0, bg_weight=1e-2)],
             optimizer=torch.optim.Adam, optimizer_params=dict(lr=1e-3, weight_decay=1e-6, amsgrad=True),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[([loader[1][0][0][:1]], [loader[1][1][0][:1]])], split_into_tiles=False,
             pretrained_weights=None, train_metrics=[rmse, probe], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice",
             epoches=1, default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rmse_w%d_r%d.npz" % (world, rank)), rmse=logged["train/RMSE-0"], probe=probe.get(),
             data_parallel=rmse.data_parallel)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
