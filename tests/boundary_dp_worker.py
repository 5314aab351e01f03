#!/usr/bin/env python3
"""One data-parallel rank on cuda:0 training with the boundary and Hausdorff-DT losses (child process of tests/test_boundary_dp.py).

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/boundary_dp_worker.py <outdir>

train.Trainer.train for one epoch of 2 global batches of 2 at 32^3 with criterion=[BoundaryLoss(priority=0.01),
HausdorffDTLoss(priority=0.01)] and plain SGD (why not Adam: tests/test_hardcrit_dp.py); W ranks share the GPU over gloo, with W = 1 the
same script gives the single-process global-batch run.  Writes <outdir>/boundary_w<W>_r<rank>.npz: the flat weights and the logged
loss values.
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
SEED = 53


def train(out_dir, tag, world, criterion, loader):
    from brats2019_amd import model as M, train as TR, metrics as MT
    net = M.UNet(**CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_params(SEED, **CFG).items()})
    tr = TR.Trainer(name=tag, models_root=os.path.join(out_dir, "models_w%d" % world), model=net, rewrite=True, connect_tb=False)
    losses = []

    class Rec:
        def add_scalar(self, name, val, step):
            if name.startswith("loss/"):
                losses.append(float(val))
    tr.tb_writer = Rec()
    tr.train(criterion=criterion, optimizer=torch.optim.SGD, optimizer_params=dict(lr=1e-2),
             scheduler=torch.optim.lr_scheduler.StepLR, scheduler_params=dict(step_size=1, gamma=0.5),
             training_data_loader=loader, evaluation_data_loader=[([loader[1][0][0][:1]], [loader[1][1][0][:1]])], split_into_tiles=False,
             pretrained_weights=None, train_metrics=[MT.Dice(name="Dice")], val_metrics=[MT.Dice(name="Dice")], track_metric="Dice",
             epoches=1, default_val=np.zeros(3), comparator=lambda a, b: np.min(a) + np.mean(a) > np.min(b) + np.mean(b),
             eval_cpu=False, continue_form_pretraining=False)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()
    return flat, np.asarray(losses), tr.state.global_step


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from brats2019_amd import loss as L
    loader = [([torch.from_numpy(O.make_input(2, *DHW, seed=SEED + i))], [torch.from_numpy(O.make_target(2, *DHW, seed=SEED + i))])
              for i in range(2)]
    out = {}
    criterion = [L.BoundaryLoss(priority=0.01), L.HausdorffDTLoss(priority=0.01)]
    out["weights"], out["losses"], out["global_step"] = train(out_dir, "pair", world, criterion, loader)
    out["data_parallel"] = np.asarray([bool(c.data_parallel) for c in criterion])
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "boundary_w%d_r%d.npz" % (world, rank)), **out)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
