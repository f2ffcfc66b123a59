"""Worker for tests/test_replica_check_gpu.py: WORLD_SIZE gloo ranks on ONE GPU.

  table | moment   4 MFP steps as tests/dp_worker.py runs them, flush, check_replicas (must pass); then rank 1 alone
                   moves one element of the NCE table's parameter (table) or of a dense first moment (moment: the
                   weights stay equal, only optimizer state differs) by one ulp, and every rank must catch
                   ReplicaDivergence from the next check_replicas;
  trainer          one epoch of Trainer.MFP_pretrain on a tiny synthetic table; rank 1 moves one element of the NCE
                   table behind the epoch-end flush.  With MAPX_REPLICA_CHECK=0 the run finishes; by default every
                   rank's MFP_pretrain raises ReplicaDivergence.

Every rank writes what it saw as JSON to `out.{rank}` and leaves through destroy_process_group."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROW, COL = 7, 3                 # table / moment runs: the NCE-table element rank 1 moves
TRAINER_ROW = 2900              # trainer run: a row in the second chunk of the [3000, 32] table


def _one_ulp(tensor, index):
    tensor.view(-1).view(torch.int32)[index] += 1


def _report(e):
    return dict(raised=True, entry=e.entry, row_lo=e.row_lo, row_hi=e.row_hi, ranks=e.ranks, where=e.where,
                elem_lo=e.elem_lo, elem_hi=e.elem_hi)


def steps_then_perturb(what, rank, world):
    import paramgen as pg
    from util import build_model, load_case, t
    from mapx import ops, parallel, replica
    from mapx.arguments import TrainingArguments
    from mapx.optim import MapxOptimizer
    case = "B_f25_b64"
    cfg = pg.CASES[case]
    _, _, inp, params = load_case(case, "MFP")
    model = build_model(cfg, "MFP", params, inp["feat_count"])
    targs = TrainingArguments(output_dir="/tmp/x", learning_rate=1e-3, weight_decay=5e-2, lr_sched="cosine")
    opt = MapxOptimizer(model, targs, num_training_steps=8, num_warmup_steps=0)
    B = cfg["B"]
    lo, hi = (rank * B // world, (rank + 1) * B // world)
    L = inp["masked_index"].shape[1]
    model.train()
    for step in range(4):
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(step))
        ids, mi, noise = (t(inp[k])[perm][lo:hi].to("cuda") for k in ("input_ids", "masked_index", "noise"))
        masked, labels, _ = ops.dynamic_mask_mfp(ids, L, masked_index=mi)
        model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=noise)[0].backward()
        parallel.sync_gradients(opt)
        opt.step()
    opt.flush()
    replica.check_replicas(model, opt, "after 4 steps")            # identical replicas: returns
    if rank == 1:
        if what == "table":
            w = model.mfp_criterion.table.p0.data
            _one_ulp(w, ROW * w.shape[1] + COL)
        else:
            _one_ulp(opt.groups[0]["m"], 5)
    try:
        replica.check_replicas(model, opt, "after the perturbation")
    except replica.ReplicaDivergence as e:
        return _report(e)
    return dict(raised=False)


def trainer_epoch(rank, world, out):
    from mapx import replica
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(256 * 2 * 2, 23, cfg["V"], seed=3)             # 2 rounds of 2 x 256 rows
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    torch.manual_seed(5)
    config = make_config(cfg, "MFP", cnt)
    config.rank = rank
    model = BaseModel.from_config(config)
    targs = TrainingArguments(output_dir=os.path.dirname(out), per_gpu_train_batch_size=256,
                              per_gpu_eval_batch_size=256, learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2,
                              num_train_epochs=1, pretrain=True, pt_type="MFP", sampling_method="randint",
                              mask_ratio=0.3, logging_steps=100, seed=11)
    targs._device = torch.device("cuda:0")
    fired = []

    class Hooked(Trainer):
        def get_optimizer(self, *a):
            opt = super().get_optimizer(*a)
            flush = opt.flush

            def flush_then_perturb():
                flush()
                if rank == 1 and not fired:         # once, behind the epoch-end flush: before the epoch's check
                    w = self.model.mfp_criterion.table.p0.data
                    _one_ulp(w, TRAINER_ROW * w.shape[1] + COL)
                fired.append(1)
            opt.flush = flush_then_perturb
            return opt

    tr = Hooked(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:256], labels[:256]))
    assert tr.world == world and tr.rank == rank
    tr.use_graph = False
    try:
        tr.MFP_pretrain()
    except replica.ReplicaDivergence as e:
        return _report(e)
    assert tr.global_step == 2 and fired
    return dict(raised=False)


def main(out, what):
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    seen = trainer_epoch(rank, world, out) if what == "trainer" else steps_then_perturb(what, rank, world)
    with open(f"{out}.{rank}", "w") as f:
        json.dump(seen, f)
    torch.cuda.synchronize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
