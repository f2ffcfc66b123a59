"""Step time of the FGCNN backbone (model_name=fgcnn) on one GPU: Avazu-shaped synthetic data, batch 4096, F = 23,
E = 16, the flag-default channel lists (channels 14,16,18,20, kernel heights 7, pooling 2, recombined 3: T = 92
feature rows); MFP, RFD and finetune (CTR) steps through Trainer.run_step (the captured step replayed after the first
few).  One JSON line per arm.
--dtype fp32 bf16 runs every step arm in both compute modes, alternated arm by arm in the one process;
--rounds N repeats the whole alternation N times (take the median of an arm's lines).
--torch-trunk adds forward + backward of the trunk alone (embeddings [B,23,16] -> the heads' input [B,5658]): the mapx
conv / batch-norm / pool / inner-product kernels against torch's own conv2d / batch_norm / max_pool2d / bmm +
masked_select on the same GPU, same fp32 weights (the recombine layers are torch.nn.Linear there).
    python tools/fgcnn_bench.py [--pt MFP RFD CTR] [--dtype fp32 bf16] [--rounds 3] [--steps 100] [--torch-trunk]
                                [--no-steps]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))

F_AVAZU, V_AVAZU = 23, 9449445


def make_config(a, pt, feat_count, dtype="fp32"):
    from mapx.arguments import MODEL_FLAGS, Config
    fg = {n: d for n, _t, d, _h in MODEL_FLAGS if n in ("share_embedding", "channels", "kernel_heights", "pooling_sizes",
                                                        "recombined_channels", "conv_act")}      # the flag defaults
    return Config(**fg, model_name="fgcnn", data_dir=None, input_size=a.vocab, num_fields=F_AVAZU, embed_size=16,
                  embed_dropout_rate=0.0, embed_norm=False, hidden_size=a.hidden, num_hidden_layers=a.layers,
                  hidden_act="relu", hidden_dropout_rate=0.0, num_cross_layers=0, pt_neg_num=25, proj_size=32,
                  pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt, RFD_replace="Unigram",
                  feat_count=feat_count, seed=42, rank=0, compute_dtype=dtype)


def step_arm(a, pt, dtype, ids, labels, feat_count, device):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    torch.manual_seed(42)
    cfg = make_config(a, pt, feat_count, dtype)
    model = build_backbone(cfg)
    targs = TrainingArguments(output_dir="/tmp/mapx_fgcnn_bench", per_gpu_train_batch_size=a.batch,
                              per_gpu_eval_batch_size=a.batch, learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2,
                              num_train_epochs=1000, pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt,
                              RFD_replace="Unigram", sampling_method="randint", mask_ratio=0.3, seed=42)
    targs._device = device
    tr = Trainer(model, cfg, targs, OurDataset(ids, labels), OurDataset(ids[:a.batch], labels[:a.batch]))
    train = tr._begin("fgcnn_bench")
    gen = tr._generator()
    state = {"it": train.batches(a.batch, True, gen, (0, 1), rows=True)}

    def next_batch():
        try:
            return next(state["it"])
        except StopIteration:
            state["it"] = train.batches(a.batch, True, gen, (0, 1), rows=True)
            return next(state["it"])

    kind = pt.lower()
    tr.model.train()
    for _ in range(a.warmup):
        tr.run_step(kind, *next_batch())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.run_step(kind, *next_batch())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    live = [g for g in tr._graphs.values() if not isinstance(g, int)]
    return {"arm": f"fgcnn {pt}", "dtype": dtype, "batch": a.batch, "feature_rows": model.total_features,
            "ms_per_step": 1e3 * dt / a.steps, "samples_per_s": a.batch * a.steps / dt, "graphed": bool(live),
            "loss": float(out[0].detach())}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


class TorchTrunk(torch.nn.Module):
    """The same trunk on torch's own ops, with the mapx block's weights."""

    def __init__(self, block, total):
        super().__init__()
        self.convs, self.bns, self.pools, self.recs = (torch.nn.ModuleList() for _ in range(4))
        height = F_AVAZU
        for stage, rec, ps in zip(block.conv_layers, block.recombine_layers, block.pooling_sizes):
            w = stage["0"].weight
            conv = torch.nn.Conv2d(w.shape[1], w.shape[0], (w.shape[2], 1), padding=((w.shape[2] - 1) // 2, 0))
            conv.load_state_dict(stage["0"].state_dict())
            bn = torch.nn.BatchNorm2d(w.shape[0])
            bn.load_state_dict(stage["1"].state_dict())
            lin = torch.nn.Linear(rec["0"].in_features, rec["0"].out_features)
            lin.load_state_dict(rec["0"].state_dict())
            self.convs.append(conv), self.bns.append(bn), self.recs.append(lin)
            self.pools.append(torch.nn.MaxPool2d((ps, 1), padding=(height % ps, 0)))
            height = -(-height // ps)
        self.act = torch.tanh if block.act == "tanh" else torch.relu
        self.register_buffer("mask", torch.triu(torch.ones(total, total), 1).bool())

    def forward(self, e):
        x, new = e.unsqueeze(1), []
        for conv, bn, pool, rec in zip(self.convs, self.bns, self.pools, self.recs):
            x = pool(self.act(bn(conv(x))))
            new.append(self.act(rec(x.flatten(1))).reshape(e.shape[0], -1, e.shape[2]))
        c = torch.cat([e] + new, dim=1)
        ip = torch.masked_select(torch.bmm(c, c.transpose(1, 2)), self.mask).view(e.shape[0], -1)
        return torch.cat([c.flatten(1), ip], dim=1)


def trunk_arm(a, feat_count, device):
    from mapx.layers import inner_product
    from mapx.models import BaseModel
    torch.manual_seed(42)
    model = BaseModel.from_config(make_config(a, "CTR", feat_count)).to(device).train()
    block = model.fgcnn_layer
    ref = TorchTrunk(block, model.total_features).to(device).train()

    def mapx_trunk(e):
        c = torch.cat([e, block(e.unsqueeze(1))], dim=1)
        return torch.cat([c.flatten(1), inner_product(c)], dim=1)

    x = torch.randn(a.batch, F_AVAZU, 16, device=device, requires_grad=True)
    g = torch.randn(a.batch, model.final_dim, device=device)
    err = float((mapx_trunk(x) - ref(x)).abs().max())

    def run(m):
        def fn():
            m(x).backward(g)
        return fn
    ms_mapx = _time(run(mapx_trunk), a.steps, a.warmup)
    ms_torch = _time(run(ref), a.steps, a.warmup)
    with torch.no_grad():
        fwd_mapx = _time(lambda: mapx_trunk(x), a.steps, a.warmup)
        fwd_torch = _time(lambda: ref(x), a.steps, a.warmup)
    return {"arm": "fgcnn trunk fwd+bwd", "batch": a.batch, "feature_rows": model.total_features, "mapx_ms": ms_mapx,
            "torch_ms": ms_torch, "speedup": ms_torch / ms_mapx, "mapx_fwd_ms": fwd_mapx, "torch_fwd_ms": fwd_torch,
            "max_abs_diff": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pt", nargs="+", default=["MFP", "RFD", "CTR"], choices=["MFP", "RFD", "CTR"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--vocab", type=int, default=V_AVAZU)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["fp32"], choices=["fp32", "bf16"], help="compute_dtype of the step arms")
    ap.add_argument("--rounds", type=int, default=1, help="repeat the alternation of the step arms")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-trunk", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="only the --torch-trunk arm")
    a = ap.parse_args()
    from mapx.dataset import synth_table
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ids, labels, _, _ = synth_table(a.rows, F_AVAZU, a.vocab, seed=42)
    feat_count = torch.from_numpy(np.bincount(ids.reshape(-1), minlength=a.vocab).astype(np.float32))
    if not a.no_steps:
        for rnd in range(a.rounds):
            for pt in a.pt:
                for dtype in a.dtype:
                    print(json.dumps(dict(step_arm(a, pt, dtype, ids, labels, feat_count, device), round=rnd)), flush=True)
    if a.torch_trunk:
        print(json.dumps(trunk_arm(a, feat_count, device)), flush=True)


if __name__ == "__main__":
    main()
