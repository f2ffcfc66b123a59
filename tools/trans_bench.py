"""Step time of the Transformer backbone (model_name=trans) on one GPU: Avazu-shaped synthetic data, batch 4096,
E = hidden = 16, 3 layers, intermediate 128, 1 and 2 heads; MFP, RFD and finetune (CTR, output_reduction attn,fc)
steps through Trainer.run_step (the captured step replayed after the first few).  One JSON line per arm.
--dtype fp32 bf16 runs every step arm in both compute modes, alternated arm by arm in the one process.
--torch-trunk adds, per head count, forward + backward of the trunk alone: the mapx encoder against
torch.nn.TransformerEncoder (fp32, same weights, same GPU).
    python tools/trans_bench.py [--heads 1 2] [--pt MFP RFD CTR] [--dtype fp32 bf16] [--steps 100] [--torch-trunk]"""
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


def make_config(a, heads, pt, feat_count, dtype="fp32"):
    from mapx.arguments import Config
    return Config(model_name="trans", data_dir=None, input_size=a.vocab, num_fields=F_AVAZU, embed_size=16,
                  embed_dropout_rate=0.0, embed_norm=False, hidden_size=16, num_hidden_layers=3, hidden_act="relu",
                  hidden_dropout_rate=a.dropout, num_attn_heads=heads, intermediate_size=128, norm_first=False,
                  layer_norm_eps=1e-12, output_reduction="attn,fc", use_lr=False, dnn_size=1000, num_dnn_layers=0,
                  dnn_act="relu", dnn_drop=0.0, num_cross_layers=0, pt_neg_num=25, proj_size=32, pretrain=pt != "CTR",
                  pt_type="MFP" if pt == "CTR" else pt, RFD_replace="Unigram", feat_count=feat_count, seed=42, rank=0,
                  compute_dtype=dtype)


def step_arm(a, heads, pt, dtype, ids, labels, feat_count, device):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    torch.manual_seed(42)
    cfg = make_config(a, heads, pt, feat_count, dtype)
    model = build_backbone(cfg)
    targs = TrainingArguments(output_dir="/tmp/mapx_trans_bench", per_gpu_train_batch_size=a.batch,
                              per_gpu_eval_batch_size=a.batch, learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2,
                              num_train_epochs=1000, pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt,
                              RFD_replace="Unigram", sampling_method="randint", mask_ratio=0.3, seed=42)
    targs._device = device
    tr = Trainer(model, cfg, targs, OurDataset(ids, labels), OurDataset(ids[:a.batch], labels[:a.batch]))
    train = tr._begin("trans_bench")
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
    return {"arm": f"trans {pt}", "dtype": dtype, "heads": heads, "batch": a.batch, "ms_per_step": 1e3 * dt / a.steps,
            "samples_per_s": a.batch * a.steps / dt, "graphed": bool(live), "loss": float(out[0].detach())}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def trunk_arm(a, heads, feat_count, device):
    """Forward + backward of the 3-layer trunk on x [4096, 23, 16]: mapx against torch, same fp32 weights."""
    from mapx.models import BaseModel
    torch.manual_seed(42)
    model = BaseModel.from_config(make_config(a, heads, "CTR", feat_count)).to(device).train()
    enc = model.encoder
    layer = torch.nn.TransformerEncoderLayer(16, heads, 128, dropout=a.dropout, activation="relu", layer_norm_eps=1e-12,
                                             batch_first=True, norm_first=False)
    ref = torch.nn.TransformerEncoder(layer, 3, enable_nested_tensor=False).to(device).train()
    ref.load_state_dict(enc.state_dict())
    x = torch.randn(a.batch, F_AVAZU, 16, device=device, requires_grad=True)
    g = torch.randn(a.batch, F_AVAZU, 16, device=device)

    def run(m):
        def fn():
            m(x).backward(g)
        return fn
    ms_mapx = _time(run(enc), a.steps, a.warmup)
    ms_torch = _time(run(ref), a.steps, a.warmup)
    with torch.no_grad():
        fwd_mapx = _time(lambda: enc(x), a.steps, a.warmup)
        fwd_torch = _time(lambda: ref(x), a.steps, a.warmup)
    return {"arm": "trunk fwd+bwd", "heads": heads, "batch": a.batch, "layers": 3, "mapx_ms": ms_mapx,
            "torch_ms": ms_torch, "speedup": ms_torch / ms_mapx, "mapx_fwd_ms": fwd_mapx, "torch_fwd_ms": fwd_torch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--pt", nargs="+", default=["MFP", "RFD", "CTR"], choices=["MFP", "RFD", "CTR"])
    ap.add_argument("--dtype", nargs="+", default=["fp32"], choices=["fp32", "bf16"], help="compute_dtype of the step arms")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--vocab", type=int, default=V_AVAZU)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-trunk", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="only the --torch-trunk arms")
    a = ap.parse_args()
    from mapx.dataset import synth_table
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ids, labels, _, _ = synth_table(a.rows, F_AVAZU, a.vocab, seed=42)
    feat_count = torch.from_numpy(np.bincount(ids.reshape(-1), minlength=a.vocab).astype(np.float32))
    for heads in a.heads:
        if not a.no_steps:
            for pt in a.pt:
                for dtype in a.dtype:
                    print(json.dumps(step_arm(a, heads, pt, dtype, ids, labels, feat_count, device)), flush=True)
        if a.torch_trunk:
            print(json.dumps(trunk_arm(a, heads, feat_count, device)), flush=True)


if __name__ == "__main__":
    main()
