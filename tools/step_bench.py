"""Step time of the OTHER BASELINE configs on one GPU (no bench line: the headline metric is bench.py's MFP step):
configs[3] DCNv2 + RFD (Unigram replacement) and configs[4] DCNv2 finetune (CTR), Avazu / Criteo shapes, batch 4096,
the Trainer's own captured step.
    python tools/step_bench.py --pt RFD|CTR|MFP [--workload avazu|criteo] [--dtype f32|bf16] [--steps 200]
                               [--sampling randint|normal]
--sampling: the pretraining steps' mask draw (--sampling_method of run.py): randint = with replacement (the run
scripts' and bench.py's), normal = L distinct fields per row (run.py's default)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts map-code_amd on the path)


def build(args, device):
    """bench.build's configuration, table and Trainer with the model from models.build_backbone, which also builds the
    modes BaseModel.from_config still refuses (xDeepFM with --dtype bf16)."""
    import numpy as np
    from mapx.arguments import Config, TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    wl = bench.WORKLOADS[args.workload]
    F, V = wl["F"], wl["V"]
    ids, labels, _, _ = synth_table(args.rows, F, V, seed=42, uniform=args.uniform)
    feat_count = torch.from_numpy(np.bincount(ids.reshape(-1), minlength=V).astype(np.float32))
    pt = args.pt
    cfg = Config(model_name=args.model, data_dir=None, input_size=V, num_fields=F, embed_size=16,
                 embed_dropout_rate=0.0, embed_norm=False, hidden_size=1000, num_hidden_layers=3,
                 hidden_act="relu", hidden_dropout_rate=0.0, num_cross_layers=3, pt_neg_num=25,
                 proj_size=32, pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt, RFD_replace="Unigram",
                 feat_count=feat_count, seed=42, rank=0, compute_dtype="bf16" if args.dtype == "bf16" else "fp32",
                 cin_layer_units="50,50", use_lr=False, num_attn_layers=2, attn_size=40, num_attn_heads=1,
                 attn_probs_dropout_rate=0.0, res_conn=False, attn_scale=False, dnn_size=1000, num_dnn_layers=0,
                 dnn_act="relu", dnn_drop=0.0)
    torch.manual_seed(42)
    model = build_backbone(cfg)
    steps_per_epoch = max(1, args.rows // args.batch)
    need = 2 * (args.preroll + args.warmup + args.steps + 64)
    targs = TrainingArguments(output_dir="/tmp/mapx_bench", per_gpu_train_batch_size=args.batch,
                              per_gpu_eval_batch_size=args.batch, learning_rate=1e-3, lr_sched="cosine",
                              weight_decay=5e-2, num_train_epochs=max(3, -(-need // steps_per_epoch)),
                              pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt, sampling_method="randint",
                              mask_ratio=0.3, seed=42)
    targs._device = device
    return Trainer(model, cfg, targs, OurDataset(ids, labels), OurDataset(ids[:args.batch], labels[:args.batch]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pt", default="RFD", choices=["MFP", "RFD", "CTR"])
    ap.add_argument("--model", default="DCNv2", choices=["DCNv2", "DNN", "DeepFM", "xDeepFM", "AutoInt"])
    ap.add_argument("--workload", default="avazu", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--sampling", default="randint", choices=["randint", "normal"])
    ap.add_argument("--tensors", action="store_true", help="deal the batches as tensors (A/B of the row references)")
    a = ap.parse_args()
    a.uniform = False
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tr = build(a, device)
    tr.args.sampling_method = a.sampling
    train = tr._begin("bench")
    gen = tr._generator()
    kind = a.pt.lower()
    rows = not a.tensors                       # as the Trainer's loops deal them: row references into the split
    state = {"it": train.batches(a.batch, True, gen, (0, 1), rows=rows)}

    def next_batch():
        try:
            return next(state["it"])
        except StopIteration:
            state["it"] = train.batches(a.batch, True, gen, (0, 1), rows=rows)
            return next(state["it"])

    tr.model.train()
    for _ in range(a.preroll + a.warmup):
        tr.run_step(kind, *next_batch())
    live = [g for g in tr._graphs.values() if not isinstance(g, int)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.run_step(kind, *next_batch())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"step": f"{a.model} {a.pt}", "workload": a.workload, "dtype": a.dtype, "batch": a.batch,
                      "sampling": a.sampling, "ms_per_step": 1e3 * dt / a.steps, "samples_per_s": a.batch * a.steps / dt,
                      "graphed": bool(tr.use_graph and live), "loss": float(out[0].detach())}))


if __name__ == "__main__":
    main()
