"""Step time of the FiGNN backbone (model_name=fignn) on one GPU: Avazu-shaped synthetic data, batch 4096, F = 23,
E = 16, three graph layers; MFP, RFD and finetune (CTR) steps through Trainer.run_step (the captured step replayed
after the first few).  One JSON line per arm.
--torch-trunk adds forward + backward of the trunk alone (embeddings [B,23,16] -> the state [B,23,16]): the mapx
graph / layer / GRU kernels against the reference's own torch ops (broadcast matmul, bmm, nn.GRUCell, masked softmax) on
the same GPU with the same fp32 weights.  The two are timed in alternating rounds of the same run; every round's time
is printed, so the run-to-run spread can be read next to the difference.
    python tools/fignn_bench.py [--pt MFP RFD CTR] [--steps 100] [--torch-trunk] [--no-steps] [--res-conn] [--reuse]"""
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


def make_config(a, pt, feat_count):
    from mapx.arguments import Config
    return Config(model_name="fignn", data_dir=None, input_size=a.vocab, num_fields=a.fields, embed_size=a.embed,
                  embed_dropout_rate=0.0, embed_norm=False, hidden_size=a.embed, num_hidden_layers=a.layers,
                  hidden_act="relu", hidden_dropout_rate=0.0, num_cross_layers=0, pt_neg_num=25, proj_size=32,
                  res_conn=a.res_conn, reuse_graph_layer=a.reuse, pretrain=pt != "CTR",
                  pt_type="MFP" if pt == "CTR" else pt, RFD_replace="Unigram", feat_count=feat_count, seed=42, rank=0,
                  compute_dtype="fp32")


def step_arm(a, pt, ids, labels, feat_count, device):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    torch.manual_seed(42)
    cfg = make_config(a, pt, feat_count)
    model = build_backbone(cfg)
    targs = TrainingArguments(output_dir="/tmp/mapx_fignn_bench", per_gpu_train_batch_size=a.batch,
                              per_gpu_eval_batch_size=a.batch, learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2,
                              num_train_epochs=1000, pretrain=pt != "CTR", pt_type="MFP" if pt == "CTR" else pt,
                              RFD_replace="Unigram", sampling_method="randint", mask_ratio=0.3, seed=42)
    targs._device = device
    tr = Trainer(model, cfg, targs, OurDataset(ids, labels), OurDataset(ids[:a.batch], labels[:a.batch]))
    train = tr._begin("fignn_bench")
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
    rounds = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = tr.run_step(kind, *next_batch())
        torch.cuda.synchronize()
        rounds.append(1e3 * (time.perf_counter() - t0) / a.steps)
    live = [g for g in tr._graphs.values() if not isinstance(g, int)]
    ms = float(np.median(rounds))
    return {"arm": f"fignn {pt}", "batch": a.batch, "fields": a.fields, "embed": a.embed, "layers": a.layers,
            "ms_per_step": ms, "rounds_ms": [round(r, 4) for r in rounds], "samples_per_s": a.batch / ms * 1e3,
            "graphed": bool(live), "loss": float(out[0].detach())}


class TorchTrunk(torch.nn.Module):
    """The same trunk on torch's own ops (the reference's FiGNNBlock.forward), with the mapx block's weights."""

    def __init__(self, block):
        super().__init__()
        self.block = block
        E = block.embedding_dim
        self.gru = torch.nn.GRUCell(E, E)
        self.gru.load_state_dict(block.gru.state_dict())
        self.register_buffer("eye", torch.eye(block.num_fields).bool())

    def forward(self, x):
        b = self.block
        E = b.embedding_dim
        w = b.W_attn.weight
        pre = (x @ w[0, :E]).unsqueeze(2) + (x @ w[0, E:]).unsqueeze(1)
        g = torch.softmax(torch.nn.functional.leaky_relu(pre, 0.01).masked_fill(self.eye, float("-inf")), dim=-1)
        h = x
        for l in range(b.gnn_layers):
            gl = b.gnn if b.reuse_graph_layer else b.gnn[l]
            h_out = torch.matmul(gl.W_out, h.unsqueeze(-1)).squeeze(-1)
            a = torch.matmul(gl.W_in, torch.bmm(g, h_out).unsqueeze(-1)).squeeze(-1) + gl.bias_p
            h = self.gru(a.reshape(-1, E), h.reshape(-1, E)).view(-1, b.num_fields, E)
            if b.use_residual:
                h = h + x
        return h


def _round(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def trunk_arm(a, feat_count, device):
    from mapx.models import build_backbone
    torch.manual_seed(42)
    model = build_backbone(make_config(a, "CTR", feat_count)).to(device).train()
    block = model.fignn
    ref = TorchTrunk(block).to(device).train()
    x = (torch.randn(a.batch, a.fields, a.embed, device=device) * 0.3).requires_grad_(True)
    g = torch.randn(a.batch, a.fields, a.embed, device=device)
    err = float((block(x) - ref(x)).detach().abs().max())

    def run(m):
        def fn():
            m(x).backward(g)
        return fn

    def fwd(m):
        def fn():
            with torch.no_grad():
                m(x)
        return fn
    arms = {"mapx_ms": run(block), "torch_ms": run(ref), "mapx_fwd_ms": fwd(block), "torch_fwd_ms": fwd(ref)}
    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):                     # alternating: every arm once per round
        for k, fn in arms.items():
            rounds[k].append(_round(fn, a.steps))
    out = {"arm": "fignn trunk fwd+bwd", "batch": a.batch, "fields": a.fields, "embed": a.embed, "layers": a.layers,
           "res_conn": a.res_conn, "reuse_graph_layer": a.reuse, "max_abs_diff": err}
    for k, v in rounds.items():
        out[k] = float(np.median(v))
        out[k.replace("_ms", "_rounds_ms")] = [round(r, 4) for r in v]
    out["speedup"] = out["torch_ms"] / out["mapx_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pt", nargs="+", default=["MFP", "RFD", "CTR"], choices=["MFP", "RFD", "CTR"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--vocab", type=int, default=V_AVAZU)
    ap.add_argument("--fields", type=int, default=F_AVAZU)
    ap.add_argument("--embed", type=int, default=16)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--res-conn", action="store_true")
    ap.add_argument("--reuse", action="store_true", help="reuse_graph_layer")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds of --steps each (the median is reported)")
    ap.add_argument("--torch-trunk", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="only the --torch-trunk arm")
    a = ap.parse_args()
    from mapx.dataset import synth_table
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ids, labels, _, _ = synth_table(a.rows, a.fields, a.vocab, seed=42)
    feat_count = torch.from_numpy(np.bincount(ids.reshape(-1), minlength=a.vocab).astype(np.float32))
    if not a.no_steps:
        for pt in a.pt:
            print(json.dumps(step_arm(a, pt, ids, labels, feat_count, device)), flush=True)
    if a.torch_trunk:
        print(json.dumps(trunk_arm(a, feat_count, device)), flush=True)


if __name__ == "__main__":
    main()
