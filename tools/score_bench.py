#!/usr/bin/env python3
"""Rows per second of scoring (mapx/score.py) against the Trainer.eval loop, and the two scoring kernels against
their byte model.

    python tools/score_bench.py [--batches 200] [--batch 4096] [--repeats 5] [--raw_rows 2000000] [--out FILE.jsonl]

Avazu-shaped synthetic ids (mapx.dataset.synth_table, F = 23, V = 9 449 445), the flagship DCNv2 of bench.py in
finetune configuration with seeded random weights, --batches x --batch rows resident on the device.  Per compute
dtype (fp32, bf16) three arms score the same rows and end with ops.eval_metrics over all logits:
  eval     Trainer.eval(test_eval=True) behind an optimizer: one eager forward per batch, the parent's only way;
  eager    Scorer with MAPX_GRAPH=0: block -> forward -> sink -> advance, launched from Python;
  graph    Scorer: the same step replayed from one hipGraph.
In this process alone, one warm-up pass per arm, then --repeats rounds that alternate the arms; the figure is the
median of a host clock around work that ends in a device synchronise.  The arms' logits are compared (eager == graph
bit for bit; eval within the fp32 / bf16 bound of the tests).
Kernels: 100 launches of mapx_score_block / mapx_score_sink captured in one graph each (no launch gaps), device events
around a replay, median of --repeats.  Byte model (kept here): block B F 16 + B, sink B 12.
Raw file: score_raw_file once on a synthetic Avazu file of --raw_rows lines (tools/preprocess_bench.write_file; the
vocabulary fitted on the same file at n_core 2): seconds of the host read, the host-to-device copies, the parse, the
encode, the scoring steps and the results' way to the host.  A run that finds no GPU fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12           # bytes/s, the MI355X's specified HBM3E bandwidth
F, V = 23, 9449445


def config(dtype, input_size=V, num_fields=F):
    from mapx.arguments import Config
    return Config(model_name="DCNv2", data_dir=None, input_size=input_size, num_fields=num_fields, embed_size=16,
                  embed_dropout_rate=0.0, embed_norm=False, layer_norm_eps=1e-12, hidden_size=1000, num_hidden_layers=3,
                  hidden_act="relu", hidden_dropout_rate=0.0, num_cross_layers=3, pt_neg_num=25, proj_size=32,
                  pretrain=False, pt_type="MFP", RFD_replace="Unigram", feat_count=None, seed=42, rank=0,
                  compute_dtype=dtype, device=None, n_gpu=1, idx_low=None, idx_high=None, feat_num_per_field=None)


def model_of(cfg):
    import torch
    from mapx.models import build_backbone
    torch.manual_seed(42)
    return build_backbone(cfg).to("cuda")


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def arms_of(dtype, ids, labels, batch):
    """-> {arm: callable -> logits [N] on the device}"""
    import torch
    from mapx import score
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.trainer import Trainer
    cfg = config(dtype)
    targs = TrainingArguments(output_dir=tempfile.gettempdir(), per_gpu_train_batch_size=batch,
                              per_gpu_eval_batch_size=batch, learning_rate=1e-3, weight_decay=5e-2)
    targs._device = torch.device("cuda", 0)
    ds = OurDataset(ids.cpu().numpy(), labels.cpu().numpy())
    tr = Trainer(model_of(cfg), cfg, targs, ds, ds)
    tr.optimizer = tr.scheduler = tr.get_optimizer(1, 0)
    kept = {}

    def eval_arm():                                         # (the split is resident after the warm-up pass)
        log = tr.eval(ds, test_eval=True)
        return {"auc": log["eval_auc"], "logloss": log["eval_loss"]}

    def eval_logits():                                      # what eval() threw away, once, for the comparison
        tr.model.eval()
        with torch.no_grad():
            return torch.cat([tr.model(input_ids=X, labels=Y)[1].view(-1) for X, Y in tr._split(ds).batches(batch, False)])
    kept["eval_logits"] = eval_logits
    arms = {"eval": eval_arm}
    for name, env in (("eager", "0"), ("graph", "1")):
        os.environ["MAPX_GRAPH"] = env
        sc = score.Scorer(model_of(cfg), batch, "cuda")
        os.environ.pop("MAPX_GRAPH")

        def arm(sc=sc, name=name):
            s, m = sc.score(ids, labels)
            kept[name] = s.logits
            return m
        arms[name] = arm
    return arms, kept


def kernel_times(batch, repeats):
    import torch
    from mapx import ops
    dev = "cuda"
    ids = torch.randint(0, V, (64 * batch, F), dtype=torch.int64, device=dev)
    oov_id = torch.randint(0, V, (F,), dtype=torch.int64, device=dev)
    out = torch.empty(batch, F, dtype=torch.int64, device=dev)
    oov = torch.empty(64 * batch, dtype=torch.uint8, device=dev)
    logits = torch.randn(batch, device=dev)
    probs, lout = torch.empty(64 * batch, device=dev), torch.empty(64 * batch, device=dev)
    cursor, done = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    res = {}
    for name, fn, nbytes in (("score_block", lambda: ops.score_block(ids, 64 * batch, cursor, oov_id, out, oov),
                              batch * F * 16 + batch),
                             ("score_sink", lambda: ops.score_sink(logits, 64 * batch, cursor, probs, lout), batch * 12)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for k in range(100):
                fn()
        g.replay()
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e-3 / 100)
        med = statistics.median(times)
        res[name] = {"seconds_median": med, "seconds_all": times, "model_bytes": nbytes, "bytes_per_s": nbytes / med,
                     "share_of_hbm_peak": nbytes / med / HBM_PEAK, "launches_per_replay": 100}
    return res


def raw_file_run(rows, batch):
    import torch
    from mapx import rawtext, score, vocab
    from preprocess_bench import write_file
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "day.csv")
        nbytes = write_file(path, "avazu", rows, 7)
        vocab.generate_dataset_from_text(path, rawtext.AVAZU, 2, d, "avazu")
        voc = vocab.Vocabulary.from_meta(os.path.join(d, "avazu-meta.json"), rawtext.AVAZU)
        sc = score.Scorer(model_of(config("fp32", voc.input_size, len(voc.fields))), batch, "cuda",
                          oov_id=[f.oov for f in voc.fields])
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()                # (the fit above held the whole file's columns)
        timing = {}
        seconds, res = _clock(lambda: score.score_raw_file(sc, path, rawtext.AVAZU, voc, chunk_bytes=64 << 20, timing=timing))
        return {"rows": res["info"]["rows"], "file_bytes": nbytes, "seconds": seconds, "rows_per_s": rows / seconds,
                "graph": res["info"]["graph"], **{k: round(v, 4) for k, v in timing.items()},
                "peak_device_bytes": torch.cuda.max_memory_allocated()}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--batches", type=int, default=200)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--raw_rows", type=int, default=2_000_000)
    p.add_argument("--dtypes", default="fp32,bf16")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.repeats < 5 or args.batches < 200:
        p.error("--repeats: at least 5; --batches: at least 200")
    import torch
    if not torch.cuda.is_available():
        sys.exit("score_bench: no GPU; nothing is measured without one")
    from mapx.dataset import synth_table
    N = args.batches * args.batch
    ids_np, labels_np, _, _ = synth_table(N, F, V, seed=42)
    ids, labels = torch.from_numpy(ids_np).cuda(), torch.from_numpy(labels_np).cuda()
    lines = []
    for dtype in args.dtypes.split(","):
        arms, kept = arms_of(dtype, ids, labels, args.batch)
        metrics = {name: fn() for name, fn in arms.items()}                     # the warm-up pass (and the capture)
        times = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():                                        # alternating
                times[name].append(_clock(fn)[0])
        kept["eval"] = kept.pop("eval_logits")()
        scale = float(kept["eval"].abs().max())
        line = {"what": "rows_per_s", "dtype": dtype, "rows": N, "batch": args.batch, "device": torch.cuda.get_device_name(0),
                "eager_equals_graph": bool(torch.equal(kept["eager"], kept["graph"])),
                "eval_vs_graph_of_scale": float((kept["eval"] - kept["graph"]).abs().max()) / scale,
                "auc": {k: m["auc"] for k, m in metrics.items()}}
        for name, ts in times.items():
            med = statistics.median(ts)
            line[name] = {"seconds_median": med, "seconds_all": ts, "rows_per_s": N / med}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del arms, kept
        torch.cuda.empty_cache()
    lines.append({"what": "kernels", "batch": args.batch, "fields": F, **kernel_times(args.batch, args.repeats)})
    print(json.dumps(lines[-1]), flush=True)
    if args.raw_rows > 0:
        torch.cuda.reset_peak_memory_stats()
        lines.append({"what": "raw_file", "batch": args.batch, **raw_file_run(args.raw_rows, args.batch)})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
