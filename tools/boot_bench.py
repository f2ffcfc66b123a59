#!/usr/bin/env python3
"""The bootstrap of the evaluation metrics (ops.bootstrap_metrics, csrc/bootstrap.hip) against the torch form of the
same computation on the same rows.

    python tools/boot_bench.py [--rows 819200] [--replicates 1000] [--torch_replicates 32] [--repeats 5]
                               [--out profiles/boot_bench.jsonl]

N = 819 200 seeded random logits and labels at a CTR of 0.17 (tools/slice_bench.py's rows), R = 1 000 replicates.  The
yardstick is what one would write with torch ops, run on the first 32 of the same replicates: the weights from
ops.bootstrap_weights, one sort of the probabilities' bits (shared by the replicates, as the kernel's is), the weights
gathered through the sort permutation, cumsum over the sorted rows, and the run formula at the last row of every tie
run; its integers are compared with the kernel's.  In this process alone: one warm-up call of each, then --repeats
rounds that alternate the two; each figure is a host clock around a call that ends in a device-to-host read of its
results, median and range, and is reported per replicate too.  From the shapes: the Philox draws per second of the
replicate kernel (N draws per four replicates) and the bytes per second it reads (17 bytes a row and quad: unit id,
flag, loss term) against the HBM peak of 8 TB/s -- an upper figure for the whole call, which also sorts.  A run that
finds no GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))

HBM_PEAK = 8.0e12
ROW_BYTES = 17
EPS = 2.220446049250313e-16


def torch_form(x, y, replicates, seed):
    """-> (u2, pos_w, neg_w int64 [R], sum_loss f64 [R]) with torch ops."""
    import torch
    from mapx import ops
    w = ops.bootstrap_weights(x.numel(), replicates, seed)
    p32, logits = torch.empty_like(x), torch.empty_like(x)       # the project's fp32 sigmoid, as a scoring step writes it
    ops.score_sink(x, x.numel(), torch.zeros(1, dtype=torch.int64, device=x.device), p32, logits)
    bits = p32.view(torch.int32)
    key, order = torch.sort(bits, stable=True)
    ys = y[order] > 0.5
    last = torch.ones_like(ys)
    last[:-1] = key[1:] != key[:-1]
    ends = last.nonzero().view(-1)
    p = p32[order].double()
    q = torch.where(ys, p, 1.0 - p).clamp(EPS, 1.0 - EPS)
    term = -torch.log(q)
    zero = torch.zeros(1, dtype=torch.int64, device=x.device)
    out = [[], [], [], []]
    for r in range(replicates):
        ws = w[r][order].to(torch.int64)
        pp = torch.cumsum(ws * ys, 0)[ends]
        nn = torch.cumsum(ws * ~ys, 0)[ends]
        pp0, nn0 = torch.cat([zero, pp[:-1]]), torch.cat([zero, nn[:-1]])
        out[0].append(((pp - pp0) * (nn0 + nn)).sum())
        out[1].append(pp[-1])
        out[2].append(nn[-1])
        out[3].append((ws.double() * term).sum())
    return tuple(torch.stack(v) for v in out)


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [t.cpu() for t in fn()]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", type=int, default=819200)
    p.add_argument("--replicates", type=int, default=1000)
    p.add_argument("--torch_replicates", type=int, default=32)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.repeats < 5:
        p.error("--repeats: at least 5")
    if not 1 <= args.torch_replicates <= args.replicates:
        p.error("--torch_replicates: between 1 and --replicates")
    import torch
    if not torch.cuda.is_available():
        sys.exit("boot_bench: no GPU; nothing is measured without one")
    from mapx import ops
    n, R, Rt = args.rows, args.replicates, args.torch_replicates
    rng = np.random.RandomState(42)
    x = torch.from_numpy((rng.randn(n) * 1.5 - 1.8).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.rand(n) < 0.17).astype(np.float32)).cuda()
    arms = {"bootstrap_metrics": lambda: ops.bootstrap_metrics(x, y, R, seed=args.seed),
            "torch_form": lambda: torch_form(x, y, Rt, args.seed)}
    first = {k: _clock(fn)[1] for k, fn in arms.items()}                         # warm-up (workspace, code objects)
    times = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():                                               # alternating
            times[k].append(_clock(fn)[0])
    ours, theirs = first["bootstrap_metrics"], first["torch_form"]
    m = ops.eval_metrics(x, y)
    auc = ours[0].double() * 0.5 / (ours[1].double() * ours[2].double())
    line = {"what": "bootstrap of AUC and log-loss", "rows": n, "replicates": R, "torch_replicates": Rt,
            "device": torch.cuda.get_device_name(0),
            "integers_agree": all(bool(torch.equal(a[:Rt], b)) for a, b in zip(ours[:3], theirs[:3])),
            "sum_loss_rel_diff": float(((ours[3][:Rt] - theirs[3]).abs() / theirs[3]).max()),
            "auc_point": m["auc"], "auc_boot_mean": float(auc.mean()), "auc_boot_std": float(auc.std())}
    for k, ts in times.items():
        reps = R if k == "bootstrap_metrics" else Rt
        med = statistics.median(ts)
        line[k] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts),
                   "seconds_per_replicate_median": med / reps, "seconds_per_replicate_min": min(ts) / reps,
                   "seconds_per_replicate_max": max(ts) / reps}
    quads = (R + 3) // 4
    med = line["bootstrap_metrics"]["seconds_median"]
    line["philox_draws_per_second"] = n * quads / med
    line["replicate_bytes_per_second"] = n * quads * ROW_BYTES / med
    line["share_of_hbm_peak"] = line["replicate_bytes_per_second"] / HBM_PEAK
    line["torch_over_kernel_per_replicate"] = (line["torch_form"]["seconds_per_replicate_median"]
                                               / line["bootstrap_metrics"]["seconds_per_replicate_median"])
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
