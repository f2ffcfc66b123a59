#!/usr/bin/env python3
"""Sliced evaluation (ops.slice_metrics, csrc/slice_metrics.hip) against the global metric (ops.eval_metrics,
csrc/metrics.hip) on the same rows.

    python tools/slice_bench.py [--rows 819200] [--repeats 5] [--out profiles/slice_bench.jsonl]

N = 819 200 rows (tools/score_bench.py's size), seeded random logits and labels at a CTR of 0.17, and three group
columns: G = 24 uniform (an hour-of-day column: every chunk of 256 sorted rows lies inside one group), G = 10^4
uniform, G = 10^6 with Zipf-distributed sizes (exponent 1.2: one group holds a large share of the rows, most groups are
empty or hold a row or two).  In this process alone: one warm-up call of each, then --repeats rounds that alternate
slice_metrics and eval_metrics; each figure is a host clock around a call that ends in its own device-to-host read
(slice_metrics: the two status words; eval_metrics: its six doubles), median and range.  eval_metrics is the yardstick:
the expectation is the cost of sorting 64-bit keys over 31 + bit_length(G - 1) bits where it sorts 30-bit ones, plus
the zeroing of 5 G outputs and one launch.  A run that finds no GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))


def columns(n, rng):
    yield "G=24 uniform", rng.randint(0, 24, n).astype(np.int32), 24
    yield "G=1e4 uniform", rng.randint(0, 10 ** 4, n).astype(np.int32), 10 ** 4
    yield "G=1e6 zipf(1.2)", np.minimum(rng.zipf(1.2, n) - 1, 10 ** 6 - 1).astype(np.int32), 10 ** 6


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", type=int, default=819200)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.repeats < 5:
        p.error("--repeats: at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("slice_bench: no GPU; nothing is measured without one")
    from mapx import ops
    n = args.rows
    rng = np.random.RandomState(42)
    x = torch.from_numpy((rng.randn(n) * 1.5 - 1.8).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.rand(n) < 0.17).astype(np.float32)).cuda()
    lines = []
    for name, g_np, G in columns(n, rng):
        g = torch.from_numpy(g_np).cuda()
        arms = {"slice_metrics": lambda: ops.slice_metrics(x, y, g, G), "eval_metrics": lambda: ops.eval_metrics(x, y)}
        first = {k: fn() for k, fn in arms.items()}                             # warm-up (workspace, code objects)
        times = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():                                           # alternating
                times[k].append(_clock(fn)[0])
        rows, pos, u2, _, sl = (t.cpu().numpy() for t in first["slice_metrics"])
        line = {"what": name, "rows": n, "groups": G, "non_empty": int((rows > 0).sum()), "largest": int(rows.max()),
                "device": torch.cuda.get_device_name(0),
                "positives_agree": int(pos.sum()) == first["eval_metrics"]["positives"],
                "logloss_rel_diff": abs(float(sl.sum()) / n / first["eval_metrics"]["logloss"] - 1.0)}
        for k, ts in times.items():
            line[k] = {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}
        line["ratio_of_medians"] = line["slice_metrics"]["seconds_median"] / line["eval_metrics"]["seconds_median"]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()
