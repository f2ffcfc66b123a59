#!/usr/bin/env python3
"""Throughput of the raw-text reader (mapx/rawtext.py over csrc/rawtext.hip) on a seeded synthetic file.

    python tools/preprocess_bench.py --dataset criteo|avazu --rows 4000000 [--repeats 5] [--pandas] [--out FILE.json]
    python tools/preprocess_bench.py --dataset criteo --rows 4000000 --kernels_only      (under a kernel trace)

The file: --rows lines drawn (seeded) from a pool of 50 000 distinct seeded lines of the dataset's shape, LF only,
written to a temporary directory.  Timed, after a warm-up, with device events over --repeats launches each:
  index      the three line-index launches on one resident chunk (the first --chunk_mb of the file);
  parse/0    the parse launch, every wave staging its lines in LDS when they fit;
  parse/1    the parse launch, every wave reading global memory;
and with a host clock around work that ends in a device synchronise:
  read_columns end to end, with the host read, the host-to-device copies and the device work listed separately;
  pandas.read_csv of the same file with the reference's arguments (--pandas; "not measured" otherwise or when
  pandas is not importable).
Kernel times proper come from a kernel trace of a --kernels_only run (warm-up + --repeats launches, nothing else).

Byte model (kept here): the index pass reads n bytes twice (count, fill) and writes 8 bytes per line; the parse pass
reads n bytes and writes 8 x columns x lines bytes.  bytes/s = those bytes over the measured time, given as a share of
the HBM peak.  A measurement path that finds no GPU fails."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))
HBM_PEAK = 8.0e12           # bytes/s, the MI355X's specified HBM3E bandwidth
POOL = 50_000


def _hex8(rng, n, vocab):
    return np.array([format(int(v), "08x") for v in (rng.randint(0, 1 << 32, n, dtype=np.int64) % vocab * 1000003 % (1 << 32))])


def pool_lines(dataset, seed):
    rng = np.random.RandomState(seed)
    n = POOL
    if dataset == "criteo":
        cells = [(rng.rand(n) < 0.25).astype(np.int64).astype(str)]
        for j in range(13):
            v = np.minimum(rng.pareto(0.7, n) * 4, 2e9).astype(np.int64)
            cells.append(np.where(rng.rand(n) < 0.15, "", v.astype(str)))
        for j in range(26):
            cells.append(np.where(rng.rand(n) < 0.1, "", _hex8(rng, n, [50, 5000, 1 << 22, 1 << 32][j % 4])))
        sep = "\t"
    else:
        cells = [(rng.randint(10 ** 18, 9 * 10 ** 18, n, dtype=np.int64)).astype(str),
                 (rng.rand(n) < 0.17).astype(np.int64).astype(str),
                 np.array(["1410%02d%02d" % (d, h) for d, h in zip(rng.randint(21, 31, n), rng.randint(0, 24, n))]),
                 rng.choice([1005, 1002, 1010], n).astype(str), rng.randint(0, 8, n).astype(str)]
        cells += [_hex8(rng, n, [30, 3000, 1 << 20][j % 3]) for j in range(9)]
        cells += [rng.randint(0, 6, n).astype(str), rng.randint(0, 6, n).astype(str)]
        cells += [rng.randint(lo, hi, n).astype(str) for lo, hi in ((375, 24052), (120, 1024), (20, 1024), (112, 2758),
                                                                   (0, 4), (33, 1959))]
        cells += [np.where(rng.rand(n) < 0.4, "-1", rng.randint(100000, 100250, n).astype(str)), rng.randint(1, 255, n).astype(str)]
        sep = ","
    return [sep.join(row).encode() for row in zip(*cells)]


def write_file(path, dataset, rows, seed):
    from mapx import rawtext
    pool = pool_lines(dataset, seed)
    rng = np.random.RandomState(seed + 1)
    with open(path, "wb") as f:
        if rawtext.SCHEMAS[dataset].header:
            f.write(",".join(rawtext.SCHEMAS[dataset].source_names).encode() + b"\n")
        for lo in range(0, rows, 500_000):
            idx = rng.randint(0, POOL, min(500_000, rows - lo))
            f.write(b"\n".join(pool[i] for i in idx.tolist()) + b"\n")
    return os.path.getsize(path)


def _events(fn, repeats, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return times


def _rate(nbytes, seconds):
    bps = nbytes / seconds
    return {"seconds_min": seconds, "bytes": int(nbytes), "bytes_per_s": bps, "share_of_hbm_peak": bps / HBM_PEAK}


def kernel_timings(path, schema, chunk_bytes, repeats):
    import torch
    from mapx import rawtext
    from mapx.native import check, lib, ptr, stream
    with open(path, "rb") as f:
        data, _ = next(rawtext.iter_chunks(f, chunk_bytes))
    n = len(data)
    n16 = (n + 15) // 16 * 16
    buf = torch.zeros(n16, dtype=torch.uint8, device="cuda")
    buf[:n].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    ls, ln, n_lines, _ = rawtext.index_lines(buf, n, n // schema.min_line_bytes + 1)
    ws = torch.empty(lib.mapx_rawtext_index_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    ls2, ln2 = torch.empty_like(ls), torch.empty_like(ln)

    def index():
        check(lib.mapx_rawtext_index(ptr(buf), n, ptr(ws), ws.numel(), ptr(ls2), ptr(ln2), n_lines, ptr(counts), stream()))
    first = 1 if schema.header else 0
    ls, ln = ls[first:], ln[first:]
    rows = n_lines - first
    out = torch.empty(len(schema.columns), rows, dtype=torch.int64, device="cuda")
    err = torch.empty(1, dtype=torch.int64, device="cuda")
    thr = rawtext._thresholds_on(buf.device)
    s = schema.struct()
    import ctypes as C

    def parse(mode):
        check(lib.mapx_rawtext_parse(ptr(buf), n, ls.data_ptr(), ln.data_ptr(), rows, C.addressof(s), ptr(thr), thr.numel(),
                                     ptr(out), rows, 0, len(schema.columns), ptr(err), mode, stream()))
    res = {"chunk_bytes": n, "chunk_lines": rows, "columns": len(schema.columns),
           "mean_line_bytes": n / max(n_lines, 1)}
    t = _events(index, repeats)
    res["index"] = dict(_rate(2 * n + 8 * n_lines, min(t)), seconds_all=t)
    kept = {}
    for mode in (0, 1):
        t = _events(lambda: parse(mode), repeats)
        assert int(err.item()) == -1, "the synthetic file must parse"
        kept[mode] = out.clone()
        res[f"parse_mode{mode}"] = dict(_rate(n + 8 * len(schema.columns) * rows, min(t)), seconds_all=t)
    assert torch.equal(kept[0], kept[1])
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--dataset", choices=("criteo", "avazu"), default="criteo")
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--chunk_mb", type=int, default=256)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--pandas", action="store_true", help="also time pandas.read_csv with the reference's arguments")
    p.add_argument("--kernels_only", action="store_true", help="warm-up + repeats of the kernels and nothing else")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.repeats < 5:
        p.error("--repeats: at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("preprocess_bench: no GPU; nothing is measured without one")
    from mapx import rawtext
    schema = rawtext.SCHEMAS[args.dataset]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "train.txt")
        t0 = time.perf_counter()
        size = write_file(path, args.dataset, args.rows, args.seed)
        res = {"dataset": args.dataset, "rows": args.rows, "file_bytes": size, "write_seconds": time.perf_counter() - t0,
               "device": torch.cuda.get_device_name(0)}
        res["kernels"] = kernel_timings(path, schema, args.chunk_mb << 20, args.repeats)
        if not args.kernels_only:
            e2e = []
            for mode in (0, 1):
                for rep in range(3):
                    timing = {}
                    t0 = time.perf_counter()
                    labels, cols, _, _ = rawtext.read_columns(path, schema, chunk_bytes=args.chunk_mb << 20, mode=mode,
                                                              timing=timing)
                    torch.cuda.synchronize()
                    total = time.perf_counter() - t0
                    assert labels.numel() == args.rows
                    e2e.append(dict(mode=mode, rep=rep, seconds=total, file_bytes_per_s=size / total, **timing))
                    del labels, cols
            res["read_columns"] = e2e
            res["pandas_read_csv"] = "not measured"
            if args.pandas:
                try:
                    import pandas as pd
                except ImportError:
                    res["pandas_read_csv"] = "not measured: pandas is not importable here"
                else:
                    t0 = time.perf_counter()
                    if args.dataset == "criteo":       # proc_criteo.py:53
                        df = pd.read_csv(path, sep="\t", header=None, names=schema.source_names, encoding="utf-8", dtype=object)
                    else:                              # proc_avazu.py:38 reads one column per pass; one pass over all here
                        df = pd.read_csv(path, sep=",")
                    res["pandas_read_csv"] = {"seconds": time.perf_counter() - t0, "rows": len(df),
                                              "note": "the parse alone: no bucketing, no date parts, no copy to the device"}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
