#!/usr/bin/env python3
"""Times of growing a vocabulary and of moving a table to the grown id space (mapx/vocab.py Vocabulary.grow,
mapx/grow.py migrate_table over csrc/vocab_grow.hip).

    python tools/grow_bench.py --part migrate [--vocab 9449445] [--width 16] [--fields 24] [--growth 0.01] [--out FILE.jsonl]
    python tools/grow_bench.py --part grow [--rows 2000000] [--n_core 2] [--out FILE.jsonl]

One process per run, one warm-up, --rounds (5) alternating rounds of the forms compared, median (min-max).

migrate  a table of --vocab rows x --width floats, --fields fields sized by mapx.dataset.field_sizes, every field
         grown by --growth of its keys.  mapx_table_migrate (device events) against the torch form a user would write,
         old.index_select(0, src_rows) with src_rows built on the device from the same plan (its build is timed apart).
         Both must agree bit for bit.  Byte model (kept here): V_new x W x 4 bytes read and as many written; the torch
         form reads 8 more per row for its index.  bytes/s = those bytes over the median time, also as a share of the
         HBM peak.
grow     a synthetic Avazu-shaped file of --rows lines (tools/preprocess_bench.py's generator, seed 7) is fitted into a
         dataset directory; a second file of the same shape from another pool of lines (seed 8) is then (a) grown on:
         mapx.vocab.grow_dataset_from_text, with the phases read_columns / Vocabulary.from_meta / grow / encode / write
         timed apart by a host clock that ends in a device synchronise, and (b) refitted from scratch:
         generate_dataset_from_text.  A run that finds no GPU fails."""
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


def _stat(times):
    return {"median_ms": statistics.median(times) * 1e3, "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3}


def _event_time(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def source_rows_on_device(plan, device):
    """The torch form's index: src_rows [V_new] from the plan's per-field arrays, with torch ops on the device."""
    import torch
    par = torch.from_numpy(plan.arrays()).to(device)
    n_old, added, base_old, base_new = par[0], par[1], par[2], par[3]
    rows = torch.arange(plan.V_new, device=device)
    f = (torch.searchsorted(base_new, rows, right=True) - 1).clamp_(min=0)
    rank = rows - base_new[f]
    src = base_old[f] + torch.minimum(rank, n_old[f])
    return torch.where(rows < plan.reserved, rows, src)


def bench_migrate(args):
    import torch
    from mapx import grow
    from mapx.dataset import field_sizes
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in field_sizes(args.fields, args.vocab)]
    fields, b_old, b_new = [], 10, 10
    for j, size in enumerate(sizes):
        n, a = size - 1, int((size - 1) * args.growth)
        fields.append(grow.FieldPlan(f"f{j}", n, a, b_old, b_new))
        b_old, b_new = b_old + n + 1, b_new + n + a + 1
    plan = grow.Plan(fields, b_old, b_new, 10)
    W = args.width
    src = torch.randn(plan.V_old, W, device=dev)
    out = torch.empty(plan.V_new, W, device=dev)
    t_build, rows = _event_time(lambda: source_rows_on_device(plan, dev))
    t_build, rows = _event_time(lambda: source_rows_on_device(plan, dev))
    from mapx.native import check, lib, stream
    par = torch.from_numpy(plan.arrays()).to(dev)                  # (the launch alone: the plan's arrays are resident)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def kernel():
        check(lib.mapx_table_migrate(src.data_ptr(), W, plan.V_old, out.data_ptr(), W, plan.V_new, W, len(fields),
                                     par[0].data_ptr(), par[1].data_ptr(), par[2].data_ptr(), par[3].data_ptr(), None,
                                     W, 0, err.data_ptr(), stream()))
        return out
    assert torch.equal(grow.migrate_table(src, plan).view(torch.int32), kernel().view(torch.int32)) and int(err) == 0
    torch_form = lambda: src.index_select(0, rows)
    assert torch.equal(kernel().view(torch.int32), torch_form().view(torch.int32))
    tk, tt = [], []
    for _ in range(args.rounds):
        tk.append(_event_time(kernel)[0])
        tt.append(_event_time(torch_form)[0])
    moved = 2 * plan.V_new * W * 4
    res = {"part": "migrate", "V_old": plan.V_old, "V_new": plan.V_new, "width": W, "fields": args.fields,
           "added": plan.added_total, "rounds": args.rounds, "kernel": _stat(tk), "index_select": _stat(tt),
           "index_build_ms": t_build * 1e3, "bytes_kernel": moved, "bytes_index_select": moved + 8 * plan.V_new}
    for k, nbytes in (("kernel", moved), ("index_select", moved + 8 * plan.V_new)):
        rate = nbytes / (res[k]["median_ms"] * 1e-3)
        res[k].update(bytes_per_s=rate, hbm_share=rate / HBM_PEAK)
    res["kernel_over_index_select"] = res["kernel"]["median_ms"] / res["index_select"]["median_ms"]
    return res


def bench_grow(args):
    import torch
    import preprocess_bench as pb
    from mapx import rawtext, vocab
    dev = torch.device("cuda", 0)
    schema = rawtext.SCHEMAS["avazu"]
    sync = lambda: torch.cuda.synchronize(dev)
    with tempfile.TemporaryDirectory() as tmp:
        day1, day2 = os.path.join(tmp, "day1.csv"), os.path.join(tmp, "day2.csv")
        pb.write_file(day1, "avazu", args.rows, 7)
        pb.write_file(day2, "avazu", args.rows, 8)
        a_dir = os.path.join(tmp, "A")
        vocab.generate_dataset_from_text(day1, schema, args.n_core, a_dir, "avazu", device=dev)
        meta_a = os.path.join(a_dir, "avazu-meta.json")

        def grown():
            clock, t = time.perf_counter, {}
            t0 = clock()
            with open(meta_a) as f:
                saved = json.load(f)
            voc = vocab.Vocabulary.from_meta(saved, schema, device=dev)
            sync(); t1 = clock()
            labels, columns, _d, _s = rawtext.read_columns(day2, schema, device=dev)
            sync(); t2 = clock()
            g, added, before, after = voc.grow(columns, args.n_core)
            sync(); t3 = clock()
            ids, oov_rows, types = g.encode(columns, type_ids=True)
            sync(); t4 = clock()
            t.update(load_vocab_s=t1 - t0, read_columns_s=t2 - t1, grow_s=t3 - t2, encode_s=t4 - t3,
                     added=sum(added), oov_before=sum(before), oov_after=sum(after), V_old=voc.input_size,
                     V_new=g.input_size)
            return t

        def end_to_end():
            t0 = time.perf_counter()
            vocab.grow_dataset_from_text(day2, schema, meta_a, args.n_core, os.path.join(tmp, "B"), "avazu", device=dev)
            sync()
            return time.perf_counter() - t0

        def refit():
            t0 = time.perf_counter()
            vocab.generate_dataset_from_text(day2, schema, args.n_core, os.path.join(tmp, "C"), "avazu", device=dev)
            sync()
            return time.perf_counter() - t0
        grown(), end_to_end(), refit()                                  # the warm-up
        phases, te, tr = [], [], []
        for _ in range(args.rounds):
            phases.append(grown())
            te.append(end_to_end())
            tr.append(refit())
        res = {"part": "grow", "rows": args.rows, "n_core": args.n_core, "rounds": args.rounds,
               "file_bytes": os.path.getsize(day2), "grow_dataset_from_text": _stat(te),
               "generate_dataset_from_text": _stat(tr)}
        for k in ("load_vocab_s", "read_columns_s", "grow_s", "encode_s"):
            res[k.replace("_s", "")] = _stat([p[k] for p in phases])
        res.update({k: phases[0][k] for k in ("added", "oov_before", "oov_after", "V_old", "V_new")})
        res["grow_over_refit"] = res["grow_dataset_from_text"]["median_ms"] / res["generate_dataset_from_text"]["median_ms"]
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--part", choices=("migrate", "grow"), required=True)
    p.add_argument("--vocab", type=int, default=9_449_445)
    p.add_argument("--width", type=int, default=16)
    p.add_argument("--fields", type=int, default=24)
    p.add_argument("--growth", type=float, default=0.01)
    p.add_argument("--rows", type=int, default=2_000_000)
    p.add_argument("--n_core", type=int, default=2)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=None, help="append the JSON line to this file")
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/grow_bench.py measures on an MI355X only")
    res = bench_migrate(args) if args.part == "migrate" else bench_grow(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
