#!/usr/bin/env python3
"""Time of applying a saved vocabulary (mapx/vocab.py Vocabulary over csrc/vocab_apply.hip) on Avazu-shaped columns.

    python tools/vocab_apply_bench.py [--rows 40000000] [--fields 24] [--vocab 9449445] [--repeats 5] [--out FILE.json]
    python tools/vocab_apply_bench.py --tables none|hot|cold        (what the lookups cost: see below)

Columns: --fields int64 columns of --rows values drawn on the device, field cardinalities from
mapx.dataset.field_sizes(fields, vocab), ranks by a power-law draw, every rank printed as an 8-digit hash code.  The
vocabulary is fitted on them at n_core 2 by the existing builder (mapx.vocab.build_vocab); a second, independent draw
of the same shape is the file that is encoded.  Timed with device events, median of --repeats launches after a
warm-up, in this process alone (the fit: a host clock that ends in a device synchronise, the same warm-up and repeats):
  fit         mapx.vocab.build_vocab on the first draw: count, rank and translate all fields, feat_map names included;
  load        mapx_vocab_apply_load (clear + insert of all kept keys);
  apply/0     mapx_vocab_apply, ids through LDS and stored along the rows, without and with type_ids;
  apply/1     the same with one strided 8-byte store per row and field.
Byte model (kept here): per value 8 B of column read, 8 B of feat_ids written (+ 8 B of type_ids), and one random
12-byte probe (8 B key + 4 B rank; a hit reads both, a miss the key only — counted as 12); the load writes 12 B per
slot and reads 8 B per key.  bytes/s = those bytes over the median time, also as a share of the HBM peak.  The modes
must agree bit for bit.  A run that finds no GPU fails.

--tables replaces fit and draw by uniform random columns over tables built directly: `none` no keys at all (every
value <oov> without a probe: the column read, the LDS tile and the stores alone), `hot` 1 000 keys per field and every
value a hit (slices that stay in the caches), `cold` 4 M keys per field drawn uniformly (nearly every probe misses)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))
HBM_PEAK = 8.0e12           # bytes/s, the MI355X's specified HBM3E bandwidth


def draw_columns(rows, sizes, seed, device="cuda"):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    cols = {}
    for f, size in enumerate(sizes):
        rank = (torch.rand(rows, generator=g, device=device, dtype=torch.float64) ** 6 * int(size)).long()
        rank.clamp_(max=int(size) - 1)
        cols[f"f{f}"] = (((rank * 2654435761 + f) & 0xFFFFFFFF) << 4) | 8       # the code of an 8-digit hash string
    return cols


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


def _host_clock(fn, repeats, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def _rate(nbytes, times):
    med = statistics.median(times)
    return {"seconds_median": med, "seconds_all": times, "model_bytes": int(nbytes), "bytes_per_s": nbytes / med,
            "share_of_hbm_peak": nbytes / med / HBM_PEAK}


def direct_tables(args, N, F):
    import torch
    from mapx import vocab
    from mapx.native import check, lib, ptr, stream
    n = {"none": 0, "hot": 1000, "cold": 4_000_000}[args.tables]
    g = torch.Generator(device="cuda").manual_seed(3)
    fields, cols, base = [], [], 10
    for f in range(F):
        fields.append(vocab.FieldKeys(f"f{f}", np.arange(n, dtype=np.int64) * 7 + f, base))
        base = fields[-1].oov + 1
        cols.append(torch.randint(0, n if n else 1 << 40, (N,), generator=g, device="cuda", dtype=torch.int64) * 7 + f)
    voc = vocab.Vocabulary(fields)
    par = voc._par
    col_ptrs = torch.tensor([c.data_ptr() for c in cols], dtype=torch.int64).cuda()
    ids = torch.empty(N, F, dtype=torch.int64, device="cuda")
    stat = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    res = {"rows": N, "fields": F, "tables": args.tables, "keys": voc.n_keys_total, "slots": voc.n_slots}
    for mode in (0, 1):
        def apply():
            check(lib.mapx_vocab_apply(ptr(col_ptrs), N, F, ptr(voc._tkey), ptr(voc._trank), ptr(par[1]), voc.n_slots,
                                       ptr(par[2]), ptr(par[3]), ptr(par[4]), ptr(par[5]), 0, ptr(ids), F, None, F,
                                       ptr(stat), stat.data_ptr() + 8 * F, mode, stream()))
        res[f"apply_mode{mode}"] = _rate(N * F * (8 + 8 + (12 if n else 0)), _events(apply, args.repeats))
        res[f"oov_share_mode{mode}"] = sum(stat.cpu()[:F].tolist()) / max(N * F, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", type=int, default=40_000_000)
    p.add_argument("--fields", type=int, default=24)
    p.add_argument("--vocab", type=int, default=9_449_445)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--tables", choices=("none", "hot", "cold"), default=None)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.repeats < 5:
        p.error("--repeats: at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("vocab_apply_bench: no GPU; nothing is measured without one")
    from mapx import dataset, vocab
    from mapx.native import check, lib, ptr, stream
    N, F = args.rows, args.fields
    if args.tables:
        return direct_tables(args, N, F)
    sizes = dataset.field_sizes(F, args.vocab)
    fit_cols = draw_columns(N, sizes, seed=1)
    last = {}

    def fit():
        last["fit"] = vocab.build_vocab(fit_cols, 2)
    fit_times = _host_clock(fit, args.repeats)
    feat_ids, fitted, _, input_size = last.pop("fit")
    print(f"fitted {F} fields of {N} rows at n_core 2 in {statistics.median(fit_times):.2f} s: input_size "
          f"{input_size}", file=sys.stderr, flush=True)
    fields = [vocab.FieldKeys(fv.name, fv.keys.cpu().numpy(), fv.base) for fv in fitted]
    del feat_ids, fitted, fit_cols
    torch.cuda.empty_cache()
    voc = vocab.Vocabulary(fields, flags=[1] * F, field_types=[1] * F, missing_type=2)
    cols = list(draw_columns(N, sizes, seed=2).values())
    res = {"rows": N, "fields": F, "keys": voc.n_keys_total, "slots": voc.n_slots, "input_size": input_size,
           "device": torch.cuda.get_device_name(0),
           "fit": {"seconds_median": statistics.median(fit_times), "seconds_all": fit_times}}
    par, err = voc._par, torch.empty(2, dtype=torch.int32, device="cuda")

    def load():
        check(lib.mapx_vocab_apply_load(ptr(voc._keys), ptr(par[0]), ptr(par[1]), F, voc.n_keys_total, voc.n_slots,
                                        ptr(voc._tkey), ptr(voc._trank), ptr(err), stream()))
    res["load"] = _rate(12 * voc.n_slots + 8 * voc.n_keys_total + 12 * voc.n_keys_total, _events(load, args.repeats))
    assert err.tolist()[0] == 0
    col_ptrs = torch.tensor([c.data_ptr() for c in cols], dtype=torch.int64).cuda()
    ids = torch.empty(N, F, dtype=torch.int64, device="cuda")
    types = torch.empty(N, F, dtype=torch.int64, device="cuda")
    stat = torch.empty(F + 1, dtype=torch.int64, device="cuda")

    def apply(mode, with_types):
        check(lib.mapx_vocab_apply(ptr(col_ptrs), N, F, ptr(voc._tkey), ptr(voc._trank), ptr(par[1]), voc.n_slots,
                                   ptr(par[2]), ptr(par[3]), ptr(par[4]), ptr(par[5]), voc.missing_type, ptr(ids), F,
                                   ptr(types) if with_types else None, F, ptr(stat), stat.data_ptr() + 8 * F, mode,
                                   stream()))
    kept = {}
    for with_types in (False, True):
        for mode in (0, 1):
            t = _events(lambda: apply(mode, with_types), args.repeats)
            host = stat.cpu()
            assert host[F:].view(torch.int32).tolist()[0] == 0
            kept[mode] = (ids.clone(), types.clone() if with_types else None, host[:F].tolist())
            res[f"apply_mode{mode}" + ("_types" if with_types else "")] = _rate(N * F * (8 + 8 + 12 + 8 * with_types), t)
        assert torch.equal(kept[0][0], kept[1][0]) and kept[0][2] == kept[1][2]
        if with_types:
            assert torch.equal(kept[0][1], kept[1][1])
        res["oov_share"] = sum(kept[0][2]) / max(N * F, 1)
        kept.clear()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
