"""Cost of a full replica.state_fingerprint pass at the Avazu MFP state sizes: buffers of the real
shapes filled with random words — two row tables (embedding [V, 16], NCE table [V, 32] + bias) with their moments
records and row clocks, the dense flat groups — fingerprinted the way mapx.replica does it (one launch pair per
entry, one host sync).  Warm, median of --reps host-clock windows that end in the sync; also the largest entry alone
by device events.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-code_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9449445)          # Avazu vocabulary
    ap.add_argument("--embed", type=int, default=16)
    ap.add_argument("--proj", type=int, default=32)
    ap.add_argument("--dense", type=int, default=3_900_000, help="words of dense parameters (both groups together)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from mapx import ops, replica
    dev = torch.device("cuda", 0)

    def words(*shape):
        return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev)
    V, E, P = a.rows, a.embed, a.proj
    entries = [(f"dense0.{k}", words(a.dense), None) for k in "pmv"]
    entries += [("embed.embedding.p0", words(V, E), E), ("embed.embedding.mv0", words(V, 2 * E), 2 * E),
                ("embed.embedding.last", words(V), 1),
                ("mfp_criterion.p0", words(V, P), P), ("mfp_criterion.mv0", words(V, 2 * P), 2 * P),
                ("mfp_criterion.last", words(V), 1), ("mfp_criterion.p1", words(V, 1), 1),
                ("mfp_criterion.mv1", words(V, 2), 2), ("done", words(1), None)]
    nbytes = sum(4 * t.numel() for _, t, _ in entries)

    def one_pass():
        return replica._fingerprints(entries).tolist()
    first = one_pass()
    for _ in range(a.warmup):
        assert one_pass() == first
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        one_pass()
        times.append(time.perf_counter() - t0)
    big = max(entries, key=lambda e: e[1].numel())[1]
    total = torch.empty(1, dtype=torch.int64, device=dev)
    chunks = torch.empty((big.numel() + ops.FP_CHUNK - 1) // ops.FP_CHUNK, dtype=torch.int64, device=dev)
    ev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.fingerprint_into(big, total, chunks)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    one = statistics.median(x.elapsed_time(y) for x, y in ev) * 1e-3
    med = statistics.median(times)
    print(json.dumps(dict(what="state_fingerprint, Avazu MFP state sizes, one GPU", entries=len(entries), bytes=nbytes,
                          pass_ms=round(1e3 * med, 4), pass_ms_min=round(1e3 * min(times), 4),
                          pass_ms_max=round(1e3 * max(times), 4), pass_TBps=round(nbytes / med / 1e12, 3),
                          largest_entry_bytes=4 * big.numel(), largest_entry_ms=round(1e3 * one, 4),
                          largest_entry_TBps=round(4 * big.numel() / one / 1e12, 3), reps=a.reps)))


if __name__ == "__main__":
    main()
