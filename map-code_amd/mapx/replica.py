"""Replica-consistency check: a device-side fingerprint of the whole training state.

mapx.parallel never broadcasts parameters: every rank applies the same merged gradients with the same deterministic
kernels and the replicas are taken to stay bit-identical (Trainer.eval's common branch, the all-rank flush, rank 0's
checkpoint all rely on it).  This module checks it: one read pass over the raw state per rank (ops.fingerprint, an
order-independent 64-bit integer sum per buffer), two small all-reduces, and an error on EVERY rank that names the
tensor and the row range when two replicas differ.  Nothing here flushes or writes state: lazy replay is closed-form
per gap, so a new flush point would change the trajectory bitwise.
"""
import os
from collections import OrderedDict

import torch
import torch.distributed as dist

from . import ops, parallel

MASK64 = 0xFFFFFFFFFFFFFFFF


class ReplicaDivergence(RuntimeError):
    """Two replicas hold different training state.  Raised on every rank (the verdict comes from reduced values).
    entry: the first differing entry of state_fingerprint; ranks: the ranks that differ from rank 0; chunk: the
    first differing chunk of that entry, as elements [elem_lo, elem_hi) and, for a table entry, rows
    [row_lo, row_hi) (None otherwise)."""

    def __init__(self, where, entry, ranks, chunk, elem_lo, elem_hi, row_lo=None, row_hi=None):
        self.where, self.entry, self.ranks, self.chunk = where, entry, list(ranks), chunk
        self.elem_lo, self.elem_hi, self.row_lo, self.row_hi = elem_lo, elem_hi, row_lo, row_hi
        rows = f", rows [{row_lo}, {row_hi})" if row_lo is not None else ""
        super().__init__(f"replicas diverged at {where}: entry '{entry}' differs from rank 0 on rank(s) {self.ranks}; "
                         f"first differing chunk {chunk} = elements [{elem_lo}, {elem_hi}){rows}")


def enabled():
    """MAPX_REPLICA_CHECK (default 1; 0 turns the Trainer's checks off).  Read at call time."""
    return os.environ.get("MAPX_REPLICA_CHECK", "1") != "0"


def _words(t):
    """`t` as a contiguous tensor of a 4-byte dtype whose words determine its values: fp32 / int32 as they are,
    fp64 as pairs of words, 2-byte floats widened to fp32 (exact)."""
    t = t.detach()
    if t.element_size() == 2:
        t = t.float()
    if not t.is_contiguous():
        t = t.contiguous()
    if t.element_size() == 8:
        t = t.view(torch.int32)
    return t


def state_entries(model, optimizer):
    """[(name, tensor, row_words)] of everything a replica must share, in an order that depends on the model alone:
    the dense flat groups (parameters, both moments), every row table's raw parameters, moments records and row
    clocks, the update counter, and any other floating-point parameter / buffer of the model.  row_words: words per
    table row (None for the rest).  Derived state — bf16 shadows, magnitude records, weight planes — is left out."""
    out, covered = [], set()
    for i, g in enumerate(optimizer.groups):
        for key in ("p", "m", "v"):
            out.append((f"dense{i}.{key}", g[key], None))
        covered.update(id(p) for p in g["params"])
    for t in optimizer.tables:
        tb, name = t.table, t.table.name
        out.append((f"{name}.p0", tb.p0.data, tb.p0.shape[1]))
        out.append((f"{name}.mv0", t.mv0, t.mv0.shape[1]))
        out.append((f"{name}.last", t.last, 1))
        covered.add(id(tb.p0))
        if tb.p1 is not None:
            out.append((f"{name}.p1", tb.p1.data, 1))
            out.append((f"{name}.mv1", t.mv1, 2))
            covered.add(id(tb.p1))
    out.append(("done", optimizer.done, None))
    tensors = dict(model.named_parameters(remove_duplicate=False))
    tensors.update(model.named_buffers(remove_duplicate=False))
    for name in model.state_dict().keys():
        v = tensors.get(name)
        if v is None or not v.is_floating_point() or id(v) in covered:
            continue
        out.append((name, v.data, None))
    return out


def _fingerprints(entries):
    """int64 device vector of the entries' fingerprints: one launch pair each, no host sync."""
    dev = entries[0][1].device
    totals = torch.empty(len(entries), dtype=torch.int64, device=dev)
    most = max(t.numel() * max(1, t.element_size() // 4) for _, t, _ in entries)
    scratch = torch.empty((most + ops.FP_CHUNK - 1) // ops.FP_CHUNK, dtype=torch.int64, device=dev)
    for i, (_, t, _) in enumerate(entries):
        ops.fingerprint_into(_words(t), totals[i:i + 1], scratch)       # (stream order: the scratch is free again)
    return totals


def state_fingerprint(model, optimizer):
    """Ordered mapping entry name -> fingerprint (int in [0, 2^64)) of the raw training state.  Reads only: no flush,
    stale lazy rows stay stale.  One host sync."""
    entries = state_entries(model, optimizer)
    vals = _fingerprints(entries).tolist()
    return OrderedDict((name, v & MASK64) for (name, _, _), v in zip(entries, vals))


def _all_reduce(t, op):
    s = parallel._staged(t)
    dist.all_reduce(s, op=op)
    return s.cpu()


def check_replicas(model, optimizer, where):
    """Raise ReplicaDivergence on every rank unless all ranks hold bit-identical training state.  Nothing happens on
    a single rank.  Cost when the replicas agree: one read pass over the state, a MIN and a MAX all-reduce of one
    int64 per entry."""
    if parallel.world() <= 1:
        return
    entries = state_entries(model, optimizer)
    fp = _fingerprints(entries)
    lo, hi = _all_reduce(fp.clone(), dist.ReduceOp.MIN), _all_reduce(fp.clone(), dist.ReduceOp.MAX)
    differ = (lo != hi).nonzero()
    if differ.numel() == 0:
        return
    # every rank sees the same lo / hi, so every rank picks the same entry and joins the same gather
    name, t, row_words = entries[int(differ[0])]
    w = _words(t)
    total = torch.empty(1, dtype=torch.int64, device=w.device)
    chunks = ops.fingerprint_into(w, total)
    mine = parallel._staged(torch.cat([total, chunks]))
    everyone = torch.empty(parallel.world() * mine.numel(), dtype=torch.int64, device=mine.device)
    dist.all_gather_into_tensor(everyone, mine)
    everyone = everyone.view(parallel.world(), -1).cpu()
    ranks = [r for r in range(1, parallel.world()) if int(everyone[r, 0]) != int(everyone[0, 0])]
    off = (everyone[:, 1:] != everyone[0:1, 1:]).any(0).nonzero()
    chunk = int(off[0]) if off.numel() else 0
    elem_lo, elem_hi = chunk * ops.FP_CHUNK, min((chunk + 1) * ops.FP_CHUNK, w.numel())
    row_lo = row_hi = None
    if row_words:
        row_lo, row_hi = elem_lo // row_words, (elem_hi + row_words - 1) // row_words
    raise ReplicaDivergence(where, name, ranks, chunk, elem_lo, elem_hi, row_lo, row_hi)
