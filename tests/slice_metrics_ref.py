"""ops.slice_metrics restated with numpy and Python integers (a plain helper module, no fixtures).

p32 = torch.sigmoid on fp32 on the CPU; per group, 2U is counted in Python integers over (bits of p32, label) — a
positive above a negative counts 2, a tie 1 — and the probability and log-loss sums are float64 with sklearn's clip to
[eps, 1 - eps], eps = 2^-52.  A test that relies on p32 asserts first that the device sigmoid gives the same bits on its
logits (the probabilities a scoring step writes)."""
import numpy as np
import torch

EPS = float(np.finfo(np.float64).eps)
NAMES = ("rows", "positives", "u2", "sum_prob", "sum_loss")
BLOCK = 4096


def p32_of(logits):
    """torch.sigmoid on fp32 on the CPU, as a function of each value alone.  On a plain vector it is not: the last
    elements, short of two SIMD vectors, go through a scalar loop whose exp differs in the last bit on some values, so
    the same logit can give two results depending on the length of the vector it sits in.  Here every element is
    evaluated inside the vector loop: blocks of a fixed length, zero-padded."""
    x = np.ascontiguousarray(logits, dtype=np.float32).ravel()
    out = np.empty_like(x)
    buf = torch.zeros(BLOCK + 64, dtype=torch.float32)
    for s in range(0, len(x), BLOCK):
        part = x[s:s + BLOCK]
        buf[:len(part)] = torch.from_numpy(part)
        out[s:s + len(part)] = torch.sigmoid(buf)[:len(part)].numpy()
    return out


def u2_of(bits, y):
    """Twice the U statistic of one group, a Python integer."""
    uniq, inv = np.unique(bits, return_inverse=True)
    pos = np.bincount(inv[y], minlength=len(uniq))
    neg = np.bincount(inv[~y], minlength=len(uniq))
    total, before = 0, 0
    for p, q in zip(pos.tolist(), neg.tolist()):
        total += p * (2 * before + q)              # = p * (negatives before the run + negatives through it)
        before += q
    return total


def reference(logits, labels, groups, n_groups, p32=None):
    """-> dict of the five arrays (rows, positives int64; u2 uint64; sum_prob, sum_loss float64), n_groups each."""
    p32 = p32_of(logits) if p32 is None else np.asarray(p32, dtype=np.float32)
    y = np.asarray(labels) > 0.5
    g = np.asarray(groups).astype(np.int64)
    bits = p32.view(np.uint32)
    p = p32.astype(np.float64)
    loss = -np.log(np.clip(np.where(y, p, 1.0 - p), EPS, 1.0 - EPS))
    out = dict(rows=np.zeros(n_groups, np.int64), positives=np.zeros(n_groups, np.int64),
               u2=np.zeros(n_groups, np.uint64), sum_prob=np.zeros(n_groups, np.float64),
               sum_loss=np.zeros(n_groups, np.float64))
    order = np.argsort(g, kind="stable")
    ids, starts = np.unique(g[order], return_index=True)
    for k, s, e in zip(ids.tolist(), starts.tolist(), starts.tolist()[1:] + [len(g)]):
        idx = order[s:e]
        out["rows"][k] = e - s
        out["positives"][k] = int(y[idx].sum())
        out["u2"][k] = u2_of(bits[idx], y[idx])
        out["sum_prob"][k] = p[idx].sum()
        out["sum_loss"][k] = loss[idx].sum()
    return out
