"""The Poisson bootstrap of ops.bootstrap_metrics restated with numpy (a plain helper module, no fixtures).

philox4x32_10 is the standard Philox4x32-10 (Random123), vectorised over counters; weights() is the weight rule of
include/mapx_hip.h (mapx_bootstrap_metrics); reference() ranks given fp32 probabilities (a test passes the device's own),
takes per tie run the weighted positives and negatives with bincount and counts u2 in integers, the loss in float64
with sklearn's clip, eps = 2^-52."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
NAMES = ("u2", "pos_w", "neg_w", "sum_loss")
T = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291,
     4294609777, 4294923276, 4294962463, 4294966817, 4294967252, 4294967292)
COUNTER_HI = 0x424F4F54 << 32
ONE_BITS = 0x3F800000
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, counter):
    """key: (k0, k1) Python ints; counter: four arrays (or ints) of 32-bit words -> four uint32 arrays."""
    k0, k1 = (np.uint64(k & 0xFFFFFFFF) for k in key)
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & M32 for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def weight_of(words):
    words = np.asarray(words, dtype=np.uint32)
    return sum((words >= np.uint32(t)).astype(np.uint8) for t in T)


def weights(units, replicates, seed):
    """units: int64 [n] (or a row count: every row its own unit) -> uint8 [replicates, n]."""
    u = (np.arange(units, dtype=np.int64) if np.isscalar(units) else np.asarray(units, dtype=np.int64)).view(np.uint64)
    out = np.empty((replicates, len(u)), dtype=np.uint8)
    for q in range((replicates + 3) // 4):
        hi = COUNTER_HI | q
        words = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (u & M32, u >> np.uint64(32), hi & 0xFFFFFFFF, hi >> 32))
        for e in range(min(4, replicates - 4 * q)):
            out[4 * q + e] = weight_of(words[e])
    return out


def segment_rows(n):
    """csrc/bootstrap.hip: boot_segment_rows / boot_segments, the nominal rows of a segment and their number."""
    return max(384, -(-(-(-n // 256)) // 64) * 64)


def segments(n):
    return -(-n // segment_rows(n))


def reference(p32, labels, w):
    """p32: float32 [n] probabilities (a NaN ranks as 1); w: [R, n] integer weights -> dict of the four arrays
    (u2, pos_w, neg_w uint64; sum_loss float64), R each."""
    bits = np.minimum(np.asarray(p32, dtype=np.float32).view(np.uint32), np.uint32(ONE_BITS))
    y = np.asarray(labels) > 0.5
    p = bits.view(np.float32).astype(np.float64)
    term = -np.log(np.clip(np.where(y, p, 1.0 - p), EPS, 1.0 - EPS))
    uniq, inv = np.unique(bits, return_inverse=True)
    R = len(w)
    out = dict(u2=np.zeros(R, np.uint64), pos_w=np.zeros(R, np.uint64), neg_w=np.zeros(R, np.uint64),
               sum_loss=np.zeros(R, np.float64))
    for r in range(R):
        wr = np.asarray(w[r]).astype(np.int64)
        pos = np.bincount(inv[y], weights=wr[y], minlength=len(uniq)).astype(np.int64)      # (exact: below 2^53)
        neg = np.bincount(inv[~y], weights=wr[~y], minlength=len(uniq)).astype(np.int64)
        before = np.cumsum(neg) - neg
        out["u2"][r] = sum(int(a) * (2 * int(b) + int(c)) for a, b, c in zip(pos[pos > 0], before[pos > 0], neg[pos > 0]))
        out["pos_w"][r], out["neg_w"][r] = int(pos.sum()), int(neg.sum())
        out["sum_loss"][r] = float((wr.astype(np.float64) * term).sum())
    return out


def auc_of(a):
    """The four arrays -> float64 [R] AUCs (NaN where a class has no weight)."""
    pw, nw = a["pos_w"].astype(np.float64), a["neg_w"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((pw > 0) & (nw > 0), a["u2"].astype(np.float64) * 0.5 / (pw * nw), np.nan)
