"""numpy restatement of the state fingerprint (include/mapx_hip.h: mapx_fingerprint_words).  Unsigned 64-bit
arithmetic that wraps:

    G = 0x9E3779B97F4A7C15
    mix(x):  x += G;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^ x >> 31
    c_k = sum_j mix(j << 32 | w[k * 65536 + j])        (j: index inside chunk k; the last chunk may be short)
    F   = sum_k mix(c_k + (k + 1) * G)                 (0 for an empty buffer)
"""
import numpy as np

CHUNK = 65536
G = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def mix(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + G
        x = (x ^ (x >> np.uint64(30))) * M1
        x = (x ^ (x >> np.uint64(27))) * M2
        return x ^ (x >> np.uint64(31))


def words_of(a):
    """The raw 32-bit words of an array of a 4-byte dtype."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.reshape(-1).view(np.uint32)


def chunk_values(words):
    """uint64 [ceil(n / CHUNK)]."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1)
    out = np.zeros((w.size + CHUNK - 1) // CHUNK, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(out.size):
            part = w[k * CHUNK:(k + 1) * CHUNK].astype(np.uint64)
            j = np.arange(part.size, dtype=np.uint64)
            out[k] = mix((j << np.uint64(32)) | part).sum(dtype=np.uint64)
    return out


def fold(chunks):
    c = np.asarray(chunks, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k1 = np.arange(1, c.size + 1, dtype=np.uint64)
        return int(mix(c + k1 * G).sum(dtype=np.uint64)) if c.size else 0


def fingerprint(words):
    """-> (F as a Python int, chunk values uint64)."""
    c = chunk_values(words)
    return fold(c), c
