"""The reference's translation line (data_preprocess/proc_avazu.py:252-257, proc_criteo.py:155-160) restated with a
Python dict (a helper, not a test): what mapx.vocab.Vocabulary.encode must give for a saved feat_map.  It shares no
code with the product.

    apply(feat_map, columns, decode) -> int64 [N, F]
        feat_map  {key string: id}, keys f'{name}-{value as printed}' and f'{name}-<oov>'
        columns   ordered {field name: int64 array [N]} of raw codes
        decode    {field name: code -> the value as printed}
"""
import numpy as np


def apply(feat_map, columns, decode):
    names = list(columns)
    n = len(next(iter(columns.values()))) if names else 0
    rows = np.empty((n, len(names)), dtype=np.int64)
    for j, name in enumerate(names):
        printed = decode[name]
        oov = feat_map[f"{name}-<oov>"]
        for i, v in enumerate(np.asarray(columns[name]).tolist()):
            key = f"{name}-{printed(v)}"
            rows[i, j] = feat_map[key] if key in feat_map else oov
    return rows


def outcomes(feat_map, columns, decode):
    """-> (hits, <oov> rows, number of fields in which both occur), from the restatement alone."""
    rows = apply(feat_map, columns, decode)
    is_oov = np.stack([rows[:, j] == feat_map[f"{name}-<oov>"] for j, name in enumerate(columns)], axis=1) \
        if len(columns) else np.zeros((0, 0), dtype=bool)
    both = int(sum(1 for j in range(is_oov.shape[1]) if is_oov[:, j].any() and (~is_oov[:, j]).any()))
    return int((~is_oov).sum()), int(is_oov.sum()), both
