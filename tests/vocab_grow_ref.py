"""Growing a saved vocabulary and moving tables to the grown id space, restated with a Counter and numpy (a helper,
not a test): what mapx.vocab.Vocabulary.grow, mapx.grow.plan's source rows and mapx_table_migrate must give.  It shares
no code with the product.

    grow(feat_map, columns, decode, n_core) -> (grown feat_map, {field: keys added})
        feat_map  {key string: id}: ten reserved tokens, then per field f'{name}-{value as printed}' in id order and
                  f'{name}-<oov>'
        columns   ordered {field name: int64 array [N]} of raw codes;  decode {field name: code -> value as printed}
        Per field: the values whose key the map lacks, Counter(misses).most_common() (descending count, ties by first
        occurrence), those seen >= n_core times appended behind the field's old keys, then <oov>; ids consecutive.
    fit(columns, decode, n_core) = grow of the map that holds the reserved tokens and every field's <oov> only.
    oov_cells(feat_map, columns, decode) -> cells whose key the map lacks.
    src_rows(plan) -> int64 [V_new]: the old row every new row reads (added rows and the new <oov>: the old <oov>).
    migrate(table, plan, fresh=None) -> [V_new, W]; fresh [sum added, W]: the added rows in id order instead.
        plan: anything with .fields (each .n_old .added .base_old .base_new), .V_old, .V_new.
    halves / decoders / half_case / FIGURES: the committed raw files cut in halves, shared by the host and GPU tests.
"""
import os
from collections import Counter

import numpy as np

import rawtext_ref

RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}

RESERVED = ("<pad>", "<cls>", "<sep>", "<mask>", "<unused0>", "<unused1>", "<unused2>", "<unused3>", "<unused4>",
            "<unused5>")


def _field_keys(feat_map, name):
    oov = f"{name}-<oov>"
    keys = [k for k in feat_map if k.startswith(name + "-") and k != oov]
    return keys, oov


def grow(feat_map, columns, decode, n_core):
    grown = {k: i for i, k in enumerate(list(feat_map)[:len(RESERVED)])}
    added = {}
    for name, col in columns.items():
        printed = decode[name]
        old_keys, oov = _field_keys(feat_map, name)
        misses = [k for k in (f"{name}-{printed(v)}" for v in np.asarray(col).tolist()) if k not in feat_map]
        new_keys = [k for k, c in Counter(misses).most_common() if c >= n_core]
        for k in old_keys + new_keys:
            grown[k] = len(grown)
        grown[oov] = len(grown)
        added[name] = len(new_keys)
    return grown, added


def fit(columns, decode, n_core):
    empty = {k: i for i, k in enumerate(RESERVED)}
    for name in columns:
        empty[f"{name}-<oov>"] = len(empty)
    return grow(empty, columns, decode, n_core)[0]


def oov_cells(feat_map, columns, decode):
    return sum(1 for name, col in columns.items() for v in np.asarray(col).tolist()
               if f"{name}-{decode[name](v)}" not in feat_map)


def src_rows(plan):
    src = np.full(plan.V_new, -1, dtype=np.int64)
    first = plan.fields[0].base_new
    src[:first] = np.arange(first)
    for f in plan.fields:
        for rank in range(f.n_old + f.added + 1):
            src[f.base_new + rank] = f.base_old + min(rank, f.n_old)
    assert (src >= 0).all() and (src < plan.V_old).all()
    return src


def migrate(table, plan, fresh=None):
    table = np.asarray(table)
    out = table[src_rows(plan)].copy()
    if fresh is not None:
        j = 0
        for f in plan.fields:
            for rank in range(f.n_old, f.n_old + f.added):
                out[f.base_new + rank] = np.asarray(fresh)[j]
                j += 1
        assert j == len(fresh)
    return out


# ---------------------------------------------------------------- the committed raw files cut in halves
def halves(golden_dir, name, schema):
    """The file cut at the middle one of its physical lines below the header, as tests/test_vocab_apply_gpu.py cuts it."""
    with open(os.path.join(golden_dir, RAW[name]), "rb") as f:
        lines = f.read().split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    head, lines = (lines[:1], lines[1:]) if schema.header else ([], lines)
    mid = len(lines) // 2
    return b"\n".join(head + lines[:mid]) + b"\n", b"\n".join(head + lines[mid:]) + b"\n"


def decoders(schema):
    return {n: (rawtext_ref.decode_hex if k == rawtext_ref.HEX else (lambda v: str(int(v))))
            for n, k in zip(schema.columns, schema.column_kinds) if n != schema.label}


# fields that grow, keys added at n_core 2, <oov> cells of the second half before -> after; keys added at n_core 1
FIGURES = {"avazu": (25, 11, 55, 254, 105, 160), "criteo": (39, 30, 168, 821, 350, 518)}
_HALF = {}


def half_case(golden_dir, name, schema):
    """schema: the file's mapx.rawtext.Schema (its description of the columns; nothing of it computes here).
    -> (schema, first half bytes, second half bytes, columns of the first, of the second, decoders, feat_map fitted on
    the first half with n_core 2) — parsed and fitted once per session, by the restatements alone."""
    if name not in _HALF:
        first, second = halves(golden_dir, name, schema)
        (_, c1), (_, c2) = rawtext_ref.parse(first, schema), rawtext_ref.parse(second, schema)
        dec = decoders(schema)
        _HALF[name] = (schema, first, second, c1, c2, dec, fit(c1, dec, 2))
    return _HALF[name]
