"""Vocabulary builder on the GPU: the per-field id assignment of the reference's offline
preprocessing, data_preprocess/proc_avazu.py:213-262 and proc_criteo.py:109-163, for datasets whose raw
columns are resident on the device.

    feat_map: <pad> <cls> <sep> <mask> <unused0..5> = ids 0..9 (proc_avazu.py:213-220), then field by field
    the values seen at least n_core times in Counter.most_common() order — descending count, ties in order of
    first occurrence — and one <oov> id per field (proc_avazu.py:247-250); every row's value is translated
    through it (:252-257).  The resulting matrix is `feat_ids` of the HDF5 file that code/dataset.py:20-40 reads.

Counting / ranking are kernels of csrc/vocab.hip behind include/mapx_hip.h (mapx_vocab_*); the two stable sorts of a
field's distinct values are the segment plans' radix sort (mapx_seg_plan); the rows are translated, and given their
type_ids, through the vocabulary just fitted by the lookup kernel of csrc/vocab_apply.hip (below).  Raw values
are 64-bit integers: the hexadecimal hash strings of Avazu / Criteo parse to them exactly (`encode_column`),
anything else is coded by first occurrence on the host.  There is no CPU path.

A fitted vocabulary can be applied to other rows (a later day's log, a held-out file, a test file): `parse_meta`
reads the `feat_map` of a `<name>-meta.json` back into per-field key arrays (pure host), `Vocabulary` holds them as
lookup tables on the device and `encode` translates all fields of a file in one launch — the reference's own line
`feat_map[key] if key in feat_map else feat_map[f'{name}-<oov>']` (proc_avazu.py:252-257) against a map saved
earlier (csrc/vocab_apply.hip, mapx_vocab_apply*).  `encode_dataset_from_text` is the raw-file form."""
import json
import os

import numpy as np
import torch

from . import ops
from .native import MapxError, RT_MAX_FIELDS, check, lib, ptr, require_gpu, stream

RESERVED = ("<pad>", "<cls>", "<sep>", "<mask>", "<unused0>", "<unused1>", "<unused2>", "<unused3>", "<unused4>",
            "<unused5>")                                  # proc_avazu.py:213-220: ids 0..9


_HEX = __import__("re").compile(r"[0-9a-f]*")


def encode_column(values):
    """A raw column -> (int64 codes, decode) with decode(code) = the value as the reference's f-string prints
    it (proc_avazu.py:249: f'{name}-{k}').  Integer columns are their own codes; columns of hexadecimal
    strings (the 8-digit hashes of Avazu / Criteo) parse exactly; anything else is numbered by first occurrence."""
    a = np.asarray(values)
    if a.dtype.kind in "iu":
        return a.astype(np.int64), (lambda c: str(int(c)))
    if a.dtype.kind in "USO":
        strs = [str(x) for x in a.tolist()]
        # fixed-width lower-case hexadecimal — EVERY string matches [0-9a-f]{w} (int(s, 16) alone also takes '1A',
        # ' 1f', '1_0', '+1f', which would merge values the reference's Counter keeps apart): code <-> string is a bijection
        w = len(strs[0]) if strs else 0
        if 0 < w <= 15 and all(len(s) == w for s in strs) and _HEX.fullmatch("".join(strs)) is not None:
            codes = np.array([int(s, 16) for s in strs], dtype=np.int64)
            return codes, (lambda c, w=w: format(int(c), f"0{w}x"))
        first = {}
        codes = np.fromiter((first.setdefault(s, len(first)) for s in strs), dtype=np.int64, count=len(strs))
        names = list(first)
        return codes, (lambda c: names[int(c)])
    raise TypeError(f"encode_column: dtype {a.dtype} (integers or strings)")


class FieldVocab:
    """Result for one field: `keys` [n_kept] the kept raw values in id order, `counts` their frequencies,
    `base` the id of the first of them, `oov` = base + n_kept."""

    def __init__(self, name, keys, counts, base, n_distinct):
        self.name, self.keys, self.counts, self.base = name, keys, counts, int(base)
        self.n_kept, self.n_distinct = int(keys.shape[0]), int(n_distinct)
        self.oov = self.base + self.n_kept

    @property
    def size(self):
        return self.n_kept + 1


def fit_field(keys, n_core, base, name="", capacity=None):
    """The vocabulary of one field: count, compact, rank (two stable sorts), n-core cut.  keys int64 [N] on the
    device.  -> FieldVocab (device tensors).  No row is translated here."""
    require_gpu(keys)
    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous():
        raise TypeError("fit_field: keys must be a contiguous int64 vector")
    N, dev = keys.numel(), keys.device
    if N == 0:
        return FieldVocab(name, torch.empty(0, dtype=torch.int64, device=dev),
                          torch.empty(0, dtype=torch.int32, device=dev), base, 0)
    cap = capacity or max(64, 1 << int(np.ceil(np.log2(2 * N + 1))))
    i32 = dict(dtype=torch.int32, device=dev)
    tkey = torch.empty(cap, dtype=torch.int64, device=dev)
    tcount, tfirst, err = torch.empty(cap, **i32), torch.empty(cap, **i32), torch.zeros(1, **i32)
    check(lib.mapx_vocab_table_init(ptr(tkey), ptr(tcount), ptr(tfirst), cap, stream()))
    check(lib.mapx_vocab_count(ptr(keys), N, ptr(tkey), ptr(tcount), ptr(tfirst), cap, ptr(err), stream()))
    ranked_keys, ranked_counts, U = _rank_counted(name, tkey, tcount, tfirst, cap, N, err, n_core)
    return FieldVocab(name, ranked_keys, ranked_counts, base, U)


def _rank_counted(name, tkey, tcount, tfirst, cap, N, err, n_core):
    """A filled count table (mapx_vocab_count, or mapx_vocab_count_missing for the values a saved field lacks) of a
    column of N rows -> (kept keys in id order, their counts, number of distinct values counted): compact, the two
    stable sorts, the n-core cut.  `err`: the counting launch's error word."""
    dev, i32 = tkey.device, dict(dtype=torch.int32, device=tkey.device)
    ent_cap = min(N, cap)
    ekey = torch.empty(ent_cap, dtype=torch.int64, device=dev)
    ecount, efirst, nm = torch.empty(ent_cap, **i32), torch.empty(ent_cap, **i32), torch.zeros(2, **i32)
    check(lib.mapx_vocab_compact(ptr(tkey), ptr(tcount), ptr(tfirst), cap, ptr(ekey), ptr(ecount), ptr(efirst),
                                 ptr(nm), stream()))
    e, (U, maxc) = int(err.item()), (int(x) for x in nm.tolist())          # offline path: host syncs are fine
    if e & 1:
        raise ValueError(f"field {name!r}: the value -2^63 is reserved by the vocabulary builder")
    if e & 2:
        raise MapxError(f"field {name!r}: hash table of {cap} slots is full")
    if U == 0:                                                   # (a grown field none of whose rows is missing)
        return ekey[:0], ecount[:0], 0
    # rank = (count descending, first occurrence ascending): stable sort by first position, then by max - count
    by_first = ops.SegPlan(efirst[:U].contiguous(), N).perm
    keys2 = torch.empty(U, **i32)
    check(lib.mapx_vocab_rank_keys(ptr(ecount), ptr(by_first), U, maxc, ptr(keys2), stream()))
    by_count = ops.SegPlan(keys2, maxc + 1).perm
    ranked_counts, n_kept = torch.empty(U, **i32), torch.zeros(1, **i32)
    ranked_keys = torch.empty(U, dtype=torch.int64, device=dev)
    check(lib.mapx_vocab_assign(ptr(by_first), ptr(by_count), ptr(ecount), ptr(ekey), U, int(n_core),
                                ptr(ranked_keys), ptr(ranked_counts), ptr(n_kept), stream()))
    k = int(n_kept.item())
    return ranked_keys[:k], ranked_counts[:k], U


def build_field(keys, n_core, base, out_col, name="", capacity=None):
    """Ids of one field.  keys int64 [N] on the device; out_col: an int64 column view (stride = row length) that
    receives the ids: fit_field, then the column through a one-field Vocabulary of the fitted keys.
    -> FieldVocab (device tensors)."""
    require_gpu(keys, out_col)
    if out_col.dtype != torch.int64 or out_col.dim() != 1 or out_col.shape[0] != keys.numel():
        raise TypeError("build_field: out_col must be an int64 column of N rows")
    fv = fit_field(keys, n_core, base, name=name, capacity=capacity)
    Vocabulary([fv], device=keys.device).encode([keys], feat_ids_out=out_col.unsqueeze(1))
    return fv


def _feat_map(fields, decoders):
    """proc_avazu.py:213-250: the reserved tokens, then per field f'{name}-{value as printed}' of the kept values in
    id order and f'{name}-<oov>'.  decoders: {field name: code -> str}; absent names print as integers."""
    feat_map = {tok: i for i, tok in enumerate(RESERVED)}
    for f in fields:
        dec = decoders.get(f.name, lambda v: str(int(v)))
        for v in f.keys.tolist():                               # (the one device -> host copy of a fitted field's keys)
            feat_map[f"{f.name}-{dec(v)}"] = len(feat_map)
        feat_map[f"{f.name}-<oov>"] = len(feat_map)
        assert feat_map[f"{f.name}-<oov>"] == f.oov
    return feat_map


def _feat_type_map(names, feat_types):
    """'<rsv>' = 0, the fields' types in order of first appearance, then '<oov>' (proc_avazu.py:211-231)."""
    tmap = {"<rsv>": 0}
    for n in names:
        tmap.setdefault(feat_types[n], len(tmap))
    tmap.setdefault("<oov>", len(tmap))
    return tmap


def _field_ids(field_map, names, n_rows):
    return np.tile(np.array([field_map[n] for n in names], dtype=np.int32), (n_rows, 1))


def _fit_encode(columns, n_core, device, decoders, types=None):
    """build_vocab, and with types = (string_columns, feat_types, feat_type_map) also type_ids int64 [N, F] from the
    same launches: the '<oov>' type where an integer-origin value is -1, else the field's own type."""
    names = list(columns)
    decoders = decoders or {}
    dec, cols, flags = {}, [], []
    for name in names:
        c = columns[name]
        if torch.is_tensor(c):
            cols.append(c.to(device=device, dtype=torch.int64).contiguous())
            dec[name] = decoders.get(name, lambda v: str(int(v)))
            flags.append(True)
        else:
            codes, dec[name] = encode_column(c)
            cols.append(torch.as_tensor(codes).to(device))
            flags.append(np.asarray(c).dtype.kind in "iu")
    N = cols[0].numel() if cols else 0
    if any(c.numel() != N for c in cols):
        raise ValueError("build_vocab: columns of different lengths")
    fields, base = [], len(RESERVED)
    for name, keys in zip(names, cols):
        fields.append(fit_field(keys, n_core, base, name=name))
        base = fields[-1].oov + 1
    feat_ids = torch.empty(N, len(names), dtype=torch.int64, device=device)
    type_ids, field_types, missing_type = None, [0] * len(names), 0
    if types is not None:
        strings, feat_types, tmap = types
        type_ids = torch.empty_like(feat_ids)
        flags = [flag and n not in strings for n, flag in zip(names, flags)]
        field_types, missing_type = [tmap[feat_types[n]] for n in names], tmap["<oov>"]
    for g in range(0, len(names), RT_MAX_FIELDS):               # a Vocabulary holds at most RT_MAX_FIELDS fields
        h = slice(g, g + RT_MAX_FIELDS)
        voc = Vocabulary(fields[h], device=device, flags=flags[h], field_types=field_types[h],
                         missing_type=missing_type)
        voc.encode(cols[h], feat_ids_out=feat_ids[:, h], type_ids_out=None if type_ids is None else type_ids[:, h])
    return feat_ids, fields, _feat_map(fields, dec), base, type_ids


def build_vocab(columns, n_core, device="cuda", decoders=None):
    """columns: ordered {field name: raw column [N]} (the reference's valid_fields without 'click'), host arrays or
    device int64 tensors.  -> (feat_ids int64 [N, F] on the device, [FieldVocab], feat_map {str: id},
    input_size) — `feat_map` as proc_avazu.py:213-250 builds it, `input_size` = len(feat_map).  Every field is fitted
    (fit_field), then all columns are translated through the fitted keys, up to RT_MAX_FIELDS fields a launch.
    decoders: {field name: code -> str} for tensor columns whose codes do not print as themselves (the hash-string
    codes of mapx.rawtext); absent names print as integers."""
    return _fit_encode(columns, n_core, device, decoders)[:4]


def _write_dataset(data_dir, name, meta, feat_ids, field_ids, type_ids, labels, split, seed):
    """`<name>-meta.json` and `<name>.npz` {feat_ids, field_ids, type_ids, labels} in the layout mapx/dataset.py reads;
    with `split` = (train, valid, test) fractions and no `split.pkl` there yet, a seeded random one."""
    import pickle as pkl
    os.makedirs(data_dir, exist_ok=True)
    with open(os.path.join(data_dir, f"{name}-meta.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False)
    np.savez(os.path.join(data_dir, f"{name}.npz"), feat_ids=feat_ids.cpu().numpy(), field_ids=field_ids,
             type_ids=type_ids.cpu().numpy(), labels=labels.astype(np.int64))
    if split is not None and not os.path.exists(os.path.join(data_dir, "split.pkl")):
        N = len(labels)
        perm = np.random.RandomState(seed).permutation(N)
        a, b = int(N * split[0]), int(N * (split[0] + split[1]))
        with open(os.path.join(data_dir, "split.pkl"), "wb") as f:
            pkl.dump({"train_index": np.sort(perm[:a]), "valid_index": np.sort(perm[a:b]),
                      "test_index": np.sort(perm[b:])}, f)


def generate_dataset(columns, labels, n_core, data_dir, dataset_name, feat_types=None, seed=42, device="cuda",
                     split=None, string_columns=None, decoders=None, shuffle=True):
    """The whole of reference generate_dataset() (proc_avazu.py:193-302 / proc_criteo.py:90-196) for raw columns
    held in memory: rows shuffled by numpy's seeded permutation (np.random.seed(42); shuffle(arange(N)) —
    :194-199), vocabulary and ids on the GPU (build_vocab), the reference's meta JSON (index, num_pos, num_neg,
    avg_ctr, field_names, field_map, feat_type_map, feat_map) and the table {feat_ids, field_ids, type_ids,
    labels}, written in the layout code/dataset.py:20-40 reads (here: mapx/dataset.py — `<name>-meta.json`,
    `<name>.npz`).  feat_types: {field: '<cat>' | '<num>'} (default all '<cat>', proc_avazu.py:24); a raw value of
    -1 gets the '<oov>' type (proc_avazu.py:258-261, proc_criteo.py:161-166), in the launch that translates the ids.
    split: None, or (train, valid, test) fractions for a seeded random `split.pkl` (the reference's own split
    files come from split_criteo_x4.py — scikit-learn's StratifiedKFold — and are used as they are when present).
    Columns (and labels) may be device int64 tensors (mapx.rawtext): the seeded permutation is still numpy's, on
    the host; the rows are gathered on the device.  string_columns: names whose values were strings in the raw
    file: no row of theirs gets the '<oov>' type, because the reference compares a string with -1 there
    (proc_criteo.py:162); host columns of string dtype are such columns too.  decoders: see build_vocab.
    shuffle=False keeps the file's row order, as proc_criteo.py:98-102 does unless it down-samples."""
    names = list(columns)
    feat_types = feat_types or {n: "<cat>" for n in names}
    labels = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    np.random.seed(seed)
    index = np.arange(len(labels))
    if shuffle:
        np.random.shuffle(index)
    labels = labels[index]
    index_dev = None
    shuffled = {}
    for n in names:
        if torch.is_tensor(columns[n]):
            if index_dev is None:
                index_dev = torch.from_numpy(index).to(columns[n].device)
            shuffled[n] = columns[n].to(torch.int64)[index_dev]
        else:
            shuffled[n] = np.asarray(columns[n])[index]
    field_map = {n: i for i, n in enumerate(["<rsv>"] + names)}
    feat_type_map = _feat_type_map(names, feat_types)
    feat_ids, _fields, feat_map, input_size, type_ids = _fit_encode(
        shuffled, n_core, device, decoders, types=(set(string_columns or ()), feat_types, feat_type_map))
    N = len(labels)
    meta = {"index": index.tolist(), "num_pos": int(labels.sum()), "num_neg": int(N - labels.sum()),
            "avg_ctr": float(labels.mean()) if N else 0.0, "field_names": ["<rsv>"] + names, "field_map": field_map,
            "feat_type_map": feat_type_map, "feat_map": feat_map}
    _write_dataset(data_dir, dataset_name, meta, feat_ids, _field_ids(field_map, names, N), type_ids, labels, split,
                   seed)
    return meta, input_size


def generate_dataset_from_text(path, schema, n_core, data_dir, dataset_name, chunk_bytes=256 << 20, mode=0, seed=42,
                               device="cuda", split=None):
    """Raw file -> dataset directory: mapx.rawtext.read_columns (read_feat on the device), then generate_dataset
    with the schema's field types, string columns, decoders and row order."""
    from . import rawtext
    labels, columns, decode, strings = rawtext.read_columns(path, schema, device=device, chunk_bytes=chunk_bytes,
                                                            mode=mode)
    return generate_dataset(columns, labels, n_core, data_dir, dataset_name, feat_types=schema.feat_types, seed=seed,
                            device=device, split=split, string_columns=strings, decoders=decode,
                            shuffle=schema.shuffle)


# ------------------------------------------------------------------ a saved vocabulary applied to other rows
class FieldKeys:
    """One field of a saved feat_map: `keys` int64 [n] = the kept raw values in id order (the codes mapx.rawtext
    gives the file's values), on the host, `base` the id of the first of them, `oov` = base + n the id of
    `<name>-<oov>`.  (A fitted field, FieldVocab, is the same with its keys on the device.)"""

    def __init__(self, name, keys, base):
        self.name, self.keys, self.base = name, np.ascontiguousarray(keys, dtype=np.int64), int(base)
        self.oov = self.base + int(self.keys.shape[0])


def _invert(name, kind, text, key):
    """The printed value of a feat_map key -> the column's int64 code."""
    from . import rawtext
    if kind == rawtext.HEX:
        if text == "-1":
            return -1
        try:
            if not text:
                raise ValueError(text)
            return rawtext.encode_hex(text)
        except ValueError:
            raise ValueError(f"feat_map key {key!r}: {text!r} is not a value of the hash-string column {name!r} "
                             f"(1 to 14 lower-case hexadecimal digits, or -1)") from None
    try:
        v = int(text)
    except ValueError:
        v = None
    if v is None or str(v) != text or not (-(1 << 63) < v < (1 << 63)):
        raise ValueError(f"feat_map key {key!r}: {text!r} is not an integer value of column {name!r} as it prints")
    return v


def parse_meta(meta, schema):
    """`field_names` and `feat_map` of a `<name>-meta.json` (a dict, or the file's path) -> [FieldKeys], one per
    field in order.  Pure host work.  The printed value of every key is inverted by the kind of the schema's
    column: hash strings through rawtext.encode_hex ('-1', the empty field, -> -1), integers through int(), which
    must print back as the text.  A feat_map written by the reference's own data_preprocess scripts for the same
    raw file has exactly these keys (f'{name}-{value}' in Counter.most_common() order, then f'{name}-<oov>'), so it
    loads too.  ValueError, naming the key or field, when the first ten entries are not RESERVED, the fields are
    not the schema's columns (label excluded) in order, an id is not the next one, a field's `<name>-<oov>` is
    missing or not its last id, a value does not invert, or two values of a field invert to one code."""
    if not isinstance(meta, dict):
        with open(os.fspath(meta)) as f:
            meta = json.load(f)
    kinds = {n: k for n, k in zip(schema.columns, schema.column_kinds) if n != schema.label}
    names = list(kinds)
    if list(meta["field_names"]) != ["<rsv>"] + names:
        raise ValueError(f"field_names {list(meta['field_names'])} are not '<rsv>' and the {schema.name} schema's "
                         f"columns {names}")
    items = list(meta["feat_map"].items())
    if [k for k, _ in items[:len(RESERVED)]] != list(RESERVED):
        raise ValueError(f"feat_map: the first {len(RESERVED)} keys {[k for k, _ in items[:len(RESERVED)]]} are not "
                         f"the reserved tokens {list(RESERVED)}")
    for pos, (key, i) in enumerate(items):
        if type(i) is not int or i != pos:
            raise ValueError(f"feat_map key {key!r}: id {i!r} where the ids are consecutive from 0 (expected {pos})")
    fields, pos = [], len(RESERVED)
    for name in names:
        prefix, start = name + "-", pos
        while pos < len(items) and items[pos][0].startswith(prefix):
            pos += 1
        run = [k[len(prefix):] for k, _ in items[start:pos]]
        if not run:
            found = repr(items[pos][0]) if pos < len(items) else "the end of the map"
            raise ValueError(f"feat_map: field {name!r} has no keys where the schema's column order puts them "
                             f"(found {found})")
        if run[-1] != "<oov>" or "<oov>" in run[:-1]:
            raise ValueError(f"feat_map key {prefix + '<oov>'!r} is missing or is not the last id of field {name!r}")
        codes = np.array([_invert(name, kinds[name], t, prefix + t) for t in run[:-1]], dtype=np.int64)
        uniq, first = np.unique(codes, return_index=True)
        if len(uniq) != len(codes):
            twice = np.setdiff1d(np.arange(len(codes)), first)[0]
            same = [prefix + t for t, c in zip(run[:-1], codes.tolist()) if c == codes[twice]]
            raise ValueError(f"feat_map keys {same[0]!r} and {same[1]!r} of field {name!r} are one value ({codes[twice]})")
        fields.append(FieldKeys(name, codes, start))
    if pos != len(items):
        raise ValueError(f"feat_map key {items[pos][0]!r}: not a key of the schema's columns {names} in order")
    return fields


def _is_pow2(c):
    return c >= 1 and (c & (c - 1)) == 0


class Vocabulary:
    """The lookup tables of a vocabulary on the device (csrc/vocab_apply.hip).  fields: [FieldKeys] (a saved
    vocabulary) or [FieldVocab] (one just fitted: its keys stay on the device) with consecutive id ranges.
    flags[f] != 0: a raw -1 in field f gets `missing_type` in type_ids (integer-origin columns; string-origin
    columns have flag 0: generate_dataset's rule, which it applies through here); field_types[f]: the type id otherwise.
    capacities: table slots per field instead of the default (the smallest power of two >= max(2, 2 n_f)); each a
    power of two > n_f.  `feat_map`, `field_names`, `input_size` are those of the meta the vocabulary came from."""

    def __init__(self, fields, device="cuda", capacities=None, flags=None, field_types=None, missing_type=0,
                 decoders=None, meta=None):
        F = len(fields)
        if not 1 <= F <= RT_MAX_FIELDS:
            raise ValueError(f"Vocabulary: 1 to {RT_MAX_FIELDS} fields")
        n = [int(f.keys.shape[0]) for f in fields]
        if capacities is None:
            capacities = [int(lib.mapx_vocab_apply_table_slots(k)) for k in n]
            if 0 in capacities:
                raise ValueError("Vocabulary: a field holds at most 2^30 - 1 keys")
        capacities = [int(c) for c in capacities]
        if len(capacities) != F:
            raise ValueError(f"Vocabulary: {len(capacities)} capacities for {F} fields")
        for f, c, k in zip(fields, capacities, n):
            if not _is_pow2(c) or c <= k or c > (1 << 31):
                raise ValueError(f"field {f.name!r}: a capacity of {c} slots for {k} keys (a power of two > {k}, at "
                                 f"most 2^31)")
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise MapxError("mapx.vocab.Vocabulary looks up on the device (HIP); there is no CPU path")
        self.fields, self.device, self.capacities = list(fields), dev, capacities
        self.decoders = decoders or {}
        self.meta = meta
        self.field_names = [f.name for f in fields]
        self.missing_type = int(missing_type)
        par = np.zeros((6, F + 1), dtype=np.int64)            # key_off, tab_off, n_keys, base, flag, field_type
        par[0, 1:], par[1, 1:] = np.cumsum(n), np.cumsum(capacities)
        par[2, :F], par[3, :F] = n, [f.base for f in fields]
        par[4, :F] = [1] * F if flags is None else [int(bool(x)) for x in flags]
        par[5, :F] = [0] * F if field_types is None else [int(x) for x in field_types]
        self._par_host = par
        self._par = torch.from_numpy(par).to(dev)
        self.n_keys_total, self.n_slots = int(par[0, F]), int(par[1, F])
        self._keys = torch.cat([torch.as_tensor(f.keys).to(dev) for f in fields])
        self._tkey = torch.empty(self.n_slots, dtype=torch.int64, device=dev)
        self._trank = torch.empty(self.n_slots, dtype=torch.int32, device=dev)
        err = torch.empty(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib.mapx_vocab_apply_load(ptr(self._keys), ptr(self._par[0]), ptr(self._par[1]), F,
                                            self.n_keys_total, self.n_slots, ptr(self._tkey), ptr(self._trank),
                                            ptr(err), stream()))
        bits, field = err.tolist()
        self._raise(bits, field, "a key of the vocabulary")

    def _raise(self, bits, field, what):
        if not bits:
            return
        name = self.field_names[field] if 0 <= field < len(self.fields) else "?"
        if bits & 1:
            raise ValueError(f"field {name!r}: {what} is -2^63, the value the lookup tables reserve")
        if bits & 4:
            raise ValueError(f"field {name!r}: one key twice in the vocabulary")
        raise MapxError(f"field {name!r}: the table slice of {self.capacities[field]} slots does not fit its keys")

    @classmethod
    def from_meta(cls, meta, schema, device="cuda", capacities=None):
        """meta: the dict of a `<name>-meta.json`, or its path.  Field types and the '<oov>' type come from the
        meta's feat_type_map when it has one, else they are numbered as generate_dataset numbers them."""
        if not isinstance(meta, dict):
            with open(os.fspath(meta)) as f:
                meta = json.load(f)
        fields = parse_meta(meta, schema)
        tmap = meta.get("feat_type_map") or _feat_type_map([f.name for f in fields], schema.feat_types)
        return cls(fields, device=device, capacities=capacities,
                   flags=[f.name not in schema.string_columns for f in fields],
                   field_types=[tmap[schema.feat_types[f.name]] for f in fields], missing_type=tmap["<oov>"],
                   decoders={f.name: schema.decoder(f.name) for f in fields}, meta=meta)

    @property
    def feat_map(self):
        return self.meta["feat_map"] if self.meta is not None else _feat_map(self.fields, self.decoders)

    @property
    def input_size(self):
        return self.fields[-1].oov + 1

    def _column(self, f, c):
        """One input column as a contiguous device int64 vector."""
        if torch.is_tensor(c):
            if c.dtype != torch.int64 or c.dim() != 1:
                raise TypeError(f"field {f.name!r}: a tensor column must be an int64 vector")
            return c.to(self.device).contiguous()
        a = np.asarray(c)
        if a.dtype.kind in "iu":
            codes, _ = encode_column(a)
        elif a.dtype.kind in "USO":                             # hash strings: the codes the keys were inverted to
            from . import rawtext
            codes = np.array([-1 if s in ("-1", "") else rawtext.encode_hex(s) for s in map(str, a.tolist())],
                             dtype=np.int64)
        else:
            raise TypeError(f"field {f.name!r}: dtype {a.dtype} (integers or hash strings)")
        return torch.from_numpy(np.ascontiguousarray(codes)).to(self.device)

    def _columns(self, columns, who):
        """The F input columns of encode / grow as contiguous device int64 vectors of one length.  -> (columns, N)."""
        F = len(self.fields)
        if isinstance(columns, dict):
            if list(columns) != self.field_names:
                raise ValueError(f"{who}: columns {list(columns)} are not the vocabulary's fields {self.field_names}")
            columns = list(columns.values())
        if len(columns) != F:
            raise ValueError(f"{who}: {len(columns)} columns for {F} fields")
        cols = [self._column(f, c) for f, c in zip(self.fields, columns)]
        N = cols[0].numel()
        if any(c.numel() != N for c in cols):
            raise ValueError(f"{who}: columns of different lengths")
        return cols, N

    def grow(self, columns, n_core, capacities=None):
        """The vocabulary extended by the values of `columns` (as encode takes them) that it does not hold: per field
        the misses are counted behind a lookup in the field's table slice (mapx_vocab_count_missing), ranked by the
        fit's own rule — descending count, ties by first occurrence, i.e. Counter(misses).most_common() — through
        fit_field's compact / sort / assign steps, and those seen at least n_core times are appended behind the
        field's keys; every old key keeps its rank, ids stay consecutive (base'_f = 10 + sum_{g<f} (n_g + a_g + 1)).
        -> (grown Vocabulary, added: keys appended per field, missing_before: rows per field that take <oov> under
        this vocabulary, missing_after: ... under the grown one) — F host ints each.  The grown feat_map keeps the
        old keys' strings and order and prints the added keys with this vocabulary's decoders.  capacities: count
        table slots per field (each a power of two >= 64 and more than the field's distinct misses) instead of the
        fit's default.  ValueError, naming the field, when a column holds -2^63."""
        F, dev = len(self.fields), self.device
        cols, N = self._columns(columns, "grow")
        if capacities is not None and len(capacities) != F:
            raise ValueError(f"grow: {len(capacities)} capacities for {F} fields")
        i32 = dict(dtype=torch.int32, device=dev)
        tab_off, n_keys = self._par_host[1], self._par_host[2]
        grown_fields, added, before, after, base = [], [], [], [], self.fields[0].base
        with torch.cuda.device(dev):
            for f, (fld, keys) in enumerate(zip(self.fields, cols)):
                new_keys, miss, kept_rows = np.empty(0, dtype=np.int64), 0, 0
                if N:
                    cap = int(capacities[f]) if capacities is not None else \
                        max(64, 1 << int(np.ceil(np.log2(2 * N + 1))))
                    tkey = torch.empty(cap, dtype=torch.int64, device=dev)
                    tcount, tfirst, err = torch.empty(cap, **i32), torch.empty(cap, **i32), torch.zeros(1, **i32)
                    missing = torch.zeros(1, dtype=torch.int64, device=dev)
                    check(lib.mapx_vocab_table_init(ptr(tkey), ptr(tcount), ptr(tfirst), cap, stream()))
                    check(lib.mapx_vocab_count_missing(ptr(keys), N, ptr(self._tkey), ptr(self._trank), int(tab_off[f]),
                                                       int(tab_off[f + 1] - tab_off[f]), self.n_slots, int(n_keys[f]),
                                                       ptr(tkey), ptr(tcount), ptr(tfirst), cap, ptr(err), ptr(missing),
                                                       stream()))
                    rk, rc, _ = _rank_counted(fld.name, tkey, tcount, tfirst, cap, N, err, n_core)
                    new_keys, miss, kept_rows = rk.cpu().numpy(), int(missing.item()), int(rc.sum().item())
                old = fld.keys.cpu().numpy() if torch.is_tensor(fld.keys) else np.asarray(fld.keys)
                grown_fields.append(FieldKeys(fld.name, np.concatenate([old.astype(np.int64), new_keys]), base))
                base = grown_fields[-1].oov + 1
                added.append(len(new_keys))
                before.append(miss)
                after.append(miss - kept_rows)
        old_items = list(self.feat_map)
        feat_map = {tok: i for i, tok in enumerate(old_items[:self.fields[0].base])}
        for fld, g, a in zip(self.fields, grown_fields, added):
            for key in old_items[fld.base:fld.oov]:
                feat_map[key] = len(feat_map)
            dec = self.decoders.get(fld.name, lambda v: str(int(v)))
            for v in g.keys[len(g.keys) - a:].tolist():
                key = f"{fld.name}-{dec(v)}"
                if key in feat_map:
                    raise ValueError(f"grow: the added value {v} of field {fld.name!r} prints as {key!r}, a key the "
                                     f"vocabulary holds already")
                feat_map[key] = len(feat_map)
            feat_map[f"{fld.name}-<oov>"] = len(feat_map)
            assert feat_map[f"{fld.name}-<oov>"] == g.oov
        meta = dict(self.meta if self.meta is not None else {"field_names": ["<rsv>"] + self.field_names},
                    feat_map=feat_map)
        par = self._par_host
        grown = Vocabulary(grown_fields, device=dev, flags=par[4, :F].tolist(), field_types=par[5, :F].tolist(),
                           missing_type=self.missing_type, decoders=self.decoders, meta=meta)
        return grown, added, before, after

    def encode(self, columns, type_ids=False, feat_ids_out=None, type_ids_out=None, mode=0):
        """columns: {field name: column} in the vocabulary's field order, or a sequence of F columns; each a device
        int64 vector or a host array (integers as they are; hash strings through rawtext.encode_hex).
        -> (feat_ids int64 [N, F] on the device, oov_rows: F host ints, the rows per field that took the field's
        <oov> id[, type_ids int64 [N, F]]).  One launch for all fields and one device -> host read (error word and
        counters) at the end.  feat_ids_out / type_ids_out: int64 [N, F] views with unit column stride and any row
        pitch to write into.  mode: see mapx_vocab_apply (0: row-contiguous stores through LDS, 1: strided stores).
        ValueError, naming the field, when a column holds -2^63."""
        F = len(self.fields)
        cols, N = self._columns(columns, "encode")
        dev = self.device

        def out(t, what):
            if t is None:
                return torch.empty(N, F, dtype=torch.int64, device=dev)
            require_gpu(t)
            if t.dtype != torch.int64 or tuple(t.shape) != (N, F) or (F > 1 and t.stride(1) != 1) or \
                    (N > 1 and t.stride(0) < F):
                raise TypeError(f"encode: {what} must be int64 [{N}, {F}] with unit column stride and a row pitch >= {F}")
            return t
        ids = out(feat_ids_out, "feat_ids_out")
        types = out(type_ids_out, "type_ids_out") if (type_ids or type_ids_out is not None) else None
        ld = lambda t: t.stride(0) if N > 1 else F             # (the pitch of a single row is never used)
        col_ptrs = torch.tensor([c.data_ptr() for c in cols], dtype=torch.int64).to(dev)
        stat = torch.empty(F + 1, dtype=torch.int64, device=dev)   # oov_rows [F] | the two error words
        par = self._par
        with torch.cuda.device(dev):
            check(lib.mapx_vocab_apply(ptr(col_ptrs), N, F, ptr(self._tkey), ptr(self._trank), ptr(par[1]),
                                       self.n_slots, ptr(par[2]), ptr(par[3]), ptr(par[4]), ptr(par[5]),
                                       self.missing_type, ids.data_ptr(), ld(ids),
                                       None if types is None else types.data_ptr(), F if types is None else ld(types),
                                       ptr(stat), stat.data_ptr() + 8 * F, int(mode), stream()))
        host = stat.cpu()                                       # the one read; it also ends the launch's use of cols
        bits, field = host[F:].view(torch.int32).tolist()
        self._raise(bits, field, "a value of the column")
        oov_rows = host[:F].tolist()
        return (ids, oov_rows, types) if types is not None else (ids, oov_rows)


def encode_dataset_from_text(path, schema, meta_path, data_dir, dataset_name, chunk_bytes=256 << 20, split=None,
                             seed=42, device="cuda"):
    """Raw file -> dataset directory through the vocabulary SAVED in meta_path (the `<name>-meta.json` of an earlier
    fit): mapx.rawtext.read_columns, then Vocabulary.encode.  Writes `<name>.npz` {feat_ids, field_ids, type_ids,
    labels} and `<name>-meta.json` with the vocabulary's field_names / field_map / feat_type_map / feat_map verbatim
    (same key order), this file's num_pos / num_neg / avg_ctr, index = 0..N-1 and `oov_rows` {field: rows that took
    the field's <oov> id}; with `split`, a `split.pkl` by generate_dataset's seeded rule.  The rows stay in file
    order: encode mode never shuffles (the ids of a row do not depend on the order, and a file that is scored or
    evaluated is wanted as it is).  -> (meta, input_size)."""
    from . import rawtext
    with open(os.fspath(meta_path)) as f:
        saved = json.load(f)
    voc = Vocabulary.from_meta(saved, schema, device=device)
    labels, columns, _decode, _strings = rawtext.read_columns(path, schema, device=device, chunk_bytes=chunk_bytes)
    return _encode_and_write(voc, saved, schema, columns, labels, data_dir, dataset_name, split, seed, {})


def _encode_and_write(voc, saved, schema, columns, labels, data_dir, dataset_name, split, seed, extra):
    """The columns of a file through `voc` into a dataset directory, rows in file order; the meta takes field_names /
    field_map / feat_type_map from the saved meta, feat_map from the vocabulary, and `extra`."""
    feat_ids, oov_rows, type_ids = voc.encode(columns, type_ids=True)
    labels = labels.cpu().numpy()
    N, names = len(labels), voc.field_names
    field_map = saved.get("field_map") or {n: i for i, n in enumerate(["<rsv>"] + names)}
    feat_type_map = saved.get("feat_type_map") or _feat_type_map(names, schema.feat_types)
    meta = {"index": list(range(N)), "num_pos": int(labels.sum()), "num_neg": int(N - labels.sum()),
            "avg_ctr": float(labels.mean()) if N else 0.0, "field_names": saved["field_names"], "field_map": field_map,
            "feat_type_map": feat_type_map, "feat_map": voc.feat_map,
            "oov_rows": {n: int(c) for n, c in zip(names, oov_rows)}}
    meta.update(extra)
    _write_dataset(data_dir, dataset_name, meta, feat_ids, _field_ids(field_map, names, N), type_ids, labels, split,
                   seed)
    return meta, voc.input_size


def grow_dataset_from_text(path, schema, meta_path, n_core, data_dir, dataset_name, chunk_bytes=256 << 20, split=None,
                           seed=42, device="cuda"):
    """encode_dataset_from_text with the SAVED vocabulary grown on the file first: the file is read once
    (mapx.rawtext.read_columns), its values the saved feat_map lacks and that occur at least n_core times are appended
    per field (Vocabulary.grow: old ids keep their meaning, ids stay consecutive), and the file is encoded with the
    grown vocabulary.  The meta carries the grown feat_map, `oov_rows` under the grown vocabulary and
    `grown` {field: keys added}; rows stay in file order.  mapx.grow moves a checkpoint trained on the saved
    vocabulary, or a dataset encoded with it, to the grown id space.  -> (meta, input_size)."""
    from . import rawtext
    with open(os.fspath(meta_path)) as f:
        saved = json.load(f)
    voc = Vocabulary.from_meta(saved, schema, device=device)
    labels, columns, _decode, _strings = rawtext.read_columns(path, schema, device=device, chunk_bytes=chunk_bytes)
    grown, added, _before, _after = voc.grow(columns, n_core)
    return _encode_and_write(grown, saved, schema, columns, labels, data_dir, dataset_name, split, seed,
                             {"grown": {n: int(a) for n, a in zip(voc.field_names, added)}})
