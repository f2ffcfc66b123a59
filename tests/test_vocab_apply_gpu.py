"""A saved vocabulary applied on the GPU (mapx/vocab.py Vocabulary over csrc/vocab_apply.hip, the --vocab mode of
mapx/preprocess.py) against the reference's translation line restated with a Python dict (tests/vocab_apply_ref.py):
the committed raw files round trip and held out, synthetic tables (extents around the 64-row tile, empty and
near-full slices, one raw value in two fields), guard bands, every error, and the properties at two million rows.
Integer work: every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import rawtext_ref as R
import vocab_apply_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}
I64_MIN = -(1 << 63)


def _load(directory, name):
    with open(os.path.join(directory, f"{name}-meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(directory, f"{name}.npz"))


def _decoders(schema):
    return {n: (R.decode_hex if k == R.HEX else (lambda v: str(int(v))))
            for n, k in zip(schema.columns, schema.column_kinds) if n != schema.label}


# ---------------------------------------------------------------- 1. the committed raw files, round trip
@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_round_trip_through_the_command_line(golden_dir, tmp_path, name, capsys):
    """Fit into A, encode the SAME file with A's meta into B: B is A's table in file order.  (tests/test_rawtext_gpu.py
    pins A to the reference, which anchors B to it.)"""
    from mapx import preprocess
    from mapx.dataset import BaseDataset
    z = np.load(os.path.join(golden_dir, f"rawtext_{name}.npz"))
    path, a_dir, b_dir = os.path.join(golden_dir, RAW[name]), str(tmp_path / "A"), str(tmp_path / "B")
    assert preprocess.main(["--dataset", name, "--raw", path, "--n_core", str(int(z["n_core"])), "--out", a_dir,
                            "--chunk_mb", "1"]) == 0
    capsys.readouterr()
    assert preprocess.main(["--dataset", name, "--raw", path, "--vocab", os.path.join(a_dir, f"{name}-meta.json"),
                            "--out", b_dir, "--chunk_mb", "1", "--split", "0.8,0.1,0.1"]) == 0
    said = capsys.readouterr().out
    (ma, ta), (mb, tb) = _load(a_dir, name), _load(b_dir, name)
    index = np.array(ma["index"])
    N, F = ta["feat_ids"].shape
    if name == "criteo":
        assert np.array_equal(index, np.arange(N))
    assert mb["index"] == list(range(N))
    for what in ("feat_ids", "labels", "type_ids", "field_ids"):
        assert tb[what].dtype == ta[what].dtype and np.array_equal(tb[what][index], ta[what]), what
    assert list(mb["feat_map"].items()) == list(ma["feat_map"].items())
    for key in ("field_names", "field_map", "feat_type_map"):
        assert mb[key] == ma[key] and list(mb[key]) == list(ma[key]), key
    assert (mb["num_pos"], mb["num_neg"], mb["avg_ctr"]) == (ma["num_pos"], ma["num_neg"], ma["avg_ctr"])
    names = ma["field_names"][1:]
    assert list(mb["oov_rows"]) == names
    shares = []
    for j, n in enumerate(names):
        count = int((ta["feat_ids"][:, j] == ma["feat_map"][f"{n}-<oov>"]).sum())
        assert mb["oov_rows"][n] == count, n
        shares.append((count / N, n))
    top = sorted(shares, key=lambda x: -x[0])[:3]
    assert "<oov> share " + ", ".join(f"{n} {s:.4f}" for s, n in top) in said

    class Args:
        data_dir, dataset_name, pretrain, pt_type, RFD_replace = b_dir, name, True, "MFP", "Unigram"
    ds = BaseDataset(Args())
    assert ds.get_splited_dataset("train").X.shape == (int(N * 0.8), F) and ds.feat_map == ma["feat_map"]


# ---------------------------------------------------------------- 2. held-out rows
def _halves(golden_dir, name, schema):
    """The file cut at the middle one of its physical lines below the header (the Criteo file holds a blank one)."""
    with open(os.path.join(golden_dir, RAW[name]), "rb") as f:
        lines = f.read().split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    head, lines = (lines[:1], lines[1:]) if schema.header else ([], lines)
    mid = len(lines) // 2
    return b"\n".join(head + lines[:mid]) + b"\n", b"\n".join(head + lines[mid:]) + b"\n"


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_held_out_half_against_the_restatement(golden_dir, tmp_path, name):
    """Fit on the first half of the data lines (n_core 2), encode the second half."""
    from mapx import preprocess, rawtext, vocab
    schema = rawtext.SCHEMAS[name]
    first, second = _halves(golden_dir, name, schema)
    p1, p2, a_dir = tmp_path / "first.txt", tmp_path / "second.txt", str(tmp_path / "A")
    p1.write_bytes(first)
    p2.write_bytes(second)
    assert preprocess.main(["--dataset", name, "--raw", str(p1), "--n_core", "2", "--out", a_dir]) == 0
    ma, _ = _load(a_dir, name)
    labels, cols = R.parse(second, schema)
    dec = _decoders(schema)
    want = V.apply(ma["feat_map"], cols, dec)
    hits, oov, both = V.outcomes(ma["feat_map"], cols, dec)
    print(f"{name}: {hits} hits, {oov} <oov>, {want.shape[1]} fields, {both} with both outcomes")
    assert hits >= 1 and oov >= 1 and both >= 5                      # from the restatement alone
    assert (hits, oov, want.shape[1], both) == {"avazu": (5996, 254, 25, 11), "criteo": (8968, 821, 39, 30)}[name]
    oov_ids = [ma["feat_map"][f"{n}-<oov>"] for n in cols]
    for chunk_bytes in (None, 700):
        b_dir = str(tmp_path / f"B{chunk_bytes}")
        mb, input_size = vocab.encode_dataset_from_text(str(p2), schema, os.path.join(a_dir, f"{name}-meta.json"),
                                                        b_dir, name, chunk_bytes=chunk_bytes)
        _, tb = _load(b_dir, name)
        assert np.array_equal(tb["feat_ids"], want) and np.array_equal(tb["labels"], labels)
        assert input_size == len(ma["feat_map"]) and list(mb["feat_map"].items()) == list(ma["feat_map"].items())
        assert list(mb["oov_rows"].values()) == [int((want[:, j] == o).sum()) for j, o in enumerate(oov_ids)]
        t_oov = ma["feat_type_map"]["<oov>"]
        for j, n in enumerate(cols):
            plain = ma["feat_type_map"][schema.feat_types[n]]
            missing = np.zeros(len(labels), dtype=bool) if n in schema.string_columns else cols[n] == -1
            assert np.array_equal(tb["type_ids"][:, j], np.where(missing, t_oov, plain)), n


# ---------------------------------------------------------------- 3. synthetic tables against the restatement
SPECIAL = [0, -1, 1 << 62, -(1 << 40)]
KEY_COUNTS = (0, 1, 2, 1000, 100000)
SIZES = (0, 1, 63, 64, 65, 255, 257, 5000)
_UNIVERSE, _CASES = [], {}


def _universe():
    if not _UNIVERSE:
        rng = np.random.RandomState(5)
        u = np.unique(np.concatenate([rng.randint(-(1 << 40), 1 << 40, 260_000, dtype=np.int64),
                                      rng.randint(1 << 61, 1 << 62, 20_000, dtype=np.int64)]))
        u = u[~np.isin(u, SPECIAL)]
        rng.shuffle(u)
        assert len(u) > 200_000
        _UNIVERSE.append(u)
    return _UNIVERSE[0]


def _fields(F):
    """Field f holds KEY_COUNTS[f % 5] keys: the special values rotated by f, then a window of the shared universe that
    overlaps its neighbours', in an order of its own: one raw value has different ranks in different fields."""
    from mapx import vocab
    u, rng, fields, base = _universe(), np.random.RandomState(100 + F), [], len(vocab.RESERVED)
    for f in range(F):
        n = KEY_COUNTS[f % len(KEY_COUNTS)]
        special = (SPECIAL[f % 4:] + SPECIAL[:f % 4])[:n]
        keys = np.array(special + u[7 * f:7 * f + n - len(special)].tolist(), dtype=np.int64)
        if n > 4:
            rng.shuffle(keys)
        fields.append(vocab.FieldKeys(f"f{f}", keys, base))
        base = fields[-1].oov + 1
    return fields


def _feat_map(fields):
    from mapx import vocab
    fm = {tok: i for i, tok in enumerate(vocab.RESERVED)}
    for f in fields:
        for v in f.keys.tolist():
            fm[f"{f.name}-{v}"] = len(fm)
        fm[f"{f.name}-<oov>"] = len(fm)
    return fm


def _case(F):
    """(fields, feat_map, {N: (columns, expected rows)}) of one F: the restatement runs once."""
    if F not in _CASES:
        fields, u = _fields(F), _universe()
        fm = _feat_map(fields)
        rng = np.random.RandomState(1000 + F)
        dec = {f.name: (lambda v: str(int(v))) for f in fields}
        per_n = {}
        for N in SIZES:
            cols = {}
            for f in fields:
                any_value = np.where(rng.rand(N) < 0.2, rng.choice(np.array(SPECIAL, dtype=np.int64), N),
                                     u[rng.randint(0, len(u), N)])
                if len(f.keys):
                    any_value = np.where(rng.rand(N) < 0.5, f.keys[rng.randint(0, len(f.keys), N)], any_value)
                cols[f.name] = any_value.astype(np.int64)
            per_n[N] = (cols, V.apply(fm, cols, dec))
        if F >= 25:                                                    # one raw value, two fields, two ranks
            a, b = fields[3], fields[8]
            shared = np.intersect1d(a.keys, b.keys)
            assert len(shared) > 900 and any(int(np.nonzero(a.keys == s)[0][0]) != int(np.nonzero(b.keys == s)[0][0])
                                            for s in shared[:50])
        hit = sum(int((rows != [f.oov for f in fields]).sum()) for _, rows in per_n.values())
        total = sum(rows.size for _, rows in per_n.values())
        assert F < 25 or 0.35 * total <= hit <= 0.65 * total          # roughly half are keys (F = 1: no field has one)
        _CASES[F] = (fields, fm, per_n)
    return _CASES[F]


def _tight(fields):
    """The smallest power of two above n_f: 1 slot for no key, 2 for one key, 1024 for 1000 — long chains that wrap
    around the end of a slice."""
    return [1 << int(len(f.keys)).bit_length() for f in fields]


@pytest.mark.parametrize("capacities", ["default", "tight"])
@pytest.mark.parametrize("F", [1, 2, 25, 39, 64])
def test_synthetic_tables_against_the_restatement(F, capacities):
    from mapx import vocab
    fields, fm, per_n = _case(F)
    caps = _tight(fields) if capacities == "tight" else None
    if caps:
        assert caps[:5] == [1, 2, 4, 1024, 131072][:F]
    voc = vocab.Vocabulary(fields, device=DEV, capacities=caps)
    again = vocab.Vocabulary(fields, device=DEV, capacities=caps)     # the same keys, slots claimed in another order
    assert voc.feat_map == fm and voc.input_size == len(fm) and voc.field_names == [f.name for f in fields]
    for N, (cols, want) in per_n.items():
        ids, oov_rows = voc.encode(cols)
        assert ids.shape == (N, F) and ids.dtype == torch.int64 and ids.is_cuda
        assert np.array_equal(ids.cpu().numpy(), want), N
        assert oov_rows == [int((want[:, j] == f.oov).sum()) for j, f in enumerate(fields)], N
        dev_cols = [torch.from_numpy(c).to(DEV) for c in cols.values()]
        for other, mode in ((voc, 0), (again, 0), (voc, 1)):         # twice; another table; the strided store form
            ids2, oov2 = other.encode(dev_cols, mode=mode)
            assert torch.equal(ids2, ids) and oov2 == oov_rows, (N, mode)


# ---------------------------------------------------------------- 4. extents
@pytest.mark.parametrize("N,F", [(65, 25), (257, 64)])
def test_guard_bands_stay_intact(N, F):
    from guarded import guarded, padded_copy
    from mapx import vocab
    fields, fm, per_n = _case(F)
    rng = np.random.RandomState(N)
    cols, _ = per_n[257]
    cols = {n: c[:N] for n, c in cols.items()}
    want = V.apply(fm, cols, {n: (lambda v: str(int(v))) for n in cols})
    flags, ftypes, missing = [f % 2 for f in range(F)], [1 + f % 3 for f in range(F)], 7
    voc = vocab.Vocabulary(fields, device=DEV, flags=flags, field_types=ftypes, missing_type=missing)
    inputs = [padded_copy(torch.from_numpy(c).to(DEV)[None, :], ld=N + 9, col0=5, what=f"column {n}")
              for n, c in cols.items()]
    ld = F + 3 + int(rng.randint(1, 6))
    ids_view, ids_chk = guarded(N, F, torch.int64, ld=ld, col0=3, what="feat_ids")
    typ_view, typ_chk = guarded(N, F, torch.int64, ld=ld + 2, col0=3, what="type_ids")
    want_types = np.stack([np.where((c == -1) & bool(flags[j]), missing, ftypes[j]) for j, c in enumerate(cols.values())],
                          axis=1)
    assert (want_types == missing).any()
    for mode in (0, 1):
        ids_view.fill_(-77)
        typ_view.fill_(-77)
        ids, oov_rows, types = voc.encode([v[0] for v, _ in inputs], type_ids=True, feat_ids_out=ids_view,
                                          type_ids_out=typ_view, mode=mode)
        assert ids.data_ptr() == ids_view.data_ptr() and types.data_ptr() == typ_view.data_ptr()
        for chk in [ids_chk, typ_chk] + [c for _, c in inputs]:
            chk()
        assert np.array_equal(ids_view.cpu().numpy(), want) and np.array_equal(typ_view.cpu().numpy(), want_types)
        typ_view.fill_(-77)                                            # type_ids=False: the buffer is not touched
        ids_view.fill_(-77)
        ids, _ = voc.encode([v[0] for v, _ in inputs], feat_ids_out=ids_view, mode=mode)
        assert bool((typ_view == -77).all()) and np.array_equal(ids_view.cpu().numpy(), want)
        for chk in [ids_chk, typ_chk] + [c for _, c in inputs]:
            chk()


# ---------------------------------------------------------------- 5. errors
def test_int64_min_in_a_column_names_the_field():
    from mapx import vocab
    fields, fm, per_n = _case(25)
    voc = vocab.Vocabulary(fields, device=DEV)
    cols = {n: c.copy() for n, c in per_n[257][0].items()}
    cols["f17"][200] = I64_MIN
    cols["f21"][3] = I64_MIN
    with pytest.raises(ValueError, match="'f17'"):
        voc.encode(cols)
    ids, _ = voc.encode(per_n[257][0])                                 # the vocabulary is still good
    assert np.array_equal(ids.cpu().numpy(), per_n[257][1])
    with pytest.raises(ValueError, match="'f4'"):                      # ... and as a key of the vocabulary
        bad = list(fields)
        bad[4] = vocab.FieldKeys("f4", np.array([5, I64_MIN, 6]), fields[4].base)
        vocab.Vocabulary(bad[:5], device=DEV)


def test_duplicate_key_sets_the_load_entrys_error_words():
    from mapx.native import check, lib, ptr, stream
    i64 = dict(dtype=torch.int64, device=DEV)
    keys = torch.tensor([10, 11, 12, 20, 21, 20, 30], **i64)          # field 1 holds 20 twice
    key_off, tab_off = torch.tensor([0, 3, 6, 7], **i64), torch.tensor([0, 8, 16, 18], **i64)
    tkey, trank = torch.empty(18, **i64), torch.empty(18, dtype=torch.int32, device=DEV)
    err = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    check(lib.mapx_vocab_apply_load(ptr(keys), ptr(key_off), ptr(tab_off), 3, 7, 18, ptr(tkey), ptr(trank), ptr(err),
                                    stream()))
    assert err.tolist() == [4, 1]
    keys[5] = 22
    check(lib.mapx_vocab_apply_load(ptr(keys), ptr(key_off), ptr(tab_off), 3, 7, 18, ptr(tkey), ptr(trank), ptr(err),
                                    stream()))
    assert err.tolist() == [0, 2 ** 31 - 1]
    held = {(int(k), int(r)) for k, r in zip(tkey.tolist(), trank.tolist()) if k != I64_MIN}
    assert held == {(10, 0), (11, 1), (12, 2), (20, 0), (21, 1), (22, 2), (30, 0)}
    assert int((tkey[:8] != I64_MIN).sum()) == 3 and int((tkey[16:] != I64_MIN).sum()) == 1


def test_bad_capacities_are_refused_on_the_host():
    from mapx import vocab
    from mapx.native import lib
    fields = _case(2)[0] + []
    assert [len(f.keys) for f in fields] == [0, 1]
    for caps in ([2, 3], [2, 1], [0, 2], [2, 6], [2], [-4, 2]):
        with pytest.raises(ValueError):
            vocab.Vocabulary(fields, device=DEV, capacities=caps)
    assert [lib.mapx_vocab_apply_table_slots(n) for n in (0, 1, 2, 3, 1000, 1024, 1025)] == [2, 2, 4, 8, 2048, 2048, 4096]
    assert lib.mapx_vocab_apply_table_slots(-1) == 0 and lib.mapx_vocab_apply_table_slots(1 << 30) == 0


# ---------------------------------------------------------------- 6. properties at size
def test_two_million_rows_keep_the_lookup_properties():
    from mapx import vocab
    N, F = 2_000_000, 25
    rng = np.random.RandomState(23)
    counts = [int(c) for c in np.maximum(1, (480_000 * 0.62 ** np.arange(F))).astype(np.int64)]
    assert 1_150_000 < sum(counts) < 1_300_000
    fields, base = [], 10
    for f, n in enumerate(counts):
        keys = np.unique(rng.randint(0, 1 << 48, int(n * 1.1) + 8, dtype=np.int64))
        rng.shuffle(keys)
        fields.append(vocab.FieldKeys(f"f{f}", keys[:n], base))
        base = fields[-1].oov + 1
    voc = vocab.Vocabulary(fields, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    cols = []
    for f in fields:
        keys = torch.from_numpy(f.keys).to(DEV)
        rank = (torch.rand(N, generator=g, device=DEV) ** 4 * len(f.keys)).long().clamp_(max=len(f.keys) - 1)  # Zipf-like
        unseen = torch.randint(0, 1 << 48, (N,), generator=g, device=DEV, dtype=torch.int64)
        cols.append(torch.where(torch.rand(N, generator=g, device=DEV) < 0.7, keys[rank], unseen))
    ids, oov_rows = voc.encode(cols)
    for j, f in enumerate(fields):
        keys, raw, col = torch.from_numpy(f.keys).to(DEV), cols[j], ids[:, j]
        assert int(col.min()) >= f.base and int(col.max()) <= f.oov, j
        is_oov = col == f.oov
        assert torch.equal(keys[(col - f.base).clamp_(max=len(f.keys) - 1)][~is_oov], raw[~is_oov]), j
        assert not bool(torch.isin(raw[is_oov], keys).any()), j
        assert oov_rows[j] == int(is_oov.sum()) and 0.2 * N < oov_rows[j] < 0.4 * N, j
