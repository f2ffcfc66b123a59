"""Growing a saved vocabulary on the GPU (mapx/vocab.py Vocabulary.grow and the --grow mode of mapx/preprocess.py over
csrc/vocab_grow.hip) and the table migration kernel (mapx/grow.py migrate_table) against the restatements of
tests/vocab_grow_ref.py (a Counter over the misses; numpy row gathers): the committed raw files through the command
line, synthetic columns around the wave and tile extents, guard bands and row pitches, and the errors.  Integer work
and pure copies: every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import rawtext_ref as R
import vocab_apply_ref as V
import vocab_grow_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64_MIN = -(1 << 63)
SPECIAL = [0, -1, 1 << 62, -(1 << 40)]


def _load(directory, name):
    with open(os.path.join(directory, f"{name}-meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(directory, f"{name}.npz"))


# ---------------------------------------------------------------- 1. the committed raw files
@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_committed_files_through_the_command_line(golden_dir, tmp_path, name, capsys):
    from mapx import preprocess, vocab
    from mapx.dataset import BaseDataset
    from mapx import rawtext
    schema, first, second, c1, c2, dec, fit_in_file_order = G.half_case(golden_dir, name, rawtext.SCHEMAS[name])
    F, fields_grown, added2, before, after, _ = G.FIGURES[name]
    p1, p2, a_dir, b_dir = tmp_path / "first.txt", tmp_path / "second.txt", str(tmp_path / "A"), str(tmp_path / "B")
    p1.write_bytes(first)
    p2.write_bytes(second)
    assert preprocess.main(["--dataset", name, "--raw", str(p1), "--n_core", "2", "--out", a_dir]) == 0
    a_meta = os.path.join(a_dir, f"{name}-meta.json")
    ma, _ = _load(a_dir, name)
    fm = ma["feat_map"]             # (tests/test_rawtext_gpu.py pins the fit; Avazu's shuffles its rows, so ties rank otherwise)
    assert sorted(fm) == sorted(fit_in_file_order) and len(fm) == len(fit_in_file_order)
    if not schema.shuffle:
        assert list(fm.items()) == list(fit_in_file_order.items())
    capsys.readouterr()
    assert preprocess.main(["--dataset", name, "--raw", str(p2), "--vocab", a_meta, "--grow", "2", "--out", b_dir,
                            "--chunk_mb", "1", "--split", "0.8,0.1,0.1"]) == 0
    said = capsys.readouterr().out
    want_map, want_added = G.grow(fm, c2, dec, 2)
    want_ids = V.apply(want_map, c2, dec)
    labels, _ = R.parse(second, schema)
    mb, tb = _load(b_dir, name)
    assert list(mb["feat_map"].items()) == list(want_map.items())
    assert np.array_equal(tb["feat_ids"], want_ids) and np.array_equal(tb["labels"], labels)
    assert mb["grown"] == want_added and list(mb["grown"]) == list(c2)
    assert sum(1 for a in mb["grown"].values() if a) == fields_grown and sum(mb["grown"].values()) == added2
    oov_ids = [want_map[f"{n}-<oov>"] for n in c2]
    assert list(mb["oov_rows"].values()) == [int((want_ids[:, j] == o).sum()) for j, o in enumerate(oov_ids)]
    assert sum(mb["oov_rows"].values()) == after and mb["index"] == list(range(len(labels)))
    for key in ("field_names", "field_map", "feat_type_map"):
        assert mb[key] == ma[key] and list(mb[key]) == list(ma[key]), key
    assert f"input_size {len(fm)} -> {len(want_map)}" in said and f"{added2} keys added" in said
    top = sorted(want_added.items(), key=lambda x: -x[1])[:3]
    assert ", ".join(f"{n} +{a}" for n, a in top) in said
    # type_ids as --vocab mode writes them
    t_oov = ma["feat_type_map"]["<oov>"]
    for j, n in enumerate(c2):
        plain = ma["feat_type_map"][schema.feat_types[n]]
        missing = np.zeros(len(labels), dtype=bool) if n in schema.string_columns else c2[n] == -1
        assert np.array_equal(tb["type_ids"][:, j], np.where(missing, t_oov, plain)), n
    # any chunking gives the same files
    for chunk_bytes in (None, 700):
        c_dir = str(tmp_path / f"C{chunk_bytes}")
        mc, input_size = vocab.grow_dataset_from_text(str(p2), schema, a_meta, 2, c_dir, name, chunk_bytes=chunk_bytes)
        _, tc = _load(c_dir, name)
        assert input_size == len(want_map) and list(mc["feat_map"].items()) == list(want_map.items())
        assert mc["grown"] == mb["grown"] and mc["oov_rows"] == mb["oov_rows"]
        for what in ("feat_ids", "labels", "type_ids", "field_ids"):
            assert np.array_equal(tc[what], tb[what]), what
    # the grown meta is a vocabulary like any other, and the directory a dataset
    voc = vocab.Vocabulary.from_meta(os.path.join(b_dir, f"{name}-meta.json"), schema)
    assert voc.input_size == len(want_map) and [f.oov for f in voc.fields] == oov_ids
    ids, oov_rows = voc.encode(c2)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and oov_rows == list(mb["oov_rows"].values())

    class Args:
        data_dir, dataset_name, pretrain, pt_type, RFD_replace = b_dir, name, True, "MFP", "Unigram"
    ds = BaseDataset(Args())
    assert ds.get_splited_dataset("train").X.shape == (int(len(labels) * 0.8), F) and ds.feat_map == want_map
    # the file the vocabulary was fitted on, the same n_core: nothing to add
    d_dir = str(tmp_path / "D")
    md, input_size = vocab.grow_dataset_from_text(str(p1), schema, a_meta, 2, d_dir, name)
    assert input_size == len(fm) and sum(md["grown"].values()) == 0
    assert list(md["feat_map"].items()) == list(ma["feat_map"].items())
    # n_core 1 leaves no <oov> cell
    e_dir = str(tmp_path / "E")
    me, _ = vocab.grow_dataset_from_text(str(p2), schema, a_meta, 1, e_dir, name)
    assert sum(me["grown"].values()) == G.FIGURES[name][5] and sum(me["oov_rows"].values()) == 0
    assert list(me["feat_map"].items()) == list(G.grow(fm, c2, dec, 1)[0].items())


# ---------------------------------------------------------------- 2. count_missing against the restatement
SIZES = (0, 1, 63, 64, 65, 257, 5000)
KEY_COUNTS = (0, 1, 1000)
_UNIVERSE = []


def _universe():
    if not _UNIVERSE:
        rng = np.random.RandomState(11)
        u = np.unique(np.concatenate([rng.randint(-(1 << 40), 1 << 40, 6000, dtype=np.int64),
                                      rng.randint(1 << 61, 1 << 62, 500, dtype=np.int64)]))
        u = u[~np.isin(u, SPECIAL)]
        rng.shuffle(u)
        _UNIVERSE.append(u)
    return _UNIVERSE[0]


def _saved_fields():
    """Six fields of 0, 1, 1000, 0, 1, 1000 keys: the special values rotated by the field, then a window of the shared
    universe (the two large fields share the special values only)."""
    from mapx import vocab
    u, fields, base = _universe(), [], len(vocab.RESERVED)
    for f in range(6):
        n = KEY_COUNTS[f % 3]
        special = (SPECIAL[f % 4:] + SPECIAL[:f % 4])[:n]
        keys = np.array(special + u[500 * f:500 * f + n - len(special)].tolist(), dtype=np.int64)
        fields.append(vocab.FieldKeys(f"f{f}", keys, base))
        base = fields[-1].oov + 1
    assert len(np.intersect1d(fields[2].keys, fields[5].keys)) == len(SPECIAL)
    return fields


def _feat_map(fields):
    fm = {tok: i for i, tok in enumerate(G.RESERVED)}
    for f in fields:
        for v in f.keys.tolist():
            fm[f"{f.name}-{v}"] = len(fm)
        fm[f"{f.name}-<oov>"] = len(fm)
    return fm


def _columns(kind, N, fields, rng):
    u, cols = _universe(), {}
    unseen = u[3500:]                                                   # behind every field's window
    for j, f in enumerate(fields):
        if kind == "mixed":
            c = np.where(rng.rand(N) < 0.25, rng.choice(np.array(SPECIAL, dtype=np.int64), N), u[rng.randint(0, len(u), N)])
            if len(f.keys):
                c = np.where(rng.rand(N) < 0.4, f.keys[rng.randint(0, len(f.keys), N)], c)
            c = np.where(rng.rand(N) < 0.3, unseen[(rng.zipf(1.5, N) - 1) % 40], c)     # a few frequent misses
        elif kind == "all_missing":
            c = unseen[rng.randint(0, 300, N)]
        elif kind == "none_missing":                                    # (a field without keys cannot hit)
            c = f.keys[rng.randint(0, len(f.keys), N)] if len(f.keys) else unseen[rng.randint(0, 5, N)]
        elif kind == "other_fields_key":                                # values another field keeps and this one does not
            other = (fields[5] if j == 2 else fields[2]).keys
            other = other[~np.isin(other, f.keys)]
            c = np.where(rng.rand(N) < 0.7, other[rng.randint(0, 60, N)], unseen[rng.randint(0, 50, N)])
        elif kind == "ties":                                            # every value equally often: first occurrence ranks
            distinct = max(1, N // 3)
            c = unseen[rng.permutation(distinct)][np.arange(N) % distinct]
        elif kind == "one_hot":
            c = np.full(N, unseen[7 + j])
        cols[f.name] = c.astype(np.int64)
    return cols


def _tight(n):
    return 1 << int(n).bit_length()


@pytest.mark.parametrize("capacities", ["default", "tight"])
@pytest.mark.parametrize("kind", ["mixed", "all_missing", "none_missing", "other_fields_key", "ties", "one_hot"])
def test_count_missing_against_the_restatement(kind, capacities):
    from mapx import vocab
    fields = _saved_fields()
    fm = _feat_map(fields)
    dec = {f.name: (lambda v: str(int(v))) for f in fields}
    voc = vocab.Vocabulary(fields, device=DEV,
                           capacities=[_tight(len(f.keys)) for f in fields] if capacities == "tight" else None)
    rng = np.random.RandomState(len(kind))
    for N in SIZES:
        cols = _columns(kind, N, fields, rng)
        before = [int(sum(1 for v in c.tolist() if f"{n}-{v}" not in fm)) for n, c in cols.items()]
        if kind == "all_missing":
            assert before == [N] * len(fields)
        if kind == "none_missing":
            assert before == [0 if len(f.keys) else N for f in fields]
        for n_core in ((1, 2, 3) if N <= 257 else (2,)):
            want_map, want_added = G.grow(fm, cols, dec, n_core)
            count_caps = None
            if capacities == "tight":                                   # the smallest power of two above the distinct misses
                count_caps = [max(64, _tight(len({v for v in c.tolist() if f"{n}-{v}" not in fm})))
                              for n, c in cols.items()]
            grown, added, miss_before, miss_after = voc.grow(cols, n_core, capacities=count_caps)
            assert list(grown.feat_map.items()) == list(want_map.items()), (N, n_core)
            assert added == list(want_added.values()) and miss_before == before, (N, n_core)
            assert miss_after == [int(sum(1 for v in c.tolist() if f"{n}-{v}" not in want_map)) for n, c in cols.items()]
            assert grown.input_size == len(want_map)
            ids, oov_rows = grown.encode(cols)                          # the grown tables look the added keys up
            assert np.array_equal(ids.cpu().numpy(), V.apply(want_map, cols, dec)) and oov_rows == miss_after
        dev_cols = [torch.from_numpy(c).to(DEV) for c in cols.values()]  # device columns, a second run: the same
        again = voc.grow(dev_cols, 2)
        ref = voc.grow(cols, 2)
        assert list(again[0].feat_map.items()) == list(ref[0].feat_map.items()) and again[1:] == ref[1:]


def test_growing_nothing_keeps_the_items_and_a_fitted_vocabulary_grows_too():
    from mapx import vocab
    rng = np.random.RandomState(2)
    cols = {"a": rng.randint(0, 40, 700).astype(np.int64), "b": rng.randint(-5, 5, 700).astype(np.int64)}
    _, fitted, fm, _ = vocab.build_vocab(cols, 3, device=DEV)
    voc = vocab.Vocabulary(fitted, device=DEV)                          # FieldVocab: keys on the device
    dec = {n: (lambda v: str(int(v))) for n in cols}
    same, added, before, after = voc.grow(cols, 3)
    assert added == [0, 0] and list(same.feat_map.items()) == list(fm.items()) and before == after
    later = {"a": rng.randint(30, 80, 500).astype(np.int64), "b": rng.randint(-9, 9, 500).astype(np.int64)}
    grown, added, before, after = voc.grow(later, 2)
    want_map, want_added = G.grow(fm, later, dec, 2)
    assert list(grown.feat_map.items()) == list(want_map.items()) and added == list(want_added.values())
    assert sum(before) == G.oov_cells(fm, later, dec) and sum(after) == G.oov_cells(want_map, later, dec)


# ---------------------------------------------------------------- 3. table_migrate against the numpy restatement
def _plan(F, seed):
    """A random growth plan of F fields: some without old keys, some without added ones."""
    from mapx import grow
    rng = np.random.RandomState(seed)
    fields, b_old, b_new = [], 10, 10
    for f in range(F):
        n = int(rng.choice([0, 1, 2, 7, 40])) if F > 1 else 7
        a = int(rng.choice([0, 0, 1, 3, 11])) if F > 1 else 5
        if f == 0 and F > 1:
            n, a = 0, 2
        if f == 1:
            n, a = 5, 0
        fields.append(grow.FieldPlan(f"f{f}", n, a, b_old, b_new))
        b_old, b_new = b_old + n + 1, b_new + n + a + 1
    return grow.Plan(fields, b_old, b_new, 10)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("F", [1, 2, 25, 64])
@pytest.mark.parametrize("W", [1, 4, 16, 32, 36])
def test_table_migrate_against_the_restatement(W, F):
    from guarded import guarded, padded_copy
    from mapx import grow
    p = _plan(F, 10 * F + W)
    assert p.added_total > 0 and p.V_new == p.V_old + p.added_total
    if F > 2:
        assert any(f.n_old == 0 for f in p.fields) and any(f.added == 0 for f in p.fields)
    g = torch.Generator().manual_seed(W * 100 + F)
    src = torch.randn(p.V_old, W, generator=g)
    fresh = torch.randn(p.added_total, W, generator=g)
    want = torch.from_numpy(G.migrate(src.numpy(), p)).to(DEV)
    want_fresh = torch.from_numpy(G.migrate(src.numpy(), p, fresh.numpy())).to(DEV)
    d_src, d_fresh = src.to(DEV), fresh.to(DEV)
    # contiguous operands: the 16-byte path where W % 4 == 0
    out = grow.migrate_table(d_src, p)
    assert out.shape == (p.V_new, W) and torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(grow.migrate_table(d_src, p)), _bits(out))              # a second call: the same bits
    assert torch.equal(_bits(grow.migrate_table(d_src, p, fresh=d_fresh)), _bits(want_fresh))
    # a source base 4 bytes off a 16-byte boundary: single elements
    flat = torch.empty(p.V_old * W + 1, device=DEV)
    off = flat[1:].view(p.V_old, W)
    off.copy_(d_src)
    assert off.data_ptr() % 16 == 4
    assert torch.equal(_bits(grow.migrate_table(off, p)), _bits(want))
    assert torch.equal(_bits(grow.migrate_table(off, p, fresh=d_fresh)), _bits(want_fresh))
    # guard bands and row pitches: a pitch that keeps rows 16-byte aligned, and one that does not
    for pad, col0 in ((8, 4), (3, 1)):
        s_view, s_chk = padded_copy(d_src, ld=W + pad, col0=col0, what="src")
        f_view, f_chk = padded_copy(d_fresh, ld=W + pad + 4, col0=col0, what="fresh")
        o_view, o_chk = guarded(p.V_new, W, torch.float32, ld=W + pad, col0=col0, what="dst")
        for fr, expect in ((None, want), (f_view, want_fresh)):
            o_view.fill_(-77.0)
            got = grow.migrate_table(s_view, p, fresh=fr, out=o_view)
            assert got.data_ptr() == o_view.data_ptr()
            for chk in (s_chk, f_chk, o_chk):
                chk()
            assert torch.equal(_bits(o_view), _bits(expect)), (pad, fr is None)
    # the identity plan reproduces the source
    ident = grow.Plan([f._replace(added=0, base_new=f.base_old) for f in p.fields], p.V_old, p.V_old, 10)
    assert torch.equal(_bits(grow.migrate_table(d_src, ident)), _bits(d_src))


def test_table_migrate_fills_more_than_one_grid_pass():
    """V large enough that every lane loops (more rows than the capped grid covers at once) and the 4-row unroll has
    a ragged tail; W = 16 and W = 1."""
    from mapx import grow
    rng = np.random.RandomState(4)
    fields, b_old, b_new = [], 10, 10
    for f in range(25):
        n, a = int(rng.randint(20000, 40000)), int(rng.randint(0, 400))
        fields.append(grow.FieldPlan(f"f{f}", n, a, b_old, b_new))
        b_old, b_new = b_old + n + 1, b_new + n + a + 1
    p = grow.Plan(fields, b_old, b_new, 10)
    # one pass of the grid covers 4 rows x (blocks x 256 threads / lanes per row): csrc/common.h grid_for caps the
    # blocks at 2048, and a W = 16 row takes 4 lanes (16-byte chunks; csrc/vocab_grow.hip).  If either changes, size
    # the plan anew so that the rows still exceed one pass.
    assert p.V_new > 4 * (2048 * 256 // 4)
    src_rows = torch.from_numpy(G.src_rows(p)).to(DEV)
    for W in (16, 1):
        src = torch.randn(p.V_old, W, device=DEV)
        out = grow.migrate_table(src, p)
        assert torch.equal(_bits(out), _bits(src.index_select(0, src_rows)))


def test_a_plan_that_leaves_the_source_table_is_refused():
    """The kernel computes its source rows: one outside the table is not read (the row is zeroed) and raises."""
    from mapx import grow
    from mapx.native import MapxError
    p = _plan(2, 1)
    short = p._replace(V_old=p.V_old - 1)                               # the last field's <oov> row is not there
    with pytest.raises(MapxError, match="outside"):
        grow.migrate_table(torch.zeros(short.V_old, 4, device=DEV), short)
    with pytest.raises(TypeError):
        grow.migrate_table(torch.zeros(p.V_old + 1, 4, device=DEV), p)
    with pytest.raises(TypeError):
        grow.migrate_table(torch.zeros(p.V_old, 4, device=DEV), p, fresh=torch.zeros(p.added_total + 1, 4, device=DEV))


# ---------------------------------------------------------------- 4. errors
def test_int64_min_in_a_column_names_the_field():
    from mapx import vocab
    fields = _saved_fields()
    voc = vocab.Vocabulary(fields, device=DEV)
    cols = _columns("mixed", 257, fields, np.random.RandomState(0))
    good = {n: c.copy() for n, c in cols.items()}
    cols["f3"][200] = I64_MIN
    cols["f5"][3] = I64_MIN
    with pytest.raises(ValueError, match="'f3'"):
        voc.grow(cols, 2)
    fm = _feat_map(fields)
    dec = {f.name: (lambda v: str(int(v))) for f in fields}
    assert list(voc.grow(good, 2)[0].feat_map.items()) == list(G.grow(fm, good, dec, 2)[0].items())
    with pytest.raises(ValueError, match="columns"):
        voc.grow(list(good.values())[:-1], 2)


def test_grow_without_vocab_is_refused_by_the_parser(golden_dir, tmp_path, capsys):
    from mapx import preprocess
    raw, out = os.path.join(golden_dir, "raw_avazu.csv"), str(tmp_path / "out")
    for argv in (["--n_core", "2", "--grow", "2"], ["--grow", "2"], ["--vocab", raw, "--grow", "0"]):
        with pytest.raises(SystemExit) as e:
            preprocess.main(["--dataset", "avazu", "--raw", raw, "--out", out] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "error" in err and ("--grow" in err or "--vocab" in err or "--n_core" in err)
    assert not (tmp_path / "out").exists()
