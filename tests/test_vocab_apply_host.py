"""The host side of applying a saved vocabulary (mapx/vocab.py parse_meta, the --vocab mode of mapx/preprocess.py):
no GPU.  parse_meta is checked on the feat_map the reference's own scripts wrote for the committed raw files
(tests/golden/rawtext_*.npz): keys invert to codes that print back to the same strings, bases and <oov> ids are the
map's; then every error it promises, each naming its key or field; then the command line's argument cases."""
import copy
import json
import os

import numpy as np
import pytest

RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}


def _meta(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"rawtext_{name}.npz"))
    feat_map = {str(k): int(i) for k, i in zip(z["feat_map_keys"], z["feat_map_ids"].tolist())}
    return {"field_names": ["<rsv>"] + [str(n) for n in z["names"]][1:], "feat_map": feat_map}


def _rebuilt(meta, edit):
    """A copy of the meta whose feat_map items went through edit(list of [key, id]) -> list."""
    m = copy.deepcopy(meta)
    m["feat_map"] = dict(edit([[k, i] for k, i in meta["feat_map"].items()]))
    return m


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_parse_meta_inverts_the_reference_feat_map(golden_dir, name, tmp_path):
    from mapx import rawtext, vocab
    schema = rawtext.SCHEMAS[name]
    meta = _meta(golden_dir, name)
    fields = vocab.parse_meta(meta, schema)
    fm = meta["feat_map"]
    assert [f.name for f in fields] == schema.columns[1:] == meta["field_names"][1:]
    keys = list(fm)[:len(vocab.RESERVED)]
    for f in fields:
        assert f.keys.dtype == np.int64 and f.oov == fm[f"{f.name}-<oov>"] == f.base + len(f.keys)
        printed = schema.decoder(f.name)
        keys += [f"{f.name}-{printed(v)}" for v in f.keys.tolist()] + [f"{f.name}-<oov>"]
        if len(f.keys):
            assert fm[f"{f.name}-{printed(f.keys[0])}"] == f.base
        assert len(set(f.keys.tolist())) == len(f.keys) and -(1 << 63) not in f.keys.tolist()
    assert keys == list(fm)                                           # every key printed back, in id order
    assert fields[0].base == len(vocab.RESERVED) and fields[-1].oov + 1 == len(fm)
    assert any(-1 in f.keys.tolist() for f in fields) or name == "avazu"   # Criteo keeps the empty field ('-1')
    path = tmp_path / "m.json"
    path.write_text(json.dumps(meta))
    again = vocab.parse_meta(str(path), schema)                       # a path loads the same
    assert all(np.array_equal(a.keys, b.keys) and a.base == b.base for a, b in zip(fields, again))


def _first_key_of(meta, field, skip=0):
    return [k for k in meta["feat_map"] if k.startswith(field + "-") and not k.endswith("<oov>")][skip]


def test_parse_meta_errors_name_the_key_or_field(golden_dir, monkeypatch):
    from mapx import rawtext, vocab
    a, c = rawtext.AVAZU, rawtext.CRITEO
    ma, mc = _meta(golden_dir, "avazu"), _meta(golden_dir, "criteo")

    def fails(meta, schema, *words):
        with pytest.raises(ValueError) as e:
            vocab.parse_meta(meta, schema)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    # the first ten entries are not RESERVED
    fails(_rebuilt(ma, lambda it: [["<pad0>", 0]] + it[1:]), a, "reserved", "<pad0>")
    fails(_rebuilt(ma, lambda it: [[k, i - 10] for k, i in it[10:]]), a, "reserved")
    # the fields are not the schema's columns in order
    fails(dict(ma, field_names=ma["field_names"][:-1]), a, "field_names")
    fails(ma, c, "field_names")
    swapped = _rebuilt(ma, lambda it: (lambda w, d, rest: [[k, n] for n, (k, _) in enumerate(it[:10] + d + w + rest)])(
        [x for x in it if x[0].startswith("weekday-")], [x for x in it if x[0].startswith("day-")],
        [x for x in it[10:] if not x[0].startswith(("weekday-", "day-"))]))
    fails(swapped, a, "'weekday'", "day-")
    fails(_rebuilt(ma, lambda it: [[k, n] for n, (k, _) in enumerate(it + [["C99-7", 0], ["C99-<oov>", 0]])]), a, "C99-7")
    # a field's ids are not consecutive
    k = _first_key_of(ma, "site_id", 1)
    fails(_rebuilt(ma, lambda it: [[x, i + (x == k)] for x, i in it]), a, repr(k), "consecutive")
    fails(_rebuilt(ma, lambda it: [[x, i if x != k else float(i)] for x, i in it]), a, repr(k))
    # <name>-<oov> missing, or not the field's last id
    fails(_rebuilt(ma, lambda it: [[x, n] for n, (x, _) in enumerate(y for y in it if y[0] != "C14-<oov>")]), a,
          "'C14-<oov>'", "'C14'")

    def oov_first(it):
        run = [x for x in it if x[0].startswith("C1-")]
        at = it.index(run[0])
        moved = it[:at] + [run[-1]] + run[:-1] + it[at + len(run):]
        return [[x, n] for n, (x, _) in enumerate(moved)]
    assert len([x for x in ma["feat_map"] if x.startswith("C1-")]) > 2
    fails(_rebuilt(ma, oov_first), a, "'C1-<oov>'", "last")
    # a value does not invert
    k = _first_key_of(mc, "C3")
    fails(_rebuilt(mc, lambda it: [[x if x != k else "C3-68FD1E64", i] for x, i in it]), c, "'C3-68FD1E64'", "'C3'")
    fails(_rebuilt(mc, lambda it: [[x if x != k else "C3-", i] for x, i in it]), c, "'C3-'")
    k = _first_key_of(mc, "I5")
    for text in ("007", "+7", "7.0", "seven", str(1 << 63), ""):
        fails(_rebuilt(mc, lambda it: [[x if x != k else f"I5-{text}", i] for x, i in it]), c, repr(f"I5-{text}"), "'I5'")
    # two values of a field invert to one code ('0a' and 'a' once the width tag is dropped)
    k0, k1 = _first_key_of(mc, "C9", 0), _first_key_of(mc, "C9", 1)
    two = _rebuilt(mc, lambda it: [["C9-0a" if x == k0 else "C9-a" if x == k1 else x, i] for x, i in it])
    assert len(vocab.parse_meta(two, c)) == 39                        # different keys of the reference's Counter
    monkeypatch.setattr(rawtext, "encode_hex", lambda s: int(s, 16))
    fails(two, c, "'C9-0a'", "'C9-a'", "'C9'")


@pytest.mark.parametrize("case", ["neither", "both", "missing_vocab"])
def test_command_line_wants_exactly_one_of_n_core_and_vocab(golden_dir, tmp_path, case, capsys):
    from mapx import preprocess
    raw, out = os.path.join(golden_dir, RAW["avazu"]), str(tmp_path / "out")
    meta = tmp_path / "avazu-meta.json"
    meta.write_text(json.dumps(_meta(golden_dir, "avazu")))
    argv = ["--dataset", "avazu", "--raw", raw, "--out", out]
    argv += {"neither": [], "both": ["--n_core", "2", "--vocab", str(meta)],
             "missing_vocab": ["--vocab", str(tmp_path / "nothing-meta.json")]}[case]
    with pytest.raises(SystemExit) as e:
        preprocess.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "error" in err and ("--vocab" in err or "--n_core" in err)
    assert not (tmp_path / "out").exists()
