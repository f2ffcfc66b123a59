"""The host side of growing a vocabulary (mapx/grow.py: plan, remap_ids, migrate_state_dict's key / shape rule) and the
restatement tests/vocab_grow_ref.py on the committed raw files: no GPU.  The plan is pure arithmetic over two metas and
is checked on hand-written ones; every refusal must name its key; the figures of the committed files come from the
restatement alone (a Counter over the misses) and are what the GPU tests then hold the device path to."""
import copy
import os

import numpy as np
import pytest
import torch

import vocab_grow_ref as G


def make_meta(spec):
    """spec: [(field name, [value strings])] -> a meta dict with the reserved tokens, the keys and one <oov> per field."""
    fm = {k: i for i, k in enumerate(G.RESERVED)}
    for name, values in spec:
        for v in values:
            fm[f"{name}-{v}"] = len(fm)
        fm[f"{name}-<oov>"] = len(fm)
    return {"field_names": ["<rsv>"] + [n for n, _ in spec], "feat_map": fm}


def grown_pair(old_spec, extra):
    """-> (old meta, new meta) with extra[f] values appended to field f."""
    return make_meta(old_spec), make_meta([(n, v + list(extra.get(n, []))) for n, v in old_spec])


def check_plan(p, old, new, old_spec, extra):
    assert p.V_old == len(old["feat_map"]) and p.V_new == len(new["feat_map"]) and p.reserved == 10
    assert [f.name for f in p.fields] == [n for n, _ in old_spec]
    base_old = base_new = 10
    for f, (name, values) in zip(p.fields, old_spec):
        a = len(extra.get(name, []))
        assert (f.n_old, f.added, f.base_old, f.base_new) == (len(values), a, base_old, base_new), name
        assert old["feat_map"][f"{name}-<oov>"] == f.base_old + f.n_old
        assert new["feat_map"][f"{name}-<oov>"] == f.base_new + f.n_old + f.added
        base_old += len(values) + 1
        base_new += len(values) + a + 1
    assert p.added_total == sum(len(v) for v in extra.values()) == p.V_new - p.V_old
    # every old key reads its old row, every added key and the new <oov> the old <oov>
    src = G.src_rows(p)
    for key, i in new["feat_map"].items():
        name = key.rsplit("-", 1)[0] if key not in G.RESERVED else None
        want = old["feat_map"].get(key, old["feat_map"].get(f"{name}-<oov>"))
        assert src[i] == want, key


SPEC3 = [("a", ["1", "2", "3"]), ("b", []), ("c", ["x", "y"])]


@pytest.mark.parametrize("extra", [{}, {"a": ["9"]}, {"c": ["z", "w"]}, {"b": ["5", "6", "7"]},
                                   {"a": ["7", "8"], "b": ["0"], "c": ["q"]}],
                         ids=["nothing", "first", "last", "empty_field", "all"])
def test_plan_arithmetic_on_hand_written_metas(extra):
    from mapx import grow
    old, new = grown_pair(SPEC3, extra)
    p = grow.plan(old, new)
    check_plan(p, old, new, SPEC3, extra)
    if not extra:
        assert p == grow.identity_plan(old) and np.array_equal(G.src_rows(p), np.arange(p.V_old))


@pytest.mark.parametrize("F", [1, 64])
def test_plan_of_one_and_of_sixty_four_fields(F, tmp_path):
    import json
    from mapx import grow
    spec = [(f"f{j}", [str(v) for v in range(j % 4)]) for j in range(F)]
    extra = {f"f{j}": [str(100 + v) for v in range((j * 7) % 3)] for j in range(F) if (j * 7) % 3}
    if F == 1:
        extra = {"f0": ["100", "101"]}
    old, new = grown_pair(spec, extra)
    check_plan(grow.plan(old, new), old, new, spec, extra)
    (tmp_path / "o.json").write_text(json.dumps(old))
    (tmp_path / "n.json").write_text(json.dumps(new))
    assert grow.plan(str(tmp_path / "o.json"), str(tmp_path / "n.json")) == grow.plan(old, new)   # paths load the same


def test_every_refusal_names_its_key():
    from mapx import grow
    old, new = grown_pair(SPEC3, {"a": ["9"], "c": ["z"]})

    def fails(o, n, *words):
        with pytest.raises(ValueError) as e:
            grow.plan(o, n)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def rebuilt(meta, keys):
        return {"field_names": list(meta["field_names"]), "feat_map": {k: i for i, k in enumerate(keys)}}
    keys = list(new["feat_map"])
    # an old key missing from the new map
    fails(old, rebuilt(new, [k for k in keys if k != "a-2"]), "'a-2'", "missing")
    # an old key out of order (behind an added one; two old keys swapped)
    moved = [k for k in keys if k != "a-3"]
    moved.insert(moved.index("a-9") + 1, "a-3")
    fails(old, rebuilt(new, moved), "'a-3'", "order")
    swapped = list(keys)
    i, j = swapped.index("c-x"), swapped.index("c-y")
    swapped[i], swapped[j] = swapped[j], swapped[i]
    fails(old, rebuilt(new, swapped), "'c-x'", "order")
    # <oov> not the last id of its field, in the new and in the old meta
    early = [k for k in keys if k != "a-<oov>"]
    early.insert(early.index("a-9"), "a-<oov>")
    fails(old, rebuilt(new, early), "'a-<oov>'", "last")
    fails(rebuilt(old, [k for k in old["feat_map"] if k != "b-<oov>"]), new, "'b-<oov>'")
    # other field_names
    other = copy.deepcopy(new)
    other["field_names"][2] = "B"
    fails(old, other, "field_names", "'b'", "'B'")
    fails(old, dict(new, field_names=new["field_names"][:-1]), "field_names", "'c'")
    # ids that are not the positions; a key of no field; other reserved tokens
    gap = copy.deepcopy(new)
    gap["feat_map"]["c-z"] += 1
    fails(old, gap, "'c-z'", "consecutive")
    fails(old, rebuilt(new, keys + ["d-1"]), "'d-1'")
    fails(old, rebuilt(new, ["<PAD>"] + keys[1:]), "reserved")
    # shrinking is not growing
    fails(new, old, "'a-9'", "missing")


def test_plan_with_a_schema_checks_the_values(golden_dir):
    from mapx import grow, rawtext
    z = np.load(os.path.join(golden_dir, "rawtext_avazu.npz"))
    fm = {str(k): int(i) for k, i in zip(z["feat_map_keys"], z["feat_map_ids"].tolist())}
    meta = {"field_names": ["<rsv>"] + [str(n) for n in z["names"]][1:], "feat_map": fm}
    p = grow.plan(meta, meta, rawtext.AVAZU)
    assert p.added_total == 0 and p.V_old == p.V_new == len(fm) and len(p.fields) == 25
    keys = list(fm)
    at = keys.index("site_id-<oov>")
    bad = {"field_names": meta["field_names"], "feat_map": {k: i for i, k in enumerate(keys[:at] + ["site_id-XYZ"] + keys[at:])}}
    assert grow.plan(meta, bad).added_total == 1                       # a growth as far as the strings go ...
    with pytest.raises(ValueError, match="'site_id-XYZ'"):             # ... but no value of the hash-string column
        grow.plan(meta, bad, rawtext.AVAZU)


def test_remap_ids_against_the_source_rows():
    from mapx import grow
    old, new = grown_pair(SPEC3, {"a": ["7", "8"], "b": ["0"], "c": ["q"]})
    p = grow.plan(old, new)
    src = G.src_rows(p)
    rng = np.random.RandomState(3)
    ids = np.stack([rng.randint(f.base_old, f.base_old + f.n_old + 1, 200) for f in p.fields], axis=1).astype(np.int64)
    ids[5, 1] = 3                                                      # a reserved id (<mask>) stays
    got = grow.remap_ids(ids, p)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == ids.shape
    assert np.array_equal(src[got], ids)                               # the new row reads the old row ...
    for j, f in enumerate(p.fields):                                   # ... and is the old key's own new id
        old_oov = ids[:, j] == f.base_old + f.n_old
        assert np.array_equal(got[old_oov, j], np.full(int(old_oov.sum()), f.base_new + f.n_old + f.added))
        keep = ~old_oov & (ids[:, j] >= 10)
        assert np.array_equal(got[keep, j] - f.base_new, ids[keep, j] - f.base_old)
    assert got[5, 1] == 3
    assert torch.equal(grow.remap_ids(torch.from_numpy(ids), p), torch.from_numpy(got))
    assert np.array_equal(grow.remap_ids(ids, grow.identity_plan(old)), ids)
    wrong = ids.copy()
    wrong[7, 2] = p.fields[0].base_old                                 # an id of field a in column c
    with pytest.raises(ValueError, match="'c'"):
        grow.remap_ids(wrong, p)


def test_migrate_state_dict_goes_by_key_then_shape(monkeypatch):
    """The kernel call is stubbed by the numpy restatement: which tensors move, which are dropped, which stay."""
    from mapx import grow
    old, new = grown_pair(SPEC3, {"a": ["7", "8"], "c": ["q"]})
    p = grow.plan(old, new)
    V, A = p.V_old, p.added_total
    calls = []

    def stub(src, plan_, fresh=None, out=None):
        calls.append((tuple(src.shape), None if fresh is None else tuple(fresh.shape)))
        return torch.from_numpy(G.migrate(src.numpy(), plan_, None if fresh is None else fresh.numpy()))
    monkeypatch.setattr(grow, "migrate_table", stub)
    g = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.randn(*shape, generator=g)
    sd = {"embed.embedding.weight": r(V, 16), "lr_layer.embed_w.weight": r(V, 1),
          "fg_embed.embedding.weight": r(V, 4),
          "parallel_dnn.dnn.0.weight": r(V, 12),                      # a dense weight of V_old rows: not a table
          "parallel_dnn.dnn.0.bias": r(V), "fc_out.weight": r(1, V + 12),
          "mfp_criterion.emb.weight": r(V, 32), "mfp_criterion.bias.weight": r(V, 1),
          "mfp_criterion.logprob_noise": r(V), "mfp_criterion.alias.prob": r(V),
          "mfp_criterion.alias.alias": torch.arange(V)}
    out, report = grow.migrate_state_dict(sd, p, device="cpu")
    tables = ["embed.embedding.weight", "lr_layer.embed_w.weight", "fg_embed.embedding.weight",
              "mfp_criterion.emb.weight", "mfp_criterion.bias.weight"]
    dropped = ["mfp_criterion.logprob_noise", "mfp_criterion.alias.prob", "mfp_criterion.alias.alias"]
    assert list(report["tables"]) == tables and report["dropped"] == dropped and report["kept"] == 3
    assert report["added"] == A and report["tables"]["lr_layer.embed_w.weight"] == [V, p.V_new, 1]
    assert list(out) == [k for k in sd if k not in dropped]
    for k in tables:
        assert out[k].shape == (p.V_new, sd[k].shape[1]) and np.array_equal(out[k].numpy(), G.migrate(sd[k].numpy(), p)), k
    for k in ("parallel_dnn.dnn.0.weight", "parallel_dnn.dnn.0.bias", "fc_out.weight"):
        assert out[k] is sd[k], k
    assert len(calls) == len(tables) and all(f is None for _, f in calls)
    # normal:STD: one generator, the tables in the state dict's order
    out2, _ = grow.migrate_state_dict(sd, p, init="normal:0.5", seed=9, device="cpu")
    g2 = torch.Generator().manual_seed(9)
    for k in tables:
        fresh = torch.empty(A, sd[k].shape[1]).normal_(0.0, 0.5, generator=g2)
        assert np.array_equal(out2[k].numpy(), G.migrate(sd[k].numpy(), p, fresh.numpy())), k
    # a table key of another shape or type raises, naming the key
    for key, t in (("embed.embedding.weight", r(V + 1, 16)), ("mfp_criterion.bias.weight", r(V)),
                   ("lr_layer.embed_w.weight", r(V, 1).double())):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            grow.migrate_state_dict(dict(sd, **{key: t}), p, device="cpu")
    for bad in ("normal", "normal:0", "normal:x", "uniform:1", "normal:-1"):
        with pytest.raises(ValueError, match="init"):
            grow.migrate_state_dict(sd, p, init=bad, device="cpu")


def test_tables_on_the_host_are_refused():
    from mapx import grow
    from mapx.native import MapxError
    p = grow.identity_plan(make_meta(SPEC3))
    with pytest.raises(MapxError):
        grow.migrate_table(torch.zeros(p.V_old, 4), p)


# ---------------------------------------------------------------- the committed raw files, from the restatement alone
@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_restatement_on_the_committed_raw_files(golden_dir, name):
    import vocab_apply_ref as V
    from oracle import vocab as oracle_vocab
    from mapx import grow
    from mapx import rawtext
    schema, _first, _second, c1, c2, dec, fm = G.half_case(golden_dir, name, rawtext.SCHEMAS[name])
    F, fields_grown, added2, before, after, added1 = G.FIGURES[name]
    # the fit as a growth of the empty vocabulary is the reference's rule on printed values
    printed = {n: [dec[n](v) for v in c.tolist()] for n, c in c1.items()}
    assert list(fm.items()) == list(oracle_vocab.build_feat_map(printed, 2)[0].items())
    g2, a2 = G.grow(fm, c2, dec, 2)
    assert len(a2) == F and sum(1 for a in a2.values() if a) == fields_grown and sum(a2.values()) == added2
    assert G.oov_cells(fm, c2, dec) == before and G.oov_cells(g2, c2, dec) == after
    assert len(g2) == len(fm) + added2
    g1, a1 = G.grow(fm, c2, dec, 1)
    assert sum(a1.values()) == added1 and G.oov_cells(g1, c2, dec) == 0
    same, a0 = G.grow(fm, c1, dec, 2)                                 # the file it was fitted on adds nothing
    assert sum(a0.values()) == 0 and list(same.items()) == list(fm.items())
    # the plan between the two maps, and the ids of the second half under both
    meta = lambda m: {"field_names": ["<rsv>"] + list(c2), "feat_map": m}
    p = grow.plan(meta(fm), meta(g2), schema)
    assert [f.added for f in p.fields] == list(a2.values()) and (p.V_old, p.V_new) == (len(fm), len(g2))
    old_ids, new_ids = V.apply(fm, c2, dec), V.apply(g2, c2, dec)
    assert np.array_equal(G.src_rows(p)[new_ids], old_ids)            # what makes init=oov function-preserving
    remapped = grow.remap_ids(old_ids, p)
    oov_old = np.array([f.base_old + f.n_old for f in p.fields])
    assert np.array_equal(remapped[old_ids != oov_old], new_ids[old_ids != oov_old])
    assert int((old_ids == oov_old).sum()) == before and int((remapped != new_ids).sum()) == before - after
