"""Checkpoints carried over to a grown vocabulary (mapx/grow.py over csrc/vocab_grow.hip) on small models: F = 25,
E = 16, batch 64, the vocabulary fitted on the first half of the committed Avazu file (341 ids) and grown on the second
(396 ids).  init=oov must preserve the function bit for bit; a pretraining checkpoint must load without a skipped table
and train on; normal:STD must touch the added rows only; the command line must do what the functions do."""
import json
import os

import numpy as np
import pytest
import torch

import vocab_apply_ref as V
import vocab_grow_ref as G
from util import make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "avazu"
B = 64
TABLES = ("embed.embedding.weight", "lr_layer.embed_w.weight", "mfp_criterion.emb.weight", "mfp_criterion.bias.weight")
NOISE = ("mfp_criterion.logprob_noise", "mfp_criterion.alias.prob", "mfp_criterion.alias.alias")
_CASE = {}


def _case(golden_dir):
    """The two vocabularies, their plan, and both halves' ids under both — all from the restatements."""
    if not _CASE:
        from mapx import grow, rawtext
        schema, first, second, c1, c2, dec, fm = G.half_case(golden_dir, NAME, rawtext.SCHEMAS[NAME])
        gm, added = G.grow(fm, c2, dec, 2)
        meta = lambda m: {"field_names": ["<rsv>"] + list(c2), "feat_map": m}
        plan = grow.plan(meta(fm), meta(gm), schema)
        _CASE.update(schema=schema, first=first, second=second, c1=c1, c2=c2, dec=dec, fm=fm, gm=gm, plan=plan,
                     meta_old=meta(fm), meta_new=meta(gm), old_ids=V.apply(fm, c2, dec), new_ids=V.apply(gm, c2, dec),
                     oov_old=[fm[f"{n}-<oov>"] for n in c2], oov_new=[gm[f"{n}-<oov>"] for n in c2])
        assert (plan.V_old, plan.V_new) == (341, 396)
    return _CASE


def _cfg(V_):
    return dict(F=25, V=V_, E=16, H=64, NL=3, NC=3, P=32, K=25)


def _randomise(model, seed):
    """Every floating tensor of the state dict drawn anew (TableWeight allocates without initialising)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, t in model.state_dict().items():
            if t.is_floating_point() and not k.startswith("mfp_criterion.") or k in TABLES:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("backbone,compute_dtype", [("DCNv2", "fp32"), ("DCNv2", "bf16"), ("DeepFM", "fp32")])
def test_init_oov_preserves_the_function_bit_for_bit(golden_dir, tmp_path, backbone, compute_dtype):
    """The second half encoded with the old vocabulary through the old tables, and with the grown vocabulary through
    the migrated tables: the same file order and batch size, so the same batch mates and per-batch magnitudes."""
    from mapx import grow, score
    from mapx.models import build_backbone
    c = _case(golden_dir)
    p = c["plan"]
    old = build_backbone(make_config(_cfg(p.V_old), "CTR", backbone=backbone, compute_dtype=compute_dtype))
    sd = _randomise(old, 17)
    assert ("lr_layer.embed_w.weight" in sd) == (backbone == "DeepFM")
    old_ids, new_ids = torch.from_numpy(c["old_ids"]).to(DEV), torch.from_numpy(c["new_ids"]).to(DEV)
    assert old_ids.shape == (250, 25) and int((old_ids != new_ids).sum()) > 0
    before = score.Scorer(old.to(DEV), B, DEV, oov_id=c["oov_old"]).score(old_ids)
    moved, report = grow.migrate_state_dict(sd, p, device=DEV)
    assert list(report["tables"]) == [k for k in sd if k in TABLES] and report["dropped"] == []
    path = str(tmp_path / "9.model")
    torch.save(moved, path)
    new = build_backbone(make_config(_cfg(p.V_new), "CTR", backbone=backbone, compute_dtype=compute_dtype))
    score.load_checkpoint(new, path, input_size=p.V_new)
    after = score.Scorer(new.to(DEV), B, DEV, oov_id=c["oov_new"]).score(new_ids)
    assert before.logits.shape == (250,) and bool(torch.isfinite(before.logits).all())
    assert float(before.logits.std()) > 1e-3                           # (not a constant function)
    assert torch.equal(_bits(after.logits), _bits(before.logits)) and torch.equal(_bits(after.probs), _bits(before.probs))
    # a row keeps its <oov> fields only where the grown vocabulary still lacks the value
    assert int(before.oov_fields.sum()) == 254 and int(after.oov_fields.sum()) == 105
    # the old checkpoint itself no longer fits the grown vocabulary
    torch.save(sd, str(tmp_path / "old.model"))
    with pytest.raises(RuntimeError, match="input_size"):
        score.load_checkpoint(new, str(tmp_path / "old.model"), input_size=p.V_new)


def _mfp_model(V_, ids):
    from mapx.models import BaseModel
    count = np.bincount(ids.reshape(-1), minlength=V_).astype(np.float32)
    return BaseModel.from_config(make_config(_cfg(V_), "MFP", count))


def test_pretraining_checkpoint_loads_without_a_skipped_table_and_trains_on(golden_dir, tmp_path):
    from mapx import grow, ops
    from mapx.arguments import TrainingArguments
    from mapx.optim import MapxOptimizer
    c = _case(golden_dir)
    p = c["plan"]
    old = _mfp_model(p.V_old, V.apply(c["fm"], c["c1"], c["dec"]))
    sd = _randomise(old, 23)
    assert all(k in sd for k in NOISE) and all(k in sd for k in TABLES if not k.startswith("lr_layer"))
    moved, report = grow.migrate_state_dict(sd, p, device=DEV)
    assert report["dropped"] == list(NOISE) and sorted(set(sd) - set(moved)) == sorted(NOISE)
    assert list(report["tables"]) == ["embed.embedding.weight", "mfp_criterion.emb.weight", "mfp_criterion.bias.weight"]
    path = str(tmp_path / "3.model")
    torch.save(moved, path)
    new = _mfp_model(p.V_new, c["new_ids"])
    own_noise = {k: new.state_dict()[k].clone() for k in NOISE}
    assert new.load_for_finetune(path) == []                           # no key skipped: every table arrived
    got = new.state_dict()
    for k in NOISE:                                                    # the new dataset's own statistics stay
        assert got[k].shape[0] == p.V_new and torch.equal(got[k], own_noise[k]), k
    for k in report["tables"]:
        assert np.array_equal(got[k].numpy().view(np.int32), G.migrate(sd[k].numpy(), p).view(np.int32)), k
    for k in sd:
        if k not in TABLES and k not in NOISE:
            assert torch.equal(got[k], sd[k]), k
    # whereas the old file loses exactly those tables
    torch.save(sd, str(tmp_path / "old.model"))
    lost = _mfp_model(p.V_new, c["new_ids"]).load_for_finetune(str(tmp_path / "old.model"))
    assert sorted(lost) == sorted(list(report["tables"]) + list(NOISE))
    # one pretraining step on the grown dataset
    new = new.to(DEV).train()
    targs = TrainingArguments(output_dir=str(tmp_path / "out"), learning_rate=1e-3, weight_decay=5e-2, lr_sched="cosine")
    opt = MapxOptimizer(new, targs, num_training_steps=10, num_warmup_steps=0)
    ids = torch.from_numpy(c["new_ids"][:B]).to(DEV)
    masked, labels, mi = ops.dynamic_mask_mfp(ids, int(25 * 0.3), seed=3)
    loss, count, _acc = new(input_ids=masked, labels=labels, masked_index=mi)
    loss.backward()
    opt.step()
    opt.flush()
    torch.cuda.synchronize()
    assert count == B * 7 and bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    assert all(bool(torch.isfinite(q).all()) for q in new.parameters())


def test_init_normal_draws_the_added_rows_only(golden_dir):
    from mapx import grow
    c = _case(golden_dir)
    p = c["plan"]
    g = torch.Generator().manual_seed(31)
    sd = {"embed.embedding.weight": torch.randn(p.V_old, 16, generator=g), "fc_out.bias": torch.randn(1, generator=g),
          "lr_layer.embed_w.weight": torch.randn(p.V_old, 1, generator=g)}
    moved, report = grow.migrate_state_dict(sd, p, init="normal:0.01", seed=5, device=DEV)
    host = torch.Generator().manual_seed(5)                           # one generator, the tables in the dict's order
    added_rows = np.concatenate([np.arange(f.base_new + f.n_old, f.base_new + f.n_old + f.added) for f in p.fields])
    src = G.src_rows(p)
    others = np.setdiff1d(np.arange(p.V_new), added_rows)
    assert len(added_rows) == 55 and report["added"] == 55
    for k in ("embed.embedding.weight", "lr_layer.embed_w.weight"):
        fresh = torch.empty(55, sd[k].shape[1]).normal_(0.0, 0.01, generator=host)
        out = moved[k]
        assert out.shape == (p.V_new, sd[k].shape[1]) and out.device == sd[k].device
        assert torch.equal(_bits(out[added_rows]), _bits(fresh)), k                       # the host draw, bit for bit
        assert torch.equal(_bits(out[others]), _bits(sd[k][src[others]])), k             # old rows and <oov>': the source
        assert 0.005 < float(out[added_rows].std()) < 0.02 or out.shape[1] == 1
    assert moved["fc_out.bias"] is sd["fc_out.bias"]
    again, _ = grow.migrate_state_dict(sd, p, init="normal:0.01", seed=5, device=DEV)
    other, _ = grow.migrate_state_dict(sd, p, init="normal:0.01", seed=6, device=DEV)
    k = "embed.embedding.weight"
    assert torch.equal(_bits(again[k]), _bits(moved[k])) and not torch.equal(_bits(other[k]), _bits(moved[k]))


def test_command_line_round_trips(golden_dir, tmp_path, capsys):
    """--model: the file mapx.grow writes is migrate_state_dict's result, and the summary names what was dropped.
    --data_dir: the old dataset in the new id space.  Re-encoding its raw half with the grown vocabulary gives the same
    ids except where the old id was <oov>: there the grown vocabulary may know the value now (an added key), while a
    moved id stays <oov> — the id the row was trained on."""
    from mapx import grow, preprocess
    c = _case(golden_dir)
    p = c["plan"]
    p1, p2 = tmp_path / "first.txt", tmp_path / "second.txt"
    p1.write_bytes(c["first"])
    p2.write_bytes(c["second"])
    a_dir, b_dir, c_dir = (str(tmp_path / d) for d in "ABC")
    meta_a, meta_b = os.path.join(a_dir, f"{NAME}-meta.json"), os.path.join(b_dir, f"{NAME}-meta.json")
    assert preprocess.main(["--dataset", NAME, "--raw", str(p1), "--n_core", "2", "--out", a_dir,
                            "--split", "0.8,0.1,0.1"]) == 0
    assert preprocess.main(["--dataset", NAME, "--raw", str(p2), "--vocab", meta_a, "--grow", "2", "--out", b_dir]) == 0
    assert grow.plan(meta_a, meta_b, c["schema"]) == p
    # --model
    old = _mfp_model(p.V_old, V.apply(c["fm"], c["c1"], c["dec"]))
    sd = _randomise(old, 41)
    src_path, out_path = str(tmp_path / "ckpt" / "5.model"), str(tmp_path / "ckpt2" / "5.model")
    os.makedirs(os.path.dirname(src_path))
    torch.save(sd, src_path)
    capsys.readouterr()
    assert grow.main(["--model", src_path, "--from", meta_a, "--to", meta_b, "--out", out_path, "--dataset", NAME]) == 0
    said = capsys.readouterr().out
    want, _ = grow.migrate_state_dict(sd, p, device=DEV)
    got = torch.load(out_path, map_location="cpu")
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert "341 -> 396" in said and "55 keys added" in said and all(k in said for k in NOISE)
    assert grow.main(["--model", src_path, "--from", meta_a, "--to", meta_b, "--out", out_path, "--init", "normal:0.01",
                      "--seed", "8"]) == 0
    want, _ = grow.migrate_state_dict(sd, p, init="normal:0.01", seed=8, device=DEV)
    got = torch.load(out_path, map_location="cpu")
    assert all(torch.equal(got[k], want[k]) for k in want)
    # --data_dir
    capsys.readouterr()
    assert grow.main(["--data_dir", a_dir, "--dataset_name", NAME, "--from", meta_a, "--to", meta_b, "--out", c_dir]) == 0
    said = capsys.readouterr().out
    with open(meta_a) as f:
        ma = json.load(f)
    with open(os.path.join(c_dir, f"{NAME}-meta.json")) as f:
        mc = json.load(f)
    ta, tc = np.load(os.path.join(a_dir, f"{NAME}.npz")), np.load(os.path.join(c_dir, f"{NAME}.npz"))
    with open(meta_b) as f:
        mb = json.load(f)
    index = np.array(ma["index"])                                      # (Avazu's fit shuffles: A's rows are file rows [index])
    old_ids = V.apply(ma["feat_map"], c["c1"], c["dec"])[index]
    again = V.apply(mb["feat_map"], c["c1"], c["dec"])[index]          # the raw half re-encoded with the grown vocabulary
    assert np.array_equal(ta["feat_ids"], old_ids)
    oov_old, oov_new = np.array(c["oov_old"]), np.array(c["oov_new"])
    was_oov = old_ids == oov_old
    assert np.array_equal(tc["feat_ids"], np.where(was_oov, oov_new, again))
    known_now = was_oov & (again != oov_new)
    assert 0 < int(known_now.sum()) < int(was_oov.sum())
    lo = np.array([f.base_new + f.n_old for f in p.fields])
    assert bool(((again >= lo) & (again < oov_new))[known_now].all())  # ... and then it is an ADDED key's id
    for what in ("labels", "type_ids", "field_ids"):
        assert np.array_equal(tc[what], ta[what]), what
    assert list(mc["feat_map"].items()) == list(mb["feat_map"].items()) and mc["index"] == ma["index"]
    assert list(mb["feat_map"].items()) == list(G.grow(ma["feat_map"], c["c2"], c["dec"], 2)[0].items())
    assert sum(mc["oov_rows"].values()) == int(was_oov.sum()) and "341 -> 396" in said
    assert open(os.path.join(c_dir, "split.pkl"), "rb").read() == open(os.path.join(a_dir, "split.pkl"), "rb").read()
    # refusals of the command line: a pair that is no growth, a checkpoint of another vocabulary
    with pytest.raises(ValueError, match="missing"):
        grow.main(["--data_dir", a_dir, "--dataset_name", NAME, "--from", meta_b, "--to", meta_a, "--out", c_dir])
    with pytest.raises(ValueError, match="embed.embedding.weight"):
        grow.main(["--model", out_path, "--from", meta_a, "--to", meta_b, "--out", str(tmp_path / "x.model")])
