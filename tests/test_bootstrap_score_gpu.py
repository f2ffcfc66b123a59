"""--bootstrap end to end (mapx/score.py, mapx/compare.py): the tiny model, documents and checkpoint of
tests/test_score_run_gpu.py.  The arrays are the ones ops.bootstrap_metrics gives on the returned logits; the raw form
and the dataset form agree bitwise; the scores do not know about the flag; the listed groups' intervals are the op on the
group's rows with their global units; the comparison of two checkpoints is two op calls on the same resamples."""
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boot_ref as B
import rawtext_ref as R
import test_score_run_gpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPS, SEED = 64, 5
_RUNS = {}


def _scorer(c, ckpt=None):
    from mapx import score
    args = c["args"]
    if ckpt is not None:
        args = copy.copy(args)
        args.model = ckpt
    model = score.build_model(args, len(c["meta"]["feat_map"]), len(c["names"]), torch.device(DEV))
    return score.Scorer(model, T.B, DEV, oov_id=score.oov_ids_of(c["meta"], c["names"]), stage_batches=2)


def _raw(c, chunk_bytes=None, **kw):
    from mapx import score, vocab
    voc = vocab.Vocabulary.from_meta(c["meta"], c["schema"], device=DEV)
    model = score.build_model(c["args"], voc.input_size, len(voc.fields), torch.device(DEV))
    sc = score.Scorer(model, T.B, DEV, oov_id=[f.oov for f in voc.fields], stage_batches=2)
    return score.score_raw_file(sc, io.BytesIO(c["doc"]), c["schema"], voc, chunk_bytes=chunk_bytes, **kw)


def _runs(golden_dir, tmp_path_factory):
    """Once: the Avazu case, its ids and labels restated, and the raw file scored with a bootstrap of its rows."""
    if not _RUNS:
        import vocab_apply_ref as V
        from mapx import score
        c = T._case(golden_dir, tmp_path_factory, "avazu")
        labels, cols = R.parse(c["doc"], c["schema"])
        dec = {n: (R.decode_hex if n in c["schema"].string_columns else (lambda v: str(int(v)))) for n in cols}
        _RUNS.update(c=c, labels=labels, ids=V.apply(c["meta"]["feat_map"], cols, dec),
                     boot=score.Bootstrap(REPS, SEED), whole=_raw(c, bootstrap=score.Bootstrap(REPS, SEED)))
    return _RUNS


def _same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in B.NAMES)


def _direct(logits, labels, units=None, reps=REPS, seed=SEED):
    from mapx import ops, score
    u = None if units is None else torch.from_numpy(np.ascontiguousarray(units, dtype=np.int64)).to(DEV)
    return score.boot_arrays(ops.bootstrap_metrics(torch.from_numpy(logits).to(DEV),
                                                   torch.from_numpy(np.asarray(labels)).to(DEV), reps, seed=seed, units=u))


def test_both_forms_give_the_op_on_the_logits_and_the_scores_do_not_change(golden_dir, tmp_path_factory):
    from mapx import score
    r = _runs(golden_dir, tmp_path_factory)
    c, whole = r["c"], r["whole"]
    assert len(set(r["labels"].tolist())) == 2
    b = whole["bootstrap"]
    assert all(b["arrays"][k].shape == (REPS,) for k in B.NAMES) and b["units"] is None
    assert np.array_equal(b["labels"], r["labels"].astype(np.uint8)) and b["labels"].dtype == np.uint8
    assert _same(b["arrays"], _direct(whole["logits"], r["labels"]))
    rep = score.bootstrap_report(b["arrays"], whole["info"]["metrics"])
    assert b["report"] == rep and set(rep) == {"auc", "logloss"}
    assert whole["info"]["bootstrap"] == {k: dict(lo=rep[k]["lo"], hi=rep[k]["hi"]) for k in ("auc", "logloss")}
    plain = T._run_raw(c, c["doc"], c["schema"], None)
    assert T._bits_equal(whole, plain) and "bootstrap" not in plain and "bootstrap" not in plain["info"]
    assert {k: v for k, v in whole["info"].items() if k not in ("bootstrap", "source")} == \
        {k: v for k, v in plain["info"].items() if k != "source"}
    small = _raw(c, 700, bootstrap=r["boot"])
    table = score.score_dataset(_scorer(c), c["meta"], r["ids"], r["labels"], names=c["names"], bootstrap=r["boot"])
    for other in (small, table):
        assert _same(other["bootstrap"]["arrays"], b["arrays"]) and other["bootstrap"]["report"] == b["report"]
        assert other["info"]["bootstrap"] == whole["info"]["bootstrap"]
    with pytest.raises(ValueError, match="bootstrap needs the labels of both classes: no labels"):
        score.score_dataset(_scorer(c), c["meta"], r["ids"], None, names=c["names"], bootstrap=r["boot"])
    with pytest.raises(ValueError, match="bootstrap needs the labels of both classes: .*[Oo]ne class"):
        score.score_dataset(_scorer(c), c["meta"], r["ids"], np.ones(T.ROWS, np.int64), names=c["names"],
                            bootstrap=r["boot"])


def test_units_of_a_field_in_both_forms(golden_dir, tmp_path_factory):
    from mapx import score
    r = _runs(golden_dir, tmp_path_factory)
    c = r["c"]
    boot = score.Bootstrap(REPS, SEED, 0.9, "device_id")
    column = r["ids"][:, c["names"].index("device_id")].astype(np.int64)
    assert len(np.unique(column)) < T.ROWS                               # some rows share a unit
    table = score.score_dataset(_scorer(c), c["meta"], r["ids"], r["labels"], names=c["names"], bootstrap=boot)
    raw = _raw(c, 700, bootstrap=boot)
    for res in (table, raw):
        assert np.array_equal(res["bootstrap"]["units"], column) and res["bootstrap"]["units"].dtype == np.int64
        assert _same(res["bootstrap"]["arrays"], _direct(res["logits"], r["labels"], column))
    assert not np.array_equal(table["bootstrap"]["arrays"]["pos_w"], r["whole"]["bootstrap"]["arrays"]["pos_w"])
    out = str(c["dir"] / "S_units")
    score.write_scores(out, table)
    assert set(os.listdir(out)) == {"probs.npy", "logits.npy", "oov_fields.npy", "score.json", "bootstrap.json",
                                    "bootstrap.npz", "labels.npy", "boot_units.npy"}
    assert np.array_equal(np.load(os.path.join(out, "boot_units.npy")), column)
    z = np.load(os.path.join(out, "bootstrap.npz"))
    assert set(z.files) == set(B.NAMES) | {"seed", "level", "units"}
    assert (int(z["seed"]), float(z["level"]), str(z["units"])) == (SEED, 0.9, "device_id")
    assert all(z[k].tobytes() == table["bootstrap"]["arrays"][k].tobytes() for k in B.NAMES)
    with open(os.path.join(out, "bootstrap.json")) as f:
        doc = json.load(f)
    assert {k: doc[k] for k in ("auc", "logloss")} == table["bootstrap"]["report"]
    assert (doc["replicates"], doc["seed"], doc["level"], doc["units"]) == (REPS, SEED, 0.9, "device_id")
    with pytest.raises(ValueError, match="'nope' is not a field"):
        score.score_dataset(_scorer(c), c["meta"], r["ids"], r["labels"], names=c["names"],
                            bootstrap=score.Bootstrap(8, by="nope"))


def _group_intervals(r, logits, listed, groups, units=None):
    """The five keys of every listed group, from the op on the group's rows with their global units."""
    from mapx import score
    want = []
    for t in listed:
        idx = np.flatnonzero(groups == t["group"])
        a = _direct(logits[idx], r["labels"][idx], idx if units is None else units[idx])
        rep = score.bootstrap_report(a, dict(auc=0.0, logloss=0.0))      # (the point is not among the five keys)
        want.append(dict(auc_lo=rep["auc"]["lo"], auc_hi=rep["auc"]["hi"], logloss_lo=rep["logloss"]["lo"],
                         logloss_hi=rep["logloss"]["hi"], boot_undefined=rep["auc"]["undefined"]))
    return want


def test_the_command_with_group_by_and_bootstrap_and_without(golden_dir, tmp_path_factory):
    r = _runs(golden_dir, tmp_path_factory)
    c = r["c"]
    env = dict(os.environ, PYTHONPATH=os.path.join(T.ROOT, "map-code_amd"))
    base = [sys.executable, "-m", "mapx.score", "--model", c["ckpt"], "--vocab", c["meta_path"], "--dataset", "avazu",
            "--raw", c["raw_path"], "--batch_size", str(T.B), "--chunk_mb", "1"] + T.MODEL_FLAGS
    out = str(c["dir"] / "S_boot")
    done = subprocess.run(base + ["--out", out, "--group_by", "C1", "--top", "3", "--bootstrap", str(REPS),
                                  "--bootstrap_seed", str(SEED)], env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    plain = {"probs.npy", "logits.npy", "oov_fields.npy", "score.json"}
    assert set(os.listdir(out)) == plain | {"slices.json", "slices_C1.npz", "bootstrap.json", "bootstrap.npz", "labels.npy"}
    with open(os.path.join(out, "score.json")) as f:
        doc = json.load(f)
    whole = r["whole"]
    assert doc["bootstrap"] == whole["info"]["bootstrap"]
    z = np.load(os.path.join(out, "bootstrap.npz"))
    assert all(z[k].tobytes() == whole["bootstrap"]["arrays"][k].tobytes() for k in B.NAMES)
    assert (int(z["seed"]), float(z["level"]), str(z["units"])) == (SEED, 0.95, "@row")
    labels = np.load(os.path.join(out, "labels.npy"))
    assert labels.dtype == np.uint8 and np.array_equal(labels, r["labels"])
    with open(os.path.join(out, "bootstrap.json")) as f:
        assert {k: v for k, v in json.load(f).items() if k in ("auc", "logloss")} == whole["bootstrap"]["report"]
    # the listed groups: the op on the group's rows, a row's unit its number in the file
    with open(os.path.join(out, "slices.json")) as f:
        top = json.load(f)["C1"]["top"]
    fm = c["meta"]["feat_map"]
    base_id = min(i for k, i in fm.items() if k.startswith("C1-"))
    groups = r["ids"][:, c["names"].index("C1")] - base_id
    logits = np.load(os.path.join(out, "logits.npy"))
    assert logits.tobytes() == whole["logits"].tobytes() and 1 <= len(top) <= 3
    new = ("auc_lo", "auc_hi", "logloss_lo", "logloss_hi", "boot_undefined")
    for t, want in zip(top, _group_intervals(r, logits, top, groups)):
        got = {k: t[k] for k in new}
        want = {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in want.items()}
        assert got == want and type(t["boot_undefined"]) is int, t["name"]
        assert t["rows"] == int((groups == t["group"]).sum())
    # without the flags: the four files, score.json's keys of before, the same scores
    out2 = str(c["dir"] / "S_plain_boot")
    done = subprocess.run(base + ["--out", out2], env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    assert set(os.listdir(out2)) == plain
    with open(os.path.join(out2, "score.json")) as f:
        doc2 = json.load(f)
    assert list(doc2) == ["rows", "batch_size", "graph", "oov_rows", "metrics", "metrics_reason", "source", "model",
                          "compute_dtype", "seconds"]
    assert {k: v for k, v in doc.items() if k not in ("slices", "bootstrap", "seconds")} == \
        {k: v for k, v in doc2.items() if k != "seconds"}
    for k in ("probs", "logits", "oov_fields"):
        assert np.load(os.path.join(out, f"{k}.npy")).tobytes() == np.load(os.path.join(out2, f"{k}.npy")).tobytes()


def test_compare_two_checkpoints_on_the_same_resamples(golden_dir, tmp_path_factory):
    from mapx import compare, score
    r = _runs(golden_dir, tmp_path_factory)
    c = r["c"]
    sd = torch.load(c["ckpt"], map_location="cpu")
    name = next(k for k, v in sd.items() if v.dim() == 2 and v.shape[0] != len(c["meta"]["feat_map"]))
    sd[name] = sd[name].clone()
    sd[name][0, 0] += 0.5                                                # one perturbed weight
    ckpt_b = str(c["dir"] / "4.model")
    torch.save(sd, ckpt_b)
    a = score.score_dataset(_scorer(c), c["meta"], r["ids"], r["labels"], names=c["names"], bootstrap=r["boot"])
    b = score.score_dataset(_scorer(c, ckpt_b), c["meta"], r["ids"], r["labels"], names=c["names"])
    assert a["logits"].tobytes() != b["logits"].tobytes()
    dir_a, dir_b, out = (str(c["dir"] / k) for k in ("CMP_A", "CMP_B", "CMP"))
    score.write_scores(dir_a, a)
    score.write_scores(dir_b, b)
    assert os.path.isfile(os.path.join(dir_a, "labels.npy")) and not os.path.exists(os.path.join(dir_b, "labels.npy"))
    env = dict(os.environ, PYTHONPATH=os.path.join(T.ROOT, "map-code_amd"), PYTHONIOENCODING="utf-8")
    done = subprocess.run([sys.executable, "-m", "mapx.compare", "--a", dir_a, "--b", dir_b, "--replicates", "50",
                           "--seed", "9", "--level", "0.9", "--out", out], env=env, capture_output=True, text=True,
                          encoding="utf-8", timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    arrays = {k: _direct(res["logits"], r["labels"], reps=50, seed=9) for k, res in (("a", a), ("b", b))}
    want = score.bootstrap_report(arrays["a"], a["info"]["metrics"], 0.9, other=arrays["b"],
                                  other_point=b["info"]["metrics"])
    with open(os.path.join(out, "compare.json")) as f:
        doc = json.load(f)
    assert doc["delta"] == want["delta"] and doc["a"] == {k: want[k] for k in ("auc", "logloss")}
    assert doc["b"] == score.bootstrap_report(arrays["b"], b["info"]["metrics"], 0.9)
    assert (doc["rows"], doc["replicates"], doc["seed"], doc["level"], doc["units"]) == (T.ROWS, 50, 9, 0.9, None)
    z = np.load(os.path.join(out, "compare.npz"))
    assert all(z[f"{m}_{k}"].tobytes() == arrays[m][k].tobytes() for m in ("a", "b") for k in B.NAMES)
    assert np.array_equal(z["a_pos_w"], z["b_pos_w"]) and np.array_equal(z["a_neg_w"], z["b_neg_w"])
    assert done.stdout.strip() == compare.summary_line(want, 0.9, 50)
    assert done.stdout.startswith("AUC a − b = ") and "(90 %, 50 replicates, a better in " in done.stdout
