"""Raw text to probabilities end to end (mapx/score.py: score_raw_file, score_dataset, the command): an Avazu-shaped and
a Criteo-shaped document built from the committed raw files' lines (tests/rawtext_ref.document), the vocabulary of the
golden feat_map, a tiny DCNv2 with random weights saved as a checkpoint.  Every comparison between two ways of
scoring the same rows is bitwise."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rawtext_ref as R
import vocab_apply_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}
ROWS, B = 150, 32
MODEL_FLAGS = ["--model_name", "DCNv2", "--embed_size", "8", "--hidden_size", "16", "--num_hidden_layers", "1",
               "--num_cross_layers", "1"]
_CASE = {}


def _without_click(line, schema):
    toks = line.split(schema.delimiter.encode())
    del toks[schema.source_names.index("click")]
    return schema.delimiter.encode().join(toks)


def _case(golden_dir, tmp_path_factory, name):
    """Once per dataset: the documents (with and without click), the meta of the golden feat_map, a checkpoint."""
    if name in _CASE:
        return _CASE[name]
    from mapx import rawtext, score
    from mapx.arguments import Config
    from mapx.models import build_backbone
    schema, bare = rawtext.SCHEMAS[name], rawtext.UNLABELED[name]
    z = np.load(os.path.join(golden_dir, f"rawtext_{name}.npz"))
    with open(os.path.join(golden_dir, RAW[name]), "rb") as f:
        lines = [line for _, line in R.lines(f.read())][1 if schema.header else 0:][:ROWS]
    doc = R.document(schema, lines, blank_at=(5, ROWS))
    doc_bare = R.document(bare, [_without_click(x, schema) for x in lines], blank_at=(5, ROWS))
    if bare.header:
        doc_bare = doc_bare.replace(R.AVAZU_HEADER, R.AVAZU_HEADER.replace(b",click", b""), 1)
    names = [c for c in schema.columns if c != schema.label]
    meta = {"field_names": ["<rsv>"] + names, "field_map": {n: i for i, n in enumerate(["<rsv>"] + names)},
            "feat_map": {str(k): int(i) for k, i in zip(z["feat_map_keys"], z["feat_map_ids"])}}
    d = tmp_path_factory.mktemp(f"score_{name}")
    meta_path, raw_path, ckpt = str(d / f"{name}-meta.json"), str(d / "day.txt"), str(d / "3.model")
    with open(meta_path, "w") as f:
        json.dump(meta, f)
    with open(raw_path, "wb") as f:
        f.write(doc)
    args = score.parse_args(["--model", ckpt, "--out", str(d / "S"), "--raw", raw_path, "--vocab", meta_path,
                             "--dataset", name, "--batch_size", str(B)] + MODEL_FLAGS)
    cfg = {n: getattr(args, n) for n, *_ in score.MODEL_FLAGS + score.EXTENSION_MODEL_FLAGS}
    cfg.update(data_dir=None, input_size=len(meta["feat_map"]), num_fields=len(names), pretrain=False, pt_type="MFP",
               RFD_replace="Unigram", feat_count=None, device=None, n_gpu=1, idx_low=None, idx_high=None,
               feat_num_per_field=None, seed=11, rank=0)
    torch.manual_seed(11)
    model = build_backbone(Config.from_dict(cfg))
    torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, ckpt)
    _CASE[name] = dict(schema=schema, bare=bare, doc=doc, doc_bare=doc_bare, meta=meta, meta_path=meta_path,
                       raw_path=raw_path, ckpt=ckpt, args=args, names=names, dir=d)
    return _CASE[name]


def _run_raw(c, data, schema, chunk_bytes):
    from mapx import score, vocab
    voc = vocab.Vocabulary.from_meta(c["meta"], schema, device=DEV)
    model = score.build_model(c["args"], voc.input_size, len(voc.fields), torch.device(DEV))
    sc = score.Scorer(model, B, DEV, oov_id=[f.oov for f in voc.fields], stage_batches=2)
    return score.score_raw_file(sc, io.BytesIO(data), schema, voc, chunk_bytes=chunk_bytes)


def _bits_equal(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
               for k in ("logits", "probs", "oov_fields"))


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_raw_file_scores_do_not_depend_on_the_chunks_and_equal_the_dataset_form(golden_dir, tmp_path_factory, name):
    from mapx import score, vocab
    c = _case(golden_dir, tmp_path_factory, name)
    whole = _run_raw(c, c["doc"], c["schema"], None)
    assert whole["probs"].shape == (ROWS,) and whole["probs"].dtype == np.float32 and whole["oov_fields"].dtype == np.uint8
    assert whole["info"]["rows"] == ROWS and whole["info"]["batch_size"] == B
    small = _run_raw(c, c["doc"], c["schema"], 700)                      # two to four lines a chunk
    assert _bits_equal(whole, small) and small["info"]["oov_rows"] == whole["info"]["oov_rows"]
    assert small["info"]["metrics"] == whole["info"]["metrics"]
    # every <oov> count against the reference's translation line restated with a dict
    labels, cols = R.parse(c["doc"], c["schema"])
    dec = {n: (R.decode_hex if n in c["schema"].string_columns else (lambda v: str(int(v)))) for n in cols}
    want = V.apply(c["meta"]["feat_map"], cols, dec)
    oov_ids = np.array([c["meta"]["feat_map"][f"{n}-<oov>"] for n in cols])
    assert list(whole["info"]["oov_rows"]) == c["names"]
    assert list(whole["info"]["oov_rows"].values()) == [int(x) for x in (want == oov_ids).sum(0)]
    assert np.array_equal(whole["oov_fields"], (want == oov_ids).sum(1).astype(np.uint8))
    assert int((want == oov_ids).sum()) >= 1                             # (n_core 2 on 500 rows: some values are unseen)
    # the metrics are eval_metrics over the logits and the file's labels
    if len(set(labels.tolist())) == 2:
        from mapx import ops
        assert whole["info"]["metrics"] == ops.eval_metrics(torch.from_numpy(whole["logits"]).to(DEV),
                                                            torch.from_numpy(labels).to(DEV))
    else:
        assert whole["info"]["metrics"] is None and "class" in whole["info"]["metrics_reason"]
    # encode_dataset_from_text, then the --data_dir form
    data_dir = str(c["dir"] / "encoded")
    vocab.encode_dataset_from_text(c["raw_path"], c["schema"], c["meta_path"], data_dir, name)
    meta, feat_ids, y = score.read_dataset(data_dir, name, "all")
    assert np.array_equal(feat_ids, want) and np.array_equal(y, labels)
    model = score.build_model(c["args"], len(meta["feat_map"]), feat_ids.shape[1], torch.device(DEV))
    sc = score.Scorer(model, B, DEV, oov_id=score.oov_ids_of(meta, c["names"]), stage_batches=2)
    table = score.score_dataset(sc, meta, feat_ids, y, names=c["names"])
    assert _bits_equal(whole, table) and table["info"]["oov_rows"] == whole["info"]["oov_rows"]
    assert table["info"]["metrics"] == whole["info"]["metrics"]


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_a_file_without_the_click_column_scores_the_same(golden_dir, tmp_path_factory, name):
    c = _case(golden_dir, tmp_path_factory, name)
    labelled = _run_raw(c, c["doc"], c["schema"], 900)
    bare = _run_raw(c, c["doc_bare"], c["bare"], 900)
    assert _bits_equal(labelled, bare) and bare["info"]["oov_rows"] == labelled["info"]["oov_rows"]
    assert bare["info"]["metrics"] is None and bare["info"]["metrics_reason"] == "no labels"


def test_a_single_class_file_gives_null_metrics_and_a_reason(golden_dir, tmp_path_factory):
    from mapx import rawtext
    c = _case(golden_dir, tmp_path_factory, "criteo")
    lines = [b"0" + x[x.index(b"\t"):] for _, x in R.lines(c["doc"])][:40]
    res = _run_raw(c, R.document(rawtext.CRITEO, lines), rawtext.CRITEO, None)
    assert res["info"]["rows"] == 40 and res["info"]["metrics"] is None and "one class" in res["info"]["metrics_reason"]


def test_the_command_writes_its_four_files(golden_dir, tmp_path_factory):
    """The command once, as a fresh process: its files, their shapes and score.json's keys; the probabilities are the
    ones score_raw_file gives in this process."""
    c = _case(golden_dir, tmp_path_factory, "avazu")
    out = str(c["dir"] / "S_cli")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "map-code_amd"))
    cmd = [sys.executable, "-m", "mapx.score", "--model", c["ckpt"], "--vocab", c["meta_path"], "--dataset", "avazu",
           "--raw", c["raw_path"], "--out", out, "--batch_size", str(B), "--chunk_mb", "1"] + MODEL_FLAGS
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    assert f"{ROWS} rows" in done.stdout
    probs, logits, oov = (np.load(os.path.join(out, f"{k}.npy")) for k in ("probs", "logits", "oov_fields"))
    assert (probs.dtype, logits.dtype, oov.dtype) == (np.float32, np.float32, np.uint8)
    assert probs.shape == logits.shape == oov.shape == (ROWS,)
    with open(os.path.join(out, "score.json")) as f:
        doc = json.load(f)
    assert {"rows", "batch_size", "compute_dtype", "model", "oov_rows", "metrics"} <= set(doc)
    assert (doc["rows"], doc["batch_size"], doc["compute_dtype"], doc["model"]) == (ROWS, B, "fp32", c["ckpt"])
    assert list(doc["oov_rows"]) == c["names"]
    assert doc["metrics"] is None or {"auc", "logloss", "avg_logits", "avg_probs"} <= set(doc["metrics"])
    here = _run_raw(c, c["doc"], c["schema"], None)
    assert here["probs"].tobytes() == probs.tobytes() and here["oov_fields"].tobytes() == oov.tobytes()
    assert doc["metrics"] == here["info"]["metrics"]
