"""mapx/score.py without a GPU: the command's parser, the label-less raw schemas, the batcher that cuts a stream handed
over in pieces into batches [kB, (k+1)B) (pure arithmetic over row counts), and the refusals of a checkpoint."""
import numpy as np
import pytest
import torch

BASE = ["--model", "m.model", "--out", "S", "--model_name", "DCNv2"]
RAW = ["--raw", "day.gz", "--vocab", "avazu-meta.json", "--dataset", "avazu"]


# ---------------------------------------------------------------- the parser
def test_parser_takes_both_forms_and_the_model_flags():
    from mapx import score
    a = score.parse_args(BASE + RAW + ["--unlabeled", "--compute_dtype", "bf16", "--hidden_size=64", "--chunk_mb", "8"])
    assert (a.raw, a.vocab, a.dataset, a.unlabeled, a.data_dir) == ("day.gz", "avazu-meta.json", "avazu", True, None)
    assert (a.batch_size, a.chunk_mb, a.compute_dtype, a.hidden_size, a.model_name) == (4096, 8, "bf16", 64, "DCNv2")
    b = score.parse_args(BASE + ["--data_dir", "D", "--dataset_name", "criteo", "--batch_size", "100"])
    assert (b.data_dir, b.dataset_name, b.split, b.batch_size, b.raw) == ("D", "criteo", "test", 100, None)
    from mapx.arguments import EXTENSION_MODEL_FLAGS, MODEL_FLAGS
    for name, *_ in MODEL_FLAGS + EXTENSION_MODEL_FLAGS:                 # run.py's model flags, every one
        assert hasattr(a, name), name


@pytest.mark.parametrize("argv", [
    BASE + ["--raw", "day.gz", "--dataset", "avazu"],                       # --raw needs --vocab
    BASE + ["--raw", "day.gz", "--vocab", "m.json"],                        # ... and --dataset
    BASE + RAW + ["--data_dir", "D"],                                       # --raw and --data_dir exclude each other
    BASE,                                                                   # one of them is needed
    BASE + RAW + ["--batch_size", "0"], BASE + RAW + ["--batch_size", "-3"], BASE + RAW + ["--batch_size", "x"],
    BASE + ["--data_dir", "D", "--unlabeled"], BASE + ["--data_dir", "D", "--vocab", "m.json"],
    BASE + RAW + ["--chunk_mb", "2000"], BASE + RAW + ["--dataset", "kdd"],
    ["--out", "S", "--model_name", "DCNv2"] + RAW,                          # --model is required
])
def test_parser_refuses(argv, capsys):
    from mapx import score
    with pytest.raises(SystemExit) as e:
        score.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


# ---------------------------------------------------------------- the label-less schemas
def test_unlabeled_schemas_are_the_labelled_ones_without_click():
    import rawtext_ref as R
    from mapx import rawtext
    for name in ("avazu", "criteo"):
        full, bare = rawtext.SCHEMAS[name], rawtext.UNLABELED[name]
        assert bare.label is None and "click" not in bare.columns and "click" not in bare.source_names
        assert bare.columns == [c for c in full.columns if c != "click"]
        assert bare.source_names == [c for c in full.source_names if c != "click"]
        assert (bare.delimiter, bare.header, bare.shuffle) == (full.delimiter, full.header, full.shuffle)
        assert bare.string_columns == full.string_columns and bare.feat_types == full.feat_types
        assert bare.min_line_bytes == full.min_line_bytes - 2               # the click digit and its delimiter
        kinds = dict(zip(full.source_names, full.kinds))
        assert bare.kinds == [kinds[n] for n in bare.source_names]
        s = bare.struct()
        assert s.n_fields == len(full.kinds) - 1 and list(s.out_col[:s.n_fields]) == bare.out_cols
    a = rawtext.AVAZU_UNLABELED
    assert a.source_names[:3] == ["id", "hour", "C1"] and a.kinds[0] == rawtext.SKIP and len(a.columns) == 25
    assert R.AVAZU_HEADER.replace(b",click", b"").decode().split(",") == a.source_names       # test.gz's header
    assert len(rawtext.CRITEO_UNLABELED.kinds) == 39 and not rawtext.CRITEO_UNLABELED.header
    # the restatement parses a line without its click field through the label-less schema to the same feature values
    for name in ("avazu", "criteo"):
        full, bare = rawtext.SCHEMAS[name], rawtext.UNLABELED[name]
        toks = R.GOOD_LINE[name].split(full.delimiter.encode())
        del toks[full.source_names.index("click")]
        row_full = R.parse_line(R.GOOD_LINE[name], full)
        assert R.parse_line(full.delimiter.encode().join(toks), bare) == \
            [v for c, v in zip(full.columns, row_full) if c != "click"]
    assert set(rawtext.SCHEMAS) == {"avazu", "criteo"}                        # the labelled pair is as it was


# ---------------------------------------------------------------- the batcher
def _replay(B, cap, pieces):
    """Runs the batcher's instructions on an array of stream row numbers -> (the batches scored, the rows emitted)."""
    from mapx.score import Batcher
    bt, stage = Batcher(B, cap), np.full(cap, -1, dtype=np.int64)
    batches, emitted, row0 = [], [], 0

    def run(todo, piece):
        for op, a, b, c in todo:
            if op == "load":
                assert 0 <= c and c + (b - a) <= cap and 0 <= a <= b <= len(piece)
                stage[c:c + b - a] = piece[a:b]
            elif op == "move":
                assert 0 <= a and a + b <= cap and 0 <= c and c + b <= cap
                stage[c:c + b] = stage[a:a + b].copy()
            else:
                assert op == "run" and 0 <= a and a + c <= cap
                for k in range(b):                                            # what the block kernel hands the model
                    rows = np.arange(a + k * B, a + (k + 1) * B)
                    batches.append(np.where(rows < cap, stage[np.minimum(rows, cap - 1)], -7))
                emitted.extend(stage[a:a + c].tolist())
    for n in pieces:
        piece = np.arange(row0, row0 + n)
        row0 += n
        run(bt.push(n), piece)
        assert bt.held < B and bt.rows_in == row0 and bt.rows_out + bt.held == row0
    run(bt.finish(), None)
    assert bt.held == 0 and bt.rows_out == row0
    return batches, emitted, row0


@pytest.mark.parametrize("B,cap", [(1, 1), (4, 4), (4, 12), (7, 21), (64, 64 * 64)])
def test_batch_k_is_rows_kB_to_kB_plus_B_however_the_stream_is_cut(B, cap):
    rng = np.random.RandomState(B * 1000 + cap)
    cuts = [[0], [1], [B], [B - 1, 1] if B > 1 else [1], [B + 1], [2 * B + 3], [1] * (2 * B + 3), [cap], [cap + 1],
            [cap - 1, 2, cap + B + 1], [0, 3 * cap + 5, 0, 1], rng.randint(0, 3 * B + 2, 40).tolist(),
            rng.randint(0, 2 * cap + 2, 6).tolist()]
    for pieces in cuts:
        batches, emitted, N = _replay(B, cap, pieces)
        assert emitted == list(range(N)), pieces                               # every row once, in stream order
        assert len(batches) == -(-N // B), pieces
        for k, rows in enumerate(batches):
            want = np.arange(k * B, (k + 1) * B)
            assert np.array_equal(rows, np.where(want < N, want, -7)), (pieces, k)   # the tail: pad rows behind N


def test_batcher_refuses_a_staging_area_that_is_no_multiple_of_the_batch():
    from mapx.score import Batcher
    for B, cap in ((0, 4), (4, 2), (4, 6), (-1, 4)):
        with pytest.raises(ValueError):
            Batcher(B, cap)


# ---------------------------------------------------------------- checkpoints
def _tiny(pretrain=False, V=50, hidden=8):
    from mapx.arguments import Config
    from mapx.models import build_backbone
    return build_backbone(Config(
        compute_dtype="fp32", model_name="DCNv2", data_dir=None, input_size=V, num_fields=3, embed_size=4,
        embed_dropout_rate=0.0, embed_norm=False, layer_norm_eps=1e-12, hidden_size=hidden, num_hidden_layers=1,
        hidden_act="relu", hidden_dropout_rate=0.0, num_cross_layers=1, pt_neg_num=2, proj_size=4, pretrain=pretrain,
        pt_type="MFP", RFD_replace="Unigram", feat_count=torch.ones(V) if pretrain else None, device=None, n_gpu=1,
        idx_low=None, idx_high=None, feat_num_per_field=None, seed=1))


def test_checkpoint_refusals_name_the_keys(tmp_path):
    from mapx import score
    model = _tiny()
    good = {k: v.clone() for k, v in model.state_dict().items()}
    path = str(tmp_path / "1.model")
    torch.save(good, path)
    score.load_checkpoint(_tiny(), path, input_size=50)                      # the good one loads

    def refused(sd, match, target=None, input_size=50):
        torch.save(sd, path)
        with pytest.raises(RuntimeError, match=match):
            score.load_checkpoint(target or _tiny(), path, input_size=input_size)
    some = sorted(good)[0]
    refused({k: v for k, v in good.items() if k != some}, f"missing \\['{some}'\\]")
    refused(dict(good, extra_key=torch.zeros(1)), "unexpected \\['extra_key'\\]")
    pre = {k: v.clone() for k, v in _tiny(pretrain=True).state_dict().items()}
    head = sorted(k for k in pre if k.startswith(score.PRETRAIN_KEYS))
    assert head and "fc_out.weight" not in pre
    refused(pre, "pretraining checkpoint.*" + head[0].replace(".", "\\."))
    refused(pre, "fc_out")                                                   # ... and names what it lacks
    wide = {k: v.clone() for k, v in _tiny(hidden=16).state_dict().items()}
    refused(wide, "another shape.*parallel_dnn")
    table = [k for k, v in good.items() if v.dim() == 2 and v.shape[0] == 50]
    assert table
    other_vocab = {k: v.clone() for k, v in _tiny(V=60).state_dict().items()}
    refused(other_vocab, f"input_size 50 .* 60 rows of '{table[0]}'")
    torch.save({"model": good, "global_step": 3}, path)                      # a training state, not a {step}.model
    with pytest.raises(RuntimeError, match="not a state_dict"):
        score.load_checkpoint(_tiny(), path)
    # the refusals on shapes alone
    with pytest.raises(RuntimeError, match="missing \\['b'\\], unexpected \\['c'\\]"):
        score.check_state_dict({"a": (2, 3), "b": (4,)}, {"a": (2, 3), "c": (4,)})
    score.check_state_dict({"a": (2, 3)}, {"a": torch.zeros(2, 3)})


def test_scorer_refuses_a_pretraining_model_before_touching_the_device():
    from mapx import score
    with pytest.raises(ValueError, match="pretrain"):
        score.Scorer(_tiny(pretrain=True), 8, "cuda")


def test_iter_columns_and_read_columns_refuse_the_cpu():
    import io
    from mapx import rawtext
    from mapx.native import MapxError
    with pytest.raises(MapxError):
        next(rawtext.iter_columns(io.BytesIO(b"1\n"), rawtext.CRITEO_UNLABELED, device="cpu"))
    with pytest.raises(MapxError):
        rawtext.parse_bytes(b"1\n", rawtext.CRITEO, device="cpu")
