"""The FGCNN backbone (model_name=fgcnn, reference models.py:325-407) on the host: construction for every step kind,
the reference's state-dict layout (names, shapes, dtypes), the width of the heads' input, the two row tables, and the
configurations that are refused."""
import json
import os

import pytest
import torch

import fgcnn_params as fp
import paramgen as pg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = pg.CASES[fp.CASE]
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]


def _feat_count():
    return pg.make_inputs(fp.CASE, CFG)["feat_count"]


def _model(mode, variant="FGCNN", **over):
    from mapx.models import BaseModel
    torch.manual_seed(0)
    return BaseModel.from_config(fp.make_config(CFG, mode, variant, _feat_count() if mode == "MFP" else None, **over))


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_state_dict_names_shapes_and_dtypes_equal_the_reference(mode, variant):
    from mapx.models import FGCNN
    model = _model(mode, variant)
    assert isinstance(model, FGCNN)
    want = json.load(open(os.path.join(GOLD, "fgcnn_manifest.json")))[f"{fp.CASE}_{mode}_{variant}"]
    got = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
    assert got == want
    # the fixture helper draws exactly the trainable parameters of the reference's model
    assert set(fp.param_shapes(CFG, mode, variant)) == {k for k, p in model.named_parameters()}
    sd = model.state_dict()
    assert tuple(sd["fgcnn_layer.conv_layers.1.0.weight"].shape) == (4, 3, 5, 1)
    assert sd["fgcnn_layer.conv_layers.0.1.num_batches_tracked"].dtype == torch.int64
    assert ("fg_embed.embedding.weight" in sd) == (variant == "FGCNN")


@pytest.mark.parametrize("variant", list(fp.VARIANTS))
def test_final_dim_matches_compute_input_dim(variant):
    model = _model("CTR", variant)
    ch, _, ps, rc = fp._lists(variant)
    final_dim, total = model.compute_input_dim(CFG["E"], CFG["F"], ch, ps, rc)
    assert total == fp.total_features(CFG, variant) == 25 + 13 * 2 + 7 * 1
    assert final_dim == fp.final_dim(CFG, variant) == total * (total - 1) // 2 + total * CFG["E"]
    first = model.dnn.dnn["0"] if model.dnn is not None else model.fc_out
    assert first.in_features == final_dim
    assert tuple(model.ip_layer.upper_triangle_mask.shape) == (total, total)
    assert model.ip_layer.field_p.numel() == total * (total - 1) // 2
    for mode in ("MFP", "RFD"):
        m = _model(mode, "FGCNN")
        head = m.feat_encoder if mode == "MFP" else m.pred_rfd["0"]
        assert head.in_features == fp.final_dim(CFG, "FGCNN")


def test_flag_defaults_give_the_documented_feature_rows():
    from mapx.arguments import MODEL_FLAGS
    from mapx.models import FGCNN
    default = {name: d for name, _typ, d, _help in MODEL_FLAGS}
    lists = [[int(x) for x in default[k].split(",")] for k in ("channels", "pooling_sizes", "recombined_channels")]
    assert FGCNN.compute_input_dim(16, 23, *lists)[1] == 92          # Avazu
    assert FGCNN.compute_input_dim(16, 39, *lists)[1] == 153         # Criteo


def test_two_row_tables_with_distinct_names():
    model = _model("MFP")
    names = [t.name for t in model.row_tables()]
    assert len(names) == 3 and len(set(names)) == 3
    assert "embed.embedding" in names and "fg_embed.embedding" in names
    assert model.fg_embed.table.p0 is model.fg_embed.embedding.weight
    shared = _model("CTR", "FGCNNShare")
    assert [t.name for t in shared.row_tables()] == ["embed.embedding"] and shared.fg_embed is None


def test_reference_checkpoint_loads_for_finetune(tmp_path):
    """A checkpoint with the reference's keys and shapes (the manifest's) loads one-to-one: nothing is skipped but the
    pretraining heads."""
    want = json.load(open(os.path.join(GOLD, "fgcnn_manifest.json")))[f"{fp.CASE}_RFD_FGCNN"]
    dt = {"float32": torch.float32, "int64": torch.int64, "bool": torch.bool}
    ckpt = {k: torch.ones(shape, dtype=dt[d]) for k, (shape, d) in want.items()}
    path = str(tmp_path / "ref.model")
    torch.save(ckpt, path)
    model = _model("CTR")
    skipped = model.load_for_finetune(path)
    assert sorted(skipped) == sorted(k for k in want if k.startswith("pred_rfd."))
    sd = model.state_dict()
    for k in want:
        if not k.startswith("pred_rfd."):
            assert bool((sd[k] == 1).all()), k
    assert int(sd["fgcnn_layer.conv_layers.1.1.num_batches_tracked"]) == 1


@pytest.mark.parametrize("over,exc,word", [
    (dict(compute_dtype="bf16"), NotImplementedError, "compute_dtype"),
    (dict(kernel_heights="3,4"), NotImplementedError, "kernel_heights"),
    (dict(kernel_heights="3,17"), NotImplementedError, "kernel_heights"),
    (dict(channels="3,40"), NotImplementedError, "channels"),
    (dict(channels="3,4,5"), ValueError, "channels"),
    (dict(pooling_sizes="2"), ValueError, "pooling_sizes"),
    (dict(recombined_channels="2,1,1"), ValueError, "recombined_channels"),
    (dict(kernel_heights="3"), ValueError, "kernel_heights"),
    (dict(conv_act="gelu"), NotImplementedError, "conv_act"),
    (dict(embed_size=64, channels="30,32"), NotImplementedError, "embed_size"),       # 151 KB of LDS in conv backward
    (dict(pooling_sizes="2,5"), ValueError, "pooling_sizes"),             # 13 % 5 = 3 rows of padding > 5 / 2
])
def test_refused_configurations_name_the_flag(over, exc, word):
    with pytest.raises(exc, match=word):
        _model("CTR", **over)


def test_data_parallel_is_refused(monkeypatch, tmp_path):
    from mapx import trainer as T
    from mapx.arguments import TrainingArguments
    model = _model("CTR")
    targs = TrainingArguments(output_dir=str(tmp_path))
    targs._device = torch.device("cpu")
    monkeypatch.setattr(T.parallel, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="one replica"):
        T.Trainer(model, model.config, targs, None, None)
    monkeypatch.setattr(T.parallel, "world", lambda: 1)
    T.Trainer(model, model.config, targs, None, None)


def test_fignn_still_raises():
    from mapx.models import BaseModel
    c = fp.make_config(CFG, "CTR", "FGCNN")
    c.model_name = "fignn"
    with pytest.raises(NotImplementedError, match="FGCNN"):
        BaseModel.from_config(c)


def test_kernels_refuse_cpu_tensors():
    from mapx import ops
    from mapx.native import MapxError
    with pytest.raises(MapxError):
        ops.inner_product_fwd(torch.zeros(2, 3, 4))
    with pytest.raises(MapxError):
        ops.fgcnn_conv_fwd(torch.zeros(2, 1, 3, 4), torch.zeros(2, 1, 3, 1), torch.zeros(2))
