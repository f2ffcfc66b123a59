"""The FiGNN backbone (reference models.py:410-438) on the host: `FiGNN` and `build_backbone` for every variant and
step kind, the reference's state-dict layout (names, shapes, dtypes), the weight-decay rule for its three bias names,
initialisation, a checkpoint load, the configurations that are refused, and what `build_backbone` does for the other
names."""
import json
import math
import os

import pytest
import torch

import fignn_params as fp
import paramgen as pg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = pg.CASES[fp.CASE]
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]
MANIFEST = json.load(open(os.path.join(GOLD, "fignn_manifest.json")))


def _feat_count():
    return pg.make_inputs(fp.CASE, CFG)["feat_count"]


def _config(mode, variant="FiGNN", **over):
    return fp.make_config(CFG, mode, variant, _feat_count() if mode == "MFP" else None, **over)


def _model(mode, variant="FiGNN", **over):
    from mapx.models import build_backbone
    torch.manual_seed(0)
    return build_backbone(_config(mode, variant, **over))


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_state_dict_names_shapes_and_dtypes_equal_the_reference(mode, variant):
    from mapx.models import FiGNN
    model = _model(mode, variant)
    assert isinstance(model, FiGNN)
    direct = FiGNN(_config(mode, variant))                       # the public class builds the same thing
    want = MANIFEST[f"{fp.CASE}_{mode}_{variant}"]
    for m in (model, direct):
        got = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()}
        assert got == want
    # the trunk has no buffers; the fixture helper draws exactly the trainable parameters of the reference's model
    assert not list(model.fignn.buffers()) and not list(model.embed.buffers())
    assert set(fp.param_shapes(CFG, mode, variant)) == {k for k, p in model.named_parameters()}
    sd = model.state_dict()
    F, E = CFG["F"], CFG["E"]
    first = "fignn.gnn.W_in" if variant == "FiGNNShare" else "fignn.gnn.0.W_in"
    assert tuple(sd[first].shape) == (F, E, E)
    assert ("fignn.gnn.1.W_out" in sd) == (variant == "FiGNN")
    assert tuple(sd["fignn.gru.weight_hh"].shape) == (3 * E, E) and tuple(sd["fignn.W_attn.weight"].shape) == (1, 2 * E)
    assert ("fc.linear2.0.weight" in sd) == (mode == "CTR")
    assert not hasattr(model, "single_replica_only")


def test_hidden_size_other_than_embed_size_only_warns():
    model = _model("CTR", hidden_size=64)
    assert model.fignn.embedding_dim == CFG["E"] and model.fc.linear2["0"].weight.shape[1] == CFG["F"] * CFG["E"]


def test_bias_names_fall_in_the_no_decay_group():
    from mapx.optim import decays
    model = _model("CTR")
    names = [n for n, _ in model.named_parameters()]
    no_decay = sorted(n for n in names if not decays(n))
    assert no_decay == sorted([f"fignn.gnn.{l}.bias_p" for l in range(3)] + ["fignn.gru.bias_hh", "fignn.gru.bias_ih"])
    assert decays("fignn.gnn.0.W_in") and decays("fignn.gru.weight_ih") and decays("fignn.W_attn.weight")
    shared = [n for n, _ in _model("CTR", "FiGNNShare").named_parameters() if not decays(n)]
    assert sorted(shared) == ["fignn.gnn.bias_p", "fignn.gru.bias_hh", "fignn.gru.bias_ih"]


def test_initialisation_follows_the_reference():
    model = _model("CTR")
    F, E = CFG["F"], CFG["E"]
    bound = 1.0 / math.sqrt(E)
    for gl in model.fignn.gnn:
        assert bool((gl.bias_p == 0).all())
        # xavier_normal_ on [F,E,E]: fan_in = E * E, fan_out = F * E
        std = math.sqrt(2.0 / (E * E + F * E))
        for w in (gl.W_in, gl.W_out):
            assert abs(float(w.detach().std()) - std) < 0.1 * std and abs(float(w.detach().mean())) < 0.05 * std
    for p in model.fignn.gru.parameters():
        assert 0.8 * bound < float(p.detach().abs().max()) <= bound
    # nn.Linear's default (kaiming_uniform_, a = sqrt(5)): U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    for w, fan_in in ((model.fignn.W_attn.weight, 2 * E), (model.fc.linear1.weight, E),
                      (model.fc.linear2["0"].weight, F * E)):
        assert float(w.detach().abs().max()) <= 1.0 / math.sqrt(fan_in) + 1e-7
    assert all(getattr(p, "_mapx_row_resident", False) for p in model.fignn.parameters())
    assert not any(getattr(p, "_mapx_row_resident", False) for p in model.fc.parameters())


def test_reference_checkpoint_loads_for_finetune(tmp_path):
    """A checkpoint with the reference's keys and shapes (the manifest's) loads one-to-one: nothing is skipped but the
    pretraining heads."""
    want = MANIFEST[f"{fp.CASE}_RFD_FiGNN"]
    ckpt = {k: torch.ones(shape, dtype=getattr(torch, d)) for k, (shape, d) in want.items()}
    path = str(tmp_path / "ref.model")
    torch.save(ckpt, path)
    model = _model("CTR")
    skipped = model.load_for_finetune(path)
    assert sorted(skipped) == sorted(k for k in want if k.startswith("pred_rfd."))
    sd = model.state_dict()
    for k in want:
        if not k.startswith("pred_rfd."):
            assert bool((sd[k] == 1).all()), k
    assert not bool((sd["fc.linear1.weight"] == 1).all())        # the finetune head keeps its initialisation


@pytest.mark.parametrize("over,word", [
    (dict(compute_dtype="bf16"), "compute_dtype"),
    (dict(embed_size=36), "embed_size"),
    (dict(embed_size=64), "embed_size"),
    (dict(num_fields=1), "num_fields"),
    (dict(num_fields=65), "num_fields"),
    (dict(num_hidden_layers=0), "num_hidden_layers"),
])
def test_refused_configurations_name_the_flag(over, word):
    from mapx.models import FiGNN
    with pytest.raises(NotImplementedError, match=word):
        _model("CTR", **over)
    with pytest.raises(NotImplementedError, match=word):
        FiGNN(_config("CTR", **over))


def test_embed_size_must_be_a_multiple_of_four():
    with pytest.raises(NotImplementedError, match="embed_size"):
        _model("CTR", embed_size=18)


def _other_config(backbone):
    import fgcnn_params as gp
    import trans_params as tp
    from util import make_config
    if backbone == "Trans":
        return tp.make_config(CFG, "CTR", "Trans")
    if backbone == "FGCNN":
        return gp.make_config(CFG, "CTR", "FGCNN")
    return make_config(CFG, "CTR", None, backbone=backbone)


@pytest.mark.parametrize("backbone", ["DCNv2", "DNN", "DeepFM", "xDeepFM", "AutoInt", "Trans", "FGCNN"])
def test_build_backbone_returns_what_from_config_returns(backbone):
    from mapx.models import BaseModel, build_backbone
    c = _other_config(backbone)
    torch.manual_seed(3)
    a = build_backbone(c)
    torch.manual_seed(3)
    b = BaseModel.from_config(c)
    assert type(a) is type(b) and type(a) is not BaseModel
    assert type(a).__name__.lower() in (backbone.lower(), "transformer")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_build_backbone_for_nonsense_and_the_unchanged_factory():
    from mapx.models import BaseModel, build_backbone
    c = _config("CTR")
    c.model_name = "nonsense"
    with pytest.raises(NotImplementedError, match="nonsense"):
        build_backbone(c)
    c.model_name = "FiGNN"                                      # the name is matched in lower case
    assert type(build_backbone(c)).__name__ == "FiGNN"
    c.model_name = "fignn"
    with pytest.raises(NotImplementedError):                    # the factory itself is unchanged
        BaseModel.from_config(c)


def test_kernels_refuse_cpu_tensors():
    from mapx import ops
    from mapx.native import MapxError
    F, E = 3, 4
    x, g = torch.zeros(2, F, E), torch.zeros(2, F, F)
    w = [torch.zeros(F, E, E), torch.zeros(F, E, E), torch.zeros(E), torch.zeros(3 * E, E), torch.zeros(3 * E, E),
         torch.zeros(3 * E), torch.zeros(3 * E)]
    with pytest.raises(MapxError):
        ops.fignn_graph_fwd(x, torch.zeros(1, 2 * E))
    with pytest.raises(MapxError):
        ops.fignn_layer_fwd(x, g, *w)
    with pytest.raises(MapxError):
        ops.fignn_layer_bwd(x, x, g, *w, torch.zeros_like(g), True)
    with pytest.raises(MapxError):
        ops.fignn_graph_bwd(g, g, torch.zeros(2, F), torch.zeros(2, F), x, torch.zeros(1, 2 * E), x)
    with pytest.raises(MapxError):
        ops.fignn_pred_fwd(torch.zeros(2, F), torch.zeros(2, F))
    with pytest.raises(MapxError):
        ops.fignn_pred_bwd(torch.zeros(2, 1), torch.zeros(2, F), torch.zeros(2, F))


def test_lds_decision_has_both_ends_in_the_supported_range():
    """W_in / W_out are staged in LDS while two workgroups still fit a CU (80 KB), else streamed."""
    from mapx import ops
    assert ops.fignn_weights_staged(23, 16) and not ops.fignn_weights_staged(23, 16, backward=True)
    assert ops.fignn_weights_staged(3, 32) and ops.fignn_weights_staged(3, 32, backward=True)
    assert not ops.fignn_weights_staged(39, 16) and not ops.fignn_weights_staged(39, 16, backward=True)
    assert not ops.fignn_weights_staged(64, 32) and not ops.fignn_weights_staged(64, 32, backward=True)
    with pytest.raises(ValueError):
        ops.fignn_weights_staged(65, 16)
