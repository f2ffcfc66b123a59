"""The Transformer backbone (model_name=trans, reference models.py:491-568) on the host: construction for every step
kind and finetune reduction, the reference's state-dict layout, torch's initialisation facts, weight-decay grouping
and the configurations that are refused."""
import json
import os

import pytest
import torch

import paramgen as pg
import trans_params as tp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = pg.CASES[tp.CASE]


def _feat_count():
    return pg.make_inputs(tp.CASE, CFG)["feat_count"]


def _model(mode, variant="Trans", **over):
    from mapx.models import BaseModel
    torch.manual_seed(0)
    return BaseModel.from_config(tp.make_config(CFG, mode, variant, _feat_count() if mode == "MFP" else None, **over))


@pytest.mark.parametrize("mode,variant", [(m, v) for v in tp.VARIANTS for m in tp.modes_of(v)])
def test_state_dict_names_and_shapes_equal_the_reference(mode, variant):
    from mapx.models import Transformer
    model = _model(mode, variant)
    assert isinstance(model, Transformer)
    want = json.load(open(os.path.join(GOLD, "trans_manifest.json")))[f"{tp.CASE}_{mode}_{variant}"]
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    # the fixture helper draws exactly the trainable parameters of the reference's model
    assert set(tp.param_shapes(CFG, mode, variant)) == {k for k, p in model.named_parameters()}


@pytest.mark.parametrize("reduction", ["fc", "mean,fc", "sum,fc", "attn,fc"])
def test_every_finetune_reduction_builds(reduction):
    model = _model("CTR", output_reduction=reduction)
    assert ("field_reduction_attn.0.weight" in model.state_dict()) == (reduction == "attn,fc")
    width = CFG["F"] * CFG["E"] if reduction == "fc" else CFG["E"]
    assert tuple(model.trans_out.weight.shape) == (1, width)


def test_layers_start_identical_with_torch_init():
    model = _model("MFP", num_hidden_layers=3)
    sds = [layer.state_dict() for layer in model.encoder.layers]
    assert len(sds) == 3
    for sd in sds[1:]:
        assert sd.keys() == sds[0].keys()
        for k in sd:
            assert torch.equal(sd[k], sds[0][k]), k
    sa = model.encoder.layers[0].self_attn
    E = CFG["E"]
    bound = (6.0 / (E + 3 * E)) ** 0.5                # xavier_uniform_ over [3E, E]
    w = sa.in_proj_weight.detach().abs().max()
    assert 0.5 * bound < float(w) <= bound
    assert not sa.in_proj_bias.any() and not sa.out_proj.bias.any()
    layer = model.encoder.layers[1]
    assert torch.equal(layer.norm1.weight, torch.ones(E)) and not layer.norm2.bias.any()
    # each copy has dropout sites of its own
    from mapx.layers import HipDropout
    sites = [m.site for m in model.encoder.modules() if isinstance(m, HipDropout)]
    assert len(sites) == 3 * 4 and len(set(sites)) == len(sites)


def test_weight_decay_follows_the_reference_name_rule():
    from mapx.optim import decays
    model = _model("CTR", "TransPre")
    names = [n for n, _ in model.named_parameters()]
    assert decays("encoder.layers.0.norm1.weight") and decays("encoder.layers.1.self_attn.in_proj_weight")
    assert not decays("encoder.layers.0.self_attn.in_proj_bias") and not decays("encoder.layers.0.norm2.bias")
    for n in names:
        assert decays(n) == (not any(nd in n for nd in ("bias", "LayerNorm.weight"))), n


def test_refused_configurations():
    from mapx.models import BaseModel
    model = _model("CTR", embed_size=16, hidden_size=32)
    with pytest.raises(AssertionError):
        model.validate_model_config()
    _model("CTR").validate_model_config()
    with pytest.raises(NotImplementedError):
        _model("CTR", num_attn_heads=8)                       # head size 2: not a multiple of 4
    with pytest.raises(NotImplementedError):
        _model("CTR", hidden_size=24, embed_size=24, num_attn_heads=4)     # head size 6
    big = dict(CFG, F=65)
    with pytest.raises(NotImplementedError):
        BaseModel.from_config(tp.make_config(big, "CTR", "Trans"))
    with pytest.raises(NotImplementedError):
        BaseModel.from_config(tp.make_config(CFG, "CTR", "Trans", compute_dtype="bf16"))
    with pytest.raises(NotImplementedError):
        _model("CTR", output_reduction="sum,max,sum")
    with pytest.raises(ValueError):
        _model("CTR", hidden_act="tanh")
