"""AutoInt with attention dropout on the host side (no GPU): the factory builds the model at the reference's flag
default `attn_probs_dropout_rate` = 0.1 (code/arguments.py:116), the state_dict does not change with the rate, and
only a rate above 0 creates dropout sites: two per attention layer, as the reference creates its nn.Dropout objects
(code/layers.py:729-730, 874)."""
import pytest

import paramgen as pg
from util import make_config

CASE = "B_f25_b64"


def _config(mode, rate=None):
    """The AutoInt fixture config with `attn_probs_dropout_rate` replaced by the flag default (rate=None) or `rate`."""
    from mapx.arguments import ModelArguments
    cfg = pg.CASES[CASE]
    inp = pg.make_inputs(CASE, cfg)
    c = make_config(cfg, mode, inp["feat_count"] if mode == "MFP" else None, backbone="AutoInt")
    default = ModelArguments(model_name="autoint").attn_probs_dropout_rate
    assert default == 0.1
    c.attn_probs_dropout_rate = default if rate is None else rate
    return c


def _sites(model):
    from mapx.layers import HipDropout
    return [m for m in model.modules() if isinstance(m, HipDropout)]


@pytest.mark.parametrize("mode", ["MFP", "RFD", "CTR"])
def test_factory_builds_autoint_at_the_flag_default_rate(mode):
    from mapx.layers import MhaDropout
    from mapx.models import AutoInt, BaseModel
    model = BaseModel.from_config(_config(mode))
    assert isinstance(model, AutoInt)
    for layer in model.self_attention:
        assert isinstance(layer.dot_product_attention.dropout, MhaDropout) and layer.dot_product_attention.dropout.p == 0.1
        assert isinstance(layer.dropout, MhaDropout) and layer.dropout.p == 0.1


@pytest.mark.parametrize("mode", ["MFP", "RFD", "CTR"])
def test_state_dict_does_not_depend_on_the_rate(mode):
    from mapx.models import BaseModel
    a = BaseModel.from_config(_config(mode, 0.0)).state_dict()
    b = BaseModel.from_config(_config(mode, 0.1)).state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k


@pytest.mark.parametrize("mode", ["MFP", "CTR"])
def test_only_a_rate_above_zero_creates_dropout_sites(mode):
    """Rate 0 must hold no site of the attention layers: the Trainer numbers the HipDropout modules in order, so an
    extra one would shift the masks of every other dropout of an existing configuration.  Before attention dropout
    existed the attention stack held none, so a rate-0 model holds exactly the sites outside `self_attention`."""
    from mapx.models import BaseModel
    c0, c1 = _config(mode, 0.0), _config(mode, 0.1)
    m0 = BaseModel.from_config(c0)
    inside = {id(m) for m in m0.self_attention.modules()}
    assert not [m for m in _sites(m0) if id(m) in inside]
    assert all(layer.dropout is None and not hasattr(layer, "dot_product_attention") for layer in m0.self_attention)
    m1 = BaseModel.from_config(c1)
    assert len(_sites(m1)) - len(_sites(m0)) == 2 * c1.num_attn_layers
    inside = {id(m) for m in m1.self_attention.modules()}
    new = [m for m in _sites(m1) if id(m) in inside]
    assert len(new) == 2 * c1.num_attn_layers and len({m.site for m in new}) == len(new)
    assert not any(True for m in new for _ in m.parameters())


def test_rate_outside_the_unit_interval_is_rejected():
    from mapx.layers import MultiHeadSelfAttention
    with pytest.raises(ValueError):
        MultiHeadSelfAttention(16, 8, 2, dropout_rate=1.0)
    assert MultiHeadSelfAttention(16, 8, 2, dropout_rate=0.0).dropout is None
    assert MultiHeadSelfAttention(16, 8, 2, dropout_rate=0.5).dropout.p == 0.5
