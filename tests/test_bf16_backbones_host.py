"""compute_dtype=bf16 for DeepFM and AutoInt: what can be checked without a GPU.

1. The float64 restatement of the two trunks (tests/bf16_backbones_ref.py), which the GPU tests compare against,
   reproduces the committed fixtures of the reference's own classes.
2. BaseModel.from_config builds the two backbones in bf16 mode and keeps refusing what is not built.
3. The bf16 emulation alone (rounding at the tensor boundaries of DESIGN §4.6, everything else float64) stays inside
   the caps the GPU tests apply to the real step: the inputs are fit for those caps."""
import functools

import numpy as np
import pytest
import torch

import bf16_backbones_ref as BR
import paramgen as pg
from util import check_pattern, load_case, make_config

CASE = "B_f25_b64"
CASES = [(b, m) for b in ("DeepFM", "AutoInt") for m in ("MFP", "RFD", "CTR")] + [("AutoIntFull", "CTR")]
IDS = [f"{b}-{m}" for b, m in CASES]


def family(backbone):
    return "AutoInt" if backbone.startswith("AutoInt") else backbone


@functools.lru_cache(maxsize=None)
def reference(backbone, mode, emulate=False):
    """(loss, logits, grads, preacts) of the restatement on the fixture case, on its own ReLU pattern."""
    cfg, z, inp, params = load_case(CASE, mode, backbone)
    pre = {}
    loss, logits, grads = BR.step(family(backbone), mode, params, BR.fixture_batch(mode, cfg, inp), num_hidden=cfg["NL"],
                                  ai=pg.extras_of(backbone) or None, preacts=pre, emulate=emulate)
    return loss, logits, grads, pre


@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_restatement_reproduces_the_fixtures(backbone, mode):
    z = load_case(CASE, mode, backbone)[1]
    loss, logits, _, _ = reference(backbone, mode)
    print(f"loss error {abs(loss - float(z['out/loss'])) / abs(float(z['out/loss'])):.2e}")
    assert abs(loss - float(z["out/loss"])) <= 1e-5 * abs(float(z["out/loss"]))
    if mode == "RFD":         # the RFD fixtures keep what the reference's step returns of its logits: the accuracy
        acc = float(((logits > 0) == (z["in/labels"] > 0.5)).mean())
        assert abs(acc - float(z["out/acc"])) <= 1e-6
    else:
        print(f"logits error {BR.rel(logits, z['out/logits']):.2e} of scale")
        assert BR.rel(logits, z["out/logits"]) <= 1e-5


# --------------------------------------------------------------------------- the gate
def _config(backbone, mode, **over):
    cfg, _, inp, _ = load_case(CASE, mode, backbone if backbone in ("DeepFM", "AutoInt", "AutoIntFull") else "DNN")
    c = make_config(cfg, mode, inp["feat_count"] if mode == "MFP" else None,
                    backbone=backbone if backbone in ("DeepFM", "AutoInt", "AutoIntFull") else "DNN",
                    compute_dtype="bf16")
    if backbone not in ("DeepFM", "AutoInt", "AutoIntFull"):
        c.model_name = backbone
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_from_config_builds_deepfm_and_autoint_in_bf16_mode(backbone, mode):
    from mapx.models import BaseModel
    model = BaseModel.from_config(_config(backbone, mode))
    assert model.embed.compute_dtype == torch.bfloat16
    assert all(p.dtype == torch.float32 for p in model.parameters())          # master weights and tables stay fp32
    last = {"DeepFM": "dnn_fc_out", "AutoInt": "attn_out"}[family(backbone)]
    if mode == "CTR":
        assert getattr(model, last).out_fp32
        if backbone == "AutoIntFull":
            assert model.dnn_out.out_fp32
    elif mode == "MFP":
        assert model.feat_encoder.out_fp32
    else:
        assert model.pred_rfd["2"].out_fp32


def test_autoint_default_attention_dropout_is_built_in_bf16_mode():
    from mapx.models import BaseModel
    model = BaseModel.from_config(_config("AutoInt", "MFP", attn_probs_dropout_rate=0.1))
    assert all(layer.dropout is not None and layer.dropout.p == 0.1 for layer in model.self_attention)


@pytest.mark.parametrize("name", ["xDeepFM", "trans", "fgcnn"])
def test_the_other_backbones_still_refuse_bf16_mode(name):
    from mapx.models import BaseModel
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        BaseModel.from_config(_config(name, "CTR"))


@pytest.mark.parametrize("backbone,over,flag", [
    ("DeepFM", dict(hidden_dropout_rate=0.1), "hidden_dropout_rate"),
    ("DeepFM", dict(hidden_act="tanh"), "hidden_act"),
    ("DeepFM", dict(embed_norm=True), "embed_norm"),
    ("DeepFM", dict(embed_dropout_rate=0.1), "embed_dropout_rate"),
    ("DeepFM", dict(embed_size=12), "embed_size"),
    ("AutoInt", dict(embed_norm=True), "embed_norm"),
    ("AutoInt", dict(embed_dropout_rate=0.1), "embed_dropout_rate"),
    ("AutoInt", dict(embed_size=12), "embed_size"),
    ("AutoIntFull", dict(dnn_drop=0.1), "dnn_drop"),
    ("AutoIntFull", dict(dnn_act="tanh"), "dnn_act"),
], ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_options_that_bf16_mode_does_not_build_raise_naming_their_flag(backbone, over, flag):
    from mapx.models import BaseModel
    with pytest.raises(NotImplementedError, match=flag):
        BaseModel.from_config(_config(backbone, "CTR", **over))
    # the same options build in fp32 mode (AutoInt's embed_size = 12 too: a multiple of 4; DeepFM's does not: its FM
    # kernels take 4, 8, 16, 32 and 64, tests/test_host_surface.py)
    c = _config(backbone, "CTR", **over)
    c.compute_dtype = "fp32"
    if not (backbone in ("AutoIntFull", "DeepFM") and "embed_size" in over):
        BaseModel.from_config(c)


# --------------------------------------------------------------------------- the emulation against the caps
@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_emulated_bf16_step_stays_inside_the_caps_of_the_gpu_tests(backbone, mode):
    """Rounding alone moves the loss, the logits and the ReLU pattern by less than the GPU tests allow the real step:
    flipped units only at |z| <= 2e-2 of their layer's scale (util.check_pattern), loss and logits within 1e-2."""
    loss, logits, _, pre = reference(backbone, mode)
    loss_e, logits_e, _, pre_e = reference(backbone, mode, True)
    flips = check_pattern({k: v > 0 for k, v in pre_e.items()}, pre, f"{backbone}/{mode} emulation")
    worst = max((float(pre[k][(pre_e[k] > 0) != (pre[k] > 0)].abs().max() / pre[k].abs().max())
                 for k in pre if bool(((pre_e[k] > 0) != (pre[k] > 0)).any())), default=0.0)
    e_loss, e_logits = abs(loss_e - loss) / abs(loss), BR.rel(logits_e, logits)
    print(f"[emulation {backbone} {mode}] {flips} flipped ReLU units, worst at {worst:.2e} of scale; "
          f"loss {e_loss:.2e}, logits {e_logits:.2e} of scale")
    assert e_loss <= 1e-2 and e_logits <= 1e-2
    assert np.isfinite(loss_e)
