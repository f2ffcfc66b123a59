"""compute_dtype=bf16 for xDeepFM: what can be checked without a GPU.

(a) The float64 restatement of the step (tests/bf16_xdeepfm_ref.py), which the GPU tests compare against, reproduces the
    six committed fixtures of the reference's own class (xDeepFM, and xDeepFMCin: the CIN alone feeds the heads).
(b) The bf16 emulation alone (rounding at the tensor boundaries of DESIGN §4.6, everything else float64) stays inside
    the caps the GPU tests apply to the real step: the fixtures are fit inputs for those caps.
(c) models.build_backbone builds the six cases in bf16 mode; BaseModel.from_config keeps refusing the mode.
(d) Options and shapes the mode does not build raise when the model is built, naming their flag."""
import functools

import numpy as np
import pytest
import torch

import bf16_xdeepfm_ref as XR
import paramgen as pg
from util import check_pattern, load_case, make_config

CASE = "B_f25_b64"
CASES = [(b, m) for b in ("xDeepFM", "xDeepFMCin") for m in ("MFP", "RFD", "CTR")]
IDS = [f"{b}-{m}" for b, m in CASES]


def hidden_of(backbone, cfg):
    return pg.extras_of(backbone).get("num_hidden_layers", cfg["NL"])


@functools.lru_cache(maxsize=None)
def reference(backbone, mode, emulate=False):
    """(loss, logits, grads, preacts) of the restatement on the fixture case, on its own ReLU pattern."""
    cfg, z, inp, params = load_case(CASE, mode, backbone)
    pre = {}
    loss, logits, grads = XR.step(mode, params, XR.fixture_batch(mode, cfg, inp), XR.units_of(pg.extras_of(backbone)),
                                  num_hidden=hidden_of(backbone, cfg), preacts=pre, emulate=emulate)
    return loss, logits, grads, pre


# --------------------------------------------------------------------------- (a)
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
        print(f"logits error {XR.rel(logits, z['out/logits']):.2e} of scale")
        assert XR.rel(logits, z["out/logits"]) <= 1e-5


# --------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_emulated_bf16_step_stays_inside_the_caps_of_the_gpu_tests(backbone, mode):
    """Rounding alone moves the loss, the logits and the ReLU pattern by less than the GPU tests allow the real step:
    flipped units only at |z| <= 2e-2 of their layer's scale (util.check_pattern), loss and logits within 1e-2."""
    loss, logits, _, pre = reference(backbone, mode)
    loss_e, logits_e, _, pre_e = reference(backbone, mode, True)
    flips = check_pattern({k: v > 0 for k, v in pre_e.items()}, pre, f"{backbone}/{mode} emulation")
    worst = max((float(pre[k][(pre_e[k] > 0) != (pre[k] > 0)].abs().max() / pre[k].abs().max())
                 for k in pre if bool(((pre_e[k] > 0) != (pre[k] > 0)).any())), default=0.0)
    e_loss, e_logits = abs(loss_e - loss) / abs(loss), XR.rel(logits_e, logits)
    print(f"[emulation {backbone} {mode}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units flipped, worst "
          f"at {worst:.2e} of scale; loss {e_loss:.2e}, logits {e_logits:.2e} of scale")
    assert np.isfinite(loss_e)
    assert e_loss <= 1e-2 and e_logits <= 1e-2


# --------------------------------------------------------------------------- (c)
def _config(backbone, mode, compute_dtype="bf16", **over):
    cfg, _, inp, _ = load_case(CASE, mode, backbone)
    c = make_config(cfg, mode, inp["feat_count"] if mode == "MFP" else None, backbone=backbone,
                    compute_dtype=compute_dtype)
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_build_backbone_builds_xdeepfm_in_bf16_mode(backbone, mode):
    from mapx.models import BaseModel, build_backbone, xDeepFM
    model = build_backbone(_config(backbone, mode))
    assert isinstance(model, xDeepFM) and model.embed.compute_dtype == torch.bfloat16
    assert all(p.dtype == torch.float32 for p in model.parameters())          # master weights and tables stay fp32
    want = BaseModel.from_config(_config(backbone, mode, compute_dtype="fp32")).state_dict()
    got = model.state_dict()
    assert list(got) == list(want) and all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype for k in want)
    params = load_case(CASE, mode, backbone)[3]
    assert set(params) <= set(got) and all(tuple(got[k].shape) == params[k].shape for k in params)
    if mode == "CTR":
        assert model.fc.out_fp32 and model.lr_layer is not None
    elif mode == "MFP":
        assert model.feat_encoder.out_fp32
    else:
        assert model.pred_rfd["2"].out_fp32
    assert (model.dnn is None) == (backbone == "xDeepFMCin")
    with pytest.raises(NotImplementedError, match="compute_dtype"):           # pinned by test_bf16_backbones_host.py
        BaseModel.from_config(_config(backbone, mode))


def test_the_fp32_model_keeps_its_fp32_head():
    from mapx.models import build_backbone
    assert not build_backbone(_config("xDeepFM", "CTR", compute_dtype="fp32")).fc.out_fp32


# --------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("over,flag", [
    (dict(hidden_act="tanh"), "hidden_act"),
    (dict(hidden_dropout_rate=0.1), "hidden_dropout_rate"),
    (dict(embed_norm=True), "embed_norm"),
    (dict(embed_size=12), "embed_size"),
    (dict(cin_layer_units="12,200"), "cin_layer_units"),
    (dict(num_fields=65), "num_fields"),
], ids=lambda v: "+".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_what_bf16_mode_does_not_build_raises_naming_its_flag(over, flag):
    from mapx.models import build_backbone
    with pytest.raises(NotImplementedError, match=flag):
        build_backbone(_config("xDeepFM", "CTR", **over))
    build_backbone(_config("xDeepFM", "CTR", compute_dtype="fp32", **over))       # fp32 mode supports every one of them
