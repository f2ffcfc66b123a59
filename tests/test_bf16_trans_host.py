"""compute_dtype=bf16 for the Transformer backbone: what can be checked without a GPU.

(a) The float64 restatement of the trunk and its heads (tests/bf16_trans_ref.py), which the GPU tests compare against,
    reproduces the eight committed fixtures of the reference's own class.
(b) The bf16 emulation alone (rounding at the tensor stores of DESIGN §4.6 / §4.8, everything else float64) stays inside
    the caps the GPU tests apply to the real step: the fixtures are fit inputs for those caps.
(c) mapx.models.build_backbone builds trans in bf16 mode and refuses what is not built; BaseModel.from_config keeps
    refusing it (two existing tests pin that)."""
import functools
import os

import numpy as np
import pytest
import torch

import bf16_trans_ref as TR
import paramgen as pg
import trans_params as tp
from util import check_pattern

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = pg.CASES[tp.CASE]
CASES = [(m, v) for v in tp.VARIANTS for m in tp.modes_of(v)]
IDS = [f"{m}-{v}" for m, v in CASES]
EPS = 1e-12                       # util.make_config's layer_norm_eps, the fixtures'


def load(mode, variant):
    """-> (fixture npz, inputs, parameters, batch) of a fixture case."""
    z = np.load(os.path.join(GOLD, f"{tp.CASE}_{mode}_{variant}.npz"))
    inp = pg.make_inputs(tp.CASE, CFG)
    return z, inp, tp.make_params(CFG, mode, variant), TR.fixture_batch(mode, CFG, inp)


@functools.lru_cache(maxsize=None)
def reference(mode, variant, emulate=False):
    """(loss, logits, grads, preacts) of the restatement on the fixture case, on its own ReLU pattern."""
    _, _, params, batch = load(mode, variant)
    pre = {}
    loss, logits, grads = TR.step(mode, params, batch, tp.VARIANTS[variant], EPS, preacts=pre, emulate=emulate)
    return loss, logits, grads, pre


@pytest.mark.parametrize("mode,variant", CASES, ids=IDS)
def test_restatement_reproduces_the_fixtures(mode, variant):
    z = load(mode, variant)[0]
    loss, logits, _, _ = reference(mode, variant)
    e_loss = abs(loss - float(z["out/loss"])) / abs(float(z["out/loss"]))
    e_logits = TR.rel(logits, z["out/logits"])
    print(f"[{mode} {variant}] loss error {e_loss:.2e}, logits error {e_logits:.2e} of scale")
    assert e_loss <= 1e-5 and e_logits <= 1e-5


@pytest.mark.parametrize("mode,variant", CASES, ids=IDS)
def test_emulated_bf16_step_stays_inside_the_caps_of_the_gpu_tests(mode, variant):
    """Rounding alone moves the loss, the logits and the ReLU pattern by less than the GPU tests allow the real step:
    flipped units only at |z| <= 2e-2 of their layer's scale (util.check_pattern), loss and logits within 1e-2."""
    loss, logits, grads, pre = reference(mode, variant)
    loss_e, logits_e, grads_e, pre_e = reference(mode, variant, True)
    flips = check_pattern({k: v > 0 for k, v in pre_e.items()}, pre, f"{mode}/{variant} emulation")
    worst = max((float(pre[k][(pre_e[k] > 0) != (pre[k] > 0)].abs().max() / pre[k].abs().max())
                 for k in pre if bool(((pre_e[k] > 0) != (pre[k] > 0)).any())), default=0.0)
    e_loss, e_logits = abs(loss_e - loss) / abs(loss), TR.rel(logits_e, logits)
    print(f"[emulation {mode} {variant}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units flipped, worst at "
          f"{worst:.2e} of scale; loss {e_loss:.2e}, logits {e_logits:.2e} of scale")
    assert np.isfinite(loss_e)
    assert e_loss <= 1e-2 and e_logits <= 1e-2


# --------------------------------------------------------------------------- the gate
def _config(mode, variant="Trans", **over):
    inp = pg.make_inputs(tp.CASE, CFG)
    return tp.make_config(CFG, mode, variant, inp["feat_count"] if mode == "MFP" else None,
                          **dict(dict(compute_dtype="bf16"), **over))


@pytest.mark.parametrize("mode,variant", CASES, ids=IDS)
def test_build_backbone_builds_trans_in_bf16_mode(mode, variant):
    from mapx.models import BaseModel, Transformer, build_backbone
    model = build_backbone(_config(mode, variant))
    assert isinstance(model, Transformer)
    assert model.embed.compute_dtype == torch.bfloat16
    assert all(p.dtype == torch.float32 for p in model.parameters())          # master weights and tables stay fp32
    if mode == "CTR":
        assert model.trans_out.out_fp32
        if tp.VARIANTS[variant]["output_reduction"] == "attn,fc":
            assert model.field_reduction_attn["2"].out_fp32
        if tp.VARIANTS[variant]["num_dnn_layers"]:
            assert model.mlp_out.out_fp32
    elif mode == "MFP":
        assert model.feat_encoder.out_fp32
    else:
        assert model.pred_rfd["2"].out_fp32
    # the state dict is the fp32 model's
    fp32 = BaseModel.from_config(_config(mode, variant, compute_dtype="fp32"))
    assert {k: v.shape for k, v in model.state_dict().items()} == {k: v.shape for k, v in fp32.state_dict().items()}
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        BaseModel.from_config(_config(mode, variant))


def test_hidden_dropout_builds_in_bf16_mode():
    from mapx.layers import HipDropout, MhaDropout
    from mapx.models import build_backbone
    model = build_backbone(_config("MFP", hidden_dropout_rate=0.1))
    sites = [m for m in model.encoder.modules() if isinstance(m, HipDropout)]
    assert len(sites) == 2 * 4 and all(m.p == 0.1 for m in sites)
    assert sum(isinstance(m, MhaDropout) for m in sites) == 2


@pytest.mark.parametrize("variant,over,flag", [
    ("TransPre", dict(dnn_act="tanh"), "dnn_act"),
    ("TransPre", dict(dnn_drop=0.1), "dnn_drop"),
    ("Trans", dict(embed_norm=True), "embed_norm"),
    ("Trans", dict(embed_size=12, hidden_size=12, num_attn_heads=1), "embed_size"),
], ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_options_that_bf16_mode_does_not_build_raise_naming_their_flag(variant, over, flag):
    from mapx.models import build_backbone
    with pytest.raises(NotImplementedError, match=flag):
        build_backbone(_config("CTR", variant, **over))
    build_backbone(_config("CTR", variant, compute_dtype="fp32", **over))       # the same options build in fp32 mode
