"""The Transformer backbone in compute_dtype=bf16 at model level.

Parity: the eight fixture cases of the reference's own class (B = 64, F = 25, E = 16; post-norm relu 2 heads, pre-norm
gelu 4 heads with the LR term and the MLP tower, the four finetune reductions).  Loss and logits within 1e-2 of the
fixture (the project's bf16 tolerance).  The step's own ReLU pattern is hooked and may differ from the exact one only at
units whose pre-activation is zero to 2e-2 of the layer's scale (util.check_pattern); every gradient is then compared
with the float64 restatement (tests/bf16_trans_ref.py) ON THAT PATTERN.

Gradient bound, per tensor, as a share of the tensor's scale: max(1e-2, 2 * e_emul), e_emul = the error of the CPU
emulation of the roundings (bf16_trans_ref.step(emulate=True)) for that tensor on the same pattern.  Margin 2: the
kernels accumulate in fp32 in another order than the emulation's float64, and a tensor with several consumers gets its
gradient rounded once per consumer before autograd adds the pieces, where the emulation rounds the sum once.
field_reduction_attn.2.bias has an exactly zero gradient (the pooling softmax is shift-invariant): it is compared
absolutely, against the scale of field_reduction_attn.2.weight's gradient.  Each case prints measured error, e_emul and
bound of its worst tensor."""
import math
import os

import numpy as np
import pytest
import torch

import bf16_trans_ref as TR
import model_harness as H
import trans_params as tp
from test_bf16_trans_host import CASES, CFG, EPS, IDS, load, reference
from util import hook_relu_pattern

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SHIFT_INVARIANT = {"field_reduction_attn.2.bias": "field_reduction_attn.2.weight"}


def _build(cfg, mode, variant, params=None, feat_count=None, **over):
    from mapx.models import build_backbone
    model = build_backbone(tp.make_config(cfg, mode, variant, feat_count, **dict(dict(compute_dtype="bf16"), **over)))
    if params is not None:
        H.load_params(model, params)
    return model.to(DEV)


def _is_trunk(name, mod):
    from mapx.layers import HipLayerNorm, HipLinear, MLPBlock, TransformerEncoderLayer
    return isinstance(mod, (TransformerEncoderLayer, HipLayerNorm, MLPBlock)) or \
        (isinstance(mod, HipLinear) and name.startswith("encoder."))


def _err(name, got, ref):
    """Error of a gradient as a share of its tensor's scale (of the weight's, for the shift-invariant bias)."""
    scale_of = ref[SHIFT_INVARIANT.get(name, name)]
    want = np.asarray(ref[name], dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max()
                 / max(np.abs(scale_of).max(), 1e-30))


def _compare(what, model, mode, params, batch, T, eps, exact, fixture=None):
    """The checks of the module docstring (model_harness.compare_bf16_step) against bf16_trans_ref.step."""
    def restate(relu_masks, emulate):
        return TR.step(mode, params, batch, T, eps, relu_masks=relu_masks, emulate=emulate)[2]
    H.compare_bf16_step(what, model, mode, batch, hook_relu_pattern(model), restate, _err, exact, fixture,
                        is_trunk=_is_trunk)


# --------------------------------------------------------------------------- 6. the fixtures
@pytest.mark.parametrize("mode,variant", CASES, ids=IDS)
def test_bf16_step_vs_fixture_and_float64_restatement(mode, variant):
    z, inp, params, batch = load(mode, variant)
    model = _build(CFG, mode, variant, params, inp["feat_count"] if mode == "MFP" else None)
    loss_x, logits_x, _, pre = reference(mode, variant)
    _compare(f"bf16 trans {mode} {variant}", model, mode, params, batch, tp.VARIANTS[variant], EPS,
             (loss_x, logits_x, pre), (float(z["out/loss"]), z["out/logits"]))


# --------------------------------------------------------------------------- 7. F > 32 inside a model
def test_bf16_trans_with_more_than_32_fields():
    """RFD at B = 96, F = 39, E = 32, 4 heads, post-norm relu: the one-group-per-wave attention kernels (F > 32) and
    the 8-lane LayerNorm groups inside a model, against the restatement (there is no fixture of this shape)."""
    cfg = dict(F=39, V=2000, E=32, H=32, NL=0, NC=0, P=8, K=5)
    T = dict(tp.TRANS, hidden_size=32, num_attn_heads=4)
    torch.manual_seed(39)
    model = _build(cfg, "RFD", "Trans", hidden_size=32, num_attn_heads=4)
    with torch.no_grad():                      # layers made different from each other, biases and norms non-trivial
        for p in model.encoder.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    g = torch.Generator().manual_seed(39)
    batch = dict(ids=torch.randint(10, cfg["V"], (96, 39), generator=g),
                 labels=(torch.rand(96, 39, generator=g) < 0.3).float())
    params = {n: p.detach().cpu().numpy() for n, p in model.named_parameters()}
    pre = {}
    loss_x, logits_x, _ = TR.step("RFD", params, batch, T, EPS, preacts=pre)
    _compare("bf16 trans RFD F=39", model, "RFD", params, batch, T, EPS, (loss_x, logits_x, pre))


# --------------------------------------------------------------------------- dropout, graphs, checkpoints: the Trainer
TCFG = dict(F=23, V=300, E=16, H=16, NL=2, NC=0, P=32, K=25)
B = 64
PRE_NORM = dict(norm_first=True, hidden_act="gelu", num_attn_heads=4, output_reduction="mean,fc", use_lr=True,
                num_dnn_layers=2, dnn_size=40, layer_norm_eps=1e-5)


def _config(mode, cnt=None, compute_dtype="bf16", **over):
    return tp.make_config(TCFG, mode, "Trans", cnt, **dict(dict(compute_dtype=compute_dtype), **over))


def _start(mode, data, out_dir, seed=5, **over):
    from mapx.models import build_backbone
    torch.manual_seed(seed)
    config = _config(mode, data[2], **over)
    return H.make_trainer(config, build_backbone(config), mode, data, out_dir, B, 1, B, begin=True)


# --------------------------------------------------------------------------- 8. dropout
def test_bf16_trans_dropout_eval_is_the_rate_zero_model_and_replays_draw_new_masks(tmp_path):
    from mapx.models import build_backbone
    data = H.synth_data(B * 4, TCFG["F"], TCFG["V"], seed=8)
    torch.manual_seed(2)
    m1 = build_backbone(_config("MFP", data[2], hidden_dropout_rate=0.1)).to(DEV)
    m0 = build_backbone(_config("MFP", data[2], hidden_dropout_rate=0.0)).to(DEV)
    m0.load_state_dict(m1.state_dict())
    ids = torch.from_numpy(data[0][:B]).to(DEV)
    m0.eval()
    m1.eval()
    with torch.no_grad():
        x0, x1 = m0.encoder(m0.embed(ids)), m1.encoder(m1.embed(ids))
    assert x0.dtype == BF and torch.equal(x0, x1) and bool(torch.isfinite(x1.float()).all())
    # in training mode the four sites per layer act (attention probabilities inside the kernel + three elementwise)
    m1.train()
    with torch.no_grad():
        xt = m1.encoder(m1.embed(ids))
    assert xt.dtype == BF and not torch.equal(xt, x1) and bool(torch.isfinite(xt.float()).all())
    # the captured step replayed on the same batch: another loss each time (the masks follow the step counter)
    tr, model, batches = _start("MFP", data, str(tmp_path), hidden_dropout_rate=0.1)
    tr.use_graph = True
    X, Y = batches[0]
    losses = [float(tr.run_step("mfp", X, Y)[0]) for _ in range(tr.GRAPH_AFTER + 3)]      # eager, capture, two replays
    assert H.captured(tr), "no step was captured"
    assert all(math.isfinite(x) for x in losses) and len(set(losses[-2:])) == 2, losses


# --------------------------------------------------------------------------- 9. graph replay, checkpoint, run.py
@pytest.mark.parametrize("mode,over", [("MFP", {}), ("CTR", PRE_NORM)], ids=["MFP-postnorm-relu", "CTR-prenorm-gelu"])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(mode, over, tmp_path):
    """Six AdamW steps with the captured graph (behind the Trainer's eager warm-up steps) against six eager ones: the
    same losses and the same state, bit for bit.  The checkpoint holds fp32 tensors only under the keys of the fp32
    model and loads into one; every 2-D dense weight's bf16 shadow is the rounded master weight."""
    from mapx.models import BaseModel
    data = H.synth_data(B * 6, TCFG["F"], TCFG["V"], seed=3)

    def run(use_graph):
        tr, model, batches = _start(mode, data, str(tmp_path / str(use_graph)), **over)
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool(H.captured(tr)) == use_graph
        tr.optimizer.flush()
        for p in tr.optimizer.dense_params:
            if p.dim() == 2:
                assert torch.equal(p._mapx_bf16, p.detach().to(BF))
        assert all(getattr(layer.self_attn.in_proj_weight, "_mapx_bf16", None) is not None
                   for layer in model.encoder.layers)
        tr.save_model(str(tmp_path / str(use_graph)))
        return losses, H.model_state(model)

    H.graph_vs_eager(run)
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    H.assert_checkpoint_is_fp32(ck, BaseModel.from_config(_config(mode, data[2], compute_dtype="fp32", **over)))


def test_run_py_trans_bf16_pretrain_then_finetune(tmp_path):
    common = ["--model_name=trans", "--embed_size=16", "--hidden_size=16", "--num_hidden_layers=2", "--num_attn_heads=2",
              "--intermediate_size=64", "--hidden_dropout_rate=0.1", "--logging_steps=3", "--compute_dtype", "bf16"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"],
                                       ["--output_reduction=attn,fc", "--use_lr=True"])
    assert all(v.dtype != BF for v in sd.values())
    enc = sorted(k for k in sd if k.startswith("encoder."))
    assert len(enc) == 2 * 12 and "encoder.layers.1.self_attn.in_proj_weight" in enc
    for k in enc:
        assert f"Load tensor: {k}," in log, k
    H.finite_metrics(log)
