"""xDeepFM in compute_dtype=bf16 at model level.

Parity: the six fixture cases of the reference's own class (B = 64, F = 25, E = 16, cin_layer_units = 12,8; with the
MLP tower and, xDeepFMCin, the CIN alone; the CTR models carry the LR term).  Loss and logits within 1e-2 of the fixture
(the project's bf16 tolerance).  The step's own ReLU pattern is hooked and may differ from the exact one only at units
whose pre-activation is zero to 2e-2 of the layer's scale (util.check_pattern); every gradient is then compared with the
float64 restatement (tests/bf16_xdeepfm_ref.py) ON THAT PATTERN.

Gradient bound, per tensor, as a share of the tensor's scale: max(1e-2, 2 * e_emul), e_emul = the error of the CPU
emulation of the roundings (bf16_xdeepfm_ref.step(emulate=True)) for that tensor on the same pattern.  Margin 2 for the
reasons tests/test_bf16_trans_model_gpu.py gives: the kernels accumulate in fp32 in another order than the emulation's
float64 (and the MFMA adds its products in its own order).  Each case prints measured error, e_emul and bound of its
worst tensor."""
import math
import os

import pytest
import torch

import bf16_xdeepfm_ref as XR
import model_harness as H
import paramgen as pg
from test_bf16_xdeepfm_host import CASE, CASES, IDS, hidden_of, reference
from util import hook_relu_pattern, load_case, make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _build(cfg, mode, backbone, params=None, feat_count=None, **over):
    from mapx.models import build_backbone
    c = make_config(cfg, mode, feat_count, backbone=backbone, compute_dtype="bf16")
    for k, v in over.items():
        setattr(c, k, v)
    model = build_backbone(c)
    if params is not None:
        H.load_params(model, params)
    return model.to(DEV)


def _is_trunk(name, mod):
    from mapx.layers import CIN, MLPBlock
    return isinstance(mod, (CIN, MLPBlock))


def _compare(what, model, mode, params, batch, units, num_hidden, exact, fixture=None):
    """The checks of the module docstring (model_harness.compare_bf16_step) against bf16_xdeepfm_ref.step."""
    def restate(relu_masks, emulate):
        return XR.step(mode, params, batch, units, num_hidden, relu_masks=relu_masks, emulate=emulate)[2]
    H.compare_bf16_step(what, model, mode, batch, hook_relu_pattern(model), restate, H.rel_err, exact, fixture,
                        is_trunk=_is_trunk)


# --------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_bf16_step_vs_fixture_and_float64_restatement(backbone, mode):
    cfg, z, inp, params = load_case(CASE, mode, backbone)
    model = _build(cfg, mode, backbone, params, inp["feat_count"] if mode == "MFP" else None)
    loss_x, logits_x, _, pre = reference(backbone, mode)
    # (the RFD fixtures keep the accuracy of their logits only: None has them compared with the restatement's)
    fixture = (float(z["out/loss"]), None if mode == "RFD" else z["out/logits"])
    _compare(f"bf16 {backbone} {mode}", model, mode, params, XR.fixture_batch(mode, cfg, inp),
             XR.units_of(pg.extras_of(backbone)), hidden_of(backbone, cfg), (loss_x, logits_x, pre), fixture)


# --------------------------------------------------------------------------- a case with no fixture
def test_bf16_xdeepfm_at_the_production_widths_and_more_than_32_fields():
    """RFD at B = 96, F = 39, E = 32, cin_layer_units = 50,50: K = 1521 and 1950, two unit tiles, rows that do not fill
    the last workgroup's tile; against the restatement (there is no fixture of this shape)."""
    cfg = dict(F=39, V=2000, E=32, H=48, NL=2, NC=0, P=8, K=5)
    torch.manual_seed(39)
    model = _build(cfg, "RFD", "xDeepFM", cin_layer_units="50,50")
    with torch.no_grad():                      # biases non-trivial
        for n, p in model.named_parameters():
            if n.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.1)
    g = torch.Generator().manual_seed(39)
    batch = dict(ids=torch.randint(10, cfg["V"], (96, 39), generator=g),
                 labels=(torch.rand(96, 39, generator=g) < 0.3).float())
    params = {n: p.detach().cpu().numpy() for n, p in model.named_parameters()}
    pre = {}
    loss_x, logits_x, _ = XR.step("RFD", params, batch, [50, 50], cfg["NL"], preacts=pre)
    _compare("bf16 xDeepFM RFD F=39", model, "RFD", params, batch, [50, 50], cfg["NL"], (loss_x, logits_x, pre))


# --------------------------------------------------------------------------- graphs, checkpoints: the Trainer
TCFG = dict(F=23, V=300, E=16, H=32, NL=2, NC=0, P=32, K=25)
B = 64


def _config(mode, cnt=None, compute_dtype="bf16"):
    return make_config(TCFG, mode, cnt, backbone="xDeepFM", compute_dtype=compute_dtype)       # cin 12,8; use_lr


def _start(mode, data, out_dir, seed=5):
    from mapx.models import build_backbone
    torch.manual_seed(seed)
    config = _config(mode, data[2])
    return H.make_trainer(config, build_backbone(config), mode, data, out_dir, B, 1, B, begin=True)


@pytest.mark.parametrize("mode", ["MFP", "CTR"], ids=["MFP", "CTR-use_lr"])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(mode, tmp_path):
    """Six AdamW steps with the captured graph (behind the Trainer's eager warm-up steps) against six eager ones: the
    same losses and the same state, bit for bit.  The checkpoint holds fp32 tensors only under the keys of the fp32
    model and loads into one; the CIN weights' bf16 shadows are the rounded master weights."""
    from mapx.models import BaseModel
    data = H.synth_data(B * 6, TCFG["F"], TCFG["V"], seed=3)

    def run(use_graph):
        tr, model, batches = _start(mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool(H.captured(tr)) == use_graph
        tr.optimizer.flush()
        for conv in model.cin.cin_layer.values():
            assert torch.equal(conv.weight._mapx_bf16, conv.weight.detach().to(BF))
        tr.save_model(str(tmp_path / str(use_graph)))
        return losses, H.model_state(model)

    H.graph_vs_eager(run)
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    H.assert_checkpoint_is_fp32(ck, BaseModel.from_config(_config(mode, data[2], compute_dtype="fp32")))


def test_run_py_xdeepfm_bf16_pretrain_then_finetune(tmp_path):
    """run.py --model_name=xDeepFM --compute_dtype bf16: RFD pretraining, then finetune with use_lr from that
    checkpoint."""
    common = ["--model_name=xDeepFM", "--embed_size=16", "--hidden_size=64", "--num_hidden_layers=2",
              "--hidden_dropout_rate=0.0", "--logging_steps=3", "--cin_layer_units=16,8", "--compute_dtype", "bf16"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=RFD", "--RFD_replace=Unigram"], ["--use_lr=True"])
    assert all(v.dtype != BF for v in sd.values())
    assert tuple(sd["cin.cin_layer.layer_1.weight"].shape) == (16, 23 * 23, 1)
    assert tuple(sd["cin.cin_layer.layer_2.weight"].shape) == (8, 23 * 16, 1)
    assert "Load tensor: cin.cin_layer.layer_2.weight" in log
    H.finite_metrics(log)
