"""DeepFM and AutoInt in compute_dtype=bf16 at model level.

Parity: fixture case B (B = 64, F = 25, E = 16, H = 64; AutoInt 2 layers x 2 heads x 12; AutoIntFull 2 x 8 with the LR
term and the MLP tower).  Loss and logits within 1e-2 of the fixture (the project's bf16 tolerance; the RFD fixtures
keep no logits: there the float64 restatement that test_bf16_backbones_host.py pins to the fixture stands in).  The
step's own ReLU pattern is hooked and may differ from the exact one only at units whose pre-activation is zero to
2e-2 of the layer's scale (util.check_pattern); every gradient is then compared with the float64 restatement ON THAT
PATTERN (on another pattern the same gradients differ by 5e-2 .. 1.3e-1 of scale: ReLU branches, not arithmetic).

Gradient bound, per tensor, as a share of the tensor's scale: max(1e-2, 2 * e_emul), e_emul = the error of the CPU
emulation of the roundings (bf16_backbones_ref.step(emulate=True)) for that tensor on the same pattern.  Margin 2: the
kernels accumulate in fp32 in another order than the emulation's float64, and the embedding's gradient is rounded once
per consumer (MLP and FM term; attention and tower) before autograd adds the pieces, where the emulation rounds the
sum once.  Each case prints measured error, e_emul and bound of its worst tensor."""
import math
import os

import pytest
import torch

import bf16_backbones_ref as BR
import model_harness as H
import paramgen as pg
from test_bf16_backbones_host import CASE, CASES, IDS, family, reference
from util import build_model, hook_relu_pattern, load_case, make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _masks(model):
    """The ReLU masks by layer; the attention layers' outputs (ReLU inside the kernel) are part of the pattern."""
    from mapx.layers import MultiHeadSelfAttention
    masks = hook_relu_pattern(model)
    for name, mod in model.named_modules():
        if isinstance(mod, MultiHeadSelfAttention):
            def attn_hook(m, i, o, name=name):          # (a hook that returns a value would replace the output)
                masks[name] = (o.detach() > 0).cpu()
            mod.register_forward_hook(attn_hook)
    return masks


def _is_trunk(name, mod):
    from mapx.layers import MLPBlock, MultiHeadSelfAttention
    return isinstance(mod, (MultiHeadSelfAttention, MLPBlock))


def _compare(what, model, fam, mode, params, batch, num_hidden, ai, exact, fixture=None):
    """The checks of the module docstring (model_harness.compare_bf16_step) against bf16_backbones_ref.step."""
    def restate(relu_masks, emulate):
        return BR.step(fam, mode, params, batch, num_hidden=num_hidden, ai=ai, relu_masks=relu_masks, emulate=emulate)[2]
    H.compare_bf16_step(what, model, mode, batch, _masks(model), restate, H.rel_err, exact, fixture, is_trunk=_is_trunk)


@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_bf16_step_vs_fixture_and_float64_restatement(backbone, mode):
    cfg, z, inp, params = load_case(CASE, mode, backbone)
    model = build_model(cfg, mode, params, inp["feat_count"] if mode == "MFP" else None, backbone=backbone,
                        compute_dtype="bf16")
    loss_x, logits_x, _, pre = reference(backbone, mode)
    fixture = (float(z["out/loss"]), z["out/logits"] if "out/logits" in z.files else None)
    _compare(f"bf16 {backbone} {mode}", model, family(backbone), mode, params, BR.fixture_batch(mode, cfg, inp),
             cfg["NL"], pg.extras_of(backbone) or None, (loss_x, logits_x, pre), fixture)


def test_bf16_autoint_with_more_than_32_fields():
    """AutoInt RFD at B = 96, F = 39, E = 16, 2 heads x 16: the one-group-per-wave attention kernels (F > 32) inside a
    model, a first layer with W_res (16 -> 32) and a second without (32 -> 32)."""
    from mapx.models import BaseModel
    cfg = dict(F=39, V=2000, E=16, H=16, NL=0, NC=0, P=8, K=5)
    ai = dict(pg.extras_of("AutoInt"), attn_size=16)
    c = make_config(cfg, "RFD", None, backbone="AutoInt", compute_dtype="bf16")
    c.attn_size = 16
    torch.manual_seed(39)
    model = BaseModel.from_config(c).to(DEV)
    assert model.self_attention[0].W_res is not None and model.self_attention[1].W_res is None
    g = torch.Generator().manual_seed(39)
    batch = dict(ids=torch.randint(10, cfg["V"], (96, 39), generator=g),
                 labels=(torch.rand(96, 39, generator=g) < 0.3).float())
    params = {n: p.detach().cpu().numpy() for n, p in model.named_parameters()}
    pre = {}
    loss_x, logits_x, _ = BR.step("AutoInt", "RFD", params, batch, ai=ai, preacts=pre)
    _compare("bf16 AutoInt RFD F=39", model, "AutoInt", "RFD", params, batch, 0, ai, (loss_x, logits_x, pre))


@pytest.mark.parametrize("K,N", [(1001, 64), (37, 40)])
def test_bf16_linear_with_an_input_width_that_is_not_a_multiple_of_8(K, N):
    """DeepFM's heads read cat([dnn, lr + fm]) — H + 1 columns.  From 256 rows on layers._Linear pads x and the
    weight's bf16 shadow with zero columns to the next multiple of 8 (the bf16 GEMM's 16-byte operand chunks), as it
    does in fp32 mode, and cuts the gradients back.  Inputs are bf16-representable, the reference is float64 on the
    same values.  Bounds: a sum of n products accumulated in fp32 in any order is off by at most n 2^-24 sum |terms|
    (the products of two bf16 values are exact in fp32); a bf16 output adds 2^-8 |ref| (one rounding)."""
    from mapx import layers, ops
    M, u = 512, 2.0 ** -24
    torch.manual_seed(K)
    lin = layers.HipLinear(K, N, out_fp32=True).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(lin.weight.to(BF).float())
    x = torch.randn(M, K, device=DEV).to(BF).requires_grad_(True)
    r = torch.randn(M, N, device=DEV).to(BF).float()          # (the fp32 gradient of the logits is cast to bf16)
    xd, wd, bd, rd = x.detach().double(), lin.weight.detach().double(), lin.bias.detach().double(), r.double()

    def check(what, got, ref, n, scale, half):
        bound = (n + 1) * u * scale + (2.0 ** -8 * ref.abs() if half else 0.0) + 1e-30
        ratio = float(((got.double() - ref).abs() / bound).max())
        print(f"{what}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (what, ratio)

    for slot in (None, torch.zeros_like(lin.weight)):
        x.grad = lin.weight.grad = lin.bias.grad = None
        if slot is not None:
            lin.weight._mapx_grad = slot           # the optimizer-owned slot: dW is copied into it, autograd gets None
        y = lin(x)
        assert y.dtype == torch.float32 and y.shape == (M, N)
        (y * r).sum().backward()
        ops.flush_deferred()
        check("y", y.detach(), xd @ wd.T + bd, K, xd.abs() @ wd.abs().T + bd.abs(), False)
        assert x.grad.dtype == BF and x.grad.shape == (M, K)
        check("dX", x.grad, rd @ wd, N, rd.abs() @ wd.abs(), True)
        dw = lin.weight.grad if slot is None else slot
        assert (lin.weight.grad is None) == (slot is not None) and dw.dtype == torch.float32
        check("dW", dw, rd.T @ xd, M, rd.abs().T @ xd.abs(), False)
        check("db", lin.bias.grad, rd.sum(0), M, rd.abs().sum(0), False)


# --------------------------------------------------------------------------- dropout, graphs, checkpoints: the Trainer
CFG = dict(F=23, V=300, E=16, H=32, NL=2, NC=0, P=32, K=25)
B = 64


def _config(backbone, mode, cnt=None, rate=0.0, compute_dtype="bf16"):
    c = make_config(CFG, mode, cnt, backbone=backbone, compute_dtype=compute_dtype)
    if backbone == "AutoInt":
        for k, v in dict(num_attn_layers=2, num_attn_heads=2, attn_size=8, res_conn=True, attn_scale=True,
                         attn_probs_dropout_rate=rate).items():
            setattr(c, k, v)
    return c


def _start(backbone, mode, data, out_dir, rate=0.0, seed=5):
    from mapx.models import BaseModel
    torch.manual_seed(seed)
    config = _config(backbone, mode, data[2], rate)
    return H.make_trainer(config, BaseModel.from_config(config), mode, data, out_dir, B, 1, B, begin=True)


def test_bf16_autoint_dropout_eval_is_the_rate_zero_model_and_replays_draw_new_masks(tmp_path):
    from mapx.models import BaseModel
    data = H.synth_data(B * 4, CFG["F"], CFG["V"], seed=8)
    torch.manual_seed(2)
    m1 = BaseModel.from_config(_config("AutoInt", "MFP", data[2], rate=0.1)).to(DEV)
    m0 = BaseModel.from_config(_config("AutoInt", "MFP", data[2], rate=0.0)).to(DEV)
    m0.load_state_dict(m1.state_dict())
    ids = torch.from_numpy(data[0][:B]).to(DEV)
    m0.eval()
    m1.eval()
    with torch.no_grad():
        x0, x1 = m0.self_attention(m0.embed(ids)), m1.self_attention(m1.embed(ids))
    assert x0.dtype == BF and torch.equal(x0, x1) and bool(torch.isfinite(x1.float()).all())
    # the captured step replayed on the same batch: another loss each time (the masks follow the step counter)
    tr, model, batches = _start("AutoInt", "MFP", data, str(tmp_path), rate=0.1)
    tr.use_graph = True
    X, Y = batches[0]
    losses = [float(tr.run_step("mfp", X, Y)[0]) for _ in range(tr.GRAPH_AFTER + 3)]      # eager, capture, two replays
    assert H.captured(tr), "no step was captured"
    assert all(math.isfinite(x) for x in losses) and len(set(losses[-2:])) == 2, losses


@pytest.mark.parametrize("backbone,mode", [("DeepFM", "MFP"), ("AutoInt", "CTR")])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(backbone, mode, tmp_path):
    """Three AdamW steps from the captured graph (behind the Trainer's three eager warm-up steps) against six eager
    ones: the same losses and the same state, bit for bit.  The checkpoint
    holds fp32 tensors only under the keys of the fp32 model (the reference's manifest) and loads into one; every
    dense weight's bf16 shadow is the rounded master weight."""
    from mapx.models import BaseModel
    data = H.synth_data(B * 6, CFG["F"], CFG["V"], seed=3)

    def run(use_graph):
        tr, model, batches = _start(backbone, mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool(H.captured(tr)) == use_graph
        tr.optimizer.flush()
        for p in tr.optimizer.dense_params:
            if p.dim() == 2:
                assert torch.equal(p._mapx_bf16, p.detach().to(BF))
        if backbone == "AutoInt":
            assert all(getattr(m.weight, "_mapx_bf16", None) is not None
                       for layer in model.self_attention for m in (layer.W_q, layer.W_k, layer.W_v))
        tr.save_model(str(tmp_path / str(use_graph)))
        return losses, H.model_state(model)

    H.graph_vs_eager(run)
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    H.assert_checkpoint_is_fp32(ck, BaseModel.from_config(_config(backbone, mode, data[2], compute_dtype="fp32")))


def test_run_py_autoint_bf16_pretrain_then_finetune(tmp_path):
    """--model_name=autoint --compute_dtype bf16 at the reference's default attention dropout (0.1, not passed)."""
    common = ["--model_name=autoint", "--embed_size=16", "--num_attn_layers=2", "--num_attn_heads=2", "--attn_size=8",
              "--res_conn=True", "--logging_steps=3", "--compute_dtype", "bf16"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"], ["--use_lr=True"])
    assert all(v.dtype != BF for v in sd.values())
    attn = sorted(k for k in sd if k.startswith("self_attention."))
    assert len(attn) == 2 * 3
    assert "attn_probs_dropout_rate = 0.1" in open(tmp_path / "out" / "pretrain" / "results.log").read()
    for k in attn:
        assert f"Load tensor: {k}," in log, k
    H.finite_metrics(log)
