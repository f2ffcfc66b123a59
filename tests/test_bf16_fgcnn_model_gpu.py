"""FGCNN in compute_dtype=bf16 at model level.

Parity: the four fixture cases of the reference's own class (B = 64, F = 25, E = 16; FGCNN x MFP / RFD / CTR with tanh
and a second table, FGCNNShare x CTR with relu and one table).  The loss is within 1e-2 of the fixture's.  The step's own
decisions — the ReLU pattern of every fused-ReLU layer, the pooling winners (the uint8 argmax each stage saved) and,
conv_act relu, the sign of every pooled value — are read from the model; they may differ from those of the emulated,
free-running float64 restatement (tests/bf16_fgcnn_ref.py, emulate=True) in at most 1 decision in 1000: the two differ
only where an fp32 and a float64 accumulation round to different bf16 values AND that ulp decides a comparison
(tests/test_bf16_fgcnn_host.py measures 0 for fp32 torch on these fixtures).  Logits and every gradient are then compared
with the plain float64 restatement ON THOSE DECISIONS, per tensor, as a share of the tensor's scale:
max(1e-2, 2 * e_emul), e_emul = the emulated restatement against the plain one on the same decisions (margin 2: the
kernels accumulate in fp32 and in another order than the emulation's float64).  The conv-bias gradients are zero in exact
arithmetic and exempt from the relative rule: they are held to what tests/test_fgcnn_model_gpu.py::test_reference_fixture
applies to the same entries (util.assert_digest against the fixture).  The batch-norm buffers after one training forward
and the eval-mode logits are compared with the fixture at the same per-tensor rule."""
import math
import os

import pytest
import torch

import bf16_fgcnn_ref as GR
import fgcnn_params as fp
import model_harness as H
import paramgen as pg
from util import assert_digest, hook_relu_pattern

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CFG = pg.CASES[fp.CASE]
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]
SMALL = dict(channels="3,4", kernel_heights="3,5", pooling_sizes="2,2", recombined_channels="2,1")


def _build(mode, variant, params, feat_count):
    from mapx.models import build_backbone
    model = build_backbone(fp.make_config(CFG, mode, variant, feat_count, compute_dtype="bf16"))
    return H.load_params(model, params).to(DEV)


def _hook_stages(model):
    """-> list filled per stage with (saved z, saved uint8 argmax, pooled y), read from the stage's autograd node when
    the recombine layer is entered."""
    seen = []

    def pre(mod, args):
        node = args[0].grad_fn
        if node is None:                   # (eval mode under no_grad: nothing is saved)
            return
        while node is not None and "_ConvBnActPool" not in type(node).__name__:
            node = node.next_functions[0][0]
        x, w, z, idx, *_ = node.saved_tensors
        seen.append((z.detach(), idx.detach().cpu(), args[0].detach().reshape(idx.shape).cpu()))

    for rec in model.fgcnn_layer.recombine_layers:
        rec["0"].register_forward_pre_hook(pre)
    return seen


def _rule(what, got, ref, emu, rows):
    e, e_emul = GR.rel(got, ref), GR.rel(emu, ref)
    bound = max(1e-2, 2 * e_emul)
    rows.append((e / bound, what, e, e_emul, bound))
    return None if e <= bound else f"{what}: {e:.3e} of scale > {bound:.3e} (e_emul {e_emul:.3e})"


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_bf16_step_vs_fixture_and_float64_restatement(mode, variant):
    from mapx import ops
    z = GR.fixture(mode, variant)
    inp = pg.make_inputs(fp.CASE, CFG)
    params = fp.make_params(CFG, mode, variant)
    batch = GR.fixture_batch(mode, CFG, inp)
    model = _build(mode, variant, params, inp["feat_count"] if mode == "MFP" else None)
    masks, stages, seen = hook_relu_pattern(model), _hook_stages(model), {}
    model.fgcnn_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("new", o))
    model.train()
    ids = batch["ids"].to(DEV)
    if mode == "MFP":
        model.mfp_criterion.return_logits = True
        model.mfp_criterion.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o[1].detach()))
        out = model(input_ids=ids, labels=batch["labels"].to(DEV), masked_index=batch["masked_index"].to(DEV),
                    noise_samples=batch["noise"].to(DEV))
    elif mode == "RFD":
        model.pred_rfd["2"].register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach()))
        out = model(input_ids=ids, labels=batch["labels"].to(DEV))
    else:
        out = model(input_ids=ids, labels=batch["y"].to(DEV))
        seen["logits"] = out[1].detach()
    loss, logits = out[0], seen["logits"]
    # what is bf16 and what is not
    assert seen["new"].dtype == BF and all(s[0].dtype == BF for s in stages) and len(stages) == 2
    assert model.embed.compute_dtype == BF and loss.dtype == torch.float32 and logits.dtype == torch.float32
    loss.backward()
    ops.flush_deferred()
    grads = H.all_grads(model)
    assert set(grads) == set(params)
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values())
    e_loss = abs(float(loss.detach()) - float(z["out/loss"])) / abs(float(z["out/loss"]))
    print(f"[bf16 {variant} {mode}] loss {float(loss.detach()):.6f} vs {float(z['out/loss']):.6f} ({e_loss:.2e})")
    assert e_loss <= 1e-2
    # the step's own decisions against the emulated, free-running restatement's
    winners = [s[1] for s in stages]
    relu = fp.VARIANTS[variant]["conv_act"] == "relu"
    stage_on = [s[2].float() > 0 for s in stages] if relu else None
    free = GR.step(CFG, mode, variant, params, batch, emulate=True)
    assert set(masks) == set(free.preacts), (sorted(masks), sorted(free.preacts))
    units = sum(v.numel() for v in free.preacts.values())
    d_relu = sum(int((masks[k] != (free.preacts[k] > 0)).sum()) for k in masks)
    d_pool, pooled = 0, 0
    for i, w in enumerate(winners):
        live = torch.ones_like(w, dtype=torch.bool) if not relu else (stage_on[i] | free.stage_on[i])
        d_pool += int(((w != free.winners[i]) & live).sum())
        pooled += w.numel()
        if relu:
            d_relu += int((stage_on[i] != free.stage_on[i]).sum())
            units += w.numel()
    print(f"[bf16 {variant} {mode}] decisions other than the emulated restatement's: {d_relu} of {units} ReLU units, "
          f"{d_pool} of {pooled} pooling winners")
    assert (d_relu + d_pool) * 1000 <= units + pooled
    # logits and every gradient on those decisions
    ref = GR.step(CFG, mode, variant, params, batch, relu_masks=masks, winners=winners, stage_on=stage_on)
    emu = GR.step(CFG, mode, variant, params, batch, relu_masks=masks, winners=winners, stage_on=stage_on, emulate=True)
    rows = []
    fails = [_rule("logits", logits.cpu().numpy(), ref.logits, emu.logits, rows)]
    for n, g in grads.items():
        if ".conv_layers." in n and n.endswith(".0.bias"):           # zero in exact arithmetic: the fixture's entry
            print(f"[bf16 {variant} {mode}] {n}: largest |db| {float(g.abs().max()):.3e}")
            assert_digest(z, "grad", n, g.cpu().numpy())
            continue
        fails.append(_rule(n, g.cpu().numpy(), ref.grads[n], emu.grads[n], rows))
    # the batch-norm buffers after ONE training forward, against the fixture
    sd = model.state_dict()
    for k in fp.bn_buffer_names(CFG, variant):
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(z[f"bn/{k}"]) == 1
        else:
            assert sd[k].dtype == torch.float32
            e_emul = GR.rel(emu.buffers[k], ref.buffers[k])
            e, bound = GR.rel(sd[k].cpu().numpy(), z[f"bn/{k}"]), max(1e-2, 2 * e_emul)
            rows.append((e / bound, k, e, e_emul, bound))
            fails.append(None if e <= bound else f"{k}: {e:.3e} > {bound:.3e}")
    # eval mode on other running statistics: the buffers are left alone, the logits are the fixture's
    H.load_params(model, fp.eval_buffers(CFG, variant))
    model.eval()
    before = {k: sd[k].clone() for k in fp.bn_buffer_names(CFG, variant)}
    with torch.no_grad():
        if mode == "CTR":
            ev = model(input_ids=ids)[0]
        elif mode == "RFD":
            from mapx.layers import inner_product
            combined = model.combined_features(ids)
            ev = model.pred_rfd(torch.cat([combined.flatten(1), inner_product(combined)], dim=1))
        else:
            ev = None
            assert model.combined_features(ids).dtype == BF
    if ev is not None:
        assert ev.dtype == torch.float32
        args = (CFG, mode, variant, params, batch, fp.eval_buffers(CFG, variant))
        e_emul = GR.rel(GR.eval_logits(*args, emulate=True), GR.eval_logits(*args))
        e, bound = GR.rel(ev.cpu().numpy(), z["eval/logits"]), max(1e-2, 2 * e_emul)
        rows.append((e / bound, "eval logits", e, e_emul, bound))
        fails.append(None if e <= bound else f"eval logits: {e:.3e} > {bound:.3e}")
    for k, v in before.items():
        assert torch.equal(model.state_dict()[k], v), k
    rows.sort(reverse=True)
    gr = [r for r in rows if r[1] in grads]
    print(f"[bf16 {variant} {mode}] logits {[r[2] for r in rows if r[1] == 'logits'][0]:.2e} of scale; worst gradient "
          f"error {max(r[2] for r in gr):.2e}, worst e_emul {max(r[3] for r in gr):.2e}; closest to its bound: "
          f"{rows[0][1]} measured {rows[0][2]:.2e} e_emul {rows[0][3]:.2e} bound {rows[0][4]:.2e}")
    fails = [f for f in fails if f]
    assert not fails, fails


# --------------------------------------------------------------------------- graphs, checkpoints: the Trainer
TCFG = dict(F=23, V=300, E=16, H=32, NL=2, NC=0, P=32, K=25)
B = 64


def _config(mode, variant, cnt=None, compute_dtype="bf16"):
    return fp.make_config(TCFG, mode, variant, cnt, compute_dtype=compute_dtype, **SMALL)


def _start(mode, variant, data, out_dir, seed=5):
    from mapx.models import build_backbone
    torch.manual_seed(seed)
    config = _config(mode, variant, data[2])
    return H.make_trainer(config, build_backbone(config), mode, data, out_dir, B, 1, B, begin=True)


def _gemm_weights(model):
    from mapx.layers import HipLinear
    return [m.weight for m in model.modules() if isinstance(m, HipLinear)]


@pytest.mark.parametrize("mode,variant", [("MFP", "FGCNN"), ("CTR", "FGCNNShare")], ids=["MFP", "CTR-Share"])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(mode, variant, tmp_path):
    """Six AdamW steps with the captured graph (behind the Trainer's eager warm-up steps) against six eager ones: the
    same losses and the same state, bit for bit, batch-norm buffers and num_batches_tracked included.  Every 2-D GEMM
    weight's bf16 shadow is the rounded master; the checkpoint holds fp32 tensors under the fp32 model's keys."""
    from mapx.models import BaseModel
    data = H.synth_data(B * 6, TCFG["F"], TCFG["V"], seed=3)

    def run(use_graph):
        tr, model, batches = _start(mode, variant, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool(H.captured(tr)) == use_graph
        tr.optimizer.flush()
        ws = _gemm_weights(model)
        assert len(ws) >= 3
        for w in ws:
            assert torch.equal(w._mapx_bf16, w.detach().to(BF))
        tr.save_model(str(tmp_path / str(use_graph)))
        return losses, H.model_state(model)

    (_, sa), _ = H.graph_vs_eager(run)
    tracked = [k for k in sa if k.endswith("num_batches_tracked")]
    assert len(tracked) == 2 and all(int(sa[k]) == 6 for k in tracked)
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    H.assert_checkpoint_is_fp32(ck, BaseModel.from_config(_config(mode, variant, data[2], compute_dtype="fp32")))


def test_bf16_resume_state_continues_bit_exactly(tmp_path):
    """6 steps == 3 steps + save_training_state + fresh trainer + load_training_state + 3 steps."""
    data = H.synth_data(B * 6, TCFG["F"], TCFG["V"], seed=4)

    def make():
        tr, model, batches = _start("MFP", "FGCNN", data, str(tmp_path), seed=9)
        tr.use_graph = False
        return tr, batches

    def after_load(tr):
        assert int(tr.model.state_dict()["fgcnn_layer.conv_layers.0.1.num_batches_tracked"]) == 3
        for w in _gemm_weights(tr.model):
            assert torch.equal(w._mapx_bf16, w.detach().to(BF))

    ref = H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"), after_load=after_load)
    assert int(ref["fgcnn_layer.conv_layers.1.1.num_batches_tracked"]) == 6


def test_run_py_fgcnn_bf16_pretrain_then_finetune(tmp_path):
    """run.py --model_name=fgcnn --compute_dtype bf16 on the tiny dataset of the fp32 round-trip test: MFP pretraining,
    then finetuning from that (fp32) checkpoint."""
    common = ["--model_name=fgcnn", "--embed_size=16", "--hidden_size=32", "--num_hidden_layers=2",
              "--hidden_dropout_rate=0.0", "--logging_steps=3", "--compute_dtype", "bf16"] \
        + [f"--{k}={v}" for k, v in SMALL.items()]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"], [])
    assert all(v.dtype != BF for v in sd.values())
    trunk = sorted(k for k in sd if k.startswith(("fgcnn_layer.", "fg_embed.", "embed.", "ip_layer.")))
    assert "fgcnn_layer.conv_layers.1.1.running_var" in trunk and "fg_embed.embedding.weight" in trunk
    assert int(sd["fgcnn_layer.conv_layers.0.1.num_batches_tracked"]) == (3200 + 511) // 512
    for k in trunk:
        assert f"Load tensor: {k}," in log, k
    H.finite_metrics(log)

