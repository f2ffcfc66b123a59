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
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_trans_ref as TR
import trans_params as tp
from test_bf16_trans_host import CASES, CFG, EPS, IDS, load, reference
from util import check_pattern, hook_relu_pattern

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT_INVARIANT = {"field_reduction_attn.2.bias": "field_reduction_attn.2.weight"}


def _build(cfg, mode, variant, params=None, feat_count=None, **over):
    from mapx.models import build_backbone
    model = build_backbone(tp.make_config(cfg, mode, variant, feat_count, **dict(dict(compute_dtype="bf16"), **over)))
    if params is not None:
        with torch.no_grad():
            sd = model.state_dict()
            for k, v in params.items():
                sd[k].copy_(torch.from_numpy(v))
    return model.to(DEV)


def _hooks(model):
    """-> (ReLU masks by layer, dtypes of the trunk tensors, the heads' logits), all filled by forward hooks."""
    from mapx.layers import HipLayerNorm, HipLinear, MLPBlock, TransformerEncoderLayer
    masks, dtypes, logits = hook_relu_pattern(model), {}, {}
    for name, mod in model.named_modules():
        trunk = isinstance(mod, (TransformerEncoderLayer, HipLayerNorm, MLPBlock)) or \
            (isinstance(mod, HipLinear) and name.startswith("encoder."))
        if trunk:
            mod.register_forward_hook(lambda m, i, o, name=name: dtypes.__setitem__(name, o.dtype))
    if hasattr(model, "mfp_criterion"):
        model.mfp_criterion.return_logits = True
        model.mfp_criterion.register_forward_hook(lambda m, i, o: logits.__setitem__("out", o[1].detach()))
    if hasattr(model, "pred_rfd"):
        model.pred_rfd["2"].register_forward_hook(lambda m, i, o: logits.__setitem__("out", o.detach()))
    return masks, dtypes, logits


def _all_grads(model):
    tab = model.table_parameter_ids()
    names = {id(p): n for n, p in model.named_parameters()}
    out = {n: p.grad for n, p in model.named_parameters() if id(p) not in tab}
    for table in model.row_tables():
        g0, g1 = table.dense_grad()
        out[names[id(table.p0)]] = g0
        if g1 is not None:
            out[names[id(table.p1)]] = g1
    return out


def _forward(model, mode, batch):
    ids = batch["ids"].to(DEV)
    if mode == "MFP":
        return model(input_ids=ids, labels=batch["labels"].to(DEV), masked_index=batch["masked_index"].to(DEV),
                     noise_samples=batch["noise"].to(DEV))
    if mode == "RFD":
        return model(input_ids=ids, labels=batch["labels"].to(DEV))
    return model(input_ids=ids, labels=batch["y"].to(DEV))


def _err(name, got, ref):
    """Error of a gradient as a share of its tensor's scale (of the weight's, for the shift-invariant bias)."""
    scale_of = ref[SHIFT_INVARIANT.get(name, name)]
    want = np.asarray(ref[name], dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max()
                 / max(np.abs(scale_of).max(), 1e-30))


def _compare(what, model, mode, params, batch, T, eps, exact, fixture=None):
    """Runs the bf16 step and the checks of the module docstring.  exact = (loss, logits, preacts) of the float64
    restatement on its own pattern; fixture = (loss, logits) of the reference, when there is one."""
    from mapx import ops
    masks, dtypes, logits = _hooks(model)
    model.train()
    out = _forward(model, mode, batch)
    loss = out[0]
    got_logits = out[1] if mode == "CTR" else logits["out"]
    # what is bf16 and what is not
    assert dtypes and all(d == BF for d in dtypes.values()), dtypes
    assert model.embed.compute_dtype == BF
    assert loss.dtype == torch.float32 and got_logits.dtype == torch.float32
    loss.backward()
    ops.flush_deferred()
    grads = _all_grads(model)
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values()), \
        {n: None if g is None else g.dtype for n, g in grads.items()}
    loss_x, logits_x, pre = exact
    loss_f, logits_f = fixture if fixture is not None else (loss_x, logits_x)
    e_loss = abs(float(loss.detach()) - loss_f) / abs(loss_f)
    e_logits = TR.rel(got_logits.detach().cpu().numpy(), logits_f)
    print(f"[{what}] loss {float(loss.detach()):.6f} vs {loss_f:.6f} ({e_loss:.2e}); logits {e_logits:.2e} of scale")
    assert e_loss <= 1e-2 and e_logits <= 1e-2
    # the step's own ReLU pattern, then every gradient on that pattern
    flips = check_pattern(masks, pre, what)
    _, _, ref = TR.step(mode, params, batch, T, eps, relu_masks=masks)
    _, _, emu = TR.step(mode, params, batch, T, eps, relu_masks=masks, emulate=True)
    assert set(ref) == set(grads), (sorted(ref), sorted(grads))
    rows, fails = [], []
    for n, g in grads.items():
        e, e_emul = _err(n, g.cpu().numpy(), ref), _err(n, emu[n], ref)
        bound = max(1e-2, 2 * e_emul)
        rows.append((e / bound, n, e, e_emul, bound))
        if not e <= bound:
            fails.append(f"{n}: {e:.3e} of scale > {bound:.3e} (e_emul {e_emul:.3e})")
    rows.sort(reverse=True)
    print(f"[{what}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units on the other side of the kink; "
          f"worst gradient error {max(r[2] for r in rows):.2e} of scale, worst e_emul {max(r[3] for r in rows):.2e}; "
          f"closest to its bound: {rows[0][1]} measured {rows[0][2]:.2e} e_emul {rows[0][3]:.2e} bound {rows[0][4]:.2e}")
    assert not fails, fails


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


def _data(steps, seed):
    from mapx.dataset import synth_table
    ids, labels, _, _ = synth_table(B * steps, TCFG["F"], TCFG["V"], seed=seed)
    return ids, labels, np.bincount(ids.reshape(-1), minlength=TCFG["V"]).astype(np.float32)


def _start(mode, data, out_dir, seed=5, **over):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    ids, labels, cnt = data
    torch.manual_seed(seed)
    config = _config(mode, cnt, **over)
    model = build_backbone(config)
    targs = TrainingArguments(output_dir=out_dir, per_gpu_train_batch_size=B, per_gpu_eval_batch_size=B,
                              learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2, num_train_epochs=1,
                              pretrain=mode != "CTR", pt_type="MFP", sampling_method="randint", mask_ratio=0.3,
                              logging_steps=7, seed=11, patience=100)
    targs._device = torch.device(DEV)
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:B], labels[:B]))
    train = tr._begin("test")
    model.train()
    return tr, model, list(train.batches(B, True, tr._generator(), (0, 1)))


# --------------------------------------------------------------------------- 8. dropout
def test_bf16_trans_dropout_eval_is_the_rate_zero_model_and_replays_draw_new_masks(tmp_path):
    from mapx.models import build_backbone
    data = _data(4, seed=8)
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
    assert [g for g in tr._graphs.values() if not isinstance(g, int)], "no step was captured"
    assert all(math.isfinite(x) for x in losses) and len(set(losses[-2:])) == 2, losses


# --------------------------------------------------------------------------- 9. graph replay, checkpoint, run.py
@pytest.mark.parametrize("mode,over", [("MFP", {}), ("CTR", PRE_NORM)], ids=["MFP-postnorm-relu", "CTR-prenorm-gelu"])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(mode, over, tmp_path):
    """Six AdamW steps with the captured graph (behind the Trainer's eager warm-up steps) against six eager ones: the
    same losses and the same state, bit for bit.  The checkpoint holds fp32 tensors only under the keys of the fp32
    model and loads into one; every 2-D dense weight's bf16 shadow is the rounded master weight."""
    from mapx.models import BaseModel
    data = _data(6, seed=3)
    runs = []
    for use_graph in (True, False):
        tr, model, batches = _start(mode, data, str(tmp_path / str(use_graph)), **over)
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool([g for g in tr._graphs.values() if not isinstance(g, int)]) == use_graph
        tr.optimizer.flush()
        for p in tr.optimizer.dense_params:
            if p.dim() == 2:
                assert torch.equal(p._mapx_bf16, p.detach().to(BF))
        assert all(getattr(layer.self_attn.in_proj_weight, "_mapx_bf16", None) is not None
                   for layer in model.encoder.layers)
        tr.save_model(str(tmp_path / str(use_graph)))
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    fp32_model = BaseModel.from_config(_config(mode, data[2], compute_dtype="fp32", **over))
    assert set(ck) == set(fp32_model.state_dict())
    assert all(v.dtype != BF and (not v.dtype.is_floating_point or v.dtype == torch.float32) for v in ck.values())
    fp32_model.load_state_dict(ck)


def _run_py(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "map-code_amd", "run.py")] + args
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_run_py_trans_bf16_pretrain_then_finetune(tmp_path):
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=4000, num_fields=23, vocab=2000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3", "--model_name=trans", "--embed_size=16",
              "--hidden_size=16", "--num_hidden_layers=2", "--num_attn_heads=2", "--intermediate_size=64",
              "--hidden_dropout_rate=0.1", "--logging_steps=3", "--compute_dtype", "bf16"]
    out = str(tmp_path / "out" / "mfp")
    r = _run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=1", "--lr_sched=cosine",
                 "--weight_decay=5e-2", "--pt_type=MFP", "--sampling_method=randint", "--mask_ratio=0.3",
                 "--pt_neg_num=25", "--proj_size=32"] + common, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = os.path.join(out, f"{(3200 + 511) // 512}.model")
    sd = torch.load(ckpt)
    assert all(v.dtype != BF for v in sd.values())
    enc = sorted(k for k in sd if k.startswith("encoder."))
    assert len(enc) == 2 * 12 and "encoder.layers.1.self_attn.in_proj_weight" in enc
    fo = str(tmp_path / "out" / "finetune")
    r2 = _run_py(["--finetune", f"--pretrained_model_path={ckpt}", f"--output_dir={fo}", "--num_train_epochs=1",
                  "--lr_sched=const", "--weight_decay=1e-1", "--output_reduction=attn,fc", "--use_lr=True"] + common,
                 str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-3000:]
    log = open(os.path.join(fo, "results.log")).read()
    for k in enc:
        assert f"Load tensor: {k}," in log, k
    for key in ("eval_auc", "eval_loss"):
        vals = [float(v) for v in re.findall(rf"{key}\W+([-+0-9.eE]+|nan|inf)", log)]
        assert vals and all(math.isfinite(v) for v in vals), (key, vals)
