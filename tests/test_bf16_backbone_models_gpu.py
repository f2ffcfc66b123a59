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
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_backbones_ref as BR
import paramgen as pg
from test_bf16_backbones_host import CASE, CASES, IDS, family, reference
from util import build_model, check_pattern, hook_relu_pattern, load_case, make_config, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hooks(model):
    """-> (ReLU masks by layer, dtypes of the trunk tensors, the heads' logits), all filled by forward hooks."""
    from mapx.layers import MLPBlock, MultiHeadSelfAttention
    masks, dtypes, logits = hook_relu_pattern(model), {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, MultiHeadSelfAttention):
            def attn_hook(m, i, o, name=name):          # (a hook that returns a value would replace the output)
                masks[name] = (o.detach() > 0).cpu()
                dtypes[name] = o.dtype
            mod.register_forward_hook(attn_hook)
        elif isinstance(mod, MLPBlock):
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


def _compare(what, model, fam, mode, params, batch, num_hidden, ai, exact, fixture=None):
    """Runs the bf16 step and the checks of the module docstring.  exact = (loss, logits, preacts) of the float64
    restatement on its own pattern; fixture = (loss, logits | None) of the reference, when there is one."""
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
    grads = _all_grads(model)
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values()), \
        {n: None if g is None else g.dtype for n, g in grads.items()}
    # loss and logits
    loss_x, logits_x, pre = exact
    loss_f, logits_f = fixture if fixture is not None else (loss_x, None)
    logits_f = logits_x if logits_f is None else logits_f
    e_loss = abs(float(loss.detach()) - loss_f) / abs(loss_f)
    e_logits = BR.rel(got_logits.detach().cpu().numpy(), logits_f)
    print(f"[{what}] loss {float(loss.detach()):.6f} vs {loss_f:.6f} ({e_loss:.2e}); logits {e_logits:.2e} of scale")
    assert e_loss <= 1e-2 and e_logits <= 1e-2
    # the step's own ReLU pattern, then every gradient on that pattern
    flips = check_pattern(masks, pre, what)
    _, _, ref = BR.step(fam, mode, params, batch, num_hidden=num_hidden, ai=ai, relu_masks=masks)
    _, _, emu = BR.step(fam, mode, params, batch, num_hidden=num_hidden, ai=ai, relu_masks=masks, emulate=True)
    assert set(ref) == set(grads), (sorted(ref), sorted(grads))
    rows, fails = [], []
    for n, g in grads.items():
        e, e_emul = BR.rel(g.cpu().numpy(), ref[n]), BR.rel(emu[n], ref[n])
        bound = max(1e-2, 2 * e_emul)
        rows.append((e / bound, n, e, e_emul, bound))
        if not e <= bound:
            fails.append(f"{n}: {e:.3e} of scale > {bound:.3e} (e_emul {e_emul:.3e})")
    rows.sort(reverse=True)
    worst_e = max(r[2] for r in rows)
    worst_emul = max(r[3] for r in rows)
    print(f"[{what}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units on the other side of the kink; "
          f"worst gradient error {worst_e:.2e} of scale, worst e_emul {worst_emul:.2e}; closest to its bound: "
          f"{rows[0][1]} measured {rows[0][2]:.2e} e_emul {rows[0][3]:.2e} bound {rows[0][4]:.2e}")
    assert not fails, fails


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


def _data(steps, seed):
    from mapx.dataset import synth_table
    ids, labels, _, _ = synth_table(B * steps, CFG["F"], CFG["V"], seed=seed)
    return ids, labels, np.bincount(ids.reshape(-1), minlength=CFG["V"]).astype(np.float32)


def _start(backbone, mode, data, out_dir, rate=0.0, seed=5):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    ids, labels, cnt = data
    torch.manual_seed(seed)
    config = _config(backbone, mode, cnt, rate)
    model = BaseModel.from_config(config)
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


def test_bf16_autoint_dropout_eval_is_the_rate_zero_model_and_replays_draw_new_masks(tmp_path):
    from mapx.models import BaseModel
    data = _data(4, seed=8)
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
    assert [g for g in tr._graphs.values() if not isinstance(g, int)], "no step was captured"
    assert all(math.isfinite(x) for x in losses) and len(set(losses[-2:])) == 2, losses


@pytest.mark.parametrize("backbone,mode", [("DeepFM", "MFP"), ("AutoInt", "CTR")])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(backbone, mode, tmp_path):
    """Three AdamW steps from the captured graph (behind the Trainer's three eager warm-up steps) against six eager
    ones: the same losses and the same state, bit for bit.  The checkpoint
    holds fp32 tensors only under the keys of the fp32 model (the reference's manifest) and loads into one; every
    dense weight's bf16 shadow is the rounded master weight."""
    from mapx.models import BaseModel
    data = _data(6, seed=3)
    runs = []
    for use_graph in (True, False):
        tr, model, batches = _start(backbone, mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool([g for g in tr._graphs.values() if not isinstance(g, int)]) == use_graph
        tr.optimizer.flush()
        for p in tr.optimizer.dense_params:
            if p.dim() == 2:
                assert torch.equal(p._mapx_bf16, p.detach().to(BF))
        if backbone == "AutoInt":
            assert all(getattr(m.weight, "_mapx_bf16", None) is not None
                       for layer in model.self_attention for m in (layer.W_q, layer.W_k, layer.W_v))
        tr.save_model(str(tmp_path / str(use_graph)))
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    fp32_model = BaseModel.from_config(_config(backbone, mode, data[2], compute_dtype="fp32"))
    assert set(ck) == set(fp32_model.state_dict())
    assert all(v.dtype != BF and (not v.dtype.is_floating_point or v.dtype == torch.float32) for v in ck.values())
    fp32_model.load_state_dict(ck)


def _run_py(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "map-code_amd", "run.py")] + args
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_run_py_autoint_bf16_pretrain_then_finetune(tmp_path):
    """--model_name=autoint --compute_dtype bf16 at the reference's default attention dropout (0.1, not passed)."""
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=4000, num_fields=23, vocab=2000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3", "--model_name=autoint", "--embed_size=16",
              "--num_attn_layers=2", "--num_attn_heads=2", "--attn_size=8", "--res_conn=True", "--logging_steps=3",
              "--compute_dtype", "bf16"]
    out = str(tmp_path / "out" / "mfp")
    r = _run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=1", "--lr_sched=cosine",
                 "--weight_decay=5e-2", "--pt_type=MFP", "--sampling_method=randint", "--mask_ratio=0.3",
                 "--pt_neg_num=25", "--proj_size=32"] + common, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = os.path.join(out, f"{(3200 + 511) // 512}.model")
    sd = torch.load(ckpt)
    assert all(v.dtype != BF for v in sd.values())
    attn = sorted(k for k in sd if k.startswith("self_attention."))
    assert len(attn) == 2 * 3
    log = open(os.path.join(out, "results.log")).read()
    assert "attn_probs_dropout_rate = 0.1" in log
    fo = str(tmp_path / "out" / "finetune")
    r2 = _run_py(["--finetune", f"--pretrained_model_path={ckpt}", f"--output_dir={fo}", "--num_train_epochs=1",
                  "--lr_sched=const", "--weight_decay=1e-1", "--use_lr=True"] + common, str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-3000:]
    log = open(os.path.join(fo, "results.log")).read()
    for k in attn:
        assert f"Load tensor: {k}," in log, k
    for key in ("eval_auc", "eval_loss"):
        vals = [float(v) for v in re.findall(rf"{key}\W+([-+0-9.eE]+|nan|inf)", log)]
        assert vals and all(math.isfinite(v) for v in vals), (key, vals)
