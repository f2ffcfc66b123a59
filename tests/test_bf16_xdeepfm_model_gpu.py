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
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_xdeepfm_ref as XR
import paramgen as pg
from test_bf16_xdeepfm_host import CASE, CASES, IDS, hidden_of, reference
from util import check_pattern, hook_relu_pattern, load_case, make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(cfg, mode, backbone, params=None, feat_count=None, **over):
    from mapx.models import build_backbone
    c = make_config(cfg, mode, feat_count, backbone=backbone, compute_dtype="bf16")
    for k, v in over.items():
        setattr(c, k, v)
    model = build_backbone(c)
    if params is not None:
        with torch.no_grad():
            sd = model.state_dict()
            for k, v in params.items():
                sd[k].copy_(torch.from_numpy(v))
    return model.to(DEV)


def _hooks(model):
    """-> (ReLU masks by layer, dtypes of the trunk tensors, the heads' logits), all filled by forward hooks."""
    from mapx.layers import CIN, MLPBlock
    masks, dtypes, logits = hook_relu_pattern(model), {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, (CIN, MLPBlock)):
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


def _compare(what, model, mode, params, batch, units, num_hidden, exact, fixture=None):
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
    print(f"[{what}] loss {float(loss.detach()):.6f} vs {loss_f:.6f} ({e_loss:.2e})")
    assert e_loss <= 1e-2
    if logits_f is not None:
        e_logits = XR.rel(got_logits.detach().cpu().numpy(), logits_f)
        print(f"[{what}] logits {e_logits:.2e} of scale")
        assert e_logits <= 1e-2
    # the step's own ReLU pattern, then every gradient on that pattern
    flips = check_pattern(masks, pre, what)
    _, _, ref = XR.step(mode, params, batch, units, num_hidden, relu_masks=masks)
    _, _, emu = XR.step(mode, params, batch, units, num_hidden, relu_masks=masks, emulate=True)
    assert set(ref) == set(grads), (sorted(ref), sorted(grads))
    rows, fails = [], []
    for n, g in grads.items():
        e, e_emul = XR.rel(g.cpu().numpy(), ref[n]), XR.rel(emu[n], ref[n])
        bound = max(1e-2, 2 * e_emul)
        rows.append((e / bound, n, e, e_emul, bound))
        if not e <= bound:
            fails.append(f"{n}: {e:.3e} of scale > {bound:.3e} (e_emul {e_emul:.3e})")
    rows.sort(reverse=True)
    print(f"[{what}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units on the other side of the kink; "
          f"worst gradient error {max(r[2] for r in rows):.2e} of scale, worst e_emul {max(r[3] for r in rows):.2e}; "
          f"closest to its bound: {rows[0][1]} measured {rows[0][2]:.2e} e_emul {rows[0][3]:.2e} bound {rows[0][4]:.2e}")
    assert not fails, fails


# --------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("backbone,mode", CASES, ids=IDS)
def test_bf16_step_vs_fixture_and_float64_restatement(backbone, mode):
    cfg, z, inp, params = load_case(CASE, mode, backbone)
    model = _build(cfg, mode, backbone, params, inp["feat_count"] if mode == "MFP" else None)
    loss_x, logits_x, _, pre = reference(backbone, mode)
    # (the RFD fixtures keep the accuracy of their logits only: those are compared with the restatement's)
    fixture = (float(z["out/loss"]), logits_x if mode == "RFD" else z["out/logits"])
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


def _data(steps, seed):
    from mapx.dataset import synth_table
    ids, labels, _, _ = synth_table(B * steps, TCFG["F"], TCFG["V"], seed=seed)
    return ids, labels, np.bincount(ids.reshape(-1), minlength=TCFG["V"]).astype(np.float32)


def _start(mode, data, out_dir, seed=5):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.models import build_backbone
    from mapx.trainer import Trainer
    ids, labels, cnt = data
    torch.manual_seed(seed)
    config = _config(mode, cnt)
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


@pytest.mark.parametrize("mode", ["MFP", "CTR"], ids=["MFP", "CTR-use_lr"])
def test_bf16_graph_replay_equals_eager_bitwise_and_the_checkpoint_is_fp32(mode, tmp_path):
    """Six AdamW steps with the captured graph (behind the Trainer's eager warm-up steps) against six eager ones: the
    same losses and the same state, bit for bit.  The checkpoint holds fp32 tensors only under the keys of the fp32
    model and loads into one; the CIN weights' bf16 shadows are the rounded master weights."""
    from mapx.models import BaseModel
    data = _data(6, seed=3)
    runs = []
    for use_graph in (True, False):
        tr, model, batches = _start(mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        assert tr.optimizer.bf16
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
        assert bool([g for g in tr._graphs.values() if not isinstance(g, int)]) == use_graph
        tr.optimizer.flush()
        for conv in model.cin.cin_layer.values():
            assert torch.equal(conv.weight._mapx_bf16, conv.weight.detach().to(BF))
        tr.save_model(str(tmp_path / str(use_graph)))
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ck = torch.load(os.path.join(str(tmp_path / "True"), "6.model"))
    fp32_model = BaseModel.from_config(_config(mode, data[2], compute_dtype="fp32"))
    assert set(ck) == set(fp32_model.state_dict())
    assert all(v.dtype != BF and (not v.dtype.is_floating_point or v.dtype == torch.float32) for v in ck.values())
    fp32_model.load_state_dict(ck)


def _run_py(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "map-code_amd", "run.py")] + args
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_run_py_xdeepfm_bf16_pretrain_then_finetune(tmp_path):
    """run.py --model_name=xDeepFM --compute_dtype bf16: RFD pretraining, then finetune with use_lr from that
    checkpoint."""
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=4000, num_fields=23, vocab=2000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3", "--model_name=xDeepFM", "--embed_size=16",
              "--hidden_size=64", "--num_hidden_layers=2", "--hidden_dropout_rate=0.0", "--logging_steps=3",
              "--cin_layer_units=16,8", "--compute_dtype", "bf16"]
    out = str(tmp_path / "out" / "rfd")
    r = _run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=1", "--lr_sched=cosine",
                 "--weight_decay=5e-2", "--pt_type=RFD", "--sampling_method=randint", "--mask_ratio=0.3",
                 "--RFD_replace=Unigram", "--proj_size=32"] + common, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = os.path.join(out, f"{(3200 + 511) // 512}.model")
    sd = torch.load(ckpt)
    assert all(v.dtype != BF for v in sd.values())
    assert tuple(sd["cin.cin_layer.layer_1.weight"].shape) == (16, 23 * 23, 1)
    assert tuple(sd["cin.cin_layer.layer_2.weight"].shape) == (8, 23 * 16, 1)
    fo = str(tmp_path / "out" / "finetune")
    r2 = _run_py(["--finetune", f"--pretrained_model_path={ckpt}", f"--output_dir={fo}", "--num_train_epochs=1",
                  "--lr_sched=const", "--weight_decay=1e-1", "--use_lr=True"] + common, str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-3000:]
    log = open(os.path.join(fo, "results.log")).read()
    assert "Load tensor: cin.cin_layer.layer_2.weight" in log
    for key in ("eval_auc", "eval_loss"):
        vals = [float(v) for v in re.findall(rf"{key}\W+([-+0-9.eE]+|nan|inf)", log)]
        assert vals and all(math.isfinite(v) for v in vals), (key, vals)
