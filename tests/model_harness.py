"""What the backbone model tests share: step plumbing, the bf16 step comparison, the Trainer set-up with its graph,
resume and checkpoint checks, and run.py as a child process.  Plain functions; what is specific to a backbone (shapes,
hooks, table names, shadows, counters) stays in that backbone's test file."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import torch

from bf16_backbones_ref import rel
from util import check_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ----------------------------------------------------------------------------- model and step plumbing
def load_params(model, params):
    """Copies a fixture's parameters (name -> numpy array) into the model's state."""
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    return model


def all_grads(model):
    """name -> gradient of every parameter; the row tables' sparse gradients as dense tensors."""
    tab = model.table_parameter_ids()
    names = {id(p): n for n, p in model.named_parameters()}
    out = {n: p.grad for n, p in model.named_parameters() if id(p) not in tab}
    for table in model.row_tables():
        g0, g1 = table.dense_grad()
        out[names[id(table.p0)]] = g0
        if g1 is not None:
            out[names[id(table.p1)]] = g1
    return out


def forward(model, mode, batch, device):
    ids = batch["ids"].to(device)
    if mode == "MFP":
        return model(input_ids=ids, labels=batch["labels"].to(device), masked_index=batch["masked_index"].to(device),
                     noise_samples=batch["noise"].to(device))
    if mode == "RFD":
        return model(input_ids=ids, labels=batch["labels"].to(device))
    return model(input_ids=ids, labels=batch["y"].to(device))


def hook_head_logits(model):
    """-> dict whose "out" the pretraining heads' forward hooks fill with their logits."""
    logits = {}
    if hasattr(model, "mfp_criterion"):
        model.mfp_criterion.return_logits = True
        model.mfp_criterion.register_forward_hook(lambda m, i, o: logits.__setitem__("out", o[1].detach()))
    if hasattr(model, "pred_rfd"):
        model.pred_rfd["2"].register_forward_hook(lambda m, i, o: logits.__setitem__("out", o.detach()))
    return logits


def capture_mfp_logits(crit, seen):
    """seen["logits"] = the MFP head's logits, whichever form of the head the model takes."""
    crit.return_logits = True
    for name in ("forward", "forward_with_encoder"):

        def keep(*a, _orig=getattr(crit, name), **k):
            out = _orig(*a, **k)
            seen["logits"] = out[1].detach()
            return out
        setattr(crit, name, keep)


def hook_dtypes(model, is_trunk):
    """-> dict filled by forward hooks: name -> output dtype of every module with is_trunk(name, module)."""
    dtypes = {}
    for name, mod in model.named_modules():
        if is_trunk(name, mod):
            mod.register_forward_hook(lambda m, i, o, name=name: dtypes.__setitem__(name, o.dtype))
    return dtypes


# ----------------------------------------------------------------------------- the bf16 step comparison
def rel_err(name, got, ref):
    """Error of gradient `name` as a share of its own scale."""
    return rel(got, ref[name])


def grad_bound_failures(errors, emul_errors):
    """Per tensor, as a share of its scale: the measured error may not exceed max(1e-2, 2 * e_emul), e_emul = the error
    of the CPU emulation of the roundings.  -> one line per tensor over its bound (a nan is over it)."""
    fails = []
    for n, e in errors.items():
        e_emul = emul_errors[n]
        bound = max(1e-2, 2 * e_emul)
        if not e <= bound:
            fails.append(f"{n}: {e:.3e} of scale > {bound:.3e} (e_emul {e_emul:.3e})")
    return fails


def compare_bf16_step(what, model, mode, batch, masks, restate, err, exact, fixture=None, *, is_trunk):
    """Runs the bf16 step and checks it.  masks = the step's hooked ReLU pattern (util.hook_relu_pattern and what the
    family adds); restate(relu_masks, emulate) -> the float64 restatement's gradients on that pattern; err(name, got,
    ref) -> a gradient's error as a share of scale; exact = (loss, logits, preacts) of the restatement on its own
    pattern; fixture = (loss, logits | None) of the reference, when there is one (None: the restatement's stand in)."""
    from mapx import ops
    dtypes, logits = hook_dtypes(model, is_trunk), hook_head_logits(model)
    model.train()
    out = forward(model, mode, batch, next(model.parameters()).device)
    loss = out[0]
    got_logits = out[1] if mode == "CTR" else logits["out"]
    # what is bf16 and what is not
    assert dtypes and all(d == BF for d in dtypes.values()), dtypes
    assert model.embed.compute_dtype == BF
    assert loss.dtype == torch.float32 and got_logits.dtype == torch.float32
    loss.backward()
    ops.flush_deferred()
    grads = all_grads(model)
    assert all(g is not None and g.dtype == torch.float32 for g in grads.values()), \
        {n: None if g is None else g.dtype for n, g in grads.items()}
    # loss and logits
    loss_x, logits_x, pre = exact
    loss_f, logits_f = fixture if fixture is not None else (loss_x, None)
    logits_f = logits_x if logits_f is None else logits_f
    e_loss = abs(float(loss.detach()) - loss_f) / abs(loss_f)
    e_logits = rel(got_logits.detach().cpu().numpy(), logits_f)
    print(f"[{what}] loss {float(loss.detach()):.6f} vs {loss_f:.6f} ({e_loss:.2e}); logits {e_logits:.2e} of scale")
    assert e_loss <= 1e-2 and e_logits <= 1e-2
    # the step's own ReLU pattern, then every gradient on that pattern
    flips = check_pattern(masks, pre, what)
    ref, emu = restate(masks, False), restate(masks, True)
    assert set(ref) == set(grads), (sorted(ref), sorted(grads))
    e = {n: err(n, g.cpu().numpy(), ref) for n, g in grads.items()}
    e_emul = {n: err(n, emu[n], ref) for n in grads}
    fails = grad_bound_failures(e, e_emul)
    near = max(grads, key=lambda n: e[n] / max(1e-2, 2 * e_emul[n]))
    print(f"[{what}] {flips} of {sum(v.numel() for v in pre.values())} ReLU units on the other side of the kink; "
          f"worst gradient error {max(e.values()):.2e} of scale, worst e_emul {max(e_emul.values()):.2e}; closest to "
          f"its bound: {near} measured {e[near]:.2e} e_emul {e_emul[near]:.2e} bound {max(1e-2, 2 * e_emul[near]):.2e}")
    assert not fails, fails


# ----------------------------------------------------------------------------- the Trainer
def synth_data(rows, F, V, seed):
    """-> (ids, labels, how often each id occurs)."""
    from mapx.dataset import synth_table
    ids, labels, _, _ = synth_table(rows, F, V, seed=seed)
    return ids, labels, np.bincount(ids.reshape(-1), minlength=V).astype(np.float32)


def make_trainer(config, model, mode, data, out_dir, batch, epochs, eval_rows, begin=False):
    """The Trainer of the model tests over data = (ids, labels, counts), evaluating on the first eval_rows rows.
    -> (tr, model), or with begin (tr, model, the first epoch's batches) with the run begun for stepping by hand."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset
    from mapx.trainer import Trainer
    ids, labels, _ = data
    targs = TrainingArguments(output_dir=out_dir, per_gpu_train_batch_size=batch, per_gpu_eval_batch_size=batch,
                              learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2, num_train_epochs=epochs,
                              pretrain=mode != "CTR", pt_type="MFP", sampling_method="randint", mask_ratio=0.3,
                              logging_steps=7, seed=11, patience=100)
    targs._device = torch.device("cuda")
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:eval_rows], labels[:eval_rows]))
    if not begin:
        return tr, model
    train = tr._begin("test")
    model.train()
    return tr, model, list(train.batches(batch, True, tr._generator(), (0, 1)))


def captured(tr):
    """The step graphs the trainer holds (an integer in their place counts a step kind's eager warm-up steps)."""
    return [g for g in tr._graphs.values() if not isinstance(g, int)]


def model_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def assert_same_state(a, b):
    """Two state dicts with the same keys and, per key, the same bits."""
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def graph_vs_eager(run):
    """run(use_graph) -> state dict, or (losses, state dict): the captured step must leave what the eager one leaves,
    bit for bit, and give the same losses.  -> (what the graphed run returned, what the eager run returned)."""
    g, e = run(True), run(False)
    if isinstance(g, tuple):
        assert g[0] == e[0], (g[0], e[0])
        assert_same_state(g[1], e[1])
    else:
        assert_same_state(g, e)
    return g, e


def resume_roundtrip(make, steps, split, state_path, kind="mfp", after_load=None):
    """`steps` steps == `split` steps + save_training_state + fresh trainer + load_training_state + the rest, bit for
    bit.  make() -> (tr, batches); after_load(tr) runs on the resumed trainer before it steps.  -> the final state."""
    tr_a, batches = make()
    assert len(batches) == steps
    for X, Y in batches:
        tr_a.run_step(kind, X, Y)
    tr_a.optimizer.flush()
    ref = model_state(tr_a.model)
    tr_b, batches_b = make()
    for X, Y in batches_b[:split]:
        tr_b.run_step(kind, X, Y)
    tr_b.save_training_state(state_path)
    tr_c, batches_c = make()
    tr_c.load_training_state(state_path)
    assert tr_c.global_step == split and tr_c.optimizer.steps_done == split
    if after_load is not None:
        after_load(tr_c)
    for X, Y in batches_c[split:]:
        tr_c.run_step(kind, X, Y)
    tr_c.optimizer.flush()
    for k, v in tr_c.model.state_dict().items():
        assert torch.equal(v.detach().cpu(), ref[k]), k
    return ref


def assert_checkpoint_is_fp32(ck, fp32_model):
    """A checkpoint of a bf16 run: the fp32 model's keys, fp32 master weights only, and it loads into that model."""
    assert set(ck) == set(fp32_model.state_dict())
    assert all(v.dtype != BF and (not v.dtype.is_floating_point or v.dtype == torch.float32) for v in ck.values())
    fp32_model.load_state_dict(ck)


# ----------------------------------------------------------------------------- run.py
def run_py(args, cwd, timeout=600):
    """run.py in a fresh child process -> its CompletedProcess (stdout and stderr as text)."""
    cmd = [sys.executable, os.path.join(ROOT, "map-code_amd", "run.py")] + args
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def finite_metrics(log, keys=("eval_auc", "eval_loss")):
    """Every value a results log reports under each key (there must be one) is finite.  -> key -> values."""
    found = {}
    for key in keys:
        vals = [float(v) for v in re.findall(rf"{key}\W+([-+0-9.eE]+|nan|inf)", log)]
        assert vals and all(math.isfinite(v) for v in vals), (key, vals)
        found[key] = vals
    return found


def pretrain_then_finetune(tmp_path, common, pretrain_args, finetune_args):
    """Writes a synthetic dataset in the reference's layout (4000 rows of which 3200 train, 23 fields), pretrains one
    epoch into out/pretrain and finetunes one epoch from that checkpoint into out/finetune, each in a child process.
    `common` goes to both.
    -> (the pretraining checkpoint's state dict, the finetuning results.log)."""
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=4000, num_fields=23, vocab=2000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3"] + common
    out, fo = str(tmp_path / "out" / "pretrain"), str(tmp_path / "out" / "finetune")
    r = run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=1", "--lr_sched=cosine",
                "--weight_decay=5e-2", "--sampling_method=randint", "--mask_ratio=0.3", "--proj_size=32"]
               + pretrain_args + common, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = os.path.join(out, f"{(3200 + 511) // 512}.model")
    sd = torch.load(ckpt)
    r2 = run_py(["--finetune", f"--pretrained_model_path={ckpt}", f"--output_dir={fo}", "--num_train_epochs=1",
                 "--lr_sched=const", "--weight_decay=1e-1"] + finetune_args + common, str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-3000:]
    return sd, open(os.path.join(fo, "results.log")).read()
