"""Step-loop parity on the GPU: several optimizer steps of mapx (HIP kernels, row-sparse lazy
AdamW) against the oracle running the reference's semantics (dense gradients, dense
transformers-4.26 AdamW over EVERY parameter every step), on identical injected masks and
negatives; run.py end to end; checkpoint layout; 2-rank data parallelism on one GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_harness as H
import paramgen as pg
from util import build_model, load_case, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _targs(**kw):
    from mapx.arguments import TrainingArguments
    base = dict(output_dir="/tmp/mapx_test", learning_rate=1e-3, weight_decay=5e-2, lr_sched="cosine",
                warmup_ratio=0.0, mask_ratio=0.3, sampling_method="randint", pt_type="MFP", pretrain=True)
    base.update(kw)
    return TrainingArguments(**base)


def _step_inputs(case, cfg, step):
    """Per-step reproducible batch: rows permuted, fresh masks / negatives / replacements."""
    inp = pg.make_inputs(case, cfg)
    r = np.random.default_rng(1000 + step)
    B, F, K, V = cfg["B"], cfg["F"], cfg["K"], cfg["V"]
    L = int(F * cfg["mask_ratio"])
    ids = inp["input_ids"][r.permutation(B)]
    lo, hi = pg.field_ranges(F, V)
    ids = np.where(r.random((B, F)) < 0.3, lo[None, :] + r.integers(0, 1 << 30, (B, F)) % (hi - lo)[None, :], ids)
    return dict(ids=ids.astype(np.int64), mi=r.integers(0, F, (B, L)).astype(np.int64),
                noise=r.integers(0, V, (B, L, K)).astype(np.int64),
                repl=ids[r.integers(0, B, (B, L)), r.integers(0, F, (B, L))].astype(np.int64),
                y=(r.random(B) < 0.3).astype(np.int64), feat_count=inp["feat_count"])


def _synth_step_inputs(cfg, step):
    """_step_inputs without a fixture case: ids of a skewed per-field vocabulary (cfg carries B and mask_ratio), fresh
    masks / negatives / labels per step."""
    r = np.random.default_rng(7000 + step)
    B, F, K, V = cfg["B"], cfg["F"], cfg["K"], cfg["V"]
    L = int(F * cfg["mask_ratio"])
    lo, hi = pg.field_ranges(F, V)
    ids = lo[None, :] + np.floor(r.random((B, F)) ** 3 * (hi - lo)[None, :]).astype(np.int64)
    cnt = (1.0 + np.random.default_rng(7).integers(0, 50, V)).astype(np.float32)
    return dict(ids=ids.astype(np.int64), mi=r.integers(0, F, (B, L)).astype(np.int64),
                noise=r.integers(0, V, (B, L, K)).astype(np.int64),
                repl=ids[r.integers(0, B, (B, L)), r.integers(0, F, (B, L))].astype(np.int64),
                y=(r.random(B) < 0.3).astype(np.int64), feat_count=cnt)


def _oracle_loop(mode, cfg, params, steps, case, total, warmup, kind, lr0, wd, backbone="DCNv2", step_inputs=None,
                 relu_masks=None):
    """`params`: the arrays of a fixture case, or a model's state_dict() (its trainable tensors are taken: the sampler's
    and the noise distribution's buffers are not parameters).  `step_inputs(s)`: the batch of step s, default the
    fixture case's (_step_inputs).  `relu_masks[s]` (DCNv2, MFP / CTR): the ReLU pattern of the step under test at step
    s, imposed on the oracle after checking that the two patterns differ only at units whose pre-activation is zero to
    fp32 rounding (util.check_pattern, 2e-6 of the layer's scale): one such unit on the other side of the kink changes
    a whole row of the first layer's weight gradient, and AdamW turns any change of a gradient into a step of ~lr."""
    from oracle import ref_model as R
    from util import check_pattern
    inputs_of = step_inputs or (lambda s: _step_inputs(case, cfg, s))
    params = {k: (v.detach().cpu() if torch.is_tensor(v) else t(v)) for k, v in params.items()}
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()
         if v.dtype.is_floating_point and "alias" not in k and "logprob" not in k}
    m = {k: torch.zeros_like(p) for k, p in P.items()}
    v = {k: torch.zeros_like(p) for k, p in P.items()}
    losses = []
    for s in range(steps):
        si = inputs_of(s)
        ids = t(si["ids"])
        pre = {}
        trunk = lambda x: R.trunk(P, x, cfg["NC"], cfg["NL"], relu_masks=relu_masks[s], preacts=pre)
        if mode == "MFP":
            logq, _, _ = R.nce_buffers(si["feat_count"])
            masked, labels = R.dynamic_mask_mfp(ids, t(si["mi"]))
            fin = trunk(masked) if relu_masks is not None else \
                R.final_of(backbone, P, masked, cfg["NC"], cfg["NL"], pg.extras_of(backbone))
            loss, _, _ = R.mfp_head(P, fin, labels, t(si["mi"]), t(si["noise"]), logq, cfg["F"], cfg["P"], cfg["K"])
        elif mode == "RFD":
            rep, labels = R.dynamic_mask_rfd(ids, t(si["mi"]), t(si["repl"]))
            loss = R.rfd_head(P, R.final_of(backbone, P, rep, cfg["NC"], cfg["NL"], pg.extras_of(backbone)), labels)[0]
        else:
            logits = R.ctr_head(P, trunk(ids))[0] if relu_masks is not None else \
                R.ctr_logits_of(backbone, P, ids, cfg["NC"], cfg["NL"], pg.extras_of(backbone))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), t(si["y"]).float())
        if relu_masks is not None:
            assert backbone == "DCNv2" and mode != "RFD"
            check_pattern(relu_masks[s], pre, f"{mode} step {s}", tol=2e-6)
        loss.backward()
        losses.append(float(loss.detach()))
        lr = lr0 * R.lr_lambda(kind, s, total, warmup)
        with torch.no_grad():
            for k, p in P.items():      # the reference: dense grads, every parameter, every step
                R.hf_adamw_step(p, p.grad, m[k], v[k], s + 1, lr, wd=wd if R.decays(k) else 0.0)
                p.grad = None
    return losses, {k: p.detach() for k, p in P.items()}


@pytest.mark.parametrize("mode,kind,warm,backbone",
                         [("MFP", "cosine", 0.2, "DCNv2"), ("RFD", "cosine", 0.0, "DCNv2"), ("CTR", "const", 0.0, "DCNv2"),
                          ("MFP", "cosine", 0.0, "DNN"), ("CTR", "const", 0.0, "DNN"),
                          ("MFP", "cosine", 0.2, "DeepFM"), ("RFD", "cosine", 0.0, "DeepFM"),
                          ("CTR", "const", 0.0, "DeepFM"),
                          ("MFP", "cosine", 0.0, "AutoInt"), ("CTR", "const", 0.0, "AutoInt"),
                          ("MFP", "cosine", 0.2, "xDeepFM"), ("RFD", "cosine", 0.0, "xDeepFM"),
                          ("CTR", "const", 0.0, "xDeepFM")])
def test_training_trajectory_matches_reference_semantics(mode, kind, warm, backbone):
    from mapx import ops
    from mapx.optim import MapxOptimizer
    case = "B_f25_b64"
    cfg = pg.CASES[case]
    _, _, inp, params = load_case(case, mode, backbone)
    steps, total = 8, 10
    warmup = int(total * warm)
    lr0, wd = 1e-3, 5e-2
    ref_losses, ref_params = _oracle_loop(mode, cfg, params, steps, case, total, warmup, kind, lr0, wd, backbone)

    model = build_model(cfg, mode, params, inp["feat_count"] if mode == "MFP" else None, backbone=backbone)
    targs = _targs(lr_sched=kind, learning_rate=lr0, weight_decay=wd)
    opt = MapxOptimizer(model, targs, num_training_steps=total, num_warmup_steps=warmup, max_gap=3)
    model.train()
    L = int(cfg["F"] * cfg["mask_ratio"])
    losses = []
    for s in range(steps):
        si = _step_inputs(case, cfg, s)
        ids = t(si["ids"], DEV)
        if mode == "MFP":
            masked, labels, mi = ops.dynamic_mask_mfp(ids, L, masked_index=t(si["mi"], DEV))
            loss = model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=t(si["noise"], DEV))[0]
        elif mode == "RFD":
            rep, labels, _ = ops.dynamic_mask_rfd(ids, L, masked_index=t(si["mi"], DEV), replace_feat=t(si["repl"], DEV))
            loss = model(input_ids=rep, labels=labels)[0]
        else:
            loss = model(input_ids=ids, labels=t(si["y"], DEV))[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        assert opt.get_last_lr()[0] == pytest.approx(lr0 * __import__("mapx.optim", fromlist=["x"]).lr_lambda(kind, s + 1, total, warmup))
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-5)
    opt.flush()                       # lazy rows -> reference-equivalent weights
    if mode == "CTR":
        # BASELINE config 5: AUC on held-out rows after the same training within 1e-4 of the
        # reference path (here: identical to ~1e-6 because the parameters agree to 1e-4)
        from sklearn.metrics import roc_auc_score
        from oracle import ref_model as R
        held = _step_inputs(case, cfg, 999)
        model.eval()
        with torch.no_grad():
            (logits,) = model(input_ids=t(held["ids"], DEV))
            ref_logits = R.ctr_logits_of(backbone, ref_params, t(held["ids"]), cfg["NC"], cfg["NL"], pg.extras_of(backbone))
        y = held["y"]
        auc = roc_auc_score(y, torch.sigmoid(logits.view(-1)).cpu().numpy())
        auc_ref = roc_auc_score(y, torch.sigmoid(ref_logits.view(-1)).numpy())
        assert abs(auc - auc_ref) < 1e-4, (auc, auc_ref)
        np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.numpy(), rtol=1e-4, atol=1e-5)
        model.train()
    sd = model.state_dict()
    for k, ref in ref_params.items():
        got = sd[k].cpu()
        # 8 AdamW steps move parameters by ~8e-3; fp32 parity of the whole trajectory
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("E", [12, 64])
@pytest.mark.parametrize("mode,kind", [("MFP", "cosine"), ("CTR", "const")])
def test_training_trajectory_at_other_embed_sizes(mode, kind, E):
    """Eight optimizer steps of DCNv2 at embed_size 12 (rows on four lanes, one idle) and 64 (sixteen lanes) with the
    assertions of test_training_trajectory_matches_reference_semantics: batches of 64 over 3000 ids leave most rows
    without a gradient for several steps, so the replay of the lazy AdamW runs at these widths (max_gap = 3).

    The oracle runs on each step's own ReLU pattern (_oracle_loop): at E = 12 in CTR mode unit 18 of the first deep layer
    sits on the kink for one batch row of the second step; compared on the oracle's own pattern that one unit's row
    of the weight gradient differs, AdamW makes ~lr of it, and after eight steps 178 of 36 000 embedding elements were
    off by up to 2.9e-3 with every kernel right (each gradient within 2e-7 of float64 from the step's own
    parameters)."""
    from mapx import ops
    from mapx.models import BaseModel
    from mapx.optim import MapxOptimizer
    from util import make_config
    cfg = dict(F=23, V=3000, E=E, H=64, NL=3, NC=3, P=32, K=25, B=64, mask_ratio=0.3)
    steps, total, warmup, lr0, wd = 8, 10, 0, 1e-3, 5e-2
    inputs = lambda s: _synth_step_inputs(cfg, s)
    torch.manual_seed(E)
    model = BaseModel.from_config(make_config(cfg, mode, inputs(0)["feat_count"] if mode == "MFP" else None)).to(DEV)
    start = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    from util import hook_relu_pattern
    masks, patterns = hook_relu_pattern(model), []
    opt = MapxOptimizer(model, _targs(lr_sched=kind, learning_rate=lr0, weight_decay=wd), num_training_steps=total,
                        num_warmup_steps=warmup, max_gap=3)
    model.train()
    L = int(cfg["F"] * cfg["mask_ratio"])
    losses = []
    for s in range(steps):
        si = inputs(s)
        ids = t(si["ids"], DEV)
        if mode == "MFP":
            masked, labels, mi = ops.dynamic_mask_mfp(ids, L, masked_index=t(si["mi"], DEV))
            loss = model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=t(si["noise"], DEV))[0]
        else:
            loss = model(input_ids=ids, labels=t(si["y"], DEV))[0]
        patterns.append(dict(masks))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    ref_losses, ref_params = _oracle_loop(mode, cfg, start, steps, None, total, warmup, kind, lr0, wd,
                                          step_inputs=inputs, relu_masks=patterns)
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-5)
    opt.flush()
    sd = model.state_dict()
    assert set(ref_params) == {n for n, _ in model.named_parameters()}
    off = {}
    for k, ref in ref_params.items():                 # every tensor, so that a failure names all that moved wrongly
        bad = ~torch.isclose(sd[k].cpu(), ref, rtol=1e-4, atol=2e-6)
        if bool(bad.any()):
            off[k] = (int(bad.sum()), ref.numel(), float((sd[k].cpu() - ref).abs().max()))
    assert not off, f"(elements off, of, max |difference|) per tensor: {off}"


def test_untouched_rows_still_decay_like_the_reference():
    """A row that never receives a gradient must end where dense AdamW puts it: p * prod(1 - lr_s*wd)."""
    from mapx.optim import MapxOptimizer, lr_lambda
    case = "A_f23_b7"
    cfg = pg.CASES[case]
    _, _, inp, params = load_case(case, "CTR")
    model = build_model(cfg, "CTR", params, None)
    opt = MapxOptimizer(model, _targs(lr_sched="cosine"), num_training_steps=6, num_warmup_steps=0, max_gap=1000)
    ids = t(inp["input_ids"], DEV)
    untouched = sorted(set(range(100, cfg["V"])) - set(inp["input_ids"].reshape(-1).tolist()))[:50]   # beyond the 5 swept rows
    w0 = model.embed.embedding.weight.detach().cpu()[untouched].double()
    model.train()
    for _ in range(5):
        model(input_ids=ids, labels=t(inp["y"], DEV))[0].backward()
        opt.step()
    stale = model.embed.embedding.weight.detach().cpu()[untouched].double()
    assert torch.equal(stale, w0)                       # lazy: not yet applied ...
    opt.flush()
    w = model.embed.embedding.weight.detach().cpu()[untouched].double()
    factor = np.prod([1 - 1e-3 * lr_lambda("cosine", s, 6, 0) * 5e-2 for s in range(5)])
    np.testing.assert_allclose(w.numpy(), (w0 * factor).numpy(), rtol=1e-6)   # ... until flushed


def test_dynamic_mask_normal_mode_has_distinct_fields():
    from mapx.dataset import OurDataset
    from mapx.trainer import Trainer
    case = "A_f23_b7"
    cfg = pg.CASES[case]
    _, _, inp, params = load_case(case, "MFP")
    model = build_model(cfg, "MFP", params, inp["feat_count"])
    targs = _targs()
    targs._device = torch.device(DEV)
    ds = OurDataset(inp["input_ids"], inp["y"])
    tr = Trainer(model, model.config, targs, ds, ds)
    out = tr.dynamic_mask({"input_ids": t(inp["input_ids"], DEV), "labels": None}, "normal")
    mi = out["masked_index"].cpu()
    assert all(len(set(r.tolist())) == mi.shape[1] for r in mi)
    with pytest.raises(NotImplementedError):
        tr.dynamic_mask({"input_ids": t(inp["input_ids"], DEV)}, "bogus")


def test_run_py_pretrain_then_finetune(tmp_path):
    """The four run scripts' flow on a small synthetic dataset in the reference's on-disk layout."""
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=6000, num_fields=23, vocab=3000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3", "--model_name=DCNv2", "--embed_size=16",
              "--hidden_size=64", "--num_hidden_layers=3", "--num_cross_layers=3", "--hidden_dropout_rate=0.0",
              "--logging_steps=5"]
    for pt in ("MFP", "RFD"):
        out = str(tmp_path / "out" / pt)
        r = H.run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=2", "--lr_sched=cosine",
                     "--weight_decay=5e-2", f"--pt_type={pt}", "--sampling_method=randint", "--mask_ratio=0.3",
                     "--pt_neg_num=25", "--proj_size=32"] + common, str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        steps = 2 * ((4800 + 511) // 512)
        ckpt = os.path.join(out, f"{steps}.model")
        assert os.path.exists(ckpt) and os.path.exists(os.path.join(out, "results.log"))
        sd = torch.load(ckpt)
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json")))[f"A_f23_b7_{pt}"]
        assert set(sd) == set(gold) and all(v.dtype in (torch.float32, torch.int64) for v in sd.values())
        log = open(os.path.join(out, "train.log")).read()
        assert "window_" in log and "eval_" in log
    r2 = H.run_py(["--pretrain=True", f"--output_dir={tmp_path / 'out' / 'MFP'}", "--pt_type=MFP"] + common, str(tmp_path))
    assert r2.returncode == 0 and "job already finished" in r2.stdout
    fo = str(tmp_path / "out" / "finetune")
    r3 = H.run_py(["--finetune", f"--pretrained_model_path={tmp_path / 'out' / 'MFP' / f'{steps}.model'}",
                  f"--output_dir={fo}", "--num_train_epochs=1", "--lr_sched=const", "--weight_decay=1e-1"] + common,
                 str(tmp_path))
    assert r3.returncode == 0, r3.stderr[-3000:]
    log = open(os.path.join(fo, "results.log")).read()
    assert "Load tensor: embed.embedding.weight" in log and "Unmatched tensor in the target model: feat_encoder.weight" in log
    assert "eval_auc" in log and "running TEST" in log
    assert any(f.endswith(".model") for f in os.listdir(fo))


def test_data_parallel_two_ranks_equal_single_process(tmp_path):
    """2 ranks (gloo rendezvous, both on this GPU), each with half of the batch, must produce the
    same parameters as one process with the whole batch."""
    worker = os.path.join(ROOT, "tests", "dp_worker.py")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "map-code_amd"),
                                                        os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]))
    one = subprocess.run([sys.executable, worker, str(tmp_path / "single.pt")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29533", worker, str(tmp_path / "dp.pt")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert two.returncode == 0, two.stderr[-3000:]
    a, b0, b1 = (torch.load(str(tmp_path / n)) for n in ("single.pt", "dp.pt.0", "dp.pt.1"))
    for k in a:
        assert torch.equal(b0[k], b1[k]), f"replicas diverged on {k}"
        np.testing.assert_allclose(b0[k].numpy(), a[k].numpy(), rtol=2e-4, atol=2e-6, err_msg=k)


def test_one_rank_rccl_exchange_equals_plain_step(tmp_path):
    """The N-rank gradient exchange rehearsed on one GPU (one-rank RCCL group, MAPX_FORCE_DP=1):
    dense all-reduce, early segment counts published by the graph, MAX over ranks, pack,
    all-gathers, merge.  With one rank the exchange is the identity, so parameters must equal the
    plain single-GPU run bit for bit — through the captured graphs (GraphedBackward +
    GraphedExchangeTail) and eagerly."""
    worker = os.path.join(ROOT, "tests", "dp_rehearsal_worker.py")
    base = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "map-code_amd"),
                                                         os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]))
    outs = {}
    for name, forced, mode in (("plain", "0", "eager"), ("dp_eager", "1", "eager"), ("dp_graph", "1", "graph")):
        path = str(tmp_path / f"{name}.pt")
        r = subprocess.run([sys.executable, worker, path, mode], env=dict(base, MAPX_FORCE_DP=forced),
                           capture_output=True, text=True, timeout=600)
        errors = [ln for ln in r.stderr.splitlines() if "rror" in ln or "fault" in ln][:20]
        assert r.returncode == 0, (name, errors, r.stderr[-2000:])
        outs[name] = torch.load(path)
    for k in outs["plain"]:
        assert torch.equal(outs["plain"][k], outs["dp_eager"][k]), ("eager exchange", k)
        assert torch.equal(outs["plain"][k], outs["dp_graph"][k]), ("graphed exchange", k)


def test_two_ranks_graphed_exchange_equals_eager(tmp_path):
    """the GRAPHED data-parallel step at world size 2 — GraphedBackward (mask + forward + backward
    replayed, segment counts published to the host mid-graph, MAX over ranks) and GraphedExchangeTail (pack graph,
    all-gathers, merge + optimizer graph) — with two gloo ranks on this one GPU, each on its own rows, masks and
    negatives: replicas bit-identical, and bit-identical to the same two ranks stepping eagerly (which
    test_data_parallel_two_ranks_equal_single_process ties to the single-process step)."""
    worker = os.path.join(ROOT, "tests", "dp_graph_worker.py")
    env = dict(os.environ, MAPX_DP_GLOO_GRAPH="1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "map-code_amd"), os.path.join(ROOT, "tests"),
                                           os.path.join(ROOT, "tests", "golden")]))
    outs = {}
    for mode, port in (("eager", "29547"), ("graph", "29549")):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port, worker, str(tmp_path / f"{mode}.pt"),
                            mode], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (mode, r.stderr[-3000:])
        outs[mode] = [torch.load(str(tmp_path / f"{mode}.pt.{k}")) for k in (0, 1)]
    for k in outs["eager"][0]:
        assert torch.equal(outs["graph"][0][k], outs["graph"][1][k]), f"graphed replicas diverged on {k}"
        assert torch.equal(outs["eager"][0][k], outs["eager"][1][k]), f"eager replicas diverged on {k}"
        assert torch.equal(outs["graph"][0][k], outs["eager"][0][k]), f"graphed exchange != eager exchange on {k}"


@pytest.mark.parametrize("max_grad_norm,backbone,full,epochs,E",
                         [pytest.param(0.0, "DCNv2", 9, 2, 16, id="0.0-DCNv2-9-2"),
                          pytest.param(0.5, "DCNv2", 9, 2, 16, id="0.5-DCNv2-9-2"),
                          pytest.param(0.0, "DeepFM", 9, 2, 16, id="0.0-DeepFM-9-2"),
                          # GRAPH_AFTER full batches per epoch: the step is captured right after the
                          # epoch-end flush (no stale row at trace time) — the lazy catch-up must be
                          # in the graph all the same
                          pytest.param(0.0, "DCNv2", 3, 4, 16, id="0.0-DCNv2-3-4"),
                          pytest.param(0.5, "DCNv2", 3, 4, 16, id="0.5-DCNv2-3-4"),
                          # the row kernels' other lane-group forms (tests/row_widths_ref.py)
                          pytest.param(0.0, "DCNv2", 9, 2, 12, id="0.0-DCNv2-9-2-E12"),
                          pytest.param(0.0, "DCNv2", 9, 2, 64, id="0.0-DCNv2-9-2-E64")])
def test_graph_replay_equals_eager_bitwise(max_grad_norm, backbone, full, epochs, E):
    """The captured-hipGraph step and the eager step draw the same Philox streams (device-side
    counter) and run the same kernels: identical parameters after two epochs, bit for bit.
    With gradient clipping (as with N > 1) only mask + forward + backward are captured and the
    rest of the step runs eagerly after each replay (trainer.GraphedBackward)."""
    _graph_equals_eager(max_grad_norm, backbone, full, epochs, E=E)


@pytest.mark.gpu
def test_graph_replay_equals_eager_bitwise_with_streaming_hidden_layers(monkeypatch):
    """The same with the 64-wide hidden layers' weight gradients on the streaming kernels (MAPX_SKINNY_MAX_BWD=64:
    skinny_dw_tall_kernel on the deep tower's stream beside the cross tower's GEMMs).  Round 3: with the compiler's
    packed FMAs in that kernel about half of these runs differed from the eager loop in a few elements of one
    weight gradient."""
    from mapx import ops
    monkeypatch.setattr(ops, "SKINNY_MAX_BWD", 64)
    monkeypatch.setattr(ops, "SKINNY_TALL", True)
    # one run (not a loop: a result that comes and goes with timing is not chased by repetition — the instruction form
    # behind it is kept out of every shipped kernel by tests/test_isa_guard.py instead)
    _graph_equals_eager(0.0, "DCNv2", 18, 1, tail=0)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph,E", [pytest.param(True, 16, id="True"), pytest.param(False, 16, id="False"),
                                         (True, 12), (False, 12), (True, 64), (False, 64)])
def test_rows_read_through_pending_updates_train_like_the_catch_up_pass(use_graph, E):
    """nce.LAZY_FOLD and layers.EMB_LAZY_FOLD (opt-in, MAPX_LAZY_FOLD=1 / MAPX_EMB_LAZY_FOLD=1): a training step without
    the tables' catch-up passes — the loss kernel and the embedding gather replay stale rows in registers, the gradient
    updates write them once — leaves, after two epochs with a ragged last batch, the parameters of the step with the
    catch-up passes, bit for bit (graphed and eager)."""
    _graph_equals_eager(0.0, "DCNv2", 9, 2, arms=((use_graph, True), (use_graph, False)), E=E)


def _graph_equals_eager(max_grad_norm, backbone, full, epochs, tail=100, arms=((True, None), (False, None)), E=16):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=E, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * full + tail, 23, cfg["V"], seed=3)    # ragged last batch
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    out = []
    from mapx import layers as _layers, nce
    fold_default, emb_default = nce.LAZY_FOLD, _layers.EMB_LAZY_FOLD
    for use_graph, fold in arms:
        nce.LAZY_FOLD = fold_default if fold is None else fold
        _layers.EMB_LAZY_FOLD = emb_default if fold is None else fold
        torch.manual_seed(5)
        config = make_config(cfg, "MFP", cnt, backbone=backbone)
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir="/tmp/mapx_graph_test", per_gpu_train_batch_size=512,
                                  per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine",
                                  weight_decay=5e-2, num_train_epochs=epochs, pretrain=True, pt_type="MFP",
                                  sampling_method="randint", mask_ratio=0.3, logging_steps=7, seed=11,
                                  max_grad_norm=max_grad_norm)
        targs._device = torch.device(DEV)
        os.makedirs(targs.output_dir, exist_ok=True)
        ds = OurDataset(ids, labels)
        tr = Trainer(model, config, targs, ds, OurDataset(ids[:600], labels[:600]))
        tr.use_graph = use_graph
        tr.MFP_pretrain()
        assert tr.global_step == epochs * (full + (1 if tail else 0))
        assert (len(tr._graphs) == 1 and len(H.captured(tr)) == 1) == use_graph
        if use_graph:
            kind = type(H.captured(tr)[0]).__name__
            assert kind == ("GraphedBackward" if max_grad_norm > 0 else "GraphedStep")
        out.append(H.model_state(model))
    nce.LAZY_FOLD, _layers.EMB_LAZY_FOLD = fold_default, emb_default
    H.assert_same_state(out[0], out[1])


@pytest.mark.gpu
@pytest.mark.parametrize("pt,max_grad_norm", [("RFD", 0.0), ("CTR", 0.0), ("RFD", 0.5), ("CTR", 0.5)])
def test_rfd_and_finetune_steps_walk_row_references_like_the_eager_loop(pt, max_grad_norm):
    """RFD pretraining and finetune epochs deal their batches as row references too (round 3): the captured step cuts
    its rows from the resident split itself (mapx_take_rows_i64 behind the device cursor).  Same parameters as the
    eager loop after two epochs with a ragged tail, bit for bit; the graph is the walking kind.  With gradient
    clipping (as with N > 1) forward + backward replay from a graph that takes the batch's row numbers."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import GraphedStep, Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * 9 + 100, 23, cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)

    def run(use_graph):
        torch.manual_seed(5)
        config = make_config(cfg, pt, cnt)
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir="/tmp/mapx_rows_test", per_gpu_train_batch_size=512,
                                  per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine",
                                  weight_decay=5e-2, num_train_epochs=2, pretrain=pt != "CTR",
                                  pt_type="MFP" if pt == "CTR" else pt, RFD_replace="Unigram",
                                  sampling_method="randint", mask_ratio=0.3, logging_steps=7, seed=11,
                                  patience=100, max_grad_norm=max_grad_norm)
        targs._device = torch.device(DEV)
        os.makedirs(targs.output_dir, exist_ok=True)
        tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:600], labels[:600]))
        tr.use_graph = use_graph
        tr.RFD_pretrain() if pt == "RFD" else tr.train()
        assert tr.global_step == 2 * 10
        graphs = H.captured(tr)
        assert bool(graphs) == use_graph
        if use_graph and max_grad_norm > 0:
            assert type(graphs[0]).__name__ == "GraphedBackward"
        elif use_graph:
            assert isinstance(graphs[0], GraphedStep) and graphs[0].walk
        return H.model_state(model)

    H.graph_vs_eager(run)


def test_resume_state_continues_bit_exactly(tmp_path):
    """save_training_state / load_training_state: 6 steps == 3 steps + save + fresh trainer + load + 3 steps."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * 6, 23, cfg["V"], seed=4)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)

    def make():
        torch.manual_seed(9)
        config = make_config(cfg, "MFP", cnt)
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir=str(tmp_path), per_gpu_train_batch_size=512,
                                  per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine",
                                  weight_decay=5e-2, num_train_epochs=1, pretrain=True, pt_type="MFP",
                                  sampling_method="randint", mask_ratio=0.3, seed=3)
        targs._device = torch.device(DEV)
        ds = OurDataset(ids, labels)
        tr = Trainer(model, config, targs, ds, ds)
        tr.use_graph = False
        train = tr._begin("test")
        model.train()
        return tr, list(train.batches(512, True, tr._generator(), (0, 1)))

    H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"))


def test_run_py_deepfm_pretrain_then_finetune(tmp_path):
    """run.py --model_name=DeepFM: MFP pretraining, then finetune from that checkpoint (LR / FM /
    MLP weights are loaded by name, the pretraining head is reported as unmatched)."""
    common = ["--model_name=DeepFM", "--embed_size=16", "--hidden_size=64", "--num_hidden_layers=2",
              "--hidden_dropout_rate=0.0", "--logging_steps=3"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"], [])
    assert {"lr_layer.embed_w.weight", "lr_layer.bias", "ip_layer.field_p", "dnn.dnn.0.weight",
            "feat_encoder.weight", "mfp_criterion.emb.weight"} <= set(sd)
    assert "Load tensor: lr_layer.embed_w.weight" in log and "Unmatched tensor in the target model: feat_encoder.weight" in log
    assert "eval_auc" in log


def test_run_py_xdeepfm_pretrain_then_finetune(tmp_path):
    """run.py --model_name=xDeepFM: RFD pretraining (graph replay of the CIN step), then finetune with
    use_lr from that checkpoint (CIN / MLP weights loaded by name, the LR term starts fresh)."""
    common = ["--model_name=xDeepFM", "--embed_size=16", "--hidden_size=64", "--num_hidden_layers=2",
              "--hidden_dropout_rate=0.0", "--logging_steps=3", "--cin_layer_units=16,8"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=RFD", "--RFD_replace=Unigram"], ["--use_lr=True"])
    assert {"cin.cin_layer.layer_1.weight", "cin.cin_layer.layer_2.bias", "dnn.dnn.0.weight",
            "pred_rfd.0.weight"} <= set(sd)
    assert tuple(sd["cin.cin_layer.layer_1.weight"].shape) == (16, 23 * 23, 1)
    assert tuple(sd["cin.cin_layer.layer_2.weight"].shape) == (8, 23 * 16, 1)
    assert "Load tensor: cin.cin_layer.layer_2.weight" in log and "Unmatched tensor in the target model: pred_rfd.0.weight" in log
    assert "eval_auc" in log


@pytest.mark.parametrize("F,V,pt,dtype", [(23, 9_449_445, "MFP", "fp32"), (39, 33_762_577, "MFP", "fp32"),
                                          (23, 9_449_445, "RFD", "fp32"), (39, 33_762_577, "MFP", "bf16")])
def test_full_vocabulary_step_properties(F, V, pt, dtype):
    """BASELINE configs[1] / [2] / [3] at their real sizes (Avazu: F = 23, V = 9 449 445; Criteo: F = 39,
    V = 33 762 577, in fp32 and — configs[2] as BASELINE words it — in bf16 compute mode; B = 4096, H = 1000,
    K = 25; config [3] = RFD with Unigram replacement)
    through size-independent properties, since the oracle's dense step is too slow to iterate here:
    (1) the captured-graph step and the eager step leave bit-identical parameters;
    (2) linearity: the embedding table's sparse gradient rows sum to the column sums of dL/dX0, and
        every sampled NCE row is listed exactly once;
    (3) rows that no step touched hold, after flush(), what transformers-4.26 AdamW gives a
        parameter with zero gradient (oracle hf_adamw_step iterated) — the lazy replay at scale."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from oracle import ref_model as R
    from util import make_config
    cfg = dict(F=F, V=V, E=16, H=1000, NL=3, NC=3, P=32, K=25)
    B, steps = 4096, 7
    ids, labels, _, _ = synth_table(B * steps, F, cfg["V"], seed=5)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    probe = torch.from_numpy(np.random.default_rng(0).choice(cfg["V"], 4000, replace=False)).to(DEV)
    finals, first = [], {}
    for use_graph in (True, False):
        torch.manual_seed(5)
        config = make_config(cfg, pt, cnt if pt == "MFP" else None, compute_dtype=dtype)
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir="/tmp/mapx_full_vocab", per_gpu_train_batch_size=B,
                                  per_gpu_eval_batch_size=B, learning_rate=1e-3, lr_sched="cosine",
                                  weight_decay=5e-2, num_train_epochs=1, pretrain=True, pt_type=pt,
                                  RFD_replace="Unigram",
                                  sampling_method="randint", mask_ratio=0.3, logging_steps=100, seed=11)
        targs._device = torch.device(DEV)
        os.makedirs(targs.output_dir, exist_ok=True)
        tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:B], labels[:B]))
        tr.use_graph = use_graph
        train = tr._begin("full-vocabulary test")
        model.train()
        if not first:
            first = {n: p.detach()[probe].clone() for n, p in model.named_parameters()
                     if n in ("embed.embedding.weight", "mfp_criterion.emb.weight", "mfp_criterion.bias.weight")}
        touched = torch.zeros(cfg["V"], dtype=torch.bool, device=DEV)
        for k, (X, Y) in enumerate(train.batches(B, True, tr._generator(), (0, 1))):
            if not use_graph and k == 0:           # (2) on one eager step, before the optimizer consumes the gradients
                inputs = tr.dynamic_mask({"input_ids": X, "labels": Y}, "randint")
                x3 = model.embed(inputs["input_ids"])
                x3.retain_grad()
                flat = x3.flatten(1)
                final = torch.cat([model.cross_net(flat), model.parallel_dnn(flat)], -1)
                if pt == "MFP" and dtype == "bf16":        # bf16 mode: the dense encoder GEMM, fp32 head
                    loss, _, idx = model.mfp_criterion(inputs["labels"], model.feat_encoder(final),
                                                       masked_index=inputs["masked_index"])
                elif pt == "MFP":
                    loss, _, idx = model.mfp_criterion.forward_with_encoder(inputs["labels"], final,
                                                                           model.feat_encoder, inputs["masked_index"])
                else:
                    # replaced ids stay inside the vocabulary and differ from the originals where labelled
                    assert int(inputs["input_ids"].min()) >= 0 and int(inputs["input_ids"].max()) < V
                    assert torch.equal(inputs["labels"] > 0, inputs["input_ids"] != X)
                    loss = model.get_outputs(final, inputs["labels"])[0]
                loss.backward()
                plan, rows, _ = model.embed.table.sparse_grad
                U = plan.count()
                np.testing.assert_allclose(rows[:U].double().sum(0).cpu().numpy(),
                                           x3.grad.double().sum((0, 1)).cpu().numpy(), rtol=1e-4,
                                           atol=1e-7 if dtype == "fp32" else 1e-5)
                assert torch.equal(plan.uniq[:U].long(), torch.unique(inputs["input_ids"]))
                if pt == "MFP":
                    nplan = model.mfp_criterion.table.sparse_grad[0]
                    assert torch.equal(nplan.uniq[:nplan.count()].long(), torch.unique(idx.long()))
                for t in tr.optimizer.tables:
                    t.table.sparse_grad = None
                # this backward pass had no optimizer.step(): sum what it queued NOW — left in the list, its partial
                # sums would share one launch with the real step's and race them for the same gradient slots
                from mapx import ops
                ops.join_pending()
                ops.run_late_tasks()
                ops.flush_deferred()
            tr.run_step(pt.lower(), X, Y)
        assert tr.global_step == steps
        tr.optimizer.flush()
        finals.append({n: p.detach().clone() for n, p in model.named_parameters()})
        del tr, model
        torch.cuda.empty_cache()
    H.assert_same_state(finals[0], finals[1])                             # (1)
    # (3) rows whose value equals "zero-gradient AdamW from the initial value" must be exactly the
    # untouched ones; check the prediction on the probe rows that stayed untouched in every table
    lambdas = [R.lr_lambda("cosine", s, steps, 0) for s in range(steps)]
    for n, p0 in first.items():
        p = p0.double().cpu()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for s in range(steps):
            R.hf_adamw_step(p, torch.zeros_like(p), m, v, s + 1, 1e-3 * lambdas[s], wd=5e-2 if R.decays(n) else 0.0)
        got = finals[0][n][probe].double().cpu()
        same = ((got - p).abs() <= 1e-6 * p.abs() + 1e-9).all(dim=1)
        assert int(same.sum()) >= int(0.9 * probe.numel()), (n, int(same.sum()))     # Zipf tails: most rows untouched
        moved = ((got - p0.double().cpu()).abs() > 0).any(dim=1)
        if R.decays(n):
            assert bool(moved[same].all()), n          # decayed rows did move, by exactly the predicted amount


def test_pretrain_then_finetune_auc_on_12k_heldout_rows_batch_256_vs_oracle():
    """BASELINE configs[4]: "DCNv2 finetune after MFP — AUC parity vs reference within 1e-4"
    (reference flow: run.py:64-67 load_for_finetune, trainer.py:87-161 train, :163-215 eval).
    30 MFP steps -> name+shape transfer into the CTR model -> 40 finetune steps, on the GPU (HIP
    kernels, lazy row-sparse AdamW) and on the oracle (dense grads, dense HF AdamW on every
    parameter every step) from identical injected masks / negatives / batches; then AUC and
    log-loss on 12 000 held-out rows (AUC granularity 1e-8 there, not the 1.2e-3 of a 64-row set)."""
    from sklearn.metrics import log_loss, roc_auc_score
    from mapx import ops
    from mapx.dataset import synth_table
    from mapx.models import BaseModel
    from mapx.optim import MapxOptimizer, lr_lambda
    from oracle import ref_model as R
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    F, V, K, B = cfg["F"], cfg["V"], cfg["K"], 256
    n_pre, n_ft, n_held = 30, 40, 12000
    L = int(F * 0.3)
    ids_all, _, _, _ = synth_table((n_pre + n_ft) * B + n_held, F, V, seed=5)
    rng = np.random.default_rng(77)
    a = rng.normal(0.0, 0.6, V)
    logit = a[ids_all].sum(1)
    y_all = (rng.random(len(logit)) < 1.0 / (1.0 + np.exp(-(logit - np.median(logit) - 1.0)))).astype(np.int64)
    cnt = np.bincount(ids_all[:n_pre * B].reshape(-1), minlength=V).astype(np.float32)
    rows = lambda s: slice(s * B, (s + 1) * B)
    mis = rng.integers(0, F, (n_pre, B, L)).astype(np.int64)
    noises = rng.integers(0, V, (n_pre, B, L, K)).astype(np.int64)
    held_ids, held_y = ids_all[-n_held:], y_all[-n_held:]

    # ---- GPU: pretrain
    torch.manual_seed(0)
    pre = BaseModel.from_config(make_config(cfg, "MFP", cnt)).to(DEV)
    P0 = {k: v.detach().cpu().clone() for k, v in pre.state_dict().items()}
    opt = MapxOptimizer(pre, _targs(lr_sched="cosine", weight_decay=5e-2), num_training_steps=n_pre, num_warmup_steps=0)
    pre.train()
    for s in range(n_pre):
        masked, labels, mi = ops.dynamic_mask_mfp(t(ids_all[rows(s)], DEV), L, masked_index=t(mis[s], DEV))
        loss = pre(input_ids=masked, labels=labels, masked_index=mi, noise_samples=t(noises[s], DEV))[0]
        loss.backward()
        opt.step()
    opt.flush()
    pre_sd = {k: v.detach().cpu().clone() for k, v in pre.state_dict().items()}
    # ---- GPU: finetune
    torch.manual_seed(1)
    ft = BaseModel.from_config(make_config(cfg, "CTR", None))
    F0 = {k: v.detach().clone() for k, v in ft.state_dict().items()}
    skipped = ft.load_from_target_model(pre_sd)
    assert any(k.startswith("mfp_criterion") for k in skipped) and "embed.embedding.weight" not in skipped
    ft = ft.to(DEV)
    opt = MapxOptimizer(ft, _targs(lr_sched="const", weight_decay=1e-1, pretrain=False), num_training_steps=n_ft,
                        num_warmup_steps=0)
    ft.train()
    for s in range(n_ft):
        r = rows(n_pre + s)
        loss = ft(input_ids=t(ids_all[r], DEV), labels=t(y_all[r], DEV))[0]
        loss.backward()
        opt.step()
    opt.flush()
    ft.eval()
    with torch.no_grad():
        logits = torch.cat([ft(input_ids=t(held_ids[i:i + 4096], DEV))[0].view(-1) for i in range(0, n_held, 4096)])
    met = ops.eval_metrics(logits, t(held_y, DEV))

    # ---- oracle: the same two phases with the reference's dense optimizer
    def adam_all(Pm, m, v, step, lr, wd):
        with torch.no_grad():
            for k, p in Pm.items():
                if p.requires_grad:
                    R.hf_adamw_step(p, p.grad, m[k], v[k], step, lr, wd=wd if R.decays(k) else 0.0)
                    p.grad = None
    trainable = lambda k, v: v.dtype.is_floating_point and "alias" not in k and "logprob" not in k
    Pm = {k: (v.clone().requires_grad_(True) if trainable(k, v) else v) for k, v in P0.items()}
    m = {k: torch.zeros_like(p) for k, p in Pm.items() if p.requires_grad}
    v = {k: torch.zeros_like(p) for k, p in Pm.items() if p.requires_grad}
    logq = R.nce_buffers(cnt)[0]
    for s in range(n_pre):
        masked, labels = R.dynamic_mask_mfp(t(ids_all[rows(s)]), t(mis[s]))
        fin = R.trunk(Pm, masked, cfg["NC"], cfg["NL"])
        R.mfp_head(Pm, fin, labels, t(mis[s]), t(noises[s]), logq, F, cfg["P"], K)[0].backward()
        adam_all(Pm, m, v, s + 1, 1e-3 * lr_lambda("cosine", s, n_pre, 0), 5e-2)
    Pf = {k: (Pm[k].detach().clone() if k in Pm and Pm[k].shape == w.shape else w.clone()) for k, w in F0.items()}
    Pf = {k: w.requires_grad_(True) for k, w in Pf.items()}
    m = {k: torch.zeros_like(p) for k, p in Pf.items()}
    v = {k: torch.zeros_like(p) for k, p in Pf.items()}
    for s in range(n_ft):
        r = rows(n_pre + s)
        R.ctr_head(Pf, R.trunk(Pf, t(ids_all[r]), cfg["NC"], cfg["NL"]), t(y_all[r]))[0].backward()
        adam_all(Pf, m, v, s + 1, 1e-3, 1e-1)
    with torch.no_grad():
        ref_logits = R.ctr_head(Pf, R.trunk(Pf, t(held_ids), cfg["NC"], cfg["NL"]))[0].view(-1)
    prob = torch.sigmoid(ref_logits).double().numpy()
    auc_ref, ll_ref = roc_auc_score(held_y, prob), log_loss(held_y, prob)
    assert auc_ref > 0.6, f"the finetuned oracle learned nothing (AUC {auc_ref:.4f}): the comparison would be vacuous"
    assert abs(met["auc"] - auc_ref) < 1e-4, (met["auc"], auc_ref)
    assert abs(met["logloss"] - ll_ref) < 1e-4, (met["logloss"], ll_ref)
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.numpy(), rtol=2e-3, atol=2e-4)
    print(f"held-out AUC hip {met['auc']:.6f} / oracle {auc_ref:.6f}; log-loss {met['logloss']:.6f} / {ll_ref:.6f}")


def test_graph_replay_equals_eager_bitwise_with_dropout():
    """hidden / embedding dropout on (layers.py:95,183): the Philox masks advance with the device-side
    update counter, so the captured step draws what the eager step draws — identical parameters."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * 6, 23, cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)

    def run(use_graph):
        torch.manual_seed(5)
        config = make_config(cfg, "MFP", cnt)
        config.hidden_dropout_rate, config.embed_dropout_rate = 0.2, 0.1
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir="/tmp/mapx_graph_drop", per_gpu_train_batch_size=512,
                                  per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine",
                                  weight_decay=5e-2, num_train_epochs=2, pretrain=True, pt_type="MFP",
                                  sampling_method="randint", mask_ratio=0.3, logging_steps=7, seed=11)
        targs._device = torch.device(DEV)
        os.makedirs(targs.output_dir, exist_ok=True)
        tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:600], labels[:600]))
        tr.use_graph = use_graph
        tr.MFP_pretrain()
        assert (len(tr._graphs) == 1 and len(H.captured(tr)) == 1) == use_graph
        return H.model_state(model)

    H.graph_vs_eager(run)


def test_capture_refuses_a_join_with_a_stream_outside_the_capture():
    """Round-1 DESIGN 4.5: a side-stream <- side-stream join once crashed hipStreamEndCapture.  The
    family of that failure — a captured stream made to wait for a stream that never forked from the
    capture's origin — is refused by ops.stream_wait / stream_wait_event with a Python error before
    HIP sees it; legal joins (fork from the origin, join back) still capture and replay."""
    from mapx import ops
    a = torch.zeros(1024, device=DEV)
    side, stranger = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        main = torch.cuda.current_stream()
        assert ops.stream_wait(side, main)                     # fork: side joins the capture
        with torch.cuda.stream(side):
            a.add_(1)
        ev = ops.record_event()
        with pytest.raises(ops.CaptureIsolationError):
            ops.stream_wait(side, stranger)                    # side is captured, stranger is not
        with pytest.raises(ops.CaptureIsolationError):
            with torch.cuda.stream(stranger):
                ev2 = ops.record_event()
            ops.stream_wait_event(main, ev2, stranger)
        assert ops.stream_wait_event(side, ev, main)           # legal: event of the origin
        assert not ops.stream_wait(main, main)                 # self-wait: skipped
        assert ops.stream_wait(main, side)                     # join back
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert float(a[0]) == 2.0


def _small_mfp_trainer(tmp, use_graph, seed=5, steps_rows=512 * 8):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(steps_rows, 23, cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    torch.manual_seed(seed)
    config = make_config(cfg, "MFP", cnt)
    model = BaseModel.from_config(config)
    targs = TrainingArguments(output_dir=str(tmp), per_gpu_train_batch_size=512, per_gpu_eval_batch_size=512,
                              learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2, num_train_epochs=1,
                              pretrain=True, pt_type="MFP", sampling_method="randint", mask_ratio=0.3, seed=11)
    targs._device = torch.device(DEV)
    ds = OurDataset(ids, labels)
    tr = Trainer(model, config, targs, ds, ds)
    tr.use_graph = use_graph
    train = tr._begin("test")
    model.train()
    return tr, list(train.batches(512, True, tr._generator(), (0, 1)))


def test_capture_that_dies_inside_backward_leaves_a_clean_eager_step(tmp_path):
    """a hipGraph capture that raises in the middle of the step (here: behind forward + backward,
    in front of the optimizer) leaves joins, deferred partial sums and the dense-ready event of the dead
    capture in the per-backward lists of mapx.ops; the eager retry must not see them.  Parameters after the
    run == the same run with capture never attempted, bit for bit."""
    from mapx import ops
    from mapx.trainer import Trainer
    out = []
    for sabotage in (True, False):
        tr, batches = _small_mfp_trainer(tmp_path, use_graph=sabotage)
        if sabotage:
            real = tr._optimizer_step

            def dying(*a, **k):
                if torch.cuda.is_current_stream_capturing():
                    # what a capture leaves behind when it dies here: the lists are NOT empty
                    assert ops.pending_joins or ops._deferred or ops.dense_ready[0] is not None
                    raise RuntimeError("capture sabotaged by the test")
                return real(*a, **k)
            tr._optimizer_step = dying
        for X, Y in batches:
            tr.run_step("mfp", X, Y)
        if sabotage:
            assert tr.use_graph is False               # the trainer fell back to eager steps
            assert not ops.pending_joins and not ops._deferred and ops.dense_ready[0] is None
        tr.optimizer.flush()
        out.append({k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()})
        del tr
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


def test_optimizer_state_with_another_flat_slot_size_is_repacked(tmp_path):
    """the dense moments are saved as the flat buffers; a state written with slots of 4 elements per
    parameter (round 1 / early round 2) must be re-packed into today's slots of 8, not copied misaligned."""
    tr, batches = _small_mfp_trainer(tmp_path, use_graph=False)
    for X, Y in batches[:3]:
        tr.run_step("mfp", X, Y)
    opt = tr.optimizer
    sd = opt.state_dict()
    assert sd["flat_pad"] == opt.FLAT_PAD == 8
    old = dict(sd)
    old.pop("flat_pad")                                 # a state from before the key existed: slots of 4
    old["groups"] = []
    for g, s in zip(opt.groups, sd["groups"]):
        m4, v4 = [], []
        off = 0
        for n in g["numels"]:
            pad4 = (n + 3) // 4 * 4
            for dst, src in ((m4, s["m"]), (v4, s["v"])):
                piece = torch.zeros(pad4)
                piece[:n] = src[off:off + n]
                dst.append(piece)
            off += (n + 7) // 8 * 8
        old["groups"].append(dict(names=s["names"], m=torch.cat(m4), v=torch.cat(v4)))
    before = [(g["m"].clone(), g["v"].clone()) for g in opt.groups]
    for g in opt.groups:
        g["m"].zero_(); g["v"].zero_()
    opt.load_state_dict(old)
    for (m, v), g in zip(before, opt.groups):
        assert torch.equal(m, g["m"]) and torch.equal(v, g["v"])
    bad = dict(old)
    bad["groups"] = [dict(names=s["names"], m=s["m"][:-4], v=s["v"][:-4]) for s in old["groups"]]
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)
    # a state WITHOUT the key but already in slots of 8 (written between the two changes): inferred, not assumed 4
    # (with a one-element parameter in it: tests/test_host_surface.py)
    keyless8 = dict(sd)
    keyless8.pop("flat_pad")
    for g in opt.groups:
        g["m"].zero_(); g["v"].zero_()
    opt.load_state_dict(keyless8)
    for (m, v), g in zip(before, opt.groups):
        assert torch.equal(m, g["m"]) and torch.equal(v, g["v"])


@pytest.mark.parametrize("pt", ["MFP", "RFD"])
def test_fused_backward_epilogues_equal_the_unfused_chain(tmp_path, pt):
    """The heads' dX GEMM doing both towers' first backward step, the cross layers' dX GEMMs doing the next
    layer's elementwise backward, and the cross layers' weight gradients from one launch (ops.JOIN_FUSE / CROSS_FUSE /
    DW_BATCH, whatever their defaults) against
    the chain of separate launches they replace: same parameters after 6 steps up to the order of the sums
    (bias gradients are added tile by tile instead of chunk by chunk, split-K slabs are cut differently)."""
    from mapx import ops
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * 6, 23, cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    out, calls = [], []
    real = ops.gemm_bwd_fused
    defaults = (ops.JOIN_FUSE, ops.CROSS_FUSE, ops.DW_BATCH)
    for fuse in (True, False):
        ops.JOIN_FUSE = ops.CROSS_FUSE = ops.DW_BATCH = fuse
        try:
            if fuse:
                ops.gemm_bwd_fused = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
            torch.manual_seed(5)
            config = make_config(cfg, pt, cnt if pt == "MFP" else None)
            model = BaseModel.from_config(config)
            targs = TrainingArguments(output_dir=str(tmp_path), per_gpu_train_batch_size=512,
                                      per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine",
                                      weight_decay=5e-2, num_train_epochs=1, pretrain=True, pt_type=pt,
                                      RFD_replace="Unigram", sampling_method="randint", mask_ratio=0.3, seed=11)
            targs._device = torch.device(DEV)
            ds = OurDataset(ids, labels)
            tr = Trainer(model, config, targs, ds, ds)
            tr.use_graph = False
            train = tr._begin("test")
            model.train()
            for X, Y in train.batches(512, True, tr._generator(), (0, 1)):
                tr.run_step(pt.lower(), X, Y)
            tr.optimizer.flush()
            out.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        finally:
            (ops.JOIN_FUSE, ops.CROSS_FUSE, ops.DW_BATCH), ops.gemm_bwd_fused = defaults, real
    assert len(calls) == 6 * 3          # per step: the cross half of the head's dX + two of the three cross layers'
    for k in out[0]:
        if out[0][k].dtype.is_floating_point:
            np.testing.assert_allclose(out[0][k].numpy(), out[1][k].numpy(), rtol=2e-4, atol=2e-6, err_msg=k)
