"""The FiGNN backbone (model_name=fignn through build_backbone / run.py) on the GPU: fixtures of the reference's own
`FiGNN` class (loss, logits, the attention graph, the trunk's output, every gradient), graph replay == eager over
Trainer steps, bit-exact resume, run.py pretraining followed by finetuning, and a short AdamW trajectory."""
import math
import os

import numpy as np
import pytest
import torch

import fignn_params as fp
import model_harness as H
import paramgen as pg
from util import GOLD, assert_digest, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]
SMALL = dict(F=23, V=3000, E=16, H=16, NL=2, NC=0, P=32, K=25)


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_reference_fixture(mode, variant):
    from mapx import ops
    cfg = pg.CASES[fp.CASE]
    z = np.load(os.path.join(GOLD, f"{fp.CASE}_{mode}_{variant}.npz"))
    inp = pg.make_inputs(fp.CASE, cfg)
    params = fp.make_params(cfg, mode, variant)
    model = fp.build_model(cfg, mode, variant, params, inp["feat_count"] if mode == "MFP" else None, device=DEV)
    ids, mi = t(inp["input_ids"], DEV), t(inp["masked_index"], DEV)
    model.train()
    seen = {}
    hook = model.fignn.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach(), h=o.detach()))
    if mode == "MFP":
        ids_in, labels, _ = ops.dynamic_mask_mfp(ids, mi.shape[1], masked_index=mi)
        H.capture_mfp_logits(model.mfp_criterion, seen)
        loss, count, acc = model(input_ids=ids_in, labels=labels, masked_index=mi, noise_samples=t(inp["noise"], DEV))
        assert count == int(z["out/count"]) and int(acc) == int(z["out/total_acc"])
        np.testing.assert_allclose(seen["logits"].cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    elif mode == "RFD":
        ids_in, labels, _ = ops.dynamic_mask_rfd(ids, mi.shape[1], masked_index=mi,
                                                 replace_feat=t(inp["replace_feat"], DEV))
        cap = model.pred_rfd.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach()))
        loss, count, acc, pos = model(input_ids=ids_in, labels=labels)
        cap.remove()
        np.testing.assert_allclose(float(acc), float(z["out/acc"]), rtol=1e-6)
        np.testing.assert_allclose(float(pos), float(z["out/pos_ratio"]), rtol=1e-6)
        np.testing.assert_allclose(seen["logits"].cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    else:
        loss, logits = model(input_ids=ids, labels=t(inp["y"], DEV))
        np.testing.assert_allclose(logits.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    hook.remove()
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    rows = z["mid/h"].shape[0]
    np.testing.assert_allclose(seen["h"][:rows].cpu().numpy(), z["mid/h"], rtol=1e-5, atol=2e-5)
    g, _, _ = ops.fignn_graph_fwd(seen["x"].contiguous(), model.fignn.W_attn.weight.detach())
    np.testing.assert_allclose(g[:rows].cpu().numpy(), z["mid/graph"], rtol=1e-5, atol=1e-6)
    loss.backward()
    grads = H.all_grads(model)
    assert set(grads) == set(params)
    for n, gr in grads.items():
        assert gr is not None, n
        assert_digest(z, "grad", n, gr.cpu().numpy())


def _trainer(mode, data, out_dir, epochs=2, seed=5, variant="FiGNN", begin=False):
    from mapx.models import build_backbone
    torch.manual_seed(seed)
    config = fp.make_config(SMALL, mode, variant, data[2])
    return H.make_trainer(config, build_backbone(config), mode, data, out_dir, 512, epochs, 600, begin=begin)


@pytest.mark.parametrize("mode,variant", [("MFP", "FiGNN"), ("CTR", "FiGNNShare")])
def test_graph_replay_equals_eager_bitwise(mode, variant, tmp_path):
    """Identical parameters after two epochs with a ragged last batch, bit for bit; and the optimizer keeps no weight
    planes and attaches no magnitude record for the parameters that only the FiGNN kernels read."""
    data = H.synth_data(512 * 4 + 100, SMALL["F"], SMALL["V"], 3)

    def run(use_graph):
        tr, model = _trainer(mode, data, str(tmp_path / str(use_graph)), variant=variant)
        tr.use_graph = use_graph
        tr.MFP_pretrain() if mode == "MFP" else tr.train()
        assert tr.global_step == 2 * 5
        assert bool(H.captured(tr)) == use_graph
        for n, p in model.fignn.named_parameters():
            assert getattr(p, "_planes", None) is None and getattr(p, "_amax", None) is None, n
            assert getattr(p, "_mapx_grad", None) is not None, n
        return H.model_state(model)

    state, _ = H.graph_vs_eager(run)
    for k in state:
        assert bool(torch.isfinite(state[k]).all()), k


def test_resume_state_continues_bit_exactly(tmp_path):
    """6 steps == 3 steps + save_training_state + fresh trainer + load_training_state + 3 steps."""
    data = H.synth_data(512 * 6, SMALL["F"], SMALL["V"], 4)

    def make():
        tr, _, batches = _trainer("MFP", data, str(tmp_path), epochs=1, seed=9, begin=True)
        tr.use_graph = False
        assert sorted(tb.table.name for tb in tr.optimizer.tables) == ["embed.embedding", "mfp_criterion"]
        return tr, batches

    H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"))


def test_run_py_fignn_pretrain_then_finetune(tmp_path):
    common = ["--model_name=fignn", "--embed_size=16", "--hidden_size=16", "--num_hidden_layers=2", "--res_conn=True",
              "--logging_steps=3"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"], [])
    trunk = sorted(k for k in sd if k.startswith(("fignn.", "embed.")))
    assert "fignn.gnn.1.W_out" in trunk and "fignn.gru.bias_hh" in trunk and "fignn.W_attn.weight" in trunk
    for k in trunk:
        assert f"Load tensor: {k}," in log, k
    assert "Unmatched tensor in the target model: feat_encoder.weight" in log
    H.finite_metrics(log)


def test_adamw_trajectory_lowers_the_loss_of_a_fixed_batch():
    """Eight AdamW steps on one CTR batch (res_conn, three layers): the loss falls and every parameter moves."""
    from mapx.arguments import TrainingArguments
    from mapx.models import build_backbone
    from mapx.optim import MapxOptimizer
    ids, labels, _ = H.synth_data(256, SMALL["F"], SMALL["V"], 6)
    torch.manual_seed(2)
    model = build_backbone(fp.make_config(SMALL, "CTR", "FiGNN", None, res_conn=True)).to(DEV).train()
    targs = TrainingArguments(output_dir="unused", learning_rate=1e-2, weight_decay=0.0, lr_sched="const")
    opt = MapxOptimizer(model, targs, num_training_steps=8, num_warmup_steps=0)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith(("fignn.", "fc."))}
    X, Y = t(ids, DEV), t(labels, DEV).float()
    losses = []
    for _ in range(8):
        loss, _ = model(input_ids=X, labels=Y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0] - 1e-3, losses
    for n, p in model.named_parameters():
        if n in before:
            assert not torch.equal(p.detach(), before[n]), n
