"""The FGCNN backbone (model_name=fgcnn) on the GPU: fixtures of the reference's own `FGCNN` class (loss, logits,
`combined`, every gradient, the batch-norm buffers after one training forward, eval-mode outputs), graph replay ==
eager over Trainer steps (batch-norm buffers and num_batches_tracked included), bit-exact resume, and run.py
pretraining followed by finetuning."""
import os

import numpy as np
import pytest
import torch

import fgcnn_params as fp
import model_harness as H
import paramgen as pg
from util import GOLD, assert_digest, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]
SMALL = dict(channels="3,4", kernel_heights="3,5", pooling_sizes="2,2", recombined_channels="2,1")
TCFG = dict(F=23, V=3000, E=16, H=32, NL=2, NC=0, P=32, K=25)


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
    hook = model.fgcnn_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("new", o.detach()))
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
        ids_in = ids
        loss, logits = model(input_ids=ids, labels=t(inp["y"], DEV))
        np.testing.assert_allclose(logits.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    hook.remove()
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    want = z["mid/combined"]
    F = cfg["F"]
    np.testing.assert_allclose(seen["new"][:want.shape[0]].cpu().numpy(), want[:, F:], rtol=1e-5, atol=2e-5)
    loss.backward()
    grads = H.all_grads(model)
    assert set(grads) == set(params)
    for n, g in grads.items():
        assert g is not None, n
        assert_digest(z, "grad", n, g.cpu().numpy())
    # the batch-norm buffers after ONE training forward
    sd = model.state_dict()
    for k in fp.bn_buffer_names(cfg, variant):
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(z[f"bn/{k}"]) == 1
        else:
            np.testing.assert_allclose(sd[k].cpu().numpy(), z[f"bn/{k}"], rtol=1e-5, atol=1e-6, err_msg=k)
    # eval mode on other running statistics: no plan, no gradient state, buffers untouched
    H.load_params(model, fp.eval_buffers(cfg, variant))
    model.eval()
    before = {k: sd[k].clone() for k in fp.bn_buffer_names(cfg, variant)}
    for tb in model.row_tables():
        tb.plan = None                  # (the training step's): eval must not ask for a new one
    with torch.no_grad():
        combined = model.combined_features(ids_in)
        want = z["eval/combined"]
        np.testing.assert_allclose(combined[:want.shape[0]].cpu().numpy(), want, rtol=1e-5, atol=2e-5)
        if mode == "CTR":
            np.testing.assert_allclose(model(input_ids=ids)[0].cpu().numpy(), z["eval/logits"], rtol=1e-5, atol=1e-5)
        elif mode == "RFD":
            from mapx.layers import inner_product
            dense = torch.cat([combined.flatten(1), inner_product(combined)], dim=1)
            np.testing.assert_allclose(model.pred_rfd(dense).cpu().numpy(), z["eval/logits"], rtol=1e-5, atol=1e-5)
    assert all(tb.plan is None for tb in model.row_tables())
    for k, v in before.items():
        assert torch.equal(model.state_dict()[k], v), k


def _trainer(mode, data, out_dir, epochs=2, seed=5, begin=False):
    from mapx.models import BaseModel
    torch.manual_seed(seed)
    config = fp.make_config(TCFG, mode, "FGCNN", data[2], **SMALL)
    return H.make_trainer(config, BaseModel.from_config(config), mode, data, out_dir, 512, epochs, 600, begin=begin)


@pytest.mark.parametrize("mode", ["MFP", "CTR"])
def test_graph_replay_equals_eager_bitwise(mode, tmp_path):
    """Identical state after two epochs with a ragged last batch, bit for bit: parameters of both embedding tables,
    the batch-norm running statistics and num_batches_tracked (all moved by kernels inside the captured step)."""
    data = H.synth_data(512 * 4 + 100, TCFG["F"], TCFG["V"], seed=3)

    def run(use_graph):
        tr, model = _trainer(mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        tr.MFP_pretrain() if mode == "MFP" else tr.train()
        assert tr.global_step == 2 * 5
        assert bool(H.captured(tr)) == use_graph
        return H.model_state(model)

    state, _ = H.graph_vs_eager(run)
    tracked = [k for k in state if k.endswith("num_batches_tracked")]
    assert len(tracked) == 2
    assert all(int(state[k]) == 10 for k in tracked)       # train-mode forwards only: evaluation does not count


def test_resume_state_continues_bit_exactly(tmp_path):
    """6 steps == 3 steps + save_training_state + fresh trainer + load_training_state + 3 steps: three row tables'
    lazy state, the batch-norm buffers and the batch counters all travel."""
    data = H.synth_data(512 * 6, TCFG["F"], TCFG["V"], seed=4)

    def make():
        tr, _, batches = _trainer("MFP", data, str(tmp_path), epochs=1, seed=9, begin=True)
        tr.use_graph = False
        assert sorted(tb.table.name for tb in tr.optimizer.tables) == ["embed.embedding", "fg_embed.embedding",
                                                                      "mfp_criterion"]
        return tr, batches

    def after_load(tr):
        assert int(tr.model.state_dict()["fgcnn_layer.conv_layers.0.1.num_batches_tracked"]) == 3

    ref = H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"), after_load=after_load)
    assert int(ref["fgcnn_layer.conv_layers.1.1.num_batches_tracked"]) == 6


def test_run_py_fgcnn_pretrain_then_finetune(tmp_path):
    common = ["--model_name=fgcnn", "--embed_size=16", "--hidden_size=32", "--num_hidden_layers=2",
              "--logging_steps=3"] + [f"--{k}={v}" for k, v in SMALL.items()]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"], [])
    trunk = sorted(k for k in sd if k.startswith(("fgcnn_layer.", "fg_embed.", "embed.", "ip_layer.")))
    assert "fgcnn_layer.conv_layers.1.1.running_var" in trunk and "fg_embed.embedding.weight" in trunk
    assert int(sd["fgcnn_layer.conv_layers.0.1.num_batches_tracked"]) == (3200 + 511) // 512
    for k in trunk:
        assert f"Load tensor: {k}," in log, k
    assert "Unmatched tensor in the target model: feat_encoder.weight" in log
    H.finite_metrics(log)

