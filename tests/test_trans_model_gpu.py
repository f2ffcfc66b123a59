"""The Transformer backbone (model_name=trans) on the GPU: fixtures of the reference's own `Transformer` class (loss,
logits, every encoder layer's output, every gradient), the trunk at the benchmark's batch against a float64
torch.nn.TransformerEncoder with the same weights, graph replay == eager over Trainer steps, and bit-exact resume."""
import os

import numpy as np
import pytest
import torch

import model_harness as H
import paramgen as pg
import trans_params as tp
from util import assert_digest, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [(m, v) for v in tp.VARIANTS for m in tp.modes_of(v)]
TCFG = dict(F=23, V=3000, E=16, H=16, NL=2, NC=0, P=32, K=25)


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_reference_fixture(mode, variant):
    from mapx import ops
    cfg = pg.CASES[tp.CASE]
    z = np.load(os.path.join(GOLD, f"{tp.CASE}_{mode}_{variant}.npz"))
    inp = pg.make_inputs(tp.CASE, cfg)
    params = tp.make_params(cfg, mode, variant)
    model = tp.build_model(cfg, mode, variant, params, inp["feat_count"] if mode == "MFP" else None, device=DEV)
    ids, mi = t(inp["input_ids"], DEV), t(inp["masked_index"], DEV)
    model.train()
    if mode == "MFP":
        ids_in, labels, _ = ops.dynamic_mask_mfp(ids, mi.shape[1], masked_index=mi)
        loss, count, acc = model(input_ids=ids_in, labels=labels, masked_index=mi, noise_samples=t(inp["noise"], DEV))
        assert count == int(z["out/count"]) and int(acc) == int(z["out/total_acc"])
    elif mode == "RFD":
        ids_in, labels, _ = ops.dynamic_mask_rfd(ids, mi.shape[1], masked_index=mi,
                                                 replace_feat=t(inp["replace_feat"], DEV))
        loss, count, acc, pos = model(input_ids=ids_in, labels=labels)
        np.testing.assert_allclose(float(acc), float(z["out/acc"]), rtol=1e-6)
        np.testing.assert_allclose(float(pos), float(z["out/pos_ratio"]), rtol=1e-6)
    else:
        ids_in = ids
        loss, logits = model(input_ids=ids, labels=t(inp["y"], DEV))
        np.testing.assert_allclose(logits.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    loss.backward()
    for n, g in H.all_grads(model).items():
        assert g is not None, n
        assert_digest(z, "grad", n, g.cpu().numpy())
    with torch.no_grad():
        x = model.embed(ids_in)
        for li, layer in enumerate(model.encoder.layers):
            x = layer(x)
            want = z[f"mid/enc{li}"]
            np.testing.assert_allclose(x[:want.shape[0]].cpu().numpy(), want, rtol=1e-5, atol=2e-5)
        if mode == "RFD":
            np.testing.assert_allclose(model.pred_rfd(x.flatten(1)).cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("norm_first,act,heads", [(False, "relu", 1), (True, "gelu", 2)])
def test_full_batch_trunk_vs_float64_torch_encoder(norm_first, act, heads):
    """B = 4096, F = 23 (the benchmark's shape): the mapx trunk against torch.nn.TransformerEncoder in float64 with the
    same weights (the state-dict names are torch's), forward and every gradient of the trunk.  With relu, a hidden unit
    whose pre-activation is zero to fp32 rounding may sit on the other side of the kink than in float64: the reference
    then runs on the mapx step's own ReLU pattern, after checking that the patterns differ only at such units."""
    from mapx.models import BaseModel
    cfg = dict(F=23, V=3000, E=16, H=16, NL=3, NC=0, P=32, K=25)
    torch.manual_seed(1)
    over = dict(norm_first=norm_first, hidden_act=act, num_attn_heads=heads, num_hidden_layers=3, intermediate_size=128,
                layer_norm_eps=1e-5)
    model = BaseModel.from_config(tp.make_config(cfg, "CTR", "Trans", **over)).to(DEV)
    with torch.no_grad():                      # layers made different from each other, biases non-zero
        for p in model.encoder.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    model.train()
    B = 4096
    g = torch.Generator().manual_seed(2)
    x64 = torch.randn(B, 23, 16, generator=g, dtype=torch.float64)
    r64 = torch.randn(B, 23, 16, generator=g, dtype=torch.float64)
    masks = {}
    for i, lay in enumerate(model.encoder.layers):
        lay.linear1.register_forward_hook(lambda m, inp, o, i=i: masks.__setitem__(i, (o.detach() > 0).cpu()))
    x = x64.float().to(DEV).requires_grad_(True)
    out = model.encoder(x)
    (out * r64.float().to(DEV)).sum().backward()

    layer = torch.nn.TransformerEncoderLayer(16, heads, 128, dropout=0.0, activation=act, layer_norm_eps=1e-5,
                                             batch_first=True, norm_first=norm_first)
    ref = torch.nn.TransformerEncoder(layer, 3, enable_nested_tensor=False).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in model.encoder.state_dict().items()})
    ref.train()
    flips = 0
    if act == "relu":
        def pinned(z, i):
            nonlocal flips
            m = masks[i].view(z.shape)
            differ = m != (z > 0)
            flips += int(differ.sum())
            if differ.any():
                assert float(z[differ].abs().max()) <= 1e-5 * float(z.abs().max()), f"layer {i}: a unit off the kink flipped"
            return z * m.to(z.dtype)
        for i, lay in enumerate(ref.layers):
            lay.activation = lambda z, i=i: pinned(z, i)
    xr = x64.clone().requires_grad_(True)
    out_ref = ref(xr)
    (out_ref * r64).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().double().numpy(), out_ref.detach().numpy(), rtol=1e-4, atol=5e-5)
    assert flips < 1000

    def close(a, b, what):
        scale = float(b.abs().max())
        np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.numpy(), rtol=1e-4, atol=2e-5 * scale,
                                   err_msg=what)
    close(x.grad, xr.grad, "dX")
    refp = dict(ref.named_parameters())
    for n, p in model.encoder.named_parameters():
        close(p.grad, refp[n].grad, n)


def _trainer(mode, data, out_dir, epochs=2, seed=5, begin=False, **over):
    from mapx.models import BaseModel
    torch.manual_seed(seed)
    config = tp.make_config(TCFG, mode, "Trans", data[2], **over)
    return H.make_trainer(config, BaseModel.from_config(config), mode, data, out_dir, 512, epochs, 600, begin=begin)


@pytest.mark.parametrize("mode,p", [("MFP", 0.0), ("MFP", 0.1), ("CTR", 0.0)])
def test_graph_replay_equals_eager_bitwise(mode, p, tmp_path):
    """The captured step draws the Philox streams of the eager step (the attention-probability site included: a
    HipDropout the Trainer gives its seed, site and device-side step counter): identical parameters after two epochs
    with a ragged last batch, bit for bit."""
    data = H.synth_data(512 * 4 + 100, TCFG["F"], TCFG["V"], seed=3)

    def run(use_graph):
        tr, model = _trainer(mode, data, str(tmp_path / str(use_graph)), hidden_dropout_rate=p)
        tr.use_graph = use_graph
        tr.MFP_pretrain() if mode == "MFP" else tr.train()
        assert tr.global_step == 2 * 5
        assert bool(H.captured(tr)) == use_graph
        if p > 0:
            from mapx.layers import MhaDropout
            sites = [m for m in model.modules() if isinstance(m, MhaDropout)]
            assert len(sites) == 2 and all(m.step_counter is not None for m in sites)
        return H.model_state(model)

    H.graph_vs_eager(run)


def test_resume_state_continues_bit_exactly(tmp_path):
    """6 steps == 3 steps + save_training_state + fresh trainer + load_training_state + 3 steps (dropout on)."""
    data = H.synth_data(512 * 6, TCFG["F"], TCFG["V"], seed=4)

    def make():
        tr, _, batches = _trainer("MFP", data, str(tmp_path), epochs=1, seed=9, begin=True, hidden_dropout_rate=0.1)
        tr.use_graph = False
        return tr, batches

    H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"))


@pytest.mark.parametrize("M,N,K", [(94208, 1, 16), (94208, 16, 128), (94208, 16, 16)])
def test_narrow_layers_cover_every_row(M, N, K):
    """The Transformer's narrow layers run over B*F rows (94 208 at the benchmark's batch): field_reduction_attn's
    Linear(E, 1) forward and the input gradients of out_proj / linear2 take the streaming kernels (csrc/skinny.hip),
    whose grids must cover every row."""
    from mapx import ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    y = ops.linear_fwd(x.float().to(DEV), w.float().to(DEV), b.float().to(DEV))
    np.testing.assert_allclose(y.cpu().double().numpy(), (x @ w.T + b).numpy(), rtol=1e-4, atol=1e-4)
    dx = ops.linear_bwd_input(dy.float().to(DEV), w.float().to(DEV))
    np.testing.assert_allclose(dx.cpu().double().numpy(), (dy @ w).numpy(), rtol=1e-4, atol=1e-4)
