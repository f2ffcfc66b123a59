"""Model-level parity on the GPU: mapx.DCNV2 (HIP kernels through the C ABI) against
(1) the committed golden vectors captured from the real reference and (2) the oracle on
larger seeded inputs, for the three modes of the hot path.  fp32 tolerance = north star 1e-5
relative on logits/loss; gradients 2e-5 relative to their scale against the fixtures, and 1e-5 of
their scale against the oracle run in fp64 at the BASELINE batch size (test_full_batch_vs_fp64_oracle)."""
import numpy as np
import pytest
import torch

import paramgen as pg
import row_widths_ref as RW
from model_harness import all_grads, load_params
from util import assert_digest, build_model, load_case, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = list(pg.CASES)
OTHER = [("B_f25_b64", b) for b in pg.BACKBONES[1:]]      # DNN, DeepFM


def _check_grads(z, model, pattern=None, tag=None):
    """Every gradient against the fixture of the real reference; `tag` names the case in the summary of what
    was compared (util.note_golden: "direct" or "pattern-fallback" + the number of flipped units), and a case
    that is not listed in tests/golden/pattern_fallback_allowed.json must pass directly.  `pattern` = (masks of the step's fused
    ReLU layers, mode, cfg, params, inp): with 7 or 64 rows ONE hidden unit whose pre-activation is
    zero to fp32 rounding, and which this arithmetic puts on the other side of the ReLU's kink than the
    reference's did, is a visible share of a gradient row.  Then — and only then — the comparison
    falls back to the oracle (pinned to the same fixture, tests/test_oracle_golden.py) re-run on the
    step's own activation pattern, after checking that the patterns differ only at such units."""
    from util import fallback_allowed, note_golden
    grads = all_grads(model)
    try:
        for n, g in grads.items():
            assert g is not None, n
            assert_digest(z, "grad", n, g.cpu().numpy())
        note_golden(tag, "direct")
        return
    except AssertionError:
        if pattern is None:
            raise
    from util import check_pattern, oracle_case_grads
    masks, mode, cfg, params, inp = pattern
    pre = {}
    oracle_case_grads(mode, cfg, params, inp, preacts=pre)
    flips = check_pattern(masks, pre, f"golden {mode}", tol=2e-6)
    assert flips > 0, "gradients differ from the fixture although the ReLU pattern is the reference's"
    note_golden(tag, "pattern-fallback", flips)
    assert fallback_allowed(tag), (f"{tag}: the gradients no longer match the reference's fixture directly ({flips} hidden "
                                   "units on the other side of the ReLU kink); this case passed directly when "
                                   "tests/golden/pattern_fallback_allowed.json was written")
    _, _, ref = oracle_case_grads(mode, cfg, params, inp, relu_masks=masks)
    for n, g in grads.items():
        scale = float(np.abs(ref[n]).max())
        np.testing.assert_allclose(g.cpu().numpy(), ref[n], rtol=2e-5, atol=2e-5 * scale + 1e-12, err_msg=n)


@pytest.fixture(params=["x3", "h2"])
def arith(request, monkeypatch):
    """The golden and full-batch tests run twice: a model nobody optimizes has no magnitude records, so its products
    take the six-product bf16 arithmetic ("x3"); with ops.AUTO_AMAX every product gets the records — and weight
    planes — a training step's kernels leave, and takes the two-piece fp16 arithmetic the Trainer's steps run on
    ("h2": csrc/gemm_h2.hip, gemm_h2w.hip).  Same fixtures, same tolerances."""
    from mapx import ops
    monkeypatch.setattr(ops, "AUTO_AMAX", request.param == "h2")
    return "" if request.param == "x3" else "/h2"


@pytest.mark.parametrize("case", CASES)
def test_mfp_golden(case, arith):
    cfg, z, inp, params = load_case(case, "MFP")
    model = build_model(cfg, "MFP", params, inp["feat_count"])
    from util import hook_relu_pattern
    masks = hook_relu_pattern(model)
    model.mfp_criterion.return_logits = True
    np.testing.assert_allclose(model.mfp_criterion.logprob_noise.cpu().numpy(), z["nce/logprob_noise"],
                               rtol=1e-6, atol=1e-6)
    assert np.array_equal(model.mfp_criterion.alias.alias.cpu().numpy(), z["nce/alias_alias"])
    assert np.array_equal(model.mfp_criterion.alias.prob.cpu().numpy(), z["nce/alias_prob"])
    from mapx import ops
    ids = t(inp["input_ids"], DEV)
    mi = t(inp["masked_index"], DEV)
    masked, labels, _ = ops.dynamic_mask_mfp(ids, mi.shape[1], masked_index=mi)
    assert np.array_equal(masked.cpu().numpy(), z["in/input_ids_masked"])
    assert np.array_equal(labels.cpu().numpy(), z["in/labels"])
    model.train()
    loss, count, acc = model(input_ids=masked, labels=labels, masked_index=mi,
                             noise_samples=t(inp["noise"], DEV))
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    assert count == int(z["out/count"]) and int(acc) == int(z["out/total_acc"])
    loss.backward()
    _check_grads(z, model, (masks, "MFP", cfg, params, inp), tag=f"DCNv2/MFP/{case}{arith}")


@pytest.mark.parametrize("case", CASES)
def test_mfp_logits_golden(case):
    cfg, z, inp, params = load_case(case, "MFP")
    model = build_model(cfg, "MFP", params, inp["feat_count"])
    model.mfp_criterion.return_logits = True
    model.eval()
    with torch.no_grad():
        feat = model.embed(t(z["in/input_ids_masked"], DEV)).flatten(1)
        final = torch.cat([model.cross_net(feat), model.parallel_dnn(feat)], -1)
        enc = model.feat_encoder(final)
        _, logits, idx = model.mfp_criterion(t(z["in/labels"], DEV), enc,
                                             masked_index=t(inp["masked_index"], DEV),
                                             noise_samples=t(inp["noise"], DEV))
    np.testing.assert_allclose(logits.cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(idx.cpu().numpy(), z["out/indices"])


@pytest.mark.parametrize("case", CASES)
def test_rfd_golden(case, arith):
    cfg, z, inp, params = load_case(case, "RFD")
    model = build_model(cfg, "RFD", params, None)
    from util import hook_relu_pattern
    masks = hook_relu_pattern(model)
    from mapx import ops
    ids, mi = t(inp["input_ids"], DEV), t(inp["masked_index"], DEV)
    replaced, labels, _ = ops.dynamic_mask_rfd(ids, mi.shape[1], masked_index=mi,
                                               replace_feat=t(inp["replace_feat"], DEV))
    assert np.array_equal(replaced.cpu().numpy(), z["in/input_ids_replaced"])
    assert np.array_equal(labels.cpu().numpy(), z["in/labels"])
    model.train()
    loss, count, acc, pos = model(input_ids=replaced, labels=labels)
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    assert count == int(z["out/count"])
    np.testing.assert_allclose(float(acc), float(z["out/acc"]), rtol=1e-6)
    np.testing.assert_allclose(float(pos), float(z["out/pos_ratio"]), rtol=1e-6)
    loss.backward()
    _check_grads(z, model, (masks, "RFD", cfg, params, inp), tag=f"DCNv2/RFD/{case}{arith}")


@pytest.mark.parametrize("case", CASES)
def test_ctr_golden(case, arith):
    cfg, z, inp, params = load_case(case, "CTR")
    model = build_model(cfg, "CTR", params, None)
    from util import hook_relu_pattern
    masks = hook_relu_pattern(model)
    ids = t(inp["input_ids"], DEV)
    model.train()
    feat = model.embed(ids).flatten(1)
    assert np.array_equal(feat.detach().cpu().numpy(), z["mid/embed_flat"])           # bit-exact gather
    np.testing.assert_allclose(model.cross_net(feat).detach().cpu().numpy(), z["mid/cross_out"],
                               rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(model.parallel_dnn(feat).detach().cpu().numpy(), z["mid/dnn_out"],
                               rtol=1e-5, atol=1e-5)
    loss, logits = model(input_ids=ids, labels=t(inp["y"], DEV))
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
    loss.backward()
    _check_grads(z, model, (dict(masks), "CTR", cfg, params, inp), tag=f"DCNv2/CTR/{case}{arith}")
    (logits_only,) = model(input_ids=ids)
    np.testing.assert_allclose(logits_only.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)


def _three_way(name, got, g32, g64, tol=1e-5):
    """North star for BASELINE-size tensors: `got` (HIP, fp32) lies within `tol` of the EXACT value
    (the oracle run in fp64 on the same activation pattern), relative to the tensor's scale,
    element by element.  Returned for the report: the same error of the reference's own CPU fp32
    arithmetic (the oracle in fp32) — NOT the yardstick: at 4096-row reductions its rounding is of
    the size of the differences being judged (and its summation order is not the MFMA's).
    -> (hip error / scale, cpu fp32 error / scale)."""
    g64 = g64.detach().double().cpu().numpy()
    scale = float(np.abs(g64).max())
    e_hip = float(np.abs(got.detach().double().cpu().numpy() - g64).max())
    e_cpu = float(np.abs(g32.detach().double().cpu().numpy() - g64).max())
    assert e_hip <= tol * scale, f"{name}: |hip - exact| = {e_hip:.3e} > {tol:g} x scale {scale:.3e} (cpu fp32: {e_cpu:.3e})"
    return (e_hip / scale, e_cpu / scale) if scale > 0 else (0.0, 0.0)


def _oracle_pass(mode, P, model_inputs, cfg, cnt, dtype, relu_masks=None, preacts=None):
    """The oracle's loss / outputs / gradients from state_dict `P` in fp32 or fp64 arithmetic
    (`relu_masks`: impose an activation pattern; `preacts`: collect the pre-activations)."""
    from oracle import ref_model as R
    Q = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.dtype.is_floating_point
             and "alias" not in k and "logprob" not in k else v) for k, v in P.items()}
    fin = R.trunk(Q, model_inputs["ids"], cfg["NC"], cfg["NL"], relu_masks=relu_masks, preacts=preacts)
    if mode == "MFP":
        logq = R.nce_buffers(cnt)[0].to(dtype)
        loss, out, acc = R.mfp_head(Q, fin, model_inputs["labels"], model_inputs["mi"], model_inputs["noise"], logq,
                                    cfg["F"], cfg["P"], cfg["K"])
    elif mode == "RFD":
        loss, _, acc, _, out = R.rfd_head(Q, fin, model_inputs["labels"].to(dtype), relu_masks=relu_masks,
                                          preacts=preacts)
    else:
        logits = fin @ Q["fc_out.weight"].t() + Q["fc_out.bias"]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), model_inputs["labels"].to(dtype))
        out, acc = logits, None
    loss.backward()
    return loss.detach(), out.detach(), acc, {k: v.grad for k, v in Q.items() if torch.is_tensor(v) and v.requires_grad}


@pytest.mark.parametrize("mode,B,F", [("MFP", 4096, 23), ("RFD", 4096, 23), ("CTR", 4096, 23), ("MFP", 777, 39),
                                      ("RFD", 777, 39)])
def test_full_batch_vs_fp64_oracle(mode, B, F, arith):
    """BASELINE configs[1], [3], [4] at their real batch size (4096 x 23, K = 25, P = 32, H = 1000):
    generated masks / negatives / replacements of the GPU step are fed to the oracle, which runs
    twice — in fp64 (the exact answer) and in fp32 (the reference's CPU arithmetic).  Loss, logits
    and EVERY gradient (dense and table rows) must be within 1e-5 of the exact value at the tensor's
    scale (north star: 1e-5 fp32) and not noisier than the CPU fp32 path."""
    _full_batch_vs_fp64_oracle(mode, B, F)


# (E, B): the widths whose rows take another lane-group form than 16 (tests/row_widths_ref.py) and whose dense side has
# D = 23 E = 184, 276, 552, 1472 instead of 368; B = 1024 x H = 1000 is 8 x 16 tiles, the threshold of ops.planes_wanted
WIDTH_STEPS = [(8, 1024), (12, 1024), (24, 1024), (64, 1024), (12, 96)]


@pytest.mark.parametrize("E,B", WIDTH_STEPS)
@pytest.mark.parametrize("mode", ["MFP", "RFD", "CTR"])
def test_full_batch_vs_fp64_oracle_at_other_embed_sizes(mode, E, B, arith):
    """The step of test_full_batch_vs_fp64_oracle, same assertions, at embed_size 8, 12, 24 and 64 (F = 23, H = 1000).
    At E = 12 the first layers have K = 276 (K % 8 == 4: no weight planes) and the hidden ones K = 1000 (planes at
    B = 1024, none at B = 96); the encoder and head widths D + H are 4 mod 8 too."""
    from mapx import ops
    assert E in RW.ROW_WIDTHS
    if B == 1024:
        assert ops.planes_wanted(1024, 1000, 1000) and not ops.planes_wanted(1024, 1000, 23 * 12)
    else:
        assert not ops.planes_wanted(B, 1000, 1000) and not ops.planes_wanted(B, 1000, 23 * E)
    _full_batch_vs_fp64_oracle(mode, B, 23, E=E)


def _full_batch_vs_fp64_oracle(mode, B, F, E=16, H=1000):
    from mapx import ops
    from mapx.dataset import synth_table
    from util import make_config
    from mapx.models import BaseModel
    cfg = dict(F=F, V=60000, E=E, H=H, NL=3, NC=3, P=32, K=25)
    tag = f"{mode} B={B} F={F}" + ("" if E == 16 else f" E={E}")
    ids_np, y_np, _, _ = synth_table(B, F, cfg["V"], seed=1)
    cnt = np.bincount(ids_np.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    torch.manual_seed(0)
    model = BaseModel.from_config(make_config(cfg, mode, cnt if mode == "MFP" else None)).to(DEV)
    L = int(F * 0.3)
    ids = torch.from_numpy(ids_np).to(DEV)
    model.train()
    hip_masks = {}
    for name, mod in model.named_modules():             # the activation pattern of the step under test
        if getattr(mod, "relu", False):
            mod.register_forward_hook(lambda m, i, o, name=name: hip_masks.__setitem__(name, (o.detach() > 0).cpu()))
    if mode == "MFP":
        model.mfp_criterion.return_logits = True
        masked, labels, mi = ops.dynamic_mask_mfp(ids, L, seed=7, offset=1)
        feat = model.embed(masked).flatten(1)
        final = torch.cat([model.cross_net(feat), model.parallel_dnn(feat)], -1)
        enc = model.feat_encoder(final)
        loss, out, idx = model.mfp_criterion(labels, enc, masked_index=mi)
        acc = int(model.mfp_criterion.last_acc)
        assert torch.equal(idx[..., 0].long(), labels)
        inputs = dict(ids=masked.cpu(), labels=labels.cpu(), mi=mi.cpu(), noise=idx[..., 1:].long().cpu())
    elif mode == "RFD":
        x_train = torch.from_numpy(synth_table(3 * B, F, cfg["V"], seed=2)[0]).to(DEV)
        replaced, labels, _ = ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=7, offset=1, mode="Unigram")
        assert 0.05 < float(labels.mean()) < 0.4
        model.pred_rfd["2"].register_forward_hook(lambda m, i, o: setattr(model, "_rfd_logits", o.detach()))
        loss, _, acc, _ = model(input_ids=replaced, labels=labels)
        out = model._rfd_logits
        inputs = dict(ids=replaced.cpu(), labels=labels.cpu())
    else:
        y = torch.from_numpy(y_np).to(DEV)
        loss, out = model(input_ids=ids, labels=y)
        acc = None
        inputs = dict(ids=ids.cpu(), labels=y.cpu())
    loss.backward()

    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    # The exact pass runs on the activation pattern of the step under test.  Where that pattern
    # differs from what fp64 itself decides, the pre-activation must be zero to rounding (a unit
    # that fp32 puts on the other side of the ReLU's kink): anything else is an arithmetic error.
    pre64 = {}
    _oracle_pass(mode, P, inputs, cfg, cnt, torch.float64, preacts=pre64)
    assert set(pre64) == set(hip_masks), (sorted(pre64), sorted(hip_masks))
    flips = 0
    for k, z in pre64.items():
        differ = hip_masks[k] != (z > 0)
        flips += int(differ.sum())
        if differ.any():
            assert float(z[differ].abs().max()) <= 2e-6 * float(z.abs().max()), \
                f"{k}: a unit with pre-activation {float(z[differ].abs().max()):.3e} is on the wrong side of the ReLU"
    loss64, out64, acc64, g64 = _oracle_pass(mode, P, inputs, cfg, cnt, torch.float64, relu_masks=hip_masks)
    pre32 = {}
    loss32, out32, _, g32 = _oracle_pass(mode, P, inputs, cfg, cnt, torch.float32, preacts=pre32)
    flips32 = sum(int(((z > 0) != hip_masks[k]).sum()) for k, z in pre32.items())
    print(f"[{tag}] ReLU units decided differently from fp64: hip {flips}, hip vs cpu fp32 {flips32} "
          f"of {sum(z.numel() for z in pre64.values())}")
    assert abs(float(loss.detach()) - float(loss64)) <= 2e-6 * abs(float(loss64)), (float(loss.detach()), float(loss64))
    # logits: 1e-5 of max(1, |logit|) element by element
    d = (out.detach().double().cpu().view(out64.shape) - out64).abs() / out64.abs().clamp(min=1.0)
    assert float(d.max()) <= 1e-5, float(d.max())
    if mode == "MFP":
        assert abs(acc - acc64) <= 2                      # exact ties aside
    elif mode == "RFD":
        assert abs(float(acc) - float(acc64)) <= 2.0 / out64.numel()
    report = {n: _three_way(n, g, g32[n], g64[n]) for n, g in all_grads(model).items()}
    worst = max(report, key=lambda k: report[k][0])
    print(f"[{tag}] worst gradient error vs fp64 / scale: hip {report[worst][0]:.2e} at {worst}; "
          f"cpu fp32 oracle on its own pattern: {max(v[1] for v in report.values()):.2e}")


def test_eval_mode_needs_no_plan_and_matches_train_forward():
    cfg, z, inp, params = load_case("A_f23_b7", "CTR")
    model = build_model(cfg, "CTR", params, None)
    ids = t(inp["input_ids"], DEV)
    model.eval()
    with torch.no_grad():
        (a,) = model(input_ids=ids)
    assert model.embed.table.plan is None
    model.train()
    (b,) = model(input_ids=ids)
    assert torch.equal(a, b.detach())


def test_unknown_backbones_raise_like_the_reference():
    from mapx.models import BaseModel
    from util import make_config
    cfg = pg.CASES["A_f23_b7"]
    for name in ("fignn", "nonsense"):
        c = make_config(cfg, "CTR")
        c.model_name = name
        with pytest.raises(NotImplementedError):
            BaseModel.from_config(c)


@pytest.mark.parametrize("E,NC", [(4, 2), (16, 1), (16, 0)])
def test_cross_tower_depths_vs_oracle(E, NC):
    """Narrow rows, a hidden width that is not a multiple of 4, and 0 / 1 / 2 cross layers:
    forward and every gradient of the DCNv2 trunk + CTR head against the oracle."""
    from mapx.models import BaseModel
    from oracle import ref_model as R
    from util import make_config
    cfg = dict(F=5, V=300, E=E, H=10, NL=2, NC=NC, P=32, K=5)
    torch.manual_seed(3)
    model = BaseModel.from_config(make_config(cfg, "CTR", None)).to(DEV)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, cfg["V"], (9, cfg["F"]), generator=g)
    y = torch.randint(0, 2, (9,), generator=g)
    loss, logits = model(input_ids=ids.to(DEV), labels=y.to(DEV))
    loss.backward()
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()
              if v.dtype.is_floating_point}
    fin = R.trunk(params, ids, NC, cfg["NL"])
    loss_ref, logits_ref = R.ctr_head(params, fin, y)
    loss_ref.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy().ravel(), logits_ref.detach().numpy().ravel(),
                               rtol=1e-5, atol=1e-6)
    from mapx.optim import decays  # noqa: F401  (import check only)
    for name, p in model.named_parameters():
        if name == "embed.embedding.weight":
            got = model.embed.table.dense_grad()[0].cpu()
        else:
            got = p.grad.cpu()
        np.testing.assert_allclose(got.numpy(), params[name].grad.numpy(), rtol=2e-5, atol=2e-6, err_msg=name)


@pytest.mark.parametrize("backbone,mode,E", [("DeepFM", "MFP", 8), ("AutoInt", "CTR", 12)])
def test_other_backbones_at_narrow_embed_sizes_vs_float64(backbone, mode, E):
    """Rows on four lanes of which two (E = 8) or one (E = 12) idle, at B = 96, in the manner of
    test_cross_tower_depths_vs_oracle, same tolerances, the reference in float64 on the step's own ReLU pattern
    (bf16_backbones_ref.step).  DeepFM MFP: the LR weight is the scalar table p1 of the embedding's rows, so its
    gradient comes out of the reduction with the extra scalar and the heads read H + 1 columns; E = 8 because the FM
    kernels take 4, 8, 16, 32 and 64 (DeepFM refuses 12 when it is built: tests/test_host_surface.py).  AutoInt CTR:
    2 layers x 2 heads x 12, the first with W_res (12 -> 24)."""
    import bf16_backbones_ref as BR
    from mapx import ops
    from mapx.layers import MultiHeadSelfAttention
    from mapx.models import BaseModel
    from oracle import ref_model as R
    from util import check_pattern, hook_relu_pattern, make_config
    B, cfg = 96, dict(F=23, V=2000, E=E, H=64, NL=2, NC=0, P=32, K=25)
    F, L = cfg["F"], int(cfg["F"] * 0.3)
    g = torch.Generator().manual_seed(12)
    cnt = (1.0 + 50.0 * torch.rand(cfg["V"], generator=g) ** 4).numpy().astype(np.float32)
    torch.manual_seed(12)
    model = BaseModel.from_config(make_config(cfg, mode, cnt if mode == "MFP" else None, backbone=backbone)).to(DEV)
    ai = pg.extras_of(backbone) or None
    masks, logits = hook_relu_pattern(model), {}
    for name, mod in model.named_modules():
        if isinstance(mod, MultiHeadSelfAttention):
            def attn_hook(m, i, o, name=name):
                masks[name] = (o.detach() > 0).cpu()
            mod.register_forward_hook(attn_hook)
    ids = torch.randint(10, cfg["V"], (B, F), generator=g)
    model.train()
    if mode == "MFP":
        mi = torch.stack([torch.randperm(F, generator=g)[:L] for _ in range(B)])
        noise = torch.randint(0, cfg["V"], (B, L, cfg["K"]), generator=g)
        masked, labels, _ = ops.dynamic_mask_mfp(ids.to(DEV), L, masked_index=mi.to(DEV))
        model.mfp_criterion.return_logits = True
        model.mfp_criterion.register_forward_hook(lambda m, i, o: logits.__setitem__("out", o[1].detach()))
        loss = model(input_ids=masked, labels=labels, masked_index=mi.to(DEV), noise_samples=noise.to(DEV))[0]
        batch = dict(ids=masked.cpu(), labels=labels.cpu(), masked_index=mi, noise=noise,
                     logq=R.nce_buffers(cnt)[0], dims=(F, cfg["P"], cfg["K"]))
    else:
        y = torch.randint(0, 2, (B,), generator=g)
        loss, out = model(input_ids=ids.to(DEV), labels=y.to(DEV))
        logits["out"] = out.detach()
        batch = dict(ids=ids, y=y)
    loss.backward()
    params = {n: p.detach().cpu().numpy() for n, p in model.named_parameters()}
    pre = {}
    BR.step(backbone, mode, params, batch, num_hidden=cfg["NL"], ai=ai, preacts=pre)
    flips = check_pattern(masks, pre, f"{backbone} {mode} E={E}", tol=2e-6)
    loss_ref, logits_ref, ref = BR.step(backbone, mode, params, batch, num_hidden=cfg["NL"], ai=ai, relu_masks=masks)
    np.testing.assert_allclose(float(loss.detach()), loss_ref, rtol=1e-5)
    np.testing.assert_allclose(logits["out"].cpu().numpy().ravel(), logits_ref.ravel(), rtol=1e-5, atol=1e-6)
    grads = all_grads(model)
    assert set(grads) == set(ref), (sorted(grads), sorted(ref))
    worst = max((BR.rel(grads[n].cpu().numpy(), ref[n]), n) for n in grads)
    print(f"[{backbone} {mode} B={B} F={F} E={E}] {flips} ReLU units on the other side of the kink; worst gradient error "
          f"vs fp64 / scale: hip {worst[0]:.2e} at {worst[1]}")
    for n, got in grads.items():
        np.testing.assert_allclose(got.cpu().numpy(), ref[n].reshape(got.shape), rtol=2e-5, atol=2e-6, err_msg=n)


# ----------------------------------------------------------------------------- other backbones (§8 f4)
@pytest.mark.parametrize("case,backbone", OTHER)
@pytest.mark.parametrize("mode", ["MFP", "RFD", "CTR"])
def test_other_backbones_golden(case, backbone, mode):
    """DNN / DeepFM through the same C-ABI kernels, heads and row tables vs golden vectors of the
    reference's own classes (models.py:164-233): loss, outputs and every gradient (for DeepFM
    including the LR weight rows, reduced together with the embedding rows)."""
    _other_backbone_case(case, backbone, mode)


def test_autoint_finetune_with_lr_term_and_dnn_tower_golden():
    """AutoInt's finetune-only options (use_lr, num_dnn_layers > 0; models.py:463-471, 482-486) against a fixture of the
    reference's own class: logits = attn_out(attention) + LR(ids) + dnn_out(dnn(embeddings)); the LR weight is the
    secondary parameter of the embedding's row table, so its gradient rows come out of the same reduction.  (The
    reference sizes the tower for the attention output and feeds it the embeddings: the fixture uses embed_size ==
    heads x attn_size, the only setting in which the reference itself runs; any other raises here as it fails there.)"""
    _other_backbone_case("B_f25_b64", "AutoIntFull", "CTR")
    from util import make_config
    from mapx.models import BaseModel
    cfg = dict(pg.CASES["B_f25_b64"])
    c = make_config(cfg, "CTR", None, backbone="AutoIntFull")
    c.attn_size = 12                                    # 2 heads x 12 != embed_size 16
    with pytest.raises(ValueError):
        BaseModel.from_config(c)


@pytest.mark.parametrize("mode", ["MFP", "RFD", "CTR"])
def test_xdeepfm_without_the_mlp_tower_golden(mode):
    """xDeepFM with num_hidden_layers = 0 (models.py:253-255: the CIN's output alone feeds the heads / `fc`) against
    fixtures of the reference's own class, all three step kinds."""
    _other_backbone_case("B_f25_b64", "xDeepFMCin", mode)


def _other_backbone_case(case, backbone, mode):
    from mapx import ops
    cfg, z, inp, params = load_case(case, mode, backbone)
    model = build_model(cfg, mode, params, inp["feat_count"] if mode == "MFP" else None, backbone=backbone)
    ids, mi = t(inp["input_ids"], DEV), t(inp["masked_index"], DEV)
    model.train()
    if mode == "MFP":
        masked, labels, _ = ops.dynamic_mask_mfp(ids, mi.shape[1], masked_index=mi)
        loss, count, acc = model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=t(inp["noise"], DEV))
        assert count == int(z["out/count"]) and int(acc) == int(z["out/total_acc"])
    elif mode == "RFD":
        replaced, labels, _ = ops.dynamic_mask_rfd(ids, mi.shape[1], masked_index=mi,
                                                   replace_feat=t(inp["replace_feat"], DEV))
        loss, count, acc, pos = model(input_ids=replaced, labels=labels)
        np.testing.assert_allclose(float(acc), float(z["out/acc"]), rtol=1e-6)
        np.testing.assert_allclose(float(pos), float(z["out/pos_ratio"]), rtol=1e-6)
    else:
        loss, logits = model(input_ids=ids, labels=t(inp["y"], DEV))
        np.testing.assert_allclose(logits.detach().cpu().numpy(), z["out/logits"], rtol=1e-5, atol=1e-5)
        if backbone == "DeepFM":
            x3, lr = model.embed.forward_with_linear(ids, model.lr_layer.embed_w.weight)
            np.testing.assert_allclose((lr.view(-1, 1) + model.lr_layer.bias).detach().cpu().numpy(), z["mid/lr"],
                                       rtol=1e-5, atol=1e-6)
            from mapx.layers import fm_product_sum
            # 0.5 * sum_e((sum_f x)^2 - sum_f x^2) cancels: absolute tolerance at the scale of its two terms
            np.testing.assert_allclose(fm_product_sum(x3).detach().cpu().numpy(), z["mid/fm"], rtol=1e-5, atol=5e-6)
        if backbone.startswith("AutoInt"):
            x = model.embed(ids)
            for li, layer in enumerate(model.self_attention):
                x = layer(x)
                np.testing.assert_allclose(x.detach().cpu().numpy(), z[f"mid/attn{li}"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(float(loss.detach()), float(z["out/loss"]), rtol=1e-5)
    loss.backward()
    _check_grads(z, model, tag=f"{backbone}/{mode}/{case}")      # no fallback for these: direct or fail


def test_embed_norm_and_dropout_options_vs_torch():
    """Options of the hot-path classes that the run scripts leave off (layers.py:92-95, 183): the
    embeddings' LayerNorm + dropout and the deep tower's dropout.  With dropout in eval mode the
    model equals the oracle + torch LayerNorm; in train mode the masks are consistent between forward
    and backward (finite-difference-free check: gradient of sum(out) w.r.t. a layer's input is zero
    exactly where the mask dropped the unit) and state_dict keys follow the reference's names."""
    from mapx.models import BaseModel
    from oracle import ref_model as R
    from util import make_config
    cfg = dict(F=5, V=300, E=16, H=24, NL=2, NC=2, P=32, K=5)
    c = make_config(cfg, "CTR", None)
    c.embed_norm, c.embed_dropout_rate, c.hidden_dropout_rate, c.layer_norm_eps = True, 0.25, 0.4, 1e-12
    torch.manual_seed(3)
    model = BaseModel.from_config(c).to(DEV)
    assert {"embed.layer_norm.weight", "embed.layer_norm.bias"} <= set(model.state_dict())
    assert not any("dropout" in k or ".dnn.2" in k for k in model.state_dict())
    with torch.no_grad():
        model.embed.layer_norm.weight.uniform_(0.5, 1.5)
        model.embed.layer_norm.bias.uniform_(-0.2, 0.2)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, cfg["V"], (64, cfg["F"]), generator=g)
    y = torch.randint(0, 2, (64,), generator=g)
    # eval: dropout is the identity; LayerNorm vs torch on the oracle's trunk
    model.eval()
    with torch.no_grad():
        (logits,) = model(input_ids=ids.to(DEV))
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x3 = torch.nn.functional.layer_norm(P["embed.embedding.weight"][ids], (cfg["E"],), P["embed.layer_norm.weight"],
                                        P["embed.layer_norm.bias"], 1e-12)
    x0 = x3.flatten(1)
    fin = torch.cat([R.cross(P, x0, cfg["NC"]), R.dnn(P, x0, cfg["NL"])], -1)
    ref = R.ctr_head(P, fin)[0]
    np.testing.assert_allclose(logits.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5)
    # train: two forward passes draw different masks; gradients flow only through kept units
    model.train()
    a = model(input_ids=ids.to(DEV), labels=y.to(DEV))[1].detach().clone()
    b = model(input_ids=ids.to(DEV), labels=y.to(DEV))[1].detach().clone()
    assert not torch.equal(a, b)
    x = model.embed(ids.to(DEV))
    kept = (x != 0)
    assert 0.6 < float(kept.float().mean()) < 0.9                     # p = 0.25
    loss = model(input_ids=ids.to(DEV), labels=y.to(DEV))[0]
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for n, p in model.named_parameters() if p.grad is not None)
    assert model.embed.layer_norm.weight.grad is not None and float(model.embed.layer_norm.weight.grad.abs().sum()) > 0


# --------------------------------------------------------------------------- hidden_act other than relu
ACT_KINDS = ["tanh", "sigmoid", "none", "elu", "leu", "gelu", "gelu_new", "swish", "mish"]


@pytest.mark.parametrize("kind", ACT_KINDS)
def test_hidden_act_kernels_and_mlp_vs_reference(golden_dir, kind):
    """`--hidden_act` other than relu (layers.py:55-80): the activation kernels and MLPBlock with them against outputs
    and gradients of the reference's own classes (tests/golden/activations.npz), incl. +-0, +-1e-6, +-20 and +-88."""
    import os
    from mapx import ops
    from mapx.layers import MLPBlock
    z = np.load(os.path.join(golden_dir, "activations.npz"))
    x = torch.from_numpy(z["x"]).to(DEV).view(4, -1).contiguous()
    y = ops.act_fwd(kind, x)
    dz = ops.act_bwd(kind, torch.ones_like(x), x)
    # (absolute floor 3e-7 of values of order 1: where 1 + erf(z / sqrt 2) or 1 - tanh^2 cancel — z < -4 — the
    # reference's own fp32 result has no more correct digits than that)
    np.testing.assert_allclose(y.cpu().numpy().reshape(-1), z[f"{kind}/y"], rtol=2e-6, atol=3e-7)
    np.testing.assert_allclose(dz.cpu().numpy().reshape(-1), z[f"{kind}/dy_dx"], rtol=1e-5, atol=1e-6)
    # a destination that is a column slice of a wider buffer, an upstream gradient that is one too
    wide = torch.full((4, x.shape[1] + 8), 7.0, device=DEV)
    ops.act_fwd(kind, x, out=wide[:, 4:4 + x.shape[1]])
    assert torch.equal(wide[:, 4:4 + x.shape[1]], y) and bool((wide[:, :4] == 7).all()) and bool((wide[:, -4:] == 7).all())
    gw = torch.randn(4, x.shape[1] + 8, device=DEV)
    assert torch.equal(ops.act_bwd(kind, gw[:, 2:2 + x.shape[1]], x), ops.act_bwd(kind, gw[:, 2:2 + x.shape[1]].contiguous(), x))
    mlp = MLPBlock(24, hidden_size=20, num_hidden_layers=2, hidden_act=kind, hidden_dropout_rate=0.0).to(DEV)
    with torch.no_grad():
        for n, p in mlp.named_parameters():
            p.copy_(torch.from_numpy(z[f"mlp/{kind}/p/{n}"]))
    xin = torch.from_numpy(z["mlp/x"]).to(DEV).requires_grad_(True)
    out = mlp(xin)
    (out * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), z[f"mlp/{kind}/y"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(xin.grad.cpu().numpy(), z[f"mlp/{kind}/dx"], rtol=1e-4, atol=1e-6)
    for n, p in mlp.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), z[f"mlp/{kind}/g/{n}"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kind", ["tanh", "gelu", "mish"])
def test_dcnv2_step_with_another_hidden_act_vs_oracle(kind):
    """DCNv2 + MFP with `hidden_act` != relu through the whole forward / backward (no fused ReLU links, the towers'
    plain join): loss, logits and every gradient against the oracle on the same injected masks and negatives."""
    import paramgen as pg
    from oracle import ref_model as R
    from util import load_case, make_config, t
    from mapx import ops
    from mapx.models import BaseModel
    case = "B_f25_b64"
    cfg, z, inp, params = load_case(case, "MFP")
    config = make_config(cfg, "MFP", inp["feat_count"])
    config.hidden_act = kind
    model = load_params(BaseModel.from_config(config), params).to(DEV)
    model.mfp_criterion.return_logits = True
    ids, mi = t(inp["input_ids"], DEV), t(inp["masked_index"], DEV)
    masked, labels, _ = ops.dynamic_mask_mfp(ids, mi.shape[1], masked_index=mi)
    model.train()
    loss, count, acc = model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=t(inp["noise"], DEV))
    loss.backward()
    P = {k: t(v).requires_grad_(True) for k, v in params.items()}
    logq, _, _ = R.nce_buffers(inp["feat_count"])
    m_ref, l_ref = R.dynamic_mask_mfp(t(inp["input_ids"]), t(inp["masked_index"]))
    fin = R.trunk(P, m_ref, cfg["NC"], cfg["NL"], hidden_act=kind)
    loss_ref, _, acc_ref = R.mfp_head(P, fin, l_ref, t(inp["masked_index"]), t(inp["noise"]), logq, cfg["F"], cfg["P"], cfg["K"])
    loss_ref.backward()
    np.testing.assert_allclose(float(loss.detach()), float(loss_ref), rtol=1e-5)
    assert int(acc) == acc_ref
    for name, p in model.named_parameters():
        if name in ("embed.embedding.weight", "mfp_criterion.emb.weight", "mfp_criterion.bias.weight"):
            continue
        g = p.grad if p.grad is not None else getattr(p, "_mapx_grad", None)
        ref = P[name].grad
        scale = float(ref.abs().max()) + 1e-12
        np.testing.assert_allclose(g.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-5 * scale, err_msg=name)
    g0, _ = model.embed.table.dense_grad()
    np.testing.assert_allclose(g0.cpu().numpy(), P["embed.embedding.weight"].grad.numpy(), rtol=1e-4, atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("K,relu", [(1001, False), (1001, True), (37, True)])
def test_linear_with_an_input_width_that_is_not_a_multiple_of_8(K, relu):
    """DeepFM's heads read cat([dnn, lr + fm]) — 1001 columns: layers._Linear pads both GEMM operands with zero
    columns to the next multiple of 8 (the vectorised operand path) and cuts the gradients back.  Forward, dX, dW
    and db against fp64, with and without the optimizer's gradient slot."""
    from mapx import layers
    torch.manual_seed(K)
    lin = layers.HipLinear(K, 64, relu=relu).to(DEV)
    x = torch.randn(512, K, device=DEV, requires_grad=True)
    r = torch.randn(512, 64, device=DEV)
    y = lin(x)
    (y * r).sum().backward()
    xd = x.detach().double().requires_grad_(True)
    wd, bd = lin.weight.detach().double().requires_grad_(True), lin.bias.detach().double().requires_grad_(True)
    yd = xd @ wd.T + bd
    yd = torch.relu(yd) if relu else yd
    (yd * r.double()).sum().backward()
    tol = lambda ref: 3e-6 * max(1.0, float(ref.detach().abs().max()))
    assert float((y.detach().double() - yd.detach()).abs().max()) <= tol(yd)
    assert x.grad.shape == (512, K) and float((x.grad.double() - xd.grad).abs().max()) <= tol(xd.grad)
    assert float((lin.weight.grad.double() - wd.grad).abs().max()) <= tol(wd.grad)
    assert float((lin.bias.grad.double() - bd.grad).abs().max()) <= tol(bd.grad)
    # the optimizer-owned slot: the padded dW is copied into it, autograd gets None
    slot = torch.zeros_like(lin.weight)
    lin.weight._mapx_grad = slot
    lin.weight.grad = None
    (lin(x.detach()) * r).sum().backward()
    assert lin.weight.grad is None
    from mapx import ops
    ops.flush_deferred()
    assert float((slot.double() - wd.grad).abs().max()) <= tol(wd.grad)
