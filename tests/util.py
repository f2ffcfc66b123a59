"""Helpers shared by the parity tests: golden loading and digest comparison."""
import os

import numpy as np
import torch

import paramgen as pg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("MFP", "RFD", "CTR")


def load_case(case, mode, backbone="DCNv2"):
    cfg = pg.CASES[case]
    suffix = "" if backbone == "DCNv2" else f"_{backbone}"
    z = np.load(os.path.join(GOLD, f"{case}_{mode}{suffix}.npz"))
    inp = pg.make_inputs(case, cfg)
    params = pg.make_params(case, cfg, mode, backbone)
    return cfg, z, inp, params


def t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def assert_digest(z, prefix, name, got, rtol=2e-5, atol=1e-6):
    """Compare `got` with what the fixture kept of tensor `name` (see paramgen.digest)."""
    got = np.asarray(got, dtype=np.float32)
    want = {k.split("/")[-1]: z[k] for k in z.files if k.startswith(f"{prefix}/{name}/")}
    assert want, f"no golden entry for {prefix}/{name}"
    mine = pg.digest(name, got)
    assert set(mine) == set(want), (name, set(mine), set(want))
    for k, w in want.items():
        g = np.asarray(mine[k], dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        scale = max(1.0, float(np.abs(w).max())) if k.startswith("proj") or k == "full" else 1.0
        if k in ("proj_r", "proj_l", "sum"):
            # linear functionals of ~N(0, s) entries: tolerance relative to the abs-sum scale
            scale = max(scale, float(np.asarray(want.get("abssum", 1.0))) * 1e-3)
        np.testing.assert_allclose(g, w, rtol=rtol, atol=atol * scale,
                                   err_msg=f"{prefix}/{name}/{k}")


def make_config(cfg, mode, feat_count=None, data_dir=None, seed=42, backbone="DCNv2", compute_dtype="fp32"):
    """mapx Config for a fixture case (the 11 runtime keys of reference run.py:50-61 + flags)."""
    from mapx.arguments import Config
    extra = pg.extras_of(backbone)
    nl = extra.pop("num_hidden_layers", cfg["NL"])          # (a fixture variant may override the case's tower depth)
    return Config(**extra, compute_dtype=compute_dtype, model_name=pg.model_name_of(backbone), data_dir=data_dir, input_size=cfg["V"], num_fields=cfg["F"],
                  embed_size=cfg["E"], embed_dropout_rate=0.0, embed_norm=False, layer_norm_eps=1e-12,
                  hidden_size=cfg["H"], num_hidden_layers=nl, hidden_act="relu",
                  hidden_dropout_rate=0.0, num_cross_layers=cfg["NC"], pt_neg_num=cfg["K"],
                  proj_size=cfg["P"], pretrain=(mode != "CTR"),
                  pt_type=("RFD" if mode == "RFD" else "MFP"), RFD_replace="Unigram",
                  feat_count=None if feat_count is None else torch.as_tensor(feat_count),
                  device=None, n_gpu=1, idx_low=None, idx_high=None, feat_num_per_field=None, seed=seed)


def build_model(cfg, mode, params, feat_count, device="cuda", backbone="DCNv2", compute_dtype="fp32"):
    """The backbone with the fixture's reproducible parameters loaded."""
    from mapx.models import BaseModel
    from model_harness import load_params
    model = BaseModel.from_config(make_config(cfg, mode, feat_count, backbone=backbone, compute_dtype=compute_dtype))
    return load_params(model, params).to(device)


# ----------------------------------------------------------------------------- ReLU pattern of a step
def hook_relu_pattern(model):
    """-> dict filled by forward hooks: layer name -> (output > 0) of every fused-ReLU layer."""
    masks = {}
    for name, mod in model.named_modules():
        if getattr(mod, "relu", False):
            mod.register_forward_hook(lambda m, i, o, name=name: masks.__setitem__(name, (o.detach() > 0).cpu()))
    return masks


def check_pattern(masks, preacts, what, tol=2e-2):
    """The step under test may put a unit on the other side of the ReLU's kink only where the oracle's
    pre-activation is zero to the step's rounding (|z| <= tol of the layer's scale: 2e-2 for bf16
    activations, 2e-6 for fp32); -> number of such units."""
    assert set(masks) == set(preacts), (sorted(masks), sorted(preacts))
    flips = 0
    for k, z in preacts.items():
        differ = masks[k] != (z > 0)
        flips += int(differ.sum())
        if differ.any():
            worst = float(z[differ].abs().max()) / float(z.abs().max())
            assert worst <= tol, f"{what}: {k}: a unit with pre-activation {worst:.3e} of the layer's scale flipped"
    return flips


def oracle_case_grads(mode, cfg, params, inp, relu_masks=None, preacts=None):
    """fp32 oracle (the reference's CPU arithmetic) on a fixture case: loss, outputs, gradients.
    `relu_masks`: impose the activation pattern of the step under test (see oracle/ref_model._relu)."""
    from oracle import ref_model as R
    P = {k: t(v).clone().requires_grad_(True) for k, v in params.items()}
    ids, mi = t(inp["input_ids"]), t(inp["masked_index"])
    kw = dict(relu_masks=relu_masks, preacts=preacts)
    if mode == "MFP":
        logq = R.nce_buffers(inp["feat_count"])[0]
        masked, labels = R.dynamic_mask_mfp(ids, mi)
        loss, out, _ = R.mfp_head(P, R.trunk(P, masked, cfg["NC"], cfg["NL"], **kw), labels, mi, t(inp["noise"]), logq,
                                  cfg["F"], cfg["P"], cfg["K"])
    elif mode == "RFD":
        rep, labels = R.dynamic_mask_rfd(ids, mi, t(inp["replace_feat"]))
        loss, _, _, _, out = R.rfd_head(P, R.trunk(P, rep, cfg["NC"], cfg["NL"], **kw), labels, **kw)
    else:
        loss, out = R.ctr_head(P, R.trunk(P, ids, cfg["NC"], cfg["NL"], **kw), t(inp["y"]))
    loss.backward()
    return float(loss), out.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


# ----------------------------------------------------------------------------- what a golden check compared
# tests/test_model_gpu.py::_check_grads compares every gradient with the fixture of the real reference and, when
# that fails because a hidden unit sits on the ReLU's kink, with the oracle re-run on the step's own pattern.
# Which of the two happened is recorded here per test case, printed in the terminal summary (conftest.py) and
# checked against tests/golden/pattern_fallback_allowed.json: a case that passes directly today may not start
# to need the fallback unnoticed.
GOLDEN_LOG = []


def note_golden(tag, how, flips=0):
    GOLDEN_LOG.append((tag, how, int(flips)))


def fallback_allowed(tag):
    import json
    import os
    if os.environ.get("MAPX_GOLDEN_ALLOW_ALL") == "1":
        return True
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pattern_fallback_allowed.json")
    with open(path) as f:
        return tag in json.load(f)["allowed"]
