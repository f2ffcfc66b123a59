"""Fixture settings and reproducible parameters of the Transformer backbone (reference models.py:491-568).

Pure numpy like paramgen.py, whose inputs, parameter draws and digests it reuses: the fixture generator
(gen_trans_golden.py, which runs the real reference on the CPU) and the tests rebuild bit-identical parameters from
a variant's name, so the fixtures only hold outputs.
"""
import numpy as np

import paramgen as pg

CASE = "B_f25_b64"
# post-norm, 2 heads, relu; CTR reduces the fields with attention weights
TRANS = dict(hidden_size=16, num_hidden_layers=2, num_attn_heads=2, intermediate_size=48, hidden_act="relu",
             hidden_dropout_rate=0.0, norm_first=False, layer_norm_eps=1e-12, output_reduction="attn,fc",
             use_lr=False, num_dnn_layers=0, dnn_size=1000, dnn_act="relu", dnn_drop=0.0)
# pre-norm, gelu, 4 heads; CTR: mean over fields + the LR term + a 2-layer MLP tower over the embeddings
TRANS_PRE = dict(TRANS, num_attn_heads=4, hidden_act="gelu", norm_first=True, output_reduction="mean,fc",
                 use_lr=True, num_dnn_layers=2, dnn_size=40)
VARIANTS = {"Trans": TRANS, "TransPre": TRANS_PRE,
            "TransFc": dict(TRANS, output_reduction="fc"), "TransSum": dict(TRANS, output_reduction="sum,fc")}
CTR_ONLY = ("TransFc", "TransSum")


def modes_of(variant):
    return ("CTR",) if variant in CTR_ONLY else ("MFP", "RFD", "CTR")


def extras_of(variant):
    """Config keys of the variant (on top of the case's, as paramgen.extras_of)."""
    return dict(VARIANTS[variant])


def param_shapes(cfg, mode, variant):
    """state_dict key of every trainable parameter -> (shape, init scale); LayerNorm weights are drawn around 1."""
    T = VARIANTS[variant]
    F, V, E, P = cfg["F"], cfg["V"], cfg["E"], cfg["P"]
    assert E == T["hidden_size"]
    I = T["intermediate_size"]
    out = {"embed.embedding.weight": ((V, E), (2.0 / (F + E)) ** 0.5)}
    for i in range(T["num_hidden_layers"]):
        pre = f"encoder.layers.{i}."
        out[pre + "self_attn.in_proj_weight"] = ((3 * E, E), E ** -0.5)
        out[pre + "self_attn.in_proj_bias"] = ((3 * E,), 0.1)
        out[pre + "self_attn.out_proj.weight"] = ((E, E), E ** -0.5)
        out[pre + "self_attn.out_proj.bias"] = ((E,), 0.1)
        out[pre + "linear1.weight"] = ((I, E), E ** -0.5)
        out[pre + "linear1.bias"] = ((I,), 0.1)
        out[pre + "linear2.weight"] = ((E, I), I ** -0.5)
        out[pre + "linear2.bias"] = ((E,), 0.1)
        for n in ("norm1", "norm2"):
            out[pre + n + ".weight"] = ((E,), 0.1)
            out[pre + n + ".bias"] = ((E,), 0.1)
    D = F * E
    if mode == "MFP":
        out["feat_encoder.weight"] = ((F * P, D), D ** -0.5)
        out["feat_encoder.bias"] = ((F * P,), 0.1)
        out["mfp_criterion.emb.weight"] = ((V, P), P ** -0.5)
        out["mfp_criterion.bias.weight"] = ((V, 1), 0.5)
        return out
    if mode == "RFD":
        out["pred_rfd.0.weight"] = ((F * P, D), D ** -0.5)
        out["pred_rfd.0.bias"] = ((F * P,), 0.1)
        out["pred_rfd.2.weight"] = ((F, F * P), (F * P) ** -0.5)
        out["pred_rfd.2.bias"] = ((F,), 0.1)
        return out
    red = T["output_reduction"]
    if red == "attn,fc":
        out["field_reduction_attn.0.weight"] = ((E, E), E ** -0.5)
        out["field_reduction_attn.0.bias"] = ((E,), 0.1)
        out["field_reduction_attn.2.weight"] = ((1, E), E ** -0.5)
        out["field_reduction_attn.2.bias"] = ((1,), 0.1)
    d_out = D if red == "fc" else E
    out["trans_out.weight"] = ((1, d_out), d_out ** -0.5)
    out["trans_out.bias"] = ((1,), 0.1)
    if T["use_lr"]:
        out["lr_layer.embed_w.weight"] = ((V, 1), 0.3)
        out["lr_layer.bias"] = ((1,), 0.1)
    d_in, Hd = D, T["dnn_size"]
    for i in range(T["num_dnn_layers"]):
        out[f"mlp.dnn.{3 * i}.weight"] = ((Hd, d_in), d_in ** -0.5)
        out[f"mlp.dnn.{3 * i}.bias"] = ((Hd,), 0.1)
        d_in = Hd
    if T["num_dnn_layers"]:
        out["mlp_out.weight"] = ((1, Hd), Hd ** -0.5)
        out["mlp_out.bias"] = ((1,), 0.1)
    return out


def make_params(cfg, mode, variant, case=CASE):
    out = {}
    for k, (shp, sc) in param_shapes(cfg, mode, variant).items():
        v = pg.make_param(case, f"{variant}/{k}", shp, sc)
        out[k] = (v + np.float32(1.0)).astype(np.float32) if k.endswith(("norm1.weight", "norm2.weight")) else v
    return out


def make_config(cfg, mode, variant, feat_count=None, **over):
    """mapx Config of a variant (tests only: util.make_config plus the variant's keys, model_name "trans")."""
    from util import make_config as base
    c = base(cfg, mode, feat_count, backbone="trans")
    for k, v in dict(extras_of(variant), **over).items():
        setattr(c, k, v)
    return c


def build_model(cfg, mode, variant, params, feat_count=None, device="cuda"):
    """The Transformer model of a variant with the fixture's parameters loaded (tests only)."""
    import torch
    from mapx.models import BaseModel
    model = BaseModel.from_config(make_config(cfg, mode, variant, feat_count))
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    return model.to(device)
