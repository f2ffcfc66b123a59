"""Fixture settings and reproducible parameters of the FGCNN backbone (reference models.py:325-407,
layers.py:204-251).

Pure numpy like paramgen.py, whose inputs, parameter draws and digests it reuses: the fixture generator
(gen_fgcnn_golden.py, which runs the real reference on the CPU) and the tests rebuild bit-identical parameters from
a variant's name, so the fixtures only hold outputs.
"""
import math

import numpy as np

import paramgen as pg

CASE = "B_f25_b64"
# F = 25 fields: stage heights 25 -> 13 -> 7, so the pooling pads one row at both stages
FGCNN = dict(share_embedding=False, channels="3,4", kernel_heights="3,5", pooling_sizes="2,2",
             recombined_channels="2,1", conv_act="tanh", hidden_act="relu", hidden_dropout_rate=0.0)
# one table feeding both consumers, relu in the kernels and in the recombine layers, fc_out straight on the features
FGCNN_SHARE = dict(FGCNN, share_embedding=True, conv_act="relu", num_hidden_layers=0)
VARIANTS = {"FGCNN": FGCNN, "FGCNNShare": FGCNN_SHARE}
CTR_ONLY = ("FGCNNShare",)
MID_ROWS = 8            # samples of which `combined` is kept
EVAL_ROWS = 2           # ... of the eval-mode `combined`


def modes_of(variant):
    return ("CTR",) if variant in CTR_ONLY else ("MFP", "RFD", "CTR")


def extras_of(variant):
    """Config keys of the variant (on top of the case's, as paramgen.extras_of)."""
    return dict(VARIANTS[variant])


def _lists(variant):
    T = VARIANTS[variant]
    return [[int(c) for c in T[k].split(",")] for k in ("channels", "kernel_heights", "pooling_sizes",
                                                        "recombined_channels")]


def stages(cfg, variant):
    """[(Cin, Cout, kh, ps, R, H_in, H_out)] of the variant's stages."""
    out, c_in, h = [], 1, cfg["F"]
    for c, kh, ps, r in zip(*_lists(variant)):
        h_out = int(math.ceil(h / ps))
        out.append((c_in, c, kh, ps, r, h, h_out))
        c_in, h = c, h_out
    return out


def total_features(cfg, variant):
    return cfg["F"] + sum(r * h_out for _, _, _, _, r, _, h_out in stages(cfg, variant))


def final_dim(cfg, variant):
    T = total_features(cfg, variant)
    return T * (T - 1) // 2 + T * cfg["E"]


def num_hidden_layers(cfg, variant):
    return VARIANTS[variant].get("num_hidden_layers", cfg["NL"])


def param_shapes(cfg, mode, variant):
    """state_dict key of every trainable parameter -> (shape, init scale); batch-norm weights are drawn around 1."""
    F, V, E, P, H = cfg["F"], cfg["V"], cfg["E"], cfg["P"], cfg["H"]
    out = {"embed.embedding.weight": ((V, E), (2.0 / (F + E)) ** 0.5)}
    if not VARIANTS[variant]["share_embedding"]:
        out["fg_embed.embedding.weight"] = ((V, E), (2.0 / (F + E)) ** 0.5)
    for i, (c_in, c, kh, ps, r, h, h_out) in enumerate(stages(cfg, variant)):
        pre = f"fgcnn_layer.conv_layers.{i}."
        out[pre + "0.weight"] = ((c, c_in, kh, 1), (c_in * kh) ** -0.5)
        out[pre + "0.bias"] = ((c,), 0.1)
        out[pre + "1.weight"] = ((c,), 0.1)
        out[pre + "1.bias"] = ((c,), 0.1)
        d_in, d_out = h_out * E * c, h_out * E * r
        out[f"fgcnn_layer.recombine_layers.{i}.0.weight"] = ((d_out, d_in), d_in ** -0.5)
        out[f"fgcnn_layer.recombine_layers.{i}.0.bias"] = ((d_out,), 0.1)
    D = final_dim(cfg, variant)
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
    d_in = D
    for i in range(num_hidden_layers(cfg, variant)):
        out[f"dnn.dnn.{3 * i}.weight"] = ((H, d_in), d_in ** -0.5)
        out[f"dnn.dnn.{3 * i}.bias"] = ((H,), 0.1)
        d_in = H
    out["fc_out.weight"] = ((1, d_in), d_in ** -0.5)
    out["fc_out.bias"] = ((1,), 0.1)
    return out


def make_params(cfg, mode, variant, case=CASE):
    out = {}
    for k, (shp, sc) in param_shapes(cfg, mode, variant).items():
        v = pg.make_param(case, f"{variant}/{k}", shp, sc)
        bn_weight = ".conv_layers." in k and k.endswith(".1.weight")
        out[k] = (v + np.float32(1.0)).astype(np.float32) if bn_weight else v
    return out


def eval_buffers(cfg, variant, case=CASE):
    """Running statistics the eval-mode fixture is computed with: means around 0, variances in [0.5, 1.5)."""
    out = {}
    for i, (_, c, *_rest) in enumerate(stages(cfg, variant)):
        pre = f"fgcnn_layer.conv_layers.{i}.1."
        out[pre + "running_mean"] = pg.make_param(case, f"{variant}/{pre}running_mean", (c,), 0.2)
        u = pg.make_param(case, f"{variant}/{pre}running_var", (c,), 1.0)
        out[pre + "running_var"] = (np.float32(0.5) + np.abs(np.tanh(u))).astype(np.float32)
    return out


def bn_buffer_names(cfg, variant):
    return [f"fgcnn_layer.conv_layers.{i}.1.{n}" for i in range(len(stages(cfg, variant)))
            for n in ("running_mean", "running_var", "num_batches_tracked")]


def make_config(cfg, mode, variant, feat_count=None, **over):
    """mapx Config of a variant (tests only: util.make_config plus the variant's keys, model_name "fgcnn")."""
    from util import make_config as base
    c = base(cfg, mode, feat_count, backbone="fgcnn")
    for k, v in dict(extras_of(variant), **over).items():
        setattr(c, k, v)
    return c


def build_model(cfg, mode, variant, params, feat_count=None, device="cuda"):
    """The FGCNN model of a variant with the fixture's parameters loaded (tests only)."""
    import torch
    from mapx.models import BaseModel
    model = BaseModel.from_config(make_config(cfg, mode, variant, feat_count))
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    return model.to(device)
