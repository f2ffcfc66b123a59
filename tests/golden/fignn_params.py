"""Fixture settings and reproducible parameters of the FiGNN backbone (reference models.py:410-438,
layers.py:300-379).

Pure numpy like paramgen.py, whose inputs, parameter draws and digests it reuses: the fixture generator
(gen_fignn_golden.py, which runs the real reference on the CPU) and the tests rebuild bit-identical parameters from
a variant's name, so the fixtures only hold outputs.  Every parameter is drawn non-trivially, `bias_p` (zero at
initialisation) included.
"""
import numpy as np

import paramgen as pg

CASE = "B_f25_b64"
FIGNN = dict(res_conn=False, reuse_graph_layer=False, num_hidden_layers=3)
# the residual to the embeddings after every step, ONE GraphLayer for both steps
FIGNN_SHARE = dict(res_conn=True, reuse_graph_layer=True, num_hidden_layers=2)
VARIANTS = {"FiGNN": FIGNN, "FiGNNShare": FIGNN_SHARE}
CTR_ONLY = ("FiGNNShare",)
MID_ROWS = 2            # samples of which the graph and the trunk's output are kept
SALT = ""               # appended to the parameter seed if an off-diagonal `pre` of the graph falls within 1e-6 of zero
PRE_MARGIN = 1e-6


def modes_of(variant):
    return ("CTR",) if variant in CTR_ONLY else ("MFP", "RFD", "CTR")


def extras_of(variant):
    """Config keys of the variant (on top of the case's, as paramgen.extras_of)."""
    return dict(VARIANTS[variant])


def layer_prefixes(variant):
    T = VARIANTS[variant]
    return ["fignn.gnn."] if T["reuse_graph_layer"] else [f"fignn.gnn.{l}." for l in range(T["num_hidden_layers"])]


def param_shapes(cfg, mode, variant):
    """state_dict key of every trainable parameter -> (shape, scale of the draw)."""
    F, V, E, P = cfg["F"], cfg["V"], cfg["E"], cfg["P"]
    out = {"embed.embedding.weight": ((V, E), 0.3)}
    for pre in layer_prefixes(variant):
        out[pre + "W_in"] = ((F, E, E), (2.0 / (E * E + F * E)) ** 0.5 * 4)
        out[pre + "W_out"] = ((F, E, E), (2.0 / (E * E + F * E)) ** 0.5 * 4)
        out[pre + "bias_p"] = ((E,), 0.1)
    for k, shp in (("weight_ih", (3 * E, E)), ("weight_hh", (3 * E, E)), ("bias_ih", (3 * E,)), ("bias_hh", (3 * E,))):
        out["fignn.gru." + k] = (shp, E ** -0.5)
    out["fignn.W_attn.weight"] = ((1, 2 * E), 1.0)
    D = F * E
    if mode == "MFP":
        out["feat_encoder.weight"] = ((F * P, D), D ** -0.5)
        out["feat_encoder.bias"] = ((F * P,), 0.1)
        out["mfp_criterion.emb.weight"] = ((V, P), P ** -0.5)
        out["mfp_criterion.bias.weight"] = ((V, 1), 0.5)
    elif mode == "RFD":
        out["pred_rfd.0.weight"] = ((F * P, D), D ** -0.5)
        out["pred_rfd.0.bias"] = ((F * P,), 0.1)
        out["pred_rfd.2.weight"] = ((F, F * P), (F * P) ** -0.5)
        out["pred_rfd.2.bias"] = ((F,), 0.1)
    else:
        out["fc.linear1.weight"] = ((1, E), E ** -0.5)
        out["fc.linear2.0.weight"] = ((F, D), D ** -0.5)
    return out


def make_params(cfg, mode, variant, case=CASE):
    return {k: pg.make_param(case, f"{variant}{SALT}/{k}", shp, sc)
            for k, (shp, sc) in param_shapes(cfg, mode, variant).items()}


def smallest_pre(x, w_attn):
    """min |pre| over the off-diagonal pairs, in float64: x [B,F,E] embeddings, w_attn [1,2E]."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w_attn, dtype=np.float64).reshape(-1)
    E = x.shape[-1]
    pre = (x @ w[:E])[:, :, None] + (x @ w[E:])[:, None, :]
    off = ~np.eye(x.shape[1], dtype=bool)
    return float(np.abs(pre[:, off]).min())


def make_config(cfg, mode, variant, feat_count=None, **over):
    """mapx Config of a variant (tests only: util.make_config plus the variant's keys, model_name "fignn")."""
    from util import make_config as base
    c = base(cfg, mode, feat_count, backbone="fignn")
    for k, v in dict(extras_of(variant), **over).items():
        setattr(c, k, v)
    return c


def build_model(cfg, mode, variant, params, feat_count=None, device="cuda"):
    """The FiGNN model of a variant with the fixture's parameters loaded (tests only)."""
    import torch
    from mapx.models import build_backbone
    model = build_backbone(make_config(cfg, mode, variant, feat_count))
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    return model.to(device)
