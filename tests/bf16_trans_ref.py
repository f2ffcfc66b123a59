"""float64 torch restatement of the Transformer trunk and its heads (reference models.py:491-568:
nn.TransformerEncoderLayer post-norm / pre-norm, relu / gelu, the four finetune reductions, the LR term and the MLP
tower) for the bf16 compute mode's tests.  The heads, the MLP tower, the rounding sites and the fixture batch come from
oracle.ref_model and bf16_backbones_ref; the attention core is tests/test_mha_gpu.restate.

Two switches, as in bf16_backbones_ref:
  relu_masks / preacts   impose / collect the ReLU pattern, one key per fused-ReLU module of the model:
                         "encoder.layers.<i>.linear1" (relu variants), "field_reduction_attn.0", "pred_rfd.0",
                         "mlp.dnn.<3i>";
  emulate=True           round to bf16 at exactly the tensor stores of DESIGN §4.6 / §4.8.  Value and gradient: the
                         gathered rows; qkv, O, and the outputs of out_proj, linear1 (+relu), gelu and linear2 (the saved
                         gelu pre-activation is linear1's bf16 output); the LayerNorm output; the pre-norm residual
                         sums; the pooled vectors; the heads' stores.  Gradient only: dsum of the add + LayerNorm kernel
                         (its forward sum is never stored) and every fp32 logit or score that enters the trunk.  Weight
                         operands forward only.  P and the pooling weights are never rounded."""
import math

import numpy as np
import torch

import bf16_backbones_ref as BR
from bf16_backbones_ref import F64, _Em, _dnn, _head_linear, _mfp, fixture_batch, rel  # noqa: F401  (re-exported)
from oracle import ref_model as R
from test_mha_gpu import restate


def _layernorm(s, w, b, eps):
    mean = s.mean(dim=-1, keepdim=True)
    var = ((s - mean) ** 2).mean(dim=-1, keepdim=True)              # biased, as nn.LayerNorm
    return (s - mean) / torch.sqrt(var + eps) * w + b


def encoder_layer(P, x, i, B, F, T, eps, em, relu_masks, preacts):
    """One encoder layer on x [B*F, E] (a bf16 tensor under emulation)."""
    pre = f"encoder.layers.{i}."
    E, H = x.shape[1], T["num_attn_heads"]

    def lin(h, name):
        return h @ em.weight(P[pre + name + ".weight"]).t() + P[pre + name + ".bias"]

    def sa(h):
        qkv = em.act(h @ em.weight(P[pre + "self_attn.in_proj_weight"]).t() + P[pre + "self_attn.in_proj_bias"])
        o, _ = restate(qkv, B, F, E, H)                               # P stays unrounded
        return em.act(lin(em.act(o), "self_attn.out_proj"))

    def ff(h):
        z = lin(h, "linear1")
        if T["hidden_act"] == "relu":
            a = em.act(R._relu(z, pre + "linear1", relu_masks, preacts))
        else:
            a = em.act(R.act(T["hidden_act"], em.act(z)))
        return em.act(lin(a, "linear2"))

    def norm(s, name):          # s: the fp32 sum (post-norm) or the bf16 input (pre-norm); dsum leaves in bf16
        return em.act(_layernorm(em.grad(s), P[pre + name + ".weight"], P[pre + name + ".bias"], eps))

    if T["norm_first"]:
        x = em.act(x + sa(norm(x, "norm1")))
        return em.act(x + ff(norm(x, "norm2")))
    x = norm(x + sa(x), "norm1")
    return norm(x + ff(x), "norm2")


def step(mode, params, batch, T, eps, relu_masks=None, preacts=None, emulate=False):
    """One forward + backward.  mode: MFP | RFD | CTR; params: name -> array; batch: bf16_backbones_ref.fixture_batch;
    T: the variant's keys (trans_params.VARIANTS); eps: layer_norm_eps.
    -> (loss float, logits float64 array, {name: gradient float64 array})."""
    em = _Em(emulate)
    P = {k: torch.as_tensor(np.asarray(v)).to(F64).clone().requires_grad_(True) for k, v in params.items()}
    ids = batch["ids"]
    kw = dict(relu_masks=relu_masks, preacts=preacts)
    x3 = em.act(P["embed.embedding.weight"][ids])                  # the gathered rows
    B, F, E = x3.shape
    x = x3.reshape(B * F, E)
    for i in range(T["num_hidden_layers"]):
        x = encoder_layer(P, x, i, B, F, T, eps, em, **kw)
    final = x.view(B, F * E)
    if mode == "MFP":
        F_, Pj, K = batch["dims"]
        Ph = dict(P)
        Ph["feat_encoder.weight"] = em.weight(P["feat_encoder.weight"])
        loss, logits, _ = _mfp(Ph, final, batch, em, F_, Pj, K)
    elif mode == "RFD":
        z = em.act(R._relu(final @ em.weight(P["pred_rfd.0.weight"]).t() + P["pred_rfd.0.bias"], "pred_rfd.0", **kw))
        logits = _head_linear(P, z, "pred_rfd.2", em)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, batch["labels"].to(F64))
    else:
        red = T["output_reduction"]
        enc3 = x.view(B, F, E)
        if red == "fc":
            pooled = final
        elif red == "attn,fc":
            h = em.act(R._relu(x @ em.weight(P["field_reduction_attn.0.weight"]).t() + P["field_reduction_attn.0.bias"],
                               "field_reduction_attn.0", **kw))
            scores = _head_linear(P, h, "field_reduction_attn.2", em).view(B, F)      # fp32 scores
            w = torch.softmax(scores, dim=1)                                          # fp32 weights, never rounded
            pooled = em.act((enc3 * w.unsqueeze(-1)).sum(1))
        elif red == "mean,fc":
            pooled = em.act(enc3.sum(1) / F)
        elif red == "sum,fc":
            pooled = em.act(enc3.sum(1))
        else:
            raise NotImplementedError(red)
        logits = _head_linear(P, pooled, "trans_out", em)
        if T["use_lr"]:
            logits = logits + R.lr_logit(P, ids)
        if T["num_dnn_layers"]:
            logits = logits + _head_linear(P, _dnn(P, x3.flatten(1), T["num_dnn_layers"], "mlp", em, **kw), "mlp_out", em)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), batch["y"].to(F64))
    assert math.isfinite(float(loss.detach()))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return float(loss.detach()), logits.detach().numpy(), grads
