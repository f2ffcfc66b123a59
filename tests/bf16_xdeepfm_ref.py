"""float64 torch restatement of the xDeepFM step (reference models.py:235-279, layers.py:696-721) for the bf16 compute
mode's tests.  The heads come from oracle.ref_model, the rounding sites, the MLP and the head helpers from
tests/bf16_backbones_ref.py; with emulation off the CIN is oracle.ref_model.cin to the last bit of float64.

The same two switches as bf16_backbones_ref.step:
  relu_masks / preacts   impose / collect the ReLU pattern: "dnn.dnn.0", ... and "pred_rfd.0";
  emulate=True           round to bf16 (nearest even) where the kernels store bf16: the gathered rows (and
                         x0t, the same values transposed), every CIN layer's Y, the pooled [B, sum(units)] vector, the
                         MLP activations, and the gradients crossing the same boundaries.  The Hadamard operand
                         a = bf16(x0 * xi) is rounded in value only (it is never stored: no gradient rounding), weight
                         operands in forward only.  A layer's Y feeds the pooling and the next layer: autograd adds the
                         two gradients before the site rounds them, one rounding of the sum as in the dX kernel.  The
                         gathered rows feed the CIN and the MLP through one gradient-rounding site each, as each of the
                         two backward chains stores its own bf16 dx3 before autograd adds them.  The LR term, the bias
                         adds, the pooling sums, dW / db and every logit stay unrounded."""
import numpy as np
import torch

from bf16_backbones_ref import F64, _Em, _Round, _dnn, _head_linear, _mfp, fixture_batch, rel  # noqa: F401
from oracle import ref_model as R


def units_of(extra):
    return [int(c) for c in str(extra["cin_layer_units"]).split(",")]


def cin(P, x3, units, em):
    """R.cin with the rounding sites.  x3 [B,F,E] -> pooled [B, sum(units)]."""
    if not em.on:
        return R.cin(P, x3, units)
    B, F, E = x3.shape
    xi, pooled = x3, []
    for i, u in enumerate(units):
        a = _Round.apply(torch.einsum("bhd,bmd->bhmd", x3, xi).reshape(B, -1, E), True, False)     # value only
        w = em.weight(P[f"cin.cin_layer.layer_{i + 1}.weight"])[:, :, 0]
        xi = em.act(torch.einsum("ok,bkd->bod", w, a) + P[f"cin.cin_layer.layer_{i + 1}.bias"].view(1, -1, 1))
        pooled.append(em.act(xi.sum(-1)))
    return torch.cat(pooled, dim=-1)


def step(mode, params, batch, units, num_hidden=0, relu_masks=None, preacts=None, emulate=False):
    """One forward + backward.  mode: MFP | RFD | CTR; params: name -> array (the LR term is on when its weight is
    among them); batch: as bf16_backbones_ref.step's.  -> (loss float, logits float64 array, {name: gradient})."""
    em = _Em(emulate)
    P = {k: torch.as_tensor(np.asarray(v)).to(F64).clone().requires_grad_(True) for k, v in params.items()}
    ids = batch["ids"]
    x3 = em.act(P["embed.embedding.weight"][ids])                  # the gathered rows
    kw = dict(relu_masks=relu_masks, preacts=preacts)
    final = cin(P, em.grad(x3), units, em)
    if num_hidden > 0:
        final = torch.cat([final, _dnn(P, em.grad(x3).flatten(1), num_hidden, "dnn", em, **kw)], dim=1)
    if mode == "MFP":
        F_, Pj, K = batch["dims"]
        Ph = dict(P)
        Ph["feat_encoder.weight"] = em.weight(P["feat_encoder.weight"])
        loss, logits, _ = _mfp(Ph, final, batch, em, F_, Pj, K)
    elif mode == "RFD":
        z = em.act(R._relu(final @ em.weight(P["pred_rfd.0.weight"]).t() + P["pred_rfd.0.bias"], "pred_rfd.0",
                           relu_masks, preacts))
        logits = _head_linear(P, z, "pred_rfd.2", em)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, batch["labels"].to(F64))
    else:
        logits = _head_linear(P, final, "fc", em)
        if "lr_layer.embed_w.weight" in P:
            logits = logits + R.lr_logit(P, ids)                   # fp32 term, added to the fp32 logit
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), batch["y"].to(F64))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return float(loss.detach()), logits.detach().numpy(), grads
