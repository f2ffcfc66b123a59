"""float64 torch restatement of the DeepFM and AutoInt trunks and their heads (reference models.py:196-233, 440-488;
layers.py:848-914) for the bf16 compute mode's tests.  The pieces come from oracle.ref_model (dnn, lr_logit,
fm_product_sum, mfp_head, rfd_head, dynamic_mask_*); the AutoInt layer is restated here so that its ReLU goes through
oracle.ref_model._relu like every other one.

Two switches:
  relu_masks / preacts   impose / collect the ReLU pattern: one key per MLP layer ("dnn.dnn.0", ...), one per
                         attention layer ("self_attention.0", ...) and "pred_rfd.0";
  emulate=True           round to bf16 (nearest even) at exactly the tensor boundaries where the kernels store bf16
                         (DESIGN §4.6): a straight-through function that rounds the value in forward and the gradient
                         in backward; weight operands are rounded in forward only (their gradients stay fp32); the
                         fp32 tensors (LR sum, FM term, P, logits) are not rounded, only the gradients that enter the
                         bf16 trunk through them are."""
import numpy as np
import torch

from oracle import ref_model as R

F64 = torch.float64


def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _bf16(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_bf16(g) if ctx.bwd else g), None, None


class _Em:
    """The rounding sites; every method is the identity when emulation is off."""

    def __init__(self, on):
        self.on = on

    def act(self, x):            # a bf16 activation: value and gradient rounded
        return _Round.apply(x, True, True) if self.on else x

    def weight(self, w):         # a bf16 GEMM operand of an fp32 master weight
        return _Round.apply(w, True, False) if self.on else w

    def grad(self, x):           # an fp32 value whose gradient enters the bf16 trunk
        return _Round.apply(x, False, True) if self.on else x


def _dnn(P, x, num_hidden, tower, em, relu_masks, preacts):
    if not em.on:
        return R.dnn(P, x, num_hidden, tower=tower, relu_masks=relu_masks, preacts=preacts)
    for i in range(num_hidden):
        key = f"{tower}.dnn.{3 * i}"
        z = x @ em.weight(P[key + ".weight"]).t() + P[key + ".bias"]
        x = em.act(R._relu(z, key, relu_masks, preacts))
    return x


def autoint_layer(P, x, i, ai, em, relu_masks, preacts):
    """oracle.ref_model.autoint_layer with the ReLU through R._relu (key self_attention.<i>) and the rounding sites."""
    B = x.shape[0]
    pre = f"self_attention.{i}."
    H, A = ai["num_attn_heads"], ai["attn_size"]
    q, k, v = (em.act(x @ em.weight(P[pre + n + ".weight"]).t()) for n in ("W_q", "W_k", "W_v"))
    qh, kh, vh = (t.reshape(B * H, -1, A) for t in (q, k, v))
    att = torch.bmm(qh, kh.transpose(1, 2))
    if ai["attn_scale"]:
        att = att / (A ** 0.5)
    out = em.act(torch.bmm(torch.softmax(att, dim=2), vh).reshape(B, -1, H * A))        # P stays unrounded
    if ai["res_conn"]:
        res = x @ em.weight(P[pre + "W_res.weight"]).t() if (pre + "W_res.weight") in P else x
        out = em.act(out + res)
    return R._relu(out, f"self_attention.{i}", relu_masks, preacts)


def _head_linear(P, x, name, em):
    return em.grad(x @ em.weight(P[name + ".weight"]).t() + P[name + ".bias"])


def step(backbone, mode, params, batch, num_hidden=0, ai=None, relu_masks=None, preacts=None, emulate=False):
    """One forward + backward.  backbone: "DeepFM" | "AutoInt"; mode: MFP | RFD | CTR; params: name -> array;
    batch: ids (already masked / replaced) and, by mode, labels, masked_index, noise, logq, dims (F, P, K) | labels |
    y.  -> (loss float, logits float64 array, {name: gradient float64 array})."""
    em = _Em(emulate)
    P = {k: torch.as_tensor(np.asarray(v)).to(F64).clone().requires_grad_(True) for k, v in params.items()}
    ids = batch["ids"]
    x3 = em.act(P["embed.embedding.weight"][ids])                  # the gathered rows
    kw = dict(relu_masks=relu_masks, preacts=preacts)
    lr = None
    if backbone == "DeepFM":
        vec = _dnn(P, x3.flatten(1), num_hidden, "dnn", em, **kw)
        lr_fm = R.lr_logit(P, ids) + R.fm_product_sum(em.grad(x3))         # fp32; the FM term's dx is bf16
        final = torch.cat([vec, em.act(lr_fm)], dim=1) if mode != "CTR" else vec
    elif backbone == "AutoInt":
        x = x3
        for i in range(ai["num_attn_layers"]):
            x = autoint_layer(P, x, i, ai, em, **kw)
        final = x.flatten(1)
        if "lr_layer.embed_w.weight" in P:
            lr = R.lr_logit(P, ids)
    else:
        raise NotImplementedError(backbone)
    if mode == "MFP":
        F_, Pj, K = batch["dims"]
        Ph = dict(P)
        Ph["feat_encoder.weight"] = em.weight(P["feat_encoder.weight"])       # the operand the bf16 GEMM reads
        loss, logits, _ = _mfp(Ph, final, batch, em, F_, Pj, K)
    elif mode == "RFD":
        z = em.act(R._relu(final @ em.weight(P["pred_rfd.0.weight"]).t() + P["pred_rfd.0.bias"], "pred_rfd.0",
                           relu_masks, preacts))
        logits = _head_linear(P, z, "pred_rfd.2", em)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, batch["labels"].to(F64))
        if not emulate:           # the oracle's own head, to the last bit of float64
            l2 = R.rfd_head(P, final, batch["labels"].to(F64), **kw)[0]
            assert float((l2 - loss).abs()) <= 1e-12 * max(1.0, float(loss.abs()))
    else:
        if backbone == "DeepFM":
            logits = _head_linear(P, final, "dnn_fc_out", em) + lr_fm
        else:
            logits = _head_linear(P, final, "attn_out", em)
            if lr is not None:
                logits = logits + lr
            if "dnn_out.weight" in P:
                logits = logits + _head_linear(P, _dnn(P, x3.flatten(1), ai["num_dnn_layers"], "dnn", em, **kw),
                                               "dnn_out", em)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), batch["y"].to(F64))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return float(loss), logits.detach().numpy(), grads


def _mfp(Ph, final, batch, em, F_, Pj, K):
    """R.mfp_head with the encoder's output passed through the gradient-rounding site: the head's formulae are the
    oracle's, only the product is formed here so that the site sits between it and the NCE loss."""
    enc = em.grad(final @ Ph["feat_encoder.weight"].t() + Ph["feat_encoder.bias"])
    # an identity encoder makes R.mfp_head read `enc` as it is
    n = enc.shape[1]
    Pi = dict(Ph)
    Pi["feat_encoder.weight"] = torch.eye(n, dtype=F64)
    Pi["feat_encoder.bias"] = torch.zeros(n, dtype=F64)
    return R.mfp_head(Pi, enc, batch["labels"], batch["masked_index"], batch["noise"], batch["logq"].to(F64), F_, Pj, K)


def fixture_batch(mode, cfg, inp):
    """The batch of a fixture case as the reference's step sees it."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ids, mi = t(inp["input_ids"]), t(inp["masked_index"])
    if mode == "MFP":
        masked, labels = R.dynamic_mask_mfp(ids, mi)
        return dict(ids=masked, labels=labels, masked_index=mi, noise=t(inp["noise"]),
                    logq=R.nce_buffers(inp["feat_count"])[0], dims=(cfg["F"], cfg["P"], cfg["K"]))
    if mode == "RFD":
        rep, labels = R.dynamic_mask_rfd(ids, mi, t(inp["replace_feat"]))
        return dict(ids=rep, labels=labels)
    return dict(ids=ids, y=t(inp["y"]))


def rel(got, want):
    """max |got - want| / max |want|: an error as a share of the tensor's scale."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))
