"""float64 torch restatement of the FGCNN trunk and its heads (reference models.py:325-407, layers.py:204-251 and
:105-137) for the bf16 compute mode's tests.  The rounding sites, the heads and the fixture batch come from
tests/bf16_backbones_ref.py; the ReLUs go through oracle.ref_model._relu.

Switches of step():
  relu_masks        impose the ReLU pattern of the recombine layers ("fgcnn_layer.recombine_layers.<i>.0", conv_act
                    relu), the MLP ("dnn.dnn.<3i>") and "pred_rfd.0";
  winners           impose the pooling winners: per stage the uint8 position inside the window that the kernels saved
                    ([B, C, Hp, E]); `stage_on` = per stage the sign pattern of the pooled output (conv_act relu: the
                    winner's ReLU);
  emulate=True      round to bf16 (nearest even) exactly where the kernels store bf16: the gathered rows, z (forward
                    only: dz stays fp32), the pooled output, the recombine Linear's output (with conv_act tanh that
                    is the saved pre-activation, and tanh's output is rounded too), the inner products, the MLP
                    activations; backward, the gradients crossing the same boundaries, each branch of a tensor with
                    two consumers before autograd adds them, and the fp32 heads' gradient where it enters the trunk.
                    The batch statistics are those of the ROUNDED z.  Weight operands of the GEMMs are rounded in forward
                    only; conv weights, batch-norm parameters and statistics are not rounded at all;
  dtype             float64, or float32 for "an fp32 accumulation, then the rounding" (what the kernels do).
Everything the step decided is returned, so that two runs can be compared unit by unit (pattern_difference)."""
import collections
import os

import numpy as np
import torch
import torch.nn.functional as F

import bf16_backbones_ref as BR
import fgcnn_params as fp
from bf16_backbones_ref import fixture_batch, rel          # noqa: F401  (re-exported)
from oracle import ref_model as R

EPS, MOMENTUM = 1e-5, 0.1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Result = collections.namedtuple("Result", "loss logits grads combined buffers preacts winners stage_on")


def fixture(mode, variant):
    return np.load(os.path.join(GOLD, f"{fp.CASE}_{mode}_{variant}.npz"))


def _pool(a, ps, winners):
    """MaxPool2d((ps,1), padding (H % ps, 0)) of a [B,C,H,E] -> (y, k uint8): the first of equal maxima wins; with
    `winners` the given positions are read instead."""
    H = a.shape[2]
    pad = H % ps
    Hp = (H + 2 * pad - ps) // ps + 1
    if winners is None:
        _, flat = F.max_pool2d(a.detach(), (ps, 1), padding=(pad, 0), return_indices=True)
        h = flat // a.shape[3]
    else:
        h = winners.long() + (torch.arange(Hp).view(1, 1, -1, 1) * ps - pad)
    assert tuple(h.shape) == (a.shape[0], a.shape[1], Hp, a.shape[3]) and int(h.min()) >= 0 and int(h.max()) < H
    k = (h - (torch.arange(Hp).view(1, 1, -1, 1) * ps - pad)).to(torch.uint8)
    return torch.gather(a, 2, h), k


def _trunk(cfg, variant, P, ids, em, relu_masks, preacts, winners, stage_on, training=True, buffers=None):
    """-> (combined [B,T,E], winners per stage, sign pattern per stage, new running statistics)."""
    act = fp.VARIANTS[variant]["conv_act"]
    x3 = em.act(P["embed.embedding.weight"][ids])
    x3g = x3 if fp.VARIANTS[variant]["share_embedding"] else em.act(P["fg_embed.embedding.weight"][ids])
    x = em.grad(x3g).unsqueeze(1)
    new, won, on, moved = [], [], [], {}
    for i, (c_in, c, kh, ps, r, h, h_out) in enumerate(fp.stages(cfg, variant)):
        pre = f"fgcnn_layer.conv_layers.{i}."
        z = em.weight(F.conv2d(x, P[pre + "0.weight"], P[pre + "0.bias"], padding=((kh - 1) // 2, 0)))
        if training:
            mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
            n = z.numel() // z.shape[1]
            if buffers is not None:
                rm, rv = buffers[pre + "1.running_mean"], buffers[pre + "1.running_var"]
                moved[pre + "1.running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean.detach())
                moved[pre + "1.running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var.detach() * n / (n - 1))
        else:
            mean, var = buffers[pre + "1.running_mean"], buffers[pre + "1.running_var"]
        sh = (1, -1, 1, 1)
        u = (z - mean.view(sh)) * (var.view(sh) + EPS).rsqrt() * P[pre + "1.weight"].view(sh) + P[pre + "1.bias"].view(sh)
        if act == "tanh":
            y, k = _pool(torch.tanh(u), ps, None if winners is None else winners[i])
            on.append(None)
        else:
            # (the winner of relu(u) is the winner of u wherever the pooled value is positive; elsewhere the value and
            # the gradient are zero whichever row wins)
            yu, k = _pool(torch.relu(u) if winners is None else u, ps, None if winners is None else winners[i])
            live = (yu.detach() > 0) if stage_on is None else stage_on[i]
            y = yu * live.to(yu.dtype)
            on.append(live)
        won.append(k)
        x = em.act(y)
        key = f"fgcnn_layer.recombine_layers.{i}.0"
        lin = x.flatten(1) @ em.weight(P[key + ".weight"]).t() + P[key + ".bias"]
        rec = em.act(torch.tanh(em.act(lin))) if act == "tanh" else em.act(R._relu(lin, key, relu_masks, preacts))
        new.append(rec.reshape(x.shape[0], -1, cfg["E"]))
    combined = em.grad(torch.cat([em.grad(x3)] + new, dim=1))
    return combined, won, on, moved


def _dense_input(combined, em):
    T = combined.shape[1]
    a = em.grad(combined)
    b = em.grad(combined)
    mask = torch.triu(torch.ones(T, T), 1).bool()
    ip = em.act(torch.masked_select(torch.bmm(b, b.transpose(1, 2)), mask).view(combined.shape[0], -1))
    return torch.cat([a.flatten(1), ip], dim=1)


def _head(cfg, mode, variant, P, dense, batch, em, relu_masks, preacts):
    if mode == "MFP":
        F_, Pj, K = batch["dims"]
        Ph = dict(P)
        Ph["feat_encoder.weight"] = em.weight(P["feat_encoder.weight"])
        Ph = {k: v.to(torch.float64) for k, v in Ph.items()}
        loss, logits, _ = BR._mfp(Ph, dense.to(torch.float64), batch, em, F_, Pj, K)
        return loss, logits
    if mode == "RFD":
        z = em.act(R._relu(dense @ em.weight(P["pred_rfd.0.weight"]).t() + P["pred_rfd.0.bias"], "pred_rfd.0",
                           relu_masks, preacts))
        logits = BR._head_linear(P, z, "pred_rfd.2", em)
        return F.binary_cross_entropy_with_logits(logits, batch["labels"].to(logits.dtype)), logits
    x = dense
    nh = fp.num_hidden_layers(cfg, variant)
    if nh > 0:
        if em.on:
            x = BR._dnn(P, x, nh, "dnn", em, relu_masks, preacts)
        else:
            x = R.dnn(P, x, nh, tower="dnn", relu_masks=relu_masks, preacts=preacts)
    logits = BR._head_linear(P, x, "fc_out", em)
    loss = None if "y" not in batch else F.binary_cross_entropy_with_logits(logits.view(-1), batch["y"].to(logits.dtype))
    return loss, logits


def step(cfg, mode, variant, params, batch, emulate=False, relu_masks=None, winners=None, stage_on=None,
         dtype=torch.float64, accumulate=None):
    """One training forward + backward from zeroed running statistics (mean 0, variance 1) -> Result."""
    dtype = accumulate or dtype
    em = BR._Em(emulate)
    P = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    buffers = {}
    for i, (_, c, *_r) in enumerate(fp.stages(cfg, variant)):
        buffers[f"fgcnn_layer.conv_layers.{i}.1.running_mean"] = torch.zeros(c, dtype=dtype)
        buffers[f"fgcnn_layer.conv_layers.{i}.1.running_var"] = torch.ones(c, dtype=dtype)
    preacts = {}
    combined, won, on, moved = _trunk(cfg, variant, P, batch["ids"], em, relu_masks, preacts, winners, stage_on,
                                      buffers=buffers)
    loss, logits = _head(cfg, mode, variant, P, _dense_input(combined, em), batch, em, relu_masks, preacts)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in P.items()}
    return Result(float(loss.detach()), logits.detach().double().numpy(), grads, combined.detach().double().numpy(),
                  {k: v.double().numpy() for k, v in moved.items()}, preacts, won, on)


def eval_logits(cfg, mode, variant, params, batch, buffers, emulate=False):
    """Eval mode on the given running statistics: the CTR logits / the RFD head's (None for MFP: the fixture has none)."""
    if mode == "MFP":
        return None
    em = BR._Em(emulate)
    with torch.no_grad():
        P = {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in params.items()}
        buf = {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in buffers.items()}
        combined, *_ = _trunk(cfg, variant, P, batch["ids"], em, None, None, None, None, training=False, buffers=buf)
        _, logits = _head(cfg, mode, variant, P, _dense_input(combined, em),
                          {k: v for k, v in batch.items() if k != "y"}, em, None, None)
    return logits.numpy()


def pattern_difference(a, b):
    """-> (decisions on which two Results differ, decisions): ReLU units of every hooked layer, pooling winners and,
    conv_act relu, the sign of every pooled value."""
    differ = total = 0
    assert set(a.preacts) == set(b.preacts)
    for k in a.preacts:
        differ += int(((a.preacts[k] > 0) != (b.preacts[k] > 0)).sum())
        total += a.preacts[k].numel()
    for wa, wb, oa, ob in zip(a.winners, b.winners, a.stage_on, b.stage_on):
        both = torch.ones_like(wa, dtype=torch.bool) if oa is None else (oa | ob)     # (a dead window has no winner)
        differ += int(((wa != wb) & both).sum())
        total += wa.numel()
        if oa is not None:
            differ += int((oa != ob).sum())
            total += oa.numel()
    return differ, total
