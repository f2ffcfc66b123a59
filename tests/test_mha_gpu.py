"""csrc/mha.hip against a float64 torch restatement of nn.MultiheadAttention's core: the packed in-projection output
qkv [B*F, 3E] in, head h = columns [h*dh, (h+1)*dh) of each third, P = softmax(Q K^T / sqrt(dh)), dropout on P,
O = P~ V with the heads concatenated; backward into one packed d_qkv.  And the finetune head's field pooling."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (F, E, H): Avazu / proc_avazu / Criteo field counts, the largest shapes the kernel takes, a tiny odd one; B = 7
# leaves a half-filled wave for the two-groups-per-wave form (F <= 32) whenever B*H is odd
SHAPES = [(23, 16, 1), (23, 16, 2), (25, 16, 4), (39, 32, 4), (64, 64, 1), (5, 8, 2)]


def restate(qkv, B, F, E, H, keep=None, p=0.0):
    """float64 nn.MultiheadAttention core -> (o [B*F, E], P [B*H, F, F])."""
    dh = E // H
    x = qkv.view(B, F, 3, H, dh)
    q, k, v = (x[:, :, s].permute(0, 2, 1, 3) for s in range(3))          # [B, H, F, dh]
    P = torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, dim=-1)
    Pd = P if keep is None else P * keep.view(B, H, F, F).to(P.dtype) / (1.0 - p)
    o = (Pd @ v).permute(0, 2, 1, 3).reshape(B * F, E)
    return o, P.reshape(B * H, F, F)


def _qkv(B, F, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * F, 3 * E, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("F,E,H", SHAPES)
def test_forward_and_backward_match_float64_torch(F, E, H):
    from mapx import ops
    B = 7
    q64 = _qkv(B, F, E).requires_grad_(True)
    do64 = torch.randn(B * F, E, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    o_ref, P_ref = restate(q64, B, F, E, H)
    (o_ref * do64).sum().backward()
    qkv = q64.detach().float().to(DEV)
    o, P = ops.mha_fwd(qkv, B, F, E, H)
    np.testing.assert_allclose(P.cpu().double().numpy(), P_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o.cpu().double().numpy(), o_ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    d = ops.mha_bwd(qkv, P, do64.float().to(DEV), B, F, E, H)
    np.testing.assert_allclose(d.cpu().double().numpy(), q64.grad.numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("F,E,H", [(23, 16, 2), (39, 32, 4), (5, 8, 2)])
def test_dropout_mask_forward_and_backward(F, E, H):
    from mapx import ops
    B, p, seed, offset = 96, 0.1, 1234, (3 << 36) + 5
    keep = ops.mha_dropout_mask(B, F, H, p, seed, offset, device=DEV)
    n = keep.numel()
    kept = int(keep.sum())
    sd = (n * p * (1 - p)) ** 0.5
    assert abs((n - kept) - n * p) < 5 * sd, (n, kept)
    assert int(keep.max()) == 1 and int(keep.min()) == 0
    # a different offset draws a different mask
    assert not torch.equal(keep, ops.mha_dropout_mask(B, F, H, p, seed, offset + 1, device=DEV))
    q64 = _qkv(B, F, E, seed=2).requires_grad_(True)
    do64 = torch.randn(B * F, E, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    o_ref, P_ref = restate(q64, B, F, E, H, keep=keep.cpu(), p=p)
    (o_ref * do64).sum().backward()
    qkv = q64.detach().float().to(DEV)
    o, P = ops.mha_fwd(qkv, B, F, E, H, p, seed, offset)
    np.testing.assert_allclose(P.cpu().double().numpy(), P_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o.cpu().double().numpy(), o_ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    d = ops.mha_bwd(qkv, P, do64.float().to(DEV), B, F, E, H, p, seed, offset)
    np.testing.assert_allclose(d.cpu().double().numpy(), q64.grad.numpy(), rtol=1e-4, atol=2e-5)
    # the device-side offset word is added to `offset`, as HipDropout's
    dev = torch.tensor([7], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.mha_dropout_mask(B, F, H, p, seed, offset, dev, device=DEV),
                       ops.mha_dropout_mask(B, F, H, p, seed, offset + 7, device=DEV))
    o2, _ = ops.mha_fwd(qkv, B, F, E, H, p, seed, offset - 7, dev)
    assert torch.equal(o, o2)


def test_two_runs_are_bitwise_equal():
    from mapx import ops
    B, F, E, H = 1001, 23, 16, 2
    qkv = _qkv(B, F, E, seed=4).float().to(DEV)
    do = torch.randn(B * F, E, device=DEV)
    runs = []
    for _ in range(2):
        o, P = ops.mha_fwd(qkv, B, F, E, H, 0.1, 9, 77)
        runs.append((o, P, ops.mha_bwd(qkv, P, do, B, F, E, H, 0.1, 9, 77)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_unsupported_shapes_are_rejected():
    from mapx import ops
    from mapx.native import MapxError
    qkv = torch.zeros(2 * 65 * 48, device=DEV).view(-1, 48)
    with pytest.raises(MapxError):
        ops.mha_fwd(qkv, 2, 65, 16, 1)                      # F > 64
    with pytest.raises(MapxError):
        ops.mha_fwd(qkv[:2 * 23], 2, 23, 24, 4)               # head size 6
    with pytest.raises(MapxError):
        ops.mha_fwd(torch.zeros(2 * 23, 3 * 128, device=DEV), 2, 23, 128, 1)    # head size 128


@pytest.mark.parametrize("mode", ["sum", "mean", "attn"])
@pytest.mark.parametrize("F,E", [(23, 16), (25, 68), (5, 4)])
def test_field_pool_matches_torch(mode, F, E):
    from mapx import ops
    B = 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, F, E, generator=g, dtype=torch.float64, requires_grad=True)
    s = torch.randn(B, F, generator=g, dtype=torch.float64, requires_grad=True)
    go = torch.randn(B, E, generator=g, dtype=torch.float64)
    if mode == "sum":
        ref = x.sum(1)
    elif mode == "mean":
        ref = x.sum(1) / F
    else:
        ref = (x * torch.softmax(s, dim=1).unsqueeze(-1)).sum(1)
    (ref * go).sum().backward()
    xd, sd = x.detach().float().to(DEV), s.detach().float().to(DEV)
    out, w = ops.field_pool_fwd(xd, mode, sd if mode == "attn" else None)
    np.testing.assert_allclose(out.cpu().double().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    dx, ds = ops.field_pool_bwd(go.float().to(DEV), xd, mode, w)
    np.testing.assert_allclose(dx.cpu().double().numpy(), x.grad.numpy(), rtol=1e-5, atol=1e-6)
    if mode == "attn":
        np.testing.assert_allclose(w.cpu().double().numpy(), torch.softmax(s, 1).detach().numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(ds.cpu().double().numpy(), s.grad.numpy(), rtol=1e-4, atol=1e-5)
    else:
        assert w is None and ds is None
