"""The Transformer trunk's bf16 kernels at kernel level: the bf16 I/O forms of the attention core and the field pooling
(csrc/mha.hip), the residual add + LayerNorm pair and the bf16 forms of gelu and dropout (csrc/extras.hip).

Every input is rounded to bf16 on the CPU first, so a float64 torch restatement ON THE SAME VALUES is the reference:
the only roundings the kernels add to their fp32 arithmetic are the ones where they store a bf16 output.

Bounds (derived, not measured):
  fp32 outputs (P, LayerNorm statistics, pooling weights, d_scores, dgamma, dbeta): the fp32 test's bound;
  bf16 outputs: that fp32 bound plus 2^-8 |ref| — half an ulp of one round-to-nearest-even to 8 significand bits.
Each case prints error / bound."""
import os

import numpy as np
import pytest
import torch

from test_mha_gpu import SHAPES, restate

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
HALF_ULP = 2.0 ** -8
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _rb(x):
    """Round to bf16 (nearest even): the bf16-representable float64 values kernels and reference are given."""
    return x.float().to(BF16).double()


def _dev(x):
    """A bf16-representable float64 CPU tensor as a bf16 device tensor (exact)."""
    d = x.float().to(BF16).to(DEV)
    assert torch.equal(d.cpu().double(), x.detach())
    return d


def _ratio(got, want, rtol, atol):
    got, want = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1)
    return float(((got - want).abs() / (rtol * want.abs() + atol)).max())


def _check_f32(what, got, want, rtol, atol):
    assert got.dtype == torch.float32, (what, got.dtype)
    r = _ratio(got, want, rtol, atol)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, (what, r)


def _check_bf16(what, got, want, rtol, atol):
    """|got - want| <= (rtol + 2^-8) |want| + atol, elementwise."""
    assert got.dtype == BF16, (what, got.dtype)
    r = _ratio(got, want, rtol + HALF_ULP, atol)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, (what, r)


# --------------------------------------------------------------------------- 1. attention core
def _mha_inputs(B, F, E, seed):
    g = torch.Generator().manual_seed(seed)
    return _rb(torch.randn(B * F, 3 * E, generator=g, dtype=torch.float64)), \
        _rb(torch.randn(B * F, E, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("F,E,H", SHAPES)
def test_mha_bf16_matches_float64_torch(ops, F, E, H):
    """B = 7: an odd group count and a half-filled two-group wave (F <= 32), one group per wave at F = 39, the
    largest shape F = 64, dh = 64, and the tiny (5, 8, 2) whose head sections are 8 bytes wide."""
    B = 7
    q64, do64 = _mha_inputs(B, F, E, 10)
    q64.requires_grad_(True)
    o_ref, P_ref = restate(q64, B, F, E, H)
    (o_ref * do64).sum().backward()
    qkv, do = _dev(q64), _dev(do64)
    o, P = ops.mha_fwd(qkv, B, F, E, H)
    assert o.shape == (B * F, E) and P.shape == (B * H, F, F)
    _check_f32("P", P, P_ref, 1e-5, 1e-6)
    _check_bf16("O", o, o_ref, 1e-5, 1e-5)
    # P comes from the widened inputs by the same fp32 arithmetic: the fp32 kernel's, bit for bit; O is its O rounded
    o32, P32 = ops.mha_fwd(qkv.float(), B, F, E, H)
    assert torch.equal(P, P32) and torch.equal(o, o32.to(BF16))
    d = ops.mha_bwd(qkv, P, do, B, F, E, H)
    assert d.shape == qkv.shape
    _check_bf16("d_qkv", d, q64.grad, 1e-4, 2e-5)
    o2, P2 = ops.mha_fwd(qkv, B, F, E, H)
    assert torch.equal(o, o2) and torch.equal(P, P2) and torch.equal(d, ops.mha_bwd(qkv, P, do, B, F, E, H))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("F,E,H", [(23, 16, 2), (39, 32, 4)])
def test_mha_bf16_dropout_uses_the_mask_of_mha_dropout_mask(ops, F, E, H, p):
    B, seed, offset = 9, 4321, (5 << 36) + 3
    keep = ops.mha_dropout_mask(B, F, H, p, seed, offset, device=DEV)
    assert 0 < int(keep.sum()) < keep.numel()
    q64, do64 = _mha_inputs(B, F, E, 11)
    q64.requires_grad_(True)
    o_ref, P_ref = restate(q64, B, F, E, H, keep=keep.cpu(), p=p)
    (o_ref * do64).sum().backward()
    qkv, do = _dev(q64), _dev(do64)
    o, P = ops.mha_fwd(qkv, B, F, E, H, p, seed, offset)
    _check_f32(f"P (p={p})", P, P_ref, 1e-5, 1e-6)
    _check_bf16(f"O (p={p})", o, o_ref, 1e-5, 1e-5)
    d = ops.mha_bwd(qkv, P, do, B, F, E, H, p, seed, offset)
    _check_bf16(f"d_qkv (p={p})", d, q64.grad, 1e-4, 2e-5)
    # the fp32 kernels draw the same mask
    o32, _ = ops.mha_fwd(qkv.float(), B, F, E, H, p, seed, offset)
    assert torch.equal(o, o32.to(BF16))
    o2, P2 = ops.mha_fwd(qkv, B, F, E, H, p, seed, offset)
    assert torch.equal(o, o2) and torch.equal(P, P2) and torch.equal(d, ops.mha_bwd(qkv, P, do, B, F, E, H, p, seed, offset))


def test_mha_bf16_rejects_mixed_types_cpu_tensors_and_head_size_6(ops):
    from mapx.native import MapxError
    B, F, E, H = 2, 23, 16, 2
    q16 = torch.zeros(B * F, 3 * E, device=DEV, dtype=BF16)
    P = torch.zeros(B * H, F, F, device=DEV)
    with pytest.raises(TypeError):
        ops.mha_bwd(q16, P, torch.zeros(B * F, E, device=DEV), B, F, E, H)               # bf16 qkv, fp32 d_o
    with pytest.raises(TypeError):
        ops.mha_bwd(q16.float(), P, torch.zeros(B * F, E, device=DEV, dtype=BF16), B, F, E, H)
    with pytest.raises(TypeError):
        ops.mha_bwd(q16, P.to(BF16), torch.zeros(B * F, E, device=DEV, dtype=BF16), B, F, E, H)   # probs stay fp32
    with pytest.raises(TypeError):
        ops.mha_fwd(q16.to(torch.float16), B, F, E, H)
    with pytest.raises(MapxError):
        ops.mha_fwd(q16.cpu(), B, F, E, H)
    with pytest.raises(MapxError):
        ops.mha_fwd(torch.zeros(B * F, 3 * 24, device=DEV, dtype=BF16), B, F, 24, 4)     # head size 6


# --------------------------------------------------------------------------- 2. residual add + LayerNorm
LN_SHAPES = [(94208, 16), (7, 16), (1000, 32), (33, 64), (5, 8)]


def _ln_case(R, E, with_s, eps):
    """Inputs and the float64 reference of a case.  The reference normalises the UNROUNDED sum x + s.
    The rows are drawn around 1.5, not 0: the saved mean is checked to a RELATIVE bound, which a row whose mean
    cancels to (nearly) zero cannot meet in any fp32 arithmetic — the sum of E values carries an error relative to
    sum |v|, not to the mean.  (A LayerNorm input in the trunk has no reason to be centred either.)"""
    g = torch.Generator().manual_seed(R + E)
    x = _rb(torch.randn(R, E, generator=g, dtype=torch.float64) + 1.5).requires_grad_(True)
    s = _rb(torch.randn(R, E, generator=g, dtype=torch.float64) + 1.5).requires_grad_(True) if with_s else None
    w = (torch.randn(E, generator=g) * 0.5 + 1.0).double().requires_grad_(True)
    b = (torch.randn(E, generator=g) * 0.5).double().requires_grad_(True)
    dy = _rb(torch.randn(R, E, generator=g, dtype=torch.float64))
    v = x + s if with_s else x
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    y = (v - mean) * rstd * w + b
    (y * dy).sum().backward()
    if with_s:
        assert torch.equal(x.grad, s.grad)
    return tuple(t.detach() for t in (x, s if with_s else x, w, b, dy, y, torch.cat([mean, rstd], 1), x.grad, w.grad,
                                      b.grad))


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("with_s", [True, False], ids=["add", "plain"])
@pytest.mark.parametrize("R,E", LN_SHAPES)
def test_add_layernorm_bf16_matches_float64_torch(ops, R, E, with_s, eps):
    x, s, w, b, dy, y_ref, stats_ref, dsum_ref, dw_ref, db_ref = _ln_case(R, E, with_s, eps)
    xd, sd, dyd = _dev(x), (_dev(s) if with_s else None), _dev(dy)
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    y, stats = ops.add_layernorm_fwd(xd, sd, wd, bd, eps)
    assert y.shape == (R, E) and stats.shape == (R, 2)
    _check_bf16("y", y, y_ref, 2e-5, 2e-5)
    _check_f32("stats", stats, stats_ref, 2e-5, 0.0)
    dw, db = torch.full((E,), 7.0, device=DEV), torch.full((E,), 7.0, device=DEV)
    dsum, dw_out, db_out = ops.add_layernorm_bwd(dyd, xd, sd, wd, stats, dw=dw, db=db, defer=True)
    assert dw_out is dw and db_out is db
    ops.flush_deferred()
    _check_bf16("dsum", dsum, dsum_ref, 1e-4, 1e-4)
    _check_f32("dgamma", dw, dw_ref, 1e-4, 1e-3)
    _check_f32("dbeta", db, db_ref, 1e-4, 1e-3)
    # the partial rows summed at once give the same bits as the deferred sum; two runs are bitwise equal
    y2, stats2 = ops.add_layernorm_fwd(xd, sd, wd, bd, eps)
    dsum2, dw2, db2 = ops.add_layernorm_bwd(dyd, xd, sd, wd, stats2)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    assert torch.equal(dsum, dsum2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("R,E", [(5, 12), (67, 64), (3, 4)])
def test_layernorm_fp32_and_bf16_entries_are_one_forward_kernel(ops, R, E):
    """On bf16-representable rows the fp32 entry and the bf16 entry (no second addend) see the same fp32 values: the
    saved (mean, rstd) are bitwise equal, and the bf16 y is the fp32 y rounded once."""
    g = torch.Generator().manual_seed(100 * R + E)
    x = _rb(torch.randn(R, E, generator=g, dtype=torch.float64) + 1.5)
    w = (torch.randn(E, generator=g) * 0.5 + 1.0).to(DEV)
    b = (torch.randn(E, generator=g) * 0.5).to(DEV)
    y32, stats32 = ops.layernorm_fwd(x.float().to(DEV), w, b, 1e-5)
    y16, stats16 = ops.add_layernorm_fwd(_dev(x), None, w, b, 1e-5)
    assert y32.dtype == torch.float32 and y16.dtype == BF16 and y16.shape == y32.shape == (R, E)
    assert torch.equal(stats32, stats16)
    assert torch.equal(y16, y32.to(BF16))


def test_add_layernorm_bf16_rejects_fp32_rows_and_wide_rows(ops):
    from mapx.native import MapxError
    x = torch.zeros(8, 16, device=DEV, dtype=BF16)
    w = torch.ones(16, device=DEV)
    with pytest.raises(TypeError):
        ops.add_layernorm_fwd(x.float(), None, w, w, 1e-5)
    with pytest.raises(TypeError):
        ops.add_layernorm_fwd(x, x.float(), w, w, 1e-5)
    with pytest.raises(MapxError):
        ops.add_layernorm_fwd(torch.zeros(8, 68, device=DEV, dtype=BF16), None, torch.ones(68, device=DEV),
                              torch.ones(68, device=DEV), 1e-5)


# --------------------------------------------------------------------------- 3. gelu
def test_gelu_bf16_forward_and_backward(ops):
    """The bf16-representable points of tests/golden/activations.npz (+-0, +-20 and +-88) and random ones,
    against float64 on the same values.  Bounds: those of test_hidden_act_kernels_and_mlp_vs_reference (y: rtol 2e-6,
    atol 3e-7; dz at dy = 1: rtol 1e-5, atol 1e-6, which scales with |dy|) + 2^-8 |ref|."""
    from oracle import ref_model as R
    pts = torch.from_numpy(np.load(os.path.join(GOLD, "activations.npz"))["x"]).double().reshape(-1)
    pts = pts[_rb(pts) == pts]
    assert pts.numel() >= 6 and float(pts.abs().max()) >= 20
    g = torch.Generator().manual_seed(3)
    for M, Nn in [(pts.numel(), 1), (37, 48), (5, 7)]:      # one column (scalar path), rows of 4-element groups, odd
        z = (pts.clone() if Nn == 1 else _rb(torch.randn(M, Nn, generator=g, dtype=torch.float64) * 2)).view(M, Nn)
        dy = _rb(torch.randn(M, Nn, generator=g, dtype=torch.float64))
        z.requires_grad_(True)
        y_ref = R.act("gelu", z)
        (y_ref * dy).sum().backward()
        zd, dyd = _dev(z.detach()), _dev(dy)
        y = ops.act_fwd("gelu", zd)
        dz = ops.act_bwd("gelu", dyd, zd)
        got, want = dz.cpu().double(), z.grad
        r = float(((got - want).abs() / ((1e-5 + HALF_ULP) * want.abs() + 1e-6 * dy.abs().clamp(min=1e-30))).max())
        _check_bf16(f"gelu y [{M},{Nn}]", y, y_ref, 2e-6, 3e-7)
        print(f"gelu dz [{M},{Nn}]: error / bound = {r:.3f}")
        assert dz.dtype == BF16 and r <= 1.0
        # a destination / an upstream gradient that is a column slice of a wider buffer
        wide = torch.full((M, Nn + 8), 7.0, device=DEV, dtype=BF16)
        ops.act_fwd("gelu", zd, out=wide[:, 4:4 + Nn])
        assert torch.equal(wide[:, 4:4 + Nn], y) and bool((wide[:, :4] == 7).all()) and bool((wide[:, -4:] == 7).all())
        gw = torch.randn(M, Nn + 8, device=DEV).to(BF16)
        assert torch.equal(ops.act_bwd("gelu", gw[:, 4:4 + Nn], zd), ops.act_bwd("gelu", gw[:, 4:4 + Nn].contiguous(), zd))
    with pytest.raises(TypeError):
        ops.act_bwd("gelu", dyd.float(), zd)


# --------------------------------------------------------------------------- 4. dropout
@pytest.mark.parametrize("n", [94208 * 16, 1001, 3])
def test_dropout_bf16_is_the_fp32_dropout_rounded_once(ops, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(BF16).to(DEV)
    dev = torch.tensor([5], dtype=torch.int32, device=DEV)
    for p, offset, off_dev in [(0.1, (17 << 36) + 1, None), (0.5, 9, dev)]:
        y = ops.dropout(x, p, 42, offset, off_dev)
        assert y.dtype == BF16 and torch.equal(y, ops.dropout(x.float(), p, 42, offset, off_dev).to(BF16))
        # backward draws the same mask: a gradient is zeroed exactly where the forward value was
        gy = (torch.rand(n, generator=g) + 0.5).to(BF16).to(DEV)
        gx = ops.dropout(gy, p, 42, offset, off_dev)
        nz = x != 0
        assert torch.equal((gx != 0)[nz], (y != 0)[nz])
        assert 0 < int((gx == 0).sum()) < n or n < 8
    assert torch.equal(ops.dropout(x, 0.0, 42, 1), x)
    # an 8-byte misaligned view takes the element path and gives the same values
    if n > 8:
        assert torch.equal(ops.dropout(x[1:], 0.1, 42, 3), ops.dropout(x[1:].clone(), 0.1, 42, 3))


# --------------------------------------------------------------------------- 5. field pooling
@pytest.mark.parametrize("mode", ["sum", "mean", "attn"])
@pytest.mark.parametrize("F,E", [(23, 16), (25, 64), (5, 8)])
def test_field_pool_bf16_matches_float64_torch(ops, mode, F, E):
    """Bounds of test_mha_gpu.test_field_pool_matches_torch, + 2^-8 |ref| on the bf16 outputs (pooled, dx)."""
    B = 37
    g = torch.Generator().manual_seed(5)
    x = _rb(torch.randn(B, F, E, generator=g, dtype=torch.float64)).requires_grad_(True)
    s = torch.randn(B, F, generator=g).double().requires_grad_(True)              # fp32 scores
    go = _rb(torch.randn(B, E, generator=g, dtype=torch.float64))
    if mode == "sum":
        ref = x.sum(1)
    elif mode == "mean":
        ref = x.sum(1) / F
    else:
        ref = (x * torch.softmax(s, dim=1).unsqueeze(-1)).sum(1)
    (ref * go).sum().backward()
    xd, sd = _dev(x.detach()), s.detach().float().to(DEV)
    out, w = ops.field_pool_fwd(xd, mode, sd if mode == "attn" else None)
    _check_bf16("pooled", out, ref, 1e-5, 1e-5)
    dx, ds = ops.field_pool_bwd(_dev(go), xd, mode, w)
    _check_bf16("dx", dx, x.grad, 1e-5, 1e-6)
    if mode == "attn":
        _check_f32("weights", w, torch.softmax(s, 1), 1e-5, 1e-7)
        _check_f32("d_scores", ds, s.grad, 1e-4, 1e-5)
    else:
        assert w is None and ds is None
    with pytest.raises(TypeError):
        ops.field_pool_bwd(go.float().to(DEV), xd, mode, w)
