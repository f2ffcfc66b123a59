"""bf16 I/O forms of the AutoInt attention core, the DeepFM FM term and the segment reduction with the extra scalar
(csrc/attn.hip, csrc/fm.hip, csrc/segplan.hip: the *_bf16 entries), at kernel level.

Every input is rounded to bf16 on the CPU first, so a float64 torch restatement ON THE SAME VALUES is the reference:
the only roundings the kernels add to their fp32 arithmetic are the ones where they store a bf16 output.  Cases,
restatements and fp32 bounds are those of test_backbone_kernels_gpu.py and test_attn_dropout_gpu.py.

Bounds (derived, not measured):
  fp32 outputs (P, fm, s, the reduced rows and scalars): the fp32 bound of the test the case comes from;
  bf16 outputs (o, dq, dk, dv, dx): that fp32 bound plus 2^-8 |ref| — half an ulp of one round-to-nearest-even to
  8 significand bits (the rounding is of the fp32 value, which itself lies within the fp32 bound of the reference)."""
import numpy as np
import pytest
import torch

import test_attn_dropout_gpu as TD
import test_backbone_kernels_gpu as TB

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
HALF_ULP = 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _cpu(x):
    return x.detach().cpu()


def _rb(x):
    """Round to bf16 (nearest even) and back: the bf16-representable float32 values the kernels are given."""
    return x.to(BF16).float()


def _check_f32(what, got, want, rtol, atol):
    assert got.dtype == torch.float32, (what, got.dtype)
    print(f"{what}: error / bound = {TD._ratio(got, want, rtol, atol):.3f}")
    np.testing.assert_allclose(_cpu(got).double().numpy().reshape(-1), want.detach().numpy().reshape(-1), rtol=rtol,
                               atol=atol, err_msg=what)


def _check_bf16(what, got, want, rtol, atol):
    """|got - want| <= (rtol + 2^-8) |want| + atol, elementwise."""
    assert got.dtype == BF16, (what, got.dtype)
    got, want = _cpu(got).double().reshape(-1), want.detach().double().reshape(-1)
    bound = (rtol + HALF_ULP) * want.abs() + atol
    ratio = float(((got - want).abs() / bound).max())
    print(f"{what}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


def _attn_inputs(G, F, A):
    return [_rb(t) for t in TB.attn_inputs(G, F, A)]


# --------------------------------------------------------------------------- attention core
@pytest.mark.parametrize("G,F,A,scaled", TB.ATTN_CASES)
def test_attn_bf16_matches_float64_torch(ops, G, F, A, scaled):
    q, k, v, d_o = _attn_inputs(G, F, A)
    p_ref, o_ref, dq_ref, dk_ref, dv_ref = TB.attn_restate(q, k, v, d_o, G, F, A, scaled)
    qd, kd, vd, dod = (t.to(DEV).to(BF16) for t in (q, k, v, d_o))
    assert all(torch.equal(a.float().cpu(), b) for a, b in zip((qd, kd, vd, dod), (q, k, v, d_o)))
    o, p = ops.attn_fwd(qd, kd, vd, G, F, A, scaled)
    assert p.shape == (G, F, F) and o.shape == qd.shape
    _check_f32("P", p, p_ref, **TB.P_TOL)
    _check_bf16("O", o, o_ref, **TB.O_TOL)
    rows = _cpu(p).double().sum(-1)
    assert float((rows - 1).abs().max()) <= 1e-6, float((rows - 1).abs().max())
    dq, dk, dv = ops.attn_bwd(qd, kd, vd, p, dod, G, F, A, scaled)
    _check_bf16("dQ", dq, dq_ref, **TB.GRAD_TOL)
    _check_bf16("dK", dk, dk_ref, **TB.GRAD_TOL)
    _check_bf16("dV", dv, dv_ref, **TB.GRAD_TOL)
    # same inputs -> same bits
    o2, p2 = ops.attn_fwd(qd, kd, vd, G, F, A, scaled)
    assert torch.equal(o, o2) and torch.equal(p, p2)
    for a, b in zip((dq, dk, dv), ops.attn_bwd(qd, kd, vd, p, dod, G, F, A, scaled)):
        assert torch.equal(a, b)


def test_attn_bf16_probabilities_are_those_of_the_fp32_kernel(ops):
    """P is computed from the widened inputs by the same fp32 arithmetic: on bf16-representable inputs the two element
    types give the same P bit for bit, and the bf16 O is the fp32 O rounded once."""
    G, F, A = 7, 23, 12
    q, k, v, _ = _attn_inputs(G, F, A)
    o32, p32 = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), G, F, A, 1)
    o16, p16 = ops.attn_fwd(q.to(DEV).to(BF16), k.to(DEV).to(BF16), v.to(DEV).to(BF16), G, F, A, 1)
    assert torch.equal(p32, p16)
    assert torch.equal(o32.to(BF16), o16)


def test_attn_bf16_rejects_mixed_types_sizes_and_cpu_tensors(ops):
    from mapx.native import MapxError
    G, F, A = 2, 8, 8
    x16 = torch.zeros(G * F * A, device=DEV, dtype=BF16)
    x32 = torch.zeros(G * F * A, device=DEV)
    p = torch.zeros(G, F, F, device=DEV)
    with pytest.raises(TypeError):
        ops.attn_fwd(x16, x32, x16, G, F, A, 1)
    with pytest.raises(TypeError):
        ops.attn_bwd(x16, x16, x16, p, x32, G, F, A, 1)
    with pytest.raises(TypeError):
        ops.attn_bwd(x16, x16, x16, p.to(BF16), x16, G, F, A, 1)
    for Gb, Fb, Ab in [(2, 65, 8), (2, 8, 65)]:
        xb = torch.zeros(Gb * Fb * Ab, device=DEV, dtype=BF16)
        with pytest.raises(MapxError):
            ops.attn_fwd(xb, xb, xb, Gb, Fb, Ab, 1)
        with pytest.raises(MapxError):
            ops.attn_drop_fwd(xb, xb, xb, Gb, Fb, Ab, 1, 0.1, 1, 2, 3)
    with pytest.raises(MapxError):
        ops.attn_fwd(x16.cpu(), x16.cpu(), x16.cpu(), G, F, A, 1)
    e = torch.zeros(0, device=DEV, dtype=BF16)
    o, pr = ops.attn_fwd(e, e, e, 0, 23, 12, 1)
    assert o.numel() == 0 and o.dtype == BF16 and pr.shape == (0, 23, 23)


# --------------------------------------------------------------------------- dropout forms
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("G,F,A,scaled", TD.CASES)
def test_attn_drop_bf16_matches_float64_torch_with_the_exported_masks(ops, G, F, A, scaled, p):
    q, k, v, d_o = _attn_inputs(G, F, A)
    keep_p, keep_o = ops.attn_dropout_masks(G, F, A, p, TD.SEED, TD.OFF_P, TD.OFF_O)
    p_ref, o_ref, dq_ref, dk_ref, dv_ref = TD.drop_restate(q, k, v, d_o, _cpu(keep_p), _cpu(keep_o), G, F, A, scaled, p)
    qd, kd, vd, dod = (t.to(DEV).to(BF16) for t in (q, k, v, d_o))
    o, probs = ops.attn_drop_fwd(qd, kd, vd, G, F, A, scaled, p, TD.SEED, TD.OFF_P, TD.OFF_O)
    assert probs.shape == (G, F, F) and o.shape == qd.shape
    _check_f32("P", probs, p_ref, **TD.P_TOL)
    _check_bf16("O", o, o_ref, **TD.O_TOL)
    assert bool((o.view(G, F, A)[keep_o == 0] == 0).all())          # a dropped output is an exact zero
    rows = _cpu(probs).double().sum(-1)
    assert float((rows - 1).abs().max()) <= 1e-6
    dq, dk, dv = ops.attn_drop_bwd(qd, kd, vd, probs, dod, G, F, A, scaled, p, TD.SEED, TD.OFF_P, TD.OFF_O)
    _check_bf16("dQ", dq, dq_ref, **TD.GRAD_TOL)
    _check_bf16("dK", dk, dk_ref, **TD.GRAD_TOL)
    _check_bf16("dV", dv, dv_ref, **TD.GRAD_TOL)
    # same inputs -> same bits
    o2, probs2 = ops.attn_drop_fwd(qd, kd, vd, G, F, A, scaled, p, TD.SEED, TD.OFF_P, TD.OFF_O)
    assert torch.equal(o, o2) and torch.equal(probs, probs2)
    for a, b in zip((dq, dk, dv),
                    ops.attn_drop_bwd(qd, kd, vd, probs, dod, G, F, A, scaled, p, TD.SEED, TD.OFF_P, TD.OFF_O)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("G,F,A,scaled", [(7, 23, 12, 1), (5, 33, 16, 0), (4, 25, 7, 0)])
def test_attn_drop_bf16_rate_zero_is_the_plain_bf16_core_bitwise(ops, G, F, A, scaled):
    q, k, v, d_o = (t.to(DEV).to(BF16) for t in _attn_inputs(G, F, A))
    o, pr = ops.attn_fwd(q, k, v, G, F, A, scaled)
    o2, pr2 = ops.attn_drop_fwd(q, k, v, G, F, A, scaled, 0.0, TD.SEED, TD.OFF_P, TD.OFF_O)
    assert o2.dtype == BF16 and torch.equal(o, o2) and torch.equal(pr, pr2)
    for x, y in zip(ops.attn_bwd(q, k, v, pr, d_o, G, F, A, scaled),
                    ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, scaled, 0.0, TD.SEED, TD.OFF_P, TD.OFF_O)):
        assert x.dtype == BF16 and torch.equal(x, y)


# --------------------------------------------------------------------------- FM term
FM_CASES_BF16 = [c for c in TB.FM_CASES if c.values[2] >= 8]


def _fm_inputs(B, F, E):
    x, g = TB.fm_inputs(B, F, E)
    return _rb(x), g                    # g stays fp32: it is the fp32 gradient of the fp32 term


def _within_bf16(what, got, ref, scale):
    """fp32 bound of TB._within plus 2^-8 |ref|."""
    assert got.dtype == BF16
    err = (_cpu(got).double() - ref).abs()
    bound = TB.FM_C * scale + 1e-6 + HALF_ULP * ref.abs()
    print(f"{what}: error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("B,F,E", FM_CASES_BF16)
def test_fm_bf16_matches_float64_torch(ops, B, F, E):
    x, g = _fm_inputs(B, F, E)
    fm_ref, s_ref, dx_ref = TB.fm_restate(x, g)
    fm_sc, s_sc, dx_sc = TB.fm_scales(x, g)
    xd = x.to(DEV).to(BF16)
    fm, s = ops.fm_fwd(xd)
    assert fm.shape == (B,) and s.shape == (B, E) and fm.dtype == s.dtype == torch.float32
    TB._within(fm, fm_ref, fm_sc)
    TB._within(s, s_ref, s_sc)
    dx = ops.fm_bwd(g.to(DEV), s, xd)
    assert dx.shape == (B, F, E)
    _within_bf16("dx", dx, dx_ref, dx_sc)
    fm2, s2 = ops.fm_fwd(xd)
    assert torch.equal(fm, fm2) and torch.equal(s, s2) and torch.equal(dx, ops.fm_bwd(g.to(DEV), s, xd))
    # the same fp32 sums as the fp32 kernel on the same values
    fm32, s32 = ops.fm_fwd(x.to(DEV))
    assert torch.equal(fm, fm32) and torch.equal(s, s32)


def test_fm_bf16_rejects_embed_size_4_other_sizes_and_cpu_tensors(ops):
    from mapx.native import MapxError
    for E in (4, 12, 128):
        with pytest.raises(MapxError):
            ops.fm_fwd(torch.zeros(2, 3, E, device=DEV, dtype=BF16))
    with pytest.raises(MapxError):
        ops.fm_bwd(torch.zeros(2, device=DEV), torch.zeros(2, 4, device=DEV), torch.zeros(2, 3, 4, device=DEV, dtype=BF16))
    with pytest.raises(MapxError):
        ops.fm_fwd(torch.zeros(2, 3, 8, dtype=BF16))
    with pytest.raises(MapxError):
        ops.fm_bwd(torch.zeros(2), torch.zeros(2, 8), torch.zeros(2, 3, 8, dtype=BF16))
    with pytest.raises(TypeError):
        ops.fm_bwd(torch.zeros(2, device=DEV, dtype=BF16), torch.zeros(2, 8, device=DEV),
                   torch.zeros(2, 3, 8, device=DEV, dtype=BF16))


def test_fm_product_sum_bf16_autograd(ops):
    """layers.fm_product_sum on bf16 rows: fp32 [B,1] out, bf16 dx back."""
    from mapx import layers
    B, F, E = 33, 23, 16
    x, g = _fm_inputs(B, F, E)
    fm_ref, _, dx_ref = TB.fm_restate(x, g)
    fm_sc, _, dx_sc = TB.fm_scales(x, g)
    xd = x.to(DEV).to(BF16).requires_grad_(True)
    out = layers.fm_product_sum(xd)
    assert out.shape == (B, 1) and out.dtype == torch.float32
    (out * g.to(DEV).view(B, 1)).sum().backward()
    TB._within(out.view(-1), fm_ref, fm_sc)
    _within_bf16("dx", xd.grad, dx_ref, dx_sc)


# --------------------------------------------------------------------------- reduction with the extra scalar
@pytest.mark.parametrize("n,V,W,group,ld,estride", TB.SEG_CASES)
def test_seg_reduce_rows_extra_bf16(ops, n, V, W, group, ld, estride):
    """bf16 source rows, fp32 scalar, fp32 sums: against a float64 index_add_ of the same values at rtol 1e-5,
    atol 2e-5 (the bound of test_bf16_gpu.py::test_bf16_gather_and_row_gradient); a second plan gives the same bits."""
    keys = TB._skewed_keys(n, V, n)
    g = torch.Generator().manual_seed(n + W)
    src = _rb(torch.randn(n, ld, generator=g))
    src_d = src.to(DEV).to(BF16)
    if estride == 1 or group > 1:
        extra = torch.randn(-(-n // group) * estride, generator=g)
        extra_d = extra.to(DEV)
    else:                                                       # a strided fp32 column: the scalar of position p at p * ld
        assert estride == ld and ld > W
        wide = torch.randn(n, ld, generator=g)
        extra, extra_d = wide.reshape(-1)[W:], wide.to(DEV)[:, W]
    terms = extra[(torch.arange(n) // group) * estride].double()
    keys_d = keys.to(torch.int32).to(DEV)
    plan = ops.SegPlan(keys_d, V)
    U = plan.count()
    uniq_ref, inv = torch.unique(keys, return_inverse=True)
    assert U == uniq_ref.numel()
    rows, scal = ops.seg_reduce_rows_extra(plan, src_d, W, extra_d, group, extra_stride=estride)
    assert rows.shape == (n, W) and scal.shape == (n,) and rows.dtype == scal.dtype == torch.float32
    ref = torch.zeros(U, W, dtype=torch.float64).index_add_(0, inv, src[:, :W].double())
    ref1 = torch.zeros(U, dtype=torch.float64).index_add_(0, inv, terms)
    np.testing.assert_allclose(_cpu(rows[:U]).double().numpy(), ref.numpy(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(_cpu(scal[:U]).double().numpy(), ref1.numpy(), rtol=1e-5, atol=2e-5)
    # a second plan of the same keys: identical bits (fixed order of the plan, no atomics)
    plan2 = ops.SegPlan(keys_d.clone(), V)
    rows2, scal2 = ops.seg_reduce_rows_extra(plan2, src_d, W, extra_d, group, extra_stride=estride)
    assert torch.equal(rows[:U], rows2[:U]) and torch.equal(scal[:U], scal2[:U])
    # the scalar rides along without disturbing the rows: the bits of the plain bf16 reduction
    plain = ops.seg_reduce_rows(plan2, src_d[:, :W].contiguous(), W)
    assert torch.equal(rows[:U], plain[:U])


def test_seg_reduce_rows_extra_bf16_rejects_a_bf16_scalar_and_cpu_tensors(ops):
    from mapx.native import MapxError
    keys = torch.arange(8, dtype=torch.int32, device=DEV)
    plan = ops.SegPlan(keys, 100)
    src = torch.zeros(8, 16, device=DEV, dtype=BF16)
    with pytest.raises(TypeError):
        ops.seg_reduce_rows_extra(plan, src, 16, torch.zeros(8, device=DEV, dtype=BF16), 1)
    with pytest.raises(MapxError):
        ops.seg_reduce_rows_extra(plan, src.cpu(), 16, torch.zeros(8), 1)
