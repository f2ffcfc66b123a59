"""Kernel-level parity for the backbone primitives that so far ran only inside whole-model tests: the AutoInt
attention core (attn.hip), the DeepFM terms (fm.hip), the segment reduction with an extra scalar and the exchange
message pack (segplan.hip), and the CIN outer product with a padded row.

Every test builds seeded inputs on the CPU, restates the operation in float64 torch from the definition in the
kernel's header comment, runs the HIP kernel through its mapx.ops wrapper and compares.  The restatements take a
dtype so that the same formulas can be evaluated in float32 on the CPU: every tolerance below is either copied from
the test it names or carries the worst float32-CPU ratio (error / bound) it was checked against."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _cpu(x):
    return x.detach().cpu()


def _close(got, want, rtol, atol):
    np.testing.assert_allclose(_cpu(got).double().numpy(), want.detach().numpy(), rtol=rtol, atol=atol)


# --------------------------------------------------------------------------- AutoInt attention core
# (G, F, A, scaled).  F <= 32: attn_*_kernel<2>, two groups per wave; F >= 33: attn_*_kernel<1>.
# Tolerances are those of test_mha_gpu.py::test_forward_and_backward_match_float64_torch.  A float32 torch-CPU
# evaluation of attn_restate stays inside them at unit-variance inputs for every case, so the inputs are plain randn:
# worst ratios error / (rtol * |ref| + atol) over the cases: P 0.10, O 0.12, gradients 0.10 (all three at
# (6, 32, 16, unscaled)); rows of P sum to 1 within 2.5e-7.
ATTN_CASES = [
    pytest.param(7, 23, 12, 1, id="G7-F23-A12-scaled:odd-G-two-per-wave-avazu"),
    pytest.param(1, 5, 1, 1, id="G1-F5-A1-scaled:empty-upper-half-wave-A1"),
    pytest.param(6, 32, 16, 0, id="G6-F32-A16-unscaled:last-F-of-two-per-wave"),
    pytest.param(5, 33, 16, 1, id="G5-F33-A16-scaled:first-F-of-one-per-wave"),
    pytest.param(14, 39, 12, 1, id="G14-F39-A12-scaled:criteo"),
    pytest.param(3, 64, 64, 1, id="G3-F64-A64-scaled:largest-raised-lds-limit"),
    pytest.param(4, 25, 7, 0, id="G4-F25-A7-unscaled:A-not-multiple-of-4"),
]
P_TOL = dict(rtol=1e-5, atol=1e-6)
O_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=2e-5)


def attn_inputs(G, F, A):
    """q, k, v, dO as float32 [G*F*A]: group g is the g-th run of F*A consecutive floats."""
    g = torch.Generator().manual_seed(1000 * G + 10 * F + A)
    return [torch.randn(G * F * A, generator=g) for _ in range(4)]


def attn_restate(q, k, v, d_o, G, F, A, scaled, dtype=torch.float64):
    """S = Q K^T (/ sqrt(A)), P = softmax(S), O = P V on [G, F, A] views; gradients by autograd of (O * dO).sum()."""
    q, k, v = (t.to(dtype).view(G, F, A).requires_grad_(True) for t in (q, k, v))
    s = q @ k.transpose(1, 2)
    if scaled:
        s = s / A ** 0.5
    p = torch.softmax(s, dim=-1)
    o = p @ v
    (o * d_o.to(dtype).view(G, F, A)).sum().backward()
    return p.detach(), o.detach().reshape(-1), q.grad.reshape(-1), k.grad.reshape(-1), v.grad.reshape(-1)


@pytest.mark.parametrize("G,F,A,scaled", ATTN_CASES)
def test_attn_matches_float64_torch(ops, G, F, A, scaled):
    q, k, v, d_o = attn_inputs(G, F, A)
    p_ref, o_ref, dq_ref, dk_ref, dv_ref = attn_restate(q, k, v, d_o, G, F, A, scaled)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, d_o))
    o, p = ops.attn_fwd(qd, kd, vd, G, F, A, scaled)
    assert p.shape == (G, F, F) and o.shape == qd.shape
    _close(p, p_ref, **P_TOL)
    _close(o, o_ref, **O_TOL)
    rows = _cpu(p).double().sum(-1)
    assert float((rows - 1).abs().max()) <= 1e-6, float((rows - 1).abs().max())
    dq, dk, dv = ops.attn_bwd(qd, kd, vd, p, dod, G, F, A, scaled)
    _close(dq, dq_ref, **GRAD_TOL)
    _close(dk, dk_ref, **GRAD_TOL)
    _close(dv, dv_ref, **GRAD_TOL)
    # same inputs -> same bits
    o2, p2 = ops.attn_fwd(qd, kd, vd, G, F, A, scaled)
    assert torch.equal(o, o2) and torch.equal(p, p2)
    for a, b in zip((dq, dk, dv), ops.attn_bwd(qd, kd, vd, p, dod, G, F, A, scaled)):
        assert torch.equal(a, b)


def large_logit_inputs(kind, G=3, F=39, A=12):
    g = torch.Generator().manual_seed(39)
    qk = 30 * torch.randn(G * F * A, generator=g)
    if kind == "integer":
        qk = qk.round()
    return qk, torch.randn(G * F * A, generator=g), G, F, A


def large_logit_bound(qk, p_ref, G, F, A):
    """Per element bound on |P - P_ref| for logits evaluated in float32: a dot product of A terms is off by at most
    D = gamma_A * sum_a |q_a k_a| (gamma_A = A u / (1 - A u), u = 2^-24, any summation order, fused or not), so a
    row's logit differences are off by at most 2 * max_j D_ij and P by the factor exp of that; 1e-6 absolute (the
    P tolerance of the test above) covers expf, the normalisation and the rounding of s - max."""
    u = 2.0 ** -24
    x = qk.double().view(G, F, A).abs()
    d = (A * u / (1 - A * u)) * (x @ x.transpose(1, 2))
    return p_ref * torch.expm1(2 * d.amax(-1, keepdim=True)) + 1e-6


@pytest.mark.parametrize("kind", ["randn", "integer"])
def test_attn_large_logits_need_the_max_subtraction(ops, kind):
    """Q = K = 30 * randn, unscaled, F = 39: logits in the thousands, exp() of which overflows unless the row maximum
    is subtracted first.  'randn': the bound is the float32 rounding of the logits themselves (large_logit_bound, a
    worst-case bound: float32-CPU ratio error / bound 1.1e-4).  'integer': the same values rounded to integers, whose
    products and 12-term sums are exact in float32 (< 2^24), so the logits are exact and P holds the plain P
    tolerance of the test above (float32-CPU ratio 0.002)."""
    qk, v, G, F, A = large_logit_inputs(kind)
    p_ref = attn_restate(qk, qk, v, v, G, F, A, 0)[0]
    assert float((qk.double().view(G, F, A) ** 2).sum(-1).max()) > 1000      # exp() of it is inf in float32
    qd = qk.to(DEV)
    _, p = ops.attn_fwd(qd, qd, v.to(DEV), G, F, A, 0)
    assert bool(torch.isfinite(p).all())
    if kind == "integer":
        _close(p, p_ref, **P_TOL)
    else:
        err = (_cpu(p).double() - p_ref).abs()
        bound = large_logit_bound(qk, p_ref, G, F, A)
        assert bool((err <= bound).all()), float((err / bound).max())
    rows = _cpu(p).double().sum(-1)
    assert float((rows - 1).abs().max()) <= 1e-6


def test_attn_rejects_unsupported_sizes(ops):
    from mapx.native import MapxError
    for G, F, A in [(2, 65, 8), (2, 8, 65), (2, 0, 8)]:
        x = torch.zeros(G * F * A, device=DEV)
        p = torch.zeros(G, F, F, device=DEV)
        with pytest.raises(MapxError):
            ops.attn_fwd(x, x, x, G, F, A, 1)
        with pytest.raises(MapxError):
            ops.attn_bwd(x, x, x, p, x, G, F, A, 1)
    # no groups: empty outputs, no launch, no error
    x = torch.zeros(0, device=DEV)
    o, p = ops.attn_fwd(x, x, x, 0, 23, 12, 1)
    assert o.numel() == 0 and p.shape == (0, 23, 23)
    assert all(t.numel() == 0 for t in ops.attn_bwd(x, x, x, p, x, 0, 23, 12, 1))


# --------------------------------------------------------------------------- DeepFM terms
# (B, F, E): every fm_fwd_kernel<E>; several rows per wave (E < 64); B * E no multiple of 256; the last adds
# fm_bwd's second grid-stride trip (B * F * E / 4 > 2048 blocks * 256 threads) at no more than 9 MB.
FM_CASES = [
    pytest.param(1, 1, 4, id="B1-F1-E4:one-field-one-row"),
    pytest.param(3, 5, 4, id="B3-F5-E4:kernel<4>-16-rows-per-wave"),
    pytest.param(33, 23, 8, id="B33-F23-E8:kernel<8>-tail"),
    pytest.param(64, 25, 16, id="B64-F25-E16:kernel<16>-fixture-shape"),
    pytest.param(17, 39, 32, id="B17-F39-E32:kernel<32>-tail"),
    pytest.param(9, 39, 64, id="B9-F39-E64:kernel<64>-tail"),
    pytest.param(1031, 23, 16, id="B1031-F23-E16:prime-B-partly-filled-last-block"),
    pytest.param(2053, 17, 64, id="B2053-F17-E64:fm_bwd-grid-stride-second-trip"),
]
# |got - ref| <= FM_C * scale + 1e-6, scale = the same expression with every term replaced by its absolute value
# (the form of test_kernels_gpu.py::test_seg_plan_and_reduce_rows).  Worst float32-CPU ratios error / bound over
# FM_CASES at 1e-6: fm 0.016, s 0.19, dx 0.23.
FM_C = 1e-6


def fm_restate(x, g, dtype=torch.float64):
    """fm[b] = 0.5 sum_e((sum_f x)^2 - sum_f x^2); s[b,e] = sum_f x; dx[b,f,e] = g[b] (s[b,e] - x[b,f,e])."""
    x, g = x.to(dtype), g.to(dtype)
    s = x.sum(1)
    fm = 0.5 * (s * s - (x * x).sum(1)).sum(1)
    dx = g[:, None, None] * (s[:, None, :] - x)
    return fm, s, dx


def fm_scales(x, g):
    x, g = x.double(), g.double()
    sa = x.abs().sum(1)
    return 0.5 * (sa * sa + (x * x).sum(1)).sum(1), sa, g.abs()[:, None, None] * (sa[:, None, :] + x.abs())


def fm_inputs(B, F, E):
    g = torch.Generator().manual_seed(B * 131 + F * 7 + E)
    return torch.randn(B, F, E, generator=g), torch.randn(B, generator=g)


def _within(got, ref, scale, c=FM_C):
    err = (_cpu(got).double() - ref).abs()
    bound = c * scale + 1e-6
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("B,F,E", FM_CASES)
def test_fm_matches_float64_torch(ops, B, F, E):
    x, g = fm_inputs(B, F, E)
    fm_ref, s_ref, dx_ref = fm_restate(x, g)
    fm_sc, s_sc, dx_sc = fm_scales(x, g)
    xd = x.to(DEV)
    fm, s = ops.fm_fwd(xd)
    assert fm.shape == (B,) and s.shape == (B, E)
    _within(fm, fm_ref, fm_sc)
    _within(s, s_ref, s_sc)
    dx = ops.fm_bwd(g.to(DEV), s, xd)
    assert dx.shape == (B, F, E)
    _within(dx, dx_ref, dx_sc)
    fm2, s2 = ops.fm_fwd(xd)
    assert torch.equal(fm, fm2) and torch.equal(s, s2) and torch.equal(dx, ops.fm_bwd(g.to(DEV), s, xd))


def test_fm_rejects_unsupported_embed_sizes(ops):
    from mapx.native import MapxError
    for E in (12, 128):
        with pytest.raises(MapxError):
            ops.fm_fwd(torch.zeros(2, 3, E, device=DEV))
    with pytest.raises(MapxError):
        ops.fm_bwd(torch.zeros(2, device=DEV), torch.zeros(2, 6, device=DEV), torch.zeros(2, 3, 6, device=DEV))


def test_fm_product_sum_on_a_column_slice(ops):
    """layers.fm_product_sum on a non-contiguous x3 (the first E columns of a [B, F, 2E] tensor): fm_bwd reads x3
    through a raw pointer, so the autograd wrapper has to hand it the contiguous copy it saved."""
    from mapx import layers
    B, F, E = 33, 23, 16
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(B, F, 2 * E, generator=g)
    gout = torch.randn(B, 1, generator=g)
    fm_ref, _, dx_ref = fm_restate(wide[:, :, :E], gout.view(-1))
    fm_sc, _, dx_sc = fm_scales(wide[:, :, :E], gout.view(-1))
    wd = wide.to(DEV).requires_grad_(True)
    x3 = wd[:, :, :E]
    assert not x3.is_contiguous()
    out = layers.fm_product_sum(x3)
    assert out.shape == (B, 1)
    (out * gout.to(DEV)).sum().backward()
    _within(out.view(-1), fm_ref, fm_sc)
    _within(wd.grad[:, :, :E], dx_ref, dx_sc)
    assert not bool(wd.grad[:, :, E:].any())


# (B, F, V): lane l of a row's 32 sums fields l, l + 32, ...: F > 32 takes the second trip of that loop.
LR_CASES = [
    pytest.param(1, 1, 3, id="B1-F1-V3:31-idle-lanes"),
    pytest.param(7, 23, 1000, id="B7-F23-V1000:avazu-partly-filled-block"),
    pytest.param(64, 39, 5000, id="B64-F39-V5000:criteo-second-trip-for-7-lanes"),
    pytest.param(300, 64, 50, id="B300-F64-V50:second-trip-for-all-lanes-many-blocks"),
    pytest.param(5, 70, 10, id="B5-F70-V10:third-trip"),
]


def lr_inputs(B, F, V):
    g = torch.Generator().manual_seed(B + 17 * F + V)
    return torch.randint(0, V, (B, F), generator=g), torch.randn(V, generator=g)


def lr_restate(ids, w, dtype=torch.float64):
    """out[b] = sum_f w[ids[b, f]]; an id outside [0, V) counts as 0."""
    ok = (ids >= 0) & (ids < w.numel())
    terms = w.to(dtype)[ids.clamp(0, w.numel() - 1)] * ok
    return terms.sum(1), terms.abs().double().sum(1)


@pytest.mark.parametrize("B,F,V", LR_CASES)
def test_lr_sum_matches_float64_torch(ops, B, F, V):
    """Same scaled bound as the FM terms; worst float32-CPU ratio error / bound over LR_CASES: 0.06."""
    ids, w = lr_inputs(B, F, V)
    ref, scale = lr_restate(ids, w)
    assert torch.equal(ref, w.double()[ids].sum(1))
    idd, wdev = ids.to(DEV), w.to(DEV)
    out = ops.lr_sum(idd, wdev, validate=True)
    assert out.shape == (B,)
    _within(out, ref, scale)
    assert torch.equal(out, ops.lr_sum(idd, wdev)) and torch.equal(out, ops.lr_sum(idd, wdev, validate=True))
    # ids out of range: loud with validate, a zero term without; in the first and in the last field
    for bad in (V, -1):
        for f in (0, F - 1):
            ids_bad = ids.clone()
            ids_bad[B // 2, f] = bad
            with pytest.raises(IndexError):
                ops.lr_sum(ids_bad.to(DEV), wdev, validate=True)
            ref_bad, scale_bad = lr_restate(ids_bad, w)
            _within(ops.lr_sum(ids_bad.to(DEV), wdev, validate=False), ref_bad, scale_bad)


# --------------------------------------------------------------------------- segment reduction with the extra scalar
def _skewed_keys(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    k = (torch.rand(n, generator=g) ** 6 * V).long().clamp_(0, V - 1)
    k[: n // 4] = 3                       # a '<mask>'-like hot key spanning many chunks
    return k[torch.randperm(n, generator=g)]


# (n, V, W, group, ld, extra_stride)
SEG_CASES = [
    pytest.param(1, 50, 16, 1, 16, 1, id="n1:single-position"),
    pytest.param(33, 7, 16, 3, 16, 1, id="n33-group3:few-keys-shared-scalar"),
    pytest.param(23 * 64, 1000, 16, 23, 16, 1, id="n1472-group23:deepfm-lr-gradient"),
    pytest.param(5000, 300, 32, 1, 36, 36, id="n5000-W32-ld36-stride36:dp-merge-scalar-column"),
    pytest.param(70001, 300, 16, 39, 20, 1, id="n70001-group39-ld20:runs-over-many-chunks-ragged-last-group"),
    pytest.param(4097, 5, 64, 1, 68, 68, id="n4097-V5-W64-ld68-stride68:five-long-runs"),
    pytest.param(20000, 9_449_445, 4, 25, 4, 1, id="n20000-W4-group25:wide-keys-narrow-rows"),
    # one per lane-group form (tests/row_widths_ref.py), a shared scalar (group > 1) at a stride of its own
    pytest.param(5000, 300, 12, 5, 20, 3, id="n5000-W12-ld20-group5-stride3:4-lanes-one-idle"),
    pytest.param(5000, 300, 24, 7, 24, 2, id="n5000-W24-group7-stride2:8-lanes-two-idle"),
    pytest.param(5000, 300, 40, 3, 48, 5, id="n5000-W40-ld48-group3-stride5:16-lanes-six-idle"),
    pytest.param(5000, 300, 68, 23, 72, 3, id="n5000-W68-ld72-group23-stride3:second-round-of-one-lane"),
    pytest.param(5000, 300, 128, 4, 128, 2, id="n5000-W128-group4-stride2:two-full-rounds"),
]


@pytest.mark.parametrize("n,V,W,group,ld,estride", SEG_CASES)
def test_seg_reduce_rows_extra(ops, n, V, W, group, ld, estride):
    """rows[u] = sum of src[p, :W], scalars[u] = sum of extra[(p // group) * extra_stride] over the positions p of
    key uniq[u].  Bounds: those of test_kernels_gpu.py::test_seg_plan_and_reduce_rows."""
    keys = _skewed_keys(n, V, n)
    g = torch.Generator().manual_seed(n + W)
    src = torch.randn(n, ld, generator=g)
    src_d = src.to(DEV)
    if estride == 1 or group > 1:
        extra = torch.randn(-(-n // group) * estride, generator=g)       # ceil(n / group) scalars, `estride` apart
        extra_d = extra.to(DEV)
    else:                                                       # the scalar is column W of src itself
        assert estride == ld and ld > W
        extra, extra_d = src.reshape(-1)[W:], src_d[:, W]
    terms = extra[(torch.arange(n) // group) * estride].double()
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    U = plan.count()
    uniq_ref, inv = torch.unique(keys, return_inverse=True)
    assert U == uniq_ref.numel()
    rows, scal = ops.seg_reduce_rows_extra(plan, src_d, W, extra_d, group, extra_stride=estride)
    assert rows.shape == (n, W) and scal.shape == (n,)
    s64 = src[:, :W].double()
    ref = torch.zeros(U, W, dtype=torch.float64).index_add_(0, inv, s64)
    scale = torch.zeros(U, W, dtype=torch.float64).index_add_(0, inv, s64.abs())
    err = (_cpu(rows[:U]).double() - ref).abs()
    assert bool((err <= 1e-6 * scale + 1e-6).all()), float(err.max())
    ref1 = torch.zeros(U, dtype=torch.float64).index_add_(0, inv, terms)
    scale1 = torch.zeros(U, dtype=torch.float64).index_add_(0, inv, terms.abs())
    err1 = (_cpu(scal[:U]).double() - ref1).abs()
    assert bool((err1 <= 1e-6 * scale1 + 1e-6).all()), float(err1.max())
    # same inputs -> same bits (the first call took the plan's zeroed owner counter, this one does not)
    rows2, scal2 = ops.seg_reduce_rows_extra(plan, src_d, W, extra_d, group, extra_stride=estride)
    assert torch.equal(rows[:U], rows2[:U]) and torch.equal(scal[:U], scal2[:U])
    # the scalar rides along without disturbing the rows: same summation order as the plain reduction
    plain = ops.seg_reduce_rows(plan, src_d[:, :W].contiguous(), W)
    assert torch.equal(rows[:U], plain[:U])


# --------------------------------------------------------------------------- exchange message pack
def _pack_check(ops, plan, uniq, U, rows0, rows1, maxc, live):
    """keys / rows of ops.pack_sparse against the definition: `live` leading entries, then padding."""
    scale, pad_id = 1.0 / 3.0, -1
    sc = torch.tensor(scale, dtype=torch.float32)
    W0 = rows0.shape[1]
    keys, rows = ops.pack_sparse(plan, rows0.to(DEV), None if rows1 is None else rows1.to(DEV), maxc, scale,
                                 pad_id=pad_id)
    keys, rows = _cpu(keys), _cpu(rows)
    assert keys.shape == (maxc,) and keys.dtype == torch.int32
    assert rows.shape == (maxc, W0 + 4 if rows1 is not None else W0)
    assert torch.equal(keys[:live], uniq[:live].to(torch.int32))
    assert torch.equal(keys[live:], torch.full((maxc - live,), pad_id, dtype=torch.int32))
    assert torch.equal(rows[:live, :W0], rows0[:live] * sc)
    if rows1 is not None:
        assert torch.equal(rows[:live, W0], rows1[:live] * sc)
        assert not bool(rows[:live, W0 + 1:].any())
    assert not bool(rows[live:].any())


@pytest.mark.parametrize("W0", [16, 32, 4, 12, 64, 128])
@pytest.mark.parametrize("with_rows1", [True, False], ids=["rows1", "no-rows1"])
def test_pack_sparse(ops, W0, with_rows1):
    n, V = 3000, 400
    keys = _skewed_keys(n, V, W0)
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    U = plan.count()
    uniq = torch.unique(keys)
    assert U == uniq.numel() and U > 8
    g = torch.Generator().manual_seed(W0)
    rows0 = torch.randn(n, W0, generator=g)
    rows1 = torch.randn(n, generator=g) if with_rows1 else None
    for maxc in (0, 1, U - 1, U, U + 7, 2 * U):       # maxc < n_uniq truncates; maxc > n_uniq pads
        _pack_check(ops, plan, uniq, U, rows0, rows1, maxc, min(U, maxc))
    # fewer gradient rows than unique ids (*n_uniq > cap): entries at and beyond cap are padding
    cap = U - 5
    for maxc in (cap - 1, U + 7):
        _pack_check(ops, plan, uniq, U, rows0[:cap], None if rows1 is None else rows1[:cap], maxc, min(cap, maxc))


@pytest.mark.parametrize("with_rows1", [True, False], ids=["rows1", "no-rows1"])
def test_pack_sparse_of_an_empty_plan(ops, with_rows1):
    plan = ops.SegPlan(torch.empty(0, dtype=torch.int32, device=DEV), 100)
    assert plan.count() == 0
    rows0 = torch.randn(4, 16, generator=torch.Generator().manual_seed(0))
    _pack_check(ops, plan, torch.empty(0, dtype=torch.int64), 0, rows0, rows0[:, 0].clone() if with_rows1 else None,
                5, 0)


# --------------------------------------------------------------------------- CIN outer product, padded row
# (R, F, H): F * H no multiple of 8; R > 8192 makes a block of the forward walk more than one row
@pytest.mark.parametrize("R,F,H", [pytest.param(17 * 16, 23, 23, id="R272-F23-H23:529-columns-padded-to-536"),
                                   pytest.param(8209, 5, 7, id="R8209-F5-H7:35-columns-padded-to-40-row-loop")])
def test_cin_outer_padded_row(ops, R, F, H):
    """cin_outer_fwd(pad_to=8), the form every real step takes: the product exactly, zero padding columns; and
    cin_outer_bwd on a dhad with that padded row stride gives bit for bit what it gives on the unpadded one."""
    g = torch.Generator().manual_seed(R + F * H)
    x0t, xi = torch.randn(R, F, generator=g), torch.randn(R, H, generator=g)
    K, ld = F * H, (F * H + 7) // 8 * 8
    assert ld > K
    x0d, xid = x0t.to(DEV), xi.to(DEV)
    had = ops.cin_outer_fwd(x0d, xid, pad_to=8)
    assert had.shape == (R, ld)
    assert torch.equal(_cpu(had[:, :K]), (x0t[:, :, None] * xi[:, None, :]).reshape(R, K))
    assert not bool(had[:, K:].any())
    assert torch.equal(had[:, :K], ops.cin_outer_fwd(x0d, xid))
    dhad = torch.randn(R, K, generator=g)
    padded = torch.full((R, ld), 7.0)             # the padding columns are not the kernel's to read
    padded[:, :K] = dhad
    outs = []
    for d in (dhad, padded):
        dx0t = torch.full((R, F), 0.5, device=DEV)
        dxi = ops.cin_outer_bwd(d.to(DEV), x0d, xid, dx0t, accumulate_x0=True)
        outs.append((dxi, dx0t))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    d3 = dhad.view(R, F, H).double()
    _close(outs[1][0], (d3 * x0t.double()[:, :, None]).sum(1), rtol=1e-5, atol=1e-5)      # as test_cin_pieces
    _close(outs[1][1], 0.5 + (d3 * xi.double()[:, None, :]).sum(2), rtol=1e-5, atol=1e-5)
