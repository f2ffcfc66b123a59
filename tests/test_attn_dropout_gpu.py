"""The dropout forms of the AutoInt attention core (csrc/attn.hip: attn_drop_*; reference layers.py:740-742 on the
probabilities and :901-904 on the heads' output) at kernel and layer level.

Every parity test builds seeded inputs on the CPU, exports the two keep masks that the kernels draw
(ops.attn_dropout_masks: the same device functions), restates the operation in float64 torch with those masks and
compares.  Tolerances are those of test_backbone_kernels_gpu.py (P_TOL, O_TOL, GRAD_TOL).  The restatements take a
dtype; evaluated in float32 on the CPU with seeded Bernoulli(1-p) masks (five draws per case) and plain randn inputs,
the worst ratios error / (rtol * |ref| + atol) over the cases were, at p = 0.5 (values grow by up to 1 / (1-p)^2 = 4):
  kernel level  P 0.10, O 0.17, dQ 0.21, dK 0.16, dV 0.10   (p = 0.1: P 0.10, O 0.15, dQ 0.17, dK 0.14, dV 0.04)
  layer level   output 0.02, dX 0.01, dW_q 0.03, dW_k 0.02, dW_v 0.04, dW_res 0.05   (p = 0.1, the rate tested)
so the inputs keep unit variance and no tolerance is widened."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
P_TOL = dict(rtol=1e-5, atol=1e-6)
O_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=2e-5)
SEED, OFF_P, OFF_O = 1234, (17 << 36) + 5, (18 << 36) + 5

# (G, F, A, scaled).  F <= 32: attn_drop_*_kernel<2>, two groups per wave; F >= 33: attn_drop_*_kernel<1>.
CASES = [
    pytest.param(7, 23, 12, 1, id="G7-F23-A12-scaled:odd-G-two-per-wave-F-not-multiple-of-4"),
    pytest.param(1, 5, 1, 1, id="G1-F5-A1-scaled:empty-upper-half-wave-A1"),
    pytest.param(6, 32, 16, 0, id="G6-F32-A16-unscaled:last-F-of-two-per-wave"),
    pytest.param(5, 33, 16, 1, id="G5-F33-A16-scaled:first-F-of-one-per-wave"),
    pytest.param(4, 25, 7, 0, id="G4-F25-A7-unscaled:partial-last-O-mask-draw"),
    pytest.param(3, 64, 64, 1, id="G3-F64-A64-scaled:largest-lds"),
]


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _cpu(x):
    return x.detach().cpu()


def _ratio(got, want, rtol, atol):
    """max of error / (rtol * |want| + atol): assert_allclose's criterion as one number."""
    got, want = _cpu(got).double().reshape(-1), want.detach().double().reshape(-1)
    return float(((got - want).abs() / (rtol * want.abs() + atol)).max())


def _close(what, got, want, rtol, atol):
    print(f"{what}: error / bound = {_ratio(got, want, rtol, atol):.3f}")
    np.testing.assert_allclose(_cpu(got).double().numpy().reshape(-1), want.detach().numpy().reshape(-1), rtol=rtol,
                               atol=atol, err_msg=what)


def attn_inputs(G, F, A):
    """q, k, v, dO as float32 [G*F*A]: group g is the g-th run of F*A consecutive floats."""
    g = torch.Generator().manual_seed(1000 * G + 10 * F + A)
    return [torch.randn(G * F * A, generator=g) for _ in range(4)]


def drop_restate(q, k, v, d_o, keep_p, keep_o, G, F, A, scaled, p, dtype=torch.float64):
    """P = softmax(Q K^T (/ sqrt(A))), P~ = P m_p / (1-p), O = (P~ V) m_o / (1-p) on [G, F, A] views; gradients by
    autograd of (O * dO).sum().  -> P (undropped), O, dQ, dK, dV."""
    q, k, v = (t.to(dtype).view(G, F, A).requires_grad_(True) for t in (q, k, v))
    s = q @ k.transpose(1, 2)
    if scaled:
        s = s / A ** 0.5
    pr = torch.softmax(s, dim=-1)
    o = ((pr * keep_p.to(dtype) / (1 - p)) @ v) * keep_o.to(dtype) / (1 - p)
    (o * d_o.to(dtype).view(G, F, A)).sum().backward()
    return pr.detach(), o.detach().reshape(-1), q.grad.reshape(-1), k.grad.reshape(-1), v.grad.reshape(-1)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("G,F,A,scaled", CASES)
def test_forward_and_backward_match_float64_torch_with_the_exported_masks(ops, G, F, A, scaled, p):
    q, k, v, d_o = attn_inputs(G, F, A)
    keep_p, keep_o = ops.attn_dropout_masks(G, F, A, p, SEED, OFF_P, OFF_O)
    assert keep_p.shape == (G, F, F) and keep_o.shape == (G, F, A) and keep_p.dtype == keep_o.dtype == torch.uint8
    assert int(keep_p.max()) <= 1 and int(keep_o.max()) <= 1
    p_ref, o_ref, dq_ref, dk_ref, dv_ref = drop_restate(q, k, v, d_o, _cpu(keep_p), _cpu(keep_o), G, F, A, scaled, p)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, d_o))
    o, probs = ops.attn_drop_fwd(qd, kd, vd, G, F, A, scaled, p, SEED, OFF_P, OFF_O)
    assert probs.shape == (G, F, F) and o.shape == qd.shape
    _close("P", probs, p_ref, **P_TOL)
    _close("O", o, o_ref, **O_TOL)
    # a dropped output is an exact zero, and the stored probabilities are the undropped ones
    assert bool((o.view(G, F, A)[keep_o == 0] == 0).all())
    rows = _cpu(probs).double().sum(-1)
    assert float((rows - 1).abs().max()) <= 1e-6
    dq, dk, dv = ops.attn_drop_bwd(qd, kd, vd, probs, dod, G, F, A, scaled, p, SEED, OFF_P, OFF_O)
    _close("dQ", dq, dq_ref, **GRAD_TOL)
    _close("dK", dk, dk_ref, **GRAD_TOL)
    _close("dV", dv, dv_ref, **GRAD_TOL)


def test_mask_statistics_and_independence(ops):
    G, F, A, p = 96, 23, 12, 0.1
    a, b = OFF_P, OFF_O
    kp, ko = ops.attn_dropout_masks(G, F, A, p, SEED, a, b)
    for keep in (kp, ko):
        n = keep.numel()
        dropped = n - int(keep.sum())
        assert abs(dropped - n * p) <= 5 * (n * p * (1 - p)) ** 0.5, (dropped, n * p)
        assert sorted(torch.unique(keep).tolist()) == [0, 1]
    # each mask follows its own offset only
    kp2, ko2 = ops.attn_dropout_masks(G, F, A, p, SEED, a + 1, b)
    assert not torch.equal(kp2, kp) and torch.equal(ko2, ko)
    kp3, ko3 = ops.attn_dropout_masks(G, F, A, p, SEED, a, b + 1)
    assert torch.equal(kp3, kp) and not torch.equal(ko3, ko)
    # swapped offsets: the P mask is drawn from offset_p, not from offset_o
    kp4, ko4 = ops.attn_dropout_masks(G, F, A, p, SEED, b, a)
    assert not torch.equal(kp4, kp) and not torch.equal(ko4, ko)
    # another seed, another pair of masks
    kp5, ko5 = ops.attn_dropout_masks(G, F, A, p, SEED + 1, a, b)
    assert not torch.equal(kp5, kp) and not torch.equal(ko5, ko)


def test_a_mask_does_not_depend_on_the_grid(ops):
    """Group g's masks are the same whether g is in the lower or the upper half of a wave, and however many groups the
    launch has: the masks of the first 3 groups of a 7-group launch are those of a 3-group launch; O likewise."""
    F, A, p = 23, 12, 0.5
    kp7, ko7 = ops.attn_dropout_masks(7, F, A, p, SEED, OFF_P, OFF_O)
    kp3, ko3 = ops.attn_dropout_masks(3, F, A, p, SEED, OFF_P, OFF_O)
    assert torch.equal(kp7[:3], kp3) and torch.equal(ko7[:3], ko3)
    q, k, v, _ = (t.to(DEV) for t in attn_inputs(7, F, A))
    o7, _ = ops.attn_drop_fwd(q, k, v, 7, F, A, 1, p, SEED, OFF_P, OFF_O)
    n = 3 * F * A
    o3, _ = ops.attn_drop_fwd(q[:n].clone(), k[:n].clone(), v[:n].clone(), 3, F, A, 1, p, SEED, OFF_P, OFF_O)
    assert torch.equal(o7[:n], o3)


def test_offset_dev_is_added_to_both_offsets(ops):
    G, F, A, p = 7, 23, 12, 0.1
    dev = torch.tensor([7], dtype=torch.int32, device=DEV)
    kp, ko = ops.attn_dropout_masks(G, F, A, p, SEED, OFF_P, OFF_O, dev)
    kp2, ko2 = ops.attn_dropout_masks(G, F, A, p, SEED, OFF_P + 7, OFF_O + 7)
    assert torch.equal(kp, kp2) and torch.equal(ko, ko2)
    q, k, v, d_o = (t.to(DEV) for t in attn_inputs(G, F, A))
    o, pr = ops.attn_drop_fwd(q, k, v, G, F, A, 1, p, SEED, OFF_P, OFF_O, dev)
    o2, pr2 = ops.attn_drop_fwd(q, k, v, G, F, A, 1, p, SEED, OFF_P + 7, OFF_O + 7)
    assert torch.equal(o, o2) and torch.equal(pr, pr2)
    for x, y in zip(ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, 1, p, SEED, OFF_P, OFF_O, dev),
                    ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, 1, p, SEED, OFF_P + 7, OFF_O + 7)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("F", [5, 23, 33])
def test_the_p_mask_is_the_transformer_cores_mask_for_the_same_draws(ops, F):
    """Both cores keep key 4c+e of query row `row` iff element e of the draw at counter row * ceil(F/4) + c is kept:
    for one (seed, offset) the Transformer core's mask of B*H groups is the AutoInt P mask of G = B*H groups."""
    B, H, A, p = 3, 2, 12, 0.3
    dev = torch.tensor([5], dtype=torch.int32, device=DEV)
    for offset_dev in (None, dev):
        mha = ops.mha_dropout_mask(B, F, H, p, SEED, OFF_P, offset_dev)
        kp, _ = ops.attn_dropout_masks(B * H, F, A, p, SEED, OFF_P, OFF_O, offset_dev)
        assert mha.shape == kp.shape == (B * H, F, F)
        assert 0 < int(kp.sum()) < kp.numel()
        assert torch.equal(mha, kp)


@pytest.mark.parametrize("G,F,A,scaled", [(7, 23, 12, 1), (5, 33, 16, 0)])
def test_rate_zero_through_the_new_entries_is_the_plain_core_bitwise(ops, G, F, A, scaled):
    q, k, v, d_o = (t.to(DEV) for t in attn_inputs(G, F, A))
    o, pr = ops.attn_fwd(q, k, v, G, F, A, scaled)
    o2, pr2 = ops.attn_drop_fwd(q, k, v, G, F, A, scaled, 0.0, SEED, OFF_P, OFF_O)
    assert torch.equal(o, o2) and torch.equal(pr, pr2)
    for x, y in zip(ops.attn_bwd(q, k, v, pr, d_o, G, F, A, scaled),
                    ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, scaled, 0.0, SEED, OFF_P, OFF_O)):
        assert torch.equal(x, y)
    kp, ko = ops.attn_dropout_masks(G, F, A, 0.0, SEED, OFF_P, OFF_O)
    assert bool(kp.all()) and bool(ko.all())


def test_two_runs_are_bitwise_equal(ops):
    G, F, A, p = 1001, 23, 16, 0.1
    q, k, v, d_o = (t.to(DEV) for t in attn_inputs(G, F, A))
    o, pr = ops.attn_drop_fwd(q, k, v, G, F, A, 1, p, SEED, OFF_P, OFF_O)
    o2, pr2 = ops.attn_drop_fwd(q, k, v, G, F, A, 1, p, SEED, OFF_P, OFF_O)
    assert torch.equal(o, o2) and torch.equal(pr, pr2)
    g1 = ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, 1, p, SEED, OFF_P, OFF_O)
    g2 = ops.attn_drop_bwd(q, k, v, pr, d_o, G, F, A, 1, p, SEED, OFF_P, OFF_O)
    for x, y in zip(g1, g2):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # the last group (alone in its wave: G is odd) is covered
    assert float(o.view(G, F, A)[-1].abs().sum()) > 0 and float(g1[0].view(G, F, A)[-1].abs().sum()) > 0


def test_unsupported_arguments_are_rejected(ops):
    from mapx.native import MapxError
    for G, F, A, p in [(2, 65, 8, 0.1), (2, 8, 65, 0.1), (2, 8, 8, 1.0), (2, 8, 8, -0.1), (2, 0, 8, 0.1)]:
        x = torch.zeros(G * max(F, 1) * A, device=DEV)
        pr = torch.zeros(G, max(F, 1), max(F, 1), device=DEV)
        with pytest.raises(MapxError):
            ops.attn_drop_fwd(x, x, x, G, F, A, 1, p, SEED, OFF_P, OFF_O)
        with pytest.raises(MapxError):
            ops.attn_drop_bwd(x, x, x, pr, x, G, F, A, 1, p, SEED, OFF_P, OFF_O)
        with pytest.raises(MapxError):
            ops.attn_dropout_masks(G, F, A, p, SEED, OFF_P, OFF_O)
    # no groups: nothing to do
    e = torch.zeros(0, device=DEV)
    o, pr = ops.attn_drop_fwd(e, e, e, 0, 8, 8, 1, 0.1, SEED, OFF_P, OFF_O)
    assert o.numel() == 0 and pr.numel() == 0


# --------------------------------------------------------------------------- layer level
def layer_restate(x, wq, wk, wv, wres, keep_p, keep_o, heads, A, res_conn, scaled, p, r, relu_mask=None,
                  dtype=torch.float64):
    """Reference layers.py:876-908 (MultiHeadAttention.forward as AutoInt builds it: align_to="output", no layer
    norm, no attention mask) with the two dropouts' keep masks given: keep_p [B*H, F, F], keep_o [B*H, F, A].
    `relu_mask`: the ReLU pattern to use instead of the restatement's own.  -> (pre-activation, output, gradients of
    (output * r).sum() with respect to x, W_q, W_k, W_v and W_res)."""
    x = x.to(dtype).requires_grad_(True)
    ws = [None if w is None else w.to(dtype).requires_grad_(True) for w in (wq, wk, wv, wres)]
    B = x.shape[0]
    residual = x
    query, key, value = x @ ws[0].T, x @ ws[1].T, x @ ws[2].T
    query = query.view(B * heads, -1, A)
    key = key.view(B * heads, -1, A)
    value = value.view(B * heads, -1, A)
    attention = torch.bmm(query, key.transpose(1, 2))
    if scaled:
        attention = attention / A ** 0.5
    attention = torch.softmax(attention, dim=2)
    attention = attention * keep_p.to(dtype) / (1 - p)                           # ScaledDotProductAttention.dropout
    output = torch.bmm(attention, value)
    output = output.view(B, -1, heads * A)
    if ws[3] is not None:
        residual = residual @ ws[3].T
    output = output * keep_o.to(dtype).view(B, -1, heads * A) / (1 - p)          # MultiHeadAttention.dropout
    if res_conn:
        output = output + residual
    pre = output
    output = output.relu() if relu_mask is None else output * relu_mask.to(dtype)
    (output * r.to(dtype)).sum().backward()
    return pre.detach(), output.detach(), [x.grad] + [None if w is None else w.grad for w in ws]


LAYER_FORMS = [
    pytest.param(16, True, id="width16-no-W_res-residual"),
    pytest.param(12, True, id="width12-W_res-residual"),
    pytest.param(12, False, id="width12-no-residual"),
]


def _layer(din, res_conn, rate, like=None):
    from mapx.layers import MultiHeadSelfAttention
    torch.manual_seed(21)
    m = MultiHeadSelfAttention(din, 8, 2, dropout_rate=rate, use_residual=res_conn, use_scale=True).to(DEV)
    if like is not None:
        m.load_state_dict(like.state_dict())
    return m


@pytest.mark.parametrize("din,res_conn", LAYER_FORMS)
def test_layer_matches_float64_restatement_of_the_reference(ops, din, res_conn):
    B, F, heads, A, p = 7, 23, 2, 8, 0.1
    m = _layer(din, res_conn, p)
    m.train()
    g = torch.Generator().manual_seed(100 + din)
    x = torch.randn(B, F, din, generator=g)
    r = torch.randn(B, F, heads * A, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out = m(xd)
    (out * r.to(DEV)).sum().backward()
    # the masks of THIS call: an untrained site counts its calls into the offset (HipDropout.forward, MhaDropout.philox)
    sp, so = m.dot_product_attention.dropout, m.dropout
    assert sp.site != so.site and sp._calls == so._calls == 1 and sp.seed == so.seed
    offs = [(s.rank << 48) + ((16 + s.site) << 36) + s._calls for s in (sp, so)]
    keep_p, keep_o = ops.attn_dropout_masks(B * heads, F, A, p, sp.seed, offs[0], offs[1])
    assert 0 < int(keep_p.sum()) < keep_p.numel() and 0 < int(keep_o.sum()) < keep_o.numel()
    ws = [_cpu(m.W_q.weight), _cpu(m.W_k.weight), _cpu(m.W_v.weight), None if m.W_res is None else _cpu(m.W_res.weight)]
    assert (ws[3] is not None) == (din != heads * A)
    # a unit whose pre-activation is zero to fp32 rounding may sit on the other side of the kink than in float64: the
    # restatement runs on the layer's own ReLU pattern after checking that the patterns differ only at such units
    pattern = _cpu(out) > 0
    pre, _, _ = layer_restate(x, *ws, _cpu(keep_p), _cpu(keep_o), heads, A, res_conn, True, p, r)
    differ = pattern != (pre > 0)
    if bool(differ.any()):
        assert float(pre[differ].abs().max()) <= 1e-5 * float(pre.abs().max()), "a unit off the kink flipped"
    _, out_ref, grads_ref = layer_restate(x, *ws, _cpu(keep_p), _cpu(keep_o), heads, A, res_conn, True, p, r,
                                          relu_mask=pattern)
    _close("output", out, out_ref, **O_TOL)
    got = [xd.grad, m.W_q.weight.grad, m.W_k.weight.grad, m.W_v.weight.grad,
           None if m.W_res is None or not res_conn else m.W_res.weight.grad]
    for name, a, b in zip(("dX", "dW_q", "dW_k", "dW_v", "dW_res"), got, grads_ref):
        if a is None:                                     # no W_res, or no residual branch for it to act in
            assert name == "dW_res" and b is None
            continue
        _close(name, a, b, **GRAD_TOL)
    # dropout did something: the same layer without it gives another output
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(xd), out)


@pytest.mark.parametrize("din,res_conn", LAYER_FORMS)
def test_layer_in_eval_mode_equals_the_rate_zero_layer_bitwise(din, res_conn):
    m = _layer(din, res_conn, 0.1)
    m0 = _layer(din, res_conn, 0.0, like=m)
    assert list(m.state_dict()) == list(m0.state_dict())
    x = torch.randn(7, 23, din, generator=torch.Generator().manual_seed(3)).to(DEV)
    m.eval()
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m(x), m0(x))
    m.train()
    with torch.no_grad():
        assert not torch.equal(m(x), m0(x))


def test_layer_masks_follow_the_device_step_counter():
    """Inside a Trainer the sites read the optimizer's device-side counter: the same input at counter 3, 4 and 3 again
    gives an output, another one, and the first one bit for bit (what lets a captured step replay with fresh masks)."""
    m = _layer(16, True, 0.1)
    m.train()
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i, site in enumerate((m.dot_product_attention.dropout, m.dropout)):
        site.step_counter, site.seed, site.rank, site.site = counter, 11, 0, i + 1
    x = torch.randn(7, 23, 16, generator=torch.Generator().manual_seed(4)).to(DEV)
    outs = []
    with torch.no_grad():
        for step in (3, 4, 3):
            counter.fill_(step)
            outs.append(m(x).clone())
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
