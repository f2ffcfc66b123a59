"""The bf16 I/O forms of csrc/fgcnn.hip at the stage shapes of tests/test_fgcnn_kernels_gpu.py (B = 5 / 67,
kh > H, odd / even H with ps 2 / 3, the 105 KB backward stage, E = 4 and 16), on bf16-representable inputs.

Forward.  z<bf16> is the fp32 kernel's z rounded once, bit for bit (same accumulation order).  Everything downstream is
compared with a float64 reference CONTINUED FROM THE DEVICE'S OWN z read back, so that a one-ulp difference in z cannot
flip a ReLU or a pooling winner; the ambiguity margins of the fp32 module (MARGIN = 1e-4) are asserted on that reference
and the inputs are repaired and the stage re-run while they fail, as its stage_case does.

Tolerances (the rule of DESIGN §4.8): outputs that stay fp32 — {mean, rstd}, the running statistics after one and two
steps, dW, db, dgamma, dbeta — are held to the fp32 module's own bounds (FWD_TOL, GRAD_TOL, DW_TOL, DB_TOL); bf16 outputs
(y, dx, the inner products and their dx) get those bounds + 2^-8 |ref|, half a bf16 ulp.  idx is equal exactly.  db
within DB_TOL is the check that the statistics are those of the STORED z: statistics of the fp32 accumulator would leave
sum(xhat) = O(2^-9 * B*H*E) and with it a conv-bias gradient far outside an fp32-level bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_fgcnn_kernels_gpu import (DB_TOL, DW_TOL, EPS, FWD_TOL, GRAD_TOL, IDS, IP_CASES, MARGIN, MOMENTUM, STAGES,
                                    _window_gap, ambiguous, close, grad_close, stage_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HALF_ULP = 2.0 ** -8


def rb(t):
    """float64 -> the nearest bf16 value, as float64."""
    return t.float().to(BF).double()


def dev16(t):
    return t.float().to(BF).to(DEV).contiguous()


def dev32(t):
    return t.float().to(DEV).contiguous()


def half_close(got, want, tol, what):
    assert got.dtype == BF, what
    close(got.float(), want, rtol=tol["rtol"] + HALF_ULP, atol=tol["atol"], what=what)


def continue_from(c, z, training=True, rm=None, rv=None):
    """float64: batch norm -> act -> pool of the given z -> (u, a, y)."""
    u = F.batch_norm(z, rm, rv, c["ga"], c["be"], training, MOMENTUM, EPS)
    a = torch.tanh(u) if c["act"] == "tanh" else torch.relu(u)
    return u, a, F.max_pool2d(a, (c["ps"], 1), padding=(z.shape[2] % c["ps"], 0))


def forward(c, x64, rm=None, rv=None, nbt=None):
    from mapx import ops
    z, part = ops.fgcnn_conv_fwd(dev16(x64), dev32(c["w"]), dev32(c["b"]))
    stats = ops.fgcnn_bn_stats(part, z.shape[2], z.shape[3], rm, rv, nbt)
    y, idx = ops.fgcnn_pool_fwd(z, dev32(c["ga"]), dev32(c["be"]), c["ps"], c["act"], stats=stats)
    return z, stats, y, idx


@functools.lru_cache(maxsize=None)
def bf_case(case):
    """The stage on bf16-representable x and dy: the device's forward, its z read back, and the float64 reference
    continued from that z (forward and every gradient).  Built once per case, shared and left unchanged."""
    from mapx import ops
    base = stage_case(*case)
    c = {k: base[k] for k in ("w", "b", "ga", "be", "ps", "act")}
    g = torch.Generator().manual_seed(77 + case[0] + case[3])
    x = rb(base["x"])
    for _ in range(50):
        z, stats, y, idx = forward(c, x)
        z64 = z.float().cpu().double()
        u, a, _ = continue_from(c, z64)
        bad = ambiguous(c, u, a)
        if not bad.any():
            break
        x = rb(x + bad[:, None].double() * 0.05 * torch.randn(x.shape, generator=g, dtype=torch.float64))
    c.update(x=x, r=rb(base["r"]))
    zl = z64.clone().requires_grad_(True)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("ga", "be")}
    u, a, yr = continue_from(dict(c, **leaves), zl)
    (yr * c["r"]).sum().backward()
    conv = {k: c[k].clone().requires_grad_(True) for k in ("x", "w", "b")}
    kh = c["w"].shape[2]
    F.conv2d(conv["x"], conv["w"], conv["b"], padding=((kh - 1) // 2, 0)).backward(zl.grad)
    _, flat = F.max_pool2d(a.detach(), (c["ps"], 1), padding=(z64.shape[2] % c["ps"], 0), return_indices=True)
    Hp, pad = yr.shape[2], z64.shape[2] % c["ps"]
    k_ref = flat // z64.shape[3] - (torch.arange(Hp).view(1, 1, -1, 1) * c["ps"] - pad)
    grads = dict(ga=leaves["ga"].grad, be=leaves["be"].grad, **{k: v.grad for k, v in conv.items()})
    c.update(z=z64, u=u.detach(), a=a.detach(), y=yr.detach(), k=k_ref, grads=grads,
             dev=dict(z=z, stats=stats, y=y, idx=idx))
    return c


def backward(c):
    from mapx import ops
    d = c["dev"]
    return ops.fgcnn_bwd(dev16(c["r"]), d["idx"], d["z"], dev16(c["x"]), dev32(c["w"]), d["stats"], dev32(c["ga"]),
                         dev32(c["be"]), c["ps"], c["act"])


@pytest.mark.parametrize("case", STAGES, ids=IDS)
def test_stage_forward_and_every_gradient(case):
    from mapx import ops
    c = bf_case(case)
    d = c["dev"]
    # the reference continued from the device's z is unambiguous at the fp32 module's margins
    assert not ambiguous(c, c["u"], c["a"]).any()
    if c["act"] == "relu":
        assert float(c["u"].abs().min()) >= MARGIN
    assert float(_window_gap(c["a"], c["ps"], c["act"] == "relu")[0].min()) >= MARGIN
    # z: the fp32 kernel's, rounded once
    z32, _ = ops.fgcnn_conv_fwd(dev32(c["x"]), dev32(c["w"]), dev32(c["b"]))
    assert d["z"].dtype == BF and torch.equal(d["z"], z32.to(BF))
    # the statistics are those of the stored z
    close(d["stats"][:, 0], c["z"].mean((0, 2, 3)), what="batch mean", **FWD_TOL)
    close(d["stats"][:, 1], (c["z"].var((0, 2, 3), unbiased=False) + EPS).rsqrt(), rtol=1e-5, atol=0, what="batch rstd")
    assert d["stats"].dtype == torch.float32 and d["idx"].dtype == torch.uint8
    half_close(d["y"], c["y"], FWD_TOL, "pooled")
    assert tuple(d["y"].shape) == tuple(c["y"].shape)
    assert torch.equal(d["idx"].cpu().long(), c["k"])
    dx, dw, db, dga, dbe = backward(c)
    gr = c["grads"]
    assert all(t.dtype == torch.float32 for t in (dw, db, dga, dbe))
    err = (dx.float().cpu().double() - gr["x"]).abs()
    bound = (GRAD_TOL["rtol"] + HALF_ULP) * gr["x"].abs() + GRAD_TOL["atol"]
    print(f"dx: worst error / bound {float((err / bound).max()):.3f}, largest error {float(err.max()):.3e}")
    half_close(dx, gr["x"], GRAD_TOL, "dx")
    grad_close(dga, gr["ga"], "dga")
    grad_close(dbe, gr["be"], "dbe")
    grad_close(dw.view(gr["w"].shape), gr["w"], "dw", **DW_TOL)
    assert float(gr["b"].abs().max()) < 1e-9           # zero in exact arithmetic
    grad_close(db, gr["b"], "db", **DB_TOL)


@pytest.mark.parametrize("case", [STAGES[1], STAGES[2], STAGES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_running_statistics_after_one_and_two_steps(case):
    """The running statistics move by momentum 0.1 with the unbiased variance OF THE STORED z; the counter counts."""
    c = bf_case(case)
    C = c["w"].shape[0]
    g = torch.Generator().manual_seed(5)
    rm64 = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    rv64 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    rm, rv, nbt = dev32(rm64), dev32(rv64), torch.zeros((), dtype=torch.int64, device=DEV)
    for step, x in enumerate((c["x"], rb(c["x"] * 0.7 + 0.3)), start=1):
        z, _, _, _ = forward(c, x, rm, rv, nbt)
        continue_from(c, z.float().cpu().double(), rm=rm64, rv=rv64)       # (F.batch_norm moves rm64 / rv64 in place)
        close(rm, rm64, rtol=1e-5, atol=1e-6, what=f"running_mean after step {step}")
        close(rv, rv64, rtol=1e-5, atol=1e-6, what=f"running_var after step {step}")
        assert int(nbt) == step


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("case", [STAGES[1], STAGES[2], STAGES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_eval_uses_the_running_statistics_and_leaves_them_alone(case, B):
    """part == NULL, the running statistics, no saved argmax."""
    from mapx import ops
    c = bf_case(case)
    C = c["w"].shape[0]
    g = torch.Generator().manual_seed(6)
    rm64 = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    rv64 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    rm, rv, nbt = dev32(rm64), dev32(rv64), torch.full((), 3, dtype=torch.int64, device=DEV)
    before = (rm.clone(), rv.clone(), nbt.clone())
    x = c["x"][:B]
    z, part = ops.fgcnn_conv_fwd(dev16(x), dev32(c["w"]), dev32(c["b"]), stats=False)
    assert part is None and z.dtype == BF
    z32, _ = ops.fgcnn_conv_fwd(dev32(x), dev32(c["w"]), dev32(c["b"]), stats=False)
    assert torch.equal(z, z32.to(BF))
    y, idx = ops.fgcnn_pool_fwd(z, dev32(c["ga"]), dev32(c["be"]), c["ps"], c["act"], running_mean=rm, running_var=rv,
                                save=False)
    assert idx is None
    _, _, y_ref = continue_from(c, z.float().cpu().double(), training=False, rm=rm64.clone(), rv=rv64.clone())
    half_close(y, y_ref, FWD_TOL, "eval pooled")
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and torch.equal(nbt, before[2])


def test_module_passes_bf16_through_and_eval_leaves_the_buffers():
    """layers.FGCNNBlock on a bf16 input: bf16 out, bf16 dx, fp32 parameter gradients; eval leaves every buffer."""
    from mapx.layers import FGCNNBlock
    torch.manual_seed(0)
    blk = FGCNNBlock(7, 8, [3, 2], [3, 3], [2, 2], [2, 1], activation="tanh").to(DEV)
    x = torch.randn(5, 1, 7, 8, device=DEV).to(BF).requires_grad_(True)
    blk.train()
    out = blk(x)
    assert tuple(out.shape) == (5, 4 * 2 + 2 * 1, 8) and out.dtype == BF
    out.float().sum().backward()
    assert x.grad is not None and x.grad.dtype == BF
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in blk.parameters())
    assert int(blk.conv_layers[0]["1"].num_batches_tracked) == 1
    blk.eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    with torch.no_grad():
        assert blk(x.detach()[:1]).dtype == BF
    for k, v in blk.state_dict().items():
        assert torch.equal(v, before[k]), k


# --------------------------------------------------------------------------- inner product
# the fp32 module's cases, and the fixtures' T = 58 (T(T-1)/2 = 1653: odd, so the output rows are 2-byte aligned) with the
# gradient read in place from a wider matrix at an odd column offset and an odd pitch
IP_SLICED = (5, 58, 16)


@functools.lru_cache(maxsize=None)
def ip_case(B, T, E):
    g = torch.Generator().manual_seed(B + T + E)
    x = rb(torch.randn(B, T, E, generator=g, dtype=torch.float64)).requires_grad_(True)
    mask = torch.triu(torch.ones(T, T), 1).bool()
    out = torch.masked_select(torch.bmm(x, x.transpose(1, 2)), mask).view(B, -1)
    r = rb(torch.randn(out.shape, generator=g, dtype=torch.float64))
    (out * r).sum().backward()
    return x.detach(), out.detach(), r, x.grad


@pytest.mark.parametrize("B,T,E", IP_CASES + [IP_SLICED])
def test_inner_product_forward_and_gradient(B, T, E):
    from mapx import ops
    x, out_ref, r, dx_ref = ip_case(B, T, E)
    P = T * (T - 1) // 2
    out = ops.inner_product_fwd(dev16(x))
    assert tuple(out.shape) == (B, P)
    half_close(out, out_ref, FWD_TOL, "inner products")
    assert torch.equal(out, ops.inner_product_fwd(dev32(x)).to(BF))          # the fp32 kernel's output rounded once
    g = dev16(r)
    if (B, T, E) == IP_SLICED:
        wide = torch.full((B, 1 + T * E + P + 3), float("nan"), dtype=BF, device=DEV)
        g = wide[:, 1 + T * E:1 + T * E + P]
        g.copy_(dev16(r))
        assert g.stride(0) % 2 == 1 and g.storage_offset() % 2 == 1 and not g.is_contiguous()
    dx = ops.inner_product_bwd(g, dev16(x))
    half_close(dx, dx_ref, GRAD_TOL, "dx")
    assert torch.equal(dx, ops.inner_product_bwd(dev32(r), dev32(x)).to(BF))


def test_mixed_element_types_are_refused():
    from mapx import ops
    z16, z32 = (lambda *s: torch.zeros(*s, device=DEV, dtype=BF)), (lambda *s: torch.zeros(*s, device=DEV))
    with pytest.raises(TypeError):
        ops.fgcnn_conv_fwd(z16(2, 1, 5, 8), z16(2, 1, 3, 1), z32(2))          # the conv weights are the fp32 masters
    with pytest.raises(TypeError):
        ops.inner_product_bwd(z32(2, 3), z16(2, 3, 8))
    with pytest.raises(TypeError):
        ops.fgcnn_bwd(z32(2, 2, 3, 8), torch.zeros(2, 2, 3, 8, dtype=torch.uint8, device=DEV), z16(2, 2, 5, 8),
                      z16(2, 1, 5, 8), z32(2, 1, 3, 1), z32(2, 2), z32(2), z32(2), 2, "tanh")


@pytest.mark.parametrize("case", [STAGES[3], STAGES[4]], ids=[IDS[3], IDS[4]])
def test_backward_is_bitwise_deterministic(case):
    from mapx import ops
    c = bf_case(case)
    a, b = backward(c), backward(c)
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), i
    x, _, r, _ = ip_case(5, 153, 16)
    outs = [(ops.inner_product_fwd(dev16(x)), ops.inner_product_bwd(dev16(r), dev16(x))) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
