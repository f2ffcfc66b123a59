"""csrc/fgcnn.hip stage by stage against float64 torch (F.conv2d, F.batch_norm in training mode, F.max_pool2d,
torch.bmm + the strict upper-triangle mask): forward and every gradient, the running-statistic update, eval mode,
refused shapes and run-to-run determinism, at the smallest shapes that can still go wrong.

Tolerances are those of tests/test_mha_gpu.py / tests/test_backbone_kernels_gpu.py: forward rtol 1e-5, atol 1e-5;
gradients rtol 1e-4, atol 2e-5 (GRAD_TOL), flat, for dx, dgamma, dbeta and the inner product's dx.  fp32 CPU torch
measured against the float64 reference on these very inputs stays at or below 0.06 of that bound for them at every
case, B = 5 included (the batch-norm backward at B = 5: 0.03; the inner product's dx: 0.17 at T = 153), so they need
nothing wider.  Two gradients sum
B*H*E products and do need more; each gets rtol 1e-4 and an atol of 4 x the fp32 CPU torch error measured here:
  dW: fp32 torch misses GRAD_TOL by 2.05 x at 67-4-2-12-7-3-16-relu, absolute error 1.34e-4 (max |dW| 162)
      -> atol 4 x 1.34e-4 = 5.4e-4;
  db: batch norm removes the channel mean, so this gradient is ZERO in exact arithmetic (1e-13 in float64) and an fp32
      implementation returns the rounding of the sum; fp32 torch's largest error is 9.16e-5 at 67-1-3-39-3-3-16-tanh
      (4.6 x GRAD_TOL) -> atol 4 x 9.16e-5 = 3.7e-4.
The test prints each gradient's worst error / bound before it asserts.

relu and the pooling are ambiguous where a pre-activation is zero or a window's two largest values are equal to
rounding: every case's inputs are repaired until no pre-activation of the float64 reference lies within 1e-4 of zero
(relu) and no window's largest value (a positive one under relu: windows whose values are all zero have one output and
one gradient whichever wins) is within 1e-4 of its runner-up, and the tests assert that on the inputs they use."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 1e-4
FWD_TOL = dict(rtol=1e-5, atol=1e-5)
EPS, MOMENTUM = 1e-5, 0.1

# B, Cin, Cout, H, kh, ps, E, act: every B / channel pair / H / kh / E of the list in the module's purpose; kh > H at
# H = 2, 3; ps = 2 with H even (2, 12) and odd (3, 7, 39); ps = 3 with H % 3 = 0 (12, 39) and 1 (7)
STAGES = [
    (5, 1, 3, 2, 3, 2, 4, "tanh"),
    (5, 1, 3, 3, 7, 2, 16, "relu"),
    (67, 4, 2, 7, 3, 3, 4, "tanh"),
    (67, 4, 2, 12, 7, 3, 16, "relu"),
    (5, 18, 20, 39, 7, 2, 16, "tanh"),        # backward takes 105 KB of LDS: above the 64 KB default
    (67, 18, 20, 12, 3, 2, 4, "relu"),
    (67, 1, 3, 39, 3, 3, 16, "tanh"),
    (5, 4, 2, 7, 7, 2, 4, "relu"),
]
IDS = ["-".join(str(v) for v in s) for s in STAGES]


def _act(u, act):
    return torch.tanh(u) if act == "tanh" else torch.relu(u)


def ref_stage(c, x=None, training=True, rm=None, rv=None):
    """float64 torch: -> (z, u, a, y)."""
    x = c["x"] if x is None else x
    H, kh, ps = x.shape[2], c["w"].shape[2], c["ps"]
    z = F.conv2d(x, c["w"], c["b"], padding=((kh - 1) // 2, 0))
    u = F.batch_norm(z, rm, rv, c["ga"], c["be"], training, MOMENTUM, EPS)
    a = _act(u, c["act"])
    y = F.max_pool2d(a, (ps, 1), padding=(H % ps, 0))
    return z, u, a, y


def _window_gap(a, ps, positive_only):
    """Per window: largest value minus runner-up (inf where the window has one real row or, with positive_only, no
    positive value)."""
    H = a.shape[2]
    pad = H % ps
    ap = F.pad(a, (0, 0, pad, pad), value=float("-inf"))
    Hp = (H + 2 * pad - ps) // ps + 1
    win = ap[:, :, :Hp * ps].reshape(a.shape[0], a.shape[1], Hp, ps, a.shape[3])
    top = torch.topk(win, min(2, ps), dim=3).values
    gap = top[:, :, :, 0] - top[:, :, :, 1] if ps > 1 else torch.full_like(top[:, :, :, 0], float("inf"))
    if positive_only:
        gap = torch.where(top[:, :, :, 0] > 0, gap, torch.full_like(gap, float("inf")))
    return gap, win


def ambiguous(c, u, a):
    """Boolean [B, H, E]: positions of the input whose column holds an ambiguous unit."""
    relu = c["act"] == "relu"
    bad = (u.abs() < MARGIN).any(1) if relu else torch.zeros_like(u[:, 0], dtype=torch.bool)
    gap, _ = _window_gap(a, c["ps"], relu)
    H, ps = a.shape[2], c["ps"]
    pad = H % ps
    tie = (gap < MARGIN).any(1)                                   # [B, Hp, E]
    rows = torch.arange(H)
    bad = bad | tie[:, ((rows + pad) // ps).clamp(max=tie.shape[1] - 1), :]
    return bad


@functools.lru_cache(maxsize=None)
def stage_case(B, Cin, Cout, H, kh, ps, E, act, seed=0):
    """Inputs (float64, CPU) of a stage and the float64 reference's outputs and gradients: built once, shared."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * B + 11 * H + Cin)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    # (rounded to fp32 here: the kernels and the reference see the same numbers)
    c = dict(x=rnd(B, Cin, H, E).float().double(), w=(rnd(Cout, Cin, kh, 1) * (Cin * kh) ** -0.5).float().double(),
             b=(0.1 * rnd(Cout)).float().double(), ga=(1 + 0.2 * rnd(Cout)).float().double(),
             be=(0.2 * rnd(Cout)).float().double(), ps=ps, act=act)
    for _ in range(50):
        _, u, a, _ = ref_stage(c)
        bad = ambiguous(c, u, a)
        if not bad.any():
            break
        c["x"] = (c["x"] + bad[:, None].double() * 0.05 * rnd(B, Cin, H, E)).float().double()
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("x", "w", "b", "ga", "be")}
    z, u, a, y = ref_stage(dict(c, **leaves))
    c["r"] = rnd(*y.shape).float().double()
    (y * c["r"]).sum().backward()
    c.update(z=z.detach(), u=u.detach(), a=a.detach(), y=y.detach(), grads={k: v.grad for k, v in leaves.items()})
    return c


def dev(t):
    return t.float().to(DEV).contiguous()


def close(got, want, rtol, atol, what=""):
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want.detach().numpy(), rtol=rtol, atol=atol,
                               err_msg=what)


GRAD_TOL = dict(rtol=1e-4, atol=2e-5)
DW_TOL = dict(rtol=1e-4, atol=4 * 1.34e-4)          # 4 x fp32 CPU torch's error: see the module docstring
DB_TOL = dict(rtol=1e-4, atol=4 * 9.16e-5)


def grad_close(got, want, what, rtol=GRAD_TOL["rtol"], atol=GRAD_TOL["atol"]):
    err = (got.detach().cpu().double() - want).abs()
    print(f"{what}: worst error / bound {float((err / (rtol * want.abs() + atol)).max()):.3f}, "
          f"largest error {float(err.max()):.3e}")
    close(got, want, rtol, atol, what)


def run_stage(c, x=None, rm=None, rv=None, nbt=None):
    """The training-mode stage on the GPU -> dict of everything it produced."""
    from mapx import ops
    x = dev(c["x"] if x is None else x)
    w, b, ga, be = dev(c["w"]), dev(c["b"]), dev(c["ga"]), dev(c["be"])
    z, part = ops.fgcnn_conv_fwd(x, w, b)
    stats = ops.fgcnn_bn_stats(part, z.shape[2], z.shape[3], rm, rv, nbt)
    y, idx = ops.fgcnn_pool_fwd(z, ga, be, c["ps"], c["act"], stats=stats)
    dx, dw, db, dga, dbe = ops.fgcnn_bwd(dev(c["r"]), idx, z, x, w, stats, ga, be, c["ps"], c["act"])
    return dict(z=z, stats=stats, y=y, idx=idx, x=dx, w=dw, b=db, ga=dga, be=dbe)


@pytest.mark.parametrize("case", STAGES, ids=IDS)
def test_inputs_are_unambiguous(case):
    c = stage_case(*case)
    assert not ambiguous(c, c["u"], c["a"]).any()
    if c["act"] == "relu":
        assert float(c["u"].abs().min()) >= MARGIN
    gap, _ = _window_gap(c["a"], c["ps"], c["act"] == "relu")
    assert float(gap.min()) >= MARGIN


@pytest.mark.parametrize("case", STAGES, ids=IDS)
def test_stage_forward_and_every_gradient(case):
    c = stage_case(*case)
    out = run_stage(c)
    close(out["z"], c["z"], what="conv", **FWD_TOL)
    n = c["z"].numel() // c["z"].shape[1]
    mean = c["z"].mean((0, 2, 3))
    var = c["z"].var((0, 2, 3), unbiased=False)
    close(out["stats"][:, 0], mean, what="batch mean", **FWD_TOL)
    close(out["stats"][:, 1], (var + EPS).rsqrt(), rtol=1e-5, atol=0, what="batch rstd")
    close(out["y"], c["y"], what="pooled", **FWD_TOL)
    assert tuple(out["y"].shape) == tuple(c["y"].shape) and n > 1
    gr = c["grads"]
    for k in ("x", "ga", "be"):
        grad_close(out[k].view(gr[k].shape), gr[k], f"d{k}")
    grad_close(out["w"].view(gr["w"].shape), gr["w"], "dw", **DW_TOL)
    assert float(gr["b"].abs().max()) < 1e-9           # zero in exact arithmetic
    grad_close(out["b"], gr["b"], "db", **DB_TOL)


@pytest.mark.parametrize("case", [STAGES[1], STAGES[2], STAGES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_running_statistics_after_one_and_two_steps(case):
    """running_mean / running_var move by momentum 0.1 with the UNBIASED variance and num_batches_tracked counts on
    the device; the second step sees another batch."""
    c = stage_case(*case)
    C = c["w"].shape[0]
    g = torch.Generator().manual_seed(5)
    rm64, rv64 = 0.3 * torch.randn(C, generator=g, dtype=torch.float64), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    rm64, rv64 = rm64.float().double(), rv64.float().double()
    rm, rv, nbt = dev(rm64), dev(rv64), torch.zeros((), dtype=torch.int64, device=DEV)
    x2 = (c["x"] * 0.7 + 0.3).float().double()
    for step, x in enumerate((c["x"], x2), start=1):
        ref_stage(c, x=x, rm=rm64, rv=rv64)            # (F.batch_norm updates rm64 / rv64 in place)
        run_stage(c, x=x, rm=rm, rv=rv, nbt=nbt)
        close(rm, rm64, rtol=1e-5, atol=1e-6, what=f"running_mean after step {step}")
        close(rv, rv64, rtol=1e-5, atol=1e-6, what=f"running_var after step {step}")
        assert int(nbt) == step


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("case", [STAGES[1], STAGES[2], STAGES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_eval_uses_the_running_statistics_and_leaves_them_alone(case, B):
    from mapx import ops
    c = stage_case(*case)
    C = c["w"].shape[0]
    g = torch.Generator().manual_seed(6)
    rm64 = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    rv64 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    x64 = c["x"][:B]
    _, _, _, y_ref = ref_stage(c, x=x64, training=False, rm=rm64.clone(), rv=rv64.clone())
    rm, rv, nbt = dev(rm64), dev(rv64), torch.full((), 3, dtype=torch.int64, device=DEV)
    before = (rm.clone(), rv.clone(), nbt.clone())
    z, part = ops.fgcnn_conv_fwd(dev(x64), dev(c["w"]), dev(c["b"]), stats=False)
    assert part is None
    y, idx = ops.fgcnn_pool_fwd(z, dev(c["ga"]), dev(c["be"]), c["ps"], c["act"], running_mean=rm, running_var=rv,
                                save=False)
    assert idx is None
    # (eval inputs are not repaired for ties: the pooled VALUE does not depend on which of two equal rows wins)
    close(y, y_ref, what="eval pooled", **FWD_TOL)
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and torch.equal(nbt, before[2])


def test_module_eval_leaves_buffers_and_train_moves_them():
    """The autograd stage (layers._ConvBnActPool through FGCNNBlock): train mode moves the buffers and counts, eval
    does not touch them and needs no gradient state."""
    from mapx.layers import FGCNNBlock
    torch.manual_seed(0)
    blk = FGCNNBlock(7, 4, [3, 2], [3, 3], [2, 2], [2, 1], activation="tanh").to(DEV)
    x = torch.randn(5, 1, 7, 4, device=DEV, requires_grad=True)
    blk.train()
    out = blk(x)
    assert tuple(out.shape) == (5, 4 * 2 + 2 * 1, 4)
    out.sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in blk.parameters())
    bn = blk.conv_layers[0]["1"]
    assert int(bn.num_batches_tracked) == 1 and bool((bn.running_mean != 0).any())
    blk(x.detach())
    assert int(bn.num_batches_tracked) == 2
    blk.eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    with torch.no_grad():
        blk(x.detach()[:1])
    for k, v in blk.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_first_of_equal_maxima_wins_as_in_torch():
    """Integer-valued activations (batch statistics given as mean 0, rstd 1; gamma 1, beta 0; relu) tie all the time:
    the saved argmax is torch's (the first)."""
    from mapx import ops
    g = torch.Generator().manual_seed(7)
    for H, ps in ((7, 2), (12, 3), (7, 3)):
        z = torch.randint(0, 3, (5, 2, H, 8), generator=g).float()
        stats = torch.tensor([[0.0, 1.0]] * 2)
        y, idx = ops.fgcnn_pool_fwd(z.to(DEV), torch.ones(2, device=DEV), torch.zeros(2, device=DEV), ps, "relu",
                                    stats=stats.to(DEV))
        pad = H % ps
        y_ref, flat = F.max_pool2d(z, (ps, 1), padding=(pad, 0), return_indices=True)
        assert torch.equal(y.cpu(), y_ref)
        h_ref = flat // 8
        o = torch.arange(y_ref.shape[2]).view(1, 1, -1, 1)
        assert torch.equal(idx.cpu().long(), h_ref - (o * ps - pad))


def test_pooling_propagates_nan_like_torch():
    from mapx import ops
    z = torch.tensor([1.0, float("nan"), 2.0, 3.0, 0.5, 0.25]).view(1, 1, 6, 1).repeat(1, 1, 1, 4)
    stats = torch.tensor([[0.0, 1.0]])
    y, _ = ops.fgcnn_pool_fwd(z.to(DEV), torch.ones(1, device=DEV), torch.zeros(1, device=DEV), 2, "relu",
                              stats=stats.to(DEV))
    y_ref = F.max_pool2d(torch.relu(z), (2, 1))
    assert torch.isnan(y_ref[0, 0, 0]).all() and torch.isnan(y[0, 0, 0]).all()
    assert torch.equal(y[0, 0, 1:].cpu(), y_ref[0, 0, 1:])


IP_CASES = [(5, 2, 4), (67, 3, 16), (5, 64, 16), (67, 65, 4), (5, 153, 16)]


@functools.lru_cache(maxsize=None)
def ip_case(B, T, E):
    g = torch.Generator().manual_seed(B + T + E)
    x = torch.randn(B, T, E, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    mask = torch.triu(torch.ones(T, T), 1).bool()
    out = torch.masked_select(torch.bmm(x, x.transpose(1, 2)), mask).view(B, -1)
    r = torch.randn(out.shape, generator=g, dtype=torch.float64).float().double()
    (out * r).sum().backward()
    return x.detach(), out.detach(), r, x.grad


@pytest.mark.parametrize("B,T,E", IP_CASES)
def test_inner_product_forward_and_gradient(B, T, E):
    from mapx import ops
    x, out_ref, r, dx_ref = ip_case(B, T, E)
    out = ops.inner_product_fwd(dev(x))
    assert tuple(out.shape) == (B, T * (T - 1) // 2)
    close(out, out_ref, what="inner products", **FWD_TOL)
    dx = ops.inner_product_bwd(dev(r), dev(x))
    grad_close(dx, dx_ref, "dx")


def test_unsupported_shapes_raise_the_library_error():
    from mapx import ops
    from mapx.native import MapxError
    z = lambda *s: torch.zeros(*s, device=DEV)
    conv = lambda Cin, Cout, H, E, kh: ops.fgcnn_conv_fwd(z(2, Cin, H, E), z(Cout, Cin, kh, 1), z(Cout))
    with pytest.raises(MapxError, match="channels"):
        conv(1, 33, 5, 4, 3)
    with pytest.raises(MapxError, match="channels"):
        conv(33, 2, 5, 4, 3)
    with pytest.raises(MapxError, match="kernel height"):
        conv(1, 2, 5, 4, 17)
    with pytest.raises(MapxError, match="kernel height"):
        conv(1, 2, 5, 4, 4)
    with pytest.raises(MapxError, match="E % 4"):
        conv(1, 2, 5, 6, 3)
    with pytest.raises(MapxError, match="LDS"):
        conv(32, 32, 64, 64, 15)
    with pytest.raises(MapxError, match="half"):                   # 5 % 3 = 2 rows of padding > 3 / 2: torch raises too
        ops.fgcnn_pool_fwd(z(2, 2, 5, 4), z(2), z(2), 3, "tanh", stats=z(2, 2))
    with pytest.raises(RuntimeError, match="half"):
        F.max_pool2d(torch.zeros(2, 2, 5, 4), (3, 1), padding=(2, 0))
    with pytest.raises(MapxError, match="more than one value"):    # torch: "Expected more than 1 value per channel"
        ops.fgcnn_bn_stats(torch.zeros(1, 2, 2, dtype=torch.float64, device=DEV), 1, 1)
    with pytest.raises(MapxError, match="feature rows"):
        ops.inner_product_fwd(z(2, 193, 4))
    with pytest.raises(MapxError, match="feature rows"):
        ops.inner_product_fwd(z(2, 1, 4))
    with pytest.raises(MapxError, match="row width"):
        ops.inner_product_bwd(z(2, 3), z(2, 3, 6))
    with pytest.raises(KeyError):
        ops.fgcnn_pool_fwd(z(2, 2, 4, 4), z(2), z(2), 2, "gelu", stats=z(2, 2))


@pytest.mark.parametrize("case", [STAGES[3], STAGES[4]], ids=[IDS[3], IDS[4]])
def test_every_stage_is_bitwise_deterministic(case):
    from mapx import ops
    c = stage_case(*case)
    a, b = run_stage(c), run_stage(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x, _, r, _ = ip_case(5, 153, 16)
    outs = [(ops.inner_product_fwd(dev(x)), ops.inner_product_bwd(dev(r), dev(x))) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
