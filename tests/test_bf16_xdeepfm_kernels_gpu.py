"""The fused CIN kernels of bf16 compute mode (csrc/cin_fused.hip) against float64.

Method: inputs are rounded to bf16 on the CPU, the reference is a float64 restatement on the same values; the Hadamard
operand a = bf16(x0 * xi) is reproduced exactly by (x0 * xi).float().bfloat16() (the product of two bf16 values is
exact in fp32).

Bounds, derived like tests/test_bf16_gpu.py's: an fp32 accumulation of n exact products is within n * 2^-24 of the sum
of the absolute products in the worst case and within a few sqrt(n) * 2^-24 in practice; 2e-6 = 2^-19 covers one
accumulation stage up to K = 4096 / R = 4096 terms with that practical margin.
  one stage (dW over rows, db, the pooling sums before their rounding):  2e-6 * sum |.||.|
  two stages (Y: contraction, then the bias add; dxi / dx0t: the MFMA contraction over the units, then the reduction
  over fields / units; plus the pooled gradient or the running sum where one is added):  4e-6 * the absolute triple sum
  bf16 outputs: that bound + 2^-8 |ref| (bf16 keeps 8 significant bits: unit roundoff 2^-8).
A kernel that misses these is a finding to report, not a bound to loosen."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
U_BF = 2.0 ** -8


def _slab():
    from mapx import ops
    return ops.CIN_DW_SLAB_ROWS


# (id, B, E, F, H, U)
SHAPES = [
    ("smallest", 1, 8, 2, 2, 1),
    ("fixture-layer1", 64, 16, 25, 25, 12),            # K = 625
    ("fixture-layer2", 64, 16, 25, 12, 8),             # K = 300
    ("avazu-layer1", 9, 16, 23, 23, 50),               # R = 144: ragged against any tile; K = 529, odd
    ("avazu-layer2", 9, 16, 23, 50, 50),               # K = 1150
    ("E-not-a-power-of-two", 5, 24, 3, 5, 7),
    ("caps", 3, 8, 64, 64, 128),                       # K = 4096
    ("caps-H", 2, 8, 5, 128, 70),                      # H at its cap, three unit tiles -> the four-tile kernels
    ("many-slabs", None, 8, 3, 5, 7),                  # R = 5 slabs of the dW kernel + 40 rows (B filled in below)
]


def _pad(t):
    """[R, n] bf16 (CPU) -> device [R, pad8(n)] with zero pad columns."""
    from mapx import ops
    out = torch.zeros(t.shape[0], ops.pad8(t.shape[1]), dtype=BF)
    out[:, :t.shape[1]] = t
    return out.to(DEV)


class Case:
    def __init__(self, name, B, E, F, H, U):
        if B is None:
            B = (5 * _slab() + 40) // E
        g = torch.Generator().manual_seed(hash((E, F, H, U)) % (1 << 31))
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.name, self.B, self.E, self.F, self.H, self.U, self.R = name, B, E, F, H, U, B * E
        R = self.R
        self.x3 = rnd(B, F, E).to(BF)
        self.x0 = self.x3.permute(0, 2, 1).reshape(R, F).contiguous()
        self.xi = rnd(R, H).to(BF)
        self.w = (rnd(U, F * H) * (F * H) ** -0.5).to(BF)
        self.bias = rnd(U) * 0.1
        self.dy = (rnd(R, U) * 0.05).to(BF)
        self.gpool = (rnd(B, H) * 0.05).to(BF)
        self.prior = rnd(R, F) * 0.05                  # a running dx0t to accumulate into

    def a(self, xi):
        return (self.x0.float()[:, :, None] * xi.float()[:, None, :]).to(BF).to(F64).reshape(self.R, -1)

    def dA(self):
        """(dA [R,F,H], sum |dy||w| [R,F,H]) in float64."""
        dy, w = self.dy.to(F64), self.w.to(F64)
        return (dy @ w).view(self.R, self.F, self.H), (dy.abs() @ w.abs()).view(self.R, self.F, self.H)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(*next(s for s in SHAPES if s[0] == name))
    return _CASES[name]


def _within(what, got, ref, bound):
    got, ref, bound = got.detach().cpu().to(F64), ref.to(F64), bound.to(F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[{what}] worst error / bound {worst:.3f} (max error {float(err.max()):.3e})")
    assert bool((err <= bound).all()), f"{what}: error up to {worst:.3f} of its bound"


NAMES = [s[0] for s in SHAPES]


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_pooling(name):
    from mapx import ops
    c = case(name)
    x0t, xi, w, bias = _pad(c.x0), _pad(c.xi), c.w.to(DEV), c.bias.to(DEV)
    y = ops.cin_fused_fwd(x0t, c.F, xi, c.H, w, bias)
    assert y.dtype == BF and y.shape == (c.R, ops.pad8(c.U))
    a = c.a(c.xi)
    ref = a @ c.w.to(F64).t() + c.bias.to(F64)
    mag = a.abs() @ c.w.to(F64).abs().t() + c.bias.to(F64).abs()
    _within(f"{name} Y", y[:, :c.U], ref, 4e-6 * mag + U_BF * ref.abs())
    assert not bool(y[:, c.U:].float().abs().any()), "pad columns are zero"
    assert torch.equal(y, ops.cin_fused_fwd(x0t, c.F, xi, c.H, w, bias))
    # pooling: fp32 sum of the STORED rows, one rounding; into a column slice of a wider buffer
    out = torch.full((c.B, c.U + 5), 7.0, dtype=BF, device=DEV)
    ops.cin_pool_fwd_bf16(y, c.U, c.B, c.E, out[:, 3:3 + c.U])
    rows = y[:, :c.U].cpu().to(F64).view(c.B, c.E, c.U)
    _within(f"{name} pooled", out[:, 3:3 + c.U], rows.sum(1), 2e-6 * rows.abs().sum(1) + U_BF * rows.sum(1).abs())
    assert bool((out[:, :3] == 7).all()) and bool((out[:, 3 + c.U:] == 7).all())


@pytest.mark.parametrize("name", NAMES)
def test_transpose_and_dx3(name):
    from mapx import ops
    c = case(name)
    x0t = ops.cin_transpose_bf16(c.x3.to(DEV))
    assert torch.equal(x0t.cpu(), _pad(c.x0).cpu())
    dx3 = ops.cin_dx3_bf16(c.prior.to(DEV), c.B, c.E, c.F)
    assert torch.equal(dx3.cpu(), c.prior.view(c.B, c.E, c.F).permute(0, 2, 1).to(BF))


@pytest.mark.parametrize("name", NAMES)
def test_weight_and_bias_gradients(name):
    from mapx import ops
    c = case(name)
    x0t, xi, dy = _pad(c.x0), _pad(c.xi), _pad(c.dy)
    dw = ops.cin_fused_bwd_weight(dy, c.U, x0t, c.F, xi, c.H)
    assert dw.dtype == torch.float32 and dw.shape == (c.U, c.F * c.H)
    a = c.a(c.xi)
    _within(f"{name} dW", dw, c.dy.to(F64).t() @ a, 2e-6 * (c.dy.to(F64).abs().t() @ a.abs()))
    slot = torch.empty(c.U, c.F * c.H, 1, device=DEV)             # the optimizer's slot has the Conv1d weight's shape
    assert ops.cin_fused_bwd_weight(dy, c.U, x0t, c.F, xi, c.H, out=slot) is slot and torch.equal(slot.view_as(dw), dw)
    db = ops.colsum(dy[:, :c.U])
    _within(f"{name} db", db, c.dy.to(F64).sum(0), 2e-6 * c.dy.to(F64).abs().sum(0))
    if c.H == c.F:                                                 # layer 1: xi is x0t itself
        dw1 = ops.cin_fused_bwd_weight(dy, c.U, x0t, c.F, x0t, c.F)
        a1 = c.a(c.x0)
        _within(f"{name} dW layer 1", dw1, c.dy.to(F64).t() @ a1, 2e-6 * (c.dy.to(F64).abs().t() @ a1.abs()))


@pytest.mark.parametrize("name", NAMES)
def test_input_gradients(name):
    from mapx import ops
    c = case(name)
    x0t, xi, dy, w = _pad(c.x0), _pad(c.xi), _pad(c.dy), c.w.to(DEV)
    dA, mag = c.dA()
    x0, xv = c.x0.to(F64), c.xi.to(F64)
    dxi, m_xi = torch.einsum("rhm,rh->rm", dA, x0), torch.einsum("rhm,rh->rm", mag, x0.abs())
    dx0, m_x0 = torch.einsum("rhm,rm->rh", dA, xv), torch.einsum("rhm,rm->rh", mag, xv.abs())
    gp = c.gpool.to(F64).repeat_interleave(c.E, dim=0)            # row r gets its sample's pooled gradient
    # without and with a pooled gradient of the layer below; dx0t overwritten and accumulated
    d0 = torch.full((c.R, c.F), float("nan"), device=DEV)
    prev = ops.cin_fused_bwd_input(dy, c.U, w, x0t, c.F, xi, c.H, d0, accumulate_x0=False, E=c.E)
    assert prev.dtype == BF and prev.shape == (c.R, ops.pad8(c.H))
    _within(f"{name} dY below, no pooled gradient", prev[:, :c.H], dxi, 4e-6 * m_xi + U_BF * dxi.abs())
    _within(f"{name} dx0t overwrite", d0, dx0, 4e-6 * m_x0)
    assert not bool(prev[:, c.H:].float().abs().any()), "pad columns are zero"
    d1 = c.prior.to(DEV).clone()
    gpool = torch.cat([torch.zeros(c.B, 3, dtype=BF), c.gpool], dim=1).to(DEV)[:, 3:]         # a column slice
    prev_g = ops.cin_fused_bwd_input(dy, c.U, w, x0t, c.F, xi, c.H, d1, accumulate_x0=True, gpool=gpool, E=c.E)
    _within(f"{name} dY below + pooled gradient", prev_g[:, :c.H], dxi + gp,
            4e-6 * (m_xi + gp.abs()) + U_BF * (dxi + gp).abs())
    _within(f"{name} dx0t accumulate", d1, c.prior.to(F64) + dx0, 4e-6 * (m_x0 + c.prior.to(F64).abs()))
    # a second call repeats the first bit for bit
    d2 = c.prior.to(DEV).clone()
    again = ops.cin_fused_bwd_input(dy, c.U, w, x0t, c.F, xi, c.H, d2, accumulate_x0=True, gpool=gpool, E=c.E)
    assert torch.equal(again, prev_g) and torch.equal(d2, d1)
    dw = ops.cin_fused_bwd_weight(dy, c.U, x0t, c.F, xi, c.H)
    assert torch.equal(dw, ops.cin_fused_bwd_weight(dy, c.U, x0t, c.F, xi, c.H))
    if c.H == c.F:
        # layer 1: xi is x0t, dxi joins dx0t
        x0d = c.x0.to(F64)
        both = torch.einsum("rhm,rh->rm", dA, x0d) + torch.einsum("rhm,rm->rh", dA, x0d)
        m_both = torch.einsum("rhm,rh->rm", mag, x0d.abs()) + torch.einsum("rhm,rm->rh", mag, x0d.abs())
        for acc in (False, True):
            d = c.prior.to(DEV).clone() if acc else torch.full((c.R, c.F), float("nan"), device=DEV)
            assert ops.cin_fused_bwd_input(dy, c.U, w, x0t, c.F, x0t, c.F, d, accumulate_x0=acc, first_layer=True) is None
            base = c.prior.to(F64) if acc else torch.zeros(c.R, c.F, dtype=F64)
            _within(f"{name} layer 1 dx0t accumulate={acc}", d, base + both, 4e-6 * (m_both + base.abs()))


def test_pool_backward_broadcasts_the_pooled_gradient():
    from mapx import ops
    c = case("E-not-a-power-of-two")
    g = torch.cat([torch.zeros(c.B, 2, dtype=BF), c.gpool], dim=1).to(DEV)[:, 2:]
    dy = ops.cin_pool_bwd_bf16(g, c.B, c.E)
    assert dy.shape == (c.R, ops.pad8(c.H))
    assert torch.equal(dy[:, :c.H].cpu(), c.gpool.repeat_interleave(c.E, dim=0))
    assert not bool(dy[:, c.H:].float().abs().any())


@pytest.mark.parametrize("F,H,U,flag", [(65, 8, 8, "num_fields"), (1, 8, 8, "num_fields"), (8, 129, 8, "cin_layer_units"),
                                        (8, 8, 129, "cin_layer_units")])
def test_shapes_outside_the_caps_are_refused(F, H, U, flag):
    from mapx import ops
    from mapx.native import MapxError
    R = 16
    z = lambda n: torch.zeros(R, ops.pad8(n), dtype=BF, device=DEV)
    w, b = torch.zeros(U, F * H, dtype=BF, device=DEV), torch.zeros(U, device=DEV)
    with pytest.raises(MapxError, match=flag):
        ops.cin_fused_fwd(z(F), F, z(H), H, w, b)
    with pytest.raises(MapxError, match=flag):
        ops.cin_fused_bwd_weight(z(U), U, z(F), F, z(H), H)
    with pytest.raises(MapxError, match=flag):
        ops.cin_fused_bwd_input(z(U), U, w, z(F), F, z(H), H, torch.zeros(R, F, device=DEV), False, E=8)


def test_cpu_tensors_and_other_element_types_are_refused():
    from mapx import ops
    from mapx.native import MapxError
    z = lambda n, dev="cpu", dt=BF: torch.zeros(16, n, dtype=dt, device=dev)
    with pytest.raises(MapxError, match="device"):
        ops.cin_fused_fwd(z(8), 8, z(8), 8, torch.zeros(4, 64, dtype=BF), torch.zeros(4))
    with pytest.raises(MapxError, match="device"):
        ops.cin_transpose_bf16(torch.zeros(2, 3, 8, dtype=BF))
    with pytest.raises(TypeError, match="bf16"):
        ops.cin_fused_fwd(z(8, DEV, torch.float32), 8, z(8, DEV), 8, torch.zeros(4, 64, dtype=BF, device=DEV),
                          torch.zeros(4, device=DEV))


def test_the_stack_allocates_nothing_of_the_hadamard_matrix_size():
    """Forward + backward of the whole stack at R = 1024, F = 25, H = 25 under torch.cuda.max_memory_allocated: the
    peak rises by less than R * F * H * 2 bytes, a bf16 Hadamard matrix.  (The stream's workspace, a fixed buffer that
    the column sums share with every other kernel, is allocated by a pass at R = 8 first.)"""
    from mapx.layers import CIN
    torch.manual_seed(0)
    F, E, B = 25, 16, 64
    cin = CIN(F, [25, 25]).to(DEV)

    def run(b):
        x = torch.randn(b, F, E, device=DEV).to(BF).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = cin(x)
        out.float().square().sum().backward()
        torch.cuda.synchronize()
        assert out.dtype == BF and x.grad.dtype == BF and bool(torch.isfinite(x.grad.float()).all())
        assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in cin.parameters())
        return torch.cuda.max_memory_allocated() - base
    run(1)
    cin.zero_grad(set_to_none=True)
    peak = run(B)
    limit = B * E * F * 25 * 2
    print(f"[allocation] peak increase {peak} bytes, limit {limit}")
    assert peak < limit
