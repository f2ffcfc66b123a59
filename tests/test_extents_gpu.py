"""Guard-band tests: every kernel writes only its extent and honours the row pitch it is given.

Every operand and output lives inside a tests/guarded.py buffer: guards in front of the first and behind the last row,
NaN canaries in every padding column, each operand with a pitch of its own.  Every case asserts
  1. the canaries of every guarded output AND input are untouched (inputs are never written),
  2. the values are bit-equal to the same call on dense, exactly-sized tensors (same kernel, same summation order),
  3. the dense result is within the entry's existing bound of an fp64 (or exact) reference at this shape.
Tier A goes through mapx.ops; Tier B calls the C entries of the wrappers that allocate their own outputs, with the
names the wrappers use (ops.lib, ptr, check, stream).  The case tables are literal lists; nothing is filtered at run
time.  Bounds are those of test_kernels_gpu.py / test_bf16_gpu.py / test_backbone_kernels_gpu.py / test_model_gpu.py.
"""
import math

import pytest
import torch

import guarded as G
import row_widths_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
EPS_BF = 2.0 ** -7           # tests/test_bf16_gpu.py
HALF_ULP = 2.0 ** -8         # tests/test_bf16_trans_kernels_gpu.py

# Tier A: the ops functions that hand the library a row pitch, and the test that runs each with every operand and
# output guarded and pitched (tests/test_guarded_host.py holds this table against ops.py).
TIER_A = [
    ("gemm", "test_gemm_layouts_tiles"), ("gemm", "test_gemm_epilogues"), ("gemm", "test_gemm_split_k_reads_pitched_operands"),
    ("gemm_bf16", "test_gemm_bf16_layouts_tiles"), ("gemm_bf16", "test_gemm_bf16_epilogues"),
    ("gemm_bwd_fused", "test_gemm_bwd_fused"),
    ("h2_weight_planes", "test_h2_weight_planes_of_a_pitched_weight"),
    ("linear_fwd", "test_skinny_linear"), ("linear_bwd_input", "test_skinny_linear"),
    ("linear_bwd_weight", "test_skinny_linear"), ("skinny_join_bwd", "test_skinny_join_bwd"),
    ("colsum", "test_colsum_family"), ("relu_mask_colsum", "test_colsum_family"),
    ("cross_bwd_pre_colsum", "test_colsum_family"),
    ("act_fwd", "test_act"), ("act_bwd", "test_act"),
    ("cin_outer_fwd", "test_cin_pieces"), ("cin_outer_bwd", "test_cin_pieces"),
    ("cin_pool_fwd", "test_cin_pieces"), ("cin_pool_bwd", "test_cin_pieces"),
    ("cin_transpose_bf16", "test_cin_fused"), ("cin_fused_fwd", "test_cin_fused"),
    ("cin_fused_bwd_input", "test_cin_fused"), ("cin_fused_bwd_weight", "test_cin_fused"),
    ("cin_pool_fwd_bf16", "test_cin_fused"), ("cin_pool_bwd_bf16", "test_cin_fused"),
    ("seg_reduce_rows_extra", "test_seg_reduce_rows_extra"),
    ("enc_grouped_fwd", "test_enc_grouped"), ("enc_grouped_dw", "test_enc_grouped"),
    ("amax", "test_amax"),
    ("pack_sparse", "test_pack_sparse"),
]


def test_tier_a_table_names_tests_of_this_file():
    for _, test in TIER_A:
        assert callable(globals().get(test)), test


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


@pytest.fixture(params=["x3", "h2"])
def arith(request, monkeypatch, ops):
    """As tests/test_kernels_gpu.py: every fp32 GEMM case runs through the six-product bf16 arithmetic (operands
    without magnitude records) and through the two-piece fp16 one (ops.AUTO_AMAX computes the records)."""
    monkeypatch.setattr(ops, "AUTO_AMAX", request.param == "h2")
    return request.param


class Guards:
    """The guarded buffers of one case; check() runs every buffer's check."""

    def __init__(self):
        self.checks = []

    def inp(self, t, extra=4, col0=0, pad_value=None, what="input"):
        t = t.to(DEV)
        v, c = G.padded_copy(t, ld=col0 + t.shape[1] + extra, col0=col0, pad_value=pad_value, what=what)
        self.checks.append(c)
        return v

    def out(self, rows, cols, dtype=F32, extra=4, col0=0, what="output", is_input=False):
        v, c = G.guarded(rows, cols, dtype, ld=col0 + cols + extra, col0=col0, device=DEV, what=what, is_input=is_input)
        self.checks.append(c)
        return v

    def vec(self, n, dtype=F32, what="output", is_input=False):
        """A guarded 1-D (or flat) tensor of n elements."""
        return self.out(1, n, dtype, extra=0, what=what, is_input=is_input)[0]

    def like(self, t, what="input", dest=False):
        """t (any shape, contiguous) copied into a guarded flat buffer: front and back guards only.  `dest`: the kernel
        writes (or adds to) it: the output canary (tests/guarded.py: inputs and outputs hold different NaNs)."""
        t = t.to(DEV).contiguous()
        v = self.vec(t.numel(), t.dtype, what=what, is_input=not dest)
        v.copy_(t.reshape(-1))
        return v.view(t.shape)

    def check(self):
        assert self.checks
        for c in self.checks:
            c()


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _within(got, ref, bound, what=""):
    err = (got.detach().cpu().double() - ref).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def _amax_kw(ops, arith, Ad, Bd):
    """AUTO_AMAX takes the record of the [rows, ld] superset of a pitched operand (ops._as2d), NaN padding and all:
    the pitched call is handed the records of the dense operands, which is what the dense call computes for itself."""
    return dict(amax_a=ops.amax(Ad), amax_b=ops.amax(Bd)) if arith == "h2" else {}


# ============================================================================================ Tier A: fp32 GEMM
LAYOUTS = [(1, 1), (1, 0), (0, 0)]
GEMM_SHAPES = [(130, 72, 40), (65, 130, 17)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_gemm_layouts_tiles(ops, arith, a_kc, b_kc, M, N, K):
    """lda / ldb / ldc = width + 4, + 8, + 12; every tile hint.  Bound: test_gemm_every_tile_layout."""
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    A = _rand(g, *((M, K) if a_kc else (K, M)))
    B = _rand(g, *((N, K) if b_kc else (K, N)))
    Am, Bm = (A if a_kc else A.t()), (B.t() if b_kc else B)
    ref = Am.double() @ Bm.double()
    bound = 2e-6 * (Am.abs().double() @ Bm.abs().double()) + 1e-6
    Ad, Bd = A.to(DEV), B.to(DEV)
    gs = Guards()
    Ap, Bp = gs.inp(A, 4, what="A"), gs.inp(B, 8, what="B")
    kw = _amax_kw(ops, arith, Ad, Bd)
    for tile in (-1, 0, 1, 2, 3):
        Cp = gs.out(M, N, extra=12, what=f"C tile {tile}")
        ops.gemm(Ap, Bp, bool(a_kc), bool(b_kc), M, N, K, out=Cp, tile=tile, **kw)
        dense = ops.gemm(Ad, Bd, bool(a_kc), bool(b_kc), M, N, K, tile=tile)
        assert torch.equal(Cp, dense), tile
        _within(dense, ref, bound, tile)
    gs.check()


@pytest.mark.parametrize("epi", ["bias_relu", "add", "cross", "relu_mask", "relu_mask_colsum"])
def test_gemm_epilogues(ops, arith, epi):
    """(129, 72, 40); aux1, aux2, out2 each with a pitch of its own.  Bounds: test_gemm_linear_forward (bias, ReLU),
    test_gemm_backward_products (add, ReLU mask), test_cross_network_fwd_bwd_vs_oracle (cross: rtol = atol = 1e-5),
    test_gemm_relu_mask_colsum_epilogue."""
    from mapx import native as N_
    M, N, K = 129, 72, 40
    g = torch.Generator().manual_seed(7 + len(epi))
    nt = epi in ("bias_relu", "cross")                     # forward layout; the others are dX = dY W
    A = _rand(g, M, K)
    B = _rand(g, *((N, K) if nt else (K, N))) / math.sqrt(K)
    Bm = B.t() if nt else B
    acc = A.double() @ Bm.double()
    bound = 2e-6 * (A.abs().double() @ Bm.abs().double()) + 1e-6
    bias, aux1, aux2 = _rand(g, N), _rand(g, M, N), _rand(g, M, N)
    d = lambda t: t.to(DEV)
    gs = Guards()
    Ap, Bp = gs.inp(A, 4, what="A"), gs.inp(B, 8, what="B")
    Cp = gs.out(M, N, extra=12, what="C")
    kw = _amax_kw(ops, arith, d(A), d(B))
    if epi == "bias_relu":
        ops.gemm(Ap, Bp, True, True, M, N, K, out=Cp, epi=N_.EPI_BIAS_RELU, bias=d(bias), **kw)
        dense = ops.gemm(d(A), d(B), True, True, M, N, K, epi=N_.EPI_BIAS_RELU, bias=d(bias))
        _within(dense, (acc + bias.double()).clamp(min=0), bound)
    elif epi == "add":
        a1 = gs.inp(aux1, 16, col0=4, what="aux1")
        ops.gemm(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_ADD, aux1=a1, **kw)
        dense = ops.gemm(d(A), d(B), True, False, M, N, K, epi=N_.EPI_ADD, aux1=d(aux1))
        _within(dense, acc + aux1.double(), bound)
    elif epi == "cross":
        a1, a2 = gs.inp(aux1, 16, col0=4, what="aux1"), gs.inp(aux2, 20, what="aux2")
        up = gs.out(M, N, extra=24, col0=8, what="out2")
        ops.gemm(Ap, Bp, True, True, M, N, K, out=Cp, epi=N_.EPI_BIAS_CROSS, bias=d(bias), aux1=a1, aux2=a2, out2=up, **kw)
        u = torch.empty(M, N, device=DEV)
        dense = ops.gemm(d(A), d(B), True, True, M, N, K, epi=N_.EPI_BIAS_CROSS, bias=d(bias), aux1=d(aux1), aux2=d(aux2),
                         out2=u)
        assert torch.equal(up, u)
        u_ref = acc + bias.double()
        torch.testing.assert_close(u.cpu().double(), u_ref, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(dense.cpu().double(), aux1.double() + aux2.double() * u_ref, rtol=1e-5, atol=1e-5)
    elif epi == "relu_mask":
        a1 = gs.inp(aux1, 16, col0=4, what="aux1")
        ops.gemm(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_RELU_MASK, aux1=a1, **kw)
        dense = ops.gemm(d(A), d(B), True, False, M, N, K, epi=N_.EPI_RELU_MASK, aux1=d(aux1))
        _within(dense, acc * (aux1 > 0), bound)
    else:
        a1 = gs.inp(aux1, 16, col0=4, what="aux1")
        pp = gs.out(ops.part_rows(M), N, extra=8, what="out2")
        ops.gemm(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_RELU_MASK_COLSUM, aux1=a1, out2=pp, **kw)
        part = torch.full((ops.part_rows(M), N), 7.0, device=DEV)
        dense = ops.gemm(d(A), d(B), True, False, M, N, K, epi=N_.EPI_RELU_MASK_COLSUM, aux1=d(aux1), out2=part)
        assert torch.equal(pp, part)
        _within(dense, acc * (aux1 > 0), bound)
        got, want = part.cpu().double().sum(0), dense.cpu().double().sum(0)
        assert bool(((got - want).abs() <= 1e-6 * dense.cpu().double().abs().sum(0) + 1e-6).all())
    assert torch.equal(Cp, dense)
    gs.check()


@pytest.mark.parametrize("case", ["add", "mask", "cross", "join"])
def test_gemm_bwd_fused(ops, arith, case):
    """(M, N, K, c0) = (129, 40, 24, 16): add / mask / x0, u, dx0 / out, every operand pitched.
    Bounds: test_gemm_bwd_fused_epilogue."""
    M, N, K = 129, 40, 24
    c0 = {"add": 0, "mask": 0, "cross": N, "join": 16}[case]
    g = torch.Generator().manual_seed(M + N + K + c0)
    dy, w = _rand(g, M, K), _rand(g, K, N)
    add = _rand(g, M, N) if case in ("add", "join") else None
    mask = _rand(g, M, N) if c0 < N else None
    x0, u, dx0_in = (_rand(g, M, c0), _rand(g, M, c0), _rand(g, M, c0)) if c0 else (None, None, None)
    plus_v = case == "join"
    d = lambda t: None if t is None else t.to(DEV)
    gs = Guards()
    opt = lambda t, extra, col0, what: None if t is None else gs.inp(t, extra, col0=col0, what=what)
    dyp, wp = gs.inp(dy, 4, what="dy"), gs.inp(w, 8, col0=4, what="w")
    Cp = gs.out(M, N, extra=12, what="C")
    dx0p = None
    if c0:
        dx0p = gs.out(M, c0, extra=4, col0=4, what="dx0")
        dx0p.copy_(d(dx0_in))
    if arith == "h2":                           # the records of the dense operands (see _amax_kw)
        ops.tag(dyp, ops.amax(d(dy)))
        ops.tag(wp, ops.amax(d(w)))
    C, t, dx0, part = ops.gemm_bwd_fused(dyp, wp, c0, add=opt(add, 16, 0, "add"), mask=opt(mask, 20, 4, "mask"),
                                         x0=opt(x0, 8, 0, "x0"), u=opt(u, 12, 4, "u"), dx0=dx0p, plus_v=plus_v, out=Cp)
    C2, t2, dx02, part2 = ops.gemm_bwd_fused(d(dy), d(w), c0, add=d(add), mask=d(mask), x0=d(x0), u=d(u),
                                             dx0=d(dx0_in), plus_v=plus_v)
    assert C is Cp and torch.equal(C, C2) and torch.equal(part, part2)
    if c0:
        assert dx0 is dx0p and torch.equal(t, t2) and torch.equal(dx0, dx02)
    gs.check()
    v = dy.double() @ w.double() + (add.double() if add is not None else 0)
    bound = 2e-6 * (dy.abs().double() @ w.abs().double() + (add.abs().double() if add is not None else 0)) + 1e-6
    vr = v.clone()
    if c0 < N:
        vr[:, c0:] = v[:, c0:] * (mask[:, c0:] > 0)
    _within(C2, vr, bound)
    Cd = C2.cpu().double()
    col_ref, absum = torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
    col_ref[c0:], absum[c0:] = Cd[:, c0:].sum(0), Cd[:, c0:].abs().sum(0)
    if c0:
        Cc = Cd[:, :c0]
        _within(t2, Cc * x0.double(), 1e-6 * (Cc * x0.double()).abs() + 1e-12)
        want = Cc * u.double() + dx0_in.double() + (Cc if plus_v else 0)
        mag = (Cc * u.double()).abs() + dx0_in.abs().double() + (Cc.abs() if plus_v else 0)
        _within(dx02, want, 3e-7 * mag + 1e-12)
        col_ref[:c0], absum[:c0] = t2.cpu().double().sum(0), t2.cpu().double().abs().sum(0)
    assert part2.shape == ((M + 63) // 64, N)
    assert bool(((part2.cpu().double().sum(0) - col_ref).abs() <= 1e-6 * absum + 1e-6).all())


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_gemm_split_k_reads_pitched_operands(ops, arith, half):
    """The weight-gradient layout with deterministic split-K: the slabs want a dense C (ldc == N), the operands keep
    their pitches.  (M, N, K) = (65, 72, 520), two slabs.  Bounds: test_gemm_weight_gradient_shapes /
    test_gemm_bf16_split_k_weight_gradient."""
    M, N, K, ns = 65, 72, 520, 2
    g = torch.Generator().manual_seed(M + N + K + ns)
    dt = BF if half else F32
    A, B = _rand(g, K, M).to(dt), _rand(g, K, N).to(dt)
    Ad, Bd = A.to(DEV), B.to(DEV)
    gs = Guards()
    Ap, Bp = gs.inp(A, 8, col0=8, what="A"), gs.inp(B, 16, what="B")
    Cp = gs.like(torch.zeros(M, N), "C", dest=True)
    if half:
        ops.gemm_bf16(Ap, Bp, False, False, M, N, K, out=Cp, nsplit=ns)
        dense = ops.gemm_bf16(Ad, Bd, False, False, M, N, K, out_dtype=F32, nsplit=ns)
    else:
        ops.gemm(Ap, Bp, False, False, M, N, K, out=Cp, nsplit=ns, **_amax_kw(ops, arith, Ad, Bd))
        dense = ops.gemm(Ad, Bd, False, False, M, N, K, nsplit=ns)
    assert torch.equal(Cp, dense)
    gs.check()
    ref, mag = A.double().t() @ B.double(), A.abs().double().t() @ B.abs().double()
    if half:
        assert float(((dense.double().cpu() - ref).abs() / mag.clamp(min=1e-30)).max()) < 2e-6
    else:
        _within(dense, ref, 4e-6 * mag + 1e-6)


def test_h2_weight_planes_of_a_pitched_weight(ops):
    """The planes of a weight read through a pitch (a column slice of a wider parameter) are, byte for byte, those of
    the dense weight; the buffer holds exactly mapx_h2_weight_planes_bytes.  What the planes hold is checked where
    they are used: tests/test_amax_gpu.py multiplies by them."""
    g = torch.Generator().manual_seed(5)
    for b_kc, (Nn, K) in ((True, (72, 40)), (False, (72, 40)), (True, (33, 17))):
        w = _rand(g, *((Nn, K) if b_kc else (K, Nn)))
        rec = ops.amax(w.to(DEV))
        nb = ops.lib.mapx_h2_weight_planes_bytes(Nn, K)
        gs = Guards()
        wp = gs.inp(w, 12, col0=4, what="w")
        out = gs.vec(nb, torch.uint8, what="planes")
        ops.h2_weight_planes(wp, b_kc, rec, out=out)
        dense = ops.h2_weight_planes(w.to(DEV), b_kc, rec)
        # the 256-byte header (csrc/gemm_h2w.hip: kPlaneHeader) holds the int32 scale exponent; the kernel leaves the
        # rest of it alone, so there the guarded buffer keeps its fill and the dense one what torch.empty found
        assert dense.numel() == nb and torch.equal(out[:4], dense[:4]) and torch.equal(out[256:], dense[256:])
        gs.check()


# ============================================================================================ Tier A: bf16 GEMM
def _bf_operands(g, a_kc, b_kc, M, N, K):
    A = _rand(g, *((M, K) if a_kc else (K, M))).to(BF)
    B = _rand(g, *((N, K) if b_kc else (K, N))).to(BF)
    return A, B, (A if a_kc else A.t()).double(), (B.t() if b_kc else B).double()


@pytest.mark.parametrize("c_dtype", [BF, F32], ids=["c-bf16", "c-fp32"])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_gemm_bf16_layouts_tiles(ops, a_kc, b_kc, c_dtype):
    """(130, 72, 40), pitches multiples of 8 elements.  Bounds: test_gemm_bf16_shapes_vs_fp64."""
    M, N, K = 130, 72, 40
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, B, Am, Bm = _bf_operands(g, a_kc, b_kc, M, N, K)
    ref, bound = Am @ Bm, Am.abs() @ Bm.abs()
    gs = Guards()
    Ap, Bp = gs.inp(A, 8, what="A"), gs.inp(B, 16, col0=8, what="B")
    for tile in (-1, 0, 1, 2):
        Cp = gs.out(M, N, c_dtype, extra=24, col0=8, what=f"C tile {tile}")
        ops.gemm_bf16(Ap, Bp, bool(a_kc), bool(b_kc), M, N, K, out=Cp, tile=tile)
        dense = ops.gemm_bf16(A.to(DEV), B.to(DEV), bool(a_kc), bool(b_kc), M, N, K, out_dtype=c_dtype, tile=tile)
        assert dense.dtype == c_dtype and torch.equal(Cp, dense), tile
        if c_dtype == F32:
            assert float(((dense.double().cpu() - ref).abs() / bound.clamp(min=1e-30)).max()) < 2e-6, tile
        else:
            _within(dense, ref, 0.5 * EPS_BF * ref.abs() + 2e-6 * bound + 1e-30, tile)
    gs.check()


# (mapx_gemm_bf16 refuses an fp32 C with the ADD, CROSS and RELU_MASK* epilogues: "!c_f32" in its argument checks)
@pytest.mark.parametrize("epi,c_dtype", [("bias_relu", BF), ("bias_relu", F32), ("add_f32", BF), ("add_bf16", BF),
                                         ("cross", BF), ("relu_mask", BF), ("relu_mask_colsum", BF)],
                         ids=["bias_relu-bf16", "bias_relu-fp32", "add_f32", "add_bf16", "cross", "relu_mask",
                              "relu_mask_colsum"])
def test_gemm_bf16_epilogues(ops, epi, c_dtype):
    """Bounds: test_gemm_bf16_epilogues (`close`), test_gemm_bf16_relu_mask_colsum_epilogue."""
    from mapx import native as N_
    M, N, K = 130, 72, 40
    g = torch.Generator().manual_seed(11 + len(epi))
    nt = epi in ("bias_relu", "cross")
    A, B, Am, Bm = _bf_operands(g, True, nt, M, N, K)
    acc, bound = Am @ Bm, Am.abs() @ Bm.abs()
    bias = _rand(g, N)
    d = lambda t: t.to(DEV)
    gs = Guards()
    Ap, Bp = gs.inp(A, 8, what="A"), gs.inp(B, 16, col0=8, what="B")
    Cp = gs.out(M, N, c_dtype, extra=24, col0=8, what="C")

    def close(got, want, slack=0.0):
        tol = (0.5 * EPS_BF * want.abs() if got.dtype == BF else 0.0) + 4e-6 * (bound + bias.abs().double()) + slack
        _within(got, want, tol + 1e-30)

    if epi == "bias_relu":
        ops.gemm_bf16(Ap, Bp, True, True, M, N, K, out=Cp, epi=N_.EPI_BIAS_RELU, bias=d(bias))
        dense = ops.gemm_bf16(d(A), d(B), True, True, M, N, K, out_dtype=c_dtype, epi=N_.EPI_BIAS_RELU, bias=d(bias))
        close(dense, (acc + bias.double()).clamp(min=0))
    elif epi in ("add_f32", "add_bf16"):
        add = _rand(g, M, N).to(F32 if epi == "add_f32" else BF)
        a1 = gs.inp(add, 8, col0=8, what="aux1")
        ops.gemm_bf16(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_ADD, aux1=a1)
        dense = ops.gemm_bf16(d(A), d(B), True, False, M, N, K, out_dtype=c_dtype, epi=N_.EPI_ADD, aux1=d(add))
        close(dense, acc + add.double(), slack=4e-6 * add.abs().double())
    elif epi == "cross":
        xi, x0 = _rand(g, M, N).to(BF), _rand(g, M, N).to(BF)
        a1, a2 = gs.inp(xi, 8, col0=8, what="aux1"), gs.inp(x0, 32, what="aux2")
        up = gs.out(M, N, BF, extra=40, col0=16, what="out2")
        ops.gemm_bf16(Ap, Bp, True, True, M, N, K, out=Cp, epi=N_.EPI_BIAS_CROSS, bias=d(bias), aux1=a1, aux2=a2, out2=up)
        u = torch.empty(M, N, dtype=BF, device=DEV)
        dense = ops.gemm_bf16(d(A), d(B), True, True, M, N, K, out_dtype=c_dtype, epi=N_.EPI_BIAS_CROSS, bias=d(bias),
                              aux1=d(xi), aux2=d(x0), out2=u)
        assert torch.equal(up, u)
        u_want = acc + bias.double()
        close(u, u_want)
        y_want = xi.double() + x0.double() * u_want
        tol = (0.5 * EPS_BF * y_want.abs() if c_dtype == BF else 0.0) + 4e-6 * (1 + x0.double().abs()) * (bound + 1)
        _within(dense, y_want, tol)
    elif epi == "relu_mask":
        y = _rand(g, M, N).clamp(min=0).to(BF)
        a1 = gs.inp(y, 8, col0=8, what="aux1")
        ops.gemm_bf16(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_RELU_MASK, aux1=a1)
        dense = ops.gemm_bf16(d(A), d(B), True, False, M, N, K, out_dtype=c_dtype, epi=N_.EPI_RELU_MASK, aux1=d(y))
        close(dense, torch.where(y.double() > 0, acc, torch.zeros_like(acc)))
    else:
        y = _rand(g, M, N).to(BF)
        a1 = gs.inp(y, 8, col0=8, what="aux1")
        rows = ops.part_rows(M, BF)
        pp = gs.out(rows, N, F32, extra=8, what="out2")
        ops.gemm_bf16(Ap, Bp, True, False, M, N, K, out=Cp, epi=N_.EPI_RELU_MASK_COLSUM, aux1=a1, out2=pp)
        part = torch.full((rows, N), 7.0, device=DEV)
        dense = ops.gemm_bf16(d(A), d(B), True, False, M, N, K, out_dtype=c_dtype, epi=N_.EPI_RELU_MASK_COLSUM,
                              aux1=d(y), out2=part)
        assert torch.equal(pp, part)
        ref = acc * (y.double() > 0)
        _within(dense, ref, (0.5 * EPS_BF * ref.abs() if c_dtype == BF else 0.0) + 4e-6 * bound + 1e-30)
        got, want = part.double().cpu().sum(0), dense.double().cpu().sum(0)
        assert bool(((got - want).abs() <= 1e-6 * dense.double().cpu().abs().sum(0) + 1e-6).all())
    assert dense.dtype == c_dtype and torch.equal(Cp, dense)
    gs.check()


# ============================================================================================ Tier A: narrow layers
SKINNY_SHAPES = [(130, 3, 20), (5, 1, 8)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES)
def test_skinny_linear(ops, half, M, N, K):
    """linear_fwd / linear_bwd_input / linear_bwd_weight on the streaming kernels.  The wrappers take x, w and dy
    through native.ptr, which refuses a pitched tensor of more than one row (pinned below), so through ops only the
    destinations are pitched; the C entries, which take a pitch for every operand, are then called with all of them
    pitched.  Bounds: test_skinny_linear_kernels_vs_fp64 / test_streaming_narrow_layers_in_bf16_mode."""
    lib, check, stream = ops.lib, ops.check, ops.stream
    dt = BF if half else F32
    g = torch.Generator().manual_seed(M + N + K)
    x = _rand(g, M, K).to(dt)
    w = (_rand(g, N, K) / K ** 0.5).to(dt)
    b = _rand(g, N)
    dy = _rand(g, M, N).to(dt)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    fkw = dict(out_dtype=F32) if half else {}
    assert (ops._skinny_h if half else ops._skinny)(N, K, xd, wd)
    y = ops.linear_fwd(xd, wd, bd, **fkw)
    yr = ops.linear_fwd(xd, wd, bd, relu=True, **fkw)
    dx = ops.linear_bwd_input(dyd, wd)
    dw = ops.linear_bwd_weight(dyd, xd)
    assert y.dtype == F32 and dx.dtype == dt and dw.dtype == F32
    # 3. the dense results against fp64
    ref = x.double() @ w.double().t() + b.double()
    dx_ref, dw_ref = dy.double() @ w.double(), dy.double().t() @ x.double()
    if half:
        _within(y, ref, 2e-6 * (x.double().abs() @ w.double().abs().t()) + 1e-6)
        _within(dw, dw_ref, 4e-6 * (dy.double().abs().t() @ x.double().abs()) + 1e-6)
        _within(dx, dx_ref, EPS_BF * dx_ref.abs() + 4e-6 * (dy.double().abs() @ w.double().abs()) + 1e-6)
    else:
        assert float((y.cpu().double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
        assert float((dw.cpu().double() - dw_ref).abs().max()) <= 3e-6 * float(dw_ref.abs().max())
        assert float((dx.cpu().double() - dx_ref).abs().max()) <= 2e-6 * float(dx_ref.abs().max())
    # 1 + 2 through ops: pitched destinations
    gs = Guards()
    xg, wg, dyg = gs.like(x, "x"), gs.like(w, "w"), gs.like(dy, "dy")
    yp = gs.out(M, N, F32, extra=5, col0=1, what="y")
    assert ops.linear_fwd(xg, wg, bd, relu=True, out=yp, **fkw) is yp and torch.equal(yp, yr)
    dxp = gs.out(M, K, dt, extra=8, col0=4, what="dx")
    assert ops.linear_bwd_input(dyg, wg, out=dxp) is dxp and torch.equal(dxp, dx)
    dwg = gs.like(torch.zeros(N, K), "dw", dest=True)
    assert ops.linear_bwd_weight(dyg, xg, out=dwg) is dwg and torch.equal(dwg, dw)
    gs.check()
    # a pitched gradient slot is not the streaming kernel's: linear_bwd_weight sends it to the GEMM with nsplit = 1
    # (ops.py, linear_bwd_weight: "if out is not None and out.stride(0) != K: ns = 1"), another summation order, so
    # equality is not owed: fp64 at the GEMM's weight-gradient bound (test_gemm_backward_products)
    gs = Guards()
    dwp = gs.out(N, K, F32, extra=12, col0=4, what="dw pitched")
    ops.linear_bwd_weight(dyd, xd, out=dwp)
    _within(dwp, dw_ref, 4e-6 * (dy.double().abs().t() @ x.double().abs()) + 1e-6)
    gs.check()
    # the refusal is loud: a pitched x of more than one row never reaches the kernel with a wrong pointer
    xp = Guards().inp(x, 4, col0=4)
    with pytest.raises(AssertionError, match="contiguous"):
        ops.linear_fwd(xp, wd, bd, **fkw)
    # 1 + 2 on the C entries: x, w, dy and the destinations all pitched, each with its own pitch
    gs = Guards()
    al = 4                                              # rows of x, w, dx: 16 bytes (fp32) / 8 bytes (bf16) = 4 elements
    xp, wp = gs.inp(x, al, col0=al, what="x"), gs.inp(w, 2 * al, what="w")
    dyp = gs.inp(dy, 3, col0=2, what="dy")
    yp = gs.out(M, N, F32, extra=5, col0=1, what="y")
    dxp = gs.out(M, K, dt, extra=3 * al, col0=al, what="dx")
    chunks = lib.mapx_skinny_chunks()
    part = gs.vec(chunks * N * K, F32, what="dw partials")
    fwd, dxf, dwf = (lib.mapx_skinny_linear_fwd_bf16, lib.mapx_skinny_linear_dx_bf16, lib.mapx_skinny_linear_dw_bf16) \
        if half else (lib.mapx_skinny_linear_fwd, lib.mapx_skinny_linear_dx, lib.mapx_skinny_linear_dw)
    check(fwd(xp.data_ptr(), xp.stride(0), wp.data_ptr(), wp.stride(0), bd.data_ptr(), M, N, K, 0, yp.data_ptr(),
              yp.stride(0), stream()))
    check(dxf(dyp.data_ptr(), dyp.stride(0), wp.data_ptr(), wp.stride(0), M, N, K, dxp.data_ptr(), dxp.stride(0), stream()))
    check(dwf(dyp.data_ptr(), dyp.stride(0), xp.data_ptr(), xp.stride(0), M, N, K, part.data_ptr(), chunks, stream()))
    dw2 = torch.empty(N, K, device=DEV)
    ops._sum_now(dw2, part, N * K, chunks, N * K)
    assert torch.equal(yp, y) and torch.equal(dxp, dx) and torch.equal(dw2, dw)
    gs.check()


def test_skinny_join_bwd(ops):
    """(M, N, D, H) = (129, 3, 8, 12).  Through ops `final` is the pitched operand (the wrapper takes dz, w, x0, u
    through native.ptr: a column slice ops.cols(w, ...) of more than one row is refused, pinned below); the C entry,
    which takes a pitch for every operand and output, is then called with all of them pitched.
    Bounds: test_skinny_join_bwd_vs_fp64."""
    lib, check, stream = ops.lib, ops.check, ops.stream
    M, N, D, H, plus_v = 129, 3, 8, 12, True
    g_ = torch.Generator().manual_seed(M + N + D)
    dz, w, final = _rand(g_, M, N), _rand(g_, N, D + H), _rand(g_, M, D + H)
    x0, u = _rand(g_, M, D), _rand(g_, M, D)
    d = lambda t: t.to(DEV)
    dense = ops.skinny_join_bwd(d(dz), d(w), d(final), D, d(x0), d(u), plus_v)
    g, t, dx0, dzr, pc, pd = dense
    v = dz.double() @ w.double()
    vc, vd = v[:, :D], v[:, D:]
    ref = dict(g=vc, t=vc * x0.double(), dx0=vc * u.double() + vc,
               dzr=torch.where(final[:, D:] > 0, vd, torch.zeros_like(vd)))
    for name, got in (("g", g), ("t", t), ("dx0", dx0), ("dzr", dzr)):
        assert float((got.cpu().double() - ref[name]).abs().max()) <= 2e-6 * max(1.0, float(ref[name].abs().max())), name
    tiles = (M + 127) // 128
    assert pc.shape == (tiles, D) and pd.shape == (tiles, H)
    assert float((pc.cpu().double().sum(0) - ref["t"].sum(0)).abs().max()) <= 1e-4 * max(1.0, float(ref["t"].sum(0).abs().max()))
    assert float((pd.cpu().double().sum(0) - ref["dzr"].sum(0)).abs().max()) <= 1e-4 * max(1.0, float(ref["dzr"].sum(0).abs().max()))
    # through ops: final pitched, the rest guarded
    gs = Guards()
    got = ops.skinny_join_bwd(gs.like(dz, "dz"), gs.like(w, "w"), gs.inp(final, 8, col0=4, what="final"), D,
                              gs.like(x0, "x0"), gs.like(u, "u"), plus_v)
    assert all(torch.equal(a, b) for a, b in zip(got, dense))
    gs.check()
    _, wide = G.padded_copy(d(w), ld=D + H + 8, col0=0)
    with pytest.raises(AssertionError, match="contiguous"):
        ops.skinny_join_bwd(d(dz), ops.cols(wide.rows, 0, D + H), d(final), D, d(x0), d(u), plus_v)
    # the C entry with everything pitched
    gs = Guards()
    dzp, wp = gs.inp(dz, 5, col0=2, what="dz"), gs.inp(w, 8, col0=4, what="w")
    fp, x0p, up = gs.inp(final, 8, col0=4, what="final"), gs.inp(x0, 4, what="x0"), gs.inp(u, 12, col0=4, what="u")
    gp, tp = gs.out(M, D, extra=4, what="g"), gs.out(M, D, extra=8, col0=4, what="t")
    dx0p, dzrp = gs.out(M, D, extra=12, what="dx0"), gs.out(M, H, extra=4, col0=8, what="dzr")
    pcp, pdp = gs.vec(tiles * D, what="part_cross"), gs.vec(tiles * H, what="part_deep")
    sd = lambda x: (x.data_ptr(), x.stride(0))
    check(lib.mapx_skinny_join_bwd(*sd(dzp), *sd(wp), M, N, D, H, *sd(fp), *sd(x0p), *sd(up), int(plus_v), *sd(gp), *sd(tp),
                                   *sd(dx0p), *sd(dzrp), pcp.data_ptr(), pdp.data_ptr(), None, None, stream()))
    for a, b_ in zip((gp, tp, dx0p, dzrp, pcp.view(tiles, D), pdp.view(tiles, H)), dense):
        assert torch.equal(a, b_)
    gs.check()


# ============================================================================================ Tier A: column sums
def _colsum_pitch(N):
    """(extra, col0) of a window whose rows stay 16-byte aligned where the float4 kernels ask for it."""
    return (8, 4) if N % 4 == 0 else (4, 3)


def _db_bound(terms, scale=2e-6, floor=1e-6):
    return scale * float(terms.abs().sum(0).max()) + floor


@pytest.mark.parametrize("N", [4, 5, 68, 132])
def test_colsum_family(ops, N):
    """M = 70; colsum at every N, relu_mask_colsum / cross_bwd_pre_colsum (float4 rows) at N % 4 == 0, fp32 and bf16
    (the bf16 forms take any N).  Bounds: test_colsum, test_fused_elementwise_colsum,
    test_bf16_elementwise_backward_kernels."""
    M = 70
    g = torch.Generator().manual_seed(M + N)
    extra, col0 = _colsum_pitch(N)
    d = lambda t: t.to(DEV)
    for dt in (F32, BF):
        half = dt == BF
        x, y = _rand(g, M, N).to(dt), _rand(g, M, N).to(dt)
        x0, u, prev = _rand(g, M, N).to(dt), _rand(g, M, N).to(dt), _rand(g, M, N)
        # ---- colsum
        gs = Guards()
        out = gs.vec(N, what="colsum out")
        assert ops.colsum(gs.inp(x, extra, col0=col0, what="x"), out=out) is out
        dense = ops.colsum(d(x))
        assert torch.equal(out, dense)
        gs.check()
        if half:
            torch.testing.assert_close(dense.cpu().double(), x.double().sum(0), rtol=1e-5,
                                       atol=1e-5 * float(x.double().abs().sum(0).max()))
        else:
            torch.testing.assert_close(dense.cpu().double(), x.double().sum(0), rtol=0, atol=_db_bound(x))
        if N % 4 and not half:
            continue                      # (mapx_relu_mask_colsum / mapx_cross_bwd_pre_colsum: N % 4 == 0)
        # ---- relu_mask_colsum
        gs = Guards()
        db = gs.vec(N, what="db")
        dz, db_ = ops.relu_mask_colsum(gs.inp(x, extra, col0=col0, what="dy"), gs.inp(y, extra + 4, what="y"), db=db)
        dz2, db2 = ops.relu_mask_colsum(d(x), d(y))
        assert db_ is db and torch.equal(dz, dz2) and torch.equal(db, db2)
        gs.check()
        want = torch.where(y > 0, x, torch.zeros_like(x))
        assert torch.equal(dz2.cpu(), want)
        if half:
            torch.testing.assert_close(db2.cpu().double(), want.double().sum(0), rtol=1e-5,
                                       atol=1e-5 * float(want.double().abs().sum(0).max()) + 1e-30)
        else:
            torch.testing.assert_close(db2.cpu().double(), want.double().sum(0), rtol=0, atol=_db_bound(want))
        # ---- cross_bwd_pre_colsum: overwrite, accumulate, plus_g
        for acc, plus_g in ((False, False), (True, False), (False, True)):
            gs = Guards()
            db = gs.vec(N, what="db")
            dx0 = gs.like(prev, "dx0", dest=True) if acc else None
            x0g, ug = gs.like(x0, "x0"), gs.like(u, "u")
            t, dx0_, db_ = ops.cross_bwd_pre_colsum(gs.inp(x, extra, col0=col0, what="g"), x0g, ug, dx0=dx0, db=db,
                                                    plus_g=plus_g)
            t2, dx02, db2 = ops.cross_bwd_pre_colsum(d(x), d(x0), d(u), dx0=d(prev).clone() if acc else None,
                                                     plus_g=plus_g)
            assert (not acc or dx0_ is dx0) and torch.equal(t, t2) and torch.equal(dx0_, dx02) and torch.equal(db, db2)
            gs.check()
            t_want = (x.float() * x0.float()).to(dt)
            assert torch.equal(t2.cpu(), t_want) and dx02.dtype == F32
            dx0_want = x.float() * u.float() + (prev if acc else 0) + (x.float() if plus_g else 0)
            torch.testing.assert_close(dx02.cpu(), dx0_want, rtol=1e-6, atol=1e-6)
            if half:
                torch.testing.assert_close(db2.cpu().double(), t_want.double().sum(0), rtol=1e-5,
                                           atol=1e-5 * float(t_want.double().abs().sum(0).max()) + 1e-30)
            else:
                torch.testing.assert_close(db2.cpu().double(), t_want.double().sum(0), rtol=0, atol=_db_bound(t_want))


@pytest.mark.parametrize("M", [70, 300])
def test_deferred_sums_equal_immediate_sums(ops, M):
    """`out` / `db` given and defer=True, then flush_deferred(): the same bits as the call that sums at once, for the
    three column-sum wrappers in fp32 and bf16 and for linear_bwd_weight on the bf16 streaming kernel (N = 3, K = 20).
    M = 70: fewer rows than the 128 row chunks; M = 300: three rows per chunk, the last used chunk partial.
    N = 5: fp32 colsum only (the fp32 fused forms need N % 4 == 0) and the bf16 column-pair form; 12: the fp32 32-lane
    form, bf16 column pairs; 136: the fp32 64-lane form, the bf16 8-column form; 264: the fp32 32-lane form over more
    than one column block, the bf16 8-column form."""
    ops.flush_deferred()
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)

    def flushed(*outs):
        assert all(bool(torch.isnan(o).all()) for o in outs)          # nothing summed yet
        ops.flush_deferred()
        return outs

    for N in (5, 12, 136, 264):
        g = torch.Generator().manual_seed(M + N)
        for dt in (F32, BF):
            half = dt == BF
            x, y, x0, u = (_rand(g, M, N).to(dt).to(DEV) for _ in range(4))
            now = ops.colsum(x, out=nan(N))
            later, = flushed(ops.colsum(x, out=nan(N), defer=True))
            assert torch.equal(later, now), (N, dt)
            if N % 4 and not half:
                continue
            dz, db = ops.relu_mask_colsum(x, y, db=nan(N))
            dz2, db2 = ops.relu_mask_colsum(x, y, db=nan(N), defer=True)
            flushed(db2)
            assert torch.equal(dz2, dz) and torch.equal(db2, db), (N, dt)
            t, dx0, db = ops.cross_bwd_pre_colsum(x, x0, u, db=nan(N))
            t2, dx02, db2 = ops.cross_bwd_pre_colsum(x, x0, u, db=nan(N), defer=True)
            flushed(db2)
            assert torch.equal(t2, t) and torch.equal(dx02, dx0) and torch.equal(db2, db), (N, dt)
    N, K = 3, 20
    g = torch.Generator().manual_seed(M)
    dy, x = _rand(g, M, N).to(BF).to(DEV), _rand(g, M, K).to(BF).to(DEV)
    assert ops._skinny_h(N, K, x)
    now = ops.linear_bwd_weight(dy, x, out=nan(N, K))
    later, = flushed(ops.linear_bwd_weight(dy, x, out=nan(N, K), defer=True))
    assert torch.equal(later, now) and not bool(torch.isnan(now).any())


def test_bf16_wrappers_copy_a_column_strided_operand(ops):
    """The bf16 wrappers .contiguous() an operand with a non-unit column stride (ops.py: colsum "if x.stride(1) != 1",
    relu_mask_colsum, cross_bwd_pre_colsum, act_bwd likewise): equality with the dense call's summation order is owed
    all the same (the copy IS the dense operand), and the caller's tensor is untouched."""
    M, N = 70, 12
    g = torch.Generator().manual_seed(3)
    wide = _rand(g, M, 2 * N).to(BF).to(DEV)
    keep = wide.clone()
    dy = wide[:, ::2]
    assert dy.stride(1) == 2
    y, x0, u, z = (_rand(g, M, N).to(BF).to(DEV) for _ in range(4))
    dense = dy.contiguous()
    assert torch.equal(ops.colsum(dy), ops.colsum(dense))
    torch.testing.assert_close(ops.colsum(dy).cpu().double(), dense.cpu().double().sum(0), rtol=1e-5,
                               atol=1e-5 * float(dense.double().abs().sum(0).max()))
    for a, b in zip(ops.relu_mask_colsum(dy, y), ops.relu_mask_colsum(dense, y)):
        assert torch.equal(a, b)
    assert torch.equal(ops.relu_mask_colsum(dy, y)[0], torch.where(y > 0, dense, torch.zeros_like(dense)))
    for a, b in zip(ops.cross_bwd_pre_colsum(dy, x0, u), ops.cross_bwd_pre_colsum(dense, x0, u)):
        assert torch.equal(a, b)
    assert torch.equal(ops.cross_bwd_pre_colsum(dy, x0, u)[0], (dense.float() * x0.float()).to(BF))
    assert torch.equal(ops.act_bwd("tanh", dy, z), ops.act_bwd("tanh", dense, z))
    assert torch.equal(wide, keep)


# ============================================================================================ Tier A: activations
ACT_KINDS = ["tanh", "sigmoid", "none", "elu", "leu", "gelu", "gelu_new", "swish", "mish"]


@pytest.mark.parametrize("M,N", [(33, 12), (7, 5)])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ACT_KINDS)
def test_act(ops, kind, half, M, N):
    """act_fwd into a column slice, act_bwd from one.  (33, 12): rows of whole 4-element groups (the bf16 vector form),
    more than one block; (7, 5): the scalar form.  Bounds: test_hidden_act_kernels_and_mlp_vs_reference (fp32: y rtol
    2e-6 / atol 3e-7, dz rtol 1e-5 / atol 1e-6 per unit of dy), test_bf16_trans_kernels_gpu (the same plus 2^-8)."""
    from oracle import ref_model as R
    dt = BF if half else F32
    g = torch.Generator().manual_seed(M * N)
    z = (_rand(g, M, N) * 2).to(dt)
    dy = _rand(g, M, N).to(dt)
    z64 = z.double().requires_grad_(True)
    y_ref = R.act(kind, z64)
    (y_ref * dy.double()).sum().backward()
    extra, col0 = (8, 4) if N % 4 == 0 else (4, 3)
    gs = Guards()
    zg = gs.like(z, "z")
    yp = gs.out(M, N, dt, extra=extra, col0=col0, what="y")
    assert ops.act_fwd(kind, zg, out=yp) is yp
    dz = ops.act_bwd(kind, gs.inp(dy, extra + 4, col0=col0, what="dy"), zg)
    y2, dz2 = ops.act_fwd(kind, z.to(DEV)), ops.act_bwd(kind, dy.to(DEV), z.to(DEV))
    assert torch.equal(yp, y2) and torch.equal(dz, dz2)
    gs.check()
    ulp = HALF_ULP if half else 0.0
    _within(y2, y_ref.detach(), (2e-6 + ulp) * y_ref.detach().abs() + 3e-7, "y")
    _within(dz2, z64.grad, (1e-5 + ulp) * z64.grad.abs() + 1e-6 * dy.double().abs().clamp(min=1e-30), "dz")


# ============================================================================================ Tier A: CIN pieces
@pytest.mark.parametrize("accumulate", [False, True])
def test_cin_pieces(ops, accumulate):
    """B, F, E, H = 3, 5, 4, 7.  Bounds: test_cin_pieces, test_cin_outer_padded_row."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    B, F, E, H = 3, 5, 4, 7
    R, K = B * E, F * H
    g = torch.Generator().manual_seed(B * F + H)
    x0t, xi, dhad = _rand(g, R, F), _rand(g, R, H), _rand(g, R, K)
    prior, gpool, xprior = _rand(g, R, F), _rand(g, B, H), _rand(g, R, H)
    d = lambda t: t.to(DEV)
    # cin_outer_fwd owns its whole row: columns [F*H, ld) are zeroed by design (the pad_to = 8 operand path), so the
    # canaries start behind ld.  The wrapper allocates `had`: the C entry is called on a guarded one.
    for pad_to in (1, 8):
        ld = (K + pad_to - 1) // pad_to * pad_to
        gs = Guards()
        had = gs.out(R, ld, extra=0, what="had")
        check(lib.mapx_cin_outer_fwd(ptr(gs.like(x0t, "x0t")), F, ptr(gs.like(xi, "xi")), H, R, had.data_ptr(), ld, stream()))
        dense = ops.cin_outer_fwd(d(x0t), d(xi), pad_to=pad_to)
        assert dense.shape == (R, ld) and torch.equal(had, dense)
        gs.check()
        assert torch.equal(dense[:, :K].cpu(), (x0t[:, :, None] * xi[:, None, :]).reshape(R, K))
        assert bool((dense[:, K:] == 0.0).all()) and not bool(torch.signbit(dense[:, K:]).any())
    # cin_outer_bwd: dhad pitched.  The wrapper takes the [R, ld] matrix itself (its row stride is the pitch, the
    # columns behind F*H are not the kernel's to read: they hold canaries); a window of more than one row is refused
    gs = Guards()
    dx0t = gs.like(prior, "dx0t", dest=True)
    window = gs.inp(dhad, 5, what="dhad")
    with pytest.raises(AssertionError, match="contiguous"):
        ops.cin_outer_bwd(window, d(x0t), d(xi), d(prior).clone(), accumulate)
    dhad_p = gs.checks[-1].rows
    assert dhad_p.shape == (R, K + 5) and bool(torch.isnan(dhad_p[:, K:]).all())
    dxi = ops.cin_outer_bwd(dhad_p, gs.like(x0t, "x0t"), gs.like(xi, "xi"), dx0t, accumulate)
    dx0t2 = d(prior).clone()
    dxi2 = ops.cin_outer_bwd(d(dhad), d(x0t), d(xi), dx0t2, accumulate)
    assert torch.equal(dxi, dxi2) and torch.equal(dx0t, dx0t2)
    gs.check()
    d3 = dhad.view(R, F, H).double()
    torch.testing.assert_close(dxi2.cpu().double(), (d3 * x0t.double()[:, :, None]).sum(1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dx0t2.cpu().double(), (prior.double() if accumulate else 0) + (d3 * xi.double()[:, None, :]).sum(2),
                               rtol=1e-5, atol=1e-5)
    # cin_pool_fwd: out pitched
    gs = Guards()
    out = gs.out(B, H, extra=3, col0=2, what="pooled")
    ops.cin_pool_fwd(gs.like(xi, "xt"), B, E, out)
    dense = ops.cin_pool_fwd(d(xi), B, E, torch.empty(B, H, device=DEV))
    assert torch.equal(out, dense)
    gs.check()
    torch.testing.assert_close(dense.cpu(), xi.view(B, E, H).sum(1), rtol=1e-5, atol=1e-5)
    # cin_pool_bwd: g pitched
    gs = Guards()
    dxt = gs.like(xprior, "dxt", dest=True)
    ops.cin_pool_bwd(gs.inp(gpool, 3, col0=1, what="g"), B, E, dxt, accumulate)
    dense = ops.cin_pool_bwd(d(gpool), B, E, d(xprior).clone(), accumulate)
    assert torch.equal(dxt, dense)
    gs.check()
    want = gpool[:, None, :].expand(B, E, H) + (xprior.view(B, E, H) if accumulate else 0)
    assert torch.equal(dense.cpu().view(B, E, H), want)


# ============================================================================================ Tier A: fused CIN (bf16)
U_BF = 2.0 ** -8             # tests/test_bf16_xdeepfm_kernels_gpu.py


def _pad8_rows(gs, t, extra, what):
    """bf16 [R, n] -> the [R, pad8(n) + extra] operand of the fused CIN kernels: columns [n, pad8(n)) are zero (the
    kernels' contract), columns [pad8(n), pad8(n) + extra) hold canaries and are checked."""
    n8 = (t.shape[1] + 7) // 8 * 8
    z = torch.zeros(t.shape[0], n8, dtype=BF)
    z[:, :t.shape[1]] = t
    gs.inp(z, extra, what=what)
    return gs.checks[-1].rows


@pytest.mark.parametrize("extra", [0, 8], ids=["pad8", "pad8+8"])
def test_cin_fused(ops, extra):
    """B, E, F, H, U = 3, 4, 5, 7, 9; every activation with a pitch of pad8(width) and of pad8(width) + 8.
    Bounds: tests/test_bf16_xdeepfm_kernels_gpu.py."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    B, E, F, H, U = 3, 4, 5, 7, 9
    R = B * E
    g = torch.Generator().manual_seed(E * F * H * U)
    x3 = _rand(g, B, F, E).to(BF)
    x0 = x3.permute(0, 2, 1).reshape(R, F).contiguous()
    xi = _rand(g, R, H).to(BF)
    w = (_rand(g, U, F * H) * (F * H) ** -0.5).to(BF)
    bias = _rand(g, U) * 0.1
    dy = (_rand(g, R, U) * 0.05).to(BF)
    gpool = (_rand(g, B, H) * 0.05).to(BF)
    gu = (_rand(g, B, U) * 0.05).to(BF)
    prior = _rand(g, R, F) * 0.05
    d = lambda t: t.to(DEV)

    def pad(t):
        z = torch.zeros(t.shape[0], ops.pad8(t.shape[1]), dtype=BF)
        z[:, :t.shape[1]] = t
        return z.to(DEV)

    a = (x0.float()[:, :, None] * xi.float()[:, None, :]).to(BF).to(F64).reshape(R, -1)
    # ---- transpose: the wrapper allocates x0t; the C entry on a guarded one.  The kernel owns its whole row (it zeroes
    # the pad columns), so the canaries start behind ld.
    gs = Guards()
    ld = ops.pad8(F) + extra
    x0t_g = gs.out(R, ld, BF, extra=0, what="x0t")
    check(lib.mapx_cin_transpose_bf16(ptr(gs.like(x3, "x3")), B, F, E, x0t_g.data_ptr(), ld, stream()))
    x0t = ops.cin_transpose_bf16(d(x3))
    assert torch.equal(x0t_g[:, :ops.pad8(F)], x0t) and not bool(x0t_g[:, F:].float().abs().any())
    assert torch.equal(x0t.cpu(), pad(x0).cpu())
    gs.check()
    # ---- forward
    gs = Guards()
    x0t_p, xi_p = _pad8_rows(gs, x0, extra, "x0t"), _pad8_rows(gs, xi, extra, "xi")
    wg, bg = gs.like(w, "w"), gs.like(bias, "bias")
    y = ops.cin_fused_fwd(x0t_p, F, xi_p, H, wg, bg)
    y2 = ops.cin_fused_fwd(pad(x0), F, pad(xi), H, d(w), d(bias))
    assert y.shape == (R, ops.pad8(U)) and torch.equal(y, y2)
    gs.check()
    ref = a @ w.to(F64).t() + bias.to(F64)
    mag = a.abs() @ w.to(F64).abs().t() + bias.to(F64).abs()
    _within(y2[:, :U], ref, 4e-6 * mag + U_BF * ref.abs(), "Y")
    assert not bool(y2[:, U:].float().abs().any())
    # ---- pooling forward: y pitched, out a pitched column slice
    gs = Guards()
    y_p = _pad8_rows(gs, y2[:, :U].cpu(), extra, "y")
    out = gs.out(B, U, BF, extra=5, col0=3, what="pooled")
    ops.cin_pool_fwd_bf16(y_p, U, B, E, out)
    dense = ops.cin_pool_fwd_bf16(y2, U, B, E, torch.empty(B, U, dtype=BF, device=DEV))
    assert torch.equal(out, dense)
    gs.check()
    rows = y2[:, :U].cpu().to(F64).view(B, E, U)
    _within(dense, rows.sum(1), 2e-6 * rows.abs().sum(1) + U_BF * rows.sum(1).abs(), "pooled")
    # ---- pooling backward: g a pitched column slice; the wrapper allocates dy, the C entry on a guarded one
    gs = Guards()
    gu_p = gs.inp(gu, 5, col0=3, what="g")
    dyb = ops.cin_pool_bwd_bf16(gu_p, B, E)
    dyb2 = ops.cin_pool_bwd_bf16(d(gu), B, E)
    ldy = ops.pad8(U) + extra
    dy_g = gs.out(R, ldy, BF, extra=0, what="dy")
    check(lib.mapx_cin_pool_bwd_bf16(gu_p.data_ptr(), gu_p.stride(0), B, E, U, dy_g.data_ptr(), ldy, stream()))
    assert torch.equal(dyb, dyb2) and torch.equal(dy_g[:, :ops.pad8(U)], dyb2) and not bool(dy_g[:, U:].float().abs().any())
    gs.check()
    assert torch.equal(dyb2[:, :U].cpu(), gu.repeat_interleave(E, dim=0)) and not bool(dyb2[:, U:].float().abs().any())
    # ---- weight gradient: into a guarded slot
    gs = Guards()
    x0t_p, xi_p, dy_p = _pad8_rows(gs, x0, extra, "x0t"), _pad8_rows(gs, xi, extra, "xi"), _pad8_rows(gs, dy, extra, "dy")
    slot = gs.like(torch.zeros(U, F * H), "dw", dest=True)
    assert ops.cin_fused_bwd_weight(dy_p, U, x0t_p, F, xi_p, H, out=slot) is slot
    dw2 = ops.cin_fused_bwd_weight(pad(dy), U, pad(x0), F, pad(xi), H)
    assert torch.equal(slot, dw2)
    gs.check()
    _within(dw2, dy.to(F64).t() @ a, 2e-6 * (dy.to(F64).abs().t() @ a.abs()), "dW")
    # ---- input gradient: dx0t overwritten and accumulated, with a pooled gradient that is a pitched column slice
    dA = (dy.to(F64) @ w.to(F64)).view(R, F, H)
    magA = (dy.to(F64).abs() @ w.to(F64).abs()).view(R, F, H)
    x0d, xv = x0.to(F64), xi.to(F64)
    dxi, m_xi = torch.einsum("rhm,rh->rm", dA, x0d), torch.einsum("rhm,rh->rm", magA, x0d.abs())
    dx0, m_x0 = torch.einsum("rhm,rm->rh", dA, xv), torch.einsum("rhm,rm->rh", magA, xv.abs())
    gp = gpool.to(F64).repeat_interleave(E, dim=0)
    for acc, with_g in ((False, False), (True, True)):
        gs = Guards()
        x0t_p, xi_p, dy_p = _pad8_rows(gs, x0, extra, "x0t"), _pad8_rows(gs, xi, extra, "xi"), _pad8_rows(gs, dy, extra, "dy")
        d0 = gs.like(prior, "dx0t", dest=True)
        gpl = gs.inp(gpool, 5, col0=3, what="gpool") if with_g else None
        prev = ops.cin_fused_bwd_input(dy_p, U, gs.like(w, "w"), x0t_p, F, xi_p, H, d0, accumulate_x0=acc, gpool=gpl, E=E)
        d1 = d(prior).clone()
        prev2 = ops.cin_fused_bwd_input(pad(dy), U, d(w), pad(x0), F, pad(xi), H, d1, accumulate_x0=acc,
                                        gpool=d(gpool) if with_g else None, E=E)
        assert prev.shape == (R, ops.pad8(H)) and torch.equal(prev, prev2) and torch.equal(d0, d1)
        gs.check()
        below = dxi + (gp if with_g else 0)
        _within(prev2[:, :H], below, 4e-6 * (m_xi + (gp.abs() if with_g else 0)) + U_BF * below.abs(), "dY below")
        base = prior.to(F64) if acc else torch.zeros(R, F, dtype=F64)
        _within(d1, base + dx0, 4e-6 * (m_x0 + base.abs()), "dx0t")
        assert not bool(prev2[:, H:].float().abs().any())


# ============================================================================================ Tier A: row reductions
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_seg_reduce_rows_extra(ops, half):
    """n, V, W = 33, 7, 4 with ld = 12: the source rows are a window of a wider matrix, the extra scalar is a column
    of it.  Bounds: tests/test_backbone_kernels_gpu.py::test_seg_reduce_rows_extra."""
    n, V, W, ld, group = 33, 7, 4, 12, 1
    keys = RW.skewed_keys(n, V, n)
    g = torch.Generator().manual_seed(n + W)
    src = _rand(g, n, W).to(BF if half else F32)
    extra = _rand(g, n)
    uniq_ref, inv = torch.unique(keys, return_inverse=True)
    U = uniq_ref.numel()
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    assert plan.count() == U
    gs = Guards()
    srcp = gs.inp(src, ld - W - 4, col0=4, what="src")
    assert srcp.stride(0) == ld
    ex = gs.like(extra, "extra")
    rows, scal = ops.seg_reduce_rows_extra(plan, srcp, W, ex, group)
    rows2, scal2 = ops.seg_reduce_rows_extra(plan, src.to(DEV), W, extra.to(DEV), group)
    assert torch.equal(rows[:U], rows2[:U]) and torch.equal(scal[:U], scal2[:U])
    gs.check()
    s64 = src.double()
    ref = torch.zeros(U, W, dtype=F64).index_add_(0, inv, s64)
    scale = torch.zeros(U, W, dtype=F64).index_add_(0, inv, s64.abs())
    _within(rows2[:U], ref, 1e-6 * scale + 1e-6)
    ref1 = torch.zeros(U, dtype=F64).index_add_(0, inv, extra.double())
    scale1 = torch.zeros(U, dtype=F64).index_add_(0, inv, extra.double().abs())
    _within(scal2[:U], ref1, 1e-6 * scale1 + 1e-6)


@pytest.mark.parametrize("with_rows1", [True, False], ids=["rows1", "no-rows1"])
def test_pack_sparse(ops, with_rows1):
    """maxc larger and smaller than n_uniq; the wrapper allocates the message, so the C entry is called on guarded keys
    and rows.  Reference: the definition (tests/test_backbone_kernels_gpu.py::_pack_check), exact."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    n, V, W0 = 300, 40, 12
    keys = RW.skewed_keys(n, V, W0)
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    U = plan.count()
    uniq = torch.unique(keys)
    assert U == uniq.numel() and U > 8
    g = torch.Generator().manual_seed(W0)
    rows0 = _rand(g, n, W0)
    rows1 = _rand(g, n) if with_rows1 else None
    scale, pad_id = 1.0 / 3.0, -1
    sc = torch.tensor(scale, dtype=F32)
    Wp = W0 + 4 if with_rows1 else W0
    for maxc in (1, U - 1, U, U + 7):
        gs = Guards()
        r0 = gs.like(rows0, "rows0")
        r1 = gs.like(rows1, "rows1") if with_rows1 else None
        kg, rg = gs.vec(maxc, torch.int32, what="keys"), gs.vec(maxc * Wp, what="rows").view(maxc, Wp)
        check(lib.mapx_pack_sparse(ptr(plan.uniq), ptr(r0), W0, ptr(r1), ptr(plan.n_uniq), min(plan.uniq.shape[0], n), maxc,
                                   float(scale), pad_id, ptr(kg), ptr(rg), stream()))
        k2, rr2 = ops.pack_sparse(plan, rows0.to(DEV), None if rows1 is None else rows1.to(DEV), maxc, scale, pad_id=pad_id)
        assert torch.equal(kg, k2) and torch.equal(rg, rr2)
        gs.check()
        live = min(U, maxc)
        k2, rr2 = k2.cpu(), rr2.cpu()
        assert torch.equal(k2[:live], uniq[:live].to(torch.int32)) and bool((k2[live:] == pad_id).all())
        assert torch.equal(rr2[:live, :W0], rows0[:live] * sc) and not bool(rr2[live:].any())
        if with_rows1:
            assert torch.equal(rr2[:live, W0], rows1[:live] * sc) and not bool(rr2[:live, W0 + 1:].any())


@pytest.mark.parametrize("rows,cols,ld", [(7, 5, 12), (130, 72, 80)])
def test_amax(ops, rows, cols, ld):
    """amax with ld > cols.  A record leaves non-finite elements out, so NaN padding would hide a wrong pitch: the
    padding holds a finite value far above the tensor's maximum instead (the guards keep their canaries).
    Reference: exact (tests/test_amax_gpu.py)."""
    g = torch.Generator().manual_seed(rows + cols)
    x = _rand(g, rows, cols)
    gs = Guards()
    xp = gs.inp(x, ld - cols - 3, col0=3, pad_value=3.0e30, what="x")
    assert xp.stride(0) == ld
    rec, dense = ops.amax(xp), ops.amax(x.to(DEV))
    assert ops.amax_value(rec) == ops.amax_value(dense)       # (which of a record's slots a block raises is not pinned)
    gs.check()
    assert ops.amax_value(dense) == float(x.abs().max())


# ============================================================================================ Tier A: grouped encoder
def test_enc_grouped(ops, arith):
    """B, F, D = 7, 5, 24 (P = 32, L = int(0.3 F) = 1 as test_grouped_feat_encoder_matches_dense draws it; D % 8 == 0 is
    the entries' own rule).  Through ops `final` is pitched (w and the gradient slot go through native.ptr); the C
    entries are then called with final, w and the outputs pitched.  Bounds: test_grouped_feat_encoder_matches_dense."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    B, F, D, P = 7, 5, 24, 32
    L = int(F * 0.3)
    g = torch.Generator().manual_seed(B + F)
    final = _rand(g, B, D)
    w = _rand(g, F * P, D) / math.sqrt(D)
    b = _rand(g, F * P)
    mi = torch.randint(0, F, (B, L), generator=g)
    d = lambda t: t.to(DEV)
    groups = ops.EncGroups(d(mi), F)
    hpos = groups.hpos.cpu().long()
    h2 = ops.enc_grouped_fwd(d(final), d(w), d(b), groups)
    enc = (final.double() @ w.double().t() + b.double()).view(B, F, P)
    want = torch.gather(enc, 1, mi.unsqueeze(-1).expand(-1, -1, P)).view(B * L, P)
    bound = 2e-6 * (final.abs().double() @ w.abs().double().t()).max() + 1e-6
    assert float((h2.cpu()[hpos].double() - want).abs().max()) <= float(bound)
    dh = _rand(g, B * L, P)
    dh_slots = torch.zeros(groups.cap, P)
    dh_slots[hpos] = dh
    dw2 = ops.enc_grouped_dw(d(dh_slots), d(final), groups)
    denc = torch.zeros(B, F, P, dtype=F64)
    denc.scatter_add_(1, mi.unsqueeze(-1).expand(-1, -1, P), dh.view(B, L, P).double())
    torch.testing.assert_close(dw2.cpu().double(), denc.view(B, F * P).t() @ final.double(), rtol=0,
                               atol=4e-6 * float((denc.view(B, -1).abs().t() @ final.abs().double()).max()) + 1e-6)
    # through ops: final pitched (under AUTO_AMAX the wrappers take amax(final) through its pitch)
    gs = Guards()
    fp = gs.inp(final, 8, col0=4, what="final")
    h = ops.enc_grouped_fwd(fp, gs.like(w, "w"), gs.like(b, "b"), groups)
    dwg = gs.like(torch.zeros(F * P, D), "dw", dest=True)
    assert ops.enc_grouped_dw(gs.like(dh_slots, "dh_slots"), fp, groups, out=dwg) is dwg
    live = groups.rowmap >= 0
    assert torch.equal(h[live], h2[live]) and torch.equal(dwg, dw2)
    gs.check()
    # the C entries: w and the outputs pitched too
    gs = Guards()
    fp, wp = gs.inp(final, 8, col0=4, what="final"), gs.inp(w, 4, col0=8, what="w")
    hg = gs.vec(groups.cap * P, what="h_slots").view(groups.cap, P)
    dwp = gs.out(F * P, D, extra=12, col0=4, what="dw")
    dsg = gs.like(dh_slots, "dh_slots")
    sc_f = sc_w = None
    if arith == "h2":
        sc_f = ops._scale_arg(ops.amax(d(final)), ops.amax(d(w)))
        sc_w = ops._scale_arg(ops.amax(d(dh_slots)), ops.amax(d(final)))
    ref_ = lambda s: None if s is None else ops.native_byref(s)
    check(lib.mapx_enc_grouped_fwd(fp.data_ptr(), fp.stride(0), B, D, wp.data_ptr(), wp.stride(0), ptr(d(b)),
                                   ptr(groups.rowmap), ptr(groups.tile_group), ptr(groups.group_start), F, groups.cap,
                                   ptr(hg), None, ref_(sc_f), stream()))
    check(lib.mapx_enc_grouped_dw(ptr(dsg), fp.data_ptr(), fp.stride(0), B, D, ptr(groups.rowmap), ptr(groups.group_start),
                                  F, None, dwp.data_ptr(), dwp.stride(0), ref_(sc_w), stream()))
    assert torch.equal(hg[live], h2[live]) and torch.equal(dwp, dw2)
    gs.check()


# ============================================================================================ Tier B
# Kernels that map several rows or groups to a wave and write a contiguous output whose last wave or block is partial.
# The wrappers allocate their outputs, so the C entries are called on guarded ones (front and back guards, ld = width)
# and compared bit for bit with the wrapper's result; counts sit one below and one above the kernel's rows per wave /
# per block, at widths other than 16 (row_widths_ref.ROW_WIDTHS).
TIER_B = [
    ("mapx_emb_gather_fwd", "test_emb_gather_extent"), ("mapx_emb_gather_fwd_bf16", "test_emb_gather_extent"),
    ("mapx_seg_reduce_rows", "test_seg_reduce_rows_extent"), ("mapx_seg_reduce_rows_bf16", "test_seg_reduce_rows_extent"),
    ("mapx_fm_fwd", "test_fm_extent"), ("mapx_fm_bwd", "test_fm_extent"),
    ("mapx_fm_fwd_bf16", "test_fm_extent"), ("mapx_fm_bwd_bf16", "test_fm_extent"),
    ("mapx_attn_fwd", "test_attn_extent"), ("mapx_attn_bwd", "test_attn_extent"),
    ("mapx_attn_fwd_bf16", "test_attn_extent"), ("mapx_attn_bwd_bf16", "test_attn_extent"),
    ("mapx_mha_fwd", "test_mha_extent"), ("mapx_mha_bwd", "test_mha_extent"),
    ("mapx_mha_fwd_bf16", "test_mha_extent"), ("mapx_mha_bwd_bf16", "test_mha_extent"),
    ("mapx_field_pool_fwd", "test_field_pool_extent"), ("mapx_field_pool_bwd", "test_field_pool_extent"),
    ("mapx_field_pool_fwd_bf16", "test_field_pool_extent"), ("mapx_field_pool_bwd_bf16", "test_field_pool_extent"),
    ("mapx_layernorm_fwd", "test_layernorm_extent"), ("mapx_layernorm_bwd", "test_layernorm_extent"),
    ("mapx_add_layernorm_fwd_bf16", "test_add_layernorm_bf16_extent"),
    ("mapx_add_layernorm_bwd_bf16", "test_add_layernorm_bf16_extent"),
    ("mapx_inner_product_fwd", "test_inner_product_extent"), ("mapx_inner_product_bwd", "test_inner_product_extent"),
]


def test_tier_b_table_names_tests_and_entries(ops):
    for entry, test in TIER_B:
        assert callable(globals().get(test)), test
        assert hasattr(ops.lib, entry), entry


def _out(gs, shape, dtype=F32, what="output"):
    return gs.vec(math.prod(shape), dtype, what=what).view(shape)


def _close(got, want, rtol, atol, ulp=0.0, what=""):
    want = want.detach().double()
    _within(got, want.reshape(got.shape), (rtol + ulp) * want.reshape(got.shape).abs() + atol, what)


assert all(E in RW.ROW_WIDTHS for E in (8, 24))

# emb_gather_kernel<4>: E / 4 lanes per row -> E = 8: 32 rows per wave, 128 per block; E = 24: 10 2/3 rows per wave (rows
# straddle waves), 42 2/3 per block.  emb_gather_bf16_kernel: E / 8 lanes per row -> E = 8: 64 / 256; E = 24: 21 1/3 / 85 1/3.
GATHER_CASES = [(n, 8, False) for n in (31, 33, 127, 129)] + [(n, 24, False) for n in (10, 11, 42, 43)] + \
               [(n, 8, True) for n in (63, 65, 255, 257)] + [(n, 24, True) for n in (21, 22, 85, 86)]


@pytest.mark.parametrize("n,E,half", GATHER_CASES)
def test_emb_gather_extent(ops, n, E, half):
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    V = 50
    g = torch.Generator().manual_seed(n + E)
    ids, table = torch.randint(0, V, (n,), generator=g), _rand(g, V, E)
    gs = Guards()
    idg, tg = gs.like(ids, "ids"), gs.like(table, "table")
    out = _out(gs, (n, E), BF if half else F32, "rows")
    if half:
        check(lib.mapx_emb_gather_fwd_bf16(ptr(idg), n, ptr(tg), V, E, ptr(out), None, None, stream()))
    else:
        check(lib.mapx_emb_gather_fwd(ptr(idg), n, ptr(tg), V, E, ptr(out), None, None, None, stream()))
    dense = ops.emb_gather(ids.to(DEV), table.to(DEV), out_dtype=BF if half else F32)
    assert torch.equal(out, dense)
    gs.check()
    assert torch.equal(dense.cpu(), table[ids].to(dense.dtype))


# seg_reduce_launch: LG = 4 (W = 8) / 8 (W = 24) lanes per row, kSegChunkSmall = 16 sorted positions per lane group
SEG_CASES = [(15, 7, 8, False), (17, 7, 8, False), (33, 7, 24, False), (33, 7, 8, True), (17, 7, 24, True)]


@pytest.mark.parametrize("n,V,W,half", SEG_CASES)
def test_seg_reduce_rows_extent(ops, n, V, W, half):
    """`out` has capacity n rows: the guard stands behind row n; the workspace is exactly
    mapx_seg_reduce_workspace_bytes long.  Bounds: test_seg_plan_and_reduce_rows / test_bf16_backbone_kernels_gpu."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    keys = RW.skewed_keys(n, V, n)
    g = torch.Generator().manual_seed(n + W)
    src = _rand(g, n, W).to(BF if half else F32)
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    uniq_ref, inv = torch.unique(keys, return_inverse=True)
    U = plan.count()
    assert U == uniq_ref.numel()
    dense = ops.seg_reduce_rows(plan, src.to(DEV), W)
    nb = lib.mapx_seg_reduce_workspace_bytes(n, W)
    assert nb > 0
    gs = Guards()
    ws, out = gs.vec(nb, torch.uint8, what="workspace"), _out(gs, (n, W), what="rows")
    fn = lib.mapx_seg_reduce_rows_bf16 if half else lib.mapx_seg_reduce_rows
    check(fn(n, ptr(plan.perm), ptr(plan.rank), ptr(plan.seg_start), ptr(gs.like(src, "src")), None, W, ptr(out), ptr(ws),
             nb, None, stream()))
    assert torch.equal(out[:U], dense[:U])
    gs.check()
    s64 = src.double()
    ref = torch.zeros(U, W, dtype=F64).index_add_(0, inv, s64)
    scale = torch.zeros(U, W, dtype=F64).index_add_(0, inv, s64.abs())
    if half:
        _close(dense[:U], ref, 1e-5, 2e-5)
    else:
        _within(dense[:U], ref, 1e-6 * scale + 1e-6)


# fm_fwd_kernel<E>: E lanes per sample -> E = 8: 8 samples per wave, 32 per block
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [7, 9, 31, 33])
def test_fm_extent(ops, B, half):
    """Bounds: tests/test_backbone_kernels_gpu.py::test_fm_matches_float64_torch (FM_C = 1e-6)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    F, E = 5, 8
    g_ = torch.Generator().manual_seed(B * 131 + F * 7 + E)
    x, g = _rand(g_, B, F, E).to(BF if half else F32), _rand(g_, B)
    fm2, s2 = ops.fm_fwd(x.to(DEV))
    dx2 = ops.fm_bwd(g.to(DEV), s2, x.to(DEV))
    gs = Guards()
    xg, gg = gs.like(x, "x"), gs.like(g, "g")
    fm, s, dx = _out(gs, (B,), what="fm"), _out(gs, (B, E), what="s"), _out(gs, (B, F, E), x.dtype, "dx")
    fwd, bwd = (lib.mapx_fm_fwd_bf16, lib.mapx_fm_bwd_bf16) if half else (lib.mapx_fm_fwd, lib.mapx_fm_bwd)
    check(fwd(ptr(xg), B, F, E, ptr(fm), ptr(s), stream()))
    check(bwd(ptr(gg), ptr(s), ptr(xg), B, F, E, ptr(dx), stream()))
    assert torch.equal(fm, fm2) and torch.equal(s, s2) and torch.equal(dx, dx2)
    gs.check()
    x64, g64 = x.double(), g.double()
    sr, sa = x64.sum(1), x64.abs().sum(1)
    _within(fm2, 0.5 * (sr * sr - (x64 * x64).sum(1)).sum(1), 1e-6 * 0.5 * (sa * sa + (x64 * x64).sum(1)).sum(1) + 1e-6)
    _within(s2, sr, 1e-6 * sa + 1e-6)
    dx_ref = g64[:, None, None] * (sr[:, None, :] - x64)
    _within(dx2, dx_ref, 1e-6 * g64.abs()[:, None, None] * (sa[:, None, :] + x64.abs()) + 1e-6
            + (HALF_ULP * dx_ref.abs() if half else 0))


# attn_*_kernel<2> (F <= 32): two groups per wave
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", [1, 3])
def test_attn_extent(ops, G, half):
    """F, A = 5, 4; G = groups per wave - 1 and + 1.  Bounds: test_attn_matches_float64_torch (P_TOL, O_TOL, GRAD_TOL),
    plus half a bf16 ulp on the bf16 outputs (test_bf16_backbone_kernels_gpu)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    F, A, dt = 5, 4, BF if half else F32
    g = torch.Generator().manual_seed(1000 * G + 10 * F + A)
    q, k, v, d_o = (_rand(g, G * F * A).to(dt) for _ in range(4))
    d = lambda t: t.to(DEV)
    o2, p2 = ops.attn_fwd(d(q), d(k), d(v), G, F, A, True)
    grads2 = ops.attn_bwd(d(q), d(k), d(v), p2, d(d_o), G, F, A, True)
    gs = Guards()
    qg, kg, vg, dog = (gs.like(t, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (d_o, "d_o")))
    o, p = _out(gs, (G * F * A,), dt, "o"), _out(gs, (G, F, F), what="p")
    dq, dk, dv = (_out(gs, (G * F * A,), dt, n) for n in ("dq", "dk", "dv"))
    fwd, bwd = (lib.mapx_attn_fwd_bf16, lib.mapx_attn_bwd_bf16) if half else (lib.mapx_attn_fwd, lib.mapx_attn_bwd)
    check(fwd(ptr(qg), ptr(kg), ptr(vg), G, F, A, 1, ptr(o), ptr(p), stream()))
    check(bwd(ptr(qg), ptr(kg), ptr(vg), ptr(p), ptr(dog), G, F, A, 1, ptr(dq), ptr(dk), ptr(dv), stream()))
    assert torch.equal(o, o2) and torch.equal(p, p2)
    assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), grads2))
    gs.check()
    q6, k6, v6 = (t.double().view(G, F, A).requires_grad_(True) for t in (q, k, v))
    pr = torch.softmax(q6 @ k6.transpose(1, 2) / A ** 0.5, dim=-1)
    orf = pr @ v6
    (orf * d_o.double().view(G, F, A)).sum().backward()
    ulp = HALF_ULP if half else 0.0
    _close(p2, pr, 1e-5, 1e-6)
    _close(o2, orf.reshape(-1), 1e-5, 1e-5, ulp)
    for got, want in zip(grads2, (q6.grad, k6.grad, v6.grad)):
        _close(got, want.reshape(-1), 1e-4, 2e-5, ulp)


# mha_*_kernel<2, ...> (F <= 32): two (sample, head) groups per wave; G = B * H
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,F,E,H", [(1, 5, 8, 1), (1, 5, 12, 3), (3, 5, 8, 1)])
def test_mha_extent(ops, B, F, E, H, half):
    """p = 0.  Bounds: tests/test_mha_gpu.py (P 1e-5 / 1e-6, O 1e-5 / 1e-5, d_qkv 1e-4 / 2e-5), plus half a bf16 ulp on
    the bf16 outputs (test_bf16_trans_kernels_gpu)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    dt, dh = BF if half else F32, E // H
    g = torch.Generator().manual_seed(B * 100 + F * 10 + E + H)
    qkv, d_o = _rand(g, B * F, 3 * E).to(dt), _rand(g, B * F, E).to(dt)
    o2, p2 = ops.mha_fwd(qkv.to(DEV), B, F, E, H)
    d2 = ops.mha_bwd(qkv.to(DEV), p2, d_o.to(DEV), B, F, E, H)
    gs = Guards()
    qg, dog = gs.like(qkv, "qkv"), gs.like(d_o, "d_o")
    o, p, dq = _out(gs, (B * F, E), dt, "o"), _out(gs, (B * H, F, F), what="probs"), _out(gs, (B * F, 3 * E), dt, "d_qkv")
    fwd, bwd = (lib.mapx_mha_fwd_bf16, lib.mapx_mha_bwd_bf16) if half else (lib.mapx_mha_fwd, lib.mapx_mha_bwd)
    check(fwd(ptr(qg), B, F, E, H, 0.0, 0, 0, None, ptr(o), ptr(p), stream()))
    check(bwd(ptr(qg), ptr(p), ptr(dog), B, F, E, H, 0.0, 0, 0, None, ptr(dq), stream()))
    assert torch.equal(o, o2) and torch.equal(p, p2) and torch.equal(dq, d2)
    gs.check()
    q64 = qkv.double().requires_grad_(True)
    heads = lambda t: t.view(B, F, H, dh).permute(0, 2, 1, 3)                 # [B, H, F, dh]
    qh, kh, vh = heads(q64[:, :E]), heads(q64[:, E:2 * E]), heads(q64[:, 2 * E:])
    pr = torch.softmax(qh @ kh.transpose(-1, -2) / dh ** 0.5, dim=-1)
    orf = (pr @ vh).permute(0, 2, 1, 3).reshape(B * F, E)
    (orf * d_o.double()).sum().backward()
    ulp = HALF_ULP if half else 0.0
    _close(p2, pr.reshape(B * H, F, F), 1e-5, 1e-6)
    _close(o2, orf, 1e-5, 1e-5, ulp)
    _close(d2, q64.grad, 1e-4, 2e-5, ulp)


# field_pool_*_kernel: kPoolLanes = 16 lanes per sample -> 4 samples per wave, 16 per block
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [3, 5, 15, 17])
def test_field_pool_extent(ops, B, half):
    """F, E = 5, 24; each mode.  Bounds: tests/test_mha_gpu.py (pooled 1e-5 / 1e-5, dx 1e-5 / 1e-6, weights 1e-5 / 1e-7,
    d_scores 1e-4 / 1e-5), plus half a bf16 ulp on the bf16 outputs."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    F, E, dt = 5, 24, BF if half else F32
    g_ = torch.Generator().manual_seed(B + F + E)
    x, g, scores = _rand(g_, B, F, E).to(dt), _rand(g_, B, E).to(dt), _rand(g_, B, F)
    fwd, bwd = (lib.mapx_field_pool_fwd_bf16, lib.mapx_field_pool_bwd_bf16) if half \
        else (lib.mapx_field_pool_fwd, lib.mapx_field_pool_bwd)
    ulp = HALF_ULP if half else 0.0
    for mode in ("sum", "mean", "attn"):
        m, attn = ops.POOL_MODES[mode], mode == "attn"
        out2, w2 = ops.field_pool_fwd(x.to(DEV), mode, scores.to(DEV) if attn else None)
        dx2, ds2 = ops.field_pool_bwd(g.to(DEV), x.to(DEV), mode, w2)
        gs = Guards()
        xg, gg, sg = gs.like(x, "x"), gs.like(g, "g"), gs.like(scores, "scores")
        out, dx = _out(gs, (B, E), dt, "pooled"), _out(gs, (B, F, E), dt, "dx")
        w = _out(gs, (B, F), what="weights") if attn else None
        ds = _out(gs, (B, F), what="d_scores") if attn else None
        check(fwd(ptr(xg), ptr(sg) if attn else None, B, F, E, m, ptr(out), ptr(w), stream()))
        check(bwd(ptr(gg), ptr(xg), ptr(w), B, F, E, m, ptr(dx), ptr(ds), stream()))
        assert torch.equal(out, out2) and torch.equal(dx, dx2), mode
        assert not attn or (torch.equal(w, w2) and torch.equal(ds, ds2))
        gs.check()
        x64, s64 = x.double().requires_grad_(True), scores.double().requires_grad_(True)
        wr = torch.softmax(s64, 1) if attn else torch.full((B, F), 1.0 if mode == "sum" else 1.0 / F, dtype=F64)
        ref = (wr[:, :, None] * x64).sum(1)
        (ref * g.double()).sum().backward()
        _close(out2, ref, 1e-5, 1e-5, ulp, mode)
        _close(dx2, x64.grad, 1e-5, 1e-6, ulp, mode)
        if attn:
            _close(w2, wr, 1e-5, 1e-7)
            _close(ds2, s64.grad, 1e-4, 1e-5)


# layernorm_*_kernel<LG>: LG = 4 lanes per row for E <= 16 (16 rows per wave, 64 per block), 8 for E <= 32 (8 / 32).
# (The suggested (R, E) = (5, 6) is refused by the entries' own check, E % 4 == 0: E = 8 takes its place.)
LN_CASES = [(5, 8), (15, 8), (17, 8), (65, 12), (7, 24), (9, 24), (33, 24)]
LN_EPS = 1e-12


def _ln_ref(x, s, w, b, dy):
    """float64 LayerNorm of x (+ s): (y, stats [R, 2], d(x + s), dw, db)."""
    v = (x.double() + (s.double() if s is not None else 0)).requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(v, (v.shape[1],), w64, b64, LN_EPS)
    (y * dy.double()).sum().backward()
    mean, var = v.detach().mean(1), v.detach().var(1, unbiased=False)
    return y.detach(), torch.stack([mean, (var + LN_EPS).rsqrt()], 1), v.grad, w64.grad, b64.grad


@pytest.mark.parametrize("R,E", LN_CASES)
def test_layernorm_extent(ops, R, E):
    """y, stats [R, 2], dx and dy * xhat all guarded.  Bounds: test_layernorm_vs_torch (y 2e-5 / 2e-5, dx 1e-4 / 1e-4,
    column sums of dy * xhat 1e-4 / 1e-3); stats 2e-5 relative (test_bf16_trans_kernels_gpu)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    g = torch.Generator().manual_seed(R + E)
    x, dy = _rand(g, R, E) + 1.0, _rand(g, R, E)
    w, b = _rand(g, E), _rand(g, E)
    d = lambda t: t.to(DEV)
    y2, st2 = ops.layernorm_fwd(d(x), d(w), d(b), LN_EPS)
    dx2, dyx2 = ops.layernorm_bwd(d(dy), d(x), d(w), st2)
    gs = Guards()
    xg, dyg, wg, bg = gs.like(x, "x"), gs.like(dy, "dy"), gs.like(w, "w"), gs.like(b, "b")
    y, st = _out(gs, (R, E), what="y"), _out(gs, (R, 2), what="stats")
    dx, dyx = _out(gs, (R, E), what="dx"), _out(gs, (R, E), what="dy*xhat")
    check(lib.mapx_layernorm_fwd(ptr(xg), R, E, ptr(wg), ptr(bg), LN_EPS, ptr(y), ptr(st), stream()))
    check(lib.mapx_layernorm_bwd(ptr(dyg), ptr(xg), ptr(wg), ptr(st), R, E, ptr(dx), ptr(dyx), stream()))
    assert torch.equal(y, y2) and torch.equal(st, st2) and torch.equal(dx, dx2) and torch.equal(dyx, dyx2)
    gs.check()
    y_ref, st_ref, dv_ref, dw_ref, _ = _ln_ref(x, None, w, b, dy)
    _close(y2, y_ref, 2e-5, 2e-5)
    _close(st2, st_ref, 2e-5, 0.0)
    _close(dx2, dv_ref, 1e-4, 1e-4)
    _close(dyx2.double().sum(0), dw_ref, 1e-4, 1e-3)


@pytest.mark.parametrize("R,E", LN_CASES)
@pytest.mark.parametrize("with_s", [False, True], ids=["ln", "add-ln"])
def test_add_layernorm_bf16_extent(ops, R, E, with_s):
    """The bf16 residual add + LayerNorm; the backward's partial rows are guarded behind exactly
    mapx_add_layernorm_bwd_groups rows.  Bounds: test_bf16_trans_kernels_gpu (y 2e-5 / 2e-5 + 2^-8, stats 2e-5,
    dsum 1e-4 / 1e-4 + 2^-8, dgamma / dbeta 1e-4 / 1e-3)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    g = torch.Generator().manual_seed(R + E + int(with_s))
    x, dy = (_rand(g, R, E) + 1.0).to(BF), _rand(g, R, E).to(BF)
    s = _rand(g, R, E).to(BF) if with_s else None
    w, b = _rand(g, E), _rand(g, E)
    d = lambda t: None if t is None else t.to(DEV)
    y2, st2 = ops.add_layernorm_fwd(d(x), d(s), d(w), d(b), LN_EPS)
    dsum2, dw2, db2 = ops.add_layernorm_bwd(d(dy), d(x), d(s), d(w), st2)
    gs = Guards()
    xg, dyg, wg, bg = gs.like(x, "x"), gs.like(dy, "dy"), gs.like(w, "w"), gs.like(b, "b")
    sg = gs.like(s, "s") if with_s else None
    y, st, dsum = _out(gs, (R, E), BF, "y"), _out(gs, (R, 2), what="stats"), _out(gs, (R, E), BF, "dsum")
    groups = lib.mapx_add_layernorm_bwd_groups(R, E)
    assert groups >= 1
    part = _out(gs, (groups, 2 * E), what="partial rows")
    check(lib.mapx_add_layernorm_fwd_bf16(ptr(xg), ptr(sg), R, E, ptr(wg), ptr(bg), LN_EPS, ptr(y), ptr(st), stream()))
    check(lib.mapx_add_layernorm_bwd_bf16(ptr(dyg), ptr(xg), ptr(sg), ptr(wg), ptr(st), R, E, ptr(dsum), ptr(part), stream()))
    dw, db = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    ops._sum_now(dw, part, 2 * E, groups, E)
    ops._sum_now(db, part[:, E:], 2 * E, groups, E)
    assert torch.equal(y, y2) and torch.equal(st, st2) and torch.equal(dsum, dsum2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    gs.check()
    y_ref, st_ref, dv_ref, dw_ref, db_ref = _ln_ref(x, s, w, b, dy)
    _close(y2, y_ref, 2e-5, 2e-5, HALF_ULP)
    _close(st2, st_ref, 2e-5, 0.0)
    _close(dsum2, dv_ref, 1e-4, 1e-4, HALF_ULP)
    _close(dw2, dw_ref, 1e-4, 1e-3)
    _close(db2, db_ref, 1e-4, 1e-3)


# inner_product_*_kernel: one workgroup per sample; rows r and T - 2 - r of the pair triangle share a line (odd and even T)
@pytest.mark.parametrize("B,T,E", [(3, 5, 8), (2, 4, 12), (1, 2, 4), (2, 3, 24)])
def test_inner_product_extent(ops, B, T, E):
    """Bounds: tests/test_fgcnn_kernels_gpu.py (FWD_TOL 1e-5 / 1e-5, GRAD_TOL 1e-4 / 2e-5)."""
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    P = T * (T - 1) // 2
    g_ = torch.Generator().manual_seed(B + T + E)
    x, g = _rand(g_, B, T, E), _rand(g_, B, P)
    out2 = ops.inner_product_fwd(x.to(DEV))
    dx2 = ops.inner_product_bwd(g.to(DEV), x.to(DEV))
    gs = Guards()
    xg, gg = gs.like(x, "x"), gs.like(g, "g")
    out, dx = _out(gs, (B, P), what="pairs"), _out(gs, (B, T, E), what="dx")
    check(lib.mapx_inner_product_fwd(ptr(xg), B, T, E, ptr(out), stream()))
    check(lib.mapx_inner_product_bwd(ptr(gg), ptr(xg), B, T, E, ptr(dx), stream()))
    assert torch.equal(out, out2) and torch.equal(dx, dx2)
    gs.check()
    x64 = x.double().requires_grad_(True)
    i, j = torch.triu_indices(T, T, offset=1)
    ref = (x64[:, i, :] * x64[:, j, :]).sum(-1)
    (ref * g.double()).sum().backward()
    _close(out2, ref, 1e-5, 1e-5)
    _close(dx2, x64.grad, 1e-4, 2e-5)
