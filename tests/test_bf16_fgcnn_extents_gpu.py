"""Guard-band cases for the bf16 I/O forms of csrc/fgcnn.hip (the rules of tests/test_extents_gpu.py): every operand and
output of a call lives inside a tests/guarded.py buffer, and each case asserts that
  1. the canaries of every guarded output and input are untouched (a 2-byte element type halves every byte offset: a
     kernel that kept an fp32 index would write past the end of its bf16 output, or read the guard's NaN),
  2. the values are bit-equal to the same call through mapx.ops on dense, exactly-sized tensors.
The values themselves are held to their bounds against float64 in tests/test_bf16_fgcnn_kernels_gpu.py.
inner_product_bwd_bf16 is the one entry that takes a row pitch: its gradient is a window of a wider guarded matrix, at
odd and even column offsets and pitches (2-byte aligned rows)."""
import pytest
import torch

from test_extents_gpu import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8

ENTRIES = ["mapx_fgcnn_conv_fwd_bf16", "mapx_fgcnn_pool_fwd_bf16", "mapx_fgcnn_pool_bwd_bf16",
           "mapx_fgcnn_conv_bwd_bf16", "mapx_inner_product_fwd_bf16", "mapx_inner_product_bwd_bf16"]


def test_every_bf16_entry_of_the_file_is_exported():
    from mapx import ops
    for e in ENTRIES:
        assert hasattr(ops.lib, e), e


def _out(gs, shape, dtype, what):
    n = 1
    for s in shape:
        n *= s
    return gs.vec(n, dtype, what=what).view(shape)


# B, Cin, Cout, H, kh, ps, E, act: B % 4 != 0 (conv_bwd groups 4 samples), kh > H, odd H with padding, E = 4 (one
# 8-byte chunk per row) and 8
STAGES = [(5, 2, 3, 7, 3, 2, 8, "tanh"), (3, 1, 2, 2, 3, 2, 4, "relu"), (6, 3, 2, 7, 5, 3, 4, "relu")]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,Cin,Cout,H,kh,ps,E,act", STAGES)
def test_stage_extent(B, Cin, Cout, H, kh, ps, E, act, training):
    from mapx import ops
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    a = ops.FGCNN_ACTS[act]
    g_ = torch.Generator().manual_seed(B + H + E)
    rnd = lambda *s: torch.randn(*s, generator=g_)
    x, w, b = rnd(B, Cin, H, E).to(BF).to(DEV), (rnd(Cout, Cin, kh, 1) * 0.5).to(DEV), (0.1 * rnd(Cout)).to(DEV)
    ga, be = (1 + 0.2 * rnd(Cout)).to(DEV), (0.2 * rnd(Cout)).to(DEV)
    rm, rv = (0.3 * rnd(Cout)).to(DEV), (0.5 + torch.rand(Cout, generator=g_)).to(DEV)
    _, Hp = ops.fgcnn_pool_shape(H, ps)
    dy = rnd(B, Cout, Hp, E).to(BF).to(DEV)
    # dense
    z2, part2 = ops.fgcnn_conv_fwd(x, w, b, stats=training)
    if training:
        stats = ops.fgcnn_bn_stats(part2, H, E)
        y2, idx2 = ops.fgcnn_pool_fwd(z2, ga, be, ps, act, stats=stats)
        dx2, dw2, db2, dga2, dbe2 = ops.fgcnn_bwd(dy, idx2, z2, x, w, stats, ga, be, ps, act)
    else:
        y2, idx2 = ops.fgcnn_pool_fwd(z2, ga, be, ps, act, running_mean=rm, running_var=rv, save=False)
    # guarded
    gs = Guards()
    xg, wg, bg, gag, beg = gs.like(x, "x"), gs.like(w, "w"), gs.like(b, "bias"), gs.like(ga, "gamma"), gs.like(be, "beta")
    z = _out(gs, (B, Cout, H, E), BF, "z")
    part = _out(gs, (B, Cout, 2), F64, "part") if training else None
    check(lib.mapx_fgcnn_conv_fwd_bf16(ptr(xg), ptr(wg), ptr(bg), B, Cin, Cout, H, E, kh, ptr(z), ptr(part), stream()))
    assert torch.equal(z, z2)
    y = _out(gs, (B, Cout, Hp, E), BF, "y")
    if not training:
        rmg, rvg = gs.like(rm, "running_mean"), gs.like(rv, "running_var")
        check(lib.mapx_fgcnn_pool_fwd_bf16(ptr(z), None, ptr(rmg), ptr(rvg), ops.BN_EPS, ptr(gag), ptr(beg), B, Cout, H,
                                           E, ps, a, ptr(y), None, stream()))
        assert torch.equal(y, y2)
        gs.check()
        return
    assert torch.equal(part, part2)
    sg = gs.like(stats, "stats")
    idx = _out(gs, (B, Cout, Hp, E), U8, "idx")
    check(lib.mapx_fgcnn_pool_fwd_bf16(ptr(z), ptr(sg), None, None, ops.BN_EPS, ptr(gag), ptr(beg), B, Cout, H, E, ps,
                                       a, ptr(y), ptr(idx), stream()))
    assert torch.equal(y, y2) and torch.equal(idx, idx2)
    dyg = gs.like(dy, "dy")
    g = _out(gs, (B, Cout, H, E), F32, "g")
    bpart = _out(gs, (B, Cout, 2), F64, "backward part")
    check(lib.mapx_fgcnn_pool_bwd_bf16(ptr(dyg), ptr(idx), ptr(z), ptr(sg), ptr(gag), ptr(beg), B, Cout, H, E, ps, a,
                                       ptr(g), ptr(bpart), stream()))
    bsum, dga, dbe = _out(gs, (Cout, 2), F32, "bsum"), _out(gs, (Cout,), F32, "dgamma"), _out(gs, (Cout,), F32, "dbeta")
    check(lib.mapx_fgcnn_bn_bwd_sums(ptr(bpart), B, Cout, H, E, ptr(bsum), ptr(dga), ptr(dbe), stream()))
    G = lib.mapx_fgcnn_conv_bwd_groups(B)
    nw = Cout * Cin * kh
    pw, pb = _out(gs, (G, nw), F32, "part_w"), _out(gs, (G, Cout), F32, "part_b")
    dx, dw, db = _out(gs, (B, Cin, H, E), BF, "dx"), _out(gs, (nw,), F32, "dw"), _out(gs, (Cout,), F32, "db")
    check(lib.mapx_fgcnn_conv_bwd_bf16(ptr(g), ptr(z), ptr(xg), ptr(wg), ptr(sg), ptr(gag), ptr(bsum), B, Cin, Cout, H,
                                       E, kh, ptr(dx), ptr(pw), ptr(pb), ptr(dw), ptr(db), stream()))
    assert torch.equal(dx, dx2) and torch.equal(dw.view(dw2.shape), dw2) and torch.equal(db, db2)
    assert torch.equal(dga, dga2) and torch.equal(dbe, dbe2)
    gs.check()


# B, T, E, columns in front of g, columns behind it: T(T-1)/2 odd (3, 15, 21) and even (6); pitch and offset odd and even
IP = [(3, 3, 8, 1, 3), (2, 6, 4, 0, 0), (3, 7, 8, 24, 0), (1, 2, 4, 3, 1), (2, 4, 12, 5, 2)]


@pytest.mark.parametrize("B,T,E,front,back", IP)
def test_inner_product_extent(B, T, E, front, back):
    from mapx import ops
    from mapx.native import MapxError
    lib, ptr, check, stream = ops.lib, ops.ptr, ops.check, ops.stream
    P = T * (T - 1) // 2
    g_ = torch.Generator().manual_seed(B + T + E)
    x, g = torch.randn(B, T, E, generator=g_).to(BF).to(DEV), torch.randn(B, P, generator=g_).to(BF).to(DEV)
    out2 = ops.inner_product_fwd(x)
    dx2 = ops.inner_product_bwd(g, x)
    gs = Guards()
    xg = gs.like(x, "x")
    gg = gs.inp(g, extra=back, col0=front, what="g")
    assert gg.stride(0) == front + P + back
    out, dx = _out(gs, (B, P), BF, "pairs"), _out(gs, (B, T, E), BF, "dx")
    check(lib.mapx_inner_product_fwd_bf16(ptr(xg), B, T, E, ptr(out), stream()))
    check(lib.mapx_inner_product_bwd_bf16(gg.data_ptr(), gg.stride(0), ptr(xg), B, T, E, ptr(dx), stream()))
    assert torch.equal(out, out2) and torch.equal(dx, dx2)
    assert torch.equal(ops.inner_product_bwd(gg, x), dx2)              # the wrapper reads the window in place too
    gs.check()
    with pytest.raises(MapxError, match="pitch"):
        check(lib.mapx_inner_product_bwd_bf16(gg.data_ptr(), P - 1, ptr(xg), B, T, E, ptr(dx), stream()))
