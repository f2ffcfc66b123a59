"""Magnitude records (csrc/amax.h) on planted maxima: every kernel that leaves a record is run on inputs whose output has
one element far above all others (tests/amax_planted.py; tests/test_amax_planted_host.py proves on the CPU that the
plant is where it is said to be), at the positions where a kernel can lose an element — tile corners and edges, every
lane of the last float4, the second trip of a grid-stride loop, the seam between two writers, two parameters or two
column ranges.  Every case asserts: the output's arg-max of |.| is the planted position; the record equals the
output's maximum exactly; the output meets the bound of the producer's existing parity test against float64.
Then the producers under the replays of a captured chain, and the two-piece cut at the top of a binade."""
import math

import numpy as np
import pytest
import torch

import amax_planted as AP

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mapx import native, ops as _ops
    assert (native.EPI_NONE, native.EPI_BIAS, native.EPI_BIAS_RELU, native.EPI_BIAS_CROSS, native.EPI_ADD, native.EPI_RELU_MASK,
            native.EPI_RELU_MASK_COLSUM) == tuple(range(7))
    return _ops


def _d(t):
    return None if t is None else t.to(DEV)


def _where(out):
    """Position of the largest finite |out| (computed on the device)."""
    a = out.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.full_like(a, -1.0))
    return tuple(int(i) for i in np.unravel_index(int(a.flatten().argmax()), tuple(a.shape)))


def _finite_max(out):
    a = out.detach().abs()
    return float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max())


def _check(ops, name, out, rec, pos, ref=None, bound=None):
    """The three assertions of a planted case."""
    assert rec is not None, name
    if pos is not None:
        assert _where(out) == tuple(pos), f"{name}: arg-max {_where(out)}"
    assert ops.amax_value(rec) == _finite_max(out), f"{name}: record {ops.amax_value(rec)!r}, maximum {_finite_max(out)!r}"
    if ref is not None:
        err = (out.detach().cpu().double() - ref).abs()
        assert bool((err <= bound).all()), f"{name}: off by {float((err - bound).max())!r} beyond the bound"


# --------------------------------------------------------------------------- GEMM epilogues
def _run_gemm(ops, c, tile, scaled, planes=False):
    A, B = _d(c.inp["A"]), _d(c.inp["B"])
    kw = {}
    if c.epi in (AP.EPI_BIAS, AP.EPI_BIAS_RELU, AP.EPI_BIAS_CROSS):
        kw["bias"] = _d(c.inp["bias"])
    if c.epi in (AP.EPI_BIAS_CROSS, AP.EPI_ADD, AP.EPI_RELU_MASK, AP.EPI_RELU_MASK_COLSUM):
        kw["aux1"] = _d(c.inp["aux1"])
    if c.epi == AP.EPI_BIAS_CROSS:
        kw["aux2"], kw["out2"] = _d(c.inp["aux2"]), torch.empty(c.M, c.N, device=DEV)
    if c.epi == AP.EPI_RELU_MASK_COLSUM:
        kw["out2"] = torch.empty(ops.part_rows(c.M), c.N, device=DEV)
    if scaled:
        kw["amax_a"], kw["amax_b"] = ops.amax(A), ops.amax(B)
    if planes:
        kw["b_planes"] = ops.h2_weight_planes(B, c.b_kc, kw["amax_b"])
    out = ops.gemm(A, B, True, c.b_kc, c.M, c.N, c.K, epi=c.epi, tile=tile, **kw)
    return out, ops.amax_of(out)


@pytest.mark.parametrize("arith", ["x3", "h2"])
@pytest.mark.parametrize("shape", ["vec_nt", "vec_nn", "scalar_n"])
def test_gemm_epilogue_records_on_planted_maxima(ops, shape, arith):
    """ops.gemm with tile = 0, 1, 2, 3 and every epilogue, without operand records ("x3": gemm_x3.hip's six-product
    kernels) and with amax_a / amax_b from ops.amax ("h2": gemm_h2.hip's two-piece kernels).  What runs
    (gemm_f32x3_launch, gemm_f32h2_try; K = 136 is more than one K-step of 32, so no hint is turned into tile 2):
    * vec_nt / vec_nn, 200 x 136 x 136, operands 16-byte loadable, N % 4 == 0: the hinted tile of the chosen family
      (0: 64 x 64, 1: 128 x 64, 2: 128 x 128 by 8 waves, 3: 128 x 128 by 4 waves) with epilogue_rows_x3_vec; for
      EPI_RELU_MASK_COLSUM the hint 0 becomes tile 1 (one partial row per 128-row tile), so its tile-0 pass is a second
      tile-1 run.  Edge tiles at 64 and at 128 in both directions.
    * scalar_n, 131 x 70 x 136: N % 4 != 0 sends every tile to the element-wise branch of epilogue_rows_x3
      (EPI_RELU_MASK_COLSUM is refused by the launcher for such N and is left out); operands stay vector loads (K % 8
      == 0), so "h2" still takes gemm_h2.hip."""
    scaled = arith == "h2"
    before = list(ops.H2_USED)
    n = 0
    for c in AP.gemm_cases(shape):
        for tile in (0, 1, 2, 3):
            out, rec = _run_gemm(ops, c, tile, scaled)
            _check(ops, f"{c.name} tile {tile} {arith}", out, rec, c.pos, c.ref, c.bound)
            n += 1
    assert ops.H2_USED[0 if scaled else 1] - before[0 if scaled else 1] == n     # every product got the records asked for


@pytest.mark.parametrize("shape", ["planes_nt", "planes_nn"])
def test_planes_kernel_records_on_planted_maxima(ops, shape):
    """gemm_h2w.hip (operand B from ops.h2_weight_planes, tile = -1): 1025 x 900 x 72 with B [N, K] and 1025 x 904 x
    72 with B [K, N] — 9 x 15 = 135 tiles of 128 x 64 (gemm_f32h2w_try: fewer than 128 tiles of 128 x 128, at least
    128 of 128 x 64), the smallest shapes ops.planes_wanted takes with partial edge tiles in both directions.  (B [K, N]
    needs N % 8 == 0 for 16-byte operand loads; with N = 900 gemm_f32x3_launch finds the operands not vector-loadable
    and neither planes nor two-piece kernel runs.)  Every epilogue, epilogue_rows_x3_vec on 128 x 64 tiles."""
    M, N, K, b_kc, _, _ = AP.GEMM_SHAPES[shape]
    assert ops.planes_wanted(M, N, K) and K >= 64 and K % 8 == 0 and (b_kc or N % 8 == 0)
    assert math.ceil(M / 128) * math.ceil(N / 128) < 128 <= math.ceil(M / 128) * math.ceil(N / 64)
    for c in AP.gemm_cases(shape):
        out, rec = _run_gemm(ops, c, -1, True, planes=True)
        _check(ops, c.name + " planes", out, rec, c.pos, c.ref, c.bound)


def test_two_kernels_raising_one_record(ops):
    """The towers' concatenated buffer (ops.tag + ops.alias_cols): cross_layer_fwd writes the left half, linear_fwd
    (ReLU) the right one, both raise the buffer's record — planted once in each writer's columns, with the operands
    bare (six-product kernels, 64 x 64 tiles) and carrying records (two-piece kernels, their own choice: 64 x 64)."""
    for c in AP.concat_cases():
        for scaled in (False, True):
            i = {k: _d(v) for k, v in c.inp.items()}
            if scaled:
                for k in ("x", "w", "xi", "wc"):
                    ops.tag(i[k], ops.amax(i[k]))
            buf = torch.empty(c.M, 2 * c.D, device=DEV)
            ops.tag(buf, ops.amax_record(buf.device))
            ops.cross_layer_fwd(i["x0"], i["xi"], i["wc"], i["bc"], out=ops.alias_cols(buf, 0, c.D))
            ops.linear_fwd(i["x"], i["w"], i["b"], relu=True, out=ops.alias_cols(buf, c.D, c.D))
            _check(ops, f"{c.name} scaled={scaled}", buf, ops.amax_of(buf), c.pos, c.ref, c.bound)


@pytest.mark.parametrize("wide", [False, True], ids=["tile1", "tile3"])
@pytest.mark.parametrize("arith", ["x3", "h2"])
def test_fused_backward_records_on_planted_maxima(ops, arith, wide):
    """ops.gemm_bwd_fused, 200 x 136 x 136, c0 = 0, N and 64: the record of t and the one of dz (C._amax_dz, defined
    over the columns >= c0 only), plants at the corners and on both sides of c0 at rows 127, 128 and M - 1, and one
    case whose largest C lies left of c0 — t's record sees it, dz's does not.  The entry point passes no tile hint:
    gemm_f32x3_launch picks tile 0 for fewer than 160 tiles of 128 x 128 and EPI_BWD_FUSED turns that into tile 1, so
    this is epilogue_bwd_fused on 128 x 64 tiles of gemm_x3.hip ("x3") or, with records on dy and w, of gemm_h2.hip
    ("h2", which keeps the caller's tile for this epilogue).  "tile3": 2500 x 1032 x 64, 20 x 9 = 180 tiles of 128 x
    128 — from 160 on the launcher picks tile 3 (128 x 128 by 4 waves), the form of the training step's products —
    with c0 = 516 inside a tile; plants at two corners, (127, 127), (128, 128) and on both sides of c0."""
    M, N, K = AP.FUSED_WIDE if wide else AP.FUSED_SHAPE
    n_left = 0
    for c in AP.fused_cases(wide):
        dy, w = _d(c.inp["dy"]), _d(c.inp["w"])
        if arith == "h2":
            ops.tag(dy, ops.amax(dy))
            ops.tag(w, ops.amax(w))
        c0 = c.c0
        C, t, dx0, part = ops.gemm_bwd_fused(dy, w, c0, add=_d(c.inp["add"]), mask=_d(c.inp["mask"]) if c0 < N else None,
                                             x0=_d(c.inp["x0"]) if c0 else None, u=_d(c.inp["u"]) if c0 else None)
        err = (C.cpu().double() - c.ref_C).abs()
        assert bool((err <= c.bound).all()), c.name
        if c0 < N:
            _check(ops, c.name + " dz", C[:, c0:], C._amax_dz, c.pos_dz)
        if c0 > 0:
            _check(ops, c.name + " t", t, ops.amax_of(t), c.pos_t)
            # t is formed from the stored v: one fp32 rounding (test_gemm_bwd_fused_epilogue)
            want = C.cpu().double()[:, :c0] * c.inp["x0"].double()
            assert bool(((t.cpu().double() - want).abs() <= 1e-6 * want.abs() + 1e-12).all()), c.name
        if c.left_big:
            assert _where(C)[1] < c0 and ops.amax_value(C._amax_dz) < ops.amax_value(ops.amax_of(t)) * AP.RUNNER_UP
            n_left += 1
    assert n_left == (0 if wide else 1)


@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("op", ["relu", "cross"])
def test_elementwise_colsum_records_on_planted_maxima(ops, op, N):
    """colsum.hip's ew_colsum_kernel through ops.relu_mask_colsum (OP 0) and ops.cross_bwd_pre_colsum (OP 1), M = 300:
    ew_narrow_lanes(N) compares ceil(N / 4 / 32) * 32 with ceil(N / 4 / 64) * 64 — N = 128 (32 float4 columns) takes
    the 32-lane form, N = 256 (64) the 64-lane one.  128 row chunks of 3 rows (100 hold rows); plants in the first and
    last row of chunks 0, 1, 49 and 99, first and last column.  Both outputs are exact in fp32."""
    for c in AP.ew_cases(op, N):
        a, b = _d(c.inp["a"]), _d(c.inp["b"])
        out = ops.relu_mask_colsum(a, b)[0] if op == "relu" else ops.cross_bwd_pre_colsum(a, b, _d(c.inp["c"]))[0]
        _check(ops, c.name, out, ops.amax_of(out), c.pos)
        assert torch.equal(out.cpu(), c.ref.float()), c.name


# --------------------------------------------------------------------------- gather
def _lazy_rows(ops, c, keep):
    """native.LazyRows over the case's stale table state (test_gather_reads_rows_through_their_pending_updates)."""
    from mapx import native as N
    L = AP.LAZY
    sched = ops.make_sched(L["lr0"], L["lambdas"], L["beta1"], L["beta2"])
    assert torch.equal(sched, AP.sched64(L["lr0"], L["lambdas"], L["beta1"], L["beta2"]))
    sched = sched.to(DEV)
    aux = ops.make_replay_aux(L["lr0"], L["lambdas"], L["beta1"], L["beta2"], L["wd"]).to(DEV)
    done = torch.full((1,), L["T_done"], dtype=torch.int32, device=DEV)
    coef = ops.replay_coef_table(aux, L["beta1"], L["beta2"], done)
    m0, v0, last = _d(c.inp["m0"]), _d(c.inp["v0"]), _d(c.inp["last"])
    lz = N.LazyRows()
    lz.m0, lz.v0, lz.ld_mv0, lz.wd0 = m0.data_ptr(), v0.data_ptr(), m0.stride(0), L["wd"]
    lz.m1, lz.v1, lz.ld_mv1, lz.wd1 = None, None, 1, 0.0
    lz.last, lz.sched, lz.sched_len, lz.done = last.data_ptr(), sched.data_ptr(), sched.shape[0], done.data_ptr()
    lz.aux, lz.aux_len, lz.aux_rows = aux.data_ptr(), aux.shape[1], aux.shape[0]
    lz.beta1, lz.beta2, lz.eps, lz.coef_opt = L["beta1"], L["beta2"], L["eps"], coef.data_ptr()
    keep += [sched, aux, done, coef, m0, v0, last]
    return lz


@pytest.mark.parametrize("E,lazy", [(16, False), (12, False), (64, False), (10, False), (16, True), (12, True), (64, True)])
def test_gather_records_on_planted_maxima(ops, E, lazy):
    """gather.hip through ops.emb_gather: emb_gather_kernel<4> (E = 16, 12, 64), emb_gather_kernel<1> (E = 10:
    mapx_emb_gather_fwd takes scalar columns when E % 4 != 0) and emb_gather_lazy_kernel<float> (lazy=, stale rows: the
    record is of the replayed values; fp32 bound of the replay against the float64 oracle as in
    test_catch_up_from_raw_repeating_ids, the plain gather bit for bit).  The launcher caps the grid at 512 blocks of
    256 threads, so n is chosen 300 rows beyond the 131072 / (threads per row) rows of the first grid-stride trip;
    plants in row 0, the rows around the first block boundary, the rows on either side of the trip boundary and the
    last row, first and last column."""
    for c in AP.gather_cases(E, lazy):
        keep = []
        out = ops.emb_gather(_d(c.inp["ids"]), _d(c.inp["table"]), lazy=_lazy_rows(ops, c, keep) if lazy else None)
        _check(ops, c.name, out, ops.amax_of(out), c.pos)
        if lazy:
            np.testing.assert_allclose(out.cpu().double().numpy(), c.ref.numpy(), rtol=1e-5, atol=1e-7, err_msg=c.name)
        else:
            assert torch.equal(out.cpu().double(), c.ref), c.name


# --------------------------------------------------------------------------- NCE head
def test_nce_records_on_planted_maxima(ops):
    """nce.hip, B = 64, L = 6, F = 23, P = 32: the dh record of ops.nce_fwd (written by nce_fwd_p32_kernel<false>, which
    ops.nce_fwd hands a record in the grouped form only: hpos + dh_slots) with explicit idx, and the denc record of
    ops.nce_scatter_dh; plants at the first and last (b, l, p) and on a field that occurs twice in its row of
    masked_index.  Bounds of test_nce_fwd_and_grads_vs_oracle (rtol 1e-4, atol 1e-7)."""
    d = AP.NCE
    for c in AP.nce_fwd_cases():
        mi = _d(c.inp["mi"])
        groups = ops.EncGroups(mi, d["F"])
        h_slots, dh_slots = torch.zeros(groups.cap, d["P"], device=DEV), torch.zeros(groups.cap, d["P"], device=DEV)
        h_slots[groups.hpos.long()] = _d(c.inp["h"])
        o = ops.nce_fwd(h_slots, mi, _d(c.inp["idx"]), _d(c.inp["emb"]), _d(c.inp["bias"]), _d(c.inp["logq"]), d["F"], d["P"],
                        hpos=groups.hpos, dh_slots=dh_slots)
        _check(ops, c.name, o["dh"], ops.amax_of(o["dh"]), c.pos)
        assert torch.equal(dh_slots[groups.hpos.long()], o["dh"])
        np.testing.assert_allclose(o["dh"].cpu().double().numpy(), c.ref.numpy(), rtol=1e-4, atol=1e-7, err_msg=c.name)
    for c in AP.nce_scatter_cases():
        denc = ops.nce_scatter_dh(_d(c.inp["dh"]), _d(c.inp["mi"]), d["F"], d["P"])
        _check(ops, c.name, denc, ops.amax_of(denc), c.pos)
        np.testing.assert_allclose(denc.cpu().double().numpy(), c.ref.numpy(), rtol=1e-4, atol=1e-7, err_msg=c.name)


# --------------------------------------------------------------------------- the narrow head's join
def test_join_records_on_planted_maxima(ops):
    """skinny.hip's skinny_join_bwd_kernel through ops.skinny_join_bwd: both records (t, dzr), M = 130 (a full 128-row
    tile and a partial one), N = 8, D = 64, H = 4; plants in the first and last row of each tile at columns 0, D - 1
    (t) and D, D + H - 1 (dzr).  Bound of test_skinny_join_bwd_vs_fp64."""
    for c in AP.join_cases():
        i = {k: _d(v) for k, v in c.inp.items()}
        g, t, dx0, dzr, pc, pd = ops.skinny_join_bwd(i["dz"], i["w"], i["final"], c.D, i["x0"], i["u"], False)
        _check(ops, c.name + " t", t, ops.amax_of(t), c.pos_t)
        _check(ops, c.name + " dzr", dzr, ops.amax_of(dzr), c.pos_dzr)
        for got, ref in ((t, c.ref_t), (dzr, c.ref_dzr)):
            assert float((got.cpu().double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max())), c.name


# --------------------------------------------------------------------------- dense AdamW
def _adamw(ops, p, g, m, v, sched, done, seg_off, seg_amax, wd):
    a = AP.ADAMW
    ops.adamw_dense(p, g, m, v, sched, done, a["beta1"], a["beta2"], a["eps"], wd, seg_off=seg_off, seg_amax=seg_amax)


@pytest.mark.parametrize("layout", list(AP.ADAMW_LAYOUTS))
def test_adamw_records_on_planted_maxima(ops, layout):
    """optim.hip's adamw_dense_kernel through ops.adamw_dense with explicit seg_off / seg_amax, one update with zero
    gradient and moments.  mapx_adamw_dense launches grid_for(n / 4 + 1, 256) = 3 blocks for n = 3000 and each takes
    per = ceil(750 / 3) = 250 float4 = 1000 elements.  "slots": a parameter over [800, 2400) straddles both block
    seams, plants at the first / last element of the parameters and of the blocks' ranges (LDS slots).  "direct": 20
    parameters of 8 elements and a long one — block 0's range touches 21, those behind the 16 LDS slots (the 17th ..
    20th small one and the long one's head) publish directly.  "tail": n = 3003, the n % 4 elements.  Every
    parameter's record == max |p| of the updated parameter read back; bound of test_adamw_dense_trajectory_vs_oracle."""
    ops.amax_record(torch.device(DEV, torch.cuda.current_device()))              # (the records' epoch word exists)
    for c in AP.adamw_cases(layout):
        p = _d(c.inp["p"]).clone()
        g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        done = torch.zeros(1, dtype=torch.int32, device=DEV)
        seg_off = torch.tensor(c.seg_off, dtype=torch.int64, device=DEV)
        nseg = len(c.seg_off) - 1
        recs = torch.zeros(nseg, ops.REC, dtype=torch.int32, device=DEV)
        _adamw(ops, p, g, m, v, _d(c.sched), done, seg_off, recs, AP.ADAMW["wd"])
        for z in range(nseg):
            seg = p[c.seg_off[z]:c.seg_off[z + 1]]
            _check(ops, f"{c.name} parameter {z}", seg, recs[z], c.pos if z == c.seg else None)
        np.testing.assert_allclose(p.cpu().double().numpy(), c.ref.numpy(), rtol=2e-6, atol=1e-7, err_msg=c.name)


def test_adamw_record_follows_a_shrinking_maximum(ops):
    """Three updates separated by ops.step_advance whose gradient pushes the planted maximum down by lr = 0.1 each
    (Adam's first steps move by lr * sign(g)): the AdamW kernel tags what it writes with epoch + 1, so each update's
    smaller maximum outranks the one before it — the record follows the parameter down, exactly."""
    n, seg_off_l, _ = AP.ADAMW_LAYOUTS["slots"]
    dev = torch.device(DEV, torch.cuda.current_device())
    ops.amax_record(dev)
    g_ = torch.Generator().manual_seed(1)
    p = (1e-3 * torch.randn(n, generator=g_)).to(DEV)
    p[1500] = 1.0
    g = torch.zeros(n, device=DEV)
    g[1500] = 1.0
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sched = ops.make_sched(0.1, [1.0] * 4, AP.ADAMW["beta1"], AP.ADAMW["beta2"]).to(DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    seg_off = torch.tensor(seg_off_l, dtype=torch.int64, device=DEV)
    recs = torch.zeros(len(seg_off_l) - 1, ops.REC, dtype=torch.int32, device=DEV)
    prev = 1.0
    for step in range(3):
        _adamw(ops, p, g, m, v, sched, done, seg_off, recs, 0.0)
        got = ops.amax_value(recs[1])
        assert got == float(p[800:2400].abs().max()) == float(p[1500]), step
        assert prev - 0.11 < got < prev - 0.09, (step, got)
        for z in (0, 2):
            assert ops.amax_value(recs[z]) == float(p[seg_off_l[z]:seg_off_l[z + 1]].abs().max())
        prev = got
        ops.step_advance(done)
    assert int(done) == 3


# --------------------------------------------------------------------------- stand-alone kernel, non-finite elements
def _amax_of_case(ops, c):
    x = _d(c.inp["x"])
    if getattr(c, "form", "") == "pitched":
        x = x[:, :60]
        assert x.stride(0) > x.shape[1] and x.stride(1) == 1
    return x, ops.amax(x)


def test_standalone_amax_on_planted_maxima(ops):
    """amax.hip through ops.amax: the contiguous float4 path, the pitched path (a column slice, ld 64 > 60 columns,
    with larger values outside the slice) and a 1-D tensor of odd length with the plant in its last element."""
    for c in AP.amax_cases():
        x, rec = _amax_of_case(ops, c)
        _check(ops, c.name, x, rec, c.pos)
        assert torch.equal(x.cpu().double(), c.ref)


def test_nonfinite_elements_stay_out_of_the_records(ops):
    """+inf and NaN in the last row (last and first lane of the last float4), a finite plant elsewhere: gather,
    ops.amax and relu_mask_colsum leave the finite maximum."""
    for c in AP.nonfinite_cases():
        if c.kind == "gather":
            out = ops.emb_gather(_d(c.inp["ids"]), _d(c.inp["table"]))
            rec = ops.amax_of(out)
        elif c.kind == "amax":
            out, rec = _amax_of_case(ops, c)
        else:
            out = ops.relu_mask_colsum(_d(c.inp["a"]), _d(c.inp["b"]))[0]
            rec = ops.amax_of(out)
        assert int((~torch.isfinite(out)).sum()) == 2, c.name
        _check(ops, c.name, out, rec, c.pos)
        assert ops.amax_value(rec) == float(c.ref[c.pos].abs())
        assert torch.equal(torch.nan_to_num(out.cpu().double(), nan=-7.0, posinf=-9.0), torch.nan_to_num(c.ref, nan=-7.0, posinf=-9.0))


# --------------------------------------------------------------------------- B. records across replays of a captured chain
class _Chain:
    """emb_gather -> linear_fwd (ReLU) -> cross_layer_fwd -> gemm_bwd_fused -> relu_mask_colsum -> nce_scatter_dh ->
    step_advance on static buffers, one stream.  The weights carry records (ops.amax), so every product takes the
    two-piece kernels and its scales come from the records its producers left."""
    Bn, F, E, V, c0 = 200, 17, 8, 300, 64

    def __init__(self, ops):
        self.ops = ops
        g = torch.Generator().manual_seed(77)
        D = self.F * self.E                                   # 136
        self.D = D
        rn = lambda *s: torch.randn(*s, generator=g)
        self.base = dict(table=rn(self.V, self.E), b1=rn(D), bc=rn(D))
        self.table, self.b1, self.bc = (_d(self.base[k]).clone() for k in ("table", "b1", "bc"))
        self.ids = torch.randint(0, self.V, (self.Bn, self.F), generator=g).to(DEV)
        self.w1, self.wc, self.w2 = (_d(rn(D, D) / math.sqrt(D)) for _ in range(3))
        for w in (self.w1, self.wc, self.w2):
            ops.tag(w, ops.amax(w))
        n = AP.NCE
        self.mi = torch.stack([torch.randperm(n["F"], generator=g)[:n["L"]] for _ in range(n["B"])]).to(DEV)
        self.done = torch.zeros(1, dtype=torch.int32, device=DEV)

    def scale(self, s):
        for k in ("table", "b1", "bc"):
            getattr(self, k).copy_(_d(self.base[k] * s))

    def run(self):
        ops, n = self.ops, AP.NCE
        x = ops.flat_rows(ops.emb_gather(self.ids, self.table))
        y1 = ops.linear_fwd(x, self.w1, self.b1, relu=True)
        y2, u = ops.cross_layer_fwd(x, y1, self.wc, self.bc)
        C, t, dx0, part = ops.gemm_bwd_fused(y2, self.w2, self.c0, mask=y1, x0=x[:, :self.c0], u=u[:, :self.c0])
        dz, db = ops.relu_mask_colsum(C, y1)
        T = n["B"] * n["L"]
        denc = ops.nce_scatter_dh(dz.view(-1)[:T * n["P"]].view(T, n["P"]), self.mi, n["F"], n["P"])
        ops.step_advance(self.done)
        recorded = [("x", x, ops.amax_of(x)), ("y1", y1, ops.amax_of(y1)), ("y2", y2, ops.amax_of(y2)),
                    ("dz of C", C[:, self.c0:], C._amax_dz), ("t", t, ops.amax_of(t)), ("dz", dz, ops.amax_of(dz)),
                    ("denc", denc, ops.amax_of(denc))]
        return recorded, dict(x=x, y1=y1, y2=y2, u=u, C=C, t=t, dx0=dx0, part=part, dz=dz, db=db, denc=denc)


def test_producer_records_across_replays_of_a_captured_chain(ops):
    """The producers themselves under replay (test_a_later_epoch_outranks_an_earlier_one covers the stand-alone kernel
    only): the chain is captured once after three eager passes (trainer._capture announces the capture's record pool),
    then replayed with the inputs rescaled in place to 1, 2^-12, 2^-24 and 2^6 times the base.  After each replay every
    record equals its output's maximum exactly — a record that an earlier, larger replay left must be outranked
    downward through the epoch tag — and every output is bit-identical to the same chain run eagerly on the same
    inputs: the consumers' fp16 scales come from the records, so a stale record shows as a bit difference."""
    from mapx.trainer import _capture
    before = list(ops.H2_USED)
    ch = _Chain(ops)
    for _ in range(3):
        recorded, _ = ch.run()
    assert all(rec is not None for _, _, rec in recorded)
    assert ops.H2_USED[0] - before[0] == 6 and ops.H2_USED[1] == before[1]       # both ops.gemm products were handed two records
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capture(graph):
        recorded, outs = ch.run()
    assert all(rec is not None for _, _, rec in recorded)
    done0 = int(ch.done)
    for k, s in enumerate((1.0, 2.0 ** -12, 2.0 ** -24, 2.0 ** 6)):
        ch.scale(s)
        graph.replay()
        torch.cuda.synchronize()
        assert int(ch.done) == done0 + 2 * k + 1
        maxima = []
        for name, out, rec in recorded:
            assert ops.amax_value(rec) == float(out.abs().max()), f"replay {k} (scale {s}): record of {name}"
            maxima.append(float(out.abs().max()))
        assert min(maxima) > 0.0
        got = {name: o.clone() for name, o in outs.items()}
        e_recorded, e_outs = ch.run()
        for name, out, rec in e_recorded:
            assert ops.amax_value(rec) == float(out.abs().max()), f"eager pass {k}: record of {name}"
        for name in got:
            assert torch.equal(got[name], e_outs[name]), f"replay {k} (scale {s}): {name} differs from the eager chain"


# --------------------------------------------------------------------------- C. the cut at the top of a binade
@pytest.mark.parametrize("e", [0, 14, -14])
def test_cut_at_the_top_of_a_binade(ops, e):
    """Every element of both operands is +-(2 - 2^-23) 2^e: scaled into [2^14, 2^15) the largest value rounds UP to
    32768 in fp16 — the case h2_scale_exp's range is chosen for (amax.h).  The result must be finite and within the
    randn bound of test_gemm_h2_operand_magnitudes, 2e-7 of sum |a||b| (gemm_h2.hip's header), at that test's M, N, K =
    256, 128, 512 through gemm_h2.hip.  gemm_h2w.hip does not take a product of 2 x 2 tiles (gemm_f32h2w_try: at
    least 128), so the planes kernel runs the same operands at the smallest shape it takes, 1025 x 900 with the same K
    (and the planes handed over at 256 x 128 must give gemm_h2.hip's result).  The reference is exact: all |values| are
    equal, so the product is c^2 times an integer matrix."""
    c = (2.0 - 2.0 ** -23) * 2.0 ** e
    K = 512
    g = torch.Generator().manual_seed(100 + e)
    for M, N in ((256, 128), (1025, 900)):
        sa = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0)
        sb = torch.where(torch.rand(N, K, generator=g) < 0.5, -1.0, 1.0)
        A, B = (sa * c).to(DEV), (sb * c).to(DEV)
        assert float(A.abs().max()) == float(A.abs().min()) == float(np.float32(c)) == c
        ra, rb = ops.amax(A), ops.amax(B)
        assert ops.amax_value(ra) == ops.amax_value(rb) == c
        ref = (sa @ sb.t()).double() * (c * c)
        assert ops.planes_wanted(M, N, K) == (M > 256)
        outs = []
        for planes in (False, True):
            pl = ops.h2_weight_planes(B, True, rb) if planes else None
            out = ops.gemm(A, B, True, True, M, N, K, amax_a=ra, amax_b=rb, b_planes=pl).cpu()
            assert bool(torch.isfinite(out).all()), (M, N, planes)
            err = float((out.double() - ref).abs().max()) / (K * c * c)
            assert err <= 2e-7, (M, N, planes, err)
            outs.append(out)
        if M == 256:
            assert torch.equal(outs[0], outs[1])          # not the planes kernel's shape: the same gemm_h2.hip launch
