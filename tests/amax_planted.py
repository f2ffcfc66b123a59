"""Planted-maximum cases for the magnitude records (csrc/amax.h) of every kernel that leaves one.

A record is a maximum, and a maximum over randn data notices a dropped element with probability ~ 1/n.  Every builder
here therefore makes inputs whose output has ONE element far above all others — the plant, at a position chosen for the
producer's structure (tile corners, the last float4 of a row, the second trip of a grid-stride loop, ...) — and returns
the output restated in float64 torch.  tests/test_amax_planted_host.py checks on the CPU that the float64 output's
largest finite |value| sits at the planted position with the runner-up at most 2^-8 of it; tests/test_amax_planted_gpu.py
runs the producer and asserts arg-max, record == maximum (exactly), and the producer's existing parity bound.

Plain module (no fixtures); reads nothing outside the repository."""
import math
from types import SimpleNamespace as Case

import numpy as np
import torch

PLANT = 2.0 ** 12
RUNNER_UP = 2.0 ** -8
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_CROSS, EPI_ADD, EPI_RELU_MASK, EPI_RELU_MASK_COLSUM = range(7)   # mapx.native's
EPI_NAMES = ("none", "bias", "bias_relu", "bias_cross", "add", "relu_mask", "relu_mask_colsum")


# --------------------------------------------------------------------------- the condition every case must meet
def plant_report(ref):
    """-> (position of the largest finite |ref|, that value, the runner-up)."""
    a = ref.detach().double().abs().clone()
    a[~torch.isfinite(a)] = -1.0
    flat = a.flatten()
    top = int(flat.argmax())
    peak = float(flat[top])
    flat[top] = -1.0
    second = max(float(flat.max()), 0.0) if flat.numel() > 1 else 0.0
    return tuple(int(i) for i in np.unravel_index(top, tuple(a.shape))), peak, second


def assert_planted(ref, pos, what=""):
    where, peak, second = plant_report(ref)
    assert where == tuple(pos), f"{what}: largest |value| at {where}, planted at {tuple(pos)}"
    assert peak > 0.0 and second <= RUNNER_UP * peak, f"{what}: runner-up {second!r} against the plant {peak!r}"
    return peak, second


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signs(n, g):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def _uniq(seq):
    out = []
    for p in seq:
        if p not in out:
            out.append(p)
    return out


# --------------------------------------------------------------------------- GEMM epilogues
TILES = ((64, 64), (128, 64), (128, 128))       # tile 0; tile 1; tiles 2 and 3 (gemm_x3.hip: launch_layout_x3)


def gemm_positions(M, N, tiles=TILES):
    """The four corners, (bm-1, bn-1) and (bm, bn) of every tile form, each lane of the last float4, one interior."""
    pos = [(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1)]
    for bm, bn in tiles:
        pos += [(r, c) for r, c in ((bm - 1, bn - 1), (bm, bn)) if r < M and c < N]
    pos += [(M - 1, N - 4 + i) for i in range(4)]
    pos.append((M // 3 + 1, N // 3 + 2))
    return _uniq(pos)


def epilogue64(epi, P, bias, aux1, aux2):
    """The epilogues of gemm_x3_common.h on the float64 product P."""
    if epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_CROSS):
        P = P + bias.double()
    if epi == EPI_BIAS_RELU:
        return P.clamp(min=0)
    if epi == EPI_BIAS_CROSS:
        return aux1.double() + aux2.double() * P
    if epi == EPI_ADD:
        return P + aux1.double()
    if epi in (EPI_RELU_MASK, EPI_RELU_MASK_COLSUM):
        return P * (aux1 > 0)
    return P


class GemmBase:
    """C = epi(A B^T) with A [M, K], B kept as [N, K] (handed over as it is, b_kc, or transposed [K, N]).  The float64
    product and sum |a||b| of the base are formed once; a plant changes one row of A and one of B, so one row and one
    column of both."""

    def __init__(self, M, N, K, b_kc, seed=0):
        g = _gen(seed)
        self.M, self.N, self.K, self.b_kc = M, N, K, b_kc
        self.A = torch.randn(M, K, generator=g)
        self.B = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.bias, self.aux1, self.aux2 = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
        self.sign = _signs(K, g)
        self.P = self.A.double() @ self.B.double().t()
        self.S = self.A.abs().double() @ self.B.abs().double().t()

    def case(self, epi, pos):
        m, n = pos
        A, B, aux1, aux2 = self.A.clone(), self.B.clone(), self.aux1.clone(), self.aux2.clone()
        if epi == EPI_BIAS_CROSS:
            # planted through x0 (aux2); row m and column n sign-aligned so that u[m, n] = sum |a||b| cannot cancel
            A[m], B[n] = self.sign * A[m].abs(), self.sign * B[n].abs()
            aux2[m, n] = 4.0 * PLANT
        else:
            A[m], B[n] = self.sign * A[m].abs() * PLANT, self.sign * B[n].abs() * PLANT
        if epi in (EPI_RELU_MASK, EPI_RELU_MASK_COLSUM):
            aux1[m, n] = 1.0
        P, S = self.P.clone(), self.S.clone()
        P[m], S[m] = A[m].double() @ B.double().t(), A[m].abs().double() @ B.abs().double().t()
        P[:, n], S[:, n] = A.double() @ B[n].double(), A.abs().double() @ B[n].abs().double()
        ref = epilogue64(epi, P, self.bias, aux1, aux2)
        if epi == EPI_BIAS_CROSS:        # test_cross_network_fwd_bwd_vs_oracle: rtol 1e-5, atol 1e-5
            bound = 1e-5 + 1e-5 * ref.abs()
        else:                            # test_gemm_linear_forward / test_gemm_backward_products / ..._relu_mask_colsum_epilogue
            bound = 2e-6 * S + 1e-6
        inp = dict(A=A, B=B if self.b_kc else B.t().contiguous(), bias=self.bias, aux1=aux1, aux2=aux2)
        return Case(name=f"gemm {self.M}x{self.N}x{self.K} {EPI_NAMES[epi]} @{pos}", inp=inp, pos=pos, ref=ref,
                    bound=bound, epi=epi, M=self.M, N=self.N, K=self.K, b_kc=self.b_kc)


# (M, N, K, b_kc, epilogues, tile forms whose corners are planted)
_FWD = (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_CROSS)
_BWD = (EPI_ADD, EPI_RELU_MASK, EPI_RELU_MASK_COLSUM)
GEMM_SHAPES = {
    # partial edge tiles at 64 and at 128 in both directions, vector I/O; forward epilogues as A W^T, backward as dY W
    "vec_nt": (200, 136, 136, True, _FWD, TILES),
    "vec_nn": (200, 136, 136, False, _BWD, TILES),
    # N % 4 != 0: the element-wise branch of epilogue_rows_x3 (EPI_RELU_MASK_COLSUM is refused there by the launcher)
    "scalar_n": (131, 70, 136, True, _FWD + (EPI_ADD, EPI_RELU_MASK), TILES),
    # the smallest shapes ops.planes_wanted takes with partial edge tiles (9 x 15 tiles of 128 x 64); operand B [K, N]
    # must keep N % 8 == 0 for 16-byte loads, or the launcher leaves the planes kernel: 904 instead of 900
    "planes_nt": (1025, 900, 72, True, _FWD + _BWD, ((128, 64),)),
    "planes_nn": (1025, 904, 72, False, _FWD + _BWD, ((128, 64),)),
}


def gemm_cases(shape):
    M, N, K, b_kc, epis, tiles = GEMM_SHAPES[shape]
    base = GemmBase(M, N, K, b_kc, seed=M + N)
    for epi in epis:
        for pos in gemm_positions(M, N, tiles):
            yield base.case(epi, pos)


# --------------------------------------------------------------------------- two kernels raising one record
def concat_cases():
    """The towers' concatenated buffer [M, 2 D]: cross_layer_fwd writes columns [0, D), linear_fwd (ReLU) [D, 2 D)."""
    M, D, K = 200, 136, 136
    g = _gen(5)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(D, K, generator=g) / math.sqrt(K), torch.randn(D, generator=g)
    x0, xi = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    wc, bc = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g)
    sk, sd = _signs(K, g), _signs(D, g)
    for side, (m, n) in [("left", p) for p in ((0, 0), (M - 1, D - 1), (128, 64))] + \
                        [("right", p) for p in ((0, 0), (M - 1, D - 1), (127, 63))]:
        x_, w_, x0_, xi_, wc_ = x.clone(), w.clone(), x0.clone(), xi.clone(), wc.clone()
        if side == "left":
            xi_[m], wc_[n] = sd * xi_[m].abs(), sd * wc_[n].abs()
            x0_[m, n] = 4.0 * PLANT
        else:
            x_[m], w_[n] = sk * x_[m].abs() * PLANT, sk * w_[n].abs() * PLANT
        left = xi_.double() + x0_.double() * (xi_.double() @ wc_.double().t() + bc.double())
        right = (x_.double() @ w_.double().t() + b.double()).clamp(min=0)
        ref = torch.cat([left, right], 1)
        bound = torch.cat([1e-5 + 1e-5 * left.abs(), 2e-6 * (x_.abs().double() @ w_.abs().double().t()) + 1e-6], 1)
        yield Case(name=f"concat {side} @{(m, n)}", inp=dict(x=x_, w=w_, b=b, x0=x0_, xi=xi_, wc=wc_, bc=bc),
                   pos=(m, n if side == "left" else D + n), ref=ref, bound=bound, M=M, D=D)


# --------------------------------------------------------------------------- fused backward epilogue
FUSED_SHAPE = (200, 136, 136)
# 20 x 9 = 180 tiles of 128 x 128: from 160 on gemm_f32x3_launch picks tile 3 (128 x 128 by 4 waves) by itself, the only
# way to that form of the fused epilogue (the entry point takes no tile hint).  Partial edge tiles both ways, c0 inside
# a tile, K of two K-steps.
FUSED_WIDE = (2500, 1032, 64)


def fused_cases(wide=False):
    """ops.gemm_bwd_fused: v = dy w;  columns >= c0: dz = mask > 0 ? v : 0;  columns < c0: t = v x0.  A plant at
    (m, n) is dz's when n >= c0 and t's otherwise.  The last case of each 0 < c0 < N also puts the largest value of C
    left of c0 (through `add`): t's record must see it, dz's must not."""
    M, N, K = FUSED_WIDE if wide else FUSED_SHAPE
    g = _gen(9 + wide)
    dy, w = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / math.sqrt(K)
    mask, x0, u = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    sk = _signs(K, g)
    P0, S0 = dy.double() @ w.double(), dy.abs().double() @ w.abs().double()
    for c0 in ((516,) if wide else (0, N, 64)):
        pos = [(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1)]
        for c in (c0 - 1, c0):
            if 0 <= c < N:
                pos += [(127, c), (128, c), (M - 1, c)]
        if wide:
            pos = [(0, 0), (M - 1, N - 1), (127, 127), (128, 128), (127, c0 - 1), (128, c0), (M - 1, c0 - 1), (M - 1, c0)]
        todo = [(p, False) for p in _uniq(pos)]
        if 0 < c0 < N and not wide:
            todo.append(((M - 1, c0), True))
        for (m, n), left_big in todo:
            dy_, w_, mask_, x0_ = dy.clone(), w.clone(), mask.clone(), x0.clone()
            dy_[m], w_[:, n] = sk * dy_[m].abs() * PLANT, sk * w_[:, n].abs() * PLANT
            add = None
            if n >= c0:
                mask_[m, n] = 1.0
            else:
                x0_[m, n] = 2.0
            P, S = P0.clone(), S0.clone()
            P[m], S[m] = dy_[m].double() @ w_.double(), dy_[m].abs().double() @ w_.abs().double()
            P[:, n], S[:, n] = dy_.double() @ w_[:, n].double(), dy_.abs().double() @ w_[:, n].abs().double()
            pos_t = (m, n) if n < c0 else None
            if left_big:
                add = torch.zeros(M, N)
                add[0, c0 - 1] = 2.0 ** 40
                x0_[0, c0 - 1] = 1.5
                P, S = P + add.double(), S + add.double()
                pos_t = (0, c0 - 1)
            C = P.clone()
            C[:, c0:] = P[:, c0:] * (mask_[:, c0:] > 0)
            yield Case(name=f"fused c0={c0} @{(m, n)}" + (" +left" if left_big else ""),
                       inp=dict(dy=dy_, w=w_, mask=mask_, x0=x0_[:, :c0].contiguous(), u=u[:, :c0].contiguous(), add=add),
                       c0=c0, ref_C=C, bound=2e-6 * S + 1e-6,        # test_gemm_bwd_fused_epilogue
                       ref_t=P[:, :c0] * x0_[:, :c0].double() if c0 else None, pos_t=pos_t,
                       ref_dz=C[:, c0:] if c0 < N else None, pos_dz=(m, n - c0) if n >= c0 else None, left_big=left_big)


# --------------------------------------------------------------------------- elementwise + column sum
EW_M = 300
EW_CHUNKS = 128                          # colsum.hip: kColChunks


def ew_positions(M, N):
    """First and last row of the row chunks 0, 1, one in the middle and the last one that holds rows (chunks are
    ceil(M / 128) rows; the chunks behind M publish zeros), first and last column."""
    per = -(-M // EW_CHUNKS)
    last = (M - 1) // per
    rows = []
    for ch in (0, 1, last // 2, last):
        rows += [ch * per, min(ch * per + per, M) - 1]
    return [(r, c) for r in _uniq(rows) for c in (0, N - 1)]


def ew_cases(op, N):
    """op "relu": ops.relu_mask_colsum(dy, y) -> dz = y > 0 ? dy : 0;  op "cross": ops.cross_bwd_pre_colsum(g, x0, u)
    -> t = g x0.  Both results are exact in fp32: the reference is compared bit for bit (test_fused_elementwise_colsum)."""
    M = EW_M
    g = _gen(N)
    a, b, c = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    for m, n in ew_positions(M, N):
        a_, b_ = a.clone(), b.clone()
        if op == "relu":
            a_[m, n], b_[m, n] = PLANT, 1.0
            ref = a_.double() * (b_ > 0)
        else:
            a_[m, n], b_[m, n] = -256.0, 256.0
            ref = a_.double() * b_.double()
        yield Case(name=f"ew {op} N={N} @{(m, n)}", inp=dict(a=a_, b=b_, c=c), pos=(m, n), ref=ref, op=op)


# --------------------------------------------------------------------------- gather
GATHER_TRIP = 512 * 256                  # gather.hip: the grid is capped at 512 blocks of 256 threads
GATHER_V = 500


def gather_geometry(E):
    per_row = E // 4 if E % 4 == 0 else E                 # threads per row: float4 lanes, or scalar columns
    second = -(-GATHER_TRIP // per_row)                   # first row that lies wholly in the second grid-stride trip
    n = second + 300
    b = 256 // per_row                                    # (E = 12, 10: row b straddles the first two blocks)
    return per_row, n, _uniq([0, b - 1, b, b + 1, second - 1, second, n - 1])


def sched64(lr0, lambdas, beta1=0.9, beta2=0.999):
    """ops.make_sched: {step size, lr} of update s = 1 .. T, rounded to fp32 as the kernels read them."""
    rows = [(lr0 * lam * math.sqrt(1.0 - beta2 ** (i + 1)) / (1.0 - beta1 ** (i + 1)), lr0 * lam) for i, lam in enumerate(lambdas)]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


LAZY = dict(lr0=1e-3, wd=0.05, beta1=0.9, beta2=0.999, eps=1e-8, T=120, T_done=41)
LAZY["lambdas"] = [min(1.0, s / 10.0) * 0.5 * (1.0 + math.cos(math.pi * s / LAZY["T"])) for s in range(LAZY["T"])]


def replay64(p, m, v, last, to, sched, wd, beta1, beta2, eps):
    """The zero-gradient AdamW updates last[r] + 1 .. `to` of every row r, in float64 (oracle: hf_adamw_step with g = 0;
    update s + 1 reads sched[s])."""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    sc = sched.double()
    for s in range(int(last.min()), to):
        act = ((last >= 0) & (last <= s)).view(-1, 1).double()
        m = m * (1 + act * (beta1 - 1))
        v = v * (1 + act * (beta2 - 1))
        p = p - act * float(sc[s, 0]) * m / (v.sqrt() + eps)
        p = p - act * float(sc[s, 1]) * wd * p
    return p


def gather_cases(E, lazy=False):
    """out = table[ids]: the plant sits in the table row of an id that occurs once, at the planted row.  lazy: the
    rows are stale (last[id] < T_done) and are read through their pending zero-gradient updates; the reference is the
    replayed table."""
    per_row, n, rows = gather_geometry(E)
    V = GATHER_V
    g = _gen(E + (1000 if lazy else 0))
    table = torch.randn(V, E, generator=g) * 3
    ids = torch.randint(0, V - 1, (n,), generator=g)
    extra = {}
    if lazy:
        L = LAZY
        m0, v0 = 0.01 * torch.randn(V, E, generator=g), 1e-4 * torch.rand(V, E, generator=g)
        last = (L["T_done"] - torch.randint(0, 30, (V,), generator=g)).clamp(min=0).to(torch.int32)
        last[:64] = L["T_done"]
        last[V - 1] = L["T_done"] - 17
        sched = sched64(L["lr0"], L["lambdas"], L["beta1"], L["beta2"])
        rp = lambda t: replay64(t, m0, v0, last, L["T_done"], sched, L["wd"], L["beta1"], L["beta2"], L["eps"])
        shown = rp(table)
        extra = dict(m0=m0, v0=v0, last=last)
    for r in rows:
        for c in (0, E - 1):
            t_, ids_ = table.clone(), ids.clone()
            ids_[r] = V - 1
            t_[V - 1, c] = -4.0 * PLANT
            if lazy:
                ref_table = shown.clone()
                ref_table[V - 1] = rp(t_)[V - 1]
            else:
                ref_table = t_.double()
            yield Case(name=f"gather E={E}{' lazy' if lazy else ''} @{(r, c)}", inp=dict(table=t_, ids=ids_, **extra),
                       pos=(r, c), ref=ref_table[ids_], E=E, lazy=lazy)


# --------------------------------------------------------------------------- NCE head
NCE = dict(B=64, L=6, F=23, P=32, K=25, V=3000)


def _nce_index():
    d = NCE
    g = _gen(17)
    mi = torch.stack([torch.randperm(d["F"], generator=g)[:d["L"]] for _ in range(d["B"])])
    mi[3, 1] = mi[3, 0]                                   # a field that occurs twice in its row
    T = d["B"] * d["L"]
    return g, mi, T, [(0, 0), (T - 1, d["P"] - 1), (3 * d["L"] + 1, 5)]


def nce_dh64(h, idx, emb, bias, logq, K, V, T):
    """dh of csrc/nce.hip for the targets given (of T in all): dlogit_j = (sigmoid(lt_j) - [j == 0]) / T,
    dh = sum_j dlogit_j emb[idx_j]."""
    lnV, lnK = float(np.float32(math.log(V))), float(np.float32(math.log(K)))
    rows = emb.double()[idx.long()]                                           # [T, K1, P]
    s = (rows * h.double()[:, None, :]).sum(-1) + bias.double()[idx.long()] - lnV
    lt = s - logq.double()[idx.long()] - lnK
    d = torch.sigmoid(lt)
    d[:, 0] -= 1.0
    return ((d / T)[:, :, None] * rows).sum(1)


def nce_fwd_cases():
    """The dh record of ops.nce_fwd (grouped form: the p32 kernel writes it).  Only the planted target's first table
    row is large: its score is far below zero, so dlogit_0 = -1 / T and dh[t, p] = 2^14 / T."""
    d = NCE
    g, mi, T, plants = _nce_index()
    V, P, K = d["V"], d["P"], d["K"]
    h = torch.randn(T, P, generator=g)
    emb = (torch.rand(V, P, generator=g) * 2 - 1) / math.sqrt(P)
    logq = torch.log_softmax(torch.randn(V, generator=g), 0)
    bias = logq + math.log(V) + 0.1 * torch.randn(V, generator=g)
    idx = torch.randint(0, V - 1, (T, K + 1), generator=g).to(torch.int32)
    base = nce_dh64(h, idx, emb, bias, logq, K, V, T)
    for t, p in plants:
        h_, emb_, idx_ = h.clone(), emb.clone(), idx.clone()
        h_[t, p], idx_[t, 0] = 1.0, V - 1
        emb_[V - 1] = 0.01 * emb_[V - 1]
        emb_[V - 1, p] = -4.0 * PLANT
        ref = base.clone()
        ref[t] = nce_dh64(h_[t:t + 1], idx_[t:t + 1], emb_, bias, logq, K, V, T)[0]
        yield Case(name=f"nce_fwd dh @{(t, p)}", inp=dict(h=h_, mi=mi, idx=idx_, emb=emb_, bias=bias, logq=logq),
                   pos=(t, p), ref=ref)


def nce_scatter_cases():
    """denc[b, f P + p] = sum over the l with masked_index[b, l] == f of dh[b, l, p]  (ops.nce_scatter_dh)."""
    d = NCE
    g, mi, T, plants = _nce_index()
    B, L, F, P = d["B"], d["L"], d["F"], d["P"]
    dh = torch.randn(T, P, generator=g) * 1e-5
    for t, p in plants:
        dh_ = dh.clone()
        dh_[t, p] = -1.0
        ref = torch.zeros(B, F * P, dtype=torch.float64)
        col = (mi.view(-1, 1) * P + torch.arange(P)).view(B, L * P)
        ref.scatter_add_(1, col, dh_.double().view(B, L * P))
        b, l = divmod(t, L)
        yield Case(name=f"nce_scatter @{(t, p)}", inp=dict(dh=dh_, mi=mi), pos=(b, int(mi[b, l]) * P + p), ref=ref)


# --------------------------------------------------------------------------- the narrow head's join
JOIN = dict(M=130, N=8, D=64, H=4)       # D, H (and N) of test_skinny_join_bwd_vs_fp64's (129, 8, 64, 4) case


def join_cases():
    """ops.skinny_join_bwd: v = dz w;  c < D: t = v x0;  c >= D: dzr = final > 0 ? v : 0."""
    M, N, D, H = JOIN["M"], JOIN["N"], JOIN["D"], JOIN["H"]
    g = _gen(23)
    dz, w = torch.randn(M, N, generator=g), torch.randn(N, D + H, generator=g)
    final, x0, u = torch.randn(M, D + H, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    sn = _signs(N, g)
    for m in (0, 127, 128, M - 1):
        for c in (0, D - 1, D, D + H - 1):
            dz_, w_, final_, x0_ = dz.clone(), w.clone(), final.clone(), x0.clone()
            dz_[m], w_[:, c] = sn * dz_[m].abs() * PLANT, sn * w_[:, c].abs() * PLANT
            if c < D:
                x0_[m, c] = 2.0
            else:
                final_[m, c] = 1.0
            v = dz_.double() @ w_.double()
            ref_t = v[:, :D] * x0_.double()
            ref_z = v[:, D:] * (final_[:, D:] > 0)
            yield Case(name=f"join @{(m, c)}", inp=dict(dz=dz_, w=w_, final=final_, x0=x0_, u=u), D=D,
                       ref_t=ref_t, ref_dzr=ref_z, pos_t=(m, c) if c < D else None, pos_dzr=(m, c - D) if c >= D else None)


# --------------------------------------------------------------------------- dense AdamW
ADAMW = dict(lr0=1e-2, wd=0.1, beta1=0.9, beta2=0.999, eps=1e-8)
# optim.hip: grid = ceil((n / 4 + 1) / 256) blocks, each one contiguous range of per = ceil(n / 4 / grid) float4.  With
# n = 3000 (and 3003): 3 blocks of 250 float4 = 1000 elements.
ADAMW_LAYOUTS = {
    # LDS slots: parameter 1 straddles block 0 / 1 and block 1 / 2
    "slots": (3000, [0, 800, 2400, 3000], [0, 799, 800, 999, 1000, 2399, 2400, 2999]),
    # direct publication: block 0's range touches 21 parameters, the 17th and later ones leave the 16 LDS slots
    "direct": (3000, [8 * i for i in range(21)] + [3000], [0, 120, 127, 128, 135, 152, 159, 160, 999, 1000, 2999]),
    # the n % 4 tail, by block 0's threads into the last parameter's record
    "tail": (3003, [0, 800, 2400, 3003], [2999, 3000, 3001, 3002]),
}


def adamw_cases(layout):
    """One update with zero gradient and zero moments: p <- p - lr wd p, so the plant stays the parameter's largest."""
    n, seg_off, plants = ADAMW_LAYOUTS[layout]
    g = _gen(n + len(seg_off))
    p0 = torch.randn(n, generator=g)
    sched = sched64(ADAMW["lr0"], [1.0] * 4, ADAMW["beta1"], ADAMW["beta2"])
    decay = float(np.float32(float(sched[0, 1])) * np.float32(ADAMW["wd"]))
    for i in plants:
        p_ = p0.clone()
        p_[i] = -PLANT
        ref = p_.double() * (1.0 - decay)
        seg = max(z for z in range(len(seg_off) - 1) if seg_off[z] <= i)
        yield Case(name=f"adamw {layout} @{i}", inp=dict(p=p_), seg_off=seg_off, seg=seg, pos=(i - seg_off[seg],),
                   ref=ref, ref_seg=ref[seg_off[seg]:seg_off[seg + 1]], sched=sched)


# --------------------------------------------------------------------------- stand-alone ops.amax
def amax_cases():
    g = _gen(31)
    x = torch.randn(37, 64, generator=g)
    for pos in ((0, 0), (36, 63), (36, 60), (17, 5)):                   # contiguous float4 path
        x_ = x.clone()
        x_[pos] = PLANT
        yield Case(name=f"amax vec @{pos}", inp=dict(x=x_), pos=pos, ref=x_.double(), form="vec")
    for pos in ((0, 0), (36, 59), (36, 56), (17, 5)):                   # a column slice: ld 64 > cols 60
        x_ = x.clone()
        x_[pos] = PLANT
        x_[:, 60:] = 2.0 * PLANT                                        # (outside the slice: must not be seen)
        yield Case(name=f"amax pitched @{pos}", inp=dict(x=x_), pos=pos, ref=x_[:, :60].double(), form="pitched")
    v = torch.randn(1001, generator=g)
    for i in (1000, 0):                                                 # 1-D, odd length
        v_ = v.clone()
        v_[i] = -PLANT
        yield Case(name=f"amax 1d @{i}", inp=dict(x=v_), pos=(i,), ref=v_.double(), form="1d")


# --------------------------------------------------------------------------- non-finite elements
def nonfinite_cases():
    """+inf and NaN in the last row — the last lane of the last float4 and its first lane —, a finite plant elsewhere:
    the record is the finite maximum."""
    inf, nan = float("inf"), float("nan")
    g = _gen(41)
    E = 16
    _, n, rows = gather_geometry(E)
    table = torch.randn(GATHER_V, E, generator=g) * 3
    ids = torch.randint(0, GATHER_V - 2, (n,), generator=g)
    ids[n - 1], ids[rows[2]] = GATHER_V - 1, GATHER_V - 2
    table[GATHER_V - 1, E - 1], table[GATHER_V - 1, E - 4] = inf, nan
    table[GATHER_V - 2, 3] = PLANT * 4
    yield Case(name="nonfinite gather", kind="gather", inp=dict(table=table, ids=ids), pos=(rows[2], 3), ref=table.double()[ids])
    x = torch.randn(37, 64, generator=g)
    x[36, 63], x[36, 60], x[17, 5] = inf, nan, PLANT
    yield Case(name="nonfinite amax", kind="amax", inp=dict(x=x), pos=(17, 5), ref=x.double())
    M, N = EW_M, 128
    dy, y = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    dy[M - 1, N - 1], dy[M - 1, N - 4], dy[5, 7] = inf, nan, PLANT
    y[M - 1, N - 1] = y[M - 1, N - 4] = y[5, 7] = 1.0
    ref = torch.where(y > 0, dy.double(), torch.zeros(M, N, dtype=torch.float64))
    yield Case(name="nonfinite relu_mask_colsum", kind="relu", inp=dict(a=dy, b=y), pos=(5, 7), ref=ref)
