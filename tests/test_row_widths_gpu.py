"""The row kernels at every lane-group form (tests/row_widths_ref.py: ROW_WIDTHS): the segment reduction against a
float64 index_add_, the lazy table AdamW against the same columns run as 16-wide tables (the form the golden fixtures
pin) and, for the raw-id catch-up, against the reference's dense AdamW.  The per-width cases of the older tests
(test_kernels_gpu.py, test_backbone_kernels_gpu.py) import the same list."""
import numpy as np
import pytest
import torch

import row_widths_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _cpu(x):
    return x.detach().cpu()


# --------------------------------------------------------------------------- segment reduction
def _index_sums(inv, U, x):
    """float64 sums of x and of |x| per key."""
    x = x.double()
    both = torch.zeros(U, 2 * x.shape[1], dtype=torch.float64).index_add_(0, inv, torch.cat([x, x.abs()], 1))
    return both[:, :x.shape[1]], both[:, x.shape[1]:]


@pytest.mark.parametrize("W,n,V", RW.seg_sizes())
def test_seg_reduce_rows_every_width(ops, W, n, V):
    """seg_reduce_rows, single and two-source, fp32 and bf16 rows, against index_add_ in float64 within
    1e-6 * sum|src| + 1e-6 per element (the bound of test_kernels_gpu.py::test_seg_plan_and_reduce_rows).  bf16: the
    reference takes the bf16 values exactly, and for two sources rounds each element sum to bf16 first (segreduce.h:
    load4_sum).  The hot key's run must be long enough for pass B's 16-deep loop at this width's lane group: asserted
    on the plan."""
    keys = RW.skewed_keys(n, V, n + W)
    plan = ops.SegPlan(keys.to(torch.int32).to(DEV), V)
    U = plan.count()
    uniq_ref, inv = torch.unique(keys, return_inverse=True)
    assert U == uniq_ref.numel() and torch.equal(_cpu(plan.uniq[:U]).long(), uniq_ref)
    if n >= 20000:
        r = int((uniq_ref == RW.HOT_KEY).nonzero())
        starts = _cpu(plan.seg_start[:U + 1]).long()
        run_chunks = int(starts[r + 1] - starts[r]) // RW.seg_chunk(n)
        assert run_chunks >= RW.deep_loop_chunks(W), (run_chunks, RW.deep_loop_chunks(W))
    a = torch.randn(n, W, generator=torch.Generator().manual_seed(1))
    b = torch.randn(n, W, generator=torch.Generator().manual_seed(2))
    ad, bd = a.to(DEV), b.to(DEV)
    ah, bh = ad.to(BF16), bd.to(BF16)
    ah_c, bh_c = a.to(BF16).float(), b.to(BF16).float()
    forms = {
        "fp32": ((ad, None), a),
        "fp32x2": ((ad, bd), a.double() + b.double()),
        "bf16": ((ah, None), ah_c),
        "bf16x2": ((ah, bh), (ah_c + bh_c).to(BF16).float()),
    }
    got = {}
    for name, ((s1, s2), terms) in forms.items():
        out = ops.seg_reduce_rows(plan, s1, W, src2=s2)
        assert out.shape == (n, W) and out.dtype == torch.float32
        ref, scale = _index_sums(inv, U, terms)
        err = (_cpu(out[:U]).double() - ref).abs()
        bad = err > 1e-6 * scale + 1e-6
        if bool(bad.any()):
            u, c = [int(i) for i in bad.nonzero()[0]]
            raise AssertionError(f"{name} W={W} n={n}: first wrong element: key {int(uniq_ref[u])} (run {u}, "
                                 f"{int((inv == u).sum())} rows) column {c}: {float(out[u, c])} vs {float(ref[u, c])}; "
                                 f"{int(bad.sum())} wrong, worst {float(err.max()):.3e}")
        assert torch.equal(out[:U], ops.seg_reduce_rows(plan, s1, W, src2=s2)[:U]), name      # same inputs -> same bits
        got[name] = out[:U]
    # two sources summed in the kernel == the reduction of their elementwise sum, bit for bit
    assert torch.equal(got["fp32x2"], ops.seg_reduce_rows(plan, ad + bd, W)[:U])
    assert torch.equal(got["bf16x2"], ops.seg_reduce_rows(plan, ah + bh, W)[:U])


# --------------------------------------------------------------------------- lazy table AdamW
def _sched(ops, T, kind="cosine", warm=0):
    from oracle import ref_model as R
    lambdas = [R.lr_lambda(kind, s, T, warm) for s in range(T)]
    return ops.make_sched(1e-3, lambdas, 0.9, 0.999).to(DEV), lambdas


class _Table:
    """A table with its optimizer state on the device: m and v separate, or the two halves of one record per row
    (row stride 2 W: the layout the product uses); optionally the scalar table p1 with its m1 | v1 record."""

    def __init__(self, p, m, v, last, side_by_side, p1=None, m1=None, v1=None):
        W = p.shape[1]
        self.p = p.to(DEV).clone()
        if side_by_side:
            self.mv = torch.cat([m, v], 1).to(DEV)
            self.m, self.v = self.mv[:, :W], self.mv[:, W:]
        else:
            self.m, self.v = m.to(DEV).clone(), v.to(DEV).clone()
        self.last = last.to(DEV).clone()
        self.kw = {}
        if p1 is not None:
            self.p1 = p1.to(DEV).clone()
            self.mv1 = torch.stack([m1, v1], 1).to(DEV)
            self.kw = dict(p1=self.p1, m1=self.mv1[:, 0], v1=self.mv1[:, 1], wd1=0.0)

    def state(self):
        out = [self.p.clone(), self.m.clone(), self.v.clone(), self.last.clone()]
        if self.kw:
            out += [self.p1.clone(), self.mv1.clone()]
        return out


def _adam_sequence(ops, tab, opt, steps, T_done):
    """Catch-up over a sorted row list, the gradient update (LATE_FROM: the kernel reads last[] itself, some of its rows
    were not caught up), the next step's catch-up from raw repeating ids, the flush.  -> the state after each."""
    sched, aux = opt
    done = torch.full((1,), T_done, dtype=torch.int32, device=DEV)
    args = (0.05, tab.last, sched, done, aux, 0.9, 0.999, 1e-8)
    snaps = []
    ops.table_adam(tab.p, tab.m, tab.v, *args, rows=steps["caught"].to(DEV), **tab.kw)
    snaps.append(tab.state())
    ops.table_adam(tab.p, tab.m, tab.v, *args, rows=steps["updated"].to(DEV), grad0=steps["grad0"].to(DEV),
                   grad1=steps["grad1"].to(DEV) if tab.kw else None, **tab.kw)
    snaps.append(tab.state())
    ops.step_advance(done)
    ops.table_adam(tab.p, tab.m, tab.v, *args, rows=steps["raw"].to(DEV), rows_may_repeat=True, **tab.kw)
    snaps.append(tab.state())
    ops.table_adam(tab.p, tab.m, tab.v, *args, **tab.kw)
    snaps.append(tab.state())
    return snaps


STAGES = ("catch-up over sorted rows", "gradient update", "catch-up from raw ids", "flush")


@pytest.mark.parametrize("with_p1", [False, True], ids=["p0", "p0+p1"])
@pytest.mark.parametrize("side_by_side", [False, True], ids=["m,v", "m|v"])
@pytest.mark.parametrize("W", RW.ROW_WIDTHS)
def test_table_adam_width_equals_16_wide_blocks(ops, W, side_by_side, with_p1):
    """The update is elementwise in the columns and a row's replay coefficients depend only on its last[], so a W-wide
    table must come out, bit for bit, as the same columns run as 16-wide tables (W split into 16-column blocks, the
    last one zero-padded; same last, rows, gradients and step counter): all three forms of table_adam and the flush,
    rows 0 .. 40 updates behind.  W = 16 is the instantiation the golden fixtures pin.  No tolerance.

    This assumes the compiler contracts adam_elem / the replay identically (the same fused multiply-adds) in the
    LG = 4, 8 and 16 instantiations.  If this fails while the comparison with hf_adamw_step
    (test_kernels_gpu.py::test_lazy_table_adam_equals_dense_reference) holds, look for that difference in the three
    instantiations' code before calling it a bug."""
    V, T_done = 700, 57
    opt_s, lambdas = _sched(ops, 200, warm=10)
    opt = (opt_s, ops.make_replay_aux(1e-3, lambdas, 0.9, 0.999, 0.05).to(DEV))
    g = torch.Generator().manual_seed(1000 + W)
    p = 0.3 * torch.randn(V, W, generator=g)
    m, v = 0.01 * torch.randn(V, W, generator=g), 1e-4 * torch.rand(V, W, generator=g)
    p1, m1, v1 = torch.randn(V, generator=g), 0.01 * torch.randn(V, generator=g), 1e-4 * torch.rand(V, generator=g)
    last = (T_done - torch.randint(0, 41, (V,), generator=g)).to(torch.int32)
    last[:20] = T_done
    steps = dict(caught=torch.randperm(V, generator=g)[:150].sort().values.to(torch.int32),
                 updated=torch.randperm(V, generator=g)[:200].sort().values.to(torch.int32))
    steps["grad0"] = 0.1 * torch.randn(200, W, generator=g)
    steps["grad1"] = 0.1 * torch.randn(200, generator=g)
    raw = torch.randint(0, V, (3000,), generator=g)
    raw[:1000] = 3
    steps["raw"] = raw.to(torch.int32)
    scal = (p1, m1, v1) if with_p1 else ()
    wide = _adam_sequence(ops, _Table(p, m, v, last, side_by_side, *scal), opt, steps, T_done)
    assert not torch.equal(wide[0][0], wide[1][0]) and not torch.equal(wide[2][0], wide[3][0])
    assert bool((wide[3][3] == T_done + 1).all())

    def block(x, c0):
        out = torch.zeros(x.shape[0], 16)
        out[:, :min(16, W - c0)] = x[:, c0:c0 + 16]
        return out

    for c0 in range(0, W, 16):
        sub = dict(steps, grad0=block(steps["grad0"], c0))
        narrow = _adam_sequence(ops, _Table(block(p, c0), block(m, c0), block(v, c0), last, side_by_side, *scal), opt, sub,
                                T_done)
        w = min(16, W - c0)
        for stage, a, b in zip(STAGES, wide, narrow):
            for name, x, y in zip(("p", "m", "v"), a, b):
                x, y = x[:, c0:c0 + w], y[:, :w]
                if not torch.equal(x, y):
                    r, c = [int(i) for i in (x != y).nonzero()[0]]
                    raise AssertionError(f"W={W}, {stage}: {name}[{r}, {c0 + c}] = {float(x[r, c])!r} but "
                                         f"{float(y[r, c])!r} as a 16-wide table; {int((x != y).sum())} elements differ")
            assert torch.equal(a[3], b[3]), (stage, "last")
            if with_p1:
                assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]), (stage, "p1 | m1 | v1")


@pytest.mark.parametrize("with_p1", [False, True], ids=["p0", "p0+p1"])
@pytest.mark.parametrize("W", RW.ROW_WIDTHS)
def test_raw_id_catch_up_and_flush_equal_dense_reference(ops, W, with_p1):
    """table_adam(rows_may_repeat) on the raw id list, then the flush, against the reference's dense every-row AdamW:
    the touched rows after the catch-up and every row after the flush, with the tolerances of
    test_kernels_gpu.py::test_catch_up_from_raw_repeating_ids and ::test_lazy_table_adam_equals_dense_reference; m | v
    as one record per row."""
    from oracle import ref_model as R
    T, V = 30, 500
    sched, lambdas = _sched(ops, T + 5)
    aux = ops.make_replay_aux(1e-3, lambdas, 0.9, 0.999, 0.05).to(DEV)
    g = torch.Generator().manual_seed(W)
    p0 = torch.randn(V, W, generator=g)
    m0, v0 = 0.01 * torch.randn(V, W, generator=g), 1e-4 * torch.rand(V, W, generator=g)
    b0, bm0, bv0 = torch.randn(V, generator=g), 0.01 * torch.randn(V, generator=g), 1e-4 * torch.rand(V, generator=g)
    pr, mr, vr, br, bmr, bvr = [t.clone() for t in (p0, m0, v0, b0, bm0, bv0)]
    for s in range(1, T + 1):
        R.hf_adamw_step(pr, torch.zeros(V, W), mr, vr, s, 1e-3 * lambdas[s - 1], wd=0.05)
        R.hf_adamw_step(br, torch.zeros(V), bmr, bvr, s, 1e-3 * lambdas[s - 1], wd=0.0)
    tab = _Table(p0, m0, v0, torch.zeros(V, dtype=torch.int32), True, *((b0, bm0, bv0) if with_p1 else ()))
    done = torch.full((1,), T, dtype=torch.int32, device=DEV)
    ids = torch.randint(0, 200, (50000,), generator=g)
    ids[:20000] = 3
    args = (0.05, tab.last, sched, done, aux, 0.9, 0.999, 1e-8)
    ops.table_adam(tab.p, tab.m, tab.v, *args, rows=ids.to(torch.int32).to(DEV), rows_may_repeat=True, **tab.kw)
    touched = torch.zeros(V, dtype=torch.bool).index_fill_(0, ids.unique(), True)
    lc = _cpu(tab.last)
    assert bool((lc[touched] == T).all()) and bool((lc[~touched] == 0).all())
    np.testing.assert_allclose(_cpu(tab.p)[touched].numpy(), pr[touched].numpy(), rtol=1e-5, atol=1e-7)
    assert torch.equal(_cpu(tab.p)[~touched], p0[~touched]) and torch.equal(_cpu(tab.m)[~touched], m0[~touched])
    if with_p1:
        np.testing.assert_allclose(_cpu(tab.p1)[touched].numpy(), br[touched].numpy(), rtol=1e-5, atol=1e-7)
        assert torch.equal(_cpu(tab.p1)[~touched], b0[~touched])
    before = tab.state()
    ops.table_adam(tab.p, tab.m, tab.v, *args, rows=ids.to(torch.int32).to(DEV), rows_may_repeat=True, **tab.kw)
    assert all(torch.equal(a, b) for a, b in zip(before, tab.state()))           # everything current: no change at all
    ops.table_adam(tab.p, tab.m, tab.v, *args, **tab.kw)                         # flush
    assert bool((_cpu(tab.last) == T).all())
    np.testing.assert_allclose(_cpu(tab.p).numpy(), pr.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(_cpu(tab.m).numpy(), mr.numpy(), rtol=1e-5, atol=2e-8)
    np.testing.assert_allclose(_cpu(tab.v).numpy(), vr.numpy(), rtol=1e-5, atol=1e-10)
    if with_p1:
        np.testing.assert_allclose(_cpu(tab.p1).numpy(), br.numpy(), rtol=1e-5, atol=1e-7)
