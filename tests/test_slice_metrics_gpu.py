"""ops.slice_metrics (csrc/slice_metrics.hip) against tests/slice_metrics_ref.py: the integers exactly, the two fp64 sums
at rtol 1e-12 (the bound of a device fp64 sum against the host in tests/test_score_kernels_gpu.py).  Shapes are the
smallest that reach each piece: one row, one chunk of 256 plus one, group edges on chunk edges, tie runs across chunk
and group edges, a group that spans many chunks between small ones, a mostly empty range of 2^20 groups.  Every case
runs once, into guard-banded outputs, and is shared by the tests.

The reference ranks torch's CPU sigmoid.  It is not sigmoid_f32 bit for bit: on normal random logits the two differ in
the last place on about one logit in twenty (54 of 1000 measured), which would change tie runs and both sums beyond any
fp64 bound.  So a case draws its random logits from candidates on which the two agree (_agreeing: the device side is
the probability a scoring step writes, ops.score_sink, not the code under test), and every case asserts the agreement
on the logits it ends up with; the fixed logits of the tie case agree as they are.  (p32_of evaluates every logit
inside torch's vector loop, whatever the vector's length: the scalar loop for a vector's last elements rounds some
values differently, so a plain torch.sigmoid is not even a function of the value alone.)"""
import numpy as np
import pytest
import torch

from guarded import guarded
from slice_metrics_ref import NAMES, p32_of, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-12
_DONE = {}


def _agreeing(rng, n, scale):
    """n logits ~ N(0, scale^2) whose torch-CPU sigmoid has the bits of the device's."""
    cand = (rng.randn(2 * n + 64) * scale).astype(np.float32)
    same = p32_of(cand).view(np.uint32) == _device_p32(cand).view(np.uint32)
    assert int(same.sum()) >= n, f"only {int(same.sum())} of {len(cand)} candidate logits agree"
    return cand[same][:n]


def _single(rng):
    return _agreeing(rng, 1, 2.0), np.array([1.0], np.float32), np.array([1], np.int32), 3


def _block_plus_one(rng):
    return _agreeing(rng, 257, 2.0), (rng.rand(257) < 0.3).astype(np.float32), np.zeros(257, np.int32), 1


def _few_groups(rng):
    return _agreeing(rng, 1000, 2.0), (rng.rand(1000) < 0.3).astype(np.float32), \
        rng.randint(0, 7, 1000).astype(np.int32), 7


def _every_row_alone(rng):
    return _agreeing(rng, 1000, 2.0), (rng.rand(1000) < 0.5).astype(np.float32), \
        rng.permutation(1000).astype(np.int32), 1000


def _mostly_empty(rng):
    g = rng.randint(0, 1 << 20, 1000).astype(np.int32)
    g[:3] = (0, (1 << 20) - 1, (1 << 20) - 1)                           # both ends of the range, one of them twice
    return _agreeing(rng, 1000, 2.0), (rng.rand(1000) < 0.5).astype(np.float32), g, 1 << 20


def _chunk_edges(rng):
    return _agreeing(rng, 1024, 2.0), (rng.rand(1024) < 0.4).astype(np.float32), \
        rng.permutation(np.repeat(np.arange(4), 256)).astype(np.int32), 4


def _heavy_ties(rng):
    x = np.array([-40.0, -1.0, 0.0, 1.0, 40.0], np.float32)[rng.randint(0, 5, 3000)]
    return x, (rng.rand(3000) < 0.4).astype(np.float32), rng.randint(0, 5, 3000).astype(np.int32), 5


def _hot_group(rng):
    """Group 17 holds 15 000 of 20 000 rows; the 50 others hold 100 each, groups 3 and 40 one class only."""
    small = np.array([k for k in range(51) if k != 17])
    g = rng.permutation(np.concatenate([np.full(15000, 17), np.repeat(small, 100)])).astype(np.int32)
    y = (rng.rand(20000) < 0.2).astype(np.float32)
    y[g == 3], y[g == 40] = 1.0, 0.0
    return _agreeing(rng, 20000, 3.0), y, g, 51


def _long_group(rng):
    """Beyond the issue's table: group 1 holds 34 000 rows, 133 chunks, so a lane of the closing wave adds more than
    one head piece (the 15 000-row group above is 59 chunks, one piece a lane)."""
    g = rng.permutation(np.concatenate([np.full(34000, 1), np.repeat([0, 2], 1000)])).astype(np.int32)
    return _agreeing(rng, 36000, 3.0), (rng.rand(36000) < 0.2).astype(np.float32), g, 3


CASES = {"single row": _single, "one block plus one": _block_plus_one, "a few groups": _few_groups,
         "every row alone": _every_row_alone, "mostly empty": _mostly_empty, "chunk edges": _chunk_edges,
         "heavy ties": _heavy_ties, "hot group": _hot_group, "long group": _long_group}


def _guarded_outputs(G):
    from mapx import ops
    pairs = [guarded(1, G, dt, what=k) for k, dt in ops.SLICE_OUTPUTS]
    return tuple(v[0] for v, _ in pairs), [chk for _, chk in pairs]


def _device_p32(logits):
    """The probabilities a scoring step writes for these logits: the device's sigmoid_f32."""
    from mapx import ops
    x = torch.from_numpy(logits).to(DEV)
    probs, lout = torch.empty_like(x), torch.empty_like(x)
    ops.score_sink(x, x.numel(), torch.zeros(1, dtype=torch.int64, device=DEV), probs, lout)
    return probs.cpu().numpy()


def _case(name):
    """Once per case: inputs, the device's five arrays (host copies) from guard-banded outputs, the reference."""
    if name in _DONE:
        return _DONE[name]
    from mapx import ops
    rng = np.random.RandomState(sorted(CASES).index(name) + 7)
    x, y, g, G = CASES[name](rng)
    p32 = p32_of(x)
    dev_p32 = _device_p32(x)
    differ = int((p32.view(np.uint32) != dev_p32.view(np.uint32)).sum())
    print(f"{name}: n {len(x)} G {G}; torch-CPU sigmoid differs from the device's on {differ} logits")
    assert differ == 0, f"{name}: the reference's p32 is not the device's on {differ} of {len(x)} logits"
    dev_in = tuple(torch.from_numpy(a).to(DEV) for a in (x, y, g))
    out, checks = _guarded_outputs(G)
    for o in out:
        o.fill_(77)                                                     # the call itself zeroes empty groups
    got = ops.slice_metrics(*dev_in, G, out=out)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    for chk in checks:
        chk()
    host = {k: t.cpu().numpy() for k, t in zip(NAMES, got)}
    host["u2"] = host["u2"].view(np.uint64)
    _DONE[name] = dict(x=x, y=y, g=g, G=G, dev_in=dev_in, got=host, want=reference(x, y, g, G, p32=p32))
    return _DONE[name]


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name):
    c = _case(name)
    got, want = c["got"], c["want"]
    for k in ("rows", "positives", "u2"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
    for k in ("sum_prob", "sum_loss"):
        nz = want[k] != 0
        rel = float(np.max(np.abs(got[k][nz] - want[k][nz]) / np.abs(want[k][nz]))) if nz.any() else 0.0
        print(f"{name}: {k} max relative difference {rel:.3e}")
        np.testing.assert_allclose(got[k], want[k], rtol=RTOL, atol=0, err_msg=f"{name}: {k}")
    assert int(got["rows"].sum()) == len(c["x"]) and int(got["positives"].sum()) == int((c["y"] > 0.5).sum())
    empty = got["rows"] == 0
    assert all(not got[k][empty].any() for k in NAMES), name            # exact zeros, +0.0 for the sums


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_call_and_another_row_order_give_the_same_bits(name):
    from mapx import ops
    c = _case(name)
    again = ops.slice_metrics(*c["dev_in"], c["G"])
    perm = torch.from_numpy(np.random.RandomState(3).permutation(len(c["x"]))).to(DEV)
    moved = ops.slice_metrics(*(t[perm] for t in c["dev_in"]), c["G"])
    for k, a, b in zip(NAMES, again, moved):
        first = _bits(c["got"][k]).view(np.int64)
        assert np.array_equal(_bits(a.cpu().numpy()).view(np.int64), first), (name, k, "second call")
        assert np.array_equal(_bits(b.cpu().numpy()).view(np.int64), first), (name, k, "rows permuted")


def test_one_group_is_eval_metrics():
    from mapx import ops
    c = _case("one block plus one")
    m = ops.eval_metrics(c["dev_in"][0], c["dev_in"][1])
    rows, pos, u2 = (int(c["got"][k][0]) for k in ("rows", "positives", "u2"))
    assert rows == 257 and pos == m["positives"] and rows - pos == m["negatives"]
    assert (float(u2) * 0.5) / (float(pos) * float(rows - pos)) == m["auc"]
    np.testing.assert_allclose(c["got"]["sum_loss"][0] / 257, m["logloss"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(c["got"]["sum_prob"][0] / 257, m["avg_probs"], rtol=RTOL, atol=0)


def test_what_the_cases_are_meant_to_reach():
    alone, ties, hot, edges = (_case(k) for k in ("every row alone", "heavy ties", "hot group", "chunk edges"))
    assert not alone["got"]["u2"].any() and (alone["got"]["rows"] == 1).all()
    p = p32_of(ties["x"])
    assert p.max() == 1.0 and len(np.unique(p)) == 5                    # (sigmoid(-40) = 4e-18 is a normal fp32 number)
    assert (edges["got"]["rows"] == 256).all()
    rows, pos = hot["got"]["rows"], hot["got"]["positives"]
    assert rows[17] == 15000 and pos[3] == rows[3] == 100 and pos[40] == 0 and hot["got"]["u2"][3] == 0
    from mapx import score
    rep = score.slice_report(**hot["got"], top=3)
    assert rep["groups"] == 51 and rep["gauc_rows"] == 20000 - 200 and rep["top"][0]["group"] == 17
    want = score.slice_report(**hot["want"], top=3)
    assert rep["gauc"] == pytest.approx(want["gauc"], rel=1e-15)


def test_refusals_do_not_touch_memory_they_should_not():
    from mapx import ops
    from mapx.native import MapxError
    x, y = torch.zeros(300, device=DEV), torch.ones(300, device=DEV)
    for bad, G, at in ((5, 5, 299), (-1, 5, 0), (2 ** 31 - 1, 2 ** 20, 150), (-2 ** 31, 1, 150)):
        g = torch.zeros(300, dtype=torch.int32, device=DEV)
        g[at] = bad
        out, checks = _guarded_outputs(G)
        with pytest.raises(ValueError, match=rf"the first is {bad} at row {at}"):
            ops.slice_metrics(x, y, g, G, out=out)
        for chk in checks:
            chk()
    g64 = torch.zeros(300, dtype=torch.int64, device=DEV)
    g64[7], g64[9] = 2 ** 32, 2 ** 40                                   # would be group 0 if narrowed carelessly
    with pytest.raises(ValueError, match=rf"2 group id\(s\) outside \[0, 4\); the first is {2 ** 32} at row 7"):
        ops.slice_metrics(x, y, g64, 4)
    g = torch.zeros(300, dtype=torch.int32, device=DEV)
    with pytest.raises(MapxError):
        ops.slice_metrics(x.cpu(), y.cpu(), g.cpu(), 4)
    with pytest.raises(MapxError):
        ops.slice_metrics(x, y, g.cpu(), 4)
    with pytest.raises(ValueError, match="300 logits, 299 labels"):
        ops.slice_metrics(x, y[:299], g, 4)
    with pytest.raises(ValueError, match="299 group ids"):
        ops.slice_metrics(x, y, g[:299], 4)
    for G in (0, 2 ** 31):
        with pytest.raises(ValueError, match="n_groups"):
            ops.slice_metrics(x, y, g, G)
    with pytest.raises(TypeError):
        ops.slice_metrics(x, y, g.float(), 4)
    with pytest.raises(TypeError):
        ops.slice_metrics(x, y, g, 4, out=tuple(torch.zeros(3, dtype=dt, device=DEV) for _, dt in ops.SLICE_OUTPUTS))
    rows = ops.slice_metrics(x, y, g, 4)[0]                             # and the next call is sound
    assert rows.tolist() == [300, 0, 0, 0]
