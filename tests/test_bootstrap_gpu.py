"""ops.bootstrap_weights and ops.bootstrap_metrics (csrc/bootstrap.hip) against tests/boot_ref.py: the weights byte for
byte, u2 / pos_w / neg_w exactly, sum_loss at rtol 1e-12 (tests/test_slice_metrics_gpu.py's bound of a device fp64 sum
against the host; n * 2^-52 stays below it at these sizes).  The reference ranks the device's own probabilities (the
ones a scoring step writes: that file's _device_p32), so a case needs no agreement between two sigmoids.

Shapes are the smallest that reach each piece: one row, a wave's 64 rows less one / exactly / plus one, several segments
of five steps and three rows (boot_ref.segments restates the n -> S rule), a size at which the segment length is no
longer the minimum, tie runs longer than a step, one tie run across every segment border, one class only, a NaN
logit, clustered units with a 2^40 id; replicate counts 1, 3, 4, 5 (a quad less one / exactly / plus one) and 260 (more
than one block of quads).  Every case runs once, into guard-banded outputs from guard-banded inputs."""
import numpy as np
import pytest
import torch

import boot_ref as B
from guarded import guarded, padded_copy
from test_slice_metrics_gpu import RTOL, _device_p32

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 42
_DONE = {}


def _random(n, R, units=None, ctr=0.3):
    def make(rng):
        return (rng.randn(n) * 2).astype(np.float32), (rng.rand(n) < ctr).astype(np.float32), units, R
    return make


def _segments(rng):
    n = 5 * 64 * 4 + 3
    assert B.segments(n) == 4                                           # n = 5 * 64 * S + 3 for the S the rule gives
    return _random(n, 5)(rng)


def _longer_segments(rng):
    n = 100003
    assert B.segment_rows(n) == 448 and B.segments(n) == 224            # past the minimum length of a segment
    return _random(n, 5)(rng)


def _one_decimal(rng):
    x, y, _, R = _random(3000, 260)(rng)
    return np.round(x, 1), y, None, R


def _all_equal(rng):
    n = 2000
    assert B.segments(n) == 6                                           # one tie run across five borders
    return np.full(n, 0.25, np.float32), (rng.rand(n) < 0.4).astype(np.float32), None, 5


def _all_positive(rng):
    x, _, _, R = _random(500, 3)(rng)
    return x, np.ones(500, np.float32), None, R


def _nan_logit(rng):
    x, y, _, R = _random(300, 4)(rng)
    x[7] = np.nan
    return x, y, None, R


def _clustered(rng):
    units = rng.randint(0, 50, 1000).astype(np.int64)
    units[::97] = 2 ** 40 + 7
    return _random(1000, 5, units)(rng)


CASES = {"one row": _random(1, 1, ctr=2.0), "63 rows": _random(63, 3), "64 rows": _random(64, 4),
         "65 rows": _random(65, 5), "segments": _segments, "longer segments": _longer_segments,
         "one decimal": _one_decimal, "all equal": _all_equal, "all positive": _all_positive, "nan logit": _nan_logit,
         "clustered": _clustered}


def _host(out):
    a = {k: t.cpu().numpy() for k, t in zip(B.NAMES, out)}
    for k in B.NAMES[:3]:
        a[k] = a[k].view(np.uint64)
    return a


def _case(name):
    """Once per case: the inputs, the device's four arrays (host copies) and the reference on the device's own weights'
    restatement (boot_ref.weights) and probabilities."""
    if name in _DONE:
        return _DONE[name]
    from mapx import ops
    rng = np.random.RandomState(sorted(CASES).index(name) + 11)
    x, y, units, R = CASES[name](rng)
    ins = [padded_copy(torch.from_numpy(a).to(DEV)[None, :], what=f"{name}: {k}")
           for k, a in (("logits", x), ("labels", y), ("units", units)) if a is not None]
    dev_in = [v[0] for v, _ in ins] + ([None] if units is None else [])
    before = [t.clone() for t in dev_in if t is not None]
    pairs = [guarded(1, R, dt, what=f"{name}: {k}") for k, dt in ops.BOOT_OUTPUTS]
    out = tuple(v[0] for v, _ in pairs)
    got = ops.bootstrap_metrics(dev_in[0], dev_in[1], R, seed=SEED, units=dev_in[2], out=out)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    for _, chk in pairs + ins:
        chk()                                                            # only [R] of each output, nothing of an input
    assert all(torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else a.dtype),
                           b.view(torch.int32 if b.dtype == torch.float32 else b.dtype))
               for a, b in zip((t for t in dev_in if t is not None), before)), f"{name}: an input changed"
    w = B.weights(len(x) if units is None else units, R, SEED)
    _DONE[name] = dict(x=x, y=y, units=units, R=R, dev_in=dev_in, got=_host(got), w=w,
                       want=B.reference(_device_p32(x), y, w))
    return _DONE[name]


@pytest.mark.parametrize("units", ["rows", "repeats", "a 2^40 id"])
def test_weights_are_the_reference_byte_for_byte(units):
    from mapx import ops
    rng = np.random.RandomState(5)
    for n in (1, 63, 64, 65, 1000):
        u = {"rows": None, "repeats": rng.randint(0, 7, n).astype(np.int64),
             "a 2^40 id": np.arange(n, dtype=np.int64) + (2 ** 40 + 7)}[units]
        for R in (1, 3, 4, 5, 260):
            got = ops.bootstrap_weights(n if u is None else torch.from_numpy(u).to(DEV), R, SEED)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (R, n)
            want = B.weights(n if u is None else u, R, SEED)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (units, n, R)
            if u is not None and units == "repeats":
                assert all((want[:, u == k] == want[:, u == k][:, :1]).all() for k in range(7))
    w = ops.bootstrap_weights(torch.tensor([0, 1, 2, 3, 4, 2 ** 40 + 7], device=DEV), 8, SEED).cpu().numpy()
    assert w.T.tolist() == [[1, 0, 1, 1, 0, 1, 0, 3], [1, 0, 0, 2, 2, 3, 0, 4], [0, 4, 0, 2, 0, 1, 0, 0],
                            [1, 0, 1, 1, 0, 1, 1, 2], [0, 1, 2, 0, 0, 0, 0, 1], [3, 0, 3, 2, 1, 1, 2, 1]]
    assert ops.bootstrap_weights(5, 3, SEED + 1).cpu().numpy().tobytes() != B.weights(5, 3, SEED).tobytes()


def test_weights_fill_a_guarded_matrix_only():
    """The entry itself, into a guard-banded [R, n]: nothing outside it is written."""
    from mapx import native
    for n, R in ((65, 5), (1000, 3)):
        view, chk = guarded(R, n, torch.uint8, what=f"weights {n} x {R}")
        native.check(native.lib.mapx_bootstrap_weights(None, n, R, SEED, view.data_ptr(), native.stream()))
        chk()
        assert view.cpu().numpy().tobytes() == B.weights(n, R, SEED).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name):
    c = _case(name)
    got, want = c["got"], c["want"]
    for k in ("u2", "pos_w", "neg_w"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
    nz = want["sum_loss"] != 0
    rel = float(np.max(np.abs(got["sum_loss"][nz] - want["sum_loss"][nz]) / want["sum_loss"][nz])) if nz.any() else 0.0
    print(f"{name}: n {len(c['x'])} R {c['R']}; sum_loss max relative difference {rel:.3e}")
    np.testing.assert_allclose(got["sum_loss"], want["sum_loss"], rtol=RTOL, atol=0, err_msg=name)
    y = c["y"] > 0.5
    assert np.array_equal(got["pos_w"], c["w"][:, y].sum(1).astype(np.uint64))
    assert np.array_equal(got["neg_w"], c["w"][:, ~y].sum(1).astype(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_call_gives_the_same_bits(name):
    from mapx import ops
    c = _case(name)
    again = _host(ops.bootstrap_metrics(c["dev_in"][0], c["dev_in"][1], c["R"], seed=SEED, units=c["dev_in"][2]))
    for k in B.NAMES:
        assert again[k].tobytes() == c["got"][k].tobytes(), (name, k)


def test_what_the_cases_are_meant_to_reach():
    pos, eq, nan, clu, dec = (_case(k) for k in ("all positive", "all equal", "nan logit", "clustered", "one decimal"))
    assert not pos["got"]["u2"].any() and not pos["got"]["neg_w"].any() and pos["got"]["pos_w"].all()
    assert np.array_equal(eq["got"]["u2"], eq["got"]["pos_w"] * eq["got"]["neg_w"])      # one tie run: AUC 0.5
    assert np.isnan(nan["x"][7]) and np.isfinite(nan["got"]["sum_loss"]).all()
    assert (clu["units"] == 2 ** 40 + 7).sum() > 1 and len(np.unique(clu["units"])) == 51
    bits = _device_p32(dec["x"]).view(np.uint32)
    assert np.bincount(np.unique(bits, return_inverse=True)[1]).max() > 64     # a tie run longer than a wave's step
    # a unit's rows share a weight, so a replicate of clustered units is not the replicate of rows
    from mapx import ops
    rows = _host(ops.bootstrap_metrics(clu["dev_in"][0], clu["dev_in"][1], clu["R"], seed=SEED))
    assert not np.array_equal(rows["pos_w"], clu["got"]["pos_w"])


def test_sizes_outside_the_limits_are_refused():
    from mapx import native, ops
    x, y = torch.zeros(10, device=DEV), torch.ones(10, device=DEV)
    for R in (0, 65537):
        with pytest.raises(ValueError, match="replicates"):
            ops.bootstrap_metrics(x, y, R)
        with pytest.raises(ValueError, match="replicates"):
            ops.bootstrap_weights(10, R)
    with pytest.raises(ValueError, match="10 logits, 9 labels"):
        ops.bootstrap_metrics(x, y[:9], 4)
    with pytest.raises(ValueError, match="10 rows, 9 units"):
        ops.bootstrap_metrics(x, y, 4, units=torch.zeros(9, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.bootstrap_metrics(x, y, 4, units=torch.zeros(10, dtype=torch.int32, device=DEV))
    with pytest.raises(native.MapxError):
        ops.bootstrap_metrics(x.cpu(), y.cpu(), 4)
    lib = native.lib
    out = torch.zeros(4, dtype=torch.int64, device=DEV)
    for n, R in ((0, 4), (2 ** 28 + 1, 4), (10, 0), (10, 65537)):
        assert lib.mapx_bootstrap_workspace_bytes(n, R) == 256
        assert lib.mapx_bootstrap_metrics(x.data_ptr(), y.data_ptr(), None, n, R, 0, *(out.data_ptr(),) * 4,
                                          out.data_ptr(), 32, native.stream()) == -1           # MAPX_EINVAL
        assert lib.mapx_bootstrap_weights(None, n, R, 0, out.data_ptr(), native.stream()) == -1
    assert not out.any()
    empty = ops.bootstrap_metrics(x[:0], y[:0], 3)
    assert all(t.numel() == 3 and not t.any() for t in empty) and tuple(ops.bootstrap_weights(0, 3).shape) == (3, 0)


def test_two_models_on_the_same_rows_see_the_same_resample():
    from mapx import ops, score
    rng = np.random.RandomState(23)
    n, R = 3000, 40
    a = (rng.randint(-6, 7, n) * 0.5).astype(np.float32)                 # 2 a + 1 is exact and keeps every tie
    b, c = 2 * a + 1, rng.randn(n).astype(np.float32)
    ranks = lambda v: np.unique(_device_p32(v).view(np.uint32), return_inverse=True)[1]
    assert np.array_equal(ranks(a), ranks(b)) and len(np.unique(ranks(a))) == 13       # on the host, first
    y = torch.from_numpy((rng.rand(n) < 0.3).astype(np.float32)).to(DEV)
    A, A2, Bm, Cm = (_host(ops.bootstrap_metrics(torch.from_numpy(v).to(DEV), y, R, seed=SEED)) for v in (a, a, b, c))
    for other in (A2, Bm, Cm):
        assert np.array_equal(other["pos_w"], A["pos_w"]) and np.array_equal(other["neg_w"], A["neg_w"])
    assert np.array_equal(Bm["u2"], A["u2"]) and not np.array_equal(Cm["u2"], A["u2"])
    point = dict(auc=0.5, logloss=0.5)
    delta = score.bootstrap_report(A, point, other=A2, other_point=point)["delta"]
    for k in ("auc", "logloss"):
        assert delta[k]["point"] == delta[k]["lo"] == delta[k]["hi"] == 0.0
        assert delta[k]["frac_zero"] == 1.0 and delta[k]["frac_positive"] == 0.0
    assert score.bootstrap_report(A, point, other=Bm, other_point=point)["delta"]["auc"]["frac_zero"] == 1.0
    other_seed = _host(ops.bootstrap_metrics(torch.from_numpy(a).to(DEV), y, R, seed=SEED + 1))
    with pytest.raises(ValueError, match="same resample"):
        score.bootstrap_report(A, point, other=other_seed, other_point=point)


def test_the_point_estimate_lies_inside_the_interval():
    from mapx import ops, score
    rng = np.random.RandomState(31)
    n, R = 20000, 200
    y = (rng.rand(n) < 0.2).astype(np.float32)
    x = (rng.randn(n) + 1.2 * y - 1.6).astype(np.float32)
    p32 = _device_p32(x)
    one = B.reference(p32, y, np.ones((1, n), np.int64))
    point = dict(auc=float(B.auc_of(one)[0]), logloss=float(one["sum_loss"][0]) / n)
    want = B.reference(p32, y, B.weights(n, R, SEED))
    dx, dy = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    got = _host(ops.bootstrap_metrics(dx, dy, R, seed=SEED))
    m = ops.eval_metrics(dx, dy)
    assert m["auc"] == point["auc"] and m["logloss"] == pytest.approx(point["logloss"], rel=RTOL)
    for arrays in (want, got):                                           # the reference first
        rep = score.bootstrap_report(arrays, point)
        for k in ("auc", "logloss"):
            print(k, rep[k])
            assert rep[k]["lo"] <= point[k] <= rep[k]["hi"] and rep[k]["undefined"] == 0 and rep[k]["replicates"] == R
            assert 0 < rep[k]["std"] < 0.05 and abs(rep[k]["mean"] - point[k]) < 3 * rep[k]["std"]
    assert all(np.array_equal(got[k], want[k]) for k in B.NAMES[:3])
