"""The two launches of a scoring step (csrc/score.hip behind ops.score_block / ops.score_sink) against torch slices:
every extent case of the cursor and N, guard bands around everything they write, the cursor's walk, and the sigmoid
they share with the evaluation metrics (csrc/common.h: sigmoid_f32)."""
import numpy as np
import pytest
import torch

from guarded import guarded, padded_copy

pytestmark = pytest.mark.gpu
DEV = "cuda"
BS, FS = (1, 63, 64, 65, 257), (1, 23, 39, 64)
OOV_FILL, F32_FILL = 0xEE, -5.0


def _cases(B):
    """(name, cursor, N, rows of the id matrix) around an id matrix of 2B + 5 rows."""
    rows = 2 * B + 5
    return [("inside, odd start", 3, rows, rows), ("inside, start at a multiple of four", 4, rows, rows),
            ("straddles N", rows - B // 2 - 1, rows, rows), ("straddles an N inside the matrix", 4, B + 2, rows),
            ("cursor == N", rows, rows, rows), ("cursor > N", rows + 7, rows, rows), ("cursor far behind N", 10 * rows, 5, rows),
            ("N == 0", 0, 0, rows), ("N == 0, cursor ahead", 9, 0, rows)]


def _logits(B, rng):
    """Logits whose sigmoid is a normal fp32 number (|x| <= 80: sigmoid(-80) = 1.8e-35), edge values first."""
    x = (rng.randn(B) * 6).astype(np.float32)
    edge = np.array([0.0, -0.0, 80.0, -80.0, 1e-8, -1e-8, 16.6, -16.6, 1.0, -1.0], dtype=np.float32)
    x[:min(B, len(edge))] = edge[:B]
    return x


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("B", BS)
def test_block_and_sink_against_torch_slices(B, F):
    from mapx import ops
    rng = np.random.RandomState(1000 * B + F)
    for pitch, col0 in ((F, 0), (F + 3, 1)):                     # dense rows; a row pitch > F at an 8-byte aligned start
        for name, cur, N, rows in _cases(B):
            what = f"B {B} F {F} pitch {pitch}: {name}"
            ids_t = torch.from_numpy(rng.randint(0, 12, (rows, F)).astype(np.int64)).to(DEV)
            oov_id = torch.from_numpy(rng.randint(0, 12, F).astype(np.int64)).to(DEV)
            ids, ids_chk = padded_copy(ids_t, ld=pitch, col0=col0, what="ids")
            batch, batch_chk = guarded(B, F, torch.int64, what="batch")
            oov2, oov_chk = guarded(1, rows, torch.uint8, what="oov_fields")
            probs2, probs_chk = guarded(1, rows, torch.float32, what="probs")
            lout2, lout_chk = guarded(1, rows, torch.float32, what="logits_out")
            oov, probs, lout = oov2[0], probs2[0], lout2[0]
            batch.fill_(-77); oov.fill_(OOV_FILL); probs.fill_(F32_FILL); lout.fill_(F32_FILL)
            logits_np = _logits(B, rng)
            logits, logits_chk = padded_copy(torch.from_numpy(logits_np).to(DEV)[None, :], what="logits")
            cursor = torch.tensor([cur], dtype=torch.int64, device=DEV)
            done = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.score_block(ids, N, cursor, oov_id, batch, oov)
            ops.score_sink(logits[0], N, cursor, probs, lout)
            assert int(cursor) == cur, what                           # the two launches only read it
            ops.step_advance(done, cursor, B)
            assert int(cursor) == cur + B and int(done) == 1, what    # the step leaves the cursor at the next batch
            for chk in (ids_chk, batch_chk, oov_chk, probs_chk, lout_chk, logits_chk):
                chk()
            lo, hi = min(cur, N), min(cur + B, N)                     # the rows of [0, N) this step owns
            want = torch.zeros(B, F, dtype=torch.int64, device=DEV)   # <pad> rows behind N
            want[:hi - lo] = ids_t[lo:hi]
            assert torch.equal(batch, want), what
            assert torch.equal(oov[lo:hi], (ids_t[lo:hi] == oov_id).sum(1).to(torch.uint8)), what
            got_l, got_p = lout.cpu().numpy(), probs.cpu().numpy()
            assert np.array_equal(got_l[lo:hi].view(np.int32), logits_np[:hi - lo].view(np.int32)), what   # -0.0 too
            x = logits_np[:hi - lo].astype(np.float64)
            np.testing.assert_allclose(got_p[lo:hi].astype(np.float64), 1.0 / (1.0 + np.exp(-x)), rtol=1e-6, atol=0,
                                       err_msg=what)
            outside = np.ones(rows, dtype=bool)
            outside[lo:hi] = False                                    # ... and nothing else of the outputs
            assert bool((oov.cpu().numpy()[outside] == OOV_FILL).all()), what
            assert bool((got_l[outside] == F32_FILL).all()) and bool((got_p[outside] == F32_FILL).all()), what


def test_saturated_logits_give_exact_zero_and_one():
    from mapx import ops
    x = torch.tensor([200.0, -200.0, float("inf"), float("-inf"), 30.0, 0.0], device=DEV)
    probs, lout = torch.full((6,), F32_FILL, device=DEV), torch.full((6,), F32_FILL, device=DEV)
    ops.score_sink(x, 6, torch.zeros(1, dtype=torch.int64, device=DEV), probs, lout)
    assert probs.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.5] and torch.equal(lout, x)


def test_a_walk_of_replays_scores_every_row_once_and_shares_the_metrics_sigmoid():
    """Four steps of B = 257 walk N = 1000 rows by the device cursor alone (the last one straddles N).  The float64
    log-loss recomputed on the host from the WRITTEN probs (sklearn's clip to [eps, 1 - eps], eps = 2^-52) equals
    eval_metrics(logits, labels)['logloss'] to the order of an fp64 sum over 1e3 terms: the metrics kernel's
    probabilities are the ones the sink wrote."""
    from mapx import ops
    B, N, F = 257, 1000, 23
    rng = np.random.RandomState(5)
    ids = torch.from_numpy(rng.randint(0, 30, (N, F)).astype(np.int64)).to(DEV)
    oov_id = torch.from_numpy(rng.randint(0, 30, F).astype(np.int64)).to(DEV)
    all_logits = torch.from_numpy((rng.randn(4 * B) * 5).astype(np.float32)).to(DEV)
    labels = torch.from_numpy((rng.rand(N) < 0.3).astype(np.float32)).to(DEV)
    batch = torch.empty(B, F, dtype=torch.int64, device=DEV)
    oov, oov_chk = guarded(1, N, torch.uint8)
    probs, probs_chk = guarded(1, N, torch.float32)
    lout, lout_chk = guarded(1, N, torch.float32)
    cursor, done = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(4):
        ops.score_block(ids, N, cursor, oov_id, batch, oov[0])
        want = torch.zeros_like(batch)
        want[:max(0, min(B, N - k * B))] = ids[k * B:(k + 1) * B]
        assert torch.equal(batch, want), k
        ops.score_sink(all_logits[k * B:(k + 1) * B], N, cursor, probs[0], lout[0])
        ops.step_advance(done, cursor, B)
    assert int(cursor) == 4 * B and int(done) == 4
    for chk in (oov_chk, probs_chk, lout_chk):
        chk()
    assert torch.equal(lout[0], all_logits[:N]) and torch.equal(oov[0], (ids == oov_id).sum(1).to(torch.uint8))
    p = probs[0].cpu().numpy().astype(np.float64)
    y = labels.cpu().numpy() > 0.5
    eps = np.finfo(np.float64).eps
    q = np.clip(np.where(y, p, 1.0 - p), eps, 1.0 - eps)
    host = float(-np.log(q).mean())
    dev = ops.eval_metrics(all_logits[:N], labels)["logloss"]
    print(f"logloss host {host!r} device {dev!r} rel {abs(host - dev) / host:.3e}")
    np.testing.assert_allclose(dev, host, rtol=1e-12, atol=0)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from mapx import ops
    from mapx.native import MapxError
    i64 = dict(dtype=torch.int64, device=DEV)
    cur, ids = torch.zeros(1, **i64), torch.zeros(8, 65, **i64)
    with pytest.raises(MapxError, match="F <= 64"):
        ops.score_block(ids, 8, cur, torch.zeros(65, **i64), torch.zeros(4, 65, **i64), torch.zeros(8, dtype=torch.uint8, device=DEV))
    ids = torch.zeros(8, 5, **i64)
    with pytest.raises(ValueError):                                           # more rows than the matrix holds
        ops.score_block(ids, 9, cur, torch.zeros(5, **i64), torch.zeros(4, 5, **i64), torch.zeros(9, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):                                            # an int32 cursor
        ops.score_block(ids, 8, cur.int(), torch.zeros(5, **i64), torch.zeros(4, 5, **i64), torch.zeros(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):                                           # outputs shorter than N
        ops.score_sink(torch.zeros(4, device=DEV), 8, cur, torch.zeros(7, device=DEV), torch.zeros(8, device=DEV))
    with pytest.raises(MapxError):
        ops.score_sink(torch.zeros(4), 4, cur, torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))
