"""The planted-maximum cases of tests/amax_planted.py, checked on the CPU: for every builder and every planted position
the float64 restatement's largest finite |value| sits at the planted position, and the runner-up is at most 2^-8 of it.
This is what keeps tests/test_amax_planted_gpu.py from passing with a plant in the wrong place."""
import pytest
import torch

import amax_planted as AP


def _check_all(cases, min_cases):
    n = 0
    for c in cases:
        AP.assert_planted(c.ref, c.pos, c.name)
        n += 1
    assert n >= min_cases


@pytest.mark.parametrize("shape", list(AP.GEMM_SHAPES))
def test_gemm_epilogue_plants(shape):
    M, N, K, b_kc, epis, tiles = AP.GEMM_SHAPES[shape]
    pos = AP.gemm_positions(M, N, tiles)
    # corners, the tile-boundary pairs, the four lanes of the last float4, an interior element
    assert {(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1), (M - 1, N - 4), (M - 1, N - 3), (M - 1, N - 2)} <= set(pos)
    for bm, bn in tiles:
        if bm < M and bn < N:
            assert (bm - 1, bn - 1) in pos and (bm, bn) in pos
    _check_all(AP.gemm_cases(shape), len(epis) * len(pos))


def test_concat_plants():
    _check_all(AP.concat_cases(), 6)


@pytest.mark.parametrize("wide", [False, True])
def test_fused_backward_plants(wide):
    n = left = 0
    M, N, K = AP.FUSED_WIDE if wide else AP.FUSED_SHAPE
    assert (-(-M // 128) * -(-N // 128) >= 160) == wide           # the launcher's own choice: tile 3 from 160 tiles on
    for c in AP.fused_cases(wide):
        assert (c.pos_t is None) != (c.pos_dz is None) or c.left_big
        if c.pos_t is not None:
            AP.assert_planted(c.ref_t, c.pos_t, c.name + " (t)")
        if c.pos_dz is not None:
            AP.assert_planted(c.ref_dz, c.pos_dz, c.name + " (dz)")
        if c.left_big:
            # the largest value of C lies left of c0: far above everything the dz record may see
            where, peak, _ = AP.plant_report(c.ref_C)
            assert where[1] < c.c0 and float(c.ref_dz.abs().max()) <= AP.RUNNER_UP * peak
            left += 1
        n += 1
    assert (n, left) == (8, 0) if wide else (n >= 20 and left == 1)


@pytest.mark.parametrize("op", ["relu", "cross"])
@pytest.mark.parametrize("N", [128, 256])
def test_elementwise_colsum_plants(op, N):
    _check_all(AP.ew_cases(op, N), 16)


@pytest.mark.parametrize("E,lazy", [(16, False), (12, False), (64, False), (10, False), (16, True), (12, True), (64, True)])
def test_gather_plants(E, lazy):
    per_row, n, rows = AP.gather_geometry(E)
    assert (n - 1) * per_row >= AP.GATHER_TRIP              # the last row lies in the second grid-stride trip
    assert rows[-3] * per_row < AP.GATHER_TRIP <= rows[-2] * per_row     # the rows on either side of the trip boundary
    _check_all(AP.gather_cases(E, lazy), 2 * len(rows))


def test_nce_plants():
    _check_all(AP.nce_fwd_cases(), 3)
    _check_all(AP.nce_scatter_cases(), 3)


def test_join_plants():
    n = 0
    for c in AP.join_cases():
        if c.pos_t is not None:
            AP.assert_planted(c.ref_t, c.pos_t, c.name + " (t)")
        else:
            AP.assert_planted(c.ref_dzr, c.pos_dzr, c.name + " (dzr)")
        n += 1
    assert n == 16


@pytest.mark.parametrize("layout", list(AP.ADAMW_LAYOUTS))
def test_adamw_plants(layout):
    n, seg_off, plants = AP.ADAMW_LAYOUTS[layout]
    assert all(s % 8 == 0 for s in seg_off[:-1]) and seg_off[-1] == n
    for c in AP.adamw_cases(layout):
        AP.assert_planted(c.ref_seg, c.pos, c.name)
        assert float(c.ref.abs().max()) == float(c.ref_seg.abs().max())
    if layout == "direct":
        # block 0's range (1000 elements) starts in parameter 0 and touches more than 16 parameters
        assert sum(1 for s in seg_off[:-1] if s < 1000) > 16


def test_amax_and_nonfinite_plants():
    _check_all(AP.amax_cases(), 10)
    n = 0
    for c in AP.nonfinite_cases():
        assert int((~torch.isfinite(c.ref)).sum()) == 2
        AP.assert_planted(c.ref, c.pos, c.name)
        n += 1
    assert n == 3
