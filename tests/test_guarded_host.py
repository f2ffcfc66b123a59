"""tests/guarded.py on CPU tensors (no GPU): an untouched buffer passes, one changed element anywhere outside the view
is reported with its offset, views have the pitch and alignment asked for; and the cap on what
tests/test_extents_gpu.py may leave out: every ops function that forwards a row pitch to the library is in its tables."""
import ast
import os
import re

import pytest
import torch

import guarded as G

HERE = os.path.dirname(os.path.abspath(__file__))
OPS_PY = os.path.join(HERE, "..", "map-code_amd", "mapx", "ops.py")
EXTENTS_PY = os.path.join(HERE, "test_extents_gpu.py")

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8]

# Every ops function whose wrapper hands the library a row pitch: an x.stride(0) inside the call (what
# test_pitched_ops_are_all_in_the_extent_tables finds by reading ops.py), or a pitch that travels as a shape / an `ld`
# (the fused CIN kernels' pad8 pitches, cin_outer_fwd's pad_to, gemm_bwd_fused's (pointer, stride) pairs).  Written down
# once from ops.py; a function that starts forwarding a pitch fails the test below until it has a case.
PITCHED_OPS = [
    "seg_reduce_rows_extra",
    "cin_outer_fwd", "cin_outer_bwd", "cin_pool_fwd", "cin_pool_bwd",
    "cin_transpose_bf16", "cin_fused_fwd", "cin_fused_bwd_input", "cin_fused_bwd_weight",
    "cin_pool_fwd_bf16", "cin_pool_bwd_bf16",
    "enc_grouped_fwd", "enc_grouped_dw",
    "gemm_bf16", "gemm", "gemm_bwd_fused", "h2_weight_planes",
    "linear_fwd", "linear_bwd_input", "linear_bwd_weight", "skinny_join_bwd",
    "colsum", "relu_mask_colsum", "cross_bwd_pre_colsum",
    "act_fwd", "act_bwd",
    "amax",
]


def _el(dtype):
    return torch.empty(0, dtype=dtype).element_size()


@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_buffer_passes_and_layout(dtype):
    rows, cols, ld, col0 = 5, 7, 16, 4
    view, check = G.guarded(rows, cols, dtype, ld=ld, col0=col0, device="cpu")
    es = _el(dtype)
    assert view.shape == (rows, cols) and view.stride() == (ld, 1) and view.dtype == dtype
    g = check.guard
    assert g * es >= max(4096, ld * es) and (g * es) % 256 == 0
    assert check.flat.numel() == g + rows * ld + g
    # the view starts col0 elements into the first row, the first row a whole guard behind the allocation's start
    assert view.data_ptr() - check.flat.data_ptr() == (g + col0) * es
    assert (view.data_ptr() - col0 * es - check.flat.data_ptr()) % 256 == 0
    check()
    # writing the whole view is what a kernel is allowed to do
    view.copy_(torch.ones(rows, cols).to(dtype))
    check()
    assert check.damage() == (0, None)


def test_guard_is_a_full_row_pitch_when_that_is_larger():
    view, check = G.guarded(2, 3000, torch.float32, ld=3000, device="cpu")
    assert check.guard * 4 >= 3000 * 4 and (check.guard * 4) % 256 == 0


def test_alignment_asked_for():
    """row_sliceable / _rows16 want 16-byte rows (ld % 4, col0 % 4 floats), the bf16 GEMM pitches of 8 elements: a
    view whose col0 and ld meet the rule is aligned like that, relative to an allocation of at least that alignment."""
    for dtype, ld, col0, align in ((torch.float32, 24, 4, 16), (torch.float32, 20, 8, 16), (torch.bfloat16, 24, 8, 16),
                                   (torch.bfloat16, 12, 4, 8), (torch.int32, 9, 1, 4)):
        view, check = G.guarded(6, 4, dtype, ld=ld, col0=col0, device="cpu")
        off = view.data_ptr() - check.flat.data_ptr()
        assert off % align == 0 and (ld * _el(dtype)) % align == 0
        assert check.flat.data_ptr() % 16 == 0 and view.data_ptr() % align == 0
        for r in range(6):
            assert view[r].data_ptr() == view.data_ptr() + r * ld * _el(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front guard", "left pad", "right pad", "back guard", "first byte before", "first byte behind"])
def test_one_changed_element_is_reported_with_its_offset(dtype, where):
    rows, cols, ld, col0 = 4, 5, 12, 3
    view, check = G.guarded(rows, cols, dtype, ld=ld, col0=col0, device="cpu", what="probe")
    es, g = _el(dtype), check.guard
    flat_index = {"front guard": 17, "left pad": g + 2 * ld + 1, "right pad": g + 1 * ld + col0 + cols,
                  "back guard": g + rows * ld + 40, "first byte before": g - 1, "first byte behind": g + rows * ld}[where]
    one = torch.ones(1).to(dtype)[0]
    check.flat[flat_index] = one                  # plain torch indexing
    n, off = check.damage()
    assert n == 1
    # offset of the element relative to view[0, 0]; the first differing byte lies inside that element
    want = (flat_index - (g + col0)) * es
    assert want <= off < want + es
    assert (off < 0) == (flat_index < g + col0)
    with pytest.raises(AssertionError, match=r"probe: 1 guard / padding element\(s\) changed; first damaged byte at offset -?\d+"):
        check()


def test_several_changed_elements_are_counted_and_the_first_is_named():
    view, check = G.guarded(3, 4, torch.float32, ld=8, col0=0, device="cpu")
    g = check.guard
    check.flat[g + 4] = 0.0          # right pad of row 0
    check.flat[g + 8 + 7] = 0.0      # right pad of row 1
    check.flat[g + 24 + 5] = 0.0     # back guard
    n, off = check.damage()
    assert n == 3 and 16 <= off < 20


def test_a_rewritten_canary_is_not_damage_but_a_changed_payload_is():
    view, check = G.guarded(2, 2, torch.float32, ld=4, device="cpu")
    idt, bits = G.canary_bits(torch.float32)
    assert bool(torch.isnan(check.flat[0])) and int(check.flat.view(idt)[0]) == bits
    check.flat.view(idt)[3] = bits
    check()
    check.flat.view(idt)[3] = bits ^ 1            # still a NaN: a value comparison would not see it
    assert check.damage()[0] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_inputs_and_outputs_hold_different_canaries(dtype):
    """A NaN's payload survives arithmetic: f(input canary) stored over an output canary must not look untouched."""
    (idt, out_bits), (_, in_bits) = G.canary_bits(dtype), G.canary_bits(dtype, is_input=True)
    assert out_bits != in_bits
    _, out_chk = G.guarded(2, 3, dtype, ld=5, device="cpu")
    _, in_chk = G.padded_copy(torch.zeros(2, 3).to(dtype), ld=5)
    assert int(out_chk.flat.view(idt)[0]) == out_bits and int(in_chk.flat.view(idt)[0]) == in_bits
    if dtype.is_floating_point:
        assert bool(torch.isnan(out_chk.flat[0])) and bool(torch.isnan(in_chk.flat[0]))
        # the payload is handed on: what a stray store of f(input canary) would write differs from the output canary
        moved = (in_chk.flat[:1].float() * 2.0 + 1.0).to(dtype)
        assert int(moved.view(idt)[0]) != out_bits
    out_chk.flat[0] = in_chk.flat[0]
    assert out_chk.damage()[0] == 1


def test_padded_copy_holds_the_values_and_pins_its_padding():
    t = torch.arange(15, dtype=torch.float32).view(3, 5)
    view, check = G.padded_copy(t, ld=8, col0=2)
    assert torch.equal(view, t) and view.stride() == (8, 1)
    rows = torch.as_strided(check.flat, (3, 8), (8, 1), check.guard)
    assert bool(torch.isnan(rows[:, :2]).all()) and bool(torch.isnan(rows[:, 7:]).all())
    check()
    view, check = G.padded_copy(t, ld=8, col0=2, pad_value=0.0)
    rows = torch.as_strided(check.flat, (3, 8), (8, 1), check.guard)
    assert bool((rows[:, :2] == 0).all()) and bool((rows[:, 7:] == 0).all()) and torch.equal(view, t)
    assert bool(torch.isnan(check.flat[:check.guard]).all())          # the guards keep the canary
    check()
    rows[1, 7] = 1.0
    n, off = check.damage()                       # (0.0 -> 1.0 changes the element's upper bytes only)
    assert n == 1 and 0 <= off - ((1 * 8 + 7) - 2) * 4 < 4
    ti = torch.arange(6, dtype=torch.int64).view(2, 3)
    view, check = G.padded_copy(ti, ld=5, col0=1)
    assert torch.equal(view, ti)
    check()


def test_bad_windows_are_refused():
    with pytest.raises(ValueError):
        G.guarded(2, 5, torch.float32, ld=4, device="cpu")
    with pytest.raises(ValueError):
        G.guarded(2, 3, torch.float32, ld=4, col0=2, device="cpu")


# ----------------------------------------------------------------------------- the cap on what the GPU tables leave out
def _functions_that_forward_a_pitch():
    """Top-level functions of ops.py with a `stride(0)` inside the arguments of a call to lib.mapx_* (directly, or
    through a local name bound to such an entry: `fn = lib.mapx_a if ... else lib.mapx_b`)."""
    with open(OPS_PY) as f:
        tree = ast.parse(f.read())
    found = []
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef):
            continue
        entries = set()
        for node in ast.walk(fn):
            if isinstance(node, ast.Assign) and "lib.mapx_" in ast.unparse(node.value):
                entries.update(t.id for t in node.targets if isinstance(t, ast.Name))
        for node in ast.walk(fn):
            if not isinstance(node, ast.Call):
                continue
            callee = ast.unparse(node.func)
            if not (callee.startswith("lib.mapx_") or callee in entries):
                continue
            args = " ".join(ast.unparse(a) for a in list(node.args) + [k.value for k in node.keywords])
            if "stride(0)" in args:
                found.append(fn.name)
                break
    return found


def test_pitched_ops_are_all_in_the_extent_tables():
    forwards = _functions_that_forward_a_pitch()
    assert len(forwards) >= 20, forwards                       # the scan itself still finds what it was written for
    missing = [f for f in forwards if f not in PITCHED_OPS]
    assert not missing, f"ops functions that forward a row pitch but have no guard-band case: {missing}"
    with open(EXTENTS_PY) as f:
        src = f.read()
    table = re.search(r"^TIER_A = \[(.*?)^\]", src, re.S | re.M)
    assert table, "tests/test_extents_gpu.py: the literal TIER_A table"
    named = set(re.findall(r'"(\w+)"', table.group(1)))
    assert not [f for f in PITCHED_OPS if f not in named], sorted(set(PITCHED_OPS) - named)
    for f in PITCHED_OPS:                                      # ... and the table's entries are really called
        assert re.search(rf"\bops\.{f}\(", src), f"TIER_A names {f} but no test calls ops.{f}"
