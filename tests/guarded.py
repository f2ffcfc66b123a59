"""Guard-band buffers for the extent and row-pitch tests (a plain helper module, no fixtures).

guarded(rows, cols, dtype, ld, col0) lays one flat allocation out as

    [ front guard | rows x ld elements | back guard ]

and hands out the [rows, cols] window at column col0 of the middle part (stride (ld, 1)).  Both guards and every padding
column ([0, col0) and [col0 + cols, ld) of each row) hold a fixed canary bit pattern (one for buffers a kernel writes,
another for operands it only reads); check() reads them back as integers and fails unless they are bit-identical to
it.  A kernel that stores outside its extent, or walks an operand with its width where it should use its pitch,
changes a canary (stores) or reads a NaN (loads).  padded_copy(t, ld, col0, pad_value) builds an input operand so.
"""
import torch

GUARD_MIN_BYTES = 4096
GUARD_ALIGN = 256

# element type -> (integer type of the same size, canary bits of an output buffer, ... of an input buffer).
# Two patterns per floating type: hardware hands a quiet NaN's payload on, so a kernel that loads one element too many
# from an input's guard and stores f(it) one element too far would write the pattern it overwrites if both guards held
# the same one.  The integer patterns differ likewise (a copy kernel moves them unchanged).
_CANARY = {
    torch.float32: (torch.int32, 0x7FC5A5A5, 0x7FD2C3B4),              # quiet NaNs, payloads 0x5A5A5 / 0x12C3B4
    torch.bfloat16: (torch.int16, 0x7FE5, 0x7FD3),                     # quiet NaNs, payloads 0x25 / 0x13
    torch.float16: (torch.int16, 0x7E5A, 0x7E33),                      # quiet NaNs, payloads 0x5A / 0x33
    torch.float64: (torch.int64, 0x7FF800005A5AA5A5, 0x7FF8000012C3B4D5),
    torch.int32: (torch.int32, 0x5A5AA5A5, 0x3C3CC3C3),
    torch.int64: (torch.int64, 0x5A5AA5A55A5AA5A5, 0x3C3CC3C33C3CC3C3),
    torch.uint8: (torch.uint8, 0xA5, 0x3C),
}


def canary_bits(dtype, is_input=False):
    """-> (integer dtype of the element size, the canary's bit pattern as a Python int)."""
    idt, out_bits, in_bits = _CANARY[dtype]
    return idt, (in_bits if is_input else out_bits)


def guard_elems(ld, dtype):
    """Elements of one guard: at least max(4096 bytes, one full row pitch), a multiple of 256 bytes."""
    es = torch.empty(0, dtype=dtype).element_size()
    nbytes = max(GUARD_MIN_BYTES, ld * es)
    nbytes = (nbytes + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN
    return nbytes // es


class Check:
    """check() of one guarded buffer; callable.  `flat` is the whole allocation (element type of the view), `origin`
    the flat index of the view's element [0, 0]."""

    def __init__(self, flat_int, expected, mask, origin, es, what):
        self.flat_int, self.expected, self.mask, self.origin, self.es, self.what = flat_int, expected, mask, origin, es, what

    def damage(self):
        """-> (elements changed, byte offset of the first damaged byte relative to the view | None)."""
        bad = (self.flat_int != self.expected) & self.mask
        n = int(bad.sum())
        if n == 0:
            return 0, None
        first = int(bad.nonzero()[0, 0])
        got = self.flat_int[first:first + 1].cpu().view(torch.uint8)
        want = self.expected[first:first + 1].cpu().view(torch.uint8)
        byte = int((got != want).nonzero()[0, 0])
        return n, (first - self.origin) * self.es + byte

    def __call__(self):
        n, off = self.damage()
        assert n == 0, (f"{self.what}: {n} guard / padding element(s) changed; first damaged byte at offset {off} "
                        f"relative to the view" + (" (before row 0)" if off < 0 else ""))


def guarded(rows, cols, dtype, ld=None, col0=0, device="cuda", pad_value=None, what="guarded", is_input=False):
    """-> (view [rows, cols] with stride (ld, 1), check).  `pad_value`: what the padding columns hold instead of the
    canary (the guards always hold the canary); check() pins them to that value's bits.  `is_input`: the buffer holds
    an operand a kernel reads (padded_copy): the input canary."""
    ld = cols if ld is None else int(ld)
    if rows < 0 or cols < 0 or col0 < 0 or col0 + cols > ld:
        raise ValueError(f"guarded: columns [{col0}, {col0 + cols}) do not fit a pitch of {ld}")
    idt, bits = canary_bits(dtype, is_input)
    g = guard_elems(ld, dtype)
    body = rows * ld
    flat_int = torch.full((g + body + g,), bits, dtype=idt, device=device)
    flat = flat_int.view(dtype)
    es = flat.element_size()
    rows_view = torch.as_strided(flat, (rows, ld), (ld, 1), g)
    if pad_value is not None:
        rows_view.fill_(pad_value)
    mask = torch.ones(g + body + g, dtype=torch.bool, device=device)
    torch.as_strided(mask, (rows, cols), (ld, 1), g + col0).fill_(False)
    view = torch.as_strided(flat, (rows, cols), (ld, 1), g + col0)
    expected = flat_int.clone()
    chk = Check(flat_int, expected, mask, g + col0, es, what)
    chk.flat, chk.guard, chk.rows = flat, g, rows_view        # (rows: the [rows, ld] matrix the view is a window of)
    return view, chk


def padded_copy(t, ld=None, col0=0, pad_value=None, what="padded input"):
    """An input operand inside a guarded buffer: -> (view holding t's values, check)."""
    if t.dim() != 2:
        raise ValueError("padded_copy: a matrix")
    view, chk = guarded(t.shape[0], t.shape[1], t.dtype, ld=ld, col0=col0, device=t.device, pad_value=pad_value,
                        what=what, is_input=True)
    view.copy_(t)
    return view, chk
