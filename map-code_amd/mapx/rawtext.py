"""Raw Avazu / Criteo text -> device-resident int64 columns: read_feat of the reference's preprocessing
(data_preprocess/proc_avazu.py:26-85, proc_criteo.py:24-88) on the GPU.

The file is streamed in chunks cut at line ends (`iter_chunks`, pure host); every chunk is copied to the device,
indexed (line starts, physical line numbers) and parsed by the kernels of csrc/rawtext.hip behind
include/mapx_hip.h (mapx_rawtext_*), straight into preallocated columns.  The columns feed `vocab.build_vocab`;
`iter_columns` hands them over chunk by chunk instead (mapx.score: files that need not fit the device), and the
UNLABELED schemas read files without the click field.  There is no CPU parsing path.

The field grammar is deliberately stricter than Python's int(): `-?[0-9]{1,18}` for integers (no '+', blanks,
'_', decimal point), `[0-9a-f]{1,14}` for hash strings, exactly eight digits of a valid date and hour for Avazu's
`hour`, no quoting at all.  What the reference would accept beyond that raises ValueError here, with the file's
1-based physical line number, the column name and the reason.

Hash strings become the code `(value << 4) | width`: the width tag keeps '0a' and 'a' apart (they are different
keys of the reference's Counter) without asking for one width per column, keeps every code positive, and leaves
-1 for the empty field, which prints as '-1' — what trans_cat_feat writes (proc_criteo.py:42-47)."""
import ctypes as C
import functools
import gzip
import io
import os
import time

import numpy as np
import torch

from .native import MapxError, RawtextSchema, RT_MAX_FIELDS, check, lib, ptr, require_gpu, stream

SKIP, INT, BUCKET, HEX, YYMMDDHH = range(5)                     # MAPX_RT_* of include/mapx_hip.h
REASONS = {1: 'a quote (") in the line', 2: "too few fields", 3: "too many fields",
           4: "not an integer of the form -?[0-9]{1,18}", 5: "not 1 to 14 lower-case hexadecimal digits",
           6: "not eight digits YYMMDDHH of a valid date and hour"}
MAX_CHUNK = 1 << 30
_DATE_PARTS = ("weekday", "day", "hour", "is_weekend")          # proc_avazu.py:48-60, in valid_fields order


class Schema:
    """fields: [(source column name, kind)] in file order.  The output columns follow in the same order, a
    YYMMDDHH field giving weekday, day, hour, is_weekend; `label` names the output column that holds the labels.
    shuffle: whether the reference's generate_dataset() permutes the rows (proc_avazu.py:202-203 always;
    proc_criteo.py:98-102 only when down-sampling)."""

    def __init__(self, name, delimiter, header, fields, feat_types, shuffle, label="click"):
        if len(fields) > RT_MAX_FIELDS:
            raise ValueError(f"at most {RT_MAX_FIELDS} source fields")
        self.name, self.delimiter, self.header, self.shuffle, self.label = name, delimiter, header, shuffle, label
        self.source_names = [n for n, _ in fields]
        self.kinds = [k for _, k in fields]
        self.out_cols, self.columns, self.column_kinds = [], [], []
        for n, k in fields:
            self.out_cols.append(len(self.columns))
            if k == YYMMDDHH:
                self.columns += list(_DATE_PARTS)
                self.column_kinds += [INT] * 4
            elif k != SKIP:
                self.columns.append(n)
                self.column_kinds.append(k)
        self.string_columns = {n for n, k in zip(self.columns, self.column_kinds) if k == HEX}
        self.feat_types = {n: feat_types(n) for n in self.columns if n != label}
        # the shortest line the grammar admits: one byte per non-empty field, the delimiters, the line end
        self.min_line_bytes = len(fields) + sum(1 for k in self.kinds if k == INT) + sum(8 for k in self.kinds if k == YYMMDDHH)

    def struct(self):
        s = RawtextSchema()
        s.delimiter, s.n_fields = ord(self.delimiter), len(self.kinds)
        for f, (k, c) in enumerate(zip(self.kinds, self.out_cols)):
            s.kind[f], s.out_col[f] = k, c
        return s

    def decoder(self, column):
        """code -> the value as the reference's f'{name}-{k}' prints it."""
        if column in self.string_columns:
            return decode_hex
        return lambda c: str(int(c))


def decode_hex(code):
    code = int(code)
    return "-1" if code == -1 else format(code >> 4, f"0{code & 15}x")


def encode_hex(s):
    """The device's code of one hash string ('' is the empty field)."""
    if s == "":
        return -1
    if not (1 <= len(s) <= 14) or any(ch not in "0123456789abcdef" for ch in s):
        raise ValueError(f"{s!r}: not 1 to 14 lower-case hexadecimal digits")
    return (int(s, 16) << 4) | len(s)


_AVAZU_HASH = ("site_id", "site_domain", "site_category", "app_id", "app_domain", "app_category", "device_id",
               "device_ip", "device_model")
# proc_avazu.py:17-22: the file's header is `id` + feat_names; valid_fields = click, the four date parts, the rest
AVAZU = Schema("avazu", ",", True,
               [("id", SKIP), ("click", INT), ("hour", YYMMDDHH)] +
               [(n, HEX if n in _AVAZU_HASH else INT) for n in
                ("C1", "banner_pos") + _AVAZU_HASH + ("device_type", "device_conn_type", "C14", "C15", "C16", "C17",
                                                     "C18", "C19", "C20", "C21")],
               feat_types=lambda n: "<cat>", shuffle=True)
# proc_criteo.py:16-21: tab-separated, no header; click, I1..I13 (bucketed), C1..C26 (hash strings)
CRITEO = Schema("criteo", "\t", False,
                [("click", INT)] + [(f"I{i}", BUCKET) for i in range(1, 14)] + [(f"C{i}", HEX) for i in range(1, 27)],
                feat_types=lambda n: "<cat>" if "C" in n else "<num>", shuffle=False)
SCHEMAS = {"avazu": AVAZU, "criteo": CRITEO}


def _without_label(schema, name):
    """The schema of the same file without its label field (a file to be scored): label=None, labels come back None."""
    fields = [(n, k) for n, k in zip(schema.source_names, schema.kinds) if n != schema.label]
    return Schema(name, schema.delimiter, schema.header, fields, feat_types=lambda n: schema.feat_types[n],
                  shuffle=schema.shuffle, label=None)


# Avazu's test.gz (`id`, then hour, C1, ... — no `click`) and Criteo's test.txt (39 fields, no click): the same
# columns, kinds and codes as the labelled files, so a vocabulary saved from those applies as it is.
AVAZU_UNLABELED = _without_label(AVAZU, "avazu-unlabeled")
CRITEO_UNLABELED = _without_label(CRITEO, "criteo-unlabeled")
UNLABELED = {"avazu": AVAZU_UNLABELED, "criteo": CRITEO_UNLABELED}


def bucket_of(v):
    """proc_criteo.py:29-32 for an integer v: the expression itself."""
    v = int(v)
    return int(np.floor(np.log(v) ** 2)) if v > 2 else v


@functools.lru_cache(maxsize=None)
def bucket_thresholds():
    """t[b-1] = the smallest v in [3, 2^63 - 1] with floor(log(v)^2) >= b, for b = 1 .. bucket(2^63 - 1) (1906 of
    them), each by bisection on the reference's expression; for v > 2 the bucket is the number of thresholds <= v."""
    top = (1 << 63) - 1
    t = []
    for b in range(1, bucket_of(top) + 1):
        lo, hi = 3, top                                  # bucket(hi) >= b throughout
        if bucket_of(lo) >= b:
            hi = lo
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if bucket_of(mid) >= b:
                hi = mid
            else:
                lo = mid
        t.append(hi)
    return np.array(t, dtype=np.int64)


def iter_chunks(stream_, chunk_bytes=None):
    """Cuts a binary stream into pieces that end at a line end: yields (bytes, physical line number of the piece's
    first line, 0-based).  Reads up to chunk_bytes (None: everything) at a time, cuts at the last '\\n' and carries
    the rest over; the last piece may lack the '\\n'.  A line longer than a chunk raises ValueError."""
    if chunk_bytes is None:
        data = stream_.read()
        if data:
            yield data, 0
        return
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive")
    tail, line0 = b"", 0
    while True:
        if len(tail) >= chunk_bytes:
            raise ValueError(f"line {line0 + 1} is longer than a chunk of {chunk_bytes} bytes")
        block = stream_.read(chunk_bytes - len(tail))
        buf = tail + block
        if not block:                                    # end of the stream
            if buf:
                yield buf, line0
            return
        cut = buf.rfind(b"\n")
        if cut < 0:
            tail = buf
            continue
        yield buf[:cut + 1], line0
        line0 += buf.count(b"\n", 0, cut + 1)
        tail = buf[cut + 1:]


def first_line(data):
    """The first non-blank line of a piece (one trailing '\\r' stripped), or None."""
    pos = 0
    while pos < len(data):
        end = data.find(b"\n", pos)
        end = len(data) if end < 0 else end
        line = data[pos:end]
        if line.endswith(b"\r"):
            line = line[:-1]
        if line:
            return line
        pos = end + 1
    return None


def _round16(n):
    return (n + 15) // 16 * 16


def index_lines(buf, n_bytes, max_lines):
    """buf: uint8 device tensor of at least round_up(n_bytes, 16) bytes.  -> (line_start, line_no int32 [n_lines],
    n_lines, number of '\\n' bytes).  max_lines is a guess: the index is built again when the chunk holds more."""
    require_gpu(buf)
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() < _round16(n_bytes):
        raise TypeError("index_lines: buf must be a contiguous uint8 vector of at least round_up(n_bytes, 16) bytes")
    if n_bytes > MAX_CHUNK:
        raise ValueError("index_lines: a chunk holds at most 2^30 bytes")
    dev = buf.device
    ws_bytes = int(lib.mapx_rawtext_index_workspace_bytes(n_bytes))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    while True:
        line_start = torch.empty(max(max_lines, 1), dtype=torch.int32, device=dev)
        line_no = torch.empty(max(max_lines, 1), dtype=torch.int32, device=dev)
        check(lib.mapx_rawtext_index(ptr(buf), n_bytes, ptr(ws), ws.numel(), ptr(line_start), ptr(line_no), max_lines,
                                     ptr(counts), stream()))
        n_lines, n_nl = (int(x) for x in counts.tolist())          # offline path: host syncs are fine
        if n_lines <= max_lines:
            return line_start[:n_lines], line_no[:n_lines], n_lines, n_nl
        max_lines = n_lines


def parse_lines(buf, n_bytes, line_start, line_no, schema, out, row0=0, mode=0):
    """Parses the indexed lines into out [n_columns, >= row0 + n_lines] (int64, unit stride along a column; any
    column pitch): line i writes out[:, row0 + i].  -> None, or (line_no, source column, reason) of the bad line
    with the smallest physical line number."""
    require_gpu(buf, line_start, line_no, out)
    n_lines = line_start.numel()
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != len(schema.columns) or \
            (out.shape[0] > 1 and out.stride(1) != 1) or out.shape[1] < row0 + n_lines:
        raise TypeError("parse_lines: out must be int64 [n_columns, >= row0 + n_lines] with unit stride in a column")
    dev = buf.device
    err = torch.empty(1, dtype=torch.int64, device=dev)
    thr = _thresholds_on(dev)
    s = schema.struct()
    ld = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)
    check(lib.mapx_rawtext_parse(ptr(buf), n_bytes, line_start.data_ptr(), line_no.data_ptr(), n_lines, C.addressof(s),
                                 ptr(thr), thr.numel(), out.data_ptr(), ld, row0, len(schema.columns), ptr(err),
                                 int(mode), stream()))
    word = int(err.item()) & 0xFFFFFFFFFFFFFFFF
    if word == 0xFFFFFFFFFFFFFFFF:
        return None
    return word >> 32, (word >> 16) & 0xFFFF, word & 0xFFFF


_THR = {}


def _thresholds_on(dev):
    key = (dev.type, dev.index)
    if key not in _THR:
        _THR[key] = torch.from_numpy(bucket_thresholds()).to(dev)
    return _THR[key]


def _error(where, schema, line, col, reason):
    return ValueError(f"{where}: line {line}, column {schema.source_names[col]!r}: {REASONS.get(reason, reason)}")


def check_header(where, schema, line, line_number):
    names = line.decode("utf-8", "replace").split(schema.delimiter)
    if names != schema.source_names:
        raise ValueError(f"{where}: line {line_number}: the header names {names} are not the {schema.name} "
                         f"schema's {schema.source_names}")


class _Columns:
    """The [n_columns, capacity] output; grows by half when a chunk does not fit."""

    def __init__(self, n_cols, dev):
        self.n_cols, self.dev, self.rows, self.t = n_cols, dev, 0, None

    def reserve(self, more, total_guess=0):
        need = self.rows + more
        if self.t is not None and need <= self.t.shape[1]:
            return
        cap = max(need, total_guess, 0 if self.t is None else self.t.shape[1] * 3 // 2)
        new = torch.empty(self.n_cols, max(cap, 1), dtype=torch.int64, device=self.dev)
        if self.rows:
            new[:, :self.rows].copy_(self.t[:, :self.rows])
        self.t = new


def _iter_stream(stream_, schema, where, device, chunk_bytes, mode, place, timing=None):
    """The chunk loop: copy, index, check the header, parse.  place(n_lines, n_bytes) -> (out, row0): where the chunk's
    lines go (parse_lines); yields (out, row0, n_lines) per chunk that holds lines.  `timing` is filled at the end."""
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise MapxError("mapx.rawtext parses on the device (HIP); there is no CPU path")
    if chunk_bytes is not None and not (1 <= chunk_bytes <= MAX_CHUNK):
        raise ValueError("chunk_bytes must lie in [1, 2^30]")
    header_pending = schema.header
    pinned = dbuf = None
    t_read = t_copy = t_dev = 0.0
    clock = time.perf_counter
    t0 = clock()
    for data, line0 in iter_chunks(stream_, chunk_bytes):
        n = len(data)
        if n > MAX_CHUNK:
            raise ValueError(f"{where}: {n} bytes in one chunk; pass chunk_bytes <= 2^30")
        t1 = clock()
        t_read += t1 - t0
        n16 = _round16(n)
        if pinned is None or pinned.numel() < n16:
            pinned = torch.empty(n16, dtype=torch.uint8, pin_memory=True)
            dbuf = torch.empty(n16, dtype=torch.uint8, device=dev)
        pinned.numpy()[:n] = np.frombuffer(data, dtype=np.uint8)
        dbuf[:n].copy_(pinned[:n], non_blocking=True)
        if timing is not None:
            torch.cuda.synchronize(dev)
        t2 = clock()
        t_copy += t2 - t1
        line_start, line_no, n_lines, _ = index_lines(dbuf, n, n // schema.min_line_bytes + 1)
        if header_pending and n_lines:
            head = first_line(data)
            first_no = int(line_no[0].item())
            check_header(where, schema, head, line0 + first_no + 1)
            line_start, line_no, n_lines, header_pending = line_start[1:], line_no[1:], n_lines - 1, False
        out = None
        if n_lines:
            out, row0 = place(n_lines, n)
            bad = parse_lines(dbuf, n, line_start, line_no, schema, out, row0=row0, mode=mode)
            if bad is not None:
                raise _error(where, schema, line0 + bad[0] + 1, bad[1], bad[2])
        if timing is not None:
            torch.cuda.synchronize(dev)
        t3 = clock()
        t_dev += t3 - t2
        if out is not None:
            yield out, row0, n_lines               # (the consumer's time is nobody's share)
        t0 = clock()
    if header_pending:
        raise ValueError(f"{where}: no header line")
    if timing is not None:
        timing.update(read_s=t_read, copy_s=t_copy, device_s=t_dev)


def _read_stream(stream_, schema, where, device, chunk_bytes, mode, size_hint=0, timing=None):
    """The whole stream in one [n_columns, N] matrix: every chunk is parsed straight into its place."""
    cols = _Columns(len(schema.columns), torch.device(device))

    def place(n_lines, n_bytes):
        guess = 0
        if cols.t is None and size_hint > n_bytes:                     # a plain file: rows of this chunk, scaled
            guess = int(n_lines * (size_hint / n_bytes) * 1.02) + 64
        cols.reserve(n_lines, guess)
        return cols.t, cols.rows
    for _out, _row0, n_lines in _iter_stream(stream_, schema, where, device, chunk_bytes, mode, place, timing):
        cols.rows += n_lines
    cols.reserve(0)
    N = cols.rows
    columns = {name: cols.t[j, :N] for j, name in enumerate(schema.columns)}
    labels = columns.pop(schema.label) if schema.label is not None else None
    decode = {name: schema.decoder(name) for name in columns}
    return labels, columns, decode, set(schema.string_columns)


def _open(path):
    path = os.fspath(path)
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def iter_columns(path, schema, device="cuda", chunk_bytes=256 << 20, mode=0, timing=None):
    """read_columns one chunk at a time, for files that need not fit the device: yields, per chunk that holds lines,
    (labels int64 [n] | None for a schema without a label, int64 [n_columns, n] = the feature columns in the
    schema's order, a matrix of the chunk's own), the chunks in file order.  `path`: a file's path (`.gz` streamed
    through gzip) or an open binary stream.  Device memory in use is one chunk's text and columns."""
    stream_ = path if hasattr(path, "read") else _open(path)
    where = getattr(path, "name", "<stream>") if hasattr(path, "read") else os.fspath(path)
    dev = torch.device(device)
    n_cols = len(schema.columns)
    li = schema.columns.index(schema.label) if schema.label is not None else None
    feat = [j for j in range(n_cols) if j != li]
    try:
        place = lambda n_lines, _n: (torch.empty(n_cols, n_lines, dtype=torch.int64, device=dev), 0)
        for out, _row0, _n in _iter_stream(stream_, schema, where, dev, chunk_bytes, mode, place, timing):
            if li is None:
                yield None, out
            else:
                yield out[li], (out[1:] if li == 0 else out[feat])
    finally:
        if stream_ is not path:
            stream_.close()


def read_columns(path, schema, device="cuda", chunk_bytes=256 << 20, mode=0, timing=None):
    """-> (labels int64 [N], {column: int64 [N]} in the reference's valid_fields order, {column: decode},
    the set of string-origin columns), all tensors on the device.  `.gz` paths are streamed through gzip.
    mode: 0 = every wave stages its lines in LDS when they fit, 1 = every wave reads global memory.
    timing: a dict that receives the seconds spent reading the file, copying to the device and on the device."""
    path = os.fspath(path)
    with _open(path) as f:
        size = 0 if path.endswith(".gz") else os.fstat(f.fileno()).st_size
        return _read_stream(f, schema, path, device, chunk_bytes, mode, size_hint=size, timing=timing)


def parse_bytes(data, schema, device="cuda", chunk_bytes=None, mode=0, where="<bytes>"):
    """read_columns for a buffer in memory."""
    return _read_stream(io.BytesIO(bytes(data)), schema, where, device, chunk_bytes, mode)
