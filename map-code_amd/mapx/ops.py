"""Functional wrappers over the C ABI: tensors in, tensors out, no autograd.

Every function enqueues HIP kernels on torch's current stream and returns immediately.
Scratch memory is a per-(device, stream) byte buffer grown on demand; kernels that share it
run in stream order, so one buffer suffices.
"""
import math
import os

import torch

import ctypes

from . import native as N
from .native import check, lib, ptr, require_gpu, stream


def native_int():
    return ctypes.c_int(0)


def native_byref(x):
    return ctypes.byref(x)

_scratch = {}
_scratch_retired = []

# --------------------------------------------------------------------------- live kernel timing
# bench.py brackets kernel classes with HIP events on the launch stream (torch's current
# stream) while the timed region runs; nothing is recorded unless a Timers object is active.
_timers = None


class Timers:
    def __init__(self):
        self.events = {}          # name -> [(start, stop, work)]

    def __enter__(self):
        global _timers
        _timers = self
        return self

    def __exit__(self, *a):
        global _timers
        _timers = None

    def calibrate(self, n=32):
        """Record `n` empty brackets: their mean is the cost of the event pair itself (two
        event commands + one dependent dispatch gap), subtracted from every interval."""
        for _ in range(n):
            with _timed("__empty__"):
                pass

    def summary(self):
        """name -> dict(launches, total_ms, avg_us, work) after a device sync."""
        out = {}
        empty = self.events.pop("__empty__", None)
        over_ms = sum(a.elapsed_time(b) for a, b, _ in empty) / len(empty) if empty else 0.0
        for name, evs in self.events.items():
            ms = [max(a.elapsed_time(b) - over_ms, 0.0) for a, b, _ in evs]
            out[name] = dict(launches=len(evs), total_ms=sum(ms), avg_us=1e3 * sum(ms) / len(evs),
                             work=sum(w for _, _, w in evs), bracket_overhead_us=1e3 * over_ms)
        return out


class _timed:
    def __init__(self, name, work=0.0):
        self.name, self.work = name, work

    def __enter__(self):
        if _timers is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *e):
        if _timers is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _timers.events.setdefault(self.name, []).append((self.a, b, self.work))


# --------------------------------------------------------------------------- auxiliary streams
# Independent pieces of a step run on named side streams so that small or tail-heavy kernels
# fill the gaps of the big GEMMs: "plan" (sort + runs of the row ids) and "tower" (DCNv2's cross
# tower next to the deep tower).
# serialize_streams = True maps them all onto the current stream (per-kernel timing passes).
_aux_streams = {}
serialize_streams = os.environ.get("MAPX_SERIAL", "0") == "1"


def aux_stream(name, device, high=False):
    """Named side stream; `high`: high priority, i.e. hardware queues of its own class (work on it
    does not wait behind packets of normal-priority streams that happen to share a queue)."""
    if serialize_streams:
        return torch.cuda.current_stream()
    key = (name, device.index)
    st = _aux_streams.get(key)
    if st is None:
        st = _aux_streams[key] = torch.cuda.Stream(device=device, priority=-1 if high else 0)
    return st


pending_joins = []                # (waiting stream, side stream) left open by a backward node; the optimizer joins


def join_pending():
    """Join the side streams that backward nodes forked and left open (optimizer.step, or the end of a captured
    forward + backward whose tail runs elsewhere)."""
    while pending_joins:
        waiter, side = pending_joins.pop()
        stream_wait(waiter, side)
# "every dense gradient of this backward pass is final": an event recorded by the model's LAST backward node
# (the embedding gather of a tower model) before its own kernels; the optimizer's dense half may start there
dense_ready = [None, None]        # [event, stream it was recorded on]
# the Trainer's device scalar 1.0 that seeds loss.backward() (held here, so its address cannot be recycled):
# a head whose incoming gradient IS that tensor skips the multiply by it
unit_gradient = [None]
# True between MapxOptimizer.backward_window(True) and (False): optimizer.step() follows this backward pass at
# once and joins what it left open; outside the window backward() joins its side streams itself
step_window = [False]


def run_side_tasks():
    """Nothing queues side tasks any more (they carried the tables' early row updates); the benchmark's
    data-parallel rehearsal still calls this between backward and the exchange."""


# Late tasks: work of a backward node that nothing but the optimizer waits for (the grouped encoder's weight and
# bias gradients), queued instead of run on the chain that the towers' backward passes wait behind; the cross
# tower's backward node runs them at its END (its chain is the shorter one), optimizer.step() whatever is left.
_late_tasks = []


def add_late_task(fn):
    _late_tasks.append(fn)


def run_late_tasks():
    tasks = list(_late_tasks)
    _late_tasks.clear()
    for fn in tasks:
        fn()


# Main tasks: stream joins a backward node wants on the MAIN stream but not yet (the wait for a segment plan that the
# node's successors do not need); the towers' join node (layers._JoinColumns.backward) runs them, optimizer.step()
# whatever is left — always before the late tasks, which may read what they joined.
_main_tasks = []


def add_main_task(fn):
    _main_tasks.append(fn)


def run_main_tasks():
    while _main_tasks:
        _main_tasks.pop(0)()


def clear_side_tasks():
    """Drop tasks that an aborted backward pass left behind."""
    _late_tasks.clear()
    _main_tasks.clear()


_DBG_SLEEP = os.environ.get("MAPX_DBG_SLEEP", "")


def dbg_sleep(site):
    """Race hunting: MAPX_DBG_SLEEP=<site>[,<site>] parks the CURRENT stream for ~0.5 ms at the named sites (a missing
    cross-stream dependency then shows as a graph != eager or a parity failure instead of depending on timing)."""
    if _DBG_SLEEP and site in _DBG_SLEEP.split(",") and torch.cuda.is_available():
        torch.cuda._sleep(1_000_000)


def reset_aux_streams():
    """Forget the named side streams (new ones are made on demand) and everything a backward pass may have
    left queued on them: after a failed graph capture the streams may be stuck in the invalidated capture,
    and the per-backward lists (joins left open, deferred partial sums, side tasks, the dense-ready event)
    still name that capture's streams, events and partial buffers — an eager retry that found them would
    wait on a dead stream in optimizer.step() or sum stale partials into the bias gradients."""
    _aux_streams.clear()
    _scratch_retired.extend(_scratch.values())
    _scratch.clear()
    pending_joins.clear()
    step_window[0] = False
    _deferred.clear()
    _late_tasks.clear()
    _main_tasks.clear()
    dense_ready[0] = dense_ready[1] = None


def _capturing(st):
    """True if HIP stream `st` currently belongs to a stream capture (hipStreamIsCapturing)."""
    with torch.cuda.stream(st):
        return torch.cuda.is_current_stream_capturing()


class CaptureIsolationError(RuntimeError):
    pass


def _check_capture_join(waiter, waited, what):
    """A stream that belongs to a capture may only wait for work of the SAME capture.  Waiting for a
    stream that never joined it (it did not fork, directly or through other streams, from the capture's
    origin) puts un-captured work in front of captured work: HIP answers with
    hipErrorStreamCaptureIsolation at best and — seen in round 1 as a crash inside
    hipStreamEndCapture for a side-stream-to-side-stream join — invalidates the capture at worst.
    Refused here, in Python, before the runtime sees it."""
    if _capturing(waiter) and not _capturing(waited):
        raise CaptureIsolationError(
            f"{what}: the waiting stream belongs to a hipGraph capture but the stream it would wait for does not "
            "(it never forked from the capture's origin): fork it from the origin first (ops.stream_wait(side, "
            "origin)) or run that work on a stream of the capture")


def stream_wait(waiter, waited):
    """waiter.wait_stream(waited), skipped when both are the same HIP stream (a self-wait is a
    no-op when run eagerly, but inside a stream capture it hands hipStreamEndCapture a node that
    depends on itself); refused when it would join un-captured work into a capture."""
    if waiter.cuda_stream != waited.cuda_stream:
        _check_capture_join(waiter, waited, "stream_wait")
        waiter.wait_stream(waited)
        return True
    return False


def record_event():
    """An event at the current tail of the current stream: a fork point another stream can be
    made to wait on later (stream_wait_event), after more work has been enqueued here."""
    ev = torch.cuda.Event()
    ev.record()
    return ev


def stream_wait_event(waiter, event, origin):
    """waiter.wait_event(event) unless waiter is the stream the event was recorded on (`origin`);
    refused when `waiter` belongs to a capture that `origin` is not part of (see stream_wait)."""
    if waiter.cuda_stream != origin.cuda_stream:
        _check_capture_join(waiter, origin, "stream_wait_event")
        waiter.wait_event(event)
        return True
    return False


class Fork:
    """Work on the stream `side` beside the stream `origin`: fork, the allocator's record_stream rule and join, once.
        fork = Fork(side, origin)                # side waits for origin's tail; event=: for that event of origin's
        with fork: ...                           # side is the current stream
        fork.reads(...); fork.produces(...)      # tensors the side work reads / leaves for origin
        fork.join()  or  fork.leave_open()       # origin waits for side now / optimizer.step() joins (join_pending)
    `forked` is False when no edge was made (side IS origin: serialize_streams, or side is None: no device): the
    body then runs in place, nothing is recorded and nothing is left to join.  `after`: side also waits for what
    that stream has enqueued so far."""

    def __init__(self, side, origin, event=None, after=None):
        self.side, self.origin = side, origin
        self.forked = side is not None and (stream_wait(side, origin) if event is None
                                            else stream_wait_event(side, event, origin))
        if after is not None:
            with torch.cuda.stream(after):
                ev = record_event()
            stream_wait_event(side, ev, after)

    def __enter__(self):
        self._ctx = torch.cuda.stream(self.side)        # (None: a context that does nothing)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)

    def reads(self, *tensors):
        if self.forked:
            for t in tensors:
                t.record_stream(self.side)

    def produces(self, *tensors):
        if self.forked:
            for t in tensors:
                t.record_stream(self.origin)

    def join(self):
        if self.forked:
            stream_wait(self.origin, self.side)

    def leave_open(self):
        if self.forked:
            pending_joins.append((self.origin, self.side))


# --------------------------------------------------------------------------- deferred sums
# Split-K slabs (weight gradients) and row-chunk partials (bias gradients) of a backward pass
# are summed by ONE kernel launch right before their consumer (optimizer / gradient exchange)
# instead of one tiny launch each.  Only used when the destination is an optimizer-owned slot.
_deferred = []
COLSUM_CHUNKS = lib.mapx_colsum_chunks()


# What is deferred: the bias gradients' row-chunk partials and the streaming kernels' dW partials (tiny second-stage
# launches on the GEMM chains otherwise, 128 x N floats each: nothing to go cold).  The MFMA GEMMs' split-K slabs are
# NOT: they are summed right behind the GEMM, where they are still in L2 / Infinity Cache (DESIGN: "Retired switches").


def defer_sum(dst, src, stride, nsplit, n):
    _deferred.append((dst, src, int(stride), int(nsplit), int(n)))


def flush_deferred():
    """Launch the pending slab sums (32 tasks per launch)."""
    global _deferred
    cur = torch.cuda.current_stream() if torch.cuda.is_available() else None
    while _deferred:
        batch, _deferred = _deferred[:32], _deferred[32:]
        if cur is not None:
            for (_, src, _, _, _) in batch:       # partial buffers die with this list: keep them from being
                src.record_stream(cur)            # recycled while another stream than their own still reads them
        arr = (N.SumTask * len(batch))()
        for i, (dst, src, stride, nsplit, n) in enumerate(batch):
            arr[i].dst, arr[i].src = dst.data_ptr(), src.data_ptr()
            arr[i].stride, arr[i].n, arr[i].nsplit = stride, n, nsplit
        check(lib.mapx_sum_tasks(arr, len(batch), stream()))


def scratch(nbytes, device):
    key = (device.index, stream())
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _scratch_retired.append(buf)    # a captured graph may have the old address baked in: never free it
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


def _err_flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


# --------------------------------------------------------------------------- embedding
BF16 = torch.bfloat16


def is_bf16(t):
    return t is not None and t.dtype == torch.bfloat16


def cast_bf16(x):
    """fp32 -> bf16 copy (round to nearest even) by the library's kernel."""
    require_gpu(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(lib.mapx_cast_f32_bf16(ptr(x), x.numel(), ptr(out), stream()))
    return out


def cast_f32(x):
    require_gpu(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib.mapx_cast_bf16_f32(ptr(x), x.numel(), ptr(out), stream()))
    return out


def bf16_weight(w):
    """The bf16 operand of a dense fp32 master weight: the shadow the optimizer keeps current
    (`w._mapx_bf16`, written by the AdamW kernel itself), or a fresh conversion when no optimizer
    owns the parameter (inference / tests)."""
    sh = getattr(w, "_mapx_bf16", None)
    return sh if sh is not None else cast_bf16(w.detach())


def emb_gather(ids, table, validate=False, out_dtype=torch.float32, lazy=None):
    """ids int64 [...], table [V,E] -> [..., E]  (layers.py:97-102); bf16 rows in bf16 compute mode.
    lazy (native.LazyRows): rows are read through their pending zero-gradient updates (no catch-up pass ran)."""
    require_gpu(ids, table)
    ids = ids.contiguous()
    out = torch.empty(*ids.shape, table.shape[1], dtype=out_dtype, device=table.device)
    err = _err_flag(table.device) if validate else None
    rec = amax_record(table.device) if out_dtype != BF16 else None
    with _timed("emb_gather", ids.numel() * (8 + (4 + out.element_size()) * table.shape[1])):
        if out_dtype == BF16:
            check(lib.mapx_emb_gather_fwd_bf16(ptr(ids), ids.numel(), ptr(table), table.shape[0], table.shape[1],
                                               ptr(out), ptr(err), None if lazy is None else native_byref(lazy), stream()))
        else:
            check(lib.mapx_emb_gather_fwd(ptr(ids), ids.numel(), ptr(table), table.shape[0], table.shape[1],
                                          ptr(out), ptr(err), ptr(rec), None if lazy is None else native_byref(lazy),
                                          stream()))
    tag(out, rec)
    if validate and int(err.item()):
        raise IndexError("index out of range in self")          # reference CPU behaviour
    return out


_keys_of = [None, None]      # (id matrix, its int32 keys) as the last dynamic_mask_mfp produced them


def ids_to_i32(ids, V, validate=False):
    require_gpu(ids)
    if not validate and _keys_of[0] is ids:
        return _keys_of[1]       # the mask kernel wrote them already
    ids = ids.contiguous()
    out = torch.empty(ids.numel(), dtype=torch.int32, device=ids.device)
    err = _err_flag(ids.device) if validate else None
    check(lib.mapx_ids_to_i32(ptr(ids), ids.numel(), V, ptr(out), ptr(err), stream()))
    if validate and int(err.item()):
        raise IndexError("index out of range in self")
    return out


class SegPlan:
    """Sorted-run description of n int32 keys (see include/mapx_hip.h: mapx_seg_plan)."""

    def __init__(self, keys_i32, V, sorted_lists=0, launch=True):
        """`sorted_lists` = w > 0: the keys are w concatenated lists of equal length, each ascending
        as unsigned values and free of repeats except trailing -1 padding (the gathered messages
        of mapx.parallel): ranked by one merge launch instead of the radix passes, same outputs.
        `launch=False`: only allocate the outputs (SegPlan.build_many launches several plans at once)."""
        require_gpu(keys_i32)
        n, dev = keys_i32.numel(), keys_i32.device
        self.n, self.V = n, V
        i32 = dict(dtype=torch.int32, device=dev)
        self.sorted_keys = torch.empty(max(n, 1), **i32)
        self.perm = torch.empty(max(n, 1), **i32)
        self.rank = torch.empty(max(n, 1), **i32)
        self.uniq = torch.empty(max(n, 1), **i32)
        self.seg_start = torch.empty(n + 1, **i32)
        self.n_uniq = torch.empty(2, **i32)         # [number of runs, owner counter (zeroed by the plan)]
        self._counter_fresh = n > 0
        if not launch:
            return
        nb = lib.mapx_seg_plan_workspace_bytes(n, V)
        ws = scratch(nb, dev)
        with _timed("seg_plan", n * 4.0):
            if sorted_lists > 0:
                if n % sorted_lists:
                    raise ValueError("sorted_lists must divide the number of keys")
                check(lib.mapx_seg_plan_merge(ptr(keys_i32), sorted_lists, n // sorted_lists, ptr(ws), ws.numel(),
                                              ptr(self.sorted_keys), ptr(self.perm), ptr(self.rank), ptr(self.uniq),
                                              ptr(self.seg_start), ptr(self.n_uniq), stream()))
            else:
                check(lib.mapx_seg_plan(ptr(keys_i32), n, V, ptr(ws), ws.numel(), ptr(self.sorted_keys),
                                        ptr(self.perm), ptr(self.rank), ptr(self.uniq), ptr(self.seg_start),
                                        ptr(self.n_uniq), stream()))

    @staticmethod
    def build_many(key_lists, Vs):
        """The plans of several key lists (the step's tables) from ONE chain of launches
        (mapx_seg_plan_multi: 8 launches for two 24-bit lists instead of 8 each) -> [SegPlan]."""
        import ctypes as C
        plans = [SegPlan(k, V, launch=False) for k, V in zip(key_lists, Vs)]
        cnt = len(plans)
        I64, PP = C.c_int64 * cnt, C.c_void_p * cnt
        n_arr, v_arr = I64(*[p.n for p in plans]), I64(*[int(v) for v in Vs])
        dev = key_lists[0].device
        ws = scratch(lib.mapx_seg_plan_multi_workspace_bytes(cnt, n_arr, v_arr), dev)
        arr = lambda ts: PP(*[t.data_ptr() for t in ts])
        with _timed("seg_plan", sum(p.n for p in plans) * 4.0):
            check(lib.mapx_seg_plan_multi(cnt, arr(key_lists), n_arr, v_arr, ptr(ws), ws.numel(),
                                          arr([p.sorted_keys for p in plans]), arr([p.perm for p in plans]),
                                          arr([p.rank for p in plans]), arr([p.uniq for p in plans]),
                                          arr([p.seg_start for p in plans]), arr([p.n_uniq for p in plans]),
                                          stream()))
        return plans

    def tensors(self):
        return (self.sorted_keys, self.perm, self.rank, self.uniq, self.seg_start, self.n_uniq)

    def count(self):
        """Number of unique keys (host sync)."""
        return int(self.n_uniq[0].item())

    def take_counter(self):
        """Address of the plan's zeroed owner counter for its first segment reduction, None after."""
        if not self._counter_fresh:
            return None
        self._counter_fresh = False
        return self.n_uniq.data_ptr() + 4


def seg_reduce_rows(plan, src, W, src2=None):
    """out[u,:] = sum of src rows whose key is plan.uniq[u]; out has capacity plan.n rows.
    `src2`: a second tensor like src, added to it element by element inside the kernel (the two towers'
    dL/dX0 of DCNv2: no elementwise launch in front of the reduction)."""
    require_gpu(src)
    if src2 is not None:
        require_gpu(src2)
        if src2.dtype != src.dtype or src2.shape != src.shape or not src2.is_contiguous():
            raise ValueError("seg_reduce_rows: src2 must match src (dtype, shape, contiguous)")
    out = torch.empty(max(plan.n, 1), W, dtype=torch.float32, device=src.device)
    nb = lib.mapx_seg_reduce_workspace_bytes(plan.n, W)
    ws = scratch(nb, src.device)
    fn = lib.mapx_seg_reduce_rows_bf16 if is_bf16(src) else lib.mapx_seg_reduce_rows
    nsrc = 2 if src2 is not None else 1
    with _timed("seg_reduce_rows", plan.n * (float(src.element_size()) * W * nsrc + 8)):
        check(fn(plan.n, ptr(plan.perm), ptr(plan.rank), ptr(plan.seg_start),
                 ptr(src), ptr(src2), W, ptr(out), ptr(ws), ws.numel(), plan.take_counter(), stream()))
    return out


def seg_reduce_rows_extra(plan, src, W, extra, group, extra_stride=1):
    """-> (rows [cap,W], scalars [cap]): the row reduction of seg_reduce_rows over the first W columns
    of src plus, per unique key, the sum of extra[(position // group) * extra_stride] (DeepFM's LR
    weight gradient rides with the embedding's; DP merge of rows that carry a scalar column).
    bf16 src (bf16 compute mode): fp32 sums and outputs, `extra` stays fp32."""
    require_gpu(src, extra)
    if extra.dtype != torch.float32:
        raise TypeError("seg_reduce_rows_extra: the extra scalars are fp32")
    out = torch.empty(max(plan.n, 1), W, dtype=torch.float32, device=src.device)
    out1 = torch.empty(max(plan.n, 1), dtype=torch.float32, device=src.device)
    ws = scratch(lib.mapx_seg_reduce_workspace_bytes(plan.n, W), src.device)
    fn = lib.mapx_seg_reduce_rows_extra_bf16 if is_bf16(src) else lib.mapx_seg_reduce_rows_extra
    with _timed("seg_reduce_rows", plan.n * (float(src.element_size()) * W + 12)):
        check(fn(plan.n, ptr(plan.perm), ptr(plan.rank), ptr(plan.seg_start),
                 src.data_ptr(), W, src.stride(0), extra.data_ptr(), group,
                 extra_stride, ptr(out), ptr(out1), ptr(ws), ws.numel(),
                 plan.take_counter(), stream()))
    return out, out1


def pack_sparse(plan, rows0, rows1, maxc, scale, pad_id=0):
    """The first n_uniq (id, row) pairs of a sparse gradient as a message of exactly `maxc` entries
    (mapx/parallel.py): -> (keys int32 [maxc], rows f32 [maxc, W0 (+4 with rows1)])."""
    require_gpu(rows0)
    W0 = rows0.shape[1]
    Wp = W0 + 4 if rows1 is not None else W0
    keys = torch.empty(maxc, dtype=torch.int32, device=rows0.device)
    rows = torch.empty(maxc, Wp, dtype=torch.float32, device=rows0.device)
    check(lib.mapx_pack_sparse(ptr(plan.uniq), ptr(rows0), W0, ptr(rows1), ptr(plan.n_uniq),
                               min(plan.uniq.shape[0], rows0.shape[0]), maxc, float(scale), pad_id, ptr(keys),
                               ptr(rows), stream()))
    return keys, rows


class HostMailbox:
    """`n` int32 words of fine-grained pinned host memory that a kernel can store into and the host
    can poll while the stream is still running (mapx_host_alloc_coherent): `.np` is the numpy
    view, `.address(i)` the address of word i for the kernel."""

    def __init__(self, n):
        import ctypes
        import numpy as np
        p = ctypes.c_void_p()
        check(lib.mapx_host_alloc_coherent(4 * n, ctypes.byref(p)))
        self._p, self.n = p.value, n
        self.np = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(p.value))

    def address(self, i=0):
        return self._p + 4 * i

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p and lib is not None:
            self.np = None
            lib.mapx_host_free(p)


def publish_i32(src, n, stamp_dev, mailbox, at=0):
    """++stamp; mailbox[at : at+n] = src[:n] (int32, device); mailbox[at+n] = stamp;
    mailbox[at+n+1] = checksum.  A kernel that stores straight into coherent host memory: usable
    from inside a captured graph, readable by the host before the graph ends (mapx_publish_i32)."""
    require_gpu(src, stamp_dev)
    if src.dtype != torch.int32 or stamp_dev.dtype != torch.int32:
        raise ValueError("publish_i32 moves int32 values")
    if at < 0 or at + n + 2 > mailbox.n:
        raise ValueError("publish_i32 needs n + 2 words of mailbox")
    check(lib.mapx_publish_i32(ptr(src), n, ptr(stamp_dev), mailbox.address(at), stream()))


# --------------------------------------------------------------------------- xDeepFM: CIN pieces
def transpose_batched(x):
    """[B,R,C] -> [B,C,R] (contiguous)."""
    require_gpu(x)
    x = x.contiguous()
    B, R, C = x.shape
    out = torch.empty(B, C, R, dtype=torch.float32, device=x.device)
    check(lib.mapx_transpose_batched(ptr(x), B, R, C, ptr(out), stream()))
    return out


def cin_outer_fwd(x0t, xi, pad_to=1):
    """had[r, h*H+m] = x0t[r,h] * xi[r,m]: x0t [R,F], xi [R,H] -> [R, F*H]  (layers.py:714-715); pad_to = 8: the row
    is padded with zero columns to a multiple of 8 floats (-> [R, ceil8(F*H)], the GEMM's vectorised operand path)."""
    require_gpu(x0t, xi)
    R, F = x0t.shape
    H = xi.shape[1]
    ld = (F * H + pad_to - 1) // pad_to * pad_to
    had = torch.empty(R, ld, dtype=torch.float32, device=x0t.device)
    check(lib.mapx_cin_outer_fwd(ptr(x0t), F, ptr(xi), H, R, ptr(had), ld, stream()))
    return had


def cin_outer_bwd(dhad, x0t, xi, dx0t, accumulate_x0):
    """-> dxi [R,H]; dx0t [R,F] is written or accumulated in place."""
    require_gpu(dhad, x0t, xi, dx0t)
    R, F = x0t.shape
    H = xi.shape[1]
    dxi = torch.empty(R, H, dtype=torch.float32, device=x0t.device)
    if dhad.stride(1) != 1 or dhad.shape[1] < F * H:
        raise ValueError("cin_outer_bwd: dhad [R, >= F*H] with unit column stride")
    check(lib.mapx_cin_outer_bwd(ptr(dhad), dhad.stride(0), ptr(x0t), F, ptr(xi), H, R, ptr(dx0t), int(accumulate_x0),
                                 ptr(dxi), stream()))
    return dxi


def cin_pool_fwd(xt, B, E, out):
    """out[b, :H] = sum_d xt[(b,d), :]: xt [B*E, H]; `out` may be a column slice (row stride ld)."""
    require_gpu(xt, out)
    H = xt.shape[1]
    check(lib.mapx_cin_pool_fwd(ptr(xt), B, E, H, out.data_ptr(), out.stride(0), stream()))
    return out


def cin_pool_bwd(g, B, E, dxt, accumulate):
    """dxt[(b,d), :] (+)= g[b, :H]; `g` may be a column slice."""
    require_gpu(g, dxt)
    H = dxt.shape[1]
    check(lib.mapx_cin_pool_bwd(g.data_ptr(), g.stride(0), B, E, H, ptr(dxt), int(accumulate), stream()))
    return dxt


# --------------------------------------------------------------------------- xDeepFM in bf16 mode: fused CIN
# csrc/cin_fused.hip.  Activations are bf16 [R, ld] tensors whose row pitch ld = pad8(width) is a multiple of 8 elements
# (pad columns zero); the logical width travels beside them.
CIN_MAX_FIELDS, CIN_MAX_UNITS = 64, 128
CIN_DW_SLAB_ROWS = lib.mapx_cin_fused_dw_slab_rows()


def pad8(n):
    return (int(n) + 7) // 8 * 8


def _cin_bf16(*tensors):
    require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != BF16:
            raise TypeError("fused CIN kernels take bf16 activations and the weight's bf16 operand")


def cin_transpose_bf16(x3):
    """bf16 [B,F,E] -> x0t [B*E, pad8(F)]."""
    _cin_bf16(x3)
    x3 = x3.contiguous()
    B, F, E = x3.shape
    out = torch.empty(B * E, pad8(F), dtype=BF16, device=x3.device)
    check(lib.mapx_cin_transpose_bf16(ptr(x3), B, F, E, ptr(out), out.shape[1], stream()))
    return out


def cin_dx3_bf16(dx0t, B, E, F):
    """fp32 dx0t [B*E, F] -> bf16 dx3 [B,F,E] (one rounding)."""
    require_gpu(dx0t)
    if dx0t.dtype != torch.float32 or dx0t.shape != (B * E, F):
        raise TypeError("cin_dx3_bf16: dx0t is fp32 [B*E, F]")
    out = torch.empty(B, F, E, dtype=BF16, device=dx0t.device)
    check(lib.mapx_cin_dx3_bf16(ptr(dx0t), B, E, F, ptr(out), stream()))
    return out


def cin_fused_fwd(x0t, F, xi, H, w, bias):
    """-> y bf16 [R, pad8(U)]: y[r, o] = bias[o] + sum_{h,m} w[o, h*H+m] * bf16(x0t[r,h] * xi[r,m]); w bf16 [U, F*H(, 1)]."""
    _cin_bf16(x0t, xi, w)
    require_gpu(bias)
    U, R = w.shape[0], x0t.shape[0]
    if w.numel() != U * F * H or xi.shape[0] != R or bias.dtype != torch.float32 or bias.numel() != U:
        raise ValueError("cin_fused_fwd: w [U, F*H], bias fp32 [U], xi [R, pad8(H)]")
    y = torch.empty(R, pad8(U), dtype=BF16, device=x0t.device)
    with _timed("cin_fused_fwd", 2.0 * R * (x0t.shape[1] + xi.shape[1] + y.shape[1])):
        check(lib.mapx_cin_fused_fwd(ptr(x0t), x0t.shape[1], F, ptr(xi), xi.shape[1], H, ptr(w), ptr(bias), U, R, ptr(y),
                                     y.shape[1], stream()))
    return y


def cin_fused_bwd_input(dy, U, w, x0t, F, xi, H, dx0t, accumulate_x0, first_layer=False, gpool=None, E=1):
    """dx0t (fp32 [R,F]) is written or accumulated in place; -> dy_prev bf16 [R, pad8(H)] = bf16(dxi + gpool[r // E])
    (`gpool`: bf16 [B, H] column slice or None), or None for layer 1 (whose dxi joins dx0t)."""
    _cin_bf16(dy, w, x0t, xi, gpool)
    require_gpu(dx0t)
    R = x0t.shape[0]
    if dx0t.dtype != torch.float32 or dx0t.shape != (R, F) or w.numel() != U * F * H or dy.shape[0] != R:
        raise ValueError("cin_fused_bwd_input: dx0t fp32 [R, F], w [U, F*H], dy [R, pad8(U)]")
    if gpool is not None and (gpool.stride(1) != 1 or gpool.shape != (R // E, H)):
        raise ValueError("cin_fused_bwd_input: gpool [R / E, H] with unit column stride")
    prev = None if first_layer else torch.empty(R, pad8(H), dtype=BF16, device=x0t.device)
    with _timed("cin_fused_bwd_input", 2.0 * R * (dy.shape[1] + x0t.shape[1] + 2 * xi.shape[1]) + 8.0 * R * F):
        check(lib.mapx_cin_fused_bwd_input(ptr(dy), dy.shape[1], U, ptr(w), ptr(x0t), x0t.shape[1], F, ptr(xi),
                                           xi.shape[1], H, R, ptr(dx0t), int(accumulate_x0), int(first_layer),
                                           None if gpool is None else gpool.data_ptr(),
                                           0 if gpool is None else gpool.stride(0), E, ptr(prev),
                                           0 if prev is None else prev.shape[1], stream()))
    return prev


def cin_fused_bwd_weight(dy, U, x0t, F, xi, H, out=None):
    """-> dw fp32 [U, F*H] = sum_r dy[r, :U]^T bf16(x0t[r,h] * xi[r,m]) (into `out`, any shape of U*F*H contiguous
    floats: the optimizer's gradient slot); slab partials added in slab order."""
    _cin_bf16(dy, x0t, xi)
    R = x0t.shape[0]
    dw = out if out is not None else torch.empty(U, F * H, dtype=torch.float32, device=dy.device)
    if dw.dtype != torch.float32 or dw.numel() != U * F * H or dy.shape[0] != R or xi.shape[0] != R:
        raise ValueError("cin_fused_bwd_weight: dw fp32 with U*F*H elements, dy / xi with R rows")
    require_gpu(dw)
    nb = lib.mapx_cin_fused_bwd_weight_workspace_bytes(F, H, U, R)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dy.device)
    with _timed("cin_fused_bwd_weight", 2.0 * R * (dy.shape[1] + x0t.shape[1] + xi.shape[1]) + 2.0 * nb):
        check(lib.mapx_cin_fused_bwd_weight(ptr(dy), dy.shape[1], U, ptr(x0t), x0t.shape[1], F, ptr(xi), xi.shape[1], H,
                                            R, ptr(ws), ws.numel(), ptr(dw), stream()))
    return dw


def cin_pool_fwd_bf16(y, U, B, E, out):
    """out[b, :U] = bf16(sum_d y[(b,d), :U]) (fp32 sum); `out`: a bf16 column slice."""
    _cin_bf16(y, out)
    if out.stride(1) != 1 or out.shape != (B, U) or y.shape[0] != B * E:
        raise ValueError("cin_pool_fwd_bf16: out [B, U] with unit column stride, y [B*E, pad8(U)]")
    check(lib.mapx_cin_pool_fwd_bf16(ptr(y), y.shape[1], B, E, U, out.data_ptr(), out.stride(0), stream()))
    return out


def cin_pool_bwd_bf16(g, B, E):
    """g bf16 [B, U] (column slice) -> dy [B*E, pad8(U)]: every row of a sample gets its pooled gradient."""
    _cin_bf16(g)
    U = g.shape[1]
    if g.stride(1) != 1 or g.shape[0] != B:
        raise ValueError("cin_pool_bwd_bf16: g [B, U] with unit column stride")
    dy = torch.empty(B * E, pad8(U), dtype=BF16, device=g.device)
    check(lib.mapx_cin_pool_bwd_bf16(g.data_ptr(), g.stride(0), B, E, U, ptr(dy), dy.shape[1], stream()))
    return dy


# --------------------------------------------------------------------------- DeepFM terms
def lr_sum(ids, w, validate=False):
    """out[b] = sum_f w[ids[b,f]]   (reference models.py:137-140, before the bias)."""
    require_gpu(ids, w)
    ids = ids.contiguous()
    B, F = ids.shape
    out = torch.empty(B, dtype=torch.float32, device=ids.device)
    err = _err_flag(ids.device) if validate else None
    check(lib.mapx_lr_sum_fwd(ptr(ids), B, F, ptr(w), w.numel(), ptr(out), ptr(err), stream()))
    if validate and int(err):
        raise IndexError("index out of range in self")
    return out


def fm_fwd(x3):
    """x3 [B,F,E] (fp32 or bf16) -> (fm [B], s [B,E] = sum over fields, kept for backward), both fp32
    (layers.py:123-131)."""
    require_gpu(x3)
    x3 = x3.contiguous()
    B, F, E = x3.shape
    out = torch.empty(B, dtype=torch.float32, device=x3.device)
    s = torch.empty(B, E, dtype=torch.float32, device=x3.device)
    fn = lib.mapx_fm_fwd_bf16 if is_bf16(x3) else lib.mapx_fm_fwd
    check(fn(ptr(x3), B, F, E, ptr(out), ptr(s), stream()))
    return out, s


def fm_bwd(g, s, x3):
    """g [B] fp32, s [B,E] fp32, x3 [B,F,E] -> dx of x3's dtype (bf16: rounded once)."""
    require_gpu(g, s, x3)
    B, F, E = x3.shape
    dx = torch.empty_like(x3)
    fn = lib.mapx_fm_bwd_bf16 if is_bf16(x3) else lib.mapx_fm_bwd
    check(fn(ptr(_f32(g, "fm_bwd: g").contiguous()), ptr(s), ptr(x3), B, F, E, ptr(dx), stream()))
    return dx


# --------------------------------------------------------------------------- AutoInt attention core
def _f32(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what} is fp32, got {t.dtype}")
    return t


def _one_dtype(what, names, *ts, contiguous=False):
    """True: the bf16 I/O forms (every tensor bf16); False: the fp32 entries.  Mixed element types are an error, and
    with `contiguous` so is a tensor that is not contiguous."""
    half = is_bf16(ts[0])
    for t in ts:
        if t.dtype != (BF16 if half else torch.float32):
            raise TypeError(f"{what}: {names} have one element type, fp32 or bf16 (got {[str(x.dtype) for x in ts]})")
        if contiguous and not t.is_contiguous():
            raise TypeError(f"{what}: {names} are contiguous tensors")
    return half


def _attn_fwd(entries, what, q, k, v, G, F, A, scaled, *drop):
    """attn_fwd (no `drop`) and attn_drop_fwd (drop = p, seed, offset_p, offset_o, offset_dev) on `entries` = their
    (fp32, bf16) C entries."""
    require_gpu(q, k, v)
    fn = entries[_one_dtype(what, "q, k, v", q, k, v, contiguous=True)]
    o = torch.empty_like(q)
    probs = torch.empty(G, F, F, dtype=torch.float32, device=q.device)
    check(fn(ptr(q), ptr(k), ptr(v), G, F, A, int(bool(scaled)), *_attn_drop_args(*drop), ptr(o), ptr(probs), stream()))
    return o, probs


def _attn_bwd(entries, what, q, k, v, probs, d_o, G, F, A, scaled, *drop):
    require_gpu(q, k, v, probs, d_o)
    d_o = d_o.contiguous()
    fn = entries[_one_dtype(what, "q, k, v and d_o", q, k, v, d_o, contiguous=True)]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(fn(ptr(q), ptr(k), ptr(v), ptr(_f32(probs, f"{what}: probs")), ptr(d_o), G, F, A, int(bool(scaled)),
             *_attn_drop_args(*drop), ptr(dq), ptr(dk), ptr(dv), stream()))
    return dq, dk, dv


def _attn_drop_args(p=None, seed=0, offset_p=0, offset_o=0, offset_dev=None):
    return () if p is None else (float(p), int(seed), int(offset_p), int(offset_o), ptr(offset_dev))


def attn_fwd(q, k, v, G, F, A, scaled):
    """q, k, v: G*F*A elements each, fp32 or bf16 (G = B*heads groups of [F, A]) -> (o same size and dtype,
    p [G,F,F] fp32)."""
    return _attn_fwd((lib.mapx_attn_fwd, lib.mapx_attn_fwd_bf16), "attn_fwd", q, k, v, G, F, A, scaled)


def attn_bwd(q, k, v, p, d_o, G, F, A, scaled):
    return _attn_bwd((lib.mapx_attn_bwd, lib.mapx_attn_bwd_bf16), "attn_bwd", q, k, v, p, d_o, G, F, A, scaled)


def attn_drop_fwd(q, k, v, G, F, A, scaled, p, seed, offset_p, offset_o, offset_dev=None):
    """attn_fwd with the layer's two dropouts inside the kernel: O = ((P * m_p / (1-p)) V) * m_o / (1-p) with
    (m_p, m_o) = attn_dropout_masks(G, F, A, p, seed, offset_p, offset_o, offset_dev) -> (o, p undropped)."""
    return _attn_fwd((lib.mapx_attn_drop_fwd, lib.mapx_attn_drop_fwd_bf16), "attn_drop_fwd", q, k, v, G, F, A, scaled,
                     p, seed, offset_p, offset_o, offset_dev)


def attn_drop_bwd(q, k, v, probs, d_o, G, F, A, scaled, p, seed, offset_p, offset_o, offset_dev=None):
    """-> (dq, dk, dv); both masks are regenerated from (seed, offsets)."""
    return _attn_bwd((lib.mapx_attn_drop_bwd, lib.mapx_attn_drop_bwd_bf16), "attn_drop_bwd", q, k, v, probs, d_o, G, F,
                     A, scaled, p, seed, offset_p, offset_o, offset_dev)


def attn_dropout_masks(G, F, A, p, seed, offset_p, offset_o, offset_dev=None, device="cuda"):
    """The keep masks (uint8, 1 = kept) that attn_drop_fwd / attn_drop_bwd draw for these arguments:
    (keep_p [G,F,F] on the probabilities, keep_o [G,F,A] on the output)."""
    keep_p = torch.empty(G, F, F, dtype=torch.uint8, device=device)
    keep_o = torch.empty(G, F, A, dtype=torch.uint8, device=device)
    check(lib.mapx_attn_dropout_masks(G, F, A, float(p), int(seed), int(offset_p), int(offset_o), ptr(offset_dev),
                                      ptr(keep_p), ptr(keep_o), stream()))
    return keep_p, keep_o


# --------------------------------------------------------------------------- Transformer attention core
def mha_fwd(qkv, B, F, E, H, p=0.0, seed=0, offset=0, offset_dev=None):
    """qkv [B*F, 3E] (the in-projection's output, read in place) -> (o [B*F, E] heads concatenated,
    probs [B*H, F, F] undropped).  p > 0: O = (P * m / (1-p)) V with m = mha_dropout_mask(B, F, H, p, seed, offset)."""
    require_gpu(qkv)
    fn = lib.mapx_mha_fwd_bf16 if _one_dtype("mha_fwd", "qkv", qkv) else lib.mapx_mha_fwd
    o = torch.empty(B * F, E, dtype=qkv.dtype, device=qkv.device)
    probs = torch.empty(B * H, F, F, dtype=torch.float32, device=qkv.device)
    check(fn(ptr(qkv), B, F, E, H, float(p), int(seed), int(offset), ptr(offset_dev), ptr(o), ptr(probs), stream()))
    return o, probs


def mha_bwd(qkv, probs, d_o, B, F, E, H, p=0.0, seed=0, offset=0, offset_dev=None):
    """-> d_qkv [B*F, 3E] (dQ, dK, dV in qkv's layout); the dropout mask is regenerated from (seed, offset)."""
    require_gpu(qkv, probs, d_o)
    d_o = d_o.contiguous()
    fn = lib.mapx_mha_bwd_bf16 if _one_dtype("mha_bwd", "qkv and d_o", qkv, d_o) else lib.mapx_mha_bwd
    d_qkv = torch.empty_like(qkv)
    check(fn(ptr(qkv), ptr(_f32(probs, "mha_bwd: probs")), ptr(d_o), B, F, E, H, float(p), int(seed), int(offset),
             ptr(offset_dev), ptr(d_qkv), stream()))
    return d_qkv


def mha_dropout_mask(B, F, H, p, seed, offset, offset_dev=None, device="cuda"):
    """The keep mask (uint8 [B*H, F, F], 1 = kept) that mha_fwd / mha_bwd draw for these arguments."""
    keep = torch.empty(B * H, F, F, dtype=torch.uint8, device=device)
    check(lib.mapx_mha_dropout_mask(B, F, H, float(p), int(seed), int(offset), ptr(offset_dev), ptr(keep), stream()))
    return keep


POOL_MODES = {"sum": 0, "mean": 1, "attn": 2}


def field_pool_fwd(x3, mode, scores=None):
    """x3 [B,F,E] -> (out [B,E], weights [B,F] | None): sum / mean over fields, or ("attn") weighted by
    softmax_f(scores [B,F])."""
    require_gpu(x3, scores)
    x3 = x3.contiguous()
    B, F, E = x3.shape
    m = POOL_MODES[mode]
    fn = lib.mapx_field_pool_fwd_bf16 if _one_dtype("field_pool_fwd", "x", x3) else lib.mapx_field_pool_fwd
    if scores is not None:
        scores = _f32(scores, "field_pool_fwd: scores").contiguous()
    out = torch.empty(B, E, dtype=x3.dtype, device=x3.device)
    w = torch.empty(B, F, dtype=torch.float32, device=x3.device) if m == 2 else None
    check(fn(ptr(x3), ptr(scores), B, F, E, m, ptr(out), ptr(w), stream()))
    return out, w


def field_pool_bwd(g, x3, mode, weights=None):
    """-> (dx [B,F,E], d_scores [B,F] | None)."""
    require_gpu(g, x3)
    B, F, E = x3.shape
    m = POOL_MODES[mode]
    fn = lib.mapx_field_pool_bwd_bf16 if _one_dtype("field_pool_bwd", "g and x", g, x3) else lib.mapx_field_pool_bwd
    dx = torch.empty(B, F, E, dtype=x3.dtype, device=g.device)
    ds = torch.empty(B, F, dtype=torch.float32, device=g.device) if m == 2 else None
    check(fn(ptr(g.contiguous()), ptr(x3.contiguous()), ptr(weights), B, F, E, m, ptr(dx), ptr(ds), stream()))
    return dx, ds


# --------------------------------------------------------------------------- FGCNN (csrc/fgcnn.hip)
FGCNN_ACTS = {"tanh": 0, "relu": 1}
BN_EPS, BN_MOMENTUM = 1e-5, 0.1          # nn.BatchNorm2d's defaults, which the reference's FGCNNBlock takes


def _f32c(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("fgcnn kernels take contiguous fp32 tensors")


def _fg_half(what, names, *ts):
    """The activations of an fgcnn kernel: contiguous, all fp32 (False) or all bf16 (True: the `_bf16` entries, whose
    parameters, statistics and parameter gradients stay fp32)."""
    return _one_dtype(what, names, *ts, contiguous=True)


def fgcnn_conv_fwd(x, w, bias, stats=True):
    """x [B,Cin,H,E], w [Cout,Cin,kh(,1)], bias [Cout] -> (z [B,Cout,H,E], part [B,Cout,2] fp64 | None): the
    convolution and, with `stats`, the per-sample partial sums of the batch statistics from the same launch."""
    require_gpu(x, w, bias)
    _f32c(w, bias)
    fn = lib.mapx_fgcnn_conv_fwd_bf16 if _fg_half("fgcnn_conv_fwd", "x", x) else lib.mapx_fgcnn_conv_fwd
    B, Cin, H, E = x.shape
    Cout, kh = w.shape[0], w.shape[2]
    if w.shape[1] != Cin or w.numel() != Cout * Cin * kh:
        raise ValueError(f"fgcnn_conv_fwd: weight {tuple(w.shape)} does not fit the input {tuple(x.shape)}")
    z = torch.empty(B, Cout, H, E, dtype=x.dtype, device=x.device)
    part = torch.empty(B, Cout, 2, dtype=torch.float64, device=x.device) if stats else None
    check(fn(ptr(x), ptr(w), ptr(bias), B, Cin, Cout, H, E, kh, ptr(z), ptr(part), stream()))
    return z, part


def fgcnn_bn_stats(part, H, E, running_mean=None, running_var=None, tracked=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """part [B,C,2] -> stats [C,2] = {mean, rstd} of the batch; moves the running statistics (unbiased variance) and
    the int64 batch counter in place, on the device."""
    require_gpu(part, running_mean, running_var, tracked)
    B, C = part.shape[0], part.shape[1]
    if tracked is not None and tracked.dtype != torch.int64:
        raise TypeError("fgcnn_bn_stats: num_batches_tracked is an int64 tensor")
    _f32c(running_mean, running_var)
    stats = torch.empty(C, 2, dtype=torch.float32, device=part.device)
    check(lib.mapx_fgcnn_bn_stats(ptr(part), B, C, H, E, float(eps), float(momentum), ptr(stats), ptr(running_mean),
                                  ptr(running_var), ptr(tracked), stream()))
    return stats


def fgcnn_pool_shape(H, ps):
    """-> (padding, pooled height) of MaxPool2d((ps, 1), padding=(H % ps, 0)) in floor mode."""
    pad = H % ps
    return pad, (H + 2 * pad - ps) // ps + 1


def fgcnn_pool_fwd(z, gamma, beta, ps, act, stats=None, running_mean=None, running_var=None, eps=BN_EPS, save=True):
    """BatchNorm (batch `stats` [C,2], or the running statistics) -> act -> max-pool over ps rows:
    z [B,C,H,E] -> (y [B,C,Hp,E], idx uint8 [B,C,Hp,E] | None)."""
    require_gpu(z, gamma, beta, stats, running_mean, running_var)
    _f32c(gamma, beta, stats, running_mean, running_var)
    fn = lib.mapx_fgcnn_pool_fwd_bf16 if _fg_half("fgcnn_pool_fwd", "z", z) else lib.mapx_fgcnn_pool_fwd
    B, C, H, E = z.shape
    _, Hp = fgcnn_pool_shape(H, ps)
    y = torch.empty(B, C, max(Hp, 0), E, dtype=z.dtype, device=z.device)
    idx = torch.empty(B, C, max(Hp, 0), E, dtype=torch.uint8, device=z.device) if save else None
    check(fn(ptr(z), ptr(stats), ptr(running_mean), ptr(running_var), float(eps), ptr(gamma), ptr(beta), B, C, H, E,
             int(ps), FGCNN_ACTS[act], ptr(y), ptr(idx), stream()))
    return y, idx


def fgcnn_bwd(dy, idx, z, x, w, stats, gamma, beta, ps, act, dw=None, db=None, dgamma=None, dbeta=None, need_dx=True):
    """Backward of pool <- act <- BatchNorm (batch statistics) <- conv: -> (dx | None, dw, db, dgamma, dbeta).
    dw / db / dgamma / dbeta: optional destinations (the optimizer's gradient slots).  dy, z, x (and dx) share one
    element type, fp32 or bf16; g = dL/du between the launches and every parameter gradient are fp32."""
    require_gpu(dy, idx, z, x, w, stats, gamma, beta)
    dy = dy.contiguous()
    _f32c(w, stats, gamma, beta, dw, db, dgamma, dbeta)
    half = _fg_half("fgcnn_bwd", "dy, z and x", dy, z, x)
    pool_bwd = lib.mapx_fgcnn_pool_bwd_bf16 if half else lib.mapx_fgcnn_pool_bwd
    conv_bwd = lib.mapx_fgcnn_conv_bwd_bf16 if half else lib.mapx_fgcnn_conv_bwd
    B, Cin, H, E = x.shape
    Cout, kh = w.shape[0], w.shape[2]
    dev = x.device
    g = torch.empty(z.shape, dtype=torch.float32, device=dev)
    part = torch.empty(B, Cout, 2, dtype=torch.float64, device=dev)
    check(pool_bwd(ptr(dy), ptr(idx), ptr(z), ptr(stats), ptr(gamma), ptr(beta), B, Cout, H, E, int(ps),
                   FGCNN_ACTS[act], ptr(g), ptr(part), stream()))
    bsum = torch.empty(Cout, 2, dtype=torch.float32, device=dev)
    dgamma = torch.empty_like(gamma) if dgamma is None else dgamma
    dbeta = torch.empty_like(beta) if dbeta is None else dbeta
    check(lib.mapx_fgcnn_bn_bwd_sums(ptr(part), B, Cout, H, E, ptr(bsum), ptr(dgamma), ptr(dbeta), stream()))
    G = lib.mapx_fgcnn_conv_bwd_groups(B)
    pw = torch.empty(G, Cout * Cin * kh, dtype=torch.float32, device=dev)
    pb = torch.empty(G, Cout, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if dw is None else dw
    db = torch.empty(Cout, dtype=torch.float32, device=dev) if db is None else db
    check(conv_bwd(ptr(g), ptr(z), ptr(x), ptr(w), ptr(stats), ptr(gamma), ptr(bsum), B, Cin, Cout, H, E, kh, ptr(dx),
                   ptr(pw), ptr(pb), ptr(dw), ptr(db), stream()))
    return dx, dw, db, dgamma, dbeta


def inner_product_fwd(x3):
    """x3 [B,T,E] -> [B, T(T-1)/2]: x_i . x_j over the pairs i < j, row-major (layers.py:132-135)."""
    require_gpu(x3)
    fn = lib.mapx_inner_product_fwd_bf16 if _fg_half("inner_product_fwd", "x", x3) else lib.mapx_inner_product_fwd
    B, T, E = x3.shape
    out = torch.empty(B, T * (T - 1) // 2, dtype=x3.dtype, device=x3.device)
    check(fn(ptr(x3), B, T, E, ptr(out), stream()))
    return out


def inner_product_bwd(g, x3):
    """g [B, T(T-1)/2], x3 [B,T,E] -> dx [B,T,E].  A bf16 g is read in place when its rows are unit-stride (a column
    slice of d(dense_input): odd offset and pitch); an fp32 one is made contiguous first."""
    require_gpu(g, x3)
    B, T, E = x3.shape
    if is_bf16(x3):
        if g.dim() != 2 or g.stride(1) != 1 or (B > 1 and g.stride(0) < g.shape[1]):
            g = g.contiguous()
        _fg_half("inner_product_bwd", "x", x3)
        if g.dtype != BF16 or tuple(g.shape) != (B, T * (T - 1) // 2):
            raise TypeError(f"inner_product_bwd: g is bf16 [B, T(T-1)/2] like x (got {g.dtype} {tuple(g.shape)})")
        dx = torch.empty_like(x3)
        # (the pitch: guard-band cases in tests/test_bf16_fgcnn_extents_gpu.py)
        ldg = g.stride()[0] if B > 1 else g.shape[1]
        check(lib.mapx_inner_product_bwd_bf16(g.data_ptr(), ldg, ptr(x3), B, T, E, ptr(dx), stream()))
        return dx
    g = g.contiguous()
    _f32c(g, x3)
    dx = torch.empty_like(x3)
    check(lib.mapx_inner_product_bwd(ptr(g), ptr(x3), B, T, E, ptr(dx), stream()))
    return dx


# --------------------------------------------------------------------------- FiGNN (csrc/fignn.hip)
FIGNN_MAX_FIELDS, FIGNN_MAX_EMBED = 64, 32          # csrc/fignn.hip kGnMaxF, kGnMaxE
FIGNN_WS_VECS = 8                                   # workspace vectors per (sample, field) row: kWsVecs


def _gn_f32c(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("fignn kernels take contiguous fp32 tensors")


def _gn_layer_weights(F, E, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh):
    want = ((F, E, E), (F, E, E), (E,), (3 * E, E), (3 * E, E), (3 * E,), (3 * E,))
    got = tuple(tuple(t.shape) for t in (w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh))
    if got != want:
        raise ValueError(f"fignn layer: weights {got} do not fit F={F}, E={E} (want {want})")


def fignn_weights_staged(F, E, backward=False):
    """True: the layer kernels keep W_in / W_out in LDS at this shape; False: they stream them through L2."""
    rc = lib.mapx_fignn_weights_staged(int(F), int(E), int(bool(backward)))
    if rc < 0:
        raise ValueError(f"fignn: num_fields={F}, embed_size={E} is outside the kernels' range")
    return bool(rc)


def fignn_graph_fwd(x3, w_attn):
    """x3 [B,F,E], w_attn [1,2E] -> (g [B,F,F], s [B,F], d [B,F]): the attention graph without self-loops."""
    require_gpu(x3, w_attn)
    _gn_f32c(x3, w_attn)
    B, F, E = x3.shape
    if w_attn.numel() != 2 * E:
        raise ValueError(f"fignn_graph_fwd: W_attn {tuple(w_attn.shape)} does not fit embed_size={E}")
    g = torch.empty(B, F, F, dtype=torch.float32, device=x3.device)
    s = torch.empty(B, F, dtype=torch.float32, device=x3.device)
    d = torch.empty(B, F, dtype=torch.float32, device=x3.device)
    check(lib.mapx_fignn_graph_fwd(ptr(x3), ptr(w_attn), B, F, E, ptr(g), ptr(s), ptr(d), stream()))
    return g, s, d


def fignn_graph_bwd(dg, g, s, d, x3, w_attn, dx_base, dx_add=None, dw_attn=None, inplace=False):
    """-> (dx = dx_base (+ dx_add) + the graph's input gradient, dW_attn); `inplace`: dx is written over dx_base."""
    require_gpu(dg, g, s, d, x3, w_attn, dx_base, dx_add, dw_attn)
    _gn_f32c(dg, g, s, d, x3, w_attn, dx_base, dx_add, dw_attn)
    B, F, E = x3.shape
    if tuple(g.shape) != (B, F, F) or dg.shape != g.shape or tuple(s.shape) != (B, F) or d.shape != s.shape \
            or dx_base.shape != x3.shape or (dx_add is not None and dx_add.shape != x3.shape) \
            or w_attn.numel() != 2 * E or (dw_attn is not None and dw_attn.numel() != 2 * E):
        raise ValueError(f"fignn_graph_bwd: operands do not fit x {tuple(x3.shape)}")
    dx = dx_base if inplace else torch.empty_like(x3)
    part = torch.empty(lib.mapx_fignn_graph_bwd_groups(B), 2 * E, dtype=torch.float32, device=x3.device)
    dw_attn = torch.empty_like(w_attn) if dw_attn is None else dw_attn
    check(lib.mapx_fignn_graph_bwd(ptr(dg), ptr(g), ptr(s), ptr(d), ptr(x3), ptr(w_attn), ptr(dx_base), ptr(dx_add), B, F,
                                   E, ptr(dx), ptr(part), ptr(dw_attn), stream()))
    return dx, dw_attn


def fignn_layer_fwd(h, g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, x_res=None):
    """One GraphLayer + GRUCell step (+ x_res): h [B,F,E], g [B,F,F] -> h_next [B,F,E]."""
    require_gpu(h, g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, x_res)
    _gn_f32c(h, g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, x_res)
    B, F, E = h.shape
    _gn_layer_weights(F, E, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh)
    if tuple(g.shape) != (B, F, F) or (x_res is not None and x_res.shape != h.shape):
        raise ValueError(f"fignn_layer_fwd: g {tuple(g.shape)} / x_res do not fit h {tuple(h.shape)}")
    out = torch.empty_like(h)
    check(lib.mapx_fignn_layer_fwd(ptr(h), ptr(g), ptr(x_res), ptr(w_in), ptr(w_out), ptr(bias_p), ptr(w_ih), ptr(w_hh),
                                   ptr(b_ih), ptr(b_hh), B, F, E, ptr(out), stream()))
    return out


def fignn_layer_bwd(dh_next, h, g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, dg, dg_init, dx_acc=None, dx_init=True,
                    grads=None, add_layer=False, add_gru=False, ws=None):
    """Backward of fignn_layer_fwd from dh_next: -> (dh, grads).  dg [B,F,F] and dx_acc [B,F,E] (res_conn) are written
    (`*_init`) or added to; grads = [dW_in, dW_out, dbias_p, dW_ih, dW_hh, db_ih, db_hh] (given: the destinations,
    overwritten or — add_layer for the first three, add_gru for the GRU's four — added to)."""
    weights = (w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh)
    require_gpu(dh_next, h, g, dg, dx_acc, ws, *weights)
    dh_next = dh_next.contiguous()
    _gn_f32c(dh_next, h, g, dg, dx_acc, ws, *weights)
    B, F, E = h.shape
    _gn_layer_weights(F, E, *weights)
    if tuple(g.shape) != (B, F, F) or tuple(dg.shape) != (B, F, F) or dh_next.shape != h.shape \
            or (dx_acc is not None and dx_acc.shape != h.shape):
        raise ValueError(f"fignn_layer_bwd: g / dg / dh_next / dx_acc do not fit h {tuple(h.shape)}")
    dev = h.device
    if grads is None:
        if add_layer or add_gru:
            raise ValueError("fignn_layer_bwd: adding needs the destinations")
        grads = [torch.empty_like(w) for w in weights]
    _gn_f32c(*grads)
    require_gpu(*grads)
    if [tuple(t.shape) for t in grads] != [tuple(w.shape) for w in weights]:
        raise ValueError("fignn_layer_bwd: gradient destinations do not fit the weights")
    if ws is None:
        ws = torch.empty(B, F, FIGNN_WS_VECS, E, dtype=torch.float32, device=dev)
    elif ws.numel() != B * F * FIGNN_WS_VECS * E:
        raise ValueError("fignn_layer_bwd: workspace of the wrong size")
    dh = torch.empty_like(h)
    check(lib.mapx_fignn_layer_bwd(ptr(dh_next), ptr(h), ptr(g), *(ptr(w) for w in weights), B, F, E, ptr(dh), ptr(dg),
                                   int(bool(dg_init)), ptr(dx_acc), int(bool(dx_init)), ptr(ws), stream()))
    pf = torch.empty(lib.mapx_fignn_wgrad_groups(B, F, 0), 2 * F * E * E, dtype=torch.float32, device=dev)
    pg = torch.empty(lib.mapx_fignn_wgrad_groups(B, F, 1), 6 * E * E + 7 * E, dtype=torch.float32, device=dev)
    check(lib.mapx_fignn_layer_wgrad(ptr(ws), ptr(h), B, F, E, ptr(pf), ptr(pg), *(ptr(t) for t in grads),
                                     int(bool(add_layer)), int(bool(add_gru)), stream()))
    return dh, grads


def fignn_pred_fwd(score, z2):
    """score, z2 [B,F] -> logits [B,1] = sum_f sigmoid(z2) score."""
    require_gpu(score, z2)
    _gn_f32c(score, z2)
    B, F = score.shape
    if z2.shape != score.shape:
        raise ValueError("fignn_pred_fwd: score and z2 differ in shape")
    out = torch.empty(B, 1, dtype=torch.float32, device=score.device)
    check(lib.mapx_fignn_pred_fwd(ptr(score), ptr(z2), B, F, ptr(out), stream()))
    return out


def fignn_pred_bwd(g_logits, score, z2):
    require_gpu(g_logits, score, z2)
    g_logits = g_logits.contiguous()
    _gn_f32c(g_logits, score, z2)
    B, F = score.shape
    if g_logits.numel() != B:
        raise ValueError("fignn_pred_bwd: one logit gradient per sample")
    dscore, dz2 = torch.empty_like(score), torch.empty_like(z2)
    check(lib.mapx_fignn_pred_bwd(ptr(g_logits), ptr(score), ptr(z2), B, F, ptr(dscore), ptr(dz2), stream()))
    return dscore, dz2


# --------------------------------------------------------------------------- NCE
def alias_build(probs_cpu):
    """Host Walker table, bit-identical to the reference's (alias_multinomial.py:39-72)."""
    probs_cpu = probs_cpu.detach().to("cpu", torch.float32).contiguous()
    V = probs_cpu.numel()
    prob = torch.empty(V, dtype=torch.float32)
    alias = torch.empty(V, dtype=torch.int64)
    check(lib.mapx_alias_build_host(probs_cpu.data_ptr(), V, prob.data_ptr(), alias.data_ptr()))
    return prob, alias


def alias_pack(prob, alias):
    require_gpu(prob, alias)
    packed = torch.empty(prob.numel(), 2, dtype=torch.int32, device=prob.device)
    check(lib.mapx_alias_pack(ptr(prob), ptr(alias), prob.numel(), ptr(packed), stream()))
    return packed


def alias_draw(packed, targets, K, seed, offset, offset_dev=None):
    """-> idx int32 [T, K+1]; column 0 = targets.  offset_dev: int32 device scalar added to
    `offset` inside the kernel (hipGraph-replay safe)."""
    require_gpu(packed, targets)
    targets = targets.contiguous()
    T = targets.numel()
    idx = torch.empty(T, K + 1, dtype=torch.int32, device=targets.device)
    check(lib.mapx_alias_draw(ptr(packed), packed.shape[0], ptr(targets), T, K, seed, offset,
                              ptr(offset_dev), ptr(idx), stream()))
    return idx


def nce_pack_idx(targets, noise, V, validate=False):
    require_gpu(targets, noise)
    targets, noise = targets.contiguous(), noise.contiguous()
    T, K = targets.numel(), noise.shape[-1]
    idx = torch.empty(T, K + 1, dtype=torch.int32, device=targets.device)
    err = _err_flag(targets.device) if validate else None
    check(lib.mapx_nce_pack_idx(ptr(targets), ptr(noise), T, K, V, ptr(idx), ptr(err), stream()))
    if validate and int(err.item()):
        raise IndexError("index out of range in self")
    return idx


def lazy_rows_supported(P, K1):
    """mapx_nce_fwd reads rows through their pending updates (lazy=) for this proj_size / sample count."""
    return P == 32 and K1 <= 32


def nce_fwd(enc, masked_index, idx, emb, bias, logq, F, P, want_logits=False, hpos=None, dh_slots=None,
            totals_later=False, lazy=None):
    """-> dict(loss [2] = {mean loss, accuracy}, acc [1] i32, h [T,P], dlogit [T,K+1], dh [T,P], logits or None).
    hpos (grouped encoder): `enc` is h_slots [slots,P]; dh_slots receives dh at the slots too.
    lazy (a native.LazyRows: optim.TableAdam.lazy_rows()): emb / bias rows are read through their pending
    zero-gradient updates — no catch-up pass ran before this call.
    totals_later: loss / acc are left UNWRITTEN and out["totals"] = (partials buffer, count, loss, acc) goes to the
    nce_scatter_dh that must follow (the head's backward inside a training step)."""
    require_gpu(enc, masked_index, idx, emb, bias, logq)
    B, L = masked_index.shape
    T, K1 = idx.shape
    assert T == B * L and (hpos is not None or enc.shape == (B, F * P))
    dev = enc.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(loss=torch.empty(2, **f32), acc=torch.empty(1, dtype=torch.int32, device=dev),
               h=torch.empty(T, P, **f32), dlogit=torch.empty(T, K1, **f32),
               dh=torch.empty(T, P, **f32),
               logits=torch.empty(T, K1, **f32) if want_logits else None)
    nws = lib.mapx_nce_fwd_workspace_bytes()
    # (partials that outlive this call get a buffer of their own, not the stream's shared scratch)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if totals_later else scratch(nws, dev)
    left = native_int() if totals_later else None
    rec = amax_record(dev) if (dh_slots is not None and P == 32 and K1 <= 32) else None     # (the p32 kernel writes it)
    # algorithmic bytes: per (target, sample) one table row + bias + log q + id
    with _timed("nce_fwd", T * K1 * (4.0 * P + 8 + 4)):
        check(lib.mapx_nce_fwd(ptr(enc), B, L, F, P, ptr(masked_index.contiguous()), ptr(idx), K1 - 1,
                               ptr(emb), ptr(bias), ptr(logq), emb.shape[0], ptr(out["h"]),
                               ptr(out["dlogit"]), ptr(out["dh"]), ptr(out["logits"]), ptr(out["loss"]),
                               ptr(out["acc"]), ptr(ws), ws.numel(), ptr(hpos), ptr(dh_slots),
                               None if left is None else native_byref(left), ptr(rec),
                               None if lazy is None else native_byref(lazy), stream()))
    tag(dh_slots, rec)
    tag(out["dh"], rec)
    out["totals"] = (ws, left.value, out["loss"], out["acc"]) if (left is not None and left.value > 0) else None
    return out


class EncGroups:
    """Padded by-field slot layout of the B*L targets (csrc/gemm.hip: grouped feat_encoder)."""

    def __init__(self, masked_index, F):
        require_gpu(masked_index)
        B, L = masked_index.shape
        T, dev = B * L, masked_index.device
        self.T, self.L, self.F = T, L, F
        # >= T + 127 F (every group padded to 128); whole rounds of 8 tiles, one per XCD (enc_grouped_fwd's order)
        self.cap = (T + 127 * F + 1023) // 1024 * 1024
        masked_index = masked_index.contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        self.rowmap = torch.empty(self.cap, **i32)
        self.hpos = torch.empty(T, **i32)
        self.tile_group = torch.empty(self.cap // 128, **i32)
        self.group_start = torch.empty(F + 1, **i32)
        check(lib.mapx_enc_group_layout(ptr(masked_index), T, L, F, self.cap, ptr(self.rowmap), ptr(self.hpos),
                                        ptr(self.tile_group), ptr(self.group_start), stream()))


def _enc_groups_tensors(self):
    return (self.rowmap, self.hpos, self.tile_group, self.group_start)


EncGroups.tensors = _enc_groups_tensors


def enc_grouped_fwd(final, w, b, groups, zero_slots=None):
    """h_slots [cap, 32]: the masked fields' encoder blocks only (26 % of the dense GEMM).
    zero_slots: a [cap, 32] buffer cleared by the same launch."""
    require_gpu(final, w, b)
    h = torch.empty(groups.cap, 32, dtype=torch.float32, device=final.device)
    ra, rb = amax_of(final), amax_of(w)
    if AUTO_AMAX and H2:
        ra = ra if ra is not None else amax(final)
        rb = rb if rb is not None else amax(w)
    sc = _scale_arg(ra, rb) if (ra is not None and rb is not None) else None
    with _timed("gemm_enc_grouped_fwd", 2.0 * groups.T * 32 * final.shape[1]):
        check(lib.mapx_enc_grouped_fwd(final.data_ptr(), final.stride(0), final.shape[0], final.shape[1],
                                       ptr(w), w.stride(0), ptr(b), ptr(groups.rowmap), ptr(groups.tile_group),
                                       ptr(groups.group_start), groups.F, groups.cap, ptr(h), ptr(zero_slots),
                                       None if sc is None else native_byref(sc), stream()))
    return h


def enc_grouped_dw(dh_slots, final, groups, out=None, gscale=None):
    """dW [F*32, D+H] of feat_encoder from the slot-ordered dh (every row written), times the
    device scalar `gscale` if given."""
    require_gpu(dh_slots, final)
    Nn = final.shape[1]
    if out is None:
        out = torch.empty(groups.F * 32, Nn, dtype=torch.float32, device=final.device)
    ra, rb = amax_of(dh_slots), amax_of(final)
    if AUTO_AMAX and H2:
        ra = ra if ra is not None else amax(dh_slots)
        rb = rb if rb is not None else amax(final)
    sc = _scale_arg(ra, rb) if (ra is not None and rb is not None) else None
    with _timed("gemm_enc_grouped_dw", 2.0 * groups.T * 32 * Nn):
        check(lib.mapx_enc_grouped_dw(ptr(dh_slots), final.data_ptr(), final.stride(0), final.shape[0], Nn,
                                      ptr(groups.rowmap), ptr(groups.group_start), groups.F, ptr(gscale),
                                      ptr(out), out.stride(0), None if sc is None else native_byref(sc), stream()))
    return out


def nce_scatter_dh(dh, masked_index, F, P, gscale=None, totals=None):
    """`totals`: nce_fwd(totals_later=True)'s out["totals"] — this launch then also writes the loss / accuracy."""
    require_gpu(dh, masked_index)
    B, L = masked_index.shape
    denc = torch.empty(B, F * P, dtype=torch.float32, device=dh.device)
    ws, n, loss, acc = totals if totals is not None else (None, 0, None, None)
    rec = amax_record(dh.device)
    check(lib.mapx_nce_scatter_dh(ptr(dh), ptr(masked_index.contiguous()), ptr(gscale), B, L, F, P,
                                  ptr(denc), ptr(ws), n, ptr(loss), ptr(acc), ptr(rec), stream()))
    return tag(denc, rec)


def nce_table_grad(plan, dlogit, h, K, P, gscale=None):
    """-> (emb grad rows [cap,P], bias grad rows [cap]) for plan.uniq; dlogit is multiplied by the
    device scalar `gscale` (incoming gradient of the loss) on the fly."""
    dev = dlogit.device
    out_emb = torch.empty(max(plan.n, 1), P, dtype=torch.float32, device=dev)
    out_bias = torch.empty(max(plan.n, 1), dtype=torch.float32, device=dev)
    nb = lib.mapx_nce_table_grad_workspace_bytes(plan.n, P)
    ws = scratch(nb, dev)
    with _timed("nce_table_grad", plan.n * (4.0 * P + 4)):
        check(lib.mapx_nce_table_grad(plan.n, ptr(plan.perm), ptr(plan.rank), ptr(plan.seg_start),
                                      ptr(dlogit), ptr(h), K, P, ptr(gscale), ptr(out_emb), ptr(out_bias),
                                      ptr(ws), ws.numel(), plan.take_counter(), stream()))
    return out_emb, out_bias


def scale_(x, g):
    check(lib.mapx_scale_inplace(ptr(x), x.numel(), ptr(g), stream()))
    return x


# --------------------------------------------------------------------------- dense
_EPI_RELU_MASK_COLSUM = N.EPI_RELU_MASK_COLSUM      # (gemm_bf16's N is a size)


def gemm_bf16(a, b, a_kc, b_kc, M, N, K, out=None, out_dtype=BF16, ldc=None, epi=N.EPI_NONE, bias=None,
              aux1=None, aux2=None, out2=None, nsplit=1, lda=None, ldb=None, tile=-1):
    """The bf16-operand GEMM (include/mapx_hip.h: mapx_gemm_bf16): a, b, aux2, out2 bf16; C bf16 or
    fp32 (`out_dtype`, or the dtype of `out`); aux1 bf16 or fp32 (EPI_ADD only); fp32 accumulation."""
    require_gpu(a, b)
    if not (is_bf16(a) and is_bf16(b)):
        raise TypeError("gemm_bf16 takes bf16 operands")
    dev = a.device
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=dev)
    c_f32 = out.dtype == torch.float32
    if not (c_f32 or is_bf16(out)):
        raise TypeError("gemm_bf16 writes bf16 or fp32")
    ldc = ldc if ldc is not None else out.stride(0)
    lda = lda if lda is not None else a.stride(0)
    ldb = ldb if ldb is not None else b.stride(0)
    ws, wsn = None, 0
    if nsplit > 1:
        wsn = lib.mapx_gemm_splitk_workspace_bytes(M, N, nsplit)
        ws = scratch(wsn, dev)
        wsn = ws.numel()
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("gemm_bf16: the bias stays fp32")
    aux1_f32 = aux1 is not None and aux1.dtype == torch.float32
    for t_ in (aux2, out2):
        if t_ is not None and not is_bf16(t_) and not (t_ is out2 and epi == _EPI_RELU_MASK_COLSUM):
            raise TypeError("gemm_bf16: aux2 / out2 are bf16 (out2 of EPI_RELU_MASK_COLSUM: fp32 partial rows)")
    kind = "gemm_fwd_nt" if (a_kc and b_kc) else ("gemm_dx_nn" if a_kc else "gemm_dw_tn")
    with _timed(kind, 2.0 * M * N * K):
        check(lib.mapx_gemm_bf16(int(a_kc), int(b_kc), M, N, K, a.data_ptr(), lda, b.data_ptr(), ldb,
                                 out.data_ptr(), ldc, int(c_f32), epi, ptr(bias),
                                 aux1.data_ptr() if aux1 is not None else None,
                                 aux1.stride(0) if aux1 is not None else 0, int(aux1_f32),
                                 aux2.data_ptr() if aux2 is not None else None,
                                 aux2.stride(0) if aux2 is not None else 0,
                                 out2.data_ptr() if out2 is not None else None,
                                 out2.stride(0) if out2 is not None else 0, nsplit, tile,
                                 ws.data_ptr() if ws is not None else None, wsn, stream()))
    return out


# Magnitude records (include/mapx_hip.h: mapx_gemm_scale; csrc/amax.h): every kernel that writes a tensor a GEMM will
# read leaves max |x| in the tensor's 8-byte record; a product whose two operands carry one is formed by the two-piece
# fp16 arithmetic (csrc/gemm_h2.hip), any other by the six-product bf16 one (csrc/gemm_x3.hip).  Here a record travels
# as the attribute `_amax` of the tensor object: outputs of autograd Functions, saved INPUTS and gradients handed from
# one backward node to the next keep their attributes; saved OUTPUTS and slices do not (carry / amax_pack below).
# An attribute also survives what torch does to the tensor in place (autograd sums a fan-out's second gradient into the
# first-arrived one), so tag() notes the tensor's version counter and amax_of() lets go of a record whose tensor has
# been written through torch since (the product then takes the six-product arithmetic); a record of the eager ring
# knows which hand-out it was and is not believed once its slot has gone to another tensor.
H2 = os.environ.get("MAPX_GEMM_H2", "1") == "1"          # A/B switch: 0 = no records anywhere, x3 arithmetic only
_epoch_word = {}
_cap_pool = [None, 0]          # records of the capture in progress: (int32 [2 n] tensor, next free)
_cap_pools = []                # ... of finished captures: a replayed graph has their addresses baked in
_ring, _RING = {}, 1 << 12     # eager records
REC = 128                      # int32 words of a record (MAPX_AMAX_RECORD_BYTES / 4: 64 slots of {bits, epoch})


def _ensure_epoch(device):
    """The process-wide epoch word of the records (mapx_amax_epoch_source): allocated once, never freed."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _epoch_word:
        w = torch.zeros(1, dtype=torch.int32, device=device)
        check(lib.mapx_amax_epoch_source(w.data_ptr()))
        _epoch_word[key] = w
    return _epoch_word[key]


def amax_capture_begin(device, n=1024):
    """Called right before a hipGraph capture: the records handed out during the capture come from one zeroed
    block allocated HERE (a record allocated inside the capture would be a memset node of its own; the epoch tags
    make resets unnecessary)."""
    if H2:
        _ensure_epoch(device)
        _cap_pool[0], _cap_pool[1] = torch.zeros(REC * n, dtype=torch.int32, device=device), 0
        _cap_pools.append(_cap_pool[0])


def amax_capture_end():
    _cap_pool[0] = None


def amax_record(device):
    """A zeroed magnitude record, or None where none can be had (records switched off; inside a capture that
    did not announce itself: the product then simply takes the six-product arithmetic)."""
    if not H2:
        return None
    if torch.cuda.is_current_stream_capturing():
        pool, i = _cap_pool
        if pool is None or REC * (i + 1) > pool.numel():
            return None
        _cap_pool[1] = i + 1
        return pool[REC * i:REC * (i + 1)]
    _ensure_epoch(device)
    # eager launches: a ring of records that is never freed (a record outlives the tensor object it hangs on
    # whenever a side stream still runs the kernel that raises it), each zeroed when it is handed out
    key = device.index if device.index is not None else torch.cuda.current_device()
    ring = _ring.get(key)
    if ring is None:
        ring = _ring[key] = [torch.zeros(REC * _RING, dtype=torch.int32, device=device), 0]
    n = ring[1]                   # hand-outs so far: this one's generation (its slot goes to hand-out n + _RING next)
    ring[1] = n + 1
    i = n % _RING
    rec = ring[0][REC * i:REC * (i + 1)]
    rec.zero_()
    rec._ring, rec._ring_n = ring, n
    return rec


def _recycled(rec):
    """Has the ring slot of record `rec` been handed to another tensor since?"""
    ring = getattr(rec, "_ring", None)
    return ring is not None and ring[1] - rec._ring_n > _RING


def amax_of(t):
    """The record of tensor `t`, or None.  A parameter's record is kept by the optimizer's kernel; when something else
    wrote the parameter through torch (load_state_dict, copy_: its version counter moved) it is recomputed here.
    Any other tensor's record is dropped when the tensor was written through torch after tag() (an in-place add_ of
    autograd's: the record no longer bounds it) or when its ring slot has been handed out again."""
    if not H2 or t is None:
        return None
    rec = getattr(t, "_amax", None)
    if rec is not None:
        ver = getattr(t, "_amax_ver", None)
        if ver is not None:
            if ver != t._version:
                amax(t.detach(), rec=rec, reset=True)
                t._amax_ver = t._version
                refresh_weight_planes(t)
        elif getattr(t, "_amax_at", t._version) != t._version or _recycled(rec):
            t._amax = rec = None
    return rec


def tag(t, rec):
    if rec is not None and t is not None:
        t._amax, t._amax_at = rec, t._version
    return t


def carry(dst, src):
    """`dst` is a slice / view / alias of `src`: the maximum over src bounds the maximum over dst."""
    return tag(dst, amax_of(src))


def flat_rows(x):
    """x.flatten(start_dim=1) with x's record (the flattened embedding rows are the towers' first operand)."""
    return carry(x.flatten(start_dim=1), x)


def cols(t, c0, c1):
    """t[:, c0:c1] with t's record (and, for a weight, the note which columns of which parameter it is)."""
    v = carry(t[:, c0:c1], t)
    if getattr(t, "_planes", None) is not None:
        v._wslice = (t, c0, c1)
    return v


def amax_pack(*ts):
    return tuple(amax_of(t) for t in ts)


def amax_unpack(ts, recs):
    for t, r in zip(ts, recs):
        tag(t, r)


def out_record(out, device):
    """The record a kernel raises for its output: the one the caller put on `out` (several kernels writing
    column ranges of one buffer share the buffer's record), else a fresh one."""
    rec = amax_of(out)
    return rec if rec is not None else amax_record(device)


def amax(x, rec=None, reset=True):
    """The magnitude record of a tensor no mapx kernel produced: one pass over x [rows, cols] (or 1-D)."""
    require_gpu(x)
    if x.dtype != torch.float32:
        raise TypeError("amax: fp32 tensors")
    _ensure_epoch(x.device)
    if rec is None:
        rec = torch.empty(REC, dtype=torch.int32, device=x.device)
        reset = True
    x2 = x if x.dim() == 2 else x.reshape(1, -1)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    check(lib.mapx_amax_f32(x2.data_ptr(), x2.shape[0], x2.shape[1], x2.stride(0), rec.data_ptr(), int(reset), stream()))
    return rec


def amax_value(rec):
    """Host value of a record (tests)."""
    return float(rec[0::2].max().view(1).view(torch.float32).item())      # (bit patterns of values >= 0 order as the values)


# MAPX_AMAX_CHECK=1 (tests): every record a product is given is compared with the operand on the host — a record
# below the operand's true maximum would overflow fp16, one far above it wastes precision.  H2_USED counts the
# products that were handed both records (tests assert that the hot path really takes the new arithmetic).
AMAX_CHECK = os.environ.get("MAPX_AMAX_CHECK", "0") == "1"
# tests: a product whose operand comes without a record gets one computed on the spot (and its weight-like operand B
# its planes), so that every GEMM test also runs through the two-piece fp16 kernels
AUTO_AMAX = os.environ.get("MAPX_AUTO_AMAX", "0") == "1"
H2_USED = [0, 0]               # products with both records / without


def _check_record(x, rec, what):
    if rec is None:
        return
    xs = x.detach().float()
    xs = xs[torch.isfinite(xs)]
    true = float(xs.abs().max()) if xs.numel() else 0.0
    got = amax_value(rec)
    if not (got >= true and (true == 0.0 or got <= true * 64.0 or got < 1e-30)):
        raise AssertionError(f"magnitude record of operand {what}: {got!r} for a tensor whose max |x| is {true!r}")


# Weight planes (include/mapx_hip.h: mapx_h2_weight_planes; csrc/gemm_h2w.hip): a weight that is operand B of large
# products is cut into its two fp16 pieces once per optimizer step instead of once per row tile of every product.  The
# optimizer owns the cache: `p._planes` {(b_kc, c0, c1): planes} on a parameter, filled at first use, refreshed by
# MapxOptimizer right after the AdamW kernel (and by refresh_bf16 after anything else wrote the parameter); each set
# is stamped with the update count it was cut at, and one that a captured step's refresh launch does not know is cut
# again at its next use (PlaneClock below).
H2W = os.environ.get("MAPX_GEMM_H2W", "1") == "1"


def h2_weight_planes(w, b_kc, rec, out=None):
    """The planes of w as operand B (b_kc: B(k,n) = w[n,k], forward; else B(k,n) = w[k,n], input gradient; w may
    be a column slice) at the scale its record `rec` gives now."""
    require_gpu(w)
    Nn, K = (w.shape[0], w.shape[1]) if b_kc else (w.shape[1], w.shape[0])
    if out is None:
        out = torch.empty(lib.mapx_h2_weight_planes_bytes(Nn, K), dtype=torch.uint8, device=w.device)
    check(lib.mapx_h2_weight_planes(w.data_ptr(), w.stride(0), Nn, K, int(b_kc), rec.data_ptr(), out.data_ptr(), stream()))
    return out


def planes_wanted(M, Nn, K):
    """Would gemm_h2w.hip take a product of this shape?  (>= 128 tiles of 128 x 128 — or of 128 x 64 —, K >= 64, K % 8 == 0)"""
    return math.ceil(M / 128) * math.ceil(Nn / 64) >= 128 and K >= 64 and K % 8 == 0


def weight_planes(w, b_kc, M):
    """The cached planes of weight (or weight slice, ops.cols) `w` for a product with M rows, or None: no optimizer
    owns the parameter, records are off, or the product is not one gemm_h2w.hip takes."""
    if not (H2 and H2W) or w is None or w.dim() != 2 or w.dtype != torch.float32:
        return None
    base, c0, c1 = getattr(w, "_wslice", (w, 0, None))
    reg = getattr(base, "_planes", None)
    rec = amax_of(base)
    if reg is None or rec is None:
        return None
    Nn, K = (w.shape[0], w.shape[1]) if b_kc else (w.shape[1], w.shape[0])
    if not planes_wanted(M, Nn, K):
        return None
    key = (bool(b_kc), c0, c1)
    pl = reg.get(key)
    clock = getattr(base, "_planes_clock", None)
    if pl is None or (clock is not None and not clock.current(base, key)):
        if torch.cuda.is_current_stream_capturing():
            return None               # (registered by the eager steps that precede a capture; a stale set: cut in-kernel)
        # first use, or a set no launch has re-cut since the optimizer last wrote the weight (registered after the
        # step was captured): cut now, into the same buffer — a later capture may have its address baked in
        pl = reg[key] = h2_weight_planes(base.detach()[:, c0:c1] if (c0, c1) != (0, None) else base.detach(), b_kc, rec,
                                         out=pl)
        if clock is not None:
            base._planes_at[key] = clock.step
    return pl


class PlaneClock:
    """How a plane set is known to be current.  `step` counts the optimizer's updates of the weights (MapxOptimizer
    .steps_done lives here); every cut stamps its set with the count the weights are at (`p._planes_at[key]`).  A
    captured step re-cuts, on every replay, exactly the sets that were registered when it was captured and runs no
    Python doing so: the replay notes that frozen set of (id(p), key) as `covered` at the new count instead of
    stamping each.  A set is current when its stamp or the covered note says so; any other — one first cut by an
    eval between two replays — is cut again at its next use (weight_planes)."""
    __slots__ = ("step", "covered", "covered_at")

    def __init__(self):
        self.step, self.covered, self.covered_at = 0, frozenset(), -1

    def current(self, p, key):
        return p._planes_at.get(key) == self.step or (self.covered_at == self.step and (id(p), key) in self.covered)

    def replayed(self, keys):
        """A captured optimizer step that re-cuts `keys` has been replayed."""
        self.step += 1
        self.covered, self.covered_at = keys, self.step

    def covers(self, keys):
        """Did the last update of the weights come from a replay that re-cut all of `keys`?"""
        return self.covered_at == self.step and (self.covered is keys or keys <= self.covered)


def plane_keys(params):
    """The registered plane sets of the parameters as a frozenset of (id(p), key): what a refresh_weight_planes launch
    captured now re-cuts on every replay."""
    return frozenset((id(p), key) for p in params for key in (getattr(p, "_planes", None) or ()))


def refresh_weight_planes(params, at=None, stamp=True, stale_only=False):
    """Re-cut every registered plane set of the parameters (their records must be current on this stream): one
    launch per 16 sets.  The sets are stamped with the update count `at` (default: the PlaneClock's present one;
    stamp=False inside a capture, which runs no kernel); stale_only: only the sets that are not current."""
    if isinstance(params, torch.Tensor):
        params = [params]
    todo = []
    for p in params:
        reg = getattr(p, "_planes", None)
        if not reg:
            continue
        clock = getattr(p, "_planes_clock", None)
        for (b_kc, c0, c1), pl in reg.items():
            if stale_only and (clock is None or clock.current(p, (b_kc, c0, c1))):
                continue
            w = p.detach()[:, c0:c1] if (c0, c1) != (0, None) else p.detach()
            Nn, K = (w.shape[0], w.shape[1]) if b_kc else (w.shape[1], w.shape[0])
            todo.append((w, Nn, K, b_kc, p._amax, pl))
            if stamp and clock is not None:
                p._planes_at[(b_kc, c0, c1)] = clock.step if at is None else at
    for i in range(0, len(todo), 16):
        part = todo[i:i + 16]
        arr = (N.PlaneTask * len(part))()
        for j, (w, Nn, K, b_kc, rec, pl) in enumerate(part):
            arr[j].W, arr[j].ldw, arr[j].N, arr[j].K, arr[j].b_kc = w.data_ptr(), w.stride(0), Nn, K, int(b_kc)
            arr[j].amax_record, arr[j].planes = rec.data_ptr(), pl.data_ptr()
        check(lib.mapx_h2_weight_planes_multi(arr, len(part), stream()))


def _as2d(t, ld):
    """The [rows, ld] matrix an operand pointer + leading dimension describes (AUTO_AMAX: a superset of the operand)."""
    return t if t.dim() == 2 else t.reshape(-1, ld)


def _scale_arg(amax_a, amax_b, amax_c=None, amax_c2=None, b_planes=None):
    if amax_a is None and amax_b is None and amax_c is None and amax_c2 is None:
        return None
    sc = N.GemmScale()
    sc.b_planes = b_planes.data_ptr() if (b_planes is not None and amax_a is not None) else None
    sc.amax_a = amax_a.data_ptr() if amax_a is not None else None
    sc.amax_b = amax_b.data_ptr() if amax_b is not None else None
    sc.amax_c = amax_c.data_ptr() if amax_c is not None else None
    sc.amax_c2 = amax_c2.data_ptr() if amax_c2 is not None else None
    return sc


def gemm(a, b, a_kc, b_kc, M, N, K, out=None, ldc=None, epi=N.EPI_NONE, bias=None, aux1=None,
         aux2=None, out2=None, nsplit=1, lda=None, ldb=None, tile=-1, out_dtype=None,
         amax_a=None, amax_b=None, amax_c=None, record=True, b_planes=None):
    """C[M,N] = epi(sum_k A(m,k) B(k,n)); see include/mapx_hip.h: mapx_gemm_f32 (fp32 operands) /
    mapx_gemm_bf16 (bf16 operands; `out_dtype` picks a bf16 or fp32 result).  amax_a / amax_b: the operands'
    magnitude records (both given: the two-piece fp16 arithmetic); amax_c: record raised with max |C|."""
    require_gpu(a, b)
    if is_bf16(a):
        return gemm_bf16(a, b, a_kc, b_kc, M, N, K, out=out, out_dtype=out_dtype or BF16, ldc=ldc, epi=epi,
                         bias=bias, aux1=aux1, aux2=aux2, out2=out2, nsplit=nsplit, lda=lda, ldb=ldb, tile=tile)
    dev = a.device
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=dev)
    ldc = ldc if ldc is not None else out.stride(0)
    lda = lda if lda is not None else a.stride(0)
    ldb = ldb if ldb is not None else b.stride(0)
    ws, wsn = None, 0
    if nsplit > 1:
        ws = scratch(lib.mapx_gemm_splitk_workspace_bytes(M, N, nsplit), dev)
        wsn = ws.numel()
    ld1 = aux1.stride(0) if aux1 is not None else 0
    ld2 = aux2.stride(0) if aux2 is not None else 0
    ldo2 = out2.stride(0) if out2 is not None else 0
    kind = "gemm_fwd_nt" if (a_kc and b_kc) else ("gemm_dx_nn" if a_kc else "gemm_dw_tn")
    amax_a = amax_a if amax_a is not None else amax_of(a)
    amax_b = amax_b if amax_b is not None else amax_of(b)
    if AUTO_AMAX and H2:
        amax_a = amax_a if amax_a is not None else amax(_as2d(a, lda))
        amax_b = amax_b if amax_b is not None else amax(_as2d(b, ldb))
        if b_planes is None and H2W and a_kc and nsplit == 1 and tile < 0 and planes_wanted(M, N, K) \
                and b.dim() == 2 and b.stride(1) == 1:
            b_planes = h2_weight_planes(b[:N, :K] if b_kc else b[:K, :N], b_kc, amax_b)
    if amax_c is None and record and nsplit == 1:      # (split-K outputs are weight gradients: nobody multiplies them)
        amax_c = out_record(out, dev)
    H2_USED[0 if (amax_a is not None and amax_b is not None) else 1] += 1
    if AMAX_CHECK and not torch.cuda.is_current_stream_capturing():
        _check_record(a, amax_a, "A")
        _check_record(b, amax_b, "B")
    sc = _scale_arg(amax_a, amax_b, amax_c, b_planes=b_planes if b_planes is not None else
                    (weight_planes(b, b_kc, M) if (a_kc and nsplit == 1 and tile < 0) else None))
    with _timed(kind, 2.0 * M * N * K):
        check(lib.mapx_gemm_f32(int(a_kc), int(b_kc), M, N, K, a.data_ptr(), lda, b.data_ptr(), ldb,
                                out.data_ptr(), ldc, epi, ptr(bias),
                                aux1.data_ptr() if aux1 is not None else None, ld1,
                                aux2.data_ptr() if aux2 is not None else None, ld2,
                                out2.data_ptr() if out2 is not None else None, ldo2, nsplit, tile,
                                ws.data_ptr() if ws is not None else None, wsn, None,
                                None if sc is None else native_byref(sc), stream()))
    return tag(out, amax_c)


# Layers with at most 32 outputs (RFD's last predictor layer, the finetune head) as fp32 streaming kernels instead of
# MFMA GEMM tiles that are mostly padding (csrc/skinny.hip).  A/B switch: MAPX_SKINNY=0.
SKINNY = os.environ.get("MAPX_SKINNY", "1") == "1"


def _rows16(t):
    return t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 \
        and t.data_ptr() % 16 == 0


def _rows8h(t):
    return t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1 and t.stride(0) % 4 == 0 \
        and t.data_ptr() % 8 == 0


# bf16 compute mode: layers of at most 8 outputs (the finetune head) on the streaming kernels' bf16 forms instead of a
# 128-wide MFMA tile per useful column
SKINNY_BF16 = os.environ.get("MAPX_SKINNY_BF16", "1") == "1"


def _skinny_h(Nn, K, *mats):
    return SKINNY and SKINNY_BF16 and 1 <= Nn <= 8 and K >= 4 and K % 4 == 0 and all(_rows8h(m) for m in mats)


_TALL_ROWS = 128
SKINNY_MAX = int(os.environ.get("MAPX_SKINNY_MAX", "8"))            # forward: wider layers measured faster on the GEMM
# dW / dX (RFD's 23-wide layer: 14.6 / 8.6 vs 28 / 12 us).  The kernels take up to 64 outputs (Criteo's 39-wide layer:
# dW 45 -> 26 us, its RFD step -2.3 %): opt-in.  (With 33..64 on, the captured step of the 64-wide test models stopped
# agreeing with the eager one — traced to the packed FMAs of skinny_dw_tall_kernel, see there; now a test of its own.)
SKINNY_MAX_BWD = int(os.environ.get("MAPX_SKINNY_MAX_BWD", "32"))
SKINNY_TALL = os.environ.get("MAPX_SKINNY_TALL", "0") == "1"


def _skinny(Nn, K, *mats, bwd=False):
    return SKINNY and 1 <= Nn <= (SKINNY_MAX_BWD if bwd else SKINNY_MAX) and K >= 4 and K % 4 == 0 \
        and all(_rows16(m) for m in mats)


def _streaming(half, Nn, K, *mats, bwd=False):
    """Do the narrow-layer streaming kernels of the element type take this layer?"""
    return _skinny_h(Nn, K, *mats) if half else _skinny(Nn, K, *mats, bwd=bwd)


def _sum_now(dst, src, stride, nsplit, n):
    arr = (N.SumTask * 1)()
    arr[0].dst, arr[0].src, arr[0].stride, arr[0].n, arr[0].nsplit = dst.data_ptr(), src.data_ptr(), stride, n, nsplit
    check(lib.mapx_sum_tasks(arr, 1, stream()))


def linear_fwd(x, w, b, relu=False, out=None, out_dtype=None):
    """nn.Linear (+ReLU): x [M,K], w [N,K], b [N] -> [M,N]; `out` may be a column slice.  bf16 x:
    `w` is the weight's bf16 operand (ops.bf16_weight), b stays fp32, the result is bf16 or
    (`out_dtype=torch.float32`: the heads' logits) fp32."""
    M, K = x.shape
    Nn = w.shape[0]
    half = is_bf16(x)
    f32_out = out_dtype == torch.float32 or (out_dtype is None and not half)
    if f32_out and _streaming(half, Nn, K, x, w) and (out is None or out.dtype == torch.float32):
        require_gpu(x, w)
        y = out if out is not None else torch.empty(M, Nn, dtype=torch.float32, device=x.device)
        fn = lib.mapx_skinny_linear_fwd_bf16 if half else lib.mapx_skinny_linear_fwd
        with _timed("skinny_linear", float(x.element_size()) * (M * K + Nn * K) + 4.0 * M * Nn):
            check(fn(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(b), M, Nn, K, int(relu), y.data_ptr(), y.stride(0),
                     stream()))
        return y
    return gemm(x, w, True, True, M, Nn, K, out=out, epi=N.EPI_BIAS_RELU if relu else N.EPI_BIAS,
                bias=b, out_dtype=out_dtype)


RELU_LINK = os.environ.get("MAPX_RELU_LINK", "1") == "1"


def fused_mask_colsum_ok(dy, relu_of):
    """Can linear_bwd_input also apply the upstream ReLU's mask and form its bias gradient?  (16-byte rows.)"""
    if not (RELU_LINK and relu_of.dim() == 2 and dy.dtype == relu_of.dtype):
        return False
    if is_bf16(dy):
        return relu_of.shape[1] % 8 == 0 and relu_of.stride(1) == 1 and relu_of.stride(0) % 8 == 0 \
            and relu_of.data_ptr() % 16 == 0
    return dy.dtype == torch.float32 and relu_of.shape[1] % 4 == 0 and row_sliceable(relu_of)


def part_rows(M, dtype=torch.float32):
    """Partial rows of a column-sum epilogue (EPI_RELU_MASK_COLSUM, mapx_gemm_f32_bwd_fused) over M rows: the fp32
    kernels write one per 64 rows (tiles of 128 rows: the sum and a row of zeros), the bf16 ones one per 128."""
    return (M + 63) // 64 if dtype == torch.float32 else (M + 127) // 128


def linear_bwd_input(dy, w, out=None, add=None, relu_of=None, colsum_to=None):
    """dX = dY W  (+ add)  or masked by relu_of > 0.  dy [M,N], w [N,K] -> [M,K] (dtype of dy;
    bf16: `add` may be fp32 — the cross tower's running dL/dX0).
    colsum_to (with relu_of; see fused_mask_colsum_ok): the masked result is the upstream ReLU layer's dZ,
    and its column sums — that layer's bias gradient — leave the same epilogue as partial rows (part_rows),
    summed into `colsum_to` by flush_deferred()."""
    M, Nn = dy.shape
    K = w.shape[1]
    half = is_bf16(dy)
    if add is None and relu_of is None and (half or dy.dtype == torch.float32) and _streaming(half, Nn, K, w, bwd=True) \
            and dy.dim() == 2 and dy.stride(1) == 1 and (out is None or (_rows8h if half else _rows16)(out)):
        require_gpu(dy, w)
        dx = out if out is not None else torch.empty(M, K, dtype=dy.dtype, device=dy.device)
        fn = lib.mapx_skinny_linear_dx_bf16 if half else lib.mapx_skinny_linear_dx
        with _timed("skinny_linear", float(dy.element_size()) * (M * K + Nn * K + M * Nn)):
            check(fn(ptr(dy), dy.stride(0), ptr(w), w.stride(0), M, Nn, K, dx.data_ptr(), dx.stride(0), stream()))
        return dx
    epi, aux, out2 = N.EPI_NONE, None, None
    if add is not None:
        epi, aux = N.EPI_ADD, add
    elif relu_of is not None and colsum_to is not None:
        epi, aux = N.EPI_RELU_MASK_COLSUM, relu_of
        out2 = torch.empty(part_rows(M, dy.dtype), K, dtype=torch.float32, device=dy.device)
    elif relu_of is not None:
        epi, aux = N.EPI_RELU_MASK, relu_of
    dx = gemm(dy, w, True, False, M, K, Nn, out=out, epi=epi, aux1=aux, out2=out2)
    if out2 is not None:
        defer_sum(colsum_to, out2, K, out2.shape[0], K)
    return dx


def _splits_wide_tiles(M, Nn, Kred, count=1):
    """split-K factor for the bf16-MFMA kernels (bf16 operands, or fp32 cut into three bf16 pieces):
    128 x 128 tiles (of `count` equal problems in one launch), split over K until they cover the 256 CUs,
    K chunk >= 256."""
    tiles = math.ceil(M / 128) * math.ceil(Nn / 128) * count
    ns = 1
    while ns < 16 and tiles * ns * 2 <= 288 and Kred // (ns * 2) >= 256:
        ns *= 2
    return ns


def linear_bwd_weight(dy, x, out=None, defer=False):
    """dW = dY^T X.  dy [B,N], x [B,K] -> [N,K].  defer (needs out): the streaming kernels leave their row-chunk
    partials for flush_deferred(); the MFMA GEMMs sum their split-K slabs at once."""
    Bn, Nn = dy.shape
    K = x.shape[1]
    # (also: both dimensions small over many rows — AutoInt's attention projections, dW [40, 16 | 40] over B*F rows.
    # Opt-in since round 4 (MAPX_SKINNY_TALL=1): this is the kernel whose compiler-generated packed FMAs
    # gave a timing-dependent wrong result beside MFMA kernels in round 3; the re-written loop has passed every
    # bitwise graph == eager run since, but the mechanism was never found, so the default is the GEMM.)
    tall = SKINNY and SKINNY_TALL and 32 < Nn <= 64 and 4 <= K <= 64 and K % 4 == 0 and Bn >= 8192 and _rows16(x)
    half = is_bf16(dy)                       # (bf16: at most 8 outputs, so none of the wide forms' rules below applies)
    ok = _skinny_h(Nn, K, x) if half else dy.dtype == torch.float32 and (_skinny(Nn, K, x, bwd=True) or tall)
    rows_cap = 64 if (Nn > 32 and K > 64) else _TALL_ROWS     # (33..64 outputs x many columns: the LDS-tiled form only)
    if ok and Nn > 32 and K > 64 and Bn > 64 * 2048:
        ok = False
    if Bn >= 1 and ok and dy.dim() == 2 and dy.stride(1) == 1 \
            and (out is None or (out.dtype == torch.float32 and out.is_contiguous())):
        require_gpu(dy, x)
        chunks = lib.mapx_skinny_chunks()
        while -(-Bn // chunks) > rows_cap and chunks < 2048:  # tall problems: a chunk is a workgroup
            chunks *= 2
        dw = out if out is not None else torch.empty(Nn, K, dtype=torch.float32, device=dy.device)
        part = torch.empty(chunks, Nn * K, dtype=torch.float32, device=dy.device)
        fn = lib.mapx_skinny_linear_dw_bf16 if half else lib.mapx_skinny_linear_dw
        with _timed("skinny_linear", float(dy.element_size()) * (Bn * K + Bn * Nn) + 4.0 * chunks * Nn * K):
            check(fn(ptr(dy), dy.stride(0), ptr(x), x.stride(0), Bn, Nn, K, ptr(part), chunks, stream()))
        if defer and out is not None:
            defer_sum(dw, part, Nn * K, chunks, Nn * K)          # with the step's other partial sums
        else:
            _sum_now(dw, part, Nn * K, chunks, Nn * K)
        return dw
    # the bf16-MFMA kernels want 128 x 128 tiles (half the L2 -> LDS bytes per flop of 64 x 64 ones)
    ns = _splits_wide_tiles(Nn, K, Bn)
    if out is not None and out.stride(0) != K:
        ns = 1
    if is_bf16(dy):                          # fp32 gradient from bf16 operands
        return gemm_bf16(dy, x, False, False, Nn, K, Bn, out=out, out_dtype=torch.float32, nsplit=ns)
    return gemm(dy, x, False, False, Nn, K, Bn, out=out, nsplit=ns, record=False)


def _partials(Nn, device, defer):
    """Workspace of the column-sum kernels, either element type: COLSUM_CHUNKS partial rows of Nn floats.  defer: a
    buffer of its own (it lives until flush_deferred sums it) instead of the stream's scratch."""
    nb = lib.mapx_colsum_workspace_bytes(Nn)
    return torch.empty(nb, dtype=torch.uint8, device=device) if defer else scratch(nb, device)


def _colsum_operand(t, half):
    """t as the fused column-sum kernels read it: in place when the rows qualify (fp32: row_sliceable, the float4
    lanes; bf16: unit column stride, the kernel picks its lanes by alignment), else a contiguous copy."""
    return t if (t.stride(1) == 1 if half else row_sliceable(t)) else t.contiguous()


def colsum(x, out=None, defer=False):
    """Column sums; defer (needs out): leave the row-chunk partials for flush_deferred()."""
    require_gpu(x)
    M, Nn = x.shape
    half = is_bf16(x)
    defer = defer and out is not None
    if out is None:
        out = torch.empty(Nn, dtype=torch.float32, device=x.device)
    if half and x.stride(1) != 1:            # (the fp32 kernel is handed x as it is)
        x = x.contiguous()
    ws = _partials(Nn, x.device, defer)
    fn = lib.mapx_colsum_bf16 if half else lib.mapx_colsum
    check(fn(x.data_ptr(), x.stride(0), M, Nn, None if defer else ptr(out), ptr(ws), ws.numel(), stream()))
    if defer:
        defer_sum(out, ws.view(torch.float32), Nn, COLSUM_CHUNKS, Nn)
    return out


def cross_layer_fwd(x0, xi, w, b, out=None):
    """-> (X_{i+1} = Xi + X0 * (Xi W^T + b), u = Xi W^T + b)   (layers.py:200)."""
    M, D = xi.shape
    u = torch.empty(M, D, dtype=xi.dtype, device=xi.device)
    y = gemm(xi, w, True, True, M, D, D, out=out, epi=N.EPI_BIAS_CROSS, bias=b, aux1=xi, aux2=x0,
             out2=u)            # (y carries its record: the next layer's operand; u is read elementwise only)
    return y, u


def cross_bwd_pre(g, x0, u, dx0=None):
    """t = g*x0; dx0 (+)= g*u.  Returns (t, dx0)."""
    t = torch.empty_like(g)
    acc = dx0 is not None
    if dx0 is None:
        dx0 = torch.empty_like(g)
    check(lib.mapx_cross_bwd_pre(ptr(g), ptr(x0), ptr(u), g.numel(), ptr(t), ptr(dx0), int(acc),
                                 stream()))
    return t, dx0


def alias_cols(buf, col0, ncols):
    """A tensor over columns [col0, col0+ncols) of the 2-D buffer `buf` that shares its memory but
    is NOT an autograd view of it: kernels write a layer's output straight into its slot of a
    concatenated buffer, and autograd's view+in-place bookkeeping never sees a relationship."""
    return carry(torch.empty(0, dtype=buf.dtype, device=buf.device).set_(
        buf.untyped_storage(), buf.storage_offset() + col0, (buf.shape[0], ncols), (buf.stride(0), 1)), buf)


def row_sliceable(x):
    """True if x [M,N] can be read in place by the float4 row kernels: unit column stride,
    16-byte aligned rows (a column slice of a wider buffer qualifies: no .contiguous() copy)."""
    return x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 \
        and x.stride(0) >= x.shape[1]


def relu_mask_colsum(dy, y, db=None, defer=False):
    """-> (dz = y > 0 ? dy : 0, db = colsum(dz)) in one pass.  dy may be a column slice.  fp32: dz carries its
    magnitude record."""
    half = is_bf16(dy)
    dy, y = _colsum_operand(dy, half), _colsum_operand(y, half)
    M, Nn = dy.shape
    dz = torch.empty(M, Nn, dtype=BF16 if half else torch.float32, device=dy.device)
    defer = defer and db is not None
    if db is None:
        db = torch.empty(Nn, dtype=torch.float32, device=dy.device)
    ws = _partials(Nn, dy.device, defer)
    rec = None if half else amax_record(dy.device)
    fn = lib.mapx_relu_mask_colsum_bf16 if half else lib.mapx_relu_mask_colsum
    check(fn(dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), M, Nn, ptr(dz), None if defer else ptr(db), ptr(ws),
             ws.numel(), *(() if half else (ptr(rec),)), stream()))
    if defer:
        defer_sum(db, ws.view(torch.float32), Nn, COLSUM_CHUNKS, Nn)
    return tag(dz, rec), db


def cross_bwd_pre_colsum(g, x0, u, dx0=None, db=None, defer=False, plus_g=False):
    """-> (t = g*x0, dx0 (+)= g*u (+ g if plus_g), db = colsum(t)) in one pass.  g may be a column slice.
    bf16 mode: g, x0, u, t bf16; the running dx0 and db fp32.  fp32: t carries its magnitude record."""
    half = is_bf16(g)
    g = _colsum_operand(g, half)
    M, Nn = g.shape
    t = torch.empty(M, Nn, dtype=BF16 if half else torch.float32, device=g.device)
    acc = dx0 is not None
    if dx0 is None:
        dx0 = torch.empty(M, Nn, dtype=torch.float32, device=g.device)
    defer = defer and db is not None
    if db is None:
        db = torch.empty(Nn, dtype=torch.float32, device=g.device)
    ws = _partials(Nn, g.device, defer)
    rec = None if half else amax_record(g.device)
    fn = lib.mapx_cross_bwd_pre_colsum_bf16 if half else lib.mapx_cross_bwd_pre_colsum
    check(fn(g.data_ptr(), g.stride(0), ptr(x0), ptr(u), M, Nn, ptr(t), ptr(dx0), int(acc) | (2 if plus_g else 0),
             None if defer else ptr(db), ptr(ws), ws.numel(), *(() if half else (ptr(rec),)), stream()))
    if defer:
        defer_sum(db, ws.view(torch.float32), Nn, COLSUM_CHUNKS, Nn)
    return tag(t, rec), dx0, db


JOIN_FUSE = os.environ.get("MAPX_JOIN_FUSE", "1") == "1"      # the heads' dX as one product per tower with fused epilogues
# cross dX GEMMs do the next layer's elementwise backward: off by default — inside the tuned schedule (tools/flag_sweep.py,
# round 3) the fused form is 1.1 % slower (0.8314 vs 0.8223 ms per step) although it saves three launches
CROSS_FUSE = os.environ.get("MAPX_CROSS_FUSE", "0") == "1"
DW_BATCH = os.environ.get("MAPX_DW_BATCH", "1") == "1"        # the cross layers' weight gradients from one launch


def gemm_bwd_fused(dy, w, c0, add=None, mask=None, x0=None, u=None, dx0=None, plus_v=False, out=None):
    """v = dy W (+ add) with the elementwise backward that follows it done in the GEMM's epilogue
    (include/mapx_hip.h: mapx_gemm_f32_bwd_fused): columns >= c0 masked by `mask` > 0 (the ReLU layer whose output
    `mask` is), columns < c0 the cross layer's  t = v x0,  dx0 (+)= v u (+ v).  fp32.
    -> (C [M,N], t [M,c0] | None, dx0 [M,c0] | None, part [ceil(M/64), N]: partial rows of the bias gradients)."""
    require_gpu(dy, w)
    M, K = dy.shape
    Nn = w.shape[1]
    dev = dy.device
    C = out if out is not None else torch.empty(M, Nn, dtype=torch.float32, device=dev)
    t = torch.empty(M, c0, dtype=torch.float32, device=dev) if c0 > 0 else None
    accumulate = dx0 is not None
    if c0 > 0 and dx0 is None:
        dx0 = torch.empty(M, c0, dtype=torch.float32, device=dev)
    part = torch.empty(part_rows(M), Nn, dtype=torch.float32, device=dev)
    sd = lambda x: (x.data_ptr(), x.stride(0)) if x is not None else (None, 0)
    # records: C's ReLU-masked columns (>= c0: the deep tower's dZ) and t, the operands of the products that follow
    rec_c = amax_record(dev) if c0 < Nn else None
    rec_t = amax_record(dev) if c0 > 0 else None
    ra, rb, pl = amax_of(dy), amax_of(w), weight_planes(w, False, M)
    if AUTO_AMAX and H2:
        ra = ra if ra is not None else amax(dy)
        rb = rb if rb is not None else amax(w)
        if pl is None and H2W and planes_wanted(M, Nn, K) and w.stride(1) == 1:
            pl = h2_weight_planes(w, False, rb)
    sc = _scale_arg(ra, rb, rec_c, rec_t, b_planes=pl)
    with _timed("gemm_dx_nn", 2.0 * M * Nn * K):
        check(lib.mapx_gemm_f32_bwd_fused(M, Nn, K, dy.data_ptr(), dy.stride(0), w.data_ptr(), w.stride(0),
                                          C.data_ptr(), C.stride(0), *sd(add), *sd(mask), c0, *sd(x0), *sd(u), *sd(t),
                                          *sd(dx0), int(accumulate), int(plus_v), part.data_ptr(), part.stride(0),
                                          None if sc is None else native_byref(sc), stream()))
    if c0 == 0:
        tag(C, rec_c)            # (0 < c0 < N: C mixes g and dZ — callers slice it and tag the slices)
    C._amax_dz = rec_c
    return C, tag(t, rec_t), dx0, part


def skinny_join_bwd(dz, w, final, D, x0, u, plus_v):
    """The input gradient of a head of at most 8 outputs over DCNv2's towers, both towers' first backward step included
    (csrc/skinny.hip; the wide heads' form: gemm_bwd_fused + linear_bwd_input(relu_of=, colsum_to=)).
    -> (g, t, dx0 [M, D], dzr [M, H], part_cross [tiles, D], part_deep [tiles, H])."""
    require_gpu(dz, w, final, x0, u)
    M, Nn = dz.shape
    H = final.shape[1] - D
    f32 = dict(dtype=torch.float32, device=dz.device)
    g, t, dx0 = torch.empty(M, D, **f32), torch.empty(M, D, **f32), torch.empty(M, D, **f32)
    dzr = torch.empty(M, H, **f32)
    tiles = (M + 127) // 128
    pc, pd = torch.empty(tiles, D, **f32), torch.empty(tiles, H, **f32)
    rec_t, rec_z = amax_record(dz.device), amax_record(dz.device)
    with _timed("skinny_linear", 4.0 * (3.0 * M * (D + H) + 3.0 * M * D)):
        check(lib.mapx_skinny_join_bwd(ptr(dz), dz.stride(0), ptr(w), w.stride(0), M, Nn, D, H, final.data_ptr(),
                                       final.stride(0), ptr(x0), x0.stride(0), ptr(u), u.stride(0), int(plus_v), ptr(g),
                                       D, ptr(t), D, ptr(dx0), D, ptr(dzr), H, ptr(pc), ptr(pd), ptr(rec_t), ptr(rec_z),
                                       stream()))
    return g, tag(t, rec_t), dx0, tag(dzr, rec_z), pc, pd


def defer_part_rows(dst, part, col0, ncols):
    """Queue dst[0:ncols] = column sums of part[:, col0 : col0 + ncols] (partial rows of a fused epilogue)."""
    defer_sum(dst, part.view(-1)[col0:], part.stride(0), part.shape[0], ncols)


def linear_bwd_weight_batched(dys, xs, outs):
    """dW_z = dy_z^T x_z for up to four equal-shaped layers in ONE launch (+ one slab sum): dy_z [B,N],
    x_z [B,K] -> outs[z] [N,K] (dense fp32, written in place).  The cross layers' weight gradients."""
    import ctypes as C
    cnt = len(dys)
    Bn, Nn = dys[0].shape
    K = xs[0].shape[1]
    for d, x, o in zip(dys, xs, outs):
        require_gpu(d, x, o)
        if d.shape != (Bn, Nn) or x.shape != (Bn, K) or o.shape != (Nn, K) or not (d.is_contiguous() and x.is_contiguous()
                                                                                   and o.is_contiguous()):
            raise ValueError("linear_bwd_weight_batched: equal shapes, contiguous operands")
    ns = _splits_wide_tiles(Nn, K, Bn, count=cnt)
    ws = scratch(cnt * lib.mapx_gemm_splitk_workspace_bytes(Nn, K, ns), dys[0].device) if ns > 1 else None
    PP = C.c_void_p * cnt
    scales = None
    if AUTO_AMAX and H2:
        for t_ in list(dys) + list(xs):
            if amax_of(t_) is None:
                tag(t_, amax(t_))
    if all(amax_of(d) is not None and amax_of(x) is not None for d, x in zip(dys, xs)):
        scales = (N.GemmScale * cnt)()
        for z, (d, x) in enumerate(zip(dys, xs)):
            scales[z].amax_a, scales[z].amax_b = amax_of(d).data_ptr(), amax_of(x).data_ptr()
    with _timed("gemm_dw_tn", 2.0 * cnt * Nn * K * Bn):
        check(lib.mapx_gemm_f32_batched(cnt, 0, 0, Nn, K, Bn, PP(*[d.data_ptr() for d in dys]), Nn,
                                        PP(*[x.data_ptr() for x in xs]), K, PP(*[o.data_ptr() for o in outs]), ns,
                                        ws.data_ptr() if ws is not None else None,
                                        ws.numel() if ws is not None else 0, scales, stream()))
    return outs


def relu_mask(dy, y):
    out = torch.empty_like(dy)
    fn = lib.mapx_relu_mask_bf16 if is_bf16(dy) else lib.mapx_relu_mask
    check(fn(ptr(dy), ptr(y), dy.numel(), ptr(out), stream()))
    return out


# --------------------------------------------------------------------------- dropout / LayerNorm options
ACT_KINDS = {"tanh": 1, "sigmoid": 2, "none": 3, "elu": 4, "leu": 5, "gelu": 6, "gelu_new": 7, "swish": 8, "mish": 9}


def act_fwd(kind, z, out=None):
    """y = f(z) for the reference's activations other than relu (layers.py:55-80); z [M,N] contiguous fp32 or bf16
    (f in fp32, y of z's type), `out`: optional destination with unit column stride (a column slice of a wider
    buffer)."""
    require_gpu(z)
    if z.dtype not in (torch.float32, BF16) or z.dim() != 2 or not z.is_contiguous():
        raise TypeError("act_fwd: z must be a contiguous fp32 or bf16 matrix")
    M, Nn = z.shape
    if out is None:
        out = torch.empty_like(z)
    if out.shape != z.shape or out.stride(1) != 1 or out.dtype != z.dtype:
        raise ValueError("act_fwd: `out` must have z's shape and element type and unit column stride")
    fn = lib.mapx_act_fwd_bf16 if is_bf16(z) else lib.mapx_act_fwd
    check(fn(ACT_KINDS[kind], ptr(z), M, Nn, out.data_ptr(), out.stride(0), stream()))
    return out


def act_bwd(kind, dy, z):
    """dz = dy * f'(z); dy may be a row-strided slice."""
    require_gpu(dy, z)
    if dy.stride(1) != 1:
        dy = dy.contiguous()
    M, Nn = z.shape
    fn = lib.mapx_act_bwd_bf16 if _one_dtype("act_bwd", "dy and z", dy, z) else lib.mapx_act_bwd
    dz = torch.empty_like(z)
    check(fn(ACT_KINDS[kind], dy.data_ptr(), dy.stride(0), ptr(z), M, Nn, ptr(dz), stream()))
    return dz


def dropout(x, p, seed, offset, offset_dev=None, out=None):
    """out = keep ? x / (1 - p) : 0, keep mask = Philox(seed, offset + *offset_dev) (never stored: the
    backward pass calls this again on the gradient with the same seed / offset).  fp32, or bf16 (x / (1 - p) in
    fp32, rounded once; the same mask)."""
    require_gpu(x)
    if x.dtype not in (torch.float32, BF16):
        raise NotImplementedError("dropout is built for fp32 and bf16 tensors")
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    if not out.is_contiguous() or out.dtype != x.dtype:
        raise ValueError("dropout writes a contiguous tensor of x's element type")
    fn = lib.mapx_dropout_bf16 if is_bf16(x) else lib.mapx_dropout
    check(fn(ptr(x), x.numel(), float(p), int(seed), int(offset), ptr(offset_dev), ptr(out), stream()))
    return out


def layernorm_fwd(x2, w, b, eps):
    """x2 [R,E] -> (y [R,E], stats [R,2] = {mean, rstd})   (nn.LayerNorm over the last dimension)."""
    require_gpu(x2, w, b)
    x2 = x2.contiguous()
    R, E = x2.shape
    y = torch.empty_like(x2)
    stats = torch.empty(R, 2, dtype=torch.float32, device=x2.device)
    check(lib.mapx_layernorm_fwd(ptr(x2), R, E, ptr(w), ptr(b), float(eps), ptr(y), ptr(stats), stream()))
    return y, stats


def layernorm_bwd(dy2, x2, w, stats):
    """-> (dx [R,E], dy * xhat [R,E]: its column sums are dL/dw; dL/db = column sums of dy)."""
    require_gpu(dy2, x2, w, stats)
    dy2 = dy2.contiguous()
    R, E = x2.shape
    dx, dyx = torch.empty_like(x2), torch.empty_like(x2)
    check(lib.mapx_layernorm_bwd(ptr(dy2), ptr(x2), ptr(w), ptr(stats), R, E, ptr(dx), ptr(dyx), stream()))
    return dx, dyx


def add_layernorm_fwd(x2, s2, w, b, eps):
    """bf16 x2 [R,E], s2 [R,E] or None -> (y = LN(x2 + s2) bf16, stats [R,2] fp32 = {mean, rstd}).  The sum is formed
    in fp32 inside the kernel and normalised unrounded (the Transformer's residual add + LayerNorm in bf16 mode)."""
    require_gpu(x2, s2, w, b)
    ts = (x2,) if s2 is None else (x2, s2)
    if not _one_dtype("add_layernorm_fwd", "x and s", *ts) or any(not t.is_contiguous() or t.shape != x2.shape
                                                                  for t in ts):
        raise TypeError("add_layernorm_fwd: x (and s) are contiguous bf16 matrices of one shape")
    R, E = x2.shape
    y = torch.empty_like(x2)
    stats = torch.empty(R, 2, dtype=torch.float32, device=x2.device)
    check(lib.mapx_add_layernorm_fwd_bf16(ptr(x2), ptr(s2), R, E, ptr(_f32(w, "add_layernorm_fwd: w")),
                                          ptr(_f32(b, "add_layernorm_fwd: b")), float(eps), ptr(y), ptr(stats), stream()))
    return y, stats


def add_layernorm_bwd(dy2, x2, s2, w, stats, dw=None, db=None, defer=False):
    """-> (dsum [R,E] bf16: the gradient of BOTH addends, dL/dw [E], dL/db [E] fp32).  The kernel leaves one fp32
    partial row (dw | db) per workgroup; they are summed at once, or (defer, with `dw` and `db` given) by
    flush_deferred() with the step's other partial sums."""
    require_gpu(dy2, x2, s2, w, stats)
    dy2 = dy2.contiguous()
    ts = (dy2, x2) if s2 is None else (dy2, x2, s2)
    if not _one_dtype("add_layernorm_bwd", "dy, x and s", *ts) or any(t.shape != x2.shape for t in ts):
        raise TypeError("add_layernorm_bwd: dy, x (and s) are bf16 matrices of one shape")
    R, E = x2.shape
    dsum = torch.empty_like(x2)
    dw = dw if dw is not None else torch.empty(E, dtype=torch.float32, device=x2.device)
    db = db if db is not None else torch.empty(E, dtype=torch.float32, device=x2.device)
    if R == 0:
        dw.zero_()
        db.zero_()
        return dsum, dw, db
    groups = lib.mapx_add_layernorm_bwd_groups(R, E)
    part = torch.empty(groups, 2 * E, dtype=torch.float32, device=x2.device)
    check(lib.mapx_add_layernorm_bwd_bf16(ptr(dy2), ptr(x2), ptr(s2), ptr(_f32(w, "add_layernorm_bwd: w")),
                                          ptr(_f32(stats, "add_layernorm_bwd: stats")), R, E, ptr(dsum), ptr(part),
                                          stream()))
    for dst, col0 in ((dw, 0), (db, E)):
        if defer:
            defer_sum(dst, part[:, col0:], 2 * E, groups, E)
        else:
            _sum_now(dst, part[:, col0:], 2 * E, groups, E)
    return dsum, dw, db


# --------------------------------------------------------------------------- heads / masks
def bce_with_logits(logits, labels, want_grad=True):
    """-> (out3 = [loss, acc, pos_ratio] f32 device, dlogits or None)."""
    require_gpu(logits, labels)
    logits, labels = logits.contiguous(), labels.contiguous()
    n = logits.numel()
    out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    ws = scratch(lib.mapx_bce_workspace_bytes(), logits.device)
    check(lib.mapx_bce_with_logits(ptr(logits), ptr(labels), n, ptr(dl), ptr(out3), ptr(ws),
                                   ws.numel(), stream()))
    return out3, dl


def eval_metrics(logits, labels):
    """ROC-AUC / log-loss / mean logit / mean probability of an eval pass, computed on the device
    (reference trainer.py:189-199 uses sklearn on host lists).  One host read of 6 doubles.
    -> dict(auc, logloss, avg_logits, avg_probs, positives, negatives)"""
    require_gpu(logits, labels)
    logits = logits.contiguous().view(-1).float()
    labels = labels.contiguous().view(-1).float()
    n = logits.numel()
    if labels.numel() != n:
        raise ValueError(f"eval_metrics: {n} logits but {labels.numel()} labels")
    out = torch.empty(6, dtype=torch.float64, device=logits.device)
    ws = scratch(lib.mapx_eval_metrics_workspace_bytes(n), logits.device)
    check(lib.mapx_eval_metrics(ptr(logits), ptr(labels), n, ptr(out), ptr(ws), ws.numel(), stream()))
    auc, ll, ml, mp, npos, nneg = out.tolist()
    if npos == 0 or nneg == 0:                     # sklearn.metrics.roc_auc_score's behaviour
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return dict(auc=auc, logloss=ll, avg_logits=ml, avg_probs=mp, positives=int(npos), negatives=int(nneg))


SLICE_OUTPUTS = (("rows", torch.int64), ("positives", torch.int64), ("u2", torch.int64),
                 ("sum_prob", torch.float64), ("sum_loss", torch.float64))


def slice_metrics(logits, labels, groups, n_groups, out=None):
    """eval_metrics' quantities per group of a column (include/mapx_hip.h: mapx_slice_metrics).
    groups: int32 or int64 [n] with values in [0, n_groups).  -> (rows i64, positives i64, u2, sum_prob f64,
    sum_loss f64), device tensors of n_groups elements; u2 (twice the group's U statistic, < 2^62) is held as int64.
    AUC_g = u2 / (2 * positives * (rows - positives)); the integers are exact, the sums bitwise reproducible.
    out: the five tensors to write (contiguous, these element types).  A group id outside the range raises ValueError
    naming the first one; one host read of two words."""
    require_gpu(logits, labels, groups)
    G = int(n_groups)
    if not 1 <= G < 2 ** 31:
        raise ValueError(f"slice_metrics: 1 <= n_groups < 2^31 (got {n_groups})")
    if groups.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"slice_metrics: groups is int32 or int64, got {groups.dtype}")
    logits = logits.contiguous().view(-1).float()
    labels = labels.contiguous().view(-1).float()
    groups = groups.contiguous().view(-1)
    n = logits.numel()
    if labels.numel() != n or groups.numel() != n:
        raise ValueError(f"slice_metrics: {n} logits, {labels.numel()} labels, {groups.numel()} group ids")
    if not n < 2 ** 31:
        raise ValueError(f"slice_metrics: at most 2^31 - 1 rows (got {n})")
    dev = logits.device
    if out is None:
        out = tuple(torch.empty(G, dtype=dt, device=dev) for _, dt in SLICE_OUTPUTS)
    out = tuple(out)
    require_gpu(*out)
    if len(out) != 5 or any(o.dtype != dt or o.numel() != G or not o.is_contiguous()
                            for o, (_, dt) in zip(out, SLICE_OUTPUTS)):
        raise TypeError(f"slice_metrics: out is five contiguous tensors of {G} elements: "
                        + ", ".join(f"{k} {str(dt)[6:]}" for k, dt in SLICE_OUTPUTS))
    if n == 0:
        for o in out:
            o.zero_()
        return out
    # (an int64 id beyond int32 stays outside [0, G) when narrowed: G < 2^31)
    g32 = groups if groups.dtype == torch.int32 else groups.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = scratch(lib.mapx_slice_metrics_workspace_bytes(n, G), dev)
    check(lib.mapx_slice_metrics(ptr(logits), ptr(labels), ptr(g32), n, G, *(ptr(o) for o in out), ptr(status),
                                 ptr(ws), ws.numel(), stream()))
    bad, first = status.tolist()
    if bad:
        raise ValueError(f"slice_metrics: {bad} group id(s) outside [0, {G}); the first is {int(groups[first])} "
                         f"at row {first}")
    return out


# floor(2^32 * P(Poisson(1) <= k)), k = 0..11: a 32-bit word's weight is the number of these it reaches
# (csrc/bootstrap.hip: boot_weight; tests/test_bootstrap_host.py recomputes them with 60-digit decimals)
BOOT_POISSON_T = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291,
                  4294609777, 4294923276, 4294962463, 4294966817, 4294967252, 4294967292)
BOOT_MAX_ROWS, BOOT_MAX_REPLICATES = 2 ** 28, 65536
BOOT_OUTPUTS = (("u2", torch.int64), ("pos_w", torch.int64), ("neg_w", torch.int64), ("sum_loss", torch.float64))


def _boot_sizes(name, n, replicates, seed):
    R, seed = int(replicates), int(seed)
    if not 1 <= R <= BOOT_MAX_REPLICATES:
        raise ValueError(f"{name}: 1 <= replicates <= {BOOT_MAX_REPLICATES} (got {replicates})")
    if not n <= BOOT_MAX_ROWS:
        raise ValueError(f"{name}: at most 2^28 rows (got {n})")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{name}: the seed is an unsigned 64-bit integer (got {seed})")
    return R, seed


def _boot_units(name, units, n):
    if units is None:
        return None
    require_gpu(units)
    if units.dtype != torch.int64:
        raise TypeError(f"{name}: units is int64, got {units.dtype}")
    units = units.contiguous().view(-1)
    if units.numel() != n:
        raise ValueError(f"{name}: {n} rows, {units.numel()} units")
    return units


def bootstrap_metrics(logits, labels, replicates, seed=0, units=None, out=None):
    """Poisson bootstrap of eval_metrics' AUC and log-loss (include/mapx_hip.h: mapx_bootstrap_metrics).
    units: int64 [n], the resampling unit of each row (rows of one unit share a weight); None: every row its own.
    -> (u2, pos_w, neg_w i64, sum_loss f64), device tensors of `replicates` elements: per replicate the weighted
    positives and negatives, twice the weighted U statistic (AUC_r = u2 / (2 pos_w neg_w), u2 < 2^63) and the weighted
    sum of the log-loss row terms.  The resample depends on (seed, units) alone, not on the logits: two models scored
    on the same rows with one seed are compared on the same resamples.  The integers are exact, sum_loss bitwise
    reproducible.  out: the four tensors to write (contiguous, these element types).  n = 0 gives zeros."""
    require_gpu(logits, labels)
    logits = logits.contiguous().view(-1).float()
    labels = labels.contiguous().view(-1).float()
    n = logits.numel()
    if labels.numel() != n:
        raise ValueError(f"bootstrap_metrics: {n} logits, {labels.numel()} labels")
    R, seed = _boot_sizes("bootstrap_metrics", n, replicates, seed)
    units = _boot_units("bootstrap_metrics", units, n)
    dev = logits.device
    if out is None:
        out = tuple(torch.empty(R, dtype=dt, device=dev) for _, dt in BOOT_OUTPUTS)
    out = tuple(out)
    require_gpu(*out)
    if len(out) != 4 or any(o.dtype != dt or o.numel() != R or not o.is_contiguous()
                            for o, (_, dt) in zip(out, BOOT_OUTPUTS)):
        raise TypeError(f"bootstrap_metrics: out is four contiguous tensors of {R} elements: "
                        + ", ".join(f"{k} {str(dt)[6:]}" for k, dt in BOOT_OUTPUTS))
    if n == 0:
        for o in out:
            o.zero_()
        return out
    ws = scratch(lib.mapx_bootstrap_workspace_bytes(n, R), dev)
    check(lib.mapx_bootstrap_metrics(ptr(logits), ptr(labels), ptr(units), n, R, seed, *(ptr(o) for o in out),
                                     ptr(ws), ws.numel(), stream()))
    return out


def bootstrap_weights(n_or_units, replicates, seed=0, device="cuda"):
    """-> uint8 [replicates, n]: the weights bootstrap_metrics gives the rows, from the device function its replicate
    kernel calls.  n_or_units: a row count (every row its own unit) or the int64 [n] units.  Test entry, and what a
    host restatement of the resample starts from."""
    if torch.is_tensor(n_or_units):
        n = n_or_units.numel()
        units = _boot_units("bootstrap_weights", n_or_units, n)
        device = units.device
    else:
        n, units = int(n_or_units), None
        if n < 0:
            raise ValueError(f"bootstrap_weights: {n} rows")
    R, seed = _boot_sizes("bootstrap_weights", n, replicates, seed)
    w = torch.empty(R, n, dtype=torch.uint8, device=device)
    require_gpu(w)
    if n:
        check(lib.mapx_bootstrap_weights(ptr(units), n, R, seed, ptr(w), stream()))
    return w


def _check_distinct(name, L, F):
    if L > F:
        raise ValueError(f"{name}: distinct=True draws L distinct fields per row and needs L <= F (L = {L}, F = {F})")


def mask_distinct_keys(B, F, seed, offset, offset_dev=None, device="cuda"):
    """-> int64 [B,F]: the unsigned 32-bit keys of the distinct draw (include/mapx_hip.h, mapx_dynamic_mask_mfp,
    draw = 1), from the device function the mask kernels call.  masked_index of a distinct=True call is
    argsort(keys, stable)[:, :L] for the same (seed, offset, offset_dev, B, F).  Test entry."""
    keys = torch.empty(B, F, dtype=torch.int32, device=device)
    require_gpu(keys)
    check(lib.mapx_mask_distinct_keys(B, F, seed, offset, ptr(offset_dev), ptr(keys), stream()))
    return keys.to(torch.int64) & 0xFFFFFFFF


def dynamic_mask_mfp(ids, L, masked_index=None, seed=0, offset=0, offset_dev=None, sel=None, sel_cursor=None,
                     batch=None, distinct=False):
    """-> (masked ids [B,F], labels [B,L], masked_index [B,L])  (trainer.py:217-232).
    Without `masked_index` the fields are drawn on the device: with replacement (sampling_method "randint"), or
    distinct=True: L distinct fields per row, the ordered prefix of a random permutation ("normal"; needs L <= F).
    `sel` int64 [B]: `ids` is the whole HBM-resident split [N,F] and the batch is its rows sel.
    `sel_cursor` (device int64 scalar) + `batch`: sel is a whole epoch's permutation and the batch is
    sel[*cursor : *cursor + batch] (a captured step walks the epoch without host copies)."""
    require_gpu(ids)
    ids = ids.contiguous()
    distinct = bool(distinct) and masked_index is None
    if distinct:
        _check_distinct("dynamic_mask_mfp", L, ids.shape[1])
    if sel is not None:
        require_gpu(sel)
        sel = sel.contiguous()
        B, F = (sel.numel() if sel_cursor is None else int(batch)), ids.shape[1]
        out = torch.empty(B, F, dtype=torch.int64, device=ids.device)
        labels = torch.empty(B, L, dtype=torch.int64, device=ids.device)
        mi_out = torch.empty(B, L, dtype=torch.int64, device=ids.device)
        mi_in = masked_index.contiguous() if masked_index is not None else None
        keys = torch.empty(B * F, dtype=torch.int32, device=ids.device)
        check(lib.mapx_dynamic_mask_mfp_rows(ptr(ids), ids.shape[0], ptr(sel), sel.numel(), ptr(sel_cursor), B, F, L, ptr(mi_in), seed, offset,
                                             ptr(offset_dev), ptr(out), ptr(labels), ptr(mi_out), ptr(keys), int(distinct),
                                             stream()))
        _keys_of[0], _keys_of[1] = out, keys
        return out, labels, mi_out
    B, F = ids.shape
    out = torch.empty_like(ids)
    labels = torch.empty(B, L, dtype=torch.int64, device=ids.device)
    mi_out = torch.empty(B, L, dtype=torch.int64, device=ids.device)
    mi_in = masked_index.contiguous() if masked_index is not None else None
    keys = torch.empty(B * F, dtype=torch.int32, device=ids.device)
    check(lib.mapx_dynamic_mask_mfp(ptr(ids), B, F, L, ptr(mi_in), seed, offset, ptr(offset_dev), ptr(out),
                                    ptr(labels), ptr(mi_out), ptr(keys), int(distinct), stream()))
    _keys_of[0], _keys_of[1] = out, keys        # Embeddings.forward asks ids_to_i32 for exactly this matrix next
    return out, labels, mi_out


RFD_MODES = {"Unigram": 0, "Uniform": 1, "Whole-Uniform": 2, "Whole-Unigram": 3}


def dynamic_mask_rfd(ids, L, masked_index=None, replace_feat=None, x_train=None, seed=0, offset=0,
                     offset_dev=None, mode="Unigram", idx_low=None, idx_high=None, vocab=0, distinct=False):
    """-> (replaced ids [B,F], labels f32 [B,F], masked_index [B,L])  (trainer.py:233-240).
    distinct=True (no `masked_index`): L distinct fields per row, as in dynamic_mask_mfp."""
    require_gpu(ids)
    ids = ids.contiguous()
    B, F = ids.shape
    distinct = bool(distinct) and masked_index is None
    if distinct:
        _check_distinct("dynamic_mask_rfd", L, F)
    out = torch.empty_like(ids)
    labels = torch.empty(B, F, dtype=torch.float32, device=ids.device)
    mi_out = torch.empty(B, L, dtype=torch.int64, device=ids.device)
    mi_in = masked_index.contiguous() if masked_index is not None else None
    rep = replace_feat.contiguous() if replace_feat is not None else None
    nrows = x_train.shape[0] if x_train is not None else 0
    if mode not in RFD_MODES:
        raise NotImplementedError(mode)                     # trainer.py:261-262
    check(lib.mapx_dynamic_mask_rfd(ptr(ids), B, F, L, ptr(mi_in), ptr(rep), ptr(x_train), nrows,
                                    RFD_MODES[mode], ptr(idx_low), ptr(idx_high), int(vocab), seed, offset,
                                    ptr(offset_dev), ptr(out), ptr(labels), ptr(mi_out), int(distinct), stream()))
    return out, labels, mi_out


# --------------------------------------------------------------------------- optimizer
def make_sched(lr0, lambdas, beta1, beta2):
    """Host (float64) -> device table [T,2] f32 of {step_size_s, lr_s}, s = 1..T."""
    rows = []
    for i, lam in enumerate(lambdas):
        s = i + 1
        lr = lr0 * lam
        rows.append((lr * math.sqrt(1.0 - beta2 ** s) / (1.0 - beta1 ** s), lr))
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


REPLAY_TERMS = 7          # kJ + 1 in csrc/optim.hip


def make_replay_aux(lr0, lambdas, beta1, beta2, wd):
    """Host fp64 tables [17, T+1] of the closed-form replay of zero-gradient AdamW steps
    (csrc/optim.hip: replay_coef): prefix products prod_{i<s}(1 - lr_i*wd), beta1^n, beta2^n, and
    R_i[s] = a_s + q_i / (1 - d_s) * R_i[s+1] for q_i = beta1 * beta2^(-(i+1)/2), i = 0..6, once with
    d_s = lr_s*wd and once with d_s = 0.  a_s and lr_s are the fp32-rounded values the kernels read
    from the schedule table."""
    T = len(lambdas)
    sched = make_sched(lr0, lambdas, beta1, beta2).to(torch.float64)        # fp32 values, as doubles
    a, lr = sched[:, 0].tolist(), sched[:, 1].tolist()
    lr_exact = torch.tensor([lr0 * l for l in lambdas], dtype=torch.float64)
    cum = torch.ones(T + 1, dtype=torch.float64)
    cum[1:] = torch.cumprod(1.0 - lr_exact * wd, 0)
    n = torch.arange(T + 1, dtype=torch.float64)
    rows = [cum, torch.pow(torch.tensor(beta1, dtype=torch.float64), n),
            torch.pow(torch.tensor(beta2, dtype=torch.float64), n)]
    beta = math.sqrt(beta2)
    cum_l = cum.tolist()
    for decay in (True, False):
        for i in range(REPLAY_TERMS):
            q = (beta1 / beta) * beta ** (-i)
            R = [0.0] * (T + 1)
            for s in range(T - 1, -1, -1):
                keep = (cum_l[s + 1] / cum_l[s]) if decay else 1.0     # 1 - d_s, consistent with row 0
                R[s] = a[s] + q / keep * R[s + 1]
            rows.append(torch.tensor(R, dtype=torch.float64))
    return torch.stack(rows).contiguous()


def adamw_dense(p, g, m, v, sched, done, beta1, beta2, eps, wd, shadow=None, seg_off=None, seg_amax=None):
    """`shadow`: bf16 [n] copy of the updated parameters, written by the same kernel (bf16 mode).
    seg_off (int64 [n_params + 1]) / seg_amax (int32 [n_params, 2]): the parameters' magnitude records, raised
    with what this launch writes (fp32 mode: the weights are the next step's GEMM operands)."""
    require_gpu(p, g, m, v, sched, done)
    with _timed("adamw_dense", p.numel() * (28.0 if shadow is None else 30.0)):
        if shadow is None:
            nseg = seg_off.numel() - 1 if (seg_off is not None and seg_amax is not None) else 0
            check(lib.mapx_adamw_dense(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(sched), sched.shape[0],
                                       ptr(done), beta1, beta2, eps, wd, ptr(seg_off) if nseg else None, nseg,
                                       ptr(seg_amax) if nseg else None, stream()))
        else:
            check(lib.mapx_adamw_dense_shadow(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(sched),
                                              sched.shape[0], ptr(done), beta1, beta2, eps, wd, ptr(shadow),
                                              stream()))


def take_rows(src, sel, cursor=None, batch=None, as_f32=False):
    """src[sel[c : c + batch]] for an int64 matrix / vector resident on the device (c = the device scalar `cursor`,
    0 and batch = len(sel) without one): the batch of an RFD / finetune step, cut inside the step.
    as_f32: the values as float32 (the finetune labels: no labels.float() launch behind it)."""
    require_gpu(src, sel)
    if src.dtype != torch.int64 or sel.dtype != torch.int64 or not src.is_contiguous() or not sel.is_contiguous():
        raise TypeError("take_rows: contiguous int64 source and row numbers")
    if cursor is not None and (cursor.dtype != torch.int64 or cursor.numel() != 1 or batch is None):
        raise TypeError("take_rows: the cursor is an int64 device scalar and comes with the batch size")
    B = int(batch) if batch is not None else sel.numel()
    if cursor is None and B > sel.numel():
        raise IndexError(f"take_rows: {B} rows of a list of {sel.numel()}")
    F = 1 if src.dim() == 1 else src.shape[1]
    out = torch.empty((B,) if src.dim() == 1 else (B, F), dtype=torch.float32 if as_f32 else torch.int64,
                      device=src.device)
    if B == 0:
        return out
    check(lib.mapx_take_rows_i64(ptr(src), src.shape[0], F, ptr(sel), sel.numel(), ptr(cursor), B, None if as_f32 else ptr(out),
                                 ptr(out) if as_f32 else None, stream()))
    return out


def step_advance(done, cursor=None, stride=0):
    """*done += 1; `cursor` (int64 device scalar): += stride in the same launch (the batch cursor of a step
    that walks the epoch's permutation, trainer.GraphedStep)."""
    if cursor is not None and (cursor.dtype != torch.int64 or not cursor.is_cuda):
        raise TypeError("step_advance: the cursor is an int64 device scalar")
    check(lib.mapx_step_advance(ptr(done), ptr(cursor), int(stride), stream()))


def _score_cursor(name, cursor):
    if cursor.dtype != torch.int64 or cursor.numel() != 1 or not cursor.is_cuda:
        raise TypeError(f"{name}: the cursor is an int64 device scalar")


def score_block(ids, n_rows, cursor, oov_id, batch, oov_fields):
    """batch [B, F] = rows [*cursor, *cursor + B) of ids (int64 [>= n_rows, F], unit column stride, any row pitch),
    zeros (<pad>) from row n_rows on; oov_fields[r] (uint8 [>= n_rows]) = the fields of row r that hold oov_id[f]
    (include/mapx_hip.h: mapx_score_block).  Everything is preallocated: the launch is one node of a captured step."""
    require_gpu(ids, cursor, oov_id, batch, oov_fields)
    _score_cursor("score_block", cursor)
    B, F = batch.shape
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[1] != F or (F > 1 and ids.stride(1) != 1) or \
            (ids.shape[0] > 1 and ids.stride(0) < F):
        raise TypeError(f"score_block: ids must be int64 [rows, {F}] with unit column stride and a row pitch >= {F}")
    if batch.dtype != torch.int64 or not batch.is_contiguous() or oov_id.dtype != torch.int64 or oov_id.numel() != F \
            or not oov_id.is_contiguous():
        raise TypeError(f"score_block: batch is contiguous int64 [B, {F}], oov_id contiguous int64 [{F}]")
    n_rows = int(n_rows)
    if not 0 <= n_rows <= ids.shape[0] or oov_fields.dtype != torch.uint8 or oov_fields.dim() != 1 \
            or not oov_fields.is_contiguous() or oov_fields.numel() < n_rows:
        raise ValueError(f"score_block: {n_rows} rows of an id matrix of {ids.shape[0]} and oov_fields (uint8) of "
                         f"{oov_fields.numel()}")
    ld = ids.stride(0) if ids.shape[0] > 1 else F
    with _timed("score_block", B * F * 16.0 + B):
        check(lib.mapx_score_block(ids.data_ptr() if n_rows else None, ld, n_rows, ptr(cursor), B, F, ptr(oov_id),
                                   ptr(batch), oov_fields.data_ptr() if n_rows else None, stream()))
    return batch


def score_sink(logits, n_rows, cursor, probs, logits_out):
    """logits_out[r] = logits[i], probs[r] = sigmoid(logits[i]) in fp32 for r = *cursor + i < n_rows (include/mapx_hip.h:
    mapx_score_sink; the sigmoid is the one eval_metrics ranks).  logits: fp32, B elements."""
    require_gpu(logits, cursor, probs, logits_out)
    _score_cursor("score_sink", cursor)
    n_rows = int(n_rows)
    for name, t in (("logits", logits), ("probs", probs), ("logits_out", logits_out)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError(f"score_sink: {name} must be contiguous fp32")
    if n_rows < 0 or probs.numel() < n_rows or logits_out.numel() < n_rows:
        raise ValueError(f"score_sink: {n_rows} rows, probs of {probs.numel()}, logits_out of {logits_out.numel()}")
    B = logits.numel()
    with _timed("score_sink", B * 12.0):
        check(lib.mapx_score_sink(logits.data_ptr() if B else None, n_rows, ptr(cursor), B,
                                  probs.data_ptr() if n_rows else None, logits_out.data_ptr() if n_rows else None,
                                  stream()))


def replay_coef_table(aux, beta1, beta2, done, coef=None):
    """The closed-form replay's coefficients for every gap ending at *done (include/mapx_hip.h:
    mapx_replay_coef_table) -> coef [2, aux_len, 12] f32 (allocated once by the caller, rewritten every step)."""
    require_gpu(aux, done)
    if coef is None:
        coef = torch.zeros(lib.mapx_replay_coef_table_bytes(aux.shape[1]) // 4, dtype=torch.float32, device=aux.device)
    with _timed("replay_coef_table", 0.0):
        check(lib.mapx_replay_coef_table(ptr(aux), aux.shape[1], aux.shape[0], beta1, beta2, ptr(done), ptr(coef),
                                         stream()))
    return coef


def table_adam(p0, m0, v0, wd0, last, sched, done, aux, beta1, beta2, eps, p1=None, m1=None, v1=None,
               wd1=0.0, rows=None, n_rows_dev=None, row_begin=0, n_rows=None, grad0=None, grad1=None,
               rows_may_repeat=False):
    require_gpu(p0, m0, v0, last, sched, done)
    W0 = p0.shape[1]
    if n_rows is None:
        n_rows = rows.numel() if rows is not None else p0.shape[0] - row_begin
    kind = "table_adam_update" if grad0 is not None else ("table_adam_catchup" if rows is not None
                                                           else "table_adam_sweep")
    # m0 / v0 (and m1 / v1) are dense arrays of their own, or the two halves of one record per row (row stride 2 W0 / 2)
    def _rows(t, width):
        if t.dim() == 1:
            return t.data_ptr(), t.stride(0)
        if t.stride(1) != 1 or t.shape[1] != width:
            raise ValueError("table_adam: moment rows must be unit-stride rows of the table's width")
        return t.data_ptr(), t.stride(0)
    (pm0, ld0), (pv0, ldv0) = _rows(m0, W0), _rows(v0, W0)
    if ld0 != ldv0:
        raise ValueError("table_adam: m0 and v0 must share their row stride")
    pm1 = pv1 = None
    ld1 = 1
    if p1 is not None:
        (pm1, ld1), (pv1, ldv1) = _rows(m1, 1), _rows(v1, 1)
        if ld1 != ldv1:
            raise ValueError("table_adam: m1 and v1 must share their stride")
    with _timed(kind, float(n_rows) * (W0 + (1 if p1 is not None else 0)) * 4.0 * 7):
        check(lib.mapx_table_adam(ptr(p0), pm0, pv0, ld0, W0, wd0, ptr(p1), pm1, pv1, ld1, wd1,
                                  ptr(last), ptr(rows), row_begin, n_rows, ptr(n_rows_dev), ptr(grad0),
                                  ptr(grad1), ptr(sched), sched.shape[0], ptr(done), ptr(aux),
                                  aux.shape[1], aux.shape[0], beta1, beta2, eps, int(rows_may_repeat), stream()))


# ----------------------------------------------------------------------------- state fingerprint
FP_CHUNK = 65536            # words per chunk value (include/mapx_hip.h: mapx_fingerprint_words)


def fingerprint_into(t, total, chunks=None, blocks=0):
    """Enqueue the fingerprint of `t` (a contiguous device tensor of a 4-byte dtype) into `total` (one element of an
    int64 device tensor); `chunks`: int64 scratch of at least ceil(numel / FP_CHUNK) elements, allocated when None.
    Nothing is synchronised: the caller reads `total` / `chunks` when it wants them.  -> the chunk values."""
    if not isinstance(t, torch.Tensor) or t.element_size() != 4 or t.is_complex():
        raise TypeError(f"fingerprint: a tensor of a 4-byte dtype, not {getattr(t, 'dtype', type(t))} "
                        "(view or cast it explicitly)")
    require_gpu(t, total)
    if not t.is_contiguous():
        raise ValueError("fingerprint: the tensor must be contiguous (nothing is copied silently)")
    n = t.numel()
    nchunks = (n + FP_CHUNK - 1) // FP_CHUNK
    if chunks is None:
        chunks = torch.empty(nchunks, dtype=torch.int64, device=t.device)
    if total.dtype != torch.int64 or total.numel() != 1 or chunks.dtype != torch.int64 or chunks.numel() < nchunks \
            or not chunks.is_contiguous():
        raise ValueError("fingerprint: `total` is one int64 element, `chunks` contiguous int64 of ceil(n / 65536)")
    with _timed("fingerprint", 4.0 * n):
        check(lib.mapx_fingerprint_words(t.data_ptr() if n else None, n, chunks.data_ptr() if nchunks else None,
                                         total.data_ptr(), int(blocks), stream()))
    return chunks[:nchunks]


def fingerprint(t, chunks=False, blocks=0):
    """Order-independent 64-bit fingerprint of the raw bit patterns of a contiguous device tensor of a 4-byte dtype
    -> Python int in [0, 2^64) (one host sync); chunks=True: also the int64 tensor of the per-chunk values (chunk k
    covers elements [k * FP_CHUNK, (k + 1) * FP_CHUNK)).  blocks: grid size of the chunk launch (0 = auto)."""
    total = torch.empty(1, dtype=torch.int64, device=t.device if isinstance(t, torch.Tensor) else None)
    c = fingerprint_into(t, total, None, blocks)
    f = int(total.item()) & 0xFFFFFFFFFFFFFFFF
    return (f, c) if chunks else f
