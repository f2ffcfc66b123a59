"""The schedule of a step as data (test helper).

`trace()` records, in program order, every kernel-library call and every stream edge that Python code issues while
it is active:

    ("launch", entry name, stream)            a mapx_* entry of native.lib, with the stream current at the call
    ("wait_stream", waiter, waited)           torch.cuda.Stream.wait_stream
    ("record", stream, k)                     torch.cuda.Event.record: the k-th record of this trace
    ("wait_event", waiter, k)                 torch.cuda.Stream.wait_event; k = ordinal of the event's last record
                                              (None: recorded before the trace began)
    ("record_stream", stream, dtype, shape)   torch.Tensor.record_stream

Streams are named: the stream current when the trace begins is "main", a stream of ops._aux_streams takes its key's
name, any other is "s0", "s1", ... by order of first appearance.  The five attributes are put back on exit.
"""
import contextlib

import torch


def split(entries):
    """-> (launches / waits / records in order, sorted record_stream entries): the position of a record_stream
    relative to the launches carries no meaning, its presence does."""
    seq = [list(e) for e in entries if e[0] != "record_stream"]
    rs = sorted(list(e) for e in entries if e[0] == "record_stream")
    return seq, rs


@contextlib.contextmanager
def trace():
    from mapx import native, ops
    entries, names, last_record = [], {torch.cuda.current_stream().cuda_stream: "main"}, {}
    nested = [0]             # Stream.wait_stream is wait_event(record_event()) inside torch: one entry, not two

    def name(st):
        h = st.cuda_stream
        if h not in names:
            for (key, _), aux in ops._aux_streams.items():
                if aux.cuda_stream == h:
                    names[h] = key
                    break
            else:
                names[h] = f"s{sum(1 for v in names.values() if v[0] == 's' and v[1:].isdigit())}"
        return names[h]

    lib = native.lib
    entry_names = [n for n in native.SIGNATURES if n.startswith("mapx_")]
    saved_entries = {n: getattr(lib, n) for n in entry_names}
    saved = (torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record,
             torch.Tensor.record_stream)

    def launcher(n, fn):
        def call(*a):
            entries.append(("launch", n, name(torch.cuda.current_stream())))
            return fn(*a)
        return call

    def wait_stream(self, other):
        entries.append(("wait_stream", name(self), name(other)))
        nested[0] += 1
        try:
            return saved[0](self, other)
        finally:
            nested[0] -= 1

    def wait_event(self, event):
        if not nested[0]:
            k = last_record.get(id(event), (None, None))[1]
            entries.append(("wait_event", name(self), k))
        return saved[1](self, event)

    def record(self, stream=None):
        if not nested[0]:
            k = sum(1 for e in entries if e[0] == "record")
            last_record[id(self)] = (self, k)          # (holds the event: its id cannot be reused inside the trace)
            entries.append(("record", name(stream if stream is not None else torch.cuda.current_stream()), k))
        return saved[2](self) if stream is None else saved[2](self, stream)

    def record_stream(self, stream):
        entries.append(("record_stream", name(stream), str(self.dtype).replace("torch.", ""), list(self.shape)))
        return saved[3](self, stream)

    for n, fn in saved_entries.items():
        setattr(lib, n, launcher(n, fn))
    torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event = wait_stream, wait_event
    torch.cuda.Event.record, torch.Tensor.record_stream = record, record_stream
    try:
        yield entries
    finally:
        for n, fn in saved_entries.items():
            setattr(lib, n, fn)
        (torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record,
         torch.Tensor.record_stream) = saved
