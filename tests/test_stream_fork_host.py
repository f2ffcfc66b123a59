"""ops.Fork where no edge can be made (no device, or the side stream is the origin): the body runs in place, `forked`
is False, no record_stream is issued and nothing is left for the optimizer to join."""
import types

import pytest
import torch


@pytest.fixture
def no_record_stream(monkeypatch):
    def refuse(self, stream):
        raise AssertionError("record_stream without a fork")
    monkeypatch.setattr(torch.Tensor, "record_stream", refuse)


def _same_stream():
    st = types.SimpleNamespace(cuda_stream=7)          # what ops.stream_wait compares

    def refuse(*a):
        raise AssertionError("a wait on the stream itself")
    st.wait_stream = st.wait_event = refuse
    return st, types.SimpleNamespace(cuda_stream=7, wait_stream=refuse, wait_event=refuse)


@pytest.mark.parametrize("where", ["no_device", "same_stream", "same_stream_event"])
def test_fork_without_an_edge_runs_in_place(where, no_record_stream):
    from mapx import ops
    x, y = torch.ones(4), torch.zeros(4)
    before = list(ops.pending_joins)
    if where == "no_device":
        fork = ops.Fork(None, None)
    else:
        side, origin = _same_stream()
        fork = ops.Fork(side, origin, event=object() if where == "same_stream_event" else None)
    assert fork.forked is False
    ran = []
    if where == "no_device":                # (entering a stream needs a device; the sites without one pass None)
        with fork as f:
            assert f is fork
            ran.append(float((x + y).sum()))
        assert ran == [4.0]
    fork.reads(x)
    fork.produces(y)
    fork.leave_open()
    assert ops.pending_joins == before
    fork.join()
    assert ops.pending_joins == before
