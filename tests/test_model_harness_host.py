"""The pure checkers of tests/model_harness.py, each on an input it must pass and on inputs it must refuse: a shared
checker that passes silently would weaken every model test at once."""
import types

import pytest
import torch

import model_harness as H


def _state():
    return {"w": torch.arange(6, dtype=torch.float32).view(2, 3) + 0.5, "steps": torch.tensor(3)}


def test_assert_same_state():
    H.assert_same_state(_state(), _state())
    off = _state()
    off["w"].view(torch.int32)[1, 2] ^= 1                    # the last bit of one element
    with pytest.raises(AssertionError, match="w"):
        H.assert_same_state(_state(), off)
    with pytest.raises(AssertionError, match="extra"):
        H.assert_same_state(_state(), dict(_state(), extra=torch.zeros(1)))
    with pytest.raises(AssertionError, match="steps"):
        H.assert_same_state(_state(), {"w": _state()["w"]})


def test_graph_vs_eager_compares_states_and_losses():
    assert H.graph_vs_eager(lambda use_graph: _state())[0].keys() == _state().keys()
    H.graph_vs_eager(lambda use_graph: ([0.5, 0.25], _state()))
    with pytest.raises(AssertionError):
        H.graph_vs_eager(lambda use_graph: ([0.5, 0.25 if use_graph else 0.26], _state()))
    with pytest.raises(AssertionError, match="steps"):
        H.graph_vs_eager(lambda use_graph: dict(_state(), steps=torch.tensor(3 if use_graph else 4)))


def test_grad_bound_failures():
    assert H.grad_bound_failures({"a": 0.9e-2}, {"a": 0.0}) == []
    assert H.grad_bound_failures({"a": 3e-2}, {"a": 2e-2}) == []
    (line,) = H.grad_bound_failures({"ok": 1e-3, "a.weight": 1.1e-2}, {"ok": 0.0, "a.weight": 1e-3})
    assert line.startswith("a.weight:")
    (line,) = H.grad_bound_failures({"ok": 1e-3, "b.bias": float("nan")}, {"ok": 0.0, "b.bias": 1e-3})
    assert line.startswith("b.bias:")


LOG = """epoch 0: eval_auc = 0.7312, eval_loss = 0.4120
epoch 1: eval_auc = 0.7401, eval_loss = 3.98e-01
"""


def test_finite_metrics():
    assert H.finite_metrics(LOG) == {"eval_auc": [0.7312, 0.7401], "eval_loss": [0.4120, 0.398]}
    with pytest.raises(AssertionError, match="eval_loss"):
        H.finite_metrics(LOG.replace("eval_loss", "loss"))
    for bad in ("nan", "inf"):
        with pytest.raises(AssertionError, match="eval_auc"):
            H.finite_metrics(LOG.replace("0.7401", bad))


def test_assert_checkpoint_is_fp32():
    def model():
        m = torch.nn.BatchNorm1d(3)                          # float parameters and buffers, an integer counter
        return m

    good = {k: v.clone() for k, v in model().state_dict().items()}
    assert good["num_batches_tracked"].dtype == torch.int64
    H.assert_checkpoint_is_fp32(good, model())
    for dtype in (torch.bfloat16, torch.float64):
        with pytest.raises(AssertionError):
            H.assert_checkpoint_is_fp32(dict(good, weight=good["weight"].to(dtype)), model())
    with pytest.raises(AssertionError):
        H.assert_checkpoint_is_fp32({k: v for k, v in good.items() if k != "bias"}, model())
    with pytest.raises(AssertionError):
        H.assert_checkpoint_is_fp32(dict(good, shadow=torch.zeros(3)), model())


def test_captured_leaves_out_the_warm_up_counters():
    graph = object()
    assert H.captured(types.SimpleNamespace(_graphs={"mfp": 2, "ctr": 0})) == []
    assert H.captured(types.SimpleNamespace(_graphs={"mfp": graph, "ctr": 1})) == [graph]
