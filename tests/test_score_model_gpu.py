"""mapx.score.Scorer on the golden CTR cases (DCNv2 and DeepFM, loaded from a saved {step}.model): the fixture's
logits, the captured step against the eager one, the tail batch, independence of how the stream is cut, metrics, and
one bf16-mode case."""
import numpy as np
import pytest
import torch

from util import build_model, load_case, make_config, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE = "B_f25_b64"
_SAVED = {}


def _checkpoint(tmp_path_factory, backbone):
    """The fixture's parameters as a {step}.model on disk, once per backbone."""
    if backbone not in _SAVED:
        cfg, z, inp, params = load_case(CASE, "CTR", backbone)
        model = build_model(cfg, "CTR", params, None, device="cpu", backbone=backbone)
        path = str(tmp_path_factory.mktemp(f"ckpt_{backbone}") / "7.model")
        torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, path)
        _SAVED[backbone] = (path, cfg, z, inp)
    return _SAVED[backbone]


def _scorer(tmp_path_factory, backbone, B, compute_dtype="fp32", **kw):
    from mapx import score
    from mapx.models import build_backbone
    path, cfg, z, inp = _checkpoint(tmp_path_factory, backbone)
    model = build_backbone(make_config(cfg, "CTR", backbone=backbone, compute_dtype=compute_dtype))
    score.load_checkpoint(model, path, input_size=cfg["V"])
    return score.Scorer(model.to(DEV), B, DEV, **kw), z, inp


def _rows(inp, n, seed=3):
    """n rows drawn from the fixture's 64 (the first 64 as they are) and their labels."""
    ids, y = inp["input_ids"], inp["y"]
    pick = np.concatenate([np.arange(min(n, len(ids))), np.random.RandomState(seed).randint(0, len(ids), max(0, n - len(ids)))])
    return t(ids[pick], DEV), t(np.asarray(y)[pick], DEV)


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32)
                           if y.dtype == torch.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("backbone", ["DCNv2", "DeepFM"])
def test_scorer_gives_the_fixtures_logits(tmp_path_factory, backbone):
    """The bound of tests/test_model_gpu.py for the same logits: rtol 1e-5, atol 1e-5."""
    sc, z, inp = _scorer(tmp_path_factory, backbone, 64)
    ids, y = _rows(inp, 64)
    s, metrics = sc.score(ids, y)
    np.testing.assert_allclose(s.logits.cpu().numpy(), z["out/logits"].reshape(-1), rtol=1e-5, atol=1e-5)
    x = s.logits.double()
    np.testing.assert_allclose(s.probs.cpu().numpy(), torch.sigmoid(x).cpu().numpy(), rtol=1e-6, atol=0)
    assert s.oov_fields.dtype == torch.uint8 and int(s.oov_fields.sum()) == 0        # no <oov> id was named
    from mapx import ops
    assert metrics == ops.eval_metrics(s.logits, y)                                 # the reported metrics, exactly


@pytest.mark.parametrize("backbone,compute_dtype", [("DCNv2", "fp32"), ("DeepFM", "fp32"), ("DCNv2", "bf16")])
def test_replay_is_bit_equal_to_the_eager_path(tmp_path_factory, monkeypatch, backbone, compute_dtype):
    B, N = 16, 10 * 16 + 3
    monkeypatch.setenv("MAPX_GRAPH", "0")
    eager, z, inp = _scorer(tmp_path_factory, backbone, B, compute_dtype, stage_batches=4)
    monkeypatch.setenv("MAPX_GRAPH", "1")
    graphed, _, _ = _scorer(tmp_path_factory, backbone, B, compute_dtype, stage_batches=4)
    assert not eager.use_graph and graphed.use_graph
    ids, _ = _rows(inp, N)
    a, b = eager.score(ids), graphed.score(ids)
    assert eager.graph is None and eager.replays == 0
    assert graphed.graph is not None and graphed.replays == 11 - graphed.GRAPH_AFTER  # the tail batch replays it too
    assert a.logits.shape == (N,) and _same(a, b)
    assert int(graphed.done) == 11 and int(eager.done) == 11


def test_tail_rows_are_scored_and_nothing_is_written_past_them(tmp_path_factory):
    B = 16
    N = 2 * B + 3
    sc, z, inp = _scorer(tmp_path_factory, "DCNv2", B, stage_batches=4)
    whole, _, _ = _scorer(tmp_path_factory, "DCNv2", N)                               # the same rows, batches of their own
    ids, _ = _rows(inp, N)
    for buf, fill in ((sc.out_logits, -5.0), (sc.out_probs, -5.0), (sc.out_oov, 0xEE)):
        buf.fill_(fill)
    s = sc.score(ids)
    assert s.logits.shape == s.probs.shape == s.oov_fields.shape == (N,)
    # the staging outputs: two batches at the front, the three tail rows at the very end, nothing in between
    quiet = slice(2 * B, 4 * B - 3)
    assert bool((sc.out_logits[quiet] == -5.0).all()) and bool((sc.out_probs[quiet] == -5.0).all())
    assert bool((sc.out_oov[quiet] == 0xEE).all())
    assert torch.equal(sc.out_logits[4 * B - 3:], s.logits[2 * B:]) and torch.isfinite(s.logits).all()
    # the same rows scored as ONE batch of N: other batch mates, so other per-batch magnitudes and other roundings,
    # but each side lies within the fixture bound (rtol = atol = 1e-5) of the exact logits: twice that between them
    ref = whole.score(ids)
    np.testing.assert_allclose(s.logits.cpu().numpy(), ref.logits.cpu().numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("backbone", ["DCNv2", "DeepFM"])
def test_scores_do_not_depend_on_how_the_stream_is_cut(tmp_path_factory, backbone):
    B = 16
    N = 5 * B + 3
    sc, z, inp = _scorer(tmp_path_factory, backbone, B, stage_batches=2)
    ids, _ = _rows(inp, N)
    base = sc.score(ids)
    for piece in (1, 7, B - 1, B + 1):
        parts = [sc.push(ids[r:r + piece]) for r in range(0, N, piece)] + [sc.finish()]
        got = [torch.cat(p) for p in zip(*parts)]
        assert got[0].shape == (N,) and _same(base, got), piece


def test_bf16_scorer_matches_the_fp32_one(tmp_path_factory):
    """The bound of tests/test_bf16_backbone_models_gpu.py for logits: 1e-2 of the tensor's scale (bf16_backbones_ref.rel)."""
    from bf16_backbones_ref import rel
    f32, z, inp = _scorer(tmp_path_factory, "DCNv2", 64)
    b16, _, _ = _scorer(tmp_path_factory, "DCNv2", 64, "bf16")
    assert b16.weights.bf16 and not f32.weights.bf16
    ids, _ = _rows(inp, 64)
    a, b = f32.score(ids), b16.score(ids)
    e = rel(b.logits.cpu().numpy(), a.logits.cpu().numpy())
    print(f"bf16 scorer logits: {e:.2e} of scale")
    assert e <= 1e-2
