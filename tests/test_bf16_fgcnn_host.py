"""compute_dtype=bf16 for FGCNN: what can be checked without a GPU.

(a) models.build_backbone builds FGCNN for MFP / RFD / CTR x {FGCNN, FGCNNShare} in bf16 mode with the fp32 model's
    state dict (names, shapes, dtypes): master weights, tables, batch-norm parameters and buffers stay fp32.
(b) BaseModel.from_config keeps refusing the mode (pinned by tests/test_fgcnn_host.py and
    tests/test_bf16_backbones_host.py), and the model still trains on one replica only.
(c) Options the mode does not build raise when the model is built, naming their flag.
(d) The float64 restatement the GPU tests compare against (tests/bf16_fgcnn_ref.py) reproduces the four committed
    fixtures of the reference's own class, and its bf16 emulation stays inside the caps the GPU tests apply: loss
    within 1e-2, ReLU units and pooling winners of fp32-then-round against float64-then-round within 1 in 1000."""
import functools

import numpy as np
import pytest
import torch

import bf16_fgcnn_ref as GR
import fgcnn_params as fp
import paramgen as pg

CFG = pg.CASES[fp.CASE]
BUILT = [(m, v) for v in fp.VARIANTS for m in ("MFP", "RFD", "CTR")]
FIXTURES = [(m, v) for v in fp.VARIANTS for m in fp.modes_of(v)]


def _config(mode, variant, compute_dtype="bf16", **over):
    cnt = pg.make_inputs(fp.CASE, CFG)["feat_count"] if mode == "MFP" else None
    return fp.make_config(CFG, mode, variant, cnt, compute_dtype=compute_dtype, **over)


# --------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("mode,variant", BUILT)
def test_build_backbone_builds_fgcnn_in_bf16_mode(mode, variant):
    from mapx.models import FGCNN, BaseModel, build_backbone
    model = build_backbone(_config(mode, variant))
    assert isinstance(model, FGCNN) and model.embed.compute_dtype == torch.bfloat16
    assert (model.fg_embed is None) == (variant == "FGCNNShare")
    if model.fg_embed is not None:
        assert model.fg_embed.compute_dtype == torch.bfloat16
    assert all(p.dtype == torch.float32 for p in model.parameters())          # masters, tables, conv / BN parameters
    want = BaseModel.from_config(_config(mode, variant, compute_dtype="fp32")).state_dict()
    got = model.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert got["fgcnn_layer.conv_layers.0.1.running_var"].dtype == torch.float32
    assert got["fgcnn_layer.conv_layers.0.1.num_batches_tracked"].dtype == torch.int64
    if mode == "CTR":
        assert model.fc_out.out_fp32
    elif mode == "MFP":
        assert model.feat_encoder.out_fp32
    else:
        assert model.pred_rfd["2"].out_fp32
    assert "one replica" in model.single_replica_only
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        BaseModel.from_config(_config(mode, variant))


def test_the_fp32_model_is_built_as_before():
    from mapx.models import BaseModel, build_backbone
    a, b = build_backbone(_config("CTR", "FGCNN", compute_dtype="fp32")), \
        BaseModel.from_config(_config("CTR", "FGCNN", compute_dtype="fp32"))
    assert type(a) is type(b) and not a.fc_out.out_fp32 and a.embed.compute_dtype == torch.float32


def test_data_parallel_is_still_refused(monkeypatch, tmp_path):
    from mapx import trainer as T
    from mapx.arguments import TrainingArguments
    from mapx.models import build_backbone
    model = build_backbone(_config("CTR", "FGCNN"))
    targs = TrainingArguments(output_dir=str(tmp_path))
    targs._device = torch.device("cpu")
    monkeypatch.setattr(T.parallel, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="one replica"):
        T.Trainer(model, model.config, targs, None, None)


# --------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("over,flag", [
    (dict(hidden_act="tanh"), "hidden_act"),
    (dict(hidden_dropout_rate=0.1), "hidden_dropout_rate"),
    (dict(embed_norm=True), "embed_norm"),
    (dict(embed_dropout_rate=0.1), "embed_dropout_rate"),
    (dict(embed_size=12), "embed_size"),
], ids=lambda v: "+".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_what_bf16_mode_does_not_build_raises_naming_its_flag(over, flag):
    from mapx.models import build_backbone
    with pytest.raises(NotImplementedError, match=flag):
        build_backbone(_config("CTR", "FGCNN", **over))
    build_backbone(_config("CTR", "FGCNN", compute_dtype="fp32", **over))         # fp32 mode builds every one of them


# --------------------------------------------------------------------------- (d)
@functools.lru_cache(maxsize=None)
def reference(mode, variant, emulate=False):
    """The restatement on the fixture case, free-running (its own ReLU pattern and pooling winners) -> GR.Result."""
    inp = pg.make_inputs(fp.CASE, CFG)
    return GR.step(CFG, mode, variant, fp.make_params(CFG, mode, variant), GR.fixture_batch(mode, CFG, inp),
                   emulate=emulate)


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_restatement_reproduces_the_fixtures(mode, variant):
    z = GR.fixture(mode, variant)
    r = reference(mode, variant)
    e_loss = abs(r.loss - float(z["out/loss"])) / abs(float(z["out/loss"]))
    e_logits = GR.rel(r.logits, z["out/logits"])
    e_comb = GR.rel(r.combined[:fp.MID_ROWS], z["mid/combined"])
    print(f"loss {e_loss:.2e}, logits {e_logits:.2e}, combined {e_comb:.2e} of scale")
    assert e_loss <= 1e-5 and e_logits <= 1e-5 and e_comb <= 1e-5
    for k in fp.bn_buffer_names(CFG, variant):
        if not k.endswith("num_batches_tracked"):
            assert GR.rel(r.buffers[k], z[f"bn/{k}"]) <= 1e-5, k
    ev = GR.eval_logits(CFG, mode, variant, fp.make_params(CFG, mode, variant),
                        GR.fixture_batch(mode, CFG, pg.make_inputs(fp.CASE, CFG)), fp.eval_buffers(CFG, variant))
    if ev is not None:
        assert GR.rel(ev, z["eval/logits"]) <= 1e-5


@pytest.mark.parametrize("mode,variant", FIXTURES)
def test_emulated_bf16_step_stays_inside_the_caps_of_the_gpu_tests(mode, variant):
    """Rounding alone moves the loss by less than 1e-2 (the logits by less than 2e-2 of scale); and the two ways of
    reaching the rounded decisions that the pattern cap of the GPU test compares — an fp32 accumulation rounded to bf16
    (what the kernels do) against a float64 one rounded to bf16 (the emulation) — differ in at most 1 ReLU unit /
    pooling winner in 1000 here."""
    r, e = reference(mode, variant), reference(mode, variant, True)
    e_loss, e_logits = abs(e.loss - r.loss) / abs(r.loss), GR.rel(e.logits, r.logits)
    print(f"[emulation {mode} {variant}] loss {e_loss:.2e}, logits {e_logits:.2e} of scale")
    # (the logits get the per-tensor rule max(1e-2, 2 e_emul) on the GPU, and this figure is their e_emul: CTR logits
    # of scale 0.3 behind an MLP of bf16 activations carry 1.3e-2 of it)
    assert np.isfinite(e.loss) and e_loss <= 1e-2 and e_logits <= 2e-2
    inp = pg.make_inputs(fp.CASE, CFG)
    f32 = GR.step(CFG, mode, variant, fp.make_params(CFG, mode, variant), GR.fixture_batch(mode, CFG, inp),
                  emulate=True, accumulate=torch.float32)
    differ, total = GR.pattern_difference(f32, e)
    print(f"[fp32-then-round vs float64-then-round] {differ} of {total} ReLU units and pooling winners differ")
    assert differ * 1000 <= total
