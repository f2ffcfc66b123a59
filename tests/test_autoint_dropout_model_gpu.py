"""AutoInt with attention dropout (attn_probs_dropout_rate > 0: two Philox sites per attention layer, drawn inside
csrc/attn.hip) at model level: graph replay == eager over Trainer steps, bit-exact resume, evaluation untouched by
the rate, and run.py at the flag default (0.1) from pretraining to finetuning."""
import math
import os

import pytest
import torch

import model_harness as H
from util import make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(F=23, V=300, E=16, H=16, NL=0, NC=0, P=32, K=25)
B = 64


def _config(mode, cnt=None, rate=0.1):
    c = make_config(CFG, mode, cnt, backbone="AutoInt")
    for k, v in dict(num_attn_layers=2, num_attn_heads=2, attn_size=8, res_conn=True, attn_scale=True,
                     attn_probs_dropout_rate=rate).items():
        setattr(c, k, v)
    return c


def _start(mode, data, out_dir, seed=5):
    from mapx.models import BaseModel
    torch.manual_seed(seed)
    config = _config(mode, data[2])
    return H.make_trainer(config, BaseModel.from_config(config), mode, data, out_dir, B, 1, B, begin=True)


@pytest.mark.parametrize("mode", ["MFP", "CTR"])
def test_graph_replay_equals_eager_bitwise(mode, tmp_path):
    """8 steps: 3 eager, then the captured step.  The captured step draws the masks of the eager one (the sites read
    the optimizer's device-side step counter), and the masks advance: every step has another loss."""
    from mapx.layers import MhaDropout
    data = H.synth_data(B * 8, CFG["F"], CFG["V"], seed=3)

    def run(use_graph):
        tr, model, batches = _start(mode, data, str(tmp_path / str(use_graph)))
        tr.use_graph = use_graph
        sites = [m for m in model.modules() if isinstance(m, MhaDropout)]
        assert len(sites) == 4 and all(m.step_counter is tr.optimizer.done for m in sites)
        assert len({m.site for m in sites}) == 4 and all(m.seed == 11 for m in sites)
        losses = [float(tr.run_step(mode.lower(), X, Y)[0]) for X, Y in batches]
        assert len(losses) == 8 and tr.global_step == 8
        assert bool(H.captured(tr)) == use_graph
        tr.optimizer.flush()
        return losses, H.model_state(model)

    (la, _), _ = H.graph_vs_eager(run)
    assert len(set(la)) == len(la) and all(math.isfinite(x) for x in la), la


def test_resume_state_continues_bit_exactly(tmp_path):
    """6 steps == 3 steps + save_training_state + fresh trainer + load_training_state + 3 steps."""
    data = H.synth_data(B * 6, CFG["F"], CFG["V"], seed=4)

    def make():
        tr, _, batches = _start("MFP", data, str(tmp_path), seed=9)
        tr.use_graph = False
        return tr, batches

    H.resume_roundtrip(make, 6, 3, str(tmp_path / "state.pt"))


def test_evaluation_does_not_depend_on_the_rate():
    from mapx.models import BaseModel
    torch.manual_seed(2)
    m1 = BaseModel.from_config(_config("CTR", rate=0.1)).to(DEV)
    m0 = BaseModel.from_config(_config("CTR", rate=0.0)).to(DEV)
    m0.load_state_dict(m1.state_dict())
    ids = torch.from_numpy(H.synth_data(B, CFG["F"], CFG["V"], seed=8)[0]).to(DEV)
    m0.eval()
    m1.eval()
    with torch.no_grad():
        (l0,), (l1,) = m0(input_ids=ids), m1(input_ids=ids)
    assert torch.equal(l0, l1) and bool(torch.isfinite(l1).all())


def test_run_py_autoint_at_the_default_rate_pretrain_then_finetune(tmp_path):
    """--attn_probs_dropout_rate is not passed: the reference's default 0.1 applies."""
    common = ["--model_name=autoint", "--embed_size=16", "--num_attn_layers=2", "--num_attn_heads=2", "--attn_size=8",
              "--res_conn=True", "--logging_steps=3"]
    pretrain, finetune = ["--pt_type=MFP", "--pt_neg_num=25"], ["--use_lr=True"]
    assert not any("attn_probs_dropout_rate" in a for a in common + pretrain + finetune)
    sd, log = H.pretrain_then_finetune(tmp_path, common, pretrain, finetune)
    attn = sorted(k for k in sd if k.startswith("self_attention."))
    assert len(attn) == 2 * 3 and "self_attention.1.W_v.weight" in attn          # (width 16 = 2 x 8: no W_res)
    assert "attn_probs_dropout_rate = 0.1" in open(tmp_path / "out" / "pretrain" / "results.log").read()
    assert [f for f in os.listdir(tmp_path / "out" / "finetune") if f.endswith(".model")]
    for k in attn:
        assert f"Load tensor: {k}," in log, k
    H.finite_metrics(log)          # (eval_loss: the log-loss)
