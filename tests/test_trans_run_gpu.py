"""run.py --model_name=trans end to end: MFP pretraining, then finetuning from that checkpoint."""
import pytest

import model_harness as H

pytestmark = pytest.mark.gpu


def test_run_py_trans_pretrain_then_finetune(tmp_path):
    common = ["--model_name=trans", "--embed_size=16", "--hidden_size=16", "--num_hidden_layers=2", "--num_attn_heads=2",
              "--intermediate_size=64", "--hidden_dropout_rate=0.1", "--logging_steps=3"]
    sd, log = H.pretrain_then_finetune(tmp_path, common, ["--pt_type=MFP", "--pt_neg_num=25"],
                                       ["--output_reduction=attn,fc", "--use_lr=True"])
    enc = sorted(k for k in sd if k.startswith("encoder."))
    assert len(enc) == 2 * 12 and "encoder.layers.1.self_attn.in_proj_weight" in enc
    for k in enc:
        assert f"Load tensor: {k}," in log, k
    assert "Unmatched tensor in the target model: feat_encoder.weight" in log
    H.finite_metrics(log)          # (eval_loss: the log-loss)
