"""run.py --model_name=trans end to end: MFP pretraining, then finetuning from that checkpoint."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_py(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "map-code_amd", "run.py")] + args
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_run_py_trans_pretrain_then_finetune(tmp_path):
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=4000, num_fields=23, vocab=2000)
    common = ["--dataset_name=avazu", f"--data_dir={data}", "--per_gpu_train_batch_size=512",
              "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3", "--model_name=trans", "--embed_size=16",
              "--hidden_size=16", "--num_hidden_layers=2", "--num_attn_heads=2", "--intermediate_size=64",
              "--hidden_dropout_rate=0.1", "--logging_steps=3"]
    out = str(tmp_path / "out" / "mfp")
    r = _run_py(["--pretrain=True", f"--output_dir={out}", "--num_train_epochs=1", "--lr_sched=cosine",
                 "--weight_decay=5e-2", "--pt_type=MFP", "--sampling_method=randint", "--mask_ratio=0.3",
                 "--pt_neg_num=25", "--proj_size=32"] + common, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = os.path.join(out, f"{(3200 + 511) // 512}.model")
    sd = torch.load(ckpt)
    enc = sorted(k for k in sd if k.startswith("encoder."))
    assert len(enc) == 2 * 12 and "encoder.layers.1.self_attn.in_proj_weight" in enc
    fo = str(tmp_path / "out" / "finetune")
    r2 = _run_py(["--finetune", f"--pretrained_model_path={ckpt}", f"--output_dir={fo}", "--num_train_epochs=1",
                  "--lr_sched=const", "--weight_decay=1e-1", "--output_reduction=attn,fc", "--use_lr=True"] + common,
                 str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-3000:]
    log = open(os.path.join(fo, "results.log")).read()
    for k in enc:
        assert f"Load tensor: {k}," in log, k
    assert "Unmatched tensor in the target model: feat_encoder.weight" in log
    for key in ("eval_auc", "eval_loss"):          # (eval_loss: the log-loss)
        vals = [float(v) for v in re.findall(rf"{key}\W+([-+0-9.eE]+|nan|inf)", log)]
        assert vals and all(math.isfinite(v) for v in vals), (key, vals)
