"""run.py with its default --sampling_method ("normal": distinct fields, drawn on the device) through an MFP
pretraining epoch: the run finishes on the captured step and writes its checkpoint."""
import os

import pytest
import torch

import model_harness as H

pytestmark = pytest.mark.gpu


def test_run_py_mfp_pretrain_with_the_default_sampling_method(tmp_path):
    from mapx.dataset import write_synth_dataset
    data = write_synth_dataset(str(tmp_path / "data" / "avazu"), num_rows=6000, num_fields=23, vocab=3000)
    out = str(tmp_path / "out")
    args = ["--pretrain=True", f"--output_dir={out}",
            "--num_train_epochs=1", "--lr_sched=cosine", "--weight_decay=5e-2", "--pt_type=MFP", "--mask_ratio=0.3",
            "--pt_neg_num=25", "--proj_size=32", "--dataset_name=avazu", f"--data_dir={data}",
            "--per_gpu_train_batch_size=512", "--per_gpu_eval_batch_size=512", "--learning_rate=1e-3",
            "--model_name=DCNv2", "--embed_size=16", "--hidden_size=64", "--num_hidden_layers=3",
            "--num_cross_layers=3", "--hidden_dropout_rate=0.0", "--logging_steps=5"]
    assert not any(a.startswith("--sampling_method") for a in args)
    r = H.run_py(args, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    steps = (4800 + 511) // 512
    ckpt = os.path.join(out, f"{steps}.model")
    assert os.path.exists(ckpt) and os.path.exists(os.path.join(out, "results.log"))
    sd = torch.load(ckpt)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    log = open(os.path.join(out, "train.log")).read()
    assert "window_" in log and "eval_" in log and "capture of the mfp step failed" not in log
