"""The schedule of a training step, pinned: which library entry is launched on which stream, every stream wait and
event, and every record_stream, for the second and third eager steps and for the capture pass + first replay of tiny
trainers that between them reach every side-stream arm (stream_trace.py; DESIGN "The schedule as a fixture").

The fixtures under golden/stream_trace/ are written by `python tests/test_stream_trace_gpu.py --write` on a GPU.  A
change that means to alter the schedule regenerates them and shows the diff; any other change leaves them alone."""
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "stream_trace")
DEV = "cuda"
B = 64

# name -> (backbone, mode, F, compute dtype, hidden dropout, serialize_streams); each reaches one arm:
CASES = {
    "dcnv2_mfp_f8": ("DCNv2", "MFP", 8, "fp32", 0.0, False),        # grouped head, _JoinLink, table gradient late
    "dcnv2_mfp_f32": ("DCNv2", "MFP", 32, "fp32", 0.0, False),      # D = 512: plan-stream arm, layout_on_main
    "dcnv2_mfp_f8_bf16": ("DCNv2", "MFP", 8, "bf16", 0.0, False),   # dense-encoder head: main task + late task
    "dcnv2_mfp_f8_drop": ("DCNv2", "MFP", 8, "fp32", 0.1, False),   # no _JoinLink: tower-stream arm
    "dcnv2_rfd_f8": ("DCNv2", "RFD", 8, "fp32", 0.0, False),
    "dcnv2_ctr_f8": ("DCNv2", "CTR", 8, "fp32", 0.0, False),        # skinny_join_bwd branch of join_bwd_input
    "dnn_mfp_f8": ("DNN", "MFP", 8, "fp32", 0.0, False),            # _sample_early / _plans_and_join
    "fgcnn_mfp": ("fgcnn", "MFP", 23, "fp32", 0.0, False),          # three tables: start_many's chunking
    "dcnv2_mfp_f8_serial": ("DCNv2", "MFP", 8, "fp32", 0.0, True),  # not forked: the inline table gradient
    "dcnv2_mfp_f8_drop_serial": ("DCNv2", "MFP", 8, "fp32", 0.1, True),
}


def _trainer(case, out_dir):
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    backbone, mode, F, dtype, drop, _ = CASES[case]
    V = 2000
    ids, labels, _, _ = synth_table(B * 8, F, V, seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=V).astype(np.float32)
    torch.manual_seed(5)
    if backbone == "fgcnn":
        import fgcnn_params as fp
        from test_fgcnn_model_gpu import SMALL
        config = fp.make_config(dict(F=F, V=V, E=16, H=32, NL=2, NC=0, P=32, K=25), mode, "FGCNN", cnt, **SMALL)
    else:
        from util import make_config
        config = make_config(dict(F=F, V=V, E=16, H=64, NL=2, NC=2, P=32, K=25), mode, cnt, backbone=backbone,
                             compute_dtype=dtype)
    config.hidden_dropout_rate = drop
    model = BaseModel.from_config(config)
    targs = TrainingArguments(output_dir=str(out_dir), per_gpu_train_batch_size=B, per_gpu_eval_batch_size=B,
                              learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2, num_train_epochs=1,
                              pretrain=mode != "CTR", pt_type="RFD" if mode == "RFD" else "MFP",
                              RFD_replace="Unigram", sampling_method="randint", mask_ratio=0.3, seed=11, patience=100)
    targs._device = torch.device(DEV)
    os.makedirs(str(out_dir), exist_ok=True)
    ds = OurDataset(ids, labels)
    tr = Trainer(model, config, targs, ds, ds)
    train = tr._begin("trace")
    model.train()
    return tr, list(train.batches(B, True, tr._generator(), (0, 1), rows=True))


def run_case(case, out_dir):
    """-> {"graphed": the fourth call ran from a captured graph, "steps": [{"seq", "record_stream"}] of steps 2-4}."""
    from mapx import ops
    from stream_trace import split, trace
    serial = CASES[case][5]
    was = ops.serialize_streams
    ops.serialize_streams = serial
    try:
        tr, batches = _trainer(case, out_dir)
        tr.use_graph = not serial               # (the serialized order is the timing passes': eager steps only)
        kind = {"MFP": "mfp", "RFD": "rfd", "CTR": "ctr"}[CASES[case][1]]
        steps = []
        for i, (X, Y) in enumerate(batches[:3 if serial else 4]):
            if i == 0:
                tr.run_step(kind, X, Y)
                continue
            with trace() as entries:
                tr.run_step(kind, X, Y)
            seq, rs = split(entries)
            steps.append({"seq": seq, "record_stream": rs})
        torch.cuda.synchronize()
        graphed = any(not isinstance(g, int) for g in tr._graphs.values())
        tr.optimizer.flush()
    finally:
        ops.serialize_streams = was
    del tr
    gc.collect()
    return {"graphed": graphed, "steps": steps}


def _dump(result, path):
    """One entry per line: a changed schedule reads as a diff."""
    with open(path, "w") as f:
        f.write('{"graphed": %s, "steps": [\n' % json.dumps(result["graphed"]))
        for i, st in enumerate(result["steps"]):
            f.write('{"seq": [\n' + ",\n".join(json.dumps(e) for e in st["seq"]) + '\n],\n"record_stream": [\n'
                    + ",\n".join(json.dumps(e) for e in st["record_stream"]) + "\n]}"
                    + (",\n" if i + 1 < len(result["steps"]) else "\n"))
        f.write("]}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_schedule_of_a_step_matches_its_fixture(case, tmp_path):
    with open(os.path.join(GOLD, case + ".json")) as f:
        want = json.load(f)
    got = run_case(case, tmp_path)
    assert got["graphed"] == want["graphed"] == (not CASES[case][5])
    assert len(got["steps"]) == len(want["steps"])
    for n, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        for i, (a, b) in enumerate(zip(g["seq"], w["seq"])):
            assert a == b, f"call {n + 2}, entry {i}: {a} where the fixture has {b}"
        assert len(g["seq"]) == len(w["seq"]), f"call {n + 2}"
        assert g["record_stream"] == w["record_stream"], f"call {n + 2}: record_stream entries differ"


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "map-code_amd"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    if sys.argv[1:2] != ["--write"]:
        sys.exit("usage: test_stream_trace_gpu.py --write [directory]")
    dest = sys.argv[2] if len(sys.argv) > 2 else GOLD
    os.makedirs(dest, exist_ok=True)
    import tempfile
    for case in sorted(CASES):
        with tempfile.TemporaryDirectory() as tmp:
            result = run_case(case, tmp)
        _dump(result, os.path.join(dest, case + ".json"))
        print(case, "graphed" if result["graphed"] else "eager", [len(s["seq"]) for s in result["steps"]], flush=True)
