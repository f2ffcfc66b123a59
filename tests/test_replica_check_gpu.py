"""mapx.replica.check_replicas with two gloo ranks on the one GPU (tests/replica_worker.py): identical replicas
pass; one ulp in one element on one rank makes EVERY rank raise ReplicaDivergence naming the entry and the rows;
MAPX_REPLICA_CHECK=0 turns the Trainer's checks off."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "replica_worker.py")


def _two_ranks(tmp_path, what, port, **env):
    """One torchrun of two ranks; MAPX_REPLICA_CHECK is at its default unless `env` sets it."""
    base = {k: v for k, v in os.environ.items() if k != "MAPX_REPLICA_CHECK"}
    env = dict(base, **env,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "map-code_amd"), os.path.join(ROOT, "tests"),
                                           os.path.join(ROOT, "tests", "golden")]))
    out = str(tmp_path / "seen")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", port, WORKER, out, what],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (what, r.stderr[-3000:])
    return [json.load(open(f"{out}.{k}")) for k in (0, 1)]


def test_one_ulp_in_a_table_row_is_caught_on_both_ranks(tmp_path):
    from replica_worker import ROW
    seen = _two_ranks(tmp_path, "table", "29561")
    assert all(s["raised"] for s in seen) and seen[0] == seen[1]
    s = seen[0]
    assert s["entry"] == "mfp_criterion.p0" and s["ranks"] == [1] and s["where"] == "after the perturbation"
    assert s["row_lo"] <= ROW < s["row_hi"] and s["row_hi"] - s["row_lo"] <= 65536 // 32 + 1
    assert s["elem_lo"] <= ROW * 32 < s["elem_hi"]


def test_a_dense_moment_alone_is_caught_on_both_ranks(tmp_path):
    seen = _two_ranks(tmp_path, "moment", "29563")
    assert all(s["raised"] for s in seen) and seen[0] == seen[1]
    s = seen[0]
    assert s["entry"] == "dense0.m" and s["ranks"] == [1] and s["row_lo"] is None and s["row_hi"] is None
    assert s["elem_lo"] <= 5 < s["elem_hi"]


def test_trainer_checks_at_the_epoch_end_unless_switched_off(tmp_path):
    from replica_worker import TRAINER_ROW
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    off = _two_ranks(tmp_path / "off", "trainer", "29565", MAPX_REPLICA_CHECK="0")
    assert [s["raised"] for s in off] == [False, False]
    on = _two_ranks(tmp_path / "on", "trainer", "29567")
    assert all(s["raised"] for s in on) and on[0] == on[1]
    s = on[0]
    assert s["entry"] == "mfp_criterion.p0" and s["ranks"] == [1] and s["where"].startswith("MFP_pretrain epoch 0")
    assert s["row_lo"] <= TRAINER_ROW < s["row_hi"] and s["row_lo"] == 65536 // 32
