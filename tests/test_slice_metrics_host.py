"""The host side of the sliced evaluation (mapx/score.py): slice_report on hand-made arrays, field -> (column, base,
groups) from a small meta, the @oov pseudo-column, the parser's refusals.  No GPU."""
import math

import numpy as np
import pytest

from mapx import score
from slice_metrics_ref import reference, u2_of

META = {"field_names": ["<rsv>", "C1", "site", "hour"],
        "feat_map": {**{f"<t{i}>": i for i in range(10)},
                     "C1-1005": 10, "C1-1002": 11, "C1-<oov>": 12,
                     "site-ab": 13, "site-<oov>": 14,
                     "hour-0": 15, "hour-1": 16, "hour-2": 17, "hour-<oov>": 18}}
NAMES = ["C1", "site", "hour"]
FLAGS = ["--model", "m", "--out", "o", "--model_name", "DCNv2"]
RAW = FLAGS + ["--raw", "r", "--vocab", "v", "--dataset", "avazu"]


def test_report_of_a_hand_made_column():
    # group 0: 3 rows, 1 positive, below one negative and tied with the other: 2U = 1
    # group 1: empty; group 2: 5 rows, all positive (one class); group 3: 5 rows, 2 positives, 2U = 8 of 12
    rows, pos = [3, 0, 5, 5], [1, 0, 5, 2]
    r = score.slice_report(rows, pos, [1, 0, 0, 8], [1.5, 0.0, 4.0, 2.0], [0.9, 0.0, 0.5, 2.0], top=10,
                           names=["a", "b", "c", "d"])
    assert r["groups"] == 3 and r["gauc_rows"] == 8
    assert r["gauc"] == pytest.approx((3 * (1 / 4) + 5 * (8 / 12)) / 8, rel=1e-15)
    assert [t["group"] for t in r["top"]] == [2, 3, 0]                   # by rows; the tie of 2 and 3 by group id
    assert [t["name"] for t in r["top"]] == ["c", "d", "a"]
    c, d, a = r["top"]
    assert math.isnan(c["auc"]) and c["ctr"] == 1.0 and c["mean_prob"] == 0.8 and c["calibration"] == 0.8
    assert d["auc"] == pytest.approx(8 / 12, rel=1e-15) and d["logloss"] == 0.4 and d["calibration"] == 1.0
    assert a["auc"] == 0.25 and a["rows"] == 3 and a["positives"] == 1 and a["mean_prob"] == 0.5
    assert a["calibration"] == pytest.approx(1.5, rel=1e-15) and a["logloss"] == pytest.approx(0.3, rel=1e-15)
    assert [t["group"] for t in score.slice_report(rows, pos, [1, 0, 0, 8], [1.5, 0, 4, 2], [1, 0, 1, 2], top=1)["top"]] == [2]
    assert score.slice_report(rows, pos, [1, 0, 0, 8], [1.5, 0, 4, 2], [1, 0, 1, 2], top=0)["top"] == []


def test_report_when_no_group_holds_both_classes():
    r = score.slice_report([2, 3, 0], [2, 0, 0], [0, 0, 0], [1.0, 0.3, 0.0], [0.2, 0.1, 0.0])
    assert r["gauc_rows"] == 0 and r["gauc"] is None and r["groups"] == 2
    assert all(math.isnan(t["auc"]) for t in r["top"]) and len(r["top"]) == 2
    assert math.isnan(r["top"][0]["calibration"]) and r["top"][0]["group"] == 1      # ctr 0: no calibration ratio
    assert score._json_safe(r)["top"][0]["auc"] is None


def test_report_takes_u2_beyond_int64_and_the_reference_counts_ties_as_one():
    big = np.array([2 ** 63 + 2 ** 11], dtype=np.uint64)
    r = score.slice_report([2 ** 32], [2 ** 31], big, [1.0], [1.0], top=1)
    assert r["top"][0]["auc"] == float(big[0]) * 0.5 / (2.0 ** 31 * 2.0 ** 31)
    bits, y = np.array([5, 5, 7, 3], dtype=np.uint32), np.array([True, False, False, True])
    assert u2_of(bits, y) == 1                                           # one tie; the other three pairs are lost
    ref = reference(np.array([0.0, 0.0, 1.0, -1.0], np.float32), y, [1, 1, 1, 1], 3)
    assert ref["u2"].tolist() == [0, 1, 0] and ref["rows"].tolist() == [0, 4, 0] and ref["positives"].tolist() == [0, 2, 0]


def test_field_to_column_base_and_groups_from_a_meta():
    oov = score.oov_ids_of(META, NAMES)
    assert oov == [12, 14, 18]
    cols = score.group_columns(["hour", "C1", "@oov", "site"], NAMES, oov, 10)
    assert cols == [("hour", 2, 15, 4), ("C1", 0, 10, 3), ("@oov", None, 0, 4), ("site", 1, 13, 2)]
    assert score.group_names(cols[0], META["feat_map"]) == ["0", "1", "2", "<oov>"]
    assert score.group_names(cols[1], META["feat_map"]) == ["1005", "1002", "<oov>"]
    assert score.group_names(cols[2], META["feat_map"]) == ["0", "1", "2", "3"]
    with pytest.raises(ValueError, match="'C2' is not a field"):
        score.group_columns(["C2"], NAMES, oov, 10)
    with pytest.raises(ValueError, match="twice"):
        score.group_columns(["C1", "C1"], NAMES, oov, 10)
    with pytest.raises(ValueError, match="no id range"):
        score.group_columns(["site"], NAMES, [12, -1, 18], 10)


def test_parser_takes_group_by_and_refuses_what_cannot_be_sliced(capsys):
    args = score.parse_args(RAW + ["--group_by", "C1,site_id,@oov", "--top", "5"])
    assert args.group_by == ["C1", "site_id", "@oov"] and args.top == 5
    args = score.parse_args(RAW)
    assert args.group_by is None and args.top == 20
    assert score.parse_args(FLAGS + ["--data_dir", "d", "--group_by", "anything"]).group_by == ["anything"]
    for extra, why in ((["--group_by", "C1,nope"], "'nope' is not a field"),
                       (["--group_by", "click"], "'click' is not a field"),
                       (["--group_by", "C1,C1"], "twice"),
                       (["--group_by", "C1", "--unlabeled"], "--unlabeled"),
                       (["--group_by", "C1", "--top", "0"], "--top")):
        with pytest.raises(SystemExit):
            score.parse_args(RAW + extra)
        assert why in capsys.readouterr().err, extra
