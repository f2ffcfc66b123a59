"""The host side of the bootstrap, no GPU: the Philox restatement of tests/boot_ref.py on the Random123
vectors, the Poisson thresholds recomputed with 60-digit decimals, the planted weight table of the issue, the mean
weight, mapx.score.bootstrap_report on hand-made arrays, the refusals of python -m mapx.compare and the new flags of
python -m mapx.score."""
import os
import subprocess
import sys
from decimal import Decimal, getcontext

import numpy as np
import pytest

import boot_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_reproduces_the_random123_vectors():
    hexes = lambda words: " ".join(f"{int(w[0]):08x}" for w in words)
    assert hexes(B.philox4x32_10((0, 0), (0, 0, 0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hexes(B.philox4x32_10((ones, ones), (ones,) * 4)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(B.philox4x32_10((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_the_thresholds_are_the_poisson_cdf():
    from mapx import ops
    getcontext().prec = 60
    e_inv = 1 / Decimal(1).exp()
    cdf, fact, want = Decimal(0), Decimal(1), []
    for k in range(12):
        fact *= max(k, 1)
        cdf += e_inv / fact
        want.append(int((cdf * 2 ** 32).to_integral_value(rounding="ROUND_FLOOR")))
    assert tuple(want) == tuple(ops.BOOT_POISSON_T) == B.T and len(ops.BOOT_POISSON_T) == 12
    steps = np.diff([0] + want + [2 ** 32])                              # P(weight = k) * 2^32, k = 0..12
    assert abs(float((steps * np.arange(13)).sum()) / 2 ** 32 - 1.0) < 2e-9


def test_the_planted_weights():
    w = B.weights(np.array([0, 1, 2, 3, 4, 2 ** 40 + 7], dtype=np.int64), 8, 42)
    assert w.dtype == np.uint8 and w.T.tolist() == [
        [1, 0, 1, 1, 0, 1, 0, 3], [1, 0, 0, 2, 2, 3, 0, 4], [0, 4, 0, 2, 0, 1, 0, 0],
        [1, 0, 1, 1, 0, 1, 1, 2], [0, 1, 2, 0, 0, 0, 0, 1], [3, 0, 3, 2, 1, 1, 2, 1]]
    assert np.array_equal(B.weights(5, 8, 42), w[:, :5])                 # a row count: the units are the row numbers
    assert np.array_equal(B.weights(5, 3, 42), w[:3, :5])                # a replicate does not depend on R


def test_the_mean_weight_is_one():
    n, R = 4096, 64
    w = B.weights(n, R, 42)
    mean = float(w.mean())
    print(f"mean weight {mean:.5f}, bound {6 / np.sqrt(n * R):.4f}")
    assert abs(mean - 1.0) <= 6 / np.sqrt(n * R)                         # six standard errors of a unit-variance draw
    assert w.max() <= 12


def _arrays(pos_w, neg_w, auc, loss):
    pos_w, neg_w = np.asarray(pos_w, np.uint64), np.asarray(neg_w, np.uint64)
    u2 = np.round(np.asarray(auc) * 2 * pos_w.astype(np.float64) * neg_w.astype(np.float64)).astype(np.uint64)
    return dict(u2=u2, pos_w=pos_w, neg_w=neg_w,
                sum_loss=np.asarray(loss, np.float64) * (pos_w + neg_w).astype(np.float64))


def test_report_quantiles_and_undefined_replicates():
    from mapx import score
    auc = np.array([0.5, 0.6, 0.7, 0.8, 0.9, 0.0, 0.0])
    a = _arrays([10, 10, 10, 10, 10, 0, 10], [20, 20, 20, 20, 20, 20, 0], auc, [0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
    rep = score.bootstrap_report(a, dict(auc=0.71, logloss=0.61), level=0.5)
    r = rep["auc"]
    assert (r["replicates"], r["undefined"]) == (7, 2) and type(r["replicates"]) is int and type(r["undefined"]) is int
    assert r["point"] == 0.71 and r["mean"] == pytest.approx(0.7) and r["std"] == pytest.approx(np.std(auc[:5], ddof=1))
    lo, hi = np.quantile(auc[:5], [0.25, 0.75])
    assert (r["lo"], r["hi"]) == (pytest.approx(lo), pytest.approx(hi)) and r["lo"] == pytest.approx(0.6)
    assert all(type(r[k]) is float for k in ("point", "mean", "std", "lo", "hi"))
    ll = rep["logloss"]                                                  # defined in all seven: a class may be missing
    assert (ll["replicates"], ll["undefined"]) == (7, 0) and ll["mean"] == pytest.approx(0.7)
    assert (ll["lo"], ll["hi"]) == tuple(pytest.approx(v) for v in np.quantile(np.linspace(0.4, 1.0, 7), [0.25, 0.75]))
    assert "delta" not in rep
    # a replicate without any weight leaves the log-loss undefined too
    b = _arrays([0, 3], [0, 3], [0.0, 0.5], [0.0, 0.3])
    rep = score.bootstrap_report(b, dict(auc=0.5, logloss=0.3))
    assert rep["auc"]["undefined"] == 1 and rep["logloss"]["undefined"] == 1 and rep["logloss"]["lo"] == pytest.approx(0.3)
    assert rep["logloss"]["std"] == 0.0
    none = score.bootstrap_report(_arrays([0], [5], [0.0], [0.2]), dict(auc=0.5, logloss=0.2))["auc"]
    assert none["undefined"] == 1 and np.isnan(none["lo"]) and np.isnan(none["mean"])
    # the default level, and u2 handed over as the int64 the op returns
    c = _arrays([7] * 101, [9] * 101, np.linspace(0.4, 0.6, 101), np.linspace(0.2, 0.3, 101))
    c["u2"] = c["u2"].view(np.int64)
    r = score.bootstrap_report(c, dict(auc=0.5, logloss=0.25))["auc"]
    assert (r["lo"], r["hi"]) == tuple(pytest.approx(v) for v in np.quantile(score.boot_values(c)["auc"], [0.025, 0.975]))
    with pytest.raises(ValueError, match="level"):
        score.bootstrap_report(c, dict(auc=0.5, logloss=0.25), level=1.0)


def test_report_delta_of_two_models():
    from mapx import score
    pw, nw = [10, 12, 8, 0], [20, 18, 22, 30]
    a = _arrays(pw, nw, [0.70, 0.75, 0.65, 0.0], [0.50, 0.52, 0.48, 0.40])
    b = _arrays(pw, nw, [0.65, 0.75, 0.70, 0.0], [0.55, 0.50, 0.49, 0.40])
    rep = score.bootstrap_report(a, dict(auc=0.7, logloss=0.5), level=0.5, other=b, other_point=dict(auc=0.68, logloss=0.52))
    d = rep["delta"]["auc"]
    va, vb = score.boot_values(a)["auc"][:3], score.boot_values(b)["auc"][:3]
    assert d["point"] == pytest.approx(0.02) and (d["replicates"], d["undefined"]) == (4, 1)
    assert d["frac_positive"] == pytest.approx(float(((va - vb) > 0).mean())) == pytest.approx(1 / 3)
    assert d["frac_zero"] == pytest.approx(1 / 3)
    assert (d["lo"], d["hi"]) == tuple(pytest.approx(v) for v in np.quantile(va - vb, [0.25, 0.75]))
    dl = rep["delta"]["logloss"]
    assert dl["undefined"] == 0 and dl["frac_positive"] == pytest.approx(0.25) and dl["frac_zero"] == pytest.approx(0.25)
    assert rep["auc"]["undefined"] == 1 and set(rep) == {"auc", "logloss", "delta"}
    same = score.bootstrap_report(a, dict(auc=0.7, logloss=0.5), other=a, other_point=dict(auc=0.7, logloss=0.5))["delta"]
    assert all(same[k]["frac_zero"] == 1.0 and same[k]["lo"] == same[k]["hi"] == same[k]["point"] == 0.0 for k in same)
    c = _arrays([10, 12, 9, 0], nw, [0.65, 0.75, 0.70, 0.0], [0.55, 0.50, 0.49, 0.40])
    with pytest.raises(ValueError, match="not scored on the same resample"):
        score.bootstrap_report(a, dict(auc=0.7, logloss=0.5), other=c, other_point=dict(auc=0.68, logloss=0.52))


def _compare(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "map-code_amd"), PYTHONIOENCODING="utf-8")
    cmd = [sys.executable, "-m", "mapx.compare", "--a", str(tmp_path / "A"), "--b", str(tmp_path / "B"),
           "--out", str(tmp_path / "C")] + list(extra)
    return subprocess.run(cmd, env=env, capture_output=True, text=True, encoding="utf-8", timeout=120)


def test_compare_refuses_directories_that_do_not_belong_together(tmp_path):
    for d in ("A", "B"):
        os.makedirs(tmp_path / d)
        np.save(tmp_path / d / "logits.npy", np.zeros(6, np.float32))
    done = _compare(tmp_path)
    assert done.returncode == 2 and "error:" in done.stderr and "score one of them with --bootstrap" in done.stderr
    np.save(tmp_path / "A" / "labels.npy", np.array([0, 1, 0, 1, 0, 1], np.uint8))
    np.save(tmp_path / "B" / "labels.npy", np.array([0, 1, 0, 1, 1, 1], np.uint8))
    done = _compare(tmp_path)
    assert done.returncode == 2 and "labels.npy" in done.stderr and "differ" in done.stderr
    os.remove(tmp_path / "B" / "labels.npy")
    np.save(tmp_path / "B" / "logits.npy", np.zeros(5, np.float32))
    done = _compare(tmp_path)
    assert done.returncode == 2 and "6 rows" in done.stderr and "5" in done.stderr
    assert not os.path.exists(tmp_path / "C")
    from mapx import compare
    np.save(tmp_path / "B" / "logits.npy", np.ones(6, np.float32))
    xa, xb, y, units = compare.read_inputs(str(tmp_path / "A"), str(tmp_path / "B"))
    assert y.dtype == np.uint8 and y.tolist() == [0, 1, 0, 1, 0, 1] and units is None and xb.tolist() == [1.0] * 6
    np.save(tmp_path / "u.npy", np.arange(5))
    with pytest.raises(compare.Refusal, match="6 elements"):
        compare.read_inputs(str(tmp_path / "A"), str(tmp_path / "B"), str(tmp_path / "u.npy"))
    rep = dict(delta=dict(auc=dict(point=0.0012, lo=0.0004, hi=0.0021, frac_positive=0.996)))
    assert compare.summary_line(rep, 0.95, 1000) == \
        "AUC a − b = +0.0012 [+0.0004, +0.0021] (95 %, 1000 replicates, a better in 99.6 %)"


BASE = ["--model", "m", "--out", "o", "--model_name", "DCNv2"]
RAW = BASE + ["--raw", "day", "--vocab", "v.json", "--dataset", "avazu"]


def test_the_new_flags_of_the_scoring_command(capsys):
    from mapx import score
    a = score.parse_args(RAW)
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level, a.bootstrap_by) == (None, None, None, None)
    a = score.parse_args(RAW + ["--bootstrap", "1000"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level, a.bootstrap_by) == (1000, 0, 0.95, "@row")
    a = score.parse_args(BASE + ["--data_dir", "d", "--bootstrap", "64", "--bootstrap_seed", "7", "--bootstrap_level",
                                 "0.9", "--bootstrap_by", "device_id", "--group_by", "C1"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level, a.bootstrap_by) == (64, 7, 0.9, "device_id")
    assert score.Bootstrap(64) == score.Bootstrap(64, 0, 0.95, "@row")
    for bad, why in ((["--bootstrap", "0"], "--bootstrap"), (["--bootstrap", "65537"], "at most 65536"),
                     (["--bootstrap_seed", "3"], "goes with --bootstrap"), (["--bootstrap_by", "C1"], "goes with --bootstrap"),
                     (["--bootstrap", "8", "--bootstrap_level", "1.5"], "--bootstrap_level"),
                     (["--bootstrap", "8", "--bootstrap_seed", "-1"], "--bootstrap_seed"),
                     (["--bootstrap", "8", "--bootstrap_by", "nope"], "'nope' is not a field of avazu")):
        with pytest.raises(SystemExit) as e:
            score.parse_args(RAW + bad)
        assert e.value.code == 2 and why in capsys.readouterr().err, bad


def test_bootstrap_without_labels_names_the_reason(capsys):
    from mapx import score
    with pytest.raises(SystemExit) as e:
        score.parse_args(RAW + ["--unlabeled", "--bootstrap", "100"])
    assert e.value.code == 2 and "needs the labels of both classes: no labels" in capsys.readouterr().err
    assert str(score._no_bootstrap("no labels")) == "bootstrap needs the labels of both classes: no labels"
    with pytest.raises(ValueError, match="'nope' is not a field"):
        score.boot_unit_column(score.Bootstrap(8, by="nope"), ["C1", "device_id"])
    assert score.boot_unit_column(score.Bootstrap(8, by="device_id"), ["C1", "device_id"]) == 1
    assert score.boot_unit_column(score.Bootstrap(8), ["C1"]) is None and score.boot_unit_column(None, ["C1"]) is None
