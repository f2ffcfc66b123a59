"""Compare two scored checkpoints on the same rows: a paired Poisson bootstrap of AUC and log-loss.

    python -m mapx.compare --a SDIR_A --b SDIR_B [--replicates 1000] [--seed 0] [--level 0.95] [--units FILE.npy]
                           --out DIR

SDIR_A / SDIR_B are output directories of python -m mapx.score on the same input; at least one of them was written
with --bootstrap, which leaves labels.npy.  Both models are resampled with the same seed and units
(ops.bootstrap_metrics twice: the weight of a row depends on the seed, its unit and the replicate alone),
so every replicate compares the two on the same resample.  --units: an int64 [N] file, for instance a boot_units.npy;
default: every row its own unit.  Writes DIR/compare.json (both reports and the delta a - b: mapx.score.bootstrap_report)
and DIR/compare.npz (the four arrays of each model), and prints one line.  Exit code 2 when the directories do not
belong together."""
import argparse
import json
import os
import sys

import numpy as np

from .preprocess import _positive


class Refusal(Exception):
    pass


def parser():
    p = argparse.ArgumentParser(prog="python -m mapx.compare", allow_abbrev=False, description=__doc__.split("\n\n")[0])
    p.add_argument("--a", required=True, help="output directory of mapx.score for the first model")
    p.add_argument("--b", required=True, help="... for the second model, on the same rows")
    p.add_argument("--out", required=True, help="directory for compare.json and compare.npz")
    p.add_argument("--replicates", type=_positive, default=1000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--level", type=float, default=0.95)
    p.add_argument("--units", metavar="FILE.npy", help="int64 [N]: the resampling unit of each row (default: the row)")
    return p


def read_inputs(a, b, units=None):
    """-> (logits a, logits b, labels u8, units int64 | None), or Refusal with the reason."""
    logits = []
    for d in (a, b):
        path = os.path.join(d, "logits.npy")
        if not os.path.isfile(path):
            raise Refusal(f"{path} is missing: {d} is not an output directory of mapx.score")
        logits.append(np.ascontiguousarray(np.load(path), dtype=np.float32).ravel())
    if len(logits[0]) != len(logits[1]):
        raise Refusal(f"{a} holds {len(logits[0])} rows and {b} holds {len(logits[1])}: not the same input")
    labels = [np.load(os.path.join(d, "labels.npy")) for d in (a, b) if os.path.isfile(os.path.join(d, "labels.npy"))]
    if not labels:
        raise Refusal(f"neither {a} nor {b} holds labels.npy; score one of them with --bootstrap")
    if len(labels) == 2 and not np.array_equal(labels[0], labels[1]):
        raise Refusal(f"labels.npy of {a} and of {b} differ: not the same input")
    y = np.ascontiguousarray(labels[0]).ravel().astype(np.uint8)
    if len(y) != len(logits[0]):
        raise Refusal(f"labels.npy holds {len(y)} rows, logits.npy {len(logits[0])}")
    u = None
    if units is not None:
        u = np.ascontiguousarray(np.load(units)).ravel()
        if u.dtype.kind not in "iu" or len(u) != len(y):
            raise Refusal(f"{units}: an integer array of {len(y)} elements (got {u.dtype} [{len(u)}])")
        u = u.astype(np.int64)
    return logits[0], logits[1], y, u


def compare(xa, xb, y, units=None, replicates=1000, seed=0, level=0.95, device="cuda"):
    """-> (report: {a, b, delta}, arrays: {a: the four, b: the four}); ValueError when a class is missing."""
    import torch
    from . import ops, score
    dy = torch.from_numpy(y.astype(np.float32)).to(device)
    du = None if units is None else torch.from_numpy(units).to(device)
    point, arrays = {}, {}
    for k, x in (("a", xa), ("b", xb)):
        dx = torch.from_numpy(x).to(device)
        point[k], why = score.metrics_of(dx, dy)
        if point[k] is None:
            raise ValueError(f"the comparison needs the labels of both classes: {why}")
        arrays[k] = score.boot_arrays(ops.bootstrap_metrics(dx, dy, replicates, seed=seed, units=du))
    rep = score.bootstrap_report(arrays["a"], point["a"], level, other=arrays["b"], other_point=point["b"])
    delta = rep.pop("delta")
    return dict(a=rep, b=score.bootstrap_report(arrays["b"], point["b"], level), delta=delta), arrays


def summary_line(report, level, replicates):
    d = report["delta"]["auc"]
    return (f"AUC a − b = {d['point']:+.4f} [{d['lo']:+.4f}, {d['hi']:+.4f}] ({100 * level:g} %, {replicates} replicates, "
            f"a better in {100 * d['frac_positive']:.1f} %)")


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not 0.0 < args.level < 1.0:
        p.error("--level: between 0 and 1")
    if not 0 <= args.seed < 2 ** 64:
        p.error("--seed: an unsigned 64-bit integer")
    if args.replicates > 65536:
        p.error("--replicates: at most 65536")
    try:
        xa, xb, y, units = read_inputs(args.a, args.b, args.units)
    except Refusal as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mapx.compare runs on an MI355X only (no CPU path)")
    from . import score
    try:
        report, arrays = compare(xa, xb, y, units, args.replicates, args.seed, args.level, torch.device("cuda", 0))
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    os.makedirs(args.out, exist_ok=True)
    np.savez(os.path.join(args.out, "compare.npz"), seed=np.uint64(args.seed), level=np.float64(args.level),
             **{f"{m}_{k}": v for m, four in arrays.items() for k, v in four.items()})
    doc = dict(report, a_dir=args.a, b_dir=args.b, rows=int(len(y)), replicates=args.replicates, seed=args.seed,
               level=args.level, units=args.units)
    with open(os.path.join(args.out, "compare.json"), "w") as f:
        json.dump(score._json_safe(doc), f, indent=1, allow_nan=False)
    line = summary_line(report, args.level, args.replicates)
    try:
        print(line)
    except UnicodeEncodeError:                       # (a terminal that cannot show the minus sign)
        print(line.replace("−", "-"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
