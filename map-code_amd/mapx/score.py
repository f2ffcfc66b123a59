"""Score a checkpoint on new data: a raw file, or a dataset directory, to per-row click probabilities.

    python -m mapx.score --model OUT/1234.model --vocab DIR/avazu-meta.json --dataset avazu --raw day11.gz
                         [--unlabeled] --out SDIR [--batch_size 4096] [--chunk_mb 256] <run.py's model flags>
    python -m mapx.score --model OUT/1234.model --data_dir DIR --dataset_name avazu [--split test|valid|train|all]
                         --out SDIR <run.py's model flags>
    either form: [--group_by C1,site_id,@oov [--top 20]]   sliced evaluation (labels of both classes needed)
    either form: [--bootstrap 1000 [--bootstrap_seed 0] [--bootstrap_level 0.95] [--bootstrap_by device_id|@row]]

writes SDIR/probs.npy (f32 [N]), logits.npy (f32 [N]), oov_fields.npy (u8 [N]: the fields of a row that took their
field's <oov> id) and score.json, rows in file order.  One device; no optimizer, no labels needed.

A scoring step is  mapx_score_block -> the model's forward -> mapx_score_sink -> mapx_step_advance  (csrc/score.hip),
captured as one hipGraph after a few eager steps and replayed with nothing but the device-side cursor changing
(`Scorer`; MAPX_GRAPH=0 keeps the eager loop).  Batches are ALWAYS the rows [kB, (k+1)B) of the input stream, however
the caller cuts the stream into pieces: fp32-mode products cut their activations at a per-batch magnitude, so a
row's bits depend on its batch mates.

--group_by adds, per named field (and '@oov': the rows by their count of <oov> fields), AUC / log-loss / CTR /
calibration per value and GAUC, the rows-weighted mean of the per-value AUCs: slices.json, slices_<name>.npz and
score.json's "slices" (ops.slice_metrics, csrc/slice_metrics.hip: one launch sequence per column).

--bootstrap R adds Poisson-bootstrap intervals of AUC and log-loss from R resamples of the rows (or of the values of a
field: --bootstrap_by, the cluster bootstrap): bootstrap.json, bootstrap.npz, labels.npy[, boot_units.npy], score.json's
"bootstrap", and with --group_by the listed groups' intervals (ops.bootstrap_metrics, csrc/bootstrap.hip; DESIGN
§4.17).  python -m mapx.compare compares two such directories on the same resamples."""
import argparse
import json
import logging
import os
import sys
import time
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .arguments import EXTENSION_MODEL_FLAGS, MODEL_FLAGS, Config, add_flags
from .optim import MapxOptimizer
from .preprocess import _positive

logger = logging.getLogger(__name__)

Scores = namedtuple("Scores", "logits probs oov_fields")


# ------------------------------------------------------------------------------- batches of a stream cut anywhere
class Batcher:
    """Pure host arithmetic over row counts: a stream arrives in pieces of any size and is scored in batches that are
    always its rows [kB, (k+1)B).  The rows wait in a staging area of `cap` rows (a multiple of B); push(n) and
    finish() return what to do with it, in order:

        ("load", lo, hi, dst)        staging[dst : dst + hi - lo] = piece[lo : hi]
        ("run", row, batches, rows)  cursor = row; `batches` steps; results = the staging outputs [row, row + rows)
        ("move", src, n, dst)        staging[dst : dst + n] = staging[src : src + n]

    A remainder below B is carried to the front of the staging area and waits for the next piece; finish() puts it at
    the END of the area, where the block kernel pads the batch with <pad> rows behind the area's last row."""

    def __init__(self, batch_size, cap):
        if batch_size < 1 or cap < batch_size or cap % batch_size:
            raise ValueError(f"Batcher: a staging area of {cap} rows for batches of {batch_size}")
        self.B, self.cap, self.held, self.rows_in, self.rows_out = int(batch_size), int(cap), 0, 0, 0

    def push(self, n):
        todo, pos = [], 0
        self.rows_in += n
        while pos < n:
            take = min(self.cap - self.held, n - pos)
            todo.append(("load", pos, pos + take, self.held))
            pos += take
            have = self.held + take
            full = have // self.B
            if full:
                todo.append(("run", 0, full, full * self.B))
                self.rows_out += full * self.B
                if have > full * self.B:
                    todo.append(("move", full * self.B, have - full * self.B, 0))
            self.held = have - full * self.B
        return todo

    def finish(self):
        todo = []
        if self.held:
            todo.append(("move", 0, self.held, self.cap - self.held))
            todo.append(("run", self.cap - self.held, 1, self.held))
            self.rows_out += self.held
            self.held = 0
        return todo


# ------------------------------------------------------------------------------- frozen weights
class FrozenWeights(MapxOptimizer):
    """What a training step re-derives through the optimizer, derived ONCE for weights nobody updates: the dense
    parameters in a flat buffer with their bf16 shadows (bf16 mode) or magnitude records and weight planes (fp32 mode),
    through MapxOptimizer's own _flatten / refresh_bf16 — a forward then runs the arithmetic of a forward inside a
    training run (Trainer.eval behind an optimizer).  No schedule, no table moments, no step()."""

    def __init__(self, model):
        from .layers import compute_dtype_of
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("mapx.score needs the model on the GPU (call model.to(device) first)")
        table_ids = model.table_parameter_ids()
        named = [(n, p) for n, p in model.named_parameters() if id(p) not in table_ids and p.requires_grad]
        self.dense_params = [p for _, p in named]
        self.bf16 = compute_dtype_of(getattr(model, "config", None)) == torch.bfloat16
        self.steps_done = 0
        self.groups = [self._flatten(named, 0.0, dev, self.bf16)] if named else []
        for g in self.groups:
            g["g"] = g["m"] = g["v"] = None              # (nothing here takes a gradient or an update)
        for p in self.dense_params:
            p._mapx_grad = None
            if getattr(p, "_planes", None) is not None:
                p._planes_clock = self._clock
        self.tables = []
        self.refresh_bf16()

    def step(self):
        raise RuntimeError("FrozenWeights: the weights of a scoring run are not updated")


# ------------------------------------------------------------------------------- the scorer
class Scorer:
    """Scores rows of ids with a model in finetune (CTR) configuration from build_backbone, on its device.

    push(ids) / finish() take a stream in pieces (int64 [n, F] on the device) and return Scores(logits f32, probs f32,
    oov_fields u8) of the rows whose batch is complete, in stream order (the remainder at finish()); score(ids) is
    push + finish for a whole input.  stage_batches: batches of staging area on the device (the graph reads its rows
    there: one copy of the piece, no copy per batch).  oov_id: int64 [F], the <oov> id of every field (default: none)."""

    GRAPH_AFTER = 3            # eager steps before the capture (allocator / workspace warm-up), as Trainer.run_step

    def __init__(self, model, batch_size, device=None, oov_id=None, stage_batches=64):
        cfg = model.config
        if getattr(cfg, "pretrain", False):
            raise ValueError("Scorer: the model is in pretraining configuration (pretrain=True): it has no CTR head")
        if batch_size < 1 or stage_batches < 1:
            raise ValueError("Scorer: batch_size and stage_batches are at least 1")
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        if self.device.type != "cuda":
            raise ops.N.MapxError("mapx.score runs on the device (HIP); there is no CPU path")
        self.model = model.to(self.device).eval()
        self.B, self.F = int(batch_size), int(cfg.num_fields)
        if not 1 <= self.F <= 64:
            raise ValueError(f"Scorer: 1 to 64 fields (num_fields = {self.F})")
        self.cap = self.B * int(stage_batches)
        self.weights = FrozenWeights(self.model)
        dev, i64 = self.device, torch.int64
        self.oov_id = (torch.full((self.F,), -1, dtype=i64) if oov_id is None
                       else torch.as_tensor(oov_id, dtype=i64).reshape(self.F)).to(dev).contiguous()
        self.stage = torch.zeros(self.cap, self.F, dtype=i64, device=dev)
        self.batch = torch.zeros(self.B, self.F, dtype=i64, device=dev)
        self.out_logits = torch.zeros(self.cap, dtype=torch.float32, device=dev)
        self.out_probs = torch.zeros(self.cap, dtype=torch.float32, device=dev)
        self.out_oov = torch.zeros(self.cap, dtype=torch.uint8, device=dev)
        self.cursor = torch.zeros(1, dtype=i64, device=dev)
        self.done = torch.zeros(1, dtype=torch.int32, device=dev)        # batches scored (mapx_step_advance's counter)
        self.use_graph = os.environ.get("MAPX_GRAPH", "1") != "0"
        self.graph, self._eager_steps, self.replays = None, 0, 0
        self.batcher = Batcher(self.B, self.cap)

    # one scoring step on the static buffers: what the graph captures and what the eager path runs
    def _step(self):
        ops.score_block(self.stage, self.cap, self.cursor, self.oov_id, self.batch, self.out_oov)
        with torch.no_grad():
            logits = self.model(input_ids=self.batch)[0]
        logits = logits.reshape(-1)
        if logits.dtype != torch.float32:
            logits = logits.float()
        if logits.numel() != self.B:
            raise RuntimeError(f"Scorer: the model gave {logits.numel()} logits for {self.B} rows")
        ops.score_sink(logits.contiguous(), self.cap, self.cursor, self.out_probs, self.out_logits)
        ops.step_advance(self.done, self.cursor, self.B)        # (+ the magnitude records' epoch: a replay outranks the last)

    def _capture(self):
        from .trainer import _capture
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        try:
            with _capture(graph):
                self._step()
        except RuntimeError as e:              # a runtime that cannot capture this step: stay eager (as Trainer.run_step)
            logger.warning(f"hipGraph capture of the scoring step failed ({e}); continuing eagerly")
            ops.reset_aux_streams()
            torch.cuda.synchronize(self.device)
            self.use_graph = False
            return
        self.graph = graph

    def _run(self, batches):
        for _ in range(batches):
            if self.use_graph and self.graph is None and self._eager_steps >= self.GRAPH_AFTER:
                self._capture()
            if self.graph is not None:
                self.graph.replay()
                self.replays += 1
            else:
                self._step()
                self._eager_steps += 1

    def _do(self, todo, piece):
        outs = []
        with torch.cuda.device(self.device):
            for op, a, b, c in todo:
                if op == "load":
                    self.stage[c:c + b - a].copy_(piece[a:b])
                elif op == "move":
                    src = self.stage[a:a + b]
                    self.stage[c:c + b].copy_(src.clone() if abs(c - a) < b else src)
                else:
                    self.cursor.fill_(a)
                    self._run(b)
                    outs.append(Scores(self.out_logits[a:a + c].clone(), self.out_probs[a:a + c].clone(),
                                       self.out_oov[a:a + c].clone()))
        if len(outs) == 1:
            return outs[0]
        if not outs:
            e = lambda dt: torch.empty(0, dtype=dt, device=self.device)
            return Scores(e(torch.float32), e(torch.float32), e(torch.uint8))
        return Scores(*(torch.cat(parts) for parts in zip(*outs)))

    def push(self, ids):
        ops.require_gpu(ids)
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[1] != self.F:
            raise TypeError(f"Scorer: ids must be int64 [n, {self.F}], not {ids.dtype} {tuple(ids.shape)}")
        return self._do(self.batcher.push(ids.shape[0]), ids)

    def finish(self):
        return self._do(self.batcher.finish(), None)

    def score(self, ids, labels=None):
        """The whole input at once -> Scores for its rows in order; with labels (int or float [n], device) ->
        (Scores, metrics): ops.eval_metrics over the returned logits (metrics_of)."""
        if self.batcher.held:
            raise RuntimeError("Scorer.score: rows of an unfinished stream are waiting (finish() first)")
        a, b = self.push(ids), self.finish()
        s = Scores(*(torch.cat(parts) for parts in zip(a, b)))
        return s if labels is None else (s, metrics_of(s.logits, labels)[0])


def metrics_of(logits, labels):
    """-> (ops.eval_metrics(logits, labels) | None, None | why not): no rows, or one class only."""
    if logits.numel() == 0:
        return None, "no rows"
    try:
        return ops.eval_metrics(logits, labels), None
    except ValueError as e:
        return None, str(e)


# ------------------------------------------------------------------------------- slices of a column
OOV_COLUMN = "@oov"                 # the pseudo-column of --group_by: a row's count of fields that took their <oov> id
SLICE_ARRAYS = tuple(k for k, _ in ops.SLICE_OUTPUTS)

GroupColumn = namedtuple("GroupColumn", "name column base groups")


def group_columns(group_by, names, oov_ids, first_base):
    """The columns of --group_by -> [GroupColumn(name, column, base, groups)].  names / oov_ids: the fields in order and
    the <oov> id of each; first_base: the first id of the first field.  A field's ids are [base, <oov> id], base the id
    behind the previous field's <oov>: the group of a row is id - base, `groups` = <oov> id - base + 1 of them.
    '@oov': column None, base 0, the group is the row's oov_fields count, F + 1 groups.  ValueError names an unknown
    or repeated column."""
    out, seen = [], set()
    for g in group_by:
        if g in seen:
            raise ValueError(f"group_by: {g!r} twice")
        seen.add(g)
        if g == OOV_COLUMN:
            out.append(GroupColumn(g, None, 0, len(names) + 1))
            continue
        if g not in names:
            raise ValueError(f"group_by: {g!r} is not a field ({', '.join(names)}) or {OOV_COLUMN}")
        c = list(names).index(g)
        base = int(first_base) if c == 0 else int(oov_ids[c - 1]) + 1
        if int(oov_ids[c]) < base or (c > 0 and int(oov_ids[c - 1]) < 0):
            raise ValueError(f"group_by: field {g!r} has no id range ending at its <oov> id in this vocabulary")
        out.append(GroupColumn(g, c, base, int(oov_ids[c]) - base + 1))
    return out


def group_names(col, feat_map):
    """The labels of a column's groups: the raw value strings of feat_map ('<oov>' the last), the counts for @oov."""
    if col.column is None:
        return [str(k) for k in range(col.groups)]
    out, cut = [None] * col.groups, len(col.name) + 1
    for key, i in feat_map.items():
        if col.base <= i < col.base + col.groups:
            out[i - col.base] = key[cut:]
    return out


def slice_report(rows, positives, u2, sum_prob, sum_loss, top=20, names=None):
    """ops.slice_metrics' five arrays (host) -> the report of one column, in float64:
         gauc       sum(rows_g * auc_g) / sum(rows_g) over the groups that hold both classes (None when there is none)
         gauc_rows  the rows those groups hold;   groups: the non-empty groups
         top        the `top` groups by rows (ties by group id): group, name, rows, positives, auc = u2 / (2 pos neg)
                    (NaN where a class is missing), logloss, ctr, mean_prob, calibration = mean_prob / ctr (NaN at ctr 0)."""
    rows, positives = np.asarray(rows, dtype=np.int64), np.asarray(positives, dtype=np.int64)
    u2 = np.asarray(u2).astype(np.uint64).astype(np.float64)
    r, p = rows.astype(np.float64), positives.astype(np.float64)
    both = (positives > 0) & (positives < rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = np.where(both, (u2 * 0.5) / (p * (r - p)), np.nan)
        ctr = p / r
        mean_prob = np.asarray(sum_prob, dtype=np.float64) / r
        logloss = np.asarray(sum_loss, dtype=np.float64) / r
        calibration = np.where(p > 0, mean_prob / ctr, np.nan)
    gauc_rows = int(rows[both].sum())
    gauc = float((r[both] * auc[both]).sum() / gauc_rows) if gauc_rows else None
    order = np.lexsort((np.arange(len(rows)), -rows))[:max(int(top), 0)]
    order = order[rows[order] > 0]
    listed = [dict(group=int(g), name=None if names is None else names[g], rows=int(rows[g]),
                   positives=int(positives[g]), auc=float(auc[g]), logloss=float(logloss[g]), ctr=float(ctr[g]),
                   mean_prob=float(mean_prob[g]), calibration=float(calibration[g])) for g in order.tolist()]
    return dict(gauc=gauc, gauc_rows=gauc_rows, groups=int((rows > 0).sum()), top=listed)


# ------------------------------------------------------------------------------- bootstrap intervals
ROW_UNITS = "@row"                  # --bootstrap_by's default: every row is its own resampling unit
BOOT_ARRAYS = tuple(k for k, _ in ops.BOOT_OUTPUTS)
BOOT_METRICS = ("auc", "logloss")

Bootstrap = namedtuple("Bootstrap", "replicates seed level by", defaults=(0, 0.95, ROW_UNITS))


def boot_values(arrays):
    """ops.bootstrap_metrics' four arrays (host) -> {auc, logloss}: float64 [R], NaN where the replicate leaves the
    metric undefined (AUC: a class without weight; log-loss: no weight at all)."""
    u2 = np.asarray(arrays["u2"]).astype(np.uint64).astype(np.float64)
    pw, nw = (np.asarray(arrays[k]).astype(np.uint64).astype(np.float64) for k in ("pos_w", "neg_w"))
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = np.where((pw > 0) & (nw > 0), (u2 * 0.5) / (pw * nw), np.nan)
        logloss = np.where(pw + nw > 0, np.asarray(arrays["sum_loss"], dtype=np.float64) / (pw + nw), np.nan)
    return dict(auc=auc, logloss=logloss)


def _quantiles(v, level):
    if not len(v):
        return float("nan"), float("nan")
    lo, hi = np.quantile(v, [(1.0 - level) / 2, (1.0 + level) / 2])
    return float(lo), float(hi)


def bootstrap_report(arrays, point, level=0.95, other=None, other_point=None):
    """The replicates of one model -> per metric of BOOT_METRICS: point (point[metric], the estimate on the rows as
    they are), mean and std (ddof 1; 0 for a single replicate) over the defined replicates, lo / hi = the
    (1 -/+ level) / 2 quantiles of the defined replicates (numpy's linear method), replicates, undefined (left out,
    never counted as 0).  Floats, the two counts ints.
    other / other_point: a second model's arrays and estimates on the same resamples (equal pos_w and neg_w, else
    ValueError) -> also 'delta': per metric point (this - other), lo, hi, frac_positive and frac_zero (the shares of
    the replicates defined for both with this - other > 0 / == 0), replicates, undefined."""
    if not 0.0 < level < 1.0:
        raise ValueError(f"bootstrap_report: 0 < level < 1 (got {level})")
    mine = boot_values(arrays)
    out = {}
    for k in BOOT_METRICS:
        v = mine[k][np.isfinite(mine[k])]
        lo, hi = _quantiles(v, level)
        out[k] = dict(point=float(point[k]), mean=float(v.mean()) if len(v) else float("nan"),
                      std=float(v.std(ddof=1)) if len(v) > 1 else (0.0 if len(v) else float("nan")), lo=lo, hi=hi,
                      replicates=int(len(mine[k])), undefined=int(len(mine[k]) - len(v)))
    if other is not None:
        same = all(np.asarray(arrays[k]).shape == np.asarray(other[k]).shape
                   and np.array_equal(np.asarray(arrays[k]).astype(np.uint64), np.asarray(other[k]).astype(np.uint64))
                   for k in ("pos_w", "neg_w"))
        if not same:
            raise ValueError("bootstrap_report: pos_w / neg_w of the two models differ: they were not scored on the "
                             "same resample (same rows, labels, units, seed and replicates)")
        theirs, out["delta"] = boot_values(other), {}
        for k in BOOT_METRICS:
            d = mine[k] - theirs[k]
            v = d[np.isfinite(d)]
            lo, hi = _quantiles(v, level)
            out["delta"][k] = dict(point=float(point[k]) - float(other_point[k]), lo=lo, hi=hi,
                                   frac_positive=float((v > 0).mean()) if len(v) else float("nan"),
                                   frac_zero=float((v == 0).mean()) if len(v) else float("nan"),
                                   replicates=int(len(d)), undefined=int(len(d) - len(v)))
    return out


def boot_arrays(out):
    """ops.bootstrap_metrics' tensors -> host arrays by name, the three integers as uint64."""
    arrays = {k: t.cpu().numpy() for k, t in zip(BOOT_ARRAYS, out)}
    return {k: (a if k == "sum_loss" else a.view(np.uint64)) for k, a in arrays.items()}


def boot_unit_column(boot, names):
    """The column of --bootstrap_by among the fields (None for @row); ValueError names an unknown one."""
    if boot is None or boot.by == ROW_UNITS:
        return None
    if boot.by not in names:
        raise ValueError(f"bootstrap_by: {boot.by!r} is not a field ({', '.join(names)}) or {ROW_UNITS}")
    return list(names).index(boot.by)


def _no_bootstrap(why):
    return ValueError(f"bootstrap needs the labels of both classes: {why}")


def slice_intervals(res, name, listed):
    """The groups a slices.json lists for column `name` gain auc_lo, auc_hi, logloss_lo, logloss_hi and
    boot_undefined (the replicates without both classes in the group): one ops.bootstrap_metrics call on the group's
    rows with their units of the whole input, so a row has the weight it has in the global resample.  A host loop over
    the listed groups, composition of the global pieces."""
    b, s = res["bootstrap"], res["slices"][name]
    boot, dev = b["boot"], b["device"]
    for entry in listed:
        idx = np.flatnonzero(s["groups"] == entry["group"])
        units = idx.astype(np.int64) if b["units"] is None else b["units"][idx]
        out = ops.bootstrap_metrics(torch.from_numpy(res["logits"][idx]).to(dev),
                                    torch.from_numpy(b["labels"][idx]).to(dev), boot.replicates, seed=boot.seed,
                                    units=torch.from_numpy(units).to(dev))
        rep = bootstrap_report(boot_arrays(out), entry, boot.level)
        entry.update(auc_lo=rep["auc"]["lo"], auc_hi=rep["auc"]["hi"], logloss_lo=rep["logloss"]["lo"],
                     logloss_hi=rep["logloss"]["hi"], boot_undefined=rep["auc"]["undefined"])
    return listed


def _json_safe(x):
    """NaN / inf -> null: what a strict JSON reader takes."""
    if isinstance(x, dict):
        return {k: _json_safe(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_json_safe(v) for v in x]
    return None if isinstance(x, float) and not np.isfinite(x) else x


# ------------------------------------------------------------------------------- checkpoints
PRETRAIN_KEYS = ("feat_encoder.", "mfp_criterion.", "pred_rfd.")


def check_state_dict(own, sd, input_size=None, where="checkpoint"):
    """The refusals of load_checkpoint, on shapes alone.  own / sd: {name: tensor or shape}."""
    shape = lambda v: tuple(v.shape) if hasattr(v, "shape") else tuple(v)
    missing, unexpected = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    heads = [k for k in unexpected if k.startswith(PRETRAIN_KEYS)]
    if heads:
        raise RuntimeError(f"{where} is a pretraining checkpoint: it holds the pretraining head {heads} and lacks "
                           f"{missing}; score a finetuned (CTR) model")
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict from {where}: missing {missing}, unexpected {unexpected}")
    tables = [k for k in own if len(shape(own[k])) == 2 and input_size is not None and shape(own[k])[0] == input_size]
    for k in tables:
        if shape(sd[k])[0] != input_size:
            raise RuntimeError(f"{where}: input_size {input_size} of the vocabulary differs from the {shape(sd[k])[0]} "
                               f"rows of {k!r}: the checkpoint was trained on another vocabulary")
    wrong = [f"{k}: {shape(sd[k])} for {shape(own[k])}" for k in own if shape(sd[k]) != shape(own[k])]
    if wrong:
        raise RuntimeError(f"{where}: tensors of another shape than the model flags give: {wrong}")


def load_checkpoint(model, path, input_size=None):
    """{step}.model (Trainer.save_model) into the model, as strictly as Trainer.load_model: missing or unexpected keys,
    a pretraining checkpoint, a wrong shape and an input_size that differs from the embedding's rows raise
    RuntimeError naming the keys."""
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise RuntimeError(f"{path}: not a state_dict (a full training state? score the {{step}}.model file)")
    own = model.state_dict()
    check_state_dict(own, sd, input_size, where=os.fspath(path))
    with torch.no_grad():
        for k, v in sd.items():
            own[k].copy_(v)
    return model


# ------------------------------------------------------------------------------- whole inputs
def _to_host(parts, s):
    for k, t in enumerate(s):
        if t.numel():
            parts[k].append(t.cpu().numpy())


def _no_slices(why):
    return ValueError(f"group_by needs the labels of both classes: {why}")


def _result(parts, labels, names, oov_rows, scorer, extra, slices=None, boot=None, unit_pieces=None):
    """slices: None, or [(GroupColumn, its group ids as int32 pieces on the host | None for @oov, group names)]: the
    columns go to the device once, with the logits.  boot: None or a Bootstrap; unit_pieces: its unit column as int64
    pieces on the host (None: every row its own unit)."""
    dts = (np.float32, np.float32, np.uint8)
    logits, probs, oov_fields = (np.concatenate(p) if p else np.empty(0, dtype=dt) for p, dt in zip(parts, dts))
    metrics, why, dev_logits, dev_y = None, "no labels", None, None
    if labels is not None:
        y = np.concatenate(labels) if labels else np.empty(0, dtype=np.int64)
        dev = scorer.device
        dev_logits, dev_y = torch.from_numpy(logits).to(dev), torch.from_numpy(y).to(dev)
        metrics, why = metrics_of(dev_logits, dev_y)
    info = dict(rows=int(logits.shape[0]), batch_size=scorer.B, graph=scorer.graph is not None,
                oov_rows={n: int(c) for n, c in zip(names, oov_rows)}, metrics=metrics, metrics_reason=why)
    info.update(extra)
    res = dict(logits=logits, probs=probs, oov_fields=oov_fields, info=info)
    if slices:
        if metrics is None:
            raise _no_slices(why)
        res["slices"], info["slices"] = {}, {}
        for col, pieces, gnames in slices:
            g = oov_fields.astype(np.int32) if pieces is None else np.concatenate(pieces)
            out = ops.slice_metrics(dev_logits, dev_y, torch.from_numpy(g).to(scorer.device), col.groups)
            arrays = {k: t.cpu().numpy() for k, t in zip(SLICE_ARRAYS, out)}
            arrays["u2"] = arrays["u2"].view(np.uint64)
            rep = slice_report(**arrays, top=0)
            info["slices"][col.name] = {k: rep[k] for k in ("gauc", "gauc_rows", "groups")}
            res["slices"][col.name] = dict(arrays, base=col.base, names=gnames)
            if boot is not None:
                res["slices"][col.name]["groups"] = g                    # (slice_intervals picks a group's rows)
    if boot is not None:
        if metrics is None:
            raise _no_bootstrap(why)
        units = None if unit_pieces is None else np.concatenate(unit_pieces).astype(np.int64)
        out = ops.bootstrap_metrics(dev_logits, dev_y, boot.replicates, seed=boot.seed,
                                    units=None if units is None else torch.from_numpy(units).to(scorer.device))
        arrays = boot_arrays(out)
        report = bootstrap_report(arrays, metrics, boot.level)
        res["bootstrap"] = dict(arrays=arrays, report=report, boot=boot, units=units, labels=(y > 0.5).astype(np.uint8),
                                device=scorer.device)
        info["bootstrap"] = {k: dict(lo=report[k]["lo"], hi=report[k]["hi"]) for k in BOOT_METRICS}
    return res


def oov_ids_of(meta, names):
    """The <oov> id of every field of a meta JSON's feat_map (-1, which no row holds, where a field has none)."""
    return [int(meta["feat_map"].get(f"{n}-<oov>", -1)) for n in names]


def score_raw_file(scorer, path, schema, voc, chunk_bytes=256 << 20, timing=None, group_by=None, bootstrap=None):
    """Raw text -> scores, chunk by chunk: rawtext.iter_columns -> Vocabulary.encode -> Scorer.push, the results to
    the host per chunk; device memory holds one chunk and the scorer's staging area whatever the file's size.
    schema: rawtext.SCHEMAS[...] or rawtext.UNLABELED[...] (no label field: metrics null).  `path`: a path or an open
    binary stream.  timing: a dict that receives read_s / copy_s / device_s (parse) of iter_columns and encode_s,
    score_s, host_s (results to the host).  -> dict(logits, probs, oov_fields: numpy [N]; info: score.json's content).
    group_by: field names and '@oov' (group_columns): the result gains 'slices' {name: ops.slice_metrics' five arrays
    over the whole file, base, names} and info 'slices' {name: gauc, gauc_rows, groups}; the requested columns are
    kept per chunk as int32 on the host, as the labels are.  ValueError without labels of both classes.
    bootstrap: a Bootstrap (replicates, seed, level, by): the result gains 'bootstrap' {arrays: ops.bootstrap_metrics'
    four, report: bootstrap_report's, units, labels} and info 'bootstrap' {auc: {lo, hi}, logloss: {lo, hi}}; the unit
    column of `by` is kept per chunk as int64 on the host.  The same ValueError."""
    from . import rawtext
    names, F = voc.field_names, len(voc.fields)
    slices = None
    if bootstrap is not None and schema.label is None:
        raise _no_bootstrap("no labels")
    unit_col = boot_unit_column(bootstrap, names)
    unit_pieces = None if unit_col is None else []
    if group_by:
        if schema.label is None:
            raise _no_slices("no labels")
        cols = group_columns(group_by, names, [f.oov for f in voc.fields], voc.fields[0].base)
        slices = [(c, None if c.column is None else [], group_names(c, voc.feat_map)) for c in cols]
    parts, labels, oov_rows = ([], [], []), ([] if schema.label is not None else None), [0] * F
    t_enc = t_score = t_host = 0.0
    clock, sync = time.perf_counter, (lambda: torch.cuda.synchronize(scorer.device)) if timing is not None else (lambda: None)
    for y, cols in rawtext.iter_columns(path, schema, device=scorer.device, chunk_bytes=chunk_bytes, timing=timing):
        t0 = clock()
        ids, oov = voc.encode(list(cols.unbind(0)))
        oov_rows = [a + int(b) for a, b in zip(oov_rows, oov)]
        sync(); t1 = clock()
        s = scorer.push(ids)
        sync(); t2 = clock()
        _to_host(parts, s)
        if labels is not None:
            labels.append(y.cpu().numpy())
        for c, pieces, _ in slices or ():
            if pieces is not None:
                pieces.append((ids[:, c.column] - c.base).to(torch.int32).cpu().numpy())
        if unit_pieces is not None:
            unit_pieces.append(ids[:, unit_col].cpu().numpy())
        t3 = clock()
        t_enc, t_score, t_host = t_enc + t1 - t0, t_score + t2 - t1, t_host + t3 - t2
    t0 = clock()
    s = scorer.finish()
    sync(); t1 = clock()
    _to_host(parts, s)
    if timing is not None:
        timing.update(encode_s=t_enc, score_s=t_score + t1 - t0, host_s=t_host + clock() - t1)
    return _result(parts, labels, names, oov_rows, scorer, dict(source=str(getattr(path, "name", path))), slices,
                   bootstrap, unit_pieces)


def read_dataset(data_dir, dataset_name, split="test"):
    """-> (meta, feat_ids int64 [n, F], labels int64 [n]) of a dataset directory (mapx/dataset.py's layout); split:
    train | valid | test through split.pkl, or all = the table's rows as they are (no split.pkl needed)."""
    import pickle as pkl
    from .dataset import SPLITS, _read_table
    with open(os.path.join(data_dir, f"{dataset_name}-meta.json")) as f:
        meta = json.load(f)
    feat_ids, labels = _read_table(data_dir, dataset_name)
    if split != "all":
        if split not in SPLITS:
            raise ValueError(f"split {split!r}: one of {SPLITS + ('all',)}")
        with open(os.path.join(data_dir, "split.pkl"), "rb") as f:
            index = pkl.load(f)[f"{split}_index"]
        feat_ids, labels = feat_ids[index], labels[index]
    return meta, np.ascontiguousarray(feat_ids, dtype=np.int64), np.asarray(labels)


def score_dataset(scorer, meta, feat_ids, labels=None, names=None, group_by=None, bootstrap=None):
    """A table on the host -> scores, one staging area of rows on the device at a time.  -> as score_raw_file; the id
    ranges of group_by's fields come from the meta's feat_map; bootstrap's unit column is the field's ids."""
    names = names if names is not None else [n for n in meta["field_names"] if n != "<rsv>"]
    slices = None
    if bootstrap is not None and labels is None:
        raise _no_bootstrap("no labels")
    unit_col = boot_unit_column(bootstrap, names)
    unit_pieces = None if unit_col is None else [np.ascontiguousarray(feat_ids[:, unit_col], dtype=np.int64)]
    if group_by:
        if labels is None:
            raise _no_slices("no labels")
        oov = oov_ids_of(meta, names)
        first = min((i for k, i in meta["feat_map"].items() if k.startswith(names[0] + "-")), default=0)
        slices = [(c, None if c.column is None else [(feat_ids[:, c.column] - c.base).astype(np.int32)],
                   group_names(c, meta["feat_map"])) for c in group_columns(group_by, names, oov, first)]
    oov_id = scorer.oov_id
    parts, oov_rows = ([], [], []), torch.zeros(feat_ids.shape[1], dtype=torch.int64, device=scorer.device)
    for r in range(0, feat_ids.shape[0], scorer.cap):
        ids = torch.from_numpy(feat_ids[r:r + scorer.cap]).to(scorer.device)
        oov_rows += (ids == oov_id).sum(0)
        _to_host(parts, scorer.push(ids))
    _to_host(parts, scorer.finish())
    y = None if labels is None else [np.asarray(labels).astype(np.int64)]
    return _result(parts, y, names, oov_rows.tolist(), scorer, {}, slices, bootstrap, unit_pieces)


def write_scores(out_dir, res, top=20, **info):
    """probs.npy, logits.npy, oov_fields.npy, score.json; with slices (group_by) also slices_<name>.npz (the five
    arrays and base) per column and slices.json {name: slice_report(top)}; with a bootstrap also bootstrap.json (the
    report, replicates, seed, level, units), bootstrap.npz (the four arrays, seed, level, units), labels.npy (u8 [N]),
    boot_units.npy (int64 [N], when the units are a field's ids), and the listed groups' intervals (slice_intervals)."""
    os.makedirs(out_dir, exist_ok=True)
    for k in ("probs", "logits", "oov_fields"):
        np.save(os.path.join(out_dir, f"{k}.npy"), res[k])
    if "slices" in res:
        reports = {}
        for name, s in res["slices"].items():
            arrays = {k: s[k] for k in SLICE_ARRAYS}
            np.savez(os.path.join(out_dir, f"slices_{name}.npz"), base=np.int64(s["base"]), **arrays)
            reports[name] = slice_report(**arrays, top=top, names=s["names"])
            if "bootstrap" in res:
                slice_intervals(res, name, reports[name]["top"])
        with open(os.path.join(out_dir, "slices.json"), "w") as f:
            json.dump(_json_safe(reports), f, indent=1, allow_nan=False)
    if "bootstrap" in res:
        b = res["bootstrap"]
        boot = b["boot"]
        np.savez(os.path.join(out_dir, "bootstrap.npz"), seed=np.uint64(boot.seed), level=np.float64(boot.level),
                 units=np.array(boot.by), **b["arrays"])
        np.save(os.path.join(out_dir, "labels.npy"), b["labels"])
        if b["units"] is not None:
            np.save(os.path.join(out_dir, "boot_units.npy"), b["units"])
        with open(os.path.join(out_dir, "bootstrap.json"), "w") as f:
            json.dump(_json_safe(dict(b["report"], replicates=boot.replicates, seed=boot.seed, level=boot.level,
                                      units=boot.by)), f, indent=1, allow_nan=False)
    doc = dict(res["info"], **info)
    with open(os.path.join(out_dir, "score.json"), "w") as f:
        json.dump(doc, f, indent=1)
    return doc


# ------------------------------------------------------------------------------- the command
def parser():
    p = argparse.ArgumentParser(prog="python -m mapx.score", allow_abbrev=False, description=__doc__.split("\n\n")[0])
    p.add_argument("--model", required=True, help="{step}.model checkpoint of a finetuned (CTR) model")
    p.add_argument("--out", required=True, help="directory for probs.npy, logits.npy, oov_fields.npy, score.json")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--raw", help="raw Avazu / Criteo text (a .gz path is streamed through gzip); needs --vocab, --dataset")
    src.add_argument("--data_dir", help="dataset directory (<name>-meta.json, <name>.npz / .h5[, split.pkl])")
    p.add_argument("--vocab", metavar="META.json", help="the <name>-meta.json whose feat_map the model was trained on")
    p.add_argument("--dataset", choices=("avazu", "criteo"), help="the raw file's schema")
    p.add_argument("--unlabeled", action="store_true", help="the raw file has no click field (Avazu's test.gz)")
    p.add_argument("--dataset_name", default="avazu", help="file prefix inside --data_dir")
    p.add_argument("--split", default="test", choices=("train", "valid", "test", "all"),
                   help="rows of --data_dir to score (all: the whole table, no split.pkl needed)")
    p.add_argument("--batch_size", type=_positive, default=4096, help="rows per scoring step")
    p.add_argument("--chunk_mb", type=_positive, default=256, help="bytes of the raw file on the device at a time (<= 1024)")
    p.add_argument("--group_by", metavar="NAME[,NAME...]", type=lambda s: [x for x in s.split(",") if x],
                   help=f"sliced evaluation: AUC, GAUC, log-loss and calibration per value of these fields ({OOV_COLUMN}: "
                        "per count of <oov> fields) -> slices.json, slices_<name>.npz; needs labels of both classes")
    p.add_argument("--top", type=_positive, default=20, help="groups listed per column in slices.json, by rows")
    p.add_argument("--bootstrap", metavar="R", type=_positive, default=None,
                   help="Poisson-bootstrap intervals of AUC and log-loss from R replicates (<= 65536) -> bootstrap.json, "
                        "bootstrap.npz, labels.npy; needs labels of both classes")
    p.add_argument("--bootstrap_seed", metavar="S", type=int, default=None, help="seed of the resamples (default 0)")
    p.add_argument("--bootstrap_level", metavar="L", type=float, default=None, help="coverage of the intervals (default 0.95)")
    p.add_argument("--bootstrap_by", metavar="NAME", default=None,
                   help=f"resampling unit: a field (its rows share a weight: the cluster bootstrap; -> boot_units.npy) "
                        f"or {ROW_UNITS}, every row alone (default)")
    add_flags(p, MODEL_FLAGS + EXTENSION_MODEL_FLAGS)
    return p


def parse_args(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.raw is not None and (args.vocab is None or args.dataset is None):
        p.error("--raw needs --vocab META.json and --dataset avazu|criteo")
    if args.raw is None and (args.vocab is not None or args.unlabeled):
        p.error("--vocab / --unlabeled go with --raw")
    if args.chunk_mb > 1024:
        p.error("--chunk_mb: at most 1024")
    if args.bootstrap is None:
        for flag in ("bootstrap_seed", "bootstrap_level", "bootstrap_by"):
            if getattr(args, flag) is not None:
                p.error(f"--{flag} goes with --bootstrap R")
    else:
        if args.unlabeled:
            p.error("--bootstrap needs the labels of both classes: no labels (it does not go with --unlabeled)")
        if args.bootstrap > ops.BOOT_MAX_REPLICATES:
            p.error(f"--bootstrap: at most {ops.BOOT_MAX_REPLICATES} replicates")
        seed = 0 if args.bootstrap_seed is None else args.bootstrap_seed
        level = 0.95 if args.bootstrap_level is None else args.bootstrap_level
        by = ROW_UNITS if args.bootstrap_by is None else args.bootstrap_by
        if not 0 <= seed < 2 ** 64:
            p.error("--bootstrap_seed: an unsigned 64-bit integer")
        if not 0.0 < level < 1.0:
            p.error("--bootstrap_level: between 0 and 1")
        if args.raw is not None and by != ROW_UNITS:
            from . import rawtext
            schema = rawtext.SCHEMAS[args.dataset]
            known = [c for c in schema.columns if c != schema.label]
            if by not in known:
                p.error(f"--bootstrap_by: {by!r} is not a field of {args.dataset} ({', '.join(known)}) or {ROW_UNITS}")
        args.bootstrap_seed, args.bootstrap_level, args.bootstrap_by = seed, level, by
    if args.group_by:
        if args.unlabeled:
            p.error("--group_by needs labels: it does not go with --unlabeled")
        if len(set(args.group_by)) != len(args.group_by):
            p.error(f"--group_by: a column twice in {args.group_by}")
        if args.raw is not None:                  # (the fields of --data_dir are known when its meta is read)
            from . import rawtext
            schema = rawtext.SCHEMAS[args.dataset]
            known = [c for c in schema.columns if c != schema.label] + [OOV_COLUMN]
            for g in args.group_by:
                if g not in known:
                    p.error(f"--group_by: {g!r} is not a field of {args.dataset} ({', '.join(known)})")
    return args


def build_model(args, input_size, num_fields, device):
    from .models import build_backbone
    cfg = {n: getattr(args, n) for n, *_ in MODEL_FLAGS + EXTENSION_MODEL_FLAGS}
    cfg.update(data_dir=args.data_dir, input_size=int(input_size), num_fields=int(num_fields), pretrain=False,
               pt_type="MFP", RFD_replace="Unigram", feat_count=None, device=device, n_gpu=1, idx_low=None,
               idx_high=None, feat_num_per_field=None, seed=42, rank=0)
    model = build_backbone(Config.from_dict(cfg))
    return load_checkpoint(model, args.model, input_size=int(input_size)).to(device)


def main(argv=None):
    args = parse_args(argv)
    for what, path in (("--model", args.model), ("--raw", args.raw), ("--vocab", args.vocab)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f"{what}: {path} is not a file")
    if not torch.cuda.is_available():
        raise SystemExit("mapx.score runs on an MI355X only (no CPU path)")
    device = torch.device("cuda", 0)
    boot = None if args.bootstrap is None else Bootstrap(args.bootstrap, args.bootstrap_seed, args.bootstrap_level,
                                                          args.bootstrap_by)
    t0 = time.time()
    if args.raw is not None:
        from . import rawtext, vocab
        schema = (rawtext.UNLABELED if args.unlabeled else rawtext.SCHEMAS)[args.dataset]
        voc = vocab.Vocabulary.from_meta(args.vocab, schema, device=device)
        model = build_model(args, voc.input_size, len(voc.fields), device)
        scorer = Scorer(model, args.batch_size, device, oov_id=[f.oov for f in voc.fields])
        res = score_raw_file(scorer, args.raw, schema, voc, chunk_bytes=args.chunk_mb << 20, group_by=args.group_by,
                             bootstrap=boot)
    else:
        meta, feat_ids, labels = read_dataset(args.data_dir, args.dataset_name, args.split)
        names = [n for n in meta["field_names"] if n != "<rsv>"]
        model = build_model(args, len(meta["feat_map"]), len(meta["field_map"]) - 1, device)
        scorer = Scorer(model, args.batch_size, device, oov_id=oov_ids_of(meta, names))
        res = score_dataset(scorer, meta, feat_ids, labels, names=names, group_by=args.group_by, bootstrap=boot)
    doc = write_scores(args.out, res, top=args.top, model=args.model, compute_dtype=args.compute_dtype,
                       seconds=round(time.time() - t0, 3))
    m = doc["metrics"]
    print(f"{args.out}: {doc['rows']} rows, batch {doc['batch_size']}, {args.compute_dtype}, "
          + (f"auc {m['auc']:.6f} logloss {m['logloss']:.6f}" if m else f"no metrics ({doc['metrics_reason']})"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
