"""Score a checkpoint on new data: a raw file, or a dataset directory, to per-row click probabilities.

    python -m mapx.score --model OUT/1234.model --vocab DIR/avazu-meta.json --dataset avazu --raw day11.gz
                         [--unlabeled] --out SDIR [--batch_size 4096] [--chunk_mb 256] <run.py's model flags>
    python -m mapx.score --model OUT/1234.model --data_dir DIR --dataset_name avazu [--split test|valid|train|all]
                         --out SDIR <run.py's model flags>

writes SDIR/probs.npy (f32 [N]), logits.npy (f32 [N]), oov_fields.npy (u8 [N]: the fields of a row that took their
field's <oov> id) and score.json, rows in file order.  One device; no optimizer, no labels needed.

A scoring step is  mapx_score_block -> the model's forward -> mapx_score_sink -> mapx_step_advance  (csrc/score.hip),
captured as one hipGraph after a few eager steps and replayed with nothing but the device-side cursor changing
(`Scorer`; MAPX_GRAPH=0 keeps the eager loop).  Batches are ALWAYS the rows [kB, (k+1)B) of the input stream, however
the caller cuts the stream into pieces: fp32-mode products cut their activations at a per-batch magnitude, so a
row's bits depend on its batch mates."""
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


def _result(parts, labels, names, oov_rows, scorer, extra):
    dts = (np.float32, np.float32, np.uint8)
    logits, probs, oov_fields = (np.concatenate(p) if p else np.empty(0, dtype=dt) for p, dt in zip(parts, dts))
    metrics, why = None, "no labels"
    if labels is not None:
        y = np.concatenate(labels) if labels else np.empty(0, dtype=np.int64)
        dev = scorer.device
        metrics, why = metrics_of(torch.from_numpy(logits).to(dev), torch.from_numpy(y).to(dev))
    info = dict(rows=int(logits.shape[0]), batch_size=scorer.B, graph=scorer.graph is not None,
                oov_rows={n: int(c) for n, c in zip(names, oov_rows)}, metrics=metrics, metrics_reason=why)
    info.update(extra)
    return dict(logits=logits, probs=probs, oov_fields=oov_fields, info=info)


def oov_ids_of(meta, names):
    """The <oov> id of every field of a meta JSON's feat_map (-1, which no row holds, where a field has none)."""
    return [int(meta["feat_map"].get(f"{n}-<oov>", -1)) for n in names]


def score_raw_file(scorer, path, schema, voc, chunk_bytes=256 << 20, timing=None):
    """Raw text -> scores, chunk by chunk: rawtext.iter_columns -> Vocabulary.encode -> Scorer.push, the results to
    the host per chunk; device memory holds one chunk and the scorer's staging area whatever the file's size.
    schema: rawtext.SCHEMAS[...] or rawtext.UNLABELED[...] (no label field: metrics null).  `path`: a path or an open
    binary stream.  timing: a dict that receives read_s / copy_s / device_s (parse) of iter_columns and encode_s,
    score_s, host_s (results to the host).  -> dict(logits, probs, oov_fields: numpy [N]; info: score.json's content)."""
    from . import rawtext
    names, F = voc.field_names, len(voc.fields)
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
        t3 = clock()
        t_enc, t_score, t_host = t_enc + t1 - t0, t_score + t2 - t1, t_host + t3 - t2
    t0 = clock()
    s = scorer.finish()
    sync(); t1 = clock()
    _to_host(parts, s)
    if timing is not None:
        timing.update(encode_s=t_enc, score_s=t_score + t1 - t0, host_s=t_host + clock() - t1)
    return _result(parts, labels, names, oov_rows, scorer, dict(source=str(getattr(path, "name", path))))


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


def score_dataset(scorer, meta, feat_ids, labels=None, names=None):
    """A table on the host -> scores, one staging area of rows on the device at a time.  -> as score_raw_file."""
    names = names if names is not None else [n for n in meta["field_names"] if n != "<rsv>"]
    oov_id = scorer.oov_id
    parts, oov_rows = ([], [], []), torch.zeros(feat_ids.shape[1], dtype=torch.int64, device=scorer.device)
    for r in range(0, feat_ids.shape[0], scorer.cap):
        ids = torch.from_numpy(feat_ids[r:r + scorer.cap]).to(scorer.device)
        oov_rows += (ids == oov_id).sum(0)
        _to_host(parts, scorer.push(ids))
    _to_host(parts, scorer.finish())
    y = None if labels is None else [np.asarray(labels).astype(np.int64)]
    return _result(parts, y, names, oov_rows.tolist(), scorer, {})


def write_scores(out_dir, res, **info):
    os.makedirs(out_dir, exist_ok=True)
    for k in ("probs", "logits", "oov_fields"):
        np.save(os.path.join(out_dir, f"{k}.npy"), res[k])
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
    t0 = time.time()
    if args.raw is not None:
        from . import rawtext, vocab
        schema = (rawtext.UNLABELED if args.unlabeled else rawtext.SCHEMAS)[args.dataset]
        voc = vocab.Vocabulary.from_meta(args.vocab, schema, device=device)
        model = build_model(args, voc.input_size, len(voc.fields), device)
        scorer = Scorer(model, args.batch_size, device, oov_id=[f.oov for f in voc.fields])
        res = score_raw_file(scorer, args.raw, schema, voc, chunk_bytes=args.chunk_mb << 20)
    else:
        meta, feat_ids, labels = read_dataset(args.data_dir, args.dataset_name, args.split)
        names = [n for n in meta["field_names"] if n != "<rsv>"]
        model = build_model(args, len(meta["feat_map"]), len(meta["field_map"]) - 1, device)
        scorer = Scorer(model, args.batch_size, device, oov_id=oov_ids_of(meta, names))
        res = score_dataset(scorer, meta, feat_ids, labels, names=names)
    doc = write_scores(args.out, res, model=args.model, compute_dtype=args.compute_dtype,
                       seconds=round(time.time() - t0, 3))
    m = doc["metrics"]
    print(f"{args.out}: {doc['rows']} rows, batch {doc['batch_size']}, {args.compute_dtype}, "
          + (f"auc {m['auc']:.6f} logloss {m['logloss']:.6f}" if m else f"no metrics ({doc['metrics_reason']})"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
