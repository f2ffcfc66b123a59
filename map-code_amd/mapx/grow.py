"""Carry a checkpoint, or a dataset, over from a saved vocabulary to the vocabulary grown from it.

    python -m mapx.grow --model OUT/1234.model --from DIR/avazu-meta.json --to DIR2/avazu-meta.json --out OUT2/1234.model
                        [--init oov|normal:0.01 --seed 42]
    python -m mapx.grow --data_dir DIR --dataset_name avazu --from DIR/avazu-meta.json --to DIR2/avazu-meta.json --out DIR3

`python -m mapx.preprocess --vocab META.json --grow K` extends a saved feat_map with a later file's values: per field
the old keys keep their order, the added keys follow them, `<oov>` stays last, ids stay consecutive.  So every old id
moves by its field's shift and nothing else changes.  `plan` derives that from the two metas alone (pure host
arithmetic, no side file) and refuses a pair that is not a growth; `migrate_state_dict` moves the [V, *] tables of a
{step}.model file with it (csrc/vocab_grow.hip: mapx_table_migrate, a row gather whose source row is computed from
the plan), `remap_ids` the feat_ids of a dataset.

Which tensors are tables is decided by their KEY (TABLE_KEYS: the TableWeight parameters) and then checked by shape;
a dense weight whose first dimension happens to equal V_old is left alone.  New rows — the added keys and the new
`<oov>` — start as copies of their field's old `<oov>` row (init=oov, the default): the migration is then
function-preserving, a row encoded with the grown vocabulary reads in the migrated tables exactly what the same row
encoded with the old vocabulary read in the old ones.  init=normal:STD draws the added rows on the host instead.  The NCE
noise buffers (NOISE_KEYS: 1-D [V] statistics of the old dataset) cannot be moved row by row: they are dropped, and
BaseModel.load_from_target_model keeps the buffers the model built from the new dataset's feat-count.pt.  Optimizer /
resume files (Trainer.save_training_state) are not migrated: a continued run starts a fresh optimizer, as any run
from a .model file does."""
import argparse
import json
import os
import sys
from collections import namedtuple

import numpy as np
import torch

from .native import MapxError, RT_MAX_FIELDS, check, lib, require_gpu, stream

# THE list of [V, *] tables of a state dict, by key suffix: Embeddings.embedding, LR.embed_w (DeepFM's [V, 1] weights),
# IndexLinear.emb / .bias.  And the [V] noise statistics of IndexLinear, which are dropped.
TABLE_KEYS = ("embedding.weight", "embed_w.weight", "mfp_criterion.emb.weight", "mfp_criterion.bias.weight")
NOISE_KEYS = ("mfp_criterion.logprob_noise", "mfp_criterion.alias.prob", "mfp_criterion.alias.alias")

FieldPlan = namedtuple("FieldPlan", "name n_old added base_old base_new")


class Plan(namedtuple("Plan", "fields V_old V_new reserved")):
    """fields: [FieldPlan] in order; V_old / V_new: rows of a table before / after; reserved: ids below the first
    field.  Field f owns the old ids [base_old, base_old + n_old] and the new ids [base_new, base_new + n_old + added],
    the last of each its `<oov>`."""

    @property
    def added_total(self):
        return sum(f.added for f in self.fields)

    def arrays(self):
        """-> int64 [4, F]: n_old, added, base_old, base_new (what mapx_table_migrate takes)."""
        return np.array([[f.n_old for f in self.fields], [f.added for f in self.fields],
                         [f.base_old for f in self.fields], [f.base_new for f in self.fields]], dtype=np.int64)


def _load_meta(meta):
    if isinstance(meta, dict):
        return meta
    with open(os.fspath(meta)) as f:
        return json.load(f)


def _field_runs(meta, what):
    """feat_map of a meta -> (reserved keys, [(field name, base, [key strings without <oov>])]).  The ids must be the
    positions; every field's keys are one run `name-...` in field_names order that ends with `name-<oov>`."""
    names = [n for n in meta["field_names"] if n != "<rsv>"]
    items = list(meta["feat_map"].items())
    for pos, (key, i) in enumerate(items):
        if type(i) is not int or i != pos:
            raise ValueError(f"{what} feat_map key {key!r}: id {i!r} where the ids are consecutive from 0 (expected {pos})")
    first = names[0] + "-" if names else None
    pos = 0
    while pos < len(items) and not (first and items[pos][0].startswith(first)):
        pos += 1
    reserved, runs = [k for k, _ in items[:pos]], []
    for name in names:
        prefix, start = name + "-", pos
        while pos < len(items) and items[pos][0].startswith(prefix):
            pos += 1
        run = [k for k, _ in items[start:pos]]
        oov = prefix + "<oov>"
        if not run or run[-1] != oov or oov in run[:-1]:
            raise ValueError(f"{what} feat_map key {oov!r} is missing or is not the last id of field {name!r}")
        runs.append((name, start, run[:-1]))
    if pos != len(items):
        raise ValueError(f"{what} feat_map key {items[pos][0]!r}: not a key of the fields {names} in order")
    return reserved, runs


def plan(old_meta, new_meta, schema=None):
    """The growth plan from the meta of the saved vocabulary to the meta of the grown one (dicts, or paths of
    `<name>-meta.json` files) -> Plan.  Verifies that new is a growth of old — the same field_names, the same reserved
    keys, per field the old keys a prefix of the new keys in order, `<oov>` last — and raises ValueError naming the
    first offending key otherwise.  schema (a rawtext.Schema): both feat_maps are also read through vocab.parse_meta,
    which checks that every key inverts to a value of its column."""
    old_meta, new_meta = _load_meta(old_meta), _load_meta(new_meta)
    if list(old_meta["field_names"]) != list(new_meta["field_names"]):
        a, b = list(old_meta["field_names"]), list(new_meta["field_names"])
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise ValueError(f"field_names differ at position {at}: {a[at] if at < len(a) else None!r} in the old meta, "
                         f"{b[at] if at < len(b) else None!r} in the new one")
    if len(old_meta["field_names"]) - 1 < 1:
        raise ValueError("field_names: no field")
    if schema is not None:
        from . import vocab
        vocab.parse_meta(old_meta, schema)
        vocab.parse_meta(new_meta, schema)
    rsv_old, old = _field_runs(old_meta, "old")
    rsv_new, new = _field_runs(new_meta, "new")
    if rsv_old != rsv_new:
        at = next((i for i, (x, y) in enumerate(zip(rsv_old, rsv_new)) if x != y), min(len(rsv_old), len(rsv_new)))
        raise ValueError(f"reserved key {(rsv_old + rsv_new)[at] if at >= len(rsv_old) else rsv_old[at]!r}: the "
                         f"reserved ids of the two feat_maps differ at id {at}")
    fields = []
    for (name, b_old, k_old), (_, b_new, k_new) in zip(old, new):
        have = set(k_new)
        for r, key in enumerate(k_old):
            if r < len(k_new) and k_new[r] == key:
                continue
            if key not in have:
                raise ValueError(f"old key {key!r} (rank {r} of field {name!r}) is missing from the new feat_map")
            raise ValueError(f"old key {key!r} is out of order in the new feat_map: rank {k_new.index(key)} of field "
                             f"{name!r} where the old feat_map has it at rank {r}")
        fields.append(FieldPlan(name, len(k_old), len(k_new) - len(k_old), b_old, b_new))
    return Plan(fields, len(old_meta["feat_map"]), len(new_meta["feat_map"]), len(rsv_old))


def identity_plan(meta):
    """The plan from a meta to itself (nothing added)."""
    return plan(meta, meta)


# ------------------------------------------------------------------------------- tables
def migrate_table(src, plan_, fresh=None, out=None):
    """src f32 [V_old, W] on the device (unit column stride, any row pitch) -> f32 [V_new, W]: mapx_table_migrate.
    fresh: None (added rows copy their field's old <oov> row) or f32 [plan.added_total, W], the added rows in id
    order.  out: a [V_new, W] view with unit column stride to write into."""
    require_gpu(src, fresh, out)
    F = len(plan_.fields)
    if not 1 <= F <= RT_MAX_FIELDS:
        raise ValueError(f"migrate_table: 1 to {RT_MAX_FIELDS} fields")

    def matrix(t, rows, what):
        W = src.shape[1] if src.dim() == 2 else -1
        if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (rows, W) or (W > 1 and t.stride(1) != 1) or \
                (rows > 1 and t.stride(0) < W):
            raise TypeError(f"migrate_table: {what} must be float32 [{rows}, {W}] with unit column stride, not "
                            f"{t.dtype} {tuple(t.shape)}")
        return t.stride(0) if rows > 1 else W
    ld_src = matrix(src, plan_.V_old, "src")
    W = src.shape[1]
    if out is None:
        out = torch.empty(plan_.V_new, W, dtype=torch.float32, device=src.device)
    ld_dst = matrix(out, plan_.V_new, "out")
    ld_fresh = matrix(fresh, plan_.added_total, "fresh") if fresh is not None else W
    par = torch.from_numpy(plan_.arrays()).to(src.device)
    err = torch.empty(1, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        check(lib.mapx_table_migrate(src.data_ptr(), ld_src, plan_.V_old, out.data_ptr(), ld_dst, plan_.V_new, W, F,
                                     par[0].data_ptr(), par[1].data_ptr(), par[2].data_ptr(), par[3].data_ptr(),
                                     None if fresh is None else fresh.data_ptr(), ld_fresh,
                                     0 if fresh is None else plan_.added_total,
                                     err.data_ptr(), stream()))
    if int(err.item()):                                      # (also ends the launch's use of par)
        raise MapxError("migrate_table: the plan places a row outside the source table")
    return out


def _is(key, suffixes):
    return any(key == s or key.endswith("." + s) for s in suffixes)


def parse_init(init):
    """'oov' -> None; 'normal:STD' -> STD (a float > 0)."""
    if init == "oov":
        return None
    kind, _, text = str(init).partition(":")
    try:
        std = float(text) if kind == "normal" else -1.0
    except ValueError:
        std = -1.0
    if not std > 0.0 or not np.isfinite(std):
        raise ValueError(f"init {init!r}: 'oov' or 'normal:STD' with STD > 0")
    return std


def migrate_state_dict(sd, plan_, init="oov", seed=42, device="cuda"):
    """A {step}.model state dict of V_old rows -> (state dict of V_new rows, report).  Tensors whose key is a table's
    (TABLE_KEYS) must be float32 [V_old, W] — ValueError naming the key otherwise — and are moved by migrate_table on
    `device`; NOISE_KEYS are dropped; everything else is handed on untouched, whatever its shape.
    init='oov': added rows and the new <oov> copy their field's old <oov> row.  init='normal:STD': the added rows are
    drawn on the host, torch.empty(added_total, W).normal_(0, STD, generator=g) per table in the state dict's order from
    one g = torch.Generator().manual_seed(seed); the new <oov> row is still the old one.
    report: {'tables': {key: [V_old, V_new, W]}, 'dropped': [keys], 'kept': number of other tensors, 'added': rows}."""
    std = parse_init(init)
    gen = torch.Generator().manual_seed(int(seed)) if std is not None else None
    out, report = {}, {"tables": {}, "dropped": [], "kept": 0, "added": plan_.added_total}
    for key, t in sd.items():
        if _is(key, NOISE_KEYS):
            report["dropped"].append(key)
        elif _is(key, TABLE_KEYS):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != plan_.V_old or t.dtype != torch.float32:
                shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"{key!r}: a table of the old vocabulary is float32 [{plan_.V_old}, W], not "
                                 f"{getattr(t, 'dtype', '')} {shape}: the checkpoint was not trained on the --from vocabulary")
            fresh = None
            if std is not None:
                fresh = torch.empty(plan_.added_total, t.shape[1]).normal_(0.0, std, generator=gen).to(device)
            moved = migrate_table(t.detach().to(device).contiguous(), plan_, fresh=fresh)
            out[key] = moved.to(t.device)
            report["tables"][key] = [plan_.V_old, plan_.V_new, int(t.shape[1])]
        else:
            out[key] = t
            report["kept"] += 1
    return out, report


# ------------------------------------------------------------------------------- ids
def remap_ids(feat_ids, plan_):
    """feat_ids int64 [N, F] of the old id space (a tensor on any device, or a numpy array) -> the same rows in the new
    id space: column f's ids shift by base_new - base_old, its old <oov> id becomes the new one, reserved ids stay.
    ValueError when a column holds an id outside its field's old range."""
    as_numpy = not torch.is_tensor(feat_ids)
    ids = torch.as_tensor(feat_ids)
    F = len(plan_.fields)
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[1] != F:
        raise TypeError(f"remap_ids: int64 [N, {F}], not {ids.dtype} {tuple(ids.shape)}")
    par = torch.from_numpy(plan_.arrays()).to(ids.device)
    n_old, added, base_old, base_new = par[0], par[1], par[2], par[3]
    rank = ids - base_old
    reserved = (ids >= 0) & (ids < plan_.reserved)
    bad = ~reserved & ((rank < 0) | (rank > n_old))
    if bool(bad.any()):
        r, c = (int(x) for x in bad.nonzero()[0])
        raise ValueError(f"remap_ids: row {r} holds id {int(ids[r, c])} in field {plan_.fields[c].name!r}, whose old ids "
                         f"are [{plan_.fields[c].base_old}, {plan_.fields[c].base_old + plan_.fields[c].n_old}]")
    out = torch.where(reserved, ids, base_new + rank + torch.where(rank == n_old, added, torch.zeros_like(added)))
    return out.numpy() if as_numpy else out


def migrate_dataset(data_dir, dataset_name, plan_, new_meta, out_dir):
    """The dataset directory of the old vocabulary -> out_dir in the new id space: feat_ids through remap_ids, every
    other array as it is; the meta keeps the dataset's own entries and takes the new feat_map; split.pkl is copied."""
    import shutil
    with open(os.path.join(data_dir, f"{dataset_name}-meta.json")) as f:
        meta = json.load(f)
    path = os.path.join(data_dir, f"{dataset_name}.npz")
    if not os.path.isfile(path):
        raise ValueError(f"{path}: mapx.grow moves the .npz table of a dataset directory")
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["feat_ids"] = remap_ids(np.ascontiguousarray(arrays["feat_ids"], dtype=np.int64), plan_)
    new_meta = _load_meta(new_meta)
    meta["feat_map"] = new_meta["feat_map"]
    oov_new = [f.base_new + f.n_old + f.added for f in plan_.fields]
    meta["oov_rows"] = {f.name: int((arrays["feat_ids"][:, j] == o).sum())
                        for j, (f, o) in enumerate(zip(plan_.fields, oov_new))}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{dataset_name}-meta.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False)
    np.savez(os.path.join(out_dir, f"{dataset_name}.npz"), **arrays)
    if os.path.isfile(os.path.join(data_dir, "split.pkl")) and os.path.abspath(data_dir) != os.path.abspath(out_dir):
        shutil.copyfile(os.path.join(data_dir, "split.pkl"), os.path.join(out_dir, "split.pkl"))
    return meta


# ------------------------------------------------------------------------------- the command
def parser():
    p = argparse.ArgumentParser(prog="python -m mapx.grow", allow_abbrev=False, description=__doc__.split("\n\n")[0])
    what = p.add_mutually_exclusive_group(required=True)
    what.add_argument("--model", help="{step}.model checkpoint trained on the --from vocabulary")
    what.add_argument("--data_dir", help="dataset directory encoded with the --from vocabulary")
    p.add_argument("--dataset_name", default="avazu", help="file prefix inside --data_dir")
    p.add_argument("--from", dest="old", required=True, metavar="META.json", help="the saved vocabulary's <name>-meta.json")
    p.add_argument("--to", dest="new", required=True, metavar="META.json",
                   help="the grown vocabulary's <name>-meta.json (mapx.preprocess --vocab ... --grow K)")
    p.add_argument("--out", required=True, help="the migrated .model file, or the new dataset directory")
    p.add_argument("--dataset", choices=("avazu", "criteo"), default=None,
                   help="also check that every feat_map key is a value of this schema's column")
    p.add_argument("--init", default="oov", help="rows of the added keys: oov (copy the field's <oov> row; "
                                                 "function-preserving) or normal:STD")
    p.add_argument("--seed", type=int, default=42, help="seed of the normal:STD draw")
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    for flag, path in (("--from", args.old), ("--to", args.new), ("--model", args.model)):
        if path is not None and not os.path.isfile(path):
            p.error(f"{flag}: {path} is not a file")
    try:
        parse_init(args.init)
    except ValueError as e:
        p.error(f"--init: {e}")
    schema = None
    if args.dataset is not None:
        from . import rawtext
        schema = rawtext.SCHEMAS[args.dataset]
    pl = plan(args.old, args.new, schema)
    most = ", ".join(f"{f.name} +{f.added}" for f in sorted(pl.fields, key=lambda f: -f.added)[:3])
    grew = f"{pl.V_old} -> {pl.V_new} ids ({pl.added_total} keys added; {most})"
    if args.model is not None:
        if not torch.cuda.is_available():
            raise SystemExit("mapx.grow moves tables on an MI355X only (no CPU path)")
        sd = torch.load(args.model, map_location="cpu")
        if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
            raise SystemExit(f"{args.model}: not a state_dict (a full training state? migrate the {{step}}.model file)")
        out, report = migrate_state_dict(sd, pl, init=args.init, seed=args.seed, device=torch.device("cuda", 0))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        torch.save(out, args.out)
        print(f"{args.out}: {grew}; moved {', '.join(report['tables']) or 'no table'} (init {args.init}); dropped "
              f"{', '.join(report['dropped']) or 'nothing'}; {report['kept']} other tensors unchanged")
        return 0
    meta = migrate_dataset(args.data_dir, args.dataset_name, pl, args.new, args.out)
    print(f"{args.out}: {len(meta['index'])} rows, {grew}; <oov> cells {sum(meta['oov_rows'].values())}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
