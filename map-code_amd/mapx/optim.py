"""Optimizer of the hot path: transformers-4.26 AdamW + cosine/const schedule, as the
reference's Trainer.get_optimizer builds it (code/trainer.py:60-85), on device.

* dense parameters live in two flat fp32 buffers (decay / no-decay group, split by the
  reference's NAME rule) and take one fused kernel per group per step;
* the [V,*] tables take row-sparse updates with exact lazy replay of the zero-gradient
  updates the reference applies to untouched rows (csrc/optim.hip);
* {step size, lr} per update come from a device table and the update counter is a device
  int, so nothing is synchronised with the host during training.
"""
import math

import torch

from . import ops

NO_DECAY = ("bias", "LayerNorm.weight")          # trainer.py:61


def decays(name):
    return not any(nd in name for nd in NO_DECAY)


def lr_lambda(kind, step, total, warmup):
    """get_{cosine,constant}_schedule_with_warmup multiplier at scheduler step `step`."""
    kind = kind.lower()
    if kind not in ("cosine", "const"):
        raise NotImplementedError(kind)                       # trainer.py:82-83
    if step < warmup:
        return float(step) / float(max(1, warmup))
    if kind == "const":
        return 1.0
    progress = float(step - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


class TableAdam:
    """Lazy exact AdamW state of one RowTable."""

    def __init__(self, table, wd0, wd1, hyper, sched, done, aux, max_gap):
        self.table, self.wd0, self.wd1, self.aux = table, wd0, wd1, aux
        self.b1, self.b2, self.eps = hyper
        self.sched, self.done = sched, done
        p0, p1 = table.p0.data, (table.p1.data if table.p1 is not None else None)
        # a row's two moments side by side in ONE record [V, 2 W] (m | v): the update reads and writes two random
        # places per row (the parameter row and this record) instead of three — random rows cost per access, not
        # per byte (csrc/optim.hip TableGroup).  m0 / v0 (m1 / v1) are views of the halves.
        W = p0.shape[1]
        self.mv0 = torch.zeros(p0.shape[0], 2 * W, dtype=p0.dtype, device=p0.device)
        self.m0, self.v0 = self.mv0[:, :W], self.mv0[:, W:]
        self.m1 = self.v1 = self.mv1 = None
        if p1 is not None:
            self.mv1 = torch.zeros(p1.shape[0], 2, device=p1.device)
            self.m1, self.v1 = self.mv1[:, 0], self.mv1[:, 1]
        self.last = torch.zeros(p0.shape[0], dtype=torch.int32, device=p0.device)
        self.stale = False
        self.cursor = 0
        # max_gap > 0: also bring V/max_gap rows up to date every step (round robin).  Not needed
        # for speed since replays have a closed-form tail (csrc/optim.hip); kept for testing.
        self.sweep = math.ceil(p0.shape[0] / max_gap) if max_gap > 0 else 0
        table.lazy = self

    def _call(self, **kw):
        t = self.table
        ops.table_adam(t.p0.data, self.m0, self.v0, self.wd0, self.last, self.sched, self.done,
                       self.aux, self.b1, self.b2, self.eps,
                       p1=t.p1.data.view(-1) if t.p1 is not None else None,
                       m1=self.m1, v1=self.v1, wd1=self.wd1, **kw)

    def catch_up(self, plan):
        self._call(rows=plan.uniq, n_rows=plan.n, n_rows_dev=plan.n_uniq)

    def refresh_coef(self):
        """This step's replay coefficients (ops.replay_coef_table) for the kernels that take lazy_rows()."""
        self.coef = ops.replay_coef_table(self.aux, self.b1, self.b2, self.done, getattr(self, "coef", None))

    def lazy_rows(self):
        """native.LazyRows over this table's state (include/mapx_hip.h: mapx_lazy_rows)."""
        from . import native as N
        if getattr(self, "coef", None) is None:
            self.refresh_coef()
        lz = N.LazyRows()
        lz.m0, lz.v0, lz.ld_mv0, lz.wd0 = self.m0.data_ptr(), self.v0.data_ptr(), self.m0.stride(0), self.wd0
        if self.m1 is not None:
            lz.m1, lz.v1, lz.ld_mv1, lz.wd1 = self.m1.data_ptr(), self.v1.data_ptr(), self.m1.stride(0), self.wd1
        else:
            lz.m1, lz.v1, lz.ld_mv1, lz.wd1 = None, None, 1, 0.0
        lz.last, lz.sched, lz.sched_len, lz.done = self.last.data_ptr(), self.sched.data_ptr(), self.sched.shape[0], self.done.data_ptr()
        lz.aux, lz.aux_len, lz.aux_rows = self.aux.data_ptr(), self.aux.shape[1], self.aux.shape[0]
        lz.beta1, lz.beta2, lz.eps = self.b1, self.b2, self.eps
        lz.coef_opt = self.coef.data_ptr()
        return lz

    def catch_up_raw(self, keys_i32):
        """Catch-up straight from a raw id list (repeats allowed; no sort on the critical path)."""
        self._call(rows=keys_i32, n_rows=keys_i32.numel(), rows_may_repeat=True)

    def update(self):
        sg = self.table.sparse_grad
        if sg is None:
            return
        plan, r0, r1 = sg
        self._call(rows=plan.uniq, n_rows=plan.n, n_rows_dev=plan.n_uniq, grad0=r0, grad1=r1)
        self.table.sparse_grad = None
        self.stale = True

    def sweep_some(self):
        """Bound the replay length: every row is brought up to date at least every max_gap steps."""
        if self.sweep <= 0:
            return
        V = self.table.num_rows
        n = min(self.sweep, V - self.cursor)
        self._call(row_begin=self.cursor, n_rows=n)
        self.cursor = (self.cursor + n) % V

    def flush(self):
        if self.stale:
            self._call(row_begin=0, n_rows=self.table.num_rows)
            self.stale = False


class MapxOptimizer:
    """optimizer + scheduler of reference Trainer.get_optimizer, fused.  `step()` = the
    reference's optimizer.step(); scheduler.step(); model.zero_grad()."""

    def __init__(self, model, args, num_training_steps, num_warmup_steps, max_gap=0):
        b1, b2 = (float(x) for x in args.adam_betas.split(","))
        self.hyper = (b1, b2, float(args.adam_epsilon))
        self.lr0, self.wd = float(args.learning_rate), float(args.weight_decay)
        self.kind, self.total, self.warmup = args.lr_sched.lower(), int(num_training_steps), int(num_warmup_steps)
        self.max_grad_norm = float(getattr(args, "max_grad_norm", 0.0))
        lambdas = [lr_lambda(self.kind, s, self.total, self.warmup) for s in range(max(1, self.total))]
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("MapxOptimizer needs the model on the GPU (call model.to(device) first)")
        self.sched = ops.make_sched(self.lr0, lambdas, b1, b2).to(dev)
        self.aux = ops.make_replay_aux(self.lr0, lambdas, b1, b2, self.wd).to(dev)
        self.done = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps_done = 0                         # (kept in an ops.PlaneClock: the weight planes' stamps are read against it)
        table_ids = model.table_parameter_ids()
        named = [(n, p) for n, p in model.named_parameters() if id(p) not in table_ids and p.requires_grad]
        self.dense_params = [p for _, p in named]
        # bf16 compute mode: every dense weight gets a bf16 shadow (`p._mapx_bf16`, the operand of the
        # bf16 GEMMs) inside one flat buffer per group, written by the AdamW kernel with the update
        from .layers import compute_dtype_of
        self.bf16 = compute_dtype_of(getattr(model, "config", None)) == torch.bfloat16
        self.groups = []
        for wd, members in ((self.wd, [(n, p) for n, p in named if decays(n)]),
                            (0.0, [(n, p) for n, p in named if not decays(n)])):
            if members:
                self.groups.append(self._flatten(members, wd, dev, self.bf16))
        for p in self.dense_params:
            if getattr(p, "_planes", None) is not None:
                p._planes_clock = self._clock
        self.refresh_bf16()
        names = {id(p): n for n, p in model.named_parameters()}
        self.tables = []
        for t in model.row_tables():
            wd0 = self.wd if decays(names[id(t.p0)]) else 0.0
            wd1 = (self.wd if decays(names[id(t.p1)]) else 0.0) if t.p1 is not None else 0.0
            self.tables.append(TableAdam(t, wd0, wd1, self.hyper, self.sched, self.done, self.aux, max_gap))
        # (int64 device cursor, stride) of a captured step that walks the epoch's permutation: moved to the next
        # batch by the launch that advances the update counter (trainer.GraphedStep sets it around its capture)
        self.walk_cursor = None

    @property
    def steps_done(self):
        return self._clock.step

    @steps_done.setter
    def steps_done(self, n):
        if "_clock" not in self.__dict__:
            self._clock = ops.PlaneClock()
        self._clock.step = int(n)

    def plane_keys(self):
        """The plane sets registered now: what the refresh launches of an optimizer step captured now re-cut on every
        replay (ops.PlaneClock)."""
        return ops.plane_keys(self.dense_params)

    def replayed(self, keys):
        """A captured step() that re-cuts the plane sets `keys` has been replayed (a replay runs no Python)."""
        self._clock.replayed(keys)

    def planes_ready(self, keys):
        """Before a captured forward that reads the plane sets `keys` is replayed: whatever wrote the weights last
        re-cut them — else (another graph's replay that knows fewer sets) the stale ones are cut here."""
        if keys and not self._clock.covers(keys):
            ops.refresh_weight_planes(self.dense_params, stale_only=True)

    def backward_window(self, open_):
        """Between backward_window(True) and (False) — the Trainer brackets loss.backward() of a step
        whose optimizer.step() follows at once — backward nodes may leave side streams open and queue work for
        optimizer.step() to pick up (ops.pending_joins, late and main tasks).  Outside the window backward() joins
        what it forked itself."""
        if open_:
            ops.clear_side_tasks()      # leftovers of a backward pass that raised
        ops.step_window[0] = bool(open_)

    FLAT_PAD = 8          # elements every parameter's slot of a flat buffer is rounded up to (saved with the state)

    @staticmethod
    def _flatten(members, wd, dev, bf16=False):
        pad = MapxOptimizer.FLAT_PAD
        sizes = [(p.numel() + pad - 1) // pad * pad for _, p in members]   # every view 16-B aligned (fp32 and bf16)
        total = sum(sizes)
        flat_p = torch.zeros(total, device=dev)
        flat_g = torch.zeros(total, device=dev)
        flat_h = torch.zeros(total, dtype=torch.bfloat16, device=dev) if bf16 else None
        # fp32 mode: every parameter's magnitude record (ops: "Magnitude records"), kept current by the AdamW kernel
        # with what it writes — `p._amax` is what the GEMMs that read p as an operand look at
        recs = None if (bf16 or not ops.H2) else torch.zeros(len(members), ops.REC, dtype=torch.int32, device=dev)
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + sz)
        off = 0
        for i, ((_, p), sz) in enumerate(zip(members, sizes)):
            # (FiGNN's graph, GRU and W_attn parameters are read by row-resident kernels only, never as a GEMM operand:
            # no record is attached to them and no planes are kept; their rows of `recs` are written and never read)
            if recs is not None and not getattr(p, "_mapx_row_resident", False):
                p._amax = recs[i]
                if p.dim() == 2:
                    p._planes = {}           # ops.weight_planes: filled at first use, refreshed behind every update
                    p._planes_at = {}        # ... and the update count each set was cut at (ops.PlaneClock)
            view = flat_p[off:off + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = None
            p._mapx_grad = flat_g[off:off + p.numel()].view_as(p)   # backward kernels write here
            p._mapx_bf16 = flat_h[off:off + p.numel()].view_as(p) if bf16 else None
            off += sz
        return dict(p=flat_p, g=flat_g, m=torch.zeros_like(flat_p), v=torch.zeros_like(flat_p), wd=wd,
                    names=[n for n, _ in members], numels=[p.numel() for _, p in members], h=flat_h,
                    amax=recs, seg_off=torch.tensor(offs, dtype=torch.int64, device=dev) if recs is not None else None,
                    params=[p for _, p in members])

    def refresh_bf16(self):
        """Re-derive what the optimizer keeps beside the fp32 master weights — the bf16 shadows (bf16 mode), the
        magnitude records (fp32 mode) — after anything other than step() wrote the parameters (construction,
        load_model / load_state_dict, a test poking .data)."""
        for g in self.groups:
            if g.get("amax") is not None:
                for p, rec in zip(g["params"], g["amax"]):
                    if getattr(p, "_mapx_row_resident", False):
                        continue
                    ops.amax(p.data.reshape(1, -1) if p.dim() != 2 else p.data, rec=rec, reset=True)
                    p._amax_ver = p._version
                    ops.refresh_weight_planes(p)
        if not self.bf16:
            return
        for g in self.groups:
            ops.check(ops.lib.mapx_cast_f32_bf16(ops.ptr(g["p"]), g["p"].numel(), ops.ptr(g["h"]), ops.stream()))

    # ------------------------------------------------------------------
    def clip_grad_norm_(self):
        sq = sum((g["g"] ** 2).sum() for g in self.groups)
        for t in self.tables:
            if t.table.sparse_grad is not None:
                plan, r0, r1 = t.table.sparse_grad
                if plan.n_uniq is None:          # gathered list (mapx.parallel): padding rows are zero
                    live = torch.ones(r0.shape[0], dtype=torch.bool, device=r0.device)
                else:
                    live = torch.arange(r0.shape[0], device=r0.device) < plan.n_uniq[0]
                # rows at and beyond n_uniq are never written (ops.seg_reduce_rows: torch.empty): selected out, not
                # multiplied by zero — what the allocator left there may be inf or NaN, and NaN * 0 is NaN
                zero = torch.zeros((), dtype=r0.dtype, device=r0.device)
                sq = sq + torch.where(live, (r0 ** 2).sum(1), zero).sum()
                if r1 is not None:
                    sq = sq + torch.where(live, r1.view(-1) ** 2, zero).sum()
        coef = (self.max_grad_norm / (sq.sqrt() + 1e-6)).clamp(max=1.0)
        for g in self.groups:
            g["g"].mul_(coef)
        for t in self.tables:
            if t.table.sparse_grad is not None:
                _, r0, r1 = t.table.sparse_grad
                r0.mul_(coef)
                if r1 is not None:
                    r1.mul_(coef)

    def collect_torch_grads(self):
        """Parameters that a model uses through plain torch ops (e.g. DeepFM's one-element LR bias)
        get their gradient in `.grad`, not in the flat buffer the fused kernels write: move it."""
        moved = 0
        for p in self.dense_params:
            if p.grad is not None:
                p._mapx_grad.copy_(p.grad)
                p.grad = None
                moved += 1
        return moved

    def step(self):
        ops.run_main_tasks()            # stream joins nobody picked up
        main = torch.cuda.current_stream() if torch.cuda.is_available() else None
        ev, ev_stream = ops.dense_ready
        from . import parallel
        ops.join_pending()              # side work a backward node forked and left open
        ops.run_late_tasks()            # optimizer-only gradients nobody picked up
        moved = self.collect_torch_grads()
        ops.dense_ready[0] = ops.dense_ready[1] = None
        # (the copies collect_torch_grads enqueued on the main stream come AFTER the dense-ready event: a side
        # stream that waits for that event alone could read the flat gradient before they land)
        if ev is not None and moved == 0 and self.max_grad_norm <= 0 and ev_stream == main \
                and not parallel.exchanging():
            # The dense half (partial sums + dense AdamW, HBM-bound, ~30 us) beside the tables' half (the
            # embedding gradient's reduction + row updates, ~30 us) instead of behind it: it forks from the
            # point where the dense gradients were final, on the tower stream, which is idle by then.
            with ops.Fork(ops.aux_stream("tower", self.done.device), main, event=ev) as fork:
                ops.flush_deferred()
                self._dense_update()
            for t in self.tables:
                t.update()
            fork.join()
        else:
            ops.flush_deferred()            # split-K slabs / colsum partials of this backward pass
            if self.max_grad_norm > 0:
                self.clip_grad_norm_()
            self._dense_update()
            for t in self.tables:
                t.update()
        ops.step_advance(self.done, *(self.walk_cursor or ()))
        self.steps_done += 1
        for t in self.tables:
            t.sweep_some()
        self.zero_grad()

    def _dense_update(self):
        b1, b2, eps = self.hyper
        for g in self.groups:
            ops.adamw_dense(g["p"], g["g"], g["m"], g["v"], self.sched, self.done, b1, b2, eps, g["wd"],
                            shadow=g["h"], seg_off=g.get("seg_off"), seg_amax=g.get("amax"))
        # the weights' fp16 pieces for the next step's products, stamped with the count step() is about to reach (a
        # capture runs no kernel and stamps nothing: its replays report the sets they re-cut, MapxOptimizer.replayed)
        eager = not torch.cuda.is_current_stream_capturing()
        for g in self.groups:
            if g.get("amax") is not None:
                ops.refresh_weight_planes(g["params"], at=self.steps_done + 1, stamp=eager)

    def zero_grad(self):
        """Dense gradients are overwritten by the next backward (see layers._grad_slot); only
        the sparse side channel needs clearing."""
        for t in self.tables:
            t.table.sparse_grad = None
        ops.dense_ready[0] = ops.dense_ready[1] = None

    def flush(self):
        """Materialise reference-equivalent table weights (before eval / checkpoint)."""
        for t in self.tables:
            t.flush()

    # ------------------------------------------------------------------ resume state
    def state_dict(self):
        """Everything needed to continue training bit-exactly: dense and table Adam moments, the
        per-row replay clocks, the update counter.  (The reference saves model weights only and
        cannot resume mid-run: trainer.py:517-519.)"""
        return dict(steps_done=self.steps_done, done=self.done.cpu(), flat_pad=self.FLAT_PAD,
                    groups=[dict(names=g["names"], m=g["m"].cpu(), v=g["v"].cpu()) for g in self.groups],
                    tables=[dict(name=t.table.name, m0=t.m0.contiguous().cpu(), v0=t.v0.contiguous().cpu(),
                                 m1=None if t.m1 is None else t.m1.contiguous().cpu(),
                                 v1=None if t.v1 is None else t.v1.contiguous().cpu(), last=t.last.cpu(),
                                 stale=t.stale, cursor=t.cursor) for t in self.tables])

    def load_state_dict(self, sd):
        self.steps_done = int(sd["steps_done"])
        self.done.copy_(sd["done"])
        saved_pad = sd.get("flat_pad")
        for g, s in zip(self.groups, sd["groups"]):
            if g["names"] != s["names"]:
                raise ValueError("optimizer state: the parameter list changed since the state was saved")
            sizes = g["numels"]
            if s["v"].numel() != s["m"].numel():
                raise ValueError("optimizer state: m and v of a group differ in length")
            if s["m"].numel() == g["m"].numel() and saved_pad in (None, self.FLAT_PAD):
                g["m"].copy_(s["m"])
                g["v"].copy_(s["v"])
                continue
            # another slot size: the flat moments do not line up — re-pack them parameter by parameter.  States
            # written before the `flat_pad` key existed used slots of 4, then of 8 elements: take the one that fits.
            fits = [pad for pad in ([int(saved_pad)] if saved_pad is not None else [8, 4])
                    if sum((n + pad - 1) // pad * pad for n in sizes) == s["m"].numel()]
            if not fits:
                raise ValueError(f"optimizer state: flat moments of {s['m'].numel()} elements do not match the "
                                 f"parameters at a slot size of {saved_pad if saved_pad is not None else '8 or 4'}")
            pad = fits[0]
            src_off = dst_off = 0
            for n in sizes:
                for key in ("m", "v"):
                    g[key][dst_off:dst_off + n].copy_(s[key][src_off:src_off + n])
                src_off += (n + pad - 1) // pad * pad
                dst_off += (n + self.FLAT_PAD - 1) // self.FLAT_PAD * self.FLAT_PAD
        for t, s in zip(self.tables, sd["tables"]):
            assert t.table.name == s["name"]
            t.m0.copy_(s["m0"]); t.v0.copy_(s["v0"]); t.last.copy_(s["last"])
            if t.m1 is not None:
                t.m1.copy_(s["m1"]); t.v1.copy_(s["v1"])
            t.stale, t.cursor = bool(s["stale"]), int(s["cursor"])
        self.refresh_bf16()

    def get_last_lr(self):
        return [self.lr0 * lr_lambda(self.kind, self.steps_done, self.total, self.warmup)]
