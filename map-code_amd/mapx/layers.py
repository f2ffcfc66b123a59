"""DCNv2 building blocks over the gfx950 kernels (host mirror of reference code/layers.py:
Embeddings :83-102, MLPBlock :173-188, CrossNetV2 :191-201).  autograd.Function = glue only:
every forward/backward body is a C-ABI call (mapx.ops)."""
import copy
import math
import os

import torch
from torch import nn
from torch.autograd import Function

from . import ops, parallel


def compute_dtype_of(config):
    """torch dtype of the trunk's activations: Config key `compute_dtype` ("fp32" default | "bf16")."""
    name = str(getattr(config, "compute_dtype", "fp32") or "fp32").lower()
    if name in ("fp32", "float32", "f32"):
        return torch.float32
    if name in ("bf16", "bfloat16"):
        return torch.bfloat16
    raise NotImplementedError(f"compute_dtype={name!r}: fp32 | bf16")


# ----------------------------------------------------------------------------- row tables
def _side_stream(device, table_name=""):
    """All tables' plans share one side stream.  (One stream per table was tried: inside the
    captured graph the embedding table's sort then ran at the very end of the step and the
    optimizer waited 70 us for it.)"""
    return ops.aux_stream("plan", device)


class RowTable:
    """A [V, W] parameter table read by row id, with row-sparse gradients.

    The reference keeps such tables as nn.Embedding with DENSE gradients and lets AdamW sweep
    all V rows every step.  Here the gradient of a step is (plan.uniq, rows) — see
    csrc/segreduce.h — and the optimizer (mapx.optim.TableAdam) updates touched rows only,
    replaying the zero-gradient updates the reference would have applied to a row when the
    row is next read (`prepare`) or when the table is flushed."""

    def __init__(self, name, p0, p1=None):
        self.name, self.p0, self.p1 = name, p0, p1
        self.sparse_grad = None      # (plan, rows0, rows1|None) after backward
        self.lazy = None             # TableAdam state once an optimizer is attached
        self.plan = None

    @property
    def num_rows(self):
        return self.p0.shape[0]

    def prepare(self, keys_i32, need_plan, defer_plan=False, through_replay=False):
        """Called by the forward pass with this step's row ids (repeats allowed).
        * stale rows among them are brought up to date on the current stream, straight from the
          raw id list (ownership by atomicCAS in the kernel): nothing on the critical path
          waits for a sort;
        * when gradients will be needed, the segment plan (sort + runs) is built on a side
          stream, concurrently with the forward/backward GEMMs, and joined in backward.  With
          `defer_plan` the caller picks the fork point by calling start_plan() once the kernels
          that must not queue behind the sort are enqueued (a captured graph keeps the first
          forked branch on the parent's queue); backward starts it itself if nobody did."""
        self.plan = PlanSlot(self, keys_i32) if need_plan else None      # fork point: keys are final
        # `stale` is a host flag of the moment this code runs; a step being CAPTURED is replayed
        # many times, nearly always with stale rows, so the catch-up is always part of a capture
        # (it is a read of last[] and nothing else for rows that are current).  Capturing right
        # after a flush (stale == False: first step of an epoch, or after eval / save) otherwise
        # gave a graph whose replays read rows that had missed their zero-gradient updates.
        # through_replay: the kernel that reads these rows replays a stale row's missing updates in registers
        # (ops.nce_fwd(lazy=)) and the gradient update that ends the step writes it once — no catch-up pass; what
        # is refreshed instead is the step's table of replay coefficients (one tiny launch).
        if self.lazy is not None and through_replay:
            self.lazy.refresh_coef()
        elif self.lazy is not None and (self.lazy.stale or torch.cuda.is_current_stream_capturing()):
            self.lazy.catch_up_raw(keys_i32)
        if need_plan and not defer_plan:
            self.plan.start()
        return self.plan

    def start_plan(self, after=None):
        """`after`: a stream whose work enqueued so far the sort must not delay (PlanSlot.start_many)."""
        if self.plan is not None:
            self.plan.start(after=after)

    def join_plan(self, device):
        """Make the current stream wait for the plan being built on this table's side stream."""
        ops.stream_wait(torch.cuda.current_stream(), _side_stream(device, self.name))

    def dense_grad(self):
        """Reference-layout dense gradients [(V,W), (V,1)|None] from the sparse ones (tests)."""
        plan, r0, r1 = self.sparse_grad
        if plan.n_uniq is None:                      # gathered list with -1 padding (mapx.parallel)
            keep = plan.uniq >= 0
            uniq, r0 = plan.uniq[keep].long(), r0[keep]
            r1 = r1[keep] if r1 is not None else None
        else:
            U = plan.count()
            keep = plan.uniq[:U] >= 0                # a merged list ends with the -1 padding run
            uniq, r0 = plan.uniq[:U][keep].long(), r0[:U][keep]
            r1 = r1[:U][keep] if r1 is not None else None
        g0 = torch.zeros_like(self.p0).index_copy_(0, uniq, r0)
        g1 = None
        if self.p1 is not None:
            g1 = torch.zeros_like(self.p1).index_copy_(0, uniq, r1.unsqueeze(1))
        return g0, g1


# "1": a training step's embedding gather replays stale rows in registers instead of a catch-up launch in front of it
# (the first kernels of the step's critical chain: mask -> catch-up -> gather -> first GEMM).  Built, bit-identical,
# and worth nothing on the step (one box, tools/ab_env.sh): gather 5.0 -> 9.0 us, the 7.9-us catch-up launch gone,
# the update +1.4 us: 0.6884 / 0.6907 ms per step against 0.6880 / 0.6899 with the catch-up pass.  Opt-in.
EMB_LAZY_FOLD = os.environ.get("MAPX_EMB_LAZY_FOLD", "0") == "1"

# callables (table, plan) run on the plan stream right after a table's plan has been enqueued
# (trainer.GraphedBackward publishes the plan's unique-row count to the host from there)
plan_observers = []


class PlanSlot:
    """This step's segment plan of one table: created by prepare(), filled by start() on the
    side stream, read (after join_plan) by the backward kernels through get().

    The sort depends on the key list only, so the slot remembers the point where the keys
    became final (an event) and start() forks from THAT point whenever it is called.  Callers
    call start() late — after the kernels of the critical chain are enqueued — because a
    captured hipGraph keeps the first-captured successor of a node on the node's own queue and
    makes the later ones wait on another queue (measured: a sort chain captured first delayed
    the trunk's first GEMM by 150 us)."""

    def __init__(self, table, keys_i32):
        self.table, self.keys, self.value = table, keys_i32, None
        self.origin = torch.cuda.current_stream()
        self.ready = ops.record_event()

    def start(self, after=None):
        if self.value is not None:
            return
        keys, self.keys = self.keys, None
        side = _side_stream(keys.device, self.table.name)
        # (after: see start_many: left to itself the graph runtime runs the chain LAST)
        with ops.Fork(side, self.origin, event=self.ready, after=after) as fork:
            self.value = ops.SegPlan(keys, self.table.num_rows)
            for observe in plan_observers:
                observe(self.table, self.value)
        fork.reads(keys)
        fork.produces(*self.value.tensors())

    MAX_PER_CHAIN = 2       # key lists one chain of launches sorts (csrc/radixsort.h kMaxSortProbs)

    @staticmethod
    def start_many(slots, implied=(), after=None):
        """Build the plans of several tables' slots with ONE chain of launches (ops.SegPlan.build_many:
        both sorts of a step cost one sort's chain of dependent kernels).  The side stream waits for
        every slot's keys; slots that were started already are left alone."""
        slots = [s for s in slots if s is not None and s.value is None]
        if len(slots) <= 1:
            for s in slots:
                s.start(after=after)
            return
        if len(slots) > PlanSlot.MAX_PER_CHAIN:        # (FGCNN + MFP: two embedding tables and the NCE table)
            for i in range(0, len(slots), PlanSlot.MAX_PER_CHAIN):
                PlanSlot.start_many(slots[i:i + PlanSlot.MAX_PER_CHAIN], implied=implied, after=after)
            return
        keys = [s.keys for s in slots]
        side = _side_stream(keys[0].device)
        # `implied`: slots whose keys are known to be final once the OTHER slots' events have fired (the
        # caller's stream order guarantees it): the side stream then forks from one point of the step
        # instead of joining two streams (measured: no difference, 0.756 vs 0.757 ms in bf16 mode)
        # `after`, on the last fork: also behind what that stream has enqueued so far: the graph runtime runs a
        # side chain AHEAD of later-captured work of the queue it lands on, so the caller names the kernels the
        # chain must not delay (bf16 mode: the deep tower's GEMMs waited 140 us behind the sort)
        waited = [(s, k) for s, k in zip(slots, keys) if s not in implied]
        forks = [ops.Fork(side, s.origin, event=s.ready, after=after if s is waited[-1][0] else None)
                 for s, _ in waited]
        with forks[-1]:
            plans = ops.SegPlan.build_many(keys, [s.table.num_rows for s in slots])
            for s, plan in zip(slots, plans):
                s.value, s.keys = plan, None
                for observe in plan_observers:
                    observe(s.table, plan)
        for fork, (s, k) in zip(forks, waited):
            fork.reads(k)
            fork.produces(*s.value.tensors())

    def get(self):
        """The plan, usable on the current stream."""
        self.start()
        self.table.join_plan(self.value.uniq.device)
        return self.value


class TableWeight(nn.Module):
    """Holds `weight` [V, W] under the attribute name the reference's nn.Embedding has."""

    def __init__(self, num_rows, width):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_rows, width))

    @property
    def embedding_dim(self):
        return self.weight.shape[1]


class _Gather(Function):
    @staticmethod
    def forward(ctx, weight, ids, table, out_dtype=torch.float32, lazy=None):
        ctx.table, ctx.plan, ctx.width = table, table.plan, weight.shape[1]
        return ops.emb_gather(ids, weight, out_dtype=out_dtype, lazy=lazy)

    @staticmethod
    def backward(ctx, g):
        if ctx.plan is None:
            raise RuntimeError("embedding backward without a segment plan")
        if getattr(ctx.table, "mark_dense_ready", False) and not parallel.exchanging():
            # this node is the model's last: every dense gradient of THIS stream is enqueued (the tower stream's
            # are behind it in that stream's own order, which is where the optimizer's dense half runs) — the
            # optimizer's dense half need not wait for the table's
            ops.dense_ready[0], ops.dense_ready[1] = ops.record_event(), torch.cuda.current_stream()
        plan = ctx.plan.get()
        g = g.contiguous().view(-1, ctx.width)           # bf16 rows in bf16 mode: summed in fp32
        ops.dbg_sleep("gather_bwd")
        g2, link = None, getattr(ctx.table, "x0_link", None)
        if link is not None and link.g is not None:
            # the cross tower's dL/dX0, left aside by its backward node (_X0Link): summed with the deep tower's
            # inside the reduction; this stream waits for the cross chain's LAST GEMM only, not for what that
            # stream runs behind it (the NCE table's gradient and update, the encoder's dW: ~120 us)
            g2, ev, st, link.g = link.g.view(-1, ctx.width), link.event, link.stream, None
            if g.is_cuda and ops.stream_wait_event(torch.cuda.current_stream(), ev, st):
                g2.record_stream(torch.cuda.current_stream())
            if g2.dtype != g.dtype or g2.shape != g.shape:
                g, g2 = g + g2, None
        ctx.table.sparse_grad = (plan, ops.seg_reduce_rows(plan, g, ctx.width, src2=g2), None)
        if not ops.step_window[0]:
            ops.join_pending()            # no optimizer.step() follows at once: leave nothing open behind backward()
        return None, None, None, None, None


class _GatherLinear(Function):
    """Embedding rows [B,F,E] and the LR term sum_f w[id] [B] from one id matrix; backward reduces
    both gradients with the table's one segment plan (rows + a scalar per batch row)."""

    @staticmethod
    def forward(ctx, weight, lin_weight, ids, table, out_dtype=torch.float32):
        ctx.table, ctx.plan, ctx.width, ctx.F = table, table.plan, weight.shape[1], ids.shape[1]
        x = ops.emb_gather(ids, weight, out_dtype=out_dtype)      # bf16 rows in bf16 compute mode
        lr = ops.lr_sum(ids, lin_weight.view(-1))                 # the LR sum stays fp32
        return x, lr

    @staticmethod
    def backward(ctx, gx, glr):
        if ctx.plan is None:
            raise RuntimeError("embedding backward without a segment plan")
        plan = ctx.plan.get()
        gx = gx.contiguous().view(-1, ctx.width)          # bf16 rows in bf16 mode: summed in fp32, like the scalar
        rows0, rows1 = ops.seg_reduce_rows_extra(plan, gx, ctx.width, glr.contiguous().view(-1), ctx.F)
        ctx.table.sparse_grad = (plan, rows0, rows1)
        return None, None, None, None, None


class _FmProductSum(Function):
    """InnerProductLayer(output='product_sum') (reference layers.py:123-131) on [B,F,E] -> [B,1].
    bf16 x3 (bf16 compute mode): the term and the field sums stay fp32, backward returns bf16 dx."""

    @staticmethod
    def forward(ctx, x3):
        x3 = x3.contiguous()
        out, s = ops.fm_fwd(x3)
        ctx.save_for_backward(x3, s)
        return out.view(-1, 1)

    @staticmethod
    def backward(ctx, g):
        x3, s = ctx.saved_tensors
        return ops.fm_bwd(g.contiguous().view(-1), s, x3)


def fm_product_sum(x3):
    return _FmProductSum.apply(x3)


class _ToBf16(Function):
    """An fp32 tensor enters the bf16 trunk (DeepFM's lr + fm column of the heads' input): rounded once by the
    library's cast kernel; its gradient comes back as fp32."""

    @staticmethod
    def forward(ctx, x):
        return ops.cast_bf16(x)

    @staticmethod
    def backward(ctx, g):
        return ops.cast_f32(g) if ops.is_bf16(g) else g


def to_bf16(x):
    return _ToBf16.apply(x)


class _Dropout(Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset, offset_dev, out):
        ctx.cfg = (p, seed, offset, offset_dev)
        if out is not None and not out.is_contiguous():      # a column slice of the concatenated buffer
            out.copy_(ops.dropout(x, p, seed, offset, offset_dev))
            return out
        return ops.dropout(x, p, seed, offset, offset_dev, out=out)

    @staticmethod
    def backward(ctx, g):
        p, seed, offset, offset_dev = ctx.cfg
        return ops.dropout(g.contiguous(), p, seed, offset, offset_dev), None, None, None, None, None


class HipDropout(nn.Module):
    """nn.Dropout(p) (reference layers.py:95, 183) with a Philox mask that is regenerated, not stored.
    Every site owns a Philox stream; inside a Trainer the stream advances with the optimizer's
    device-side update counter (`step_counter`), so a captured step replays with fresh masks."""
    _sites = 0

    def __init__(self, p):
        super().__init__()
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout probability has to be in [0, 1), but got {p}")
        self.p = float(p)
        HipDropout._sites += 1
        self.site, self.seed, self.rank, self._calls, self.step_counter = HipDropout._sites, 42, 0, 0, None

    def forward(self, x, out=None):
        if not self.training or self.p == 0.0:
            if out is not None and out.data_ptr() != x.data_ptr():
                out.copy_(x)
                return out
            return x
        base = (self.rank << 48) + ((16 + self.site) << 36)
        if self.step_counter is not None:
            offset, dev = base, self.step_counter
        else:
            self._calls += 1
            offset, dev = base + self._calls, None
        return _Dropout.apply(x, self.p, self.seed, offset, dev, out)


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        shape = x.shape
        x2 = x.contiguous().view(-1, shape[-1])
        y, stats = ops.layernorm_fwd(x2, w, b, eps)
        ctx.slots = (_grad_slot(w), _grad_slot(b))
        ctx.save_for_backward(x2, w, stats)
        return y.view(shape)

    @staticmethod
    def backward(ctx, g):
        x2, w, stats = ctx.saved_tensors
        sw, sb = ctx.slots
        g2 = g.contiguous().view(-1, x2.shape[1])
        dx, dyx = ops.layernorm_bwd(g2, x2, w, stats)
        dw = ops.colsum(dyx, out=sw)
        db = ops.colsum(g2, out=sb)
        return dx.view(g.shape), (None if sw is not None else dw), (None if sb is not None else db), None


class _AddLayerNorm(Function):
    """bf16 compute mode: y = LN(x + s) (s None: LN(x)) on bf16 rows in one kernel.  The fp32 sum is normalised without
    being stored, so it is not rounded; backward recomputes it from the two saved addends and returns ONE bf16 tensor
    as the gradient of both.  dL/dw and dL/db leave the backward kernel as fp32 partial rows, summed with the step's
    other deferred sums (ops.flush_deferred) when the optimizer owns the parameters."""

    @staticmethod
    def forward(ctx, x, s, w, b, eps):
        shape = x.shape
        x2 = x.contiguous().view(-1, shape[-1])
        s2 = s.contiguous().view(-1, shape[-1]) if s is not None else None
        y, stats = ops.add_layernorm_fwd(x2, s2, w, b, eps)
        ctx.slots = (_grad_slot(w), _grad_slot(b))
        ctx.has_s = s is not None
        ctx.save_for_backward(x2, s2, w, stats)
        return y.view(shape)

    @staticmethod
    def backward(ctx, g):
        x2, s2, w, stats = ctx.saved_tensors
        sw, sb = ctx.slots
        g2 = g.contiguous().view(-1, x2.shape[1])
        if not ops.is_bf16(g2):
            g2 = ops.cast_bf16(g2)
        dsum, dw, db = ops.add_layernorm_bwd(g2, x2, s2, w, stats, dw=sw, db=sb, defer=sw is not None and sb is not None)
        dsum = dsum.view(g.shape)
        return (dsum, dsum if ctx.has_s else None, (None if sw is not None else dw), (None if sb is not None else db),
                None)


class HipLayerNorm(nn.Module):
    """nn.LayerNorm(E, eps): `weight`, `bias` [E] (ones / zeros), normalisation over the last dimension.
    bf16 input (the Transformer in bf16 compute mode): the bf16 kernel pair, which also takes the residual addend."""

    def __init__(self, width, eps):
        super().__init__()
        self.eps = float(eps)
        self.weight = nn.Parameter(torch.ones(width))
        self.bias = nn.Parameter(torch.zeros(width))

    def forward(self, x, add=None):
        """`add` (bf16 mode only): LN(x + add), the sum formed inside the kernel."""
        if ops.is_bf16(x):
            return _AddLayerNorm.apply(x, add, self.weight, self.bias, self.eps)
        if add is not None:
            raise NotImplementedError("the fused residual add + LayerNorm is the bf16 kernel pair")
        return _LayerNorm.apply(x, self.weight, self.bias, self.eps)


MAX_EMBED_SIZE = 256      # csrc/segreduce.h: seg_reduce_launch refuses wider rows (inside the first backward otherwise)


class Embeddings(nn.Module):
    """One shared id space over all fields (reference layers.py:83-102): gather, optional LayerNorm
    over the embedding width (`embed_norm`), optional dropout (`embed_dropout_rate`)."""

    def __init__(self, config):
        super().__init__()
        self.embed_norm = bool(getattr(config, "embed_norm", False))
        p_drop = float(getattr(config, "embed_dropout_rate", 0.0) or 0.0)
        if (self.embed_norm or p_drop > 0) and compute_dtype_of(config) != torch.float32:
            raise NotImplementedError("embed_norm / embed_dropout_rate are built for compute_dtype=fp32")
        if config.embed_size % 4 != 0:
            raise NotImplementedError("embed_size must be a multiple of 4 (16-byte rows for the gather, "
                                      "segment-reduce and float4 elementwise kernels)")
        if config.embed_size > MAX_EMBED_SIZE:
            raise NotImplementedError(f"embed_size {config.embed_size} > {MAX_EMBED_SIZE}: the segment reduction of "
                                      f"the gradient rows is built for rows of at most {MAX_EMBED_SIZE} floats")
        self.embedding = TableWeight(config.input_size, config.embed_size)
        std = math.sqrt(2.0 / float(config.num_fields + config.embed_size))
        with torch.no_grad():
            self.embedding.weight.normal_(0.0, std)
        if self.embed_norm:
            if config.embed_size > 64:
                raise NotImplementedError("embed_norm is built for embed_size <= 64")
            self.layer_norm = HipLayerNorm(config.embed_size, getattr(config, "layer_norm_eps", 1e-12))
        self.dropout = HipDropout(p_drop)
        self.table = RowTable("embed.embedding", self.embedding.weight)
        self.validate_ids = False
        self.defer_plan = False     # the owning model calls table.start_plan() at its chosen fork point
        # bf16 compute mode (mapx extension, BASELINE configs[2]): the gathered rows leave the kernel as
        # bf16 and every dense layer behind them runs on the bf16 MFMA; the table itself, its gradient
        # rows, every weight gradient and the optimizer state stay fp32
        self.compute_dtype = compute_dtype_of(config)
        if self.compute_dtype == torch.bfloat16 and config.embed_size % 8 != 0:
            raise NotImplementedError("compute_dtype=bf16 needs embed_size % 8 == 0 (16-byte bf16 rows)")

    def forward(self, input_ids):
        w = self.embedding.weight
        need_grad = torch.is_grad_enabled() and w.requires_grad
        keys = ops.ids_to_i32(input_ids, w.shape[0], validate=self.validate_ids) \
            if (need_grad or self.table.lazy is not None) else None
        # a training step reads the rows through their pending updates inside the gather (no catch-up launch at the head
        # of the step; the gradient update writes each row once); eval / no optimizer: the catch-up pass or nothing
        lazy = self.table.lazy
        fold = (EMB_LAZY_FOLD and need_grad and lazy is not None and lazy.m1 is None
                and w.shape[1] % (8 if self.compute_dtype == torch.bfloat16 else 4) == 0 and w.is_cuda)
        if keys is not None:
            self.table.prepare(keys, need_grad, defer_plan=self.defer_plan, through_replay=fold)
        x = _Gather.apply(w, input_ids, self.table, self.compute_dtype, lazy.lazy_rows() if fold else None)
        if self.embed_norm:
            x = self.layer_norm(x)
        return self.dropout(x)

    def forward_with_linear(self, input_ids, lin_weight):
        """-> (embeddings [B,F,E], sum_f lin_weight[id] [B]).  `lin_weight` [V,1] must be the
        table's secondary parameter (RowTable p1): both are read with the same ids, kept current
        by the same lazy optimizer state and get their gradients from one segment reduction."""
        if self.table.p1 is not lin_weight:
            raise ValueError("lin_weight must be the secondary parameter of this embedding's RowTable")
        w = self.embedding.weight
        need_grad = torch.is_grad_enabled() and w.requires_grad
        keys = ops.ids_to_i32(input_ids, w.shape[0], validate=self.validate_ids) \
            if (need_grad or self.table.lazy is not None) else None
        if keys is not None:
            self.table.prepare(keys, need_grad, defer_plan=self.defer_plan)
        x, lr = _GatherLinear.apply(w, lin_weight, input_ids, self.table, self.compute_dtype)
        if self.embed_norm:
            x = self.layer_norm(x)
        return self.dropout(x), lr


# ----------------------------------------------------------------------------- dense layers
def _grad_slot(p):
    """MapxOptimizer gives every dense parameter a slice of its flat gradient buffer
    (`p._mapx_grad`).  When present, backward kernels write the gradient straight into it
    (overwrite, one backward per step) and return None to autograd: no per-parameter
    accumulate kernel, no flat-buffer copy.  The final slab / partial sums of those gradients
    are deferred (ops.defer_sum) and done by one launch in MapxOptimizer.step()."""
    return getattr(p, "_mapx_grad", None)


def _weight_grads(ctx, dz, x, sw, sb, need=None):
    """dW = dz^T x and db = colsum(dz), written into the optimizer-owned slots when present.
    (Measured: moving these onto a side stream next to the dX chain made the step 5 % SLOWER —
    both are full-GPU GEMMs and only steal each other's CUs — so they stay on the main stream.)"""
    need_w, need_b = need if need is not None else (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
    dw = ops.linear_bwd_weight(dz, x, out=sw, defer=True) if need_w else None
    db = ops.colsum(dz, out=sb, defer=True) if need_b else None
    return (None if sw is not None else dw), (None if sb is not None else db)


class _ReluLink:
    """Between a ReLU layer and the ONE Linear that consumes its output (MLPBlock's chain): the consumer's
    input-gradient GEMM can apply the producer's ReLU mask (its saved input IS the producer's output) and
    form the producer's bias gradient in its epilogue; it then sets `premasked` and the producer's backward
    finds dZ instead of dY — one elementwise + column-sum launch less per layer on the backward chain."""

    def __init__(self):
        self.premasked, self.sb = False, None


class _X0Link:
    """Between DCNv2's cross tower and the embedding gather, both of which autograd would join through an
    elementwise add of the two towers' dL/dX0 in front of the gather's backward — a launch that also makes the
    main stream wait for EVERYTHING the cross tower's stream holds when its node returns.  The cross tower's
    node leaves its dL/dX0 here with an event recorded behind its last GEMM and returns None; the gather's
    backward adds the two tensors inside the segment reduction (ops.seg_reduce_rows(src2=))."""

    def __init__(self, consumer_stream):
        self.g = self.event = self.stream = None
        self.consumer_stream = consumer_stream


class _JoinLink:
    """Between the two towers of DCNv2 and the ONE layer that consumes their concatenated output (the heads'
    first Linear, or the grouped feat_encoder).  That layer's input gradient is formed as TWO products, one per
    tower, each on its tower's stream and each doing the tower's first backward step in its epilogue:
      deep tower (columns D.. of the weight, main stream): dZ = ReLU mask of the last MLP layer applied, its bias
        gradient's partial rows queued (EPI_RELU_MASK_COLSUM) — 4096 x 1000 outputs are exactly one round of
        128 x 128 tiles, where the joint 4096 x 1368 product ran 1.4 rounds;
      cross tower (columns ..D, tower stream): g, t = g X0, dX0 = g u and the bias gradient's partial rows
        (ops.gemm_bwd_fused).
    Both backward chains start from their own GEMM instead of waiting for one joint GEMM plus three elementwise
    launches.  The towers fill in what the consumer needs in forward (x0, u, bias-gradient slots); the consumer
    leaves g / dz / t / dx0 here and returns a placeholder as dL/d(final); _JoinColumns.backward hands the two
    tensors to the towers (as _ReluLink does for the mask inside the MLP)."""

    def __init__(self, D):
        self.D = D
        self.relu = _ReluLink()              # the deep tower's last layer
        self.x0 = self.u = self.sb_cross = None
        self.plus_v = False                  # a single cross layer: X_i IS X0, g joins dX0 at once
        self.t = self.dx0 = self.g = self.dz = None

    def usable(self, dz, final):
        return (ops.JOIN_FUSE and dz.dtype == torch.float32 and final.dtype == torch.float32
                and self.relu.sb is not None and self.sb_cross is not None and self.x0 is not None
                and self.D % 4 == 0 and final.shape[1] % 4 == 0 and final.shape[1] > self.D
                and ops.row_sliceable(final) and self.x0.is_contiguous() and self.u.is_contiguous())


def join_bwd_input(dz, w, final, link):
    """dL/d(final) = dz W as one product per tower (see _JoinLink) -> a placeholder of dL/d(final)'s shape."""
    D, Nn = link.D, final.shape[1]
    if dz.is_cuda and dz.stride(1) == 1 and ops._skinny(dz.shape[1], Nn, w) and ops._rows16(link.x0) and ops._rows16(link.u) \
            and (Nn - D) % 4 == 0:
        # a narrow head (finetune: one output): v = dz w is a handful of FMAs per element — one streaming launch does
        # both towers' products and epilogues (two MFMA GEMMs of inner dimension 1 before: 14 + 17 us -> 9)
        g, t, dx0, dzr, pc, pd = ops.skinny_join_bwd(dz, w, final, D, link.x0, link.u, link.plus_v)
        ops.defer_part_rows(link.sb_cross, pc, 0, D)
        ops.defer_part_rows(link.relu.sb, pd, 0, Nn - D)
        link.relu.premasked = True
        link.t, link.dx0, link.g, link.dz = t, dx0, g, dzr
        return torch.empty(1, 1, dtype=final.dtype, device=final.device).expand(final.shape[0], Nn)    # never read
    main = torch.cuda.current_stream() if dz.is_cuda else None
    side = ops.aux_stream("tower", dz.device) if dz.is_cuda else None
    # (the graph runtime keeps a node's FIRST-captured successor on the node's hardware queue and sends later ones
    # to the other queue, behind whatever that one holds — at this point of the step the segment plans' sort
    # chain: the deep tower's product, the longer backward chain's first link, is enqueued first)
    ops.dbg_sleep("join_deep")
    dzr = ops.linear_bwd_input(dz, ops.cols(w, D, None), relu_of=final[:, D:], colsum_to=link.relu.sb)
    with ops.Fork(side, main) as fork:
        ops.dbg_sleep("join_cross")
        g, t, dx0, part = ops.gemm_bwd_fused(dz, ops.cols(w, 0, D), D, x0=link.x0, u=link.u, plus_v=link.plus_v)
        ops.defer_part_rows(link.sb_cross, part, 0, D)
    fork.reads(dz)
    fork.leave_open()
    link.relu.premasked = True
    link.t, link.dx0, link.g, link.dz = t, dx0, g, dzr
    return torch.empty(1, 1, dtype=final.dtype, device=final.device).expand(final.shape[0], Nn)    # never read


class _Linear(Function):
    @staticmethod
    def forward(ctx, x, w, b, relu, out=None, out_f32=False, link_in=None, link_out=None):
        x = x.contiguous()
        half = ops.is_bf16(x)
        ctx.kpad, ctx.sw_real = 0, None
        wop = None
        if x.is_cuda and x.shape[1] % 8 != 0 and x.shape[0] >= 256 and w.shape[0] > 32 and link_in is None:
            # An input width that is not a multiple of 8 floats (DeepFM's heads read cat([dnn, lr + fm]): 1001 columns)
            # leaves the GEMMs their scalar operand path — 172 / 161 / 123 us for the forward / dW / dX of a
            # 4096 x 736 x 1001 layer against ~40 each.  Both operands are padded with zero columns to the next multiple
            # of 8 instead (two pad launches, one copy of dW back into its slot).  The same in bf16 mode (the bf16
            # GEMM's 16-byte chunks hold 8 elements): x and the weight's shadow are padded.
            ctx.kpad, ctx.sw_real = (-x.shape[1]) % 8, _grad_slot(w)
            x = torch.nn.functional.pad(x, (0, ctx.kpad))
            wop = torch.nn.functional.pad(ops.bf16_weight(w) if half else w.detach(), (0, ctx.kpad))
        if half and relu and out_f32:
            raise NotImplementedError("a ReLU layer with an fp32 result inside the bf16 trunk")
        if wop is None:
            wop = ops.bf16_weight(w) if half else w       # bf16 mode: the optimizer's bf16 shadow of w
        y = ops.linear_fwd(x, wop, b, relu=relu, out=out, out_dtype=torch.float32 if (half and out_f32) else None)
        ctx.relu, ctx.half = relu, half
        ctx.slots = (_grad_slot(w) if not ctx.kpad else None, _grad_slot(b))
        ctx.link_in, ctx.link_out = link_in, (link_out if relu else None)
        if ctx.link_out is not None:
            ctx.link_out.sb = ctx.slots[1]
        ctx.amax = ops.amax_pack(x, wop)
        ctx.save_for_backward(x, wop, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        ops.amax_unpack((x, w), ctx.amax)
        sw, sb = ctx.slots
        if ctx.half and gy.dtype == torch.float32:
            gy = ops.cast_bf16(gy)                 # the fp32 gradient of a head's logits enters the bf16 trunk
        if ctx.relu and ctx.link_out is not None and ctx.link_out.premasked:
            # the consumer's dX GEMM has applied this layer's mask and queued its bias gradient (_ReluLink)
            dz, db = (gy if ops.row_sliceable(gy) else gy.contiguous()), None
            dw = ops.linear_bwd_weight(dz, x, out=sw, defer=True) if ctx.needs_input_grad[1] else None
            dw = None if sw is not None else dw
        elif ctx.relu and (ctx.half or gy.shape[1] % 4 == 0):      # ReLU mask and bias gradient in one pass over dY
            dz, db = ops.relu_mask_colsum(gy, y, db=sb, defer=True)      # gy may be a slice of d(concat)
            if (isinstance(ctx.link_in, _JoinLink) and ops.step_window[0] and sw is not None
                    and ctx.needs_input_grad[1]):
                # The heads' first layer (RFD's 1368 -> 736 predictor): both towers' backward passes wait for this
                # node's dX, only the optimizer for its dW (83 us alone on the stream while the other queue idled) —
                # it goes to the end of the cross tower's chain, like the MFP encoder's (ops.run_late_tasks).
                def head_dw(dz=dz, x=x, sw=sw):
                    cur = torch.cuda.current_stream()
                    dz.record_stream(cur)
                    x.record_stream(cur)
                    ops.linear_bwd_weight(dz, x, out=sw, defer=True)
                ops.add_late_task(head_dw)
                dw = None
            else:
                dw = ops.linear_bwd_weight(dz, x, out=sw, defer=True) if ctx.needs_input_grad[1] else None
            dw, db = (None if sw is not None else dw), (None if sb is not None else db)
        else:
            dz = ops.relu_mask(gy.contiguous(), y.contiguous()) if ctx.relu else gy.contiguous()
            dw, db = _weight_grads(ctx, dz, x, sw, sb)
        dx = None
        if ctx.needs_input_grad[0]:
            link = ctx.link_in
            if isinstance(link, _JoinLink):
                dx = join_bwd_input(dz, w, x, link) if link.usable(dz, x) else ops.linear_bwd_input(dz, w)
            elif link is not None and link.sb is not None and ops.fused_mask_colsum_ok(dz, x):
                dx = ops.linear_bwd_input(dz, w, relu_of=x, colsum_to=link.sb)     # x = the producer's ReLU output
                link.premasked = True
            else:
                dx = ops.linear_bwd_input(dz, w)
        if ctx.kpad:                              # operands padded to a multiple of 8 columns in forward: cut them off
            K = w.shape[1] - ctx.kpad
            if dx is not None:
                dx = dx[:, :K]
            if dw is not None:
                if ctx.sw_real is not None:
                    ctx.sw_real.copy_(dw[:, :K])
                    dw = None
                else:
                    dw = dw[:, :K].contiguous()
        return dx, dw, db, None, None, None, None, None


class HipLinear(nn.Module):
    """nn.Linear (y = x W^T + b, optional fused ReLU) on the MFMA GEMM (fp32, or bf16 operands when
    the input is bf16); parameters keep nn.Linear's names, shapes and default initialisation.
    `out_fp32`: in bf16 mode the result stays fp32 (the heads' logits / encoder output)."""

    def __init__(self, in_features, out_features, relu=False, out_fp32=False):
        super().__init__()
        self.in_features, self.out_features, self.relu = in_features, out_features, relu
        self.out_fp32 = out_fp32
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        bound = 1.0 / math.sqrt(in_features)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.uniform_(-bound, bound)

    def forward(self, x, out=None, link_in=None, link_out=None):
        """`out`: optional pre-allocated destination (ops.alias_cols of a wider buffer).  link_in / link_out:
        _ReluLink objects of a chain in which this layer's input / output has exactly one consumer."""
        return _Linear.apply(x, self.weight, self.bias, self.relu, out, self.out_fp32, link_in, link_out)


class _Act(Function):
    """One of the reference's activations other than relu (layers.py:55-80) behind a plain Linear: y = f(z), the
    pre-activation z saved for dz = dy f'(z)."""

    @staticmethod
    def forward(ctx, z, kind, out):
        z = z.contiguous()
        ctx.kind = kind
        ctx.save_for_backward(z)
        return ops.act_fwd(kind, z, out=out)

    @staticmethod
    def backward(ctx, dy):
        (z,) = ctx.saved_tensors
        return ops.act_bwd(ctx.kind, dy, z), None, None


class MLPBlock(nn.Module):
    """[Linear, act, Dropout(p)] x n; state_dict keys dnn.{0,3,6,...} like the reference's nn.Sequential
    (layers.py:173-188).  relu (every DCNv2 script) is fused into the GEMM epilogues; the other values of
    `hidden_act` (layers.py:55-80: tanh, sigmoid, none, elu, leu, gelu, gelu_new, swish, mish) run as one
    elementwise pass behind the Linear GEMM, fp32 only."""

    def __init__(self, input_dim, hidden_size=128, num_hidden_layers=3, hidden_act="relu",
                 hidden_dropout_rate=0.5, batch_norm=False):
        super().__init__()
        self.act = str(hidden_act).lower()
        if self.act != "relu" and self.act not in ops.ACT_KINDS:
            raise NotImplementedError(f"hidden_act={hidden_act!r}")                 # layers.py:79: get_act raises too
        self.dnn = nn.ModuleDict()
        self.p_drop = float(hidden_dropout_rate or 0.0)
        for i in range(num_hidden_layers):
            self.dnn[str(3 * i)] = HipLinear(input_dim, hidden_size, relu=self.act == "relu")
            if self.p_drop > 0:                      # the reference's slot 3i+2 (no parameters, no state_dict key)
                self.dnn[str(3 * i + 2)] = HipDropout(self.p_drop)
            input_dim = hidden_size

    def forward(self, x, out=None, link_last=None):
        """`link_last`: the _ReluLink of the block's last layer when its output has exactly one consumer that
        can apply its ReLU mask (DCNv2: _JoinLink.relu)."""
        layers = [m for m in self.dnn.values() if isinstance(m, HipLinear)]
        drops = [m for m in self.dnn.values() if isinstance(m, HipDropout)]
        link = None
        if self.act != "relu":
            if x.dtype != torch.float32:
                raise NotImplementedError(f"hidden_act={self.act!r} is built for compute_dtype=fp32")
            for i, layer in enumerate(layers):
                last = i == len(layers) - 1
                to = out if (last and not drops) else None
                x = _Act.apply(layer(x), self.act, to)
                if drops:
                    x = drops[i](x, out=out if last else None)
            return x
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            if drops:
                if x.dtype != torch.float32:
                    raise NotImplementedError("hidden_dropout_rate > 0 is built for compute_dtype=fp32")
                x = drops[i](layer(x), out=out if last else None)
            else:
                # layer i's output feeds layer i+1 and nothing else: their backward passes are linked
                link_out = link_last if last else _ReluLink()
                x = layer(x, out=out if last else None, link_in=link, link_out=link_out)
                link = link_out
        return x


class _CrossTower(Function):
    """All cross layers in one autograd node: X_{i+1} = X_i + X_0 * (X_i W_i^T + b_i).
    One node instead of one per layer lets backward keep a single running dL/dX0 inside the
    kernels (cross_bwd_pre accumulates g*u_i, layer 0 also adds its g, the last dX GEMM adds the
    total in its epilogue) — autograd would otherwise add the four contributions with four
    elementwise launches at the very end of the step."""

    @staticmethod
    def forward(ctx, x0, out, link, x0_link, *wb):
        x0 = x0.contiguous()
        n = len(wb) // 2
        wops = [ops.bf16_weight(w) for w in wb[0::2]] if ops.is_bf16(x0) else list(wb[0::2])
        xi, xs, us = x0, [], []
        for i in range(n):
            xs.append(xi)
            xi, u = ops.cross_layer_fwd(x0, xi, wops[i], wb[2 * i + 1], out=out if i == n - 1 else None)
            us.append(u)
        ctx.n = n
        ctx.slots = [(_grad_slot(wb[2 * i]), _grad_slot(wb[2 * i + 1])) for i in range(n)]
        ctx.link, ctx.x0_link = link, x0_link
        ctx.amax = ops.amax_pack(x0, *xs[1:], *us, *wops)        # (records of the saved tensors, in their order)
        if link is not None:                 # what the consumer of the towers' output needs (see _JoinLink)
            link.x0, link.u, link.sb_cross, link.plus_v = x0, us[-1], ctx.slots[n - 1][1], n == 1
        ctx.save_for_backward(x0, *xs[1:], *us, *wops)
        return xi

    @staticmethod
    def backward(ctx, g):
        n = ctx.n
        saved = ctx.saved_tensors
        ops.amax_unpack(saved, ctx.amax)
        x0 = saved[0]
        xs = (x0,) + tuple(saved[1:n])
        us = saved[n:2 * n]
        ws = saved[2 * n:3 * n]
        if not ops.row_sliceable(g):
            g = g.contiguous()                   # else read in place: a slice of d(concat) costs no copy
        ops.dbg_sleep("cross_bwd")
        grads = [None] * (2 * n)
        D = x0.shape[1]
        t = dx0 = None
        link = ctx.link
        if link is not None and link.t is not None:
            # the producer of g (the heads' first layer) has done the last layer's elementwise backward in its
            # GEMM's epilogue and queued the bias gradient (_JoinLink)
            t, dx0, link.t, link.dx0 = link.t, link.dx0, None, None
            if t.is_cuda:
                cur = torch.cuda.current_stream()
                t.record_stream(cur)
                dx0.record_stream(cur)
        f32 = g.dtype == torch.float32 and x0.dtype == torch.float32
        have_slots = all(sw is not None and sb is not None for sw, sb in ctx.slots)
        # fused epilogues / one launch for all weight gradients: fp32, optimizer-owned gradient slots, 16-byte rows
        ok = f32 and have_slots and D % 4 == 0 and n <= 4
        fuse, batch_dw = ops.CROSS_FUSE and ok, ops.DW_BATCH and ok
        pend = []
        for i in range(n - 1, -1, -1):
            sw, sb = ctx.slots[i]
            first = i == 0
            if t is None:
                # width D = F * embed_size is a multiple of 4 (Embeddings enforces embed_size % 4 == 0)
                t, dx0, db = ops.cross_bwd_pre_colsum(g, x0, us[i], dx0=dx0, db=sb, defer=True, plus_g=first)
                if ctx.needs_input_grad[5 + 2 * i]:
                    grads[2 * i + 1] = None if sb is not None else db
            if batch_dw:
                pend.append((t, xs[i], sw))                                         # t^T X_i, all layers in one launch
            else:
                dw = ops.linear_bwd_weight(t, xs[i], out=sw, defer=True)            # t^T X_i
                if ctx.needs_input_grad[4 + 2 * i]:
                    grads[2 * i] = None if sw is not None else dw
            # dL/dX_i = g + t W_i; for layer 0 that is part of dL/dX0 and g is already inside dx0
            if first:
                g = ops.linear_bwd_input(t, ws[i], add=dx0)
                t = None
            elif fuse:
                # ... and the NEXT layer's t = dX_i X0, dX0 += dX_i u_{i-1} (+ dX_i), bias-gradient partials
                g, t, dx0, part = ops.gemm_bwd_fused(t, ws[i], D, add=g, x0=x0, u=us[i - 1], dx0=dx0, plus_v=i == 1)
                ops.defer_part_rows(ctx.slots[i - 1][1], part, 0, D)
            else:
                g = ops.linear_bwd_input(t, ws[i], add=g)
                t = None
        xl = ctx.x0_link
        if xl is not None and g.is_cuda and g.is_contiguous():
            # dL/dX0 goes to the gather's backward through the link, with an event HERE: the gather waits for the
            # dX chain above, not for the weight gradients and late tasks below
            cur = torch.cuda.current_stream()
            ops.dbg_sleep("x0_event")
            xl.g, xl.event, xl.stream = g, ops.record_event(), cur
            if cur.cuda_stream != xl.consumer_stream.cuda_stream:
                ops.pending_joins.append((xl.consumer_stream, cur))
            g = None
        if pend:
            ops.linear_bwd_weight_batched([p[0] for p in pend], [p[1] for p in pend], [p[2] for p in pend])
        ops.run_late_tasks()                     # what only the optimizer waits for (the encoder's dW / db)
        return (g, None, None, None, *grads)


class CrossNetV2(nn.Module):
    """X_{i+1} = X_i + X_0 * (W_i X_i + b_i) with full-rank W_i (reference layers.py:191-201);
    the Hadamard/residual epilogue is fused into the MFMA GEMM."""

    def __init__(self, input_dim, num_cross_layers):
        super().__init__()
        self.num_layers = num_cross_layers
        self.cross_layers = nn.ModuleList(HipLinear(input_dim, input_dim) for _ in range(num_cross_layers))

    def forward(self, x0, out=None, link=None, x0_link=None):
        """`out`: optional pre-allocated destination of the last layer (ops.alias_cols); `link`: the _JoinLink to
        the consumer of the towers' concatenated output; `x0_link`: the _X0Link to the embedding gather."""
        if self.num_layers == 0:
            return x0
        wb = [p for layer in self.cross_layers for p in (layer.weight, layer.bias)]
        return _CrossTower.apply(x0, out, link, x0_link, *wb)


class _SelfAttention(Function):
    """One AutoInt-style MultiHeadSelfAttention (reference layers.py:848-914, align_to="output"):
    out = relu(softmax(Q K^T [/ sqrt(A)]) V [+ residual]), Q/K/V/residual = bias-free projections
    of x [B,F,Din]; heads are the reference's .view(B*H, -1, A) chunks.  Projections and all
    weight / input gradients are MFMA GEMMs, the F x F core is csrc/attn.hip.  `drops`: None, or the layer's two
    dropout sites (on the probabilities, on the heads' output: layers.py:740-742, 901-904), whose masks the core's
    dropout forms draw themselves; the output they return is already dropped, so the residual branches do not change.
    bf16 x (bf16 compute mode): the projections are bf16 GEMMs on the weights' bf16 shadows; q, k, v, o,
    the output and dq, dk, dv, dpre, dx are bf16; the probabilities P and every weight gradient stay fp32."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, wres, heads, attn_size, res_conn, scaled, drops=None):
        B, F, Din = x.shape
        HA = heads * attn_size
        x2 = x.contiguous().view(B * F, Din)
        M = B * F
        ctx.slots = [_grad_slot(w) if w is not None else None for w in (wq, wk, wv, wres)]
        if ops.is_bf16(x2):            # the optimizer's bf16 shadows are the GEMM operands (saved for backward too)
            wq, wk, wv = ops.bf16_weight(wq), ops.bf16_weight(wk), ops.bf16_weight(wv)
            wres = ops.bf16_weight(wres) if wres is not None else None
        q = ops.gemm(x2, wq, True, True, M, HA, Din)
        k = ops.gemm(x2, wk, True, True, M, HA, Din)
        v = ops.gemm(x2, wv, True, True, M, HA, Din)
        drop = None
        if drops is not None:
            (rate, seed, off_p, dev), (_, seed_o, off_o, dev_o) = drops[0].philox(), drops[1].philox()
            if rate > 0:
                assert seed == seed_o and dev is dev_o, "the two dropout sites of a layer belong to one Trainer"
                drop = (rate, seed, off_p, off_o, dev)
        if drop is None:
            o, p = ops.attn_fwd(q, k, v, B * heads, F, attn_size, scaled)
        else:
            o, p = ops.attn_drop_fwd(q, k, v, B * heads, F, attn_size, scaled, *drop)
        if res_conn:
            pre = ops.gemm(x2, wres, True, True, M, HA, Din, epi=ops.N.EPI_ADD, aux1=o) if wres is not None \
                else o + x2
        else:
            pre = o
        out = torch.relu(pre)
        ctx.cfg = (B, F, Din, heads, attn_size, res_conn, scaled)
        ctx.drop = drop
        ctx.save_for_backward(x2, wq, wk, wv, wres, q, k, v, p, out)
        return out.view(B, F, HA)

    @staticmethod
    def backward(ctx, g):
        x2, wq, wk, wv, wres, q, k, v, p, out = ctx.saved_tensors
        B, F, Din, heads, A, res_conn, scaled = ctx.cfg
        HA = heads * A
        if ops.is_bf16(out) and g.dtype == torch.float32:
            g = ops.cast_bf16(g)                   # an fp32 gradient enters the bf16 trunk
        dpre = ops.relu_mask(g.contiguous().view(B * F, HA), out)
        if ctx.drop is None:
            dq, dk, dv = ops.attn_bwd(q, k, v, p, dpre, B * heads, F, A, scaled)
        else:
            dq, dk, dv = ops.attn_drop_bwd(q, k, v, p, dpre, B * heads, F, A, scaled, *ctx.drop)
        sq, sk, sv, sr = ctx.slots
        grads = []
        for d, slot in ((dq, sq), (dk, sk), (dv, sv)):
            dw = ops.linear_bwd_weight(d, x2, out=slot)
            grads.append(None if slot is not None else dw)
        dx = ops.linear_bwd_input(dq, wq)
        dx = ops.linear_bwd_input(dk, wk, add=dx)
        dx = ops.linear_bwd_input(dv, wv, add=dx)
        gres = None
        if res_conn:
            if wres is not None:
                dwr = ops.linear_bwd_weight(dpre, x2, out=sr)
                gres = None if sr is not None else dwr
                dx = ops.linear_bwd_input(dpre, wres, add=dx)
            else:
                dx = dx + dpre
        return dx.view(B, F, Din), grads[0], grads[1], grads[2], gres, None, None, None, None, None


class _ProjWeight(nn.Module):
    """`weight` [out, in] of a bias-free nn.Linear (same default initialisation)."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))


class MultiHeadSelfAttention(nn.Module):
    """Reference layers.py:848-914 restricted to what AutoInt builds (models.py:451-460):
    layer_norm off, align_to="output".  dropout_rate > 0 creates, as the reference does only then, its two dropouts
    (`dot_product_attention.dropout` on the probabilities, `dropout` on the heads' output before the residual add):
    MhaDropout sites without parameters, applied inside the attention kernels."""

    def __init__(self, input_dim, attention_dim, num_heads, dropout_rate=0.0, use_residual=True, use_scale=False):
        super().__init__()
        self.attention_dim, self.num_heads = attention_dim, num_heads
        self.output_dim = num_heads * attention_dim
        self.use_residual, self.use_scale = use_residual, use_scale
        self.W_q = _ProjWeight(input_dim, self.output_dim)
        self.W_k = _ProjWeight(input_dim, self.output_dim)
        self.W_v = _ProjWeight(input_dim, self.output_dim)
        self.W_res = _ProjWeight(input_dim, self.output_dim) if input_dim != self.output_dim else None
        if dropout_rate > 0:            # (a rate-0 model creates no site: the other dropouts keep their site numbers)
            self.dot_product_attention = nn.Module()
            self.dot_product_attention.dropout = MhaDropout(dropout_rate)
            self.dropout = MhaDropout(dropout_rate)
        else:
            self.dropout = None

    def forward(self, x):
        drops = (self.dot_product_attention.dropout, self.dropout) if self.dropout is not None else None
        return _SelfAttention.apply(x, self.W_q.weight, self.W_k.weight, self.W_v.weight,
                                    self.W_res.weight if self.W_res is not None else None, self.num_heads,
                                    self.attention_dim, self.use_residual, self.use_scale, drops)


class _CinStack(Function):
    """All CIN layers as one autograd node (reference layers.py:708-721).  Activations are kept
    embedding-major (rows r = (b, d)), so a layer is: outer product of two short row vectors ->
    Hadamard matrix [B*E, F*H_i] -> one MFMA GEMM with the 1x1 convolution's weight (+ bias) ->
    the next layer's input as it is; every layer's output is sum-pooled over the E rows of a sample
    into its columns of `out` [B, sum(units)].  Backward walks the layers in reverse: pooled
    gradient broadcast (+ the gradient from the layer above), dW / db / dHad GEMMs, outer-product
    backward accumulating into dX0."""

    @staticmethod
    def _forward_bf16(ctx, x3, ws, bs):
        """bf16 x3 (bf16 compute mode): the fused kernels of csrc/cin_fused.hip, which form the Hadamard
        operand inside the MFMA loop.  x0t, every layer's Y and the pooled vector are bf16 (one rounding per store); the
        weights' bf16 shadows are the operands.  Saved for backward: x0t and every layer's bf16 input, nothing of
        extent R x F*H."""
        B, F, E = x3.shape
        x0t = ops.cin_transpose_bf16(x3)
        units = [w.shape[0] for w in ws]
        out = torch.empty(B, sum(units), dtype=torch.bfloat16, device=x3.device)
        wops = [ops.bf16_weight(w) for w in ws]
        xi, h_in, xs, col = x0t, F, [], 0
        for w, b, u in zip(wops, bs, units):
            xs.append(xi)
            xi = ops.cin_fused_fwd(x0t, F, xi, h_in, w, b)
            ops.cin_pool_fwd_bf16(xi, u, B, E, out[:, col:col + u])
            h_in, col = u, col + u
        ctx.half, ctx.shape, ctx.units = True, (B, F, E), units
        ctx.slots = [(_grad_slot(w), _grad_slot(b)) for w, b in zip(ws, bs)]
        ctx.save_for_backward(*xs, *wops)
        return out

    @staticmethod
    def _backward_bf16(ctx, g):
        """Layers in reverse: the top layer's dY is its pooled gradient alone; every dX kernel adds the pooled gradient
        of the layer below to its dxi and rounds the sum once; dx0t is one running fp32 sum."""
        B, F, E = ctx.shape
        units, n = ctx.units, len(ctx.units)
        xs, wops = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        x0t = xs[0]
        if g.dtype == torch.float32:
            g = ops.cast_bf16(g)                  # an fp32 gradient enters the bf16 trunk
        if g.stride(1) != 1:
            g = g.contiguous()                    # else read in place: a slice of d(concat) costs no copy
        grads = [None] * (2 * n)
        cols = [sum(units[:i]) for i in range(n)]
        dx0t = torch.empty(B * E, F, dtype=torch.float32, device=g.device)
        dy = ops.cin_pool_bwd_bf16(g[:, cols[-1]:cols[-1] + units[-1]], B, E)
        for i in range(n - 1, -1, -1):
            u, h_in = units[i], (units[i - 1] if i else F)
            sw, sb = ctx.slots[i]
            db = ops.colsum(dy[:, :u], out=sb)
            grads[2 * i + 1] = None if sb is not None else db
            dw = ops.cin_fused_bwd_weight(dy, u, x0t, F, xs[i], h_in, out=sw)
            grads[2 * i] = None if sw is not None else dw.view(u, F * h_in, 1)
            gpool = g[:, cols[i - 1]:cols[i - 1] + h_in] if i else None
            dy = ops.cin_fused_bwd_input(dy, u, wops[i], x0t, F, xs[i], h_in, dx0t, accumulate_x0=i != n - 1,
                                         first_layer=i == 0, gpool=gpool, E=E)
        return (ops.cin_dx3_bf16(dx0t, B, E, F),) + tuple(grads)

    @staticmethod
    def forward(ctx, x3, *wb):
        B, F, E = x3.shape
        ws, bs = wb[0::2], wb[1::2]
        if ops.is_bf16(x3):
            return _CinStack._forward_bf16(ctx, x3, ws, bs)
        ctx.half = False
        x0t = ops.transpose_batched(x3).view(B * E, F)
        units = [w.shape[0] for w in ws]
        out = torch.empty(B, sum(units), dtype=torch.float32, device=x3.device)
        xi, saved, col = x0t, [], 0
        pad = B * E >= 256
        wps = []
        for w, b in zip(ws, bs):
            # The Hadamard matrix has F * H_i columns (529, 1150 at Avazu's sizes) and the layer `units` = 50 outputs:
            # neither a multiple of 8 floats, which left all three GEMMs of a layer the scalar operand path (380 + 167 us
            # forward, 266 + 133 dX, 238 + 188 dW in a 2.9-ms step).  Its rows are padded with zero columns by the kernel
            # that writes them, the weight (50 x K floats) by a copy.
            had = ops.cin_outer_fwd(x0t, xi, pad_to=8 if pad else 1)
            w2 = w.detach().view(w.shape[0], -1)
            wp = torch.nn.functional.pad(w2, (0, had.shape[1] - w2.shape[1])) if had.shape[1] != w2.shape[1] else w2
            nxt = ops.linear_fwd(had, wp, b)
            ops.cin_pool_fwd(nxt, B, E, out[:, col:col + w.shape[0]])
            saved.append((xi, had))
            wps.append(wp)
            xi, col = nxt, col + w.shape[0]
        ctx.wps = wps
        ctx.saved, ctx.x0t, ctx.shape = saved, x0t, (B, F, E)
        ctx.ws = ws
        ctx.slots = [(_grad_slot(w), _grad_slot(b)) for w, b in zip(ws, bs)]
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.half:
            return _CinStack._backward_bf16(ctx, g)
        B, F, E = ctx.shape
        ws, x0t = ctx.ws, ctx.x0t
        dx0t = torch.empty_like(x0t)
        grads = [None] * (2 * len(ws))
        col = g.shape[1]
        dnext = None                          # gradient w.r.t. the layer's output from the layer above
        for i in range(len(ws) - 1, -1, -1):
            w = ws[i]
            u = w.shape[0]
            col -= u
            xi, had = ctx.saved[i]
            dy = dnext if dnext is not None else torch.empty(B * E, u, dtype=torch.float32, device=g.device)
            ops.cin_pool_bwd(g[:, col:col + u], B, E, dy, accumulate=dnext is not None)
            sw, sb = ctx.slots[i]
            wp = ctx.wps[i]
            Kc, Kp = w[0].numel(), wp.shape[1]
            db = ops.colsum(dy, out=sb)
            grads[2 * i + 1] = None if sb is not None else db
            if Kp != Kc or (u % 8 != 0 and dy.shape[0] >= 256):
                # dy's `units` columns padded to a multiple of 8 as well (a 15-MB copy): dW and dX both read it
                up = (u + 7) // 8 * 8
                dyp = torch.nn.functional.pad(dy, (0, up - u))
                wpp = torch.nn.functional.pad(wp, (0, 0, 0, up - u))
                dwp = ops.linear_bwd_weight(dyp, had)                       # [up, Kp]
                if sw is not None:
                    sw.view(u, -1).copy_(dwp[:u, :Kc])
                else:
                    grads[2 * i] = dwp[:u, :Kc].contiguous().view_as(w)
                dhad = ops.linear_bwd_input(dyp, wpp)                       # [R, Kp]
            else:
                dw = ops.linear_bwd_weight(dy, had, out=None if sw is None else sw.view(u, -1))
                grads[2 * i] = None if sw is not None else dw.view_as(w)
                dhad = ops.linear_bwd_input(dy, wp)
            dxi = ops.cin_outer_bwd(dhad, x0t, xi, dx0t, accumulate_x0=i != len(ws) - 1)
            if i == 0:                         # layer 1's X_i IS X_0
                dx0t += dxi
            dnext = dxi
        dx3 = ops.transpose_batched(dx0t.view(B, E, F))
        return (dx3,) + tuple(grads)


class CIN(nn.Module):
    """Reference layers.py:696-721; parameters keep nn.Conv1d's names and shapes
    (`cin_layer.layer_{i}.weight` [out, F*H_{i-1}, 1], `.bias` [out])."""

    def __init__(self, num_fields, cin_layer_units):
        super().__init__()
        self.cin_layer_units = list(cin_layer_units)
        self.cin_layer = nn.ModuleDict()
        h_in = num_fields
        for i, unit in enumerate(self.cin_layer_units):
            self.cin_layer["layer_" + str(i + 1)] = nn.Conv1d(num_fields * h_in, unit, kernel_size=1)
            h_in = unit

    def forward(self, x3):
        wb = []
        for i in range(len(self.cin_layer_units)):
            conv = self.cin_layer["layer_" + str(i + 1)]
            wb += [conv.weight, conv.bias]
        return _CinStack.apply(x3, *wb)


class _JoinColumns(Function):
    """torch.cat([a, b], dim=1) when a and b were already written into their column ranges of
    `buf` (ops.alias_cols): no copy forward, two slices backward."""

    @staticmethod
    def forward(ctx, a, b, buf, link=None):
        ctx.split, ctx.link = a.shape[1], link
        return buf

    @staticmethod
    def backward(ctx, g):
        ops.run_main_tasks()          # joins that the head's backward left for this point of the main stream
        link = ctx.link
        if link is not None and link.g is not None:
            # the consumer formed the two towers' gradients separately (_JoinLink); `g` is a placeholder
            gc, gd, link.g, link.dz = link.g, link.dz, None, None
            return gc, gd, None, None
        return g[:, :ctx.split], g[:, ctx.split:], None, None


class _Bce(Function):
    @staticmethod
    def forward(ctx, logits, labels):
        out3, dl = ops.bce_with_logits(logits, labels, want_grad=True)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(out3)
        ctx.set_materialize_grads(False)
        return out3[0], out3                   # (a view of the non-differentiable statistics: no copy launch)

    @staticmethod
    def backward(ctx, g, _):
        (dl,) = ctx.saved_tensors
        unit = ops.unit_gradient[0]
        if unit is not None and g.numel() == 1 and g.data_ptr() == unit.data_ptr():
            return dl, None            # the Trainer's loss.backward(ones): no elementwise launch on the head's chain
        return dl * g, None


def bce_with_logits(logits, labels):
    """-> (mean loss, stats = [loss, accuracy, mean(label)])  (BCEWithLogitsLoss, models.py:81,91)."""
    return _Bce.apply(logits, labels)


# ----------------------------------------------------------------------------- Transformer encoder
class MhaDropout(HipDropout):
    """A dropout applied inside an attention kernel: nn.MultiheadAttention's dropout of the attention probabilities
    (p = the layer's `dropout`), and AutoInt's two per attention layer.  A HipDropout site like the others (Trainer
    gives it its seed, site and step counter), whose mask the attention kernels draw themselves: ops.mha_fwd / mha_bwd
    and ops.attn_drop_fwd / attn_drop_bwd take (p, seed, offset, offset_dev) from `philox()`."""

    def philox(self):
        """-> (p, seed, offset, offset_dev) of this forward call; p = 0 in eval mode (no mask)."""
        if not self.training or self.p == 0.0:
            return 0.0, 0, 0, None
        base = (self.rank << 48) + ((16 + self.site) << 36)
        if self.step_counter is not None:
            return self.p, self.seed, base, self.step_counter
        self._calls += 1
        return self.p, self.seed, base + self._calls, None

    def forward(self, x, out=None):
        raise RuntimeError("MhaDropout is applied inside the attention kernels (_MhaCore, _SelfAttention)")


class _MhaCore(Function):
    """softmax(Q K^T / sqrt(dh)) -> dropout -> V per (sample, head), reading the packed in-projection output
    qkv [B*F, 3E] and returning O [B*F, E] heads concatenated (csrc/mha.hip).  Backward writes dQ / dK / dV into
    one packed [B*F, 3E] tensor: the in-projection's _Linear then forms its weight, bias and input gradients with
    one launch each."""

    @staticmethod
    def forward(ctx, qkv, B, F, E, H, drop):
        p, seed, offset, dev = drop.philox() if drop is not None else (0.0, 0, 0, None)
        o, probs = ops.mha_fwd(qkv, B, F, E, H, p, seed, offset, dev)
        ctx.cfg = (B, F, E, H, p, seed, offset, dev)
        ctx.save_for_backward(qkv, probs)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, probs = ctx.saved_tensors
        B, F, E, H, p, seed, offset, dev = ctx.cfg
        return ops.mha_bwd(qkv, probs, do, B, F, E, H, p, seed, offset, dev), None, None, None, None, None


class HipMultiheadAttention(nn.Module):
    """nn.MultiheadAttention(E, H, dropout, batch_first=True) as self-attention: parameters `in_proj_weight` [3E, E]
    (Xavier-uniform), `in_proj_bias` [3E] (zeros), `out_proj.{weight,bias}` (nn.Linear's init, bias zeroed), torch's
    names and initialisation.  forward() returns the heads' concatenated output BEFORE out_proj (the encoder layer
    applies out_proj)."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        if embed_dim % num_heads:
            raise ValueError(f"embed_dim {embed_dim} is not divisible by num_heads {num_heads}")
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = HipLinear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        with torch.no_grad():
            self.out_proj.bias.zero_()
        self.attn_drop = MhaDropout(dropout)

    def forward(self, x2, B, F):
        qkv = _Linear.apply(x2, self.in_proj_weight, self.in_proj_bias, False, None, False, None, None)
        return _MhaCore.apply(qkv, B, F, self.embed_dim, self.num_heads, self.attn_drop)


class TransformerEncoderLayer(nn.Module):
    """nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation in {relu, gelu},
    layer_norm_eps, batch_first=True, norm_first) with torch's parameter names:
      post-norm: x = norm1(x + dropout1(SA(x)));  x = norm2(x + dropout2(linear2(dropout(act(linear1(x))))))
      pre-norm:  x = x + dropout1(SA(norm1(x)));  x = x + dropout2(FF(norm2(x)))
    relu is fused into linear1's GEMM epilogue, gelu (erf form) is one elementwise pass behind it.
    bf16 input (compute_dtype=bf16): every tensor between the kernels is bf16; post-norm layers form both residual sums
    inside the add + LayerNorm kernels (_AddLayerNorm), pre-norm layers keep their elementwise adds."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.0, activation="relu", layer_norm_eps=1e-5,
                 norm_first=False):
        super().__init__()
        self.act = str(activation).lower()
        if self.act not in ("relu", "gelu"):
            raise ValueError(f"activation should be relu/gelu, not {activation}")
        self.self_attn = HipMultiheadAttention(d_model, nhead, dropout)
        self.linear1 = HipLinear(d_model, dim_feedforward, relu=self.act == "relu")
        self.dropout = HipDropout(dropout)
        self.linear2 = HipLinear(dim_feedforward, d_model)
        self.norm_first = bool(norm_first)
        self.norm1 = HipLayerNorm(d_model, layer_norm_eps)
        self.norm2 = HipLayerNorm(d_model, layer_norm_eps)
        self.dropout1 = HipDropout(dropout)
        self.dropout2 = HipDropout(dropout)

    def _sa(self, x2, B, F):
        return self.dropout1(self.self_attn.out_proj(self.self_attn(x2, B, F)))

    def _ff(self, x2):
        h = self.linear1(x2)
        if self.act == "gelu":
            h = _Act.apply(h, "gelu", None)
        return self.dropout2(self.linear2(self.dropout(h)))

    def forward(self, x3):
        B, F, E = x3.shape
        x = x3.reshape(B * F, E)
        # (the residual adds stay elementwise: the GEMM's EPI_ADD epilogue has no bias term, and every projection
        # here has one)
        if self.norm_first:
            x = x + self._sa(self.norm1(x), B, F)
            x = x + self._ff(self.norm2(x))
        elif ops.is_bf16(x):
            # bf16 compute mode: the residual add happens inside the LayerNorm kernels (the sum is never stored, so it
            # is not rounded; one backward output is the gradient of both addends)
            x = self.norm1(x, add=self._sa(x, B, F))
            x = self.norm2(x, add=self._ff(x))
        else:
            x = self.norm1(x + self._sa(x, B, F))
            x = self.norm2(x + self._ff(x))
        return x.view(B, F, E)


class TransformerEncoder(nn.Module):
    """nn.TransformerEncoder(layer, num_layers) without a final norm: `layers.{i}` are copies of ONE layer, so every
    layer starts with the same parameters (torch deep-copies too); each copy gets dropout sites of its own."""

    def __init__(self, encoder_layer, num_layers):
        super().__init__()
        layers = [encoder_layer] + [copy.deepcopy(encoder_layer) for _ in range(num_layers - 1)]
        for layer in layers[1:]:
            for m in layer.modules():
                if isinstance(m, HipDropout):
                    HipDropout._sites += 1
                    m.site = HipDropout._sites
        self.layers = nn.ModuleList(layers[:num_layers])
        self.num_layers = num_layers

    def forward(self, x3):
        for layer in self.layers:
            x3 = layer(x3)
        return x3


class _FieldPool(Function):
    """Reduction over the fields of the Transformer's finetune head: x3 [B,F,E] -> [B,E], "sum" / "mean", or "attn":
    weighted by softmax_f(scores [B,F]) (the softmax is inside the kernel; backward returns the gradient of the
    scores before it)."""

    @staticmethod
    def forward(ctx, x3, scores, mode):
        x3 = x3.contiguous()
        out, w = ops.field_pool_fwd(x3, mode, scores)
        ctx.mode = mode
        ctx.save_for_backward(x3, w)
        return out

    @staticmethod
    def backward(ctx, g):
        x3, w = ctx.saved_tensors
        dx, ds = ops.field_pool_bwd(g, x3, ctx.mode, w)
        return dx, ds, None


def field_pool(x3, mode, scores=None):
    return _FieldPool.apply(x3, scores, mode)


# ----------------------------------------------------------------------------- FGCNN
class _InnerProduct(Function):
    """InnerProductLayer(output='inner_product') (reference layers.py:132-135): x [B,T,E] -> x_i . x_j over the pairs
    i < j in masked_select's order, [B, T(T-1)/2]  (csrc/fgcnn.hip).  fp32 or bf16: the output and dx take x's
    element type; a bf16 gradient that is a column slice of d(dense_input) is read in place."""

    @staticmethod
    def forward(ctx, x3):
        x3 = x3.contiguous()
        ctx.save_for_backward(x3)
        return ops.inner_product_fwd(x3)

    @staticmethod
    def backward(ctx, g):
        (x3,) = ctx.saved_tensors
        return ops.inner_product_bwd(g, x3)


def inner_product(x3):
    return _InnerProduct.apply(x3)


class _ConvBnActPool(Function):
    """One FGCNN stage: Conv2d((kh,1)) -> BatchNorm2d -> act -> MaxPool2d((ps,1)) (reference layers.py:226-232) as
    three launches forward (conv + partial statistics, their finalise, normalise + act + pool) and four backward
    (csrc/fgcnn.hip).  Train mode normalises with the batch statistics and moves the running ones (and the batch
    counter) on the device; saved for backward: the input, z (the conv output) and one uint8 argmax per pooled
    element.  Eval mode normalises with the running statistics, saves nothing and has no backward.
    A bf16 input gives a bf16 z, output and dx; the parameters, the statistics, the buffers and every
    parameter gradient stay fp32."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, tracked, ps, act, training):
        x = x.contiguous()
        ctx.training = training
        if not training:
            z, _ = ops.fgcnn_conv_fwd(x, w, b, stats=False)
            y, _ = ops.fgcnn_pool_fwd(z, gamma, beta, ps, act, running_mean=running_mean, running_var=running_var,
                                      save=False)
            return y
        z, part = ops.fgcnn_conv_fwd(x, w, b)
        stats = ops.fgcnn_bn_stats(part, z.shape[2], z.shape[3], running_mean, running_var, tracked)
        y, idx = ops.fgcnn_pool_fwd(z, gamma, beta, ps, act, stats=stats)
        ctx.cfg = (ps, act)
        ctx.slots = tuple(_grad_slot(p) for p in (w, b, gamma, beta))
        ctx.save_for_backward(x, w, z, idx, stats, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise NotImplementedError("FGCNN in eval mode (BatchNorm on its running statistics) is forward only")
        x, w, z, idx, stats, gamma, beta = ctx.saved_tensors
        ps, act = ctx.cfg
        sw, sb, sg, sbe = ctx.slots
        dx, dw, db, dgamma, dbeta = ops.fgcnn_bwd(dy, idx, z, x, w, stats, gamma, beta, ps, act, dw=sw, db=sb,
                                                  dgamma=sg, dbeta=sbe, need_dx=ctx.needs_input_grad[0])
        return (dx, None if sw is not None else dw, None if sb is not None else db,
                None if sg is not None else dgamma, None if sbe is not None else dbeta, None, None, None, None, None,
                None)


class _ConvWeights(nn.Module):
    """`weight` [Cout, Cin, kh, 1] and `bias` [Cout] of an nn.Conv2d with a (kh, 1) kernel (its default
    initialisation)."""

    def __init__(self, in_channels, out_channels, kernel_height):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_height, 1))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_channels * kernel_height)
        with torch.no_grad():
            self.bias.uniform_(-bound, bound)


class _BatchNormState(nn.Module):
    """The parameters and buffers of an nn.BatchNorm2d (eps 1e-5, momentum 0.1, affine, tracked statistics)."""

    def __init__(self, channels):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class FGCNNBlock(nn.Module):
    """Reference layers.py:204-251: stage i is Conv2d(C_{i-1}, C_i, (kh_i, 1), padding ((kh_i-1)//2, 0)) ->
    BatchNorm2d -> act -> MaxPool2d((ps_i, 1), padding (H_{i-1} % ps_i, 0)) on [B, C_{i-1}, H_{i-1}, E], then
    Linear -> act from the flattened stage output to R_i * H_i new feature rows; the new rows of all stages are
    concatenated.  state_dict keys `conv_layers.{i}.0.*` (conv), `.1.*` (batch norm), `recombine_layers.{i}.0.*`."""
    ACTS = ("tanh", "relu")

    def __init__(self, num_fields, embedding_dim, channels, kernel_heights, pooling_sizes, recombined_channels,
                 activation="tanh"):
        super().__init__()
        self.act = str(activation).lower()
        if self.act not in self.ACTS:
            raise NotImplementedError(f"conv_act={activation!r}: the FGCNN kernels build {' | '.join(self.ACTS)}")
        self.embedding_dim = embedding_dim
        self.pooling_sizes = list(pooling_sizes)
        self.conv_layers, self.recombine_layers = nn.ModuleList(), nn.ModuleList()
        c_in, height = 1, num_fields
        for c_out, kh, ps, rc in zip(channels, kernel_heights, pooling_sizes, recombined_channels):
            if 2 * (height % ps) > ps:
                raise ValueError(f"pooling_sizes: a stage of height {height} pooled by {ps} pads {height % ps} rows, "
                                 "more than half of the pooling size (torch's MaxPool2d raises too)")
            self.conv_layers.append(nn.ModuleDict({"0": _ConvWeights(c_in, c_out, kh), "1": _BatchNormState(c_out)}))
            height = int(math.ceil(height / ps))
            self.recombine_layers.append(nn.ModuleDict({
                "0": HipLinear(height * embedding_dim * c_out, height * embedding_dim * rc, relu=self.act == "relu")}))
            c_in = c_out

    def forward(self, x):
        """x [B, 1, F, E] -> the new feature rows [B, sum_i R_i H_i, E]."""
        B, new = x.shape[0], []
        for stage, rec, ps in zip(self.conv_layers, self.recombine_layers, self.pooling_sizes):
            conv, bn = stage["0"], stage["1"]
            x = _ConvBnActPool.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                     bn.num_batches_tracked, ps, self.act, self.training)
            r = rec["0"](x.flatten(start_dim=1))
            if self.act != "relu":
                r = _Act.apply(r, self.act, None)
            new.append(r.reshape(B, -1, self.embedding_dim))
        return torch.cat(new, dim=1)


# ----------------------------------------------------------------------------- FiGNN
class _FiGNNTrunk(Function):
    """FiGNNBlock.forward (reference layers.py:333-365) as one autograd node over csrc/fignn.hip: the attention graph
    once, then one launch per layer (GraphLayer + the shared GRUCell + the optional residual).  Saved for backward: x,
    the graph g with its two projections s and d, and every layer's input h; the layer's intermediates are recomputed.
    Backward walks the layers in reverse (one recompute-and-backward launch, then the weight gradients from per-chunk
    partials added in a fixed order), accumulating dg and — res_conn — dx, and ends in the graph's backward.  The
    shared GRU's gradients, and with reuse_graph_layer the one GraphLayer's, are added up in that (layer) order."""

    @staticmethod
    def forward(ctx, x, w_attn, w_ih, w_hh, b_ih, b_hh, res_conn, reuse, num_layers, *layer_params):
        x = x.contiguous()
        g, s, d = ops.fignn_graph_fwd(x, w_attn)
        hs = [x]
        for l in range(num_layers):
            w_in, w_out, bias_p = layer_params[0:3] if reuse else layer_params[3 * l:3 * l + 3]
            hs.append(ops.fignn_layer_fwd(hs[-1], g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh,
                                          x_res=x if res_conn else None))
        ctx.cfg = (bool(res_conn), bool(reuse), int(num_layers))
        ctx.params = (w_attn, w_ih, w_hh, b_ih, b_hh) + tuple(layer_params)
        ctx.slots = tuple(_grad_slot(p) for p in ctx.params)
        ctx.save_for_backward(g, s, d, *hs[:-1])
        return hs[-1]

    @staticmethod
    def backward(ctx, dh):
        g, s, d, *hs = ctx.saved_tensors
        res_conn, reuse, L = ctx.cfg
        w_attn, w_ih, w_hh, b_ih, b_hh = ctx.params[:5]
        layer_params = ctx.params[5:]
        x = hs[0]
        B, F, E = x.shape
        # destinations: the optimizer's slots, else fresh tensors handed back to autograd
        dst = [sl if sl is not None else torch.empty_like(p) for sl, p in zip(ctx.slots, ctx.params)]
        dg = torch.empty_like(g)
        dx_acc = torch.empty_like(x) if res_conn else None
        ws = torch.empty(B, F, ops.FIGNN_WS_VECS, E, dtype=torch.float32, device=x.device)
        dh = dh.contiguous()
        for l in reversed(range(L)):
            first = l == L - 1
            k = 0 if reuse else 3 * l
            dh, _ = ops.fignn_layer_bwd(dh, hs[l], g, *layer_params[k:k + 3], w_ih, w_hh, b_ih, b_hh, dg, first,
                                        dx_acc=dx_acc, dx_init=first, grads=dst[5 + k:5 + k + 3] + dst[1:5],
                                        add_layer=reuse and not first, add_gru=not first, ws=ws)
        dx, _ = ops.fignn_graph_bwd(dg, g, s, d, x, w_attn, dh, dx_add=dx_acc, dw_attn=dst[0], inplace=True)
        grads = [None if sl is not None else t for sl, t in zip(ctx.slots, dst)]
        return (dx, *grads[:5], None, None, None, *grads[5:])


class GraphLayer(nn.Module):
    """Reference layers.py:300-313: per-field E x E matrices `W_in`, `W_out` [F,E,E] (xavier_normal_) and `bias_p` [E]
    (zeros).  Read by the FiGNN kernels only (`_mapx_row_resident`: the optimizer keeps no weight planes for them)."""

    def __init__(self, config):
        super().__init__()
        F, E = config.num_fields, config.embed_size
        self.W_in = nn.Parameter(torch.empty(F, E, E))
        self.W_out = nn.Parameter(torch.empty(F, E, E))
        nn.init.xavier_normal_(self.W_in)
        nn.init.xavier_normal_(self.W_out)
        self.bias_p = nn.Parameter(torch.zeros(E))


class _GRUCellWeights(nn.Module):
    """The parameters of an nn.GRUCell(E, E): `weight_ih`, `weight_hh` [3E,E], `bias_ih`, `bias_hh` [3E], gate order
    r, z, n, all U(-1/sqrt(E), 1/sqrt(E))."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.weight_ih = nn.Parameter(torch.empty(3 * hidden_size, input_size))
        self.weight_hh = nn.Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.bias_ih = nn.Parameter(torch.empty(3 * hidden_size))
        self.bias_hh = nn.Parameter(torch.empty(3 * hidden_size))
        bound = 1.0 / math.sqrt(hidden_size)
        with torch.no_grad():
            for p in self.parameters():
                p.uniform_(-bound, bound)


class FiGNNBlock(nn.Module):
    """Reference layers.py:316-365: `gnn` (one GraphLayer per layer, or ONE with reuse_graph_layer), `gru`
    (nn.GRUCell(E, E), shared by all layers) and `W_attn` (Linear(2E, 1, bias=False))."""

    def __init__(self, config):
        super().__init__()
        self.num_fields = config.num_fields
        self.embedding_dim = config.embed_size
        self.gnn_layers = int(config.num_hidden_layers)
        self.use_residual = bool(config.res_conn)
        self.reuse_graph_layer = bool(config.reuse_graph_layer)
        if self.reuse_graph_layer:
            self.gnn = GraphLayer(config)
        else:
            self.gnn = nn.ModuleList([GraphLayer(config) for _ in range(self.gnn_layers)])
        self.gru = _GRUCellWeights(config.embed_size, config.embed_size)
        self.W_attn = _ProjWeight(config.embed_size * 2, 1)
        for p in self.parameters():
            p._mapx_row_resident = True

    def forward(self, feat_embed):
        layers = [self.gnn] if self.reuse_graph_layer else list(self.gnn)
        flat = [p for gl in layers for p in (gl.W_in, gl.W_out, gl.bias_p)]
        return _FiGNNTrunk.apply(feat_embed, self.W_attn.weight, self.gru.weight_ih, self.gru.weight_hh,
                                 self.gru.bias_ih, self.gru.bias_hh, self.use_residual, self.reuse_graph_layer,
                                 self.gnn_layers, *flat)


class _BiasFreeLinear(Function):
    """y = x W^T on the existing GEMM / streaming kernels (the AutoInt projections' calls), dW into the optimizer's slot."""

    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        M, K = x.shape
        Nn = w.shape[0]
        ctx.slot = _grad_slot(w)
        ctx.save_for_backward(x, w)
        if ops._skinny(Nn, K, x, w):
            return ops.linear_fwd(x, w, None)
        return ops.gemm(x, w, True, True, M, Nn, K)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        dw = ops.linear_bwd_weight(gy, x, out=ctx.slot)
        dx = ops.linear_bwd_input(gy, w) if ctx.needs_input_grad[0] else None
        return dx, (None if ctx.slot is not None else dw)


class _AttnPredict(Function):
    """logits = sum_f sigmoid(z2) score (reference layers.py:375-379), csrc/fignn.hip."""

    @staticmethod
    def forward(ctx, score, z2):
        score, z2 = score.contiguous(), z2.contiguous()
        ctx.save_for_backward(score, z2)
        return ops.fignn_pred_fwd(score, z2)

    @staticmethod
    def backward(ctx, g):
        score, z2 = ctx.saved_tensors
        return ops.fignn_pred_bwd(g, score, z2)


class AttentionalPrediction(nn.Module):
    """Reference layers.py:368-379: `linear1` = Linear(E, 1, bias=False), `linear2` = Sequential(Linear(F E, F,
    bias=False), Sigmoid()) — keys `linear1.weight`, `linear2.0.weight`; the sigmoid is inside the combining kernel."""

    def __init__(self, config):
        super().__init__()
        self.linear1 = _ProjWeight(config.embed_size, 1)
        self.linear2 = nn.ModuleDict({"0": _ProjWeight(config.num_fields * config.embed_size, config.num_fields)})

    def forward(self, h):
        B, F, E = h.shape
        h = h.contiguous()
        score = _BiasFreeLinear.apply(h.view(B * F, E), self.linear1.weight).view(B, F)
        z2 = _BiasFreeLinear.apply(h.view(B, F * E), self.linear2["0"].weight)
        return _AttnPredict.apply(score, z2)
