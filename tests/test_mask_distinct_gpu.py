"""Distinct-field masking on the device (sampling_method="normal": L distinct fields per row, drawn inside the mask
kernels).  The draw is pinned to its definition — masked_index == argsort(keys, stable)[:, :L] of the keys the test
entry returns, and those keys to a numpy restatement of Philox4x32-10 on the documented counters — through every
entry that draws; the law of the draw by chi-square; the Trainer's captured step by its eager twin."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, OFF = 0x5EED0123456789, 17
RFD_MODES = ("Unigram", "Uniform", "Whole-Uniform", "Whole-Unigram")


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as o
    return o


def _field_low(F):
    return torch.arange(F) * 100 + 10          # the id layout of test_dynamic_mask_generated_properties


def _ids(B, F, seed=0):
    g = torch.Generator().manual_seed(1000 * F + B + seed)
    return _field_low(F)[None, :] + torch.randint(0, 100, (B, F), generator=g)


def _philox(seed, ctr_lo, ctr_hi):
    """Philox4x32-10 of csrc/common.h on numpy uint64 arrays -> the four 32-bit words."""
    m32 = np.uint64(0xFFFFFFFF)
    u = lambda v: np.asarray(v, dtype=np.uint64)
    ctr_lo, ctr_hi = np.broadcast_arrays(u(ctr_lo), u(ctr_hi))
    k0, k1 = u(seed & 0xFFFFFFFF), u(seed >> 32)
    c0, c1, c2, c3 = ctr_lo & m32, ctr_lo >> np.uint64(32), ctr_hi & m32, ctr_hi >> np.uint64(32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + u(0x9E3779B9)) & m32, (k1 + u(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _keys_ref(B, F, seed, offset):
    """key(b, f) = word f & 3 of Philox(seed, counter 2^63 | (b * ceil(F/4) + f/4), offset)  (include/mapx_hip.h)."""
    nf4 = (F + 3) // 4
    b, f = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(F, dtype=np.uint64), indexing="ij")
    words = _philox(seed, np.uint64(1 << 63) | (b * np.uint64(nf4) + f // np.uint64(4)), np.uint64(offset))
    return np.choose((f & np.uint64(3)).astype(np.int64), [w.astype(np.int64) for w in words])


def _prefix(keys, L):
    return torch.argsort(keys, dim=1, stable=True)[:, :L]


@functools.lru_cache(maxsize=None)
def _keys(B, F, seed=SEED, offset=OFF):
    from mapx import ops as o
    return o.mask_distinct_keys(B, F, seed, offset).cpu()


# ------------------------------------------------------------------ 1. the definition
SHAPES = [(1, 1, 1), (33, 3, 1), (33, 4, 4), (257, 5, 2), (300, 23, 6), (300, 39, 11), (64, 64, 19), (64, 65, 65),
          (40, 130, 39), (33, 3, 0)]


@pytest.mark.parametrize("B,F,L", SHAPES)
def test_masked_index_is_the_stable_argsort_prefix_of_the_keys(ops, B, F, L):
    """F not a multiple of 4, F across 64, L = F (a whole permutation), L = 0, B across the kernel's 32-row blocks."""
    keys = _keys(B, F)
    assert keys.shape == (B, F) and int(keys.min()) >= 0 and int(keys.max()) < (1 << 32)
    assert np.array_equal(keys.numpy(), _keys_ref(B, F, SEED, OFF)), "keys != Philox on the documented counters"
    want = _prefix(keys, L)
    ids = _ids(B, F)
    m, labels, mi = ops.dynamic_mask_mfp(ids.to(DEV), L, seed=SEED, offset=OFF, distinct=True)
    k32 = ops.ids_to_i32(m, 10 + 100 * F)
    mi_c, m_c = mi.cpu(), m.cpu()
    assert mi_c.shape == (B, L) and torch.equal(mi_c, want)
    assert all(len(set(r)) == L for r in mi_c.tolist())
    assert torch.equal(labels.cpu(), torch.gather(ids, 1, mi_c))
    assert torch.equal(m_c, torch.scatter(ids, 1, mi_c, torch.full_like(mi_c, 3)))
    assert torch.equal(k32.cpu().view(B, F).long(), m_c)
    if L == 0:
        assert torch.equal(m_c, ids)
        r, y, _ = ops.dynamic_mask_rfd(ids.to(DEV), 0, x_train=ids.to(DEV), seed=SEED, offset=OFF, distinct=True)
        assert torch.equal(r.cpu(), ids) and not bool(y.any())


# ------------------------------------------------------------------ 2. one draw everywhere
def _rfd(ops, ids, L, mode, x_train, **kw):
    F = ids.shape[1]
    lo = _field_low(F).to(DEV)
    return ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=SEED, offset=OFF, mode=mode, idx_low=lo,
                                idx_high=lo + 100, vocab=10 + 100 * F, **kw)


def test_every_entry_draws_the_same_index(ops):
    N_, B, F, L, start = 2000, 300, 23, 6, 512
    split = _ids(N_, F).to(DEV)
    order = torch.randperm(N_, generator=torch.Generator().manual_seed(2)).to(DEV)
    sel = order[start:start + B].contiguous()
    plain = ops.dynamic_mask_mfp(split[sel], L, seed=SEED, offset=OFF, distinct=True)
    rows = ops.dynamic_mask_mfp(split, L, seed=SEED, offset=OFF, sel=sel, distinct=True)
    cur = torch.tensor([start], dtype=torch.int64, device=DEV)
    walk = ops.dynamic_mask_mfp(split, L, seed=SEED, offset=OFF, sel=order, sel_cursor=cur, batch=B, distinct=True)
    assert torch.equal(plain[2].cpu(), _prefix(_keys(B, F), L))
    for other in (rows, walk):                      # b is the batch row, not the split row
        for a, b in zip(plain, other):
            assert torch.equal(a, b)
    for mode in RFD_MODES:
        _, _, mi = _rfd(ops, split[sel], L, mode, split, distinct=True)
        assert torch.equal(mi, plain[2]), mode


# ------------------------------------------------------------------ 3. RFD
@pytest.mark.parametrize("mode", RFD_MODES)
def test_rfd_replaces_exactly_the_drawn_fields_from_the_stream_of_their_position(ops, mode):
    B, F, L, Ntrain = 300, 23, 6, 5000
    x_train = _ids(Ntrain, F, seed=1).to(DEV)
    ids = x_train[:B].clone()
    r, y, mi = _rfd(ops, ids, L, mode, x_train, distinct=True)
    ids_c, r_c, y_c, mi_c = ids.cpu(), r.cpu(), y.cpu(), mi.cpu()
    assert torch.equal(mi_c, _prefix(_keys(B, F), L))
    untouched = torch.ones(B, F, dtype=torch.bool).scatter_(1, mi_c, False)
    assert torch.equal(r_c[untouched], ids_c[untouched])
    assert torch.equal(y_c, (r_c != ids_c).float())
    if mode in ("Unigram", "Uniform"):              # replacements stay inside their own field's id range
        assert torch.equal((r_c - 10) // 100, torch.arange(F).expand(B, F))
    frac = float(y_c.mean())                        # L/F of the fields drawn, 1 in 100 (own range) replaced by itself
    assert 0.8 * L / F < frac <= L / F
    # the replacement of position l comes from philox(seed, b*L + l, offset): the injected index reproduces it
    r2, y2, mi2 = _rfd(ops, ids, L, mode, x_train, masked_index=mi)
    assert torch.equal(r2, r) and torch.equal(y2, y) and torch.equal(mi2, mi)


# ------------------------------------------------------------------ 4. streams
def test_streams_and_the_with_replacement_draw(ops):
    B, F, L = 257, 23, 6
    ids = _ids(B, F).to(DEV)
    a = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF, distinct=True)
    b = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF, distinct=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    k = torch.tensor([5], dtype=torch.int32, device=DEV)
    c = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF, offset_dev=k, distinct=True)
    d = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF + 5, distinct=True)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    assert not torch.equal(a[2], d[2])
    assert torch.equal(ops.mask_distinct_keys(B, F, SEED, OFF, offset_dev=k).cpu(), _keys(B, F, SEED, OFF + 5))
    x_train = _ids(3000, F, seed=1).to(DEV)
    e = ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=SEED, offset=OFF, offset_dev=k, distinct=True)
    f = ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=SEED, offset=OFF + 5, distinct=True)
    assert all(torch.equal(x, y) for x, y in zip(e, f)) and torch.equal(e[2], d[2])
    # the with-replacement instantiation: the old keyword set, distinct=False, and the definition it has always had
    # (masked_index[b,l] = word x of philox(seed, b*L + l, offset) scaled to [0, F)) agree
    old = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF)
    new = ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF, distinct=False)
    assert all(torch.equal(x, y) for x, y in zip(old, new))
    x = _philox(SEED, np.arange(B * L, dtype=np.uint64), np.uint64(OFF))[0]
    assert np.array_equal(old[2].cpu().numpy().reshape(-1), ((x * np.uint64(F)) >> np.uint64(32)).astype(np.int64))
    assert not torch.equal(old[2], a[2])
    old = ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=SEED, offset=OFF)
    new = ops.dynamic_mask_rfd(ids, L, x_train=x_train, seed=SEED, offset=OFF, distinct=False)
    assert all(torch.equal(x, y) for x, y in zip(old, new)) and torch.equal(old[2], ops.dynamic_mask_mfp(ids, L, seed=SEED, offset=OFF)[2])
    # an injected index wins over the flag
    inj = ops.dynamic_mask_mfp(ids, L, masked_index=old[2], seed=SEED, offset=OFF, distinct=True)
    assert torch.equal(inj[2], old[2])
    small = _ids(8, 3).to(DEV)
    with pytest.raises(ValueError, match="L = 4, F = 3"):
        ops.dynamic_mask_mfp(small, 4, distinct=True)
    with pytest.raises(ValueError, match="L = 4, F = 3"):
        ops.dynamic_mask_rfd(small, 4, x_train=small, distinct=True)


# ------------------------------------------------------------------ 5. the law
def test_the_draw_has_the_law_of_a_permutation_prefix(ops):
    """chi-square of the field marginals, of every position's field histogram and of the co-masked pairs against
    the uniform law of randperm(F)[:L]; bound df + 6 sqrt(2 df), the one of the with-replacement test."""
    B, F, L = 4096, 23, 6
    _, _, mi = ops.dynamic_mask_mfp(_ids(B, F).to(DEV), L, seed=42, offset=3, distinct=True)
    mi = mi.cpu()
    bound = lambda df: df + 6 * math.sqrt(2 * df)

    def chi2(counts, expect):
        return float(((counts.double() - expect) ** 2 / expect).sum())

    stats = {"marginal": chi2(torch.bincount(mi.view(-1), minlength=F), B * L / F)}
    for r in range(L):
        stats[f"position {r}"] = chi2(torch.bincount(mi[:, r], minlength=F), B / F)
    s = mi.sort(1).values
    pair = torch.zeros(F, F, dtype=torch.int64)
    for i in range(L):
        for j in range(i + 1, L):
            pair.index_put_((s[:, i], s[:, j]), torch.ones(B, dtype=torch.int64), accumulate=True)
    cells = pair[torch.triu(torch.ones(F, F, dtype=torch.bool), 1)]
    assert cells.numel() == 253 and int(cells.sum()) == B * 15 and int(pair.sum()) == B * 15
    stats["pairs"] = chi2(cells, B * 15 / 253)
    print(stats)
    for name, v in stats.items():
        assert v < bound(252 if name == "pairs" else F - 1), (name, v)


# ------------------------------------------------------------------ 6. Trainer
def _trajectory(pt, use_graph, monkeypatch):
    from mapx import ops
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import GraphedStep, Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(512 * 8, 23, cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    seen = []                                       # masked_index tensors as the mask wrappers returned them
    for name in ("dynamic_mask_mfp", "dynamic_mask_rfd"):
        def spy(*a, _f=getattr(ops, name), **kw):
            assert kw.get("distinct") is True and kw.get("masked_index") is None
            out = _f(*a, **kw)
            seen.append(out[2])
            return out
        monkeypatch.setattr(ops, name, spy)
    monkeypatch.setenv("MAPX_GRAPH", "1" if use_graph else "0")
    torch.manual_seed(5)
    config = make_config(cfg, pt, cnt)
    model = BaseModel.from_config(config)
    targs = TrainingArguments(output_dir="/tmp/mapx_mask_distinct_test", per_gpu_train_batch_size=512,
                              per_gpu_eval_batch_size=512, learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2,
                              num_train_epochs=1, pretrain=True, pt_type=pt, RFD_replace="Unigram",
                              sampling_method="normal", mask_ratio=0.3, logging_steps=7, seed=11)
    targs._device = torch.device(DEV)
    tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:600], labels[:600]))
    assert tr.use_graph == use_graph
    train = tr._begin("test")
    tr.model.train()
    losses, masks = [], []
    for X, Y in train.batches(512, True, tr._generator(), (0, 1), rows=True):
        out = tr.run_step(pt.lower(), X, Y)
        losses.append(out[0].detach().clone())
        masks.append(seen[-1].clone())              # under replay: the captured step's own output buffer
    assert tr.global_step == 8
    live = [g for g in tr._graphs.values() if not isinstance(g, int)]
    if use_graph:                                   # held as captured steps, not as counters of eager steps
        assert len(tr._graphs) == 1 and len(live) == 1 and isinstance(live[0], GraphedStep) and live[0].walk
        assert len(seen) == Trainer.GRAPH_AFTER + 1           # three eager steps and the capture; replays run no Python
    else:
        assert not live and len(seen) == 8
    tr.optimizer.flush()
    torch.cuda.synchronize()
    return (torch.stack(losses).cpu(), [m.cpu() for m in masks],
            {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})


@pytest.mark.parametrize("pt", ["MFP", "RFD"])
def test_trainer_captures_the_normal_step_and_replays_the_eager_trajectory(pt, monkeypatch):
    """sampling_method="normal": after GRAPH_AFTER eager steps the step is a captured hipGraph, and 8 steps of it
    leave the losses and every parameter of the eager loop (MAPX_GRAPH=0), bit for bit; the masks move with the
    device-side update counter under replay."""
    loss_g, masks_g, sd_g = _trajectory(pt, True, monkeypatch)
    loss_e, masks_e, sd_e = _trajectory(pt, False, monkeypatch)
    assert torch.equal(loss_g, loss_e), (loss_g, loss_e)
    for k in sd_e:
        assert torch.equal(sd_g[k], sd_e[k]), k
    for s, (a, b) in enumerate(zip(masks_g, masks_e)):
        assert a.shape == (512, 6) and torch.equal(a, b), s
        assert all(len(set(r)) == 6 for r in a.tolist())
    assert not torch.equal(masks_g[5], masks_g[6]) and not torch.equal(masks_g[6], masks_g[7])     # two replays
