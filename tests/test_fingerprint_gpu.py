"""State fingerprint on the GPU: the HIP kernel against the numpy restatement (tests/fingerprint_ref.py: exact
equality of F and of every chunk value), independence of the launch geometry, sensitivity to single bits / swapped
words / swapped chunks, argument checks; replica.state_fingerprint over a small model's training state (coverage,
one entry per buffer, no effect on the trajectory, no flush); the fingerprint stored in the resume file."""
import functools

import numpy as np
import pytest
import torch

import fingerprint_ref as R
import paramgen as pg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = R.CHUNK
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 65535, 65536, 65537, 3 * 65536 + 17]
GUARD = 0x5EEDFACE          # words around a view: reading one of them changes every sum it enters


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _case(kind, n):
    """(words uint32 [n], reference F, reference chunk values): computed once, shared, never written."""
    rng = np.random.default_rng(1000 * n + len(kind))
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)     # any bit pattern: NaNs, subnormals too
    if kind == "fp32" and n:
        special = np.array([0x7FC00000, 0xFFC00001, 0x7FA00123,      # quiet NaN, negative NaN, a payload
                            0x7F800000, 0xFF800000,                  # +inf, -inf
                            0x80000000, 0x00000000,                  # -0.0, +0.0
                            0x00000001, 0x807FFFFF], dtype=np.uint32)                 # smallest / largest subnormal
        k = min(n, special.size)
        w[np.arange(k) * 7 % n] = special[:k]
        w[-1] = 0x80000000
    w.setflags(write=False)
    f, c = R.fingerprint(w)
    return w, f, c


def _device_view(words, kind, offset):
    """The words as a device tensor of dtype `kind` that starts `offset` words into a buffer of guard words."""
    n = words.size
    buf = np.full(n + 8, GUARD, dtype=np.uint32)
    buf[offset:offset + n] = words
    t = torch.from_numpy(buf.view(np.float32 if kind == "fp32" else np.int32)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t[offset:offset + n]


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("kind", ["fp32", "int32"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement(ops, kind, n):
    words, f_ref, c_ref = _case(kind, n)
    for offset in (0, 1, 2, 3):                 # 16-byte aligned base, and views 1, 2, 3 words into a buffer
        view = _device_view(words, kind, offset)
        assert view.is_contiguous() and (n == 0 or view.data_ptr() % 16 == 4 * offset)   # (an empty view has no address)
        f, c = ops.fingerprint(view, chunks=True)
        assert c.dtype == torch.int64 and c.numel() == c_ref.size
        assert np.array_equal(_u64(c), c_ref), (kind, n, offset)
        assert f == f_ref, (kind, n, offset, hex(f), hex(f_ref))
        assert ops.fingerprint(view) == f_ref


def test_known_answers(ops):
    assert ops.fingerprint(torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)) == 0xb2b8f3852e23cea7
    w = ((np.arange(65537, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.uint32)
    f, c = ops.fingerprint(torch.from_numpy(w.view(np.int32)).to(DEV), chunks=True)
    assert [int(x) for x in _u64(c)] == [0xbd77ee3b23bb79a2, 0x0f49c86dbf34c4e0] and f == 0xb1d74df72eaa0ad7


def test_result_does_not_depend_on_the_grid(ops):
    words, f_ref, c_ref = _case("fp32", 3 * C + 17)
    view = _device_view(words, "fp32", 1)
    for blocks in (0, 1, 7):
        f, c = ops.fingerprint(view, chunks=True, blocks=blocks)
        assert f == f_ref and np.array_equal(_u64(c), c_ref), blocks


def test_grid_stride_over_300_chunks(ops):
    n = 299 * C + 123
    words = np.random.default_rng(5).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    f_ref, c_ref = R.fingerprint(words)
    assert c_ref.size == 300
    t = torch.from_numpy(words.view(np.int32)).to(DEV)
    for blocks in (7, 0):
        f, c = ops.fingerprint(t, chunks=True, blocks=blocks)
        assert f == f_ref and np.array_equal(_u64(c), c_ref), blocks


@pytest.mark.parametrize("where", ["first", "last", "65535", "65536"])
def test_one_flipped_bit_changes_F_and_exactly_its_chunk(ops, where):
    words, f_ref, c_ref = _case("int32", 3 * C + 17)
    i = {"first": 0, "last": words.size - 1, "65535": 65535, "65536": 65536}[where]
    t = torch.from_numpy(words.view(np.int32).copy()).to(DEV)
    t[i] ^= 1 << 9
    f, c = ops.fingerprint(t, chunks=True)
    assert f != f_ref
    assert np.flatnonzero(_u64(c) != c_ref).tolist() == [i // C]


def test_swapped_words_and_swapped_chunks_change_F(ops):
    words, f_ref, _ = _case("int32", 3 * C + 17)
    a, b = 10, 40000                            # the same chunk
    assert words[a] != words[b]
    w = words.copy()
    w[a], w[b] = words[b], words[a]
    assert ops.fingerprint(torch.from_numpy(w.view(np.int32)).to(DEV)) != f_ref
    w = words.copy()                            # chunks 0 and 1, whole
    assert not np.array_equal(words[:C], words[C:2 * C])
    w[:C], w[C:2 * C] = words[C:2 * C], words[:C]
    f, c = ops.fingerprint(torch.from_numpy(w.view(np.int32)).to(DEV), chunks=True)
    assert f != f_ref
    assert sorted(int(x) for x in _u64(c)) == sorted(int(x) for x in _case("int32", 3 * C + 17)[2])   # same chunk values


def test_wrong_dtype_and_strided_input_raise(ops):
    for dtype in (torch.float64, torch.int64, torch.bfloat16, torch.float16, torch.bool, torch.uint8):
        with pytest.raises((TypeError, ValueError)):
            ops.fingerprint(torch.zeros(8, device=DEV).to(dtype))
    with pytest.raises((TypeError, ValueError)):
        ops.fingerprint(torch.zeros(16, device=DEV)[::2])
    with pytest.raises((TypeError, ValueError)):
        ops.fingerprint(torch.zeros(4, 6, device=DEV).t())


# ----------------------------------------------------------------------------- the training state
CASE = "B_f25_b64"


def _make(backbone):
    from mapx.arguments import TrainingArguments
    from mapx.optim import MapxOptimizer
    from util import build_model, t
    cfg = pg.CASES[CASE]
    inp = pg.make_inputs(CASE, cfg)
    model = build_model(cfg, "MFP", pg.make_params(CASE, cfg, "MFP", backbone), inp["feat_count"], device=DEV,
                        backbone=backbone)
    targs = TrainingArguments(output_dir="/tmp/mapx_fp", learning_rate=1e-3, weight_decay=5e-2, lr_sched="cosine")
    opt = MapxOptimizer(model, targs, num_training_steps=8, num_warmup_steps=0)
    model.train()
    L = inp["masked_index"].shape[1]

    def step(k):
        from mapx import ops as O
        perm = torch.randperm(cfg["B"], generator=torch.Generator().manual_seed(k))
        ids, mi, noise = (t(inp[key])[perm].to(DEV) for key in ("input_ids", "masked_index", "noise"))
        masked, labels, _ = O.dynamic_mask_mfp(ids, L, masked_index=mi)
        model(input_ids=masked, labels=labels, masked_index=mi, noise_samples=noise)[0].backward()
        opt.step()
    return model, opt, step


@pytest.fixture(scope="module", params=["DCNv2", "DeepFM"])
def trained(request):
    model, opt, step = _make(request.param)
    step(0)
    step(1)
    torch.cuda.synchronize()
    return request.param, model, opt


def test_state_fingerprint_entry_names(trained):
    from mapx import replica
    backbone, model, opt = trained
    fp = replica.state_fingerprint(model, opt)
    want = [f"dense{i}.{k}" for i in range(len(opt.groups)) for k in "pmv"]
    covered = {id(p) for g in opt.groups for p in g["params"]}
    for tb in model.row_tables():
        want += [f"{tb.name}.p0", f"{tb.name}.mv0", f"{tb.name}.last"]
        covered.add(id(tb.p0))
        if tb.p1 is not None:
            want += [f"{tb.name}.p1", f"{tb.name}.mv1"]
            covered.add(id(tb.p1))
    want.append("done")
    named = dict(model.named_parameters())
    named.update(model.named_buffers())
    want += [k for k in model.state_dict() if named[k].is_floating_point() and id(named[k]) not in covered]
    assert list(fp) == want
    assert len(opt.groups) == 2 and all(isinstance(v, int) and 0 <= v < 1 << 64 for v in fp.values())
    assert {"mfp_criterion.p0", "mfp_criterion.mv0", "mfp_criterion.last", "mfp_criterion.p1", "mfp_criterion.mv1",
            "embed.embedding.p0", "embed.embedding.mv0", "embed.embedding.last", "done"} <= set(fp)
    assert ("embed.embedding.p1" in fp and "embed.embedding.mv1" in fp) == (backbone == "DeepFM")
    assert not any(v.dtype == torch.bool and k in fp for k, v in model.state_dict().items())
    assert list(replica.state_fingerprint(model, opt).items()) == list(fp.items())          # a pure function of the state


def test_one_ulp_in_one_buffer_changes_that_entry_only(trained):
    from mapx import replica
    _, model, opt = trained
    base = replica.state_fingerprint(model, opt)
    entries = replica.state_entries(model, opt)
    assert [e[0] for e in entries] == list(base)
    for name, tensor, _ in entries:
        assert tensor.element_size() == 4 and tensor.is_contiguous(), name
        bits = tensor.view(-1).view(torch.int32)
        i = bits.numel() // 2
        bits[i] += 1                    # the next representable value of a float, the next integer of a clock
        got = replica.state_fingerprint(model, opt)
        bits[i] -= 1
        assert [k for k in base if got[k] != base[k]] == [name]
    assert replica.state_fingerprint(model, opt) == base


def test_fingerprinting_between_steps_leaves_the_trajectory_and_the_stale_rows_alone():
    from mapx import replica
    finals = []
    for watch in (True, False):
        model, opt, step = _make("DCNv2")
        for k in range(4):
            step(k)
            if watch:
                stale = [t.stale for t in opt.tables]
                assert all(stale)                      # every table took a sparse update: rows wait for their replay
                fp = replica.state_fingerprint(model, opt)
                assert [t.stale for t in opt.tables] == stale and len(fp) > 8
        torch.cuda.synchronize()
        state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        for t in opt.tables:
            state[f"{t.table.name}/mv0"], state[f"{t.table.name}/last"] = t.mv0.cpu().clone(), t.last.cpu().clone()
        finals.append(state)
    assert set(finals[0]) == set(finals[1])
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


def test_resume_file_carries_and_checks_the_fingerprint(tmp_path):
    from mapx import replica
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    cfg = dict(F=23, V=3000, E=16, H=64, NL=3, NC=3, P=32, K=25)
    ids, labels, _, _ = synth_table(256 * 3, 23, cfg["V"], seed=4)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)

    def make():
        torch.manual_seed(9)
        config = make_config(cfg, "MFP", cnt)
        model = BaseModel.from_config(config)
        targs = TrainingArguments(output_dir=str(tmp_path), per_gpu_train_batch_size=256, per_gpu_eval_batch_size=256,
                                  learning_rate=1e-3, lr_sched="cosine", weight_decay=5e-2, num_train_epochs=1,
                                  pretrain=True, pt_type="MFP", sampling_method="randint", mask_ratio=0.3, seed=3)
        targs._device = torch.device(DEV)
        ds = OurDataset(ids, labels)
        tr = Trainer(model, config, targs, ds, ds)
        tr.use_graph = False
        train = tr._begin("test")
        model.train()
        return tr, list(train.batches(256, True, tr._generator(), (0, 1)))

    tr, batches = make()
    for X, Y in batches:
        tr.run_step("mfp", X, Y)
    good = str(tmp_path / "state.pt")
    tr.save_training_state(good)
    st = torch.load(good, map_location="cpu")
    assert st["fingerprint"] == dict(replica.state_fingerprint(tr.model, tr.optimizer))
    assert any(t.stale for t in tr.optimizer.tables)                # saved raw: nothing was flushed for it

    tr2, _ = make()
    tr2.load_training_state(good)                                   # round trip
    assert tr2.global_step == 3
    assert replica.state_fingerprint(tr2.model, tr2.optimizer) == replica.state_fingerprint(tr.model, tr.optimizer)

    m = st["optimizer"]["groups"][0]["m"]
    m[m.numel() // 3] += 1.0
    bad = str(tmp_path / "damaged.pt")
    torch.save(st, bad)
    tr3, _ = make()
    with pytest.raises(ValueError, match=r"dense0\.m"):
        tr3.load_training_state(bad)

    st = torch.load(good, map_location="cpu")
    del st["fingerprint"]
    old = str(tmp_path / "old.pt")
    torch.save(st, old)
    tr4, _ = make()
    tr4.load_training_state(old)                                    # files without the key load as before
    assert tr4.global_step == 3
