"""The host state the fp32 GEMMs are handed (csrc/gemm_h2.hip, csrc/gemm_h2w.hip) still describes the tensor when the
product runs: weight planes first cut by an evaluation between the replays of a captured step, the magnitude record
of a gradient that autograd accumulated in place, a record whose ring slot went to another tensor — and the on-call
check of every record (ops.AMAX_CHECK) over one eager step of every model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mapx import ops as _ops
    return _ops


def _cpu(x):
    return x.detach().cpu()


def _trainer(cfg, pt, rows, batch, out_dir, backbone="DCNv2", use_graph=False, lr=1e-3, sched="cosine", eval_rows=600):
    """A Trainer over synthetic rows, begun (optimizer built), as tools/h2_usage.py and tests/test_trainer_gpu.py
    build theirs -> (trainer, model, the resident train split)."""
    from mapx.arguments import TrainingArguments
    from mapx.dataset import OurDataset, synth_table
    from mapx.models import BaseModel
    from mapx.trainer import Trainer
    from util import make_config
    ids, labels, _, _ = synth_table(rows, cfg["F"], cfg["V"], seed=3)
    cnt = np.bincount(ids.reshape(-1), minlength=cfg["V"]).astype(np.float32)
    torch.manual_seed(5)
    if backbone == "Trans":
        import trans_params as tp
        config = tp.make_config(cfg, pt, "Trans", cnt)
    elif backbone == "FGCNN":
        import fgcnn_params as fp
        config = fp.make_config(cfg, pt, "FGCNN", cnt, channels="3,4", kernel_heights="3,5", pooling_sizes="2,2",
                                recombined_channels="2,1")
    else:
        config = make_config(cfg, pt, cnt, backbone=backbone)
    model = BaseModel.from_config(config)
    targs = TrainingArguments(output_dir=str(out_dir), per_gpu_train_batch_size=batch, per_gpu_eval_batch_size=batch,
                              learning_rate=lr, lr_sched=sched, weight_decay=5e-2, num_train_epochs=1,
                              pretrain=pt != "CTR", pt_type=pt if pt != "CTR" else "MFP", sampling_method="randint",
                              RFD_replace="Unigram", mask_ratio=0.3, seed=11)
    targs._device = torch.device(DEV)
    tr = Trainer(model, config, targs, OurDataset(ids, labels), OurDataset(ids[:eval_rows], labels[:eval_rows]))
    tr.use_graph = use_graph
    train = tr._begin("test")
    model.train()
    return tr, model, train


# ----------------------------------------------------------------------------- A: planes registered after the capture
A_CFG = dict(F=24, V=300, E=16, H=384, NL=2, NC=2, P=32, K=5)      # D = F E = 384 = 12 x 32: whole K-steps
A_TRAIN, A_EVAL = 128, 2816        # 1 x 6 tiles: no layer wants planes | 22 x 6 = 132 >= 128: every 384-wide weight does


class _Run:
    """DCNv2 / CTR through Trainer.run_step with use_graph: 3 eager steps, then the captured step's replays."""

    def __init__(self, tmp_path):
        from mapx.trainer import GraphedStep
        self.tr, self.model, train = _trainer(A_CFG, "CTR", A_TRAIN * 32, A_TRAIN, tmp_path, use_graph=True, lr=1e-2,
                                              sched="const", eval_rows=A_EVAL)
        self.batches = iter(train.batches(A_TRAIN, True, self.tr._generator(), (0, 1)))
        self.Xe, self.Ye = next(iter(self.tr._split(self.tr.eval_dataset).batches(A_EVAL, False)))
        assert self.Xe.shape[0] == A_EVAL
        self.GraphedStep = GraphedStep

    def steps(self, n):
        for _ in range(n):
            X, Y = next(self.batches)
            self.tr.run_step("ctr", X, Y)

    def replays(self, n):
        self.steps(n)
        graphs = list(self.tr._graphs.values())
        assert len(graphs) == 1 and isinstance(graphs[0], self.GraphedStep)

    def eval_logits(self):
        """The eval batch's logits by the call Trainer.eval makes."""
        self.tr.optimizer.flush()
        self.model.eval()
        with torch.no_grad():
            out = self.model(input_ids=self.Xe, labels=self.Ye)[1].view(-1).clone()
        self.model.train()
        return out

    def plane_keys(self):
        return {(n, key) for n, p in self.model.named_parameters() for key in (getattr(p, "_planes", None) or {})}


def test_eval_between_replays_reads_the_current_weights(ops, monkeypatch, tmp_path):
    """Train batch 128 (no product wants weight planes), eval batch 2816 (every 384-wide weight does): the planes are
    first cut by the evaluation that follows the capture, so the captured step's refresh launch does not know them.
    The second evaluation, 20 replays later, must read planes of the weights as they are then: bit-identical to the
    logits after MapxOptimizer.refresh_bf16() re-cut every set (both cuts use the exact maximum).  Power: the
    weights moved by far more than planes and in-kernel cut differ (which, at K = 384 = whole K-steps, is nothing)."""
    monkeypatch.setattr(ops, "H2", True)
    monkeypatch.setattr(ops, "H2W", True)
    run = _Run(tmp_path)
    run.steps(3)
    run.replays(2)
    before = run.plane_keys()
    eval1 = run.eval_logits()
    late = run.plane_keys() - before
    assert late, "the evaluation registered no plane set of its own: not the scenario meant"
    run.replays(20)
    eval2 = run.eval_logits()
    run.tr.optimizer.refresh_bf16()
    fresh = run.eval_logits()
    with monkeypatch.context() as m:
        m.setattr(ops, "H2W", False)
        plain = run.eval_logits()
    moved = float((eval1 - eval2).abs().max())
    cut = float((fresh - plain).abs().max())
    scale = max(1.0, float(plain.abs().max()))
    stale = float((eval2 - fresh).abs().max())
    print(f"\nsets first cut by the evaluation: {len(late)}; max|eval1 - eval2| = {moved:.3e}, max|eval2 - fresh| = "
          f"{stale:.3e}, max|fresh - plain| = {cut:.3e}, logit scale {scale:.3e}")
    assert torch.equal(eval2, fresh), f"the second evaluation read stale planes: max|eval2 - fresh| = {stale:.3e}"
    assert cut <= 1e-5 * scale
    assert moved >= 100.0 * cut and moved >= 100.0 * 1e-5 * scale


def test_input_gradient_between_replays_reads_the_current_weights(ops, monkeypatch, tmp_path):
    """The same with the planes of the weight as operand B of the INPUT gradient (ops.linear_bwd_input ->
    weight_planes(w, False, M)): one eager forward + backward of the 2816-row batch registers them after the capture,
    a second one 20 replays later must multiply by the current weights — every such dX against the same call with
    H2W off (the in-kernel cut of the weight as it is), by test_gemm_backward_products' bound."""
    monkeypatch.setattr(ops, "H2", True)
    monkeypatch.setattr(ops, "H2W", True)
    run = _Run(tmp_path)
    run.steps(3)
    run.replays(2)
    seen = []
    orig = ops.linear_bwd_input

    def spy(dy, w, out=None, add=None, relu_of=None, colsum_to=None):
        dx = orig(dy, w, out=out, add=add, relu_of=relu_of, colsum_to=colsum_to)
        if add is None and out is None and ops.weight_planes(w, False, dy.shape[0]) is not None:
            with monkeypatch.context() as m:
                m.setattr(ops, "H2W", False)
                seen.append((dy.detach().clone(), w.detach().clone(), dx.detach().clone(),
                             orig(dy, w, relu_of=relu_of).detach().clone()))
        return dx

    def fwd_bwd():
        loss, _ = run.model(input_ids=run.Xe, labels=run.Ye)
        loss.backward()
        ops.join_pending()
        ops.flush_deferred()
        run.tr.optimizer.zero_grad()

    before = run.plane_keys()
    fwd_bwd()
    late = run.plane_keys() - before
    assert any(not key[0] for _, key in late), "the backward pass registered no input-gradient planes"
    run.replays(20)
    monkeypatch.setattr(ops, "linear_bwd_input", spy)
    fwd_bwd()
    assert seen, "no input gradient took weight planes"
    worst = 0.0
    for dy, w, dx, dx_plain in seen:
        assert bool(torch.isfinite(dx).all())
        bound = 2e-6 * (dy.abs().double() @ w.abs().double()) + 1e-6
        err = (dx.double() - dx_plain.double()).abs()
        worst = max(worst, float((err / bound).max()))
        # (the step's gradients are small enough for the bound's absolute 1e-6 to dominate; at K = 384, whole K-steps,
        # planes of the current weight give the in-kernel cut's very sums: tests/test_amax_gpu.py)
        assert torch.equal(dx, dx_plain)
    print(f"\ninput gradients from planes: {len(seen)}; worst |dX - dX(H2W off)| / bound = {worst:.3e}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------- B: a gradient accumulated in place
@pytest.mark.parametrize("large", ["L1", "L2"])
def test_fan_out_gradient_carries_a_true_record(ops, monkeypatch, large):
    """y = L0(x) feeds L1 and L2: autograd sums the second branch's gradient into the first-arrived one in place, and
    the Python attribute that carried the first one's record survives the add_.  One branch's weight is 2^6 times the
    other's, so the sum's maximum is far above either order's first record.  L0.backward's two products (dW = gy^T x,
    dX = gy W0) must not be scaled by it: the on-call check passes, both results are finite and within
    test_gemm_backward_products' bounds of fp64.  (The branch weights are multiples of 2^-6 with |w| <= 1/8: the
    accumulated gy is exact in fp32 under every arithmetic, so the fp64 reference has the products' own operands.)"""
    from mapx import layers
    monkeypatch.setattr(ops, "H2", True)
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    M = W = 64
    g = torch.Generator().manual_seed(7)
    L0, L1, L2 = (layers.HipLinear(W, W).to(DEV) for _ in range(3))
    with torch.no_grad():
        for L in (L1, L2):
            L.weight.copy_(torch.randint(-8, 9, (W, W), generator=g).float() / 64)
        (L1 if large == "L1" else L2).weight.mul_(64.0)
    for L in (L0, L1, L2):                          # records of the weights (an optimizer would keep them)
        ops.tag(L.weight, ops.amax(L.weight.detach()))
    x = torch.randn(M, W, generator=g).to(DEV).requires_grad_(True)
    ops.tag(x, ops.amax(x.detach()))
    y = L0(x)
    loss = L1(y).sum() + L2(y).sum()
    loss.backward()                                 # (AMAX_CHECK: a record below its operand's maximum raises here)
    dw, dx = L0.weight.grad, x.grad
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dx).all())
    gy = (L1.weight.detach().double().sum(0) + L2.weight.detach().double().sum(0)).cpu().expand(M, W)
    xd, w0 = _cpu(x).double(), _cpu(L0.weight).double()
    bound = 2e-6 * (gy.abs() @ w0.abs()) + 1e-6
    assert bool(((_cpu(dx).double() - gy @ w0).abs() <= bound).all())
    boundw = 4e-6 * (gy.abs().t() @ xd.abs()) + 1e-6
    assert bool(((_cpu(dw).double() - gy.t() @ xd).abs() <= boundw).all())


# ----------------------------------------------------------------------------- C: a recycled ring slot
def test_a_recycled_ring_slot_is_not_believed(ops, monkeypatch):
    """y's record comes from the ring of eager records; 4096 hand-outs later its slot belongs to another tensor (and
    was zeroed).  A product with y as operand A must not be scaled by what the slot holds now."""
    monkeypatch.setattr(ops, "H2", True)
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    g = torch.Generator().manual_seed(3)
    M = N = K = 64
    x, w, b = (torch.randn(*s, generator=g).to(DEV) for s in ((M, K), (N, K), (N,)))
    w2, b2 = torch.randn(N, N, generator=g).to(DEV) / 8, torch.randn(N, generator=g).to(DEV)
    ops.tag(w2, ops.amax(w2))                       # operand B's record: the product would take the two-piece arithmetic
    y = ops.linear_fwd(x, w, b)
    assert ops.amax_value(ops.amax_of(y)) == float(y.abs().max())
    for _ in range(ops._RING):
        ops.amax_record(y.device)
    z = ops.linear_fwd(y, w2, b2)                   # (AMAX_CHECK: a record below y's maximum raises here)
    rec = ops.amax_of(y)
    assert rec is None or ops.amax_value(rec) == float(y.abs().max())
    ref = _cpu(y).double() @ _cpu(w2).double().t() + _cpu(b2).double()
    bound = 2e-6 * (_cpu(y).abs().double() @ _cpu(w2).abs().double().t()) + 1e-6
    assert bool(((_cpu(z).double() - ref).abs() <= bound).all())


# ----------------------------------------------------------------------------- D: the on-call check, switched on
D_CFG = dict(F=23, V=3000, E=16, H=256, NL=3, NC=3, P=32, K=25)     # tools/h2_usage.py's sizes


def _checked_steps(ops, monkeypatch, tmp_path, backbone, pt, cfg=D_CFG, steps=3):
    monkeypatch.setattr(ops, "H2", True)
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    tr, model, train = _trainer(cfg, pt, 512 * steps, 512, tmp_path, backbone=backbone)
    kind = {"MFP": "mfp", "RFD": "rfd", "CTR": "ctr"}[pt]
    for i, (X, Y) in enumerate(train.batches(512, True, tr._generator(), (0, 1))):
        monkeypatch.setattr(ops, "H2_USED", [0, 0])
        tr.run_step(kind, X, Y)                     # (eager: the check skips captures; a wrong record raises)
    torch.cuda.synchronize()
    assert tr.global_step == steps and not tr._graphs
    print(f"\n{backbone} {pt}: products with both records {ops.H2_USED[0]}, without {ops.H2_USED[1]}")
    return ops.H2_USED


@pytest.mark.parametrize("backbone", ["DCNv2", "DNN"])
@pytest.mark.parametrize("pt", ["MFP", "RFD", "CTR"])
def test_every_record_of_the_tower_models_steps_is_true_and_used(ops, monkeypatch, tmp_path, backbone, pt):
    """Three eager steps with every record compared with its operand on the host; on the third, every fp32 product
    is handed both records: the hot path takes the two-piece arithmetic at all."""
    used = _checked_steps(ops, monkeypatch, tmp_path, backbone, pt)
    assert used[1] == 0 and used[0] > 0, used


@pytest.mark.parametrize("backbone,pt", [("AutoInt", "CTR"), ("DeepFM", "MFP"), ("xDeepFM", "CTR"), ("Trans", "MFP"),
                                         ("FGCNN", "CTR")])
def test_every_record_of_the_other_backbones_steps_is_true(ops, monkeypatch, tmp_path, backbone, pt):
    """The same check over the other backbones' steps (products without records are allowed there).  The
    Transformer's hidden_size is its d_model (= embed_size, <= 64): 16 instead of the towers' 256."""
    cfg = dict(D_CFG, H=16, NL=2, NC=0) if backbone == "Trans" else D_CFG
    _checked_steps(ops, monkeypatch, tmp_path, backbone, pt, cfg=cfg)
