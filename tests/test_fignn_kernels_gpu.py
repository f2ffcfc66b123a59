"""csrc/fignn.hip against float64 torch restatements of the reference's FiGNN arithmetic (layers.py:300-379) on the
same inputs: the attention graph, one GraphLayer + GRUCell step, their backward kernels with the weight gradients,
the prediction head's combining kernel, and the whole trunk through its autograd node.

Forward at FWD_TOL, gradients at GRAD_TOL (both tests/test_mha_gpu.py's bounds); no tensor needed more.  Inputs are
repaired so that no off-diagonal pre-activation of the graph lies within 1e-5 of the Leaky-ReLU's kink.  Shapes: B in
{1, 5, 67} (no multiple of a sample tile), F in {2, 3, 23, 39, 64}, E in {4, 16, 32}: W_in / W_out staged in LDS in
both directions (F <= 3), staged forward but streamed backward (F=23, E=16) and streamed in both (F=39, F=64)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=2e-5)
SHAPES = [(1, 2, 4), (5, 3, 4), (67, 2, 16), (67, 23, 16), (5, 39, 16), (1, 39, 16), (67, 3, 32), (5, 23, 32),
          (5, 64, 32), (67, 64, 4)]
# (B, F, E, L, res_conn, reuse_graph_layer)
TRUNKS = [(5, 3, 4, 1, False, False), (67, 23, 16, 3, True, True), (5, 39, 16, 3, False, False),
          (67, 23, 16, 3, True, False), (1, 2, 16, 1, True, True), (5, 64, 32, 3, False, True)]
PRE_MARGIN = 1e-5


def _close(got, want, tol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = float((got - want).abs().max()) if got.numel() else 0.0
    print(f"{what}: max |err| {err:.3e}, max |ref| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got, want, msg=lambda m: f"{what}: {m}", **tol)


def _repair(x, wa):
    """Move s_i by 1e-3 wherever an off-diagonal pre = s_i + d_j is within the margin of zero; assert the result."""
    E = x.shape[-1]
    off = ~torch.eye(x.shape[1], dtype=torch.bool)
    src = wa[0, :E].double()
    for _ in range(20):
        xd = x.double()
        pre = (xd @ src)[:, :, None] + (xd @ wa[0, E:].double())[:, None, :]
        bad = ((pre.abs() < 4 * PRE_MARGIN) & off).any(dim=2)
        if not bool(bad.any()):
            break
        x = x + (bad.float()[:, :, None] * 1e-3) * (src / (src @ src)).float()
    xd = x.double()
    pre = (xd @ src)[:, :, None] + (xd @ wa[0, E:].double())[:, None, :]
    assert float(pre.abs()[:, off].min()) > PRE_MARGIN
    return x


@functools.lru_cache(maxsize=None)
def _inputs(B, F, E, layers=1):
    gen = torch.Generator().manual_seed(1000 * B + 10 * F + E)
    rnd = lambda *shape, scale=1.0: torch.randn(*shape, generator=gen) * scale            # noqa: E731
    wa = rnd(1, 2 * E, scale=0.7)
    x = _repair(rnd(B, F, E, scale=0.5), wa)
    bound = E ** -0.5
    gru = [torch.empty(3 * E, E).uniform_(-bound, bound, generator=gen), torch.empty(3 * E, E).uniform_(-bound, bound, generator=gen),
           torch.empty(3 * E).uniform_(-bound, bound, generator=gen), torch.empty(3 * E).uniform_(-bound, bound, generator=gen)]
    gnn = [[rnd(F, E, E, scale=0.3), rnd(F, E, E, scale=0.3), rnd(E, scale=0.2)] for _ in range(layers)]
    return dict(x=x, wa=wa, gru=gru, gnn=gnn, h=rnd(B, F, E, scale=0.6), dh=rnd(B, F, E), dg=rnd(B, F, F),
                base=rnd(B, F, E), add=rnd(B, F, E))


def ref_graph(x, wa):
    E = x.shape[-1]
    s, d = x @ wa[0, :E], x @ wa[0, E:]
    pre = s[:, :, None] + d[:, None, :]
    alpha = torch.nn.functional.leaky_relu(pre, 0.01)
    alpha = alpha.masked_fill(torch.eye(x.shape[1], dtype=torch.bool), float("-inf"))
    return torch.softmax(alpha, dim=-1), s, d


def ref_layer(h, g, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, x_res=None):
    E = h.shape[-1]
    h_out = torch.matmul(w_out, h.unsqueeze(-1)).squeeze(-1)
    aggr = torch.bmm(g, h_out)
    a = torch.matmul(w_in, aggr.unsqueeze(-1)).squeeze(-1) + bias_p
    gi, gh = a @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[..., :E] + gh[..., :E])
    z = torch.sigmoid(gi[..., E:2 * E] + gh[..., E:2 * E])
    n = torch.tanh(gi[..., 2 * E:] + r * gh[..., 2 * E:])
    out = (1 - z) * n + z * h
    return out + x_res if x_res is not None else out


def _dev(ts):
    return [t.to(DEV) for t in ts]


def _f64(ts, grad=True):
    return [t.double().clone().requires_grad_(grad) for t in ts]


@pytest.mark.parametrize("B,F,E", SHAPES)
def test_graph_forward_and_backward(B, F, E):
    from mapx import ops
    I = _inputs(B, F, E)
    x, wa = I["x"].to(DEV), I["wa"].to(DEV)
    g, s, d = ops.fignn_graph_fwd(x, wa)
    xr, war = _f64([I["x"], I["wa"]])
    gr, sr, dr = ref_graph(xr, war)
    _close(g, gr, FWD_TOL, "g")
    _close(s, sr, FWD_TOL, "s")
    _close(d, dr, FWD_TOL, "d")
    assert bool((torch.diagonal(g, dim1=1, dim2=2) == 0).all())
    assert float((g.sum(dim=2) - 1).abs().max()) <= 1e-6
    if F == 2:
        assert bool((g[:, 0, 1] == 1).all()) and bool((g[:, 1, 0] == 1).all())
    # backward: dx = base + add + the graph's input gradient, dW_attn
    dg, base, add = I["dg"].to(DEV), I["base"].to(DEV), I["add"].to(DEV)
    (gr * I["dg"].double()).sum().backward()
    dx, dwa = ops.fignn_graph_bwd(dg, g, s, d, x, wa, base, dx_add=add)
    _close(dx, xr.grad + I["base"].double() + I["add"].double(), GRAD_TOL, "dx")
    _close(dwa, war.grad, GRAD_TOL, "dW_attn")
    dx1, _ = ops.fignn_graph_bwd(dg, g, s, d, x, wa, base)
    _close(dx1, xr.grad + I["base"].double(), GRAD_TOL, "dx without add")
    # a second run is bitwise equal; in place over the base too
    dx2, dwa2 = ops.fignn_graph_bwd(dg, g, s, d, x, wa, base.clone(), dx_add=add, inplace=True)
    assert torch.equal(dx2, dx) and torch.equal(dwa2, dwa)


@pytest.mark.parametrize("B,F,E", SHAPES)
def test_layer_forward_and_backward(B, F, E):
    from mapx import ops
    I = _inputs(B, F, E)
    weights = I["gnn"][0] + I["gru"]
    g64 = ref_graph(I["x"].double(), I["wa"].double())[0]
    g = g64.float()
    h, x = I["h"], I["x"]
    wd, hd, gd, xd = _dev(weights), h.to(DEV), g.to(DEV), x.to(DEV)
    for res in (False, True):
        got = ops.fignn_layer_fwd(hd, gd, *wd, x_res=xd if res else None)
        want = ref_layer(h.double(), g.double(), *[w.double() for w in weights], x_res=x.double() if res else None)
        _close(got, want, FWD_TOL, f"h_next (res={res})")
    # backward against autograd in float64 (g as a leaf: dg is the gradient with respect to the graph)
    hr, gr, *wr = _f64([h, g] + weights)
    (ref_layer(hr, gr, *wr) * I["dh"].double()).sum().backward()
    dhd = I["dh"].to(DEV)
    dg = torch.full((B, F, F), float("nan"), device=DEV)
    dxa = torch.full((B, F, E), float("nan"), device=DEV)
    dh, grads = ops.fignn_layer_bwd(dhd, hd, gd, *wd, dg, True, dx_acc=dxa, dx_init=True)
    _close(dh, hr.grad, GRAD_TOL, "dh")
    _close(dg, gr.grad, GRAD_TOL, "dg")
    assert torch.equal(dxa, dhd)
    names = ("dW_in", "dW_out", "dbias_p", "dW_ih", "dW_hh", "db_ih", "db_hh")
    for name, got, ref in zip(names, grads, wr):
        _close(got, ref.grad, GRAD_TOL, name)
    # a second run that ADDS to everything gives exactly twice the first (x + x is exact): bitwise repeatable, and
    # the accumulating forms (dg, dx over the layers; the shared GRU; reuse_graph_layer) add in place
    first = [t.clone() for t in [dh, dg, dxa] + list(grads)]
    dh2, grads2 = ops.fignn_layer_bwd(dhd, hd, gd, *wd, dg, False, dx_acc=dxa, dx_init=False, grads=list(grads),
                                      add_layer=True, add_gru=True)
    assert torch.equal(dh2, first[0])
    for name, now, was in zip(("dg", "dx_acc") + names, [dg, dxa] + list(grads2), first[1:]):
        assert torch.equal(now, 2 * was), name
    # ... and overwriting destinations that hold something else gives the first result again
    dh3, grads3 = ops.fignn_layer_bwd(dhd, hd, gd, *wd, dg, True, grads=list(grads2))
    assert torch.equal(dh3, first[0]) and torch.equal(dg, first[1])
    for name, now, was in zip(names, grads3, first[3:]):
        assert torch.equal(now, was), name


def test_lds_decision_at_the_tested_shapes():
    from mapx import ops
    staged = {(F, E): (ops.fignn_weights_staged(F, E), ops.fignn_weights_staged(F, E, backward=True))
              for _, F, E in SHAPES}
    assert staged[(23, 16)] == (True, False) and staged[(3, 32)] == (True, True) and staged[(2, 16)] == (True, True)
    assert staged[(39, 16)] == (False, False) and staged[(64, 32)] == (False, False)


@pytest.mark.parametrize("B,F", [(1, 2), (5, 23), (67, 39), (67, 64)])
def test_prediction_head(B, F):
    from mapx import ops
    gen = torch.Generator().manual_seed(B + F)
    score, z2, gl = torch.randn(B, F, generator=gen), torch.randn(B, F, generator=gen) * 2, torch.randn(B, 1, generator=gen)
    sr, zr = _f64([score, z2])
    want = (torch.sigmoid(zr) * sr).sum(dim=1, keepdim=True)
    got = ops.fignn_pred_fwd(score.to(DEV), z2.to(DEV))
    _close(got, want, FWD_TOL, "logits")
    (want * gl.double()).sum().backward()
    ds, dz = ops.fignn_pred_bwd(gl.to(DEV), score.to(DEV), z2.to(DEV))
    _close(ds, sr.grad, GRAD_TOL, "dscore")
    _close(dz, zr.grad, GRAD_TOL, "dz2")
    ds2, dz2 = ops.fignn_pred_bwd(gl.to(DEV), score.to(DEV), z2.to(DEV))
    assert torch.equal(ds, ds2) and torch.equal(dz, dz2)


@pytest.mark.parametrize("B,F,E,L,res,reuse", TRUNKS)
def test_trunk_autograd_node(B, F, E, L, res, reuse):
    """FiGNNBlock.forward through layers._FiGNNTrunk: output and every gradient against float64 autograd."""
    from mapx.layers import _FiGNNTrunk
    I = _inputs(B, F, E, layers=3)
    nl = 1 if reuse else L
    flat = [w for layer in I["gnn"][:nl] for w in layer]
    leaves = [I["x"], I["wa"]] + I["gru"] + flat
    xr, war, *rest = _f64(leaves)
    g64 = ref_graph(xr, war)[0]
    hr = xr
    for l in range(L):
        k = 0 if reuse else 3 * l
        hr = ref_layer(hr, g64, *rest[4 + k:4 + k + 3], *rest[:4], x_res=xr if res else None)
    (hr * I["dh"].double()).sum().backward()

    def run():
        dev = [t.to(DEV).requires_grad_(True) for t in leaves]
        out = _FiGNNTrunk.apply(dev[0], dev[1], *dev[2:6], res, reuse, L, *dev[6:])
        out.backward(I["dh"].to(DEV))
        return out.detach(), [t.grad for t in dev]
    out, grads = run()
    _close(out, hr, FWD_TOL, "h")
    names = ["dx", "dW_attn", "dW_ih", "dW_hh", "db_ih", "db_hh"] + [f"{n}[{i // 3}]" for i, n in
                                                                    enumerate(["dW_in", "dW_out", "dbias_p"] * nl)]
    for name, got, ref in zip(names, grads, [xr, war] + rest):
        _close(got, ref.grad, GRAD_TOL, name)
    out2, grads2 = run()
    assert torch.equal(out, out2)
    for name, a, b in zip(names, grads, grads2):
        assert torch.equal(a, b), name


def test_shapes_outside_the_range_are_refused():
    from mapx import ops
    from mapx.native import MapxError

    def graph(B, F, E):
        return ops.fignn_graph_fwd(torch.zeros(B, F, E, device=DEV), torch.zeros(1, 2 * E, device=DEV))
    for F, E, word in ((1, 16, "num_fields"), (65, 16, "num_fields"), (23, 36, "embed_size"), (23, 6, "embed_size")):
        with pytest.raises(MapxError, match=word):
            graph(2, F, E)
        w = [torch.zeros(F, E, E), torch.zeros(F, E, E), torch.zeros(E), torch.zeros(3 * E, E), torch.zeros(3 * E, E),
             torch.zeros(3 * E), torch.zeros(3 * E)]
        with pytest.raises(MapxError, match=word):
            ops.fignn_layer_fwd(torch.zeros(2, F, E, device=DEV), torch.zeros(2, F, F, device=DEV), *_dev(w))
    with pytest.raises(ValueError):         # weights of another shape than the state
        ops.fignn_layer_fwd(torch.zeros(2, 3, 4, device=DEV), torch.zeros(2, 3, 3, device=DEV),
                            *_dev([torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), torch.zeros(4), torch.zeros(12, 8),
                                   torch.zeros(12, 4), torch.zeros(12), torch.zeros(12)]))
    with pytest.raises(TypeError):
        ops.fignn_graph_fwd(torch.zeros(2, 3, 4, device=DEV, dtype=torch.float64), torch.zeros(1, 8, device=DEV))
