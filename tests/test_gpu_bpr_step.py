"""The fused BPR training step on the HIP device (gcn_recommendation_amd.train, csrc/
lgcn_bpr_step.hip): the indexed loss against the gathered one, the deterministic scatter against
the sequential CPU index_put_, and whole steps against main.py's route (model(adj), six gathers,
bpr_loss_reg, backward) on the same device. Every comparison is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Cfg, case_dims, load_case
from gcn_recommendation_amd import engine, graph, train
from gcn_recommendation_amd.loss import bpr_loss_reg
from models.lightgcn import LightGCN
from models.lightgcn_fusion import LightGCN_Fusion

pytestmark = pytest.mark.gpu

LAMBDA = 1e-4


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- 1. indexed loss == gathered loss -----------------------------------------------------------
@pytest.mark.parametrize("B,d,sliced", [(1, 12, False), (5, 32, False), (257, 64, True),
                                        (512, 128, False)])
def test_indexed_loss_equals_gathered_loss(gpu_device, B, d, sliced):
    lib = engine.load_library()
    dev = gpu_device
    R = 300
    g = torch.Generator().manual_seed(B * 131 + d)
    if sliced:  # column slices of wider tables: ld > d
        tabs = [torch.randn(R, d + 8, generator=g).to(dev)[:, 3:3 + d] for _ in range(4)]
    else:
        tabs = [torch.randn(R, d, generator=g).to(dev) for _ in range(4)]
    fu, fi, u0, i0 = tabs
    bu, bp, bn = (torch.randint(0, R, (B,), generator=g).to(dev) for _ in range(3))

    def outputs():
        return (torch.empty(2 * B, device=dev), torch.full((), 7.0, device=dev),
                torch.full((6, B, d), 7.0, device=dev))

    t1, l1, g1 = outputs()
    t2, l2, g2 = outputs()
    stream = engine._stream(dev)
    args = []
    for t in tabs:
        args += [engine._ptr(t), t.stride(0)]
    assert lib.lgcn_bpr_loss_indexed(*args, R, R, engine._ptr(bu), engine._ptr(bp),
                                     engine._ptr(bn), B, d, LAMBDA, engine._ptr(t1),
                                     engine._ptr(l1), engine._ptr(g1), stream) == 0
    rows = [t.contiguous() for t in (fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn])]
    args = []
    for t in rows:
        args += [engine._ptr(t), t.stride(0)]
    assert lib.lgcn_bpr_loss(*args, B, d, LAMBDA, engine._ptr(t2), engine._ptr(l2),
                             engine._ptr(g2), stream) == 0
    assert same(l1, l2)
    for k in range(6):
        assert same(g1[k], g2[k]), k
    assert torch.isfinite(l1).item() and g1.abs().max().item() > 0


def test_indexed_loss_skips_samples_out_of_range(gpu_device):
    """A sample with an index outside its table: nothing of it is read, its gradient rows are
    zero; the other samples are untouched."""
    lib = engine.load_library()
    dev = gpu_device
    R, B, d = 50, 6, 32
    g = torch.Generator().manual_seed(2)
    tabs = [torch.randn(R, d, generator=g).to(dev) for _ in range(4)]
    bu, bp, bn = (torch.randint(0, R, (B,), generator=g) for _ in range(3))
    bu[1], bp[2], bn[4] = R, -1, 1 << 40
    bu, bp, bn = bu.to(dev), bp.to(dev), bn.to(dev)
    terms = torch.empty(2 * B, device=dev)
    loss = torch.empty((), device=dev)
    grads = torch.full((6, B, d), 7.0, device=dev)
    args = []
    for t in tabs:
        args += [engine._ptr(t), d]
    assert lib.lgcn_bpr_loss_indexed(*args, R, R, engine._ptr(bu), engine._ptr(bp),
                                     engine._ptr(bn), B, d, LAMBDA, engine._ptr(terms),
                                     engine._ptr(loss), engine._ptr(grads),
                                     engine._stream(dev)) == 0
    assert grads[:, [1, 2, 4]].count_nonzero().item() == 0
    assert all(grads[:, b].count_nonzero().item() > 0 for b in (0, 3, 5))
    assert torch.isfinite(loss).item()


# ---- 2. scatter == sequential index_put_ --------------------------------------------------------
def _sequential_index_put(rows, idx, src):
    """IndexBackward's reference on the host: index_put_ into zeros, accumulating in batch order.
    ATen's CPU kernel is sequential below 32768 elements and adds with atomics from several
    threads from there on (B = 512, d = 64 is exactly that size): one thread keeps it sequential
    at every size."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return torch.zeros(rows, src.shape[1]).index_put_((idx,), src, accumulate=True)
    finally:
        torch.set_num_threads(n)


def _sorted_keys(lib, ws, bu, bp, bn, U, I, stream):
    B = int(bu.shape[0])
    m, n_keys = 3 * B, 2 * (U + I) + 1
    ws.sort_scratch(lib, m, n_keys, stream)
    assert lib.lgcn_bpr_keys(engine._ptr(bu), engine._ptr(bp), engine._ptr(bn), B, U, I,
                             engine._ptr(ws.keys), stream) == 0
    b = ws.i32
    nbytes = ctypes.c_size_t(ws.temp_bytes)
    assert lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                  engine._ptr(b[1]), engine._ptr(b[2]), engine._ptr(b[3]),
                                  engine._ptr(ws.temp), ctypes.byref(nbytes), stream) == 0
    return m


@pytest.mark.parametrize("d", [12, 32, 64])
@pytest.mark.parametrize("R,B", [(64, 256), (1000, 512)])
def test_scatter_equals_sequential_reference(gpu_device, R, B, d):
    lib = engine.load_library()
    dev = gpu_device
    U = I = R
    extra = 37  # brand rows: never touched
    n = U + I + extra
    g = torch.Generator().manual_seed(R + d)
    bu, bp, bn = (torch.randint(0, R, (B,), generator=g) for _ in range(3))
    assert max(int(torch.bincount(t).max()) for t in (bu, bp, bn)) >= 3
    src = torch.randn(3 * B, d, generator=g)
    src[torch.rand(3 * B, d, generator=g) < 0.15] = 0.0
    src[torch.rand(3 * B, d, generator=g) < 0.15] = -0.0
    zero_rows = torch.rand(3 * B, generator=g) < 0.3
    src[zero_rows] = 0.0
    src[zero_rows & (torch.rand(3 * B, generator=g) < 0.5)] = -0.0
    want = torch.cat([_sequential_index_put(U, bu, src[:B]),
                      _sequential_index_put(I, bp, src[B:2 * B])
                      + _sequential_index_put(I, bn, src[2 * B:]),
                      torch.zeros(extra, d)])
    assert 0 < (want != 0).any(1).sum().item() < n

    ws = train._Workspace(n, d, dev)
    stream = engine._stream(dev)
    m = _sorted_keys(lib, ws, bu.to(dev), bp.to(dev), bn.to(dev), U, I, stream)
    s = src.to(dev)
    train._scatter(lib, ws, m, s, 0, U + I, ws.G, engine.LGCN_SCATTER_STORE, ws.mask, ws.count,
                   stream)
    assert same(ws.G.cpu(), want)
    mask, count = engine.rows_nonzero([ws.G], d, dev)
    assert torch.equal(ws.mask, mask)
    assert ws.count.item() == count.item() == (want != 0).any(1).sum().item()

    # ADD: one plain add per element of the touched rows == the dense add (dst holds no -0)
    dst = torch.randn(n, d, generator=g)
    dst[torch.rand(n, d, generator=g) < 0.2] = 0.0
    got = dst.to(dev)
    train._scatter(lib, ws, m, s, 0, U + I, got, engine.LGCN_SCATTER_ADD, None, None, stream)
    assert same(got.cpu(), dst + want)
    # a row range: only the item rows, rebased to a table of their own, without a mask
    items = torch.zeros(I, d, device=dev)
    train._scatter(lib, ws, m, s, U, U + I, items, engine.LGCN_SCATTER_STORE, None, None, stream)
    assert same(items.cpu(), want[U:U + I])

    assert lib.lgcn_rows_clear(engine._ptr(ws.i32[1]), m, 0, U + I, engine._ptr(ws.G), d, d,
                               engine._ptr(ws.mask), engine._ptr(ws.count), stream) == 0
    assert ws.G.count_nonzero().item() == 0
    assert bits(ws.G).count_nonzero().item() == 0
    assert ws.mask.count_nonzero().item() == 0 and ws.count.item() == 0


# ---- 3..7: whole steps against main.py's route --------------------------------------------------
def _adj(z, dev):
    U, I, B, d, K = case_dims(z)
    return graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                                z["ib_brand"], bool(z["use_brand"]), device=dev)


def _lightgcn(z, dev, scale=None):
    U, I, B, d, K = case_dims(z)
    torch.manual_seed(42)
    m = LightGCN(U, I, B, Cfg(d, K)).to(dev)
    if scale is not None:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(scale)
    return m


def _batch(z, dev, size, seed=11, items=None):
    U, I = case_dims(z)[:2]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, n, (size,), generator=g).to(dev)
                 for n in (U, items or I, items or I))


def _main_route(m, adj, bu, bp, bn):
    """main.py:495-522"""
    fu, fi, fb, u0, i0 = m(adj, use_brand=True)
    return bpr_loss_reg(fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], LAMBDA,
                        final_brand_emb=fb)


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters()}


def _assert_same_grads(got, want):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), k


def _workspace_of(adj):
    (ws,) = adj._lgcn_graph[1]._bpr_workspaces.values()
    return ws


def _assert_workspace_zero(adj):
    ws = _workspace_of(adj)
    assert not ws.dirty
    assert bits(ws.G).count_nonzero().item() == 0
    assert ws.mask.count_nonzero().item() == 0 and ws.count.item() == 0


def _compare_step(z, dev, size, factor=1, items=None, scale=None):
    batch = _batch(z, dev, size, items=items)
    a, b = _lightgcn(z, dev, scale), _lightgcn(z, dev, scale)
    want = _main_route(a, _adj(z, dev), *batch)   # a fresh adjacency per route
    (want if factor == 1 else factor * want).backward()
    adj = _adj(z, dev)
    got = b.bpr_step(adj, *batch, LAMBDA)
    (got if factor == 1 else factor * got).backward()
    assert same(got, want)
    _assert_same_grads(_grads(b), _grads(a))
    for k in ("user_embedding.weight", "item_embedding.weight"):
        assert _grads(b)[k].abs().max().item() > 0, k
    _assert_workspace_zero(adj)
    return batch


@pytest.mark.parametrize("name,size,items", [("c1_brand", 512, None), ("c1_nobrand", 256, None),
                                             ("hub_d32", 256, 64), ("micro_d12", 64, None),
                                             ("debug_c1_brand_k0", 256, None)])
def test_step_equals_main_route(gpu_device, name, size, items):
    _compare_step(load_case(name), gpu_device, size, items=items)


def test_step_equals_main_route_sided_backward(gpu_device, monkeypatch):
    monkeypatch.setenv("LGCN_SIDES_MIN_NNZ", "0")
    _compare_step(load_case("c1_brand"), gpu_device, 512)


def test_step_equals_main_route_scaled_loss(gpu_device):
    _compare_step(load_case("c1_brand"), gpu_device, 512, factor=2)


def test_two_steps_reuse_a_clean_workspace(gpu_device):
    z = load_case("c1_brand")
    dev = gpu_device
    a, b = _lightgcn(z, dev), _lightgcn(z, dev)
    adj_a, adj_b = _adj(z, dev), _adj(z, dev)
    for seed, size in ((11, 512), (12, 300)):
        batch = _batch(z, dev, size, seed=seed)
        for m in (a, b):
            m.zero_grad(set_to_none=True)
        want = _main_route(a, adj_a, *batch)
        want.backward()
        got = b.bpr_step(adj_b, *batch, LAMBDA)
        got.backward()
        assert same(got, want)
        _assert_same_grads(_grads(b), _grads(a))
        _assert_workspace_zero(adj_b)
    train.release_workspace(adj_b._lgcn_graph[1])
    assert not hasattr(adj_b._lgcn_graph[1], "_bpr_workspaces")


def test_a_step_that_raises_leaves_the_workspace_dirty_and_the_next_rezeroes_it(gpu_device,
                                                                               monkeypatch):
    z = load_case("c1_brand")
    dev = gpu_device
    a, b = _lightgcn(z, dev), _lightgcn(z, dev)
    adj_a, adj_b = _adj(z, dev), _adj(z, dev)

    def refuse(*args, **kw):
        raise engine.LgcnError("refused (test)")

    with monkeypatch.context() as mp:
        mp.setattr(engine, "propagate_backward", refuse)
        loss = b.bpr_step(adj_b, *_batch(z, dev, 256, seed=3), LAMBDA)
        with pytest.raises(engine.LgcnError):
            loss.backward()
    ws = _workspace_of(adj_b)
    assert ws.dirty and ws.G.count_nonzero().item() > 0   # scattered, never cleared
    b.zero_grad(set_to_none=True)
    batch = _batch(z, dev, 512, seed=4)
    want = _main_route(a, adj_a, *batch)
    want.backward()
    got = b.bpr_step(adj_b, *batch, LAMBDA)
    got.backward()
    assert same(got, want)
    _assert_same_grads(_grads(b), _grads(a))
    _assert_workspace_zero(adj_b)


def test_saturated_batch(gpu_device, monkeypatch):
    """Weights x 100: sigmoid saturates, the final-row gradients are +-0 — rows the scatter
    writes without marking them live. Gradients and the live-row count equal main.py's route."""
    dev = gpu_device
    counts = []
    real = engine.propagate_backward

    def recording(graph_, grad_out, *args, nz=None, **kw):
        segs = list(grad_out) if isinstance(grad_out, (list, tuple)) else [grad_out]
        segs = [t.contiguous() for t in segs]
        dense = engine.rows_nonzero(segs, segs[0].shape[1], dev)[1].item()
        counts.append((dense, None if nz is None else nz[1].item()))
        return real(graph_, grad_out, *args, nz=nz, **kw)

    monkeypatch.setattr(engine, "propagate_backward", recording)
    z = load_case("c1_brand")
    bu, bp, bn = _compare_step(z, dev, 512, scale=100.0)
    (main_dense, none), (step_dense, step_count) = counts
    assert none is None
    assert step_count == step_dense == main_dense
    # some touched rows stayed all +-0: their only samples saturated
    touched = bu.unique().numel() + torch.cat([bp, bn]).unique().numel()
    assert step_count < touched


def test_fusion_step_equals_main_route(gpu_device):
    z = load_case("c1_fusion")
    dev = gpu_device
    U, I, B, d, K = case_dims(z)
    content = z["content"]
    batch = _batch(z, dev, 256, seed=5)

    def model():
        torch.manual_seed(3)
        return LightGCN_Fusion(U, I, B, Cfg(d, K), pretrained_item_emb=content).to(dev)

    a, b = model(), model()
    fu, fi, fb, u0, i0 = a(_adj(z, dev))
    bu, bp, bn = batch
    want = bpr_loss_reg(fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], LAMBDA,
                        final_brand_emb=fb)
    want.backward()
    adj = _adj(z, dev)
    got = b.bpr_step(adj, *batch, LAMBDA)
    got.backward()
    assert same(got, want)
    ga, gb = _grads(a), _grads(b)
    assert len(ga) == 5
    _assert_same_grads(gb, ga)
    _assert_workspace_zero(adj)


def test_twelve_adam_steps_bit_equal(gpu_device):
    z = load_case("c1_brand")
    dev = gpu_device
    U, I = case_dims(z)[:2]

    def train_loop(fused):
        m = _lightgcn(z, dev)
        adj = _adj(z, dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        rng = np.random.default_rng(5)
        for _ in range(12):
            bu, bp, bn = (torch.from_numpy(rng.integers(0, n, 256)).to(dev) for n in (U, I, I))
            opt.zero_grad()
            loss = m.bpr_step(adj, bu, bp, bn, LAMBDA) if fused else \
                _main_route(m, adj, bu, bp, bn)
            loss.backward()
            opt.step()
        return m.state_dict()

    got, want = train_loop(True), train_loop(False)
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), k


def test_wrong_index_tensors_raise_before_any_launch(gpu_device):
    z = load_case("micro_d12")
    dev = gpu_device
    m, adj = _lightgcn(z, dev), _adj(z, dev)
    bu, bp, bn = _batch(z, dev, 8)
    with pytest.raises(engine.LgcnError):
        m.bpr_step(adj, bu.cpu(), bp, bn, LAMBDA)
    with pytest.raises(engine.LgcnError):
        m.bpr_step(adj, bu, bp.to(torch.int32), bn, LAMBDA)
    bad = bp.clone()
    bad[0] = case_dims(z)[1]
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu, bad, bn, LAMBDA, check_indices=True)
