"""The fused BPR training step (gcn_recommendation_amd.train) without a GPU: the new C symbols
validate their arguments on the host, and `bpr_step` on a CPU adjacency runs the reference's own
expression — loss and every gradient bitwise those of the hand-written route (main.py:495-525)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Cfg, case_dims, load_case
from gcn_recommendation_amd import _build, engine, graph, train
from gcn_recommendation_amd.loss import bpr_loss_reg
from models.lightgcn import LightGCN


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


def test_new_symbols_validate_arguments_without_gpu(lib):
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host
    f = ctypes.c_float(1e-4)

    def loss(fu=p, ld_fu=64, fi=p, ld_fi=64, u0=p, ld_u0=64, i0=p, ld_i0=64, users=p, pos=p,
             neg=p, B=4, d=64, terms=p, out=p, grads=p):
        return lib.lgcn_bpr_loss_indexed(fu, ld_fu, fi, ld_fi, u0, ld_u0, i0, ld_i0, 10, 10, users,
                                         pos, neg, B, d, f, terms, out, grads, None)

    for bad in (dict(fu=None), dict(fi=None), dict(u0=None), dict(i0=None), dict(users=None),
                dict(pos=None), dict(neg=None), dict(terms=None), dict(out=None),
                dict(grads=None), dict(B=0), dict(d=0), dict(ld_fu=63), dict(ld_fi=63),
                dict(ld_u0=63), dict(ld_i0=63)):
        assert loss(**bad) == -1, bad
    assert lib.lgcn_bpr_keys(None, p, p, 4, 10, 10, p, None) == -1
    assert lib.lgcn_bpr_keys(p, p, p, 4, 10, 10, None, None) == -1
    assert lib.lgcn_bpr_keys(p, p, p, 0, 10, 10, p, None) == -1
    assert lib.lgcn_bpr_keys(p, p, p, 4, 1 << 30, 10, p, None) == -1  # keys past int32

    def scatter(keys=p, perm=p, n=8, src=p, ld_src=64, lo=0, hi=10, dst=p, ld_dst=64, d=64,
                mode=engine.LGCN_SCATTER_STORE, mask=None, count=None):
        return lib.lgcn_rows_scatter(keys, perm, n, src, ld_src, lo, hi, dst, ld_dst, d, mode,
                                     mask, count, None)

    for bad in (dict(keys=None), dict(perm=None), dict(src=None), dict(dst=None), dict(n=-1),
                dict(d=0), dict(ld_src=63), dict(ld_dst=63), dict(lo=-1), dict(lo=5, hi=4),
                dict(mode=2), dict(count=p), dict(mode=engine.LGCN_SCATTER_ADD, mask=p)):
        assert scatter(**bad) == -1, bad
    assert scatter(n=0, keys=None, perm=None, src=None, dst=None) == 0  # nothing to do
    assert lib.lgcn_rows_clear(None, 8, 0, 10, p, 64, 64, None, None, None) == -1
    assert lib.lgcn_rows_clear(p, 8, 0, 10, None, 64, 64, None, None, None) == -1
    assert lib.lgcn_rows_clear(p, -1, 0, 10, p, 64, 64, None, None, None) == -1
    assert lib.lgcn_rows_clear(p, 8, 0, 10, p, 63, 64, None, None, None) == -1
    assert lib.lgcn_rows_clear(p, 8, 0, 10, p, 64, 0, None, None, None) == -1
    assert lib.lgcn_rows_clear(None, 0, 0, 10, None, 64, 64, None, None, None) == 0


def _setup(name="c1_brand", batch=256):
    # batch x d stays under ATen's 32768-element grain: above it the CPU index_put_ of
    # IndexBackward adds with atomics from several threads, and the hand-written route itself is
    # no longer reproducible run to run
    z = load_case(name)
    U, I, B, d, K = case_dims(z)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]))
    g = torch.Generator().manual_seed(11)
    idx = tuple(torch.randint(0, n, (batch,), generator=g) for n in (U, I, I))
    return z, adj, idx


def _model(z):
    U, I, B, d, K = case_dims(z)
    torch.manual_seed(42)
    return LightGCN(U, I, B, Cfg(d, K))


def test_cpu_bpr_step_is_the_hand_written_route_bitwise():
    z, adj, (bu, bp, bn) = _setup()
    a, b = _model(z), _model(z)
    fu, fi, fb, u0, i0 = a(adj, use_brand=True)
    want = bpr_loss_reg(fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], 1e-4, final_brand_emb=fb)
    want.backward()
    got = b.bpr_step(adj, bu, bp, bn, 1e-4)
    got.backward()
    assert torch.equal(got.detach().view(torch.int32), want.detach().view(torch.int32))
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert set(ga) == set(gb) and len(ga) == 3
    for k in ga:
        assert ga[k].grad is not None and gb[k].grad is not None, k
        assert torch.equal(gb[k].grad.view(torch.int32), ga[k].grad.view(torch.int32)), k
    # the module-level entry point is the same call
    c = _model(z)
    again = train.bpr_step(c, adj, bu, bp, bn, 1e-4, check_indices=True)
    assert torch.equal(again.detach().view(torch.int32), want.detach().view(torch.int32))


def test_check_indices_and_index_tensor_validation():
    z, adj, (bu, bp, bn) = _setup(batch=16)
    U, I = case_dims(z)[:2]
    m = _model(z)
    for which, n in ((0, U), (1, I), (2, I)):
        for v in (n, -1):
            idx = [bu.clone(), bp.clone(), bn.clone()]
            idx[which][3] = v
            with pytest.raises(engine.LgcnError):
                train.bpr_step(m, adj, *idx, 1e-4, check_indices=True)
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu.to(torch.int32), bp, bn, 1e-4, check_indices=True)
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu, bp.to(torch.int32), bn, 1e-4)
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu.view(4, 4), bp, bn, 1e-4)
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu, bp[:8], bn, 1e-4)
    assert np.isfinite(train.bpr_step(m, adj, bu, bp, bn, 1e-4, check_indices=True).item())


def test_release_workspace_without_any():
    train.release_workspace()
