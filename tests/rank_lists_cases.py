"""What the tests of the list rank evaluation (tests/test_rank_lists_api.py,
tests/test_gpu_rank_lists.py) share: the per-entry reference, the caller of the C ABI, the list
builders and the exact regular-graph model (not a test module)."""
import ctypes

import numpy as np
import torch

from conftest import Cfg
from eval_cases import POISON_RANK, POISON_SCORE, dev as _dev, rank_ref
from gcn_recommendation_amd import engine, graph

LIST_CAP = 32  # sorted places per slot one pass of the count kernel holds (include/lgcn.h)


def csr(lists):
    """(rowptr int32, items int64) of a list of lists, in the order given."""
    rowptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if len(lists) \
        else np.zeros(0, np.int64)
    return rowptr, items.astype(np.int64)


def expand(users, rowptr):
    """The slot and the user of every entry."""
    slot = np.repeat(np.arange(len(users)), np.diff(np.asarray(rowptr, dtype=np.int64)))
    return slot, np.asarray(users)[slot]


def lists_ref(full, rowptr, items):
    """rank_ref of every entry on its own: full holds one float64 masked score row per slot."""
    slot = expand(np.arange(full.shape[0]), rowptr)[0]
    items = np.asarray(items, dtype=np.int64)
    out = np.empty(len(items), np.int64)
    for s in range(0, len(items), 512):
        out[s:s + 512] = rank_ref(full[slot[s:s + 512]], items[s:s + 512])
    return out


def assert_lists(got, full, rowptr, items, what=""):
    """got: the kernel's (rank int32, target_score fp32) per entry; every rank must be rank_ref's
    and every score the fp32 of the float64 masked score (+0 for an exact zero), bitwise."""
    rank, score = got
    items = np.asarray(items, dtype=np.int64)
    assert rank.dtype == np.int32 and score.dtype == np.float32
    assert rank.shape == score.shape == items.shape
    want = lists_ref(full, rowptr, items)
    bad = np.nonzero(rank != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} ranks differ, first entry {bad[0]}: "
                           f"got {rank[bad[0]]}, want {want[bad[0]]}, target {items[bad[0]]}")
    inside = want >= 0
    assert np.isnan(score[~inside]).all(), what
    slot = expand(np.arange(full.shape[0]), rowptr)[0]
    want_s = full[slot[inside], items[inside]].astype(np.float32) + np.float32(0)
    assert np.array_equal(score[inside].view(np.uint32), want_s.view(np.uint32)), what
    return want


def score_rank_lists(device, ue, ie, users, rowptr, items, mrow, mit, n_splits, n_items=None,
                     window=None):
    """lgcn_score_rank_lists through the C ABI on device tensors ue / ie (row views allowed).
    rowptr and items are the whole set; window = (s, e) passes the slots [s, e) as users + s and
    target_rowptr + s with the same three base pointers. Every output and scratch element starts
    as a poison value. Returns host (rank int32, target_score fp32), one per entry of items."""
    lib = engine.load_library()
    d = ie.shape[1]
    assert ue.shape[1] == d and ue.stride(1) == 1 and ie.stride(1) == 1
    n_items = ie.shape[0] if n_items is None else n_items
    rowptr = np.asarray(rowptr, dtype=np.int32)
    assert len(rowptr) == len(users) + 1 and rowptr[-1] == len(items)
    s, e = window if window is not None else (0, len(users))
    n = e - s
    users_t = _dev(np.asarray(users, dtype=np.int32), device)
    rowptr_t = _dev(rowptr, device)
    items_t = _dev(np.asarray(items, dtype=np.int32), device) if len(items) else \
        torch.zeros(1, dtype=torch.int32, device=device)
    mrow_t = _dev(np.asarray(mrow, dtype=np.int32), device)
    mit_t = _dev(np.asarray(mit, dtype=np.int32), device) if len(mit) else \
        torch.zeros(1, dtype=torch.int32, device=device)
    n_win = int(rowptr[e] - rowptr[s])
    nbytes = lib.lgcn_score_rank_lists_scratch_bytes(n, n_win, n_splits)
    assert nbytes >= 4 * n + (12 + 4 * n_splits) * n_win and nbytes % 4 == 0
    scratch = torch.full((max(nbytes // 4, 1),), POISON_RANK, dtype=torch.int32, device=device)
    score = torch.full((max(len(items), 1),), POISON_SCORE, dtype=torch.float32, device=device)
    rank = torch.full((max(len(items), 1),), POISON_RANK, dtype=torch.int32, device=device)
    P = engine._ptr
    at = lambda t, k: ctypes.c_void_p(t.data_ptr() + 4 * k)  # noqa: E731
    with torch.cuda.device(device):
        rc = lib.lgcn_score_rank_lists(P(ue), ue.stride(0), at(users_t, s), n, P(ie), ie.stride(0),
                                       n_items, d, P(mrow_t), P(mit_t), at(rowptr_t, s),
                                       P(items_t), n_splits, P(scratch), nbytes, P(score), P(rank),
                                       engine._stream(device))
        assert rc == 0, rc
        torch.cuda.synchronize(device)
    if n:  # the ranked entries per slot: written for every slot, never more than the list holds
        cnt = scratch[:n].cpu().numpy()
        assert ((cnt >= 0) & (cnt <= np.diff(rowptr[s:e + 1]))).all()
    return rank.cpu().numpy()[:len(items)], score.cpu().numpy()[:len(items)]


def regular_graph():
    """192 users x 256 items x 64 brands, every node of degree 4 (a user 4 items, an item 3 users
    and 1 brand, a brand 4 items), no repeated edge: every entry of the normalised adjacency is
    1/4, so few-bit embeddings stay few-bit through the propagation."""
    rng = np.random.default_rng(81)
    U, I, B = 192, 256, 64
    passes = [rng.permutation(I) for _ in range(3)]
    tu = np.repeat(np.arange(U), 4)
    ti = np.concatenate(passes)  # user u: passes[u // 64][4 (u % 64) : +4], four distinct items
    ib_item = rng.permutation(I)
    ib_brand = np.arange(I) // 4
    return U, I, B, tu, ti, ib_item, ib_brand


def exact_model(dev, U, I, B, d, K, tu, ti, ib_item, ib_brand):
    """A LightGCN on `dev` over the regular graph with embeddings in multiples of 3/4 (the mean
    over K + 1 = 3 layers then divides exactly), and its propagated tables as numpy: multiples of
    1/64 up to 1.5, the same numbers from the CPU's torch.sparse.mm and from the engine."""
    from models.lightgcn import LightGCN
    assert K == 2
    rng = np.random.default_rng(82)
    host = LightGCN(U, I, B, Cfg(d, K))
    with torch.no_grad():
        for w, n in ((host.user_embedding.weight, U), (host.item_embedding.weight, I),
                     (host.brand_embedding.weight, B)):
            w.copy_(torch.from_numpy(rng.integers(-2, 3, (n, d)).astype(np.float32) * 0.75))
        adj_host = graph.build_norm_adj(tu, ti, U, I, B, ib_item, ib_brand, True)
        assert np.array_equal(np.unique(adj_host.coalesce().values().numpy()), [0.25])
        fu, fi = (t.numpy() for t in host(adj_host)[:2])
    assert np.array_equal(fu * 64, np.round(fu * 64)) and np.array_equal(fi * 64, np.round(fi * 64))
    assert np.abs(fu).max() <= 1.5 and np.abs(fi).max() <= 1.5
    if torch.device(dev).type == "cpu":
        return host, adj_host, fu, fi
    model = LightGCN(U, I, B, Cfg(d, K))
    model.load_state_dict(host.state_dict())
    model = model.to(dev)
    adj = graph.build_norm_adj(tu, ti, U, I, B, ib_item, ib_brand, True, device=dev)
    with torch.no_grad():
        gu, gi = model(adj)[:2]
    assert np.array_equal(gu.cpu().numpy(), fu) and np.array_equal(gi.cpu().numpy(), fi)
    return model, adj, fu, fi


def held_out_frame(rng, fu, fi, mrow, mit, U, I):
    """(users, items) rows of a held-out frame over the exact model: 1-6 items per user for 170
    users, every other one among the user's first 20 places, a few users once more further down
    the frame (with a repeated row among them)."""
    from util import masked_scores64, topk_total_order
    us = rng.permutation(U)[:170]
    first = topk_total_order(masked_scores64(fu, fi, us, mrow, mit), 20)[1]
    vu, vi = [], []
    for b, u in enumerate(us):
        for j in range(1 + b % 6):
            vu.append(u)
            vi.append(first[b, (b + 3 * j) % 20] if j % 2 == 0 else rng.integers(0, I))
    vu += [us[5], us[9], us[5]]
    vi += [int(rng.integers(0, I)), int(rng.integers(0, I)), vi[0]]
    return np.asarray(vu, dtype=np.int64), np.asarray(vi, dtype=np.int64)
