"""Recall@K / NDCG@K on device (the semantics of main.py:404-439).

Scores = user rows · item tableᵀ (hipBLASLt via torch.matmul), every training item of the user
masked to -1e10 (main.py:422-424), topk(K) (main.py:426), hit -> recall 1, NDCG 1/log2(pos+2)
(main.py:430-438). The training items come straight from the engine's CSR (a user's row holds its
items at column offset U), so no Python loop over users is needed.
"""
import ctypes

import numpy as np
import torch

from . import engine


def recall_ndcg(user_emb, item_emb, users, heldout_items, train_rowptr, train_cols, U, k=20,
                batch_size=1024, return_topk=False):
    """users: int64 [n] user ids; heldout_items: int64 [n] item ids (one per user);
    train_rowptr/train_cols: host CSR of Â (numpy) — a user row's cols >= U are its items."""
    dev = user_emb.device
    users = np.asarray(users, dtype=np.int64)
    heldout_items = np.asarray(heldout_items, dtype=np.int64)
    hits, ndcgs, tops = [], [], []
    with torch.no_grad():
        for s in range(0, len(users), batch_size):
            bu = users[s:s + batch_size]
            scores = torch.matmul(user_emb[torch.from_numpy(bu).to(dev)], item_emb.T)
            lens = train_rowptr[bu + 1] - train_rowptr[bu]
            rr = np.repeat(np.arange(len(bu)), lens)
            cc = np.concatenate([train_cols[train_rowptr[u]:train_rowptr[u + 1]] for u in bu]) \
                if lens.sum() else np.zeros(0, np.int64)
            keep = cc >= U
            if keep.any():
                scores[torch.from_numpy(rr[keep]).to(dev),
                       torch.from_numpy(cc[keep] - U).to(dev)] = -1e10
            _, top = torch.topk(scores, k=k)
            top = top.cpu().numpy()
            if return_topk:
                tops.append(top)
            truth = heldout_items[s:s + batch_size]
            for j in range(len(bu)):
                pos = np.nonzero(top[j] == truth[j])[0]
                hits.append(1 if pos.size else 0)
                ndcgs.append(1 / np.log2(pos[0] + 2) if pos.size else 0)
    if return_topk:
        return float(np.mean(hits)), float(np.mean(ndcgs)), np.concatenate(tops)
    return float(np.mean(hits)), float(np.mean(ndcgs))


# ----------------------------------------------------------------------------------------------
# fused path: lgcn_score_topk (score GEMM + train mask + top-K in one kernel, no score matrix)
# ----------------------------------------------------------------------------------------------
def mask_csr(users, items, n_users):
    """Sorted, de-duplicated per-user item lists (the train_user_items dict of main.py:407)."""
    users = np.asarray(users, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    key = np.unique(users * (items.max(initial=0) + 1) + items) if users.size else users
    if users.size:
        span = items.max(initial=0) + 1
        u, it = key // span, key % span
    else:
        u, it = users, items
    rowptr = np.searchsorted(u, np.arange(n_users + 1)).astype(np.int32)
    return rowptr, it.astype(np.int32)


def _items_to_pass(mask_items):
    """mask_items, or one int32 zero when every list is empty: the kernels want a pointer."""
    if mask_items.numel():
        return mask_items
    return torch.zeros(1, dtype=torch.int32, device=mask_items.device)


def topk_fused(user_emb, item_emb, users, mask_rowptr, mask_items, k=20):
    """Top-k items per user (scores, indices) with the train items masked to -1e10.
    user_emb [U x d], item_emb [I x d] fp32 on the HIP device; users: int32/int64 ids."""
    lib = engine.load_library()
    dev = item_emb.device
    d = item_emb.shape[1]
    users = torch.as_tensor(users, device=dev).to(torch.int32).contiguous()
    n = int(users.numel())
    ue, ie = user_emb.contiguous(), item_emb.contiguous()
    mrow = torch.as_tensor(mask_rowptr, device=dev).to(torch.int32).contiguous()
    mit = _items_to_pass(torch.as_tensor(mask_items, device=dev).to(torch.int32).contiguous())
    splits = lib.lgcn_eval_splits(n, int(ie.shape[0]), _device_cus(dev))
    part_s = torch.empty((splits, max(n, 1), k), dtype=torch.float32, device=dev)
    part_i = torch.empty((splits, max(n, 1), k), dtype=torch.int32, device=dev)
    top_s = torch.empty((max(n, 1), k), dtype=torch.float32, device=dev)
    top_i = torch.empty((max(n, 1), k), dtype=torch.int32, device=dev)
    P = engine._ptr
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_score_topk(P(ue), ue.stride(0), P(users), n, P(ie), ie.stride(0),
                                          int(ie.shape[0]), d, P(mrow), P(mit), k, splits,
                                          P(part_s), P(part_i), P(top_s), P(top_i),
                                          engine._stream(dev)), "lgcn_score_topk")
    return top_s[:n], top_i[:n]


FUSED_DIMS = (32, 64, 128, 256)   # lgcn_score_topk's widths (include/lgcn.h)
FUSED_MAX_K = 32


def fused_supported(d, k):
    return d in FUSED_DIMS and 1 <= k <= FUSED_MAX_K


def topk_torch(user_emb, item_emb, users, mask_rowptr, mask_items, k=20):
    """main.py:420-426 as torch ops for any d and k: scores = user rows · item tableᵀ, every
    training item of the user set to -1e10, topk(k)."""
    dev = item_emb.device
    users = np.asarray(users, dtype=np.int64)
    scores = torch.matmul(user_emb[torch.from_numpy(users).to(dev)], item_emb.T)
    lens = mask_rowptr[users + 1] - mask_rowptr[users]
    if lens.sum():
        rr = np.repeat(np.arange(len(users)), lens)
        cc = np.concatenate([mask_items[mask_rowptr[u]:mask_rowptr[u + 1]] for u in users])
        scores[torch.from_numpy(rr).to(dev), torch.from_numpy(cc.astype(np.int64)).to(dev)] = -1e10
    return torch.topk(scores, k=k)


def evaluate(model, val_or_test_data, train_data, norm_adj_tensor, k, device, batch_size=8192,
             use_brand=True, item_brand_df=None):
    """main.py:404-439 (same signature and metrics): one propagation, then per batch of users
    one lgcn_score_topk launch (fused score + mask + top-k) when the width and k are ones the
    kernel has (d in FUSED_DIMS, k <= FUSED_MAX_K), torch matmul + mask + topk otherwise — the
    reference works for any d and k, so does this; hit -> recall 1, NDCG = 1/log2(pos + 2)."""
    model.eval()
    test_user_items = dict(zip(val_or_test_data["user_idx"], val_or_test_data["item_idx"]))
    test_users = np.fromiter(test_user_items.keys(), dtype=np.int64, count=len(test_user_items))
    truth = np.fromiter(test_user_items.values(), dtype=np.int64, count=len(test_user_items))
    with torch.no_grad():
        all_user_emb, all_item_emb, _, _, _ = model(norm_adj_tensor)
        mrow, mit = mask_csr(train_data["user_idx"].to_numpy(), train_data["item_idx"].to_numpy(),
                             all_user_emb.shape[0])
        fused = fused_supported(all_item_emb.shape[1], k) and all_item_emb.is_cuda
        tops = []
        for s in range(0, len(test_users), batch_size):
            bu = test_users[s:s + batch_size]
            if fused:
                _, ti = topk_fused(all_user_emb, all_item_emb, bu, mrow, mit, k)
            else:
                _, ti = topk_torch(all_user_emb, all_item_emb, bu, mrow, mit, k)
            tops.append(ti.cpu().numpy())
    top = np.concatenate(tops) if tops else np.zeros((0, k), np.int32)
    hit = top == truth[:, None]
    found = hit.any(1)
    pos = hit.argmax(1)
    ndcg = np.where(found, 1.0 / np.log2(pos + 2), 0.0)
    return float(found.mean()) if len(found) else float("nan"), \
        float(ndcg.mean()) if len(found) else float("nan")


# ----------------------------------------------------------------------------------------------
# rank path: lgcn_score_rank (the held-out item's exact rank; no top-k, any k, every k at once)
# ----------------------------------------------------------------------------------------------
# The reference evaluates leave-one-out (one held-out item per user, main.py:406), so Recall@k and
# NDCG@k are functions of one integer per user: the 0-based rank of the held-out item among all
# items under include/lgcn.h's total order (score descending, item index ascending, the user's
# train items at -1e10). Recall@k = (rank < k), NDCG@k = 1 / log2(rank + 2) when rank < k.
_n_cu = {}


def _device_cus(dev):
    idx = dev.index or 0
    if idx not in _n_cu:
        n_cu = ctypes.c_int32(0)
        engine._check(engine.load_library().lgcn_device_info(idx, ctypes.byref(n_cu), None),
                      "device_info")
        _n_cu[idx] = n_cu.value
    return _n_cu[idx]


def _check_tables(user_emb, item_emb):
    for name, t in (("user_emb", user_emb), ("item_emb", item_emb)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise engine.LgcnError(f"rank: {name} must be a 2-D float32 tensor")
    if user_emb.device != item_emb.device or user_emb.shape[1] != item_emb.shape[1]:
        raise engine.LgcnError("rank: user_emb and item_emb must share a device and a width")


def _index_tensor(name, a, dev):
    """users / targets as a 1-D integer tensor on dev: a tensor must already be there (nothing is
    moved silently), anything else is uploaded once."""
    if torch.is_tensor(a):
        if a.device != dev:
            raise engine.LgcnError(f"rank: {name} on {a.device}, tables on {dev}")
        if a.dtype not in (torch.int32, torch.int64):
            raise engine.LgcnError(f"rank: {name} must be int32 or int64, not {a.dtype}")
    else:
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu":
            raise engine.LgcnError(f"rank: {name} must be integers, not {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    if a.dim() != 1:
        raise ValueError(f"rank: {name} must be 1-D")
    return a


def _mask_tensor(name, a, dev):
    """A mask CSR array as a contiguous int32 tensor on dev: a device tensor is used as it is (no
    upload, no copy), numpy is uploaded."""
    if torch.is_tensor(a):
        if a.device != dev or a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous():
            raise engine.LgcnError(f"rank: {name} must be a contiguous 1-D int32 tensor on {dev}")
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _slots(users, targets, n_table, n_items, dev):
    """(users int32, targets int32) for the kernel: a target outside [0, n_items) becomes -1 (the
    kernel's 'no target'), and so does the target of a user outside the table, whose id becomes 0:
    such a slot ranks -1 and nothing of it is dereferenced. Device ops only."""
    users = _index_tensor("users", users, dev)
    targets = _index_tensor("targets", targets, dev)
    if users.shape != targets.shape:
        raise ValueError(f"rank: {users.numel()} users but {targets.numel()} targets")
    bad_u = (users < 0) | (users >= n_table)
    bad_t = bad_u | (targets < 0) | (targets >= n_items)
    users = torch.where(bad_u, torch.zeros_like(users), users).to(torch.int32)
    targets = torch.where(bad_t, torch.full_like(targets, -1), targets).to(torch.int32)
    return users.contiguous(), targets.contiguous()


def _rows(t):
    return t if t.stride(1) == 1 or t.shape[0] == 0 else t.contiguous()


def _rank_launch(ue, ie, users, targets, mrow, mit, rank, score, part, n_splits):
    """One lgcn_score_rank on prepared device tensors (int32 users / targets / outputs of one
    length n > 0, part >= n_splits * n int32), on the current stream."""
    lib = engine.load_library()
    dev = ie.device
    P = engine._ptr
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_score_rank(P(ue), ue.stride(0), P(users), int(users.numel()), P(ie),
                                          ie.stride(0), int(ie.shape[0]), int(ie.shape[1]), P(mrow),
                                          P(mit), P(targets), n_splits, P(part), P(score), P(rank),
                                          engine._stream(dev)), "lgcn_score_rank")


def rank_fused(user_emb, item_emb, users, targets, mask_rowptr, mask_items):
    """(ranks int32 [n], target_scores fp32 [n]) on the tables' HIP device: lgcn_score_rank for
    batch slot b = (users[b], targets[b]). mask_rowptr / mask_items that are already int32 tensors
    on the device are passed as they are; numpy arrays are uploaded. A width the kernel does not
    have is an error (rank_torch takes any)."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    if dev.type != "cuda":
        raise engine.LgcnError("rank_fused needs tables on a HIP device (rank_torch runs anywhere)")
    if item_emb.shape[1] not in FUSED_DIMS:
        raise engine.LgcnError(f"rank_fused: d = {item_emb.shape[1]} not in {FUSED_DIMS}")
    mrow = _mask_tensor("mask_rowptr", mask_rowptr, dev)
    mit = _mask_tensor("mask_items", mask_items, dev)
    if mrow.numel() != user_emb.shape[0] + 1:
        raise ValueError("rank: mask_rowptr must hold one entry per user row and one more")
    users, targets = _slots(users, targets, user_emb.shape[0], item_emb.shape[0], dev)
    n = int(users.numel())
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return rank, score
    splits = engine.load_library().lgcn_eval_splits(n, int(item_emb.shape[0]), _device_cus(dev))
    part = torch.empty(splits * n, dtype=torch.int32, device=dev)
    _rank_launch(_rows(user_emb), _rows(item_emb), users, targets, mrow, _items_to_pass(mit), rank,
                 score, part, splits)
    return rank, score


def rank_torch(user_emb, item_emb, users, targets, mask_rowptr, mask_items, batch_size=1024):
    """rank_fused's result with torch ops, for any width and device (CPU included): scores by
    matmul (main.py:420), the user's train items filled with -1e10 (main.py:422-424), then the
    count of items ahead of the target under the total order. Its scores are matmul's, so on
    rounded inputs a rank may differ from the kernel's where two scores meet in the last bit."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    n_table, n_items = user_emb.shape[0], item_emb.shape[0]
    mrow = _mask_tensor("mask_rowptr", mask_rowptr, dev).long()
    mit = _mask_tensor("mask_items", mask_items, dev).long()
    if mrow.numel() != n_table + 1:
        raise ValueError("rank: mask_rowptr must hold one entry per user row and one more")
    users, targets = _slots(users, targets, n_table, n_items, dev)
    users, targets = users.long(), targets.long()
    n = int(users.numel())
    rank = torch.full((n,), -1, dtype=torch.int32, device=dev)
    score = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    if n == 0 or n_items == 0:
        return rank, score
    item = torch.arange(n_items, device=dev)
    for s in range(0, n, batch_size):
        u, t = users[s:s + batch_size], targets[s:s + batch_size]
        scores = torch.matmul(user_emb[u], item_emb.T)
        lens = mrow[u + 1] - mrow[u]
        total = int(lens.sum())
        if total:
            rr = torch.repeat_interleave(torch.arange(len(u), device=dev), lens)
            first = torch.cumsum(lens, 0) - lens
            pos = torch.arange(total, device=dev) - first[rr] + mrow[u][rr]
            scores[rr, mit[pos]] = -1e10
        ok = t >= 0
        tc = t.clamp(min=0)[:, None]
        ts = scores.gather(1, tc)
        ahead = (scores > ts) | ((scores == ts) & (item[None, :] < tc))
        rank[s:s + batch_size] = torch.where(ok, ahead.sum(1), torch.full_like(t, -1)).int()
        score[s:s + batch_size] = torch.where(ok, ts[:, 0], torch.full_like(ts[:, 0], float("nan")))
    return rank, score


def metrics_from_ranks(ranks, ks=(20,)):
    """{'recall@k', 'ndcg@k' for k in ks, 'mrr'} from 0-based ranks (a tensor or an array; -1 = no
    rank, a miss everywhere): the float64 numpy expressions of evaluate(), whose list position of
    a hit is the rank. Empty input gives NaN, as evaluate() does."""
    if torch.is_tensor(ranks):
        ranks = ranks.detach().cpu().numpy()
    r = np.asarray(ranks).astype(np.int64).reshape(-1)
    out = {}
    for k in ks:
        k = int(k)
        found = (r >= 0) & (r < k)
        pos = np.where(found, r, 0)
        ndcg = np.where(found, 1.0 / np.log2(pos + 2), 0.0)
        out[f"recall@{k}"] = float(found.mean()) if len(found) else float("nan")
        out[f"ndcg@{k}"] = float(ndcg.mean()) if len(found) else float("nan")
    ranked = r >= 0
    rr = np.where(ranked, 1.0 / (np.where(ranked, r, 0) + 1), 0.0)
    out["mrr"] = float(rr.mean()) if len(r) else float("nan")
    return out


# ----------------------------------------------------------------------------------------------
# list path: lgcn_score_rank_lists (several held-out items per user, one pass over the score row)
# ----------------------------------------------------------------------------------------------
# The usual LightGCN splits hold out many items per user. Every entry's rank is what
# lgcn_score_rank gives for the pair on its own (the other held-out items of the user count as
# ordinary items), so the list metrics are functions of the ranks and the lists' lengths.
def target_csr(users, items):
    """(eval_users int64 [n], rowptr int32 [n + 1], items int32 [rowptr[-1]]) as numpy: the
    distinct users that occur, ascending, each with its de-duplicated, sorted item list. Every
    row of the frame is kept (evaluate()'s dict(zip(...)) keeps a user's last). An item that no
    int32 holds becomes -1: there is no such item, it ranks -1."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    items = np.asarray(items, dtype=np.int64).reshape(-1)
    if users.shape != items.shape:
        raise ValueError(f"target_csr: {users.size} users but {items.size} items")
    if users.size == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int32), np.zeros(0, np.int32)
    if users.size >= 1 << 31:
        raise ValueError("target_csr: the pair count must be below 2^31")
    pairs = np.unique(np.stack([users, items], 1), axis=0)  # sorted by (user, item), distinct
    eval_users, counts = np.unique(pairs[:, 0], return_counts=True)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    it = pairs[:, 1]
    it = np.where((it < 0) | (it >= 1 << 31), -1, it).astype(np.int32)
    return eval_users, rowptr, it


def _list_slots(users, rowptr, items, n_table, n_items, dev):
    """(users int32, rowptr int32, items int32) for the kernel, as _slots gives them for pairs: a
    target outside [0, n_items) becomes -1, and so does every target of a user outside the table,
    whose id becomes 0. Device ops only, no read-back."""
    users = _index_tensor("users", users, dev)
    rowptr = _index_tensor("target_rowptr", rowptr, dev)
    items = _index_tensor("target_items", items, dev)
    if rowptr.numel() != users.numel() + 1:
        raise ValueError(f"rank lists: {users.numel()} users need {users.numel() + 1} offsets, "
                         f"not {rowptr.numel()}")
    bad_u = (users < 0) | (users >= n_table)
    bad_t = (items < 0) | (items >= n_items)
    if users.numel() and items.numel():
        entry = torch.arange(items.numel(), device=dev, dtype=rowptr.dtype)
        slot = (torch.searchsorted(rowptr, entry, right=True) - 1).clamp_(0, users.numel() - 1)
        bad_t = bad_t | bad_u[slot]
    users = torch.where(bad_u, torch.zeros_like(users), users).to(torch.int32)
    items = torch.where(bad_t, torch.full_like(items, -1), items).to(torch.int32)
    return users.contiguous(), rowptr.to(torch.int32).contiguous(), items.contiguous()


def _rank_lists_launch(ue, ie, users, rowptr, items, mrow, mit, rank, score, scratch, n_splits):
    """One lgcn_score_rank_lists on prepared device tensors: int32 users [n > 0], rowptr (a view
    of n + 1 offsets into items / rank / score, which are passed whole) and a uint8 scratch, on
    the current stream."""
    lib = engine.load_library()
    dev = ie.device
    P = engine._ptr
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_score_rank_lists(
            P(ue), ue.stride(0), P(users), int(users.numel()), P(ie), ie.stride(0),
            int(ie.shape[0]), int(ie.shape[1]), P(mrow), P(mit), P(rowptr), P(items), n_splits,
            P(scratch), int(scratch.numel()), P(score), P(rank), engine._stream(dev)),
            "lgcn_score_rank_lists")


def _lists_scratch(n_slots, n_targets, n_splits, dev):
    nbytes = engine.load_library().lgcn_score_rank_lists_scratch_bytes(n_slots, n_targets,
                                                                       n_splits)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def rank_lists_fused(user_emb, item_emb, users, target_rowptr, target_items, mask_rowptr,
                     mask_items):
    """(ranks int32 [n_targets], target_scores fp32 [n_targets]) on the tables' HIP device:
    lgcn_score_rank_lists. Slot b is users[b] with the entries target_rowptr[b]:target_rowptr[b+1]
    of target_items; every entry gets what rank_fused gives the pair on its own. Entries that
    belong to no slot keep rank -1 and a NaN score. The argument rules are rank_fused's."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    if dev.type != "cuda":
        raise engine.LgcnError("rank_lists_fused needs tables on a HIP device (rank_lists_torch "
                               "runs anywhere)")
    if item_emb.shape[1] not in FUSED_DIMS:
        raise engine.LgcnError(f"rank_lists_fused: d = {item_emb.shape[1]} not in {FUSED_DIMS}")
    mrow = _mask_tensor("mask_rowptr", mask_rowptr, dev)
    mit = _mask_tensor("mask_items", mask_items, dev)
    if mrow.numel() != user_emb.shape[0] + 1:
        raise ValueError("rank: mask_rowptr must hold one entry per user row and one more")
    users, rowptr, items = _list_slots(users, target_rowptr, target_items, user_emb.shape[0],
                                       item_emb.shape[0], dev)
    n, n_targets = int(users.numel()), int(items.numel())
    rank = torch.full((n_targets,), -1, dtype=torch.int32, device=dev)
    score = torch.full((n_targets,), float("nan"), dtype=torch.float32, device=dev)
    if n == 0 or n_targets == 0:
        return rank, score
    splits = engine.load_library().lgcn_eval_splits(n, int(item_emb.shape[0]), _device_cus(dev))
    _rank_lists_launch(_rows(user_emb), _rows(item_emb), users, rowptr, items, mrow,
                       _items_to_pass(mit), rank, score, _lists_scratch(n, n_targets, splits, dev),
                       splits)
    return rank, score


def rank_lists_torch(user_emb, item_emb, users, target_rowptr, target_items, mask_rowptr,
                     mask_items, batch_size=1024):
    """rank_lists_fused's result with torch ops, for any width and device (CPU included):
    rank_torch on the (user, item) pairs the lists expand to. The offsets are read on the host."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    users = _index_tensor("users", users, dev)
    items = _index_tensor("target_items", target_items, dev)
    rowptr = target_rowptr.detach().cpu().numpy() if torch.is_tensor(target_rowptr) \
        else np.asarray(target_rowptr)
    if rowptr.ndim != 1 or (rowptr.size and rowptr.dtype.kind not in "iu"):
        raise engine.LgcnError("rank lists: target_rowptr must be 1-D integers")
    rowptr = rowptr.astype(np.int64)
    if rowptr.size != users.numel() + 1:
        raise ValueError(f"rank lists: {users.numel()} users need {users.numel() + 1} offsets, "
                         f"not {rowptr.size}")
    lo, hi = int(rowptr[0]), int(rowptr[-1])
    if (np.diff(rowptr) < 0).any() or lo < 0 or hi > items.numel():
        raise ValueError("rank lists: target_rowptr must ascend inside target_items")
    n_targets = int(items.numel())
    rank = torch.full((n_targets,), -1, dtype=torch.int32, device=dev)
    score = torch.full((n_targets,), float("nan"), dtype=torch.float32, device=dev)
    lens = torch.from_numpy(np.diff(rowptr)).to(dev)
    pair_users = torch.repeat_interleave(users, lens, output_size=hi - lo)
    rank[lo:hi], score[lo:hi] = rank_torch(user_emb, item_emb, pair_users, items[lo:hi],
                                           mask_rowptr, mask_items, batch_size)
    return rank, score


def metrics_from_rank_lists(ranks, rowptr, ks=(20,)):
    """{'recall@k', 'precision@k', 'hit@k', 'ndcg@k' for k in ks, 'mrr'} from the 0-based ranks of
    every held-out entry (a tensor or an array; -1 = no rank: a miss that still counts in its
    user's list length) and the lists' offsets into them, each a mean over the users with a
    non-empty list. With hits_k(u) the user's entries ranked below k and n_u its list length:
    recall hits_k / n_u, precision hits_k / k, hit hits_k > 0, NDCG the DCG of the hits over the
    DCG of min(k, n_u) hits at the first places, MRR 1 / (best rank + 1). With one entry per user
    recall, NDCG and MRR are metrics_from_ranks' numbers to the bit. Empty input gives NaN."""
    if torch.is_tensor(ranks):
        ranks = ranks.detach().cpu().numpy()
    if torch.is_tensor(rowptr):
        rowptr = rowptr.detach().cpu().numpy()
    rp = np.asarray(rowptr).astype(np.int64).reshape(-1)
    r = np.asarray(ranks).astype(np.int64).reshape(-1)
    lens = np.diff(rp) if rp.size else np.zeros(0, np.int64)
    keep = lens > 0
    n_u = lens[keep]
    nu = int(n_u.size)
    r = r[rp[0]:rp[-1]] if rp.size else r[:0]
    seg = np.repeat(np.arange(nu), n_u)  # the entries' user among those with a list
    nan = float("nan")
    out = {}
    for k in ks:
        k = int(k)
        found = (r >= 0) & (r < k)
        pos = np.where(found, r, 0)
        hits = np.bincount(seg, weights=found, minlength=nu)
        dcg = np.bincount(seg, weights=np.where(found, 1.0 / np.log2(pos + 2), 0.0), minlength=nu)
        top = int(min(k, n_u.max(initial=0)))
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(top) + 2))])
        out[f"recall@{k}"] = float((hits / n_u).mean()) if nu else nan
        out[f"precision@{k}"] = float((hits / k).mean()) if nu else nan
        out[f"hit@{k}"] = float((hits > 0).mean()) if nu else nan
        out[f"ndcg@{k}"] = float((dcg / ideal[np.minimum(k, n_u)]).mean()) if nu else nan
    if nu:
        big = np.iinfo(np.int64).max
        best = np.minimum.reduceat(np.where(r >= 0, r, big), (np.cumsum(n_u) - n_u))
        ranked = best < big
        rr = np.where(ranked, 1.0 / (np.where(ranked, best, 0) + 1), 0.0)
    out["mrr"] = float(rr.mean()) if nu else nan
    return out


# ----------------------------------------------------------------------------------------------
# recommendation lists: lgcn_score_topk_wide (the first k items per user for k up to 1024)
# ----------------------------------------------------------------------------------------------
# The lists are the ones the rank kernels describe: entry j of a user's list is the item whose
# lgcn_score_rank rank is j (score descending, item index ascending, the user's mask items at
# -1e10), positions past the listable items hold -inf / -1.
WIDE_MAX_K = 1024                 # LGCN_TOPK_WIDE_MAX_K (include/lgcn.h)


def wide_supported(d, k):
    return d in FUSED_DIMS and 1 <= k <= WIDE_MAX_K


def _user_ids(name, users, n_table):
    """users as a host int64 array, every id inside [0, n_table) (ValueError otherwise): the
    kernels read the rows they are given."""
    if torch.is_tensor(users):
        users = users.detach().cpu().numpy()
    users = np.asarray(users)
    if users.ndim != 1:
        raise ValueError(f"{name}: users must be 1-D")
    if users.size and users.dtype.kind not in "iu":
        raise engine.LgcnError(f"{name}: users must be integers, not {users.dtype}")
    users = users.astype(np.int64)
    if users.size and (users.min() < 0 or users.max() >= n_table):
        raise ValueError(f"{name}: a user id lies outside [0, {n_table})")
    return users


def _wide_launch(ue, ie, users, mrow, mit, k, n_splits, scratch, top_s, top_i):
    """One lgcn_score_topk_wide on prepared device tensors (int32 users [n > 0], outputs [n x k],
    a uint8 scratch), on the current stream."""
    lib = engine.load_library()
    dev = ie.device
    P = engine._ptr
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_score_topk_wide(
            P(ue), ue.stride(0), P(users), int(users.numel()), P(ie), ie.stride(0),
            int(ie.shape[0]), int(ie.shape[1]), P(mrow), P(mit), k, n_splits, P(scratch),
            int(scratch.numel()), P(top_s), P(top_i), engine._stream(dev)), "lgcn_score_topk_wide")


def _wide_batches(ue, ie, users, mrow, mit, k, batch_size):
    """(scores fp32 [n x k], items int32 [n x k]): one lgcn_score_topk_wide per batch_size slots
    on views of the device-resident int32 users, one scratch (sized by the library) for the
    largest batch. No read-back."""
    lib = engine.load_library()
    dev = ie.device
    n, n_items = int(users.numel()), int(ie.shape[0])
    top_s = torch.empty((n, k), dtype=torch.float32, device=dev)
    top_i = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return top_s, top_i
    cus = _device_cus(dev)
    sizes = sorted({min(batch_size, n), n % batch_size or min(batch_size, n)})
    splits = {b: lib.lgcn_topk_wide_splits(b, n_items, k, cus) for b in sizes}
    scratch = torch.empty(max(lib.lgcn_score_topk_wide_scratch_bytes(b, k, s)
                              for b, s in splits.items()), dtype=torch.uint8, device=dev)
    ue, ie = _rows(ue), _rows(ie)
    for s in range(0, n, batch_size):
        e = min(s + batch_size, n)
        _wide_launch(ue, ie, users[s:e], mrow, mit, k, splits[e - s], scratch, top_s[s:e],
                     top_i[s:e])
    return top_s, top_i


def topk_wide(user_emb, item_emb, users, mask_rowptr, mask_items, k):
    """(scores fp32 [n x k], items int32 [n x k]) on the tables' HIP device: lgcn_score_topk_wide
    for the batch slots users[b], one launch. Every id must be a row of user_emb (ValueError). The
    mask arrays as for rank_fused. A width or k the kernel does not have is an error
    (topk_total_order_torch takes any)."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    k = int(k)
    if dev.type != "cuda":
        raise engine.LgcnError("topk_wide needs tables on a HIP device (topk_total_order_torch "
                               "runs anywhere)")
    if not wide_supported(item_emb.shape[1], k):
        raise engine.LgcnError(f"topk_wide: d = {item_emb.shape[1]}, k = {k} outside "
                               f"{FUSED_DIMS} x [1, {WIDE_MAX_K}]")
    mrow = _mask_tensor("mask_rowptr", mask_rowptr, dev)
    mit = _mask_tensor("mask_items", mask_items, dev)
    if mrow.numel() != user_emb.shape[0] + 1:
        raise ValueError("topk_wide: mask_rowptr must hold one entry per user row and one more")
    ids = _user_ids("topk_wide", users, user_emb.shape[0])
    users = torch.from_numpy(ids.astype(np.int32)).to(dev)
    return _wide_batches(user_emb, item_emb, users, mrow, _items_to_pass(mit), k,
                         max(int(users.numel()), 1))


def topk_total_order_torch(user_emb, item_emb, users, mask_rowptr, mask_items, k,
                           batch_size=1024):
    """topk_wide's contract with torch ops, for any width, any k >= 1 and any device (CPU
    included): scores by matmul in chunks of at most 1024 users, the user's mask items set to
    -1e10, the first k of a stable descending sort (equal scores keep ascending item index),
    -inf / -1 past the listable items. Its scores are matmul's, so on rounded inputs a list may
    differ from the kernel's where two scores meet in the last bit."""
    _check_tables(user_emb, item_emb)
    dev = item_emb.device
    k = int(k)
    if k < 1:
        raise ValueError("topk_total_order_torch: k must be positive")
    n_table, n_items = user_emb.shape[0], item_emb.shape[0]
    mrow = _mask_tensor("mask_rowptr", mask_rowptr, dev).long()
    mit = _mask_tensor("mask_items", mask_items, dev).long()
    if mrow.numel() != n_table + 1:
        raise ValueError("topk_total_order_torch: mask_rowptr must hold one entry per user row "
                         "and one more")
    users = torch.from_numpy(_user_ids("topk_total_order_torch", users, n_table)).to(dev)
    n = int(users.numel())
    top_s = torch.full((n, k), float("-inf"), dtype=torch.float32, device=dev)
    top_i = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    if n == 0 or n_items == 0:
        return top_s, top_i
    batch_size = max(1, min(int(batch_size), 1024))
    kk = min(k, n_items)
    for s in range(0, n, batch_size):
        u = users[s:s + batch_size]
        scores = torch.matmul(user_emb[u], item_emb.T)
        lens = mrow[u + 1] - mrow[u]
        total = int(lens.sum())
        if total:
            rr = torch.repeat_interleave(torch.arange(len(u), device=dev), lens)
            first = torch.cumsum(lens, 0) - lens
            pos = torch.arange(total, device=dev) - first[rr] + mrow[u][rr]
            scores[rr, mit[pos]] = -1e10
        # a NaN is never listed (and -inf is what an empty position holds)
        scores.masked_fill_(torch.isnan(scores), float("-inf"))
        vals, idx = torch.sort(scores, dim=1, descending=True, stable=True)
        vals, idx = vals[:, :kk], idx[:, :kk]
        listed = vals > float("-inf")
        top_s[s:s + batch_size, :kk] = vals
        top_i[s:s + batch_size, :kk] = torch.where(listed, idx, torch.full_like(idx, -1)).int()
    return top_s, top_i


def similar_items(item_emb, items, k):
    """Item-to-item lists: (scores fp32 [n x k], items int32 [n x k]) on item_emb's device, the k
    items with the largest dot product with each query item, the query itself excluded (it counts
    at -1e10, as a user's train items do). The query table is the item table and the mask of row i
    is {i}. HIP tables with wide_supported run lgcn_score_topk_wide (no fallback from it),
    anything else the torch route."""
    if not torch.is_tensor(item_emb) or item_emb.dim() != 2:
        raise engine.LgcnError("similar_items: item_emb must be a 2-D float32 tensor")
    _check_tables(item_emb, item_emb)
    dev = item_emb.device
    k = int(k)
    n_items = item_emb.shape[0]
    rowptr = torch.arange(n_items + 1, dtype=torch.int32, device=dev)
    own = torch.arange(n_items, dtype=torch.int32, device=dev)
    if item_emb.is_cuda and wide_supported(item_emb.shape[1], k):
        return topk_wide(item_emb, item_emb, items, rowptr, own, k)
    return topk_total_order_torch(item_emb, item_emb, items, rowptr, own, k)


class Evaluator:
    """Evaluator(train_users, train_items, num_users, num_items, device)

    Leave-one-out evaluation (main.py:404-439) that stays on the device. Built once: the train
    mask (mask_csr: per user the sorted, de-duplicated train items) is computed and uploaded here
    and never again; `from_sampler` takes a BprSampler's resident copy of the same CSR instead.

        ev = Evaluator.from_sampler(sampler)          # or Evaluator(train_u, train_i, U, I, dev)
        metrics = ev.evaluate(model, adj, val_df, ks=(10, 20, 50))
        metrics = ev.evaluate_lists(model, adj, test_df, ks=(10, 20, 50))  # every row of the frame
        scores, items = ev.recommend(model, adj, users, k=100)      # the lists, k up to WIDE_MAX_K

    evaluate() keeps one held-out item per user (the last row of a user wins, as main.py's
    dict(zip(...))); evaluate_lists() keeps them all and ranks a user's whole list from one pass.

    Device dispatch, as the sampler's: tables on a HIP device with a width in FUSED_DIMS run
    lgcn_score_rank / lgcn_score_rank_lists (no fallback for them), any other width and a CPU
    device run rank_torch / rank_lists_torch."""

    def __init__(self, train_users, train_items, num_users, num_items, device):
        users = np.asarray(train_users, dtype=np.int64)
        items = np.asarray(train_items, dtype=np.int64)
        if users.ndim != 1 or users.shape != items.shape:
            raise ValueError("Evaluator: train_users and train_items must be 1-D and of one length")
        num_users, num_items = int(num_users), int(num_items)
        if not (0 <= num_users < 1 << 31 and 0 <= num_items < 1 << 31 and users.size < 1 << 31):
            raise ValueError("Evaluator: num_users, num_items and the interaction count must be "
                             "below 2^31")
        if users.size and (users.min() < 0 or users.max() >= num_users or items.min() < 0
                           or items.max() >= num_items):
            raise ValueError("Evaluator: an interaction lies outside [0, num_users) x "
                             "[0, num_items)")
        rowptr, it = mask_csr(users, items, num_users)
        dev = self._device(device)
        if dev.type == "cuda":
            engine.load_library()  # a missing kernel is an error, here and not at the first call
        self._init(torch.from_numpy(rowptr).to(dev),
                   torch.from_numpy(np.ascontiguousarray(it, dtype=np.int32)).to(dev), num_users,
                   num_items, dev)

    @staticmethod
    def _device(device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:  # tensors report 'cuda:<current>'
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def _init(self, rowptr, items, num_users, num_items, dev):
        self._rowptr, self._items = rowptr, _items_to_pass(items)
        self.num_users, self.num_items, self.device = num_users, num_items, dev

    @classmethod
    def from_sampler(cls, sampler):
        """The evaluator of a BprSampler's train interactions: its pos_rowptr / pos_items are the
        mask CSR (include/lgcn.h), so they are held, not rebuilt or copied."""
        self = cls.__new__(cls)
        rowptr, items = sampler._rowptr, sampler._pos_items
        if not torch.is_tensor(rowptr):  # a CPU sampler keeps numpy: the same memory as tensors
            rowptr, items = torch.from_numpy(rowptr), torch.from_numpy(items)
        self._init(rowptr, items, sampler.num_users, sampler.num_items, cls._device(sampler.device))
        return self

    def _tables(self, model, adj):
        """The model's propagated (user, item) tables in eval mode (call under no_grad), checked
        against what this evaluator was built for."""
        model.eval()
        ue, ie = model(adj)[:2]
        _check_tables(ue, ie)
        if ie.device != self.device:
            raise engine.LgcnError(f"Evaluator on {self.device}, the model's tables on "
                                   f"{ie.device}")
        if ue.shape[0] != self.num_users or ie.shape[0] != self.num_items:
            raise engine.LgcnError(f"Evaluator for {self.num_users} x {self.num_items}, the "
                                   f"model's tables are {ue.shape[0]} x {ie.shape[0]}")
        return ue, ie

    def ranks(self, model, adj, eval_users, eval_items, batch_size=8192):
        """The rank of eval_items[j] for eval_users[j], as one int32 tensor on the device: one
        propagation under no_grad in model.eval() (left in eval mode, as main.py's evaluate leaves
        it), then one lgcn_score_rank per batch on views of the device-resident users and targets.
        No read-back. A pair outside [0, num_users) x [0, num_items) ranks -1."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("Evaluator.ranks: batch_size must be positive")
        with torch.no_grad():
            ue, ie = self._tables(model, adj)
            if not (ie.is_cuda and ie.shape[1] in FUSED_DIMS):
                return rank_torch(ue, ie, eval_users, eval_items, self._rowptr, self._items,
                                  min(batch_size, 1024))[0]
            users, targets = _slots(eval_users, eval_items, self.num_users, self.num_items,
                                    self.device)
            n = int(users.numel())
            rank = torch.empty(n, dtype=torch.int32, device=self.device)
            if n == 0:
                return rank
            lib = engine.load_library()
            score = torch.empty(n, dtype=torch.float32, device=self.device)
            cus = _device_cus(self.device)
            sizes = sorted({min(batch_size, n), n % batch_size or min(batch_size, n)})
            splits = {b: lib.lgcn_eval_splits(b, self.num_items, cus) for b in sizes}
            part = torch.empty(max(b * s for b, s in splits.items()), dtype=torch.int32,
                               device=self.device)
            ue, ie = _rows(ue), _rows(ie)
            for s in range(0, n, batch_size):
                e = min(s + batch_size, n)
                _rank_launch(ue, ie, users[s:e], targets[s:e], self._rowptr, self._items,
                             rank[s:e], score[s:e], part, splits[e - s])
        return rank

    def evaluate(self, model, adj, eval_data, ks=(20,)):
        """metrics_from_ranks of ranks(): eval_data is a (users, items) pair, or a DataFrame (any
        mapping) with 'user_idx' / 'item_idx', one held-out item per user as
        dict(zip(user_idx, item_idx)) keeps them (the last one wins). One read-back."""
        if hasattr(eval_data, "keys") and "user_idx" in eval_data.keys():
            held = dict(zip(eval_data["user_idx"], eval_data["item_idx"]))
            users = np.fromiter(held.keys(), dtype=np.int64, count=len(held))
            items = np.fromiter(held.values(), dtype=np.int64, count=len(held))
        else:
            users, items = eval_data
        return metrics_from_ranks(self.ranks(model, adj, users, items), ks)

    def rank_lists(self, model, adj, eval_users, eval_items, batch_size=8192):
        """Every held-out (user, item) pair ranked: (users int64, rowptr int32, ranks) with
        target_csr's users and offsets as numpy and ranks an int32 tensor on the device, entry e
        of user j at rowptr[j] <= e < rowptr[j+1] in item order. One propagation under no_grad in
        model.eval(), the lists built once, then one lgcn_score_rank_lists per batch_size user
        slots on pointer-offset views of the resident offsets (no per-batch copy, one scratch for
        the largest batch). No read-back. A pair outside [0, num_users) x [0, num_items) ranks
        -1."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("Evaluator.rank_lists: batch_size must be positive")
        host = [a.detach().cpu().numpy() if torch.is_tensor(a) else a
                for a in (eval_users, eval_items)]
        eu, rowptr, items = target_csr(*host)
        with torch.no_grad():
            ue, ie = self._tables(model, adj)
            if not (ie.is_cuda and ie.shape[1] in FUSED_DIMS):
                return eu, rowptr, rank_lists_torch(ue, ie, eu, rowptr, items, self._rowptr,
                                                    self._items, min(batch_size, 1024))[0]
            users_t, rowptr_t, items_t = _list_slots(eu, rowptr, items, self.num_users,
                                                     self.num_items, self.device)
            n = len(eu)
            rank = torch.full((len(items),), -1, dtype=torch.int32, device=self.device)
            if n == 0:
                return eu, rowptr, rank
            lib = engine.load_library()
            score = torch.empty(len(items), dtype=torch.float32, device=self.device)
            cus = _device_cus(self.device)
            batches = [(s, min(s + batch_size, n)) for s in range(0, n, batch_size)]
            splits = {e - s: lib.lgcn_eval_splits(e - s, self.num_items, cus) for s, e in batches}
            scratch = torch.empty(max(lib.lgcn_score_rank_lists_scratch_bytes(
                e - s, int(rowptr[e] - rowptr[s]), splits[e - s]) for s, e in batches),
                dtype=torch.uint8, device=self.device)
            ue, ie = _rows(ue), _rows(ie)
            for s, e in batches:
                _rank_lists_launch(ue, ie, users_t[s:e], rowptr_t[s:e + 1], items_t, self._rowptr,
                                   self._items, rank, score, scratch, splits[e - s])
        return eu, rowptr, rank

    def recommend(self, model, adj, users, k, batch_size=8192, exclude_train=True):
        """The k best items of every user of `users` in rank order: (scores fp32 [n x k], items
        int32 [n x k]) on the evaluator's device, -inf / -1 past the listable items. One
        propagation under no_grad in model.eval(), the ids checked on the host (one outside
        [0, num_users) is a ValueError) and uploaded once, then one lgcn_score_topk_wide per batch
        on views of them. No read-back. exclude_train=False lists the train items too (an
        all-empty mask). HIP tables with wide_supported(d, k) run the kernel (no fallback from
        it), anything else topk_total_order_torch."""
        batch_size, k = int(batch_size), int(k)
        if batch_size < 1:
            raise ValueError("Evaluator.recommend: batch_size must be positive")
        if k < 1:
            raise ValueError("Evaluator.recommend: k must be positive")
        ids = _user_ids("Evaluator.recommend", users, self.num_users)
        with torch.no_grad():
            ue, ie = self._tables(model, adj)
            if exclude_train:
                mrow, mit = self._rowptr, self._items
            else:
                mrow = torch.zeros(self.num_users + 1, dtype=torch.int32, device=self.device)
                mit = torch.zeros(1, dtype=torch.int32, device=self.device)
            if not (ie.is_cuda and wide_supported(ie.shape[1], k)):
                return topk_total_order_torch(ue, ie, ids, mrow, mit, k, min(batch_size, 1024))
            users_t = torch.from_numpy(ids.astype(np.int32)).to(self.device)
            return _wide_batches(ue, ie, users_t, mrow, mit, k, batch_size)

    def evaluate_lists(self, model, adj, eval_data, ks=(20,)):
        """metrics_from_rank_lists of rank_lists(): eval_data is a (users, items) pair, or a
        DataFrame (any mapping) with 'user_idx' / 'item_idx'. Every row is kept: a user's list is
        all its distinct held-out items. One read-back."""
        if hasattr(eval_data, "keys") and "user_idx" in eval_data.keys():
            users, items = np.asarray(eval_data["user_idx"]), np.asarray(eval_data["item_idx"])
        else:
            users, items = eval_data
        _, rowptr, ranks = self.rank_lists(model, adj, users, items)
        return metrics_from_rank_lists(ranks, rowptr, ks)
