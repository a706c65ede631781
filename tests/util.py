import hashlib

import numpy as np


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


MASKED = float(np.float32(-1e10))  # the -1e10 train-item fill as the fp32 it becomes


def masked_scores64(user_emb, item_emb, users, mask_rowptr, mask_items):
    """[len(users) x n_items] float64 scores user_emb[users] · item_embᵀ with every (user, train
    item) pair of the mask CSR set to MASKED."""
    users = np.asarray(users, dtype=np.int64)
    s = np.asarray(user_emb, dtype=np.float64)[users] @ np.asarray(item_emb, dtype=np.float64).T
    for b, u in enumerate(users):
        s[b, np.asarray(mask_items[mask_rowptr[u]:mask_rowptr[u + 1]], dtype=np.int64)] = MASKED
    return s


def topk_total_order(scores, k):
    """The first k of every row of `scores` under include/lgcn.h's total order (score descending,
    item index ascending): (scores float64 [n x k], indices int64 [n x k]), padded with
    -inf / -1 where a row has fewer than k entries."""
    n, m = scores.shape
    top_s = np.full((n, k), -np.inf)
    top_i = np.full((n, k), -1, dtype=np.int64)
    item = np.arange(m)
    for b in range(n):
        order = np.lexsort((item, -scores[b]))[:k]
        top_s[b, :order.size] = scores[b, order]
        top_i[b, :order.size] = order
    return top_s, top_i


def topk_reference(user_emb, item_emb, users, mask_rowptr, mask_items, k):
    """lgcn_score_topk in plain numpy, float64: all scores, masked pairs at MASKED, the first k
    under the header's total order."""
    return topk_total_order(masked_scores64(user_emb, item_emb, users, mask_rowptr, mask_items), k)


def assert_close_normwise(got, ref, tol=1e-5, what=""):
    """Parity gate of north_star / SURVEY §8d: max|got-ref| <= tol * max|ref| per tensor."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err <= tol * max(scale, 1e-30), f"{what}: max|d|={err:.3e} > {tol}*{scale:.3e}"
