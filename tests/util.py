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


def stacked_mean_torch_order(layers, tail_width):
    """torch.mean(torch.stack(layers, 0), 0) on the CPU for 2..17 float32 layers of one shape,
    restated in numpy float32 (measured: tests/test_reference_mean.py). Over the flattened
    [n*d] result ATen sums the layers one after the other from +0 below
    cut = (n*d // tail_width) * tail_width. From cut on its row_sum keeps four partial sums from
    +0, p[k] += layer[4*j + k] over the complete groups of four layers, adds the leftover layers
    into p[0] in order and returns ((p0 + p1) + p2) + p3. Then the divide by the layer count.
    tail_width belongs to the ATen build (its vector width times its unroll)."""
    x = np.stack([np.asarray(a, dtype=np.float32) for a in layers])
    shape = x.shape[1:]
    x = x.reshape(x.shape[0], -1)
    L, m = x.shape
    cut = (m // tail_width) * tail_width
    s = np.zeros(m, np.float32)
    for i in range(L):
        s[:cut] = s[:cut] + x[i, :cut]
    p = np.zeros((4, m - cut), np.float32)
    for i in range(L - L % 4):
        p[i % 4] = p[i % 4] + x[i, cut:]
    for i in range(L - L % 4, L):
        p[0] = p[0] + x[i, cut:]
    s[cut:] = ((p[0] + p[1]) + p[2]) + p[3]
    return (s / np.float32(L)).reshape(shape)


# ---- fusion pre-layer and BPR loss references (float64, plain numpy) ----------------------------
U32 = 2.0 ** -24  # unit roundoff of fp32


def gamma(n):
    """Higham's gamma_n = n*u / (1 - n*u) for fp32: the relative bound on n chained roundings."""
    return n * U32 / (1.0 - n * U32)


def fusion_reference(id_emb, content, W, b, slope=None):
    """(z64, mag) of the fusion pre-layer: z64 = [id | content] @ W.T + b in float64 and
    mag = |[id | content]| @ |W|.T + |b|, the sum of absolute products a rounding bound scales
    with. b None = no bias. The activation is applied by leaky64 / fusion_exact (slope is
    accepted so that a call names the whole operation)."""
    x = np.concatenate([np.asarray(id_emb, dtype=np.float64),
                        np.asarray(content, dtype=np.float64)], axis=1)
    W = np.asarray(W, dtype=np.float64)
    b = np.zeros(W.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
    return x @ W.T + b, np.abs(x) @ np.abs(W).T + np.abs(b)


def leaky64(z64, slope):
    return np.where(z64 > 0, z64, z64 * float(slope))


def fusion_exact(z64, slope):
    """The fp32 output of the documented expression when every partial sum is exact (few-bit
    inputs): fp32(z) where z > 0, else fp32(fp32(z) * fp32(slope)). An accumulator starts from +0,
    so a sum that is zero is +0 (z64 + 0.0 turns a -0 of the float64 product into it); the
    product with the slope keeps IEEE signs (a negative z times slope 0 is -0)."""
    z = (np.asarray(z64) + 0.0).astype(np.float32)
    assert np.array_equal(z.astype(np.float64), np.asarray(z64) + 0.0), "z is not an exact fp32"
    return np.where(z > 0, z, z * np.float32(slope))


def fewbit_fusion_case(n, d, c_dim, seed):
    """Few-bit inputs: id / content integers in [-8, 8], W and b multiples of 1/8 of magnitude
    <= 2, so every partial sum of the <= 257 terms of an output is an exact fp32 in any order
    (asserted: mag * 8 is an integer below 2^24). Planted rows (rows 0..3, then i % 97 in
    5 / 11 / 17 / 23), with b = -W[:, j0] and W[:, d] = W[:, d-1]:
      A  x = e_j0                          z == 0 in every column, from b = -sum
      B  x = e_j0 + 5 e_{d-1} - 5 e_d      z == 0, from cancellation across the two tables and b
      C  x = 7 e_{d-1} - 7 e_d             the products cancel: z == b (zero without a bias)
      D  x = -8 e_{K-1}, W[:, K-1] in [1, 2]   every z < 0
    Returns (id, content, W, b) as float32."""
    rng = np.random.default_rng(seed)
    K = d + c_dim
    x = rng.integers(-8, 9, (n, K)).astype(np.float32)
    W = (rng.integers(-16, 17, (d, K)) / 8.0).astype(np.float32)
    j0, j1, j2, j3 = 3, d - 1, d, K - 1
    W[:, j2] = W[:, j1]
    W[:, j3] = ((8 + rng.integers(0, 9, d)) / 8.0).astype(np.float32)
    b = -W[:, j0]
    rows = np.arange(n)
    kinds = {"A": (0, 5), "D": (1, 23), "B": (2, 11), "C": (3, 17)}
    for kind, (first, residue) in kinds.items():
        sel = (rows == first) | ((rows >= 4) & (rows % 97 == residue))
        x[sel] = 0
        if kind in "AB":
            x[sel, j0] = 1
        if kind in "BC":
            v = 5 if kind == "B" else 7
            x[sel, j1], x[sel, j2] = v, -v
        if kind == "D":
            x[sel, j3] = -8
    idw, content = np.ascontiguousarray(x[:, :d]), np.ascontiguousarray(x[:, d:])
    _, mag = fusion_reference(idw, content, W, b)
    assert np.array_equal(mag * 8, np.rint(mag * 8)) and (mag * 8 < 2 ** 24).all()
    return idw, content, W, b


def fewbit_planted_rows(n):
    """Row indices of fewbit_fusion_case's planted kinds: {"A": [...], ...}."""
    rows = np.arange(n)
    out = {}
    for kind, (first, residue) in {"A": (0, 5), "D": (1, 23), "B": (2, 11), "C": (3, 17)}.items():
        out[kind] = rows[(rows == first) | ((rows >= 4) & (rows % 97 == residue))]
    return out


EPS32 = np.float64(np.float32(1e-8))  # the 1e-8 of the loss as the fp32 the kernel adds


def bpr_reference(u, p, n, u0, p0, n0, lam):
    """Per-sample float64 values of the BPR loss expression on fp32 inputs, as a dict:
    x = <u,p> - <u,n>; mag_x = sum|u*p| + sum|u*n|; log = log(sigmoid(x) + fp32(1e-8));
    c = (-1/B) / (s + 1e-8) * (1 - s) * s (d loss / d x); sq = |u0|^2 + |p0|^2 + |n0|^2; and
    loss = -mean(log) + fp32(lam) * sum(sq) / B."""
    u, p, n, u0, p0, n0 = (np.asarray(t, dtype=np.float64) for t in (u, p, n, u0, p0, n0))
    B = u.shape[0]
    x = (u * p).sum(1) - (u * n).sum(1)
    mag_x = np.abs(u * p).sum(1) + np.abs(u * n).sum(1)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    log = np.log(s + EPS32)
    c = (-1.0 / B) / (s + EPS32) * (1.0 - s) * s
    sq = (u0 * u0).sum(1) + (p0 * p0).sum(1) + (n0 * n0).sum(1)
    loss = -log.mean() + float(np.float32(lam)) * sq.sum() / B
    return dict(x=x, mag_x=mag_x, log=log, c=c, sq=sq, loss=loss)


def bpr_reduce_fp32(terms, B, lam):
    """k_bpr_reduce restated in numpy float32: thread i < 256 sums terms[i], terms[i + 256], ...
    in index order from +0; the halving tree 128, 64, ..., 1; loss = -(sl / B) + (lam * sr) / B,
    every operation rounded once (the build does not contract a*b+c)."""
    f = np.float32
    t = np.asarray(terms, dtype=np.float32).reshape(2, B)
    pad = np.zeros((2, -B % 256), dtype=np.float32)
    t = np.concatenate([t, pad], axis=1).reshape(2, -1, 256)
    part = np.zeros((2, 256), dtype=np.float32)
    for j in range(t.shape[1]):
        part = part + t[:, j, :]
    w = 128
    while w > 0:
        part[:, :w] = part[:, :w] + part[:, w:2 * w]
        w >>= 1
    sl, sr = part[0, 0], part[1, 0]
    return f(-(sl / f(B))) + f(f(f(lam) * sr) / f(B))


def fewbit_bpr_case(B, d, seed):
    """Six [B x d] blocks of integers in [-8, 8] as float32: every dot product and squared norm
    (at most 3 * 256 * 64) is an exact fp32 in any order."""
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, (B, d)).astype(np.float32) for _ in range(6)]
