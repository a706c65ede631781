"""The BPR negative sampler (main.py:349-363, BPRDataset behind a DataLoader) without the Python
call per interaction: one draw for a whole epoch, on the device the training step runs on.

    sampler = BprSampler(train_df['user_idx'], train_df['item_idx'], U, I, device, seed=0)
    for users, pos, neg in sampler.epoch(epoch, batch_size):      # views of one draw
        loss = model.bpr_step(adj, users, pos, neg, weight_decay)

The draw (include/lgcn.h, lgcn_bpr_sample; DESIGN §5 "Sampler"). The negative of interaction idx
— its index in the arrays the sampler was built from — is a pure function of (seed, epoch, idx, the
user's positive list, num_items):

    r64   = Philox4x32-10(counter (idx_lo32, idx_hi32, epoch, 0), key (seed_lo32, seed_hi32)),
            r64 = out[1] << 32 | out[0]
    j     = mulhi64(r64, n_free),  n_free = num_items - deg(user)
    neg   = j + m,  m = #{t : L[t] - t <= j},  L = the user's sorted, de-duplicated items

i.e. the j-th item the user has not interacted with: uniform over the complement, the
distribution of the reference's rejection loop, without the loop. A user with every item as a
positive (the reference never returns for one) gets neg = -1 and is counted in `unsampled`;
bpr_step skips such a sample on a HIP device. Batch size, shuffle order, first / count windows and
the launch geometry do not enter the draw; `epoch` and `seed` do.

Several negatives per sample (`n_neg`, lgcn_bpr_sample_multi): ordinal m of an interaction is the
same draw with the counter's last word set to m, so the ordinals are independent draws (repeats
possible), column 0 is the one-negative draw and no column depends on n_neg. bpr_step trains on the
hardest of them or on all (train.bpr_step, negatives=).

Weighted negatives (`weights=`, lgcn_bpr_sample_weighted): integer item weights w[i] in
[0, 2^24] — popularity_weights (count^alpha) through quantise_weights — as two int64 prefix-sum
tables, item_cumw [I + 1] over the items and pos_cumw [n_pos + 1] over the positive CSR. r64 is
the draw's above; with beg / end the user's CSR range and pw[t] = pos_cumw[beg + t] - pos_cumw[beg]:

    W_free = item_cumw[I] - (pos_cumw[end] - pos_cumw[beg])     # <= 0: neg = -1, `unsampled`
    r      = mulhi64_wide(r64, W_free)
    t*     = #{t : item_cumw[L[t]] - pw[t] <= r}                # upper-bound binary search
    neg    = (the first k with item_cumw[k] > r + pw[t*]) - 1   # upper-bound binary search

a free item is drawn with probability w[i] / W_free, a positive or a zero-weight item never; no
alias table, no rejection loop, the same pure function on both devices, and with all weights 1 the
uniform draw bit for bit. neg_log_q() is the matching logQ correction of the sampled softmax.

Device dispatch, as the models and loss.py: a HIP `device` runs csrc/lgcn_sampler.hip (no
fallback), a CPU `device` runs the same arithmetic as vectorised numpy — what a CPU-only user
gets, and the reference the GPU tests compare the kernel against, bit for bit.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import engine
from .evaluate import mask_csr

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
SHUFFLE_MIX = 0x9E3779B97F4A7C15  # epoch()'s permutation seed: (seed + SHUFFLE_MIX * epoch) mod 2^63
INT31 = 1 << 31


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words: counter (c0..c3), key (k0, k1) ->
    the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0 = np.asarray(k0, dtype=np.uint64) & _MASK32
    k1 = np.asarray(k1, dtype=np.uint64) & _MASK32
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]   # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK32]
        k0 = (k0 + np.uint64(PHILOX_W0)) & _MASK32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _MASK32
    return tuple(x.astype(np.uint32) for x in c)


def mulhi64(r64, n):
    """The high 64 bits of r64 * n for uint64 r64 and 0 <= n < 2^31, exactly, without 128-bit
    integers: (hi * n + ((lo * n) >> 32)) >> 32 — both products and the sum stay below 2^64."""
    r64 = np.asarray(r64, dtype=np.uint64)
    n = np.asarray(n, dtype=np.uint64)
    hi, lo = r64 >> _S32, r64 & _MASK32
    return (hi * n + ((lo * n) >> _S32)) >> _S32


def random_r64(idx, seed, epoch, ordinal=0):
    """r64(seed, epoch, idx, ordinal) per element (uint64): the draw's 64 Philox bits; ordinal (a
    scalar or an array that broadcasts against idx) is the counter's fourth word."""
    idx = np.asarray(idx, dtype=np.int64).astype(np.uint64)
    seed = int(seed)
    o0, o1, _, _ = philox4x32_10(idx & _MASK32, idx >> _S32, np.uint64(int(epoch)),
                                 np.asarray(ordinal, dtype=np.uint64),
                                 np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF))
    return (o1.astype(np.uint64) << _S32) | o0.astype(np.uint64)


def random_j(idx, n_free, seed, epoch, ordinal=0):
    """j = mulhi64(r64(seed, epoch, idx, ordinal), n_free) per element (int64)."""
    return mulhi64(random_r64(idx, seed, epoch, ordinal), n_free).astype(np.int64)


def kth_missing(pos_rowptr, pos_items, users, j):
    """Per element the j-th (0-based) item missing from its user's sorted list L: j + m with
    m = #{t : L[t] - t <= j}, by the kernel's upper-bound binary search (L[t] - t is
    non-decreasing), every element's search advanced one step per vectorised round; elements
    drop out as their interval closes, so the rounds after the first few touch only the users
    with long lists."""
    rowptr = np.asarray(pos_rowptr)
    items = np.asarray(pos_items)
    users = np.asarray(users, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    base = rowptr[users].astype(np.int64)
    lo, hi = base.copy(), rowptr[users + 1].astype(np.int64)
    act = np.nonzero(lo < hi)[0]
    while act.size:
        l, h = lo[act], hi[act]
        mid = (l + h) >> 1
        up = items[mid] - (mid - base[act]) <= j[act]
        l, h = np.where(up, mid + 1, l), np.where(up, h, mid)
        lo[act], hi[act] = l, h
        act = act[l < h]
    return j + (lo - base)


def mulhi64_wide(r64, n):
    """The high 64 bits of r64 * n for uint64 r64 and 0 <= n < 2^63, exactly, from 32-bit limbs:
    the four partial products each fit uint64, the middle column's carries are summed apart."""
    r64 = np.asarray(r64, dtype=np.uint64)
    n = np.asarray(n, dtype=np.uint64)
    rh, rl = r64 >> _S32, r64 & _MASK32
    nh, nl = n >> _S32, n & _MASK32
    lh, hl = rl * nh, rh * nl
    mid = ((rl * nl) >> _S32) + (lh & _MASK32) + (hl & _MASK32)
    return rh * nh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def random_r(idx, w_free, seed, epoch, ordinal=0):
    """random_j for a weighted range: mulhi64_wide(r64(seed, epoch, idx, ordinal), w_free), int64."""
    return mulhi64_wide(random_r64(idx, seed, epoch, ordinal), w_free).astype(np.int64)


def weighted_missing(pos_rowptr, pos_items, pos_cumw, item_cumw, users, r):
    """Per element the free item of its user that covers position r of the user's concatenated
    free weights (0 <= r < W_free): lgcn_bpr_sample_weighted's two upper-bound binary searches,
    every element advanced one step per vectorised round like kth_missing. An L[t] outside
    [0, I) counts as greater than r; a result outside [0, I) is -1."""
    rowptr = np.asarray(pos_rowptr)
    items = np.asarray(pos_items)
    pcw = np.asarray(pos_cumw, dtype=np.int64)
    icw = np.asarray(item_cumw, dtype=np.int64)
    n_items = icw.shape[0] - 1
    users = np.asarray(users, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    base = rowptr[users].astype(np.int64)
    lo, hi = base.copy(), rowptr[users + 1].astype(np.int64)
    act = np.nonzero(lo < hi)[0]
    while act.size:
        l, h = lo[act], hi[act]
        mid = (l + h) >> 1
        it = items[mid].astype(np.int64)
        ok = (it >= 0) & (it < n_items)
        up = ok & (icw[np.where(ok, it, 0)] - (pcw[mid] - pcw[base[act]]) <= r[act])
        l, h = np.where(up, mid + 1, l), np.where(up, h, mid)
        lo[act], hi[act] = l, h
        act = act[l < h]
    rr = r + (pcw[lo] - pcw[base])
    lo, hi = np.zeros_like(rr), np.full_like(rr, n_items + 1)
    act = np.arange(rr.shape[0])
    while act.size:
        l, h = lo[act], hi[act]
        mid = (l + h) >> 1
        up = icw[mid] <= rr[act]
        l, h = np.where(up, mid + 1, l), np.where(up, h, mid)
        lo[act], hi[act] = l, h
        act = act[l < h]
    neg = lo - 1
    return np.where((neg >= 0) & (neg < n_items), neg, -1)


MAX_WEIGHT = 1 << 24  # an item's largest integer weight: I < 2^31 items keep the totals below 2^55


def popularity_weights(items, num_items, alpha=0.75):
    """float64 [num_items]: count_i ** alpha, count_i the number of interactions (duplicates
    included) with item i; 0 for an item without one, whatever alpha. word2vec's alpha = 0.75
    flattens the popularity; 1 is the interaction distribution, 0 uniform over the seen items."""
    count = np.bincount(np.asarray(items, dtype=np.int64), minlength=int(num_items))
    count = count.astype(np.float64)
    return np.where(count > 0, count ** float(alpha), 0.0)


def quantise_weights(w, num_items=None):
    """The int64 weights in [0, 2^24] the draw takes. A float array becomes
    rint(w / max(w) * 2^24), a positive weight that rounds to 0 raised to 1 (a rare item stays
    drawable); an integer array in [0, 2^24] is taken verbatim. Anything negative, non-finite,
    above 2^24 (integers), not 1-D, not of num_items entries (when given) or all zero raises
    ValueError."""
    w = np.asarray(w)
    if w.ndim != 1 or (num_items is not None and w.shape[0] != int(num_items)):
        raise ValueError(f"quantise_weights: a 1-D array of {num_items} weights expected, got "
                         f"shape {w.shape}")
    if np.issubdtype(w.dtype, np.integer):
        if w.size and (w.min() < 0 or w.max() > MAX_WEIGHT):
            raise ValueError(f"quantise_weights: integer weights must lie in [0, {MAX_WEIGHT}]")
        q = w.astype(np.int64)
    elif np.issubdtype(w.dtype, np.floating):
        if not np.isfinite(w).all() or (w.size and w.min() < 0):
            raise ValueError("quantise_weights: weights must be finite and not negative")
        top = float(w.max()) if w.size else 0.0
        if top <= 0:
            raise ValueError("quantise_weights: every weight is zero")
        q = np.rint(w.astype(np.float64) / top * MAX_WEIGHT).astype(np.int64)
        q[(w > 0) & (q == 0)] = 1
    else:
        raise ValueError(f"quantise_weights: integer or float weights expected, got {w.dtype}")
    if not q.any():
        raise ValueError("quantise_weights: every weight is zero")
    return q


def cumulative_weights(w, pos_items):
    """(pos_cumw [n_pos + 1], item_cumw [I + 1]): the exclusive int64 prefix sums of w over the
    positive CSR's items and over the items."""
    w = np.asarray(w, dtype=np.int64)
    item_cumw = np.zeros(w.shape[0] + 1, dtype=np.int64)
    np.cumsum(w, out=item_cumw[1:])
    pos_items = np.asarray(pos_items, dtype=np.int64)
    pos_cumw = np.zeros(pos_items.shape[0] + 1, dtype=np.int64)
    np.cumsum(w[pos_items], out=pos_cumw[1:])
    return pos_cumw, item_cumw


CHUNK = 1 << 16  # slots per piece of the numpy path: its temporaries stay in cache
MAX_NEG = engine.BPR_MAX_NEG  # LGCN_BPR_MAX_NEG


def check_n_neg(n_neg, what="sampler"):
    """n_neg as every entry point here takes it: None (one negative, a 1-D `neg`) or an integer in
    [1, MAX_NEG] (`neg` of shape [count, n_neg]); anything else raises ValueError."""
    if n_neg is None:
        return None
    if isinstance(n_neg, bool) or not isinstance(n_neg, (int, np.integer)) or \
            not 1 <= n_neg <= MAX_NEG:
        raise ValueError(f"{what}: n_neg must be None or an integer in [1, {MAX_NEG}], "
                         f"got {n_neg!r}")
    return int(n_neg)


def sample_numpy(inter_user, inter_item, order, first, count, pos_rowptr, pos_items, n_users,
                 n_items, seed, epoch, n_neg=None, cumw=None):
    """lgcn_bpr_sample's contract on the host, vectorised: (users, pos, neg) int64 arrays of
    `count` slots and the number of samples left without a negative. Slots whose interaction
    index or user lies outside its range are -1 in all three, as the kernel writes them. Runs in
    pieces of CHUNK slots on a few threads (numpy releases the GIL; a slot's result does not
    depend on the split). n_neg = an integer: lgcn_bpr_sample_multi's contract, neg of shape
    [count, n_neg], column m drawn with counter word 3 = m (column 0 = the one-negative draw); a
    slot without a free item counts once. cumw = (pos_cumw, item_cumw): lgcn_bpr_sample_weighted's
    contract, the weighted draw (n_neg=None: one column, a 1-D neg)."""
    n_neg = check_n_neg(n_neg, "sample_numpy")
    inter_user = np.asarray(inter_user)
    inter_item = np.asarray(inter_item)
    rowptr = np.asarray(pos_rowptr)
    items = np.asarray(pos_items)
    order = None if order is None else np.asarray(order, dtype=np.int64)
    users = np.full(count, -1, dtype=np.int64)
    pos = np.full(count, -1, dtype=np.int64)
    neg = np.full(count if n_neg is None else (count, n_neg), -1, dtype=np.int64)
    cols = neg.reshape(count, n_neg or 1)  # a view

    def piece(b):
        e = min(b + CHUNK, count)
        idx = np.arange(first + b, first + e, dtype=np.int64)
        if order is not None:
            idx = order[idx]
        sel = np.nonzero((idx >= 0) & (idx < inter_user.shape[0]))[0]
        u = inter_user[idx[sel]].astype(np.int64)
        ok = (u >= 0) & (u < n_users)
        sel, u = sel[ok], u[ok]
        idx = idx[sel]
        users[b:e][sel] = u
        pos[b:e][sel] = inter_item[idx]
        if cumw is not None:
            pcw, icw = cumw
            w_free = icw[n_items] - (pcw[rowptr[u + 1]] - pcw[rowptr[u]])
            free = w_free > 0
            for m in range(cols.shape[1]):
                r = random_r(idx[free], w_free[free], seed, epoch, m)
                cols[b:e, m][sel[free]] = weighted_missing(rowptr, items, pcw, icw, u[free], r)
            return int(free.size - free.sum())
        n_free = n_items - (rowptr[u + 1].astype(np.int64) - rowptr[u])
        free = n_free > 0
        for m in range(cols.shape[1]):
            j = random_j(idx[free], n_free[free], seed, epoch, m)
            cols[b:e, m][sel[free]] = kth_missing(rowptr, items, u[free], j)
        return int(free.size - free.sum())

    starts = range(0, count, CHUNK)
    if len(starts) > 1:
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            missed = sum(pool.map(piece, starts))
    else:
        missed = sum(piece(b) for b in starts)
    return users, pos, neg, missed


def sample_device(inter_user, inter_item, order, first, count, pos_rowptr, pos_items, n_users,
                  n_items, seed, epoch, unsampled=None, n_neg=None, cumw=None):
    """lgcn_bpr_sample on the HIP device of `inter_user` (int32 tensors; order: int64 or None),
    on the caller's current stream: (users, pos, neg) int64 tensors of `count` slots. unsampled:
    None, or the device int32 counter the kernel adds to (the caller zeroes it). n_neg = an
    integer: lgcn_bpr_sample_multi, neg of shape [count, n_neg]; still one launch. cumw =
    (pos_cumw, item_cumw), int64 tensors of n_pos + 1 and n_items + 1 entries:
    lgcn_bpr_sample_weighted (n_neg=None: its n_neg = 1 into a 1-D neg)."""
    n_neg = check_n_neg(n_neg, "sample_device")
    lib = engine.load_library()
    dev = inter_user.device
    for name, t, dt in (("inter_user", inter_user, torch.int32), ("inter_item", inter_item,
                                                                   torch.int32),
                        ("pos_rowptr", pos_rowptr, torch.int32), ("pos_items", pos_items,
                                                                  torch.int32),
                        ("order", order, torch.int64), ("unsampled", unsampled, torch.int32),
                        ("pos_cumw", cumw and cumw[0], torch.int64),
                        ("item_cumw", cumw and cumw[1], torch.int64)):
        if t is None:
            continue
        if t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise engine.LgcnError(f"sampler: {name} must be a contiguous {dt} tensor on {dev}")
    if order is not None and first + count > order.numel():
        raise engine.LgcnError(f"sampler: first + count = {first + count} past the order's "
                               f"{order.numel()} entries")
    if pos_rowptr.numel() != n_users + 1:
        raise engine.LgcnError("sampler: pos_rowptr must hold num_users + 1 entries")
    if first < 0 or count < 0:
        raise engine.LgcnError("sampler: negative first or count")
    P = engine._ptr
    if cumw is not None:
        pos_cumw, item_cumw = cumw
        if item_cumw.numel() != n_items + 1 or pos_cumw.numel() != pos_items.numel() + 1:
            raise engine.LgcnError("sampler: item_cumw must hold num_items + 1 entries and "
                                   "pos_cumw one more than pos_items")
        out = torch.empty((2, count), dtype=torch.int64, device=dev)
        neg = torch.empty(count if n_neg is None else (count, n_neg), dtype=torch.int64,
                          device=dev)
        if count:
            with torch.cuda.device(dev):
                engine._check(lib.lgcn_bpr_sample_weighted(
                    P(inter_user), P(inter_item), inter_user.numel(), P(order), first, count,
                    P(pos_rowptr), P(pos_items), P(pos_cumw), P(item_cumw), n_users, n_items,
                    ctypes.c_uint64(int(seed)), ctypes.c_uint32(int(epoch)), n_neg or 1,
                    P(out[0]), P(out[1]), P(neg), P(unsampled), engine._stream(dev)),
                    "lgcn_bpr_sample_weighted")
        return out[0], out[1], neg
    if n_neg is not None:
        out = torch.empty((2, count), dtype=torch.int64, device=dev)
        neg = torch.empty((count, n_neg), dtype=torch.int64, device=dev)
        if count:
            with torch.cuda.device(dev):
                engine._check(lib.lgcn_bpr_sample_multi(
                    P(inter_user), P(inter_item), inter_user.numel(), P(order), first, count,
                    P(pos_rowptr), P(pos_items), n_users, n_items, ctypes.c_uint64(int(seed)),
                    ctypes.c_uint32(int(epoch)), n_neg, P(out[0]), P(out[1]), P(neg),
                    P(unsampled), engine._stream(dev)), "lgcn_bpr_sample_multi")
        return out[0], out[1], neg
    out = torch.empty((3, count), dtype=torch.int64, device=dev)
    if count == 0:  # nothing to launch (and an empty tensor has no pointer to pass)
        return out[0], out[1], out[2]
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_bpr_sample(
            P(inter_user), P(inter_item), inter_user.numel(), P(order), first, count,
            P(pos_rowptr), P(pos_items), n_users, n_items, ctypes.c_uint64(int(seed)),
            ctypes.c_uint32(int(epoch)), P(out[0]), P(out[1]), P(out[2]), P(unsampled),
            engine._stream(dev)), "lgcn_bpr_sample")
    return out[0], out[1], out[2]


class BprSampler:
    """BprSampler(users, items, num_users, num_items, device, seed=0, weights=None, alpha=0.75)

    users / items: the train interactions (train_df['user_idx'], train_df['item_idx']), each one
    a sample as in BPRDataset, duplicates included. Built once: the per-user positive lists are
    evaluate.mask_csr's (sorted, de-duplicated; numpy, no groupby), uploaded with the interactions
    as int32. len(sampler) = the number of interactions.

    weights=None: negatives uniform over the items the user has not interacted with. weights =
    "popularity": in proportion to popularity_weights(items, num_items, alpha); weights = an array
    of num_items entries: in proportion to it; either through quantise_weights (integer weights
    in [0, 2^24], `item_weights`). An item of weight 0 is never drawn; a user whose free items
    all have weight 0 gets neg = -1. draw and epoch then run lgcn_bpr_sample_weighted (a CPU
    device: the numpy twin); neg_log_q() is the matching correction of a sampled softmax."""

    def __init__(self, users, items, num_users, num_items, device, seed=0, weights=None,
                 alpha=0.75):
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int64))
        items = np.ascontiguousarray(np.asarray(items, dtype=np.int64))
        if users.ndim != 1 or users.shape != items.shape:
            raise ValueError("BprSampler: users and items must be 1-D and of one length")
        num_users, num_items = int(num_users), int(num_items)
        if not (0 <= num_users < INT31 and 0 <= num_items < INT31 and users.size < INT31):
            raise ValueError("BprSampler: num_users, num_items and the interaction count must be "
                             "below 2^31")
        if users.size and (users.min() < 0 or users.max() >= num_users or items.min() < 0
                           or items.max() >= num_items):
            raise ValueError("BprSampler: an interaction lies outside [0, num_users) x "
                             "[0, num_items)")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("BprSampler: seed must fit 64 unsigned bits")
        self.num_users, self.num_items, self.seed = num_users, num_items, seed
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # main.py:59 builds torch.device('cuda'); tensors report 'cuda:<current>', and the two
            # compare unequal: keep the indexed form every later comparison meets
            self.device = torch.device("cuda", torch.cuda.current_device())
        rowptr, pos_items = mask_csr(users, items, num_users)
        self._n = int(users.size)
        self._log_q = self._neg_log_q = None
        self.item_weights = self._cumw = None
        if weights is not None:
            if isinstance(weights, str):
                if weights != "popularity":
                    raise ValueError(f"BprSampler: weights={weights!r} (None, 'popularity' or an "
                                     "array)")
                weights = popularity_weights(items, num_items, alpha)
            self.item_weights = quantise_weights(weights, num_items)
            self._cumw = cumulative_weights(self.item_weights, pos_items)
            if self.device.type == "cuda":
                self._cumw = tuple(torch.from_numpy(a).to(self.device) for a in self._cumw)
                if pos_items.shape[0] == 0:
                    # _pos_items is padded to one entry below (no row holds it): keep
                    # pos_cumw one entry longer than it
                    self._cumw = (torch.zeros(2, dtype=torch.int64, device=self.device),
                                  self._cumw[1])
        host = (users.astype(np.int32), items.astype(np.int32), rowptr,
                np.ascontiguousarray(pos_items, dtype=np.int32))
        if self.device.type == "cuda":
            engine.load_library()  # a missing kernel is an error, here and not at the first draw
            self._user, self._item, self._rowptr, self._pos_items = (
                torch.from_numpy(a).to(self.device) for a in host)
            if self._pos_items.numel() == 0:
                self._pos_items = torch.zeros(1, dtype=torch.int32, device=self.device)
        else:
            self._user, self._item, self._rowptr, self._pos_items = host
        # samples of the latest draw left without a negative (users with no free item)
        self.unsampled = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __len__(self):
        return self._n

    def positives(self):
        """(rowptr, items): the per-user sorted, de-duplicated positive lists the draw excludes,
        int32 tensors on the sampler's device (rowptr of num_users + 1 entries) — what
        train.inbatch_step takes as `positives` to drop a user's known positives from its
        in-batch negatives."""
        if self.device.type == "cuda":
            return self._rowptr, self._pos_items
        return torch.from_numpy(self._rowptr), torch.from_numpy(self._pos_items)

    def item_log_q(self):
        """float32 [num_items] on the sampler's device: log(count_i / n), count_i the number of
        interactions (duplicates included) with item i and n their total — the logQ correction of
        an in-batch softmax, whose negatives arrive in proportion to their popularity. Computed
        in float64 on the host; an item without an interaction gets 0 (it is never a positive, so
        never read). Cached."""
        if self._log_q is None:
            items = self._item.cpu().numpy() if torch.is_tensor(self._item) else self._item
            count = np.bincount(items, minlength=self.num_items).astype(np.float64)
            q = np.zeros(self.num_items, dtype=np.float64)
            np.log(count / max(self._n, 1), out=q, where=count > 0)
            self._log_q = torch.from_numpy(q.astype(np.float32)).to(self.device)
        return self._log_q

    def neg_log_q(self):
        """float32 [num_items] on the sampler's device: the log of the probability the draw gives
        item i before the user's positives are taken out — log(w_i / W) with weights (0 for an
        item of weight 0: it is never drawn), the constant log(1 / num_items) without. The logQ
        correction of a sampled softmax over this sampler's negatives (bpr_step's neg_log_q);
        computed in float64 on the host. Cached."""
        if self._neg_log_q is None:
            if self.item_weights is None:
                q = np.full(self.num_items, np.log(1.0 / max(self.num_items, 1)))
            else:
                w = self.item_weights.astype(np.float64)
                q = np.zeros(self.num_items, dtype=np.float64)
                np.log(w / w.sum(), out=q, where=w > 0)
            self._neg_log_q = torch.from_numpy(q.astype(np.float32)).to(self.device)
        return self._neg_log_q

    def draw(self, epoch, order=None, first=0, count=None, n_neg=None):
        """(users, pos, neg): int64 tensors on the sampler's device for output slots [0, count):
        slot s is interaction order[first + s] (order: an int64 index tensor on the device, e.g. a
        permutation; None = identity). count=None: up to the end of the order. One launch on the
        current stream, no host read-back; `unsampled` is reset and counts this draw.

        n_neg=None: one negative per sample, `neg` 1-D (lgcn_bpr_sample). n_neg = an integer in
        [1, 64]: `neg` of shape [count, n_neg] (lgcn_bpr_sample_multi), column m the draw with
        counter word 3 = m — independent draws over the user's complement (the same item may come
        up twice), column 0 the one-negative draw, no column depending on n_neg; `unsampled` still
        counts slots. Anything else raises ValueError. A sampler built with weights draws every
        column by the weighted draw (lgcn_bpr_sample_weighted), the rest as stated. The draw holds count * (2 + n_neg) * 8
        bytes (a whole C3 epoch of 29.5M samples at n_neg = 16: 4.2 GB); it is one launch
        whatever n_neg."""
        n_neg = check_n_neg(n_neg, "BprSampler.draw")
        epoch = int(epoch)
        if not 0 <= epoch < 1 << 32:
            raise ValueError("BprSampler.draw: epoch must fit 32 unsigned bits")
        total = self._n if order is None else int(order.numel())
        first = int(first)
        count = total - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > total:
            raise ValueError(f"BprSampler.draw: window [{first}, {first + count}) outside the "
                             f"{total} entries")
        if self.device.type == "cuda":
            if order is not None and (not torch.is_tensor(order) or order.dtype != torch.int64
                                      or order.device != self.device or order.dim() != 1):
                raise engine.LgcnError("BprSampler.draw: order must be a 1-D int64 tensor on "
                                       f"{self.device}")
            self.unsampled.zero_()
            return sample_device(self._user, self._item,
                                 None if order is None else order.contiguous(), first, count,
                                 self._rowptr, self._pos_items, self.num_users, self.num_items,
                                 self.seed, epoch, self.unsampled, n_neg, self._cumw)
        if torch.is_tensor(order):
            order = order.numpy()
        u, p, n, missed = sample_numpy(self._user, self._item, order, first, count, self._rowptr,
                                       self._pos_items, self.num_users, self.num_items, self.seed,
                                       epoch, n_neg, self._cumw)
        self.unsampled.fill_(missed)
        return torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(n)

    def permutation(self, epoch):
        """epoch()'s shuffle: torch.randperm(len, generator=g, device=device) with g a generator
        of the sampler's device seeded (seed + SHUFFLE_MIX * epoch) mod 2^63. The order is an
        input of the draw, not part of its contract: the CPU and HIP generators give different
        permutations of the same seed, the negative of an interaction is the same under both."""
        g = torch.Generator(device=self.device)
        g.manual_seed((self.seed + SHUFFLE_MIX * int(epoch)) % (1 << 63))
        return torch.randperm(self._n, generator=g, device=self.device)

    def epoch(self, epoch, batch_size, shuffle=True, drop_last=False, n_neg=None):
        """One draw for the whole epoch (one launch), made by this call (so `unsampled` counts it
        on return), then an iterator of (users, pos, neg) views of it batch by batch: no launch,
        copy or sync per batch. The last batch is short unless drop_last. n_neg is draw()'s: with
        an integer a batch's `neg` is the [batch, n_neg] row view of the draw (contiguous), what
        bpr_step takes for negatives="hardest" / "all"; the draw then holds
        len(self) * (2 + n_neg) * 8 bytes."""
        n_neg = check_n_neg(n_neg, "BprSampler.epoch")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("BprSampler.epoch: batch_size must be positive")
        users, pos, neg = self.draw(epoch, self.permutation(epoch) if shuffle else None,
                                    n_neg=n_neg)
        end = self._n - self._n % batch_size if drop_last else self._n

        def views():
            for b in range(0, end, batch_size):
                e = min(b + batch_size, end)
                yield users[b:e], pos[b:e], neg[b:e]
        return views()
