"""engine.lean_plan on CPU tensors: the `empty` and `derived` row masks of a side-major CSR and the
per-segment empty tails, against a brute-force restatement of the two definitions:

  empty:   the row holds no stored record and no stored record names it as its column;
  derived: a side-0 row (user or brand) with exactly one stored record (p, w) such that every
           stored record naming it as its column lies in row p and carries w's value bits.

The graph (220 rows: 150 users, 60 items, 10 brands) plants every case the definitions separate."""
import numpy as np
import torch

from gcn_recommendation_amd import engine

U, I, B = 150, 60, 10
N = U + I + B
ITEM0, BRAND0 = U, U + I

# planted rows (the random part keeps off users 140.., items 50.., brands 8..)
U_SYM, U_ULP, U_DUP, U_PAIR, U_REF, U_E1, U_E2 = 140, 141, 142, 143, 144, 145, 146
I_P, I_PAIR, I_E1, I_E2, I_DIRECTED = ITEM0 + 50, ITEM0 + 51, ITEM0 + 52, ITEM0 + 53, ITEM0 + 54
B_ONE, B_EMPTY = BRAND0 + 8, BRAND0 + 9


def _records():
    """Stored records (row, col, value) in stored order; not coalesced."""
    rng = np.random.default_rng(4)
    rec = []
    for u in range(140):  # users with 1..6 items each, both directions, equal value bits
        for it in rng.choice(50, rng.integers(1, 7), replace=False):
            w = np.float32(rng.uniform(0.01, 1.0))
            rec += [(u, ITEM0 + it, w), (ITEM0 + it, u, w)]
    for b in range(8):    # the brand segment: brands over several items
        for it in rng.choice(50, 5, replace=False):
            w = np.float32(rng.uniform(0.01, 1.0))
            rec += [(BRAND0 + b, ITEM0 + it, w), (ITEM0 + it, BRAND0 + b, w)]
    w = np.float32(0.3)
    rec += [(U_SYM, I_P, w), (I_P, U_SYM, w)]                      # symmetric single edge
    rec += [(U_ULP, I_P, w), (I_P, U_ULP, np.nextafter(w, np.float32(1)))]  # reverse 1 ulp off
    rec += [(U_DUP, I_P, w), (U_DUP, I_P, w), (I_P, U_DUP, w)]     # duplicated record
    rec += [(U_PAIR, I_PAIR, w), (I_PAIR, U_PAIR, w)]              # degree 1 on both ends
    rec += [(I_DIRECTED, U_REF, w), (I_DIRECTED, 0, w)]            # U_REF: empty but referenced
    rec += [(B_ONE, I_P, w), (I_P, B_ONE, w)]                      # a single-item brand
    r, c, v = (np.array(x) for x in zip(*rec))
    order = np.argsort(r, kind="stable")                           # row-sorted, stored order kept
    return r[order].astype(np.int64), c[order].astype(np.int64), v[order].astype(np.float32)


def _slot_csr(r, c, v):
    """Side-major degree-descending slots: side 0 (users, brands) then the items."""
    deg = np.bincount(r, minlength=N)
    rows = np.arange(N)
    side1 = (rows >= ITEM0) & (rows < BRAND0)
    s0, s1 = rows[~side1], rows[side1]
    ids = np.concatenate([s0[np.argsort(-deg[s0], kind="stable")],
                          s1[np.argsort(-deg[s1], kind="stable")]])
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(deg[ids])
    start = np.searchsorted(r, ids)
    edges = np.empty(r.size, np.int64)
    for s, row in enumerate(ids):
        k = slice(start[s], start[s] + deg[row])
        bits = v[k].view(np.uint32).astype(np.int64)
        edges[rowptr[s]:rowptr[s + 1]] = (bits << 32) | c[k]
    return rowptr.astype(np.int32), edges, ids.astype(np.int32), int(s0.size)


def _brute(r, c, v):
    bits = v.view(np.uint32)
    empty = np.zeros(N, bool)
    derived = np.zeros(N, bool)
    for row in range(N):
        own = np.flatnonzero(r == row)
        named = np.flatnonzero(c == row)
        empty[row] = own.size == 0 and named.size == 0
        side0 = row < ITEM0 or row >= BRAND0
        if side0 and own.size == 1:
            p, w = c[own[0]], bits[own[0]]
            derived[row] = all(r[j] == p and bits[j] == w for j in named)
    return empty, derived


def _unpack(mask, n):
    w = mask.numpy().view(np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


def test_lean_masks_match_the_definitions():
    r, c, v = _records()
    rowptr, edges, ids, split = _slot_csr(r, c, v)
    segments = [(0, split), (split, split), (split, split), (split, N)]
    lp = engine.lean_plan(torch.from_numpy(rowptr), torch.from_numpy(edges), torch.from_numpy(ids),
                          split, segments)
    empty, derived = _brute(r, c, v)
    assert np.array_equal(_unpack(lp.empty, N), empty)
    assert np.array_equal(_unpack(lp.derived, N), derived)
    assert lp.n_empty == empty.sum() and lp.n_derived == derived.sum()
    # the planted cases, one by one
    assert derived[U_SYM] and derived[U_PAIR] and derived[B_ONE]
    assert not derived[U_ULP] and not derived[U_DUP]
    assert not derived[I_PAIR] and not derived[I_P]          # side 1 is never derived
    assert not empty[U_REF] and not derived[U_REF]
    assert empty[[U_E1, U_E2, I_E1, I_E2, B_EMPTY]].all()
    # the tails: trailing slots of each segment whose rows are all empty
    for (a, b), tail in zip(segments, lp.empty_tail):
        e = empty[ids[a:b]]
        assert e[e.size - tail:].all() and (tail == e.size or not e[e.size - tail - 1])
    assert lp.empty_tail[0] >= 3 and lp.empty_tail[3] >= 2
    assert lp.empty_tail[1] == lp.empty_tail[2] == 0
    # U_REF has no record but is referenced: it sits among side 0's degree-0 slots and ends the
    # tail wherever it falls
    s_ref = int(np.flatnonzero(ids == U_REF)[0])
    assert s_ref < split - lp.empty_tail[0]


def test_lean_struct_carries_the_tails():
    r, c, v = _records()
    rowptr, edges, ids, split = _slot_csr(r, c, v)
    segments = [(0, split), (split, split), (split, split), (split, N)]
    lp = engine.lean_plan(torch.from_numpy(rowptr), torch.from_numpy(edges), torch.from_numpy(ids),
                          split, segments)
    assert tuple(lp.struct().empty_tail) == lp.empty_tail
