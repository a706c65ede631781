"""engine.shared_plan on CPU tensors: the groups of single-record side-0 rows that can share one
layer row, their representatives, the partitioned slot order and the two re-written edge arrays,
against a brute-force restatement:

  start set: side-0 rows with exactly one stored record (p, w) such that every stored record
             naming them lies in row p with w's value bits (LeanPlan.derived);
  group:     the rows of the start set with equal (p, value bits of w);
  representative: the group's member in the lowest slot; every other member is shared.

The graph (150 users, 60 items, 10 brands, side-major degree-descending slots as
test_lean_plan.py builds them) plants every case the definitions separate."""
import numpy as np
import torch

from gcn_recommendation_amd import engine

from test_lean_plan import BRAND0, ITEM0, N, _slot_csr

# planted rows (the random part keeps off users 120.., items 50.., brands 8..)
GROUP_A = [121, 123, 126]          # item I_P, w = 0.3 (+ the brand B_ONE)
GROUP_B = [122, 125]               # item I_P, w = 0.5: a second group on the same item
U_ALONE = 127                      # item I_Q's only single-record user: a group of size 1
U_ULP_W = 128                      # item I_P, w one ulp above 0.3, both directions: its own group
U_ULP_BACK = 129                   # item I_P, w = 0.3 but the reverse record one ulp off
U_DUP = 130                        # item I_P, the record stored twice
I_P, I_Q = ITEM0 + 50, ITEM0 + 51
B_ONE = BRAND0 + 8                 # a single-item brand on I_P with w = 0.3: joins group A
W_A, W_B = np.float32(0.3), np.float32(0.5)


def _records():
    rng = np.random.default_rng(11)
    rec = []
    for u in range(120):  # users with 2..6 items each, both directions, equal value bits
        for it in rng.choice(50, rng.integers(2, 7), replace=False):
            w = np.float32(rng.uniform(0.01, 1.0))
            rec += [(u, ITEM0 + it, w), (ITEM0 + it, u, w)]
    for b in range(8):
        for it in rng.choice(50, 5, replace=False):
            w = np.float32(rng.uniform(0.01, 1.0))
            rec += [(BRAND0 + b, ITEM0 + it, w), (ITEM0 + it, BRAND0 + b, w)]
    for u in GROUP_A + [B_ONE]:
        rec += [(u, I_P, W_A), (I_P, u, W_A)]
    for u in GROUP_B:
        rec += [(u, I_P, W_B), (I_P, u, W_B)]
    rec += [(U_ALONE, I_Q, W_A), (I_Q, U_ALONE, W_A), (0, I_Q, W_B), (I_Q, 0, W_B)]
    up = np.nextafter(W_A, np.float32(1))
    rec += [(U_ULP_W, I_P, up), (I_P, U_ULP_W, up)]
    rec += [(U_ULP_BACK, I_P, W_A), (I_P, U_ULP_BACK, up)]
    rec += [(U_DUP, I_P, W_A), (U_DUP, I_P, W_A), (I_P, U_DUP, W_A)]
    r, c, v = (np.array(x) for x in zip(*rec))
    order = np.argsort(r, kind="stable")
    return r[order].astype(np.int64), c[order].astype(np.int64), v[order].astype(np.float32)


def _plans(segments=None):
    r, c, v = _records()
    rowptr, edges, ids, split = _slot_csr(r, c, v)
    segments = segments or [(0, split), (split, split), (split, split), (split, N)]
    t = [torch.from_numpy(a) for a in (rowptr, edges, ids)]
    lp = engine.lean_plan(*t, split, segments)
    keep = [a.clone() for a in t]
    sp = engine.shared_plan(*t, split, segments, lp)
    assert all(torch.equal(a, b) for a, b in zip(t, keep))   # the graph's arrays are not mutated
    return (r, c, v), (rowptr, edges, ids, split), lp, sp


def _brute(r, c, v, ids):
    """{(p, bits): members in slot order} over the start set."""
    bits = v.view(np.uint32)
    slot_of = np.empty(N, np.int64)
    slot_of[ids] = np.arange(N)
    groups = {}
    for row in list(range(ITEM0)) + list(range(BRAND0, N)):
        own = np.flatnonzero(r == row)
        if own.size != 1:
            continue
        p, w = int(c[own[0]]), int(bits[own[0]])
        if all(r[j] == p and bits[j] == w for j in np.flatnonzero(c == row)):
            groups.setdefault((p, w), []).append(row)
    return {k: sorted(m, key=lambda x: slot_of[x]) for k, m in groups.items()}


def test_groups_and_representatives_match_the_definitions():
    (r, c, v), (rowptr, edges, ids, split), lp, sp = _plans()
    groups = _brute(r, c, v, ids)
    want_rep = {u: m[0] for m in groups.values() for u in m[1:]}
    got = dict(zip(sp.shared_rows().tolist(), sp.rep.tolist()))
    assert got == want_rep
    assert sp.n_shared == len(want_rep) == sum(sp.shared_tail) and sp.n_groups == len(groups)
    assert sp.rep.dtype == torch.int32
    bits = lambda w: int(np.float32(w).view(np.uint32))
    # two groups of different value bits on one item; the single-record brand takes part
    a, b = groups[(I_P, bits(W_A))], groups[(I_P, bits(W_B))]
    assert sorted(a) == sorted(GROUP_A + [B_ONE]) and sorted(b) == sorted(GROUP_B)
    assert B_ONE in got or a[0] == B_ONE
    assert {got[u] for u in a[1:]} == {a[0]} and {got[u] for u in b[1:]} == {b[0]}
    # a group of size 1 has no shared row
    assert groups[(I_Q, bits(W_A))] == [U_ALONE] and U_ALONE not in got
    assert U_ALONE not in got.values()
    # one ulp off in its own value: a group of its own; one ulp off in the reverse record, or a
    # duplicated record: not in the start set at all
    assert groups[(I_P, bits(np.nextafter(W_A, np.float32(1))))] == [U_ULP_W]
    for u in (U_ULP_W, U_ULP_BACK, U_DUP):
        assert u not in got and u not in got.values()
    assert not any(U_ULP_BACK in m or U_DUP in m for m in groups.values())


def test_slots_are_partitioned_inside_the_single_record_range():
    (r, c, v), (rowptr, edges, ids, split), lp, sp = _plans()
    ids_s = sp.row_ids_s.numpy()
    assert np.array_equal(np.sort(ids_s), np.arange(N))
    deg = np.diff(rowptr)
    one = np.flatnonzero(deg[:split] == 1)
    s0, s1 = one[0], one[-1] + 1
    assert s1 - s0 == one.size
    outside = np.ones(N, bool)
    outside[s0:s1] = False
    assert np.array_equal(ids_s[outside], ids[outside]) and not np.array_equal(ids_s, ids)
    # the shared rows are that range's tail, directly before the empty tail
    assert s1 == split - lp.empty_tail[0] and lp.empty_tail[0] > 0
    assert sp.tail_slots[0] == (s1 - sp.n_shared, s1) and sp.shared_tail == (sp.n_shared, 0, 0, 0)
    shared = np.zeros(N, bool)
    shared[sp.shared_rows().numpy()] = True
    assert shared[ids_s[s1 - sp.n_shared:s1]].all() and not shared[ids_s[:s1 - sp.n_shared]].any()
    # a stable partition: both parts keep their order
    assert np.array_equal(ids_s[s0:s1 - sp.n_shared], ids[s0:s1][~shared[ids[s0:s1]]])
    assert np.array_equal(ids_s[s1 - sp.n_shared:s1], ids[s0:s1][shared[ids[s0:s1]]])
    # edges_l1: every slot still holds its row's record
    e1 = sp.edges_l1.numpy()
    where = {row: s for s, row in enumerate(ids)}
    for s in range(N):
        old = where[ids_s[s]]
        assert np.array_equal(e1[rowptr[s]:rowptr[s + 1]], edges[rowptr[old]:rowptr[old + 1]])


def test_re_pointed_columns():
    (r, c, v), (rowptr, edges, ids, split), lp, sp = _plans()
    e1, en = sp.edges_l1.numpy(), sp.edges_ln.numpy()
    rep = dict(zip(sp.shared_rows().tolist(), sp.rep.tolist()))
    assert np.array_equal(e1 >> 32, en >> 32)                # no value bit changes
    side0 = slice(0, rowptr[split])
    assert np.array_equal(e1[side0], en[side0])              # side 0's records are equal
    c1, cn = e1 & 0xffffffff, en & 0xffffffff
    want = np.array([rep.get(int(x), int(x)) for x in c1])   # same position, representative
    assert np.array_equal(cn, want) and (c1 != cn).sum() == sp.n_shared
    assert not np.isin(cn, list(rep)).any()


def test_three_side0_segments_turn_sharing_off():
    """LGCN_CLASSES=1: side 0 runs as three segments and nothing is shared."""
    _, (rowptr, edges, ids, split), _, _ = _plans()
    segments = [(0, 40), (40, 90), (90, split), (split, N)]
    _, _, lp, sp = _plans(segments)
    assert sp.shared_tail == (0, 0, 0, 0) and sp.n_shared == 0 and sp.rep.numel() == 0
    assert torch.equal(sp.row_ids_s, torch.from_numpy(ids))
    assert torch.equal(sp.edges_l1, torch.from_numpy(edges))
    assert torch.equal(sp.edges_ln, torch.from_numpy(edges))
    assert sp.empty_tail == lp.empty_tail


def test_struct_carries_the_tails():
    _, _, lp, sp = _plans()
    st = sp.struct()
    assert tuple(st.shared_tail) == sp.shared_tail and tuple(st.empty_tail) == lp.empty_tail
    assert st.row_ids == sp.row_ids_s.data_ptr() and st.rep == sp.rep.data_ptr()
    assert st.edges_l1 == sp.edges_l1.data_ptr() and st.edges_ln == sp.edges_ln.data_ptr()
