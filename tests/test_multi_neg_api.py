"""Several negatives per positive without a GPU: the multi-negative draw (sampler.sample_numpy(
n_neg=M), the reference the device kernel is compared against) pinned by a scalar restatement in
plain Python ints, its invariances and edge users; BprSampler.draw / epoch shapes; the host-side
validation of lgcn_bpr_sample_multi and lgcn_bpr_select_hardest; and train.bpr_step with a [B, M]
neg on a CPU adjacency ("hardest" against an argmax made here, "all" against the expanded call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, Cfg, case_dims, load_case
from gcn_recommendation_amd import _build, engine, graph, sampler, train
from models.lightgcn import LightGCN
from sampler_cases import (EDGE_I, EDGE_LISTS, EDGE_SAMPLES, M32, edge_case, kth_missing_py,
                           philox_py, random_case)

NS = (1, 2, 5, 64)
SEED, EPOCH = 0xDEADBEEF12345678, 5


def draw_multi_py(idx, L, n_items, seed, epoch, m):
    """Ordinal m of interaction idx for a user with sorted positives L: counter word 3 = m."""
    n_free = n_items - len(L)
    if n_free <= 0:
        return -1
    o = philox_py((idx & M32, idx >> 32, epoch, m), (seed & M32, seed >> 32))
    j = (((o[1] << 32) | o[0]) * n_free) >> 64
    return kth_missing_py(L, j)


def _low(case, n_neg=None, order=None, first=0, count=None, seed=SEED, epoch=EPOCH):
    count = len(case) - first if count is None else count
    return sampler.sample_numpy(case.user, case.item, order, first, count, case.rowptr,
                                case.pos_items, case.U, case.I, seed, epoch, n_neg=n_neg)


def _cases():
    return [random_case()] + [edge_case(name) for name in EDGE_LISTS]


# ---- the draw ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", NS)
def test_numpy_path_equals_scalar_restatement(M):
    for c in _cases():
        users, pos, neg, missed = _low(c, M)
        assert neg.shape == (len(c), M) and neg.dtype == np.int64
        assert np.array_equal(users, c.user) and np.array_equal(pos, c.item)
        lists = [c.positives(u) for u in range(c.U)]
        want = [[draw_multi_py(i, lists[int(c.user[i])], c.I, SEED, EPOCH, m) for m in range(M)]
                for i in range(len(c))]
        assert neg.tolist() == want
        full = sum(1 for i in range(len(c)) if len(lists[int(c.user[i])]) >= c.I)
        assert missed == full
        for i in range(len(c)):  # every entry lies in the user's complement
            L = lists[int(c.user[i])]
            if len(L) < c.I:
                assert all(0 <= x < c.I and x not in L for x in want[i])


def test_column_zero_is_the_one_negative_draw():
    for c in _cases():
        u1, p1, n1, m1 = _low(c)
        assert n1.shape == (len(c),)
        for M in NS:
            u, p, n, m = _low(c, M)
            assert np.array_equal(n[:, 0], n1) and m == m1
            assert np.array_equal(u, u1) and np.array_equal(p, p1)


def test_column_does_not_depend_on_n_neg_order_or_window():
    c = random_case()
    wide = _low(c, 64)[2]
    for m in (0, 1, 4, 63):
        assert np.array_equal(_low(c, m + 1)[2][:, m], wide[:, m])
    order = np.random.default_rng(1).permutation(len(c))
    for M in (3, 64):
        got = _low(c, M, order=order)
        assert np.array_equal(got[2], wide[order][:, :M])
        assert np.array_equal(got[0], c.user[order])
        win = _low(c, M, first=37, count=101)[2]
        assert np.array_equal(win, wide[37:138, :M])
        win = _low(c, M, order=order, first=590, count=10)[2]
        assert np.array_equal(win, wide[order[590:600], :M])
    assert _low(c, 5, count=0)[2].shape == (0, 5)


def test_edge_users():
    c = edge_case("full")
    users, pos, neg, missed = _low(c, 64)
    edge = c.user == 1
    assert (neg[edge] == -1).all() and missed == EDGE_SAMPLES == int(edge.sum())
    assert (neg[~edge] >= 0).all() and (users >= 0).all()
    c = edge_case("free_middle")
    neg = _low(c, 64)[2]
    assert (neg[c.user == 1] == 4).all()
    c = edge_case("deg0")  # 9 free items, 200 x 64 draws: every one of them comes up
    neg = _low(c, 64)[2][c.user == 1]
    assert neg.shape == (EDGE_SAMPLES, 64)
    assert sorted(np.unique(neg).tolist()) == list(range(EDGE_I))


def test_ordinals_are_different_draws():
    neg = _low(random_case(), 64)[2]
    assert (neg != neg[:, :1]).any(axis=1).any()
    assert (neg != neg[:, :1]).any(axis=1).sum() > len(neg) // 2


def test_invalid_slots_are_minus_one_in_every_entry():
    c = random_case()
    order = np.array([0, -1, len(c), 5, 1 << 40], dtype=np.int64)
    u, p, n, missed = _low(c, 3, order=order, count=5)
    assert u.tolist()[1:3] == [-1, -1] and p.tolist()[1:3] == [-1, -1] and u[4] == -1
    assert (n[[1, 2, 4]] == -1).all() and (n[[0, 3]] >= 0).all() and missed == 0


# ---- BprSampler ---------------------------------------------------------------------------------
def test_draw_and_epoch_shapes_and_validation():
    c = random_case()
    s = sampler.BprSampler(c.user, c.item, c.U, c.I, "cpu", seed=9)
    u, p, n = s.draw(2)
    assert n.shape == (600,) and n.dtype == torch.int64
    u1, p1, n1 = s.draw(2, n_neg=1)
    assert n1.shape == (600, 1) and torch.equal(n1[:, 0], n) and torch.equal(u1, u)
    u5, p5, n5 = s.draw(2, n_neg=5, first=10, count=20)
    assert n5.shape == (20, 5) and torch.equal(n5[:, :1], n1[10:30])
    want = _low(c, 5, seed=9, epoch=2)[2]
    assert np.array_equal(s.draw(2, n_neg=5)[2].numpy(), want)
    for bad in (0, 65, -1, 2.0, "4", True):
        with pytest.raises(ValueError):
            s.draw(2, n_neg=bad)
        with pytest.raises(ValueError):
            s.epoch(2, 64, n_neg=bad)
        with pytest.raises(ValueError):
            _low(c, bad)
    batches = list(s.epoch(3, 128, shuffle=False, n_neg=4))
    assert [tuple(b[2].shape) for b in batches] == [(128, 4)] * 4 + [(88, 4)]
    assert all(b[2].is_contiguous() and b[0].shape == (b[2].shape[0],) for b in batches)
    whole = s.draw(3, n_neg=4)[2]
    assert torch.equal(torch.cat([b[2] for b in batches]), whole)
    assert torch.equal(torch.cat([b[2][:, 0] for b in batches]),
                       torch.cat([b[2] for b in s.epoch(3, 128, shuffle=False)]))
    one = list(s.epoch(3, 128, shuffle=False))
    assert one[0][2].shape == (128,)
    perm = s.permutation(3)
    shuffled = torch.cat([b[2] for b in s.epoch(3, 100, n_neg=4)])
    assert torch.equal(shuffled, whole[perm])
    # user 0 has every item: its three samples are left without a negative, counted per slot
    s = sampler.BprSampler([0, 0, 0, 1], [0, 1, 2, 1], 2, 3, "cpu")
    neg = s.draw(0, n_neg=7)[2]
    assert s.unsampled.item() == 3 and (neg[:3] == -1).all() and (neg[3] >= 0).all()


# ---- host-side validation of the two C entry points ----------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


def test_sample_multi_validates_arguments_without_gpu(lib):
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host

    def call(iu=p, ii=p, n_inter=10, first=0, count=4, rowptr=p, items=p, U=5, I=7, n_neg=4,
             users=p, pos=p, neg=p):
        return lib.lgcn_bpr_sample_multi(iu, ii, n_inter, None, first, count, rowptr, items, U, I,
                                         ctypes.c_uint64(1), ctypes.c_uint32(0), n_neg, users, pos,
                                         neg, None, None)

    for bad in (dict(n_neg=0), dict(n_neg=65), dict(n_neg=-3), dict(count=-1), dict(first=-1),
                dict(iu=None), dict(ii=None), dict(rowptr=None), dict(items=None),
                dict(users=None), dict(pos=None), dict(neg=None), dict(n_inter=-1),
                dict(U=1 << 31), dict(I=1 << 31), dict(count=(1 << 62), n_neg=2),
                dict(count=(1 << 63) - 1, first=1)):
        assert call(**bad) == -1, bad   # LGCN_EINVAL
    none = dict(iu=None, ii=None, rowptr=None, items=None, users=None, pos=None, neg=None)
    assert call(count=0, **none) == 0
    assert call(count=0, n_neg=65, **none) == -1   # the sizes are checked first
    assert engine.BPR_MAX_NEG == sampler.MAX_NEG == 64


def test_select_hardest_validates_arguments_without_gpu(lib):
    p = ctypes.c_void_p(256)

    def call(fu=p, ld_fu=64, fi=p, ld_fi=64, U=10, I=10, users=p, cand=p, B=4, n_neg=4, d=64,
             out=p, score=None):
        return lib.lgcn_bpr_select_hardest(fu, ld_fu, fi, ld_fi, U, I, users, cand, B, n_neg, d,
                                           out, score, None)

    for bad in (dict(n_neg=0), dict(n_neg=65), dict(B=-1), dict(d=0), dict(ld_fu=63),
                dict(ld_fi=63), dict(U=-1), dict(I=-1), dict(fu=None), dict(fi=None),
                dict(users=None), dict(cand=None), dict(out=None)):
        assert call(**bad) == -1, bad
    none = dict(fu=None, fi=None, users=None, cand=None, out=None)
    assert call(B=0, **none) == 0
    assert call(B=0, n_neg=0, **none) == -1
    header = open(os.path.join(ROOT, "include", "lgcn.h")).read()
    assert "#define LGCN_BPR_MAX_NEG 64" in header


# ---- bpr_step with a [B, M] neg on a CPU adjacency -----------------------------------------------
LAMBDA = 1e-4


def _setup(batch=128, M=4, name="c1_brand"):
    z = load_case(name)
    U, I, B, d, K = case_dims(z)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]))
    g = torch.Generator().manual_seed(23)
    bu, bp = (torch.randint(0, n, (batch,), generator=g) for n in (U, I))
    cand = torch.randint(0, I, (batch, M), generator=g)
    return z, adj, bu, bp, cand


def _model(z):
    U, I, B, d, K = case_dims(z)
    torch.manual_seed(42)
    return LightGCN(U, I, B, Cfg(d, K))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32),
                                              b.detach().view(torch.int32))


def _assert_same_step(a, b, la, lb):
    la.backward()
    lb.backward()
    assert _same_bits(la, lb)
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert ga[k].grad is not None and _same_bits(ga[k].grad, gb[k].grad), k


def test_cpu_hardest_is_the_step_on_the_argmax():
    z, adj, bu, bp, cand = _setup()
    cand[3, 1] = cand[3, 0]   # the same item twice: still the first maximum
    cand[5, 0] = -1           # a candidate out of range is passed over
    cand[6, 2] = case_dims(z)[1]
    a, b = _model(z), _model(z)
    with torch.no_grad():
        fu, fi = a(adj)[:2]
        scores = (fu[bu].unsqueeze(1) * fi[cand.clamp(0, fi.shape[0] - 1)]).sum(-1)
        scores[5, 0] = scores[6, 2] = -float("inf")
        pick = cand.gather(1, scores.argmax(1, keepdim=True)).squeeze(1)  # argmax: the first max
    want = a.bpr_step(adj, bu, bp, pick, LAMBDA)
    got, used = b.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="hardest", return_negatives=True)
    assert torch.equal(used, pick) and used.dtype == torch.int64
    assert (pick != cand[:, 0]).any()
    _assert_same_step(a, b, want, got)
    # the default mode is "hardest"; a 1-D neg ignores the keyword and hands neg back
    c = _model(z)
    again = train.bpr_step(c, adj, bu, bp, cand, LAMBDA, check_indices=False)
    assert _same_bits(again, want)
    loss, used = train.bpr_step(c, adj, bu, bp, pick, LAMBDA, negatives="whatever",
                                return_negatives=True)
    assert _same_bits(loss, want) and used is pick


def test_cpu_all_is_the_expanded_call():
    z, adj, bu, bp, cand = _setup(batch=64, M=3)
    a, b = _model(z), _model(z)
    want = a.bpr_step(adj, bu.repeat_interleave(3), bp.repeat_interleave(3), cand.reshape(-1),
                      LAMBDA)
    got, used = b.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="all", return_negatives=True)
    assert torch.equal(used, cand.reshape(-1))
    _assert_same_step(a, b, want, got)


def test_cpu_step_refusals():
    z, adj, bu, bp, cand = _setup(batch=16, M=4)
    I = case_dims(z)[1]
    m = _model(z)
    lost = cand.clone()
    lost[7] = -1
    with pytest.raises(engine.LgcnError):
        m.bpr_step(adj, bu, bp, lost, LAMBDA)
    for bad in ("hard", "", None, "ALL"):
        with pytest.raises(ValueError):
            m.bpr_step(adj, bu, bp, cand, LAMBDA, negatives=bad)
    wide = torch.zeros((16, 8), dtype=torch.int64)
    for bad in (wide[:, ::2], cand.view(16, 2, 2), cand.to(torch.int32), cand[:8],
                torch.zeros((16, 65), dtype=torch.int64), torch.zeros((16, 0), dtype=torch.int64),
                cand.t().contiguous().t()):
        with pytest.raises(engine.LgcnError):
            m.bpr_step(adj, bu, bp, bad, LAMBDA)
    high = cand.clone()
    high[2, 3] = I
    with pytest.raises(engine.LgcnError):
        train.bpr_step(m, adj, bu, bp, high, LAMBDA, check_indices=True)
    assert np.isfinite(train.bpr_step(m, adj, bu, bp, high, LAMBDA).item())  # passed over
    assert np.isfinite(train.bpr_step(m, adj, bu, bp, cand, LAMBDA, check_indices=True).item())


def test_cpu_epoch_with_candidates_equals_the_hand_loop():
    z = load_case("c1_brand")
    U, I, B, d, K = case_dims(z)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]))
    n = min(len(z["train_user"]), 600)
    s = sampler.BprSampler(z["train_user"][:n], z["train_item"][:n], U, I, "cpu", seed=4)
    a, b = _model(z), _model(z)
    oa, ob = (torch.optim.Adam(m.parameters(), lr=1e-3) for m in (a, b))
    got = a.bpr_epoch(adj, s, oa, LAMBDA, 256, 1, n_neg=4)
    want = []
    for bu, bp, cand in s.epoch(1, 256, n_neg=4):
        ob.zero_grad()
        loss = b.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="hardest")
        loss.backward()
        ob.step()
        want.append(loss.detach())
    assert _same_bits(got, torch.stack(want))
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert _same_bits(p, q), k
    with pytest.raises(ValueError):
        a.bpr_epoch(adj, s, oa, LAMBDA, 256, 1, n_neg=4, negatives="most")
