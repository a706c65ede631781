"""The rank evaluation without a GPU (gcn_recommendation_amd/evaluate.py: metrics_from_ranks,
rank_torch, Evaluator on a CPU device; lgcn_score_rank's host-side validation): the metrics
against values worked out by hand, rank_torch against tests/eval_cases.py's rank_ref on float64
scores, the Evaluator end to end against a loop written after main.py:404-439, and everything the
Python layer and the C entry point refuse before a launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import Cfg
from eval_cases import assert_exact, few_bits, random_mask, rank_ref
from gcn_recommendation_amd import _build, engine, evaluate as E, graph, sampler
from util import MASKED, masked_scores64

EINVAL, EALIGN = -1, -2  # include/lgcn.h


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


# ----------------------------------------------------------------------------------------------
# metrics_from_ranks
# ----------------------------------------------------------------------------------------------
def test_metrics_by_hand():
    ranks = np.array([0, 19, 20, -1, 4], np.int32)  # first, k - 1, k, no rank, inside
    m = E.metrics_from_ranks(ranks, ks=(1, 5, 20, 21))
    assert sorted(m) == sorted(["mrr"] + [f"{n}@{k}" for n in ("recall", "ndcg")
                                          for k in (1, 5, 20, 21)])
    assert all(type(v) is float for v in m.values())
    assert m["recall@1"] == 0.2 and m["ndcg@1"] == 0.2
    assert m["recall@5"] == 0.4
    assert m["ndcg@5"] == pytest.approx((1 + 1 / math.log2(6)) / 5, rel=1e-15)
    assert m["recall@20"] == 0.6          # rank 19 is the last hit, rank 20 the first miss
    assert m["ndcg@20"] == pytest.approx((1 + 1 / math.log2(21) + 1 / math.log2(6)) / 5, rel=1e-15)
    assert m["recall@21"] == 0.8
    assert m["ndcg@21"] == pytest.approx(
        (1 + 1 / math.log2(21) + 1 / math.log2(22) + 1 / math.log2(6)) / 5, rel=1e-15)
    assert m["mrr"] == pytest.approx((1 + 1 / 20 + 1 / 21 + 0 + 1 / 5) / 5, rel=1e-15)
    # the very expressions evaluate() uses, to the bit
    assert m["ndcg@20"] == float(np.array([1.0, 1.0 / np.log2(19 + 2), 0.0, 0.0,
                                           1.0 / np.log2(4 + 2)]).mean())
    # a tensor, a list, int64: the same numbers
    for other in (torch.from_numpy(ranks), ranks.tolist(), ranks.astype(np.int64)):
        assert E.metrics_from_ranks(other, ks=(1, 5, 20, 21)) == m
    assert E.metrics_from_ranks(ranks) == {k: m[k] for k in ("recall@20", "ndcg@20", "mrr")}


def test_metrics_edges():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no mean of an empty slice, no division by zero
        m = E.metrics_from_ranks(np.zeros(0, np.int32), ks=(20, 50))
        assert sorted(m) == ["mrr", "ndcg@20", "ndcg@50", "recall@20", "recall@50"]
        assert all(math.isnan(v) for v in m.values())
        m = E.metrics_from_ranks(torch.zeros(0, dtype=torch.int32))
        assert all(math.isnan(v) for v in m.values())
        miss = E.metrics_from_ranks([-1, -1, -1], ks=(1, 1000))
        assert set(miss.values()) == {0.0}
        first = E.metrics_from_ranks([0, 0], ks=(1, 20))
        assert set(first.values()) == {1.0}
        big = E.metrics_from_ranks([2 ** 31 - 2], ks=(20, 2 ** 31 - 1))
        assert big["recall@20"] == 0.0 and big[f"recall@{2 ** 31 - 1}"] == 1.0
        assert big["mrr"] == 1.0 / (2 ** 31 - 1)


# ----------------------------------------------------------------------------------------------
# rank_torch on CPU tensors
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64])
def test_rank_torch_cpu_matches_reference(d):
    rng = np.random.default_rng(300 + d)
    U, I = 60, 500
    ue, ie = few_bits(rng, U, d), few_bits(rng, I, d)
    ie[100:104] = ie[97]  # equal rows around a target: the index tie-break
    mrow, mit = random_mask(rng, U, I, 6)
    users = rng.integers(0, U, 90)
    targets = rng.integers(0, I, 90)
    targets[:4] = [100, 97, 103, 101]
    for b in range(10, 20):  # the target itself a train item
        lst = mit[mrow[users[b]]:mrow[users[b] + 1]]
        if lst.size:
            targets[b] = lst[b % lst.size]
    targets[20], targets[21], targets[22] = -1, I, 2 ** 40  # no such item
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    want = rank_ref(full, targets)
    inside = (targets >= 0) & (targets < I)
    assert (want[~inside] == -1).all() and (~inside).sum() == 3
    masked_target = full[np.arange(90), np.where(inside, targets, 0)] == MASKED
    assert (masked_target & inside).sum() >= 5
    # ties are what the input is for
    assert np.mean([(full[b] == full[b, targets[b]]).sum() > 1 for b in np.nonzero(inside)[0]]) > .8
    uet, iet = torch.from_numpy(ue), torch.from_numpy(ie)
    for bs in (1024, 7):
        for us, ts_, mr, mi in ((users, targets, mrow, mit),
                                (torch.from_numpy(users), torch.from_numpy(targets),
                                 torch.from_numpy(mrow), torch.from_numpy(mit))):
            r, s = E.rank_torch(uet, iet, us, ts_, mr, mi, batch_size=bs)
            assert r.dtype == torch.int32 and s.dtype == torch.float32 and r.shape == s.shape == (90,)
            assert np.array_equal(r.numpy(), want)
            s = s.numpy()
            assert np.isnan(s[~inside]).all()
            assert np.array_equal(s[inside], full[inside, targets[inside]].astype(np.float32))
    # no users, no items
    r, s = E.rank_torch(uet, iet, [], [], mrow, mit)
    assert r.shape == s.shape == (0,) and r.dtype == torch.int32
    r, s = E.rank_torch(uet, iet[:0], users[:5], targets[:5], np.zeros(U + 1, np.int32), [])
    assert r.tolist() == [-1] * 5 and np.isnan(s.numpy()).all()


# ----------------------------------------------------------------------------------------------
# Evaluator on a CPU device, end to end
# ----------------------------------------------------------------------------------------------
def _evaluate_by_hand(model, eval_users, eval_items, train_users, train_items, adj, k):
    """main.py:404-439 written out: one held-out item per user (the last pair of a user wins),
    scores by matmul, the user's train items at -1e10, topk, hit -> 1 and 1 / log2(pos + 2)."""
    held = {}
    for u, i in zip(eval_users, eval_items):
        held[int(u)] = int(i)
    seen = {}
    for u, i in zip(train_users, train_items):
        seen.setdefault(int(u), []).append(int(i))
    model.eval()
    recalls, ndcgs = [], []
    with torch.no_grad():
        fu, fi = model(adj)[:2]
        order = list(held)
        scores = fu[torch.tensor(order, dtype=torch.long)] @ fi.T
        for j, u in enumerate(order):
            if u in seen:
                scores[j, seen[u]] = -1e10
        top = torch.topk(scores, k=k)[1].numpy()
    for j, u in enumerate(order):
        where = np.nonzero(top[j] == held[u])[0]
        recalls.append(1 if where.size else 0)
        ndcgs.append(1 / np.log2(where[0] + 2) if where.size else 0)
    return float(np.mean(recalls)), float(np.mean(ndcgs)), scores.numpy(), order


def test_evaluator_cpu_end_to_end():
    import pandas as pd
    from models.lightgcn import LightGCN
    rng = np.random.default_rng(17)
    U, I, B, d, K, k = 70, 90, 0, 12, 2, 20
    tu, ti = rng.integers(0, U, 400), rng.integers(0, I, 400)
    adj = graph.build_norm_adj(tu, ti, U, I, B, use_brand=False)
    torch.manual_seed(5)
    model = LightGCN(U, I, B, Cfg(d, K))
    with torch.no_grad():  # the reference's initial scale gives scores too close to tell apart
        model.user_embedding.weight.mul_(30.0)
        model.item_embedding.weight.mul_(30.0)
    # 80 pairs for 70 users: some users twice (the last pair wins), some never
    vu, vi = rng.integers(0, U, 80), rng.integers(0, I, 80)
    assert len(set(vu.tolist())) < 80
    val = pd.DataFrame({"user_idx": vu, "item_idx": vi})
    rec, ndcg, scores, order = _evaluate_by_hand(model, vu, vi, tu, ti, adj, k)
    # torch.topk fixes no order among equal scores: the comparison needs a row without ties
    # (the train items' -1e10 aside, which only matter to a target that is one)
    for j in range(len(order)):
        live = scores[j][scores[j] != np.float32(-1e10)]
        assert np.unique(live).size == live.size
    assert 0.1 < rec < 0.9 and 0 < ndcg < rec

    ev = E.Evaluator(tu, ti, U, I, "cpu")
    got = ev.evaluate(model, adj, val, ks=(k,))
    assert (got["recall@20"], got["ndcg@20"]) == (rec, ndcg)
    assert not model.training
    # a pair of arrays (already one item per user), the model's method, several k at once
    held = dict(zip(vu.tolist(), vi.tolist()))
    pu, pi = np.array(list(held)), np.array(list(held.values()))
    assert ev.evaluate(model, adj, (pu, pi), ks=(k,)) == got
    assert model.evaluate_ranks(adj, ev, pu, pi, ks=(k,)) == got
    ranks = ev.ranks(model, adj, pu, pi)
    assert ranks.dtype == torch.int32 and ranks.device.type == "cpu" and ranks.shape == pu.shape
    mrow, mit = E.mask_csr(tu, ti, U)
    with torch.no_grad():
        fu, fi = model(adj)[:2]
    want = rank_ref(masked_scores64(fu.numpy(), fi.numpy(), pu, mrow, mit), pi)
    unmasked = np.array([i not in mit[mrow[u]:mrow[u + 1]] for u, i in zip(pu, pi)])
    # (float64 and fp32 scores order a tie-free row alike unless two scores meet within rounding:
    # the by-hand metrics above are the exact check, this one names the ranks)
    assert (ranks.numpy()[unmasked] == want[unmasked]).mean() > 0.9
    many = ev.evaluate(model, adj, (pu, pi), ks=(1, 5, 20, 90))
    assert many == E.metrics_from_ranks(ranks, ks=(1, 5, 20, 90))
    assert many["recall@1"] <= many["recall@5"] <= many["recall@20"] <= many["recall@90"]
    # small batches give the same ranks; so does the sampler's CSR, which is held and not copied
    assert torch.equal(ev.ranks(model, adj, pu, pi, batch_size=16), ranks)
    s = sampler.BprSampler(tu, ti, U, I, "cpu")
    ev2 = E.Evaluator.from_sampler(s)
    assert ev2._rowptr.data_ptr() == s._rowptr.ctypes.data
    assert ev2._items.data_ptr() == s._pos_items.ctypes.data
    assert torch.equal(ev2.ranks(model, adj, pu, pi), ranks)
    # no held-out pair at all
    empty = ev.evaluate(model, adj, val.iloc[:0])
    assert all(math.isnan(v) for v in empty.values())


# ----------------------------------------------------------------------------------------------
# refusals before any launch
# ----------------------------------------------------------------------------------------------
class _Tables(torch.nn.Module):
    def __init__(self, ue, ie):
        super().__init__()
        self.ue, self.ie = ue, ie

    def forward(self, adj):
        return self.ue, self.ie, None, None, None


def test_python_layer_refuses_bad_arguments():
    U, I, d = 6, 9, 64
    ue, ie = torch.zeros(U, d), torch.zeros(I, d)
    mrow, mit = E.mask_csr([0, 1], [2, 3], U)
    users, targets = np.arange(4), np.arange(4)
    # rank_fused is the HIP kernel: CPU tables are refused, not sent to another path
    with pytest.raises(engine.LgcnError):
        E.rank_fused(ue, ie, users, targets, mrow, mit)
    for fn in (E.rank_fused, E.rank_torch):
        with pytest.raises(engine.LgcnError):
            fn(ue.double(), ie.double(), users, targets, mrow, mit)
        with pytest.raises(engine.LgcnError):
            fn(ue, ie[:, :32], users, targets, mrow, mit)
        with pytest.raises(engine.LgcnError):
            fn(ue[0], ie, users, targets, mrow, mit)
    with pytest.raises(ValueError):
        E.rank_torch(ue, ie, users, targets[:3], mrow, mit)
    with pytest.raises(ValueError):
        E.rank_torch(ue, ie, users, targets, mrow[:-1], mit)
    with pytest.raises(ValueError):
        E.rank_torch(ue, ie, users[None, :], targets[None, :], mrow, mit)
    with pytest.raises(engine.LgcnError):
        E.rank_torch(ue, ie, users.astype(np.float32), targets, mrow, mit)
    with pytest.raises(engine.LgcnError):
        E.rank_torch(ue, ie, torch.arange(4, dtype=torch.int16), targets, mrow, mit)
    with pytest.raises(engine.LgcnError):  # a mask tensor must already be int32
        E.rank_torch(ue, ie, users, targets, torch.from_numpy(mrow).long(), mit)

    with pytest.raises(ValueError):
        E.Evaluator([0, 1], [2], U, I, "cpu")
    with pytest.raises(ValueError):
        E.Evaluator([0, U], [2, 3], U, I, "cpu")
    with pytest.raises(ValueError):
        E.Evaluator([0, 1], [2, -1], U, I, "cpu")
    with pytest.raises(ValueError):
        E.Evaluator([0, 1], [2, 3], 2 ** 31, I, "cpu")
    ev = E.Evaluator([0, 1], [2, 3], U, I, "cpu")
    model = _Tables(ue, ie)
    with pytest.raises(ValueError):
        ev.ranks(model, None, users, targets[:3])
    with pytest.raises(ValueError):
        ev.ranks(model, None, users, targets, batch_size=0)
    with pytest.raises(engine.LgcnError):
        ev.ranks(model, None, users.astype(np.float64), targets)
    with pytest.raises(engine.LgcnError):  # an evaluator of another graph
        ev.ranks(_Tables(ue[:5], ie), None, users, targets)
    with pytest.raises(engine.LgcnError):
        ev.ranks(_Tables(ue.double(), ie.double()), None, users, targets)
    # and what is fine: pairs outside the tables rank -1
    r = ev.ranks(model, None, [0, U, -1, 2], [0, 1, 1, I])
    assert r.tolist() == [0, -1, -1, -1]


# ----------------------------------------------------------------------------------------------
# lgcn_score_rank: everything it refuses before its first HIP call
# ----------------------------------------------------------------------------------------------
def _rank_call(lib):
    p = ctypes.c_void_p(256)  # 16-B aligned, never dereferenced: every call is refused on the host

    def call(ue=p, ld_u=64, users=p, n_users=4, ie=p, ld_i=64, n_items=100, d=64, mrow=p, mit=p,
             targets=p, n_splits=1, part=p, score=p, rank=p):
        return lib.lgcn_score_rank(ue, ld_u, users, n_users, ie, ld_i, n_items, d, mrow, mit,
                                   targets, n_splits, part, score, rank, None)
    return call


@pytest.mark.parametrize("bad", [
    dict(n_splits=0), dict(n_splits=257), dict(n_splits=-1), dict(n_users=-1), dict(n_items=-1),
    dict(d=0), dict(d=12), dict(d=100), dict(d=-64), dict(d=512), dict(ue=None), dict(users=None),
    dict(ie=None), dict(mrow=None), dict(targets=None), dict(part=None), dict(score=None),
    dict(rank=None)], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_score_rank_refuses_bad_sizes_and_null_pointers(lib, bad):
    assert _rank_call(lib)(**bad) == EINVAL


@pytest.mark.parametrize("bad", [
    dict(ld_u=65), dict(ld_u=66), dict(ld_i=67), dict(ld_i=130),
    dict(ue=ctypes.c_void_p(260)), dict(ue=ctypes.c_void_p(257)),
    dict(ie=ctypes.c_void_p(264)), dict(ie=ctypes.c_void_p(271))],
    ids=lambda b: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in b.items()))
def test_score_rank_refuses_unaligned_rows(lib, bad):
    assert _rank_call(lib)(**bad) == EALIGN


def test_score_rank_with_no_users_is_a_no_op(lib):
    call = _rank_call(lib)
    assert call(n_users=0) == 0
    assert call(n_users=0, ue=None, users=None, ie=None, mrow=None, mit=None, targets=None,
                part=None, score=None, rank=None) == 0
    # the sizes and the alignment are checked first (include/lgcn.h)
    assert call(n_users=0, d=12) == EINVAL
    assert call(n_users=0, n_splits=257) == EINVAL
    assert call(n_users=0, ld_u=63) == EALIGN


def test_rank_widths_are_the_topk_kernels(lib):
    """lgcn_score_rank takes the widths lgcn_score_topk takes (evaluate.FUSED_DIMS): a supported
    one gets as far as LGCN_EALIGN with a misaligned table, no further."""
    call = _rank_call(lib)
    for d in (0, 4, 12, 16, 31, 32, 33, 64, 100, 128, 192, 256, 260, 512):
        rc = call(ue=ctypes.c_void_p(260), d=d, ld_u=max(d, 4), ld_i=max(d, 4))
        assert rc == (EALIGN if d in E.FUSED_DIMS else EINVAL), d
