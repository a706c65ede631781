"""The list rank evaluation without a GPU (gcn_recommendation_amd/evaluate.py: target_csr,
metrics_from_rank_lists, rank_lists_torch, Evaluator.rank_lists / evaluate_lists on a CPU device;
lgcn_score_rank_lists' host-side validation): the lists against a dict of sets, the metrics
against a double loop in plain Python, the ranks against tests/eval_cases.py's rank_ref per entry
on float64 scores, and everything the C entry point refuses before a launch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from eval_cases import assert_exact, few_bits, random_mask, rank_ref
from gcn_recommendation_amd import _build, engine, evaluate as E
from rank_lists_cases import (csr, exact_model, expand, held_out_frame, lists_ref, regular_graph)
from util import masked_scores64

EINVAL, EALIGN = -1, -2  # include/lgcn.h


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


# ----------------------------------------------------------------------------------------------
# the ABI
# ----------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(lib):
    bound = {name for name, _, _ in engine.ABI}
    for name in ("lgcn_score_rank_lists", "lgcn_score_rank_lists_scratch_bytes"):
        assert name in bound and hasattr(lib, name)
        assert name + "(" in open(os.path.join(ROOT, "include", "lgcn.h")).read()
    assert lib.lgcn_abi_version() == 14


def test_scratch_bytes(lib):
    q = lib.lgcn_score_rank_lists_scratch_bytes
    assert q(0, 0, 1) == 0
    assert q(100, 0, 1) >= 400
    for n_users, n, splits in ((1, 1, 1), (8192, 81920, 8), (33, 700, 256), (5, 2 ** 33, 3)):
        assert q(n_users, n, splits) >= 4 * n_users + (12 + 4 * splits) * n
        assert q(n_users, n, splits) % 4 == 0
        assert q(n_users, n + 1, splits) >= q(n_users, n, splits)
    assert q(-1, 0, 1) == q(1, -1, 1) == q(1, 1, 0) == q(1, 1, 257) == 0


def _lists_call(lib):
    p = ctypes.c_void_p(256)  # 16-B aligned, never dereferenced: every call is refused on the host

    def call(ue=p, ld_u=64, users=p, n_users=4, ie=p, ld_i=64, n_items=100, d=64, mrow=p, mit=p,
             trow=p, titems=p, n_splits=1, scratch=p, scratch_bytes=1 << 20, score=p, rank=p):
        return lib.lgcn_score_rank_lists(ue, ld_u, users, n_users, ie, ld_i, n_items, d, mrow, mit,
                                         trow, titems, n_splits, scratch, scratch_bytes, score,
                                         rank, None)
    return call


@pytest.mark.parametrize("bad", [
    dict(n_splits=0), dict(n_splits=257), dict(n_splits=-1), dict(n_users=-1), dict(n_items=-1),
    dict(d=0), dict(d=12), dict(d=100), dict(d=-64), dict(d=512), dict(ue=None), dict(users=None),
    dict(ie=None), dict(mrow=None), dict(trow=None), dict(titems=None), dict(scratch=None),
    dict(score=None), dict(rank=None), dict(scratch_bytes=0), dict(scratch_bytes=15)],
    ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_refuses_bad_sizes_and_null_pointers(lib, bad):
    assert _lists_call(lib)(**bad) == EINVAL


def test_refuses_a_short_scratch(lib):
    """The host never reads target_rowptr: what it can refuse is a scratch below the size query
    for the slots alone (the kernels leave a slot past the scratch's entries unwritten)."""
    call = _lists_call(lib)
    for n_users, n_splits in ((4, 1), (129, 7), (8192, 256)):
        need = lib.lgcn_score_rank_lists_scratch_bytes(n_users, 0, n_splits)
        assert need >= 4 * n_users
        assert call(n_users=n_users, n_splits=n_splits, scratch_bytes=need - 1) == EINVAL
        assert call(n_users=n_users, n_splits=n_splits, scratch_bytes=4 * n_users - 1) == EINVAL


@pytest.mark.parametrize("bad", [
    dict(ld_u=65), dict(ld_u=66), dict(ld_i=67), dict(ld_i=130),
    dict(ue=ctypes.c_void_p(260)), dict(ue=ctypes.c_void_p(257)),
    dict(ie=ctypes.c_void_p(264)), dict(ie=ctypes.c_void_p(271)),
    dict(scratch=ctypes.c_void_p(258))],
    ids=lambda b: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in b.items()))
def test_refuses_unaligned_rows(lib, bad):
    assert _lists_call(lib)(**bad) == EALIGN


def test_no_users_is_a_no_op(lib):
    call = _lists_call(lib)
    assert call(n_users=0) == 0
    assert call(n_users=0, ue=None, users=None, ie=None, mrow=None, mit=None, trow=None,
                titems=None, scratch=None, scratch_bytes=0, score=None, rank=None) == 0
    # the sizes and the alignment are checked first, as lgcn_score_rank's
    assert call(n_users=0, d=12) == EINVAL
    assert call(n_users=0, n_splits=257) == EINVAL
    assert call(n_users=0, ld_u=63) == EALIGN
    for d in (0, 4, 12, 16, 31, 32, 33, 64, 100, 128, 192, 256, 260, 512):
        rc = call(ue=ctypes.c_void_p(260), d=d, ld_u=max(d, 4), ld_i=max(d, 4))
        assert rc == (EALIGN if d in E.FUSED_DIMS else EINVAL), d


# ----------------------------------------------------------------------------------------------
# target_csr
# ----------------------------------------------------------------------------------------------
def test_target_csr_against_a_dict_of_sets():
    rng = np.random.default_rng(5)
    users = rng.integers(0, 60, 500) * 3 + 1  # users that do not occur lie between those that do
    items = rng.integers(0, 40, 500)
    users[:50], items[:50] = users[100:150], items[100:150]  # repeated rows
    assert (np.diff(users) < 0).any()
    ref = {}
    for u, i in zip(users.tolist(), items.tolist()):
        ref.setdefault(u, set()).add(i)
    assert sum(len(v) for v in ref.values()) < 500
    for us, its in ((users, items), (users.tolist(), items.tolist()),
                    (users.astype(np.int32), items.astype(np.int32))):
        eu, rowptr, it = E.target_csr(us, its)
        assert eu.dtype == np.int64 and rowptr.dtype == np.int32 and it.dtype == np.int32
        assert eu.tolist() == sorted(ref) and rowptr[0] == 0 and rowptr[-1] == len(it)
        assert len(rowptr) == len(eu) + 1
        for j, u in enumerate(eu):
            assert it[rowptr[j]:rowptr[j + 1]].tolist() == sorted(ref[u])
    assert 0 not in eu and 2 not in eu
    # one row per user: the lists are the pairs; nothing at all: one offset
    eu, rowptr, it = E.target_csr([7, 3, 5], [1, 2, 0])
    assert eu.tolist() == [3, 5, 7] and rowptr.tolist() == [0, 1, 2, 3] and it.tolist() == [2, 0, 1]
    eu, rowptr, it = E.target_csr([], [])
    assert eu.shape == (0,) and rowptr.tolist() == [0] and it.shape == (0,)
    # an item no int32 holds is no item
    eu, rowptr, it = E.target_csr([1, 1, 1], [4, 2 ** 40, -3])
    assert rowptr.tolist() == [0, 3] and sorted(it.tolist()) == [-1, -1, 4]
    with pytest.raises(ValueError):
        E.target_csr([1, 2], [3])


# ----------------------------------------------------------------------------------------------
# metrics_from_rank_lists
# ----------------------------------------------------------------------------------------------
def _metrics_by_loops(ranks, rowptr, ks):
    """The table of the metrics' definitions as a double loop; the means by math.fsum."""
    per = {f"{m}@{k}": [] for k in ks for m in ("recall", "precision", "hit", "ndcg")}
    per["mrr"] = []
    for j in range(len(rowptr) - 1):
        mine = [int(r) for r in ranks[rowptr[j]:rowptr[j + 1]]]
        if not mine:
            continue
        for k in ks:
            hits, dcg, ideal = 0, 0.0, 0.0
            for r in mine:
                if 0 <= r < k:
                    hits += 1
                    dcg += 1.0 / np.log2(r + 2)
            for i in range(min(k, len(mine))):
                ideal += 1.0 / np.log2(i + 2)
            per[f"recall@{k}"].append(hits / len(mine))
            per[f"precision@{k}"].append(hits / k)
            per[f"hit@{k}"].append(1.0 if hits else 0.0)
            per[f"ndcg@{k}"].append(dcg / ideal)
        ranked = [r for r in mine if r >= 0]
        per["mrr"].append(1.0 / (min(ranked) + 1) if ranked else 0.0)
    return {m: math.fsum(v) / len(v) if v else float("nan") for m, v in per.items()}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_against_a_double_loop(seed):
    """Every per-user value is computed by the same operations in the same order on both sides;
    only the mean differs. 24 users have a list: numpy's sum of 24 float64 values is eight running
    sums of three (two roundings) joined by a tree of depth three, so with the division a mean
    carries at most 6 roundings, fsum's 2: the two differ by at most 8 * 2^-53 < 1e-15 relative
    (the values are not negative)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, 28)
    lens[[0, 11, 17, 27]] = 0   # empty lists, at both ends too
    lens[3], lens[4] = 1, 60    # one entry; more entries than any k below but the last
    assert (lens > 0).sum() == 24
    rowptr, _ = csr([np.zeros(n) for n in lens])
    ranks = rng.integers(0, 70, rowptr[-1]).astype(np.int32)
    ranks[rng.random(len(ranks)) < 0.15] = -1
    ranks[rowptr[5]:rowptr[6]] = -1  # a user none of whose entries is ranked
    ks = (1, 5, 20, 50, 1000)
    got = E.metrics_from_rank_lists(ranks, rowptr, ks=ks)
    want = _metrics_by_loops(ranks, rowptr, ks)
    assert sorted(got) == sorted(want) and all(type(v) is float for v in got.values())
    for m in want:
        assert got[m] == pytest.approx(want[m], rel=1e-15, abs=0), m
    assert 0 < got["recall@5"] < got["recall@50"] <= 1 and 0 < got["mrr"] < 1
    assert got["hit@1000"] < 1  # the unranked user
    # a tensor, int64, a window of a longer rank array: the same numbers
    assert E.metrics_from_rank_lists(torch.from_numpy(ranks), torch.from_numpy(rowptr), ks) == got
    padded = np.concatenate([[0, 0, 0], ranks.astype(np.int64), [0]])
    assert E.metrics_from_rank_lists(padded, rowptr + 3, ks) == got
    assert E.metrics_from_rank_lists(ranks, rowptr) == \
        {m: got[m] for m in ("recall@20", "precision@20", "hit@20", "ndcg@20", "mrr")}


def test_metrics_with_one_entry_per_user_are_metrics_from_ranks():
    rng = np.random.default_rng(9)
    ranks = rng.integers(-1, 60, 333).astype(np.int32)
    ranks[:5] = [0, 19, 20, -1, 4]
    ks = (1, 20, 50, 1000)
    lists = E.metrics_from_rank_lists(ranks, np.arange(334), ks=ks)
    single = E.metrics_from_ranks(ranks, ks=ks)
    for m in single:
        assert lists[m] == single[m], m
    for k in ks:
        assert lists[f"hit@{k}"] == single[f"recall@{k}"]
        assert lists[f"precision@{k}"] == pytest.approx(single[f"recall@{k}"] / k, rel=1e-15)


def test_metrics_edges():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no mean of an empty slice, no division by zero
        for ranks, rowptr in (([], [0]), ([], []), ([], [0, 0, 0]), ([3, 4], [1, 1]),
                              (torch.zeros(0, dtype=torch.int32), np.zeros(1, np.int32))):
            m = E.metrics_from_rank_lists(ranks, rowptr, ks=(20, 50))
            assert sorted(m) == sorted(["mrr"] + [f"{n}@{k}" for k in (20, 50) for n in
                                                  ("recall", "precision", "hit", "ndcg")])
            assert all(math.isnan(v) for v in m.values())
        miss = E.metrics_from_rank_lists([-1, -1, -1], [0, 2, 3], ks=(1, 1000))
        assert set(miss.values()) == {0.0}
        best = E.metrics_from_rank_lists([1, 0, 2, 0], [0, 3, 4], ks=(3,))
        assert best == {"recall@3": 1.0, "precision@3": (1.0 + 1 / 3) / 2, "hit@3": 1.0,
                        "ndcg@3": 1.0, "mrr": 1.0}


# ----------------------------------------------------------------------------------------------
# rank_lists_torch on CPU tensors
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64])
def test_rank_lists_torch_cpu_matches_reference(d):
    rng = np.random.default_rng(400 + d)
    U, I = 50, 400
    ue, ie = few_bits(rng, U, d), few_bits(rng, I, d)
    mrow, mit = random_mask(rng, U, I, 6)
    users = rng.integers(0, U, 40)
    lists = [rng.integers(0, I, n) for n in rng.integers(0, 12, 40)]
    lists[0], lists[39] = [], []
    lists[3] = [5, 5, -1, I, 7]                      # twice; outside the table
    lists[4] = mit[mrow[users[4]]:mrow[users[4] + 1]]  # train items only
    rowptr, items = csr(lists)
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    want = lists_ref(full, rowptr, items)
    slot = expand(users, rowptr)[0]
    inside = want >= 0
    assert (~inside).sum() == 2 and len(lists[4]) > 0
    uet, iet = torch.from_numpy(ue), torch.from_numpy(ie)
    for us, rp, its, mr, mi in ((users, rowptr, items, mrow, mit),
                                (torch.from_numpy(users), torch.from_numpy(rowptr),
                                 torch.from_numpy(items), torch.from_numpy(mrow),
                                 torch.from_numpy(mit))):
        for bs in (1024, 7):
            r, s = E.rank_lists_torch(uet, iet, us, rp, its, mr, mi, batch_size=bs)
            assert r.dtype == torch.int32 and s.dtype == torch.float32
            assert r.shape == s.shape == items.shape
            assert np.array_equal(r.numpy(), want)
            assert np.isnan(s.numpy()[~inside]).all()
            assert np.array_equal(s.numpy()[inside],
                                  full[slot[inside], items[inside]].astype(np.float32))
    # a window of the slots: entries outside it rank -1
    r, _ = E.rank_lists_torch(uet, iet, users[10:20], rowptr[10:21], items, mrow, mit)
    lo, hi = rowptr[10], rowptr[20]
    assert np.array_equal(r.numpy()[lo:hi], want[lo:hi])
    assert (r.numpy()[:lo] == -1).all() and (r.numpy()[hi:] == -1).all()
    # nothing at all; offsets that do not fit
    r, s = E.rank_lists_torch(uet, iet, [], [0], [], mrow, mit)
    assert r.shape == s.shape == (0,) and r.dtype == torch.int32
    with pytest.raises(ValueError):
        E.rank_lists_torch(uet, iet, users, rowptr[:-1], items, mrow, mit)
    with pytest.raises(engine.LgcnError):
        E.rank_lists_fused(uet, iet, users, rowptr, items, mrow, mit)  # the HIP kernel only


# ----------------------------------------------------------------------------------------------
# Evaluator on a CPU device, end to end on the exact regular-graph model
# ----------------------------------------------------------------------------------------------
def test_evaluator_lists_cpu_on_an_exact_model():
    import pandas as pd
    U, I, B, tu, ti, ib_item, ib_brand = regular_graph()
    model, adj, fu, fi = exact_model("cpu", U, I, B, 64, 2, tu, ti, ib_item, ib_brand)
    mrow, mit = E.mask_csr(tu, ti, U)
    vu, vi = held_out_frame(np.random.default_rng(84), fu, fi, mrow, mit, U, I)
    eu, rowptr, items = E.target_csr(vu, vi)
    assert len(eu) == 170 and 1 <= np.diff(rowptr).min() and np.diff(rowptr).max() >= 6
    full = masked_scores64(fu, fi, eu, mrow, mit)
    assert_exact(full)
    want = lists_ref(full, rowptr, items)
    assert (want < 20).sum() * 4 >= len(want) and (want >= 20).sum() * 4 >= len(want)
    ks = (1, 20, 50, 1000)
    ev = E.Evaluator(tu, ti, U, I, "cpu")
    model.train()
    gu, grow, ranks = ev.rank_lists(model, adj, vu, vi)
    assert not model.training
    assert np.array_equal(gu, eu) and np.array_equal(grow, rowptr)
    assert ranks.dtype == torch.int32 and ranks.device.type == "cpu"
    assert np.array_equal(ranks.numpy(), want)
    val = pd.DataFrame({"user_idx": vu, "item_idx": vi})
    got = ev.evaluate_lists(model, adj, val, ks=ks)
    assert got == E.metrics_from_rank_lists(want, rowptr, ks=ks)
    assert ev.evaluate_lists(model, adj, (vu, vi), ks=ks) == got
    assert model.evaluate_rank_lists(adj, ev, vu, vi, ks=ks) == got
    assert torch.equal(ev.rank_lists(model, adj, vu, vi, batch_size=16)[2], ranks)
    empty = ev.evaluate_lists(model, adj, val.iloc[:0])
    assert all(math.isnan(v) for v in empty.values())
    with pytest.raises(ValueError):
        ev.rank_lists(model, adj, vu, vi, batch_size=0)


def test_two_rows_of_one_user_are_a_list_of_two():
    """evaluate_lists keeps every row of a frame; evaluate keeps a user's last, as before."""
    import pandas as pd
    U, I, B, tu, ti, ib_item, ib_brand = regular_graph()
    model, adj, fu, fi = exact_model("cpu", U, I, B, 64, 2, tu, ti, ib_item, ib_brand)
    mrow, mit = E.mask_csr(tu, ti, U)
    full = masked_scores64(fu, fi, [7], mrow, mit)
    order = np.lexsort((np.arange(I), -full[0]))  # the user's items, best first
    val = pd.DataFrame({"user_idx": [7, 7], "item_idx": [order[0], order[30]]})
    ev = E.Evaluator(tu, ti, U, I, "cpu")
    eu, rowptr, ranks = ev.rank_lists(model, adj, val["user_idx"], val["item_idx"])
    assert eu.tolist() == [7] and rowptr.tolist() == [0, 2]
    assert sorted(ranks.tolist()) == [0, 30]
    lists = ev.evaluate_lists(model, adj, val, ks=(20,))
    assert lists["recall@20"] == 0.5 and lists["hit@20"] == 1.0 and lists["mrr"] == 1.0
    single = ev.evaluate(model, adj, val, ks=(20,))  # the last row wins: rank 30, a miss
    assert single["recall@20"] == 0.0 and single["mrr"] == 1.0 / 31
    assert single == E.metrics_from_ranks(rank_ref(full, [order[30]]), ks=(20,))
