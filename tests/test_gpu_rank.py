"""The rank evaluation kernel lgcn_score_rank (gcn_recommendation_amd/csrc/lgcn_eval.hip: the
target's score from a gathered MFMA tile, an integer count per (user, item split) in the tile
loop, the train-item correction from gathered tiles) against tests/eval_cases.py's rank_ref on
tests/util.py's float64 masked scores:

    rank_ref[b] = #{i != t : s[b,i] > s[b,t] or (s[b,i] == s[b,t] and i < t)}

A. Exact inputs (integers in [-4, 4] / 8: every dot product is exact in fp32 in any order, ties
   are plentiful): rank must equal rank_ref for every slot and target_score must be bitwise
   fp32(s[b,t]) + 0. Each test first asserts that its float64 scores survive an fp32 round trip.
B. Gaussian inputs: the rank is the target's place in lgcn_score_topk's list whenever it is
   there (and its score that list's score, bitwise); it lies inside the interval the dot-product
   rounding bound tau(u, i) = gamma_d · sum_j |u_j·v_j| leaves; split count, slot and run do not
   change a bit.
C. evaluate.rank_fused / rank_torch / Evaluator and the models' evaluate_ranks.

The kernel is called through the C ABI (engine.load_library()) so that a test chooses n_splits,
ld_u and ld_i; every output and scratch element starts as a poison value."""
import functools

import numpy as np
import pytest
import torch

from conftest import Cfg
from eval_cases import (assert_exact, dev as _dev, few_bits, random_mask, rank_ref, score_rank,
                        score_topk)
from gcn_recommendation_amd import engine, evaluate as E, graph, sampler
from util import MASKED, masked_scores64, topk_total_order

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------
def _assert_ranks(got, full, targets, what=""):
    """got: the kernel's (rank int32, target_score fp32); full: the float64 masked scores."""
    rank, score = got
    targets = np.asarray(targets, dtype=np.int64)
    assert rank.dtype == np.int32 and score.dtype == np.float32
    assert rank.shape == score.shape == targets.shape
    want = rank_ref(full, targets)
    bad = np.nonzero(rank != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} ranks differ, first slot {bad[0]}: "
                           f"got {rank[bad[0]]}, want {want[bad[0]]}, target {targets[bad[0]]}")
    inside = want >= 0
    assert np.isnan(score[~inside]).all(), what
    rows = np.nonzero(inside)[0]
    want_s = full[rows, targets[rows]].astype(np.float32) + np.float32(0)  # an exact zero is +0
    assert np.array_equal(score[rows].view(np.uint32), want_s.view(np.uint32)), what
    return want


def _check_exact(dev, ue, ie, users, targets, mrow, mit, n_splits, what=""):
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    got = score_rank(dev, _dev(ue, dev), _dev(ie, dev), users, targets, mrow, mit, n_splits)
    return got, _assert_ranks(got, full, targets, what), full


def _mixed_targets(rng, full, head=40):
    """Per slot a target: every other slot one of its row's first `head` places (where ties and
    the mask decide), the others any item."""
    n, m = full.shape
    t = rng.integers(0, m, n)
    first = topk_total_order(full, min(head, m))[1]
    for b in range(0, n, 2):
        t[b] = first[b, rng.integers(0, first.shape[1])]
    return t


# ----------------------------------------------------------------------------------------------
# A1. widths
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _widths_case(d):
    rng = np.random.default_rng(100 + d)
    n_table, n_items = 200, 2100
    ue, ie = few_bits(rng, n_table, d), few_bits(rng, n_items, d)
    users = rng.permutation(n_table)[:150]
    mrow, mit = random_mask(rng, n_table, n_items)
    full = masked_scores64(ue, ie, users, mrow, mit)
    targets = _mixed_targets(rng, full)
    for b in range(1, 150, 10):  # and some targets that are train items
        lst = mit[mrow[users[b]]:mrow[users[b] + 1]]
        if lst.size:
            targets[b] = lst[-1]
    full.setflags(write=False)
    tied = [(full[b] == full[b, targets[b]]).sum() > 1 for b in range(150)]
    assert np.mean(tied) > 0.5  # ties are what this input is for (rarer among the first places)
    return ue, ie, users, targets, mrow, mit, full


@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_exact_widths(gpu_device, d, n_splits):
    ue, ie, users, targets, mrow, mit, full = _widths_case(d)
    assert_exact(full)
    got = score_rank(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), users, targets, mrow,
                      mit, n_splits)
    want = _assert_ranks(got, full, targets, f"d={d} splits={n_splits}")
    assert (want < 40).sum() >= 60 and (want > 200).sum() >= 30


# ----------------------------------------------------------------------------------------------
# A2. item geometry: partial last tile, short last split, empty trailing splits
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geometry_tables():
    rng = np.random.default_rng(7)
    return few_bits(rng, 40, 64), few_bits(rng, 2049, 64), rng.permutation(40)[:37]


@pytest.mark.parametrize("n_splits", [1, 2, 5, 256])
@pytest.mark.parametrize("n_items", [1, 31, 32, 33, 2049])
def test_exact_item_geometry(gpu_device, n_items, n_splits):
    ue, ie, users = _geometry_tables()
    rng = np.random.default_rng(n_items)
    mrow, mit = random_mask(rng, 40, n_items, 2 if n_items > 1 else 1)
    targets = rng.integers(0, n_items, len(users))
    targets[0], targets[1] = 0, n_items - 1
    _check_exact(gpu_device, ue, ie[:n_items], users, targets, mrow, mit, n_splits,
                 f"items={n_items} splits={n_splits}")


@pytest.mark.parametrize("n_splits", [1, 4])
def test_no_items_at_all(gpu_device, n_splits):
    """n_items == 0: no target is in range, every slot ranks -1."""
    ue, _, _ = _geometry_tables()
    ie = torch.zeros((1, 64), device=gpu_device)  # a table to point at; none of it is an item
    mrow = np.zeros(41, np.int32)
    rank, score = score_rank(gpu_device, _dev(ue, gpu_device), ie, [3, 5, 0, 5], [0, -1, 1, 7],
                              mrow, [], n_splits, n_items=0)
    assert rank.tolist() == [-1] * 4 and np.isnan(score).all()


# ----------------------------------------------------------------------------------------------
# A3. user geometry: wave (32) and block (128) boundaries, unsorted and repeated ids
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 2])
@pytest.mark.parametrize("n_users", [1, 31, 32, 33, 127, 128, 129])
def test_exact_user_geometry(gpu_device, n_users, n_splits):
    rng = np.random.default_rng(21)
    ue, ie = few_bits(rng, 60, 64), few_bits(rng, 700, 64)
    mrow, mit = random_mask(rng, 60, 700)
    rng = np.random.default_rng(n_users)
    users = rng.integers(0, 60, n_users)
    targets = rng.integers(0, 700, n_users)
    if n_users > 1:
        users[-1], targets[-1] = users[0], targets[0]  # the same pair at the batch's two ends
        assert (np.diff(users) < 0).any()
    (rank, score), _, _ = _check_exact(gpu_device, ue, ie, users, targets, mrow, mit, n_splits,
                                       f"users={n_users} splits={n_splits}")
    assert rank[-1] == rank[0] and score[-1:].view(np.uint32) == score[:1].view(np.uint32)
    assert n_users < 31 or len(set(users.tolist())) < n_users


# ----------------------------------------------------------------------------------------------
# A4. all scores equal: the order is the index order, train items after the others
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 3])
def test_exact_all_scores_equal(gpu_device, n_splits):
    rng = np.random.default_rng(40)
    n_users, n_items, d = 40, 2100, 64
    ue = few_bits(rng, n_users, d)
    ie = np.zeros((n_items, d), np.float32)
    mrow, mit = random_mask(rng, n_users, n_items, 30)
    users = np.repeat(np.arange(n_users), 4)
    targets = np.tile(np.array([0, n_items - 1, n_items // 2, 0]), n_users)
    for u in range(n_users):  # the fourth slot of a user: one of its train items
        lst = mit[mrow[u]:mrow[u + 1]]
        targets[4 * u + 3] = lst[len(lst) // 2]
    (rank, score), _, full = _check_exact(gpu_device, ue, ie, users, targets, mrow, mit, n_splits)
    for b, (u, t) in enumerate(zip(users, targets)):  # in words of its own
        lst = mit[mrow[u]:mrow[u + 1]]
        if t in lst:  # every free item first, then the train items below t
            assert rank[b] == n_items - len(lst) + (lst < t).sum() and score[b] == MASKED
        else:         # the free items below t
            assert rank[b] == t - (lst < t).sum() and score[b] == 0
    assert (score == MASKED).sum() >= n_users


# ----------------------------------------------------------------------------------------------
# A5. equal item rows on both sides of the target: the index tie-break
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 2])
def test_exact_duplicated_rows_around_the_target(gpu_device, n_splits):
    rng = np.random.default_rng(50)
    n_users, n_items, d = 45, 500, 64
    ue, ie = few_bits(rng, n_users, d), few_bits(rng, n_items, d)
    t = 250
    same = np.array([3, 31, 32, 200, 249, 251, 256, 300, 499])  # other tiles, both splits
    ie[same] = ie[t]
    below, above = (same < t).sum(), (same > t).sum()
    assert below == 5 and above == 4
    mrow, mit = E.mask_csr([], [], n_users)
    users = np.arange(n_users)
    for target, ties_ahead in ((t, below), (3, 0), (499, len(same)), (251, below + 1)):
        targets = np.full(n_users, target)
        (rank, _), _, full = _check_exact(gpu_device, ue, ie, users, targets, mrow, mit, n_splits)
        others = np.delete(full, np.append(same, t), 1)  # (a chance tie elsewhere counts too)
        others_i = np.delete(np.arange(n_items), np.append(same, t))
        ahead = (others > full[:, [target]]) | ((others == full[:, [target]]) &
                                                (others_i[None, :] < target))
        assert np.array_equal(rank, ahead.sum(1) + ties_ahead)


# ----------------------------------------------------------------------------------------------
# A6. mask edges
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 2])
def test_exact_mask_edges(gpu_device, n_splits):
    rng = np.random.default_rng(44)
    n_users, n_items, d = 8, 300, 64
    ue, ie = few_bits(rng, n_users, d), few_bits(rng, n_items, d)
    nothing = E.mask_csr([], [], n_users)
    free = masked_scores64(ue, ie, np.arange(n_users), *nothing)
    order = topk_total_order(free, n_items)[1]  # every user's order with nothing masked
    t2, t3 = order[2, 150], order[3, 150]
    lists = {0: [],                                          # no train item
             1: np.arange(n_items),                          # every item
             2: order[2, :100],                              # 100 items that beat the target raw
             3: order[3, 200:],                              # 100 items the target beats raw
             4: [order[4, 10]],                              # the target itself, alone
             5: order[5, 5:40],                              # the target and items on both sides
             6: np.setdiff1d(np.arange(n_items), [order[6, 7]]),  # all but the target
             7: []}
    mrow, mit = E.mask_csr(np.concatenate([np.full(len(v), u) for u, v in lists.items()]),
                           np.concatenate([np.asarray(v, np.int64) for v in lists.values()]),
                           n_users)
    users = np.array([0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 1])
    targets = np.array([order[0, 33], 0, n_items - 1, 77, t2, t3, order[4, 10], order[5, 20],
                        order[6, 7], order[7, 0], 150])
    (rank, score), want, full = _check_exact(gpu_device, ue, ie, users, targets, mrow, mit,
                                             n_splits)
    # each list once more, in words of its own
    assert rank[1] == 0 and rank[2] == n_items - 1 and rank[3] == 77 and rank[10] == 150
    assert (score[[1, 2, 3, 10]] == MASKED).all()          # a user whose list is every item
    raw2 = rank_ref(free[[2]], [t2])[0]
    assert rank[4] == raw2 - 100                           # masked items that were ahead
    assert rank[5] == rank_ref(free[[3]], [t3])[0]         # masked items that were behind
    assert score[6] == MASKED and rank[6] == (free[4] > MASKED).sum() - 1  # last but for itself
    assert score[7] == MASKED
    assert rank[8] == 0 and score[8] == np.float32(free[6, order[6, 7]])
    assert rank[9] == 0
    # every list empty, mask_items a one-element dummy
    got = score_rank(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), users, targets,
                      nothing[0], [], n_splits)
    _assert_ranks(got, masked_scores64(ue, ie, users, *nothing), targets, "no train item")


# ----------------------------------------------------------------------------------------------
# A7. -1e10 is a value: unmasked items scoring below it rank after the masked ones
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 2])
def test_exact_scores_below_the_mask_value(gpu_device, n_splits):
    rng = np.random.default_rng(55)
    n_users, n_items, d = 33, 48, 32
    vals = np.array([0, 0, 0, 2.0 ** 16, -2.0 ** 16, 2.0 ** 17, -2.0 ** 17], np.float32)
    ue, ie = rng.choice(vals, (n_users, d)), rng.choice(vals, (n_items, d))
    # user 0 · item j = -2^34, -2^33, 0, -2^34 for j % 4 = 0, 1, 2, 3
    ue[0] = 0
    ue[0, 0] = -2.0 ** 17
    ie[:, 0] = np.tile(np.array([2.0 ** 17, 2.0 ** 16, 0, 2.0 ** 17], np.float32), n_items // 4)
    mu, mi = rng.integers(0, n_users, 250), rng.integers(0, n_items, 250)
    keep = mu != 0
    mrow, mit = E.mask_csr(np.concatenate([mu[keep], np.zeros(6, np.int64)]),
                           np.concatenate([mi[keep], [1, 2, 4, 10, 40, 47]]), n_users)
    assert -2.0 ** 34 < MASKED < -2.0 ** 33
    # every (user, item) pair is a slot
    users = np.repeat(np.arange(n_users), n_items)
    targets = np.tile(np.arange(n_items), n_users)
    (rank, score), _, full = _check_exact(gpu_device, ue, ie, users, targets, mrow, mit, n_splits)
    # user 0: 10 zeros, 11 at -2^33, its 6 train items at -1e10 in index order, then -2^34s
    r0 = rank[:n_items]
    assert np.argsort(r0)[21:32].tolist() == [1, 2, 4, 10, 40, 47, 0, 3, 7, 8, 11]
    assert score[:n_items][[1, 2, 4, 10, 40, 47]].tolist() == [MASKED] * 6
    assert sorted(r0.tolist()) == list(range(n_items))  # a user's ranks are a permutation
    below = (full < MASKED).any(1) & (full == MASKED).any(1)
    rows = np.nonzero(below.reshape(n_users, n_items)[:, 0])[0]
    assert rows.size >= 5
    for u in rows:  # above -1e10 | at -1e10 | below it, in that order
        r, s = rank[u * n_items:(u + 1) * n_items], score[u * n_items:(u + 1) * n_items]
        assert r[s > MASKED].max(initial=-1) < r[s == MASKED].min()
        assert r[s == MASKED].max() < r[s < MASKED].min()


# ----------------------------------------------------------------------------------------------
# A8. strides
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 128])
def test_exact_row_strides(gpu_device, d):
    """ld_u = d + 4 and ld_i = 2d: views of wider tables that hold NaN outside the view."""
    rng = np.random.default_rng(66 + d)
    n_table, n_items = 50, 777
    ue, ie = few_bits(rng, n_table, d), few_bits(rng, n_items, d)
    mrow, mit = random_mask(rng, n_table, n_items)
    users = rng.integers(0, n_table, 45)
    wide_u = torch.full((n_table, d + 4), float("nan"), device=gpu_device)
    wide_i = torch.full((n_items, 2 * d), float("nan"), device=gpu_device)
    wide_u[:, 4:] = _dev(ue, gpu_device)
    wide_i[:, d:] = _dev(ie, gpu_device)
    vu, vi = wide_u[:, 4:], wide_i[:, d:]
    assert vu.stride(0) == d + 4 and vi.stride(0) == 2 * d and not vu.is_contiguous()
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    targets = _mixed_targets(rng, full)
    for n_splits in (1, 3):
        got = score_rank(gpu_device, vu, vi, users, targets, mrow, mit, n_splits)
        _assert_ranks(got, full, targets, f"d={d} splits={n_splits}")


def test_exact_tables_in_one_allocation(gpu_device):
    """User and item tables as the two row ranges of one allocation (the models' propagated
    table: users first, items after)."""
    rng = np.random.default_rng(77)
    U, I, d = 50, 900, 64
    table = few_bits(rng, U + I + 30, d)  # (rows past the items: never an item)
    mrow, mit = random_mask(rng, U, I)
    users = rng.permutation(U)
    full = masked_scores64(table[:U], table[U:U + I], users, mrow, mit)
    assert_exact(full)
    targets = _mixed_targets(rng, full)
    t = _dev(table, gpu_device)
    for n_splits in (1, 2):
        got = score_rank(gpu_device, t[:U], t[U:], users, targets, mrow, mit, n_splits, n_items=I)
        _assert_ranks(got, full, targets, f"splits={n_splits}")


# ----------------------------------------------------------------------------------------------
# A9. targets outside the table; an empty batch
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 3])
def test_targets_outside_the_table(gpu_device, n_splits):
    ue, ie, users, targets, mrow, mit, full = _widths_case(64)
    n_items = ie.shape[0]
    targets = targets.copy()
    out = np.array([0, 5, 31, 32, 33, 100, 149])  # among slots that keep their targets
    targets[out] = [-1, n_items, -1, n_items, -(2 ** 31), 2 ** 31 - 1, n_items + 31]
    got = score_rank(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), users, targets, mrow,
                      mit, n_splits)
    want = _assert_ranks(got, full, targets)
    assert (want[out] == -1).all() and (np.delete(want, out) >= 0).all()
    assert (got[0][out] == -1).all() and np.isnan(got[1][out]).all()


def test_no_users_is_a_no_op(gpu_device):
    lib = engine.load_library()
    with torch.cuda.device(gpu_device):
        assert lib.lgcn_score_rank(None, 64, None, 0, None, 64, 100, 64, None, None, None, 1, None,
                                   None, None, engine._stream(gpu_device)) == 0
        torch.cuda.synchronize(gpu_device)


# ----------------------------------------------------------------------------------------------
# B. Gaussian inputs
# ----------------------------------------------------------------------------------------------
GAUSS_SEED = {32: 932, 256: 1156}  # chosen on the CPU so that the conditions below hold


@functools.lru_cache(maxsize=None)
def _gauss_case(d):
    rng = np.random.default_rng(GAUSS_SEED[d])
    n_table, n_items, n = 120, 3000, 100
    ue = rng.standard_normal((n_table, d)).astype(np.float32)
    ie = rng.standard_normal((n_items, d)).astype(np.float32)
    mrow, mit = random_mask(rng, n_table, n_items, 10)
    users = rng.permutation(n_table)[:n]
    full = masked_scores64(ue, ie, users, mrow, mit)
    masked = np.zeros(full.shape, bool)
    for b, u in enumerate(users):
        masked[b, mit[mrow[u]:mrow[u + 1]]] = True
    gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    tau = gamma * (np.abs(ue.astype(np.float64))[users] @ np.abs(ie.astype(np.float64)).T)
    tau[masked] = 0.0  # a masked pair's score is the constant -1e10: nothing is rounded
    # half the targets from each user's reference top 32, the others anywhere
    first = topk_total_order(full, 32)[1]
    targets = rng.integers(0, n_items, n)
    targets[::2] = first[np.arange(0, n, 2), rng.integers(0, 32, (n + 1) // 2)]
    for a in (full, masked, tau, targets):
        a.setflags(write=False)
    return ue, ie, users, targets, mrow, mit, full, masked, tau


def _interval(full, tau, targets):
    rows = np.arange(len(targets))
    st, tt = full[rows, targets][:, None], tau[rows, targets][:, None]
    sure = full - tau > st + tt
    maybe = full + tau >= st - tt
    sure[rows, targets] = False
    maybe[rows, targets] = False
    return sure.sum(1), maybe.sum(1)


@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_rank_is_the_place_in_the_topk_list(gpu_device, d):
    ue, ie, users, targets, mrow, mit, full = _gauss_case(d)[:7]
    want = rank_ref(full, targets)
    assert (want < 32).sum() * 3 >= len(want) and (want >= 32).sum() * 3 >= len(want)
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    rank, score = score_rank(gpu_device, uet, iet, users, targets, mrow, mit, 3)
    ts, ti = score_topk(gpu_device, uet, iet, users, mrow, mit, 32, 2)
    hit = ti == targets[:, None]
    listed = hit.any(1)
    place = hit.argmax(1)
    assert listed.sum() * 4 >= len(want) and (~listed).sum() * 4 >= len(want)
    assert np.array_equal(rank[listed], place[listed])
    assert np.array_equal(score[listed].view(np.uint32),
                          ts[listed, place[listed]].view(np.uint32))
    assert (rank[~listed] >= 32).all()


@pytest.mark.parametrize("n_splits", [1, 4])
@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_rank_within_rounding(gpu_device, d, n_splits):
    ue, ie, users, targets, mrow, mit, full, masked, tau = _gauss_case(d)
    lo, hi = _interval(full, tau, targets)
    assert (lo <= hi).all() and (lo == hi).sum() * 2 >= len(lo)  # the bound cannot hide a count
    rank, score = score_rank(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), users,
                              targets, mrow, mit, n_splits)
    assert ((lo <= rank) & (rank <= hi)).all(), np.nonzero((rank < lo) | (rank > hi))[0]
    rows = np.arange(len(targets))
    err = np.abs(score.astype(np.float64) - full[rows, targets])
    assert (err <= tau[rows, targets]).all()


@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_bits_do_not_depend_on_splits_slots_or_runs(gpu_device, d):
    ue, ie, users, targets, mrow, mit = _gauss_case(d)[:6]
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)

    def run(sel, n_splits):
        r, s = score_rank(gpu_device, uet, iet, users[sel], targets[sel], mrow, mit, n_splits)
        return r, s.view(np.uint32)

    everyone = np.arange(len(users))
    r1, s1 = run(everyone, 1)
    for n_splits in (4, 256, 1):  # other split counts; and the same call again
        r, s = run(everyone, n_splits)
        assert np.array_equal(r, r1) and np.array_equal(s, s1), n_splits
    perm = np.random.default_rng(d).permutation(len(users))  # another slot, wave and block
    r, s = run(perm, 4)
    assert np.array_equal(r, r1[perm]) and np.array_equal(s, s1[perm])
    r, s = run(perm[:33], 256)  # and another batch size
    assert np.array_equal(r, r1[perm[:33]]) and np.array_equal(s, s1[perm[:33]])


# ----------------------------------------------------------------------------------------------
# C. the surrounding Python
# ----------------------------------------------------------------------------------------------
def test_rank_fused_is_the_abi_call(gpu_device):
    ue, ie, users, targets, mrow, mit, full = _widths_case(64)
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    want = score_rank(gpu_device, uet, iet, users, targets, mrow, mit, 2)
    _assert_ranks(want, full, targets)
    mrow_t, mit_t = _dev(mrow, gpu_device), _dev(mit, gpu_device)
    for us, ts_, mr, mi in ((users, targets, mrow, mit),
                            (users.astype(np.int32), targets.tolist(), mrow_t, mit_t),
                            (_dev(users, gpu_device), _dev(targets, gpu_device), mrow_t, mit_t)):
        r, s = E.rank_fused(uet, iet, us, ts_, mr, mi)
        assert r.device == s.device == gpu_device
        assert r.dtype == torch.int32 and s.dtype == torch.float32 and r.shape == s.shape == (150,)
        assert np.array_equal(r.cpu().numpy(), want[0])
        assert np.array_equal(s.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    # targets outside the table (beyond int32 too), tables that are not contiguous, no train item
    odd = targets.copy()
    odd[:3] = [-1, ie.shape[0], 2 ** 40]
    wide = torch.full((ue.shape[0], 2 * 64), float("nan"), device=gpu_device)
    wide[:, :64] = uet
    r, s = E.rank_fused(wide[:, :64], iet, users, odd, mrow_t, mit_t)
    _assert_ranks((r.cpu().numpy(), s.cpu().numpy()), full, np.where(odd == 2 ** 40, -1, odd))
    none = E.mask_csr([], [], ue.shape[0])
    r, s = E.rank_fused(uet, iet, users, targets, *none)
    _assert_ranks((r.cpu().numpy(), s.cpu().numpy()), masked_scores64(ue, ie, users, *none),
                  targets)
    # an empty batch
    r, s = E.rank_fused(uet, iet, [], [], mrow_t, mit_t)
    assert r.shape == s.shape == (0,) and r.dtype == torch.int32 and s.dtype == torch.float32
    # and what the kernel does not have is an error, not another path
    with pytest.raises(engine.LgcnError):
        E.rank_fused(uet[:, :12].contiguous(), iet[:, :12].contiguous(), users, targets, mrow, mit)
    with pytest.raises(engine.LgcnError):
        E.rank_fused(uet, iet, torch.from_numpy(users), targets, mrow, mit)  # users on the host
    with pytest.raises(engine.LgcnError):
        E.rank_fused(uet, iet, users, targets, mrow_t.long(), mit_t)
    with pytest.raises(ValueError):
        E.rank_fused(uet, iet, users, targets[:-1], mrow, mit)


@pytest.mark.parametrize("d", [64, 12])
def test_rank_torch_on_the_device(gpu_device, d):
    rng = np.random.default_rng(1300 + d)
    U, I = 120, 1500
    ue, ie = few_bits(rng, U, d), few_bits(rng, I, d)
    mrow, mit = random_mask(rng, U, I, 6)
    users = rng.integers(0, U, 200)
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    targets = _mixed_targets(rng, full)
    targets[:2] = [-1, I]
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    for bs in (1024, 37):
        r, s = E.rank_torch(uet, iet, users, targets, _dev(mrow, gpu_device),
                            _dev(mit, gpu_device), batch_size=bs)
        assert r.device == gpu_device and r.dtype == torch.int32
        _assert_ranks((r.cpu().numpy(), s.cpu().numpy()), full, targets, f"d={d} bs={bs}")


def _regular_graph():
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


def _exact_model(dev, U, I, B, d, K, tu, ti, ib_item, ib_brand):
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


def test_evaluator_on_an_exact_model(gpu_device):
    import pandas as pd
    from models.lightgcn import LightGCN
    dev = gpu_device
    U, I, B, tu, ti, ib_item, ib_brand = _regular_graph()
    d, K = 64, 2
    model, adj, fu, fi = _exact_model(dev, U, I, B, d, K, tu, ti, ib_item, ib_brand)
    rng = np.random.default_rng(83)
    mrow, mit = E.mask_csr(tu, ti, U)

    # one held-out item per user, a few users twice in the frame (the last one wins); every
    # other one among the user's first 20 places
    vu = np.concatenate([rng.permutation(U)[:170], [5, 9]])
    vi = rng.integers(0, I, len(vu))
    first = topk_total_order(masked_scores64(fu, fi, vu, mrow, mit), 20)[1]
    vi[::2] = first[::2][np.arange(len(vu[::2])), np.arange(len(vu[::2])) % 20]
    val = pd.DataFrame({"user_idx": vu, "item_idx": vi})
    train = pd.DataFrame({"user_idx": tu, "item_idx": ti})
    held = dict(zip(vu.tolist(), vi.tolist()))
    pu, pi = np.array(list(held)), np.array(list(held.values()))
    full = masked_scores64(fu, fi, pu, mrow, mit)
    assert_exact(full)
    want = rank_ref(full, pi)
    assert 10 <= (want < 20).sum() <= len(want) - 10

    ev = E.Evaluator(tu, ti, U, I, dev)
    old = E.evaluate(model, val, train, adj, 20, dev)
    new = ev.evaluate(model, adj, val, ks=(20,))
    assert (new["recall@20"], new["ndcg@20"]) == old
    assert old == tuple(E.metrics_from_ranks(want, ks=(20,))[k] for k in ("recall@20", "ndcg@20"))
    ks = (1, 20, 50, 1000)
    assert ev.evaluate(model, adj, val, ks=ks) == E.metrics_from_ranks(want, ks=ks)
    assert model.evaluate_ranks(adj, ev, pu, pi, ks=ks) == E.metrics_from_ranks(want, ks=ks)
    ranks = ev.ranks(model, adj, _dev(pu, dev), _dev(pi, dev), batch_size=50)  # four launches
    assert torch.is_tensor(ranks) and ranks.device == dev and ranks.dtype == torch.int32
    assert np.array_equal(ranks.cpu().numpy(), want)
    assert not model.training

    s = sampler.BprSampler(tu, ti, U, I, dev)
    ev2 = E.Evaluator.from_sampler(s)
    assert ev2._rowptr.data_ptr() == s._rowptr.data_ptr()
    assert ev2._items.data_ptr() == s._pos_items.data_ptr()
    assert ev2.device == dev and (ev2.num_users, ev2.num_items) == (U, I)
    assert ev2.evaluate(model, adj, val, ks=ks) == E.metrics_from_ranks(want, ks=ks)
    # a width the kernel does not have goes to torch ops
    small = LightGCN(U, I, B, Cfg(12, K)).to(dev)
    r = ev.ranks(small, adj, pu, pi)
    assert r.device == dev and r.dtype == torch.int32 and r.shape == (len(pu),)
    assert ((r >= 0) & (r < I)).all().item()
