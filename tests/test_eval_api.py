"""The evaluation path (gcn_recommendation_amd/csrc/lgcn_eval.hip, evaluate.py) without a GPU:
the host-side argument validation of lgcn_score_topk, the split heuristic lgcn_eval_splits, the
mask CSR builder evaluate.mask_csr against a dict-of-sets restatement of the train_user_items
dict, the limits of evaluate.fused_supported, and the numpy top-k reference of tests/util.py (the
yardstick of tests/test_gpu_eval.py) against torch.topk."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from gcn_recommendation_amd import _build, engine, evaluate as E
from util import MASKED, masked_scores64, topk_reference, topk_total_order

EINVAL, EALIGN = -1, -2  # include/lgcn.h


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


# ----------------------------------------------------------------------------------------------
# lgcn_score_topk: everything it refuses before its first HIP call
# ----------------------------------------------------------------------------------------------
def _topk_call(lib):
    p = ctypes.c_void_p(256)  # 16-B aligned, never dereferenced: every call is refused on the host

    def call(ue=p, ld_u=64, users=p, n_users=4, ie=p, ld_i=64, n_items=100, d=64, mrow=p, mit=p,
             k=20, n_splits=1, part_s=p, part_i=p, top_s=p, top_i=p):
        return lib.lgcn_score_topk(ue, ld_u, users, n_users, ie, ld_i, n_items, d, mrow, mit, k,
                                   n_splits, part_s, part_i, top_s, top_i, None)
    return call


@pytest.mark.parametrize("bad", [
    dict(k=0), dict(k=33), dict(k=-1), dict(n_splits=0), dict(n_splits=257), dict(n_splits=-1),
    dict(n_users=-1), dict(n_items=-1), dict(d=0), dict(d=12), dict(d=100), dict(d=-64),
    dict(d=512), dict(ue=None), dict(users=None), dict(ie=None), dict(mrow=None),
    dict(part_s=None), dict(part_i=None), dict(top_s=None), dict(top_i=None)],
    ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_score_topk_refuses_bad_sizes_and_null_pointers(lib, bad):
    assert _topk_call(lib)(**bad) == EINVAL


@pytest.mark.parametrize("bad", [
    dict(ld_u=65), dict(ld_u=66), dict(ld_u=67), dict(ld_i=65), dict(ld_i=66), dict(ld_i=130),
    dict(ue=ctypes.c_void_p(260)), dict(ue=ctypes.c_void_p(264)), dict(ue=ctypes.c_void_p(257)),
    dict(ie=ctypes.c_void_p(260)), dict(ie=ctypes.c_void_p(264)), dict(ie=ctypes.c_void_p(271))],
    ids=lambda b: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in b.items()))
def test_score_topk_refuses_unaligned_rows(lib, bad):
    assert _topk_call(lib)(**bad) == EALIGN


def test_score_topk_with_no_users_is_a_no_op(lib):
    call = _topk_call(lib)
    assert call(n_users=0) == 0
    # nothing is read or written for an empty batch: no pointer is required (include/lgcn.h)
    assert call(n_users=0, ue=None, users=None, ie=None, mrow=None, mit=None, part_s=None,
                part_i=None, top_s=None, top_i=None) == 0
    # the sizes and the alignment are checked first (include/lgcn.h)
    assert call(n_users=0, k=0) == EINVAL
    assert call(n_users=0, d=12) == EINVAL
    assert call(n_users=0, n_splits=257) == EINVAL
    assert call(n_users=0, ld_u=63) == EALIGN


# ----------------------------------------------------------------------------------------------
# lgcn_eval_splits
# ----------------------------------------------------------------------------------------------
I32_MAX = 2 ** 31 - 1
SPLIT_USERS = [0, 1, 2, 127, 128, 129, 1024, 8192, 100_000, 10_000_000, I32_MAX]
SPLIT_ITEMS = [0, 1, 20, 2047, 2048, 2049, 4096, 4097, 70_000, 524_288, 524_289, 4_400_000,
               I32_MAX]
SPLIT_CUS = [0, 1, 8, 256, 304, 100_000, I32_MAX]


def test_eval_splits_properties(lib):
    for n_items, n_cu in itertools.product(SPLIT_ITEMS, SPLIT_CUS):
        prev = None
        for n_users in SPLIT_USERS:
            s = lib.lgcn_eval_splits(n_users, n_items, n_cu)
            what = (n_users, n_items, n_cu, s)
            assert 1 <= s <= 256, what
            by_len = -(-n_items // 2048)
            if by_len >= 1:
                assert s <= by_len, what          # no split shorter than 2048 items
            if n_items <= 2048:
                assert s == 1, what
            if prev is not None:
                assert s <= prev, what            # more user tiles never ask for more splits
            prev = s


def test_eval_splits_fills_the_device(lib):
    """The heuristic itself (about two blocks per CU) where neither limit binds: one user tile
    (<= 128 users) on 256 CUs and plenty of items asks for the cap, and 512 user tiles for 1."""
    assert lib.lgcn_eval_splits(128, 4_400_000, 256) == 256
    assert lib.lgcn_eval_splits(128, 4_400_000, 0) == 256     # unknown CU count: 256 assumed
    assert lib.lgcn_eval_splits(128, 4_400_000, 8) == 16
    assert lib.lgcn_eval_splits(129, 4_400_000, 8) == 8       # two user tiles
    assert lib.lgcn_eval_splits(512 * 128, 4_400_000, 256) == 1
    assert lib.lgcn_eval_splits(128, 3 * 2048 + 1, 256) == 4  # limited by the 2048-item floor


# ----------------------------------------------------------------------------------------------
# evaluate.mask_csr
# ----------------------------------------------------------------------------------------------
def _dict_of_sets(users, items):
    """The train_user_items dict that evaluate.mask_csr stands for (user -> its train items), as
    sets: the mask loop writes -1e10 once per distinct item."""
    out = {}
    for u, i in zip(users, items):
        out.setdefault(int(u), set()).add(int(i))
    return out


def _check_mask_csr(users, items, n_users):
    rowptr, it = E.mask_csr(users, items, n_users)
    assert rowptr.dtype == np.int32 and it.dtype == np.int32
    assert rowptr.shape == (n_users + 1,) and rowptr[0] == 0 and rowptr[-1] == it.size
    assert (np.diff(rowptr) >= 0).all()
    want = _dict_of_sets(users, items)
    for u in range(n_users):
        row = it[rowptr[u]:rowptr[u + 1]]
        assert row.tolist() == sorted(want.get(u, ())), u   # sorted, no duplicates, nothing lost
    return rowptr, it


def test_mask_csr_matches_dict_of_sets():
    rng = np.random.default_rng(3)
    # unsorted pairs with duplicates; users 0, 1 (start), 7..9 (middle) and 18, 19 (end) have no
    # item; item ids 0 and the largest one occur
    pool = np.array([2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17])
    users = rng.choice(pool, 400)
    items = rng.integers(0, 50, 400)
    items[:5] = 0
    items[5:9] = 49
    users[5] = 17   # the last user with items holds the largest item id
    users[0] = 2    # the first user with items holds item 0
    assert len(set(zip(users.tolist(), items.tolist()))) < 400  # duplicates are present
    rowptr, it = _check_mask_csr(users, items, 20)
    assert rowptr[2] == 0 and rowptr[20] == rowptr[18]
    assert it[0] == 0 and it[-1] == 49
    # n_users larger than any id: empty trailing rows
    _check_mask_csr(users, items, 64)
    # already sorted input, and its reverse
    order = np.lexsort((items, users))
    a = _check_mask_csr(users[order], items[order], 20)
    b = _check_mask_csr(users[order][::-1], items[order][::-1], 20)
    for x, y, z in zip(a, b, (rowptr, it)):
        assert np.array_equal(x, z) and np.array_equal(y, z)


def test_mask_csr_edges():
    rowptr, it = E.mask_csr(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    assert rowptr.dtype == np.int32 and it.dtype == np.int32
    assert rowptr.tolist() == [0] * 6 and it.size == 0
    rowptr, it = E.mask_csr([], [], 0)
    assert rowptr.tolist() == [0] and it.size == 0
    # one pair; item id 0 only (span 1); the same pair many times
    _check_mask_csr(np.array([3]), np.array([0]), 4)
    _check_mask_csr(np.array([0, 0, 0]), np.array([0, 0, 0]), 1)
    _check_mask_csr(np.array([1, 1, 1, 0]), np.array([7, 7, 7, 7]), 2)
    # int32 and list inputs, large item ids (the key users * span + items needs 64 bits)
    big = 2 ** 31 - 2
    rowptr, it = _check_mask_csr(np.array([5, 0, 5, 2], np.int32),
                                 np.array([big, big, 0, 1], np.int32), 6)
    assert it.tolist() == [big, 1, 0, big]
    _check_mask_csr([2, 1, 2], [9, 0, 3], 3)


def test_fused_supported_limits():
    for d in range(0, 300):
        for k in (-1, 0, 1, 2, 20, 31, 32, 33, 64):
            want = d in (32, 64, 128, 256) and 1 <= k <= 32
            assert E.fused_supported(d, k) == want, (d, k)
    assert not E.fused_supported(512, 20) and not E.fused_supported(16, 20)
    assert E.FUSED_DIMS == (32, 64, 128, 256) and E.FUSED_MAX_K == 32


def test_fused_limits_are_the_kernels(lib):
    """evaluate.fused_supported says yes exactly where lgcn_score_topk does not refuse d and k
    (asked with misaligned tables: a supported pair gets as far as LGCN_EALIGN, no further)."""
    call = _topk_call(lib)
    odd = ctypes.c_void_p(260)
    for d in (0, 4, 12, 16, 31, 32, 33, 64, 100, 128, 192, 256, 260, 512):
        for k in (0, 1, 20, 32, 33):
            rc = call(ue=odd, d=d, k=k, ld_u=max(d, 4), ld_i=max(d, 4))
            assert rc == (EALIGN if E.fused_supported(d, k) else EINVAL), (d, k)


# ----------------------------------------------------------------------------------------------
# the numpy reference itself
# ----------------------------------------------------------------------------------------------
def test_reference_topk_matches_torch_on_tie_free_scores():
    rng = np.random.default_rng(5)
    n, m = 40, 700
    # a tie-free float64 matrix: every row a permutation of distinct values
    s = np.stack([rng.permutation(m) for _ in range(n)]).astype(np.float64) / 7.0 - 31.0
    for k in (1, 2, 20, 32, m):
        ts, ti = torch.topk(torch.from_numpy(s), k)
        rs, ri = topk_total_order(s, k)
        assert np.array_equal(ri, ti.numpy()) and np.array_equal(rs, ts.numpy()), k
    rs, ri = topk_total_order(s[:, :5], 8)  # fewer entries than k
    ts, ti = torch.topk(torch.from_numpy(s[:, :5].copy()), 5)
    assert np.array_equal(ri[:, :5], ti.numpy()) and np.array_equal(rs[:, :5], ts.numpy())
    assert (ri[:, 5:] == -1).all() and np.isneginf(rs[:, 5:]).all()
    rs, ri = topk_total_order(np.zeros((3, 0)), 4)
    assert (ri == -1).all() and np.isneginf(rs).all() and ri.dtype == np.int64


def test_reference_topk_orders_ties_by_index_and_masks():
    s = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 1.0]])
    rs, ri = topk_total_order(s, 6)
    assert ri.tolist() == [[1, 2, 4, 0, 5, 3]] and rs.tolist() == [[3, 3, 3, 1, 1, -2]]
    # masked pairs score MASKED (a value: above anything lower), users index the mask CSR by id
    ue = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]], np.float32)
    ie = np.array([[4.0, 1.0], [3.0, 2.0], [2.0, 3.0], [-2e10, 4.0]], np.float32)
    mrow, mit = E.mask_csr([1, 1, 2], [3, 2, 0], 3)
    users = [2, 1, 1, 0]
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert full.tolist() == [[MASKED, -3, -2, 2e10], [1, 2, MASKED, MASKED],
                             [1, 2, MASKED, MASKED], [4, 3, 2, -2e10]]
    assert MASKED == -1e10
    rs, ri = topk_reference(ue, ie, users, mrow, mit, 4)
    assert ri.tolist() == [[3, 2, 1, 0], [1, 0, 2, 3], [1, 0, 2, 3], [0, 1, 2, 3]]
    assert rs[0].tolist() == [2e10, -2, -3, MASKED] and rs[3].tolist() == [4, 3, 2, -2e10]
    ts, ti = torch.topk(torch.from_numpy(full[[0, 3]]), 4)  # the two tie-free rows
    assert np.array_equal(ti.numpy(), ri[[0, 3]])
