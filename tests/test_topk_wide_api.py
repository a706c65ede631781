"""The recommendation lists without a GPU: everything lgcn_score_topk_wide refuses before its first
HIP call, its scratch and split helpers, evaluate.wide_supported against the kernel's own limits,
and the torch route (topk_total_order_torch, Evaluator.recommend and similar_items on a CPU
device) against tests/util.py's topk_total_order on exact few-bit tables."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Cfg
from eval_cases import assert_exact, few_bits
from gcn_recommendation_amd import _build, engine, evaluate as E, graph
from topk_wide_cases import assert_bitwise
from util import MASKED, masked_scores64, topk_total_order

EINVAL, EALIGN = -1, -2  # include/lgcn.h
MAX_K = 1024             # LGCN_TOPK_WIDE_MAX_K


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


# ----------------------------------------------------------------------------------------------
# lgcn_score_topk_wide: everything it refuses before its first HIP call
# ----------------------------------------------------------------------------------------------
def _wide_call(lib):
    p = ctypes.c_void_p(256)  # 16-B aligned, never dereferenced: every call is refused on the host

    def call(ue=p, ld_u=64, users=p, n_users=4, ie=p, ld_i=64, n_items=100, d=64, mrow=p, mit=p,
             k=100, n_splits=1, scratch=p, scratch_bytes=None, top_s=p, top_i=p):
        if scratch_bytes is None:
            scratch_bytes = lib.lgcn_score_topk_wide_scratch_bytes(max(n_users, 0),
                                                                   min(max(k, 1), MAX_K),
                                                                   min(max(n_splits, 1), 256))
        return lib.lgcn_score_topk_wide(ue, ld_u, users, n_users, ie, ld_i, n_items, d, mrow, mit,
                                        k, n_splits, scratch, scratch_bytes, top_s, top_i, None)
    return call


@pytest.mark.parametrize("bad", [
    dict(k=0), dict(k=1025), dict(k=-1), dict(d=48), dict(d=0), dict(d=512), dict(n_splits=0),
    dict(n_splits=257), dict(n_users=-1), dict(n_items=-1), dict(ue=None), dict(users=None),
    dict(ie=None), dict(mrow=None), dict(scratch=None), dict(top_s=None), dict(top_i=None)],
    ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_refuses_bad_sizes_and_null_pointers(lib, bad):
    assert _wide_call(lib)(**bad) == EINVAL


@pytest.mark.parametrize("bad", [
    dict(ld_u=65), dict(ld_i=66), dict(ue=ctypes.c_void_p(260)), dict(ie=ctypes.c_void_p(264)),
    dict(scratch=ctypes.c_void_p(258))],
    ids=lambda b: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in b.items()))
def test_refuses_unaligned_rows_and_scratch(lib, bad):
    assert _wide_call(lib)(**bad) == EALIGN


def test_refuses_a_scratch_one_byte_short(lib):
    call = _wide_call(lib)
    for n_users, k, n_splits in ((4, 100, 1), (1, 1, 1), (130, 1024, 7), (5, 33, 256)):
        need = lib.lgcn_score_topk_wide_scratch_bytes(n_users, k, n_splits)
        assert need > 0
        assert call(n_users=n_users, k=k, n_splits=n_splits, scratch_bytes=need - 1) == EINVAL
        assert call(n_users=n_users, k=k, n_splits=n_splits, scratch_bytes=0) == EINVAL
        # the size itself passes every host check: the next one is the scratch's alignment
        assert call(n_users=n_users, k=k, n_splits=n_splits, scratch_bytes=need,
                    scratch=ctypes.c_void_p(258)) == EALIGN


def test_no_users_is_a_no_op(lib):
    call = _wide_call(lib)
    assert call(n_users=0) == 0
    assert call(n_users=0, ue=None, users=None, ie=None, mrow=None, mit=None, scratch=None,
                scratch_bytes=0, top_s=None, top_i=None) == 0
    # k, the sizes and the alignment are checked first (include/lgcn.h)
    assert call(n_users=0, k=1025) == EINVAL
    assert call(n_users=0, d=48) == EINVAL
    assert call(n_users=0, n_splits=257) == EINVAL
    assert call(n_users=0, ld_u=63) == EALIGN


# ----------------------------------------------------------------------------------------------
# helpers and limits
# ----------------------------------------------------------------------------------------------
def test_scratch_bytes(lib):
    f = lib.lgcn_score_topk_wide_scratch_bytes
    for args in ((-1, 10, 1), (4, 0, 1), (4, 1025, 1), (4, -5, 1), (4, 10, 0), (4, 10, 257)):
        assert f(*args) == 0, args
    assert f(0, 10, 1) == 0  # no slot needs no buffer
    ks = list(range(1, 70)) + [100, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024]
    for n, s in ((1, 1), (33, 3), (8192, 16)):
        sizes = [f(n, k, s) for k in ks]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        for k, size in zip(ks, sizes):
            kp = 32
            while kp < k:
                kp *= 2
            assert size == (s * n * (16 * kp + 4) + 15) // 16 * 16  # the header's formula
            assert size >= s * n * k * 8                            # a k-list per (split, slot)
    for k in (1, 100, 1024):
        assert all(f(n, k, 2) < f(n + 1, k, 2) for n in (1, 2, 31, 32, 127, 128, 8191))
        assert all(f(5, k, s) < f(5, k, s + 1) for s in (1, 2, 3, 100, 255))
    assert f(2 ** 31 - 1, 1024, 256) > 2 ** 52  # 64-bit arithmetic


def test_split_rule(lib):
    f = lib.lgcn_topk_wide_splits
    for n_items in (0, 1, 2047, 2048, 4096, 20000, 100000, 4_400_000, 2 ** 31 - 1):
        for k in (1, 20, 32, 33, 100, 256, 257, 1000, 1024):
            for n_cu in (0, 1, 64, 256):
                prev = None
                for n_users in (0, 1, 128, 129, 1024, 8192, 100000):
                    s = f(n_users, n_items, k, n_cu)
                    assert 1 <= s <= 256
                    assert s <= lib.lgcn_eval_splits(n_users, n_items, n_cu)
                    assert s * k <= 16384                              # the merge stays small
                    if s > 1:                                          # the documented length floor
                        assert n_items // s >= max(2048, 8 * k)
                    assert prev is None or s <= prev                   # never grows with n_users
                    prev = s
    # the C3 evaluation shape: more than one split at every k
    assert f(8192, 4_400_000, 20, 256) == lib.lgcn_eval_splits(8192, 4_400_000, 256) == 8
    assert f(8192, 4_400_000, 1024, 256) == 8
    assert f(128, 4_400_000, 1024, 256) == 16 and f(128, 4_400_000, 20, 256) == 256
    # out-of-range k is clamped, not an error: the launch refuses it
    assert f(128, 4_400_000, 0, 256) == f(128, 4_400_000, 1, 256)
    assert f(128, 4_400_000, 5000, 256) == f(128, 4_400_000, 1024, 256)


def test_wide_supported_is_where_the_kernel_does_not_refuse(lib):
    """A supported (d, k) gets as far as LGCN_EALIGN with a misaligned table, no further."""
    assert E.WIDE_MAX_K == MAX_K and E.FUSED_MAX_K == 32
    call = _wide_call(lib)
    for d in (0, 4, 12, 16, 31, 32, 33, 48, 64, 100, 128, 192, 256, 260, 512):
        for k in (-1, 0, 1, 32, 33, 1000, 1024, 1025, 4096):
            rc = call(ue=ctypes.c_void_p(260), d=d, ld_u=max(d, 4), ld_i=max(d, 4), k=k)
            assert rc == (EALIGN if E.wide_supported(d, k) else EINVAL), (d, k)
            assert E.wide_supported(d, k) == (d in E.FUSED_DIMS and 1 <= k <= MAX_K)
            if E.fused_supported(d, k):
                assert E.wide_supported(d, k)


# ----------------------------------------------------------------------------------------------
# the torch route on CPU tensors
# ----------------------------------------------------------------------------------------------
def _tie_case(d):
    rng = np.random.default_rng(900 + d)
    U, I = 50, 400
    ue, ie = few_bits(rng, U, d, lim=2), few_bits(rng, I, d, lim=2)
    ie[100:104] = ie[97]  # equal rows: the index tie-break
    tu, ti = rng.integers(0, U, 300), rng.integers(0, I, 300)
    return U, I, ue, ie, tu, ti


class _Tables(torch.nn.Module):
    def __init__(self, ue, ie):
        super().__init__()
        self.ue, self.ie = ue, ie

    def forward(self, adj):
        return self.ue, self.ie, None, None, None


@pytest.mark.parametrize("d", [12, 64])
def test_torch_route_matches_the_total_order(d):
    U, I, ue, ie, tu, ti = _tie_case(d)
    mrow, mit = E.mask_csr(tu, ti, U)
    users = np.concatenate([np.random.default_rng(d).permutation(U)[:40], [7, 7]])
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    first = topk_total_order(full, 399)[0]
    assert (first[:, :-1] == first[:, 1:]).any(1).all()  # ties in every list
    uet, iet = torch.from_numpy(ue), torch.from_numpy(ie)
    ev = E.Evaluator(tu, ti, U, I, "cpu")
    model = _Tables(uet, iet)
    for k in (1, 33, 399, 400, 401, 1500):  # k > n_items: -inf / -1 behind the last item
        ref = topk_total_order(full, k)
        for bs in (1024, 7):
            s, i = E.topk_total_order_torch(uet, iet, users, mrow, mit, k, batch_size=bs)
            assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.shape == (42, k)
            assert_bitwise((s.numpy(), i.numpy()), ref, f"k={k} bs={bs}")
            s, i = ev.recommend(model, None, users, k, batch_size=bs)
            assert s.device.type == "cpu" and i.dtype == torch.int32
            assert_bitwise((s.numpy(), i.numpy()), ref, f"recommend k={k} bs={bs}")
        if k > I:
            assert (i[:, I:] == -1).all() and torch.isinf(s[:, I:]).all()
    # tensors as arguments, an empty batch, no items
    s, i = E.topk_total_order_torch(uet, iet, torch.from_numpy(users), torch.from_numpy(mrow),
                                    torch.from_numpy(mit), 33)
    assert_bitwise((s.numpy(), i.numpy()), topk_total_order(full, 33), "tensors")
    s, i = E.topk_total_order_torch(uet, iet, [], mrow, mit, 5)
    assert s.shape == i.shape == (0, 5)
    s, i = E.topk_total_order_torch(uet, iet[:0], users[:3], np.zeros(U + 1, np.int32), [], 4)
    assert (i == -1).all() and torch.isinf(s).all()
    # exclude_train=False lists the train items too
    raw = masked_scores64(ue, ie, users, np.zeros(U + 1, np.int32), np.zeros(0, np.int32))
    s, i = ev.recommend(model, None, users, 60, exclude_train=False)
    assert_bitwise((s.numpy(), i.numpy()), topk_total_order(raw, 60), "no mask")
    assert (full == MASKED).any() and not (s == np.float32(MASKED)).any()


def test_a_nan_score_is_never_listed():
    ue = torch.tensor([[1.0, 0.0], [float("nan"), 0.0]])
    ie = torch.tensor([[1.0, 0.0], [float("inf"), 1.0], [3.0, 0.0], [float("nan"), 0.0]])
    mrow, mit = np.zeros(3, np.int32), np.zeros(0, np.int32)
    s, i = E.topk_total_order_torch(ue, ie, [0, 1], mrow, mit, 4)
    assert i.tolist() == [[1, 2, 0, -1], [-1, -1, -1, -1]]
    assert s[0].tolist() == [float("inf"), 3.0, 1.0, float("-inf")]


def test_recommend_refuses_bad_arguments():
    U, I, ue, ie, tu, ti = _tie_case(12)
    mrow, mit = E.mask_csr(tu, ti, U)
    uet, iet = torch.from_numpy(ue), torch.from_numpy(ie)
    ev = E.Evaluator(tu, ti, U, I, "cpu")
    model = _Tables(uet, iet)
    for bad in ([0, U], [-1, 2], torch.tensor([U + 5])):
        with pytest.raises(ValueError):
            ev.recommend(model, None, bad, 10)
        with pytest.raises(ValueError):
            E.topk_total_order_torch(uet, iet, bad, mrow, mit, 10)
    with pytest.raises(ValueError):
        ev.recommend(model, None, [[0, 1]], 10)
    with pytest.raises(ValueError):
        ev.recommend(model, None, [0], 0)
    with pytest.raises(ValueError):
        ev.recommend(model, None, [0], 10, batch_size=0)
    with pytest.raises(engine.LgcnError):
        ev.recommend(model, None, np.array([0.0, 1.0]), 10)
    with pytest.raises(engine.LgcnError):  # an evaluator of another graph
        ev.recommend(_Tables(uet[:5], iet), None, [0], 10)
    # topk_wide is the HIP kernel: CPU tables are refused, not sent to another path
    with pytest.raises(engine.LgcnError):
        E.topk_wide(torch.zeros(U, 64), torch.zeros(I, 64), [0], mrow, mit, 10)
    with pytest.raises(ValueError):
        E.topk_total_order_torch(uet, iet, [0], mrow[:-1], mit, 10)
    assert ev.recommend(model, None, [], 10)[1].shape == (0, 10)


@pytest.mark.parametrize("d", [12, 64])
def test_similar_items_cpu(d):
    _, I, _, ie, _, _ = _tie_case(d)
    items = np.array([97, 100, 103, 0, I - 1, 97])
    rowptr, own = np.arange(I + 1, dtype=np.int32), np.arange(I, dtype=np.int32)
    full = masked_scores64(ie, ie, items, rowptr, own)
    assert_exact(full)
    for k in (5, 450):
        s, i = E.similar_items(torch.from_numpy(ie), items, k)
        assert_bitwise((s.numpy(), i.numpy()), topk_total_order(full, k), f"k={k}")
    i = i.numpy()
    assert i[0, I - 1] == 97 and np.float32(MASKED) == s.numpy()[0, I - 1]  # the query item is last
    assert (i[:, I:] == -1).all()
    # the duplicated rows are each other's neighbours, in index order among equal scores
    near = E.similar_items(torch.from_numpy(ie), [97], 400)[1][0].tolist()
    assert near.index(100) < near.index(101) < near.index(102) < near.index(103)
    with pytest.raises(ValueError):
        E.similar_items(torch.from_numpy(ie), [I], 5)
    with pytest.raises(engine.LgcnError):
        E.similar_items(torch.from_numpy(ie).double(), [0], 5)


@pytest.mark.parametrize("fusion", [False, True])
def test_model_recommend_delegates(fusion):
    from models.lightgcn import LightGCN
    from models.lightgcn_fusion import LightGCN_Fusion
    rng = np.random.default_rng(19)
    U, I, B, d, K, k = 40, 60, 0, 12, 2, 15
    tu, ti = rng.integers(0, U, 250), rng.integers(0, I, 250)
    adj = graph.build_norm_adj(tu, ti, U, I, B, use_brand=False)
    torch.manual_seed(6)
    if fusion:
        model = LightGCN_Fusion(U, I, B, Cfg(d, K),
                                pretrained_item_emb=rng.standard_normal((I, 8)).astype(np.float32))
    else:
        model = LightGCN(U, I, B, Cfg(d, K))
    ev = E.Evaluator(tu, ti, U, I, "cpu")
    users = rng.permutation(U)[:25]
    s, i = model.recommend(adj, users, k, ev)
    assert not model.training and s.shape == i.shape == (25, k)
    with torch.no_grad():
        fu, fi = model(adj)[:2]
    mrow, mit = E.mask_csr(tu, ti, U)
    ws, wi = E.topk_total_order_torch(fu, fi, users, mrow, mit, k)
    assert torch.equal(s, ws) and torch.equal(i, wi)
    for b, u in enumerate(users):
        assert not np.isin(i[b].numpy(), mit[mrow[u]:mrow[u + 1]]).any()
    s2, i2 = model.recommend(adj, users, k, ev, batch_size=4, exclude_train=False)
    ws, wi = E.topk_total_order_torch(fu, fi, users, np.zeros(U + 1, np.int32), [], k)
    assert torch.equal(i2, wi)
