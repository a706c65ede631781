"""The recommendation-list kernel lgcn_score_topk_wide (gcn_recommendation_amd/csrc/lgcn_eval.hip:
k_score_topk's tile loop, per-(split, slot) candidate buffers in scratch, a bitonic selection in
LDS when a buffer could overflow, a merge by rank) for k up to 1024.

A. Exact few-bit inputs (every dot product is exact in fp32 in any order, ties are plentiful):
   tests/util.py's topk_total_order on float64 scores is the one right answer and both outputs
   must equal it BITWISE. Each test first asserts that its float64 scores survive an fp32 round
   trip.
B. Gaussian inputs, no tolerance: every listed item's lgcn_score_rank is its place and its
   target_score the listed score as raw bits (k distinct items with ranks 0..k-1 are the top k);
   for k <= 32 the outputs are lgcn_score_topk's; split count, slot order and the run change no
   bit.
C. evaluate.topk_wide / similar_items / Evaluator.recommend and the models' recommend.

The kernel is called through the C ABI (tests/topk_wide_cases.py), which lets a test choose
n_splits, ld_u and ld_i, poisons every output and scratch element and guards the bytes behind the
scratch."""
import functools

import numpy as np
import pytest
import torch

from conftest import Cfg, case_dims, load_case
from eval_cases import assert_exact, dev as _dev, few_bits, random_mask, score_rank, score_topk
from gcn_recommendation_amd import engine, evaluate as E, graph
from topk_wide_cases import assert_bitwise, same_bits, score_topk_wide
from util import MASKED, masked_scores64, topk_total_order

pytestmark = pytest.mark.gpu


def _check_exact(dev, ue, ie, users, mrow, mit, k, n_splits, what="", n_items=None):
    """One exact case end to end; returns the kernel's output and the float64 score matrix."""
    m = ie.shape[0] if n_items is None else n_items
    full = masked_scores64(ue, ie[:m], users, mrow, mit)
    assert_exact(full)
    got = score_topk_wide(dev, _dev(ue, dev), _dev(ie, dev), users, mrow, mit, k, n_splits, m)
    assert_bitwise(got, topk_total_order(full, k), what)
    return got, full


# ----------------------------------------------------------------------------------------------
# A1. widths and k (k = 1024 in one split of 2500 items: a buffer is selected before the end)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _widths_case(d):
    rng = np.random.default_rng(500 + d)
    n_table, n_items = 50, 2500
    ue, ie = few_bits(rng, n_table, d), few_bits(rng, n_items, d)
    users = rng.permutation(n_table)[:33]  # two waves
    mrow, mit = random_mask(rng, n_table, n_items, 6)
    full = masked_scores64(ue, ie, users, mrow, mit)
    full.setflags(write=False)
    first = topk_total_order(full, 64)[0]  # ties are what this input is for
    assert (first[:, :-1] == first[:, 1:]).any(1).mean() > 0.9
    return ue, ie, users, mrow, mit, full


@functools.lru_cache(maxsize=None)
def _widths_ref(d, k):
    return topk_total_order(_widths_case(d)[5], k)


@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("k", [33, 64, 100, 1000, 1024])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_exact_widths_and_k(gpu_device, d, k, n_splits):
    ue, ie, users, mrow, mit, full = _widths_case(d)
    assert_exact(full)
    got = score_topk_wide(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), users, mrow, mit,
                          k, n_splits)
    assert_bitwise(got, _widths_ref(d, k), f"d={d} k={k} splits={n_splits}")


# ----------------------------------------------------------------------------------------------
# A2. several selections per buffer: scores rising / falling / mixed with the item index
# ----------------------------------------------------------------------------------------------
def _trend_case(n_items, trend, seed):
    """few-bit tables whose feature 0 adds trend * item / 2 to every score: rising scores make
    every item a candidate (a selection every (cap - k) / 32 tiles), falling ones none after the
    first k."""
    rng = np.random.default_rng(seed)
    d, n_table = 64, 24
    ue, ie = few_bits(rng, n_table, d), few_bits(rng, n_items, d)
    ue[:, 0] = 4.0
    ie[:, 0] = trend * np.arange(n_items, dtype=np.float32) / 8
    users = rng.permutation(n_table)[:20]
    mrow, mit = random_mask(rng, n_table, n_items, 8)
    return ue, ie, users, mrow, mit


@pytest.mark.parametrize("trend", [1, -1, 0], ids=["rising", "falling", "mixed"])
@pytest.mark.parametrize("k,n_items", [(1024, 5000), (33, 300)])
def test_exact_several_selections(gpu_device, k, n_items, trend):
    ue, ie, users, mrow, mit = _trend_case(n_items, trend, 40 + k)
    (gs, gi), full = _check_exact(gpu_device, ue, ie, users, mrow, mit, k, 1,
                                  f"k={k} items={n_items} trend={trend}")
    assert n_items >= 4 * k  # rising: 2 kp-entry buffers, k kept, so four selections or more
    if trend == 1 and k == 1024:  # the best items are the last ones: the buffers were refilled
        assert (gi[:, :100] >= n_items - k).all()


# ----------------------------------------------------------------------------------------------
# A3. ties: every score equal, the list is 0..k-1
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 3, 7])
def test_exact_all_scores_equal(gpu_device, n_splits):
    d, n_items, k = 32, 5000, 1024
    ue = np.full((5, d), 0.5, np.float32)
    ie = np.full((n_items, d), 0.25, np.float32)
    users = np.array([3, 0, 4, 1, 2, 3])
    mrow, mit = np.zeros(6, np.int32), np.zeros(0, np.int32)
    (gs, gi), _ = _check_exact(gpu_device, ue, ie, users, mrow, mit, k, n_splits,
                               f"splits={n_splits}")
    assert (gi == np.arange(k)).all() and (gs == np.float32(d / 8)).all()


# ----------------------------------------------------------------------------------------------
# A4. item and split geometry: padding, splits shorter than k, empty splits, no items at all
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geometry_tables():
    rng = np.random.default_rng(57)
    return few_bits(rng, 40, 64), few_bits(rng, 2049, 64), rng.permutation(40)[:37]


@pytest.mark.parametrize("n_splits", [1, 2, 5, 256])
@pytest.mark.parametrize("n_items", [0, 1, 31, 32, 33, 99, 100, 101, 2049])
def test_exact_item_and_split_geometry(gpu_device, n_items, n_splits):
    ue, ie, users = _geometry_tables()
    k = 100
    if n_items:
        mrow, mit = random_mask(np.random.default_rng(n_items), 40, n_items,
                                2 if n_items > 1 else 1)
    else:
        mrow, mit = np.zeros(41, np.int32), np.zeros(0, np.int32)
    (gs, gi), _ = _check_exact(gpu_device, ue, ie, users, mrow, mit, k, n_splits,
                               f"items={n_items} splits={n_splits}", n_items=n_items)
    if n_items < k:  # the tail past the last item
        assert (gi[:, n_items:] == -1).all() and np.isneginf(gs[:, n_items:]).all()
        assert (np.sort(gi[:, :n_items], 1) == np.arange(n_items)).all()


# ----------------------------------------------------------------------------------------------
# A5. user geometry: partial waves and blocks, a user in two slots, a permuted batch
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _user_tables():
    rng = np.random.default_rng(58)
    n_table, n_items = 140, 1500
    ue, ie = few_bits(rng, n_table, 64), few_bits(rng, n_items, 64)
    mrow, mit = random_mask(rng, n_table, n_items, 5)
    return ue, ie, mrow, mit


@pytest.mark.parametrize("n_users", [1, 31, 32, 33, 127, 128, 129])
def test_exact_user_geometry(gpu_device, n_users):
    ue, ie, mrow, mit = _user_tables()
    rng = np.random.default_rng(n_users)
    users = rng.permutation(ue.shape[0])[:n_users]
    if n_users > 1:
        users[-1] = users[0]  # one user in two slots
    k = 200
    got, _ = _check_exact(gpu_device, ue, ie, users, mrow, mit, k, 2, f"users={n_users}")
    if n_users > 1:
        assert np.array_equal(got[1][0], got[1][-1])
        perm = rng.permutation(n_users)
        again = score_topk_wide(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device),
                                users[perm], mrow, mit, k, 2)
        assert same_bits((got[0][perm], got[1][perm]), again)


# ----------------------------------------------------------------------------------------------
# A6. masks
# ----------------------------------------------------------------------------------------------
def _mask_case():
    """Items scaled by 2^17 and user 2 by 2^20 more (powers of two: still exact): user 2's scores
    reach +-2^40, far below -1e10. user 0: its best item masked; user 1: every item masked;
    user 2: unmasked scores below -1e10 and a few masked items between them; user 3: a mask list
    longer than k; user 4: no mask."""
    rng = np.random.default_rng(59)
    d, n_items, k = 32, 1500, 50
    ue, ie = few_bits(rng, 5, d), few_bits(rng, n_items, d) * np.float32(2.0 ** 17)
    ue[2] *= np.float32(2.0 ** 20)
    raw = ue.astype(np.float64) @ ie.astype(np.float64).T
    lists = [np.array([np.lexsort((np.arange(n_items), -raw[0]))[0]]),
             np.arange(n_items),
             np.sort(rng.permutation(n_items)[:7]),
             np.sort(rng.permutation(n_items)[:k + 10]),
             np.zeros(0, np.int64)]
    mrow = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    mit = np.concatenate(lists).astype(np.int32)
    return ue, ie, mrow, mit, k, raw, lists


@pytest.mark.parametrize("n_splits", [1, 4])
def test_exact_mask_edges(gpu_device, n_splits):
    ue, ie, mrow, mit, k, raw, lists = _mask_case()
    users = np.arange(5)
    (gs, gi), full = _check_exact(gpu_device, ue, ie, users, mrow, mit, k, n_splits,
                                  f"splits={n_splits}")
    best0 = lists[0][0]
    assert best0 not in gi[0] and raw[0, best0] >= gs[0, 0]         # it would have been first
    assert (gi[1] == np.arange(k)).all() and (gs[1] == np.float32(MASKED)).all()
    # user 2: more than k unmasked scores above -1e10 would hide the case: look at its whole row
    below = (raw[2] < MASKED).sum()
    assert below > 100 and (raw[2] > MASKED).sum() > 100
    n_above = int((full[2] > MASKED).sum())
    gs2, gi2 = score_topk_wide(gpu_device, _dev(ue, gpu_device), _dev(ie, gpu_device), [2], mrow,
                               mit, 1024, n_splits)
    assert_bitwise((gs2, gi2), topk_total_order(full[2:3], 1024), "user 2, k = 1024")
    assert n_above + 7 < 1024 and sorted(gi2[0, n_above:n_above + 7]) == lists[2].tolist()
    assert (gs2[0, n_above + 7:] < np.float32(MASKED)).all()        # they rank after the masked
    assert not np.isin(gi[3], lists[3]).any()
    # no mask at all: mask_items points at one zero
    _check_exact(gpu_device, ue, ie, users, np.zeros(6, np.int32), np.zeros(0, np.int32), k,
                 n_splits, "empty mask")


# ----------------------------------------------------------------------------------------------
# A7. strides and aliasing
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 128])
def test_exact_row_strides_and_one_allocation(gpu_device, d):
    rng = np.random.default_rng(60 + d)
    U, I, k = 40, 900, 70
    ue, ie = few_bits(rng, U, d), few_bits(rng, I, d)
    mrow, mit = random_mask(rng, U, I, 5)
    users = rng.permutation(U)[:35]
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    ref = topk_total_order(full, k)
    # ld > d: both tables as column windows of wider ones, the rest poisoned
    wu = torch.full((U, d + 8), float("nan"), device=gpu_device)
    wi = torch.full((I, d + 12), float("nan"), device=gpu_device)
    wu[:, 4:4 + d] = _dev(ue, gpu_device)
    wi[:, 8:8 + d] = _dev(ie, gpu_device)
    got = score_topk_wide(gpu_device, wu[:, 4:4 + d], wi[:, 8:8 + d], users, mrow, mit, k, 3)
    assert_bitwise(got, ref, "ld > d")
    # both tables as row views of one allocation
    both = torch.cat([_dev(ue, gpu_device), _dev(ie, gpu_device)])
    got = score_topk_wide(gpu_device, both[:U], both[U:], users, mrow, mit, k, 2)
    assert_bitwise(got, ref, "one allocation")


def test_similar_items_is_the_item_table_against_itself(gpu_device):
    rng = np.random.default_rng(61)
    I, d, k = 700, 64, 120
    ie = few_bits(rng, I, d)
    items = rng.permutation(I)[:45]
    rowptr, own = np.arange(I + 1, dtype=np.int32), np.arange(I, dtype=np.int32)
    full = masked_scores64(ie, ie, items, rowptr, own)
    assert_exact(full)
    iet = _dev(ie, gpu_device)
    s, i = E.similar_items(iet, items, k)
    assert s.device == gpu_device and s.dtype == torch.float32 and i.dtype == torch.int32
    assert_bitwise((s.cpu().numpy(), i.cpu().numpy()), topk_total_order(full, k), "similar_items")
    assert not (i.cpu().numpy() == items[:, None]).any()  # a query item is not its own neighbour
    # the same call through the C ABI with user_emb == item_emb
    got = score_topk_wide(gpu_device, iet, iet, items, rowptr, own, k, 2)
    assert same_bits(got, (s.cpu().numpy(), i.cpu().numpy()))
    with pytest.raises(ValueError):
        E.similar_items(iet, [0, I], k)


# ----------------------------------------------------------------------------------------------
# B. Gaussian inputs
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss_case(d):
    rng = np.random.default_rng(700 + d)
    U, I = 30, 3000
    ue = (0.1 * rng.standard_normal((U, d))).astype(np.float32)
    ie = (0.1 * rng.standard_normal((I, d))).astype(np.float32)
    mrow, mit = random_mask(rng, U, I, 9)
    users = rng.permutation(U)[:16]
    return ue, ie, users, mrow, mit


@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_every_listed_item_ranks_at_its_place(gpu_device, d):
    ue, ie, users, mrow, mit = _gauss_case(d)
    k = 300
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    gs, gi = score_topk_wide(gpu_device, uet, iet, users, mrow, mit, k, 3)
    assert (gi >= 0).all() and all(np.unique(row).size == k for row in gi)
    rank, score = score_rank(gpu_device, uet, iet, np.repeat(users, k), gi.reshape(-1), mrow, mit, 2)
    assert np.array_equal(rank.reshape(-1, k), np.tile(np.arange(k), (len(users), 1)))
    assert np.array_equal(score.view(np.uint32), gs.reshape(-1).view(np.uint32))
    assert all(not np.isin(gi[b], mit[mrow[u]:mrow[u + 1]]).any() for b, u in enumerate(users))


@pytest.mark.parametrize("k", [1, 20, 32])
@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_small_k_is_lgcn_score_topk(gpu_device, d, k):
    ue, ie, users, mrow, mit = _gauss_case(d)
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    wide = score_topk_wide(gpu_device, uet, iet, users, mrow, mit, k, 3)
    narrow = score_topk(gpu_device, uet, iet, users, mrow, mit, k, 2)
    assert same_bits(wide, narrow)


@pytest.mark.parametrize("d", [32, 256])
def test_gaussian_bits_do_not_depend_on_splits_slots_or_runs(gpu_device, d):
    ue, ie, users, mrow, mit = _gauss_case(d)
    k = 300
    uet, iet = _dev(ue, gpu_device), _dev(ie, gpu_device)
    base = score_topk_wide(gpu_device, uet, iet, users, mrow, mit, k, 1)
    for n_splits in (1, 4, 37):
        assert same_bits(base, score_topk_wide(gpu_device, uet, iet, users, mrow, mit, k, n_splits))
    perm = np.random.default_rng(1).permutation(len(users))
    moved = score_topk_wide(gpu_device, uet, iet, users[perm], mrow, mit, k, 4)
    assert same_bits((base[0][perm], base[1][perm]), moved)


# ----------------------------------------------------------------------------------------------
# C. the Python layer
# ----------------------------------------------------------------------------------------------
class _Tables(torch.nn.Module):
    """A model whose propagation returns two given tables."""

    def __init__(self, ue, ie):
        super().__init__()
        self.ue, self.ie = ue, ie

    def forward(self, adj):
        return self.ue, self.ie, None, None, None


def test_evaluator_recommend_on_exact_tables(gpu_device, monkeypatch):
    dev = gpu_device
    rng = np.random.default_rng(62)
    U, I, d, k = 90, 1300, 64, 150
    ue, ie = few_bits(rng, U, d), few_bits(rng, I, d)
    tu, ti = rng.integers(0, U, 700), rng.integers(0, I, 700)
    mrow, mit = E.mask_csr(tu, ti, U)
    ev = E.Evaluator(tu, ti, U, I, dev)
    uet, iet = _dev(ue, dev), _dev(ie, dev)
    model = _Tables(uet, iet)
    users = np.concatenate([rng.permutation(U)[:70], [3, 3]])
    full = masked_scores64(ue, ie, users, mrow, mit)
    assert_exact(full)
    want_s, want_i = E.topk_total_order_torch(torch.from_numpy(ue), torch.from_numpy(ie), users,
                                              mrow, mit, k)
    assert_bitwise((want_s.numpy(), want_i.numpy()), topk_total_order(full, k), "the torch route")

    launches = []
    real = E._wide_launch
    monkeypatch.setattr(E, "_wide_launch", lambda *a: (launches.append(a[2].numel()), real(*a)))
    # no host synchronisation once the ids are on the device
    for bs, sizes in ((8192, [72]), (32, [32, 32, 8])):
        launches.clear()
        s, i = ev.recommend(model, None, users, k, batch_size=bs)
        assert launches == sizes
        assert s.device == dev and i.device == dev
        assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.shape == i.shape == (72, k)
        assert torch.equal(s.cpu(), want_s) and torch.equal(i.cpu(), want_i)
    assert model.training is False
    # device-resident ids, and E.topk_wide directly
    s2, i2 = ev.recommend(model, None, _dev(users, dev), k)
    assert torch.equal(s2, s) and torch.equal(i2, i)
    s3, i3 = E.topk_wide(uet, iet, users, mrow, mit, k)
    assert torch.equal(s3, s) and torch.equal(i3, i)

    # exclude_train=False: the lists differ exactly by the masked items
    sa, ia = ev.recommend(model, None, users, k, exclude_train=False)
    raw = masked_scores64(ue, ie, users, np.zeros(U + 1, np.int32), np.zeros(0, np.int32))
    assert_bitwise((sa.cpu().numpy(), ia.cpu().numpy()), topk_total_order(raw, k), "no mask")
    ia, i = ia.cpu().numpy(), i.cpu().numpy()
    some = 0
    for b, u in enumerate(users):
        train = mit[mrow[u]:mrow[u + 1]]
        gone = np.setdiff1d(ia[b], i[b])
        assert np.isin(gone, train).all()
        keep = ia[b][~np.isin(ia[b], train)]
        assert np.array_equal(keep, i[b][:keep.size])  # the others keep their order
        some += gone.size
    assert some > 20

    for bad in ([0, U], [-1], np.array([0.5])):
        with pytest.raises((ValueError, engine.LgcnError)):
            ev.recommend(model, None, bad, k)
    with pytest.raises(ValueError):
        ev.recommend(model, None, [0, U], k)
    # a k or a width the kernel does not have goes to the torch route
    s, i = ev.recommend(model, None, users[:5], 1100)
    assert s.shape == (5, 1100) and s.device == dev
    assert_bitwise((s.cpu().numpy(), i.cpu().numpy()), topk_total_order(full[:5], 1100), "k=1100")
    with pytest.raises(engine.LgcnError):
        E.topk_wide(uet, iet, users, mrow, mit, 1100)


@pytest.mark.parametrize("name,fusion", [("c1_brand", False), ("c1_fusion", True)])
def test_model_recommend(gpu_device, name, fusion):
    from models.lightgcn import LightGCN
    from models.lightgcn_fusion import LightGCN_Fusion
    dev = gpu_device
    z = load_case(name)
    U, I, B, d, K = case_dims(z)
    k = 100
    assert E.wide_supported(d, k)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]), device=dev)
    torch.manual_seed(3)
    if fusion:
        model = LightGCN_Fusion(U, I, B, Cfg(d, K), pretrained_item_emb=z["content"]).to(dev)
    else:
        model = LightGCN(U, I, B, Cfg(d, K)).to(dev)
    ev = E.Evaluator(z["train_user"], z["train_item"], U, I, dev)
    users = np.random.default_rng(4).permutation(U)[:200]
    s, i = model.recommend(adj, users, k, ev, batch_size=128)
    assert s.shape == i.shape == (200, k) and i.dtype == torch.int32 and i.device == dev
    assert not model.training
    with torch.no_grad():
        fu, fi = model(adj)[:2]
    mrow, mit = E.mask_csr(z["train_user"], z["train_item"], U)
    # every listed item ranks at its place on the model's own tables (the first 40 users)
    gi = i[:40].cpu().numpy()
    rank, score = score_rank(dev, fu.contiguous(), fi.contiguous(), np.repeat(users[:40], k),
                             gi.reshape(-1), mrow, mit, 2)
    assert np.array_equal(rank.reshape(-1, k), np.tile(np.arange(k), (40, 1)))
    assert np.array_equal(score.view(np.uint32), s[:40].cpu().numpy().reshape(-1).view(np.uint32))
    for b, u in enumerate(users[:40]):
        assert not np.isin(gi[b], mit[mrow[u]:mrow[u + 1]]).any()
