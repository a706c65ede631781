"""What the tests of the two evaluation kernels (tests/test_gpu_eval.py, tests/test_gpu_rank.py,
tests/test_rank_api.py) share: the rank reference, the input builders and the callers of the C ABI
(not a test module)."""
import numpy as np
import torch

from gcn_recommendation_amd import engine, evaluate as E

POISON_IDX = POISON_RANK = -7  # what an int32 output or scratch element holds before the call
POISON_SCORE = 12345.0         # target_score before the call (NaN is one of its values)


def rank_ref(scores, targets):
    """rank_ref[b] = #{i != t : s[b,i] > s[b,t] or (s[b,i] == s[b,t] and i < t)} on a score matrix
    (tests/util.py's masked_scores64): int64 [n]; -1 where t lies outside the row."""
    s = np.asarray(scores)
    t = np.asarray(targets, dtype=np.int64)
    n, m = s.shape
    out = np.full(n, -1, dtype=np.int64)
    ok = np.nonzero((t >= 0) & (t < m))[0]
    if ok.size == 0:
        return out
    st = s[ok, t[ok]][:, None]
    ahead = (s[ok] > st) | ((s[ok] == st) & (np.arange(m)[None, :] < t[ok][:, None]))
    ahead[np.arange(ok.size), t[ok]] = False
    out[ok] = ahead.sum(1)
    return out


def few_bits(rng, n, d, lim=4, den=8.0):
    """Integers in [-lim, lim] / den as fp32: every dot product is exact in fp32 in any order."""
    return (rng.integers(-lim, lim + 1, (n, d)) / den).astype(np.float32)


def random_mask(rng, n_users, n_items, per_user=4):
    n = per_user * n_users
    return E.mask_csr(rng.integers(0, n_users, n), rng.integers(0, n_items, n), n_users)


def assert_exact(scores64):
    """Every score is an fp32 number: with few-bit inputs the reference is the one right answer."""
    assert np.array_equal(scores64.astype(np.float32).astype(np.float64), scores64)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _mask_items(mit, device):
    """The mask's item list on the device; one zero to point at when every list is empty."""
    return dev(np.asarray(mit, dtype=np.int32), device) if len(mit) else \
        torch.zeros(1, dtype=torch.int32, device=device)


def score_topk(device, ue, ie, users, mrow, mit, k, n_splits, n_items=None):
    """lgcn_score_topk through the C ABI on device tensors ue / ie (row views allowed: their
    row strides are ld_u / ld_i). Every output and scratch element starts as a poison value, so
    anything the kernel leaves unwritten shows. Returns host (top_scores, top_idx)."""
    lib = engine.load_library()
    d = ie.shape[1]
    assert ue.shape[1] == d and ue.stride(1) == 1 and ie.stride(1) == 1
    n_items = ie.shape[0] if n_items is None else n_items
    users_t = dev(np.asarray(users, dtype=np.int32), device)
    n = int(users_t.numel())
    mrow_t = dev(np.asarray(mrow, dtype=np.int32), device)
    mit_t = _mask_items(mit, device)
    part_s = torch.full((n_splits, n, k), float("nan"), dtype=torch.float32, device=device)
    part_i = torch.full((n_splits, n, k), POISON_IDX, dtype=torch.int32, device=device)
    top_s = torch.full((n, k), float("nan"), dtype=torch.float32, device=device)
    top_i = torch.full((n, k), POISON_IDX, dtype=torch.int32, device=device)
    P = engine._ptr
    with torch.cuda.device(device):
        rc = lib.lgcn_score_topk(P(ue), ue.stride(0), P(users_t), n, P(ie), ie.stride(0),
                                 n_items, d, P(mrow_t), P(mit_t), k, n_splits, P(part_s),
                                 P(part_i), P(top_s), P(top_i), engine._stream(device))
        assert rc == 0, rc
        torch.cuda.synchronize(device)
    return top_s.cpu().numpy(), top_i.cpu().numpy()


def score_rank(device, ue, ie, users, targets, mrow, mit, n_splits, n_items=None):
    """lgcn_score_rank through the C ABI on device tensors ue / ie (row views allowed: their row
    strides are ld_u / ld_i). Returns host (rank int32 [n], target_score fp32 [n])."""
    lib = engine.load_library()
    d = ie.shape[1]
    assert ue.shape[1] == d and ue.stride(1) == 1 and ie.stride(1) == 1
    n_items = ie.shape[0] if n_items is None else n_items
    users_t = dev(np.asarray(users, dtype=np.int32), device)
    targets_t = dev(np.asarray(targets, dtype=np.int32), device)
    n = int(users_t.numel())
    assert targets_t.numel() == n
    mrow_t = dev(np.asarray(mrow, dtype=np.int32), device)
    mit_t = _mask_items(mit, device)
    part = torch.full((n_splits, n), POISON_RANK, dtype=torch.int32, device=device)
    score = torch.full((n,), POISON_SCORE, dtype=torch.float32, device=device)
    rank = torch.full((n,), POISON_RANK, dtype=torch.int32, device=device)
    P = engine._ptr
    with torch.cuda.device(device):
        rc = lib.lgcn_score_rank(P(ue), ue.stride(0), P(users_t), n, P(ie), ie.stride(0), n_items,
                                 d, P(mrow_t), P(mit_t), P(targets_t), n_splits, P(part), P(score),
                                 P(rank), engine._stream(device))
        assert rc == 0, rc
        torch.cuda.synchronize(device)
    assert (part.cpu().numpy() >= 0).all()  # every split wrote every slot
    return rank.cpu().numpy(), score.cpu().numpy()
