"""What tests/test_rank_api.py and tests/test_gpu_rank.py share: the rank reference and the input
builders (not a test module)."""
import numpy as np

from gcn_recommendation_amd import evaluate as E


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
