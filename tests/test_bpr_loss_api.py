"""The BPR loss references of tests/util.py without a GPU: bpr_reference on a 2 x 2 case worked by
hand, bpr_reduce_fp32 (k_bpr_reduce restated in numpy float32) on cases whose order of summation
shows and against a float64 sum, and the few-bit generator's exactness claim."""
import numpy as np
import pytest

from util import bpr_reduce_fp32, bpr_reference, fewbit_bpr_case, gamma


def test_bpr_reference_by_hand():
    u = np.array([[1, 2], [0, 0]], dtype=np.float32)
    p = np.array([[3, -1], [5, 5]], dtype=np.float32)
    n = np.array([[1, 1], [7, 7]], dtype=np.float32)
    u0 = np.array([[1, 0], [0, 2]], dtype=np.float32)
    p0 = np.array([[0, 0], [1, 1]], dtype=np.float32)
    n0 = np.array([[2, 2], [0, 0]], dtype=np.float32)
    lam = 0.5
    r = bpr_reference(u, p, n, u0, p0, n0, lam)
    eps = float(np.float32(1e-8))
    # sample 0: <u,p> = 1, <u,n> = 3, x = -2; sample 1: x = 0
    assert r["x"].tolist() == [-2.0, 0.0]
    assert r["mag_x"].tolist() == [3 + 2 + 1 + 2, 0.0]
    s = np.array([1 / (1 + np.exp(2.0)), 0.5])
    assert np.allclose(r["log"], np.log(s + eps), rtol=1e-15, atol=0)
    assert np.allclose(r["c"], -0.5 / (s + eps) * (1 - s) * s, rtol=1e-15, atol=0)
    assert abs(r["c"][1] + 0.25) < 1e-8  # -(1/B) * (1 - s) at s = 1/2, up to the 1e-8
    assert r["sq"].tolist() == [1 + 0 + 8, 4 + 2 + 0]
    assert np.isclose(r["loss"], -np.log(s + eps).mean() + 0.5 * 15 / 2, rtol=1e-15, atol=0)
    # lam is taken as the fp32 the kernel receives
    lam32 = float(np.float32(1e-4))
    assert lam32 != 1e-4
    assert bpr_reference(u, p, n, u0, p0, n0, 1e-4)["loss"] == \
        -np.log(s + eps).mean() + lam32 * 15 / 2


def test_bpr_reference_saturates_without_overflow_warnings():
    u = np.array([[8, 8, 8]] * 2, dtype=np.float32)
    p = np.array([[8, 8, 8], [-8, -8, -8]], dtype=np.float32)
    r = bpr_reference(u, p, -p, u, u, u, 0.0)
    assert r["x"].tolist() == [384.0, -384.0]
    assert r["c"][0] == 0 and abs(r["c"][1]) < 1e-150
    assert r["log"][1] == np.log(np.float64(np.float32(1e-8)))
    assert 0 < r["log"][0] < 1.1e-8


def test_reduce_by_hand():
    f = np.float32
    # B = 2: sl = t0 + t1 via the tree (partials 0 and 1), loss = -(sl/2) + (lam*sr)/2
    t = np.array([1.5, 2.25, 4.0, 6.0], dtype=f)
    assert bpr_reduce_fp32(t, 2, 0.5) == f(-(3.75 / 2) + (0.5 * 10.0) / 2)
    assert bpr_reduce_fp32(np.array([3.0, 7.0], dtype=f), 1, 2.0) == f(-3.0 + 14.0)
    assert isinstance(bpr_reduce_fp32(t, 2, 0.5), np.float32)


def test_reduce_order_is_the_kernels():
    """Values whose fp32 sum depends on the order: 2^24 absorbs a lone 1.0, not 1.0 + 1.0."""
    f = np.float32
    big = f(2.0 ** 24)
    # B = 257: partial 0 = terms[0] + terms[256] (strided), the tree then adds partial 128, ...
    t = np.zeros(2 * 257, dtype=f)
    t[0], t[256], t[128] = big, 1.0, 1.0
    # partial 0 = fl(2^24 + 1) = 2^24; the tree adds partial 128 = 1 -> 2^24 again
    assert bpr_reduce_fp32(t, 257, 0.0) == f(-(big / f(257)))
    t[:] = 0
    t[1], t[129], t[0] = 1.0, 1.0, big
    # partials 1 and 129 meet at tree width 128 (1 + 1 = 2) and reach partial 0 at width 1
    assert bpr_reduce_fp32(t, 257, 0.0) == f(-((big + f(2.0)) / f(257)))
    # lam * sr is rounded before the division
    t[:] = 0
    t[257] = f(1.0) + f(2.0 ** -23)
    lam = f(1.0) + f(2.0 ** -23)
    assert bpr_reduce_fp32(t, 257, lam) == f(-f(0.0)) + f(f(lam * t[257]) / f(257))


@pytest.mark.parametrize("B", [16, 255, 256, 257, 1000])
def test_reduce_within_gamma_of_float64(B):
    rng = np.random.default_rng(B)
    lam = 1e-4
    t = np.concatenate([-np.abs(rng.standard_normal(B)) * 3, rng.standard_normal(B) ** 2 * 50]) \
        .astype(np.float32)
    t64 = t.astype(np.float64)
    lam64 = float(np.float32(lam))
    want = -t64[:B].sum() / B + lam64 * t64[B:].sum() / B
    mag = np.abs(t64[:B]).sum() / B + lam64 * np.abs(t64[B:]).sum() / B
    # a term passes through at most ceil(B/256) + 8 adds, the product, the division and the
    # final add: fewer than B roundings from B = 16 on
    assert abs(float(bpr_reduce_fp32(t, B, lam)) - want) <= gamma(B) * mag


@pytest.mark.parametrize("B,d", [(1, 1), (5, 65), (257, 256)])
def test_fewbit_bpr_generator_is_exact(B, d):
    blocks = fewbit_bpr_case(B, d, seed=1)
    assert len(blocks) == 6 and all(b.shape == (B, d) and b.dtype == np.float32 for b in blocks)
    assert all(np.array_equal(b, np.rint(b)) and np.abs(b).max() <= 8 for b in blocks)
    r = bpr_reference(*blocks, 1e-4)
    # 3 * 256 * 64 < 2^24: every partial sum is an integer fp32 represents
    assert (r["sq"] <= 3 * 256 * 64).all() and (r["mag_x"] <= 2 * 256 * 64).all()
    u, p, n, u0, p0, n0 = blocks
    sq32 = np.zeros(B, dtype=np.float32)
    for k in range(d - 1, -1, -1):
        sq32 = sq32 + n0[:, k] * n0[:, k] + u0[:, k] * u0[:, k] + p0[:, k] * p0[:, k]
    assert np.array_equal(sq32.astype(np.float64), r["sq"])
    x32 = (u * p).sum(1, dtype=np.float32) - (u * n).sum(1, dtype=np.float32)
    assert np.array_equal(x32.astype(np.float64), r["x"])
