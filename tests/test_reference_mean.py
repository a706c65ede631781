"""The reference's final step, torch.mean(torch.stack([E0..EK], 0), 0) (models/lightgcn.py:54), as
ATen's CPU sum kernel runs it — pinned here because the engine's MEAN epilogue and the oracle sum
E0..EK one after the other, and the claim "bitwise the reference" holds exactly as far as ATen
does the same.

Measured: for 2..17 stacked layers ATen sums them in order, except on the last n*d mod W elements
of the flattened [n x d] result, where its scalar row_sum interleaves four partial sums
(util.stacked_mean_torch_order). With <= 4 layers the two orders are one. With 18 layers ATen
cascades everywhere: the reason the engine stops at K = 16. W belongs to the ATen build: the
tests find it and state the value they found (DESIGN §3 records it)."""
import numpy as np
import pytest
import torch

from oracle import oracle
from util import stacked_mean_torch_order

WIDTHS = (16, 32, 64)
# n*d mod 64: 24, 15, 31, 0, 21, 49 — [199 x 7] tells 32 from both 16 and 64
SHAPES = [(1000, 7), (3, 5), (33, 2047), (257, 64), (41, 13), (199, 7)]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stack(shape, n_layers):
    rng = np.random.default_rng(1000 * n_layers + shape[0])
    xs = [rng.standard_normal(shape).astype(np.float32) for _ in range(n_layers)]
    for x in xs:                      # an element that is -0 in every layer: both orders start
        x.reshape(-1)[[0, -1]] = -0.0  # from +0, so its mean is +0 (below the cut and in the tail)
    return xs


def _torch_mean(xs):
    return torch.mean(torch.stack([torch.from_numpy(x) for x in xs], 0), 0).numpy()


def _sequential(xs):
    return stacked_mean_torch_order(xs, 1)      # cut = n*d: no tail


def _explaining_widths():
    """The widths of WIDTHS for which the helper is torch's mean, bit for bit, for 2..17 layers
    at every shape of SHAPES."""
    if "widths" not in _cache:
        ok = set(WIDTHS)
        for shape in SHAPES:
            for n_layers in range(2, 18):
                xs = _stack(shape, n_layers)
                want = _bits(_torch_mean(xs))
                ok = {w for w in ok if np.array_equal(_bits(stacked_mean_torch_order(xs, w)), want)}
        _cache["widths"] = sorted(ok)
    return _cache["widths"]


def tail_width():
    ws = _explaining_widths()
    assert ws, f"no tail width of {WIDTHS} explains torch {torch.__version__}'s mean"
    return ws[0]


def test_torch_mean_is_sequential_with_an_interleaved_tail():
    ws = _explaining_widths()
    print(f"torch {torch.__version__} ({torch.backends.cpu.get_cpu_capability()}): "
          f"tail width(s) {ws}")
    assert ws, f"no tail width of {WIDTHS} explains every shape"
    w = ws[0]
    # what the width means: up to four layers there is no tail at all, from five on the tail
    # is where the mean leaves the sequential sum
    for shape in SHAPES:
        m = shape[0] * shape[1]
        for n_layers in (2, 3, 4, 5, 9, 17):
            xs = _stack(shape, n_layers)
            got, seq = _bits(_torch_mean(xs)).reshape(-1), _bits(_sequential(xs)).reshape(-1)
            cut = m - m % w
            assert np.array_equal(got[:cut], seq[:cut]), (shape, n_layers)
            if n_layers <= 4:
                assert np.array_equal(got, seq), (shape, n_layers)
        xs = _stack(shape, 2)
        assert (_bits(_torch_mean(xs)).reshape(-1)[[0, -1]] == 0).all()   # -0 + -0 from +0
    # [1000 x 7] has a tail of 7000 mod w elements and they do differ
    xs = _stack((1000, 7), 17)
    assert not np.array_equal(_bits(_torch_mean(xs)), _bits(_sequential(xs)))


def test_eighteen_layers_are_neither():
    """The depth limit: with 18 stacked layers (K = 17) ATen's cascade rounds differently from
    the sequential sum all over the table, so K stops at 16 (LGCN_MAX_LAYERS)."""
    xs = _stack((257, 64), 18)
    got = _bits(_torch_mean(xs))
    seq = _bits(_sequential(xs))
    assert not np.array_equal(got, seq)
    assert not np.array_equal(got, _bits(stacked_mean_torch_order(xs, tail_width())))
    differ = got != seq
    print(f"18 layers at [257 x 64]: {int(differ.sum())} of {differ.size} elements differ")
    assert differ.reshape(-1)[:256].any()     # no tail effect: the head of the table differs too
    xs17 = _stack((257, 64), 17)      # one layer fewer: sequential everywhere (257*64 % 64 == 0)
    assert np.array_equal(_bits(_torch_mean(xs17)), _bits(_sequential(xs17)))


# ---- the oracle against the reference's own torch ops ------------------------------------------
N_ROWS = 199      # 199*7 % 64 = 49, 199*13 % 64 = 27: a tail for every candidate width


def _graph():
    """199 rows, ~3,000 symmetric unique nonzeros in the reference's layout (row-sorted), rows
    190..198 and a few others without an edge."""
    if "graph" not in _cache:
        rng = np.random.default_rng(77)
        live = np.setdiff1d(np.arange(190), [0, 17, 101])
        r, c = rng.choice(live, 1600), rng.choice(live, 1600)
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
        key = np.unique(r * N_ROWS + c)
        r, c = key // N_ROWS, key % N_ROWS
        lo = np.minimum(r, c) * N_ROWS + np.maximum(r, c)
        _, inv = np.unique(lo, return_inverse=True)
        v = (rng.uniform(0.02, 0.3, inv.max() + 1).astype(np.float32))[inv]
        assert 2000 < key.size < 4000 and (np.bincount(r, minlength=N_ROWS) == 0).sum() >= 12
        _cache["graph"] = (r, c, v)
    return _cache["graph"]


@pytest.mark.parametrize("K", [0, 1, 2])
def test_sum_starts_from_plus_zero(K):
    """ATen's sum starts from +0, so an element that is -0 in every stacked layer has the mean
    +0: at K = 0 a -0 of E0, at K = 1 a -0 of E0 whose chain underflowed to -0 (row 0: one edge
    of weight 0.01 into a row holding the smallest negative subnormal). The oracle does the
    same."""
    e0 = np.array([[-0.0, 1.0], [-1e-45, -0.0]], np.float32)
    r, c, v = np.array([0]), np.array([1]), np.array([0.01], np.float32)
    adj = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.from_numpy(v), (2, 2))
    want = oracle.reference_forward_torch(adj, torch.from_numpy(e0), K).numpy()
    got, layers = oracle.forward(r, c, v, e0, K, return_layers=True)
    if K >= 1:
        assert _bits(layers[0])[0, 0] == 0x80000000      # E1[0, 0] = fma(0.01, -1e-45, +0) = -0
    assert _bits(want)[0, 0] == 0 and _bits(want)[1, 1] == 0
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("K", [0, 1, 3, 4, 5, 8, 16])
@pytest.mark.parametrize("d", [7, 13, 64])
def test_oracle_is_torch_outside_the_tail(d, K):
    r, c, v = _graph()
    n = N_ROWS
    w = tail_width()
    assert d == 64 or (n * d) % 64 != 0
    e0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    e0[[17, 195]] = -0.0      # rows without an edge, the second inside the tail: their mean is +0
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([r, c])), torch.from_numpy(v), (n, n))
    want = oracle.reference_forward_torch(adj, torch.from_numpy(e0), K).numpy()
    got, layers = oracle.forward(r, c, v, e0, K, return_layers=True)
    x = torch.from_numpy(e0)
    for k in range(K):                      # E1..EK: torch.sparse.mm, layer by layer
        x = torch.sparse.mm(adj, x)
        assert np.array_equal(_bits(layers[k]), _bits(x.numpy())), f"E{k + 1}"
    cut = n * d - (n * d) % w
    gb, wb = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert np.array_equal(gb[:cut], wb[:cut])
    if K <= 3:
        assert np.array_equal(gb, wb)
    if K >= 1:    # the tail: ATen's interleaved order over the oracle's own layers
        ref = _bits(stacked_mean_torch_order([e0] + list(layers), w)).reshape(-1)
        assert np.array_equal(ref, wb)
