"""The weighted draw on the HIP device: lgcn_bpr_sample_weighted against the numpy twin
(sampler.sample_numpy with cumw) — all three outputs and the counter, bit for bit — over random
cases, the edge users, order windows, malformed slots, grid-stride boundaries and a side stream;
and with unit weights against lgcn_bpr_sample_multi."""
import functools

import numpy as np
import pytest
import torch

from gcn_recommendation_amd import engine, sampler
from sampler_cases import random_case as uniform_random_case
from weighted_cases import EDGE_LISTS, EDGE_SAMPLES, EPOCH, SEED, edge_case, random_case

pytestmark = pytest.mark.gpu

NS = (None, 1, 5, 64)


def _kernel(dev, c, n_neg, order=None, first=0, count=None, cumw="own", inter_user=None):
    iu, ii, rowptr, items = (torch.tensor(a).to(dev) for a in (
        c.user if inter_user is None else inter_user, c.item, c.rowptr, c.pos_items))
    if cumw == "own":
        cumw = c.cumw
    tables = None if cumw is None else tuple(torch.tensor(a).to(dev) for a in cumw)
    total = len(c) if order is None else len(order)
    count = total - first if count is None else count
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    o = None if order is None else torch.tensor(order, dtype=torch.int64).to(dev)
    out = sampler.sample_device(iu, ii, o, first, count, rowptr, items, c.U, c.I, SEED, EPOCH,
                                counter, n_neg=n_neg, cumw=tables)
    return [t.cpu().numpy() for t in out], int(counter.item())


@functools.lru_cache(maxsize=None)
def _reference(name, n_neg):
    """The numpy twin's whole draw of a case at n_neg, computed once and never modified."""
    c = random_case(name) if isinstance(name, int) else edge_case(name)
    u, p, n, missed = sampler.sample_numpy(c.user, c.item, None, 0, len(c), c.rowptr, c.pos_items,
                                           c.U, c.I, SEED, EPOCH, n_neg=n_neg, cumw=c.cumw)
    for a in (u, p, n):
        a.setflags(write=False)
    return c, u, p, n, missed


def _assert_same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("n_neg", NS)
@pytest.mark.parametrize("name", [1, 37, 300] + sorted(EDGE_LISTS))
def test_draw_equals_numpy_twin(gpu_device, name, n_neg):
    c, u, p, n, missed = _reference(name, n_neg)
    got, counted = _kernel(gpu_device, c, n_neg)
    assert got[2].shape == ((len(c),) if n_neg is None else (len(c), n_neg))
    _assert_same(got, (u, p, n))
    edge = c.user == 1
    if name in ("every_item_positive", "free_weight_zero"):
        assert counted == missed == EDGE_SAMPLES and (n[edge] == -1).all() and (n[~edge] >= 0).all()
    elif isinstance(name, str):
        assert counted == missed == 0 and (n >= 0).all()
    else:   # user by user: -1 exactly where no free item has weight
        free_w = np.array([c.weights.sum() - c.weights[c.positives(x)].sum() for x in range(c.U)])
        dead = free_w[c.user] == 0
        assert counted == missed == dead.sum()
        assert ((n.reshape(len(c), -1) == -1).all(1) == dead).all()
    assert (c.weights[n[n >= 0]] > 0).all()
    # an order with a window
    order = np.random.default_rng(8).permutation(len(c))
    got, _ = _kernel(gpu_device, c, n_neg, order=order, first=37, count=130)
    sel = order[37:167]
    _assert_same(got, (u[sel], p[sel], n[sel]))


def test_malformed_slots_leave_their_neighbours_alone(gpu_device):
    c, u, p, n, _ = _reference(37, 5)
    order = np.arange(200)
    bad_order = [3, 64, 199]
    order[bad_order] = [-1, len(c), 1 << 40]
    bad_user = [10, 63, 128]
    user = c.user.copy()
    user[bad_user] = [-1, c.U, 1 << 30]
    got, counted = _kernel(gpu_device, c, 5, order=order, inter_user=user)
    bad = sorted(bad_order + bad_user)
    keep = np.setdiff1d(np.arange(200), bad)
    for g, w in zip(got, (u, p, n)):
        assert (g[bad] == -1).all() and np.array_equal(g[keep], w[keep])
    assert counted == (n[keep] == -1).all(1).sum()   # malformed slots are not "unsampled"
    # identity order past the end of the interactions
    got, _ = _kernel(gpu_device, c, 5, first=len(c) - 2, count=5)
    assert (got[2][2:] == -1).all() and (got[0][2:] == -1).all()
    assert np.array_equal(got[2][:2], n[len(c) - 2:])


@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_draw_does_not_depend_on_the_grid(gpu_device, blocks):
    lib = engine.load_library()
    c, u, p, n, _ = _reference(300, 5)
    order = np.random.default_rng(6).integers(0, len(c), 2049)
    old = lib.lgcn_tune(engine.TUNE_SAMPLE_BLOCKS, blocks)   # 0: the default, a block per 256
    try:
        for count in (255, 256, 257, 2049):   # at one block: up to 9 grid-stride passes
            got, _ = _kernel(gpu_device, c, 5, order=order, count=count)
            sel = order[:count]
            _assert_same(got, (u[sel], p[sel], n[sel]))
    finally:
        lib.lgcn_tune(engine.TUNE_SAMPLE_BLOCKS, old)


@pytest.mark.parametrize("n_neg", NS)
def test_unit_weights_are_the_uniform_kernel(gpu_device, n_neg):
    c = uniform_random_case()
    cumw = sampler.cumulative_weights(np.ones(c.I, dtype=np.int64), c.pos_items)
    order = np.random.default_rng(2).permutation(len(c))
    want, missed = _kernel(gpu_device, c, n_neg, order=order, cumw=None)
    got, counted = _kernel(gpu_device, c, n_neg, order=order, cumw=cumw)
    _assert_same(got, want)
    assert counted == missed == 0


def test_sampler_object_routes_to_the_weighted_kernel(gpu_device):
    dev = gpu_device
    c, u, p, n, missed = _reference(300, 5)
    s = sampler.BprSampler(c.user, c.item, c.U, c.I, dev, seed=SEED, weights=c.weights)
    ref = sampler.BprSampler(c.user, c.item, c.U, c.I, "cpu", seed=SEED, weights=c.weights)
    got = s.draw(EPOCH, n_neg=5)
    assert all(t.device == dev and t.dtype == torch.int64 for t in got) and got[2].is_contiguous()
    _assert_same([t.cpu().numpy() for t in got], (u, p, n))
    assert s.unsampled.item() == missed
    assert torch.equal(s.draw(EPOCH)[2], got[2][:, 0]) and s.draw(EPOCH)[2].dim() == 1
    assert s.draw(EPOCH, n_neg=3, first=len(c))[2].shape == (0, 3)
    # an epoch: the device permutation is an input; the draw under it is the twin's
    perm = s.permutation(2)
    want = ref.draw(2, order=perm.cpu(), n_neg=4)
    seen = [torch.cat(x) for x in zip(*s.epoch(2, 256, n_neg=4))]
    for g, w in zip(seen, want):
        assert torch.equal(g.cpu(), w)
    q = s.neg_log_q()
    assert q.device == dev and torch.equal(q.cpu(), ref.neg_log_q())
    uniform = sampler.BprSampler(c.user, c.item, c.U, c.I, dev, seed=SEED)
    assert not torch.equal(uniform.draw(EPOCH, n_neg=5)[2], got[2])


def test_work_is_issued_on_the_current_stream(gpu_device):
    dev = gpu_device
    c, u, p, n, missed = _reference(300, 5)
    s = sampler.BprSampler(c.user, c.item, c.U, c.I, dev, seed=SEED, weights=c.weights)
    a = torch.randn(8192, 8192, device=dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    # The default stream is kept busy for tens of milliseconds; the draw and its read-back are
    # issued on the side stream and only that stream is waited for. A kernel launched on the
    # default stream instead would still be queued behind the matmuls when the copies run.
    for _ in range(16):
        a @ a
    with torch.cuda.stream(side):
        got = s.draw(EPOCH, n_neg=5)
        host = [torch.empty(g.shape, dtype=g.dtype, pin_memory=True) for g in got]
        for h, g in zip(host, got):
            h.copy_(g, non_blocking=True)
        count = torch.empty(1, dtype=torch.int32, pin_memory=True)
        count.copy_(s.unsampled, non_blocking=True)
    side.synchronize()
    _assert_same([h.numpy() for h in host], (u, p, n))
    assert count.item() == missed
    torch.cuda.synchronize(dev)
