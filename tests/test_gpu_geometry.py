"""Every launch geometry and every depth the propagation claims to be bitwise, against
the oracle (the reference's CPU arithmetic), compared as uint32.

  * Width classes: a list of d that lands on all 18 (vector type, G, NV) cells of dispatch_geo
    (csrc/lgcn_kernels.h), odd widths from 3 to 2047, vector widths from 12 to 2048 and a 4-byte
    misaligned base at d = 256 / 1024 / 2048 — asserted by a restatement of pick_geo, so the list
    cannot rot into covering fewer. One small graph (301 rows, a row of 40 edges, a row of ~300,
    a few empty rows) serves all of them: with hub_threshold=8, emu_min=16 its rows run as
    bundles, whole-row chains, chain rows and emulated blocks, with hub_mode="chunk" through
    k_hub_combine.
  * Depths: K = 5, 8, 16 (the MEAN epilogue's generic loop with up to 15 dense layers) on the
    one-operator and the two-lane schedule; K = 17 raises.
  * The bundle ladder of launch_layer_t: every rung RPG = 1, 2, 4, 8, RB with a ragged last
    bundle, chosen through LGCN_TUNE_MIN_GROUPS — asserted by a restatement of the choice.
  * The seven explicit d = 64 (rows per group, gathers in flight) variants behind lgcn_tune.

Only the chunk plan is not bitwise: it is compared at the north_star tolerance and with itself."""
import numpy as np
import pytest
import torch

from gcn_recommendation_amd import engine
from oracle import oracle
from util import assert_close_normwise

from test_gpu_exact import _adj

pytestmark = pytest.mark.gpu

PLAIN = dict(hub_threshold=engine.INT32_MAX)
EXACT = dict(hub_threshold=8, hub_mode="exact", emu_min=16)
_cache = {}


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def _dev(a, dev, misaligned=False):
    """`a` on the device; misaligned: as a view 4 bytes into a buffer (no 16-B aligned row)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if not misaligned:
        return t
    big = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    big[1:] = t.reshape(-1)
    mis = big[1:].view(*t.shape)
    assert mis.data_ptr() % 16 != 0
    return mis


class _Tune:
    """lgcn_tune knobs set for a block and put back after it."""

    KNOBS = (engine.TUNE_ROWS_PER_GROUP, engine.TUNE_UNROLL, engine.TUNE_MEAN_PREFETCH,
             engine.TUNE_MIN_GROUPS)

    def __enter__(self):
        self.lib = engine.load_library()
        self.saved = [(k, self.lib.lgcn_tune(k, -1)) for k in self.KNOBS]
        return self

    def set(self, knob, value):
        self.lib.lgcn_tune(knob, value)
        assert self.lib.lgcn_tune(knob, -1) == value

    def __exit__(self, *exc):
        for k, v in self.saved:
            self.lib.lgcn_tune(k, v)
        return False


# ---- restatements of the host-side dispatch (csrc/lgcn_kernels.h) --------------------------------
def _next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def pick_geo(d, vec_ok):
    """(vector type, G, NV, dW) of pick_geo."""
    vec = vec_ok and d % 4 == 0
    dW = d // 4 if vec else d
    G = min(max(_next_pow2(dW), 4), 64)
    NV = _next_pow2((dW + G - 1) // G)
    return ("float4" if vec else "float", G, NV, dW)


CELLS = {("float4", G, NV) for G, NV in ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2),
                                         (64, 4), (64, 8))} | \
        {("float", G, NV) for G, NV in ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4),
                                        (64, 8), (64, 16), (64, 32))}


def pick_rung(mean, G, NV, dW, n_rows, min_groups, prefetch, n_prev):
    """Rows per group that launch_layer_t chooses (knobs LGCN_TUNE_ROWS_PER_GROUP / _UNROLL at 0);
    mean: the MEAN epilogue (its bundle prefetch has rungs of its own)."""
    RB = 15 if G >= 16 else G - 1
    per = n_rows // (min_groups if min_groups > 0 else 65536)
    if RB <= 1 or per < 2:
        return 1
    if mean and NV == 1 and 4 <= G <= 8:          # LGCN_MEAN_PF_MAX_G = 8
        RM = 4 if G >= 8 else RB
        if prefetch != 2 and per >= RM and dW & (dW - 1) == 0 and n_prev in (2, 3, 4):
            return RM
    for r in (RB, 8, 4, 2):
        if RB >= r and per >= r:
            return r
    return 1


# ---- width classes -------------------------------------------------------------------------------
ODD = [3, 7, 13, 31, 63, 127, 255, 257, 511, 513, 1023, 1025, 2046, 2047]
VEC = [12, 16, 20, 32, 64, 100, 128, 256, 512, 516, 1024, 1028, 2044, 2048]
MISALIGNED = [256, 1024, 2048]
WIDTH_CASES = [(d, False) for d in ODD + VEC] + [(d, True) for d in MISALIGNED]
N_W = 301
W_EMPTY = [0, 57, 150, 299, 300]
W_HUB40, W_HUB300 = 11, 203


def _symmetric(r, c, n, rng):
    """The reference's layout: both directions, row-sorted, unique, symmetric values."""
    r, c = np.concatenate([r, c]), np.concatenate([c, r])
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    lo = np.minimum(r, c) * n + np.maximum(r, c)
    _, inv = np.unique(lo, return_inverse=True)
    v = rng.standard_normal(inv.max() + 1).astype(np.float32)[inv]
    return r, c, v


def _width_graph():
    if "wg" not in _cache:
        rng = np.random.default_rng(41)
        live = np.setdiff1d(np.arange(N_W), W_EMPTY)
        others = np.setdiff1d(live, [W_HUB40, W_HUB300])
        r = np.concatenate([rng.choice(others, 900), np.full(38, W_HUB40),
                            np.full(live.size, W_HUB300)])
        c = np.concatenate([rng.choice(others, 900), rng.choice(others, 38, replace=False), live])
        r, c, v = _symmetric(r, c, N_W, rng)
        deg = np.bincount(r, minlength=N_W)
        assert 2200 <= r.size <= 2800 and (deg[W_EMPTY] == 0).all()
        assert 36 <= deg[W_HUB40] <= 44 and 290 <= deg[W_HUB300] <= 300
        assert (deg <= 8).sum() > 50 and ((deg > 8) & (deg <= 16)).sum() > 20
        _cache["wg"] = (r, c, v)
    return _cache["wg"]


def _width_case(d):
    """Inputs and oracle results at width d (the latest width is kept: both row orders share it)."""
    if _cache.get("wd") != d:
        r, c, v = _width_graph()
        rng = np.random.default_rng(9000 + d)
        e0 = rng.standard_normal((N_W, d)).astype(np.float32)
        G = rng.standard_normal((N_W, d)).astype(np.float32)
        Gs = np.zeros_like(G)             # a few live rows (a hub, an empty row, bundle rows)
        live = np.array([3, W_HUB300, 57, 120, 121, 260])
        Gs[live] = G[live]
        Gs[200] = -0.0                    # a row of -0: not a live row, and no -0 reaches dE0
        z = dict(e0=e0, G=G, Gs=Gs)
        z["fwd"] = {K: oracle.forward(r, c, v, e0, K) for K in (2, 5)}
        z["bwd"] = {K: oracle.backward(r, c, v, G, K) for K in (2, 3)}
        z["bwds"] = {K: oracle.backward(r, c, v, Gs, K) for K in (2, 3)}
        _cache["wd"], _cache["wz"] = d, z
    return _cache["wz"]


def test_width_list_reaches_every_cell():
    """The width list lands on all 18 cells of dispatch_geo (a misaligned base: the scalar cell
    of its d in the first and the last forward layer and in every backward layer, the vector
    cell in the layers between)."""
    hit = set()
    for d, mis in WIDTH_CASES:
        hit.add(pick_geo(d, not mis)[:3])
        if mis:
            assert pick_geo(d, False)[0] == "float" and pick_geo(d, True)[0] == "float4"
    assert len(CELLS) == 18 and hit == CELLS, CELLS ^ hit
    # and on every width dispatch_geo accepts there is a cell (d = 1..2048, aligned or not)
    assert {pick_geo(d, ok)[:3] for d in range(1, 2049) for ok in (False, True)} == CELLS


def test_width_graph_runs_every_path(gpu_device):
    r, c, v = _width_graph()
    g = engine.graph_from_coo(_adj(r, c, v, N_W, gpu_device))
    hp = g.hubs(8, mode="exact", emu_min=16)
    assert hp.n_items > 20                      # whole-row chains: 8 < degree <= 16
    assert hp.n_emu_rows >= 2 and hp.n_emu_blocks > hp.n_emu_rows   # a row of two blocks
    lib = engine.load_library()                 # emulated rows: chain rows at some widths,
    chain = {d for d, _ in WIDTH_CASES if lib.lgcn_chain_supported(d)}   # walked at the others
    assert chain and chain != {d for d, _ in WIDTH_CASES}
    hc = g.hubs(8, mode="chunk")
    assert hc.n_rows > 20 and hc.n_slots > hc.n_rows                # k_hub_combine, several slots


@pytest.mark.parametrize("order", ["degree", "stored"])
@pytest.mark.parametrize("d,mis", WIDTH_CASES,
                         ids=[f"{d}{'-misaligned' if m else ''}" for d, m in WIDTH_CASES])
def test_width_class_bitwise(gpu_device, monkeypatch, d, mis, order):
    monkeypatch.setenv("LGCN_ROW_ORDER", order)
    r, c, v = _width_graph()
    z = _width_case(d)
    g = engine.graph_from_coo(_adj(r, c, v, N_W, gpu_device))
    assert (g.row_ids is not None) == (order == "degree")
    x = [_dev(z["e0"], gpu_device, mis)]
    G, Gs = _dev(z["G"], gpu_device, mis), _dev(z["Gs"], gpu_device, mis)
    with _Tune() as tune:
        # one row per group; bundles forced (301 rows: the last bundle is ragged) with the MEAN
        # bundle prefetch on, the emulated rows all walked; bundles with the prefetch off
        for min_groups, prefetch, chain in ((0, 0, "1"), (1, 0, "0"), (1, 2, "1")):
            tune.set(engine.TUNE_MIN_GROUPS, min_groups)
            tune.set(engine.TUNE_MEAN_PREFETCH, prefetch)
            monkeypatch.setenv("LGCN_CHAIN", chain)
            for plan, kw in (("plain", PLAIN), ("exact", EXACT)):
                what = (d, mis, order, min_groups, prefetch, plan)
                for K in (2, 5):
                    _same(engine.propagate_forward(g, x, K, **kw), z["fwd"][K], what + ("fwd", K))
                for K in (2, 3):    # G / 3 on load (IEEE division), G * 0.25 (exact reciprocal)
                    _same(engine.propagate_backward(g, G, K, sparse="off", **kw), z["bwd"][K],
                          what + ("bwd", K))
                    _same(engine.propagate_backward(g, Gs, K, sparse="on", **kw), z["bwds"][K],
                          what + ("sparse bwd", K))
        tune.set(engine.TUNE_MIN_GROUPS, 0)
        tune.set(engine.TUNE_MEAN_PREFETCH, 0)
        # the chunk plan: deterministic, and the oracle within the north_star tolerance
        f1 = engine.propagate_forward(g, x, 2, hub_threshold=8, hub_mode="chunk").cpu().numpy()
        f2 = engine.propagate_forward(g, x, 2, hub_threshold=8, hub_mode="chunk").cpu().numpy()
        assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32))
        assert_close_normwise(f1, z["fwd"][2], what=f"d={d} chunk plan")


# ---- depths ----------------------------------------------------------------------------------
D_I, D_POOL, D_EMPTY_USERS, D_EMPTY_ITEMS = 24, 150, 3, 3


def _bipartite():
    """test_gpu_lean_rows' builder at a few hundred users: item i gets single[i] users of its own
    and shared[i] from a pool other items draw from too; item rows of ~380 (two emulated
    blocks), ~150, ~50, ~20 edges and bundle rows, three items and three users without an edge."""
    if "bip" not in _cache:
        rng = np.random.default_rng(33)
        small = rng.integers(4, 15, D_I - 4 - D_EMPTY_ITEMS)   # >= 4 edges: every weight <= 0.5
        single = [260, 90, 30, 12] + [int(t) // 2 for t in small]
        shared = [120, 60, 20, 8] + [int(t) - int(t) // 2 for t in small]
        n_single = sum(single)
        users, items, nxt = [], [], 0
        for i, (a, b) in enumerate(zip(single, shared)):
            users += [np.arange(nxt, nxt + a), n_single + rng.choice(D_POOL, b, replace=False)]
            items += [np.full(a + b, i)]
            nxt += a
        U = n_single + D_POOL + D_EMPTY_USERS
        r, c, v, n = oracle.build_norm_adj(np.concatenate(users), np.concatenate(items), U, D_I,
                                           0, use_brand=False)
        deg = np.bincount(r, minlength=n)
        assert 300 < U < 900 and deg[U] > 256 and (deg[U:] == 0).sum() == D_EMPTY_ITEMS
        _cache["bip"] = dict(r=r, c=c, v=v, n=n, U=U)
    return _cache["bip"]


def _depth_case(d, K):
    key = ("depth", d, K)
    if key not in _cache:
        z = _bipartite()
        rng = np.random.default_rng(100 * d + K)
        e0 = rng.standard_normal((z["n"], d)).astype(np.float32)
        G = rng.standard_normal((z["n"], d)).astype(np.float32)
        Gs = np.zeros_like(G)
        live = rng.choice(z["n"], 12, replace=False)
        Gs[live] = G[live]
        Gs[z["U"]] = G[z["U"]]            # the longest item row is live
        _cache[key] = dict(e0=e0, G=G, Gs=Gs,
                           fwd=oracle.forward(z["r"], z["c"], z["v"], e0, K),
                           bwd=oracle.backward(z["r"], z["c"], z["v"], G, K),
                           bwds=oracle.backward(z["r"], z["c"], z["v"], Gs, K))
    return _cache[key]


def _user_item(a, U, dev):
    return [_dev(a[:U], dev), _dev(a[U:], dev)]


@pytest.mark.parametrize("bundles", [False, True])
@pytest.mark.parametrize("schedule", ["one-operator", "two-lanes-lean", "two-lanes"])
@pytest.mark.parametrize("d", [7, 12, 64])
@pytest.mark.parametrize("K", [5, 8, 16])
def test_depths_bitwise(gpu_device, monkeypatch, K, d, schedule, bundles):
    z = _bipartite()
    U, n = z["U"], z["n"]
    sided = schedule != "one-operator"
    if sided:
        monkeypatch.setenv("LGCN_SIDES_MIN_NNZ", "0")
        monkeypatch.setenv("LGCN_AUX_STREAMS", "7")
    adj = _adj(z["r"], z["c"], z["v"], n, gpu_device)
    g = engine.graph_from_coo(adj, sides=(U, U + D_I) if sided else None)
    assert (g.split is not None) == sided
    q = _depth_case(d, K)
    x = _user_item(q["e0"], U, gpu_device)
    with _Tune() as tune:
        tune.set(engine.TUNE_MIN_GROUPS, 1 if bundles else 0)
        kw = dict(EXACT)
        if sided:
            kw["lean"] = schedule == "two-lanes-lean"
        what = (K, d, schedule, bundles)
        _same(engine.propagate_forward(g, x, K, **kw), q["fwd"], what + ("fwd",))
        if sided:
            assert engine.last_schedule["lanes"] == 2
        _same(engine.propagate_backward(g, _user_item(q["G"], U, gpu_device), K, sparse="off",
                                        **EXACT), q["bwd"], what + ("bwd",))
        _same(engine.propagate_backward(g, _user_item(q["Gs"], U, gpu_device), K, sparse="on",
                                        **EXACT), q["bwds"], what + ("sparse bwd",))


@pytest.mark.parametrize("bundles", [False, True])
@pytest.mark.parametrize("sided", [False, True])
@pytest.mark.parametrize("d", [7, 64])
def test_elements_of_minus_zero_in_every_layer(gpu_device, monkeypatch, d, sided, bundles):
    """torch.mean's sum starts from +0: an element that is -0 in every stacked layer comes out
    +0. K = 0: a -0 of E0. K = 1: a -0 of E0 whose chain underflowed to -0 — column 0 holds -0
    in the user rows and the smallest negative subnormal in the item rows (every weight of this
    graph is <= 0.5, so each product rounds to -0), column 1 the same with the sides swapped
    (item rows: whole-row chains, chain rows, emulated blocks)."""
    z = _bipartite()
    U, n = z["U"], z["n"]
    assert z["v"].max() <= 0.5
    if sided:
        monkeypatch.setenv("LGCN_SIDES_MIN_NNZ", "0")
        monkeypatch.setenv("LGCN_AUX_STREAMS", "7")
    g = engine.graph_from_coo(_adj(z["r"], z["c"], z["v"], n, gpu_device),
                              sides=(U, U + D_I) if sided else None)
    e0 = np.random.default_rng(3).standard_normal((n, d)).astype(np.float32)
    tiny = np.float32(-1e-45)
    e0[:U, 0], e0[U:, 0] = -0.0, tiny
    e0[:U, 1], e0[U:, 1] = tiny, -0.0
    x = _user_item(e0, U, gpu_device)
    deg = np.bincount(z["r"], minlength=n)
    with _Tune() as tune:
        tune.set(engine.TUNE_MIN_GROUPS, 1 if bundles else 0)
        for K in (0, 1, 2, 5):
            want, layers = oracle.forward(z["r"], z["c"], z["v"], e0, K, return_layers=True)
            if K >= 1:      # the case is live: layer 1 holds -0 wherever the row has an edge
                l1 = layers[0].view(np.uint32)
                assert (l1[:U, 0][deg[:U] > 0] == 0x80000000).all()
                assert (l1[U:, 1][deg[U:] > 0] == 0x80000000).all()
            if K <= 1:
                assert (want.view(np.uint32)[:U, 0] == 0).all()
                assert (want.view(np.uint32)[U:, 1] == 0).all()
            _same(engine.propagate_forward(g, x, K, **EXACT), want, (d, sided, bundles, K))


@pytest.mark.parametrize("sided", [False, True])
def test_k17_raises(gpu_device, monkeypatch, sided):
    """18 stacked layers: torch.mean leaves the sequential sum (tests/test_reference_mean.py), so
    the forward and the backward refuse K = 17 on either schedule."""
    z = _bipartite()
    U, n = z["U"], z["n"]
    if sided:
        monkeypatch.setenv("LGCN_SIDES_MIN_NNZ", "0")
    g = engine.graph_from_coo(_adj(z["r"], z["c"], z["v"], n, gpu_device),
                              sides=(U, U + D_I) if sided else None)
    x = _user_item(np.zeros((n, 8), np.float32), U, gpu_device)
    for K in (17, 18, -1):
        with pytest.raises(engine.LgcnError):
            engine.propagate_forward(g, x, K, **EXACT)
        with pytest.raises(engine.LgcnError):
            engine.propagate_backward(g, x, K, **EXACT)


# ---- the bundle ladder and the explicit d = 64 variants --------------------------------------
N_L = 1003                               # 17 * 59: no multiple of any RPG * 256 / G
PERS = (1, 2, 3, 4, 7, 8, 14, 15, 40)
LADDER_D = (16, 32, 64, 256)             # G = 4, 8, 16, 64


def _ladder_graph():
    """A power-law bipartite graph of 1003 rows: 900 users, 103 items of Zipf popularity."""
    if "lg" not in _cache:
        rng = np.random.default_rng(12)
        I = 103
        p = 1.0 / np.arange(1, I + 1) ** 1.1
        items = rng.choice(I, 5000, p=p / p.sum())
        users = rng.integers(0, N_L - I, 5000)
        r, c, v, n = oracle.build_norm_adj(users, items, N_L - I, I, 0, use_brand=False)
        assert n == N_L and np.bincount(r, minlength=n).max() > 256
        _cache["lg"] = (r, c, v)
    return _cache["lg"]


def _ladder_case(d):
    key = ("ladder", d)
    if key not in _cache:
        r, c, v = _ladder_graph()
        rng = np.random.default_rng(700 + d)
        e0 = rng.standard_normal((N_L, d)).astype(np.float32)
        G = rng.standard_normal((N_L, d)).astype(np.float32)
        _cache[key] = dict(e0=e0, G=G,
                           fwd={K: oracle.forward(r, c, v, e0, K) for K in (1, 3)},
                           bwd={K: oracle.backward(r, c, v, G, K) for K in (1, 3)})
    return _cache[key]


def _min_groups(per):
    mg = N_L // per
    assert N_L // mg == per
    return mg


def test_ladder_cases_select_every_rung():
    """The rungs test_bundle_ladder_bitwise selects, by the restated choice: 1, 2, 4, 8 and RB
    (3, 7, 15, 15 at G = 4, 8, 16, 64), each by a STORE / ADD layer and by a MEAN layer, and the
    MEAN prefetch's own rungs (3 at G = 4, 4 at G = 8)."""
    for d, G, RB in zip(LADDER_D, (4, 8, 16, 64), (3, 7, 15, 15)):
        kind, g_, NV, dW = pick_geo(d, True)
        assert (kind, g_, NV) == ("float4", G, 1)
        want = {r for r in (1, 2, 4, 8) if r <= RB} | {RB}
        plain = {pick_rung(False, G, NV, dW, N_L, _min_groups(per), 0, 0) for per in PERS}
        mean = {pick_rung(True, G, NV, dW, N_L, _min_groups(per), 2, 3) for per in PERS}
        pf = {pick_rung(True, G, NV, dW, N_L, _min_groups(per), 0, 3) for per in PERS}
        assert plain == want and mean == want, (d, plain, mean)
        assert pf == ({1, 2, 4} if G == 8 else want), (d, pf)   # G = 8: 4-row prefetch bundles
    assert pick_rung(False, 16, 1, 16, N_L, 0, 0, 0) == 1      # the default on a small graph


@pytest.mark.parametrize("d", LADDER_D)
def test_bundle_ladder_bitwise(gpu_device, d):
    r, c, v = _ladder_graph()
    z = _ladder_case(d)
    g = engine.graph_from_coo(_adj(r, c, v, N_L, gpu_device))
    x, G = [_dev(z["e0"], gpu_device)], _dev(z["G"], gpu_device)
    with _Tune() as tune:
        for per in PERS:
            tune.set(engine.TUNE_MIN_GROUPS, _min_groups(per))
            for K in (1, 3):
                for plan, kw in (("plain", PLAIN), ("exact", EXACT)):
                    what = (d, per, K, plan)
                    for prefetch in (0, 2):
                        tune.set(engine.TUNE_MEAN_PREFETCH, prefetch)
                        _same(engine.propagate_forward(g, x, K, **kw), z["fwd"][K],
                              what + ("fwd", prefetch))
                    _same(engine.propagate_backward(g, G, K, sparse="off", **kw), z["bwd"][K],
                          what + ("bwd",))


VARIANTS_64 = [(1, 8), (8, 4), (15, 4), (8, 6), (15, 6), (8, 8), (15, 8)]


@pytest.mark.parametrize("R,U", VARIANTS_64)
def test_explicit_d64_variants_bitwise(gpu_device, R, U):
    """The (rows per group, gathers in flight) variants of launch_layer_t at d = 64 (float4,
    G = 16, NV = 1), selected through LGCN_TUNE_ROWS_PER_GROUP / LGCN_TUNE_UNROLL."""
    assert pick_geo(64, True)[:3] == ("float4", 16, 1)
    r, c, v = _ladder_graph()
    z = _ladder_case(64)
    g = engine.graph_from_coo(_adj(r, c, v, N_L, gpu_device))
    x, G = [_dev(z["e0"], gpu_device)], _dev(z["G"], gpu_device)
    with _Tune() as tune:
        tune.set(engine.TUNE_ROWS_PER_GROUP, R)
        tune.set(engine.TUNE_UNROLL, U)
        for plan, kw in (("plain", PLAIN), ("exact", EXACT)):
            _same(engine.propagate_forward(g, x, 3, **kw), z["fwd"][3], (R, U, plan, "fwd"))
            _same(engine.propagate_backward(g, G, 3, sparse="off", **kw), z["bwd"][3],
                  (R, U, plan, "bwd"))
            _same(engine.propagate_backward(g, G, 3, sparse="on", **kw), z["bwd"][3],
                  (R, U, plan, "masked bwd"))
    lib = engine.load_library()
    assert lib.lgcn_tune(engine.TUNE_ROWS_PER_GROUP, -1) == tune.saved[0][1]
    assert lib.lgcn_tune(engine.TUNE_UNROLL, -1) == tune.saved[1][1]
