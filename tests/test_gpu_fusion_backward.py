"""lgcn_fusion_prelayer_backward (csrc/lgcn_fusion_bwd.hip) against float64 numpy of the three
sums include/lgcn.h documents, element by element:

    g = out > 0 ? g_out : fp32(g_out * slope);  d_id = g W[:, :d];  d_w = g^T [id | content];
    d_b = sum_i g[i, :]

The reference is never the kernel or the torch route.

* Few-bit inputs: every partial sum is an exact fp32 in any order (asserted on the CPU), so the
  result must be (sum64 + 0.0) as fp32, bitwise: accumulators start at +0.
* Gaussian inputs: the header's order gives, per element, at most d fmaf roundings plus the slope
  product for d_id, and R = CHUNK + n_chunks + 2 roundings on the longest path of d_w / d_b (the
  rows of a chunk, the two-level combine, the slope product); the bounds are gamma(d + 1) and
  gamma(R) (Higham) times the matching sum of absolute products. Derived, not measured.
* Bits must not depend on the grid (knob 8), the run, the row's position, the chunk a zero
  gradient sits in, or which outputs were requested; nothing outside the documented region is
  written.
* The weight-gradient combine has two levels (groups of 32 chunks, then the group sums); one case
  of 34 chunks crosses both, the other row counts stay at 3 CHUNK + 13 and below."""
import numpy as np
import pytest
import torch

from gcn_recommendation_amd import engine, fusion
from util import fewbit_fusion_case, fusion_exact, fusion_reference, gamma

pytestmark = pytest.mark.gpu

PAIRS = [(64, 32), (64, 64), (64, 128), (128, 32), (128, 64), (128, 128)]
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload no arithmetic produces (test_gpu_fusion.py)
CHUNK = engine.FUSION_BWD_CHUNK
NMAX = 3 * CHUNK + 13


def bits(t):
    return t.contiguous().view(torch.int32)


def dev_f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def sentinel(shape, dev):
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def assert_bits_equal(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at {i}: "
                             f"got {got[i].item()!r} want {want[i].item()!r}")


def backward(dev, out, g_out, idw, content, n, W, slope, d_id=None, d_w=None, d_b=None):
    """The C entry on 2-D device tensors (views allowed): leading dims are their row strides."""
    d, c = idw.shape[1], content.shape[1]
    lib = engine.load_library()
    scratch, nbytes = None, 0
    if d_w is not None or d_b is not None:
        nbytes = lib.lgcn_fusion_prelayer_backward_scratch_bytes(n, d, c)
        assert nbytes > 0
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lgcn_fusion_prelayer_backward(
            engine._ptr(out), out.stride(0), engine._ptr(g_out), g_out.stride(0),
            engine._ptr(idw), idw.stride(0), engine._ptr(content), content.stride(0), n, d, c,
            engine._ptr(W), float(slope), engine._ptr(d_id),
            d_id.stride(0) if d_id is not None else 0, engine._ptr(d_w), engine._ptr(d_b),
            engine._ptr(scratch), nbytes, engine._stream(dev))
    assert rc == 0, rc


def run_all(dev, out, g_out, idw, content, n, W, slope):
    d, c = idw.shape[1], content.shape[1]
    d_id = torch.empty(n, d, device=dev)
    d_w, d_b = torch.empty(d, d + c, device=dev), torch.empty(d, device=dev)
    backward(dev, out, g_out, idw, content, n, W, slope, d_id, d_w, d_b)
    return d_id, d_w, d_b


def masked64(out, G, slope):
    """The documented g as float64: g_out where out > 0 (false for a zero of either sign and for
    a NaN), else the fp32 product g_out * slope."""
    prod = (np.asarray(G, dtype=np.float32) * np.float32(slope)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(out) > 0, np.asarray(G, dtype=np.float64), prod)


def fewbit_g(n, d, seed):
    """g_out: multiples of 1/8 of magnitude <= 2."""
    return (np.random.default_rng(seed).integers(-16, 17, (n, d)) / 8.0).astype(np.float32)


def assert_fewbit_exact(g, x, W, d):
    """Every partial sum of the three products is an exact fp32 in any order: the sums of
    absolute products are integers below 2^24 in units of the products' common denominator."""
    ag, ax = np.abs(g), np.abs(x).astype(np.float64)
    for m, unit in ((ag.T @ ax, 32), (ag @ np.abs(W[:, :d]).astype(np.float64), 256),
                    (ag.sum(0), 32)):
        assert np.array_equal(m * unit, np.rint(m * unit)) and (m * unit < 2 ** 24).all()


def exact32(s64):
    s = (np.asarray(s64) + 0.0).astype(np.float32)   # accumulators start at +0
    assert np.array_equal(s.astype(np.float64), np.asarray(s64) + 0.0)
    return s


# ---- 1. few-bit, bitwise -------------------------------------------------------------------------
@pytest.mark.parametrize("d,c", PAIRS)
def test_fewbit_bitwise_every_row_count_and_slope(gpu_device, d, c):
    dev = gpu_device
    idw, content, W, b = fewbit_fusion_case(NMAX, d, c, seed=300 + d + c)
    x = np.concatenate([idw, content], 1).astype(np.float64)
    z64, _ = fusion_reference(idw, content, W, b)
    G = fewbit_g(NMAX, d, seed=d * 7 + c)
    ti, tc, tw, tg = (dev_f32(a, dev) for a in (idw, content, W, G))
    d_id = torch.empty(NMAX + 64, d, device=dev)
    d_w, d_b = torch.empty(d * (d + c) + 64, device=dev), torch.empty(d + 64, device=dev)
    for slope in (1.0, 0.25, 0.0):
        out = fusion_exact(z64, slope)
        assert (out[0] == 0).all() and (out[2] == 0).all() and (out[1] <= 0).all()  # rows A, B, D
        g = masked64(out, G, slope)
        assert_fewbit_exact(g, x, W, d)
        to = dev_f32(out, dev)
        for n in (1, 31, 32, 33, 129, CHUNK - 1, CHUNK, CHUNK + 1, NMAX):
            for t in (d_id, d_w, d_b):
                t.view(torch.int32).fill_(SENTINEL)
            backward(dev, to[:n], tg[:n], ti[:n], tc[:n], n, tw, slope, d_id[:n],
                     d_w[:d * (d + c)], d_b[:d])
            what = f"slope {slope} n {n}"
            assert_bits_equal(d_id[:n], dev_f32(exact32(g[:n] @ W[:, :d].astype(np.float64)), dev),
                              what + " d_id")
            assert_bits_equal(d_w[:d * (d + c)].view(d, d + c),
                              dev_f32(exact32(g[:n].T @ x[:n]), dev), what + " d_w")
            assert_bits_equal(d_b[:d], dev_f32(exact32(g[:n].sum(0)), dev), what + " d_b")
            assert (bits(d_id[n:n + 64]) == SENTINEL).all(), what
            assert (bits(d_w[d * (d + c):]) == SENTINEL).all(), what
            assert (bits(d_b[d:]) == SENTINEL).all(), what


# ---- 2. the branch is read from `out` alone ------------------------------------------------------
@pytest.mark.parametrize("d,c", [(64, 32), (128, 128)])
def test_branch_comes_from_out_alone(gpu_device, d, c):
    dev = gpu_device
    n, slope = CHUNK + 33, 0.25
    idw, content, W, _ = fewbit_fusion_case(n, d, c, seed=41)
    x = np.concatenate([idw, content], 1).astype(np.float64)
    G = fewbit_g(n, d, seed=43)
    vals = np.array([1.0, -1.0, 0.0, -0.0, np.nan], dtype=np.float32)
    out = vals[(np.arange(n)[:, None] * 3 + np.arange(d)[None, :]) % 5]   # unrelated to the inputs
    assert np.signbit(out[out == 0]).any() and not np.signbit(out[out == 0]).all()
    g = masked64(out, G, slope)
    assert np.array_equal(g[out > 0], G[out > 0].astype(np.float64))
    assert np.array_equal(g[~(out > 0)], G[~(out > 0)].astype(np.float64) * 0.25)
    assert_fewbit_exact(g, x, W, d)
    d_id, d_w, d_b = run_all(dev, dev_f32(out, dev), dev_f32(G, dev), dev_f32(idw, dev),
                             dev_f32(content, dev), n, dev_f32(W, dev), slope)
    assert_bits_equal(d_id, dev_f32(exact32(g @ W[:, :d].astype(np.float64)), dev), "d_id")
    assert_bits_equal(d_w, dev_f32(exact32(g.T @ x), dev), "d_w")
    assert_bits_equal(d_b, dev_f32(exact32(g.sum(0)), dev), "d_b")


# ---- Gaussian cases ------------------------------------------------------------------------------
def gaussian_case(d, c, n, seed, mixed=False):
    """(x, W, out, G) as float32. out = fp32(leaky_relu(z, 0.01)) of the float64 reference z, with
    every |z| <= gamma(d + c + 3) * mag (within fp32 rounding of zero, judged from the reference
    alone) moved out to twice that distance: no element of out is so close to zero that a
    forward in fp32 could have taken the other branch."""
    rng = np.random.default_rng(seed)
    K = d + c
    x = rng.standard_normal((n, K))
    W = rng.standard_normal((d, K)) * 0.3
    G = rng.standard_normal((n, d))
    if mixed:
        x = x * 10.0 ** rng.uniform(-3, 3, K)
        W = W * 10.0 ** rng.uniform(-3, 3, (d, 1))
        G = G * 10.0 ** rng.uniform(-3, 3, d)
    x, W, G = (a.astype(np.float32) for a in (x, W, G))
    z64, mag = fusion_reference(x[:, :d], x[:, d:], W, None)
    thr = gamma(K + 3) * mag
    z64 = np.where(np.abs(z64) > thr, z64, np.copysign(2 * thr, z64))
    out = np.where(z64 > 0, z64, z64 * 0.01).astype(np.float32)
    assert (out != 0).all() and np.isfinite(out).all() and (out > 0).any() and (out < 0).any()
    return x, W, out, G


# ---- 3. requested outputs are independent --------------------------------------------------------
@pytest.mark.parametrize("d,c", [(64, 64), (128, 64)])
def test_requested_outputs_are_independent(gpu_device, d, c):
    dev = gpu_device
    n, slope = CHUNK + 5, 0.25
    x, W, out, G = gaussian_case(d, c, n, seed=d + c)
    to, tg, ti, tc, tw = (dev_f32(a, dev) for a in (out, G, x[:, :d], x[:, d:], W))
    full = run_all(dev, to, tg, ti, tc, n, tw, slope)
    assert all(torch.isfinite(t).all() for t in full)
    for k, name in enumerate(("d_id", "d_w", "d_b")):
        bufs = [sentinel((n, d), dev), sentinel((d, d + c), dev), sentinel((d,), dev)]
        args = [None, None, None]
        args[k] = bufs[k]
        backward(dev, to, tg, ti, tc, n, tw, slope, *args)
        assert_bits_equal(bufs[k], full[k], name + " alone")
        for j in range(3):
            if j != k:
                assert (bits(bufs[j]) == SENTINEL).all(), (name, j)


# ---- 4. geometry and position independence -------------------------------------------------------
@pytest.mark.parametrize("d,c", [(64, 32), (128, 64)])
def test_bits_do_not_depend_on_geometry_or_position(gpu_device, d, c):
    dev = gpu_device
    n, slope = NMAX, 0.01
    x, W, out, G = gaussian_case(d, c, n, seed=900 + d + c)
    to, tg, ti, tc, tw = (dev_f32(a, dev) for a in (out, G, x[:, :d], x[:, d:], W))
    lib = engine.load_library()
    knob = engine.TUNE_FUSION_BWD_BLOCKS
    old = lib.lgcn_tune(knob, -1)
    try:
        lib.lgcn_tune(knob, 0)
        auto = run_all(dev, to, tg, ti, tc, n, tw, slope)
        again = run_all(dev, to, tg, ti, tc, n, tw, slope)
        for blocks in (1, 3):
            lib.lgcn_tune(knob, blocks)
            got = run_all(dev, to, tg, ti, tc, n, tw, slope)
            for a, b, name in zip(got, auto, ("d_id", "d_w", "d_b")):
                assert_bits_equal(a, b, f"{name}: {blocks} blocks vs auto")
    finally:
        lib.lgcn_tune(knob, old)
    for a, b, name in zip(again, auto, ("d_id", "d_w", "d_b")):
        assert_bits_equal(a, b, name + ": run to run")
    small = run_all(dev, to[:33], tg[:33], ti[:33], tc[:33], 33, tw, slope)
    assert_bits_equal(small[0], auto[0][:33], "d_id: n = 33 vs the largest n")
    # a later chunk whose gradient is zero contributes +0: the bits of the n = CHUNK call
    tz = tg.clone()
    tz[CHUNK:] = 0
    _, w_z, b_z = run_all(dev, to, tz, ti, tc, n, tw, slope)
    _, w_1, b_1 = run_all(dev, to[:CHUNK], tg[:CHUNK], ti[:CHUNK], tc[:CHUNK], CHUNK, tw, slope)
    assert_bits_equal(w_z, w_1, "d_w: zero gradient past the first chunk")
    assert_bits_equal(b_z, b_1, "d_b: zero gradient past the first chunk")
    assert not torch.equal(bits(w_1), bits(auto[1]))


# ---- 5. Gaussian, every element bounded ----------------------------------------------------------
@pytest.mark.parametrize("d,c", PAIRS)
def test_gaussian_every_element_within_gamma_bound(gpu_device, d, c):
    dev = gpu_device
    n = 2 * CHUNK + 37
    n_chunks = -(-n // CHUNK)
    R = CHUNK + n_chunks + 2   # lgcn.h: a chunk's chain, the two-level combine, the slope product
    assert R <= CHUNK + n_chunks + 4
    x, W, out, G = gaussian_case(d, c, n, seed=1000 + d + c, mixed=True)
    to, tg, ti, tc, tw = (dev_f32(a, dev) for a in (out, G, x[:, :d], x[:, d:], W))
    x64, W64 = x.astype(np.float64), W[:, :d].astype(np.float64)
    for slope in (0.01, 0.25, 0.0, 1.0):
        g64 = np.where(out > 0, G.astype(np.float64), G.astype(np.float64) * np.float64(
            np.float32(slope)))
        ag = np.abs(g64)
        got = [t.cpu().numpy().astype(np.float64)
               for t in run_all(dev, to, tg, ti, tc, n, tw, slope)]
        refs = (g64 @ W64, g64.T @ x64, g64.sum(0))
        bounds = (gamma(d + 1) * (ag @ np.abs(W64)), gamma(R) * (ag.T @ np.abs(x64)),
                  gamma(R) * ag.sum(0))
        for name, a, ref, bound in zip(("d_id", "d_w", "d_b"), got, refs, bounds):
            err = np.abs(a - ref)
            worst = np.unravel_index(np.argmax(err - bound), err.shape)
            print(f"({d},{c}) slope {slope} {name}: max err/bound "
                  f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all(), (name, slope, worst, err[worst], bound[worst])


# ---- 5b. both levels of the combine ---------------------------------------------------------------
def test_combine_tree_beyond_one_group(gpu_device):
    """n = 33 CHUNK + 37 is 34 chunks: two first-level groups (32 chunks, then 2) and the second
    level over their sums, the path every production size takes (C5: 2149 chunks, 68 groups).
    Each of d_id / d_w / d_b within its derived bound of the float64 reference (R as in the header:
    the rows of a chunk, at most n_chunks + 1 combine roundings, the slope product); the bits
    equal for knob 8 at 1, 3 and auto, for two runs and for d_w / d_b requested alone; d_w and d_b
    bitwise the header's tree restated in float32 numpy on the chunks' own partials; and with
    g_out zeroed past row 32 CHUNK the second group sums to +0, so d_w and d_b have the bits of
    the n = 32 CHUNK call, which a single group forms."""
    dev = gpu_device
    d, c, slope = 64, 32, 0.25
    n, n1 = 33 * CHUNK + 37, 32 * CHUNK
    n_chunks = -(-n // CHUNK)
    assert n_chunks == 34 and -(-n1 // CHUNK) == 32
    R = CHUNK + n_chunks + 2
    assert R <= CHUNK + n_chunks + 4
    x, W, out, G = gaussian_case(d, c, n, seed=4242, mixed=True)
    to, tg, ti, tc, tw = (dev_f32(a, dev) for a in (out, G, x[:, :d], x[:, d:], W))
    lib = engine.load_library()
    knob = engine.TUNE_FUSION_BWD_BLOCKS
    old = lib.lgcn_tune(knob, -1)
    try:
        lib.lgcn_tune(knob, 0)
        auto = run_all(dev, to, tg, ti, tc, n, tw, slope)
        again = run_all(dev, to, tg, ti, tc, n, tw, slope)
        for blocks in (1, 3):
            lib.lgcn_tune(knob, blocks)
            got = run_all(dev, to, tg, ti, tc, n, tw, slope)
            for a, b, name in zip(got, auto, ("d_id", "d_w", "d_b")):
                assert_bits_equal(a, b, f"{name}: {blocks} blocks vs auto")
    finally:
        lib.lgcn_tune(knob, old)
    for a, b, name in zip(again, auto, ("d_id", "d_w", "d_b")):
        assert_bits_equal(a, b, name + ": run to run")
    only_w, only_b = sentinel((d, d + c), dev), sentinel((d,), dev)
    backward(dev, to, tg, ti, tc, n, tw, slope, None, only_w, None)
    backward(dev, to, tg, ti, tc, n, tw, slope, None, None, only_b)
    assert_bits_equal(only_w, auto[1], "d_w alone")
    assert_bits_equal(only_b, auto[2], "d_b alone")
    # the float64 reference
    g64 = np.where(out > 0, G.astype(np.float64), G.astype(np.float64) * slope)
    ag, x64, W64 = np.abs(g64), x.astype(np.float64), W[:, :d].astype(np.float64)
    refs = (g64 @ W64, g64.T @ x64, g64.sum(0))
    bounds = (gamma(d + 1) * (ag @ np.abs(W64)), gamma(R) * (ag.T @ np.abs(x64)),
              gamma(R) * ag.sum(0))
    for name, t, ref, bound in zip(("d_id", "d_w", "d_b"), auto, refs, bounds):
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"n {n} {name}: max err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (name, worst, err[worst], bound[worst])
    # the documented tree, restated in numpy float32 on the chunks' own partials (a call on one
    # chunk alone returns its partial: +0 + p = p): groups of 32 consecutive chunks added in
    # ascending order from +0, then the group sums in ascending order from +0, bitwise
    parts = []
    for lo in range(0, n, CHUNK):
        hi = min(lo + CHUNK, n)
        _, pw, pb = run_all(dev, to[lo:hi], tg[lo:hi], ti[lo:hi], tc[lo:hi], hi - lo, tw, slope)
        parts.append((pw.cpu().numpy(), pb.cpu().numpy()))
    for k, (name, got) in enumerate((("d_w", auto[1]), ("d_b", auto[2]))):
        total = np.zeros_like(parts[0][k])
        for j in range(0, n_chunks, 32):
            group = np.zeros_like(total)
            for p in parts[j:j + 32]:
                group = group + p[k]
            total = total + group
        assert total.dtype == np.float32
        assert_bits_equal(got, dev_f32(total, dev), name + ": the header's combine order")
    # a second group that sums to +0
    tz = tg.clone()
    tz[n1:] = 0
    _, w_z, b_z = run_all(dev, to, tz, ti, tc, n, tw, slope)
    _, w_1, b_1 = run_all(dev, to[:n1], tg[:n1], ti[:n1], tc[:n1], n1, tw, slope)
    assert_bits_equal(w_z, w_1, "d_w: zero gradient past the first group")
    assert_bits_equal(b_z, b_1, "d_b: zero gradient past the first group")
    assert not torch.equal(bits(w_1), bits(auto[1]))
    # and the first group is not one chunk: a zero gradient past the first chunk gives the
    # n = CHUNK bits through both levels
    tz[CHUNK:] = 0
    _, w_c, b_c = run_all(dev, to, tz, ti, tc, n, tw, slope)
    _, w_0, b_0 = run_all(dev, to[:CHUNK], tg[:CHUNK], ti[:CHUNK], tc[:CHUNK], CHUNK, tw, slope)
    assert_bits_equal(w_c, w_0, "d_w: zero gradient past the first chunk")
    assert_bits_equal(b_c, b_0, "d_b: zero gradient past the first chunk")


# ---- 6. strided operands -------------------------------------------------------------------------
def test_strided_operands_and_untouched_surroundings(gpu_device):
    dev = gpu_device
    d, c, n, slope, lead = 64, 128, CHUNK + 37, 0.25, 8
    x, W, out, G = gaussian_case(d, c, n, seed=77)
    to, tg, ti, tc, tw = (dev_f32(a, dev) for a in (out, G, x[:, :d], x[:, d:], W))
    want = run_all(dev, to, tg, ti, tc, n, tw, slope)
    # 16-B aligned column slices of wider buffers: five distinct leading dims, multiples of 4
    wide = [torch.full((n, w), 123.0, device=dev) for w in (d + 8, d + 12, d + 16, c + 20)]
    so, sg, si, sc = wide[0][:, 4:4 + d], wide[1][:, 8:8 + d], wide[2][:, 12:12 + d], \
        wide[3][:, 16:16 + c]
    for view, src in ((so, to), (sg, tg), (si, ti), (sc, tc)):
        view.copy_(src)
    buf = sentinel((lead + n + 64, d + 24), dev)
    s_did = buf[lead:lead + n, 4:4 + d]
    strides = {t.stride(0) for t in (so, sg, si, sc, s_did)}
    assert strides == {d + 8, d + 12, d + 16, c + 20, d + 24} and len(strides) == 5
    assert all(t.data_ptr() % 16 == 0 for t in (so, sg, si, sc, s_did))
    d_w, d_b = torch.empty(d, d + c, device=dev), torch.empty(d, device=dev)
    backward(dev, so, sg, si, sc, n, tw, slope, s_did, d_w, d_b)
    for a, b, name in zip((s_did, d_w, d_b), want, ("d_id", "d_w", "d_b")):
        assert_bits_equal(a, b, name + " strided vs contiguous")
    after = buf.view(torch.int32).clone()
    after[lead:lead + n, 4:4 + d] = SENTINEL
    assert (after == SENTINEL).all(), "wrote outside rows < n, columns < d of d_id"
    assert (wide[0][:, :4] == 123.0).all() and (wide[1][:, :8] == 123.0).all()
    assert (wide[2][:, :12] == 123.0).all() and (wide[3][:, :16] == 123.0).all()
    assert torch.equal(so, to) and torch.equal(sg, tg) and torch.equal(si, ti)


# ---- 7. NaN and infinity -------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["g_out", "id"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_follow_ieee(gpu_device, where, value):
    dev = gpu_device
    d, c, n, slope, r = 64, 32, 129, 0.25, 40
    idw, content, W, b = fewbit_fusion_case(n, d, c, seed=77)
    W[np.random.default_rng(5).random(W.shape) < 0.5] = 0.0
    z64, _ = fusion_reference(idw, content, W, b)
    out = fusion_exact(z64, slope)
    G = fewbit_g(n, d, seed=9)
    x = np.concatenate([idw, content], 1)
    # the affected row has a zero and a non-zero both in g and in x (0 * inf is a NaN)
    G[r, 0], G[r, 1], x[r, 0], x[r, 1] = 0.0, 1.0, 0.0, 1.0
    z64, _ = fusion_reference(x[:, :d], x[:, d:], W, b)
    out = fusion_exact(z64, slope)
    tw, to = dev_f32(W, dev), dev_f32(out, dev)
    clean = run_all(dev, to, dev_f32(G, dev), dev_f32(x[:, :d], dev), dev_f32(x[:, d:], dev), n,
                    tw, slope)
    assert all(torch.isfinite(t).all() for t in clean)
    if where == "g_out":
        G[r, 5] = value
    else:
        x[r, 7] = value
        assert (masked64(out, G, slope)[r] == 0).any() and (masked64(out, G, slope)[r] != 0).any()
    full = run_all(dev, to, dev_f32(G, dev), dev_f32(x[:, :d], dev), dev_f32(x[:, d:], dev), n, tw,
                   slope)
    got = [t.cpu().numpy() for t in full]
    g = masked64(out, G, slope)
    with np.errstate(invalid="ignore"):   # explicit sums: IEEE per product, no BLAS in between
        refs = ((g[:, :, None] * W[:, :d].astype(np.float64)[None, :, :]).sum(1),
                (g[:, :, None] * x.astype(np.float64)[:, None, :]).sum(0), g.sum(0))
    # d_id: the special value stays inside its row
    others = torch.tensor([i for i in range(n) if i != r], device=dev)
    assert_bits_equal(full[0][others], clean[0][others], "d_id rows without a NaN / inf")
    if where == "g_out":
        assert not np.isfinite(refs[0][r]).any() and not np.isfinite(refs[1][5]).any()
        assert np.isnan(refs[0][r]).any() and np.isnan(refs[1][5]).any()
    else:
        assert_bits_equal(full[0], clean[0], "d_id does not read id_emb")
        assert np.isnan(refs[1][:, 7]).any()
        assert not np.isfinite(refs[1][:, 7]).any() and np.isfinite(refs[2]).all()
    for name, a, ref in zip(("d_id", "d_w", "d_b"), got, refs):
        assert np.array_equal(np.isnan(a), np.isnan(ref)), name
        ok = ~np.isnan(ref)
        assert np.array_equal(a[ok], ref[ok].astype(np.float32)), name


# ---- 8. through the module -----------------------------------------------------------------------
def _module_grads(dev, x, W, b, G, d, slope, train_id=True):
    ti = dev_f32(x[:, :d], dev).requires_grad_(train_id)
    tc = dev_f32(x[:, d:], dev)
    lin = torch.nn.Linear(x.shape[1], d, bias=b is not None).to(dev)
    with torch.no_grad():
        lin.weight.copy_(dev_f32(W, dev))
        if b is not None:
            lin.bias.copy_(dev_f32(b, dev))
    out = fusion.fused_item_embedding(ti, tc, lin, slope=slope)
    (out * dev_f32(G, dev)).sum().backward()
    return out.detach(), ti.grad, lin.weight.grad, lin.bias.grad if b is not None else None


@pytest.mark.parametrize("d,c", [(128, 64), (64, 32)])
def test_module_route_equals_the_c_entry(gpu_device, d, c):
    dev = gpu_device
    n, slope = CHUNK + 5, 0.01
    rng = np.random.default_rng(d * 3 + c)
    x = rng.standard_normal((n, d + c)).astype(np.float32)
    W = (rng.standard_normal((d, d + c)) * 0.3).astype(np.float32)
    b = rng.standard_normal(d).astype(np.float32)
    G = rng.standard_normal((n, d)).astype(np.float32)
    lib = engine.load_library()
    saved = fusion.BACKWARD
    calls = []
    real = lib.lgcn_fusion_prelayer_backward

    def spy(*a):
        calls.append(tuple(v is not None and bool(getattr(v, "value", v)) for v in
                           (a[13], a[15], a[16])))
        return real(*a)
    try:
        lib.lgcn_fusion_prelayer_backward = spy
        fusion.BACKWARD = "kernel"
        out, g_id, g_w, g_b = _module_grads(dev, x, W, b, G, d, slope)
        _, f_id, f_w, f_b = _module_grads(dev, x, W, b, G, d, slope, train_id=False)
        _, n_id, n_w, n_b = _module_grads(dev, x, W, None, G, d, slope)
        assert calls == [(True, True, True), (False, True, True), (True, True, False)]
        fusion.BACKWARD = "torch"
        _, t_id, t_w, t_b = _module_grads(dev, x, W, b, G, d, slope)
        assert len(calls) == 3   # the torch route never reaches the entry
    finally:
        lib.lgcn_fusion_prelayer_backward = real
        fusion.BACKWARD = saved
    # the C entry called directly on the forward's output
    want = run_all(dev, out, dev_f32(G, dev), dev_f32(x[:, :d], dev), dev_f32(x[:, d:], dev), n,
                   dev_f32(W, dev), slope)
    for a, w, name in zip((g_id, g_w, g_b), want, ("d_id", "d_W", "d_b")):
        assert_bits_equal(a, w, name + ": module vs C entry")
    assert f_id is None
    assert_bits_equal(f_w, want[1], "d_W with a frozen id table")
    assert_bits_equal(f_b, want[2], "d_b with a frozen id table")
    assert n_b is None
    # the bias-free forward has another output, hence other branches: its own direct call
    lin_out, _, _, _ = _module_grads(dev, x, W, None, G, d, slope)
    want_nb = run_all(dev, lin_out, dev_f32(G, dev), dev_f32(x[:, :d], dev),
                      dev_f32(x[:, d:], dev), n, dev_f32(W, dev), slope)
    assert_bits_equal(n_id, want_nb[0], "d_id without a bias")
    assert_bits_equal(n_w, want_nb[1], "d_W without a bias")
    # the torch route: the existing test's bound, gamma(n + d + 3), against float64 numpy of the
    # documented g (branches from the forward's fp32 output, as both routes read them)
    g64 = np.where(out.cpu().numpy() > 0, G.astype(np.float64), G.astype(np.float64) * slope)
    ag, x64, W64 = np.abs(g64), x.astype(np.float64), W[:, :d].astype(np.float64)
    refs = (g64 @ W64, g64.T @ x64, g64.sum(0))
    mags = (ag @ np.abs(W64), ag.T @ np.abs(x64), ag.sum(0))
    for name, t, ref, mag in zip(("d_id", "d_W", "d_b"), (t_id, t_w, t_b), refs, mags):
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref)
        assert (err <= gamma(n + d + 3) * mag).all(), (name, err.max())
