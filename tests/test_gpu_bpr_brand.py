"""The brand-preference term of the fused BPR step on the HIP device (csrc/lgcn_bpr_rows.h,
lgcn_bpr.hip, lgcn_bpr_step.hip, gcn_recommendation_amd.train / loss).

Kernel tests: the indexed entry point against the gathered one, both pinned without a tolerance
to lgcn_bpr_loss (itself pinned by tests/test_gpu_bpr_loss.py) at brand weight 1, the weight's
scaling bounded by the roundings it adds, every gradient block and the reduction restated in
numpy float32, planted odd samples, the 5B keys and their scatter. Whole-step tests: the fused
route against `model(adj)` -> eight gathers -> loss.bpr_brand_loss_reg, bitwise.

grads blocks are in include/lgcn.h's order: u0, p0, n0, u, p, n, bp, bn."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import Cfg, case_dims, load_case
from gcn_recommendation_amd import data, engine, graph, sampler, train
from gcn_recommendation_amd.loss import bpr_brand_loss_reg, bpr_loss_reg
from models.lightgcn import LightGCN
from models.lightgcn_fusion import LightGCN_Fusion
from util import gamma

pytestmark = pytest.mark.gpu

LAMBDA = 1e-4
GUARD = 64          # floats of 7.0 on either side of every output buffer
U0, P0, N0, GU, GP, GN, GBP, GBN = range(8)   # grads blocks


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_np(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


class Out:
    """Output buffers of one loss call, each between two guard strips that must stay 7.0."""

    def __init__(self, dev, B, d, blocks, n_terms, coef=True):
        self.full = [torch.full((n + 2 * GUARD,), 7.0, device=dev)
                     for n in (n_terms * B, 1, blocks * B * d, 2 * B)]
        mid = [t[GUARD:-GUARD] for t in self.full]
        self.terms, self.loss = mid[0].view(n_terms, B), mid[1]
        self.grads, self.coef = mid[2].view(blocks, B, d), (mid[3].view(2, B) if coef else None)

    def assert_guards(self):
        for t in self.full:
            assert (t[:GUARD] == 7.0).all().item() and (t[-GUARD:] == 7.0).all().item()


def _ld_args(tensors):
    args = []
    for t in tensors:
        assert t.stride(1) == 1 or t.shape[1] == 1
        args += [engine._ptr(t), t.stride(0)]
    return args


def run_indexed(tabs, sizes, idx, ib, d, w, lam=LAMBDA):
    """tabs = (fu, fi, fb, u0, i0); sizes = (U, I, NB); idx = (users, pos, neg)."""
    lib = engine.load_library()
    dev = tabs[0].device
    B = int(idx[0].shape[0])
    o = Out(dev, B, d, 8, 3)
    rc = lib.lgcn_bpr_brand_loss_indexed(*_ld_args(tabs), *sizes, *(engine._ptr(t) for t in idx),
                                         engine._ptr(ib), B, d, lam, w, engine._ptr(o.terms),
                                         engine._ptr(o.loss), engine._ptr(o.grads),
                                         engine._ptr(o.coef), engine._stream(dev))
    assert rc == 0
    o.assert_guards()
    return o


def run_gathered(rows, ok, d, w, lam=LAMBDA):
    """rows = the eight gathered blocks (u, p, n, u0, p0, n0, bp, bn); ok: uint8 [B] or None."""
    lib = engine.load_library()
    dev = rows[0].device
    B = int(rows[0].shape[0])
    o = Out(dev, B, d, 8, 3)
    rc = lib.lgcn_bpr_brand_loss(*_ld_args(rows), engine._ptr(ok), B, d, lam, w,
                                 engine._ptr(o.terms), engine._ptr(o.loss), engine._ptr(o.grads),
                                 engine._ptr(o.coef), engine._stream(dev))
    assert rc == 0
    o.assert_guards()
    return o


def run_base(rows, d, lam=LAMBDA):
    """lgcn_bpr_loss on six gathered blocks: grads in its own order (u, p, n, u0, p0, n0)."""
    lib = engine.load_library()
    dev = rows[0].device
    B = int(rows[0].shape[0])
    o = Out(dev, B, d, 6, 2, coef=False)
    rc = lib.lgcn_bpr_loss(*_ld_args(rows), B, d, lam, engine._ptr(o.terms), engine._ptr(o.loss),
                           engine._ptr(o.grads), engine._stream(dev))
    assert rc == 0
    o.assert_guards()
    return o


# ---- the shared kernel cases --------------------------------------------------------------------
KERNEL_CASES = [(B, d, NB, False) for B in (1, 5, 257) for d in (1, 12, 64, 100, 256)
                for NB in (1, 7, 300)] + [(257, 100, 7, True)]
R = 300  # users and items


@functools.lru_cache(maxsize=None)
def kernel_case(B, d, NB, sliced):
    """Tables, batch, map (about a fifth of the items unbranded) and the gathered rows of one
    case, on the device; column 0 of the final user table is 2.0, so that dp[:, 0] = 2c exactly.
    sliced: every table is a column slice of a wider one, each at its own leading dimension."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 1009 + d * 31 + NB)
    tabs = []
    for j, n in enumerate((R, R, NB, R, R)):
        if sliced:
            tabs.append(torch.randn(n, d + 3 + 2 * j, generator=g).to(dev)[:, j:j + d])
        else:
            tabs.append(torch.randn(n, d, generator=g).to(dev))
    tabs[0][:, 0] = 2.0
    ib = torch.randint(0, NB, (R,), generator=g, dtype=torch.int32)
    ib[torch.rand(R, generator=g) < 0.2] = -1
    idx = [torch.randint(0, R, (B,), generator=g) for _ in range(3)]
    if B >= 5:   # one sample of each kind whatever the draw: 0 branded, 1 not
        idx[1][0], idx[2][0], idx[1][1] = 0, 1, 2
        ib[0], ib[1], ib[2] = 0, NB - 1, -1
    ib = ib.to(dev)
    idx = [t.to(dev) for t in idx]
    return tabs, (R, R, NB), idx, ib, gathered_rows(tabs, idx, ib, sliced)


def gathered_rows(tabs, idx, ib, sliced=False):
    """(the eight gathered blocks, ok uint8 [B]); an unbranded sample gathers brand row 0."""
    fu, fi, fb, u0, i0 = tabs
    bu, bp, bn = idx
    NB = fb.shape[0]
    rp, rn = ib[bp].long(), ib[bn].long()
    ok = (rp >= 0) & (rp < NB) & (rn >= 0) & (rn < NB)
    rows = [fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], fb[rp.clamp(0, NB - 1)],
            fb[rn.clamp(0, NB - 1)]]
    if sliced:   # each gathered block at a leading dimension of its own too
        d = rows[0].shape[1]
        wide = [torch.zeros(r.shape[0], d + 1 + j, device=r.device) for j, r in enumerate(rows)]
        for wd, r in zip(wide, rows):
            wd[:, 1:1 + d] = r
        rows = [wd[:, 1:1 + d] for wd in wide]
    else:
        rows = [r.contiguous() for r in rows]
    return rows, ok.to(torch.uint8)


# ---- 1. indexed == gathered ---------------------------------------------------------------------
@pytest.mark.parametrize("B,d,NB,sliced", KERNEL_CASES)
def test_indexed_equals_gathered(gpu_device, B, d, NB, sliced):
    tabs, sizes, idx, ib, (rows, ok) = kernel_case(B, d, NB, sliced)
    for w in (1.0, 0.1):
        a = run_indexed(tabs, sizes, idx, ib, d, w)
        b = run_gathered(rows, ok, d, w)
        assert same(a.loss, b.loss) and same(a.terms, b.terms) and same(a.coef, b.coef)
        for k in range(8):
            assert same(a.grads[k], b.grads[k]), k
        assert torch.isfinite(a.loss).all().item()
    if ok.all().item():   # brand_ok NULL = every sample
        c = run_gathered(rows, None, d, 0.1)
        assert same(c.loss, b.loss) and same(c.grads, b.grads) and same(c.coef, b.coef)


# ---- 2. pinned to lgcn_bpr_loss at w = 1, no tolerance ------------------------------------------
@pytest.mark.parametrize("B,d,NB,sliced", KERNEL_CASES)
def test_weight_one_is_two_runs_of_the_base_kernel(gpu_device, B, d, NB, sliced):
    tabs, sizes, idx, ib, (rows, ok) = kernel_case(B, d, NB, sliced)
    u, p, n, u0, p0, n0, bp, bn = rows
    got = run_indexed(tabs, sizes, idx, ib, d, 1.0)
    base = run_base([u, p, n, u0, p0, n0], d)
    brand = run_base([u, bp, bn, u0, p0, n0], d)   # its gp / gn / gu / terms[0]: the brand parts
    okb = ok.bool()
    okc = okb[:, None]
    zero = torch.zeros_like(base.grads[0])
    # the five untouched blocks and both base terms
    for mine, theirs in ((GP, 1), (GN, 2), (U0, 3), (P0, 4), (N0, 5)):
        assert same(got.grads[mine], base.grads[theirs]), mine
    assert same(got.terms[0], base.terms[0]) and same(got.terms[1], base.terms[1])
    # the brand rows and terms: the base kernel's on (u, bp, bn), +0 for an unbranded sample
    assert same(got.grads[GBP], torch.where(okc, brand.grads[1], zero))
    assert same(got.grads[GBN], torch.where(okc, brand.grads[2], zero))
    assert same(got.terms[2], torch.where(okb, brand.terms[0], zero[:, 0]))
    # du = fp32(base + addend); exactly the base kernel's without a brand
    assert same(got.grads[GU], torch.where(okc, base.grads[0] + brand.grads[0], base.grads[0]))
    # coef through dp = fp32(c * u) on the planted column u = 2
    assert (u[:, 0] == 2.0).all().item()
    assert same(got.coef[0], base.grads[1][:, 0] / 2)
    assert same(got.coef[1], torch.where(okb, brand.grads[1][:, 0] / 2, zero[:, 0]))
    assert same(got.grads[GP][:, 0], got.coef[0] * 2)
    if B >= 5:
        assert okb.any().item() and not okb.all().item()
        assert got.coef[1].abs().max().item() > 0


# ---- 3. w != 1: the coefficient bound, every block and the reduction restated -------------------
def brand_reduce_fp32(terms, B, lam, w):
    """k_bpr_brand_reduce in numpy float32 (util.bpr_reduce_fp32 with a third row): thread
    i < 256 sums terms[i], terms[i + 256], ... from +0, the halving tree, then
    loss = (-(sl / B) + w * -(sb / B)) + (lam * sr) / B, every operation rounded once."""
    f = np.float32
    t = np.asarray(terms, dtype=np.float32).reshape(3, B)
    t = np.concatenate([t, np.zeros((3, -B % 256), dtype=np.float32)], axis=1).reshape(3, -1, 256)
    part = np.zeros((3, 256), dtype=np.float32)
    for j in range(t.shape[1]):
        part = part + t[:, j, :]
    h = 128
    while h > 0:
        part[:, :h] = part[:, :h] + part[:, h:2 * h]
        h >>= 1
    sl, sr, sb = part[0, 0], part[1, 0], part[2, 0]
    return f(f(-(sl / f(B))) + f(f(w) * f(-(sb / f(B))))) + f(f(f(lam) * sr) / f(B))


def blocks_fp32(rows, ok, coef, B, lam):
    """The eight gradient blocks from the kernel's own (c, c') in numpy float32."""
    f = np.float32
    u, p, n, u0, p0, n0, bp, bn = (np.ascontiguousarray(t.cpu().numpy()) for t in rows)
    okc = ok.cpu().numpy().astype(bool)[:, None]
    c, cb = coef[0][:, None], coef[1][:, None]
    r = f(f(2) * f(lam)) / f(B)
    with np.errstate(invalid="ignore", over="ignore"):
        base = c * p + (-c) * n
        out = {U0: r * u0, P0: r * p0, N0: r * n0, GP: c * u, GN: (-c) * u,
               GU: np.where(okc, base + (cb * bp + (-cb) * bn), base),
               GBP: np.where(okc, cb * u, f(0)), GBN: np.where(okc, (-cb) * u, f(0))}
    assert all(v.dtype == np.float32 for v in out.values())
    return out


@pytest.mark.parametrize("w", [0.1, 0.37])
@pytest.mark.parametrize("B,d,NB,sliced", KERNEL_CASES)
def test_other_weights(gpu_device, B, d, NB, sliced, w):
    tabs, sizes, idx, ib, (rows, ok) = kernel_case(B, d, NB, sliced)
    one = run_indexed(tabs, sizes, idx, ib, d, 1.0)
    got = run_indexed(tabs, sizes, idx, ib, d, w)
    assert same(got.coef[0], one.coef[0])
    # c'_w and w * c'_1 are two chains of four roundings each (-w/B or -1/B, the quotient, two
    # products; then one more product by w) over identical s' + 1e-8 and 1 - s'
    w32 = float(np.float32(w))
    cw = got.coef[1].cpu().numpy().astype(np.float64)
    ref = w32 * one.coef[1].cpu().numpy().astype(np.float64)
    err, bound = np.abs(cw - ref), gamma(8) * np.abs(ref) + 8 * 2.0 ** -149
    print(f"w={w} max err/bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    coef = got.coef.cpu().numpy()
    want = blocks_fp32(rows, ok, coef, B, LAMBDA)
    grads = got.grads.cpu().numpy()
    for k, v in want.items():
        assert same_np(grads[k], v), k
    assert same_np(got.loss.cpu().numpy(),
                   np.array([brand_reduce_fp32(got.terms.cpu().numpy(), B, LAMBDA, w)]))


# ---- 4. unbranded and odd samples ---------------------------------------------------------------
def test_planted_samples(gpu_device):
    """Nine samples on rows of their own: 0 positive item unbranded; 1 negative item unbranded;
    2 a brand index past the table; 3 user out of range; 4 x' = 30 (s' = 1); 5 x' = -100 (expf
    overflows, s' = 0); 6 the sample whose brand row gets a NaN; 7, 8 ordinary."""
    dev = gpu_device
    B, d, NB, n, w = 9, 32, 6, 20, 0.37
    g = torch.Generator().manual_seed(4)
    fu, fi, fb, u0, i0 = (torch.randn(r, d, generator=g) for r in (n, n, NB + 2, n, n))
    bu, bp, bn = torch.arange(B), torch.arange(B), torch.arange(B) + 10
    ib = torch.full((n,), -1, dtype=torch.int32)
    for b, (rp, rn) in enumerate([(-1, 0), (0, -1), (NB, 1), (0, 1), (2, 3), (3, 4), (5, 0),
                                  (0, 1), (1, 0)]):
        ib[bp[b]], ib[bn[b]] = rp, rn
    fb[2] = 30.0 * fu[4] / fu[4].square().sum()
    fb[3] = 0.0
    fb[4] = 100.0 * fu[5] / fu[5].square().sum()
    bu[3] = n
    tabs = [t.to(dev) for t in (fu, fi, fb, u0, i0)]
    tabs[2] = tabs[2][:NB]          # the table ends at NB: its two further rows are never read
    idx = [t.to(dev) for t in (bu, bp, bn)]
    ib = ib.to(dev)
    sizes = (n, n, NB)
    clean = run_indexed(tabs, sizes, idx, ib, d, w)
    # the base kernel at the same B (per-sample outputs depend on B alone): sample 3 with a
    # clamped user, never compared
    rows, _ = gathered_rows(tabs, [idx[0].clamp(max=n - 1), idx[1], idx[2]], ib)
    base = run_base(rows[:6], d)
    for b in (0, 1, 2):   # no brand term, +0 brand rows, du bitwise the base kernel's
        assert bits(clean.coef[1, b]).item() == 0 and bits(clean.terms[2, b]).item() == 0
        assert bits(clean.grads[GBP, b]).count_nonzero().item() == 0
        assert bits(clean.grads[GBN, b]).count_nonzero().item() == 0
        assert same(clean.grads[GU, b], base.grads[0, b])
        assert same(clean.terms[:2, b], base.terms[:, b])
    # skipped whole: eight zero rows, three zero terms, zero coefficients
    assert bits(clean.grads[:, 3]).count_nonzero().item() == 0
    assert bits(clean.terms[:, 3]).count_nonzero().item() == 0
    assert bits(clean.coef[:, 3]).count_nonzero().item() == 0
    # saturated: c' is a zero and the brand rows are zeros (of either sign); the base part lives
    for b in (4, 5):
        assert clean.coef[1, b].item() == 0 and clean.coef[0, b].item() != 0
        assert (clean.grads[GBP, b] == 0).all().item() and (clean.grads[GBN, b] == 0).all().item()
        assert same(clean.grads[GU, b] + 0.0, base.grads[0, b] + 0.0)   # x + (+-0), -0 aside
    assert clean.terms[2, 4].item() == 0.0                 # logf(1 + 1e-8f) = logf(1)
    assert abs(clean.terms[2, 5].item() - np.log(1e-8)) < 1e-4
    for b in (6, 7, 8):
        assert clean.coef[1, b].item() != 0 and torch.isfinite(clean.grads[:, b]).all().item()
        assert not same(clean.grads[GU, b], base.grads[0, b])
    assert torch.isfinite(clean.loss).all().item()
    # NaN in brand row 5, which sample 6 alone reads: it stays in that sample's outputs
    tabs_nan = list(tabs)
    tabs_nan[2] = tabs[2].clone()
    tabs_nan[2][5, d // 2] = float("nan")
    nan = run_indexed(tabs_nan, sizes, idx, ib, d, w)
    for k in (GU, GBP, GBN):
        assert torch.isnan(nan.grads[k, 6]).any().item(), k
    assert torch.isnan(nan.coef[1, 6]).item() and torch.isnan(nan.terms[2, 6]).item()
    assert torch.isnan(nan.loss).all().item()
    others = [b for b in range(B) if b != 6]
    assert same(nan.grads[:, others], clean.grads[:, others])
    assert same(nan.terms[:, others], clean.terms[:, others])
    assert same(nan.coef[:, others], clean.coef[:, others])
    for k in (GP, GN, U0, P0, N0):
        assert same(nan.grads[k, 6], clean.grads[k, 6]), k
    assert same(nan.terms[:2, 6], clean.terms[:2, 6]) and same(nan.coef[0, 6], clean.coef[0, 6])


# ---- 5. keys and scatter ------------------------------------------------------------------------
def keys_numpy(bu, bp, bn, ib, U, I, NB):
    bu, bp, bn, ib = (np.asarray(t, dtype=np.int64) for t in (bu, bp, bn, ib))
    ok = (bu >= 0) & (bu < U) & (bp >= 0) & (bp < I) & (bn >= 0) & (bn < I)
    rp = np.where(ok, ib[np.where(ok, bp, 0)], -1)
    rn = np.where(ok, ib[np.where(ok, bn, 0)], -1)
    brand = ok & (rp >= 0) & (rp < NB) & (rn >= 0) & (rn < NB)
    none = 2 * (U + I + NB)
    return np.concatenate([np.where(ok, 2 * bu, none), np.where(ok, 2 * (U + bp), none),
                           np.where(ok, 2 * (U + bn) + 1, none),
                           np.where(brand, 2 * (U + I + rp), none),
                           np.where(brand, 2 * (U + I + rn) + 1, none)])


def _sorted_brand_keys(lib, ws, bu, bp, bn, ib, U, I, NB, stream):
    B = int(bu.shape[0])
    m, n_keys = 5 * B, 2 * (U + I + NB) + 1
    ws.sort_scratch(lib, m, n_keys, stream)
    assert lib.lgcn_bpr_brand_keys(engine._ptr(bu), engine._ptr(bp), engine._ptr(bn),
                                   engine._ptr(ib), B, U, I, NB, engine._ptr(ws.keys),
                                   stream) == 0
    b = ws.i32
    nbytes = ctypes.c_size_t(ws.temp_bytes)
    assert lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                  engine._ptr(b[1]), engine._ptr(b[2]), engine._ptr(b[3]),
                                  engine._ptr(ws.temp), ctypes.byref(nbytes), stream) == 0
    return m


def test_brand_keys_equal_numpy(gpu_device):
    lib = engine.load_library()
    dev = gpu_device
    U, I, NB, B = 40, 30, 7, 300
    g = torch.Generator().manual_seed(8)
    bu, bp, bn = (torch.randint(0, n, (B,), generator=g) for n in (U, I, I))
    ib = torch.randint(-1, NB + 1, (I,), generator=g, dtype=torch.int32)   # -1 and NB: no brand
    bu[3], bp[4], bn[5], bu[6] = U, -1, I, -7
    keys = torch.full((5 * B + 2,), -5, dtype=torch.int64, device=dev)
    assert lib.lgcn_bpr_brand_keys(engine._ptr(bu.to(dev)), engine._ptr(bp.to(dev)),
                                   engine._ptr(bn.to(dev)), engine._ptr(ib.to(dev)), B, U, I, NB,
                                   engine._ptr(keys[1:]), engine._stream(dev)) == 0
    want = keys_numpy(bu, bp, bn, ib, U, I, NB)
    assert np.array_equal(keys[1:-1].cpu().numpy(), want)
    assert keys[0].item() == -5 and keys[-1].item() == -5
    none = 2 * (U + I + NB)
    assert (want[3 * B:] == none).sum() > 8 and (want[:B] == none).sum() == 4
    assert (want[3 * B:4 * B] % 2 == 0).all() and (want[4 * B:][want[4 * B:] != none] % 2 == 1).all()


def _sequential_index_put(rows, idx, src):
    """tests/test_gpu_bpr_step.py: IndexBackward's reference on the host, one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return torch.zeros(rows, src.shape[1]).index_put_((idx,), src, accumulate=True)
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("d", [12, 64])
def test_brand_scatter_equals_sequential_reference(gpu_device, d):
    lib = engine.load_library()
    dev = gpu_device
    U = I = 64
    NB, B = 7, 512
    n = U + I + NB
    g = torch.Generator().manual_seed(d)
    # brand 6 belongs to items I-2 and I-1 alone, and sample 0 is the only one on them; the other
    # items: brands 0..5, or none
    ib = torch.randint(0, 6, (I,), generator=g, dtype=torch.int32)
    ib[torch.rand(I, generator=g) < 0.15] = -1
    ib[I - 2], ib[I - 1] = 6, 6
    bu = torch.randint(0, U, (B,), generator=g)
    bp, bn = (torch.randint(0, I - 2, (B,), generator=g) for _ in range(2))
    bp[0], bn[0] = I - 2, I - 1
    src = torch.randn(5 * B, d, generator=g)
    src[torch.rand(5 * B, d, generator=g) < 0.15] = 0.0
    src[torch.rand(5 * B, d, generator=g) < 0.15] = -0.0
    zero_rows = torch.rand(5 * B, generator=g) < 0.3
    src[zero_rows] = 0.0
    src[zero_rows & (torch.rand(5 * B, generator=g) < 0.5)] = -0.0
    src[3 * B] = torch.randn(d, generator=g)
    src[4 * B] = -src[3 * B]           # dbp = c'u, dbn = (-c')u of the lone same-brand sample
    rp, rn = ib[bp].long(), ib[bn].long()
    ok = (rp >= 0) & (rn >= 0)
    assert ok[0].item() and 0 < ok.sum().item() < B
    assert min(int(torch.bincount(t[ok], minlength=6)[:6].min()) for t in (rp, rn)) >= 20
    want = torch.cat([_sequential_index_put(U, bu, src[:B]),
                      _sequential_index_put(I, bp, src[B:2 * B])
                      + _sequential_index_put(I, bn, src[2 * B:3 * B]),
                      _sequential_index_put(NB, rp[ok], src[3 * B:4 * B][ok])
                      + _sequential_index_put(NB, rn[ok], src[4 * B:][ok])])
    lone = U + I + 6
    assert bits(want[lone]).count_nonzero().item() == 0   # x + (-x) = +0

    ws = train._Workspace(n, d, dev)
    stream = engine._stream(dev)
    m = _sorted_brand_keys(lib, ws, bu.to(dev), bp.to(dev), bn.to(dev), ib.to(dev), U, I, NB,
                           stream)
    s = src.to(dev)
    train._scatter(lib, ws, m, s, 0, n, ws.G, engine.LGCN_SCATTER_STORE, ws.mask, ws.count,
                   stream)
    assert same(ws.G.cpu(), want)
    assert bits(ws.G[lone]).count_nonzero().item() == 0
    assert not (int(ws.mask[lone >> 5].item()) >> (lone & 31)) & 1
    mask, count = engine.rows_nonzero([ws.G], d, dev)
    assert torch.equal(ws.mask, mask)
    live = (want != 0).any(1)
    assert not live[lone].item() and live[U + I:lone].all().item()
    assert ws.count.item() == count.item() == live.sum().item()
    # the user / item range alone (the layer-0 ADD scatter's): brand keys are left out
    dst = torch.randn(U + I, d, generator=g)
    got = dst.to(dev)
    train._scatter(lib, ws, m, s, 0, U + I, got, engine.LGCN_SCATTER_ADD, None, None, stream)
    assert same(got.cpu(), dst + want[:U + I])

    assert lib.lgcn_rows_clear(engine._ptr(ws.i32[1]), m, 0, n, engine._ptr(ws.G), d, d,
                               engine._ptr(ws.mask), engine._ptr(ws.count), stream) == 0
    assert bits(ws.G).count_nonzero().item() == 0
    assert ws.mask.count_nonzero().item() == 0 and ws.count.item() == 0


# ---- 6..8: whole steps against the gathered route -----------------------------------------------
SYNTH_BRANDS = 7   # brand rows given to the cases whose fixture has none: rows without edges


def _case(name, dev):
    """(z, dims with at least one brand row, item -> brand map with unbranded items)."""
    z = load_case(name)
    U, I, NB, d, K = case_dims(z)
    rng = np.random.default_rng(5)
    if NB == 0:
        NB = SYNTH_BRANDS
        ib = data.item_brand_map(np.arange(I), rng.integers(0, NB, I), I, num_brands=NB)
    else:
        ib = data.item_brand_map(z["ib_item"], z["ib_brand"], I, num_brands=NB)
    ib[torch.from_numpy(rng.random(I) < 0.2)] = -1
    assert 0 < (ib < 0).sum().item() < I
    return z, (U, I, NB, d, K), ib.to(dev)


def _adj(z, dims, dev):
    U, I, NB = dims[:3]
    return graph.build_norm_adj(z["train_user"], z["train_item"], U, I, NB, z["ib_item"],
                                z["ib_brand"], bool(z["use_brand"]), device=dev)


def _lightgcn(dims, dev):
    U, I, NB, d, K = dims
    torch.manual_seed(42)
    return LightGCN(U, I, NB, Cfg(d, K)).to(dev)


def _batch(dims, dev, size, seed=11, items=None):
    U, I = dims[:2]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, n, (size,), generator=g).to(dev)
                 for n in (U, items or I, items or I))


def _gathered_route(m, adj, bu, bp, bn, ib, w):
    """main.py:495-522 with --brand_loss, the brand lookups on the device."""
    fu, fi, fb, u0, i0 = m(adj)
    return bpr_brand_loss_reg(fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], LAMBDA,
                              brand_loss=True, final_brand_emb=fb, pos_item_brand_idx=ib[bp],
                              neg_item_brand_idx=ib[bn], brand_loss_weight=w)


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters()}


def _assert_same_grads(got, want):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), k


def _assert_workspace_zero(adj):
    (ws,) = adj._lgcn_graph[1]._bpr_workspaces.values()
    assert not ws.dirty
    assert bits(ws.G).count_nonzero().item() == 0
    assert ws.mask.count_nonzero().item() == 0 and ws.count.item() == 0


def _compare_step(name, dev, size, w=0.1, factor=1, items=None):
    z, dims, ib = _case(name, dev)
    batch = _batch(dims, dev, size, items=items)
    unbranded = (ib[batch[1]] < 0) | (ib[batch[2]] < 0)
    assert 0 < unbranded.sum().item() < size
    a, b = _lightgcn(dims, dev), _lightgcn(dims, dev)
    want = _gathered_route(a, _adj(z, dims, dev), *batch, ib, w)   # a fresh adjacency per route
    (want if factor == 1 else factor * want).backward()
    adj = _adj(z, dims, dev)
    got = b.bpr_step(adj, *batch, LAMBDA, item_brand=ib, brand_loss_weight=w)
    (got if factor == 1 else factor * got).backward()
    assert same(got, want) and torch.isfinite(got).item()
    _assert_same_grads(_grads(b), _grads(a))
    for k in ("user_embedding.weight", "item_embedding.weight", "brand_embedding.weight"):
        assert _grads(b)[k].abs().max().item() > 0, k
    _assert_workspace_zero(adj)
    # the brand term is in it
    plain = _lightgcn(dims, dev).bpr_step(_adj(z, dims, dev), *batch, LAMBDA)
    assert not same(plain, got)


@pytest.mark.parametrize("name,size,items", [("c1_brand", 512, None), ("c1_nobrand", 256, None),
                                             ("hub_d32", 256, 64), ("micro_d12", 64, None),
                                             ("debug_c1_brand_k0", 256, None)])
def test_brand_step_equals_gathered_route(gpu_device, name, size, items):
    _compare_step(name, gpu_device, size, items=items)


def test_brand_step_equals_gathered_route_other_weight(gpu_device):
    _compare_step("c1_brand", gpu_device, 512, w=0.37)


def test_brand_step_equals_gathered_route_sided_backward(gpu_device, monkeypatch):
    monkeypatch.setenv("LGCN_SIDES_MIN_NNZ", "0")
    _compare_step("c1_brand", gpu_device, 512)


def test_brand_step_equals_gathered_route_scaled_loss(gpu_device):
    _compare_step("c1_brand", gpu_device, 512, factor=2)


def _fusion(z, dims, dev):
    U, I, NB, d, K = dims
    torch.manual_seed(3)
    return LightGCN_Fusion(U, I, NB, Cfg(d, K), pretrained_item_emb=z["content"]).to(dev)


def test_fusion_brand_step_equals_gathered_route(gpu_device):
    dev = gpu_device
    z, dims, ib = _case("c1_fusion", dev)
    batch = _batch(dims, dev, 256, seed=5)
    a, b = _fusion(z, dims, dev), _fusion(z, dims, dev)
    want = _gathered_route(a, _adj(z, dims, dev), *batch, ib, 0.1)
    want.backward()
    adj = _adj(z, dims, dev)
    got = b.bpr_step(adj, *batch, LAMBDA, item_brand=ib)
    got.backward()
    assert same(got, want)
    ga, gb = _grads(a), _grads(b)
    assert len(ga) == 5
    _assert_same_grads(gb, ga)
    assert gb["brand_embedding.weight"].abs().max().item() > 0
    _assert_workspace_zero(adj)


def test_brand_and_plain_steps_share_one_workspace(gpu_device):
    dev = gpu_device
    z, dims, ib = _case("c1_brand", dev)
    a, b = _lightgcn(dims, dev), _lightgcn(dims, dev)
    adj_a, adj_b = _adj(z, dims, dev), _adj(z, dims, dev)
    for seed, size, brand in ((11, 512, True), (12, 300, True), (13, 400, False)):
        batch = _batch(dims, dev, size, seed=seed)
        for m in (a, b):
            m.zero_grad(set_to_none=True)
        if brand:
            want = _gathered_route(a, adj_a, *batch, ib, 0.1)
            got = b.bpr_step(adj_b, *batch, LAMBDA, item_brand=ib)
        else:
            fu, fi, fb, u0, i0 = a(adj_a)
            bu, bp, bn = batch
            want = bpr_loss_reg(fu[bu], fi[bp], fi[bn], u0[bu], i0[bp], i0[bn], LAMBDA,
                                final_brand_emb=fb)
            got = b.bpr_step(adj_b, *batch, LAMBDA)
        want.backward()
        got.backward()
        assert same(got, want)
        _assert_same_grads(_grads(b), _grads(a))
        _assert_workspace_zero(adj_b)
    assert len(adj_b._lgcn_graph[1]._bpr_workspaces) == 1


def test_weight_zero_and_no_map_are_the_plain_step(gpu_device):
    dev = gpu_device
    z, dims, ib = _case("c1_brand", dev)
    batch = _batch(dims, dev, 256)
    ref = _lightgcn(dims, dev)
    want = train.bpr_step(ref, _adj(z, dims, dev), *batch, LAMBDA)
    want.backward()
    for kw in (dict(item_brand=ib, brand_loss_weight=0), dict(item_brand=ib, brand_loss_weight=0.0),
               dict(item_brand=None), dict(item_brand=None, brand_loss_weight=0.37)):
        m = _lightgcn(dims, dev)
        got = m.bpr_step(_adj(z, dims, dev), *batch, LAMBDA, **kw)
        got.backward()
        assert same(got, want), kw
        _assert_same_grads(_grads(m), _grads(ref))


def test_wrong_maps_raise_before_any_launch(gpu_device, monkeypatch):
    dev = gpu_device
    z, dims, ib = _case("micro_d12", dev)
    m, adj = _lightgcn(dims, dev), _adj(z, dims, dev)
    batch = _batch(dims, dev, 8)

    def refuse(*a, **k):
        raise AssertionError("launched before the map was validated")

    monkeypatch.setattr(engine, "propagate_forward", refuse)
    for bad in (ib.cpu(), ib.long(), ib[:-1], ib.view(1, -1), torch.stack([ib, ib], 1)[:, 0]):
        with pytest.raises(engine.LgcnError):
            m.bpr_step(adj, *batch, LAMBDA, item_brand=bad)


def test_brand_epoch_equals_hand_driven_gathered_route(gpu_device, monkeypatch):
    dev = gpu_device
    z, dims, ib = _case("c1_brand", dev)
    U, I = dims[:2]
    bs, steps = 64, 12
    s = sampler.BprSampler(z["train_user"][:bs * steps], z["train_item"][:bs * steps], U, I, dev,
                           seed=2)
    a, b = _lightgcn(dims, dev), _lightgcn(dims, dev)
    opt_a = torch.optim.Adam(a.parameters(), lr=1e-3)
    opt_b = torch.optim.Adam(b.parameters(), lr=1e-3)
    adj_a, adj_b = _adj(z, dims, dev), _adj(z, dims, dev)
    # one throw-away step builds the graph plan and the workspace of adj_a outside the epoch
    warm = _lightgcn(dims, dev)
    warm.bpr_step(adj_a, *_batch(dims, dev, bs), LAMBDA, item_brand=ib).backward()
    torch.cuda.synchronize()

    def no_readback(name, real):
        def f(self, *args, **kw):
            if self.is_cuda:
                raise AssertionError(f"Tensor.{name}() on a device tensor inside bpr_epoch")
            return real(self, *args, **kw)
        return f

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", no_readback("item", torch.Tensor.item))
        mp.setattr(torch.Tensor, "cpu", no_readback("cpu", torch.Tensor.cpu))
        got = a.bpr_epoch(adj_a, s, opt_a, LAMBDA, bs, epoch=1, item_brand=ib,
                          brand_loss_weight=0.1)
    want = []
    for users, pos, neg in s.epoch(1, bs):
        opt_b.zero_grad()
        loss = _gathered_route(b, adj_b, users, pos, neg, ib, 0.1)
        loss.backward()
        opt_b.step()
        want.append(loss.detach())
    torch.cuda.synchronize()   # the only one since the epoch began
    assert len(want) == steps and got.shape == (steps,)
    assert same(got, torch.stack(want)) and torch.isfinite(got).all().item()
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert same(sa[k], sb[k]), k
    assert not same(sa["brand_embedding.weight"], warm.state_dict()["brand_embedding.weight"])
