"""Inputs, references and direct kernel calls shared by the sampled-softmax tests.

Kernel-level cases: four tables of R = 300 rows, B = 257 samples (65 blocks of four waves, the
last with one), users in [0, 40), positives in [0, 50), candidates in [0, 60): every destination
row repeats. `expression` is loss.ssm_loss_torch on rows gathered from the tables, with the raw
scores kept as a tensor so that their gradient (the kernel's coef) can be asked for."""
import functools

import torch

from gcn_recommendation_amd import engine

R, B = 300, 257
DS = (12, 64, 200)          # fewer than 64 lanes, exactly one lane pass, no multiple of 64
MS = (1, 3, 5, 64)          # a short last group of rows in flight; every lane used
REGIMES = ((1.0, 0.1), (0.1, 1.0), (0.05, 3.0))   # (temperature, scale of the N(0,1) tables)
LAMBDA = 1e-4


@functools.lru_cache(maxsize=None)
def inputs(d, M, scale):
    """(tables fu, fi, u0, i0; users, pos, cand) on the CPU, generated once and never modified."""
    g = torch.Generator().manual_seed(d * 1000 + M)
    tabs = tuple(torch.randn(R, d, generator=g) * scale for _ in range(4))
    users = torch.randint(0, 40, (B,), generator=g)
    pos = torch.randint(0, 50, (B,), generator=g)
    cand = torch.randint(0, 60, (B, M), generator=g)
    return tabs, users, pos, cand


def expression(tabs, users, pos, cand, lam, tau):
    """The torch expression on the tables, in their dtype: (loss, scores [B, 1 + M])."""
    fu, fi, u0, i0 = tabs
    n, M = cand.shape
    flat = cand.reshape(-1)
    u, p, neg = fu[users], fi[pos], fi[flat].view(n, M, -1)
    scores = torch.cat([torch.sum(u * p, dim=1).unsqueeze(1),
                        torch.sum(u.unsqueeze(1) * neg, dim=-1)], dim=1)
    if scores.requires_grad:
        scores.retain_grad()
    logits = scores / tau
    ssm = torch.mean(torch.logsumexp(logits, dim=1) - logits[:, 0])
    reg = lam * (u0[users].norm(2).pow(2) + i0[pos].norm(2).pow(2) +
                 i0[flat].norm(2).pow(2)) / float(n)
    return ssm + reg, scores


def reference(tabs, users, pos, cand, lam, tau, dtype, device):
    """loss, the four table gradients and d(loss)/d(scores) of `expression` in dtype on device."""
    t = [x.detach().to(device=device, dtype=dtype).requires_grad_() for x in tabs]
    idx = [x.to(device) for x in (users, pos, cand)]
    loss, scores = expression(t, *idx, lam, tau)
    loss.backward()
    return loss.detach(), [x.grad for x in t], scores.grad


def _ld_args(tensors):
    out = []
    for t in tensors:
        out += [engine._ptr(t), t.stride(0)]
    return out


def _outputs(n, M, d, dev):
    return (torch.empty(2 * n, dtype=torch.float32, device=dev),
            torch.empty((), dtype=torch.float32, device=dev),
            torch.full((2, (2 + M) * n, d), float("nan"), dtype=torch.float32, device=dev),
            torch.full((n, 1 + M), float("nan"), dtype=torch.float32, device=dev))


def run_indexed(tabs, users, pos, cand, lam, tau, sizes=None):
    """lgcn_ssm_loss_indexed on device tensors: (loss, grads [2, (2+M)B, d], coef [B, 1+M])."""
    lib = engine.load_library()
    dev = tabs[0].device
    n, M = cand.shape
    d = int(tabs[0].shape[1])
    U, I = sizes or (int(tabs[0].shape[0]), int(tabs[1].shape[0]))
    terms, loss, grads, coef = _outputs(n, M, d, dev)
    with torch.cuda.device(dev):
        rc = lib.lgcn_ssm_loss_indexed(*_ld_args(tabs), U, I, engine._ptr(users),
                                       engine._ptr(pos), engine._ptr(cand), n, M, d, lam, tau,
                                       engine._ptr(terms), engine._ptr(loss), engine._ptr(grads),
                                       engine._ptr(coef), engine._stream(dev))
    assert rc == 0, rc
    return loss, grads, coef


def run_gathered(u, p, neg, u0, p0, neg0, valid, lam, tau):
    """lgcn_ssm_loss on gathered blocks (neg / neg0: [B*M x d])."""
    lib = engine.load_library()
    dev = u.device
    n, d = u.shape
    M = int(neg.shape[0]) // n
    terms, loss, grads, coef = _outputs(n, M, d, dev)
    with torch.cuda.device(dev):
        rc = lib.lgcn_ssm_loss(*_ld_args((u, p, neg, u0, p0, neg0)), engine._ptr(valid), n, M, d,
                               lam, tau, engine._ptr(terms), engine._ptr(loss),
                               engine._ptr(grads), engine._ptr(coef), engine._stream(dev))
    assert rc == 0, rc
    return loss, grads, coef


def table_grads(grads, users, pos, cand, rows):
    """The kernel's per-sample rows summed into the four table gradients the way autograd sums
    them (float32 index_put, accumulate): fu, fi, u0, i0, each [rows x d]."""
    n, M = cand.shape
    d = int(grads.shape[2])
    flat = cand.reshape(-1)
    out = []
    for half in (1, 0):
        g = grads[half]
        zero = torch.zeros((rows, d), dtype=torch.float32, device=grads.device)
        gu = zero.index_put((users,), g[:n], accumulate=True)
        gi = zero.index_put((pos,), g[n:2 * n], accumulate=True) + \
            zero.index_put((flat,), g[2 * n:], accumulate=True)
        out += [gu, gi]
    return out


def rel_err(x, x64):
    """max|x - x64| / max|x64|"""
    x64 = x64.detach().cpu().double()
    return ((x.detach().cpu().double() - x64).abs().max() / x64.abs().max()).item()
