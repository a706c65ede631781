"""The logQ correction of the sampled-softmax step without a GPU: loss.ssm_loss_torch with q_pos /
q_neg against hand-written float64, bpr_step / bpr_epoch with neg_log_q on a CPU adjacency against
the torch expression, what they refuse, and the host-side argument validation of
lgcn_ssm_loss_q, lgcn_ssm_loss_indexed_q and lgcn_bpr_sample_weighted."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Cfg, case_dims, load_case
from gcn_recommendation_amd import _build, engine, graph, loss, sampler, train
from models.lightgcn import LightGCN
from models.lightgcn_fusion import LightGCN_Fusion
from ssm_cases import LAMBDA, inputs
from weighted_cases import log_q, power_law_weights

TAU = 0.2


@pytest.fixture
def ordered_sums():
    """torch's CPU index_put sums a large gradient block with atomic adds from several threads
    unless deterministic algorithms are asked for."""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(before)


def _rows(d, M, scale, dtype):
    tabs, users, pos, cand = inputs(d, M, scale)
    fu, fi, u0, i0 = (t.to(dtype) for t in tabs)
    n = users.shape[0]
    flat = cand.reshape(-1)
    return (fu[users], fi[pos], fi[flat].view(n, M, -1), u0[users], i0[pos],
            i0[flat].view(n, M, -1)), pos, cand


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32),
                                              b.detach().view(torch.int32))


# ---- the torch expression ------------------------------------------------------------------------
def test_constant_q_cancels():
    rows, pos, cand = _rows(12, 5, 1.0, torch.float64)
    plain = loss.ssm_loss_torch(*rows, LAMBDA, TAU)
    q = torch.full((300,), -3.25, dtype=torch.float64)
    got = loss.ssm_loss_torch(*rows, LAMBDA, TAU, q_pos=q[pos], q_neg=q[cand])
    assert abs(got.item() - plain.item()) <= 1e-12 * abs(plain.item())
    assert torch.equal(loss.ssm_loss_torch(*rows, LAMBDA, TAU, q_pos=None, q_neg=None), plain)
    rows32, _, _ = _rows(12, 5, 1.0, torch.float32)
    a = loss.ssm_loss_reg(*rows32, LAMBDA, TAU)
    b = loss.ssm_loss_reg(*rows32, LAMBDA, TAU, q_pos=q[pos].float(), q_neg=q[cand].float())
    assert abs(a.item() - b.item()) <= 1e-5 * abs(a.item())


@pytest.mark.parametrize("M", [1, 5])
def test_random_q_against_hand_written_float64(M):
    rows, pos, cand = _rows(12, M, 1.0, torch.float64)
    u, p, n, u0, p0, n0 = rows
    q = torch.from_numpy(log_q(power_law_weights(300))).double()
    valid = torch.ones(cand.shape, dtype=torch.bool)
    valid[5] = False
    valid[9, : M - 1] = False
    for v in (None, valid):
        q_pos, q_neg = q[pos], q[cand]
        if v is not None:   # the q of a masked candidate or of a skipped sample is not read
            q_neg = q_neg.masked_fill(~v, float("nan"))
            q_pos = q_pos.masked_fill(~v.any(1), float("inf"))
        got = loss.ssm_loss_reg(*rows, LAMBDA, TAU, valid=v, q_pos=q_pos, q_neg=q_neg)
        assert torch.isfinite(got).item()
        total = 0.0
        for b in range(len(u)):
            on = torch.ones(M, dtype=torch.bool) if v is None else v[b]
            if not on.any():
                continue
            z = torch.cat([((u[b] * p[b]).sum() / TAU - q[pos[b]])[None],
                           (u[b] * n[b][on]).sum(-1) / TAU - q[cand[b]][on]])
            zmax = z.max()
            total = total + torch.log(torch.exp(z - zmax).sum()) + (zmax - z[0])
            total = total + LAMBDA * (u0[b].pow(2).sum() + p0[b].pow(2).sum() +
                                      n0[b][on].pow(2).sum())
        assert abs(got.item() - (total / len(u)).item()) <= 1e-12 * abs(got.item())
    plain = loss.ssm_loss_reg(*rows, LAMBDA, TAU)
    assert abs(got.item() - plain.item()) > 1e-3 * abs(plain.item())
    # each q alone is the other at zero
    only_neg = loss.ssm_loss_torch(*rows, LAMBDA, TAU, q_neg=q[cand])
    assert torch.equal(only_neg, loss.ssm_loss_torch(*rows, LAMBDA, TAU, q_neg=q[cand],
                                                     q_pos=torch.zeros(len(u)).double()))


# ---- steps and epochs on a CPU adjacency ---------------------------------------------------------
def _setup(batch=128, M=4, name="c1_brand"):
    z = load_case(name)
    U, I, B, d, K = case_dims(z)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]))
    g = torch.Generator().manual_seed(23)
    bu, bp = (torch.randint(0, n, (batch,), generator=g) for n in (U, I))
    cand = torch.randint(0, I, (batch, M), generator=g)
    q = torch.from_numpy(log_q(power_law_weights(I)))
    return z, adj, bu, bp, cand, q


def _model(z, fusion=False):
    U, I, B, d, K = case_dims(z)
    torch.manual_seed(42)
    if fusion:
        return LightGCN_Fusion(U, I, B, Cfg(d, K), pretrained_item_emb=z["content"])
    return LightGCN(U, I, B, Cfg(d, K))


def _hand_loss(m, adj, bu, bp, cand, tau, q):
    fu, fi, _, u0, i0 = m(adj)
    n, M = cand.shape
    flat = cand.reshape(-1)
    return loss.ssm_loss_reg(fu[bu], fi[bp], fi[flat].view(n, M, -1), u0[bu], i0[bp],
                             i0[flat].view(n, M, -1), LAMBDA, tau, q_pos=q[bp],
                             q_neg=q[flat].view(n, M))


@pytest.mark.parametrize("name,fusion", [("c1_brand", False), ("c1_fusion", True)])
def test_cpu_step_with_neg_log_q_is_the_torch_expression(ordered_sums, name, fusion):
    z, adj, bu, bp, cand, q = _setup(name=name)
    a, b, c = (_model(z, fusion) for _ in range(3))
    got = a.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="softmax", temperature=TAU,
                     neg_log_q=q)
    want = _hand_loss(b, adj, bu, bp, cand, TAU, q)
    assert torch.equal(got, want) and torch.isfinite(got).item()
    got.backward()
    want.backward()
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert gb[k].grad is not None and _same_bits(ga[k].grad, gb[k].grad), k
    plain = c.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="softmax", temperature=TAU)
    assert not torch.equal(plain, got)
    assert torch.equal(plain, c.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="softmax",
                                         temperature=TAU, neg_log_q=None))


def test_cpu_step_refusals():
    z, adj, bu, bp, cand, q = _setup(batch=16)
    I = case_dims(z)[1]
    m = _model(z)
    for mode in ("hardest", "all"):
        with pytest.raises(ValueError):
            m.bpr_step(adj, bu, bp, cand, LAMBDA, negatives=mode, neg_log_q=q)
    with pytest.raises(ValueError):   # a 1-D neg has no softmax
        m.bpr_step(adj, bu, bp, cand[:, 0].contiguous(), LAMBDA, neg_log_q=q)
    wide = torch.zeros(2 * I)
    for bad in (q.double(), q.to(torch.float16), q[:-1], torch.cat([q, q[:1]]), q.view(1, -1),
                wide[::2], q.numpy(), q.tolist(), q.to("meta")):
        with pytest.raises(engine.LgcnError):
            m.bpr_step(adj, bu, bp, cand, LAMBDA, negatives="softmax", neg_log_q=bad)
    assert torch.isfinite(train.bpr_step(m, adj, bu, bp, cand, LAMBDA, negatives="softmax",
                                         neg_log_q=q)).item()


def _epoch_setup(n=600, seed=4):
    z = load_case("c1_brand")
    U, I, B, d, K = case_dims(z)
    adj = graph.build_norm_adj(z["train_user"], z["train_item"], U, I, B, z["ib_item"],
                               z["ib_brand"], bool(z["use_brand"]))
    n = min(len(z["train_user"]), n)
    s = sampler.BprSampler(z["train_user"][:n], z["train_item"][:n], U, I, "cpu", seed=seed,
                           weights="popularity")
    return z, adj, s


def test_cpu_epoch_with_neg_log_q_equals_the_hand_loop(ordered_sums):
    z, adj, s = _epoch_setup()
    a, b = _model(z), _model(z)
    oa, ob = (torch.optim.Adam(m.parameters(), lr=1e-3) for m in (a, b))
    got = a.bpr_epoch(adj, s, oa, LAMBDA, 256, 1, n_neg=4, negatives="softmax", temperature=TAU,
                      neg_log_q=True)
    want = []
    q = s.neg_log_q()
    for bu, bp, cand in s.epoch(1, 256, n_neg=4):
        assert (s.item_weights[cand.numpy()] > 0).all()   # weighted candidates: seen items only
        ob.zero_grad()
        step = _hand_loss(b, adj, bu, bp, cand, TAU, q)
        step.backward()
        ob.step()
        want.append(step.detach())
    assert len(want) == 3 and _same_bits(got, torch.stack(want))
    for (k, p), (_, r) in zip(a.named_parameters(), b.named_parameters()):
        assert _same_bits(p, r), k
    c = _model(z)
    oc = torch.optim.Adam(c.parameters(), lr=1e-3)
    plain = c.bpr_epoch(adj, s, oc, LAMBDA, 256, 1, n_neg=4, negatives="softmax",
                        temperature=TAU)
    assert not _same_bits(plain, got)
    for kw in (dict(n_neg=4, negatives="hardest"), dict(n_neg=4, negatives="all"), dict(),
               dict(negatives="in_batch"), dict(negatives="softmax")):
        with pytest.raises(ValueError):
            a.bpr_epoch(adj, s, oa, LAMBDA, 256, 1, neg_log_q=True, **kw)
    with pytest.raises(ValueError):   # the in-batch keyword keeps its refusal
        a.bpr_epoch(adj, s, oa, LAMBDA, 256, 1, n_neg=4, negatives="softmax", log_q=True)


# ---- the C entry points refuse bad arguments on the host ---------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return engine.load_library()


P = ctypes.c_void_p(256)


def test_ssm_loss_q_validates_arguments_without_gpu(lib):
    names = ("u", "p", "n", "u0", "p0", "n0")

    def call(B=4, M=4, d=64, tau=0.5, terms=P, out=P, grads=P, **kw):
        args = []
        for k in names:
            args += [kw.get(k, P), kw.get("ld_" + k, 64)]
        return lib.lgcn_ssm_loss_q(*args, None, P, P, B, M, d, 1e-4, tau, terms, out, grads, None,
                                   None)

    bad = [dict(B=0), dict(d=0), dict(M=0), dict(M=65), dict(terms=None), dict(out=None),
           dict(grads=None), dict(B=1 << 30, M=2), dict(tau=0.0), dict(tau=float("nan"))]
    bad += [{k: None} for k in names] + [{"ld_" + k: 63} for k in names]
    for kw in bad:
        assert call(**kw) == -1, kw   # LGCN_EINVAL


def test_ssm_loss_indexed_q_validates_arguments_without_gpu(lib):
    tabs = ("fu", "fi", "u0", "i0")

    def call(U=10, I=10, users=P, pos=P, cand=P, B=4, M=4, d=64, tau=0.5, terms=P, out=P,
             grads=P, **kw):
        args = []
        for k in tabs:
            args += [kw.get(k, P), kw.get("ld_" + k, 64)]
        return lib.lgcn_ssm_loss_indexed_q(*args, U, I, users, pos, cand, P, B, M, d, 1e-4, tau,
                                           terms, out, grads, None, None)

    bad = [dict(B=0), dict(d=0), dict(M=0), dict(M=65), dict(U=-1), dict(I=-1), dict(users=None),
           dict(pos=None), dict(cand=None), dict(terms=None), dict(out=None), dict(grads=None),
           dict(tau=-1.0)]
    bad += [{k: None} for k in tabs] + [{"ld_" + k: 63} for k in tabs]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_sample_weighted_validates_arguments_without_gpu(lib):
    def call(iu=P, ii=P, n_inter=10, first=0, count=4, rowptr=P, items=P, pcw=P, icw=P, U=5, I=7,
             n_neg=3, users=P, pos=P, neg=P):
        return lib.lgcn_bpr_sample_weighted(iu, ii, n_inter, None, first, count, rowptr, items,
                                            pcw, icw, U, I, 1, 0, n_neg, users, pos, neg, None,
                                            None)

    for kw in (dict(n_inter=-1), dict(U=-1), dict(I=-1), dict(n_inter=1 << 31), dict(U=1 << 31),
               dict(I=1 << 31), dict(first=-1), dict(count=-1), dict(n_neg=0), dict(n_neg=65),
               dict(iu=None), dict(ii=None), dict(rowptr=None), dict(items=None), dict(pcw=None),
               dict(icw=None), dict(users=None), dict(pos=None), dict(neg=None)):
        assert call(**kw) == -1, kw
    # count == 0 launches nothing and looks at no pointer
    assert call(count=0, iu=None, pcw=None, icw=None, neg=None) == 0
    assert call(count=0, n_neg=0) == -1
