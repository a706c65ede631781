#!/usr/bin/env python
"""Time one BPR training step two ways in one process: main.py's route (model(adj), six gathers,
bpr_loss_reg, backward — bench.py's bench_train_step) and the fused model.bpr_step
(gcn_recommendation_amd.train), on bench.py's C3 graph and model construction.

  * the first batch's loss and parameter gradients are asserted bit-equal;
  * phases forward_and_loss / backward / adam: alternating blocks of steps per route, every
    phase bracketed by events on the current stream, median per block, then the median over the
    blocks; `spread_ms` is max - min of the block medians of main.py's route (what a difference
    between the routes has to exceed to mean anything);
  * whole steps (batch to device ... loss.item(), as main.py:488-531) with Adam's default
    (foreach) and fused=True, alternating blocks, median over the blocks.

--brand-loss times the brand-preference term (main.py --brand_loss) at the same shapes: the graph
gets --brands brand rows without edges, every item a brand, and three routes run in alternating
blocks — main_route_brand (model(adj), six gathers, bpr_loss_reg(brand_loss=True) fed by the device
lookups item_brand[pos] / item_brand[neg]), bpr_step_brand (model.bpr_step(item_brand=...)) and
the plain bpr_step beside them. bpr_step_brand's first batch is asserted bit-equal to the gathered
route through loss.bpr_brand_loss_reg; against bpr_loss_reg's torch expression of the brand term
the relative loss difference is reported.

--negatives M times training on the hardest of M candidate negatives instead (and nothing else):
the plain one-negative step, the fused bpr_step(neg [B, M], negatives="hardest") and the route
composed of the one-negative API (model(adj) under no_grad, gather, argmax, bpr_step), forward +
backward, in alternating blocks of one process (time_negatives).

--negatives M --softmax [--temperature T] times the sampled-softmax step over all M candidates
(time_softmax): the one-negative step, "hardest", "all", "softmax" and the autograd route of the
softmax expression (model(adj), the gathers, loss.ssm_loss_torch, backward), forward + backward,
in alternating blocks of one process; the first batch's fused loss and gradients are asserted
bit-equal to the gathered route through loss.ssm_loss_reg.

--negatives M --softmax --neg-log-q adds the route softmax_logq: the same step with neg_log_q =
the log Q of a popularity^0.75 draw over a Zipf-like catalogue (lgcn_ssm_loss_indexed_q), its first
batch asserted bit-equal to the gathered route through loss.ssm_loss_reg(q_pos=, q_neg=).

--in-batch [--mask-positives] [--log-q] [--temperature T] times the in-batch softmax step
(time_in_batch): the one-negative step, model.inbatch_step, the autograd route of the same
expression (model(adj), the gathers, loss.inbatch_off_mask, loss.inbatch_loss_torch, backward) and
the sampled-softmax step at M = 16 and M = 64, forward + backward, in alternating blocks of one
process, on batches drawn from the graph's interactions; the first batch's fused loss and gradients
are asserted bit-equal to the gathered route through loss.inbatch_loss_reg.

Prints one JSON line on stdout (progress goes to stderr).

    python tools/bpr_step_bench.py [--config c3] [--blocks 5] [--steps-per-block 4] [--brand-loss]
    python tools/bpr_step_bench.py --negatives 4
    python tools/bpr_step_bench.py --negatives 16 --softmax --temperature 0.2
    python tools/bpr_step_bench.py --negatives 16 64 --softmax --neg-log-q
    python tools/bpr_step_bench.py --in-batch --mask-positives --log-q
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, make_graph, xavier: the generator bench.py times)
from gcn_recommendation_amd import engine  # noqa: E402
from gcn_recommendation_amd.loss import (bpr_brand_loss_reg, bpr_loss_reg,  # noqa: E402
                                         inbatch_loss_reg, inbatch_loss_torch, inbatch_off_mask,
                                         ssm_loss_reg, ssm_loss_torch)
from gcn_recommendation_amd.sampler import BprSampler, quantise_weights  # noqa: E402
from models.lightgcn import LightGCN  # noqa: E402

LAMBDA = 1e-4


def make_model(emb_host, U, I, d, K, dev, brands=None):
    """bench_train_step's construction: the drop-in LightGCN over the bench's tables, no brands
    (or the [n_brands x d] table `brands`)."""
    with contextlib.redirect_stdout(io.StringIO()):
        model = LightGCN.__new__(LightGCN)
        torch.nn.Module.__init__(model)
        model.num_users, model.num_items = U, I
        model.num_brands = 0 if brands is None else int(brands.shape[0])
        model.embedding_dim, model.n_layers, model.debug = d, K, False
        model.user_embedding = torch.nn.Embedding.from_pretrained(emb_host[0].clone(), freeze=False)
        model.brand_embedding = torch.nn.Embedding(0, d) if brands is None else \
            torch.nn.Embedding.from_pretrained(brands.clone(), freeze=False)
        model.item_embedding = torch.nn.Embedding.from_pretrained(emb_host[1].clone(), freeze=False)
        model.final_brand_emb, model._graph_adj = None, None
    return model.to(dev)


def loss_main(model, adj, users, pos, neg):
    fu, fi, fb, u0, i0 = model(adj, use_brand=False)
    return bpr_loss_reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg], LAMBDA)


def loss_step(model, adj, users, pos, neg):
    return model.bpr_step(adj, users, pos, neg, LAMBDA)


ROUTES = (("main_route", loss_main), ("bpr_step", loss_step))


def bits_equal(a, b):
    if a is None or b is None:  # a parameter that got no gradient (the empty brand table)
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32),
                                              b.detach().view(torch.int32))


def time_negatives(args, M, adj, m, U, I, dev, result):
    """--negatives M: three routes in alternating blocks of whole forward + backward steps (no
    optimizer: the one model stays put, so every route sees the same tables on every batch),
      plain     the one-negative bpr_step on candidate 0;
      fused     bpr_step on the [B, M] candidates, negatives="hardest": one propagation, the
                choice made between it and the loss;
      composed  what the one-negative API alone allows: model(adj) under no_grad, gather, argmax,
                then bpr_step on the choice — two propagations.
    The first batch's fused and composed choices are compared (torch's score sums may break a
    near-tie the other way: the count of differing samples is reported, not asserted)."""
    rng = np.random.default_rng(1)
    n_batches = args.blocks * args.steps_per_block + args.warmup
    batches = [(torch.from_numpy(rng.integers(0, U, args.batch)).to(dev),
                torch.from_numpy(rng.integers(0, I, args.batch)).to(dev),
                torch.from_numpy(rng.integers(0, I, (args.batch, M))).to(dev))
               for _ in range(n_batches)]

    def plain(m, users, pos, cand):
        return m.bpr_step(adj, users, pos, cand[:, 0].contiguous(), LAMBDA)

    def fused(m, users, pos, cand):
        return m.bpr_step(adj, users, pos, cand, LAMBDA, negatives="hardest")

    def composed_choice(m, users, cand):
        with torch.no_grad():
            fu, fi = m(adj, use_brand=False)[:2]
            scores = (fu[users].unsqueeze(1) * fi[cand]).sum(-1)
            return cand.gather(1, scores.argmax(1, keepdim=True)).squeeze(1)

    def composed(m, users, pos, cand):
        return m.bpr_step(adj, users, pos, composed_choice(m, users, cand), LAMBDA)

    routes = (("plain", plain), ("fused_hardest", fused), ("composed_hardest", composed))
    users, pos, cand = batches[-1]
    _, used = m.bpr_step(adj, users, pos, cand, LAMBDA, return_negatives=True)
    differ = int((used != composed_choice(m, users, cand)).sum().item())

    def step(fn, b):
        m.zero_grad(set_to_none=True)
        fn(m, *b).backward()

    for name, fn in routes:
        for b in batches[:args.warmup]:
            step(fn, b)
    per_block = {name: [] for name, _ in routes}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for blk in range(args.blocks):
        lo = args.warmup + blk * args.steps_per_block
        for name, fn in routes:
            torch.cuda.synchronize()
            a.record()
            for b in batches[lo:lo + args.steps_per_block]:
                step(fn, b)
            e.record()
            torch.cuda.synchronize()
            per_block[name].append(a.elapsed_time(e) / args.steps_per_block)
    med = {name: float(np.median(v)) for name, v in per_block.items()}
    result.update(
        negatives=M,
        step_ms={name: round(v, 3) for name, v in med.items()},
        step_block_ms={name: [round(x, 3) for x in v] for name, v in per_block.items()},
        spread_ms={name: round(float(np.ptp(v)), 3) for name, v in per_block.items()},
        fused_minus_plain_ms=round(med["fused_hardest"] - med["plain"], 3),
        composed_minus_fused_ms=round(med["composed_hardest"] - med["fused_hardest"], 3),
        fused_not_slower_than_composed=bool(med["fused_hardest"] <= med["composed_hardest"]),
        first_batch_choices_differing=differ,
        what=("forward + backward of one batch, zero_grad before, no optimizer step; events "
              "around alternating blocks of steps per route, median over the blocks; spread_ms = "
              "max - min of a route's block medians; plain = bpr_step on candidate 0, "
              "fused_hardest = bpr_step(neg [B, M], negatives='hardest'), composed_hardest = "
              "model(adj) under no_grad + gather + argmax + bpr_step"))
    print(json.dumps(result), flush=True)


def time_softmax(args, M, adj, models, U, I, dev, result):
    """--negatives M --softmax: five routes in alternating blocks of whole forward + backward
    steps (no optimizer: the tables stay put, so every route sees the same ones on every batch),
      plain      the one-negative bpr_step on candidate 0;
      hardest    bpr_step(neg [B, M], negatives="hardest");
      all        bpr_step(neg [B, M], negatives="all"): BPR on the B*M expanded triples;
      softmax    bpr_step(neg [B, M], negatives="softmax", temperature=T);
      autograd   the same expression without the fused path: model(adj), the 2 * (2 + M) * B row
                 gathers, loss.ssm_loss_torch, backward.
    Before timing, the first batch's softmax loss and parameter gradients are asserted bit-equal
    to the gathered route through loss.ssm_loss_reg (model(adj), the gathers, lgcn_ssm_loss)."""
    T = args.temperature
    m, other = models
    rng = np.random.default_rng(1)
    n_batches = args.blocks * args.steps_per_block + args.warmup
    batches = [(torch.from_numpy(rng.integers(0, U, args.batch)).to(dev),
                torch.from_numpy(rng.integers(0, I, args.batch)).to(dev),
                torch.from_numpy(rng.integers(0, I, (args.batch, M))).to(dev))
               for _ in range(n_batches)]

    def gathered(m, users, pos, cand, reg):
        fu, fi, fb, u0, i0 = m(adj, use_brand=False)
        flat = cand.reshape(-1)
        shape = (cand.shape[0], M, -1)
        return reg(fu[users], fi[pos], fi[flat].view(shape), u0[users], i0[pos],
                   i0[flat].view(shape), LAMBDA, T)

    def plain(m, users, pos, cand):
        return m.bpr_step(adj, users, pos, cand[:, 0].contiguous(), LAMBDA)

    def mode(name):
        return lambda m, users, pos, cand: m.bpr_step(adj, users, pos, cand, LAMBDA,
                                                      negatives=name, temperature=T)

    def autograd(m, users, pos, cand):
        return gathered(m, users, pos, cand, ssm_loss_torch)

    routes = (("plain", plain), ("hardest", mode("hardest")), ("all", mode("all")),
              ("softmax", mode("softmax")), ("autograd_softmax", autograd))
    if args.neg_log_q:
        # log Q of a popularity^0.75 draw over Zipf-like counts, the ranks scattered over the ids
        count = 1e6 / (1.0 + np.random.default_rng(2).permutation(I))
        w = quantise_weights(count ** 0.75).astype(np.float64)
        q = torch.from_numpy(np.log(w / w.sum()).astype(np.float32)).to(dev)

        def softmax_logq(m, users, pos, cand):
            return m.bpr_step(adj, users, pos, cand, LAMBDA, negatives="softmax", temperature=T,
                              neg_log_q=q)

        def gathered_q(m, users, pos, cand):
            fu, fi, fb, u0, i0 = m(adj, use_brand=False)
            flat = cand.reshape(-1)
            shape = (cand.shape[0], M, -1)
            return ssm_loss_reg(fu[users], fi[pos], fi[flat].view(shape), u0[users], i0[pos],
                                i0[flat].view(shape), LAMBDA, T, q_pos=q[pos],
                                q_neg=q[flat].view(cand.shape))

        routes += (("softmax_logq", softmax_logq),)
        for x in (m, other):
            x.zero_grad(set_to_none=True)
        got = softmax_logq(m, *batches[-1])
        got.backward()
        want = gathered_q(other, *batches[-1])
        want.backward()
        assert bits_equal(got, want), f"logQ loss differs: {got.item()!r} vs {want.item()!r}"
        ga, gb = dict(m.named_parameters()), dict(other.named_parameters())
        for k in ga:
            assert bits_equal(ga[k].grad, gb[k].grad), f"logQ gradient of {k} differs"
        bench.log(f"[bpr_step_bench] softmax_logq M={M}: loss {got.item():.6f} and {len(ga)} "
                  "gradients bit-equal to the gathered route")
        del got, want

    first = batches[-1]
    for x in (m, other):  # a model timed at another M before still holds its last gradients
        x.zero_grad(set_to_none=True)
    got = mode("softmax")(m, *first)
    got.backward()
    want = gathered(other, *first, ssm_loss_reg)
    want.backward()
    assert bits_equal(got, want), f"loss differs: {got.item()!r} vs {want.item()!r}"
    ga, gb = dict(m.named_parameters()), dict(other.named_parameters())
    for k in ga:
        assert bits_equal(ga[k].grad, gb[k].grad), f"gradient of {k} differs"
    torch_loss = autograd(other, *first).item()
    bench.log(f"[bpr_step_bench] softmax M={M}: loss {got.item():.6f} and {len(ga)} gradients "
              "bit-equal to the gathered route")
    loss_rel_diff = abs(got.item() - torch_loss) / abs(torch_loss)
    other.zero_grad(set_to_none=True)
    del got, want

    def step(fn, b):
        m.zero_grad(set_to_none=True)
        fn(m, *b).backward()

    for name, fn in routes:
        for b in batches[:args.warmup]:
            step(fn, b)
    per_block = {name: [] for name, _ in routes}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for blk in range(args.blocks):
        lo = args.warmup + blk * args.steps_per_block
        for name, fn in routes:
            torch.cuda.synchronize()
            a.record()
            for b in batches[lo:lo + args.steps_per_block]:
                step(fn, b)
            e.record()
            torch.cuda.synchronize()
            per_block[name].append(a.elapsed_time(e) / args.steps_per_block)
    med = {name: float(np.median(v)) for name, v in per_block.items()}
    spread = {name: float(np.ptp(v)) for name, v in per_block.items()}
    result.update(
        negatives=M, temperature=T, first_batch_bit_equal=True,
        loss_rel_diff_vs_torch_expression=loss_rel_diff,
        step_ms={name: round(v, 3) for name, v in med.items()},
        step_block_ms={name: [round(x, 3) for x in v] for name, v in per_block.items()},
        spread_ms={name: round(v, 3) for name, v in spread.items()},
        all_minus_softmax_ms=round(med["all"] - med["softmax"], 3),
        autograd_minus_softmax_ms=round(med["autograd_softmax"] - med["softmax"], 3),
        softmax_minus_plain_ms=round(med["softmax"] - med["plain"], 3),
        softmax_faster_than_all=bool(med["softmax"] < med["all"]),
        softmax_faster_than_autograd=bool(med["softmax"] < med["autograd_softmax"]),
        **({"softmax_logq_minus_softmax_ms": round(med["softmax_logq"] - med["softmax"], 3),
            "softmax_logq_first_batch_bit_equal": True} if args.neg_log_q else {}),
        scatter_keys={"softmax": (2 + M) * args.batch, "all": 3 * M * args.batch},
        what=("forward + backward of one batch, zero_grad before, no optimizer step; device "
              "events around alternating blocks of steps per route, median over the blocks; "
              "spread_ms = max - min of a route's block medians; plain = bpr_step on candidate 0, "
              "hardest / all / softmax = bpr_step(neg [B, M], negatives=...), autograd_softmax = "
              "model(adj) + gathers + loss.ssm_loss_torch + backward" +
              ("; softmax_logq = softmax with neg_log_q" if args.neg_log_q else "")))
    print(json.dumps(result), flush=True)


def time_in_batch(args, adj, models, smp, U, I, dev, result):
    """--in-batch [--mask-positives] [--log-q]: whole forward + backward steps in alternating
    blocks (no optimizer: the tables stay put), batches drawn from the graph's own interactions —
    so popular items repeat inside a batch, as in training —
      plain        the one-negative bpr_step on a uniform negative;
      in_batch     model.inbatch_step(adj, users, pos, ..., positives=, item_log_q=);
      autograd     the same expression composed of public torch calls: model(adj), the gathers,
                   loss.inbatch_off_mask, loss.inbatch_loss_torch, backward;
      softmax_16 / softmax_64   bpr_step(neg [B, M], negatives="softmax") on uniform candidates.
    Before timing, the first batch's in_batch loss and parameter gradients are asserted bit-equal
    to the gathered route through loss.inbatch_loss_reg."""
    T = args.temperature
    m, other = models
    rng = np.random.default_rng(1)
    n_batches = args.blocks * args.steps_per_block + args.warmup
    iu, ii = smp._user, smp._item          # the interactions, int32 on the device
    batches = []
    for _ in range(n_batches):
        idx = torch.from_numpy(rng.integers(0, len(smp), args.batch)).to(dev)
        batches.append((iu[idx].long(), ii[idx].long(),
                        torch.from_numpy(rng.integers(0, I, (args.batch, 64))).to(dev)))
    csr = smp.positives() if args.mask_positives else None
    qtab = smp.item_log_q() if args.log_q else None

    def gathered(m, users, pos, reg):
        fu, fi, fb, u0, i0 = m(adj, use_brand=False)
        return reg(fu[users], fi[pos], u0[users], i0[pos], LAMBDA, T,
                   off=inbatch_off_mask(users, pos, csr), q=None if qtab is None else qtab[pos])

    def plain(m, users, pos, cand):
        return m.bpr_step(adj, users, pos, cand[:, 0].contiguous(), LAMBDA)

    def in_batch(m, users, pos, cand):
        return m.inbatch_step(adj, users, pos, LAMBDA, T, positives=csr, item_log_q=qtab)

    def autograd(m, users, pos, cand):
        return gathered(m, users, pos, inbatch_loss_torch)

    def softmax(M):
        return lambda m, users, pos, cand: m.bpr_step(
            adj, users, pos, cand[:, :M].contiguous(), LAMBDA, negatives="softmax", temperature=T)

    routes = (("plain", plain), ("in_batch", in_batch), ("autograd_in_batch", autograd),
              ("softmax_16", softmax(16)), ("softmax_64", softmax(64)))

    first = batches[-1]
    got = in_batch(m, *first)
    got.backward()
    want = gathered(other, *first[:2], inbatch_loss_reg)
    want.backward()
    assert bits_equal(got, want), f"loss differs: {got.item()!r} vs {want.item()!r}"
    ga, gb = dict(m.named_parameters()), dict(other.named_parameters())
    for k in ga:
        assert bits_equal(ga[k].grad, gb[k].grad), f"gradient of {k} differs"
    torch_loss = autograd(other, *first).item()
    bench.log(f"[bpr_step_bench] in-batch: loss {got.item():.6f} and {len(ga)} gradients "
              "bit-equal to the gathered route")
    loss_rel_diff = abs(got.item() - torch_loss) / abs(torch_loss)
    off = inbatch_off_mask(first[0], first[1], csr)
    off_fraction = off.sum().item() / (args.batch * (args.batch - 1))
    top_share = first[1].bincount().max().item() / args.batch
    other.zero_grad(set_to_none=True)
    del got, want, off

    def step(fn, b):
        m.zero_grad(set_to_none=True)
        fn(m, *b).backward()

    for name, fn in routes:
        for b in batches[:args.warmup]:
            step(fn, b)
    per_block = {name: [] for name, _ in routes}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for blk in range(args.blocks):
        lo = args.warmup + blk * args.steps_per_block
        for name, fn in routes:
            torch.cuda.synchronize()
            a.record()
            for b in batches[lo:lo + args.steps_per_block]:
                step(fn, b)
            e.record()
            torch.cuda.synchronize()
            per_block[name].append(a.elapsed_time(e) / args.steps_per_block)
    med = {name: float(np.median(v)) for name, v in per_block.items()}
    result.update(
        in_batch=True, mask_positives=bool(args.mask_positives), log_q=bool(args.log_q),
        temperature=T, first_batch_bit_equal=True,
        loss_rel_diff_vs_torch_expression=loss_rel_diff,
        first_batch_off_fraction=round(off_fraction, 5),
        first_batch_top_item_share=round(top_share, 4),
        step_ms={name: round(v, 3) for name, v in med.items()},
        step_block_ms={name: [round(x, 3) for x in v] for name, v in per_block.items()},
        spread_ms={name: round(float(np.ptp(v)), 3) for name, v in per_block.items()},
        in_batch_minus_plain_ms=round(med["in_batch"] - med["plain"], 3),
        autograd_minus_in_batch_ms=round(med["autograd_in_batch"] - med["in_batch"], 3),
        softmax_16_minus_in_batch_ms=round(med["softmax_16"] - med["in_batch"], 3),
        softmax_64_minus_in_batch_ms=round(med["softmax_64"] - med["in_batch"], 3),
        in_batch_faster_than_autograd=bool(med["in_batch"] < med["autograd_in_batch"]),
        in_batch_not_slower_than_softmax_16=bool(med["in_batch"] <= med["softmax_16"]),
        scatter_keys={"plain": 3 * args.batch, "in_batch": 2 * args.batch,
                      "softmax_16": 18 * args.batch, "softmax_64": 66 * args.batch},
        what=("forward + backward of one batch, zero_grad before, no optimizer step; device "
              "events around alternating blocks of steps per route, median over the blocks; "
              "spread_ms = max - min of a route's block medians; users / positives drawn from "
              "the graph's interactions, negatives and candidates uniform; plain = bpr_step on "
              "candidate 0, in_batch = model.inbatch_step, autograd_in_batch = model(adj) + "
              "gathers + loss.inbatch_off_mask + loss.inbatch_loss_torch + backward, softmax_M = "
              "bpr_step(neg [B, M], negatives='softmax')"))
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-batch", action="store_true",
                    help="time the in-batch softmax step beside the plain step, the autograd "
                         "route of the same expression and the sampled-softmax step at M = 16, 64")
    ap.add_argument("--mask-positives", action="store_true",
                    help="with --in-batch: drop each user's known positives from its negatives")
    ap.add_argument("--log-q", action="store_true",
                    help="with --in-batch: the logQ correction of the logits")
    ap.add_argument("--negatives", type=int, nargs="+", default=None, metavar="M",
                    help="time the hardest-of-M step against the plain step and the composed "
                         "route (and nothing else); several M: one after the other on one graph")
    ap.add_argument("--softmax", action="store_true",
                    help="with --negatives: time the sampled-softmax step over all M candidates "
                         "beside the plain, hardest and all steps and the autograd route")
    ap.add_argument("--neg-log-q", action="store_true",
                    help="with --softmax: also time the step with the logQ correction neg_log_q")
    ap.add_argument("--temperature", type=float, default=0.2, help="temperature of --softmax")
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--gen", default="powerlaw", choices=["powerlaw", "uniform"])
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps-per-block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brand-loss", action="store_true",
                    help="time the brand-preference term: main_route_brand, bpr_step_brand and "
                         "the plain bpr_step in one run")
    ap.add_argument("--brands", type=int, default=4096, help="brand rows of --brand-loss")
    ap.add_argument("--brand-loss-weight", type=float, default=0.1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bpr_step_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    engine.load_library()
    cfg = bench.CONFIGS[args.config]
    U, I, d, K = cfg["users"], cfg["items"], cfg["d"], cfg["K"]
    gen = torch.Generator().manual_seed(42)
    emb_host = [bench.xavier(U, d, gen), bench.xavier(I, d, gen)]
    if (args.mask_positives or args.log_q) and not args.in_batch:
        sys.exit("bpr_step_bench: --mask-positives and --log-q belong to --in-batch")
    if args.in_batch and (args.negatives or args.softmax or args.brand_loss):
        sys.exit("bpr_step_bench: --in-batch runs alone")
    r, c, v, _, _, inter = bench.make_graph(dict(cfg, brands=0), args.gen, 16,
                                            keep_interactions=args.in_batch)
    NB = args.brands if args.brand_loss else 0
    n = U + I + NB  # the brand rows of --brand-loss have no edges: the graph is the same
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((r, c))), torch.from_numpy(v),
                                  (n, n)).to(dev)
    nnz = len(v)
    del r, c, v
    if args.in_batch:
        smp = BprSampler(inter[0], inter[1], U, I, dev)
        del inter
        models = (make_model(emb_host, U, I, d, K, dev), make_model(emb_host, U, I, d, K, dev))
        result = {"config": cfg["name"], "nnz": nnz, "d": d, "K": K, "batch": args.batch,
                  "blocks": args.blocks, "steps_per_block": args.steps_per_block}
        time_in_batch(args, adj, models, smp, U, I, dev, result)
        return
    if args.softmax and not args.negatives:
        sys.exit("bpr_step_bench: --softmax needs --negatives M")
    if args.neg_log_q and not args.softmax:
        sys.exit("bpr_step_bench: --neg-log-q belongs to --negatives M --softmax")
    if args.negatives:
        if args.brand_loss or not all(1 <= M <= engine.BPR_MAX_NEG for M in args.negatives):
            sys.exit(f"bpr_step_bench: --negatives takes 1..{engine.BPR_MAX_NEG}, without "
                     "--brand-loss")
        model = make_model(emb_host, U, I, d, K, dev)
        for M in args.negatives:   # one JSON line per M
            result = {"config": cfg["name"], "nnz": nnz, "d": d, "K": K, "batch": args.batch,
                      "blocks": args.blocks, "steps_per_block": args.steps_per_block}
            if args.softmax:
                other = make_model(emb_host, U, I, d, K, dev)
                time_softmax(args, M, adj, (model, other), U, I, dev, result)
                del other
            else:
                time_negatives(args, M, adj, model, U, I, dev, result)
        return
    if args.brand_loss:
        if NB < 1:
            sys.exit("bpr_step_bench: --brand-loss needs --brands >= 1")
        emb_host.append(bench.xavier(NB, d, gen))
        item_brand = torch.from_numpy(np.random.default_rng(7).integers(0, NB, I)).to(
            dev, torch.int32)
        w = args.brand_loss_weight

        def loss_main_brand(model, adj, users, pos, neg, reg=bpr_loss_reg):
            fu, fi, fb, u0, i0 = model(adj, use_brand=False)
            return reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg], LAMBDA,
                       brand_loss=True, final_brand_emb=fb,
                       pos_item_brand_idx=item_brand[pos].long(),
                       neg_item_brand_idx=item_brand[neg].long(), brand_loss_weight=w)

        def loss_step_brand(model, adj, users, pos, neg):
            return model.bpr_step(adj, users, pos, neg, LAMBDA, item_brand=item_brand,
                                  brand_loss_weight=w)

        routes = (("main_route_brand", loss_main_brand), ("bpr_step_brand", loss_step_brand),
                  ("bpr_step", loss_step))
    else:
        routes = ROUTES
    REF, FUSED = routes[0][0], routes[1][0]
    models = {name: make_model(emb_host, U, I, d, K, dev, emb_host[2] if NB else None)
              for name, _ in routes}
    rng = np.random.default_rng(0)
    n_batches = max(args.blocks * args.steps_per_block, args.warmup) + 1
    batches = [tuple(torch.from_numpy(rng.integers(0, hi, args.batch)) for hi in (U, I, I))
               for _ in range(n_batches)]

    # ---- the first batch: same bits -------------------------------------------------------------
    first = tuple(t.to(dev) for t in batches[-1])
    got = {}
    for name, fn in routes:
        m = models[name]
        loss = fn(m, adj, *first)
        loss.backward()
        got[name] = (loss.detach().clone(), {k: p.grad for k, p in m.named_parameters()})
    (l0, g0), (l1, g1) = got[REF], got[FUSED]
    loss_rel_diff = None
    if args.brand_loss:  # REF's brand term is torch's expression: bit-equal to the gathered route
        loss_rel_diff = abs(l0.item() - l1.item()) / abs(l0.item())
        m = make_model(emb_host, U, I, d, K, dev, emb_host[2])
        l0 = loss_main_brand(m, adj, *first, reg=bpr_brand_loss_reg)
        l0.backward()
        l0, g0 = l0.detach().clone(), {k: p.grad for k, p in m.named_parameters()}
        del m
    assert bits_equal(l0, l1), f"loss differs: {l0.item()!r} vs {l1.item()!r}"
    for k in g0:
        assert bits_equal(g0[k], g1[k]), f"gradient of {k} differs"
    bench.log(f"[bpr_step_bench] first batch: loss {l0.item():.6f} and {len(g0)} gradients bit-equal")
    del got, g0, g1
    for m in models.values():
        m.zero_grad(set_to_none=True)

    def whole_step(name, fn, opt, b):
        users, pos, neg = (t.to(dev) for t in b)
        opt.zero_grad()
        loss = fn(models[name], adj, users, pos, neg)
        loss.backward()
        opt.step()
        return loss.item()

    def blocks_of_whole_steps(opts):
        per_block = {name: [] for name, _ in routes}
        for name, fn in routes:
            for b in batches[:args.warmup]:
                whole_step(name, fn, opts[name], b)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for blk in range(args.blocks):
            bs = batches[blk * args.steps_per_block:(blk + 1) * args.steps_per_block]
            for name, fn in routes:
                torch.cuda.synchronize()
                a.record()
                for b in bs:
                    whole_step(name, fn, opts[name], b)
                e.record()
                torch.cuda.synchronize()
                per_block[name].append(a.elapsed_time(e) / len(bs))
        return per_block

    def blocks_of_phases(opts):
        per_block = {name: [] for name, _ in routes}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for blk in range(args.blocks):
            bs = batches[blk * args.steps_per_block:(blk + 1) * args.steps_per_block]
            for name, fn in routes:
                rows = []
                for b in bs:
                    users, pos, neg = (t.to(dev) for t in b)
                    torch.cuda.synchronize()
                    ev[0].record()
                    opts[name].zero_grad()
                    loss = fn(models[name], adj, users, pos, neg)
                    ev[1].record()
                    loss.backward()
                    ev[2].record()
                    opts[name].step()
                    ev[3].record()
                    torch.cuda.synchronize()
                    rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
                per_block[name].append(np.median(np.array(rows), axis=0))
        return {name: np.array(v) for name, v in per_block.items()}

    result = {"config": cfg["name"], "nnz": nnz, "d": d, "K": K, "batch": args.batch,
              "blocks": args.blocks, "steps_per_block": args.steps_per_block,
              "first_batch_bit_equal": True}
    if args.brand_loss:
        result.update(brands=NB, brand_loss_weight=w, loss_rel_diff_vs_torch_brand_term=loss_rel_diff)
    opts = {name: torch.optim.Adam(models[name].parameters(), lr=1e-3) for name, _ in routes}
    whole = blocks_of_whole_steps(opts)
    bench.log("[bpr_step_bench] whole steps (Adam default) done")
    phases = blocks_of_phases(opts)
    bench.log("[bpr_step_bench] phases done")
    names = ("forward_and_loss", "backward", "adam")
    result["phases_ms"] = {
        name: {p: round(float(np.median(phases[name][:, i])), 3) for i, p in enumerate(names)}
        for name, _ in routes}
    result["spread_ms"] = {p: round(float(np.ptp(phases[REF][:, i])), 3)
                           for i, p in enumerate(names)}
    result["phase_block_medians_ms"] = {
        name: {p: [round(float(x), 3) for x in phases[name][:, i]] for i, p in enumerate(names)}
        for name, _ in routes}
    result["gain_ms"] = {p: round(result["phases_ms"][REF][p]
                                  - result["phases_ms"][FUSED][p], 3) for p in names[:2]}
    result["step_ms_adam_default"] = {name: round(float(np.median(whole[name])), 3)
                                      for name, _ in routes}
    result["step_block_ms_adam_default"] = {name: [round(x, 3) for x in whole[name]]
                                            for name, _ in routes}
    del opts
    opts = {name: torch.optim.Adam(models[name].parameters(), lr=1e-3, fused=True)
            for name, _ in routes}
    whole = blocks_of_whole_steps(opts)
    result["step_ms_adam_fused"] = {name: round(float(np.median(whole[name])), 3)
                                    for name, _ in routes}
    result["step_block_ms_adam_fused"] = {name: [round(x, 3) for x in whole[name]]
                                          for name, _ in routes}
    # both models saw the same batches in the same order: still the same bits
    if not args.brand_loss:
        pa, pb = (dict(models[name].named_parameters()) for name, _ in routes)
        result["parameters_bit_equal_after_run"] = all(bits_equal(pa[k], pb[k]) for k in pa)
    result["what"] = ("main.py:488-531 per batch on one device, main_route = model(adj) + six "
                      "gathers + bpr_loss_reg + backward, bpr_step = model.bpr_step + backward; "
                      "phases between events on the current stream (median per block of steps, "
                      "then over alternating blocks); spread_ms = max - min of main_route's block "
                      "medians; step_ms_* = whole steps incl. batch upload and loss.item()")
    if args.brand_loss:
        result["what"] += ("; --brand-loss: main_route_brand = the same with bpr_loss_reg("
                           "brand_loss=True) on device lookups item_brand[pos], bpr_step_brand = "
                           "model.bpr_step(item_brand=...), brand rows without edges")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
