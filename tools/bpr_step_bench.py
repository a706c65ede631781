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

Prints one JSON line on stdout (progress goes to stderr).

    python tools/bpr_step_bench.py [--config c3] [--blocks 5] [--steps-per-block 4]
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
from gcn_recommendation_amd.loss import bpr_loss_reg  # noqa: E402
from models.lightgcn import LightGCN  # noqa: E402

LAMBDA = 1e-4


def make_model(emb_host, U, I, d, K, dev):
    """bench_train_step's construction: the drop-in LightGCN over the bench's tables, no brands."""
    with contextlib.redirect_stdout(io.StringIO()):
        model = LightGCN.__new__(LightGCN)
        torch.nn.Module.__init__(model)
        model.num_users, model.num_items, model.num_brands = U, I, 0
        model.embedding_dim, model.n_layers, model.debug = d, K, False
        model.user_embedding = torch.nn.Embedding.from_pretrained(emb_host[0].clone(), freeze=False)
        model.brand_embedding = torch.nn.Embedding(0, d)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--gen", default="powerlaw", choices=["powerlaw", "uniform"])
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps-per-block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
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
    r, c, v = bench.make_graph(dict(cfg, brands=0), args.gen, 16)[:3]
    n = U + I
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((r, c))), torch.from_numpy(v),
                                  (n, n)).to(dev)
    nnz = len(v)
    del r, c, v
    models = {name: make_model(emb_host, U, I, d, K, dev) for name, _ in ROUTES}
    rng = np.random.default_rng(0)
    n_batches = max(args.blocks * args.steps_per_block, args.warmup) + 1
    batches = [tuple(torch.from_numpy(rng.integers(0, hi, args.batch)) for hi in (U, I, I))
               for _ in range(n_batches)]

    # ---- the first batch: same bits -------------------------------------------------------------
    first = tuple(t.to(dev) for t in batches[-1])
    got = {}
    for name, fn in ROUTES:
        m = models[name]
        loss = fn(m, adj, *first)
        loss.backward()
        got[name] = (loss.detach().clone(), {k: p.grad for k, p in m.named_parameters()})
    (l0, g0), (l1, g1) = got["main_route"], got["bpr_step"]
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
        per_block = {name: [] for name, _ in ROUTES}
        for name, fn in ROUTES:
            for b in batches[:args.warmup]:
                whole_step(name, fn, opts[name], b)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for blk in range(args.blocks):
            bs = batches[blk * args.steps_per_block:(blk + 1) * args.steps_per_block]
            for name, fn in ROUTES:
                torch.cuda.synchronize()
                a.record()
                for b in bs:
                    whole_step(name, fn, opts[name], b)
                e.record()
                torch.cuda.synchronize()
                per_block[name].append(a.elapsed_time(e) / len(bs))
        return per_block

    def blocks_of_phases(opts):
        per_block = {name: [] for name, _ in ROUTES}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for blk in range(args.blocks):
            bs = batches[blk * args.steps_per_block:(blk + 1) * args.steps_per_block]
            for name, fn in ROUTES:
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
    opts = {name: torch.optim.Adam(models[name].parameters(), lr=1e-3) for name, _ in ROUTES}
    whole = blocks_of_whole_steps(opts)
    phases = blocks_of_phases(opts)
    names = ("forward_and_loss", "backward", "adam")
    result["phases_ms"] = {
        name: {p: round(float(np.median(phases[name][:, i])), 3) for i, p in enumerate(names)}
        for name, _ in ROUTES}
    result["spread_ms"] = {p: round(float(np.ptp(phases["main_route"][:, i])), 3)
                           for i, p in enumerate(names)}
    result["phase_block_medians_ms"] = {
        name: {p: [round(float(x), 3) for x in phases[name][:, i]] for i, p in enumerate(names)}
        for name, _ in ROUTES}
    result["gain_ms"] = {p: round(result["phases_ms"]["main_route"][p]
                                  - result["phases_ms"]["bpr_step"][p], 3) for p in names[:2]}
    result["step_ms_adam_default"] = {name: round(float(np.median(whole[name])), 3)
                                      for name, _ in ROUTES}
    result["step_block_ms_adam_default"] = {name: [round(x, 3) for x in whole[name]]
                                            for name, _ in ROUTES}
    del opts
    opts = {name: torch.optim.Adam(models[name].parameters(), lr=1e-3, fused=True)
            for name, _ in ROUTES}
    whole = blocks_of_whole_steps(opts)
    result["step_ms_adam_fused"] = {name: round(float(np.median(whole[name])), 3)
                                    for name, _ in ROUTES}
    result["step_block_ms_adam_fused"] = {name: [round(x, 3) for x in whole[name]]
                                          for name, _ in ROUTES}
    # both models saw the same batches in the same order: still the same bits
    pa, pb = (dict(models[name].named_parameters()) for name, _ in ROUTES)
    result["parameters_bit_equal_after_run"] = all(bits_equal(pa[k], pb[k]) for k in pa)
    result["what"] = ("main.py:488-531 per batch on one device, main_route = model(adj) + six "
                      "gathers + bpr_loss_reg + backward, bpr_step = model.bpr_step + backward; "
                      "phases between events on the current stream (median per block of steps, "
                      "then over alternating blocks); spread_ms = max - min of main_route's block "
                      "medians; step_ms_* = whole steps incl. batch upload and loss.item()")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
