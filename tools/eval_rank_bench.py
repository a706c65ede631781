#!/usr/bin/env python
"""Time the rank evaluation against the top-k evaluation in one process, at the evaluation shape
bench.py times (C3: 8192 users x the 4.4M-item table, d = 64, the train mask of bench.py's
power-law interactions):

  * kernel: one lgcn_score_rank call (three launches) and one lgcn_score_topk call (k = 20, two
    launches) on the same batch, tables, mask and split count, between events on the current
    stream, alternating, median of --reps; outputs and scratch allocated beforehand;
  * pass: one Evaluator.evaluate (mask resident, users and targets resident, one read-back) and
    one evaluate.evaluate (host mask rebuilt and re-uploaded per batch, a top-k list copied back
    per batch) over the same --heldout users, wall clock around a device synchronise, alternating,
    median of --pass-reps. The model is a module whose forward returns the two tables, so the
    propagation, which both passes run once, is not in either figure.

The tables are seeded N(0, 0.1) draws of the C3 shape (the scores of a trained model are not
needed to time either kernel; the top-k kernel's candidate traffic depends on the score
distribution only through the first tiles). Checked before timing: for every slot whose target is
in the top-20 list the rank is its place there and the score is the list's, bit for bit; every
other rank is >= 20; both passes return the same recall@20 / ndcg@20.

Prints one JSON line on stdout (progress goes to stderr).

    timeout -k 10 840 python tools/eval_rank_bench.py [--config c3] [--reps 9] [--heldout 65536]

One process, so every figure comes from one machine in one run; it holds the GPU for the whole of
it and is therefore started under a time limit of its own, as every GPU step is.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, log: the shapes bench.py times)
from gcn_recommendation_amd import engine, evaluate as E, graph  # noqa: E402


class Tables(torch.nn.Module):
    """A model for both evaluation passes: its forward returns the two tables as they are."""

    def __init__(self, ue, ie):
        super().__init__()
        self.ue, self.ie = ue, ie

    def forward(self, adj):
        return self.ue, self.ie, None, None, None


def event_ms(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--heldout", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pass-reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_rank_bench: needs a HIP device")
    import pandas as pd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = engine.load_library()
    cfg = bench.CONFIGS[args.config]
    U, I, n_inter, d, k = cfg["users"], cfg["items"], cfg["interactions"], cfg["d"], args.k
    t0 = time.perf_counter()
    tu, ti = graph.powerlaw_interactions(U, I, n_inter, cfg["seed"])
    bench.log(f"[eval_rank_bench] {n_inter:,} interactions in {time.perf_counter() - t0:.1f}s")
    t0 = time.perf_counter()
    ev = E.Evaluator(tu, ti, U, I, dev)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    bench.log(f"[eval_rank_bench] evaluator (mask CSR, resident) built in {build_s:.1f}s")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ue = torch.randn((U, d), generator=g, device=dev) * 0.1
    ie = torch.randn((I, d), generator=g, device=dev) * 0.1

    # ---- the kernels: one batch of bench.py's evaluation shape ----------------------------------
    rng = np.random.default_rng(7)
    n = min(args.users, U)
    users = torch.from_numpy(np.sort(rng.choice(U, n, replace=False)).astype(np.int32)).to(dev)
    splits = lib.lgcn_eval_splits(n, I, E._device_cus(dev))
    part_s = torch.empty((splits, n, k), dtype=torch.float32, device=dev)
    part_i = torch.empty((splits, n, k), dtype=torch.int32, device=dev)
    top_s = torch.empty((n, k), dtype=torch.float32, device=dev)
    top_i = torch.empty((n, k), dtype=torch.int32, device=dev)
    part = torch.empty(splits * n, dtype=torch.int32, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    P, stream = engine._ptr, engine._stream(dev)

    def topk():
        engine._check(lib.lgcn_score_topk(P(ue), d, P(users), n, P(ie), d, I, d, P(ev._rowptr),
                                          P(ev._items), k, splits, P(part_s), P(part_i), P(top_s),
                                          P(top_i), stream), "lgcn_score_topk")

    topk()
    # targets: every other slot an item of its top-k list (a hit), the others anywhere
    targets = torch.from_numpy(rng.integers(0, I, n).astype(np.int32)).to(dev)
    place = torch.from_numpy(rng.integers(0, k, n)).to(dev)
    targets[::2] = top_i.gather(1, place[:, None])[::2, 0]

    def rank_call():
        E._rank_launch(ue, ie, users, targets, ev._rowptr, ev._items, rank, score, part, splits)

    rank_call()
    torch.cuda.synchronize()
    hit = top_i == targets[:, None]
    listed = hit.any(1)
    where = hit.int().argmax(1)
    assert torch.equal(rank[listed], where[listed].int()), "rank != place in the top-k list"
    assert torch.equal(score[listed].view(torch.int32),
                       top_s.gather(1, where[:, None])[listed, 0].view(torch.int32))
    assert bool((rank[~listed] >= k).all()), "an unlisted target ranks inside the list"
    t_rank, t_topk = [], []
    for _ in range(args.reps):  # alternating: both see the same machine state
        t_rank.append(event_ms(rank_call))
        t_topk.append(event_ms(topk))
    rank_ms, topk_ms = float(np.median(t_rank)), float(np.median(t_topk))
    bench.log(f"[eval_rank_bench] lgcn_score_rank {rank_ms:.2f} ms, lgcn_score_topk(k={k}) "
              f"{topk_ms:.2f} ms, {splits} splits")

    # ---- the passes: Evaluator.evaluate vs evaluate.evaluate ------------------------------------
    h = min(args.heldout, U)
    hu = rng.choice(U, h, replace=False)
    hi = rng.integers(0, I, h)
    with torch.no_grad():  # every other held-out item one of the user's better items
        for s in range(0, h, n):
            _, lst = E.topk_fused(ue, ie, hu[s:s + n], ev._rowptr, ev._items, k)
            lst = lst.cpu().numpy()
            hi[s:s + n:2] = lst[::2, (s // n) % k]
    val = pd.DataFrame({"user_idx": hu, "item_idx": hi})
    train = pd.DataFrame({"user_idx": tu, "item_idx": ti})
    model = Tables(ue, ie)
    new = ev.evaluate(model, None, val, ks=(k,))
    old = E.evaluate(model, val, train, None, k, dev)
    assert (new[f"recall@{k}"], new[f"ndcg@{k}"]) == old, (new, old)
    t_new, t_old = [], []
    for _ in range(args.pass_reps):
        t_new.append(wall_ms(lambda: ev.evaluate(model, None, val, ks=(1, 5, 10, k, 50, 100)))[0])
        t_old.append(wall_ms(lambda: E.evaluate(model, val, train, None, k, dev))[0])
    new_ms, old_ms = float(np.median(t_new)), float(np.median(t_old))
    bench.log(f"[eval_rank_bench] Evaluator.evaluate {new_ms:.1f} ms, evaluate.evaluate "
              f"{old_ms:.1f} ms over {h} held-out users")

    flops = 2.0 * n * I * d
    result = {
        "config": cfg["name"], "users": n, "items": I, "d": d, "k": k, "splits": splits,
        "train_pairs": int(ev._rowptr[-1].item()), "reps": args.reps,
        "kernel_ms": {"lgcn_score_rank": round(rank_ms, 3), "lgcn_score_topk": round(topk_ms, 3),
                      "rank_over_topk": round(rank_ms / topk_ms, 3),
                      "rank_all": [round(x, 3) for x in t_rank],
                      "topk_all": [round(x, 3) for x in t_topk]},
        "rank_tflops": round(flops / (rank_ms / 1e3) / 1e12, 1),
        "topk_tflops": round(flops / (topk_ms / 1e3) / 1e12, 1),
        "mfma_f32_peak_tflops": 157.3,
        "listed_targets_frac": round(float(listed.float().mean().item()), 4),
        "pass": {"heldout_users": h, "batch_size": 8192, "pass_reps": args.pass_reps,
                 "evaluator_evaluate_ms": round(new_ms, 1), "evaluate_evaluate_ms": round(old_ms, 1),
                 "evaluator_all": [round(x, 1) for x in t_new],
                 "evaluate_all": [round(x, 1) for x in t_old],
                 "evaluator_ks": [1, 5, 10, k, 50, 100], "evaluate_k": k,
                 f"recall@{k}": old[0], f"ndcg@{k}": old[1], "same_metrics": True},
        "evaluator_build_s": round(build_s, 2),
        "what": ("kernel_ms: one call each between events on one stream, alternating, median of "
                 "reps, same batch / tables / mask / splits; pass: wall clock around a device "
                 "synchronise, alternating, median of pass_reps, the propagation (common to both) "
                 "left out; flops = 2 x users x items x d over the call's time"),
    }
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
