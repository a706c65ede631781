#!/usr/bin/env python
"""Time the recommendation-list kernel at the evaluation shape bench.py times (C3: 8192 users x
the 4.4M-item table, d = 64, the train mask of bench.py's power-law interactions), in one process:

  * lgcn_score_topk_wide at k = 20, 100 and 1000: one call (two launches) between events on the
    current stream, median of --reps; outputs and scratch allocated beforehand, the split count
    lgcn_topk_wide_splits';
  * lgcn_score_topk at k = 20 alternating with the wide kernel at k = 20 (the wide kernel keeps
    its candidates in scratch, not in LDS: the ratio is reported, not gated);
  * the torch route, evaluate.topk_total_order_torch (matmul, mask, stable sort: what there is
    for k > 32 without the kernel), at k = 100 and 1000 over the same 8192 users in 1024-user
    chunks, between events, median of --torch-reps.

The tables are seeded N(0, 0.1) draws of the C3 shape. Checked before timing, for every k: for 64
sampled slots lgcn_score_rank of every listed item is its place in the list and its target_score
the listed score, as raw bits (k distinct items with ranks 0..k-1 are the top k).

Prints one JSON line on stdout (progress goes to stderr).

    timeout -k 10 900 python tools/recommend_bench.py [--config c3] [--reps 9] [--torch-reps 3]

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
from tools.eval_rank_bench import Calls, event_ms  # noqa: E402

KS = (20, 100, 1000)
TORCH_KS = (100, 1000)
CHECK_SLOTS = 64


class Wide:
    """lgcn_score_topk_wide at one k on shared inputs, with outputs and scratch of its own."""

    def __init__(self, lib, ue, ie, users, mrow, mit, k, splits):
        dev, n = ie.device, int(users.numel())
        self.lib, self.inputs, self.k, self.splits = lib, (ue, ie, users, mrow, mit), k, splits
        self.scratch = torch.empty(lib.lgcn_score_topk_wide_scratch_bytes(n, k, splits),
                                   dtype=torch.uint8, device=dev)
        self.top_s = torch.empty((n, k), dtype=torch.float32, device=dev)
        self.top_i = torch.empty((n, k), dtype=torch.int32, device=dev)

    def __call__(self):
        E._wide_launch(*self.inputs, self.k, self.splits, self.scratch, self.top_s, self.top_i)


def check_lists(lib, wide, slots):
    """Every listed item of the sampled slots ranks at its place with the listed score."""
    ue, ie, users, mrow, mit = wide.inputs
    k = wide.k
    items = wide.top_i[slots].reshape(-1).contiguous()
    assert bool((items >= 0).all()), "a list of the sample is not full"
    pair_users = users[slots].repeat_interleave(k).contiguous()
    n = int(items.numel())
    splits = lib.lgcn_eval_splits(n, ie.shape[0], E._device_cus(ie.device))
    rank = torch.empty(n, dtype=torch.int32, device=ie.device)
    score = torch.empty(n, dtype=torch.float32, device=ie.device)
    part = torch.empty(splits * n, dtype=torch.int32, device=ie.device)
    E._rank_launch(ue, ie, pair_users, items, mrow, mit, rank, score, part, splits)
    torch.cuda.synchronize()
    place = torch.arange(k, dtype=torch.int32, device=ie.device).repeat(len(slots))
    assert torch.equal(rank, place), f"k={k}: a listed item's rank is not its place"
    assert torch.equal(score.view(torch.int32), wide.top_s[slots].reshape(-1).view(torch.int32)), \
        f"k={k}: a listed score is not lgcn_score_rank's target_score"


def quartiles(t):
    lo, med, hi = (float(q) for q in np.percentile(t, [25, 50, 75]))
    return {"ms": round(med, 3), "iqr_ms": round(hi - lo, 3), "all": [round(x, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--torch-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("recommend_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = engine.load_library()
    cfg = bench.CONFIGS[args.config]
    U, I, n_inter, d = cfg["users"], cfg["items"], cfg["interactions"], cfg["d"]
    t0 = time.perf_counter()
    tu, ti = graph.powerlaw_interactions(U, I, n_inter, cfg["seed"])
    ev = E.Evaluator(tu, ti, U, I, dev)
    torch.cuda.synchronize()
    bench.log(f"[recommend_bench] {n_inter:,} interactions, mask resident in "
              f"{time.perf_counter() - t0:.1f}s")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ue = torch.randn((U, d), generator=g, device=dev) * 0.1
    ie = torch.randn((I, d), generator=g, device=dev) * 0.1
    rng = np.random.default_rng(7)
    n = min(args.users, U)
    users = torch.from_numpy(np.sort(rng.choice(U, n, replace=False)).astype(np.int32)).to(dev)
    slots = torch.from_numpy(np.sort(rng.choice(n, min(CHECK_SLOTS, n), replace=False))).to(dev)
    cus = E._device_cus(dev)

    result = {"config": cfg["name"], "users": n, "items": I, "d": d, "reps": args.reps,
              "torch_reps": args.torch_reps, "train_pairs": int(ev._rowptr[-1].item()),
              "checked_slots": int(slots.numel()), "wide": {}, "torch_route": {}}
    wides = {}
    for k in KS:
        splits = lib.lgcn_topk_wide_splits(n, I, k, cus)
        w = wides[k] = Wide(lib, ue, ie, users, ev._rowptr, ev._items, k, splits)
        w()  # warm-up, and the lists the check reads
        check_lists(lib, w, slots)
        bench.log(f"[recommend_bench] k={k}: {int(slots.numel())} x {k} listed items rank at their "
                  f"places, scores bit-equal")
    for k in KS:
        t = [event_ms(wides[k]) for _ in range(args.reps)]
        result["wide"][str(k)] = dict(quartiles(t), splits=wides[k].splits,
                                      scratch_mb=round(wides[k].scratch.numel() / 2 ** 20, 1))
        bench.log(f"[recommend_bench] lgcn_score_topk_wide k={k}: {np.median(t):.2f} ms, "
                  f"{wides[k].splits} splits")

    # ---- k = 20: the LDS kernel and the wide kernel, alternating --------------------------------
    narrow = Calls(lib, ue, ie, users, ev._rowptr, ev._items, 20,
                   lib.lgcn_eval_splits(n, I, cus))
    narrow.topk()
    torch.cuda.synchronize()
    assert torch.equal(narrow.top_i, wides[20].top_i) and torch.equal(
        narrow.top_s.view(torch.int32), wides[20].top_s.view(torch.int32)), \
        "k=20: the wide lists are not lgcn_score_topk's"
    t_narrow, t_wide = [], []
    for _ in range(args.reps):
        t_narrow.append(event_ms(narrow.topk))
        t_wide.append(event_ms(wides[20]))
    result["k20"] = {"lgcn_score_topk": quartiles(t_narrow), "lgcn_score_topk_wide":
                     quartiles(t_wide), "bit_equal": True,
                     "wide_over_topk": round(float(np.median(t_wide) / np.median(t_narrow)), 3)}
    bench.log(f"[recommend_bench] k=20: lgcn_score_topk {np.median(t_narrow):.2f} ms, wide "
              f"{np.median(t_wide):.2f} ms")

    # ---- the torch route over the same users ---------------------------------------------------
    for k in TORCH_KS:
        def route():
            return E.topk_total_order_torch(ue, ie, users, ev._rowptr, ev._items, k, 1024)
        route()  # warm-up (the allocator's blocks, hipBLASLt's choice)
        t = [event_ms(route) for _ in range(args.torch_reps)]
        q = quartiles(t)
        wide = result["wide"][str(k)]
        q["wide_faster_by_ms"] = round(q["ms"] - wide["ms"], 3)
        q["faster_by_more_than_both_iqr"] = q["ms"] - wide["ms"] > q["iqr_ms"] + wide["iqr_ms"]
        result["torch_route"][str(k)] = q
        bench.log(f"[recommend_bench] torch route k={k}: {q['ms']:.1f} ms over {n} users")
        torch.cuda.empty_cache()
    result["what"] = ("wide / k20: one call between events on one stream after a warm-up call, "
                      "median and interquartile range of reps (k20 alternating); torch_route: "
                      "evaluate.topk_total_order_torch over the same users in 1024-user chunks, "
                      "median of torch_reps; lists checked against lgcn_score_rank before timing")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
