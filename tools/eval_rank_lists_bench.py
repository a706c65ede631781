#!/usr/bin/env python
"""Time the list rank evaluation (lgcn_score_rank_lists: all of a user's held-out items from one
pass over its score row) against lgcn_score_rank on the pairs the lists expand to, in one process,
at the evaluation shape bench.py times (C3: 8192 user slots x the 4.4M-item table, d = 64, the
train mask of bench.py's power-law interactions).

For T in --targets (1, 10, 50 per user) and two target distributions:

  * uniform: every target drawn uniformly over the items. The worst target of a list of T sits
    near place items x T / (T + 1), so nearly every score beats it and is placed by the binary
    search: the bad case for the one-compare reject;
  * head: every target drawn from the user's first 1 % of places (among --sample items ranked per
    user: one item in a hundred of the sample, so about one in a hundred of the table).

Each setting runs one lgcn_score_rank_lists call (four launches) and one lgcn_score_rank call on
the 8192 x T expanded (user, item) pairs (three launches; T times the user tiles), each with the
split count lgcn_eval_splits gives its batch, between events on the current stream, alternating,
median of --reps after one warm-up call each; outputs and scratch are allocated beforehand. Before
a time is printed the two rank arrays and the two score arrays must be equal, bit for bit.

The tables are seeded N(0, 0.1) draws of the C3 shape, as tools/eval_rank_bench.py's.

Prints one progress line per setting on stderr and one JSON line on stdout.

    timeout -k 10 840 python tools/eval_rank_lists_bench.py [--targets 1 10 50] [--reps 9]

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


def event_ms(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e)


def draw_targets(dist, ue, ie, users, T, sample, g):
    """int32 [n x T] targets per slot on the device."""
    n, I = int(users.numel()), ie.shape[0]
    if dist == "uniform":
        return torch.randint(0, I, (n, T), generator=g, device=ie.device, dtype=torch.int32)
    cand = torch.randint(0, I, (sample,), generator=g, device=ie.device)
    head = max(sample // 100, 1)
    out = torch.empty((n, T), dtype=torch.int32, device=ie.device)
    for s in range(0, n, 1024):  # the first 1 % of the sample per user, T of them at random
        scores = ue[users[s:s + 1024].long()] @ ie[cand].T
        first = torch.topk(scores, head, dim=1)[1]
        pick = torch.randint(0, head, (first.shape[0], T), generator=g, device=ie.device)
        out[s:s + 1024] = cand[first.gather(1, pick)].int()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 10, 50])
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_rank_lists_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = engine.load_library()
    cfg = bench.CONFIGS[args.config]
    U, I, n_inter, d = cfg["users"], cfg["items"], cfg["interactions"], cfg["d"]
    t0 = time.perf_counter()
    tu, ti = graph.powerlaw_interactions(U, I, n_inter, cfg["seed"])
    ev = E.Evaluator(tu, ti, U, I, dev)
    torch.cuda.synchronize()
    bench.log(f"[eval_rank_lists_bench] {n_inter:,} interactions, mask resident in "
              f"{time.perf_counter() - t0:.1f}s")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ue = torch.randn((U, d), generator=g, device=dev) * 0.1
    ie = torch.randn((I, d), generator=g, device=dev) * 0.1
    rng = np.random.default_rng(7)
    n = min(args.users, U)
    users = torch.from_numpy(np.sort(rng.choice(U, n, replace=False)).astype(np.int32)).to(dev)
    cus = E._device_cus(dev)
    P, stream = engine._ptr, engine._stream(dev)
    mrow, mit = ev._rowptr, ev._items
    lines = []
    for T in args.targets:
        rowptr = (torch.arange(n + 1, device=dev, dtype=torch.int32) * T).contiguous()
        pair_users = users.repeat_interleave(T).contiguous()
        s_lists = lib.lgcn_eval_splits(n, I, cus)
        s_pairs = lib.lgcn_eval_splits(n * T, I, cus)
        scratch = E._lists_scratch(n, n * T, s_lists, dev)
        part = torch.empty(s_pairs * n * T, dtype=torch.int32, device=dev)
        out = {name: (torch.empty(n * T, dtype=torch.int32, device=dev),
                      torch.empty(n * T, dtype=torch.float32, device=dev))
               for name in ("lists", "pairs")}
        for dist in ("uniform", "head"):
            items = draw_targets(dist, ue, ie, users, T, args.sample, g).reshape(-1).contiguous()

            def lists():
                rank, score = out["lists"]
                engine._check(lib.lgcn_score_rank_lists(
                    P(ue), ue.stride(0), P(users), n, P(ie), ie.stride(0), I, d, P(mrow), P(mit),
                    P(rowptr), P(items), s_lists, P(scratch), int(scratch.numel()), P(score),
                    P(rank), stream), "lgcn_score_rank_lists")

            def pairs():
                rank, score = out["pairs"]
                engine._check(lib.lgcn_score_rank(
                    P(ue), ue.stride(0), P(pair_users), n * T, P(ie), ie.stride(0), I, d, P(mrow),
                    P(mit), P(items), s_pairs, P(part), P(score), P(rank), stream),
                    "lgcn_score_rank")

            for o in out.values():
                o[0].fill_(-7)
                o[1].fill_(12345.0)
            lists()
            pairs()
            torch.cuda.synchronize()
            assert torch.equal(out["lists"][0], out["pairs"][0]), f"T={T} {dist}: ranks differ"
            assert torch.equal(out["lists"][1].view(torch.int32),
                               out["pairs"][1].view(torch.int32)), f"T={T} {dist}: scores differ"
            t_lists, t_pairs = [], []
            for _ in range(args.reps):  # alternating: both see the same machine state
                t_lists.append(event_ms(lists))
                t_pairs.append(event_ms(pairs))
            ms_l, ms_p = float(np.median(t_lists)), float(np.median(t_pairs))
            worst = out["lists"][0].view(n, T).max(1)[0].float().mean().item()
            line = {"T": T, "targets": dist, "lists_ms": round(ms_l, 3), "pairs_ms": round(ms_p, 3),
                    "lists_over_pairs": round(ms_l / ms_p, 4), "splits_lists": s_lists,
                    "splits_pairs": s_pairs, "mean_worst_rank": round(worst, 1),
                    "lists_all": [round(x, 3) for x in t_lists],
                    "pairs_all": [round(x, 3) for x in t_pairs]}
            lines.append(line)
            bench.log(f"[eval_rank_lists_bench] T={T:3d} {dist:7s}: lgcn_score_rank_lists "
                      f"{ms_l:9.2f} ms, lgcn_score_rank on {n * T} pairs {ms_p:9.2f} ms, "
                      f"ratio {ms_l / ms_p:.3f} (ranks and scores bit-equal; mean worst rank "
                      f"{worst:,.0f})")
    print(json.dumps({
        "config": cfg["name"], "users": n, "items": I, "d": d, "reps": args.reps,
        "head_sample": args.sample, "settings": lines,
        "what": ("one call each between events on one stream after one warm-up call each, "
                 "alternating, medians of reps; same tables / mask; each call with the split "
                 "count lgcn_eval_splits gives its batch; rank and target_score compared as raw "
                 "bits before timing")}), flush=True)


if __name__ == "__main__":
    main()
