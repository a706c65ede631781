#!/usr/bin/env python
"""Time the BPR sampler three ways in one process, on bench.py's C3 interactions (power-law,
29.5M samples):

  * device: one whole-epoch BprSampler.draw (one lgcn_bpr_sample launch) between events on the
    current stream, median of --reps, for the identity order and for epoch()'s shuffled order
    (the permutation made beforehand; torch.randperm is timed on its own);
  * cpu: the same draw on the numpy path (one whole epoch, wall clock);
  * python_loop: what BPRDataset.__getitem__ does per sample — look up the user's item set, draw
    random.randint until the item is not in it — as a plain Python loop over the first --subset
    interactions, extrapolated to the epoch (the DataLoader, collation and the per-batch upload
    it sits behind are not counted).

The first --check slots of the device draw are compared with the numpy path (same bits). Prints
one JSON line on stdout (progress goes to stderr); `vs_parent_step` states the whole-epoch draw
against one training step of the commit before the sampler (profiles/bpr_step_c3.log).

    timeout -k 10 840 python tools/sampler_bench.py [--config c3] [--reps 7] [--subset 200000]

--n-neg M [M ...] times only the device draw with M negatives per sample (lgcn_bpr_sample_multi,
shuffled order) beside the one-negative draw, the variants interleaved rep by rep, and compares
the first slots of each with the numpy path.

--weighted [--alpha A] [--n-neg M ...] times only the device draw of a sampler built with
weights="popularity" (lgcn_bpr_sample_weighted, count^A weights) beside the uniform sampler's, with
one negative and with each M (default 16), shuffled order, the variants interleaved rep by rep, and
compares the first slots of each weighted draw with the numpy twin.

One process, so the three figures come from one machine in one run; it holds the GPU for the
whole of it and is therefore started under a time limit of its own, as every GPU step is.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, log: the shapes bench.py times)
from gcn_recommendation_amd import engine, graph, sampler  # noqa: E402
from gcn_recommendation_amd.evaluate import mask_csr  # noqa: E402

PARENT_STEP_MS = 38.947  # profiles/bpr_step_c3.log: step_ms_adam_default.bpr_step


def device_ms(fn, reps):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(e))
    return out


def python_loop(users, items, rowptr, pos_items, n_items, subset):
    """The reference's per-sample work, written out: returns seconds per sample."""
    sub_u = users[:subset].tolist()
    sub_i = items[:subset].tolist()
    sets = {u: set(pos_items[rowptr[u]:rowptr[u + 1]].tolist()) for u in set(sub_u)}
    rnd = random.Random(0)
    hi = n_items - 1
    out = [None] * len(sub_u)
    t0 = time.perf_counter()
    for k in range(len(sub_u)):
        u = sub_u[k]
        seen = sets[u]
        neg = rnd.randint(0, hi)
        while neg in seen:
            neg = rnd.randint(0, hi)
        out[k] = (u, sub_i[k], neg)
    return (time.perf_counter() - t0) / max(len(sub_u), 1)


def multi_neg(args, s, users, items, U, I, E, epoch, cfg):
    """--n-neg: the whole-epoch shuffled device draw at each M (lgcn_bpr_sample_multi) and with
    one negative (lgcn_bpr_sample), the variants interleaved rep by rep; the first --check slots
    of every M are compared with the numpy path."""
    perm = s.permutation(epoch)
    variants = [None] + list(args.n_neg)
    check = min(args.check, E, 100_000)
    order = perm[:check].cpu().numpy()
    c = sampler.BprSampler(users, items, U, I, "cpu", seed=args.seed)
    for M in variants:   # warm-up and the comparison
        got = s.draw(epoch, perm, n_neg=M)[2][:check].cpu().numpy()
        want = sampler.sample_numpy(c._user, c._item, order, 0, check, c._rowptr, c._pos_items, U,
                                    I, args.seed, epoch, n_neg=M)[2]
        assert np.array_equal(got, want), f"device draw differs from the numpy path at n_neg={M}"
        del got
    times = {M: [] for M in variants}
    for _ in range(args.reps):
        for M in variants:
            times[M] += device_ms(lambda: s.draw(epoch, perm, n_neg=M), 1)
    med = {M: float(np.median(v)) for M, v in times.items()}
    result = {
        "config": cfg["name"], "interactions": E, "users": U, "items": I, "reps": args.reps,
        "device_draw_ms_shuffled": {"one_negative" if M is None else f"n_neg_{M}": round(v, 3)
                                    for M, v in med.items()},
        "device_draw_ms_all": {"one_negative" if M is None else f"n_neg_{M}":
                               [round(x, 3) for x in v] for M, v in times.items()},
        "draw_bytes": {f"n_neg_{M}": E * (2 + M) * 8 for M in args.n_neg},
        "device_equals_numpy_first_slots": check,
        "what": ("one whole-epoch BprSampler.draw(order=randperm, n_neg=M) between events, the "
                 "variants interleaved rep by rep, median of reps; the output allocation "
                 "(torch.empty) is inside the timed region, as in a training epoch"),
    }
    print(json.dumps(result), flush=True)


def weighted(args, s, users, items, U, I, E, epoch, cfg):
    """--weighted: the whole-epoch shuffled device draw of the uniform sampler and of one built
    with weights="popularity", with one negative and with each M of --n-neg, the variants
    interleaved rep by rep; the first --check slots of every weighted draw are compared with the
    numpy twin."""
    t0 = time.perf_counter()
    sw = sampler.BprSampler(users, items, U, I, s.device, seed=args.seed, weights="popularity",
                            alpha=args.alpha)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    perm = s.permutation(epoch)
    variants = [(kind, M) for M in [None] + list(args.n_neg or [16])
                for kind in ("uniform", "weighted")]
    check = min(args.check, E, 100_000)
    order = perm[:check].cpu().numpy()
    c = sampler.BprSampler(users, items, U, I, "cpu", seed=args.seed, weights=sw.item_weights)
    unsampled = {}
    for kind, M in variants:   # warm-up and the comparison
        smp = sw if kind == "weighted" else s
        got = smp.draw(epoch, perm, n_neg=M)[2][:check].cpu().numpy()
        unsampled[kind] = int(smp.unsampled.item())
        if kind == "weighted":
            want = sampler.sample_numpy(c._user, c._item, order, 0, check, c._rowptr, c._pos_items,
                                        U, I, args.seed, epoch, n_neg=M, cumw=c._cumw)[2]
            assert np.array_equal(got, want), f"weighted draw differs from numpy at n_neg={M}"
        del got
    times = {v: [] for v in variants}
    for _ in range(args.reps):
        for kind, M in variants:
            smp = sw if kind == "weighted" else s
            times[(kind, M)] += device_ms(lambda: smp.draw(epoch, perm, n_neg=M), 1)

    def key(kind, M):
        return f"{kind}_" + ("one_negative" if M is None else f"n_neg_{M}")

    w = sw.item_weights
    result = {
        "config": cfg["name"], "interactions": E, "users": U, "items": I, "reps": args.reps,
        "alpha": args.alpha, "weighted_sampler_build_s": round(build_s, 2),
        "weights": {"zero": int((w == 0).sum()), "one": int((w == 1).sum()), "total": int(w.sum()),
                    "table_bytes": int((I + 1) * 8 + sw._cumw[0].numel() * 8)},
        "unsampled": unsampled,
        "device_draw_ms_shuffled": {key(*v): round(float(np.median(t)), 3)
                                    for v, t in times.items()},
        "device_draw_ms_all": {key(*v): [round(x, 3) for x in t] for v, t in times.items()},
        "weighted_equals_numpy_first_slots": check,
        "what": ("one whole-epoch BprSampler.draw(order=randperm, n_neg=M) between events, uniform "
                 "and weights='popularity' samplers and every M interleaved rep by rep, median of "
                 "reps; the output allocation (torch.empty) is inside the timed region"),
    }
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--subset", type=int, default=200_000)
    ap.add_argument("--check", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n-neg", type=int, nargs="+", default=None, metavar="M",
                    help="time only the device draw with M negatives per sample (several values: "
                         "interleaved), one negative beside them")
    ap.add_argument("--weighted", action="store_true",
                    help="time only the device draw of a weights='popularity' sampler beside the "
                         "uniform one, with one negative and with each M of --n-neg (default 16)")
    ap.add_argument("--alpha", type=float, default=0.75, help="exponent of --weighted's counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampler_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    engine.load_library()
    cfg = bench.CONFIGS[args.config]
    U, I, E = cfg["users"], cfg["items"], cfg["interactions"]
    t0 = time.perf_counter()
    users, items = graph.powerlaw_interactions(U, I, E, cfg["seed"])
    bench.log(f"[sampler_bench] {E:,} interactions in {time.perf_counter() - t0:.1f}s")

    t0 = time.perf_counter()
    s = sampler.BprSampler(users, items, U, I, dev, seed=args.seed)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    bench.log(f"[sampler_bench] device sampler built in {build_s:.1f}s")
    epoch = 1
    if args.weighted:
        weighted(args, s, users, items, U, I, E, epoch, cfg)
        return
    if args.n_neg:
        multi_neg(args, s, users, items, U, I, E, epoch, cfg)
        return
    s.draw(epoch)  # warm-up
    perm = s.permutation(epoch)
    s.draw(epoch, perm)
    ident = device_ms(lambda: s.draw(epoch), args.reps)
    shuf = device_ms(lambda: s.draw(epoch, perm), args.reps)
    rperm = device_ms(lambda: s.permutation(epoch), args.reps)
    got = [t[:args.check].cpu().numpy() for t in s.draw(epoch, perm)]
    unsampled = int(s.unsampled.item())
    bench.log(f"[sampler_bench] device draw {np.median(ident):.3f} ms identity, "
              f"{np.median(shuf):.3f} ms shuffled")

    c = sampler.BprSampler(users, items, U, I, "cpu", seed=args.seed)
    t0 = time.perf_counter()
    cu, cp, cn = c.draw(epoch)
    cpu_s = time.perf_counter() - t0
    bench.log(f"[sampler_bench] numpy draw {cpu_s:.2f}s")
    order = perm[:args.check].cpu()
    same = all(np.array_equal(g, w[order].numpy()) for g, w in zip(got, (cu, cp, cn)))
    assert same, "device draw differs from the numpy path"
    del cu, cp, cn

    rowptr, pos_items = mask_csr(users, items, U)
    per_sample = python_loop(users, items, rowptr, pos_items, I, min(args.subset, E))
    bench.log(f"[sampler_bench] python loop {per_sample * 1e6:.3f} us per sample")

    draw_ms = float(np.median(shuf))
    result = {
        "config": cfg["name"], "interactions": E, "users": U, "items": I,
        "positives": int(pos_items.shape[0]), "unsampled": unsampled, "reps": args.reps,
        "device_draw_ms": {"identity": round(float(np.median(ident)), 3),
                           "shuffled": round(draw_ms, 3),
                           "identity_all": [round(x, 3) for x in ident],
                           "shuffled_all": [round(x, 3) for x in shuf]},
        "device_randperm_ms": round(float(np.median(rperm)), 3),
        "device_ns_per_sample": round(draw_ms * 1e6 / E, 3),
        "sampler_build_s": round(build_s, 2),
        "cpu_numpy_draw_s": round(cpu_s, 3),
        "python_loop": {"subset": min(args.subset, E), "us_per_sample": round(per_sample * 1e6, 3),
                        "epoch_s_extrapolated": round(per_sample * E, 1)},
        "device_equals_numpy_first_slots": args.check,
        "vs_parent_step": {"parent_step_ms": PARENT_STEP_MS,
                           "epoch_draw_plus_randperm_ms": round(draw_ms + float(np.median(rperm)),
                                                                3),
                           "draw_below_one_step": bool(draw_ms < PARENT_STEP_MS)},
        "what": ("one whole-epoch BprSampler.draw between events (median of reps; shuffled = "
                 "order from torch.randperm, made beforehand and timed on its own); "
                 "cpu_numpy_draw_s = the same draw on the numpy path, wall clock; python_loop = "
                 "set lookup + random.randint until not in the set, per sample, on a subset, "
                 "extrapolated to the epoch"),
    }
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
