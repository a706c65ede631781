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

With --against PATH (another build of the library with the same ABI, such as the parent commit's
under gcn_recommendation_amd/_variants/) the tool compares the two builds instead of the two
passes: both are loaded into this process and run lgcn_score_topk and lgcn_score_rank on the same
batch, tables, mask and split count, each into outputs of its own. First top_scores, top_idx, rank
and target_score of the two builds must be equal as raw bits, here and on the Gaussian tables of
tests/test_gpu_eval.py at d = 32, 128, 256 (a reordered score chain shows nowhere else); then the
four calls are timed between events, PATH's and the tree's alternating, and for each entry point
the tree's median may exceed PATH's by no more than PATH's own interquartile range.

Prints one JSON line on stdout (progress goes to stderr).

    timeout -k 10 840 python tools/eval_rank_bench.py [--config c3] [--reps 9] [--heldout 65536]
    timeout -k 10 600 python tools/eval_rank_bench.py --against PATH [--reps 9]

One process, so every figure comes from one machine in one run; it holds the GPU for the whole of
it and is therefore started under a time limit of its own, as every GPU step is.
"""
import argparse
import ctypes
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


class Calls:
    """lgcn_score_topk (k) and lgcn_score_rank of one build of the library on shared inputs, with
    outputs and scratch of its own."""

    def __init__(self, lib, ue, ie, users, mrow, mit, k, splits):
        dev, n = ie.device, int(users.numel())
        self.lib, self.inputs, self.k, self.splits = lib, (ue, ie, users, mrow, mit), k, splits
        self.part_s = torch.empty((splits, n, k), dtype=torch.float32, device=dev)
        self.part_i = torch.empty((splits, n, k), dtype=torch.int32, device=dev)
        self.top_s = torch.empty((n, k), dtype=torch.float32, device=dev)
        self.top_i = torch.empty((n, k), dtype=torch.int32, device=dev)
        self.part = torch.empty(splits * n, dtype=torch.int32, device=dev)
        self.rank_out = torch.empty(n, dtype=torch.int32, device=dev)
        self.score = torch.empty(n, dtype=torch.float32, device=dev)
        self.targets = None

    def topk(self):
        ue, ie, users, mrow, mit = self.inputs
        P = engine._ptr
        engine._check(self.lib.lgcn_score_topk(
            P(ue), ue.stride(0), P(users), int(users.numel()), P(ie), ie.stride(0), ie.shape[0],
            ie.shape[1], P(mrow), P(mit), self.k, self.splits, P(self.part_s), P(self.part_i),
            P(self.top_s), P(self.top_i), engine._stream(ie.device)), "lgcn_score_topk")

    def rank(self):
        ue, ie, users, mrow, mit = self.inputs
        P = engine._ptr
        engine._check(self.lib.lgcn_score_rank(
            P(ue), ue.stride(0), P(users), int(users.numel()), P(ie), ie.stride(0), ie.shape[0],
            ie.shape[1], P(mrow), P(mit), P(self.targets), self.splits, P(self.part),
            P(self.score), P(self.rank_out), engine._stream(ie.device)), "lgcn_score_rank")

    def outputs(self):
        return {"top_scores": self.top_s, "top_idx": self.top_i, "rank": self.rank_out,
                "target_score": self.score}


def load_build(path):
    """Another build of the library beside the tree's, bound to the same ABI."""
    lib = ctypes.CDLL(path)
    for name, res, argtypes in engine.ABI:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, argtypes
    if lib.lgcn_abi_version() != engine.ABI_VERSION:
        sys.exit(f"eval_rank_bench: {path} has another ABI version")
    return lib


def same_bits(tree, other, what):
    """Both builds' calls on their shared inputs (the targets: every other slot an item of the
    tree's list): the four outputs equal as raw bits."""
    tree.topk()
    n, k = tree.top_i.shape
    g = torch.Generator(device=tree.top_i.device)
    g.manual_seed(11)
    items = tree.inputs[1].shape[0]
    targets = torch.randint(0, items, (n,), generator=g, device=tree.top_i.device,
                            dtype=torch.int32)
    place = torch.randint(0, k, (n, 1), generator=g, device=tree.top_i.device)
    targets[::2] = tree.top_i.gather(1, place)[::2, 0]
    tree.targets = other.targets = targets
    for c in (other, tree):
        c.topk()
        c.rank()
    torch.cuda.synchronize()
    for name, t in tree.outputs().items():
        o = other.outputs()[name]
        assert torch.equal(t.view(torch.int32), o.view(torch.int32)), f"{what}: {name} differs"
    bench.log(f"[eval_rank_bench] {what}: top_scores, top_idx, rank, target_score bit-equal")


def gaussian_bits(lib, other, dev, k):
    """same_bits on the tables of tests/test_gpu_eval.py's Gaussian case (300 users x 4000 items),
    the widths C3 does not have."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_eval import _gauss_case
    checked = []
    for d in (32, 128, 256):
        ue, ie, users, mrow, mit = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                    for a in _gauss_case(d)[:5])
        for splits in (1, 4):
            args = (ue, ie, users.int(), mrow, mit, k, splits)
            same_bits(Calls(lib, *args), Calls(other, *args), f"gaussian d={d} splits={splits}")
            checked.append([d, splits])
    return checked


def against(args, config, tree):
    """The --against comparison on the batch of `tree` (the tree's build): the result line."""
    ie, users = tree.inputs[1:3]
    other_lib = load_build(args.against)
    other = Calls(other_lib, *tree.inputs, tree.k, tree.splits)
    same_bits(tree, other, f"{config} d={ie.shape[1]}")
    times = {"topk": ([], []), "rank": ([], [])}  # (PATH's, the tree's)
    for _ in range(args.reps):  # alternating: both builds see the same machine state
        for name in times:
            for c, t in zip((other, tree), times[name]):
                t.append(event_ms(getattr(c, name)))
    result = {"config": config, "users": int(users.numel()), "items": ie.shape[0],
              "d": ie.shape[1], "k": tree.k, "splits": tree.splits,
              "against": os.path.relpath(args.against, ROOT), "reps": args.reps,
              "bit_equal": {args.config: True, "gaussian_d_splits":
                            gaussian_bits(tree.lib, other_lib, ie.device, tree.k)}}
    for name, (t_other, t_tree) in times.items():
        lo, med, hi = (float(q) for q in np.percentile(t_other, [25, 50, 75]))
        new_med = float(np.median(t_tree))
        result[f"lgcn_score_{name}"] = {
            "against_ms": round(med, 3), "tree_ms": round(new_med, 3),
            "against_iqr_ms": round(hi - lo, 3), "within_against_iqr": new_med - med <= hi - lo,
            "against_all": [round(x, 3) for x in t_other],
            "tree_all": [round(x, 3) for x in t_tree]}
        bench.log(f"[eval_rank_bench] lgcn_score_{name}: {med:.2f} ms against, {new_med:.2f} ms "
                  f"tree, spread (IQR) of the former {hi - lo:.2f} ms")
    result["what"] = ("one call each between events on one stream after one warm-up call each, "
                      "PATH's build and the tree's alternating, medians of reps; same batch / "
                      "tables / mask / splits; outputs compared as raw bits before timing")
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--heldout", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pass-reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--against", metavar="PATH", help="compare with this build of the library")
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
    tree = Calls(lib, ue, ie, users, ev._rowptr, ev._items, k, splits)
    if args.against:
        print(json.dumps(against(args, cfg["name"], tree)), flush=True)
        return
    top_s, top_i, rank, score = tree.outputs().values()
    topk, rank_call = tree.topk, tree.rank
    topk()
    # targets: every other slot an item of its top-k list (a hit), the others anywhere
    targets = torch.from_numpy(rng.integers(0, I, n).astype(np.int32)).to(dev)
    place = torch.from_numpy(rng.integers(0, k, n)).to(dev)
    targets[::2] = top_i.gather(1, place[:, None])[::2, 0]
    tree.targets = targets
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
