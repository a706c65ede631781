"""Benchmark of the LightGCN propagation hot path on MI355X (BASELINE.json metric:
"propagated edges/sec (SpMM) + Recall@20, Amazon-Books 3-layer d=64 at 1/2/4/8 GPU").

One step = one full K-layer propagation + fused layer mean (models/lightgcn.py:40-54) over the
whole synthetic graph, inputs resident in HBM, CSR plan already built (it is cached per
adjacency, main.py:495 passes the same tensor every batch). Edges/s = K * nnz(Â) / t_step.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c3|c2] [--gen powerlaw|uniform]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line. --dump-outputs DIR
also writes the last timed step's output (a seeded row sample of it) as DIR/*.npy; the inputs are
seeded, so two builds can be compared output for output. --full adds everything else to the
line: roofline and per-kernel timing, the device adjacency builder, C4 on the same graph,
backward, evaluation, the training step, the CPU baseline with parity, chunk mode and the
trained Recall@20 (minutes of CPU and GPU work).

N > 1 (launched by torch.distributed.run, one rank per GPU): the adjacency is row-partitioned by
nnz, each rank owns a slice of rows, and every layer all-gathers the embedding slices over RCCL
(gcn_recommendation_amd.dist). Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

# The bipartite two-lane schedule runs 8 streams (lgcn_sched_create: the caller's + 7). HIP keeps
# GPU_MAX_HW_QUEUES hardware queues (default 4) per stream priority, and the second lane's four
# streams are high priority: every stream gets a queue under the default, which is what
# main.py runs with (round 4: 17.08 ms at 4 queues vs 17.17 ms at 8). The environment is left
# alone; LGCN_HW_QUEUES=N sets GPU_MAX_HW_QUEUES for an A/B.
# Under torch.distributed (N > 1, or --force-dist) RCCL's communicator holds streams of its own,
# which then share HIP's hardware queues with the two lanes' streams: world-1 featsplit over
# RCCL 15.8 / 16.3 ms at GPU_MAX_HW_QUEUES = 4 / 8 vs 13.2 ms over gloo, 13.1 ms over RCCL at
# 16. There the process raises it to 16 per priority before the GPU is touched (an environment
# that already asks for more keeps its value).
if os.environ.get("LGCN_HW_QUEUES", ""):
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ["LGCN_HW_QUEUES"]
elif int(os.environ.get("WORLD_SIZE", "1")) > 1 or "--force-dist" in sys.argv:
    try:
        _q = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        _q = 4
    os.environ["GPU_MAX_HW_QUEUES"] = str(max(_q, 16))

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from gcn_recommendation_amd import engine, graph  # noqa: E402

PEAK_HBM_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)

CONFIGS = {
    # BASELINE.json configs[2]: full Amazon-Books 2023 shape, d=64, 3 layers, 1x MI355X
    "c3": dict(users=10_300_000, items=4_400_000, interactions=29_500_000, d=64, K=3, seed=3,
               name="C3 full Amazon-Books-2023 shape (10.3M users x 4.4M items x 29.5M interactions)"),
    # BASELINE.json configs[1]: Books subset
    "c2": dict(users=50_000, items=50_000, interactions=1_000_000, d=64, K=3, seed=2,
               name="C2 Amazon-Books subset shape (50k x 50k x 1M interactions)"),
    # BASELINE.json configs[3]: full Books, d=256, 4 layers (8-GPU config; runs on 1 GPU too)
    "c4": dict(users=10_300_000, items=4_400_000, interactions=29_500_000, d=256, K=4, seed=3,
               name="C4 full Amazon-Books-2023 shape, d=256, 4 layers"),
    # BASELINE.json configs[4]: Fusion path: Books + brand nodes (I/10, one per item) + content
    # embeddings C=64, d=128 (the LightGCN_Fusion forward: Linear+leaky_relu, then propagation)
    "c5": dict(users=10_300_000, items=4_400_000, interactions=29_500_000, d=128, K=3, seed=3,
               brands=440_000, content=64,
               name="C5 LightGCN_Fusion, Books shape + 440k brands, content C=64, d=128"),
}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def kernel_source_hash():
    """sha1 (16 hex) of the engine's kernel sources: stamps profiles/traffic_*.json."""
    import hashlib
    h = hashlib.sha1()
    for f in sorted(os.listdir(os.path.join(ROOT, "gcn_recommendation_amd", "csrc"))) + ["lgcn.h"]:
        p_ = os.path.join(ROOT, "include", f) if f == "lgcn.h" else \
            os.path.join(ROOT, "gcn_recommendation_amd", "csrc", f)
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(p_, "rb").read())
    return h.hexdigest()[:16]


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


def make_graph(cfg, gen, heldout_users, keep_interactions=False):
    t0 = time.time()
    U, I, E = cfg["users"], cfg["items"], cfg["interactions"]
    if gen == "uniform":
        u, i = graph.uniform_interactions(U, I, E, cfg["seed"])
    else:
        u, i = graph.powerlaw_interactions(U, I, E, cfg["seed"])
    B = cfg.get("brands", 0)
    ib = (np.arange(I), np.random.default_rng(cfg["seed"] + 7).integers(0, B, I)) if B else (None, None)
    t1 = time.time()
    rows, cols = graph.edge_lists(u, i, U, I, ib[0], ib[1], use_brand=bool(B))
    r, c, v = graph.normalise(rows, cols, U + I + B)
    del rows, cols
    t_norm = time.time() - t1
    # held-out items for Recall@20 parity: one random item per sampled user (not in Â)
    rng = np.random.default_rng(cfg["seed"] + 100)
    ev_users = rng.choice(U, size=min(heldout_users, U), replace=False)
    ev_items = rng.integers(0, I, ev_users.size)
    log(f"[bench] graph {gen}: N={U + I + B:,} nnz={len(v):,} built in {time.time() - t0:.1f}s "
        f"(host normalise {t_norm:.1f}s)")
    inter = (u, i, ib, t_norm) if keep_interactions else None
    return r, c, v, ev_users, ev_items, inter


def xavier(rows, d, gen):
    bound = float(np.sqrt(6.0 / (rows + d)))
    return (torch.rand(rows, d, generator=gen) * 2 - 1) * bound


DUMP_BYTES = 32 << 20  # --dump-outputs: cap of the dumped table (the whole dump stays under 64 MB)


def dump_outputs(path, out, r, hub_thr):
    """--dump-outputs: the final embeddings the timed path returned in its last timed step, as
    path/final_embeddings.npy (float32). A table above DUMP_BYTES is sampled by rows: the rows
    above the hub threshold (the exact plan's emulated and chained rows; at most a quarter of the
    sample) and a seeded draw over all rows, in row order — the same rows for the same arguments.
    path/final_embeddings_rows.npy (float64) holds their indices."""
    n, d = out.shape
    cap = DUMP_BYTES // (4 * d)
    if n > cap:
        hubs = np.nonzero(np.bincount(r, minlength=n) > hub_thr)[0][:cap // 4]
        draw = np.random.default_rng(11).choice(n, cap - hubs.size, replace=False)
        rows = np.union1d(hubs, draw)
        table = out[torch.from_numpy(rows).to(out.device)]
    else:
        rows, table = np.arange(n), out
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "final_embeddings.npy"), table.cpu().numpy())
    np.save(os.path.join(path, "final_embeddings_rows.npy"), rows.astype(np.float64))
    log(f"[bench] dumped {rows.size:,} of {n:,} output rows to {path}")


def bench_eval(final, U, I, r, c, dev, args, n_users=8192, k=20):
    """main.py:404-439 per-batch work on the propagated table: fused lgcn_score_topk vs the
    reference's torch ops (matmul + -1e10 mask of the train items + topk), same users."""
    from gcn_recommendation_amd import evaluate as E
    rng = np.random.default_rng(7)
    users = np.sort(rng.choice(U, n_users, replace=False))
    # train items per user = the user's row of Â (cols >= U)
    rp = np.searchsorted(r, np.arange(U + 1))
    lens = rp[users + 1] - rp[users]
    cols = np.concatenate([c[rp[u]:rp[u + 1]] for u in users]) - U
    mrow, mit = E.mask_csr(np.repeat(users, lens), cols, U)
    ue, ie = final[:U], final[U:U + I]
    if ie.shape[1] not in (64, 128):
        return {"skipped": "fused evaluate supports d in {64, 128}"}
    E.topk_fused(ue, ie, users, mrow, mit, k)
    torch.cuda.synchronize()
    t0 = time.time()
    reps = 3
    for _ in range(reps):
        s_f, i_f = E.topk_fused(ue, ie, users, mrow, mit, k)
    torch.cuda.synchronize()
    fused_ms = (time.time() - t0) / reps * 1e3
    # reference ops, 1024 users per batch (main.py:415), mask by one index_put per batch
    bu_all = torch.from_numpy(users).to(dev)
    rr = torch.from_numpy(np.repeat(np.arange(n_users), lens)).to(dev)
    cc = torch.from_numpy(cols).to(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    agree = 0
    for s0 in range(0, n_users, 1024):
        sc = ue[bu_all[s0:s0 + 1024]] @ ie.T
        sel = (rr >= s0) & (rr < s0 + 1024)
        sc[rr[sel] - s0, cc[sel]] = -1e10
        _, ti = torch.topk(sc, k)
        agree += int((ti == i_f[s0:s0 + 1024].long()).all(1).sum())
    torch.cuda.synchronize()
    torch_ms = (time.time() - t0) * 1e3
    flops = 2.0 * n_users * I * ue.shape[1]
    return {"users": n_users, "items": I, "k": k, "fused_ms": round(fused_ms, 2),
            "torch_ops_ms": round(torch_ms, 2), "speedup": round(torch_ms / fused_ms, 2),
            "fused_tflops": round(flops / (fused_ms / 1e3) / 1e12, 1),
            "mfma_f32_peak_tflops": 157.3,
            "top20_identical_frac": agree / n_users,
            "note": "torch_ops excludes the reference's per-user Python mask loop (main.py:422-424)"}


def bench_train_step(adj, emb_host, U, I, d, K, dev, args):
    """main.py's per-batch hot loop (main.py:488-531) with the drop-in model: full-graph forward
    through the engine, batch gathers, bpr_loss_reg, backward (K engine layers), Adam step.
    Edges/s counts the 2K propagated layers (K forward + K backward)."""
    from gcn_recommendation_amd.loss import bpr_loss_reg
    from models.lightgcn import LightGCN

    class Cfg:
        embedding_dim, n_layers, debug = d, K, False
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        model = LightGCN.__new__(LightGCN)
        torch.nn.Module.__init__(model)
        model.num_users, model.num_items, model.num_brands = U, I, 0
        model.embedding_dim, model.n_layers, model.debug = d, K, False
        model.user_embedding = torch.nn.Embedding.from_pretrained(emb_host[0].clone(), freeze=False)
        model.brand_embedding = torch.nn.Embedding(0, d)
        model.item_embedding = torch.nn.Embedding.from_pretrained(emb_host[1].clone(), freeze=False)
        model.final_brand_emb, model._graph_adj = None, None
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    rng = np.random.default_rng(0)
    # host batches, moved to the device inside the step and the loss read back after it, as
    # main.py:491 / 527 do every batch (the read-back keeps the host at most one step ahead)
    batches = [tuple(torch.from_numpy(x) for x in (rng.integers(0, U, 2048),
                                                    rng.integers(0, I, 2048),
                                                    rng.integers(0, I, 2048)))
               for _ in range(args.train_steps + 4)]

    def step(b):
        users, pos, neg = (t.to(dev) for t in b)
        opt.zero_grad()
        fu, fi, fb, u0, i0 = model(adj, use_brand=False)
        loss = bpr_loss_reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg], 1e-4)
        loss.backward()
        opt.step()
        return loss.item()
    # 4 warm-up steps: the caching allocator has settled (the bench allocated and released the
    # C4 tables before this) and the optimizer state exists
    for b in batches[:4]:
        step(b)
    torch.cuda.synchronize()
    retries0 = torch.cuda.memory_stats(dev).get("num_alloc_retries", 0)
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_host = time.time()
    a.record()
    for b in batches[4:]:
        loss = step(b)
    e.record()
    t_host = (time.time() - t_host) * 1e3 / args.train_steps
    torch.cuda.synchronize()
    ms = a.elapsed_time(e) / args.train_steps
    retries = torch.cuda.memory_stats(dev).get("num_alloc_retries", 0) - retries0
    if os.environ.get("BENCH_PROFILE_TRAIN"):  # host profile of 2 steps (diagnostics, to stderr)
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        for b in batches[:2]:
            step(b)
        pr.disable()
        torch.cuda.synchronize()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(20)
    # where a step's time goes: forward + loss, backward, optimizer, each bracketed by events on
    # the current stream (3 more steps; the events sit between the phases, no host sync inside)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    phases = np.zeros(3)
    for b in batches[:3]:
        users, pos, neg = (t.to(dev) for t in b)
        ev[0].record()
        opt.zero_grad()
        fu, fi, fb, u0, i0 = model(adj, use_brand=False)
        loss_ = bpr_loss_reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg], 1e-4)
        ev[1].record()
        loss_.backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        torch.cuda.synchronize()
        phases += [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
    phases /= 3
    # the same loop with torch's fused Adam (one kernel per parameter instead of main.py's
    # default foreach Adam, ~16 ms of multi_tensor_apply launches at C3): what the step costs
    # when the optimizer is not the bottleneck
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    for b in batches[:4]:
        step(b)
    torch.cuda.synchronize()
    a.record()
    for b in batches[4:]:
        step(b)
    e.record()
    torch.cuda.synchronize()
    ms_fused = a.elapsed_time(e) / args.train_steps
    nnz = adj._nnz()
    out = {"ms_per_step": round(ms, 3), "propagated_edges_per_s": round(2 * K * nnz / (ms / 1e3), 1),
           "batch": 2048, "optimizer": "Adam(lr=1e-3) (main.py's default: foreach)",
           "loss_last": float(loss),
           "fused_adam_ms_per_step": round(ms_fused, 3),
           "phases_ms": {"forward_and_loss": round(float(phases[0]), 3),
                         "backward": round(float(phases[1]), 3),
                         "adam": round(float(phases[2]), 3)},
           "wall_ms_per_step": round(t_host, 3), "alloc_retries": int(retries),
           "what": f"main.py:488-531 hot loop: batch to device, forward + gathers + bpr_loss_reg + "
                   f"backward + Adam over all {U + I:,} x {d} parameters; fused_adam_ms_per_step: the same "
                   f"with torch.optim.Adam(fused=True); loss.item() every step as main.py:527"}
    del model, opt
    torch.cuda.empty_cache()
    return out


def val_split(u, i):
    """main.py:201-203 verbatim: rank = groupby(user).rank(method="first", ascending=False) over
    the constant user column; rank 1 is the validation row, the rest is train. With pandas'
    "first" tie order that is each user's FIRST row in list order. Returns
    (train_u, train_i, val_u, val_i)."""
    import pandas as pd
    df = pd.DataFrame({"user_idx": u, "item_idx": i})
    rank = df.groupby("user_idx")["user_idx"].rank(method="first", ascending=False).to_numpy()
    val = rank == 1
    return u[~val], i[~val], u[val], i[val]


def bench_recall_trained_c3(dev, steps, k=20, batch=2048, n_val=2048):
    """A Recall@20 at C3 (BASELINE configs[2] shape) that carries information: the Books-shape
    power-law interactions with main.py's validation split held out (main.py:201-203), Â built
    on the device from the train rows (main.py:282-336), the drop-in LightGCN trained for `steps`
    BPR batches of main.py's loop (main.py:479-531: shuffled (user, pos) batches of 2048,
    negatives rejected against the user's train items, bpr_loss_reg, Adam lr=1e-3) through the
    engine. The trained weights are propagated by the engine (exact plan) and by the reference
    CPU path (torch.sparse.mm COO, oracle/), and both tables are scored with main.py's evaluate
    (oracle restatement) on n_val sampled validation users; the fused top-K kernel scores the
    engine's table too."""
    from gcn_recommendation_amd import evaluate as E
    from gcn_recommendation_amd.loss import bpr_loss_reg
    from models.lightgcn import LightGCN
    from oracle import oracle
    cfg = CONFIGS["c3"]
    U, I, d, K = cfg["users"], cfg["items"], cfg["d"], cfg["K"]
    t_all = time.time()
    u, i = graph.powerlaw_interactions(U, I, cfg["interactions"], cfg["seed"])
    tu, ti, vu, vi = val_split(u, i)
    del u, i
    adj = graph.build_norm_adj_device(tu, ti, U, I, 0, use_brand=False, device=dev)

    class Cfg:
        embedding_dim, n_layers, debug = d, K, False
    import contextlib
    import io
    torch.manual_seed(42)
    with contextlib.redirect_stdout(io.StringIO()):
        model = LightGCN(U, I, 0, Cfg()).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    train_keys = np.unique(tu * np.int64(I) + ti)
    rng = np.random.default_rng(0)
    perm = rng.permutation(tu.size)
    loss = None
    torch.cuda.synchronize()
    t0 = time.time()
    for st in range(steps):
        b = perm[st * batch:(st + 1) * batch]
        bu, bp = tu[b], ti[b]
        bn = rng.integers(0, I, b.size)
        while True:  # rejection against the user's train items (BPRDataset, main.py:357-363)
            key = bu * np.int64(I) + bn
            pos = np.minimum(np.searchsorted(train_keys, key), train_keys.size - 1)
            hit = train_keys[pos] == key
            if not hit.any():
                break
            bn[hit] = rng.integers(0, I, int(hit.sum()))
        users, pi, ni = (torch.from_numpy(x).to(dev) for x in (bu, bp, bn))
        opt.zero_grad()
        fu, fi, _, u0, i0 = model(adj, use_brand=False)
        loss = bpr_loss_reg(fu[users], fi[pi], fi[ni], u0[users], i0[pi], i0[ni], 1e-4)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    train_s = time.time() - t0
    del opt, train_keys
    # validation users (sampled) and their train items (the -1e10 mask of main.py:422-424)
    sel = np.sort(np.random.default_rng(1).choice(vu.size, min(n_val, vu.size), replace=False))
    su, si = vu[sel], vi[sel]
    m = np.isin(tu, su)
    mu, mi = tu[m], ti[m]
    with torch.no_grad():
        fu, fi, _, _, _ = model(adj)
        ego = torch.cat([model.user_embedding.weight, model.item_embedding.weight]).cpu()
        gpu = torch.cat([fu, fi]).cpu()
        mrow, mit = E.mask_csr(mu, mi, U)
        _, top = E.topk_fused(fu, fi, su, mrow, mit, k)
    del model
    torch.cuda.empty_cache()
    ref = oracle.reference_forward_torch(adj.cpu(), ego, K)
    rec_cpu = oracle.evaluate(ref[:U], ref[U:], su, si, mu, mi, k, batch_size=128)
    rec_gpu = oracle.evaluate(gpu[:U], gpu[U:], su, si, mu, mi, k, batch_size=128)
    hit = top.cpu().numpy() == si[:, None]
    found = hit.any(1)
    ndcg = np.where(found, 1.0 / np.log2(hit.argmax(1) + 2), 0.0)
    return {"config": "C3 power-law 10.3M x 4.4M x 29.5M, d=64, K=3; val = main.py:201-203's "
                      "split (groupby-rank 1: each user's first row)",
            "train_steps": steps, "batch": batch, "train_s": round(train_s, 1),
            "loss_last": float(loss.item()) if loss is not None else None,
            "val_users_scored": int(su.size), "val_users_total": int(vu.size),
            "recall20_gpu": rec_gpu[0], "ndcg20_gpu": rec_gpu[1],
            "recall20_cpu_ref": rec_cpu[0], "ndcg20_cpu_ref": rec_cpu[1],
            "identical": rec_gpu == rec_cpu,
            "embeddings_bitwise_equal": bool(torch.equal(gpu.view(torch.int32),
                                                         ref.view(torch.int32))),
            "fused_topk": {"recall20": float(found.mean()), "ndcg20": float(ndcg.mean())},
            "wall_s": round(time.time() - t_all, 1),
            "what": "weights trained on the GPU through the engine for `train_steps` BPR batches; "
                    "the same weights propagated by the engine and by the reference CPU path, "
                    "both scored by main.py's evaluate (oracle restatement) on sampled "
                    "validation users; fused_topk = the engine's lgcn_score_topk"}


def bench_recall_trained(dev, epochs, k=20, batch=2048):
    """Recall@20 / NDCG@20 that mean something (random-init embeddings give ~0 by construction):
    the C2 power-law graph (BASELINE configs[1] shape) with main.py's validation split held out
    (main.py:201-203: one row per user), trained for `epochs` epochs by main.py's loop (main.py:479-531:
    shuffled (user, pos) batches of 2048, uniform negatives rejected against the user's train
    items as BPRDataset does (main.py:357-363), model(adj) + bpr_loss_reg + backward + Adam
    lr=1e-3, reg 1e-4) with the drop-in LightGCN on the engine. Parity: the trained weights are
    propagated by the engine AND by the reference CPU path (torch.sparse.mm COO, oracle/), and
    both are scored with main.py's evaluate semantics; the engine's fused top-K is scored too."""
    from gcn_recommendation_amd import evaluate as E
    from gcn_recommendation_amd.loss import bpr_loss_reg
    from models.lightgcn import LightGCN
    from oracle import oracle
    cfg = CONFIGS["c2"]
    U, I, d, K = cfg["users"], cfg["items"], cfg["d"], cfg["K"]
    u, i = graph.powerlaw_interactions(U, I, cfg["interactions"], cfg["seed"])
    tu, ti, vu, vi = val_split(u, i)
    adj = graph.build_norm_adj(tu, ti, U, I, 0, use_brand=False, device=dev)

    class Cfg:
        embedding_dim, n_layers, debug = d, K, False
    import contextlib
    import io
    torch.manual_seed(42)
    with contextlib.redirect_stdout(io.StringIO()):
        model = LightGCN(U, I, 0, Cfg()).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    train_keys = np.unique(tu * I + ti)
    rng = np.random.default_rng(0)
    steps, t0, loss = 0, time.time(), None
    for _ in range(epochs):
        perm = rng.permutation(tu.size)
        for s0 in range(0, tu.size, batch):
            b = perm[s0:s0 + batch]
            bu, bp = tu[b], ti[b]
            bn = rng.integers(0, I, b.size)
            while True:  # rejection against the user's train items
                key = bu * I + bn
                pos = np.minimum(np.searchsorted(train_keys, key), train_keys.size - 1)
                hit = train_keys[pos] == key
                if not hit.any():
                    break
                bn[hit] = rng.integers(0, I, int(hit.sum()))
            users, pi, ni = (torch.from_numpy(x).to(dev) for x in (bu, bp, bn))
            opt.zero_grad()
            fu, fi, _, u0, i0 = model(adj, use_brand=False)
            loss = bpr_loss_reg(fu[users], fi[pi], fi[ni], u0[users], i0[pi], i0[ni], 1e-4)
            loss.backward()
            opt.step()
            steps += 1
    torch.cuda.synchronize()
    train_s = time.time() - t0
    with torch.no_grad():
        fu, fi, _, _, _ = model(adj)
        ego = torch.cat([model.user_embedding.weight, model.item_embedding.weight]).cpu()
    gpu = torch.cat([fu, fi]).cpu().numpy()
    ref = oracle.reference_forward_torch(adj.cpu(), ego, K).numpy()
    rec_cpu = oracle.evaluate(ref[:U], ref[U:], vu, vi, tu, ti, k)
    rec_gpu = oracle.evaluate(gpu[:U], gpu[U:], vu, vi, tu, ti, k)
    mrow, mit = E.mask_csr(tu, ti, U)
    _, top = E.topk_fused(fu, fi, vu, mrow, mit, k)
    hit = top.cpu().numpy() == vi[:, None]
    found = hit.any(1)
    ndcg = np.where(found, 1.0 / np.log2(hit.argmax(1) + 2), 0.0)
    scale = float(np.abs(ref).max())
    return {"config": "C2 power-law 50k x 50k x 1M, d=64, K=3; val = main.py:201-203's split "
                      "(groupby-rank 1: each user's first row)",
            "epochs": epochs, "train_steps": steps, "train_s": round(train_s, 1),
            "loss_last": float(loss.item()) if loss is not None else None,
            "val_users": int(vu.size),
            "recall20_gpu": rec_gpu[0], "ndcg20_gpu": rec_gpu[1],
            "recall20_cpu_ref": rec_cpu[0], "ndcg20_cpu_ref": rec_cpu[1],
            "identical": rec_gpu == rec_cpu,
            "fused_topk": {"recall20": float(found.mean()), "ndcg20": float(ndcg.mean())},
            "embeddings_normwise_vs_cpu_ref": float(np.abs(gpu - ref).max()) / scale,
            "what": "weights trained on the GPU through the engine; the same weights propagated "
                    "by the engine and by the reference CPU path, both scored by main.py's "
                    "evaluate (oracle restatement); fused_topk = the engine's lgcn_score_topk"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--gen", default="powerlaw", choices=["powerlaw", "uniform"])
    ap.add_argument("--hub-threshold", type=int, default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--recall-users", type=int, default=2048)
    ap.add_argument("--recall-epochs", type=int, default=10,
                    help="epochs of C2 training for the trained Recall@20 parity (0: skip)")
    ap.add_argument("--recall-steps-c3", type=int, default=300,
                    help="BPR steps of training on the C3 graph for a Recall@20 at C3 (0: skip)")
    ap.add_argument("--train-steps", type=int, default=10,
                    help="also time main.py's training step (forward+BPR+backward+Adam)")
    ap.add_argument("--mode", default="featsplit", choices=["rowpart", "featsplit"],
                    help="multi-GPU decomposition (N>1)")
    ap.add_argument("--no-c4", dest="c4", action="store_false",
                    help="skip the d=256 K=4 (BASELINE configs[3]) timing on the same graph")
    ap.add_argument("--no-dist-backward", dest="backward", action="store_false",
                    help="N > 1: skip the featsplit backward timing")
    ap.add_argument("--no-rowpart", dest="rowpart", action="store_false",
                    help="N > 1: skip the secondary rowpart (per-layer RCCL all-gather) timing")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the distributed path even at WORLD_SIZE=1 (testing)")
    ap.add_argument("--full", action="store_true",
                    help="one GPU: after the headline, also measure and check everything else "
                         "(roofline and per-kernel timing, adjacency builder, C4, backward, eval, "
                         "training step, CPU baseline + parity, chunk mode, trained Recall@20)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="one GPU: write the last timed step's output to DIR/*.npy (float32 "
                         "table, a seeded row sample when it is above 32 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # LGCN_SHARED_GPU=1 (with LGCN_DIST_BACKEND=gloo): every rank on cuda:0 — a rehearsal of
    # the N > 1 path on a one-GPU box; the numbers it prints are not a scaling measurement
    local_rank = 0 if os.environ.get("LGCN_SHARED_GPU") else int(os.environ.get("LOCAL_RANK", "0"))
    if args.dump_outputs and (world > 1 or args.force_dist):
        ap.error("--dump-outputs writes the one-GPU run's output")
    if world != args.gpus:
        log(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    cfg = CONFIGS[args.config]
    d, K = cfg["d"], cfg["K"]
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    engine.load_library()
    hub_thr = args.hub_threshold if args.hub_threshold is not None else engine.hub_threshold_from_env()

    U, I, B = cfg["users"], cfg["items"], cfg.get("brands", 0)

    def tables():
        gen = torch.Generator().manual_seed(42)
        return [xavier(U, d, gen), xavier(I, d, gen)] + ([xavier(B, d, gen)] if B else [])
    # the tables (a serial generator) are drawn beside the graph build: both release the GIL
    with ThreadPoolExecutor(1) as pool:
        emb_job = pool.submit(tables)
        r, c, v, ev_users, ev_items, inter = make_graph(
            cfg, args.gen, args.recall_users, keep_interactions=(world == 1 and args.full))
        emb_host = emb_job.result()
    n = U + I + B
    nnz = len(v)
    fusion = cfg.get("content", 0)

    if world > 1 or args.force_dist:
        from gcn_recommendation_amd import dist
        args.users, args.items = cfg["users"], cfg["items"]
        result = dist.bench_distributed(args, cfg, r, c, v, emb_host, dev, hub_thr)
        if rank == 0:
            print(json.dumps(result), flush=True)
        dist.shutdown()
        return

    # ---------------- single GPU ----------------
    t0 = time.time()
    idx = torch.from_numpy(np.vstack((r, c)))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(v), (n, n)).to(dev)
    del idx
    # the sides the model offers (engine.propagate_blocks: the item rows): a bipartite graph is
    # stored side-major and propagated by the two-lane schedule
    g = engine.graph_from_coo(adj, sides=(U, U + I))
    sided = g.split is not None
    hp = g.hubs(hub_thr)
    torch.cuda.synchronize()
    prep_s = time.time() - t0
    segs = [t.to(dev) for t in emb_host]
    if hp.mode == "exact":
        log(f"[bench] CSR plan {prep_s:.2f}s; exact plan: {hp.n_emu_rows} rows above the "
            f"threshold {hub_thr} ({hp.n_emu_blocks} emulation blocks; the shorter ones run as "
            f"chains); max degree {int(g.degrees().max())}; "
            f"schedule {'two lanes' if sided else 'one operator'}")
    else:
        log(f"[bench] CSR plan {prep_s:.2f}s; hubs: {hp.n_rows} rows / {hp.n_items} chunks "
            f"(threshold {hub_thr}); max degree {int(g.degrees().max())}")

    if fusion:  # LightGCN_Fusion forward: [user | leaky_relu(Linear([id | content])) | brand]
        content = torch.from_numpy(np.random.default_rng(5).standard_normal(
            (I, fusion)).astype(np.float32)).to(dev)
        lin = torch.nn.Linear(d + fusion, d).to(dev)

        from gcn_recommendation_amd import fusion as FU

        def step(ev=None, kev=None, mode=None):
            with torch.no_grad():
                fused = FU.fused_item_embedding(segs[1], content, lin)
                return engine.propagate_forward(g, [segs[0], fused] + segs[2:], K, hub_thr,
                                                layer_events=ev, kernel_events=kev,
                                                hub_mode=mode)

        def prelayer_ms(fn, reps=10):
            fn()
            torch.cuda.synchronize()
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record()
            for _ in range(reps):
                fn()
            b_.record()
            torch.cuda.synchronize()
            return a_.elapsed_time(b_) / reps

        def bench_prelayer():
            with torch.no_grad():
                t_fused = prelayer_ms(lambda: FU.fused_item_embedding(segs[1], content, lin))
                t_torch = prelayer_ms(lambda: torch.nn.functional.leaky_relu(
                    lin(torch.cat([segs[1], content], 1))))
                f_ref = torch.nn.functional.leaky_relu(lin(torch.cat([segs[1], content], 1)))
                f_got = FU.fused_item_embedding(segs[1], content, lin)
                pre_err = float((f_got - f_ref).abs().max() / f_ref.abs().max())
            fl = 2.0 * I * (d + fusion) * d
            return {"fused_ms": round(t_fused, 3), "torch_ops_ms": round(t_torch, 3),
                    "fused_tflops": round(fl / (t_fused / 1e3) / 1e12, 1),
                    "normwise_vs_torch": pre_err,
                    "what": "lightgcn_fusion.py:45-49 leaky_relu(Linear(cat([id, content]))): "
                            "lgcn_fusion_prelayer vs torch cat + Linear (hipBLASLt) + leaky_relu"}
        prelayer = bench_prelayer() if args.full else None
    else:
        def step(ev=None, kev=None, mode=None):
            return engine.propagate_forward(g, segs, K, hub_thr, layer_events=ev,
                                            kernel_events=kev, hub_mode=mode)

    def timed(mode, steps, warmup, kernels=True):
        """(ms per step, [steps x K] layer ms, [steps x K] layer-kernel ms, output). Sided: no
        layer boundary exists (the two lanes overlap layers), layer ms is None and the kernel ms
        are [steps x K x 4] — each segment's layer kernel (the side-0 classes, side 1), timed on
        its lane's stream (0 for an empty segment); they take a second loop of the same steps,
        which runs only with `kernels` (else they are None)."""
        for _ in range(warmup):
            step(mode=mode)
        torch.cuda.synchronize()
        mk = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        evs = [[mk() for _ in range(K)] for _ in range(steps)]
        kevs = [[mk() for _ in range(K)] for _ in range(steps)]
        a_, b_ = mk()
        torch.cuda.synchronize()
        a_.record()
        for s_ in range(steps):
            o = step(None, None, mode) if sided else step(evs[s_], kevs[s_], mode)
        b_.record()
        torch.cuda.synchronize()
        if sided and not kernels:
            return a_.elapsed_time(b_) / steps, None, None, o
        if sided:
            # the half-layers' layer-kernel times from a second loop of the same steps: the
            # timing events recorded on the lanes' streams cost the timed loop ~0.5 ms per step
            # at C3, so the headline loop above runs without them
            engine.side_timing = []
            for s_ in range(steps):
                step(None, None, mode)
            torch.cuda.synchronize()
            tm, engine.side_timing = engine.side_timing, None
            ker = np.array([[[t[(k, s)][0].elapsed_time(t[(k, s)][1]) if (k, s) in t else 0.0
                              for s in range(engine.N_SEGS)]
                             for k in range(1, K + 1)] for t in tm])
            return a_.elapsed_time(b_) / steps, None, ker, o
        lay = np.array([[x.elapsed_time(y) for x, y in st] for st in evs])
        ker = np.array([[x.elapsed_time(y) for x, y in st] for st in kevs])
        return a_.elapsed_time(b_) / steps, lay, ker, o

    def side_phases(fn):
        """Per-half-layer phase log of one call of fn (ms from its first fork): the lanes'
        critical paths, engine.side_trace."""
        engine.side_trace = []
        fn()
        torch.cuda.synchronize()
        tr, engine.side_trace = engine.side_trace[0], None
        t0_ = tr[min(tr)][0][1]
        return {f"layer{k}_seg{s}_lane{(k + (s == 3) + K) % 2}":
                {nm: round(t0_.elapsed_time(ev), 3) for nm, ev in tr[(k, s)]}
                for (k, s) in sorted(tr)}

    # the headline: the engine's default (exact) hub mode — every row bitwise the reference's
    hub_mode = engine.hub_mode_from_env()
    torch.cuda.synchronize()
    t_wall = time.time()
    ms_step, layer_ms, kern_ms, out = timed(hub_mode, args.steps, args.warmup, kernels=args.full)
    wall = time.time() - t_wall
    ms_total = ms_step * args.steps
    value = K * nnz * args.steps / (ms_total / 1e3)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, r, hub_thr)

    result = {
        "metric": "propagated edges/sec (SpMM) + Recall@20, Amazon-Books 3-layer d=64",
        "value": round(value, 1), "unit": "edges/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 4), "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": cfg["name"], "generator": args.gen, "users": U, "items": I,
                   "interactions": cfg["interactions"], "nnz": nnz, "d": d, "layers": K,
                   "brands": B, "content_dim": fusion,
                   "hub_threshold": hub_thr, "hub_mode": hub_mode,
                   "emu_min_degree": engine.emu_min_degree_from_env(nnz),
                   "schedule": ("bipartite two-lane (lgcn_propagate_forward_sides), "
                                f"side-0 classes {list(g.class_end or ())} (parts "
                                f"{list(g.class_parts)}), "
                                f"{engine.n_aux_streams()} aux streams, GPU_MAX_HW_QUEUES="
                                f"{os.environ.get('GPU_MAX_HW_QUEUES', 'unset (HIP default 4)')}") if sided else "one operator",
                   "parallelism": "single"},
        "wall_s_timed": round(wall, 3), "prep_s": round(prep_s, 2),
    }
    if not args.full:  # the headline alone; everything below is --full
        print(json.dumps(result), flush=True)
        return

    # the device adjacency builder on the same interactions: time + bitwise
    u_, i_, ib_, t_norm = inter
    torch.cuda.synchronize()
    t0 = time.time()
    adj_dev = graph.build_norm_adj_device(u_, i_, U, I, B, ib_[0], ib_[1], bool(B), device=dev)
    torch.cuda.synchronize()
    t_dev = time.time() - t0
    builder = {"host_numpy_s": round(t_norm, 2), "device_s": round(t_dev, 2),
               "bitwise_equal": bool(torch.equal(adj_dev._indices(), adj._indices()) and torch.equal(
                   adj_dev._values().view(torch.int32), adj._values().view(torch.int32)))}
    del adj_dev, inter, u_, i_

    # Roofline of the dominant HBM kernel: the STORE instantiation of k_layer (layers
    # 1..K-1; rocprof name k_layer<float4,16,1,0,15,4,0,0>), timed live with HIP events around
    # its launch on the stream it runs on (the emulated hub rows run beside it on side streams).
    # frac = MEASURED HBM bytes per launch (profiles/traffic_<config>_<gen>.json: rocprofv3 PMC
    # FETCH_SIZE + WRITE_SIZE, stamped with the hash of the kernel sources; a stale file is
    # refused) / launch time / peak. Algorithmic bytes are reported beside it.
    # algorithmic bytes of one layer-kernel launch (SURVEY §8d per-edge model over the rows the
    # kernel itself runs — bundle rows (degree <= threshold) and, in the exact plan, the
    # whole-row items up to emu_min_degree; longer rows run beside it): gathered X rows (4d) +
    # edge records (8) per edge, row pointers, one written row per row it runs
    rp_h = g.rowptr_host().astype(np.int64)
    emu_min = engine.emu_min_degree_from_env(nnz)

    def kernel_bytes(s0, s1):
        deg_ = np.diff(rp_h[s0:s1 + 1])
        run = deg_ <= max(min(hub_thr, engine.INT32_MAX), emu_min if hub_mode == "exact" else 0)
        return int(deg_[run].sum()) * (4 * d + 8) + 4 * (s1 - s0 + 1) + 4 * int(run.sum()) * d
    if sided:
        segs_ = g.segments()
        b_seg = [kernel_bytes(a, b) if b > a else 0 for a, b in segs_]
        live_ = [gi for gi, (a, b) in enumerate(segs_) if b > a]
        # STORE launches: layers 1..K-1, every non-empty segment; bytes and time summed over them
        st_k = kern_ms[:, :-1, :] if K > 1 else kern_ms
        n_launch = len(live_) * st_k.shape[1]
        store_ms = float(st_k.sum(axis=(1, 2)).mean()) / max(n_launch, 1)
        b_layer = sum(b_seg[gi] for gi in live_) * st_k.shape[1] / max(n_launch, 1)
        mean_ms = float(kern_ms[:, -1, :].sum(axis=1).mean()) / max(len(live_), 1)
        kname = (f"k_layer<float4,{min(64, d // 4)},{max(1, d // 256)},STORE> segment launches "
                 f"(layers 1..K-1: the users' classes and the items; bundle rows and whole-row "
                 f"items up to {emu_min} edges)")
    else:
        b_layer = kernel_bytes(0, n)
        store_ms = float(kern_ms[:, :-1].mean()) if K > 1 else float(kern_ms.mean())
        mean_ms = float(kern_ms[:, -1].mean())
        kname = (f"k_layer<float4,{min(64, d // 4)},{max(1, d // 256)},STORE> "
                 f"(layers 1..K-1: bundle rows)")
    alg = b_layer / (store_ms / 1e3) / 1e9
    # achieved / frac: ALGORITHMIC bytes per launch (SURVEY §8d per-edge model over the rows the
    # kernel runs) over the launch time measured live; traffic: the PMC HBM bytes of the same
    # kernel (profiles/traffic_*.json, below) — below the algorithmic bytes when gathered rows hit
    # L2/MALL, above them when lines are fetched twice
    roof = {"bound": "hbm", "achieved": round(alg, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(alg / PEAK_HBM_GBS, 4), "traffic": None, "kernel": kname,
            "avg_launch_ms": round(store_ms, 4),
            #  achieved / frac are on the ALGORITHMIC basis the task contract sets
            # since round 5; rounds 2-4 put the PMC-measured rate there — that one is
            # traffic_rate now, so compare like with like
            "basis": "algorithmic (SURVEY §8d); measured-traffic rate: traffic_rate",
            "algorithmic": {"bytes_per_launch": int(b_layer), "achieved": round(alg, 1),
                            "frac": round(alg / PEAK_HBM_GBS, 4),
                            "note": "SURVEY §8d byte model over the kernel's own rows"},
            "mean_layer": {"avg_launch_ms": round(mean_ms, 4)}}
    # the whole forward on the same basis: SURVEY §8d bytes of K layers over the step time
    b_fwd = K * (nnz * (4 * d + 8) + 4 * (n + 1) + 4 * n * d)
    roof["forward"] = {"bytes": int(b_fwd), "ms": round(ms_step, 4),
                       "achieved": round(b_fwd / (ms_step / 1e3) / 1e9, 1),
                       "frac": round(b_fwd / (ms_step / 1e3) / 1e9 / PEAK_HBM_GBS, 4),
                       "note": "K x (nnz (4d + 8) + 4 (N + 1) + 4 N d) per forward / ms_per_step"}
    if sided:
        roof["segment_kernel_ms"] = {f"layer{k + 1}": [round(float(x), 4) for x in row]
                                     for k, row in enumerate(kern_ms.mean(0))}
        roof["algorithmic"]["bytes_per_segment"] = b_seg
        roof["algorithmic"]["launches_per_step"] = n_launch
        roof["note"] = ("the layer kernel's time (and so frac) is measured as it runs, sharing "
                        "the GPU with the emulation kernels and the other lane")
    else:
        layer_avg = float(layer_ms.mean())
        roof["layer"] = {"avg_ms": round(layer_avg, 4),
                         "per_layer_ms": [round(x, 4) for x in layer_ms.mean(0).tolist()],
                         "per_layer_kernel_ms": [round(x, 4) for x in kern_ms.mean(0).tolist()],
                         "note": "whole layer = layer kernel + the exact emulation of the hub "
                                 "rows (block pass + walk on side streams)"}
    def attach_traffic(roof, mode, store_ms):
        """frac from the committed PMC traffic of this kernel-source build (refused if stale)."""
        suffix = "" if mode == "exact" else f"_{mode}"
        traffic_file = os.path.join(ROOT, "profiles",
                                    f"traffic_{args.config}_{args.gen}{suffix}.json")
        if not os.path.exists(traffic_file):
            roof["traffic_note"] = f"no {os.path.basename(traffic_file)}"
            return
        tj = json.load(open(traffic_file))
        stamp = kernel_source_hash()
        if tj.get("source_hash") != stamp:
            roof["traffic_note"] = (f"{os.path.basename(traffic_file)} refused: measured with "
                                    f"kernel sources {tj.get('source_hash')}, these are {stamp}")
            return
        tb = tj["hbm_bytes_per_launch"]
        roof["traffic"] = tb
        roof["traffic_rate"] = {"achieved": round(tb / (store_ms / 1e3) / 1e9, 1),
                                "frac": round(tb / (store_ms / 1e3) / 1e9 / PEAK_HBM_GBS, 4)}
        roof["traffic_source"] = f"profiles/{os.path.basename(traffic_file)} " \
                                 f"(rocprof avg {tj.get('avg_duration_ms_rocprof')} ms)"
        if tj.get("algorithmic_bytes_per_launch") is not None:
            roof["traffic_algorithmic_bytes"] = tj["algorithmic_bytes_per_launch"]
        # the exact plan's other kernels from the same PMC passes: measured HBM bytes over their
        # rocprof launch time (the walk is latency-bound: its fraction is low by design)
        ks = {}
        for full, v in tj.get("kernels", {}).items():
            nm = full.replace("void ", "").replace("(anonymous namespace)::", "")
            if nm.startswith(("k_emu_blocks<0>", "k_emu_walk<0, 0>", "k_emu_walk<3, 0>",
                              "k_chain_rows<0, 0, 32, true>", "k_layer<HIP_vector_type<float, 4u>, 16, 1, 1,")) \
                    and v.get("avg_ms"):
                rate = v["hbm_bytes_per_launch"] / (v["avg_ms"] / 1e3) / 1e9
                ks[nm] = {"avg_ms_rocprof": round(v["avg_ms"], 4),
                          "hbm_bytes_per_launch": int(v["hbm_bytes_per_launch"]),
                          "achieved": round(rate, 1), "frac": round(rate / PEAK_HBM_GBS, 4)}
        if ks:
            roof["kernels_measured"] = ks
    attach_traffic(roof, hub_mode, store_ms)

    result["roofline"] = roof
    result["adjacency_build"] = builder
    if fusion:
        result["fusion_prelayer"] = prelayer
    if sided:
        result["phases_ms"] = {"forward": side_phases(lambda: step(mode=hub_mode)),
                               "note": "one forward's half-layers (layer k, side s on lane "
                                       "(k+s+K)%2; side 0 = users(+brands), 1 = items): ms from "
                                       "the first fork at which each part is done"}

    # BASELINE configs[3] on the same graph (d=256, K=4): the 1-GPU side of the 8-GPU target
    # (dist.featsplit_c4 times the same forward on d/P columns per rank at N > 1)
    if args.c4 and not fusion and not B:
        from gcn_recommendation_amd import dist as D
        gen4 = torch.Generator(device=dev).manual_seed(1000)
        x4 = (torch.rand((n, D.C4_D), generator=gen4, device=dev) * 2 - 1) * float(
            np.sqrt(6.0 / (n + D.C4_D)))
        c4 = {"d": D.C4_D, "layers": D.C4_K}
        x4s = [x4[:U], x4[U:]]   # the model's segments: the sided schedule when g has sides
        for mode in ("exact", "chunk"):
            for _ in range(2):
                engine.propagate_forward(g, x4s, D.C4_K, hub_thr, hub_mode=mode)
            mk = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a4, z4 = mk()
            torch.cuda.synchronize()
            a4.record()
            for s_ in range(5):
                engine.propagate_forward(g, x4s, D.C4_K, hub_thr, hub_mode=mode)
            z4.record()
            torch.cuda.synchronize()
            ms4 = a4.elapsed_time(z4) / 5
            c4[mode] = {"ms_per_step": round(ms4, 3),
                        "edges_per_s": round(D.C4_K * nnz / (ms4 / 1e3), 1)}
        result["c4_same_graph"] = c4
        del x4
        torch.cuda.empty_cache()

    # backward propagation alone (the K engine layers autograd runs per training batch)
    gsegs = [out[:U].clone(), out[U:].clone()]
    for _ in range(2):
        engine.propagate_backward(g, gsegs, K, hub_thr)
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.steps):
        engine.propagate_backward(g, gsegs, K, hub_thr)
    e.record()
    torch.cuda.synchronize()
    bwd_ms = a.elapsed_time(e) / args.steps
    # the same dense G with the row mask forced (round 5's default: every row live, the masked and
    # live-edge kernels run anyway) and with the mask off (the dense kernels, as the auto mode now
    # picks from the hint ring): the round-5 16.4 vs 13.1 ms question answered on one G
    forced = {}
    for mode in ("on", "off"):
        engine.propagate_backward(g, gsegs, K, hub_thr, sparse=mode)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            engine.propagate_backward(g, gsegs, K, hub_thr, sparse=mode)
        e.record()
        torch.cuda.synchronize()
        forced[mode] = round(a.elapsed_time(e) / args.steps, 4)
    # the upstream gradient of one BPR batch (main.py:496-497: 2048 users, 2048 pos + 2048 neg
    # items): row-sparse, so the masked backward gathers only its live rows in layer 1
    rs = np.random.default_rng(1)
    for t in gsegs:
        t.zero_()
    gsegs[0][torch.from_numpy(rs.integers(0, U, 2048)).to(dev)] = 1e-3
    gsegs[1][torch.from_numpy(rs.integers(0, I, 4096)).to(dev)] = -1e-3
    for _ in range(3):   # (the first call still follows the dense G's hint)
        engine.propagate_backward(g, gsegs, K, hub_thr)
        torch.cuda.synchronize()
    a.record()
    for _ in range(args.steps):
        engine.propagate_backward(g, gsegs, K, hub_thr)
    e.record()
    torch.cuda.synchronize()
    bpr_ms = a.elapsed_time(e) / args.steps
    result["backward"] = {"ms_per_step": round(bwd_ms, 4),
                          "propagated_edges_per_s": round(K * nnz / (bwd_ms / 1e3), 1),
                          "what": "dE0 = sum_k (Â^T)^k G/(K+1), Horner order, G read in place "
                                  "(dense G; auto mode: no row mask once the hint ring says G is "
                                  "dense)",
                          "dense_G_mask_forced_ms": forced["on"],
                          "dense_G_mask_off_ms": forced["off"],
                          "bpr_batch_G_ms_per_step": round(bpr_ms, 4),
                          "bpr_batch_G": "G = a BPR batch's output gradient (<= 6144 live rows): "
                                         "row-sparse path (lgcn_rows_nonzero mask)"}
    del gsegs

    if not fusion:
        result["eval_topk"] = bench_eval(out, U, I, r, c, dev, args)

    if args.train_steps > 0 and not fusion and not B:
        result["train_step"] = bench_train_step(adj, emb_host, U, I, d, K, dev, args)

    # parity + Recall@20 vs the reference CPU path (torch.sparse.mm restated in oracle/)
    if not args.no_cpu_baseline and not fusion and d * (K + 1) <= 256:
        from oracle import oracle
        adj_cpu = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((r, c))), torch.from_numpy(v),
                                          (n, n))
        ego = torch.cat(emb_host, 0)
        # The reference's CPU path on all of this host's cores (torch's intra-op pool; on the
        # GPU box that is the job's CPU share), timed per torch.sparse.mm layer: median of the
        # K layer samples (the forward runs once — a full K-layer C3 pass is ~10-30 s of CPU)
        threads = torch.get_num_threads()
        lt = []
        t0 = time.time()
        ref = oracle.reference_forward_torch(adj_cpu, ego, K, layer_times=lt)
        cpu_s = time.time() - t0
        med = float(np.median(lt))
        result["cpu_baseline"] = {
            "value": round(nnz / med, 1), "unit": "edges/s", "cores": threads,
            "kind": "port", "cpu_model": cpu_model(), "host_cpu_count": os.cpu_count(),
            "per_layer_s": [round(x, 3) for x in lt], "forward_s": round(cpu_s, 2),
            "sample": f"median of the {K} torch.sparse.mm layers (nnz={nnz} edges each) of one "
                      f"full forward (models/lightgcn.py:40-54 restated in oracle/) over the "
                      f"same graph, {threads} intra-op threads"}
        # the same layer on every host thread (os.cpu_count()), beside the job's
        # share above: one torch.sparse.mm layer (models/lightgcn.py:45), bounded
        all_threads = os.cpu_count() or threads
        if all_threads != threads:
            lt_all = []
            torch.set_num_threads(all_threads)
            try:
                oracle.reference_forward_torch(adj_cpu, ego, 1, layer_times=lt_all)
            finally:
                torch.set_num_threads(threads)
            result["cpu_baseline"]["all_host_threads"] = {
                "threads": all_threads, "value": round(nnz / lt_all[0], 1), "unit": "edges/s",
                "layer_s": round(lt_all[0], 3),
                "sample": "layer 1 of the same forward, torch intra-op threads = os.cpu_count()"}
        got = out.cpu().numpy()
        refn = ref.numpy()
        f64 = oracle.forward_f64(r, c, v, ego.numpy(), K)   # fp64 arbiter of both fp32 paths
        scale = float(np.abs(refn).max())

        def parity(got):
            err = float(np.abs(got - refn).max())
            e_gpu = float(np.abs(got - f64).max())
            e_cpu = float(np.abs(refn - f64).max())
            return {
                "gate": "north_star: max|gpu - cpu_ref| <= 1e-5 * max|cpu_ref| per tensor",
                "bitwise_equal_to_cpu_ref": bool(np.array_equal(got, refn)),
                "rows_bitwise_equal_frac": float(np.all(got == refn, axis=1).mean()),
                "normwise_vs_cpu_ref": err / scale,
                "pass_vs_cpu_ref": err <= 1e-5 * scale,
                "fp64_arbiter": {"gpu_normwise": e_gpu / scale, "cpu_ref_normwise": e_cpu / scale}}
        result["parity"] = parity(got)
        result["parity"].update({
            "mode": hub_mode, "hub_rows": int(np.count_nonzero(g.degrees() > hub_thr)),
            "max_degree": int(g.degrees().max()),
            "what": "the timed headline output (hub_mode=exact: rows above emu_min_degree run "
                    "as a block emulation of the reference's sequential fp32 chain) vs "
                    "torch.sparse.mm on the CPU"})
        # secondary: chunked hub rows (fixed-order partial sums; faster, not bitwise at hubs)
        ms_c, lay_c, ker_c, out_c = timed("chunk", args.steps, 1)
        pc = parity(out_c.cpu().numpy())
        del out_c
        # per STORE layer: the layer kernel's launches (sided: one per segment, summed)
        store_c = float(ker_c[:, :-1].sum(axis=2).mean() if ker_c.ndim == 3
                        else ker_c[:, :-1].mean())
        b_full = nnz * (4 * d + 8) + 4 * (n + 1) + 4 * n * d  # every row runs in the kernel
        alg_c = b_full / (store_c / 1e3) / 1e9
        roof_c = {"bound": "hbm", "achieved": round(alg_c, 1), "peak": PEAK_HBM_GBS,
                  "unit": "GB/s", "frac": round(alg_c / PEAK_HBM_GBS, 4), "traffic": None,
                  "avg_launch_ms": round(store_c, 4),
                  "algorithmic": {"bytes_per_launch": int(b_full)},
                  "note": "chunk mode: every row (hub rows as chunks) runs inside the layer "
                          "kernel, so a launch covers the whole layer's SURVEY §8d bytes"}
        attach_traffic(roof_c, "chunk", store_c)
        result["chunk_mode"] = {
            "ms_per_step": round(ms_c, 4), "edges_per_s": round(K * nnz / (ms_c / 1e3), 1),
            "per_layer_ms": ([round(x, 4) for x in lay_c.mean(0).tolist()]
                             if lay_c is not None else None),
            "store_kernel_ms": round(store_c, 4), "roofline": roof_c,
            "parity": pc,
            "what": "hub_mode=chunk: rows above hub_threshold cut into fixed chunks summed in a "
                    "fixed order — deterministic, within the fp64 arbiter's reach, but not the "
                    "reference's rounding on hub rows"}
        del f64
        # Recall@20 of both tables scored by the SAME deterministic scorer (the fused kernel: an
        # ordered fmaf chain per score), so any top-20 difference comes from the embeddings —
        # torch.matmul on the GPU is not run-to-run deterministic and reorders near-ties itself
        from gcn_recommendation_amd import evaluate as E
        rp = np.searchsorted(r, np.arange(n + 1)).astype(np.int64)
        eu = np.asarray(ev_users, np.int64)
        lens = rp[eu + 1] - rp[eu]
        mcols = np.concatenate([c[rp[u]:rp[u + 1]] for u in eu]) - U
        mrow, mit = E.mask_csr(np.repeat(eu, lens), mcols, U)
        ref_d = ref.to(dev)
        tops = []
        for table in (out, ref_d):
            _, ti = E.topk_fused(table[:U], table[U:], eu, mrow, mit, 20)
            tops.append(ti.cpu().numpy())
        del ref_d

        def rec(top):
            hit = top == np.asarray(ev_items)[:, None]
            found = hit.any(1)
            return float(found.mean()), float(np.where(found, 1 / np.log2(hit.argmax(1) + 2),
                                                        0.0).mean())
        rg, rc = rec(tops[0]), rec(tops[1])
        result["recall20"] = {"gpu": rg[0], "cpu": rc[0], "ndcg_gpu": rg[1], "ndcg_cpu": rc[1],
                              "identical": rg == rc, "users": int(len(eu)),
                              "top20_lists_identical_frac": float(
                                  np.all(tops[0] == tops[1], axis=1).mean()),
                              "top20_sets_identical_frac": float(np.mean(
                                  [set(a) == set(b) for a, b in zip(tops[0], tops[1])])),
                              "scorer": "lgcn_score_topk for both tables (deterministic)",
                              "note": "random-init embeddings and random held-out items: recall "
                                      "is ~0 by construction; the top-20 list agreement is the "
                                      "informative parity number (recall20_trained has a real "
                                      "Recall@20)"}
    if args.recall_epochs > 0 and args.config == "c3" and not args.no_cpu_baseline:
        result["recall20_trained"] = bench_recall_trained(dev, args.recall_epochs)
    if args.recall_steps_c3 > 0 and args.config == "c3" and not args.no_cpu_baseline:
        out = None
        torch.cuda.empty_cache()
        result["recall20_trained_c3"] = bench_recall_trained_c3(dev, args.recall_steps_c3)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
