#!/usr/bin/env python
"""Time the optimizer of a C3 training step three ways in one process: torch.optim.Adam as main.py
constructs it (the foreach path), torch.optim.Adam(fused=True), and optim.Adam (lgcn_adam_step),
on bench.py's C3 graph and tools/bpr_step_bench.py's model construction.

  * whole steps (batch to device, model.bpr_step, backward, optimizer step, loss.item()) with each
    optimizer, alternating blocks of steps, per-step time of a block, median over the blocks;
  * the optimizer step alone on the gradients the last batch left, bracketed by events on the
    current stream, alternating blocks; `spread_ms` is max - min of an optimizer's block times;
  * bytes: 7 streams (p, g, m, v read; p, m, v written) x 4 B x elements, over the step time, as a
    fraction of 8 TB/s;
  * the three models see the same batches in the same order: `parameters_bit_equal_after_run`
    (optim.Adam against torch's default; asserted) and, as information,
    `torch_fused_bit_equal_to_default`;
  * gate (exit status 1 when missed): optim.Adam's median optimizer step is below torch default's
    by more than the larger of the two spreads.

--ab-lib PATH times lgcn_adam_step alone from two builds of the library in alternating blocks (the
loaded one, whose g, m and v accesses are non-temporal, against PATH, e.g. the plain variant from
`python -m gcn_recommendation_amd._build adam_plain LGCN_ADAM_NT=0`) on tensors of C3's table sizes.

Prints one JSON line on stdout (progress goes to stderr).

    python tools/adam_bench.py [--config c3] [--blocks 5] [--steps-per-block 4] [--ab-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (CONFIGS, make_graph, xavier: the generator bench.py times)
from bpr_step_bench import LAMBDA, bits_equal, make_model  # noqa: E402
from gcn_recommendation_amd import engine, optim  # noqa: E402

HBM_PEAK = 8e12  # bytes/s
OPTIMIZERS = (("torch_default", lambda ps: torch.optim.Adam(ps, lr=1e-3)),
              ("torch_fused", lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True)),
              ("engine", lambda ps: optim.Adam(ps, lr=1e-3)))


def timed_blocks(names, run, blocks, steps):
    """Alternating blocks: {name: [ms per step of each block]}; run(name) enqueues one step."""
    per_block = {name: [] for name in names}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(blocks):
        for name in names:
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                run(name)
            e.record()
            torch.cuda.synchronize()
            per_block[name].append(a.elapsed_time(e) / steps)
    return per_block


def summary(per_block):
    return {"median_ms": {k: round(float(np.median(v)), 3) for k, v in per_block.items()},
            "spread_ms": {k: round(float(np.ptp(v)), 3) for k, v in per_block.items()},
            "block_ms": {k: [round(x, 3) for x in v] for k, v in per_block.items()}}


def ab_libs(args, cfg, dev):
    """lgcn_adam_step alone, the loaded library against --ab-lib, same tensors, alternating."""
    libs = {"loaded": engine.load_library(), "ab": ctypes.CDLL(args.ab_lib)}
    for lib in libs.values():
        lib.lgcn_adam_step.restype = ctypes.c_int
        lib.lgcn_adam_step.argtypes = [ctypes.POINTER(engine.AdamTensorT), ctypes.c_int32,
                                       ctypes.POINTER(engine.AdamHyperT), ctypes.c_void_p]
    gen = torch.Generator(device=dev).manual_seed(3)
    sizes = [cfg["users"] * cfg["d"], cfg["items"] * cfg["d"]]
    table = (engine.AdamTensorT * len(sizes))()
    keep = []
    for d, n in zip(table, sizes):
        p, g, m = (torch.randn(n, device=dev, generator=gen) for _ in range(3))
        v = torch.rand(n, device=dev, generator=gen)
        keep.append((p, g, m, v))
        d.p, d.g, d.m, d.v, d.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n
        d.step_size, d.bc2_sqrt = -1e-3 / (1 - 0.9 ** 7), (1 - 0.999 ** 7) ** 0.5
    hyper = engine.AdamHyperT(1 - 0.9, 0.999, 1 - 0.999, 1e-8, 0.0)
    stream = engine._stream(dev)

    def run(name):
        rc = libs[name].lgcn_adam_step(table, len(sizes), ctypes.byref(hyper), stream)
        assert rc == 0, rc
    for name in libs:
        for _ in range(args.warmup):
            run(name)
    res = summary(timed_blocks(list(libs), run, args.blocks, args.steps_per_block))
    nbytes = 7 * 4 * sum(sizes)
    res.update(config=cfg["name"], elements=sum(sizes), bytes_per_step=nbytes,
               loaded=os.path.relpath(os.environ.get("LGCN_LIB") or engine.LIB_PATH, ROOT),
               ab=os.path.relpath(os.path.abspath(args.ab_lib), ROOT),
               fraction_of_8TBps={k: round(nbytes / (v * 1e-3) / HBM_PEAK, 3)
                                  for k, v in res["median_ms"].items()},
               what="lgcn_adam_step alone from two builds of the library, alternating blocks, "
                    "events on the current stream")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--gen", default="powerlaw", choices=["powerlaw", "uniform"])
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps-per-block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ab-lib", default=None, help="time lgcn_adam_step of this build of the "
                                                   "library against the loaded one, nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    engine.load_library()
    cfg = bench.CONFIGS[args.config]
    if args.ab_lib:
        return ab_libs(args, cfg, dev)
    U, I, d, K = cfg["users"], cfg["items"], cfg["d"], cfg["K"]
    gen = torch.Generator().manual_seed(42)
    emb_host = [bench.xavier(U, d, gen), bench.xavier(I, d, gen)]
    r, c, v = bench.make_graph(dict(cfg, brands=0), args.gen, 16)[:3]
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((r, c))), torch.from_numpy(v),
                                  (U + I, U + I)).to(dev)
    nnz = len(v)
    del r, c, v
    names = [name for name, _ in OPTIMIZERS]
    models = {name: make_model(emb_host, U, I, d, K, dev) for name in names}
    opts = {name: make(models[name].parameters()) for name, make in OPTIMIZERS}
    rng = np.random.default_rng(0)
    n_batches = max(args.blocks * args.steps_per_block, args.warmup)
    batches = [tuple(torch.from_numpy(rng.integers(0, hi, args.batch)) for hi in (U, I, I))
               for _ in range(n_batches)]
    it = {name: 0 for name in names}

    def whole_step(name):
        b = batches[it[name] % n_batches]
        it[name] += 1
        users, pos, neg = (t.to(dev) for t in b)
        opts[name].zero_grad()
        loss = models[name].bpr_step(adj, users, pos, neg, LAMBDA)
        loss.backward()
        opts[name].step()
        return loss.item()

    for name in names:
        for _ in range(args.warmup):
            whole_step(name)
    whole = timed_blocks(names, whole_step, args.blocks, args.steps_per_block)
    bench.log("[adam_bench] whole steps done")
    # the optimizer alone, on the gradients the last batch left (the same bits in every model
    # whose parameters are still the same bits)
    alone = timed_blocks(names, lambda name: opts[name].step(), args.blocks, args.steps_per_block)
    bench.log("[adam_bench] optimizer steps done")

    elements = sum(p.numel() for p in models["engine"].parameters() if p.grad is not None)
    nbytes = 7 * 4 * elements
    result = {"config": cfg["name"], "nnz": nnz, "d": d, "K": K, "batch": args.batch,
              "blocks": args.blocks, "steps_per_block": args.steps_per_block,
              "elements": elements, "bytes_per_step": nbytes,
              "optimizer_step": summary(alone), "training_step": summary(whole)}
    med, spread = result["optimizer_step"]["median_ms"], result["optimizer_step"]["spread_ms"]
    result["fraction_of_8TBps"] = {k: round(nbytes / (v * 1e-3) / HBM_PEAK, 3)
                                   for k, v in med.items()}
    result["engine_over_torch_default"] = round(med["engine"] / med["torch_default"], 3)
    result["engine_over_torch_fused"] = round(med["engine"] / med["torch_fused"], 3)
    noise = max(spread["engine"], spread["torch_default"])
    result["gate"] = {"engine_below_torch_default_by_ms": round(med["torch_default"]
                                                                - med["engine"], 3),
                      "larger_spread_ms": noise,
                      "passed": med["torch_default"] - med["engine"] > noise}
    pa, pb, pf = (dict(models[k].named_parameters())
                  for k in ("engine", "torch_default", "torch_fused"))
    result["parameters_bit_equal_after_run"] = all(bits_equal(pa[k], pb[k]) for k in pa)
    result["torch_fused_bit_equal_to_default"] = all(bits_equal(pf[k], pb[k]) for k in pb)
    result["what"] = ("optimizer_step = opt.step() alone between events on the current stream, "
                      "training_step = batch upload, model.bpr_step, backward, opt.step(), "
                      "loss.item(); per-step time of alternating blocks, median over the blocks, "
                      "spread = max - min of the blocks; torch_default = torch.optim.Adam(lr), "
                      "torch_fused = fused=True, engine = optim.Adam")
    print(json.dumps(result), flush=True)
    assert result["parameters_bit_equal_after_run"], "optim.Adam left torch default's bits"
    if not result["gate"]["passed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
