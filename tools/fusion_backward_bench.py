#!/usr/bin/env python
"""Time fusion.FusionPreLayer.backward two ways in one process: fusion.BACKWARD = "torch" (the
torch expression: torch.where, three library GEMMs, cat, sum) and "kernel"
(lgcn_fusion_prelayer_backward), at the C5 pre-layer shape (bench.py's C5 item count, d = 128,
C = 64, tables built as bench.py builds them) and at (64, 64) with the same row count.

  * the backward alone: torch.autograd.grad through a retained FusionPreLayer node, so a call is
    FusionPreLayer.backward and its allocations, nothing else;
  * alternating blocks of the two routes, every call bracketed by events on the current stream,
    the median per block, then the median over the blocks; `spread_ms` is max - min of the torch
    route's block medians (what a difference between the routes has to exceed to mean anything);
  * peak allocated memory above what is resident before the call, per route
    (torch.cuda.max_memory_allocated);
  * the gradients of the two routes are compared: d_id bitwise is not expected (the BLAS picks its
    order), so the largest difference relative to the largest magnitude is reported.

Prints one JSON line on stdout (progress goes to stderr).

    python tools/fusion_backward_bench.py [--rows N] [--blocks 5] [--calls-per-block 4]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, xavier: the tables bench.py times)
from gcn_recommendation_amd import engine, fusion  # noqa: E402

SLOPE = 0.01  # F.leaky_relu's default, what the model uses
ROUTES = ("torch", "kernel")


def time_shape(rows, d, c, args, dev):
    gen = torch.Generator().manual_seed(42)
    id_w = bench.xavier(rows, d, gen).to(dev).requires_grad_()
    content = torch.from_numpy(np.random.default_rng(5).standard_normal(
        (rows, c)).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    lin = torch.nn.Linear(d + c, d).to(dev)
    out = fusion.FusionPreLayer.apply(id_w, content, lin.weight, lin.bias, SLOPE)
    g_out = torch.randn(rows, d, generator=torch.Generator().manual_seed(1)).to(dev)
    wrt = (id_w, lin.weight, lin.bias)

    def call(route):
        fusion.BACKWARD = route
        return torch.autograd.grad(out, wrt, g_out, retain_graph=True)

    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    saved = fusion.BACKWARD
    try:
        grads, peak = {}, {}
        for route in ROUTES:   # warm-up, the gradients and the peak memory of one call
            for _ in range(args.warmup):
                call(route)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            grads[route] = call(route)
            torch.cuda.synchronize()
            peak[route] = torch.cuda.max_memory_allocated(dev) - base
        diff = {}
        for name, gt, gk in zip(("d_id", "d_w", "d_b"), grads["torch"], grads["kernel"]):
            diff[name] = float((gt - gk).abs().max() / gt.abs().max())
        del grads
        per_block = {r: [] for r in ROUTES}
        for _ in range(args.blocks):
            for route in ROUTES:
                times = []
                for _ in range(args.calls_per_block):
                    torch.cuda.synchronize()
                    a.record()
                    g = call(route)
                    e.record()
                    torch.cuda.synchronize()
                    times.append(a.elapsed_time(e))
                    del g
                per_block[route].append(float(np.median(times)))
    finally:
        fusion.BACKWARD = saved
    med = {r: float(np.median(per_block[r])) for r in ROUTES}
    flop = 2.0 * rows * d * d + 2.0 * rows * d * (d + c)
    return {
        "rows": rows, "d": d, "c_dim": c, "gflop": round(flop / 1e9, 1),
        "ms": {r: round(med[r], 3) for r in ROUTES},
        "block_medians_ms": {r: [round(x, 3) for x in per_block[r]] for r in ROUTES},
        "spread_ms": round(float(np.ptp(per_block["torch"])), 3),
        "gain_ms": round(med["torch"] - med["kernel"], 3),
        "tflops": {r: round(flop / med[r] / 1e9, 1) for r in ROUTES},
        "peak_bytes_above_resident": peak,
        "max_abs_diff_over_max_abs": diff,
        "scratch_bytes": int(engine.load_library().lgcn_fusion_prelayer_backward_scratch_bytes(
            rows, d, c)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=bench.CONFIGS["c5"]["items"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls-per-block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fusion_backward_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    engine.load_library()
    result = {"blocks": args.blocks, "calls_per_block": args.calls_per_block, "slope": SLOPE,
              "chunk_rows": engine.FUSION_BWD_CHUNK, "default_route": fusion.BACKWARD,
              "shapes": []}
    for d, c in ((128, 64), (64, 64)):
        result["shapes"].append(time_shape(args.rows, d, c, args, dev))
        bench.log(f"[fusion_backward_bench] ({d}, {c}) done: {result['shapes'][-1]['ms']}")
        torch.cuda.empty_cache()
    result["what"] = ("FusionPreLayer.backward alone (autograd.grad through a retained node, all "
                      "three gradients), events on the current stream, median per block of calls "
                      "then over alternating blocks; spread_ms = max - min of the torch route's "
                      "block medians; tflops = (2 I d d + 2 I d (d + C)) / time")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
