"""Plan timing: fql_route_plan_i32 against fql_route_plan_capped_i32 (csrc/fql_routing.h), in one process, the contenders
alternated after warm-up, device events around batches of calls, median and spread over the batches:
  plan            ops.route_plan(indices, E)                                   the baseline kernel
  capped_off      ops.route_plan_capped(indices, E)                            no capacity, no mask: the same outputs
  capped_cf1      ops.route_plan_capped(indices, E, ceil(n_slots / E))         capacity_factor 1.0
  capped_cf1_mask the same with a token mask (three tokens in four real)
Shapes: E=8 at 2048 slots (T=1024, top-2: the routed rows of the headline step) and E=128 at 65536 slots (T=8192, top-8),
uniformly random expert ids.  Prints one JSON line per shape: median microseconds per call, the spread of the batch means
(min, max, and the interquartile range) and the ratios to the baseline; --out appends them to a file.  These are times
per call as a user pays them, launch and host cost (the output allocations among it) included; the kernels' own times
are in a kernel trace, taken in a run of its own."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

SHAPES = [(1024, 2, 8), (8192, 8, 128)]


def time_shape(T, k, E, iters, warmup, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(T + E)
    idx = torch.randint(0, E, (T, k), device=dev, generator=g, dtype=torch.int32)
    mask = torch.rand(T, device=dev, generator=g) < 0.75
    cap = math.ceil(T * k / E)
    runs = {
        "plan": lambda: ops.route_plan(idx, E),
        "capped_off": lambda: ops.route_plan_capped(idx, E),
        "capped_cf1": lambda: ops.route_plan_capped(idx, E, cap),
        "capped_cf1_mask": lambda: ops.route_plan_capped(idx, E, cap, mask),
    }
    for a, b in zip(runs["plan"](), runs["capped_off"]()):       # faster and different is not faster
        assert torch.equal(a, b)
    times = {name: [] for name in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(iters):
        for name, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / reps)
    med = {name: round(statistics.median(v), 2) for name, v in times.items()}
    spread = {}
    for name, v in times.items():
        q = statistics.quantiles(v, n=4)
        spread[name] = {"min": round(min(v), 2), "max": round(max(v), 2), "iqr": round(q[2] - q[0], 2)}
    ratios = {f"{name}_over_plan": round(med[name] / med["plan"], 3) for name in runs if name != "plan"}
    return {"shape": f"T={T} top_k={k} E={E} slots={T * k}", "median_us": med, "spread_us": spread, **ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40, help="timed batches per contender")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="calls per batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_route_plan.py needs the GPU: a CPU run cannot give a time")
    for T, k, E in SHAPES:
        line = json.dumps(time_shape(T, k, E, args.iters, args.warmup, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
