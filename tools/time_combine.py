"""Combine timing: the typed combine (ops.combine_any, csrc/fql_routing.h) against the chain it replaces on 16-bit
activations, in one process, the contenders alternated after warm-up, device events around batches of calls, medians:
  fwd_typed      ops.combine_any(y, pos, w)                                   one launch, bfloat16 in and out
  fwd_chain      ops.combine(y.float(), pos, w).to(bfloat16)                  widen pass, float32 combine, rounding pass
  bwd_typed      ops.combine_any_backward(g, y, pos, w)                       one launch
  bwd_chain      torch autograd of the chain (graph built once outside the timed window; backward only)
  *_add          the same four with a shared expert's rows: the addend argument of the typed op, against the chain plus a
                 torch add (`+ s.float()` in front of the rounding pass)
Shapes: T=512 k=2 H=4096 and T=4096 k=8 H=4096, bfloat16.  Prints one JSON line per shape (median microseconds per call and
the ratios); --out appends them to a file.  These are times per call as a user pays them, launch and host cost included."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

SHAPES = [(512, 2, 4096), (4096, 8, 4096)]
DT = torch.bfloat16


def chain(y, pos, w, s=None):
    out = ops.combine(y.float(), pos, w)
    if s is not None:
        out = out + s.float()
    return out.to(DT)


def time_shape(T, k, H, iters, warmup, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(T + k)
    y = torch.randn(T * k, H, device=dev, generator=g).to(DT)
    s = torch.randn(T, H, device=dev, generator=g).to(DT)
    grad = torch.randn(T, H, device=dev, generator=g).to(DT)
    w = torch.rand(T, k, device=dev, generator=g)
    pos = torch.randperm(T * k, device=dev, generator=g).to(torch.int32)
    leaves = [t.clone().requires_grad_(True) for t in (y, w, s)]
    graph = chain(leaves[0], pos, leaves[1])
    graph_add = chain(leaves[0], pos, leaves[1], leaves[2])
    runs = {
        "fwd_typed": lambda: ops.combine_any(y, pos, w),
        "fwd_chain": lambda: chain(y, pos, w),
        "bwd_typed": lambda: ops.combine_any_backward(grad, y, pos, w),
        "bwd_chain": lambda: torch.autograd.grad(graph, leaves[:2], grad, retain_graph=True),
        "fwd_typed_add": lambda: ops.combine_any(y, pos, w, addend=s),
        "fwd_chain_add": lambda: chain(y, pos, w, s),
        "bwd_typed_add": lambda: ops.combine_any_backward(grad, y, pos, w, addend=s),
        "bwd_chain_add": lambda: torch.autograd.grad(graph_add, leaves, grad, retain_graph=True),
    }
    times = {name: [] for name in runs}
    with torch.no_grad():
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
    ratios = {f"{p}{sfx}_chain_over_typed": round(med[f"{p}_chain{sfx}"] / med[f"{p}_typed{sfx}"], 2)
              for p in ("fwd", "bwd") for sfx in ("", "_add")}
    return {"shape": f"T={T} k={k} H={H} bf16", "median_us": med, **ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into the shapes: that one only (for a kernel-trace run)")
    a = ap.parse_args()
    shapes = SHAPES if a.shape is None else [SHAPES[a.shape]]
    lines = [json.dumps(time_shape(T, k, H, a.iters, a.warmup, a.reps)) for T, k, H in shapes]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
