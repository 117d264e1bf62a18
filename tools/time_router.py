"""Router timing: the fused top-k router (ops.router_topk, csrc/fql_router.h) against the torch chain it replaces, in one
process, the contenders alternated after warm-up, device events around batches of calls, medians:
  fwd_fused   ops.router_topk(logits, k)                                     one launch
  fwd_torch   softmax -> topk -> sum -> div -> to(int32)                     (routing.simulate_routing's chain)
  bwd_fused   ops.router_topk_backward(logits, indices, grad_weights, None)  one launch
  bwd_torch   torch autograd of the chain (the graph is built once, outside the timed window; backward only)
Shapes: T=512 E=8 k=2 (the headline's routing), T=4096 E=64 k=8, T=4096 E=128 k=2; float32 logits.
Prints one JSON line per shape (median microseconds per call and the ratios); --out appends them to a file.  These are
times per call as a user pays them, launch and host cost included; for the kernels' own durations run one shape under
`rocprofv3 --kernel-trace --stats -- python tools/time_router.py --shape I` (profiles/router_timing.txt has both)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

SHAPES = [(512, 8, 2), (4096, 64, 8), (4096, 128, 2)]


def torch_chain(logits, k):
    probs = torch.softmax(logits, dim=-1)
    w, idx = torch.topk(probs, k, dim=-1)
    w = w / w.sum(dim=-1, keepdim=True)
    return w, idx.to(torch.int32)


def time_shape(T, E, k, iters, warmup, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(T + E)
    logits = torch.randn(T, E, device=dev, generator=g)
    gw = torch.randn(T, k, device=dev, generator=g)
    _, idx = ops.router_topk(logits, k)
    leaf = logits.clone().requires_grad_(True)
    w_graph, _ = torch_chain(leaf, k)
    runs = {
        "fwd_fused": lambda: ops.router_topk(logits, k),
        "fwd_torch": lambda: torch_chain(logits, k),
        "bwd_fused": lambda: ops.router_topk_backward(logits, idx, gw, None),
        "bwd_torch": lambda: torch.autograd.grad(w_graph, leaf, gw, retain_graph=True),
    }
    times = {name: [] for name in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(iters):
        for name, f in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / reps)
    med = {name: round(statistics.median(v), 2) for name, v in times.items()}
    return {"shape": f"T={T} E={E} k={k}", "median_us": med,
            "fwd_torch_over_fused": round(med["fwd_torch"] / med["fwd_fused"], 2),
            "bwd_torch_over_fused": round(med["bwd_torch"] / med["bwd_fused"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into the shapes: that one only (for a kernel-trace run)")
    a = ap.parse_args()
    shapes = SHAPES if a.shape is None else [SHAPES[a.shape]]
    lines = [json.dumps(time_shape(T, E, k, a.iters, a.warmup, a.reps)) for T, E, k in shapes]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
