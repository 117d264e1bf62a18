"""Scored-router timing: ops.router_score_topk (csrc/fql_router.h) against the torch chain it replaces, in one
process, the contenders alternated after warm-up, device events around batches of calls, medians:
  fwd_fused   ops.router_score_topk(...)                                     one launch
  fwd_torch   the Hugging Face DeepSeek-V3 chain: sigmoid, add, view, topk, sum, topk, scatter, mask, topk, gather, sum,
              div, mul (no groups: sigmoid, topk, gather, sum, div, mul), then to(int32)
  bwd_fused   ops.router_score_topk_backward(logits, indices, grad_weights, None, ...)   one launch
  bwd_torch   torch autograd of the chain (the graph is built once, outside the timed window; backward only)
Shapes: T=4096 E=128 k=8 n_group=8 topk_group=4, sigmoid + bias, scale 2.5 (DeepSeek-V3-like) and T=512 E=64 k=6 without
groups or bias (sigmoid, scale 1); float32 logits.
Prints one JSON line per shape (median microseconds per call and the ratios); --out appends them to a file.  These are
times per call as a user pays them, launch and host cost included."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

# (T, E, k, n_group, topk_group, bias?, scale)
SHAPES = [(4096, 128, 8, 8, 4, True, 2.5), (512, 64, 6, 1, 1, False, 1.0)]


def torch_chain(logits, k, n_group, topk_group, bias, scale):
    scores = torch.sigmoid(logits)
    choice = scores if bias is None else scores + bias
    if n_group > 1:
        T, E = scores.shape
        group_scores = choice.view(T, n_group, E // n_group).topk(2, dim=-1)[0].sum(dim=-1)
        group_idx = torch.topk(group_scores, topk_group, dim=-1, sorted=False)[1]
        group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1.0)
        mask = group_mask.unsqueeze(-1).expand(T, n_group, E // n_group).reshape(T, E)
        choice = choice.masked_fill(~mask.bool(), 0.0)
    idx = torch.topk(choice, k, dim=-1, sorted=False)[1]
    w = scores.gather(1, idx)
    w = w / (w.sum(dim=-1, keepdim=True) + 1e-20)
    return w * scale, idx.to(torch.int32)


def time_shape(T, E, k, n_group, topk_group, with_bias, scale, iters, warmup, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(T + E)
    logits = torch.randn(T, E, device=dev, generator=g)
    gw = torch.randn(T, k, device=dev, generator=g)
    bias = (torch.rand(E, device=dev, generator=g) * 0.2) if with_bias else None
    args = ("sigmoid", bias, n_group, topk_group, 2, True, scale)
    _, idx = ops.router_score_topk(logits, k, *args)
    leaf = logits.clone().requires_grad_(True)
    w_graph, _ = torch_chain(leaf, k, n_group, topk_group, bias, scale)
    runs = {
        "fwd_fused": lambda: ops.router_score_topk(logits, k, *args),
        "fwd_torch": lambda: torch_chain(logits, k, n_group, topk_group, bias, scale),
        "bwd_fused": lambda: ops.router_score_topk_backward(logits, idx, gw, None, "sigmoid", True, scale),
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
    return {"shape": f"T={T} E={E} k={k} n_group={n_group} topk_group={topk_group} sigmoid bias={with_bias} scale={scale}",
            "median_us": med, "fwd_torch_over_fused": round(med["fwd_torch"] / med["fwd_fused"], 2),
            "bwd_torch_over_fused": round(med["bwd_torch"] / med["bwd_fused"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into the shapes: that one only")
    a = ap.parse_args()
    shapes = SHAPES if a.shape is None else [SHAPES[a.shape]]
    lines = [json.dumps(time_shape(*s, a.iters, a.warmup, a.reps)) for s in shapes]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
