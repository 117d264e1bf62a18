"""Activation kinds of the gated FFN experts: the fused ops against the chains they replace, in one process, the
contenders alternated after warm-up, device events around windows of back-to-back calls, medians (as tools/time_combine.py).
At the headline's second projection, E = 8 experts, T = 1024 routed rows, F = 11008 -> H = 4096, float32 and bfloat16, for
each kind (silu, gelu_tanh, swiglu_clamp):
  fwd_fused      ops.moe_gated_forward(down, gate_up, activation=kind)        h formed in the GEMM's pre-pass, never stored
  fwd_chain      torch builds h [T, F] from gate_up, then ops.moe_forward / moe_forward_any(down, h)
  bwd_fused      ops.glu_backward(gate_up, dh, activation=kind)               one streaming kernel
  bwd_chain      torch autograd of the same expression (graph built once outside the timed window; backward only)
Prints one JSON line per element type (median microseconds per call, chain / fused ratios, and each new kind over silu);
--out appends them to a file.  These are times per call as a user pays them, launch and host cost included."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

KINDS = ("silu", "gelu_tanh", "swiglu_clamp")
ALPHA, LIMIT = 1.702, 7.0


def hidden(kind, gate_up):
    F = gate_up.shape[1] // 2
    g, u = gate_up[:, :F], gate_up[:, F:]
    if kind == "silu":
        return torch.nn.functional.silu(g) * u
    if kind == "gelu_tanh":
        return torch.nn.functional.gelu(g, approximate="tanh") * u
    gp = g.clamp(max=LIMIT)
    return gp * torch.sigmoid(ALPHA * gp) * (u.clamp(-LIMIT, LIMIT) + 1.0)


def time_dtype(dt, E, T, F, H, iters, warmup, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(F)
    packed = torch.randint(0, 256, (E, H, F // 2), dtype=torch.uint8, device=dev, generator=g)
    scales = torch.rand(E, H, device=dev, generator=g) * 0.02 + 0.002
    zps = torch.randint(0, 16, (E, H), device=dev, generator=g).float()
    tpe = torch.full((E,), T // E, dtype=torch.int32, device=dev)
    offs = (torch.cumsum(tpe, 0, dtype=torch.int32) - tpe).to(torch.int32)
    gate_up = (2.0 * torch.randn(T, 2 * F, device=dev, generator=g)).to(dt)
    dh = torch.randn(T, F, device=dev, generator=g).to(dt)
    kw = {k: dict(activation=k, activation_alpha=ALPHA, activation_limit=LIMIT) for k in KINDS}
    leaf = gate_up.clone().requires_grad_(True)
    graphs = {k: hidden(k, leaf) for k in KINDS}
    fwd = ops.moe_forward if dt == torch.float32 else ops.moe_forward_any
    runs = {}
    for k in KINDS:
        runs[f"fwd_fused_{k}"] = lambda k=k: ops.moe_gated_forward(packed, scales, zps, gate_up, tpe, offs, **kw[k])
        runs[f"fwd_chain_{k}"] = lambda k=k: fwd(packed, scales, zps, hidden(k, gate_up), None, tpe, offs)
        runs[f"bwd_fused_{k}"] = lambda k=k: ops.glu_backward(gate_up, dh, **kw[k])
        runs[f"bwd_chain_{k}"] = lambda k=k: torch.autograd.grad(graphs[k], [leaf], dh, retain_graph=True)
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
    lo_hi = {name: [round(min(v), 2), round(max(v), 2)] for name, v in times.items() if name.endswith("_silu")}
    ratios = {f"{p}_chain_over_fused_{k}": round(med[f"{p}_chain_{k}"] / med[f"{p}_fused_{k}"], 2)
              for p in ("fwd", "bwd") for k in KINDS}
    over = {f"{p}_fused_{k}_over_silu": round(med[f"{p}_fused_{k}"] / med[f"{p}_fused_silu"], 3)
            for p in ("fwd", "bwd") for k in KINDS[1:]}
    return {"shape": f"E={E} T={T} F={F} H={H} {str(dt).replace('torch.', '')}", "median_us": med, "silu_min_max_us": lo_hi,
            **ratios, **over}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--ffn", type=int, default=11008)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(time_dtype(dt, a.experts, a.rows, a.ffn, a.hidden, a.iters, a.warmup, a.reps))
             for dt in (torch.float32, torch.bfloat16)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
