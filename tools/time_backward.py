"""Backward timing at the headline MoE shape (8 experts, 1024 routed rows = 128 per expert, dY 11008 wide -> dX
4096 wide), one process, the four contenders alternated after warm-up, device events around each call:
  fwd        the forward grouped GEMM of the same flop count (x 4096 -> 11008 wide, ops.moe_forward)
  dx_fused   the fused input gradient (ops.moe_backward_input, csrc/fql_bwd.h)
  deq_f32    GPU dequantise of every expert + float32 torch.matmul per expert
  deq_bf16   GPU dequantise of every expert + bfloat16 torch.matmul per expert
Prints one JSON line (median microseconds per call, and the ratios)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fused_int4_amd as fq  # noqa: E402
from fused_int4_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=11008)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="run one contender only (profiling)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    E, T, K, N = a.experts, a.rows, a.hidden, a.ffn
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=g)
    S = torch.rand(E, N, device=dev, generator=g) * 0.01 + 1e-3
    Z = torch.randint(0, 16, (E, N), device=dev, generator=g).float()
    cnt = torch.full((E,), T // E, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
    cnt = cnt.to(dev)
    x = torch.randn(T, K, device=dev)
    gy = torch.randn(T, N, device=dev)
    bounds = [(e * (T // E), (e + 1) * (T // E)) for e in range(E)]

    def deq(dtype):
        out = torch.empty(T, K, device=dev, dtype=dtype)
        for e, (lo, hi) in enumerate(bounds):
            w = ops.dequantize_forward(P[e], S[e], Z[e]).to(dtype)
            torch.matmul(gy[lo:hi].to(dtype), w, out=out[lo:hi])
        return out

    runs = {
        "fwd": lambda: ops.moe_forward(P, S, Z, x, None, cnt, offs),
        "dx_fused": lambda: ops.moe_backward_input(P, S, Z, gy, cnt, offs),
        "deq_f32": lambda: deq(torch.float32),
        "deq_bf16": lambda: deq(torch.bfloat16),
    }
    if a.only:
        runs = {a.only: runs[a.only]}
    times = {k: [] for k in runs}
    with torch.no_grad():
        for _ in range(a.warmup):
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for k, f in runs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                e.synchronize()
                times[k].append(s.elapsed_time(e) * 1e3)
    med = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res = {"shape": f"E={E} rows={T} dY {N} -> dX {K}", "median_us": med}
    if "dx_fused" in med and "deq_f32" in med:
        res["deq_f32_over_fused"] = round(med["deq_f32"] / med["dx_fused"], 2)
    if "dx_fused" in med and "fwd" in med:
        res["fused_over_fwd"] = round(med["dx_fused"] / med["fwd"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
