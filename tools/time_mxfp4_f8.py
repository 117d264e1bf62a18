#!/usr/bin/env python3
"""Time the fp8 mode of the MXFP4 grouped ops (csrc/fql_gemm_mx4_scaled.h: the block-scaled fp4 x fp8 matrix-core kernel and
its quantising pre-pass) against the bfloat16-path op of the same shape in the same job.

The four shapes of DESIGN.md section 25, 1024 routed rows spread evenly: the gpt-oss-like ones (32 experts, 2880 -> 5760
plain and 2880 -> 2880 gated) and the headline ones (8 experts, 4096 -> 11008, plain and gated).  Per shape the forms are:
the bfloat16 path (ops.moe_forward_mxfp4 / ops.moe_gated_forward_mxfp4 as they are), e4m3 rows in
(ops.moe_forward_mxfp4_fp8: the GEMM alone), and float rows in or gated (precision="fp8": pre-pass + GEMM).  Method of
tools/time_mxfp4.py: each variant is a hipGraph of 16 calls over rotating weight sets, the variants are replayed alternately,
and the median of --repeats windows of 5 replays is printed with its spread."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="type of the float rows")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
rows_dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32


def shape(name, E, K, N, gated):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    mx = []
    for _ in range(a.sets):
        mx.append((torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                   torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)))
    xr = torch.randn(T, 2 * K if gated else K, device=dev, generator=g).to(rows_dt)
    x8, act = ops.quantize_activations_fp8(xr[:, :K])
    x8, act = x8.contiguous(), act.contiguous()

    if gated:
        variants = {
            "bf16 path, gated": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], xr, tpe, offs),
            "fp8, gated (pre-pass + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp8"),
            "fp8, e4m3 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp8(*mx[i], x8, act, tpe, offs, out_dtype=rows_dt),
        }
    else:
        variants = {
            "bf16 path": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs),
            "fp8, float rows in (pre-pass + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp8"),
            "fp8, e4m3 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp8(*mx[i], x8, act, tpe, offs, out_dtype=rows_dt),
        }
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st), torch.no_grad():
        for v, fn in variants.items():
            for i in range(min(2, a.sets)):
                fn(i)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(16):
                    fn(i % a.sets)
            gr.replay()
            graphs[v] = gr
    times = {v: [] for v in variants}
    for _ in range(a.repeats):
        for v in variants:                                      # alternating: the variants share whatever else happens
            with torch.cuda.stream(st):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(5):
                    graphs[v].replay()
                e1.record(st)
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / 80 * 1e3)
    print(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert) {'gated' if gated else 'plain'}, float rows {a.dtype}", flush=True)
    wbytes = E * N * K // 2
    base = None
    for v in variants:
        us = statistics.median(times[v])
        base = us if base is None else base
        print(f"  {v:38s} {us:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]   {base / us:5.2f} x the bf16 path   "
              f"{wbytes / us / 1e6:6.2f} TB/s of 4-bit weights   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s", flush=True)
    del mx
    torch.cuda.empty_cache()


shape("gpt-oss-like gate|up", 32, 2880, 5760, False)
shape("gpt-oss-like down", 32, 2880, 2880, True)
shape("headline", 8, 4096, 11008, False)
shape("headline gated", 8, 4096, 11008, True)
