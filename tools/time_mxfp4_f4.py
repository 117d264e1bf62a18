#!/usr/bin/env python3
"""Time the fp4 mode of the MXFP4 grouped ops (csrc/fql_gemm_mx4_scaled.h: the block-scaled fp4 x fp4 matrix-core kernel and
its MXFP4 quantiser) against the fp8 mode and the bfloat16 path of the same shape in the same job.

The four shapes of DESIGN.md section 27's table, 1024 routed rows spread evenly: the gpt-oss-like ones (32 experts,
2880 -> 5760 and 2880 -> 2880) and the headline one (8 experts, 4096 -> 11008) at both of its uses.  Every shape is timed in
three forms for each of fp4 and fp8 -- rows already quantised (the GEMM alone), float rows in (quantiser + GEMM) and gated
(gate_up [T, 2K] in) -- beside the two bfloat16-path ops.  Method of tools/time_mxfp4_f8.py: each variant is a hipGraph of 16
calls over rotating weight sets, the variants are replayed alternately, and the median of --repeats windows of 5 replays
is printed with its spread."""
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


def shape(name, E, K, N):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    mx = []
    for _ in range(a.sets):
        mx.append((torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                   torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)))
    gu = torch.randn(T, 2 * K, device=dev, generator=g).to(rows_dt)
    xr = gu[:, :K].contiguous()
    x8, act = ops.quantize_activations_fp8(xr)
    x8, act = x8.contiguous(), act.contiguous()
    x4, xs4 = ops.quantize_rows_mxfp4(xr)

    variants = {
        "bf16 path": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs),
        "fp8, e4m3 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp8(*mx[i], x8, act, tpe, offs, out_dtype=rows_dt),
        "fp4, MXFP4 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp4(*mx[i], x4, xs4, tpe, offs, out_dtype=rows_dt),
        "fp8, float rows in (pre-pass + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp8"),
        "fp4, float rows in (quantiser + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp4"),
        "bf16 path, gated": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs),
        "fp8, gated (pre-pass + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs, precision="fp8"),
        "fp4, gated (quantiser + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs, precision="fp4"),
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
    print(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert), float rows {a.dtype}", flush=True)
    wbytes = E * N * K // 2
    med = {v: statistics.median(times[v]) for v in variants}
    for v in variants:
        us = med[v]
        base = med["bf16 path, gated" if "gated" in v else "bf16 path"]
        fp8 = med.get(v.replace("fp4", "fp8").replace("MXFP4", "e4m3").replace("quantiser", "pre-pass")) if v.startswith("fp4") else None
        against8 = f"{fp8 / us:5.2f} x its fp8 form" if fp8 is not None else " " * 19
        print(f"  {v:38s} {us:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]   {base / us:5.2f} x the bf16 path   "
              f"{against8}   {wbytes / us / 1e6:6.2f} TB/s of 4-bit weights   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s", flush=True)
    del mx
    torch.cuda.empty_cache()


shape("gpt-oss-like gate|up", 32, 2880, 5760)
shape("gpt-oss-like down", 32, 2880, 2880)
shape("headline", 8, 4096, 11008)
