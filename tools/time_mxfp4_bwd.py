#!/usr/bin/env python3
"""Time the input gradient of the MXFP4 grouped GEMM (ops.moe_backward_input_mxfp4) against two yardsticks from the same job:
a per-expert loop of torch.matmul(gy_e, W_e) on pre-dequantised bfloat16 weights, and ops.moe_backward_input on per-group
INT4 weights with group_size = 32 (the float32 matrix-core kernel of csrc/fql_group_bwd.h), the closest thing the project
had before.

Three shapes, 1024 routed rows spread evenly: the two gpt-oss-like ones (32 experts; N = 2880, K = 2880, the down
projection, and N = 5760, K = 2880, gate|up) and the headline one (8 experts, K = 4096, N = 11008).  N is the contraction:
grad_out is [T, N], the result [T, K].  Method of tools/time_mxfp4.py: each variant is a hipGraph of
16 calls over rotating weight sets (so no set is resident in the caches from the call before), the variants are replayed
alternately, and the median of --repeats windows of 5 replays is printed with its spread.  The report goes to stdout and to
--out (profiles/mxfp4_bwd_timing.txt)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fused_int4_amd import ops
from fused_int4_amd.quantize import dequantize_mxfp4

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="type of grad_out and of the result")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_bwd_timing.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
rows_dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def shape(name, E, K, N):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    mx, i4, bf = [], [], []
    for _ in range(a.sets):
        blocks = torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        scales = torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)
        mx.append((blocks, scales))
        bf.append(torch.stack([dequantize_mxfp4(blocks[e], scales[e]).bfloat16() for e in range(E)]))
        i4.append((torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                   torch.full((E, N, K // 32), 0.01, device=dev), torch.full((E, N, K // 32), 8.0, device=dev)))
    gy32 = torch.randn(T, N, device=dev, generator=g)
    gyr = gy32.to(rows_dt)
    gy16 = gy32.bfloat16()

    variants = {
        "mxfp4 (this kernel)": lambda i: ops.moe_backward_input_mxfp4(*mx[i], gyr, tpe, offs, out_dtype=rows_dt),
        "int4 per-group 32": lambda i: ops.moe_backward_input(*i4[i], gyr, tpe, offs, out_dtype=rows_dt),
        "torch bf16 matmul loop": lambda i: torch.cat([gy16[e * m:(e + 1) * m] @ bf[i][e] for e in range(E)]),
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
    say(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert), grad_out and result {a.dtype}")
    wbytes = E * N * K // 2
    for v in variants:
        us = statistics.median(times[v])
        say(f"  {v:24s} {us:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]   "
            f"{wbytes / us / 1e6:6.2f} TB/s of 4-bit weights   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s")
    del mx, i4, bf
    torch.cuda.empty_cache()


shape("gpt-oss-like down", 32, 2880, 2880)
shape("gpt-oss-like gate|up", 32, 2880, 5760)
shape("headline", 8, 4096, 11008)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(report) + "\n")
