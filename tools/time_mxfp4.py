#!/usr/bin/env python3
"""Time the two MXFP4 grouped ops (ops.moe_forward_mxfp4, ops.moe_gated_forward_mxfp4) against two yardsticks from the same
job: the per-row INT4 exact path (ops.moe_forward / ops.moe_gated_forward on float32 rows) and a per-expert loop of
torch.matmul on bfloat16-dequantised weights (the gated form with h = silu(g) * u formed by torch in bfloat16 first).

Two shapes, 1024 routed rows spread evenly: the gpt-oss-like one (32 experts, 2880 -> 5760 for the plain op and
2880 -> 2880 for the gated one) and the headline one (8 experts, 4096 -> 11008, both ops).  Method of DESIGN.md section 24:
each variant is a hipGraph of 16 calls over rotating weight sets (so no set is resident in the caches from the call before),
the variants are replayed alternately, and the median of --repeats windows of 5 replays is printed with its spread."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as Fn
from fused_int4_amd import ops
from fused_int4_amd.quantize import dequantize_mxfp4

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="row type of the MXFP4 calls")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
rows_dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32


def shape(name, E, K, N, gated):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    eid = torch.arange(E, device=dev, dtype=torch.int32).repeat_interleave(m)
    mx, i4, bf = [], [], []
    for _ in range(a.sets):
        blocks = torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        scales = torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)
        mx.append((blocks, scales))
        bf.append(torch.stack([dequantize_mxfp4(blocks[e], scales[e]).bfloat16() for e in range(E)]))
        i4.append((torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                   torch.full((E, N), 0.01, device=dev), torch.full((E, N), 8.0, device=dev)))
    x32 = torch.randn(T, 2 * K if gated else K, device=dev, generator=g)
    xr = x32.to(rows_dt)
    x16 = x32.bfloat16()

    def torch_loop(w):
        h = Fn.silu(x16[:, :K]) * x16[:, K:] if gated else x16
        return torch.cat([h[e * m:(e + 1) * m] @ w[e].T for e in range(E)])

    variants = {
        "mxfp4 (this kernel)": lambda i: (ops.moe_gated_forward_mxfp4(*mx[i], xr, tpe, offs) if gated
                                          else ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs)),
        "int4 per-row exact": lambda i: (ops.moe_gated_forward(*i4[i], x32, tpe, offs, precision="exact") if gated
                                         else ops.moe_forward(*i4[i], x32, eid, tpe, offs, precision="exact")),
        "torch bf16 matmul loop": lambda i: torch_loop(bf[i]),
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
    print(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert) {'gated' if gated else 'plain'}, mxfp4 rows {a.dtype}", flush=True)
    wbytes = E * N * K // 2
    for v in variants:
        us = statistics.median(times[v])
        print(f"  {v:24s} {us:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]   "
              f"{wbytes / us / 1e6:6.2f} TB/s of 4-bit weights   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s", flush=True)
    del mx, i4, bf
    torch.cuda.empty_cache()


shape("gpt-oss-like gate|up", 32, 2880, 5760, False)
shape("gpt-oss-like down", 32, 2880, 2880, True)
shape("headline", 8, 4096, 11008, False)
shape("headline gated", 8, 4096, 11008, True)
