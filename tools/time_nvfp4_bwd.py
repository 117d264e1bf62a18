#!/usr/bin/env python3
"""Time the input gradient of the NVFP4 grouped GEMM (ops.moe_backward_input_nvfp4) against two
yardsticks from the same job: a per-expert loop of torch.matmul(gy_e, W_e) on pre-dequantised bfloat16 weights, and
ops.moe_backward_input_mxfp4 on the same code bytes (the kernel this one was derived from: the ratio is the price of the
second scale byte and of the multiply in the conversion).

The two gpt-oss shapes, 32 experts, 1024 routed rows spread evenly, bfloat16 dY and dX: N = 2880, K = 2880 (the down
projection) and N = 5760, K = 2880 (gate|up).  N is the contraction: grad_out is [T, N], the result [T, K].  Method of
DESIGN.md section 29: each variant is a hipGraph of calls over rotating weight sets, as many as it takes for the bytes
touched between two uses of one set to exceed the 256 MiB Infinity Cache, a whole number of rotations a graph; the variants
are replayed alternately in the same job, and the median of --repeats windows of 5 replays is printed with the
window-to-window range.

Acceptance (DESIGN.md section 26's): the new kernel is faster than the torch loop at both shapes by more than the larger of
the two windows' ranges.  The report goes to stdout and to --out (profiles/nvfp4_bwd_timing.txt)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fused_int4_amd import ops
from fused_int4_amd.quantize import dequantize_nvfp4

MALL = 256 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--experts", type=int, default=32)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=6)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvfp4_bwd_timing.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def shape(name, E, K, N):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    touched = E * N * (K // 2 + K // 32)                        # the smallest of the three variants' weight bytes
    sets = min(max(2, -(-MALL // touched) + 1), a.max_sets)
    calls = sets * -(-16 // sets)                               # a whole number of rotations: a replay ends where the next begins
    nv, mx, bf = [], [], []
    for _ in range(sets):
        blocks = torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        nv.append((blocks, torch.randint(0x30, 0x48, (E, N, K // 16), device=dev, generator=g, dtype=torch.uint8),
                   torch.rand(E, device=dev, generator=g) + 0.5))
        mx.append((blocks, torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)))
        bf.append(torch.stack([(dequantize_nvfp4(blocks[e], nv[-1][1][e]) * nv[-1][2][e]).bfloat16() for e in range(E)]))
    gy = torch.randn(T, N, device=dev, generator=g).bfloat16()
    variants = {
        "nvfp4 (this kernel)": lambda i: ops.moe_backward_input_nvfp4(*nv[i], gy, tpe, offs, out_dtype=torch.bfloat16),
        "mxfp4 backward": lambda i: ops.moe_backward_input_mxfp4(*mx[i], gy, tpe, offs, out_dtype=torch.bfloat16),
        "torch bf16 matmul loop": lambda i: torch.cat([gy[e * m:(e + 1) * m] @ bf[i][e] for e in range(E)]),
    }
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st), torch.no_grad():
        for v, fn in variants.items():
            for i in range(2):
                fn(i)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(calls):
                    fn(i % sets)
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
            times[v].append(e0.elapsed_time(e1) / (5 * calls) * 1e3)
    res = {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}
    say(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert), grad_out and result bfloat16, {sets} weight sets, {calls} calls a graph, "
        f"median of {a.repeats} windows of 5 replays")
    for v, (us, rng) in res.items():
        say(f"  {v:24s} {us:8.1f} us/call   (range {rng:5.1f})   {E * N * K // 2 / us / 1e6:6.2f} TB/s of 4-bit codes   "
            f"{2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s")
    new, loop, mxb = res["nvfp4 (this kernel)"], res["torch bf16 matmul loop"], res["mxfp4 backward"]
    noise = max(new[1], loop[1])
    say(f"  torch loop / nvfp4 = x{loop[0] / new[0]:.2f}: the kernel is {'FASTER' if new[0] < loop[0] - noise else 'NOT faster'} than the "
        f"loop by more than the larger range ({noise:.1f} us)")
    say(f"  nvfp4 / mxfp4 backward = {new[0] / mxb[0]:.3f} "
        f"({'beyond' if abs(new[0] - mxb[0]) > max(new[1], mxb[1]) else 'within'} the ranges)")
    del nv, mx, bf
    torch.cuda.empty_cache()
    return new[0] < loop[0] - noise


ok = [shape("gpt-oss down", a.experts, 2880, 2880), shape("gpt-oss gate|up", a.experts, 2880, 5760)]
say(f"acceptance (faster than the torch loop at both shapes, beyond the ranges): {'met' if all(ok) else 'NOT met'}")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(report) + "\n")
