#!/usr/bin/env python3
"""Time the NVFP4 GEMMs with the adapter stage fused in (ops.moe_forward_nvfp4_lora, ops.moe_gated_forward_nvfp4_lora,
ops.moe_backward_input_nvfp4_lora) against the composition they replace, in the same job: the base op with a float32 result
plus ops.lora_expand from it into bfloat16 (what the INT4 adapter layers do), and against the base op alone (bfloat16 result,
no adapter: the floor).  The yardstick is the composition, never the fused kernel itself.  The shrink that produces v / dv is
the same launch in every variant and is left out.

gpt-oss's two projections, 32 experts, 1024 routed rows spread evenly, bfloat16 rows: gate|up 2880 -> 5760 and the gated down
2880 -> 2880, forward and input gradient, r = 16 and 64, a global scale per expert that is no power of two.  Method of
tools/time_mxfp4_lora.py (DESIGN.md sections 24 and 35): each variant
is a hipGraph of 16 calls over rotating weight sets (so no set is resident in the caches from the call before), the variants
are replayed alternately, and the median of --repeats windows of 5 replays is printed with its spread.  The report goes to
stdout and to --out (profiles/nvfp4_lora_timing.txt)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fused_int4_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--experts", type=int, default=32)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvfp4_lora_timing.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
BF, F32 = torch.bfloat16, torch.float32
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def measure(title, variants):
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
    say(title)
    med = {v: statistics.median(times[v]) for v in variants}
    for v in variants:
        say(f"  {v:44s} {med[v]:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]")
    say(f"  fused / composition = {med['fused (adapter stage in the GEMM)'] / med['composition (base f32 out + lora_expand)']:.3f}, "
        f"fused - base alone = {med['fused (adapter stage in the GEMM)'] - med['base op alone (bf16 out, no adapter)']:+.1f} us")


def shape(name, E, K, N, gated):
    """A projection K -> N: ``blocks`` [E, N, K/2].  The forward reads rows [T, K] (gated: gate_up [T, 2K]) and writes [T, N];
    the input gradient reads grad_out [T, N] and writes [T, K]."""
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    mx = [(torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
           torch.randint(0x28, 0x38, (E, N, K // 16), device=dev, generator=g, dtype=torch.uint8),
           torch.rand(E, device=dev, generator=g) + 0.5) for _ in range(a.sets)]
    rows = torch.randn(T, 2 * K if gated else K, device=dev, generator=g).to(BF)
    gy = torch.randn(T, N, device=dev, generator=g).to(BF)
    base_fwd = ops.moe_gated_forward_nvfp4 if gated else ops.moe_forward_nvfp4
    lora_fwd = ops.moe_gated_forward_nvfp4_lora if gated else ops.moe_forward_nvfp4_lora
    for r in a.ranks:
        v, dv = torch.randn(T, r, device=dev, generator=g), torch.randn(T, r, device=dev, generator=g)
        Bs = [torch.randn(E, N, r, device=dev, generator=g) * 0.1 for _ in range(a.sets)]
        As = [torch.randn(E, r, K, device=dev, generator=g) * 0.1 for _ in range(a.sets)]
        measure(f"{name} forward: E={E} K={K} N={N} T={T} ({m} rows/expert) r={r}, rows and result bf16", {
            "fused (adapter stage in the GEMM)": lambda i: lora_fwd(*mx[i], rows, v, Bs[i], tpe, offs, out_dtype=BF),
            "composition (base f32 out + lora_expand)": lambda i: ops.lora_expand(
                v, Bs[i], "cr", tpe, offs, input=base_fwd(*mx[i], rows, tpe, offs, out_dtype=F32), out_dtype=BF),
            "base op alone (bf16 out, no adapter)": lambda i: base_fwd(*mx[i], rows, tpe, offs, out_dtype=BF),
        })
        measure(f"{name} input gradient: E={E} K={K} N={N} T={T} r={r}, grad_out and result bf16", {
            "fused (adapter stage in the GEMM)": lambda i: ops.moe_backward_input_nvfp4_lora(*mx[i], gy, dv, As[i], tpe, offs,
                                                                                             out_dtype=BF),
            "composition (base f32 out + lora_expand)": lambda i: ops.lora_expand(
                dv, As[i], "rc", tpe, offs, input=ops.moe_backward_input_nvfp4(*mx[i], gy, tpe, offs, out_dtype=F32), out_dtype=BF),
            "base op alone (bf16 out, no adapter)": lambda i: ops.moe_backward_input_nvfp4(*mx[i], gy, tpe, offs, out_dtype=BF),
        })
    del mx
    torch.cuda.empty_cache()


shape("gpt-oss gate|up", a.experts, 2880, 5760, gated=False)
shape("gpt-oss down (gated)", a.experts, 2880, 2880, gated=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(report) + "\n")
