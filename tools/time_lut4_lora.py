#!/usr/bin/env python3
"""Time the NF4 tile kernels with the adapter stage fused in (ops.linear_forward_lut4_lora, ops.linear_backward_input_lut4_lora)
against the composition they replace, in the same job: what LoRANF4Linear(fused=False) launches for the same result (the base op
with a float32 result, then the expand from it into bfloat16: ops._expand_into, the layer's own helper), and against the base op
alone (bfloat16 result, no adapter: the floor).  The yardstick is the composition, never the fused kernel itself.  The shrink
that produces the [T, r] rows is one launch of the same kernel in every variant and is left out (the composed route scales in
the expand, the fused one in the shrink: the same work).

Llama-7B's two projection shapes, 4096 -> 4096 and 4096 -> 11008, T in {1024, 4096}, r in {16, 64}, bfloat16 rows and results,
NF4 with block = 64.  Method of tools/time_mxfp4_lora.py (DESIGN.md sections 24 and 35): each variant is a hipGraph of 16 calls
over rotating weight sets (so no set is resident in the caches from the call before), the variants are replayed alternately, and
the median of --repeats windows of 5 replays is printed with the windows' range.  The report goes to stdout and to --out
(profiles/lut4_lora_timing.txt)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fused_int4_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lut4_lora_timing.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
BF, F32 = torch.bfloat16, torch.float32
FUSED, COMP, BASE = "fused (adapter stage in the GEMM)", "composition (base f32 out + expand)", "base op alone (bf16 out, no adapter)"
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
        say(f"  {v:40s} {med[v]:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]")
    say(f"  fused / composition = {med[FUSED] / med[COMP]:.3f} "
        f"[{min(times[FUSED]) / max(times[COMP]):.3f} .. {max(times[FUSED]) / min(times[COMP]):.3f}], "
        f"fused - base alone = {med[FUSED] - med[BASE]:+.1f} us")


def shape(K, N):
    """A projection K -> N: ``codes`` [N, K/2].  The forward reads x [T, K] and writes [T, N]; the input gradient reads grad_out
    [T, N] and writes [T, K]."""
    w = [(torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8),
          torch.rand(N, K // 64, device=dev, generator=g) * 0.1 + 0.01) for _ in range(a.sets)]
    for T in a.rows:
        x, gy = torch.randn(T, K, device=dev, generator=g).to(BF), torch.randn(T, N, device=dev, generator=g).to(BF)
        for r in a.ranks:
            v, dv = torch.randn(T, r, device=dev, generator=g), torch.randn(T, r, device=dev, generator=g)
            Bs = [torch.randn(N, r, device=dev, generator=g) * 0.1 for _ in range(a.sets)]
            As = [torch.randn(r, K, device=dev, generator=g) * 0.1 for _ in range(a.sets)]
            measure(f"forward: K={K} N={N} T={T} r={r}, rows and result bf16", {
                FUSED: lambda i: ops.linear_forward_lut4_lora(*w[i], x, v, Bs[i], out_dtype=BF),
                COMP: lambda i: ops._expand_into(v, Bs[i], "cr", ops.linear_forward_lut4(*w[i], x, out_dtype=F32), BF, scale=2.0),
                BASE: lambda i: ops.linear_forward_lut4(*w[i], x, out_dtype=BF),
            })
            measure(f"input gradient: K={K} N={N} T={T} r={r}, grad_out and result bf16", {
                FUSED: lambda i: ops.linear_backward_input_lut4_lora(*w[i], gy, dv, As[i], out_dtype=BF),
                COMP: lambda i: ops._expand_into(dv, As[i], "rc", ops.linear_backward_input_lut4(*w[i], gy), BF),
                BASE: lambda i: ops.linear_backward_input_lut4(*w[i], gy, out_dtype=BF),
            })
    del w
    torch.cuda.empty_cache()


shape(4096, 4096)
shape(4096, 11008)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(report) + "\n")
