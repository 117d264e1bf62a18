#!/usr/bin/env python3
"""Time the fp6 mode of the MXFP4 grouped ops (csrc/fql_gemm_mx4_scaled.h with ROWS = 3: e2m1 weights against MXFP6 rows, and
the MXFP6 quantiser) against the bfloat16 path and the fp8 and fp4 modes of the same shape in the same job (DESIGN.md
section 34).

--part times (tools/time_mxfp4_f4.py's method): 1024 routed rows spread evenly over the gpt-oss-like shapes (32 experts,
2880 -> 5760 plain and 2880 -> 2880 gated) and the headline shape (8 experts, 4096 -> 11008), float rows in, so every mode
pays its pre-pass; the rows-already-quantised forms (the GEMM alone) beside them.  Each variant is a hipGraph of 16 calls
over rotating weight sets, the variants are replayed alternately, and the median of --repeats windows of 5 replays is printed
with its range.  "beats fp8": the fp6 median is below the fp8 median by more than the two windows' own ranges together.

--part sweep (tools/time_mxfp4_sdecode.py's method): the fp6 tile kernel (threshold 0) against its decode kernel (threshold
INT_MAX) at 1 / 2 / 4 / 16 tokens, 4 distinct experts of 32 a token, on both gpt-oss shapes, from which
FQL_MX4_F6_DECODE_MAX_ROWS (csrc/fql_mx4.hip) is set: the largest routed-row count up to which the decode kernel wins at
every point of both shapes, 0 if it never does."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--part", default="times", choices=["times", "sweep"])
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="type of the float rows")
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 2, 4, 16])
ap.add_argument("--max-sets", type=int, default=24)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
rows_dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
lib = _native.lib()
setter = lib.fql_tune_set_mx4_f6_decode_max_rows
default = setter(-1)
print(f"library default: the fp6 decode kernel up to {default} rows", flush=True)


def windows(graphs, per_replay):
    st = torch.cuda.current_stream()
    times = {v: [] for v in graphs}
    for _ in range(a.repeats):
        for v in graphs:                                        # alternating: the variants share whatever else happens
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(5):
                graphs[v].replay()
            e1.record(st)
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / (5 * per_replay[v]) * 1e3)
    return times


def capture(fn, calls, sets):
    for i in range(min(2, sets)):
        fn(i)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=torch.cuda.current_stream()):
        for i in range(calls):
            fn(i % sets)
    gr.replay()
    return gr


def shape(name, E, K, N):
    m = a.rows // E
    T = m * E
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    mx = [(torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
           torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)) for _ in range(a.sets)]
    gu = torch.randn(T, 2 * K, device=dev, generator=g).to(rows_dt)
    xr = gu[:, :K].contiguous()
    x8, act = ops.quantize_activations_fp8(xr)
    x8, act = x8.contiguous(), act.contiguous()
    x4, xs4 = ops.quantize_rows_mxfp4(xr)
    x6, xs6 = ops.quantize_rows_mxfp6(xr)
    variants = {
        "bf16, float rows in": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs),
        "fp8, float rows in (pre-pass + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp8"),
        "fp6, float rows in (quantiser + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp6"),
        "fp4, float rows in (quantiser + GEMM)": lambda i: ops.moe_forward_mxfp4(*mx[i], xr, tpe, offs, precision="fp4"),
        "bf16, gated": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs),
        "fp8, gated (pre-pass + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs, precision="fp8"),
        "fp6, gated (quantiser + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs, precision="fp6"),
        "fp4, gated (quantiser + GEMM)": lambda i: ops.moe_gated_forward_mxfp4(*mx[i], gu, tpe, offs, precision="fp4"),
        "fp8, e4m3 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp8(*mx[i], x8, act, tpe, offs, out_dtype=rows_dt),
        "fp6, MXFP6 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp6(*mx[i], x6, xs6, tpe, offs, out_dtype=rows_dt),
        "fp4, MXFP4 rows in (GEMM alone)": lambda i: ops.moe_forward_mxfp4_fp4(*mx[i], x4, xs4, tpe, offs, out_dtype=rows_dt),
    }
    st = torch.cuda.Stream()
    with torch.cuda.stream(st), torch.no_grad():
        graphs = {v: capture(fn, 16, a.sets) for v, fn in variants.items()}
        times = windows(graphs, {v: 16 for v in graphs})
    print(f"{name}: E={E} K={K} N={N} T={T} ({m} rows/expert), float rows {a.dtype}", flush=True)
    med = {v: statistics.median(times[v]) for v in variants}
    rng = {v: max(times[v]) - min(times[v]) for v in variants}
    for v in variants:
        us = med[v]
        line = f"  {v:38s} {us:8.1f} us/call   [{min(times[v]):.1f} .. {max(times[v]):.1f}]   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s"
        if v.startswith("fp6"):
            tail = v.split(",", 1)[1]
            v8 = next(k for k in variants if k.startswith("fp8") and ("gated" in k) == ("gated" in v) and ("alone" in k) == ("alone" in v))
            v4 = next(k for k in variants if k.startswith("fp4") and k.split(",", 1)[1].split("(")[1] == tail.split("(")[1]
                      and ("gated" in k) == ("gated" in v))
            beats = med[v8] - us > rng[v8] + rng[v]
            line += (f"   fp8 / fp6 x {med[v8] / us:5.3f} ({'beats fp8' if beats else 'does not beat fp8'} by more than the ranges)"
                     f"   fp6 / fp4 x {us / med[v4]:5.3f}")
        if not v.endswith("alone)"):
            line += f"   {med['bf16, gated' if 'gated' in v else 'bf16, float rows in'] / us:5.2f} x bf16"
        print(line, flush=True)
    del mx
    torch.cuda.empty_cache()


def sweep_point(gated, K, N, tokens, pool):
    E, TOPK = 32, 4
    idx = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(tokens)])      # 4 distinct experts a token
    tpe, offs, _, _ = ops.route_plan(idx, E)
    T = tokens * TOPK
    active = int((tpe > 0).sum())
    touched = active * N * (K // 2 + K // 32)
    sets = min(max(2, -(-MALL // touched) + 1), a.max_sets, len(pool))
    calls = sets * -(-16 // sets)                                # a whole number of rotations
    x = torch.randn(T, 2 * K if gated else K, device=dev, generator=g).bfloat16()

    def fn(i):
        if gated:
            return ops.moe_gated_forward_mxfp4(*pool[i], x, tpe, offs, activation="swiglu_clamp", precision="fp6")
        return ops.moe_forward_mxfp4(*pool[i], x, tpe, offs, precision="fp6")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st), torch.no_grad():
        graphs = {}
        for v in ("tile", "decode"):
            setter(0 if v == "tile" else INT_MAX)                # (the choice is made on the host, when the graph is captured)
            assert lib.fql_tune_mx4_f6_kernel(E, T, K, N) == (v == "decode")
            graphs[v] = capture(fn, calls, sets)
        setter(default)
        times = windows(graphs, {v: calls for v in graphs})
    med = {v: statistics.median(t) for v, t in times.items()}
    spread = max(times["tile"]) - min(times["tile"])
    wins = med["decode"] < med["tile"] - spread
    cols = "   ".join(f"{v} {med[v]:7.1f} us [{min(times[v]):6.1f} .. {max(times[v]):6.1f}] {touched / med[v] / 1e6:5.2f} TB/s" for v in graphs)
    print(f"  fp6 tokens {tokens:4d} rows {T:4d} experts {active:2d} touched {touched / 1e6:6.1f} MB sets {sets:2d} calls {calls:2d}   "
          f"{cols}   tile/decode x{med['tile'] / med['decode']:5.2f} {'wins' if wins else '-'}", flush=True)
    return wins


if a.part == "times":
    shape("gpt-oss-like gate|up", 32, 2880, 5760)
    shape("gpt-oss-like down", 32, 2880, 2880)
    shape("headline", 8, 4096, 11008)
else:
    K, largest = 2880, None
    for gated in (False, True):
        N = 2880 if gated else 5760
        n_pool = min(a.max_sets, -(-MALL // (4 * N * (K // 2 + K // 32))) + 1)
        pool = [(torch.randint(0, 256, (32, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                 torch.randint(118, 122, (32, N, K // 32), device=dev, generator=g, dtype=torch.uint8)) for _ in range(n_pool)]
        print(f"gpt-oss {'down (gated, pre-pass included)' if gated else 'gate|up (plain)'}: E=32 K={K} N={N}, bfloat16 rows in, "
              f"{n_pool} weight sets", flush=True)
        best, ok = 0, True
        for tokens in a.tokens:
            ok = sweep_point(gated, K, N, tokens, pool) and ok
            if ok:
                best = tokens * 4
        print(f"  fp6: decode kernel wins at every point up to {best} routed rows", flush=True)
        largest = best if largest is None else min(largest, best)
        del pool
        torch.cuda.empty_cache()
    print(f"fp6: threshold from this job: {largest} routed rows (0: the decode kernel won at no point from the first on)", flush=True)
