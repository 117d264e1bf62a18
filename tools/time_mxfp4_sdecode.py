#!/usr/bin/env python3
"""The decode sweep of the fp8-row and MXFP4-row precisions of the MXFP4 experts: per precision the
tile kernel (threshold 0: the behaviour before the decode kernels existed) against the decode kernel (threshold INT_MAX) at
decode batch sizes, from which FQL_MX4_F8_DECODE_MAX_ROWS / FQL_MX4_F4_DECODE_MAX_ROWS (csrc/fql_mx4.hip) are set, and next
to them the bfloat16 path under its own default threshold: the column that tells a user which precision to pick for decode.

The method is tools/time_mxfp4_decode.py's: the two gpt-oss shapes, 32 experts, bfloat16 rows in (so the quantising entries,
their pre-pass included in the time): 2880 -> 5760 plain (ops.moe_forward_mxfp4) and 2880 -> 2880 gated
(ops.moe_gated_forward_mxfp4).  tokens in {1, 2, 4, .., 128}, 4 distinct random experts a token, the table built by
ops.route_plan.  Each variant is a hipGraph of calls over rotating weight sets, as many as it takes for the bytes touched
between two uses of one set to exceed 256 MiB, a whole number of rotations a graph; the variants are replayed alternately
in the same job, and the median of --repeats windows of 5 replays is printed with the window-to-window range.

"wins": the decode kernel's median is below the tile kernel's by more than the tile kernel's own range in this job.  A
mode's threshold is the largest routed-row count up to which it wins at every point of both shapes.

--shapes few adds what a threshold, a function of T alone, also lets through: 8 experts (2880 -> 5760 plain) with the rows
spread evenly, 16, 32 and 64 live rows an expert at T = 128, 256 and 512.  It decides nothing; it is there to be known."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
MODES = {"fp8": 1, "fp4": 2}
ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64, 128])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=24)
ap.add_argument("--k", type=int, default=2880, help="contraction depth (gpt-oss: 2880); a small one shows the fixed cost of a call")
ap.add_argument("--shapes", nargs="+", default=["plain", "gated", "few"], choices=["plain", "gated", "few"])
ap.add_argument("--modes", nargs="+", default=["fp8", "fp4"], choices=list(MODES))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
lib = _native.lib()
E, K, TOPK = 32, a.k, 4
setter = lib.fql_tune_set_mx4_scaled_decode_max_rows
default = {m: setter(MODES[m], -1) for m in MODES}
print(f"library defaults: decode kernel up to {default['fp8']} rows (fp8), {default['fp4']} rows (fp4), "
      f"{lib.fql_tune_set_mx4_decode_max_rows(-1)} rows (bf16)", flush=True)
VARIANTS = ("tile", "decode", "bf16")


def point(mode, gated, N, tokens, pool):
    idx = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(tokens)])      # 4 distinct experts a token
    tpe, offs, _, _ = ops.route_plan(idx, E)
    return timed(mode, gated, N, E, tpe, offs, tokens * TOPK, pool, f"tokens {tokens:4d}")


def timed(mode, gated, N, E, tpe, offs, T, pool, label):
    active = int((tpe > 0).sum())
    touched = active * N * (K // 2 + K // 32)
    sets = min(max(2, -(-MALL // touched) + 1), a.max_sets, len(pool))
    calls = sets * -(-16 // sets)                                # a whole number of rotations: a replay ends where the next begins
    x = torch.randn(T, 2 * K if gated else K, device=dev, generator=g).bfloat16()

    def fn(i, precision):
        if gated:
            return ops.moe_gated_forward_mxfp4(*pool[i], x, tpe, offs, activation="swiglu_clamp", precision=precision)
        return ops.moe_forward_mxfp4(*pool[i], x, tpe, offs, precision=precision)
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st), torch.no_grad():
        for v in VARIANTS:
            precision = "bf16" if v == "bf16" else mode
            if v != "bf16":
                setter(MODES[mode], 0 if v == "tile" else INT_MAX)   # (the choice is made on the host, when the graph is captured)
                assert lib.fql_tune_mx4_scaled_kernel(MODES[mode], E, T, K, N) == (v == "decode")
            fn(0, precision)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(calls):
                    fn(i % sets, precision)
            gr.replay()
            graphs[v] = gr
    setter(MODES[mode], default[mode])
    times = {v: [] for v in graphs}
    for _ in range(a.repeats):
        for v in graphs:                                         # alternating: the variants share whatever else happens
            with torch.cuda.stream(st):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(5):
                    graphs[v].replay()
                e1.record(st)
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / (5 * calls) * 1e3)
    med = {v: statistics.median(t) for v, t in times.items()}
    spread = max(times["tile"]) - min(times["tile"])
    wins = med["decode"] < med["tile"] - spread
    cols = "   ".join(f"{v} {med[v]:7.1f} us [{min(times[v]):6.1f} .. {max(times[v]):6.1f}] {touched / med[v] / 1e6:5.2f} TB/s"
                      for v in VARIANTS)
    print(f"  {mode} {label} rows {T:4d} experts {active:2d} touched {touched / 1e6:6.1f} MB sets {sets:2d} calls {calls:2d}   "
          f"{cols}   tile/decode x{med['tile'] / med['decode']:5.2f} {'wins' if wins else '-'}   "
          f"bf16/decode x{med['bf16'] / med['decode']:5.2f}", flush=True)
    return wins


largest = {m: None for m in a.modes}
for name in a.shapes:
    gated = name == "gated"
    few = name == "few"
    experts = 8 if few else E
    N = 2880 if gated else 5760
    smallest = (experts if few else TOPK) * N * (K // 2 + K // 32)
    n_pool = min(a.max_sets, -(-MALL // smallest) + 1)
    pool = [(torch.randint(0, 256, (experts, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
             torch.randint(118, 122, (experts, N, K // 32), device=dev, generator=g, dtype=torch.uint8)) for _ in range(n_pool)]
    what = "8 experts, rows spread evenly (plain)" if few else "gpt-oss " + ("down (gated, pre-pass included)" if gated else "gate|up (plain)")
    print(f"{what}: E={experts} K={K} N={N}, bfloat16 rows in, "
          f"{n_pool} weight sets of {experts * N * (K // 2 + K // 32) / 1e6:.0f} MB", flush=True)
    for mode in a.modes:
        if few:
            for m in (16, 32, 64):
                tpe = torch.full((experts,), m, dtype=torch.int32, device=dev)
                offs = (torch.arange(experts, device=dev, dtype=torch.int32) * m).contiguous()
                timed(mode, False, N, experts, tpe, offs, m * experts, pool, f"{m:2d} rows an expert")
        else:
            best, ok = 0, True
            for tokens in a.tokens:
                ok = point(mode, gated, N, tokens, pool) and ok
                if ok:
                    best = tokens * TOPK
            print(f"  {mode}: decode kernel wins at every point up to {best} routed rows", flush=True)
            largest[mode] = best if largest[mode] is None else min(largest[mode], best)
    del pool
    torch.cuda.empty_cache()
for mode, rows in largest.items():
    if rows is not None:
        print(f"{mode}: threshold from this job: {rows} routed rows (0: the decode kernel won at no point from the first on)", flush=True)
