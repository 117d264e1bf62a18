#!/usr/bin/env python3
"""The decode sweep of the MXFP4 experts: the tile kernel (threshold 0, the behaviour before the
decode kernel existed) against the decode kernel (threshold INT_MAX) at decode batch sizes, from which
FQL_MX4_DECODE_MAX_ROWS (csrc/fql_mx4.hip) is set.

The two gpt-oss shapes, 32 experts, bfloat16 rows: 2880 -> 5760 plain (ops.moe_forward_mxfp4) and 2880 -> 2880 gated
(ops.moe_gated_forward_mxfp4, pre-pass included).  tokens in {1, 2, 4, .., 128}, 4 distinct random experts a token, the
table built by ops.route_plan.  Method of DESIGN.md sections 24 and 25: each variant is a hipGraph of calls over rotating
weight sets, the two variants are replayed alternately in the same job, and the median of --repeats windows of 5 replays
is printed with the window-to-window range.

A decode step touches only the active experts' weights, which fit the 256 MiB Infinity Cache many times over, so the sets
are as many as it takes for the bytes touched between two uses of one set to exceed 256 MiB, and the graph holds a whole
number of rotations over them (16 calls at the least), so the distance holds across replays too; both numbers are printed.  TB/s is the touched weight bytes (blocks and scales of the experts that have
rows) over the time, to be read against the 6.3 TB/s the chip sustains.

"wins": the decode kernel's median is below the tile kernel's by more than the tile kernel's own range in this job.

--shapes few adds what the threshold, a function of T alone, also lets through: 8 experts (2880 -> 5760 plain) with the rows
spread evenly, 16, 32 and 64 live rows an expert at T = 128, 256 and 512.  It decides nothing; it is there to be known."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64, 128])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=24)
ap.add_argument("--k", type=int, default=2880, help="contraction depth (gpt-oss: 2880); a small one shows the fixed cost of a call")
ap.add_argument("--shapes", nargs="+", default=["plain", "gated", "few"], choices=["plain", "gated", "few"])
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
lib = _native.lib()
E, K, TOPK = 32, a.k, 4
default = lib.fql_tune_set_mx4_decode_max_rows(-1)
print(f"library default: decode kernel up to {default} rows", flush=True)


def point(gated, N, tokens, pool):
    idx = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(tokens)])      # 4 distinct experts a token
    tpe, offs, _, _ = ops.route_plan(idx, E)
    return timed(gated, N, E, tpe, offs, tokens * TOPK, pool, f"tokens {tokens:4d}")


def timed(gated, N, E, tpe, offs, T, pool, label):
    active = int((tpe > 0).sum())
    touched = active * N * (K // 2 + K // 32)
    sets = min(max(2, -(-MALL // touched) + 1), a.max_sets, len(pool))
    calls = sets * -(-16 // sets)                                # a whole number of rotations: a replay ends where the next begins
    x = torch.randn(T, 2 * K if gated else K, device=dev, generator=g).bfloat16()
    fn = (lambda i: ops.moe_gated_forward_mxfp4(*pool[i], x, tpe, offs, activation="swiglu_clamp")) if gated else \
         (lambda i: ops.moe_forward_mxfp4(*pool[i], x, tpe, offs))
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st), torch.no_grad():
        for v, rows in (("tile", 0), ("decode", INT_MAX)):
            lib.fql_tune_set_mx4_decode_max_rows(rows)           # (the choice is made on the host, when the graph is captured)
            assert lib.fql_tune_mx4_kernel(E, T, K, N) == (v == "decode")
            fn(0)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(calls):
                    fn(i % sets)
            gr.replay()
            graphs[v] = gr
    lib.fql_tune_set_mx4_decode_max_rows(default)
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
                      for v in ("tile", "decode"))
    print(f"  {label} rows {T:4d} experts {active:2d} touched {touched / 1e6:6.1f} MB sets {sets:2d} calls {calls:2d}   "
          f"{cols}   x{med['tile'] / med['decode']:5.2f} {'wins' if wins else '-'}", flush=True)
    return wins


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
    print(f"{what}: E={experts} K={K} N={N}, bfloat16 rows, "
          f"{n_pool} weight sets of {experts * N * (K // 2 + K // 32) / 1e6:.0f} MB", flush=True)
    if few:
        for m in (16, 32, 64):
            tpe = torch.full((experts,), m, dtype=torch.int32, device=dev)
            offs = (torch.arange(experts, device=dev, dtype=torch.int32) * m).contiguous()
            timed(False, N, experts, tpe, offs, m * experts, pool, f"{m:2d} rows an expert")
    else:
        largest = 0
        ok = True
        for tokens in a.tokens:
            w = point(gated, N, tokens, pool)
            ok = ok and w
            if ok:
                largest = tokens * TOPK
        print(f"  decode kernel wins at every point up to {largest} routed rows", flush=True)
    del pool
    torch.cuda.empty_cache()
