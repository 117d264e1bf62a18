#!/usr/bin/env python3
"""The decode sweep of the dense MXFP4 linear layer: ops.linear_forward_mxfp4 with split_k=False and
the grouped decode kernel forced (a), with the tile kernel forced (b), the split form at the library's S(K, N) (c), and
the split form at every forced S for T = 1 and T = 16 (d).  (a) and (b) are the kernels that existed before the layer and
are the yardstick; the policy table and FQL_MX4_LINEAR_DECODE_MAX_ROWS (csrc/fql_mx4.hip) are set from this output.

bfloat16 rows, T in {1, 2, 4, .., 128}; K -> N: 2880 -> 5120 and 4096 -> 2880 (gpt-oss's attention projections),
8192 -> 8192, 8192 -> 28672 and 28672 -> 8192.  Method of DESIGN.md section 29: each variant is a hipGraph of calls over
rotating weight sets, as many as it takes for the bytes touched between two uses of one set to exceed the 256 MiB Infinity
Cache, a whole number of rotations a graph; the variants are replayed alternately in the same job, and the median of
--repeats windows of 5 replays is printed with the window-to-window range.  TB/s is the weight bytes (blocks and scales)
over the time, to be read against the 6.3 TB/s the chip sustains.

"wins": the split form's median is below the better of (a) and (b) by more than the larger of the two windows' ranges."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
SHAPES = {"qkv": (2880, 5120), "o": (4096, 2880), "8k": (8192, 8192), "8k-wide": (8192, 28672), "long-k": (28672, 8192)}
ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64, 128])
ap.add_argument("--sweep-tokens", type=int, nargs="*", default=[1, 16])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=40)
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
lib = _native.lib()
defaults = (lib.fql_tune_set_mx4_decode_max_rows(-1), lib.fql_tune_set_mx4_linear_decode_max_rows(-1), lib.fql_tune_set_mx4_linear_slices(-1))
print(f"library defaults: grouped decode kernel up to {defaults[0]} rows, split form up to {defaults[1]} rows, slices hook {defaults[2]}",
      flush=True)


def restore():
    lib.fql_tune_set_mx4_decode_max_rows(defaults[0])
    lib.fql_tune_set_mx4_linear_decode_max_rows(defaults[1])
    lib.fql_tune_set_mx4_linear_slices(defaults[2])


def timed(K, N, T, pool, variants):
    """variants: name -> (grouped decode threshold, split_k, forced slices).  Returns name -> (median us, range us)."""
    touched = N * (K // 2 + K // 32)
    sets = min(max(2, -(-MALL // touched) + 1), len(pool))
    calls = sets * -(-16 // sets)
    x = torch.randn(T, K, device=dev, generator=g).bfloat16()
    st = torch.cuda.Stream()
    graphs = {}
    lib.fql_tune_set_mx4_linear_decode_max_rows(INT_MAX)
    with torch.cuda.stream(st), torch.no_grad():
        for v, (rows, split, slices) in variants.items():
            lib.fql_tune_set_mx4_decode_max_rows(rows)               # (the choices are made on the host, at capture)
            lib.fql_tune_set_mx4_linear_slices(slices)
            fn = lambda i: ops.linear_forward_mxfp4(*pool[i], x, split_k=split)
            fn(0)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(calls):
                    fn(i % sets)
            gr.replay()
            graphs[v] = gr
    restore()
    times = {v: [] for v in graphs}
    for _ in range(a.repeats):
        for v in graphs:                                             # alternating: the variants share whatever else happens
            with torch.cuda.stream(st):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(5):
                    graphs[v].replay()
                e1.record(st)
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / (5 * calls) * 1e3)
    return {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}, touched, sets, calls


def cell(name, r, touched):
    med, rng = r
    return f"{name} {med:7.1f} us (range {rng:5.1f}) {touched / med / 1e6:5.2f} TB/s"


for name in a.shapes:
    K, N = SHAPES[name]
    per_set = N * (K // 2 + K // 32)
    n_pool = min(a.max_sets, max(2, -(-MALL // per_set) + 1))
    pool = [(torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8),
             torch.randint(118, 122, (N, K // 32), device=dev, generator=g, dtype=torch.uint8)) for _ in range(n_pool)]
    lib.fql_tune_set_mx4_linear_decode_max_rows(INT_MAX)
    S = lib.fql_tune_mx4_linear_kernel(1, K, N) >> 8
    restore()
    print(f"{name}: K={K} -> N={N}, bfloat16 rows, {n_pool} weight sets of {per_set / 1e6:.1f} MB, policy S = {S}, "
          f"{-(-N // 32)} waves a slice", flush=True)
    largest, ok = 0, True
    for T in a.tokens:
        res, touched, sets, calls = timed(K, N, T, pool, {"a:decode": (INT_MAX, False, 0), "b:tile": (0, False, 0),
                                                         "c:split": (INT_MAX, True, 0)})
        best = min(("a:decode", "b:tile"), key=lambda v: res[v][0])
        wins = S > 1 and res["c:split"][0] < res[best][0] - max(res["c:split"][1], res[best][1])
        ok = ok and wins
        if ok:
            largest = T
        print(f"  T {T:4d} sets {sets:2d} calls {calls:2d}   " + "   ".join(cell(v, res[v], touched) for v in res)
              + f"   x{res[best][0] / res['c:split'][0]:5.2f} over {best} {'wins' if wins else '-'}", flush=True)
    print(f"  the split form wins at every T up to {largest}", flush=True)
    for T in a.sweep_tokens:
        res, touched, _, _ = timed(K, N, T, pool, {f"S={s}": (INT_MAX, True, s) for s in (1, 2, 4, 8, 16)})
        print(f"  sweep T {T:3d}   " + "   ".join(cell(v, res[v], touched) for v in res)
              + f"   best {min(res, key=lambda v: res[v][0])}", flush=True)
    del pool
    torch.cuda.empty_cache()
