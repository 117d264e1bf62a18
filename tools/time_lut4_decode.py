#!/usr/bin/env python3
"""The decode sweep of the dense 4-bit code-book (NF4) linear layer, after tools/time_nvfp4_linear.py:
ops.linear_forward_lut4 with split_k=False, the 256-row tile kernel (a); with split_k=True at every forced S of 1, 2, 4, 8, 16
and at the library's S(K, N) (b); and ops.linear_forward_nvfp4(split_k=True) on the same shape (c), the yardstick for what
the format costs.  FQL_LUT4_LINEAR_FILL_WAVES and FQL_LUT4_LINEAR_DECODE_MAX_ROWS (csrc/fql_mx4.hip) are set from this output.

bfloat16 rows, block 64, T in {1, 8, 16, 32, 64, 128}; K -> N: 4096 -> 4096, 4096 -> 11008, 11008 -> 4096, 8192 -> 8192 and
8192 -> 28672.  Method of DESIGN.md section 29: each variant is a hipGraph of calls over rotating weight sets, as many as it
takes for the bytes touched between two uses of one set to exceed the 256 MiB Infinity Cache, a whole number of rotations
a graph; the variants are replayed alternately in the same job, and the median of --repeats windows of 5 replays is printed
with the window-to-window range.  TB/s is the weight bytes (codes and absmax) over the time.

"wins": the policy's median is below the tile kernel's by more than the larger of the two windows' ranges.  The conversion
mechanisms are two builds (FQL_LUT4_DECODE_PREMUL = 1 / 0): run `--tokens 1 --only-policy` once under each library
(FQL_INT4_LIB names the other one), alternately."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
SHAPES = {"4k": (4096, 4096), "up": (4096, 11008), "down": (11008, 4096), "8k": (8192, 8192), "8k-wide": (8192, 28672)}
ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 8, 16, 32, 64, 128])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=40)
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--only-policy", action="store_true", help="time the split form at the policy's S alone (the mechanism A/B)")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
lib = _native.lib()
gs = torch.full((1,), 0.25, device=dev)
defaults = lib.fql_tune_set_lut4_linear_decode_max_rows(-1), lib.fql_tune_set_lut4_linear_slices(-1)
nv_rows = lib.fql_tune_set_nvfp4_linear_decode_max_rows(-1)
print(f"library {os.path.basename(_native.SO_PATH)}: decode form up to {defaults[0]} rows, slices hook {defaults[1]}", flush=True)


def restore():
    lib.fql_tune_set_lut4_linear_decode_max_rows(defaults[0])
    lib.fql_tune_set_lut4_linear_slices(defaults[1])
    lib.fql_tune_set_nvfp4_linear_decode_max_rows(nv_rows)


def timed(K, N, T, pool, nv_pool, variants):
    """variants: name -> (kind, forced slices), kind "tile" / "split" / "nvfp4".  Returns name -> (median us, range us)."""
    touched = N * (K // 2 + K // 16)
    sets = min(max(2, -(-MALL // touched) + 1), len(pool))
    calls = sets * -(-16 // sets)
    x = torch.randn(T, K, device=dev, generator=g).bfloat16()
    st = torch.cuda.Stream()
    graphs = {}
    lib.fql_tune_set_lut4_linear_decode_max_rows(INT_MAX)                # (the choices are made on the host, at capture)
    lib.fql_tune_set_nvfp4_linear_decode_max_rows(INT_MAX)
    with torch.cuda.stream(st), torch.no_grad():
        for v, (kind, slices) in variants.items():
            lib.fql_tune_set_lut4_linear_slices(slices)
            if kind == "nvfp4":
                fn = lambda i: ops.linear_forward_nvfp4(*nv_pool[i], gs, x, split_k=True)
            else:
                fn = lambda i: ops.linear_forward_lut4(*pool[i], x, split_k=kind == "split")
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
    return {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}


for name in a.shapes:
    K, N = SHAPES[name]
    per_set = N * (K // 2 + K // 16)                                     # codes + float32 absmax at block 64 (NVFP4: the same bytes)
    n_pool = min(a.max_sets, max(2, -(-MALL // per_set) + 1))
    pool = [(torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8),
             torch.rand(N, K // 64, device=dev, generator=g) + 0.5) for _ in range(n_pool)]
    nv_pool = [] if a.only_policy else [
        (torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8),
         torch.randint(0x30, 0x48, (N, K // 16), device=dev, generator=g, dtype=torch.uint8)) for _ in range(n_pool)]
    lib.fql_tune_set_lut4_linear_decode_max_rows(INT_MAX)
    S = lib.fql_tune_lut4_linear_kernel(1, K, N) >> 8
    restore()
    print(f"{name}: K={K} -> N={N}, bfloat16 rows, block 64, {n_pool} weight sets of {per_set / 1e6:.1f} MB, policy S = {S}, "
          f"{-(-N // 32)} waves a slice", flush=True)
    largest, ok = 0, True
    for T in a.tokens:
        variants = {"policy": ("split", 0)}
        if not a.only_policy:
            variants = {"a:tile": ("tile", 0), **{f"S={s}": ("split", s) for s in (1, 2, 4, 8, 16)}, **variants, "c:nvfp4": ("nvfp4", 0)}
        res = timed(K, N, T, pool, nv_pool, variants)
        line = "   ".join(f"{v} {m:7.1f} us (range {r:5.1f}) {per_set / m / 1e6:5.2f} TB/s" for v, (m, r) in res.items())
        if not a.only_policy:
            wins = res["policy"][0] < res["a:tile"][0] - max(res["policy"][1], res["a:tile"][1])
            ok = ok and wins
            largest = T if ok else largest
            best = min((v for v in res if v.startswith("S=")), key=lambda v: res[v][0])
            line += f"   x{res['a:tile'][0] / res['policy'][0]:5.2f} over the tile kernel {'wins' if wins else '-'}   best {best}"
        print(f"  T {T:4d}   {line}", flush=True)
    if not a.only_policy:
        print(f"  the split form wins at every T up to {largest}", flush=True)
    del pool, nv_pool
    torch.cuda.empty_cache()
