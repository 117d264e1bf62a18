#!/usr/bin/env python3
"""The decode sweep of the NVFP4 experts: the tile kernel (threshold 0) against the decode kernel
(threshold INT_MAX) at decode batch sizes, from which FQL_NVFP4_DECODE_MAX_ROWS (csrc/fql_mx4.hip) is set, and the MXFP4
kernels of the same tree on the same shapes in the same job (--mx-rows: routed-row counts at which ops.moe_forward_mxfp4 /
moe_gated_forward_mxfp4 run too, tile and decode).

The two gpt-oss shapes, 32 experts, bfloat16 rows: 2880 -> 5760 plain (ops.moe_forward_nvfp4) and 2880 -> 2880 gated
(ops.moe_gated_forward_nvfp4, pre-pass included).  tokens in {1, 2, 4, .., 128}, 4 distinct random experts a token, the
table built by ops.route_plan (a row count that is no multiple of 4 is that many tokens with one expert each).  Method of
DESIGN.md section 29: each variant is a hipGraph of calls over rotating weight sets, as many as it takes for the bytes
touched between two uses of one set to exceed the 256 MiB Infinity Cache, a whole number of rotations a graph; the variants
are replayed alternately in the same job, and the median of --repeats windows of 5 replays is printed with the
window-to-window range.  TB/s is the touched weight bytes (blocks and scales of the experts that have rows) over the time.

"wins": the decode kernel's median is below the tile kernel's by more than the larger of the two windows' ranges.  The
threshold is the largest routed-row count up to which that holds at every point of both shapes (DESIGN.md section 32's rule)."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fused_int4_amd import _native, ops

INT_MAX = 2 ** 31 - 1
MALL = 256 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64, 128])
ap.add_argument("--mx-rows", type=int, nargs="*", default=[1, 16, 1024], help="routed rows at which the MXFP4 kernels run as well")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--max-sets", type=int, default=24)
ap.add_argument("--k", type=int, default=2880)
ap.add_argument("--shapes", nargs="+", default=["plain", "gated"], choices=["plain", "gated"])
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
lib = _native.lib()
E, K, TOPK = 32, a.k, 4
defaults = (lib.fql_tune_set_nvfp4_decode_max_rows(-1), lib.fql_tune_set_mx4_decode_max_rows(-1))
print(f"library defaults: NVFP4 decode kernel up to {defaults[0]} rows, MXFP4 decode kernel up to {defaults[1]} rows", flush=True)
SETTERS = {"nv": lib.fql_tune_set_nvfp4_decode_max_rows, "mx": lib.fql_tune_set_mx4_decode_max_rows}


def table(rows):
    top = TOPK if rows % TOPK == 0 else 1
    idx = torch.stack([torch.randperm(E, device=dev, generator=g)[:top] for _ in range(rows // top)])
    tpe, offs, _, _ = ops.route_plan(idx, E)
    return tpe, offs


def timed(gated, N, rows, pools, with_mx):
    """name -> (median us, range us) of "nv-tile", "nv-decode" (and "mx-tile", "mx-decode"), the bytes touched per format."""
    tpe, offs = table(rows)
    active = int((tpe > 0).sum())
    touched = {"nv": active * N * (K // 2 + K // 16), "mx": active * N * (K // 2 + K // 32)}
    sets = min(max(2, -(-MALL // touched["mx"]) + 1), a.max_sets, len(pools["nv"]))
    calls = sets * -(-16 // sets)                                # a whole number of rotations: a replay ends where the next begins
    x = torch.randn(rows, 2 * K if gated else K, device=dev, generator=g).bfloat16()
    kw = dict(activation="swiglu_clamp") if gated else {}
    fns = {"nv": (lambda i: (ops.moe_gated_forward_nvfp4 if gated else ops.moe_forward_nvfp4)(*pools["nv"][i], x, tpe, offs, **kw)),
           "mx": (lambda i: (ops.moe_gated_forward_mxfp4 if gated else ops.moe_forward_mxfp4)(*pools["mx"][i], x, tpe, offs, **kw))}
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st), torch.no_grad():
        for fmt in ("nv", "mx") if with_mx else ("nv",):
            for form, thr in (("tile", 0), ("decode", INT_MAX)):
                SETTERS[fmt](thr)                                # (the choice is made on the host, when the graph is captured)
                fns[fmt](0)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=st):
                    for i in range(calls):
                        fns[fmt](i % sets)
                gr.replay()
                graphs[f"{fmt}-{form}"] = gr
    SETTERS["nv"](defaults[0])
    SETTERS["mx"](defaults[1])
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
    res = {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}
    cols = "   ".join(f"{v} {m:7.1f} us (range {r:5.1f}) {touched[v[:2]] / m / 1e6:5.2f} TB/s" for v, (m, r) in res.items())
    wins = res["nv-decode"][0] < res["nv-tile"][0] - max(res["nv-decode"][1], res["nv-tile"][1])
    line = f"  rows {rows:4d} experts {active:2d} sets {sets:2d} calls {calls:2d}   {cols}   x{res['nv-tile'][0] / res['nv-decode'][0]:5.2f} {'wins' if wins else '-'}"
    if with_mx:
        for form in ("tile", "decode"):
            nv, mx = res[f"nv-{form}"], res[f"mx-{form}"]
            ratio, noise = nv[0] / mx[0], max(nv[1], mx[1])
            line += f"   nv/mx {form} {ratio:5.3f} ({'beyond' if abs(nv[0] - mx[0]) > noise else 'within'} the ranges)"
    print(line, flush=True)
    return wins


for name in a.shapes:
    gated = name == "gated"
    N = 2880 if gated else 5760
    smallest = TOPK * N * (K // 2 + K // 32)
    n_pool = min(a.max_sets, -(-MALL // smallest) + 1)
    blocks = [torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8) for _ in range(n_pool)]
    pools = {"nv": [(b, torch.randint(0x30, 0x48, (E, N, K // 16), device=dev, generator=g, dtype=torch.uint8),
                     torch.rand(E, device=dev, generator=g) + 0.5) for b in blocks],
             "mx": [(b, torch.randint(118, 122, (E, N, K // 32), device=dev, generator=g, dtype=torch.uint8)) for b in blocks]}
    print(f"gpt-oss {'down (gated, pre-pass included)' if gated else 'gate|up (plain)'}: E={E} K={K} N={N}, bfloat16 rows, "
          f"{n_pool} weight sets (the two formats share the code bytes)", flush=True)
    largest, ok = 0, True
    for tokens in a.tokens:
        rows = tokens * TOPK
        w = timed(gated, N, rows, pools, rows in a.mx_rows)
        ok = ok and w
        if ok:
            largest = rows
    print(f"  the NVFP4 decode kernel wins at every point up to {largest} routed rows", flush=True)
    for rows in a.mx_rows:
        if rows not in [t * TOPK for t in a.tokens]:
            timed(gated, N, rows, pools, True)
    del pools, blocks
    torch.cuda.empty_cache()
