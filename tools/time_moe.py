#!/usr/bin/env python3
"""Time the grouped MoE call (8 experts 4096->11008 by default) over a sweep of routed rows per expert
(product call fql_moe_fwd_f32 = pre-pass + grouped GEMM, hipGraph of 16 launches over rotating weight sets).

--group-size G[,G...]: quantise per group of G inputs (0: per tensor, the per-row kernels, as before) and time every
listed layout in the same run, alternating them --repeats times; the median is printed last.  --op: the grouped op that
is timed, `forward` (moe_forward, rows [T, k]), `gated` (moe_gated_forward, gate|up rows [T, 2k]) or `backward`
(moe_backward_input, gradient rows [T, n])."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fused_int4_amd as fq
from fused_int4_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=4096); ap.add_argument("--n", type=int, default=11008)
ap.add_argument("--experts", type=int, default=8)
ap.add_argument("--rows", default="1,2,4,8,16,32,64,128,256")
ap.add_argument("--precision", default="exact")
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--group-size", default="0")
ap.add_argument("--op", default="forward", choices=["forward", "gated", "backward"])
ap.add_argument("--repeats", type=int, default=1)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
E = a.experts
groups = [int(v) for v in a.group_size.split(",")]
sets = {gs: [] for gs in groups}
for _ in range(a.sets):
    w = torch.randn(E, a.n, a.k, device=dev, generator=g) * 0.02
    for gs in groups:
        if gs == 0:
            sets[gs].append(fq.quantize_weights_moe(w))
        else:
            q = [fq.quantize_weights(w[e], group_size=gs) for e in range(E)]
            sets[gs].append(tuple(torch.stack([t[i] for t in q]) for i in range(3)))
    del w
wbytes = E * a.n * a.k // 2


def call(weights, rows, eid, tpe, offs):
    if a.op == "forward":
        return ops.moe_forward(*weights, rows, eid, tpe, offs, precision=a.precision)
    if a.op == "gated":
        return ops.moe_gated_forward(*weights, rows, tpe, offs, precision=a.precision)
    return ops.moe_backward_input(*weights, rows, tpe, offs, precision=a.precision)


for m in [int(b) for b in a.rows.split(",")]:
    T = m * E
    width = {"forward": a.k, "gated": 2 * a.k, "backward": a.n}[a.op]
    x = torch.randn(T, width, device=dev, generator=g)
    tpe = torch.full((E,), m, dtype=torch.int32, device=dev)
    offs = (torch.arange(E, device=dev, dtype=torch.int32) * m).contiguous()
    eid = torch.arange(E, device=dev, dtype=torch.int32).repeat_interleave(m)
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st):
        for gs in groups:
            for s in sets[gs][:2]:
                call(s, x, eid, tpe, offs)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for i in range(16):
                    call(sets[gs][i % len(sets[gs])], x, eid, tpe, offs)
            gr.replay()
            graphs[gs] = gr
    times = {gs: [] for gs in groups}
    for _ in range(a.repeats):
        for gs in groups:                                      # alternating: the layouts share whatever else the host does
            with torch.cuda.stream(st):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(5):
                    graphs[gs].replay()
                e1.record(st)
            torch.cuda.synchronize()
            times[gs].append(e0.elapsed_time(e1) / 80 * 1e3)
    for gs in groups:
        us = statistics.median(times[gs])
        layout = "per-row" if gs == 0 else f"group {gs}"
        spread = f"   [{min(times[gs]):.1f} .. {max(times[gs]):.1f}]" if a.repeats > 1 else ""
        tag = "" if (len(groups) == 1 and gs == 0 and a.op == "forward") else f"{a.op} {layout}: "
        print(f"{tag}rows/expert={m:4d} (T={T:5d}): {us:8.1f} us/call   {wbytes/us/1e6:7.2f} TB/s packed-weight   "
              f"{2.0*T*a.k*a.n/us/1e6:8.1f} TFLOP/s{spread}", flush=True)
