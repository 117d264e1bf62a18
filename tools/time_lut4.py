#!/usr/bin/env python3
"""Time the two dense code-book (NF4) ops (ops.linear_forward_lut4 / ops.linear_backward_input_lut4)
next to their nearest existing kernels, ops.linear_forward_nvfp4 / ops.linear_backward_input_nvfp4 (the same bytes per weight
within 1/16, the same matrix instruction), on the same shapes in the same job.

Dense 4096 -> 11008 and 4096 -> 4096 at 256, 1024 and 4096 rows, bfloat16 rows and results.  Method of DESIGN.md section 29
without the graph: every variant runs over rotating weight sets (as many as it takes for the bytes touched between two uses
of one set to exceed the 256 MiB Infinity Cache, at most --max-sets), the variants' windows alternate in the same job, a
window is --calls calls between two device events, and the median of --repeats windows is printed with the window-to-window
range.  No ratio is fixed in advance: the report states what was found.  It goes to stdout and to --out
(profiles/lut4_timing.txt).

--grouped: the grouped ops on 8 experts, (a) ops.moe_forward_lut4 / moe_backward_input_lut4 /
moe_gated_forward_lut4, (b) what the tree offered before them, a loop of E dense calls on the expert slices, (c)
ops.moe_forward_nvfp4 / moe_backward_input_nvfp4 / moe_gated_forward_nvfp4 as they dispatch; 4096 -> 11008 and 11008 -> 4096 at
1024 and 4096 routed rows, balanced, and 1024 rows with the benchmark's skewed routing.  The same method; the report goes to
profiles/lut4_group_timing.txt unless --out is given.

--grouped-decode: ops.moe_forward_lut4 with fql_tune_set_lut4_group_decode_max_rows alternating the 128-row
tile (0) and the one-wave decode kernel in one process, on 8 experts (4096 -> 11008 | 28672, 11008 | 14336 -> 4096, top-2) and 64
experts (2048 -> 2816, 1408 -> 2048, top-6), at 1, 2, 4, 16 and 64 tokens x top-k and at 256, 512 and 1024 routed rows; then, at one
token, the split form at S = 1, 2, 4, 8, 16 next to the one-wave kernel.  Every call moves on to the next weight set and, within
a set, to the next rotation of the expert table, so the live experts' weights come from HBM.  The report goes to
profiles/lut4_group_decode_timing.txt unless --out is given."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fused_int4_amd import ops

MALL = 256 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=[256, 1024, 4096])
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--calls", type=int, default=24)
ap.add_argument("--max-sets", type=int, default=6)
ap.add_argument("--grouped", action="store_true")
ap.add_argument("--grouped-decode", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
a.out = a.out or os.path.join(ROOT, "profiles", "lut4_group_decode_timing.txt" if a.grouped_decode else
                              "lut4_group_timing.txt" if a.grouped else "lut4_timing.txt")
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def measure(variants, sets):
    """{variant: (median us/call, window range)}: every variant warmed on every set, the windows alternated."""
    times = {v: [] for v in variants}
    with torch.no_grad():
        for fn in variants.values():
            for i in range(sets):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for v, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(a.calls):
                    fn(c % sets)
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) / a.calls * 1e3)
    return {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}


def grouped(K, N, T, routing, E=8):
    from fused_int4_amd import routing as R
    if routing == "skewed":
        idx = R.simulate_routing(T // 2, E, 2, "skewed", dev, 42).expert_indices
        tpe = torch.bincount(idx.flatten().long(), minlength=E).to(torch.int32)
    else:
        tpe = torch.full((E,), T // E, dtype=torch.int32, device=dev)
    offs = (torch.cumsum(tpe, 0) - tpe).to(torch.int32)
    seg = list(zip(offs.tolist(), tpe.tolist()))                # (host copies for the loop of dense calls only)
    sets = min(max(2, -(-MALL // (E * N * K // 2)) + 1), a.max_sets)
    lut, nv = [], []
    for _ in range(sets):
        codes = torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        lut.append((codes, torch.rand(E, N, K // 64, device=dev, generator=g) + 0.5))
        nv.append((codes, torch.randint(0x30, 0x48, (E, N, K // 16), device=dev, generator=g, dtype=torch.uint8), None))
    x = torch.randn(T, K, device=dev, generator=g).bfloat16()
    gy = torch.randn(T, N, device=dev, generator=g).bfloat16()
    gu = torch.randn(T, 2 * K, device=dev, generator=g).bfloat16()
    bf = torch.bfloat16

    def loop(op, rows, i, **kw):
        return [op(lut[i][0][e], lut[i][1][e], rows[lo:lo + n], **kw) for e, (lo, n) in enumerate(seg) if n]
    variants = {
        "a grouped forward": lambda i: ops.moe_forward_lut4(*lut[i], x, tpe, offs),
        "b dense-loop forward": lambda i: loop(ops.linear_forward_lut4, x, i),
        "c nvfp4 forward": lambda i: ops.moe_forward_nvfp4(*nv[i], x, tpe, offs),
        "a grouped input gradient": lambda i: ops.moe_backward_input_lut4(*lut[i], gy, tpe, offs, out_dtype=bf),
        "b dense-loop input gradient": lambda i: loop(ops.linear_backward_input_lut4, gy, i, out_dtype=bf),
        "c nvfp4 input gradient": lambda i: ops.moe_backward_input_nvfp4(*nv[i], gy, tpe, offs, out_dtype=bf),
    }
    if routing == "balanced" and K > N:                         # the gated down projection (no dense-loop form exists)
        variants["a grouped gated"] = lambda i: ops.moe_gated_forward_lut4(*lut[i], gu, tpe, offs)
        variants["c nvfp4 gated"] = lambda i: ops.moe_gated_forward_nvfp4(*nv[i], gu, tpe, offs)
    res = measure(variants, sets)
    say(f"E={E} K={K} N={N} T={T} {routing} {tpe.tolist()}: bfloat16 rows and results, {sets} weight sets, median of "
        f"{a.repeats} windows of {a.calls} calls")
    for v, (us, rng) in res.items():
        say(f"  {v:30s} {us:9.1f} us/call   (range {rng:6.1f})   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s")
    for kind in ("forward", "input gradient", "gated"):
        for other in ("b dense-loop", "c nvfp4"):
            if f"{other} {kind}" in res:
                new, old = res[f"a grouped {kind}"], res[f"{other} {kind}"]
                say(f"  a / {other[0]} {kind} = {new[0] / old[0]:.3f} "
                    f"({'beyond' if abs(new[0] - old[0]) > max(new[1], old[1]) else 'within'} the ranges)")
    del lut, nv
    torch.cuda.empty_cache()


def grouped_decode(E, top_k, K, N):
    from fused_int4_amd import _native
    L = _native.lib()
    sets = min(max(2, -(-MALL // (E * N * K // 2)) + 1), a.max_sets)
    lut = []
    for _ in range(sets):
        lut.append((torch.randint(0, 256, (E, N, K // 2), device=dev, generator=g, dtype=torch.uint8),
                    torch.rand(E, N, K // 64, device=dev, generator=g) + 0.5))
    say(f"E={E} top-{top_k} K={K} N={N}: bfloat16 rows and results, {sets} weight sets x {E} table rotations, median of "
        f"{a.repeats} windows of {a.calls} calls")

    def tables(tokens, rows):
        """The E rotations of one routing: `tokens` tokens with top_k distinct experts each, or `rows` balanced rows."""
        if tokens:
            idx = torch.stack([torch.randperm(E, generator=torch.Generator().manual_seed(7 + t))[:top_k] for t in range(tokens)])
            tpe = torch.bincount(idx.flatten(), minlength=E)
        else:
            tpe = torch.full((E,), rows // E)
        out = []
        for r in range(E):
            t = torch.roll(tpe, r).to(torch.int32)
            out.append((t.to(dev), (torch.cumsum(t, 0) - t).to(torch.int32).to(dev)))
        return out

    def variant(tabs, x, set_hooks, split_k=False):
        n = [0]

        def fn(_):
            set_hooks()
            i = n[0]
            n[0] += 1
            return ops.moe_forward_lut4(*lut[i % sets], x, *tabs[(i // sets) % E], split_k=split_k)
        return fn
    big, old = 1 << 30, (L.fql_tune_set_lut4_group_decode_max_rows(-1), L.fql_tune_set_lut4_group_split_max_rows(-1),
                         L.fql_tune_set_lut4_group_slices(-1))
    for tokens, rows in [(t, t * top_k) for t in (1, 2, 4, 16, 64)] + [(0, r) for r in (256, 512, 1024)]:
        tabs = tables(tokens, rows)
        x = torch.randn(rows, K, device=dev, generator=g).bfloat16()
        res = measure({"tile": variant(tabs, x, lambda: L.fql_tune_set_lut4_group_decode_max_rows(0)),
                       "decode": variant(tabs, x, lambda: L.fql_tune_set_lut4_group_decode_max_rows(big))}, sets)
        (tu, tr), (du, dr) = res["tile"], res["decode"]
        say(f"  T={rows:5d} ({tokens or '-'} tokens): tile {tu:8.1f} us (range {tr:5.1f})  decode {du:8.1f} us (range {dr:5.1f})  "
            f"decode / tile = {du / tu:.3f} ({'beyond' if abs(du - tu) > tr + dr else 'within'} the two ranges)")
    tabs, x = tables(1, top_k), torch.randn(top_k, K, device=dev, generator=g).bfloat16()
    L.fql_tune_set_lut4_group_split_max_rows(big)
    variants = {"decode": variant(tabs, x, lambda: L.fql_tune_set_lut4_group_decode_max_rows(big))}
    for S in (1, 2, 4, 8, 16):
        variants[f"split S={S}"] = variant(tabs, x, lambda S=S: L.fql_tune_set_lut4_group_slices(S), split_k=True)
    res = measure(variants, sets)
    du, dr = res["decode"]
    say(f"  one token (T={top_k}): decode {du:8.1f} us (range {dr:5.1f})")
    for v, (us, rng) in list(res.items())[1:]:
        say(f"    {v:11s} {us:8.1f} us (range {rng:5.1f})  split / decode = {us / du:.3f} "
            f"({'beyond' if abs(us - du) > rng + dr else 'within'} the two ranges)")
    for f, v in zip((L.fql_tune_set_lut4_group_decode_max_rows, L.fql_tune_set_lut4_group_split_max_rows, L.fql_tune_set_lut4_group_slices), old):
        f(v)
    del lut
    torch.cuda.empty_cache()


def shape(K, N, T):
    sets = min(max(2, -(-MALL // (N * K // 2)) + 1), a.max_sets)
    lut, nv = [], []
    for _ in range(sets):
        codes = torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        lut.append((codes, torch.rand(N, K // 64, device=dev, generator=g) + 0.5))
        nv.append((codes, torch.randint(0x30, 0x48, (N, K // 16), device=dev, generator=g, dtype=torch.uint8), None))
    x = torch.randn(T, K, device=dev, generator=g).bfloat16()
    gy = torch.randn(T, N, device=dev, generator=g).bfloat16()
    bf = torch.bfloat16
    variants = {
        "lut4 forward": lambda i: ops.linear_forward_lut4(*lut[i], x),
        "nvfp4 forward": lambda i: ops.linear_forward_nvfp4(*nv[i], x),
        "lut4 input gradient": lambda i: ops.linear_backward_input_lut4(*lut[i], gy, out_dtype=bf),
        "nvfp4 input gradient": lambda i: ops.linear_backward_input_nvfp4(*nv[i], gy, out_dtype=bf),
    }
    times = {v: [] for v in variants}
    with torch.no_grad():
        for fn in variants.values():                            # warm up every variant on every set
            for i in range(sets):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for v, fn in variants.items():                      # alternating: the variants share whatever else happens
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(a.calls):
                    fn(c % sets)
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) / a.calls * 1e3)
    res = {v: (statistics.median(t), max(t) - min(t)) for v, t in times.items()}
    say(f"K={K} N={N} T={T}: bfloat16 rows and results, {sets} weight sets, median of {a.repeats} windows of {a.calls} calls")
    for v, (us, rng) in res.items():
        say(f"  {v:22s} {us:9.1f} us/call   (range {rng:6.1f})   {2.0 * T * K * N / us / 1e6:7.1f} TFLOP/s")
    for kind in ("forward", "input gradient"):
        new, old = res[f"lut4 {kind}"], res[f"nvfp4 {kind}"]
        say(f"  lut4 / nvfp4 {kind} = {new[0] / old[0]:.3f} "
            f"({'beyond' if abs(new[0] - old[0]) > max(new[1], old[1]) else 'within'} the ranges)")
    del lut, nv
    torch.cuda.empty_cache()


if a.grouped_decode:
    for E, top_k, K, N in ((8, 2, 4096, 11008), (8, 2, 4096, 28672), (8, 2, 11008, 4096), (8, 2, 14336, 4096), (64, 6, 2048, 2816),
                           (64, 6, 1408, 2048)):
        grouped_decode(E, top_k, K, N)
elif a.grouped:
    for K, N in ((4096, 11008), (11008, 4096)):
        for T, routing in ((1024, "balanced"), (4096, "balanced"), (1024, "skewed")):
            grouped(K, N, T, routing)
else:
    for K, N in ((4096, 11008), (4096, 4096)):
        for T in a.rows:
            shape(K, N, T)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(report) + "\n")
