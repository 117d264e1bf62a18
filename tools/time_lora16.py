"""bfloat16 LoRA timing at the headline MoE shape (8 experts, 1024 balanced routed rows, 4096 -> 11008, r = 16, default
precision), one process, contenders alternated after warm-up, device events around each call, median of --iters calls:

  cast_fwd / cast_bwd    (a) what a bfloat16 caller had before the 16-bit path: x.float(), the float32 LoRAMoEINT4 forward,
                         y cast back to bfloat16; backward: gy.float(), the float32 node's backward, dX cast back.  Uses only
                         what the float32 path offers, so this route also runs on a build without the 16-bit path.
  bf16_fwd / bf16_bwd    (b) the 16-bit path: x, y, gy and dX are bfloat16 end to end, nothing is cast.
  <kernel>_f32 / _bf16   each adapter kernel and the base input gradient alone, float32 against bfloat16 operands, with the
                         algorithmic bytes and their fraction of 8 TB/s (--kernels).

The forward of both routes runs under autograd (it saves for the backward); the backward is torch.autograd.grad on a
retained graph.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fused_int4_amd  # noqa: E402,F401
from fused_int4_amd import ops  # noqa: E402

PEAK_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=11008)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="also time every kernel alone, float32 against bfloat16")
    ap.add_argument("--only", default=None, help="comma-separated contenders (profiling)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    bf = torch.bfloat16
    E, T, K, N, r = a.experts, a.rows, a.hidden, a.ffn, a.rank
    s = 2.0
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=g)
    S = torch.rand(E, N, device=dev, generator=g) * 0.01 + 1e-3
    Z = torch.randint(0, 16, (E, N), device=dev, generator=g).float()
    cnt = torch.full((E,), T // E, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
    cnt = cnt.to(dev)
    x16 = torch.randn(T, K, device=dev, generator=g).to(bf)
    gy16 = torch.randn(T, N, device=dev, generator=g).to(bf)
    A = (torch.randn(E, r, K, device=dev, generator=g) * 0.02).requires_grad_()
    B = (torch.randn(E, N, r, device=dev, generator=g) * 0.02).requires_grad_()
    has16 = hasattr(ops._native.lib(), "fql_lora_shrink")

    def cast_fwd(xin=x16):
        return ops.moe_lora_forward(P, S, Z, xin.float(), A, B, s, cnt, offs).to(bf)

    def bf16_fwd(xin=x16):
        return ops.moe_lora_forward(P, S, Z, xin, A, B, s, cnt, offs)

    # graphs for the backward: the casts of route (a) are autograd nodes of their own, so its backward pays for
    # gy.float() and dX.to(bfloat16) exactly as a caller's would
    xa = x16.clone().requires_grad_()
    ya = cast_fwd(xa)
    runs = {"cast_fwd": cast_fwd, "cast_bwd": lambda: torch.autograd.grad(ya, (xa, A, B), gy16, retain_graph=True)}
    if has16:
        xb = x16.clone().requires_grad_()
        yb = bf16_fwd(xb)
        runs["bf16_fwd"] = bf16_fwd
        runs["bf16_bwd"] = lambda: torch.autograd.grad(yb, (xb, A, B), gy16, retain_graph=True)

    kbytes = {}
    if a.kernels and has16:
        Ad, Bd = A.detach(), B.detach()
        x32, gy32 = x16.float(), gy16.float()
        U = ops.lora_shrink(x16, Ad, "rc", cnt, offs)
        dU = ops.lora_shrink(gy16, Bd, "cr", cnt, offs, scale=s)
        y32 = torch.randn(T, N, device=dev, generator=g)
        dx32 = torch.randn(T, K, device=dev, generator=g)
        y16o = torch.empty(T, N, device=dev, dtype=bf)
        dx16o = torch.empty(T, K, device=dev, dtype=bf)
        wA, wB, tr = E * r * K * 4, E * N * r * 4, T * r * 4
        for tag, xx, gg, es in (("f32", x32, gy32, 4), ("bf16", x16, gy16, 2)):
            runs[f"shrink_x_{tag}"] = lambda xx=xx: ops.lora_shrink(xx, Ad, "rc", cnt, offs)
            runs[f"shrink_g_{tag}"] = lambda gg=gg: ops.lora_shrink(gg, Bd, "cr", cnt, offs, scale=s)
            runs[f"grad_a_{tag}"] = lambda xx=xx: ops.lora_grad(xx, dU, "rc", E, cnt, offs)
            runs[f"grad_b_{tag}"] = lambda gg=gg: ops.lora_grad(gg, U, "cr", E, cnt, offs, scale=s)
            kbytes[f"shrink_x_{tag}"] = T * K * es + wA + tr
            kbytes[f"shrink_g_{tag}"] = T * N * es + wB + tr
            kbytes[f"grad_a_{tag}"] = T * K * es + wA + tr
            kbytes[f"grad_b_{tag}"] = T * N * es + wB + tr
            runs[f"base_bwd_{tag}"] = lambda gg=gg: ops.moe_backward_input(P, S, Z, gg, cnt, offs)
        # expand: the float32 layer runs in place on float32; the 16-bit layer reads float32 and writes bfloat16
        runs["expand_y_f32"] = lambda: ops.lora_expand(U, Bd, "cr", cnt, offs, scale=s, input=y32, out=y32)
        runs["expand_y_bf16"] = lambda: ops.lora_expand(U, Bd, "cr", cnt, offs, scale=s, input=y32, out=y16o)
        runs["expand_dx_f32"] = lambda: ops.lora_expand(dU, Ad, "rc", cnt, offs, input=dx32, out=dx32)
        runs["expand_dx_bf16"] = lambda: ops.lora_expand(dU, Ad, "rc", cnt, offs, input=dx32, out=dx16o)
        kbytes["expand_y_f32"] = 8 * T * N + wB + tr
        kbytes["expand_y_bf16"] = 6 * T * N + wB + tr
        kbytes["expand_dx_f32"] = 8 * T * K + wA + tr
        kbytes["expand_dx_bf16"] = 6 * T * K + wA + tr

    if a.only:
        runs = {k: runs[k] for k in a.only.split(",")}
    times = {k: [] for k in runs}
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(a.iters):
        for k, f in runs.items():
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            f()
            en.record()
            en.synchronize()
            times[k].append(st.elapsed_time(en) * 1e3)
    med = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res = {"shape": f"E={E} rows={T} {K} -> {N} r={r} bf16", "iters": a.iters, "has_16bit_path": has16, "median_us": med}
    if kbytes:
        res["algorithmic_bytes"] = {k: v for k, v in kbytes.items() if k in med}
        res["frac_of_8TBps"] = {k: round(kbytes[k] / (med[k] * 1e-6) / PEAK_BPS, 3) for k in kbytes if k in med}
    for ph in ("fwd", "bwd"):
        if {f"cast_{ph}", f"bf16_{ph}"} <= med.keys():
            res[f"{ph}_bf16_over_cast"] = round(med[f"bf16_{ph}"] / med[f"cast_{ph}"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
