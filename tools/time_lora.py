"""LoRA timing at the headline MoE shape (8 experts, 1024 balanced routed rows, 4096 -> 11008, r = 16), one process,
contenders alternated after warm-up, device events around each call:
  base_fwd / lora_fwd      ops.moe_forward vs ops.moe_lora_forward (inference)
  base_bwd / lora_bwd      ops.moe_backward_input (dX) vs the LoRA node's backward (dX + dA + dB, autograd)
  shrink_x, expand_y, shrink_g, expand_dx, grad_a, grad_b
                           each adapter kernel alone (csrc/fql_lora.h), with its fraction of 8 TB/s on algorithmic bytes
  loop_fwd / loop_bwd      the same adapter as a float32 torch loop over experts, with autograd
Prints one JSON line (median microseconds per call, and the ratios)."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="run one contender only (profiling)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    E, T, K, N, r = a.experts, a.rows, a.hidden, a.ffn, a.rank
    s = 2.0
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=g)
    S = torch.rand(E, N, device=dev, generator=g) * 0.01 + 1e-3
    Z = torch.randint(0, 16, (E, N), device=dev, generator=g).float()
    cnt = torch.full((E,), T // E, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
    cnt = cnt.to(dev)
    bounds = [(e * (T // E), (e + 1) * (T // E)) for e in range(E)]
    x = torch.randn(T, K, device=dev)
    gy = torch.randn(T, N, device=dev)
    A = (torch.randn(E, r, K, device=dev) * 0.02).requires_grad_()
    B = (torch.randn(E, N, r, device=dev) * 0.02).requires_grad_()
    U = ops.lora_shrink(x, A.detach(), "rc", cnt, offs)
    dU = ops.lora_shrink(gy, B.detach(), "cr", cnt, offs, scale=s)
    ybuf = torch.randn(T, N, device=dev)
    dxbuf = torch.randn(T, K, device=dev)

    xg = x.clone().requires_grad_()
    y_lora = ops.moe_lora_forward(P, S, Z, xg, A, B, s, cnt, offs)

    def loop_fwd(xin, Ain, Bin):
        parts = [s * (xin[lo:hi] @ Ain[e].t()) @ Bin[e].t() for e, (lo, hi) in enumerate(bounds)]
        return ybuf + torch.cat(parts)

    xl = x.clone().requires_grad_()
    y_loop = loop_fwd(xl, A, B)

    def lora_bwd():
        torch.autograd.grad(y_lora, (xg, A, B), gy, retain_graph=True)

    def loop_bwd():
        torch.autograd.grad(y_loop, (xl, A, B), gy, retain_graph=True)

    Ad, Bd = A.detach(), B.detach()
    runs = {
        "base_fwd": lambda: ops.moe_forward(P, S, Z, x, None, cnt, offs),
        "lora_fwd": lambda: ops.moe_lora_forward(P, S, Z, x, Ad, Bd, s, cnt, offs),
        "base_bwd": lambda: ops.moe_backward_input(P, S, Z, gy, cnt, offs),
        "lora_bwd": lora_bwd,
        "shrink_x": lambda: ops.lora_shrink(x, Ad, "rc", cnt, offs),
        "expand_y": lambda: ops.lora_expand(U, Bd, "cr", cnt, offs, scale=s, input=ybuf, out=ybuf),
        "shrink_g": lambda: ops.lora_shrink(gy, Bd, "cr", cnt, offs, scale=s),
        "expand_dx": lambda: ops.lora_expand(dU, Ad, "rc", cnt, offs, input=dxbuf, out=dxbuf),
        "grad_a": lambda: ops.lora_grad(x, dU, "rc", E, cnt, offs),
        "grad_b": lambda: ops.lora_grad(gy, U, "cr", E, cnt, offs, scale=s),
        "loop_fwd": lambda: loop_fwd(x, Ad, Bd),
        "loop_bwd": loop_bwd,
    }
    # algorithmic bytes: the [T, C] operand(s) once, the adapter weights once, the [T, r] operand once
    f4 = 4
    kbytes = {
        "shrink_x": (T * K + E * r * K + T * r) * f4,
        "expand_y": (2 * T * N + E * N * r + T * r) * f4,
        "shrink_g": (T * N + E * N * r + T * r) * f4,
        "expand_dx": (2 * T * K + E * r * K + T * r) * f4,
        "grad_a": (T * K + T * r + E * r * K) * f4,
        "grad_b": (T * N + T * r + E * N * r) * f4,
    }
    if a.only:
        runs = {k: runs[k] for k in a.only.split(",")}
    times = {k: [] for k in runs}
    for _ in range(a.warmup):
        for f in runs.values():
            with torch.no_grad() if not f.__name__.endswith("bwd") else torch.enable_grad():
                f()
    torch.cuda.synchronize()
    for _ in range(a.iters):
        for k, f in runs.items():
            with torch.no_grad() if not k.endswith("bwd") else torch.enable_grad():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                f()
                en.record()
                en.synchronize()
            times[k].append(st.elapsed_time(en) * 1e3)
    med = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res = {"shape": f"E={E} rows={T} {K} -> {N} r={r}", "median_us": med}
    res["frac_of_8TBps"] = {k: round(kbytes[k] / (med[k] * 1e-6) / PEAK_BPS, 3) for k in kbytes if k in med}
    if {"base_fwd", "lora_fwd"} <= med.keys():
        res["fwd_adapter_us"] = round(med["lora_fwd"] - med["base_fwd"], 1)
        res["fwd_overhead"] = round(med["lora_fwd"] / med["base_fwd"] - 1, 3)
    if {"base_bwd", "lora_bwd"} <= med.keys():
        res["bwd_adapter_us"] = round(med["lora_bwd"] - med["base_bwd"], 1)
        res["bwd_overhead"] = round(med["lora_bwd"] / med["base_bwd"] - 1, 3)
    if {"loop_fwd", "shrink_x", "expand_y"} <= med.keys():
        res["loop_fwd_over_fused"] = round(med["loop_fwd"] / (med["shrink_x"] + med["expand_y"]), 2)
    if {"loop_bwd", "shrink_g", "expand_dx", "grad_a", "grad_b"} <= med.keys():
        fused = med["shrink_g"] + med["expand_dx"] + med["grad_a"] + med["grad_b"]
        res["loop_bwd_over_fused"] = round(med["loop_bwd"] / fused, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
