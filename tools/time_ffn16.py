"""Timing of the gated FFN experts + adapters on 16-bit activations at the headline shape (8 experts, 1024 balanced routed
rows, H 4096, F 11008, r = 16, default precision), one process, contenders alternated after warm-up, device events around
each call:
  a_fwd / a_bwd   a 16-bit caller of the float32 layer: x.float() through LoRAQuantizedMoEFFN, results cast back
  b_fwd / b_bwd   LoRAQuantizedMoEFFN(activation_dtype=dtype) on the 16-bit tensors
  gated_fwd, gated_shrink, gated_grad, swiglu_bwd, each _f32 and _16
                  the ops whose kernels read gate_up, on a float32 and on a 16-bit gate_up (--kernels; these are the calls
                  to look for in a rocprofv3 --kernel-trace --stats run)
Also the peak device memory of one forward + backward of (a) and of (b).  Prints one JSON line (median microseconds)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fused_int4_amd as fq  # noqa: E402
from fused_int4_amd import ops  # noqa: E402

PEAK_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=11008)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--dtype", choices=["bfloat16", "float16"], default="bfloat16")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="also time the ops that read gate_up, float32 and 16-bit")
    a = ap.parse_args()
    dev = torch.device("cuda")
    dt = getattr(torch, a.dtype)
    E, T, H, F, r = a.experts, a.rows, a.hidden, a.ffn, a.rank
    g = torch.Generator(device=dev).manual_seed(0)

    base = fq.QuantizedMoEFFN(E, H, F).to(dev)
    base.gate_up_packed.copy_(torch.randint(0, 256, (E, 2 * F, H // 2), dtype=torch.uint8, device=dev, generator=g))
    base.gate_up_scales.copy_(torch.rand(E, 2 * F, device=dev, generator=g) * 0.002 + 2e-4)
    base.gate_up_zero_points.copy_(torch.randint(0, 16, (E, 2 * F), device=dev, generator=g).float())
    base.down_packed.copy_(torch.randint(0, 256, (E, H, F // 2), dtype=torch.uint8, device=dev, generator=g))
    base.down_scales.copy_(torch.rand(E, H, device=dev, generator=g) * 0.002 + 2e-4)
    base.down_zero_points.copy_(torch.randint(0, 16, (E, H), device=dev, generator=g).float())
    m32 = fq.LoRAQuantizedMoEFFN.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        m32.gate_up_lora_B.normal_(0, 0.02, generator=g)
        m32.down_lora_B.normal_(0, 0.02, generator=g)
    m16 = fq.LoRAQuantizedMoEFFN.from_quantized(base, r, alpha=2 * r, activation_dtype=dt)
    for name in ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"):
        setattr(m16, name, getattr(m32, name))                       # the same parameters

    cnt = torch.full((E,), T // E, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
    cnt = cnt.to(dev)
    x = torch.randn(T, H, device=dev, generator=g).to(dt)
    gy = torch.randn(T, H, device=dev, generator=g).to(dt)
    params = tuple(m32.parameters())

    def a_fwd():
        return m32(x.float(), cnt, offs).to(dt)

    def b_fwd():
        return m16(x, cnt, offs)

    xa = x.clone().requires_grad_()
    ya = m32(xa.float(), cnt, offs).to(dt)                           # the casts are part of (a)'s graph
    xb = x.clone().requires_grad_()
    yb = m16(xb, cnt, offs)

    def step(layer_fwd):
        xs = x.clone().requires_grad_()
        y = layer_fwd(xs)
        return torch.autograd.grad(y, (xs,) + params, gy)

    peak = {}
    for k, f in (("a", lambda xs: m32(xs.float(), cnt, offs).to(dt)), ("b", lambda xs: m16(xs, cnt, offs))):
        step(f)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(f)
        torch.cuda.synchronize()
        peak[k] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)

    runs = {
        "a_fwd": a_fwd, "b_fwd": b_fwd,
        "a_bwd": lambda: torch.autograd.grad(ya, (xa,) + params, gy, retain_graph=True),
        "b_bwd": lambda: torch.autograd.grad(yb, (xb,) + params, gy, retain_graph=True),
    }
    kbytes = {}
    if a.kernels:
        gu32 = torch.randn(T, 2 * F, device=dev, generator=g)
        dh32 = torch.randn(T, F, device=dev, generator=g)
        dU = torch.randn(T, r, device=dev, generator=g)
        Ad = m32.down_lora_A.detach()
        dw = (base.down_packed, base.down_scales, base.down_zero_points)
        for tag, gu, dh, es in (("f32", gu32, dh32, 4), ("16", gu32.to(dt), dh32.to(dt), 2)):
            runs["gated_fwd_" + tag] = lambda gu=gu: ops.moe_gated_forward(*dw, gu, cnt, offs)
            runs["gated_shrink_" + tag] = lambda gu=gu: ops.lora_gated_shrink(gu, Ad, "rc", cnt, offs)
            runs["gated_grad_" + tag] = lambda gu=gu: ops.lora_gated_grad(gu, dU, "rc", E, cnt, offs)
            runs["swiglu_bwd_" + tag] = lambda gu=gu, dh=dh: ops.swiglu_backward(gu, dh)
            kbytes["gated_shrink_" + tag] = 2 * T * F * es + (E * r * F + T * r) * 4
            kbytes["gated_grad_" + tag] = 2 * T * F * es + (E * r * F + T * r) * 4
            kbytes["swiglu_bwd_" + tag] = 5 * T * F * es
            kbytes["gated_prepass_" + tag] = 2 * T * F * es + 3 * T * F          # pre-pass alone: gate_up in, three limb planes out
    times = {k: [] for k in runs}
    grad_mode = lambda k: torch.enable_grad() if k in ("a_bwd", "b_bwd") else torch.no_grad()
    for _ in range(a.warmup):
        for k, f in runs.items():
            with grad_mode(k):
                f()
    torch.cuda.synchronize()
    for _ in range(a.iters):
        for k, f in runs.items():
            with grad_mode(k):
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                f()
                en.record()
                en.synchronize()
            times[k].append(st.elapsed_time(en) * 1e3)
    med = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res = {"shape": f"E={E} rows={T} H={H} F={F} r={r} {a.dtype}", "median_us": med,
           "fwd_b_over_a": round(med["b_fwd"] / med["a_fwd"], 3), "bwd_b_over_a": round(med["b_bwd"] / med["a_bwd"], 3),
           "peak_fwd_bwd_MiB": peak, "algorithmic_bytes": kbytes,
           "frac_of_8TBps": {k: round(kbytes[k] / (med[k] * 1e-6) / PEAK_BPS, 3) for k in kbytes if k in med}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
