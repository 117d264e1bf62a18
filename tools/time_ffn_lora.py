"""Timing of the adapters on the gated FFN experts at the headline shape (8 experts, 1024 balanced routed rows, H 4096,
F 11008, r = 16), one process, contenders alternated after warm-up, device events around each call:
  base_fwd / lora_fwd       QuantizedMoEFFN vs LoRAQuantizedMoEFFN (inference)
  base_bwd / lora_bwd       backward of QuantizedMoEFFN (dx) vs the LoRA node's (dx + four adapter gradients)
  gated_shrink, gated_grad, swiglu_bwd
                            each new kernel alone (csrc/fql_lora.h), with its fraction of 8 TB/s on algorithmic bytes
  h_torch                   the torch ops that materialise h = silu(g) * u ([T, F])
  plain_shrink, plain_grad  lora_shrink / lora_grad on that materialised h (what the gated kernels replace, with h_torch)
  swiglu_torch              the elementwise sequence of _GatedFFNFn.backward that swiglu_bwd replaces
  loop_fwd / loop_bwd       the same four adapters as a float32 torch loop over experts with autograd: adapter terms
                            and the gate only, random tensors stand for the INT4 GEMMs' outputs
Prints one JSON line (median microseconds per call, and the ratios)."""
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


def swiglu_torch(gate_up, dh):
    """The elementwise part of _GatedFFNFn.backward (moe.py), verbatim."""
    K = gate_up.shape[1] // 2
    g, u = gate_up[:, :K], gate_up[:, K:]
    sig = torch.sigmoid(g)
    return torch.cat([dh * u * (sig * (1.0 + g * (1.0 - sig))), dh * (g * sig)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=11008)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="run these contenders only, comma separated (profiling)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    E, T, H, F, r = a.experts, a.rows, a.hidden, a.ffn, a.rank
    g = torch.Generator(device=dev).manual_seed(0)

    base = fq.QuantizedMoEFFN(E, H, F).to(dev)
    base.gate_up_packed.copy_(torch.randint(0, 256, (E, 2 * F, H // 2), dtype=torch.uint8, device=dev, generator=g))
    base.gate_up_scales.copy_(torch.rand(E, 2 * F, device=dev, generator=g) * 0.002 + 2e-4)
    base.gate_up_zero_points.copy_(torch.randint(0, 16, (E, 2 * F), device=dev, generator=g).float())
    base.down_packed.copy_(torch.randint(0, 256, (E, H, F // 2), dtype=torch.uint8, device=dev, generator=g))
    base.down_scales.copy_(torch.rand(E, H, device=dev, generator=g) * 0.002 + 2e-4)
    base.down_zero_points.copy_(torch.randint(0, 16, (E, H), device=dev, generator=g).float())
    m = fq.LoRAQuantizedMoEFFN.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        m.gate_up_lora_B.normal_(0, 0.02, generator=g)
        m.down_lora_B.normal_(0, 0.02, generator=g)
    s = m.scaling

    cnt = torch.full((E,), T // E, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
    cnt = cnt.to(dev)
    bounds = [(e * (T // E), (e + 1) * (T // E)) for e in range(E)]
    x = torch.randn(T, H, device=dev, generator=g)
    gy = torch.randn(T, H, device=dev, generator=g)
    gate_up = torch.randn(T, 2 * F, device=dev, generator=g)
    dh = torch.randn(T, F, device=dev, generator=g)
    Ad = m.down_lora_A.detach()
    dU = torch.randn(T, r, device=dev, generator=g)
    h = torch.nn.functional.silu(gate_up[:, :F]) * gate_up[:, F:]

    xb = x.clone().requires_grad_()
    y_base = base(xb, cnt, offs)
    xg = x.clone().requires_grad_()
    y_lora = m(xg, cnt, offs)
    params = tuple(m.parameters())

    # the adapters alone as a float32 torch loop over experts: gu_base / y_base stand for the INT4 GEMMs' outputs
    gu_base = torch.randn(T, 2 * F, device=dev, generator=g)
    yd_base = torch.randn(T, H, device=dev, generator=g)

    def loop_fwd(xin, Agu, Bgu, Ad_, Bd_):
        gu = gu_base + torch.cat([s * (xin[lo:hi] @ Agu[e].t()) @ Bgu[e].t() for e, (lo, hi) in enumerate(bounds)])
        hh = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
        return yd_base + torch.cat([s * (hh[lo:hi] @ Ad_[e].t()) @ Bd_[e].t() for e, (lo, hi) in enumerate(bounds)])

    xl = x.clone().requires_grad_()
    y_loop = loop_fwd(xl, m.gate_up_lora_A, m.gate_up_lora_B, m.down_lora_A, m.down_lora_B)
    det = tuple(p.detach() for p in (m.gate_up_lora_A, m.gate_up_lora_B, m.down_lora_A, m.down_lora_B))

    runs = {
        "base_fwd": lambda: base(x, cnt, offs),
        "lora_fwd": lambda: m(x, cnt, offs),
        "base_bwd": lambda: torch.autograd.grad(y_base, (xb,), gy, retain_graph=True),
        "lora_bwd": lambda: torch.autograd.grad(y_lora, (xg,) + params, gy, retain_graph=True),
        "gated_shrink": lambda: ops.lora_gated_shrink(gate_up, Ad, "rc", cnt, offs),
        "gated_grad": lambda: ops.lora_gated_grad(gate_up, dU, "rc", E, cnt, offs),
        "swiglu_bwd": lambda: ops.swiglu_backward(gate_up, dh),
        "h_torch": lambda: torch.nn.functional.silu(gate_up[:, :F]) * gate_up[:, F:],
        "plain_shrink": lambda: ops.lora_shrink(h, Ad, "rc", cnt, offs),
        "plain_grad": lambda: ops.lora_grad(h, dU, "rc", E, cnt, offs),
        "swiglu_torch": lambda: swiglu_torch(gate_up, dh),
        "loop_fwd": lambda: loop_fwd(x, *det),
        "loop_bwd": lambda: torch.autograd.grad(y_loop, (xl,) + params, gy, retain_graph=True),
    }
    f4 = 4
    kbytes = {       # algorithmic: every operand once
        "gated_shrink": (2 * T * F + E * r * F + T * r) * f4,
        "gated_grad": (2 * T * F + T * r + E * r * F) * f4,
        "swiglu_bwd": 20 * T * F,
        "swiglu_torch": 20 * T * F,
        "plain_shrink": (T * F + E * r * F + T * r) * f4,
        "plain_grad": (T * F + T * r + E * r * F) * f4,
    }
    if a.only:
        runs = {k: runs[k] for k in a.only.split(",")}
    times = {k: [] for k in runs}
    for _ in range(a.warmup):
        for k, f in runs.items():
            with torch.enable_grad() if k.endswith("bwd") and k != "swiglu_bwd" else torch.no_grad():
                f()
    torch.cuda.synchronize()
    for _ in range(a.iters):
        for k, f in runs.items():
            with torch.enable_grad() if k.endswith("bwd") and k != "swiglu_bwd" else torch.no_grad():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                f()
                en.record()
                en.synchronize()
            times[k].append(st.elapsed_time(en) * 1e3)
    med = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res = {"shape": f"E={E} rows={T} H={H} F={F} r={r}", "median_us": med}
    res["frac_of_8TBps"] = {k: round(kbytes[k] / (med[k] * 1e-6) / PEAK_BPS, 3) for k in kbytes if k in med}
    has = lambda *ks: set(ks) <= med.keys()
    if has("base_fwd", "lora_fwd"):
        res["fwd_adapter_us"] = round(med["lora_fwd"] - med["base_fwd"], 1)
        res["fwd_overhead"] = round(med["lora_fwd"] / med["base_fwd"] - 1, 3)
    if has("base_bwd", "lora_bwd"):
        res["bwd_adapter_us"] = round(med["lora_bwd"] - med["base_bwd"], 1)
        res["bwd_overhead"] = round(med["lora_bwd"] / med["base_bwd"] - 1, 3)
    if has("loop_fwd", "base_fwd", "lora_fwd"):
        res["loop_fwd_over_fused"] = round(med["loop_fwd"] / max(res["fwd_adapter_us"], 1.0), 2)
    if has("loop_bwd", "lora_bwd"):
        # the base backward runs the torch elementwise sequence, the LoRA node swiglu_bwd, so lora_bwd - base_bwd is not
        # the adapters' cost (it can be negative); compare the loop with the WHOLE LoRA backward, INT4 GEMMs included
        res["loop_bwd_over_whole_lora_bwd"] = round(med["loop_bwd"] / med["lora_bwd"], 2)
    if has("base_bwd", "lora_bwd", "swiglu_bwd", "swiglu_torch"):
        like = med["lora_bwd"] - (med["base_bwd"] - med["swiglu_torch"] + med["swiglu_bwd"])
        res["bwd_adapter_us_same_gate_kernel"] = round(like, 1)     # base backward with the gate's kernel swapped in
    if has("swiglu_bwd", "swiglu_torch"):
        res["swiglu_torch_over_kernel"] = round(med["swiglu_torch"] / med["swiglu_bwd"], 2)
    if has("gated_shrink", "h_torch", "plain_shrink"):
        res["shrink_replaced_over_gated"] = round((med["h_torch"] + med["plain_shrink"]) / med["gated_shrink"], 2)
    if has("gated_grad", "h_torch", "plain_grad"):
        res["grad_replaced_over_gated"] = round((med["h_torch"] + med["plain_grad"]) / med["gated_grad"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
