"""Bit-for-bit fingerprint of the operator boundary: one fixed, seeded list of calls into ``ops`` (and the gated FFN
modules) on tiny shapes that still reach every branch of the wrappers; for each call one line per returned tensor and,
for the differentiable ops, per gradient: ``name  dtype  shape  sha256``.  Two checkouts that print the same lines on
the same machine compute the same bits through the Python layer.  ``--list`` prints the call names without a GPU.

Branches reached: GEMV (B = 1, 2), generic (K = 34), MFMA (B = 48, K = 64, N = 40); grouped calls on E = 3 with one empty
expert and four uncovered tail rows; per-group scales (K = 128, group 64) at B = 2 and 48; 16-bit calls on the native
path (K = 64) and on the widened fallback (K = 34); bias present and absent; 1-D and 2-D input; a misaligned float32 view
as LoRA weight and as ``v`` (the ``clone()`` branches); LoRA ranks 4 and 64; C = 30, 34, 64 (vector widths 1, 2, 4);
``lora_expand`` in place and with ``out_dtype``; ``combine`` with and without weights; the LoRA layers and the gated FFN
in float32, float16 and bfloat16 with every gradient and with the input gradient alone; the router at every group width
(E = 1, 2, 5, 8, 60, 128: G = 1 .. 64, one and two experts per lane), top_k 1, 2 and 8, three logit types, renormalised or
not, with a +inf row, an all-equal row and a row of mixed 0.0 / -0.0, each backward with both gradients and with either
alone, ``router_score_topk`` at its defaults (the plain kernel variant) and with sigmoid + bias + groups + scale (the
scored one); ``combine_any`` on four type pairs at N = 40 (16-byte accesses), 130 (pairs) and 129 (scalars), with and
without the addend and its weight, and the float32 ``combine`` on a misaligned ``y``; ``QuantizedSparseMoEBlock`` with
default and with scored routing, float32 and bfloat16, every gradient; and, behind all of these so that their operands are
the ones they always were, the four gated ops, the gated FFN layers and the sparse block (with a shared expert) for
``activation="gelu_tanh"`` and ``"swiglu_clamp"`` in the three element types; and behind those the MXFP4 experts at K = 96
(K % 64 == 32) and N = 40 on the same grouped table: ``moe_forward_mxfp4`` and ``moe_gated_forward_mxfp4`` in the three
precisions, ``moe_forward_mxfp4_fp8`` and ``moe_forward_mxfp4_fp4``, float32 and bfloat16 rows, with and without a bias, each
once on its decode kernel and once on its tile kernel (forced through the tuning hooks), then ``quantize_rows_mxfp4`` plain
and gated and ``moe_backward_input_mxfp4``; last the same lines for ``precision="fp6"``, ``moe_forward_mxfp4_fp6`` and
``quantize_rows_mxfp6``; and behind those the dense MXFP4 linear ops on one expert's matrix and 16 rows:
``linear_forward_mxfp4`` and ``linear_gated_forward_mxfp4`` with the tile kernel, the grouped decode kernel and the split
form at 2 and at 16 slices forced in turn, then ``linear_backward_input_mxfp4``; then the NVFP4 forward ops, decode and
tile, then ``moe_backward_input_nvfp4`` / ``linear_backward_input_nvfp4`` on the same operands, and last the five NVFP4 adapter
ops (``moe_forward_nvfp4_lora`` and its kin) on them."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

E, TAIL = 3, 4
COUNTS = [29, 0, 19]                       # one empty expert; T = 48 + TAIL rows, the last TAIL covered by no expert
T = sum(COUNTS) + TAIL
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


class Data:
    """Every operand comes from one CPU generator (seed 0), in a fixed order, then moves to the device."""

    def __init__(self, dev):
        self.dev = dev
        self.gen = torch.Generator().manual_seed(0)

    def randn(self, *shape, dtype=F32, scale=1.0):
        return (torch.randn(shape, generator=self.gen) * scale).to(dtype).to(self.dev)

    def weights(self, *shape, groups=None):
        """(packed uint8 [..., K/2], scales, zero_points [...] or [..., groups]) of random INT4 weights [..., K]."""
        *lead, K = shape
        packed = torch.randint(0, 256, (*lead, K // 2), dtype=torch.uint8, generator=self.gen)
        sz = tuple(lead) if groups is None else (*lead, groups)
        scales = torch.rand(sz, generator=self.gen) * 0.02 + 0.002
        zps = torch.randint(0, 16, sz, generator=self.gen).float()
        return packed.to(self.dev), scales.to(self.dev), zps.to(self.dev)

    def table(self):
        cnt = torch.tensor(COUNTS, dtype=torch.int32)
        return cnt.to(self.dev), (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(self.dev)

    def misaligned(self, t):
        """``buf[1:]`` of a float32 buffer: contiguous, 4 bytes past the allocation's alignment."""
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        return view


def with_grads(fn, tensors, gy_of, only_first=False):
    """Run ``fn(*leaves)`` under autograd on detached copies of ``tensors`` (all requiring grad, or the first alone) and
    return (output, grad of each leaf that required one)."""
    leaves = [t.detach().clone().requires_grad_(i == 0 or not only_first) for i, t in enumerate(tensors)]
    y = fn(*leaves)
    y.backward(gy_of(y))
    return (y.detach(),) + tuple(t.grad for t in leaves if t.requires_grad)


def calls(dev, fq, ops):
    d = Data(dev)
    tpe, offs = d.table()

    # ---------------------------------------------------------------- linear: GEMV, generic, MFMA, per-group, 16-bit
    for B, K, N in ((1, 64, 40), (2, 64, 40), (2, 34, 40), (48, 34, 40), (48, 64, 40)):
        p, s, z = d.weights(N, K)
        x, bias = d.randn(B, K), d.randn(N)
        yield f"linear_forward B{B} K{K}", lambda: ops.linear_forward(x, p, s, z)
        yield f"linear_forward B{B} K{K} bias", lambda: ops.linear_forward(x, p, s, z, bias=bias)
        yield f"linear_forward B{B} K{K} 1-D", lambda: ops.linear_forward(x[0], p, s, z, precision="fast")
        for dt in (F16, BF16):
            yield f"linear_forward_any B{B} K{K} {dt}", lambda: ops.linear_forward_any(x.to(dt), p, s, z, bias=bias)
            yield f"linear_forward_any B{B} K{K} f32->{dt}", lambda: ops.linear_forward_any(x, p, s, z, out_dtype=dt)
        yield f"linear_forward grad B{B} K{K}", lambda: with_grads(
            lambda x_, b_: ops.linear_forward(x_, p, s, z, bias=b_), (x, bias), torch.ones_like)
        gy = d.randn(B, N)
        for dt in (F32, F16, BF16):
            yield f"linear_backward_input B{B} K{K} {dt}", lambda: ops.linear_backward_input(gy.to(dt), p, s, z, out_dtype=dt)
    for B in (2, 48):
        p, s, z = d.weights(40, 128, groups=2)
        x, bias = d.randn(B, 128), d.randn(40)
        yield f"linear_forward per-group B{B}", lambda: ops.linear_forward(x, p, s, z)
        yield f"linear_forward per-group B{B} bias 1-D", lambda: ops.linear_forward(x[0], p, s, z, bias=bias, precision="int8")
        yield f"linear_forward per-group grad B{B}", lambda: with_grads(
            lambda x_, b_: ops.linear_forward(x_, p, s, z, bias=b_), (x, bias), torch.ones_like)
    pg, sg, zg = d.weights(E, 40, 128, groups=2)
    xg = d.randn(T, 128)
    yield "moe_group_forward", lambda: ops.moe_group_forward(pg, sg, zg, xg, tpe, offs)
    yield "moe_group_forward int8", lambda: ops.moe_group_forward(pg, sg, zg, xg, tpe, offs, precision="int8")
    p, s, z = d.weights(40, 64)
    w = d.randn(40, 64)
    yield "quantize_rows", lambda: ops.quantize_rows(w)
    yield "quantize_tensor", lambda: ops.quantize_tensor(w)
    yield "unpack_nibbles", lambda: ops.unpack_nibbles(p)
    yield "dequantize_forward", lambda: ops.dequantize_forward(p, s, z)

    # ---------------------------------------------------------------- grouped: E = 3, one empty expert, 4 tail rows
    for K in (64, 34):
        P, S, Z = d.weights(E, 40, K)
        x, gy = d.randn(T, K), d.randn(T, 40)
        yield f"moe_forward K{K}", lambda: ops.moe_forward(P, S, Z, x, None, tpe, offs)
        yield f"moe_forward K{K} exact", lambda: ops.moe_forward(P, S, Z, x, None, tpe, offs, precision="exact")
        for dt in (F16, BF16):
            yield f"moe_forward_any K{K} {dt}", lambda: ops.moe_forward_any(P, S, Z, x.to(dt), None, tpe, offs)
            yield f"moe_forward_any K{K} {dt}->f32", lambda: ops.moe_forward_any(P, S, Z, x.to(dt), None, tpe, offs, out_dtype=F32)
            yield f"moe_backward_input K{K} {dt}", lambda: ops.moe_backward_input(P, S, Z, gy.to(dt), tpe, offs, out_dtype=dt)
            yield f"moe_forward_any grad K{K} {dt}", lambda: with_grads(
                lambda x_: ops.moe_forward_any(P, S, Z, x_, None, tpe, offs), (x.to(dt),), torch.ones_like)
        yield f"moe_backward_input K{K}", lambda: ops.moe_backward_input(P, S, Z, gy, tpe, offs)
        yield f"moe_forward grad K{K}", lambda: with_grads(
            lambda x_: ops.moe_forward(P, S, Z, x_, None, tpe, offs), (x,), torch.ones_like)
    P, S, Z = d.weights(E, 40, 64)
    x = d.randn(T, 64)
    tokens, ri, rw = d.randn(16, 64), (torch.arange(T, dtype=torch.int32) % 16).to(dev), d.randn(T)
    yield "moe_gather_forward", lambda: ops.moe_gather_forward(P, S, Z, tokens, ri, tpe, offs)
    yield "moe_gather_forward row_weight", lambda: ops.moe_gather_forward(P, S, Z, tokens, ri, tpe, offs, row_weight=rw)
    gu = d.randn(T, 128)
    for dt in (F32, F16, BF16):
        yield f"moe_gated_forward {dt}", lambda: ops.moe_gated_forward(P, S, Z, gu.to(dt), tpe, offs)
        yield f"moe_gated_forward {dt}->f32", lambda: ops.moe_gated_forward(P, S, Z, gu.to(dt), tpe, offs, out_dtype=F32)
        dh = d.randn(T, 64)
        yield f"swiglu_backward {dt}", lambda: ops.swiglu_backward(gu.to(dt), dh.to(dt))
        yield f"swiglu_backward {dt} mixed", lambda: ops.swiglu_backward(gu.to(dt), dh, out_dtype=F16)
    x8, asc = ops.quantize_activations_fp8(x)
    yield "moe_forward_fp8", lambda: ops.moe_forward_fp8(P, S, Z, x8, asc, tpe, offs)
    yield "moe_forward_fp8 f16 unscaled", lambda: ops.moe_forward_fp8(P, S, Z, x8, None, tpe, offs, out_dtype=F16)
    yield "linear_forward_fp8", lambda: ops.linear_forward_fp8(x8, asc, P[0], S[0], Z[0])
    yield "linear_forward_fp8 bf16 unscaled", lambda: ops.linear_forward_fp8(x8, None, P[0], S[0], Z[0], out_dtype=BF16)
    for prec in ("exact", "int8"):
        def two_phase(prec=prec, grouped=True):
            bufs = ops.act_quant(x, prec, tpe, offs) if grouped else ops.act_quant(x, prec)
            out = ops.gemm_i8(*bufs, P, S, Z, tpe, offs, precision=prec) if grouped else \
                ops.gemm_i8(*bufs, P[0], S[0], Z[0], precision=prec)
            return bufs[1], bufs[2], out
        yield f"act_quant + gemm_i8 grouped {prec}", two_phase
        yield f"act_quant + gemm_i8 one group {prec}", lambda: two_phase(grouped=False)

    # ---------------------------------------------------------------- routing
    idx = torch.randint(0, E, (24, 2), generator=d.gen).to(dev)
    yield "route_plan", lambda: ops.route_plan(idx, E)
    y, wts = d.randn(48, 40), d.randn(24, 2)
    pos = torch.randperm(48, generator=d.gen).to(torch.int32).to(dev)
    yield "combine", lambda: ops.combine(y, pos, wts)
    yield "combine unweighted", lambda: ops.combine(y, pos, None, top_k=2)
    yield "combine grad", lambda: with_grads(lambda y_, w_: ops.combine(y_, pos, w_), (y, wts), torch.ones_like)
    yield "combine grad unweighted", lambda: with_grads(lambda y_: ops.combine(y_, pos, None, top_k=2), (y,), torch.ones_like)
    yield "combine_backward short y", lambda: ops.combine_backward(d.randn(24, 40), d.randn(60, 40), pos, wts)[0]
    yield "regroup_index", lambda: ops.regroup_index(torch.tensor([[3, 0, 2], [1, 4, 0]], dtype=torch.int32, device=dev), 10)

    # ---------------------------------------------------------------- LoRA kernels: ranks 4 / 64, C = 30 / 34 / 64
    for r in (4, 64):
        for C in (30, 34, 64):
            A, Bw = d.randn(E, r, C, scale=0.1), d.randn(E, C, r, scale=0.1)
            xin, v, base = d.randn(T, C), d.randn(T, r), d.randn(T, C)
            gu2 = d.randn(T, 2 * C)
            for dt in (F32, F16, BF16):
                yield f"lora_shrink r{r} C{C} {dt}", lambda: ops.lora_shrink(xin.to(dt), A, "rc", tpe, offs, scale=0.5)
                yield f"lora_grad r{r} C{C} {dt}", lambda: ops.lora_grad(xin.to(dt), v, "cr", E, tpe, offs, scale=0.5)
                yield f"lora_gated_shrink r{r} C{C} {dt}", lambda: ops.lora_gated_shrink(gu2.to(dt), A, "rc", tpe, offs)
                yield f"lora_gated_grad r{r} C{C} {dt}", lambda: ops.lora_gated_grad(gu2.to(dt), v, "rc", E, tpe, offs)
                yield f"lora_expand r{r} C{C} ->{dt}", lambda: ops.lora_expand(v, Bw, "cr", tpe, offs, scale=2.0, input=base, out_dtype=dt)
            yield f"lora_shrink r{r} C{C} cr", lambda: ops.lora_shrink(xin, Bw, "cr", tpe, offs)
            yield f"lora_shrink r{r} C{C} one segment", lambda: ops.lora_shrink(xin, A[0], "rc")
            yield f"lora_shrink r{r} C{C} misaligned", lambda: ops.lora_shrink(xin, d.misaligned(A), "rc", tpe, offs)
            yield f"lora_gated_shrink r{r} C{C} misaligned", lambda: ops.lora_gated_shrink(gu2, d.misaligned(A), "rc", tpe, offs)
            yield f"lora_grad r{r} C{C} misaligned v", lambda: ops.lora_grad(xin, d.misaligned(v), "rc", E, tpe, offs)
            yield f"lora_gated_grad r{r} C{C} misaligned v", lambda: ops.lora_gated_grad(gu2, d.misaligned(v), "cr", E, tpe, offs)
            yield f"lora_expand r{r} C{C} in place", lambda: ops.lora_expand(v, Bw, "cr", tpe, offs, input=(b := base.clone()), out=b)
            yield f"lora_expand r{r} C{C} no input rc", lambda: ops.lora_expand(v, A, "rc", tpe, offs, out=torch.empty_like(base))
            yield f"lora_expand r{r} C{C} misaligned", lambda: ops.lora_expand(d.misaligned(v), d.misaligned(Bw), "cr", tpe, offs, input=base.to(BF16))

    # ---------------------------------------------------------------- the LoRA layers, f32 / f16 / bf16
    for r in (4, 64):
        for K, bias_on in ((64, True), (34, False)):
            p, s, z = d.weights(40, K)
            P, S, Z = d.weights(E, 40, K)
            A1, B1, bias = d.randn(r, K, scale=0.1), d.randn(40, r, scale=0.1), d.randn(40)
            A, Bm = d.randn(E, r, K, scale=0.1), d.randn(E, 40, r, scale=0.1)
            x1, x = d.randn(2, K), d.randn(T, K)
            for dt in (F32, F16, BF16):
                b = bias if bias_on else None
                yield f"linear_lora_forward r{r} K{K} {dt}", lambda: ops.linear_lora_forward(x.to(dt), p, s, z, A1, B1, 2.0, bias=b)
                yield f"linear_lora_forward r{r} K{K} {dt} 1-D", lambda: ops.linear_lora_forward(x1[0].to(dt), p, s, z, A1, B1, 2.0, bias=b)
                yield f"moe_lora_forward r{r} K{K} {dt}", lambda: ops.moe_lora_forward(P, S, Z, x.to(dt), A, Bm, 2.0, tpe, offs)
                for only in (False, True):
                    tag = "dx only" if only else "all grads"
                    yield f"linear_lora_forward r{r} K{K} {dt} {tag}", lambda: with_grads(
                        lambda x_, A_, B_: ops.linear_lora_forward(x_, p, s, z, A_, B_, 2.0, bias=b),
                        (x.to(dt), A1, B1), torch.ones_like, only)
                    yield f"moe_lora_forward r{r} K{K} {dt} {tag}", lambda: with_grads(
                        lambda x_, A_, B_: ops.moe_lora_forward(P, S, Z, x_, A_, B_, 2.0, tpe, offs),
                        (x.to(dt), A, Bm), torch.ones_like, only)
        pg, sg, zg = d.weights(40, 128, groups=2)
        A1, B1, x = d.randn(r, 128, scale=0.1), d.randn(40, r, scale=0.1), d.randn(T, 128)
        for dt in (F32, BF16):
            yield f"linear_lora_forward per-group r{r} {dt}", lambda: with_grads(
                lambda x_, A_, B_: ops.linear_lora_forward(x_, pg, sg, zg, A_, B_, 2.0), (x.to(dt), A1, B1), torch.ones_like)

    # ---------------------------------------------------------------- the gated FFN experts, with and without adapters
    H, F = 64, 32
    for r in (4, 64):
        gup, gus, guz = d.weights(E, 2 * F, H)
        dp, ds, dz = d.weights(E, H, F)
        ad = [d.randn(E, r, H, scale=0.1), d.randn(E, 2 * F, r, scale=0.1), d.randn(E, r, F, scale=0.1),
              d.randn(E, H, r, scale=0.1)]
        x, gy = d.randn(T, H), d.randn(T, H)
        for dt in (F32, F16, BF16):
            act = None if dt == F32 else dt
            m = fq.QuantizedMoEFFN(E, H, F, activation_dtype=act).to(dev)
            for name, buf in zip(("gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales",
                                  "down_zero_points"), (gup, gus, guz, dp, ds, dz)):
                setattr(m, name, buf)

            def layer(x_, *ad_):
                return ops.moe_ffn_lora_forward(gup, gus, guz, dp, ds, dz, x_, *ad_, 2.0, tpe, offs, activation_dtype=act)
            yield f"moe_ffn_lora_forward r{r} {dt}", lambda: layer(x.to(dt), *ad)
            yield f"QuantizedMoEFFN r{r} {dt}", lambda: m(x.to(dt), tpe, offs)
            yield f"QuantizedMoEFFN r{r} {dt} dx", lambda: with_grads(
                lambda x_: m(x_, tpe, offs), (x.to(dt),), lambda y_: gy.to(y_.dtype))
            for only in (False, True):
                yield f"moe_ffn_lora_forward r{r} {dt} {'dx only' if only else 'all grads'}", lambda: with_grads(
                    layer, (x.to(dt), *ad), lambda y_: gy.to(y_.dtype), only)


    # ---------------------------------------------------------------- the combine: misaligned float32, typed, addend
    for N in (40, 130):                      # y four bytes off its alignment: no 16-byte access, at N = 130 pairs for out alone
        ym, g = d.misaligned(d.randn(48, N)), d.randn(24, N)
        yield f"combine misaligned N{N}", lambda: ops.combine(ym, pos, wts)
        yield f"combine_backward misaligned N{N}", lambda: ops.combine_backward(g, ym, pos, wts)
    for N in (40, 129, 130):
        y, add, aw, g = d.randn(48, N), d.randn(24, N), d.randn(24), d.randn(24, N)
        for di, do in ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)):
            for tag, extra in (("", ()), (" addend", (add.to(di),)), (" weighted addend", (add.to(di), aw))):
                yield f"combine_any N{N} {di}->{do}{tag}", lambda: ops.combine_any(y.to(di), pos, wts, None, *extra, out_dtype=do)
                yield f"combine_any grad N{N} {di}->{do}{tag}", lambda: with_grads(
                    lambda y_, w_, *e_: ops.combine_any(y_, pos, w_, None, *e_, out_dtype=do), (y.to(di), wts, *extra),
                    lambda o_: g.to(o_.dtype))

    # ---------------------------------------------------------------- the router: every group width, special rows
    for Er in (1, 2, 5, 8, 60, 128):
        base = d.randn(37, Er)
        base[0, 0] = float("inf")
        base[1] = 0.25
        base[2, 0::2], base[2, 1::2] = 0.0, -0.0
        bias = d.randn(Er, scale=0.1)
        for k in (min(Er, 2),) + ((8,) if Er >= 8 else ()):
            gw, gp = d.randn(37, k), d.randn(37, Er)
            for dt in (F32, F16, BF16):
                logits = base.to(dt)
                for rn in (True, False):
                    tag = f"E{Er} k{k} {dt} renormalize={rn}"
                    yield f"router_topk {tag}", lambda: ops.router_topk(logits, k, renormalize=rn, return_probs=True)
                    yield f"router_topk_backward {tag}", lambda: [
                        ops.router_topk_backward(logits, ops.router_topk(logits, k, rn)[1], a, b, renormalize=rn)
                        for a, b in ((gw, gp), (gw, None), (None, gp))]
                    yield f"router_score_topk defaults {tag}", lambda: ops.router_score_topk(
                        logits, k, renormalize=rn, return_scores=True)
                    if Er in (8, 128) and 2 * (Er // 4) >= k:
                        rule = dict(scoring="sigmoid", renormalize=rn, scale=2.5)
                        yield f"router_score_topk scored {tag}", lambda: (out := ops.router_score_topk(
                            logits, k, select_bias=bias, n_group=4, topk_group=2, return_scores=True, **rule)) + (
                            ops.router_score_topk_backward(logits, out[1], gw, gp, **rule),)

    # ---------------------------------------------------------------- the sparse MoE block, default and scored routing
    Eb, H, F = 4, 64, 32
    gup, gus, guz = d.weights(Eb, 2 * F, H)
    dp, ds, dz = d.weights(Eb, H, F)
    gate_w, x, gy = d.randn(Eb, H), d.randn(37, H), d.randn(37, H)
    for tag, rule in (("default", {}), ("scored", dict(scoring="sigmoid", n_group=2, topk_group=1,
                                                       routed_scaling_factor=2.5, selection_bias=True))):
        for dt in (F32, BF16):
            m = fq.QuantizedSparseMoEBlock(Eb, H, F, activation_dtype=None if dt == F32 else dt, **rule).to(dev)
            for name, buf in zip(("gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales",
                                  "down_zero_points"), (gup, gus, guz, dp, ds, dz)):
                setattr(m.experts, name, buf)
            m.gate.weight.data.copy_(gate_w)

            def block(m=m, dt=dt):
                x_ = x.detach().clone().to(dt).requires_grad_(True)
                m.gate.weight.grad = None
                out, logits = m(x_)
                out.backward(gy.to(out.dtype))
                return out.detach(), logits.detach(), x_.grad, m.gate.weight.grad
            yield f"QuantizedSparseMoEBlock {tag} {dt}", block

    # ---------------------------------------------------------------- activation kinds of the gated FFN (GeGLU, clamped SwiGLU)
    # (behind everything else: the operands of the calls above come from the generator in the order they always did)
    P, S, Z = d.weights(E, 40, 64)
    gu, dh = d.randn(T, 128, scale=4.0), d.randn(T, 64)
    A, v = d.randn(E, 4, 64, scale=0.1), d.randn(T, 4)
    H, F, r = 64, 32, 4
    gup, gus, guz = d.weights(E, 2 * F, H)
    dp, ds, dz = d.weights(E, H, F)
    ad = [d.randn(E, r, H, scale=0.1), d.randn(E, 2 * F, r, scale=0.1), d.randn(E, r, F, scale=0.1), d.randn(E, H, r, scale=0.1)]
    x, gy = d.randn(T, H, scale=8.0), d.randn(T, H)
    gate_w = d.randn(E, H)
    for kind, kw in (("gelu_tanh", dict(activation="gelu_tanh")),
                     ("swiglu_clamp", dict(activation="swiglu_clamp", activation_alpha=1.702, activation_limit=7.0))):
        for dt in (F32, F16, BF16):
            yield f"moe_gated_forward {kind} {dt}", lambda: ops.moe_gated_forward(P, S, Z, gu.to(dt), tpe, offs, **kw)
            yield f"moe_gated_forward {kind} {dt}->f32", lambda: ops.moe_gated_forward(P, S, Z, gu.to(dt), tpe, offs, out_dtype=F32, **kw)
            yield f"lora_gated_shrink {kind} {dt}", lambda: ops.lora_gated_shrink(gu.to(dt), A, "rc", tpe, offs, **kw)
            yield f"lora_gated_grad {kind} {dt}", lambda: ops.lora_gated_grad(gu.to(dt), v, "rc", E, tpe, offs, **kw)
            yield f"glu_backward {kind} {dt}", lambda: ops.glu_backward(gu.to(dt), dh.to(dt), **kw)
            yield f"glu_backward {kind} {dt} mixed", lambda: ops.glu_backward(gu.to(dt), dh, out_dtype=F16, **kw)
            act = None if dt == F32 else dt
            m = fq.QuantizedMoEFFN(E, H, F, activation_dtype=act, **kw).to(dev)
            for name, buf in zip(("gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales",
                                  "down_zero_points"), (gup, gus, guz, dp, ds, dz)):
                setattr(m, name, buf)

            def layer(x_, *ad_):
                return ops.moe_ffn_lora_forward(gup, gus, guz, dp, ds, dz, x_, *ad_, 2.0, tpe, offs, activation_dtype=act, **kw)
            yield f"QuantizedMoEFFN {kind} {dt} dx", lambda: with_grads(
                lambda x_: m(x_, tpe, offs), (x.to(dt),), lambda y_: gy.to(y_.dtype))
            yield f"moe_ffn_lora_forward {kind} {dt} all grads", lambda: with_grads(
                layer, (x.to(dt), *ad), lambda y_: gy.to(y_.dtype))
        blk = fq.QuantizedSparseMoEBlock(E, H, F, top_k=2, shared_ffn_dim=F, **kw).to(dev)
        for mod, sl in ((blk.experts, slice(0, E)), (blk.shared_experts, slice(0, 1))):
            for name, buf in zip(("gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales",
                                  "down_zero_points"), (gup, gus, guz, dp, ds, dz)):
                setattr(mod, name, buf[sl])
        blk.gate.weight.data.copy_(gate_w)

        def glu_block(m=blk):
            x_ = x.detach().clone().requires_grad_(True)
            m.gate.weight.grad = None
            out, logits = m(x_)
            out.backward(gy)
            return out.detach(), logits.detach(), x_.grad, m.gate.weight.grad
        yield f"QuantizedSparseMoEBlock {kind} shared", glu_block

    # ---------------------------------------------------------------- the MXFP4 experts (behind everything else, as above)
    # K = 96: K % 64 == 32, a half-filled last matrix instruction of the block-scaled kernels; N = 40: a partial 32-n block.
    # Every forward runs once on its decode kernel and once on its tile kernel, forced through the tuning hooks.
    K, N = 96, 40
    Pm = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, generator=d.gen).to(dev)
    Sm = torch.randint(118, 133, (E, N, K // 32), dtype=torch.uint8, generator=d.gen).to(dev)
    x, gu, gy, biasm = d.randn(T, K), d.randn(T, 2 * K, scale=2.0), d.randn(T, N), d.randn(E, N)
    x8, asc = ops.quantize_activations_fp8(x)
    glu = dict(activation="swiglu_clamp", activation_alpha=1.702, activation_limit=7.0)

    def forced(which, call):
        def run():
            from fused_int4_amd import _native
            lib, rows = _native.lib(), 2 ** 31 - 1 if which == "decode" else 0
            old = [lib.fql_tune_set_mx4_decode_max_rows(rows)] + [lib.fql_tune_set_mx4_scaled_decode_max_rows(m, rows) for m in (1, 2)]
            try:
                return call()
            finally:
                lib.fql_tune_set_mx4_decode_max_rows(old[0])
                for m in (1, 2):
                    lib.fql_tune_set_mx4_scaled_decode_max_rows(m, old[m])
        return run

    for which in ("decode", "tile"):
        for btag, b in (("", None), (" bias", biasm)):
            for dt in (F32, BF16):
                for prec in ("bf16", "fp8", "fp4"):
                    tag = f"{prec} {dt}{btag} {which}"
                    yield f"moe_forward_mxfp4 {tag}", forced(which, lambda: ops.moe_forward_mxfp4(
                        Pm, Sm, x.to(dt), tpe, offs, bias=b, precision=prec))
                    yield f"moe_gated_forward_mxfp4 {tag}", forced(which, lambda: ops.moe_gated_forward_mxfp4(
                        Pm, Sm, gu.to(dt), tpe, offs, bias=b, precision=prec, **glu))
                    yield f"moe_forward_mxfp4 {tag} ->f16", forced(which, lambda: ops.moe_forward_mxfp4(
                        Pm, Sm, x.to(dt), tpe, offs, bias=b, out_dtype=F16, precision=prec))
            yield f"moe_forward_mxfp4_fp8{btag} {which}", forced(which, lambda: ops.moe_forward_mxfp4_fp8(
                Pm, Sm, x8, asc, tpe, offs, bias=b))
            yield f"moe_forward_mxfp4_fp8 bf16 unscaled{btag} {which}", forced(which, lambda: ops.moe_forward_mxfp4_fp8(
                Pm, Sm, x8, None, tpe, offs, bias=b, out_dtype=BF16))
            yield f"moe_forward_mxfp4_fp4{btag} {which}", forced(which, lambda: ops.moe_forward_mxfp4_fp4(
                Pm, Sm, *ops.quantize_rows_mxfp4(x), tpe, offs, bias=b))
            yield f"moe_forward_mxfp4_fp4 f16{btag} {which}", forced(which, lambda: ops.moe_forward_mxfp4_fp4(
                Pm, Sm, *ops.quantize_rows_mxfp4(x), tpe, offs, bias=b, out_dtype=F16))
    for dt in (F32, BF16):                   # (one kernel each: nothing to force)
        yield f"quantize_rows_mxfp4 {dt}", lambda: ops.quantize_rows_mxfp4(x.to(dt))
        yield f"quantize_rows_mxfp4 gated {dt}", lambda: ops.quantize_rows_mxfp4(gu.to(dt), **glu)
        for do in (F32, BF16):
            yield f"moe_backward_input_mxfp4 {dt}->{do}", lambda: ops.moe_backward_input_mxfp4(Pm, Sm, gy.to(dt), tpe, offs, out_dtype=do)

    # the MXFP6-row precision, behind the lines above (their order and their random draws are unchanged): the same K = 96,
    # N = 40, decode and tile forced in turn through its own hook
    def forced6(which, call):
        def run():
            from fused_int4_amd import _native
            lib = _native.lib()
            old = lib.fql_tune_set_mx4_f6_decode_max_rows(2 ** 31 - 1 if which == "decode" else 0)
            try:
                return call()
            finally:
                lib.fql_tune_set_mx4_f6_decode_max_rows(old)
        return run

    for which in ("decode", "tile"):
        for btag, b in (("", None), (" bias", biasm)):
            for dt in (F32, BF16):
                tag = f"fp6 {dt}{btag} {which}"
                yield f"moe_forward_mxfp4 {tag}", forced6(which, lambda: ops.moe_forward_mxfp4(
                    Pm, Sm, x.to(dt), tpe, offs, bias=b, precision="fp6"))
                yield f"moe_gated_forward_mxfp4 {tag}", forced6(which, lambda: ops.moe_gated_forward_mxfp4(
                    Pm, Sm, gu.to(dt), tpe, offs, bias=b, precision="fp6", **glu))
                yield f"moe_forward_mxfp4 {tag} ->f16", forced6(which, lambda: ops.moe_forward_mxfp4(
                    Pm, Sm, x.to(dt), tpe, offs, bias=b, out_dtype=F16, precision="fp6"))
            yield f"moe_forward_mxfp4_fp6{btag} {which}", forced6(which, lambda: ops.moe_forward_mxfp4_fp6(
                Pm, Sm, *ops.quantize_rows_mxfp6(x), tpe, offs, bias=b))
            yield f"moe_forward_mxfp4_fp6 f16{btag} {which}", forced6(which, lambda: ops.moe_forward_mxfp4_fp6(
                Pm, Sm, *ops.quantize_rows_mxfp6(x), tpe, offs, bias=b, out_dtype=F16))
    for dt in (F32, BF16):
        yield f"quantize_rows_mxfp6 {dt}", lambda: ops.quantize_rows_mxfp6(x.to(dt))
        yield f"quantize_rows_mxfp6 gated {dt}", lambda: ops.quantize_rows_mxfp6(gu.to(dt), **glu)

    # the dense MXFP4 linear ops, behind the lines above (no new random draw: expert 0's matrix, the first 16 rows): the same
    # K = 96 (one pair and the odd block) and N = 40, each form forced in turn: the tile kernel and the grouped decode
    # kernel through split_k=False, then the split form at 2 and at 16 slices
    def forced_linear(which, call):
        def run():
            from fused_int4_amd import _native
            lib = _native.lib()
            old = (lib.fql_tune_set_mx4_decode_max_rows(0 if which == "tile" else 2 ** 31 - 1),
                   lib.fql_tune_set_mx4_linear_decode_max_rows(2 ** 31 - 1),
                   lib.fql_tune_set_mx4_linear_slices({"split2": 2, "split16": 16}.get(which, 1)))
            try:
                return call()
            finally:
                lib.fql_tune_set_mx4_decode_max_rows(old[0])
                lib.fql_tune_set_mx4_linear_decode_max_rows(old[1])
                lib.fql_tune_set_mx4_linear_slices(old[2])
        return run

    Pl, Sl, bl = Pm[0], Sm[0], biasm[0]
    for which in ("tile", "decode", "split2", "split16"):
        split = which.startswith("split")
        for btag, b in (("", None), (" bias", bl)):
            for dt in (F32, BF16):
                tag = f"{dt}{btag} {which}"
                yield f"linear_forward_mxfp4 {tag}", forced_linear(which, lambda: ops.linear_forward_mxfp4(
                    Pl, Sl, x[:16].to(dt), bias=b, split_k=split))
                yield f"linear_gated_forward_mxfp4 {tag}", forced_linear(which, lambda: ops.linear_gated_forward_mxfp4(
                    Pl, Sl, gu[:16].to(dt), bias=b, split_k=split, **glu))
                yield f"linear_forward_mxfp4 {tag} ->f16", forced_linear(which, lambda: ops.linear_forward_mxfp4(
                    Pl, Sl, x[:16].to(dt), bias=b, out_dtype=F16, split_k=split))
    for dt in (F32, BF16):
        yield f"linear_backward_input_mxfp4 {dt}", lambda: ops.linear_backward_input_mxfp4(Pl, Sl, gy[:16].to(dt))

    # the NVFP4 ops, behind the lines above (their random draws come last): the MXFP4 code bytes under e4m3 scale bytes of
    # every finite magnitude and both signs and one global scale per expert, the same K = 96, N = 40 and table, decode and
    # tile forced in turn through their own hook; the dense ops on expert 0's matrix and the first 16 rows
    Sn = torch.randint(0, 0x7F, (E, N, K // 16), dtype=torch.uint8, generator=d.gen)
    Sn = (Sn | (torch.randint(0, 2, (E, N, K // 16), dtype=torch.uint8, generator=d.gen) << 7)).to(dev)
    Gn = (torch.rand(E, generator=d.gen) + 0.5).to(dev)

    def forced_nv(which, call):
        def run():
            from fused_int4_amd import _native
            lib = _native.lib()
            old = lib.fql_tune_set_nvfp4_decode_max_rows(2 ** 31 - 1 if which == "decode" else 0)
            try:
                return call()
            finally:
                lib.fql_tune_set_nvfp4_decode_max_rows(old)
        return run

    for which in ("decode", "tile"):
        for btag, b in (("", None), (" bias", biasm)):
            for dt in (F32, BF16):
                tag = f"{dt}{btag} {which}"
                yield f"moe_forward_nvfp4 {tag}", forced_nv(which, lambda: ops.moe_forward_nvfp4(Pm, Sn, Gn, x.to(dt), tpe, offs, bias=b))
                yield f"moe_forward_nvfp4 no global {tag}", forced_nv(which, lambda: ops.moe_forward_nvfp4(
                    Pm, Sn, None, x.to(dt), tpe, offs, bias=b))
                yield f"moe_gated_forward_nvfp4 {tag}", forced_nv(which, lambda: ops.moe_gated_forward_nvfp4(
                    Pm, Sn, Gn, gu.to(dt), tpe, offs, bias=b, **glu))
                yield f"moe_forward_nvfp4 {tag} ->f16", forced_nv(which, lambda: ops.moe_forward_nvfp4(
                    Pm, Sn, Gn, x.to(dt), tpe, offs, bias=b, out_dtype=F16))
                bd = None if b is None else b[0]
                yield f"linear_forward_nvfp4 {tag}", forced_nv(which, lambda: ops.linear_forward_nvfp4(
                    Pm[0], Sn[0], Gn[:1], x[:16].to(dt), bias=bd))
                yield f"linear_gated_forward_nvfp4 {tag}", forced_nv(which, lambda: ops.linear_gated_forward_nvfp4(
                    Pm[0], Sn[0], Gn[:1], gu[:16].to(dt), bias=bd, **glu))

    # the NVFP4 input gradient, behind the lines above (no new random draw: the MXFP4 lines' gy on the NVFP4 operands); one
    # kernel, nothing to force; the dense op on expert 0's matrix and the first 16 rows
    for dt in (F32, BF16):
        for do in (F32, BF16):
            yield f"moe_backward_input_nvfp4 {dt}->{do}", lambda: ops.moe_backward_input_nvfp4(
                Pm, Sn, Gn, gy.to(dt), tpe, offs, out_dtype=do)
        yield f"moe_backward_input_nvfp4 no global {dt}", lambda: ops.moe_backward_input_nvfp4(Pm, Sn, None, gy.to(dt), tpe, offs)
        yield f"linear_backward_input_nvfp4 {dt}", lambda: ops.linear_backward_input_nvfp4(Pm[0], Sn[0], Gn[:1], gy[:16].to(dt))

    # the five NVFP4 adapter ops, behind the lines above (their random draws come last): r = 8, v / dv [T, r], B [E, N, r] and
    # A [E, r, K] on the same operands and table; always the tile kernel; the dense ops on expert 0's matrices, the first 16 rows
    Rn = 8
    vn, dvn = d.randn(x.shape[0], Rn).to(dev), d.randn(x.shape[0], Rn).to(dev)
    Bn, An = (d.randn(E, N, Rn) * 0.1).to(dev), (d.randn(E, Rn, K) * 0.1).to(dev)
    for btag, b in (("", None), (" bias", biasm)):
        for dt in (F32, BF16):
            for do in (F32, BF16):
                tag = f"{dt}->{do}{btag}"
                yield f"moe_forward_nvfp4_lora {tag}", lambda: ops.moe_forward_nvfp4_lora(
                    Pm, Sn, Gn, x.to(dt), vn, Bn, tpe, offs, bias=b, out_dtype=do)
                yield f"moe_gated_forward_nvfp4_lora {tag}", lambda: ops.moe_gated_forward_nvfp4_lora(
                    Pm, Sn, Gn, gu.to(dt), vn, Bn, tpe, offs, bias=b, out_dtype=do, **glu)
                yield f"linear_forward_nvfp4_lora {tag}", lambda: ops.linear_forward_nvfp4_lora(
                    Pm[0], Sn[0], Gn[:1], x[:16].to(dt), vn[:16].contiguous(), Bn[0], bias=None if b is None else b[0], out_dtype=do)
    for dt in (F32, BF16):
        for do in (F32, BF16):
            yield f"moe_backward_input_nvfp4_lora {dt}->{do}", lambda: ops.moe_backward_input_nvfp4_lora(
                Pm, Sn, Gn, gy.to(dt), dvn, An, tpe, offs, out_dtype=do)
            yield f"linear_backward_input_nvfp4_lora {dt}->{do}", lambda: ops.linear_backward_input_nvfp4_lora(
                Pm[0], Sn[0], Gn[:1], gy[:16].to(dt), dvn[:16].contiguous(), An[0], out_dtype=do)
        yield f"moe_forward_nvfp4_lora no global {dt}", lambda: ops.moe_forward_nvfp4_lora(Pm, Sn, None, x.to(dt), vn, Bn, tpe, offs)


def digest(t):
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.uint8) if t.numel() else t.new_empty(0, dtype=torch.uint8)
    return f"{str(t.dtype):15s} {str(tuple(t.shape)):16s} {hashlib.sha256(raw.numpy().tobytes()).hexdigest()}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the call names only (needs no GPU)")
    a = ap.parse_args()
    import fused_int4_amd as fq
    from fused_int4_amd import ops
    if a.list:
        dev = torch.device("meta")            # operands are shaped, never computed: the list itself needs no device
        names = []
        try:
            for name, _ in calls(dev, fq, ops):
                names.append(name)
        finally:
            print("\n".join(names))
        return
    dev = torch.device("cuda")
    n = 0
    for name, call in calls(dev, fq, ops):
        out = call()
        for i, t in enumerate(out if isinstance(out, (tuple, list)) else (out,)):
            print(f"{name} [{i}]  " + ("None" if t is None else digest(t)))
        n += 1
    torch.cuda.synchronize()
    print(f"# {n} calls")


if __name__ == "__main__":
    main()
