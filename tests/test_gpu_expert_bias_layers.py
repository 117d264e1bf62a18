"""The layers with per-expert biases on the GPU: QuantizedMoEFFN(expert_bias=True), LoRAQuantizedMoEFFN on top of it and
QuantizedSparseMoEBlock(expert_bias=True, router_bias=True).  E = 4, H = 64, F = 96, T = 37 (one empty expert, a gap and an
uncovered last row), random non-zero biases.

  * float32 layers, every activation kind: y, dx, the adapter gradients and both bias gradients against the float64 chain
    gate_up = W_gu x + b_gu (+ s B_gu A_gu x), y = W_d h(gate_up) + b_d (+ s B_d A_d h) on the dequantised weights, at the
    bound the project holds the unbiased layers to (FFN_REL_FRO of tests/test_gpu_ffn_lora.py, relative Frobenius).
    Measured values: DESIGN.md section 22.
  * 16-bit layers: bit for bit the documented chain of public ops, the bias gradients ops.moe_bias_grad of the layer's own
    dgu and gy.
  * a frozen bias gets no gradient and launches no reduction; the sparse block against its chain router -> plan ->
    dispatch -> experts -> combine_any, bit for bit, every gradient included."""
import functools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import ALPHA, LIMIT, hidden_autograd
from helpers import clipped_ranges, expert_table, fq, ops, rel_fro_dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H, F, RANK = 4, 64, 96, 8
COUNTS, GAPS, TAIL = [9, 0, 17, 8], [0, 0, 2, 0], 1                    # T = 37
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
FFN_REL_FRO = 2e-5             # tests/test_gpu_ffn_lora.py: the bound of the two-GEMM QuantizedMoEFFN backward
ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
BIASES = ("gate_up_bias", "down_bias")


def act_of(kind):
    return dict(activation=kind, activation_alpha=ALPHA, activation_limit=LIMIT)


@functools.lru_cache(maxsize=None)
def raw():
    torch.manual_seed(5)
    gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
    up = [torch.randn(F, H) * 0.1 for _ in range(E)]
    down = [torch.randn(H, F) * 0.1 for _ in range(E)]
    gb = [torch.randn(F) * 0.5 for _ in range(E)]
    ub = [torch.randn(F) * 0.5 for _ in range(E)]
    db = [torch.randn(H) * 0.5 for _ in range(E)]
    return gate, up, down, gb, ub, db


@functools.lru_cache(maxsize=None)
def base_layer(kind, dtype, biased=True):
    gate, up, down, gb, ub, db = raw()
    kw = dict(gate_bias=gb, up_bias=ub, down_bias=db) if biased else {}
    m = fq().QuantizedMoEFFN.from_weights(gate, up, down, activation_dtype=dtype, **act_of(kind), **kw).to(DEV)
    if biased:
        assert float(m.gate_up_bias.abs().min()) > 0 and float(m.down_bias.abs().min()) > 0
    return m


def lora_layer(kind, dtype):
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base_layer(kind, dtype), RANK, alpha=2 * RANK)
    g = torch.Generator(device=DEV).manual_seed(17)
    with torch.no_grad():
        m.gate_up_lora_B.normal_(0, 0.1, generator=g)
        m.down_lora_B.normal_(0, 0.1, generator=g)
    return m


def problem(dtype, seed=3):
    tpe, offs, T = expert_table(COUNTS, gaps=GAPS, tail=TAIL)
    assert T == 37
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, H, device=DEV, generator=g).to(dtype)
    gy = torch.randn(T, H, device=DEV, generator=g).to(dtype)
    return tpe, offs, T, x, gy


def w64(packed, scales, zps):
    return fq().dequantize_weights(packed.cpu(), scales.cpu(), zps.cpu()).double()


def ref64(m, kind, x, tpe, offs, gy, lora):
    """float64 forward and gradients (autograd on the CPU) on the dequantised weights.  Returns a dict."""
    s = m.scaling if lora else 0.0
    Wgu = [w64(m.gate_up_packed[e], m.gate_up_scales[e], m.gate_up_zero_points[e]) for e in range(E)]
    Wd = [w64(m.down_packed[e], m.down_scales[e], m.down_zero_points[e]) for e in range(E)]
    leaf = lambda t: t.detach().cpu().double().requires_grad_()
    p = {"x": leaf(x), "gate_up_bias": leaf(m.gate_up_bias), "down_bias": leaf(m.down_bias)}
    if lora:
        p.update({n: leaf(getattr(m, n)) for n in ADAPTERS})
    T = x.shape[0]
    y = torch.zeros(T, H, dtype=torch.float64)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            continue
        xe = p["x"][lo:hi]
        gu = xe @ Wgu[e].t() + p["gate_up_bias"][e]
        if lora:
            gu = gu + s * (xe @ p["gate_up_lora_A"][e].t()) @ p["gate_up_lora_B"][e].t()
        h = hidden_autograd(kind, gu[:, :F], gu[:, F:], ALPHA, LIMIT)
        ye = h @ Wd[e].t() + p["down_bias"][e]
        if lora:
            ye = ye + s * (h @ p["down_lora_A"][e].t()) @ p["down_lora_B"][e].t()
        y = y.index_put((torch.arange(lo, hi),), ye)
    y.backward(gy.cpu().double())
    out = {"y": y.detach(), "dx": p["x"].grad}
    out.update({"d" + n: t.grad for n, t in p.items() if n != "x"})
    return out


def train(m, names):
    """Exactly the parameters in ``names`` require grad; grads cleared.  Returns a function that restores the states."""
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = None
        p.requires_grad_(n in names)

    def restore():
        for n, p in m.named_parameters():
            p.requires_grad_(before[n])
            p.grad = None
    return restore


def run(m, x, tpe, offs, gy, names, x_grad=True):
    restore = train(m, names)
    try:
        xg = x.detach().clone().requires_grad_(x_grad)
        y = m(xg, tpe, offs)
        y.backward(gy)
        out = {"y": y.detach(), "dx": xg.grad}
        out.update({"d" + n: p.grad for n, p in m.named_parameters()})
        return out
    finally:
        restore()


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("kind", KINDS)
def test_float32_layers_against_float64(kind, lora):
    m = lora_layer(kind, None) if lora else base_layer(kind, None)
    tpe, offs, T, x, gy = problem(torch.float32)
    names = BIASES + (ADAPTERS if lora else ())
    got = run(m, x, tpe, offs, gy, names)
    ref = ref64(m, kind, x, tpe, offs, gy, lora)
    errs = {n: rel_fro_dev(got[n], ref[n]) for n in ref}
    print(f"ERR expert_bias {kind} {'lora' if lora else 'plain'} " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e < FFN_REL_FRO, (n, e)
    assert torch.count_nonzero(got["y"][-1]) == 0                       # the uncovered last row: the bias is an expert's
    assert torch.count_nonzero(got["dgate_up_bias"][1]) == 0 and torch.count_nonzero(got["ddown_bias"][1]) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_bias_is_not_dropped(kind):
    tpe, offs, T, x, _ = problem(torch.float32)
    with torch.no_grad():
        yb = base_layer(kind, None)(x, tpe, offs)
        y0 = base_layer(kind, None, biased=False)(x, tpe, offs)
    covered = torch.ones(T, dtype=torch.bool, device=DEV)
    covered[-1] = False
    covered[9:11] = False
    assert float((yb - y0)[covered].abs().max(dim=1).values.min()) > 1e-2      # every covered row moved
    assert torch.count_nonzero(yb[~covered]) == 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_16bit_layer_is_the_chain_of_public_ops(kind, dtype):
    m = base_layer(kind, dtype)
    tpe, offs, T, x, gy = problem(dtype)
    got = run(m, x, tpe, offs, gy, BIASES)
    o, act = ops(), act_of(kind)
    b_gu, b_d = m.gate_up_bias.detach(), m.down_bias.detach()
    gate_up = o.moe_forward_any(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, x, None, tpe, offs,
                                out_dtype=dtype, bias=b_gu)
    y = o.moe_gated_forward(m.down_packed, m.down_scales, m.down_zero_points, gate_up, tpe, offs, out_dtype=dtype, bias=b_d,
                            **act)
    dh = o.moe_backward_input(m.down_packed, m.down_scales, m.down_zero_points, gy, tpe, offs, out_dtype=dtype)
    dgu = o.glu_backward(gate_up, dh, out_dtype=dtype, **act)
    dx = o.moe_backward_input(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, dgu, tpe, offs, out_dtype=dtype)
    assert same_bits(got["y"], y)
    assert same_bits(got["dx"], dx)
    assert same_bits(got["dgate_up_bias"], o.moe_bias_grad(dgu, E, tpe, offs))
    assert same_bits(got["ddown_bias"], o.moe_bias_grad(gy, E, tpe, offs))
    # one rounding, after the bias: gate_up is the float32 result plus the bias, rounded once
    gu32 = o.moe_forward_any(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, x, None, tpe, offs,
                             out_dtype=torch.float32)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        assert same_bits(gate_up[lo:hi], (gu32[lo:hi] + b_gu[e]).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_16bit_lora_layer_is_the_chain_of_public_ops(kind, dtype):
    m = lora_layer(kind, dtype)
    tpe, offs, T, x, gy = problem(dtype)
    got = run(m, x, tpe, offs, gy, BIASES + ADAPTERS)
    o, act, s = ops(), act_of(kind), m.scaling
    b_gu, b_d = m.gate_up_bias.detach(), m.down_bias.detach()
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach() for n in ADAPTERS)
    gup, dn = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points), (m.down_packed, m.down_scales, m.down_zero_points)
    gu32 = o.moe_forward_any(*gup, x, None, tpe, offs, out_dtype=torch.float32, bias=b_gu)     # the bias: the base GEMM's
    u_gu = o.lora_shrink(x, A_gu, "rc", tpe, offs)
    gate_up = o.lora_expand(u_gu, B_gu, "cr", tpe, offs, scale=s, input=gu32, out_dtype=dtype)  # the adapter term after it
    y32 = o.moe_gated_forward(*dn, gate_up, tpe, offs, out_dtype=torch.float32, bias=b_d, **act)
    u_d = o.lora_gated_shrink(gate_up, A_d, "rc", tpe, offs, **act)
    y = o.lora_expand(u_d, B_d, "cr", tpe, offs, scale=s, input=y32, out_dtype=dtype)
    du_d = o.lora_shrink(gy, B_d, "cr", tpe, offs, scale=s)
    dh = o.lora_expand(du_d, A_d, "rc", tpe, offs, input=o.moe_backward_input(*dn, gy, tpe, offs), out_dtype=dtype)
    dgu = o.glu_backward(gate_up, dh, out_dtype=dtype, **act)
    du_gu = o.lora_shrink(dgu, B_gu, "cr", tpe, offs, scale=s)
    dx = o.lora_expand(du_gu, A_gu, "rc", tpe, offs, input=o.moe_backward_input(*gup, dgu, tpe, offs), out_dtype=dtype)
    assert same_bits(got["y"], y)
    assert same_bits(got["dx"], dx)
    assert same_bits(got["dgate_up_bias"], o.moe_bias_grad(dgu, E, tpe, offs))
    assert same_bits(got["ddown_bias"], o.moe_bias_grad(gy, E, tpe, offs))
    assert same_bits(got["dgate_up_lora_B"], o.lora_grad(dgu, u_gu, "cr", E, tpe, offs, scale=s))
    assert same_bits(got["ddown_lora_B"], o.lora_grad(gy, u_d, "cr", E, tpe, offs, scale=s))


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_a_frozen_bias_gets_no_gradient_and_no_reduction(dtype, lora, monkeypatch):
    kind = "swiglu_clamp"
    m = lora_layer(kind, dtype) if lora else base_layer(kind, dtype)
    tpe, offs, T, x, gy = problem(dtype or torch.float32)
    calls = []
    real = ops().moe_bias_grad
    monkeypatch.setattr(ops(), "moe_bias_grad", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    full = run(m, x, tpe, offs, gy, BIASES + (ADAPTERS if lora else ()))
    assert len(calls) == 2 and full["dgate_up_bias"] is not None and full["ddown_bias"] is not None
    # frozen (the state a loaded checkpoint is in): no gradient, no launch
    del calls[:]
    frozen = run(m, x, tpe, offs, gy, ADAPTERS if lora else ())
    assert frozen["dgate_up_bias"] is None and frozen["ddown_bias"] is None and calls == []
    assert same_bits(frozen["y"], full["y"]) and same_bits(frozen["dx"], full["dx"])
    # one of the two: one launch, of that one's rows
    del calls[:]
    one = run(m, x, tpe, offs, gy, ("down_bias",) + (ADAPTERS if lora else ()))
    assert one["dgate_up_bias"] is None and same_bits(one["ddown_bias"], full["ddown_bias"])
    assert calls == [torch.Size([T, H])]
    del calls[:]
    other = run(m, x, tpe, offs, gy, ("gate_up_bias",), x_grad=False)    # a bias alone can train
    assert other["dx"] is None and other["ddown_bias"] is None
    assert same_bits(other["dgate_up_bias"], full["dgate_up_bias"]) and calls == [torch.Size([T, 2 * F])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sparse_block_with_expert_and_router_bias(dtype):
    gate, up, down, gb, ub, db = raw()
    torch.manual_seed(23)
    gw, rb = torch.randn(E, H) * 0.5, torch.randn(E)
    adt = None if dtype == torch.float32 else dtype
    m = fq().QuantizedSparseMoEBlock.from_weights(gw, gate, up, down, top_k=2, activation_dtype=adt, router_bias=rb,
                                                  gate_bias=gb, up_bias=ub, down_bias=db, **act_of("swiglu_clamp")).to(DEV)
    m.experts.gate_up_bias.requires_grad_(True)
    m.experts.down_bias.requires_grad_(True)
    params = {"gate.weight": m.gate.weight, "gate.bias": m.gate.bias, "gate_up_bias": m.experts.gate_up_bias,
              "down_bias": m.experts.down_bias}
    g = torch.Generator(device=DEV).manual_seed(29)
    x = torch.randn(3, 7, H, device=DEV, generator=g).to(dtype)
    gout = torch.randn(3, 7, H, device=DEV, generator=g).to(dtype)

    def grads(fn):
        for p in params.values():
            p.grad = None
        xg = x.detach().clone().requires_grad_()
        out, logits = fn(xg)
        out.backward(gout)
        return out.detach(), logits.detach(), xg.grad, {n: p.grad.clone() for n, p in params.items()}

    def chain(xg):
        o = ops()
        x2 = xg.reshape(-1, H)
        w, b = m.gate.weight, m.gate.bias
        logits = torch.nn.functional.linear(x2, w.to(x2.dtype), b.to(x2.dtype))       # router.bias: part of the logits
        weights, indices, _ = o.router_score_topk(logits, 2, "softmax", None, 1, 1, 2, True, 1.0, return_scores=True)
        tpe, offs, token_of_sorted, pos_of_slot = o.route_plan(indices, E)
        rows = o.dispatch_rows(x2, token_of_sorted, pos_of_slot, 2)
        y = m.experts(rows, tpe, offs)                                  # (bias inside: the routing weight comes after it)
        return o.combine_any(y, pos_of_slot, weights, out_dtype=xg.dtype).reshape(xg.shape), logits

    out, logits, dx, dp = grads(m)
    out_c, logits_c, dx_c, dp_c = grads(chain)
    assert same_bits(out, out_c) and same_bits(logits, logits_c) and same_bits(dx, dx_c)
    for n in params:
        assert same_bits(dp[n], dp_c[n]), n
        assert float(dp[n].abs().max()) > 0, n
    # the router bias moves the logits, the expert biases the output
    with torch.no_grad():
        plain = fq().QuantizedSparseMoEBlock.from_weights(gw, gate, up, down, top_k=2, activation_dtype=adt,
                                                          **act_of("swiglu_clamp")).to(DEV)
        out_p, logits_p = plain(x)
    assert float((logits.float() - logits_p.float()).abs().max()) > 0.1
    assert float((out.float() - out_p.float()).abs().max()) > 1e-2
