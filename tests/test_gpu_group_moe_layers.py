"""``group_size`` in the gated INT4 FFN layers on the GPU: QuantizedMoEFFN(E = 3, H = 256, F = 256, group_size = 64),
LoRAQuantizedMoEFFN (rank 8) and QuantizedSparseMoEBlock(E = 4, top_k = 2, shared_ffn_dim = 256, group_size = 64) on 24
tokens, in float32 and with ``activation_dtype=torch.bfloat16``, against a float64 torch model built from the dequantised
weights (helpers.dequant_f64 per group): the output, ``inputs.grad``, the bias gradients, the four adapter gradients and
``gate.weight.grad``.

Bounds.  float32 layers: those of the per-row twins, tests/test_gpu_glu_layers.py and test_gpu_expert_bias_layers.py:
tol(fro_tol(3, F)) for the output, FFN_REL_FRO = 2e-5 for every gradient.  ``gate.weight.grad`` passes through the softmax
Jacobian, whose cancellation the twins of the block measure with a float32 torch router and allow four times over
(tests/test_gpu_sparse_moe_block.py): the bound here is the larger of that and the gradients' own bound, the low-precision
model being this file's float64 model evaluated in the layer's type (float32 or bfloat16).  bfloat16 layers: the twins
compare bits with the chain of public ops, which is done here too; against float64 a tensor that passed through n roundings to bfloat16 (8 significant bits, relative error at
most 2^-9 each, amplified by at most |act'| <= 1.1 on the way) is held to n * 2^-8 in the Frobenius norm: y 2 (gate_up, y),
dx 4 (gate_up, dh, dgu, dx), the gate|up bias and adapter gradients 3, the down adapter gradients 1 (h from the rounded
gate_up), the down bias 0 (a float32 sum of the gradient as it came: FFN_REL_FRO); the block's output one more (the combine).
Every test fails on a library without the feature (``group_size`` is a TypeError there), but the last, which holds
``group_size=None`` to the block built today's way."""
import functools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import hidden_autograd
from helpers import clipped_ranges, dequant_f64, expert_table, fq, fro_tol, ops, rel_fro_dev, same_bits, tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H, F, GROUP, RANK = 3, 256, 256, 64, 8
FFN_REL_FRO = 2e-5             # tests/test_gpu_ffn_lora.py: the bound of the two-GEMM QuantizedMoEFFN backward
BF16 = 2.0 ** -8
ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
BIASES = ("gate_up_bias", "down_bias")
ROUNDINGS = {"y": 2, "dx": 4, "dgate_up_bias": 3, "ddown_bias": 0, "dgate_up_lora_A": 3, "dgate_up_lora_B": 3,
             "ddown_lora_A": 1, "ddown_lora_B": 1}


@functools.lru_cache(maxsize=None)
def raw(n_experts, ffn, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, scale=0.1: torch.randn(*s, generator=g) * scale
    return ([mk(ffn, H) for _ in range(n_experts)], [mk(ffn, H) for _ in range(n_experts)],
            [mk(H, ffn) for _ in range(n_experts)], [mk(ffn, scale=0.5) for _ in range(n_experts)],
            [mk(ffn, scale=0.5) for _ in range(n_experts)], [mk(H, scale=0.5) for _ in range(n_experts)])


def ffn_layer(dtype, lora, n_experts=E, ffn=F, seed=5, group_size=GROUP, kind="silu"):
    gate, up, down, gb, ub, db = raw(n_experts, ffn, seed)
    m = fq().QuantizedMoEFFN.from_weights(gate, up, down, activation_dtype=dtype, gate_bias=gb, up_bias=ub, down_bias=db,
                                          group_size=group_size, activation=kind).to(DEV)
    if group_size is not None:
        assert tuple(m.gate_up_scales.shape) == (n_experts, 2 * ffn, H // group_size)
        assert tuple(m.down_zero_points.shape) == (n_experts, H, ffn // group_size)
    if lora:
        m = fq().LoRAQuantizedMoEFFN.from_quantized(m, RANK, alpha=2 * RANK)
        assert m.group_size == group_size
        g = torch.Generator(device=DEV).manual_seed(17)
        with torch.no_grad():
            m.gate_up_lora_B.normal_(0, 0.1, generator=g)
            m.down_lora_B.normal_(0, 0.1, generator=g)
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def leaves(m, ft):
    """The layer's parameters as ``ft`` leaves on the device, and its dequantised weights."""
    p = {n: getattr(m, n).detach().to(ft).requires_grad_() for n in BIASES + ADAPTERS if hasattr(m, n)}
    n_e = m.num_experts
    Wgu = [dequant_f64(m.gate_up_packed[e], m.gate_up_scales[e], m.gate_up_zero_points[e]).to(ft) for e in range(n_e)]
    Wd = [dequant_f64(m.down_packed[e], m.down_scales[e], m.down_zero_points[e]).to(ft) for e in range(n_e)]
    return p, Wgu, Wd


def ffn_model(m, p, Wgu, Wd, e, xe):
    """Expert e of the layer on rows xe, in the leaves' type."""
    s = getattr(m, "scaling", 0.0)
    Fm = m.ffn_dim
    gu = xe @ Wgu[e].t()
    if "gate_up_bias" in p:
        gu = gu + p["gate_up_bias"][e]
    if "gate_up_lora_A" in p:
        gu = gu + s * (xe @ p["gate_up_lora_A"][e].t()) @ p["gate_up_lora_B"][e].t()
    h = hidden_autograd(m.activation, gu[:, :Fm], gu[:, Fm:], m.activation_alpha, m.activation_limit)
    y = h @ Wd[e].t()
    if "down_bias" in p:
        y = y + p["down_bias"][e]
    if "down_lora_A" in p:
        y = y + s * (h @ p["down_lora_A"][e].t()) @ p["down_lora_B"][e].t()
    return y


def ffn_reference(m, x, tpe, offs, gy, ft=torch.float64):
    p, Wgu, Wd = leaves(m, ft)
    xl = x.detach().to(ft).requires_grad_()
    T = x.shape[0]
    y = torch.zeros(T, m.hidden_dim, dtype=ft, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi > lo:
            y = y.index_put((torch.arange(lo, hi, device=DEV),), ffn_model(m, p, Wgu, Wd, e, xl[lo:hi]))
    y.backward(gy.to(ft))
    out = {"y": y.detach(), "dx": xl.grad}
    out.update({"d" + n: t.grad for n, t in p.items()})
    return out


def run(m, x, tpe, offs, gy):
    for p in m.parameters():
        p.grad = None
    xg = x.detach().clone().requires_grad_(True)
    y = m(xg, tpe, offs)
    y.backward(gy)
    out = {"y": y.detach(), "dx": xg.grad}
    out.update({"d" + n: p.grad for n, p in m.named_parameters()})
    return out


def ffn_problem(dtype):
    tpe, offs, T = expert_table([13, 0, 9], gaps=[0, 0, 1], tail=1)            # 24 rows: the integer path (8 per expert)
    g = torch.Generator(device=DEV).manual_seed(3)
    dt = dtype or torch.float32
    return tpe, offs, T, torch.randn(T, H, device=DEV, generator=g).to(dt), torch.randn(T, H, device=DEV, generator=g).to(dt)


def check(got, ref, dtype, what, extra=0):
    assert set(ref) <= set(got), (sorted(ref), sorted(got))
    for n in ref:
        err = rel_fro_dev(got[n], ref[n])
        if dtype is None:
            bound = tol(fro_tol(3, F)) if n == "y" else FFN_REL_FRO
        else:
            bound = (ROUNDINGS[n] + (extra if n in ("y", "dx") else 0)) * BF16 or FFN_REL_FRO
        print(f"ERR group layer {what} {n}: {err:.3e} (bound {bound:.2e})")
        assert got[n].dtype == (torch.float32 if n not in ("y", "dx") or dtype is None else dtype), n
        assert err < bound, (what, n, err, bound)


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_ffn_layer_against_float64(dtype, lora):
    m = ffn_layer(dtype, lora)
    tpe, offs, T, x, gy = ffn_problem(dtype)
    got = run(m, x, tpe, offs, gy)
    ref = ffn_reference(m, x, tpe, offs, gy)
    assert set(ref) == {"y", "dx"} | {"d" + n for n in BIASES + (ADAPTERS if lora else ())}
    check(got, ref, dtype, f"ffn {'lora' if lora else 'plain'} {dtype}")
    assert torch.count_nonzero(got["y"][-1]) == 0 and torch.count_nonzero(got["dx"][-1]) == 0      # the uncovered rows
    assert torch.count_nonzero(got["y"][13]) == 0 and torch.count_nonzero(got["dgate_up_bias"][1]) == 0
    again = run(m, x, tpe, offs, gy)
    for n in got:
        assert same_bits(again[n], got[n]), n
    with torch.no_grad():
        assert same_bits(m(x, tpe, offs), got["y"])


@pytest.mark.parametrize("kind", ["silu", "swiglu_clamp"])
def test_bf16_ffn_layer_is_the_chain_of_public_ops(kind):
    dt = torch.bfloat16
    m = ffn_layer(dt, False, kind=kind)
    tpe, offs, T, x, gy = ffn_problem(dt)
    got = run(m, x, tpe, offs, gy)
    o, act = ops(), dict(zip(("activation", "activation_alpha", "activation_limit"), m.activation_args))
    gu_w = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points)
    d_w = (m.down_packed, m.down_scales, m.down_zero_points)
    b_gu, b_d = m.gate_up_bias.detach(), m.down_bias.detach()
    gate_up = o.moe_forward_any(*gu_w, x, None, tpe, offs, out_dtype=dt, bias=b_gu)
    y = o.moe_gated_forward(*d_w, gate_up, tpe, offs, out_dtype=dt, bias=b_d, **act)
    dh = o.moe_backward_input(*d_w, gy, tpe, offs, out_dtype=dt)
    dgu = o.glu_backward(gate_up, dh, out_dtype=dt, **act)
    dx = o.moe_backward_input(*gu_w, dgu, tpe, offs, out_dtype=dt)
    assert same_bits(got["y"], y) and same_bits(got["dx"], dx)
    assert same_bits(got["dgate_up_bias"], o.moe_bias_grad(dgu, E, tpe, offs))
    assert same_bits(got["ddown_bias"], o.moe_bias_grad(gy, E, tpe, offs))


# ---- the sparse block

BE, TOP_K, TOKENS, SHARED_F = 4, 2, 24, 256


def block(dtype, group_size=GROUP, **kw):
    gate, up, down, gb, ub, db = raw(BE, F, 7)
    sg, su, sd, _, _, _ = raw(1, SHARED_F, 9)
    torch.manual_seed(11)
    m = fq().QuantizedSparseMoEBlock.from_weights(torch.randn(BE, H) * 0.2, gate, up, down, top_k=TOP_K, activation_dtype=dtype,
                                                  shared=(sg[0], su[0], sd[0]), gate_bias=gb, up_bias=ub, down_bias=db,
                                                  group_size=group_size, **kw).to(DEV)
    if group_size is not None:
        assert m.experts.group_size == group_size and m.shared_experts.group_size == group_size
        assert tuple(m.shared_experts.gate_up_scales.shape) == (1, 2 * SHARED_F, H // group_size)
    m.experts.gate_up_bias.requires_grad_(True)
    m.experts.down_bias.requires_grad_(True)
    return m


def block_problem(dtype, masked):
    g = torch.Generator(device=DEV).manual_seed(21)
    dt = dtype or torch.float32
    x = torch.randn(TOKENS, H, device=DEV, generator=g).to(dt)
    gy = torch.randn(TOKENS, H, device=DEV, generator=g).to(dt)
    mask = None
    if masked:
        mask = torch.ones(TOKENS, dtype=torch.bool, device=DEV)
        mask[[2, 11, 23]] = False
    return x, gy, mask


def block_reference(m, x, gy, mask, indices, keep, ft):
    """The dense torch model in ``ft``: a softmax router on the device's own selection (``indices``) and drops (``keep``),
    every kept (token, slot) pair through its expert, the shared expert on every token."""
    T = x.shape[0]
    xl = x.detach().to(ft).requires_grad_()
    wg = m.gate.weight.detach().to(ft).requires_grad_()
    p, Wgu, Wd = leaves(m.experts, ft)
    ps, Wgus, Wds = leaves(m.shared_experts, ft)
    probs = torch.softmax(xl @ wg.t(), dim=-1)
    sel = probs.gather(1, indices.long())
    w = sel / sel.sum(dim=-1, keepdim=True)
    out = ffn_model(m.shared_experts, ps, Wgus, Wds, 0, xl)
    for e in range(m.num_experts):
        ye = ffn_model(m.experts, p, Wgu, Wd, e, xl)
        we = (w * ((indices == e) & keep).to(ft)).sum(dim=1, keepdim=True)
        out = out + we * ye
    out.backward(gy.to(ft))
    res = {"y": out.detach(), "dx": xl.grad, "dgate.weight": wg.grad}
    res.update({"dexperts." + n: p[n].grad for n in BIASES})
    return res


@pytest.mark.parametrize("capped", [False, True], ids=["plain", "capacity-mask"])
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_block_against_float64(dtype, capped):
    m = block(dtype, capacity_factor=0.75 if capped else None)
    x, gy, mask = block_problem(dtype, capped)
    for p in m.parameters():
        p.grad = None
    xg = x.detach().clone().requires_grad_(True)
    out, logits = m(xg, token_mask=mask) if capped else m(xg)
    out.backward(gy)
    indices = m.routing[2]
    if capped:
        pos = ops().route_plan_capped(indices, BE, m.expert_capacity(TOKENS), mask)[3]
        keep = (pos >= 0).view(TOKENS, TOP_K)
        assert 0 < int((~keep).sum()) < keep.numel() and bool(keep[mask].any()) and not bool(keep[~mask].any())
    else:
        keep = torch.ones(TOKENS, TOP_K, dtype=torch.bool, device=DEV)
    got = {"y": out.detach(), "dx": xg.grad, "dgate.weight": m.gate.weight.grad,
           "dexperts.gate_up_bias": m.experts.gate_up_bias.grad, "dexperts.down_bias": m.experts.down_bias.grad}
    ref = block_reference(m, x, gy, mask, indices, keep, torch.float64)
    low = block_reference(m, x, gy, mask, indices, keep, dtype or torch.float32)      # the same model in the layer's type
    what = f"block {dtype} {'capped' if capped else 'plain'}"
    for n in ref:
        err, e_low = rel_fro_dev(got[n], ref[n]), rel_fro_dev(low[n], ref[n])
        if dtype is None:
            bound = tol(fro_tol(3, F)) if n == "y" else FFN_REL_FRO
        else:                                   # y: gate_up, y, the combine; dx and the rest: the roundings of the FFN's dx
            bound = {"y": 3, "dx": 5}.get(n, 4) * BF16
        if n == "dgate.weight":                 # the softmax Jacobian cancels: four times what it does to the torch model
            bound = max(bound, 4 * e_low)
        print(f"ERR group {what} {n}: {err:.3e} (torch model in the layer's type {e_low:.3e}, bound {bound:.2e})")
        assert err < bound, (what, n, err, bound)
    assert float(torch.linalg.vector_norm(ref["dgate.weight"])) > 0


def test_group_size_none_is_the_block_of_today():
    x, gy, _ = block_problem(None, False)
    outs = []
    for kw in ({"group_size": None}, {}):
        gate, up, down, gb, ub, db = raw(BE, F, 7)
        torch.manual_seed(11)
        m = fq().QuantizedSparseMoEBlock.from_weights(torch.randn(BE, H) * 0.2, gate, up, down, top_k=TOP_K,
                                                      gate_bias=gb, up_bias=ub, down_bias=db, **kw).to(DEV)
        assert m.experts.group_size is None and m.experts.gate_up_scales.dim() == 2
        with torch.no_grad():
            outs.append(m(x)[0])
    assert same_bits(outs[0], outs[1])
    # ... and a group that spans the whole row is that layer too: one group per row in both projections
    gate, up, down, _, _, _ = raw(BE, H, 13)                      # F == H == 256
    a = fq().QuantizedMoEFFN.from_weights(gate, up, down, group_size=H).to(DEV)
    b = fq().QuantizedMoEFFN.from_weights(gate, up, down).to(DEV)
    tpe, offs, T = expert_table([6, 6, 6, 6])
    assert a.group_size is None
    with torch.no_grad():
        assert same_bits(a(x, tpe, offs), b(x, tpe, offs))
