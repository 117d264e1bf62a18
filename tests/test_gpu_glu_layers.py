"""GeGLU (tanh form) and clamped-SwiGLU activations in the gated INT4 FFN layers on the GPU: QuantizedMoEFFN,
LoRAQuantizedMoEFFN and QuantizedSparseMoEBlock built with ``activation=``.

  6. the float32 layers against a float64 chain on the dequantised weights; the 16-bit layers bit for bit against the
     documented chain of public ops; run-to-run identical gradients; nothing of shape [T, F] saved;
  7. the sparse block (with a shared expert of the same kind) is router -> plan -> dispatch -> experts -> combine_any, bit
     for bit, forward and gradients;
  8. ``activation="silu"`` given explicitly is the layer without it, gradients included.

The kernels alone are in tests/test_gpu_glu.py.  Errors measured on an MI355X are listed in DESIGN.md section 21."""
import itertools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import KINDS, LIMIT, act_kw, clamped_share, hidden_autograd
from helpers import clipped_ranges, dequant_f64, expert_table, fq, fro_tol, ops, rel_fro_dev, same_bits, tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
FFN_REL_FRO = 2e-5             # the bound tests/test_gpu_ffn_lora.py holds dx and the adapter gradients to
ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
NAMES = ("y", "dx", "dA_gu", "dB_gu", "dA_d", "dB_d")
SEEDS = [11, 12, 13, 14, 15, 16, 17, 18]


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


_BASES = {}


def base_layer(E, H, F, kind, dtype=None, seed=5):
    """A QuantizedMoEFFN of ``kind`` over buffers quantised once per shape (the activation is configuration)."""
    key = (E, H, F, seed)
    if key not in _BASES:
        torch.manual_seed(seed)
        gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
        up = [torch.randn(F, H) * 0.1 for _ in range(E)]
        down = [torch.randn(H, F) * 0.1 for _ in range(E)]
        _BASES[key] = fq().QuantizedMoEFFN.from_weights(gate, up, down).to(DEV)
    m = fq().QuantizedMoEFFN(E, H, F, activation_dtype=dtype, **act_kw(kind))
    for name, buf in _BASES[key].named_buffers():
        setattr(m, name, buf)
    return m


def lora_layer(E, H, F, kind, r, dtype=None, seed=5):
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base_layer(E, H, F, kind, dtype, seed), r, alpha=2 * r)
    assert m.activation == kind and m.activation_dtype == dtype
    g = gen(seed + r)
    with torch.no_grad():
        m.gate_up_lora_B.normal_(0, 0.1, generator=g)
        m.down_lora_B.normal_(0, 0.1, generator=g)
    return m


def run(m, x, tpe, offs, gy):
    """Forward + backward; (y, dx, dA_gu, dB_gu, dA_d, dB_d), the adapter entries None for a layer without adapters."""
    for name in ADAPTERS:
        if getattr(m, name, None) is not None:
            getattr(m, name).grad = None
    xg = x.detach().clone().requires_grad_(True)
    y = m(xg, tpe, offs)
    y.backward(gy)
    return (y.detach(), xg.grad) + tuple(getattr(getattr(m, name, None), "grad", None) for name in ADAPTERS)


def reference64(m, x, tpe, offs, gy):
    """The float64 chain on the dequantised weights (autograd on the device): (y, dx, dA_gu, dB_gu, dA_d, dB_d, gate_up)."""
    E, F, T = m.num_experts, m.ffn_dim, x.shape[0]
    s = getattr(m, "scaling", 0.0)
    Wgu = [dequant_f64(m.gate_up_packed[e], m.gate_up_scales[e], m.gate_up_zero_points[e]) for e in range(E)]
    Wd = [dequant_f64(m.down_packed[e], m.down_scales[e], m.down_zero_points[e]) for e in range(E)]
    x64 = x.detach().double().requires_grad_()
    ad = [getattr(m, n).detach().double().requires_grad_() if hasattr(m, n) else None for n in ADAPTERS]
    Agu, Bgu, Ad, Bd = ad
    y = torch.zeros(T, m.hidden_dim, dtype=torch.float64, device=DEV)
    gate_up = torch.zeros(T, 2 * F, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            continue
        xe = x64[lo:hi]
        gu = xe @ Wgu[e].t()
        if Agu is not None:
            gu = gu + s * (xe @ Agu[e].t()) @ Bgu[e].t()
        h = hidden_autograd(m.activation, gu[:, :F], gu[:, F:], m.activation_alpha, m.activation_limit)
        ye = h @ Wd[e].t()
        if Ad is not None:
            ye = ye + s * (h @ Ad[e].t()) @ Bd[e].t()
        y = y.index_put((torch.arange(lo, hi, device=DEV),), ye)
        gate_up[lo:hi] = gu.detach()
    y.backward(gy.double())
    grads = tuple(None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad) for t in ad)
    return (y.detach(), x64.grad) + grads + (gate_up,)


def float32_problem(m, tpe, offs, T):
    """x, gy and the float64 reference.  Clamped kind: x is scaled so that the reference gate_up has a standard deviation
    near 4 (1 % - 50 % of g and of u clamped), and the first of eight fixed seeds is taken for which no reference g or u lies
    within 1e-5 * limit of a clamp boundary -- a float32 GEMM error of 2e-6 could otherwise flip a mask and move one element
    by O(1)."""
    cov = torch.zeros(T, dtype=torch.bool, device=DEV)
    for lo, hi in clipped_ranges(tpe.cpu(), offs.cpu(), T):
        cov[lo:hi] = True
    for seed in SEEDS:
        g = gen(seed)
        x = torch.randn(T, m.hidden_dim, device=DEV, generator=g)
        gy = torch.randn(T, m.hidden_dim, device=DEV, generator=g)
        if m.activation != "swiglu_clamp":
            return x, gy, reference64(m, x, tpe, offs, gy)
        x = x * (4.0 / float(reference64(m, x, tpe, offs, gy)[-1][cov].std()))
        ref = reference64(m, x, tpe, offs, gy)
        gu, F, lim = ref[-1][cov], m.ffn_dim, m.activation_limit
        sg, su = clamped_share(gu, lim)
        near = min(float((gu[:, :F] - lim).abs().min()), float((gu[:, F:].abs() - lim).abs().min()))
        print(f"glu layer problem seed={seed} std={float(gu.std()):.3f} clamped g={sg:.3f} u={su:.3f} nearest={near:.3e}")
        assert 0.01 < sg < 0.5 and 0.01 < su < 0.5
        if near > 1e-5 * lim:
            return x, gy, ref
    pytest.fail("no seed keeps every reference g and u away from the clamp boundaries")


# ---- 6. the float32 layers against float64 --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lora", [False, True])
def test_float32_layer_against_float64(lora, kind):
    E, H, F = 3, 256, 384
    m = lora_layer(E, H, F, kind, 16) if lora else base_layer(E, H, F, kind)
    tpe, offs, T = expert_table([30, 0, 50], gaps=[0, 0, 2], tail=1)
    x, gy, ref = float32_problem(m, tpe, offs, T)
    got = run(m, x, tpe, offs, gy)
    errs = {n: rel_fro_dev(a, b) for n, a, b in zip(NAMES, got, ref) if a is not None}
    print(f"ERR glu layer {kind} lora={lora} " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    assert set(errs) == (set(NAMES) if lora else {"y", "dx"})
    assert errs.pop("y") < tol(fro_tol(3, F))
    for n, e in errs.items():
        assert e < FFN_REL_FRO, (n, e)
    again = run(m, x, tpe, offs, gy)                               # two passes: identical bits
    for n, a, b in zip(NAMES, got, again):
        assert a is None or same_bits(a, b), n
    with torch.no_grad():
        assert same_bits(m(x, tpe, offs), got[0])


# ---- 6. the 16-bit layers are the documented chain ------------------------------------------------------------------------

def chain_lora(m, x, tpe, offs, gy, dt):
    """INTEGRATION.md section 9 written out with the FLOAT32 public ops; .to(dt) at the five rounding points."""
    o, s, prec, E, kw = ops(), m.scaling, m.precision, m.num_experts, act_kw(*m.activation_args)
    gu_w = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points)
    d_w = (m.down_packed, m.down_scales, m.down_zero_points)
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach() for n in ADAPTERS)
    x32 = x.float()
    gu32 = o.moe_forward(*gu_w, x32, None, tpe, offs, precision=prec)
    U_gu = o.lora_shrink(x32, A_gu, "rc", tpe, offs)
    gate_up = o.lora_expand(U_gu, B_gu, "cr", tpe, offs, scale=s, input=gu32).to(dt)                 # rounding 1
    y32 = o.moe_gated_forward(*d_w, gate_up.float(), tpe, offs, precision=prec, **kw)
    U_d = o.lora_gated_shrink(gate_up.float(), A_d, "rc", tpe, offs, **kw)
    y = o.lora_expand(U_d, B_d, "cr", tpe, offs, scale=s, input=y32).to(dt)                          # rounding 2
    g32 = gy.float()
    dB_d = o.lora_grad(g32, U_d, "cr", E, tpe, offs, scale=s)
    dU_d = o.lora_shrink(g32, B_d, "cr", tpe, offs, scale=s)
    dA_d = o.lora_gated_grad(gate_up.float(), dU_d, "rc", E, tpe, offs, **kw)
    dh32 = o.moe_backward_input(*d_w, g32, tpe, offs, precision=prec)
    dh = o.lora_expand(dU_d, A_d, "rc", tpe, offs, input=dh32).to(dt)                                # rounding 3
    dgu = o.glu_backward(gate_up.float(), dh.float(), **kw).to(dt)                                   # rounding 4
    dB_gu = o.lora_grad(dgu.float(), U_gu, "cr", E, tpe, offs, scale=s)
    dU_gu = o.lora_shrink(dgu.float(), B_gu, "cr", tpe, offs, scale=s)
    gx32 = o.moe_backward_input(*gu_w, dgu.float(), tpe, offs, precision=prec)
    dx = o.lora_expand(dU_gu, A_gu, "rc", tpe, offs, input=gx32).to(dt)                              # rounding 5
    dA_gu = o.lora_grad(x32, dU_gu, "rc", E, tpe, offs)
    return y, dx, dA_gu, dB_gu, dA_d, dB_d


def chain_base(m, x, tpe, offs, gy, dt):
    o, prec, kw = ops(), m.precision, act_kw(*m.activation_args)
    gu_w = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points)
    d_w = (m.down_packed, m.down_scales, m.down_zero_points)
    gate_up = o.moe_forward(*gu_w, x.float(), None, tpe, offs, precision=prec).to(dt)
    y = o.moe_gated_forward(*d_w, gate_up.float(), tpe, offs, precision=prec, **kw).to(dt)
    dh = o.moe_backward_input(*d_w, gy.float(), tpe, offs, precision=prec).to(dt)
    dgu = o.glu_backward(gate_up.float(), dh.float(), **kw).to(dt)
    dx = o.moe_backward_input(*gu_w, dgu.float(), tpe, offs, precision=prec).to(dt)
    return y, dx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lora", [False, True])
def test_16bit_layer_is_the_documented_chain(lora, dtype, kind):
    E, H, F = 4, 128, 160
    m = lora_layer(E, H, F, kind, 16, dtype) if lora else base_layer(E, H, F, kind, dtype)
    tpe, offs, T = expert_table([17, 0, 33, 5], gaps=[2, 0, 3, 1], tail=3)
    g = gen(5)
    x = (4.0 * torch.randn(T, H, device=DEV, generator=g)).to(dtype)    # gate_up of a few units: the clamp is active
    gy = torch.randn(T, H, device=DEV, generator=g).to(dtype)
    got = run(m, x, tpe, offs, gy)
    with torch.no_grad():
        want = (chain_lora if lora else chain_base)(m, x, tpe, offs, gy, dtype)
        gate_up = ops().moe_forward(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, x.float(), None, tpe, offs)
    if kind == "swiglu_clamp":
        cov = gate_up.abs().sum(dim=1) > 0
        assert min(clamped_share(gate_up[cov])) > 0.01
    for n, a, b in zip(NAMES, got, want):
        assert a.dtype == (dtype if n in ("y", "dx") else torch.float32), n
        assert same_bits(a, b), n
        assert float(a.abs().max()) > 0, n
    again = run(m, x, tpe, offs, gy)
    for n, a, b in zip(NAMES, got, again):
        assert a is None or same_bits(a, b), n
    with torch.no_grad():
        y0 = m(x, tpe, offs)
    assert y0.grad_fn is None and same_bits(y0, got[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [None, torch.bfloat16])
@pytest.mark.parametrize("lora", [False, True])
def test_nothing_of_shape_T_F_is_saved(lora, dtype, kind):
    E, H, F = 3, 128, 192
    m = lora_layer(E, H, F, kind, 8, dtype) if lora else base_layer(E, H, F, kind, dtype)
    tpe, offs, T = expert_table([20, 0, 30])
    saved = []

    def pack(t):
        saved.append(t)
        return t

    x = torch.randn(T, H, device=DEV).to(dtype or torch.float32).requires_grad_()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = m(x, tpe, offs)
    assert any(tuple(t.shape) == (T, 2 * F) for t in saved)       # gate_up is what the backward keeps
    assert not any(tuple(t.shape) == (T, F) for t in saved)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad.float()).all()


# ---- 7. the sparse block --------------------------------------------------------------------------------------------------

def test_sparse_block_is_the_chain_of_public_ops():
    E, H, F, top_k, T = 4, 64, 64, 2, 37
    torch.manual_seed(21)
    w = lambda n, k: [torch.randn(n, k) * 0.1 for _ in range(E)]
    gate, up, down = w(F, H), w(F, H), w(H, F)
    m = fq().QuantizedSparseMoEBlock.from_weights(torch.randn(E, H) * 0.5, gate, up, down, top_k=top_k,
                                                   shared=(gate[0] * 0.5, up[1], down[2]), activation="gelu_tanh").to(DEV)
    assert m.experts.activation == "gelu_tanh" and m.shared_experts.activation == "gelu_tanh"
    g = gen(3)
    x = torch.randn(T, H, device=DEV, generator=g)
    gout = torch.randn(T, H, device=DEV, generator=g)

    xg = x.clone().requires_grad_(True)
    m.gate.weight.grad = None
    out, logits = m(xg)
    out.backward(gout)
    got = (out.detach(), logits.detach(), xg.grad.clone(), m.gate.weight.grad.clone())

    o = ops()
    xc = x.clone().requires_grad_(True)
    m.gate.weight.grad = None
    lg = torch.nn.functional.linear(xc, m.gate.weight)
    weights, indices, *_ = o.router_score_topk(lg, m.top_k, m.scoring, m.selection_bias, m.n_group, m.topk_group,
                                               m.group_top, m.renormalize, m.routed_scaling_factor, return_scores=True)
    tpe, offs, token_of_sorted, pos_of_slot = o.route_plan(indices, E)
    y = m.experts(o.dispatch_rows(xc, token_of_sorted, pos_of_slot, top_k), tpe, offs)
    s = m.shared_experts(xc, torch.full((1,), T, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    want_out = o.combine_any(y, pos_of_slot, weights, addend=s, addend_weight=None, out_dtype=x.dtype)
    want_out.backward(gout)
    want = (want_out.detach(), lg.detach(), xc.grad, m.gate.weight.grad)
    for n, a, b in zip(("out", "logits", "dx", "dgate"), got, want):
        assert same_bits(a, b), n
        assert float(a.abs().max()) > 0, n
    # the experts really are the GeGLU ones: the silu block on the same weights differs
    silu = fq().QuantizedSparseMoEBlock.from_weights(m.gate.weight.detach().cpu(), gate, up, down, top_k=top_k,
                                                      shared=(gate[0] * 0.5, up[1], down[2])).to(DEV)
    with torch.no_grad():
        assert not torch.equal(silu(x)[0], got[0])


# ---- 8. the default is untouched ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [None, torch.bfloat16])
@pytest.mark.parametrize("lora", [False, True])
def test_explicit_silu_layer_is_the_default_layer(lora, dtype):
    E, H, F = 4, 128, 160
    tpe, offs, T = expert_table([17, 0, 33, 5], gaps=[2, 0, 3, 1], tail=3)
    g = gen(9)
    x = torch.randn(T, H, device=DEV, generator=g).to(dtype or torch.float32)
    gy = torch.randn(T, H, device=DEV, generator=g).to(dtype or torch.float32)
    explicit = lora_layer(E, H, F, "silu", 16, dtype) if lora else base_layer(E, H, F, "silu", dtype)
    base = fq().QuantizedMoEFFN(E, H, F, activation_dtype=dtype)
    for name, buf in explicit.named_buffers():
        setattr(base, name, buf)
    default = base
    if lora:
        default = fq().LoRAQuantizedMoEFFN.from_quantized(base, 16, alpha=32)
        with torch.no_grad():
            for n in ADAPTERS:
                getattr(default, n).copy_(getattr(explicit, n))
    a, b = run(explicit, x, tpe, offs, gy), run(default, x, tpe, offs, gy)
    for n, p, q in zip(NAMES, a, b):
        assert (p is None and q is None) or same_bits(p, q), n


def test_explicit_silu_block_is_the_default_block():
    E, H, F, T = 4, 64, 64, 37
    torch.manual_seed(22)
    w = lambda n, k: [torch.randn(n, k) * 0.1 for _ in range(E)]
    gate, up, down, gw = w(F, H), w(F, H), w(H, F), torch.randn(E, H) * 0.5
    kw = dict(top_k=2, shared=(gate[0], up[1], down[2]))
    a = fq().QuantizedSparseMoEBlock.from_weights(gw, gate, up, down, **kw).to(DEV)
    b = fq().QuantizedSparseMoEBlock.from_weights(gw, gate, up, down, activation="silu", activation_alpha=3.0, **kw).to(DEV)
    x = torch.randn(T, H, device=DEV, generator=gen(4))
    res = []
    for m in (a, b):
        xg = x.clone().requires_grad_(True)
        out, _ = m(xg)
        out.backward(torch.ones_like(out))
        res.append((out.detach(), xg.grad, m.gate.weight.grad))
    for p, q in zip(*res):
        assert same_bits(p, q)
