"""The gated INT4 FFN experts and their adapters on float16 / bfloat16 activations (FQL_VERSION 260).

Kernels (ops.moe_gated_forward, lora_gated_shrink, lora_gated_grad, swiglu_backward): one contract, that of INTEGRATION.md
section 8 -- a 16-bit call returns, bit for bit, the float32 op on the exactly widened operands, rounded once as
``Tensor.to(dtype)`` rounds.  So they are ``torch.equal`` against the float32 ops.

Layers (QuantizedMoEFFN / LoRAQuantizedMoEFFN built with ``activation_dtype``): ``gate_up`` is stored in 16 bits, so the
layer is NOT the float32 layer rounded once; it is the chain of INTEGRATION.md section 9 with five tensors rounded once
each, and the tests write that chain out from the float32 public ops.  Against float64 the layer is held to 1.5 times the
error of a torch reference that rounds at the same five points, plus the float32 layers' 2e-5 (the 1.5: rounding ties
fall differently once the integer GEMM and a float32 matmul differ in the last bits).

Errors measured on an MI355X are listed in DESIGN.md section 13."""
import itertools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import clipped_ranges, dequant_f64, expert_table, fq, ops, rel_fro_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
FFN_REL_FRO = 2e-5             # the float32 layers' bound (tests/test_gpu_ffn_lora.py)
ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
NAMES = ("y", "dx", "dA_gu", "dB_gu", "dA_d", "dB_d")


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand16(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def offset_view(t, nbytes):
    """A contiguous copy of the 16-bit ``t`` whose storage starts ``nbytes`` past a 16-byte boundary."""
    k = nbytes // 2
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def covered_mask(tpe, offs, T):
    m = torch.zeros(T, dtype=torch.bool)
    for lo, hi in clipped_ranges(tpe.cpu(), offs.cpu(), T):
        m[lo:hi] = True
    return m.to(DEV)


# ---- gated forward --------------------------------------------------------------------------------------------------

_WEIGHTS = {}


def down_weights(E, K, N, seed=3):
    """[E, N, K/2] per-row INT4 weights of the down projection (contraction over K = F), quantised once per shape."""
    key = (E, K, N, seed)
    if key not in _WEIGHTS:
        torch.manual_seed(seed)
        q = [fq().quantize_weights(torch.randn(N, K) * 0.1) for _ in range(E)]
        _WEIGHTS[key] = tuple(torch.stack([t[i] for t in q]).to(DEV) for i in range(3))
    return _WEIGHTS[key]


def ragged(T):
    """E = 3 with an empty expert and uncovered rows: T - 4 covered rows (one uncovered in front, one between, two
    behind); for a handful of rows, T - 2 covered (one in front, one behind)."""
    if T < 10:
        return expert_table([T - 3, 0, 1], gaps=[1, 0, 0], tail=1)
    a = (T - 4) // 3
    return expert_table([a, 0, T - 4 - a], gaps=[1, 0, 1], tail=2)


def check_gated_forward(gu, P, S, Z, tpe, offs, precision, dtype):
    want32 = ops().moe_gated_forward(P, S, Z, gu.float(), tpe, offs, precision=precision)
    got = ops().moe_gated_forward(P, S, Z, gu, tpe, offs, precision=precision)
    assert got.dtype == dtype and torch.equal(got, want32.to(dtype))
    assert torch.equal(ops().moe_gated_forward(P, S, Z, gu, tpe, offs, precision=precision, out_dtype=dtype), got)
    got32 = ops().moe_gated_forward(P, S, Z, gu, tpe, offs, precision=precision, out_dtype=torch.float32)
    assert got32.dtype == torch.float32 and torch.equal(got32, want32)
    assert torch.isfinite(want32).all() and float(want32.abs().max()) > 0
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("precision", ["int8", "fast", "default"])
@pytest.mark.parametrize("T", [5, 700])                 # one row per workgroup / ACT_ROWS rows (T + 32 E > 512)
def test_gated_forward_equals_float32_on_widened(T, precision, dtype):
    K, N = 96, 160
    P, S, Z = down_weights(3, K, N)
    tpe, offs, T_ = ragged(T)
    assert T_ == T
    gu = rand16((T, 2 * K), dtype, gen(T))
    got = check_gated_forward(gu, P, S, Z, tpe, offs, precision, dtype)
    unc = ~covered_mask(tpe, offs, T)
    assert int(unc.sum()) == (2 if T < 10 else 4) and torch.count_nonzero(got[unc]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_forward_slab_loop(dtype):
    K, N, T = 4128, 160, 37                             # K > 4096: the 4096-k slab loop of the pre-pass
    P, S, Z = down_weights(3, K, N)
    tpe, offs, _ = ragged(T)
    check_gated_forward(rand16((T, 2 * K), dtype, gen(K)), P, S, Z, tpe, offs, "default", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("precision", ["fast", "default"])
def test_gated_forward_misaligned_base(precision, dtype):
    K, N, T = 96, 160, 41
    P, S, Z = down_weights(3, K, N)
    tpe, offs, _ = ragged(T)
    gu = offset_view(rand16((T, 2 * K), dtype, gen(41)), 2)      # 2 bytes off: the element-load pre-pass
    check_gated_forward(gu, P, S, Z, tpe, offs, precision, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("precision", ["fast", "default"])
def test_gated_forward_heavy_tailed_row(precision, dtype):
    K, N, T = 96, 160, 37
    P, S, Z = down_weights(3, K, N)
    tpe, offs, _ = ragged(T)
    x = torch.randn(T, 2 * K, device=DEV, generator=gen(7))
    x[5, 17] = 1.0e4                                             # h[5, 17] ~ 1e4 times the rest: the residual limb set
    x[5, K + 17] = 1.0
    check_gated_forward(x.to(dtype), P, S, Z, tpe, offs, precision, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_forward_dense(dtype):
    """E = 1 with NULL tables, straight at the C entry point (the Python op always passes a table)."""
    from fused_int4_amd import _native
    K, N, T = 96, 160, 37
    P, S, Z = down_weights(1, K, N)
    gu = rand16((T, 2 * K), dtype, gen(11))
    L = _native.lib()
    code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

    def call(x, out):
        nbytes = L.fql_moe_workspace_bytes(1, T, K, N, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        rc = L.fql_moe_gated_fwd(P.data_ptr(), S.data_ptr(), Z.data_ptr(), x.data_ptr(), code[x.dtype], None, None,
                                 out.data_ptr(), code[out.dtype], 1, T, K, N, 0, ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        return out

    want = call(gu.float(), torch.empty(T, N, device=DEV))
    assert torch.equal(call(gu, torch.empty(T, N, device=DEV, dtype=dtype)), want.to(dtype))
    assert torch.equal(call(gu, torch.empty(T, N, device=DEV)), want)
    one = torch.tensor([T], dtype=torch.int32, device=DEV)
    assert torch.equal(ops().moe_gated_forward(P, S, Z, gu, one, one * 0), want.to(dtype))


# ---- gated shrink and grad ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [4, 8, 16, 32, 64])    # every rank in ops.LORA_RANKS (asserted below)
@pytest.mark.parametrize("C", [2816, 130, 129])          # 4, 2 and 1 elements per load
@pytest.mark.parametrize("grouped", [True, False])
def test_gated_shrink_and_grad_equal_float32_on_widened(grouped, C, r, dtype):
    assert tuple(ops().LORA_RANKS) == (4, 8, 16, 32, 64)
    g = gen(C + r)
    if grouped:
        tpe, offs, T = ragged(48)
        E = 3
    else:
        tpe = offs = None
        T, E = 21, 1
    gu = rand16((T, 2 * C), dtype, g)
    v = torch.randn(T, r, device=DEV, generator=g)
    for layout in ("rc", "cr"):
        w = torch.randn((E, r, C) if layout == "rc" else (E, C, r), device=DEV, generator=g) * 0.1
        w = w if grouped else w[0]
        u16 = ops().lora_gated_shrink(gu, w, layout, tpe, offs, scale=1.5)
        d16 = ops().lora_gated_grad(gu, v, layout, E, tpe, offs, scale=0.5)
        assert u16.dtype == torch.float32 and d16.dtype == torch.float32
        assert torch.equal(u16, ops().lora_gated_shrink(gu.float(), w, layout, tpe, offs, scale=1.5))
        assert torch.equal(d16, ops().lora_gated_grad(gu.float(), v, layout, E, tpe, offs, scale=0.5))
        assert float(u16.abs().max()) > 0 and float(d16.abs().max()) > 0


# ---- swiglu_backward ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,offset", [(32, 0), (130, 0), (129, 0), (2816, 0), (2816, 2)])
def test_swiglu_backward_equals_float32_on_widened(F, offset, dtype):
    T = 19
    g = gen(F + offset)
    gu, dh = rand16((T, 2 * F), dtype, g), rand16((T, F), dtype, g)
    if offset:
        gu = offset_view(gu, offset)
    want32 = ops().swiglu_backward(gu.float(), dh.float())
    got = ops().swiglu_backward(gu, dh)
    assert got.dtype == dtype and torch.equal(got, want32.to(dtype))
    # mixed types: a float32 dh, or a float32 result
    assert torch.equal(ops().swiglu_backward(gu, dh.float()), want32.to(dtype))
    assert torch.equal(ops().swiglu_backward(gu, dh.float(), out_dtype=dtype), want32.to(dtype))
    assert torch.equal(ops().swiglu_backward(gu, dh, out_dtype=torch.float32), want32)
    assert torch.equal(ops().swiglu_backward(gu.float(), dh, out_dtype=dtype), want32.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", [0, 1])
def test_swiglu_backward_grid(pad, dtype):
    """g across both tails of the sigmoid and both zeros, crossed with a few u and dh; zeros keep their sign."""
    gs = [-200.0, -90.0, -20.0, -1.0, -0.0, 0.0, 1.0, 20.0, 90.0, 200.0]
    combos = list(itertools.product(gs, [-3.0, -0.0, 0.0, 3.0], [-3.0, -0.0, 0.0, 0.5, 3.0]))
    combos += [(0.0, 0.0, 0.0)] * ((-len(combos)) % 4 + 4 * pad + (0 if pad else 1))     # pad 0: odd width, 2-byte loads
    gv, uv, dv = (torch.tensor(c, dtype=torch.float32, device=DEV).to(dtype) for c in zip(*combos))
    gu, dh = torch.cat([gv, uv]).reshape(1, -1), dv.reshape(1, -1)
    want = ops().swiglu_backward(gu.float(), dh.float()).to(dtype)
    got = ops().swiglu_backward(gu, dh)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))          # torch.equal holds -0 == +0: check the signs
    assert bool(torch.signbit(got[got == 0]).any()) and bool((~torch.signbit(got[got == 0])).any())


def test_swiglu_backward_float16_overflow():
    F = 8
    g = torch.full((1, F), 10.0, device=DEV)
    u = torch.tensor([300.0, -300.0, 250.0, 1.0, 200.0, -200.0, 100.0, 2.0], device=DEV).reshape(1, F)
    dh = torch.tensor([300.0, 300.0, 300.0, 1.0, 300.0, 330.0, 100.0, 60000.0], device=DEV).reshape(1, F)
    gu = torch.cat([g, u], dim=1).half()
    dh = dh.half()
    want32 = ops().swiglu_backward(gu.float(), dh.float())
    assert torch.isfinite(want32).all() and int((want32.abs() > 65504).sum()) >= 4     # finite in float32, past float16
    want = want32.to(torch.float16)
    assert int(torch.isinf(want).sum()) >= 4 and int(torch.isfinite(want).sum()) >= 4
    got = ops().swiglu_backward(gu, dh)
    assert torch.equal(got, want)
    assert torch.equal(ops().swiglu_backward(gu, dh.float(), out_dtype=torch.float16), want)


# ---- the layers -----------------------------------------------------------------------------------------------------

E_, H_, F_ = 4, 128, 160
_BASES = {}


def base_layer(dtype, seed=5, E=E_, H=H_, F=F_, precision="default"):
    key = (E, H, F, seed, precision)
    if key not in _BASES:
        torch.manual_seed(seed)
        gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
        up = [torch.randn(F, H) * 0.1 for _ in range(E)]
        down = [torch.randn(H, F) * 0.1 for _ in range(E)]
        _BASES[key] = fq().QuantizedMoEFFN.from_weights(gate, up, down, precision=precision).to(DEV)
    b = _BASES[key]
    m = fq().QuantizedMoEFFN(E, H, F, precision=precision, activation_dtype=dtype)
    for name, buf in b.named_buffers():
        setattr(m, name, buf)
    return m


def ffn_layer(dtype, r, seed=5, **kw):
    base = base_layer(dtype, seed, **kw)
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, r, alpha=2 * r)
    assert m.activation_dtype == dtype
    g = gen(seed + r)
    with torch.no_grad():
        m.gate_up_lora_B.normal_(0, 0.1, generator=g)
        m.down_lora_B.normal_(0, 0.1, generator=g)
    return m


def problem(dtype, counts=(17, 0, 33, 5), gaps=(2, 0, 3, 1), tail=3, seed=5, H=H_):
    tpe, offs, T = expert_table(list(counts), gaps=list(gaps), tail=tail)
    g = gen(seed)
    return tpe, offs, T, rand16((T, H), dtype, g), rand16((T, H), dtype, g)


def run(m, x, tpe, offs, gy, requires=("x",) + ADAPTERS):
    for name in ADAPTERS:
        p = getattr(m, name, None)
        if p is not None:
            p.grad = None
            p.requires_grad_(name in requires)
    xg = x.detach().clone().requires_grad_("x" in requires)
    y = m(xg, tpe, offs)
    y.backward(gy)
    out = (y.detach(), xg.grad) + tuple(getattr(getattr(m, name, None), "grad", None) for name in ADAPTERS)
    for name in ADAPTERS:
        if getattr(m, name, None) is not None:
            getattr(m, name).requires_grad_(True)
    return out


def chain_lora(m, x, tpe, offs, gy, dt):
    """INTEGRATION.md section 9 written out with the FLOAT32 public ops; .to(dt) at the five rounding points."""
    o, s, prec, E = ops(), m.scaling, m.precision, m.num_experts
    gu_w = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points)
    d_w = (m.down_packed, m.down_scales, m.down_zero_points)
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach() for n in ADAPTERS)
    x32 = x.float()
    gu32 = o.moe_forward(*gu_w, x32, None, tpe, offs, precision=prec)
    U_gu = o.lora_shrink(x32, A_gu, "rc", tpe, offs)
    gate_up = o.lora_expand(U_gu, B_gu, "cr", tpe, offs, scale=s, input=gu32).to(dt)                 # rounding 1
    y32 = o.moe_gated_forward(*d_w, gate_up.float(), tpe, offs, precision=prec)
    U_d = o.lora_gated_shrink(gate_up.float(), A_d, "rc", tpe, offs)
    y = o.lora_expand(U_d, B_d, "cr", tpe, offs, scale=s, input=y32).to(dt)                          # rounding 2
    g32 = gy.float()
    dB_d = o.lora_grad(g32, U_d, "cr", E, tpe, offs, scale=s)
    dU_d = o.lora_shrink(g32, B_d, "cr", tpe, offs, scale=s)
    dA_d = o.lora_gated_grad(gate_up.float(), dU_d, "rc", E, tpe, offs)
    dh32 = o.moe_backward_input(*d_w, g32, tpe, offs, precision=prec)
    dh = o.lora_expand(dU_d, A_d, "rc", tpe, offs, input=dh32).to(dt)                                # rounding 3
    dgu = o.swiglu_backward(gate_up.float(), dh.float()).to(dt)                                      # rounding 4
    dB_gu = o.lora_grad(dgu.float(), U_gu, "cr", E, tpe, offs, scale=s)
    dU_gu = o.lora_shrink(dgu.float(), B_gu, "cr", tpe, offs, scale=s)
    gx32 = o.moe_backward_input(*gu_w, dgu.float(), tpe, offs, precision=prec)
    dx = o.lora_expand(dU_gu, A_gu, "rc", tpe, offs, input=gx32).to(dt)                              # rounding 5
    dA_gu = o.lora_grad(x32, dU_gu, "rc", E, tpe, offs)
    return y, dx, dA_gu, dB_gu, dA_d, dB_d


def chain_base(m, x, tpe, offs, gy, dt):
    o, prec = ops(), m.precision
    gu_w = (m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points)
    d_w = (m.down_packed, m.down_scales, m.down_zero_points)
    gate_up = o.moe_forward(*gu_w, x.float(), None, tpe, offs, precision=prec).to(dt)
    y = o.moe_gated_forward(*d_w, gate_up.float(), tpe, offs, precision=prec).to(dt)
    dh = o.moe_backward_input(*d_w, gy.float(), tpe, offs, precision=prec).to(dt)
    dgu = o.swiglu_backward(gate_up.float(), dh.float()).to(dt)
    dx = o.moe_backward_input(*gu_w, dgu.float(), tpe, offs, precision=prec).to(dt)
    return y, dx


CASES = {"ragged": dict(), "one_row": dict(counts=(1, 0, 0, 0), gaps=(0, 0, 0, 0), tail=0)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_lora_layer_is_the_documented_chain(case, r, dtype):
    m = ffn_layer(dtype, r)
    tpe, offs, T, x, gy = problem(dtype, **CASES[case])
    got = run(m, x, tpe, offs, gy)
    with torch.no_grad():
        want = chain_lora(m, x, tpe, offs, gy, dtype)
    for n, a, b in zip(NAMES, got, want):
        assert a.dtype == (dtype if n in ("y", "dx") else torch.float32), n
        assert torch.equal(a, b), n
        assert float(a.abs().max()) > 0, n
    again = run(m, x, tpe, offs, gy)                                     # run to run
    for n, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), n
    with torch.no_grad():                                                # under no_grad: same bits, no graph
        y0 = m(x, tpe, offs)
    assert y0.grad_fn is None and not y0.requires_grad and torch.equal(y0, got[0])
    unc = ~covered_mask(tpe, offs, T)
    assert torch.count_nonzero(got[0][unc]) == 0 and torch.count_nonzero(got[1][unc]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_base_layer_is_the_documented_chain(case, dtype):
    m = base_layer(dtype)
    tpe, offs, T, x, gy = problem(dtype, **CASES[case])
    y, dx = run(m, x, tpe, offs, gy)[:2]
    with torch.no_grad():
        want_y, want_dx = chain_base(m, x, tpe, offs, gy, dtype)
        y0 = m(x, tpe, offs)
    assert y.dtype == dtype and dx.dtype == dtype
    assert torch.equal(y, want_y) and torch.equal(dx, want_dx) and torch.equal(y0, y) and y0.grad_fn is None
    y2, dx2 = run(m, x, tpe, offs, gy)[:2]
    assert torch.equal(y, y2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_equals_per_expert(dtype):
    m = ffn_layer(dtype, 16)
    tpe, offs, T, x, gy = problem(dtype)
    y, dx, *grads = run(m, x, tpe, offs, gy)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            for n, gr in zip(NAMES[2:], grads):
                assert torch.count_nonzero(gr[e]) == 0, n
            continue
        xe = x[lo:hi].clone().requires_grad_()
        ad = [getattr(m, n)[e:e + 1].detach().clone().requires_grad_() for n in ADAPTERS]
        ye = ops().moe_ffn_lora_forward(m.gate_up_packed[e:e + 1], m.gate_up_scales[e:e + 1],
                                        m.gate_up_zero_points[e:e + 1], m.down_packed[e:e + 1], m.down_scales[e:e + 1],
                                        m.down_zero_points[e:e + 1], xe, *ad, m.scaling, one * (hi - lo), one * 0,
                                        precision=m.precision, activation_dtype=dtype)
        ye.backward(gy[lo:hi].clone())
        assert torch.equal(y[lo:hi], ye.detach()), e
        assert torch.equal(dx[lo:hi], xe.grad), e
        for n, gr, a in zip(NAMES[2:], grads, ad):
            assert torch.equal(gr[e], a.grad[0]), (n, e)


def reference(m, x, tpe, offs, gy, dt):
    """The same network on the dequantised weights: float64 without rounding when ``dt`` is None; else float32 matmuls
    with the intermediates rounded to ``dt`` at the five points of the layer (gate_up, y, dh, dgu, dx)."""
    wt = torch.float64 if dt is None else torch.float32
    E, F, s, T = m.num_experts, m.ffn_dim, m.scaling, x.shape[0]
    rnd = (lambda t: t) if dt is None else (lambda t: t.to(dt).to(wt))
    Wgu = [dequant_f64(m.gate_up_packed[e], m.gate_up_scales[e], m.gate_up_zero_points[e]).to(wt) for e in range(E)]
    Wd = [dequant_f64(m.down_packed[e], m.down_scales[e], m.down_zero_points[e]).to(wt) for e in range(E)]
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach().to(wt) for n in ADAPTERS)
    x_, g_ = x.to(wt), gy.to(wt)
    y, dx = torch.zeros(T, m.hidden_dim, dtype=wt, device=DEV), torch.zeros(T, m.hidden_dim, dtype=wt, device=DEV)
    dA_gu, dB_gu, dA_d, dB_d = (torch.zeros_like(t) for t in (A_gu, B_gu, A_d, B_d))
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            continue
        xe, ge = x_[lo:hi], g_[lo:hi]
        U_gu = xe @ A_gu[e].t()
        gu = rnd(xe @ Wgu[e].t() + s * U_gu @ B_gu[e].t())                                     # rounding 1
        g, u = gu[:, :F], gu[:, F:]
        sig = torch.sigmoid(g)
        h = g * sig * u
        U_d = h @ A_d[e].t()
        y[lo:hi] = rnd(h @ Wd[e].t() + s * U_d @ B_d[e].t())                                   # rounding 2
        dB_d[e] = s * ge.t() @ U_d
        dU_d = s * ge @ B_d[e]
        dA_d[e] = dU_d.t() @ h
        dh = rnd(ge @ Wd[e] + dU_d @ A_d[e])                                                   # rounding 3
        dgu = rnd(torch.cat([dh * u * (sig * (1 + g * (1 - sig))), dh * (g * sig)], dim=1))    # rounding 4
        dB_gu[e] = s * dgu.t() @ U_gu
        dU_gu = s * dgu @ B_gu[e]
        dx[lo:hi] = rnd(dgu @ Wgu[e] + dU_gu @ A_gu[e])                                        # rounding 5
        dA_gu[e] = dU_gu.t() @ xe
    return y, dx, dA_gu, dB_gu, dA_d, dB_d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [4, 16])
def test_lora_layer_against_float64(r, dtype):
    m = ffn_layer(dtype, r)
    tpe, offs, T, x, gy = problem(dtype)
    got = run(m, x, tpe, offs, gy)
    with torch.no_grad():
        ref64 = reference(m, x, tpe, offs, gy, None)
        ref_dt = reference(m, x, tpe, offs, gy, dtype)
    for n, a, t, r64 in zip(NAMES, got, ref_dt, ref64):
        ours, torch_ref = rel_fro_dev(a, r64), rel_fro_dev(t, r64)
        print(f"ERR ffn16 {dtype} r={r} {n} ours={ours:.3e} torch_ref={torch_ref:.3e}")
        assert ours <= 1.5 * torch_ref + FFN_REL_FRO, (n, ours, torch_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_saved_activations(dtype):
    r = 8
    m = ffn_layer(dtype, r)
    tpe, offs, T, x, gy = problem(dtype)
    H, F = m.hidden_dim, m.ffn_dim
    known = {t.data_ptr() for t in itertools.chain(m.parameters(), m.buffers())} | {tpe.data_ptr(), offs.data_ptr()}
    saved = []

    def pack(t):
        saved.append(t)
        return t

    xg = x.clone().requires_grad_()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = m(xg, tpe, offs)
    acts = {t.data_ptr(): t for t in saved if t.data_ptr() not in known}
    assert sum(t.numel() * t.element_size() for t in acts.values()) == T * (2 * H + 4 * F + 8 * r)
    for t in acts.values():
        assert not (t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] in (H, F, 2 * F)), tuple(t.shape)
    y.backward(gy)
    assert xg.grad.dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lora", [True, False])
def test_no_hidden_widening(lora, dtype):
    """No aten::to / aten::_to_copy touches a [T, H], [T, F] or [T, 2F] tensor in one forward + backward."""
    from torch.profiler import ProfilerActivity, profile
    T, H, F = 96, H_, F_
    sizes = {T * H, T * F, T * 2 * F}
    assert len(sizes) == 3
    m = ffn_layer(dtype, 16) if lora else base_layer(dtype)
    tpe, offs, T_ = expert_table([40, 0, 30, 26])
    assert T_ == T
    g = gen(1)
    x, gy = rand16((T, H), dtype, g), rand16((T, H), dtype, g)
    run(m, x, tpe, offs, gy)                                              # warm-up outside the profile
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        run(m, x, tpe, offs, gy)
    seen = 0
    for ev in prof.events():
        if ev.name in ("aten::to", "aten::_to_copy"):
            seen += 1
            shape = ev.input_shapes[0] if ev.input_shapes else []
            n = 1
            for d in shape:
                n *= d
            assert not (shape and n in sizes), (ev.name, shape)
    names = {ev.name for ev in prof.events()}
    assert "aten::empty" in names                                          # the profile did record operators


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(dtype):
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    m = ffn_layer(dtype, 4)
    base = base_layer(dtype)
    tpe, offs, T, x, gy = problem(dtype)
    for layer in (m, base):
        with pytest.raises(RuntimeError, match="activation_dtype"):
            layer(x.float(), tpe, offs)
        with pytest.raises(RuntimeError, match=str(dtype).replace(".", r"\.")):
            layer(x.to(other), tpe, offs)
    cast = ffn_layer(dtype, 4).to(dtype)                                   # casts the adapters too
    with pytest.raises(RuntimeError, match="stay float32|float32 CUDA"):
        cast(x, tpe, offs)
    with pytest.raises(ValueError, match="fp8"):
        fq().LoRAQuantizedMoEFFN(2, 64, 96, rank=4, precision="fp8", activation_dtype=dtype)
    with pytest.raises(ValueError, match="fp8"):
        fq().QuantizedMoEFFN(2, 64, 96, precision="fp8", activation_dtype=dtype)
    with pytest.raises(ValueError, match="activation_dtype"):
        fq().QuantizedMoEFFN(2, 64, 96, activation_dtype=torch.float64)
    # activation_dtype=None / float32 is the float32 layer: it still takes float32 and refuses 16-bit input
    plain = fq().LoRAQuantizedMoEFFN.from_quantized(base_layer(None), 4, activation_dtype=torch.float32)
    assert plain.activation_dtype is None
    assert plain(x.float(), tpe, offs).dtype == torch.float32
    with pytest.raises(RuntimeError):
        plain(x, tpe, offs)
