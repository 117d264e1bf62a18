"""float16 / bfloat16 activations on the adapter kernels, the INT4 input gradient and the LoRA modules.

One contract (include/fql_int4.h): a 16-bit call returns, bit for bit, what the float32 path
returns on the exactly widened operands, rounded once to the 16-bit type as ``Tensor.to(dtype)`` rounds -- with no float32
copy of a [T, C] tensor made on the way.  So everything here is ``torch.equal`` against the float32 ops, except the
misaligned operands (a narrower vector width than the float32 call: float64 within the float32 kernels' bound) and one
float64 check per module (u + the float32 bound, u the unit roundoff of the type)."""
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import F32_TOL, dequant_f64, expert_table, rel_fro_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TABLE = dict(counts=[7, 0, 33, 1, 20, 64], gaps=[0, 2, 0, 5, 0, 1], tail=3)    # empty expert, gaps, uncovered tail


def fq():
    import fused_int4_amd
    return fused_int4_amd


def ops():
    from fused_int4_amd import ops as o
    return o


def rand16(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, device=DEV, generator=gen) * scale).to(dtype)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def offset_view(t, nbytes):
    """A contiguous copy of the 16-bit ``t`` whose storage starts ``nbytes`` past a 16-byte boundary."""
    k = nbytes // 2
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


# ---- adapter kernels, bitwise ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("C", [4096, 1000, 130, 129])
@pytest.mark.parametrize("grouped", [True, False])
def test_kernels_equal_float32_on_widened(dtype, r, C, grouped):
    o = ops()
    g = gen(r + C)
    if grouped:
        tpe, offs, T = expert_table(**TABLE)
        E = len(TABLE["counts"])
    else:
        tpe = offs = None
        T, E = 37, 1
    X = rand16((T, C), dtype, g)
    V = torch.randn(T, r, device=DEV, generator=g)
    for layout in ("rc", "cr"):
        W = torch.randn((E, r, C) if layout == "rc" else (E, C, r), device=DEV, generator=g) * 0.1
        W = W if grouped else W[0]
        # shrink / grad: the 16-bit operand is read as it is
        assert torch.equal(o.lora_shrink(X, W, layout, tpe, offs, scale=1.5),
                           o.lora_shrink(X.float(), W, layout, tpe, offs, scale=1.5))
        assert torch.equal(o.lora_grad(X, V, layout, E, tpe, offs, scale=0.5),
                           o.lora_grad(X.float(), V, layout, E, tpe, offs, scale=0.5))
        # expand: (in, out) = (f32, 16), (16, 16), (16, 16 in place), (none, 16)
        Y32 = torch.randn(T, C, device=DEV, generator=g)
        want = o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=Y32).to(dtype)
        assert torch.equal(o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=Y32, out_dtype=dtype), want)
        want = o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=X.float()).to(dtype)
        got = o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=X)
        assert got.dtype == dtype and torch.equal(got, want)
        buf = X.clone()
        assert o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=buf, out=buf) is buf
        assert torch.equal(buf, want)
        want = o.lora_expand(V, W, layout, tpe, offs, scale=2.0, out=torch.empty(T, C, device=DEV)).to(dtype)
        assert torch.equal(o.lora_expand(V, W, layout, tpe, offs, scale=2.0, out=torch.empty(T, C, device=DEV, dtype=dtype)),
                           want)
        # 16-bit in, float32 out
        assert torch.equal(o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=X, out_dtype=torch.float32),
                           o.lora_expand(V, W, layout, tpe, offs, scale=2.0, input=X.float()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbytes", [2, 4])
@pytest.mark.parametrize("C", [4096, 130])
def test_misaligned_operand_within_the_float32_bound(dtype, nbytes, C):
    """A 16-bit operand 2 / 4 bytes past a 16-byte boundary takes a narrower vector width than the float32 call on an
    aligned copy: the float32 sums may differ in rounding, so the check is float64 within the float32 kernels' bound.
    (expand and grad do not depend on the width: they stay bitwise.)"""
    o = ops()
    g = gen(C + nbytes)
    tpe, offs, T = expert_table(**TABLE)
    E, r = len(TABLE["counts"]), 16
    X = offset_view(rand16((T, C), dtype, g), nbytes)
    A = torch.randn(E, r, C, device=DEV, generator=g) * 0.1
    V = torch.randn(T, r, device=DEV, generator=g)
    ref_u = torch.zeros(T, r, dtype=torch.float64, device=DEV)
    ref_d = torch.zeros(E, r, C, dtype=torch.float64, device=DEV)
    for e in range(E):
        lo, c = int(offs[e]), int(tpe[e])
        ref_u[lo:lo + c] = X[lo:lo + c].double() @ A[e].double().T
        ref_d[e] = V[lo:lo + c].double().T @ X[lo:lo + c].double()
    u = o.lora_shrink(X, A, "rc", tpe, offs)
    d = o.lora_grad(X, V, "rc", E, tpe, offs)
    fro_u, fro_d = rel_fro_dev(u, ref_u), rel_fro_dev(d, ref_d)
    print(f"ERR misaligned {dtype} +{nbytes}B C={C} shrink={fro_u:.3e} grad={fro_d:.3e}")
    assert fro_u < F32_TOL and fro_d < F32_TOL
    assert torch.equal(d, o.lora_grad(X.float(), V, "rc", E, tpe, offs))
    out = offset_view(torch.empty(T, C, dtype=dtype, device=DEV), nbytes)
    o.lora_expand(V, A, "rc", tpe, offs, input=X, out=out)
    assert torch.equal(out, o.lora_expand(V, A, "rc", tpe, offs, input=X.float()).to(dtype))


# ---- INT4 input gradient, bitwise -----------------------------------------------------------------------------------

def rand_weights(E, N, K, seed, frac=False):
    g = gen(seed)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    S = 0.005 + 0.01 * torch.rand(E, N, device=DEV, generator=g)
    Z = torch.randint(0, 16, (E, N), device=DEV, generator=g).float()
    if frac:
        Z = Z + torch.rand(E, N, device=DEV, generator=g) - 0.5
    return P, S, Z


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("precision", ["int8", "fast", "default"])
@pytest.mark.parametrize("K,N,frac", [(512, 1000, False), (130, 384, True)])
def test_backward_input_equals_float32_on_widened(dtype, precision, K, N, frac):
    o = ops()
    P, S, Z = rand_weights(3, N, K, seed=K + N, frac=frac)
    g = gen(7)
    def grads(T):
        """float32 randn * 0.01 with one row scaled by 1e5 and one row with a single outlier 1e4 times the rest of it
        (heavy-tailed: the residual limb set), rounded to the 16-bit type (finite in float16)."""
        g32 = torch.randn(T, N, device=DEV, generator=g) * 0.01
        if T > 9:
            g32[5] *= 1e5
            g32[9, 11] *= 1e4
        return g32.to(dtype)

    for T in (1, 3, 70):
        gy = grads(T)
        want = o.linear_backward_input(gy.float(), P[0], S[0], Z[0], precision=precision)
        for od in (torch.float32, dtype):
            got = o.linear_backward_input(gy, P[0], S[0], Z[0], precision=precision, out_dtype=od)
            assert got.dtype == od and torch.equal(got, want.to(od)), (T, od)
    tpe, offs, T = expert_table([20, 0, 37], gaps=[1, 0, 2], tail=3)
    gy = grads(T)
    want = o.moe_backward_input(P, S, Z, gy.float(), tpe, offs, precision=precision)
    for od in (torch.float32, dtype):
        got = o.moe_backward_input(P, S, Z, gy, tpe, offs, precision=precision, out_dtype=od)
        assert got.dtype == od and torch.equal(got, want.to(od)), od
    # float32 gradient in, 16-bit gradient out
    got = o.moe_backward_input(P, S, Z, gy.float(), tpe, offs, precision=precision, out_dtype=dtype)
    assert torch.equal(got, want.to(dtype))


def test_float16_overflow_follows_to_float16():
    o = ops()
    P, S, Z = rand_weights(1, 256, 256, seed=3)
    gy = rand16((8, 256), torch.float16, gen(4))
    gy[2] = 60000.0
    want = o.linear_backward_input(gy.float(), P[0], S[0] * 100.0, Z[0])
    got = o.linear_backward_input(gy, P[0], S[0] * 100.0, Z[0], out_dtype=torch.float16)
    assert torch.isinf(want.to(torch.float16)).any() and torch.isfinite(want).all()
    assert torch.equal(got, want.to(torch.float16))


# ---- modules --------------------------------------------------------------------------------------------------------

def lora_linear(N, K, r, seed, bias):
    torch.manual_seed(seed)
    base = fq().QuantizedLinear.from_linear(torch.nn.Linear(K, N, bias=bias))
    m = fq().LoRAQuantizedLinear.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        m.lora_B.normal_(0, 0.1)
    return m.to(DEV)


def lora_moe(E, N, K, r, seed):
    torch.manual_seed(seed)
    base = fq().MoEINT4.from_weights([torch.randn(N, K) * 0.05 for _ in range(E)])
    m = fq().LoRAMoEINT4.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        m.lora_B.normal_(0, 0.1)
    return m.to(DEV)


def run(m, x, gy, *table):
    for p in m.parameters():
        p.grad = None
    xx = x.detach().clone().requires_grad_()
    y = m(xx, None, *table) if table else m(xx)
    y.backward(gy)
    return y.detach(), xx.grad, m.lora_A.grad.clone(), m.lora_B.grad.clone()


def assert_contract(m, x, gy, *table):
    """16-bit run == float32 run on the widened x / gy: y and x.grad rounded once, adapter gradients float32, unrounded."""
    dtype = x.dtype
    y, gx, gA, gB = run(m, x, gy, *table)
    y32, gx32, gA32, gB32 = run(m, x.float(), gy.float(), *table)
    assert y.dtype == dtype and gx.dtype == dtype and gA.dtype == torch.float32 and gB.dtype == torch.float32
    assert torch.equal(y, y32.to(dtype))
    assert torch.equal(gx, gx32.to(dtype))
    assert torch.equal(gA, gA32) and torch.equal(gB, gB32)
    return y, gx, gA, gB


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,K,bias", [(70, 1000, 512, True), (3, 96, 64, True), (257, 384, 130, False)])
def test_linear_module_contract(dtype, B, N, K, bias):
    m = lora_linear(N, K, 16, seed=B + N, bias=bias)
    g = gen(B)
    x, gy = rand16((B, K), dtype, g), rand16((B, N), dtype, g)
    y, gx, gA, gB = assert_contract(m, x, gy)
    if B != 70:
        return
    # float64: u + the float32 bound
    W = dequant_f64(m.packed_weights, m.scales, m.zero_points)
    x64, A64, B64 = (t.detach().double().requires_grad_() for t in (x, m.lora_A, m.lora_B))
    y64 = x64 @ W.T + m.bias.double() + m.scaling * (x64 @ A64.T) @ B64.T
    y64.backward(gy.double())
    tol = UNIT[dtype] + F32_TOL
    errs = [rel_fro_dev(a, b) for a, b in ((y, y64.detach()), (gx, x64.grad), (gA, A64.grad), (gB, B64.grad))]
    print(f"ERR linear module {dtype} y={errs[0]:.3e} dx={errs[1]:.3e} dA={errs[2]:.3e} dB={errs[3]:.3e}")
    assert all(e < tol for e in errs), errs
    # 1-D input
    y1, gx1, _, _ = assert_contract(m, x[0], gy[0])
    assert y1.shape == (N,) and gx1.shape == (K,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_module_contract(dtype):
    E, N, K = 6, 1000, 256
    m = lora_moe(E, N, K, 16, seed=21)
    tpe, offs, T = expert_table(**TABLE)
    g = gen(22)
    x, gy = rand16((T, K), dtype, g), rand16((T, N), dtype, g)
    y, gx, gA, gB = assert_contract(m, x, gy, tpe, offs)
    again = run(m, x, gy, tpe, offs)
    for a, b in zip((y, gx, gA, gB), again):                       # run to run
        assert torch.equal(a, b)
    x64, A64, B64 = (t.detach().double().requires_grad_() for t in (x, m.lora_A, m.lora_B))
    parts = []
    for e in range(E):
        lo, c = int(offs[e]), int(tpe[e])
        W = dequant_f64(m.packed_weights[e], m.scales[e], m.zero_points[e])
        parts.append((lo, c, x64[lo:lo + c] @ W.T + m.scaling * (x64[lo:lo + c] @ A64[e].T) @ B64[e].T))
    y64 = torch.zeros(T, N, dtype=torch.float64, device=DEV)
    for lo, c, ye in parts:
        y64 = y64.index_put((torch.arange(lo, lo + c, device=DEV),), ye)
    y64.backward(gy.double())
    tol = UNIT[dtype] + F32_TOL
    errs = [rel_fro_dev(a, b) for a, b in ((y, y64.detach()), (gx, x64.grad), (gA, A64.grad), (gB, B64.grad))]
    print(f"ERR moe module {dtype} y={errs[0]:.3e} dx={errs[1]:.3e} dA={errs[2]:.3e} dB={errs[3]:.3e}")
    assert all(e < tol for e in errs), errs
    with torch.no_grad():                                          # same bits, nothing saved
        y0 = m(x, None, tpe, offs)
    assert y0.grad_fn is None and torch.equal(y0, y)
    lin = lora_linear(384, 256, 8, seed=23, bias=True)
    xl = rand16((40, 256), dtype, g)
    with torch.no_grad():
        y0 = lin(xl)
    assert y0.grad_fn is None and y0.dtype == dtype and torch.equal(y0, lin(xl.clone().requires_grad_()).detach())


@pytest.mark.parametrize("dtype", DTYPES)
def test_saved_activations(dtype):
    """The two nodes save x in its own type and U in float32: T (2K + 4r) bytes of [T, .] tensors, no float32 [T, K] or
    [T, N]."""
    K, N, r = 256, 384, 16

    def saved_bytes(fn, T):
        seen = {}

        def pack(t):
            seen[(t.data_ptr(), tuple(t.shape), t.dtype)] = t
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            y = fn()
        rows = [t for t in seen.values() if t.dim() == 2 and t.shape[0] == T]
        for t in rows:
            assert not (t.dtype == torch.float32 and t.shape[1] in (K, N)), (t.shape, t.dtype)
        return sum(t.numel() * t.element_size() for t in rows), y

    g = gen(31)
    T = 70
    lin = lora_linear(N, K, r, seed=30, bias=False)
    x = rand16((T, K), dtype, g).requires_grad_()
    got, _ = saved_bytes(lambda: lin(x), T)
    assert got == T * (2 * K + 4 * r)
    tpe, offs, T = expert_table(**TABLE)
    moe = lora_moe(len(TABLE["counts"]), N, K, r, seed=32)
    x = rand16((T, K), dtype, g).requires_grad_()
    got, _ = saved_bytes(lambda: moe(x, None, tpe, offs), T)
    assert got == T * (2 * K + 4 * r)


def test_no_hidden_widening():
    """One forward + backward of each layer at T = 1024, K = 4096, N = 11008 (E = 8 for the grouped one): no aten::to /
    aten::_to_copy touches a tensor of T K or T N elements."""
    from torch.profiler import ProfilerActivity, profile
    E, T, K, N, r = 8, 1024, 4096, 11008, 16
    dtype = torch.bfloat16
    g = gen(41)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    S = 0.005 + 0.01 * torch.rand(E, N, device=DEV, generator=g)
    Z = torch.randint(0, 16, (E, N), device=DEV, generator=g).float()
    A = (torch.randn(E, r, K, device=DEV, generator=g) * 0.02).requires_grad_()
    B = (torch.randn(E, N, r, device=DEV, generator=g) * 0.02).requires_grad_()
    tpe = torch.full((E,), T // E, dtype=torch.int32, device=DEV)
    offs = torch.arange(E, dtype=torch.int32, device=DEV) * (T // E)
    x = rand16((T, K), dtype, g).requires_grad_()
    gy = rand16((T, N), dtype, g)
    o = ops()

    def step():
        o.moe_lora_forward(P, S, Z, x, A, B, 2.0, tpe, offs).backward(gy)
        o.linear_lora_forward(x, P[0], S[0], Z[0], A[0], B[0], 2.0).backward(gy)
        o.moe_forward_any(P, S, Z, x, None, tpe, offs).backward(gy)
        o.linear_forward_any(x, P[0], S[0], Z[0]).backward(gy)

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        step()
        torch.cuda.synchronize()
    big = {T * K, T * N}
    casts = []
    for ev in prof.events():
        if ev.name in ("aten::to", "aten::_to_copy"):
            for shape in ev.input_shapes or []:
                n = 1
                for d in shape:
                    n *= d
                if shape and n in big:
                    casts.append((ev.name, shape))
    assert not casts, casts


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("K,N", [(130, 96), (256, 1000)])
def test_grouped_equals_per_expert_bf16(r, K, N):
    """tests/test_gpu_lora.py::test_grouped_equals_per_expert with bfloat16 [T, C] operands, and run to run."""
    o = ops()
    dt = torch.bfloat16
    tpe, offs, T = expert_table(**TABLE)
    E = len(TABLE["counts"])
    g = gen(r + K)
    X, G = rand16((T, K), dt, g), rand16((T, N), dt, g)
    A = torch.randn(E, r, K, device=DEV, generator=g) * 0.1
    B = torch.randn(E, N, r, device=DEV, generator=g) * 0.1

    def grouped():
        U = o.lora_shrink(X, A, "rc", tpe, offs)
        delta = o.lora_expand(U, B, "cr", tpe, offs, scale=2.0, out=torch.empty(T, N, device=DEV, dtype=dt))
        dU = o.lora_shrink(G, B, "cr", tpe, offs, scale=2.0)
        dX = o.lora_expand(dU, A, "rc", tpe, offs, out=torch.empty(T, K, device=DEV, dtype=dt))
        return U, delta, dU, dX, o.lora_grad(X, dU, "rc", E, tpe, offs), o.lora_grad(G, U, "cr", E, tpe, offs, scale=2.0)

    U, delta, dU, dX, dA, dB = grouped()
    for a, b in zip((U, delta, dU, dX, dA, dB), grouped()):
        assert torch.equal(a, b)
    for e in range(E):
        lo, c = int(offs[e]), int(tpe[e])
        if c == 0:
            assert (dA[e] == 0).all() and (dB[e] == 0).all()
            continue
        Xe, Ge = X[lo:lo + c].clone(), G[lo:lo + c].clone()      # (clone: a 16-byte aligned base, as the grouped call's)
        Ue = o.lora_shrink(Xe, A[e], "rc")
        dUe = o.lora_shrink(Ge, B[e], "cr", scale=2.0)
        assert torch.equal(U[lo:lo + c], Ue)
        assert torch.equal(dU[lo:lo + c], dUe)
        assert torch.equal(delta[lo:lo + c], o.lora_expand(Ue, B[e], "cr", scale=2.0, out=torch.empty(c, N, device=DEV, dtype=dt)))
        assert torch.equal(dX[lo:lo + c], o.lora_expand(dUe, A[e], "rc", out=torch.empty(c, K, device=DEV, dtype=dt)))
        assert torch.equal(dA[e], o.lora_grad(Xe, dUe, "rc")[0])
        assert torch.equal(dB[e], o.lora_grad(Ge, Ue, "cr", scale=2.0)[0])


def test_refusals():
    m = lora_moe(2, 96, 64, 4, seed=51)
    tpe, offs, T = expert_table([5, 3])
    x = torch.randn(T, 64, device=DEV)
    m.bfloat16()                                                 # casts the adapters too: refused with a clear message
    with pytest.raises(RuntimeError, match="float32"):
        m(x.bfloat16(), None, tpe, offs)
    ffn = fq().LoRAQuantizedMoEFFN(2, 64, 96, rank=4).to(DEV)
    with pytest.raises(RuntimeError, match="float32 only"):
        ffn(x.bfloat16(), tpe, offs)
