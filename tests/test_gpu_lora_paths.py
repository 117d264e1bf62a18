"""Every compiled path of the segmented LoRA kernels (csrc/fql_lora.h, fql_lora.hip) against float64 torch on the GPU.

fql_lora.hip vec_width picks the stream width of the [T][C] operands from C % 4, C % 2 and pointer alignment:
VEC = 4 / 2 / 1 floats.  Here every kernel (shrink, expand, grad) x layout (rc, cr) x VEC runs at ranks 4, 16 and 64,
through the modules and the raw ops; odd C (33, 1001) and misaligned views (helpers.misaligned) reach VEC = 1, C = 2 mod
4 (130, 1002) and 8-byte offsets reach VEC = 2.  Plus the full-size MoE shapes, segments longer than the grad kernel's
8 x 4 row blocks, tables that leave [0, T) and the edge cases of expand."""
import ctypes

import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import (ADAPTER_TOL, EXACT_REL_FRO, FMA_REL_FRO, clipped_ranges, dequant_f64, expert_table, fq, misaligned,
                     ops, rel_fro_dev, row_rel_err)

pytestmark = pytest.mark.gpu
DEV = "cuda"
# adapter terms alone: float32 FMA chains (summation order only: helpers.ADAPTER_TOL); outputs that include the INT4 GEMM:
# its exact-mode bound as well
LAYER_TOL = EXACT_REL_FRO + FMA_REL_FRO


def check(name, got, ref, tol):
    """Frobenius and per-row bound (rows of the output as stored: [T, C], or [E * r, C] / [E * C, r] for a grad)."""
    got2, ref2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    fro, row = rel_fro_dev(got2, ref2), row_rel_err(got2, ref2)
    print(f"ERR {name} fro={fro:.3e} row={row:.3e}")
    assert fro < tol, (name, fro)
    assert row < tol, (name, row)


def segment_ref(x, W, A, B, s, gy):
    """float64 y, dX, dA, dB of y = x W^T + s (x A^T) B^T for one segment (W None: the adapter alone)."""
    x, A, B, gy = (t.double() for t in (x, A, B, gy))
    u = x @ A.T
    du = s * (gy @ B)
    y = s * (u @ B.T)
    dx = du @ A
    if W is not None:
        y = y + x @ W.T
        dx = dx + gy @ W
    return y, dx, du.T @ x, s * (gy.T @ u)


def moe_refs(m, x, gy, tpe, offs):
    T = x.shape[0]
    y = torch.zeros(T, m.ffn_dim, dtype=torch.float64, device=DEV)
    dx = torch.zeros(T, m.hidden_dim, dtype=torch.float64, device=DEV)
    dA = torch.zeros(m.lora_A.shape, dtype=torch.float64, device=DEV)
    dB = torch.zeros(m.lora_B.shape, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe, offs, T)):
        if hi > lo:
            W = dequant_f64(m.packed_weights[e], m.scales[e], m.zero_points[e])
            y[lo:hi], dx[lo:hi], dA[e], dB[e] = segment_ref(x[lo:hi], W, m.lora_A[e].detach(), m.lora_B[e].detach(),
                                                            m.scaling, gy[lo:hi])
    return y, dx, dA, dB


# ---- 1. vector width x layout x rank, through the modules --------------------------------------------------------

CASES = {            # (N, K, misalignment of x in floats): the widths of the N side / K side
    "N33_K130": (33, 130, 0),          # VEC 1 / 2
    "N1001_K256mis1": (1001, 256, 1),  # VEC 1 / 1
    "N1002_K256mis2": (1002, 256, 2),  # VEC 2 / 2
}


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_modules_vector_widths(case, r):
    N, K, mis = CASES[case]
    g = torch.Generator(device=DEV).manual_seed(r + N)
    torch.manual_seed(r + N)
    base = fq().QuantizedLinear.from_linear(torch.nn.Linear(K, N, bias=False))
    m = fq().LoRAQuantizedLinear.from_quantized(base, r, alpha=3 * r).to(DEV)
    with torch.no_grad():
        m.lora_B.normal_(0, 0.1, generator=g)
    x0 = torch.randn(77, K, device=DEV, generator=g)
    x = (misaligned(x0, mis) if mis else x0.clone()).requires_grad_()
    gy = torch.randn(77, N, device=DEV, generator=g)
    y = m(x)
    y.backward(gy)
    W = dequant_f64(m.packed_weights, m.scales, m.zero_points)
    ry, rdx, rdA, rdB = segment_ref(x0, W, m.lora_A.detach(), m.lora_B.detach(), m.scaling, gy)
    check(f"linear {case} r={r} y", y.detach(), ry, LAYER_TOL)
    check(f"linear {case} r={r} dX", x.grad, rdx, LAYER_TOL)
    check(f"linear {case} r={r} dA", m.lora_A.grad, rdA, ADAPTER_TOL)
    check(f"linear {case} r={r} dB", m.lora_B.grad, rdB, ADAPTER_TOL)

    E = 4
    mb = fq().MoEINT4.from_weights([torch.randn(N, K) * 0.05 for _ in range(E)])
    mm = fq().LoRAMoEINT4.from_quantized(mb, r, alpha=3 * r).to(DEV)
    with torch.no_grad():
        mm.lora_B.normal_(0, 0.1, generator=g)
    tpe, offs, T = expert_table([20, 0, 41, 9], gaps=[1, 0, 2, 0], tail=3)
    x0 = torch.randn(T, K, device=DEV, generator=g)
    x = (misaligned(x0, mis) if mis else x0.clone()).requires_grad_()
    gy = torch.randn(T, N, device=DEV, generator=g)
    y = mm(x, None, tpe, offs)
    y.backward(gy)
    ry, rdx, rdA, rdB = moe_refs(mm, x0, gy, tpe, offs)
    check(f"moe {case} r={r} y", y.detach(), ry, LAYER_TOL)
    check(f"moe {case} r={r} dX", x.grad, rdx, LAYER_TOL)
    check(f"moe {case} r={r} dA", mm.lora_A.grad, rdA, ADAPTER_TOL)
    check(f"moe {case} r={r} dB", mm.lora_B.grad, rdB, ADAPTER_TOL)


# ---- 2. the raw ops, both layouts: float64, and grouped == E = 1 per expert, bitwise, at VEC = 1 and 2 -------------

RAW = {              # (K, N, misalignment of X / G / outputs in floats)
    "K33_N1002": (33, 1002, 0),        # VEC 1 (K side) / 2 (N side)
    "K256mis1_N1001": (256, 1001, 1),  # VEC 1 / 1
    "K130_N256mis2": (130, 256, 2),    # VEC 2 / 2
}


def place(t, mis):
    """A fresh copy with the case's alignment: the per-expert calls then take the grouped call's vector width."""
    return misaligned(t, mis) if mis else t.clone()


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("case", list(RAW))
def test_raw_ops_layouts_and_per_expert_bits(case, r):
    K, N, mis = RAW[case]
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(50 + r + K)
    counts, gaps = [7, 0, 33, 1, 20, 64], [0, 2, 0, 5, 0, 1]
    tpe, offs, T = expert_table(counts, gaps, tail=3)
    E = len(counts)
    X = place(torch.randn(T, K, device=DEV, generator=g), mis)
    G = place(torch.randn(T, N, device=DEV, generator=g), mis)
    A = torch.randn(E, r, K, device=DEV, generator=g) * 0.1          # rc: [E, r, K]
    B = torch.randn(E, N, r, device=DEV, generator=g) * 0.1          # cr: [E, N, r]
    At, Bt = A.transpose(1, 2).contiguous(), B.transpose(1, 2).contiguous()
    s = 1.75
    U = o.lora_shrink(X, A, "rc", tpe, offs)
    assert torch.equal(U, o.lora_shrink(X, At, "cr", tpe, offs))      # (same FMA order in both layouts)
    dU = o.lora_shrink(G, B, "cr", tpe, offs, scale=s)
    dU_rc = o.lora_shrink(G, Bt, "rc", tpe, offs, scale=s)
    delta = o.lora_expand(U, B, "cr", tpe, offs, scale=s, out=place(torch.empty(T, N, device=DEV), mis))
    delta_rc = o.lora_expand(U, Bt, "rc", tpe, offs, scale=s, out=place(torch.empty(T, N, device=DEV), mis))
    dX = o.lora_expand(dU, A, "rc", tpe, offs, out=place(torch.empty(T, K, device=DEV), mis))
    dX_cr = o.lora_expand(dU, At, "cr", tpe, offs, out=place(torch.empty(T, K, device=DEV), mis))
    dA = o.lora_grad(X, dU, "rc", E, tpe, offs)
    dA_cr = o.lora_grad(X, dU, "cr", E, tpe, offs)
    dB = o.lora_grad(G, U, "cr", E, tpe, offs, scale=s)
    dB_rc = o.lora_grad(G, U, "rc", E, tpe, offs, scale=s)

    rU = torch.zeros(T, r, dtype=torch.float64, device=DEV)
    rdU, rdelta, rdX = torch.zeros_like(rU), torch.zeros(T, N, dtype=torch.float64, device=DEV), \
        torch.zeros(T, K, dtype=torch.float64, device=DEV)
    rdA, rdB = torch.zeros(E, r, K, dtype=torch.float64, device=DEV), torch.zeros(E, N, r, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe, offs, T)):
        Xe, Ge = X[lo:hi].double(), G[lo:hi].double()
        rU[lo:hi] = Xe @ A[e].double().T
        rdU[lo:hi] = s * Ge @ B[e].double()
        rdelta[lo:hi] = s * U[lo:hi].double() @ B[e].double().T
        rdX[lo:hi] = dU[lo:hi].double() @ A[e].double()
        rdA[e] = dU[lo:hi].double().T @ Xe
        rdB[e] = s * Ge.T @ U[lo:hi].double()
    for name, got, ref in (("U", U, rU), ("dU", dU, rdU), ("dU rc", dU_rc, rdU), ("delta", delta, rdelta),
                           ("delta rc", delta_rc, rdelta), ("dX", dX, rdX), ("dX cr", dX_cr, rdX),
                           ("dA", dA, rdA), ("dA cr", dA_cr, rdA.transpose(1, 2)), ("dB", dB, rdB),
                           ("dB rc", dB_rc, rdB.transpose(1, 2))):
        check(f"raw {case} r={r} {name}", got, ref, ADAPTER_TOL)

    for e, (lo, hi) in enumerate(clipped_ranges(tpe, offs, T)):
        c = hi - lo
        if c == 0:
            assert (dA[e] == 0).all() and (dB[e] == 0).all()
            continue
        Xe, Ge = place(X[lo:hi], mis), place(G[lo:hi], mis)
        Ue = o.lora_shrink(Xe, A[e], "rc")
        assert torch.equal(U[lo:hi], Ue), e
        dUe = o.lora_shrink(Ge, B[e], "cr", scale=s)
        assert torch.equal(dU[lo:hi], dUe), e
        assert torch.equal(dU_rc[lo:hi], o.lora_shrink(Ge, Bt[e], "rc", scale=s)), e
        assert torch.equal(delta[lo:hi], o.lora_expand(Ue, B[e], "cr", scale=s,
                                                       out=place(torch.empty(c, N, device=DEV), mis))), e
        assert torch.equal(delta_rc[lo:hi], o.lora_expand(Ue, Bt[e], "rc", scale=s,
                                                          out=place(torch.empty(c, N, device=DEV), mis))), e
        assert torch.equal(dX[lo:hi], o.lora_expand(dUe, A[e], "rc", out=place(torch.empty(c, K, device=DEV), mis))), e
        assert torch.equal(dX_cr[lo:hi], o.lora_expand(dUe, At[e], "cr",
                                                       out=place(torch.empty(c, K, device=DEV), mis))), e
        assert torch.equal(dA[e], o.lora_grad(Xe, dUe, "rc")[0]), e
        assert torch.equal(dA_cr[e], o.lora_grad(Xe, dUe, "cr")[0]), e
        assert torch.equal(dB[e], o.lora_grad(Ge, Ue, "cr", scale=s)[0]), e
        assert torch.equal(dB_rc[e], o.lora_grad(Ge, Ue, "rc", scale=s)[0]), e


# ---- 3. full size ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_size_base():
    """8 experts 4096 -> 11008 of quantised random weights."""
    E, K, N = 8, 4096, 11008
    g = torch.Generator(device=DEV).manual_seed(60)
    m = fq().MoEINT4(E, K, N).to(DEV)
    P, S, Z = [], [], []
    for _ in range(E):
        p, s, z = fq().quantize_weights(torch.randn(N, K, device=DEV, generator=g) * 0.02)
        P.append(p); S.append(s); Z.append(z)
    m.packed_weights, m.scales, m.zero_points = torch.stack(P), torch.stack(S), torch.stack(Z)
    return m


@pytest.mark.parametrize("r,counts", [
    (16, [128] * 8),
    (16, [485, 312, 126, 48, 30, 13, 6, 4]),
    (64, [64, 0, 20, 40, 16, 60, 50, 6]),
])
def test_full_size_moe_lora(full_size_base, r, counts):
    m = fq().LoRAMoEINT4.from_quantized(full_size_base, r, alpha=2 * r)
    g = torch.Generator(device=DEV).manual_seed(61 + r + counts[0])
    with torch.no_grad():
        m.lora_A.normal_(0, 4096 ** -0.5, generator=g)
        m.lora_B.normal_(0, 0.02, generator=g)
    tpe, offs, T = expert_table(counts)
    x = torch.randn(T, 4096, device=DEV, generator=g, requires_grad=True)
    gy = torch.randn(T, 11008, device=DEV, generator=g)
    y = m(x, None, tpe, offs)
    y.backward(gy)
    ry, rdx, rdA, rdB = moe_refs(m, x.detach(), gy, tpe, offs)
    name = f"full r={r} {'balanced' if counts[0] == 128 else 'skewed'}"
    check(f"{name} y", y.detach(), ry, LAYER_TOL)
    check(f"{name} dX", x.grad, rdx, LAYER_TOL)
    check(f"{name} dA", m.lora_A.grad, rdA, ADAPTER_TOL)
    check(f"{name} dB", m.lora_B.grad, rdB, ADAPTER_TOL)


# ---- 4. long segments: the grad kernel's 8-wave row split, its 4-row blocks and its tail loop -------------------------

def test_long_segments():
    K, N, r = 1000, 1002, 16
    g = torch.Generator(device=DEV).manual_seed(70)
    o = ops()
    for counts in ([4133, 17, 0, 301], None):
        if counts is None:                                   # E = 1, no table, 4096 rows
            tpe = offs = None
            T, E, segs = 4096, 1, [(0, 4096)]
        else:
            tpe, offs, T = expert_table(counts, gaps=[3, 0, 1, 5], tail=3)
            E, segs = len(counts), clipped_ranges(tpe, offs, T)
        X = torch.randn(T, K, device=DEV, generator=g)
        G = torch.randn(T, N, device=DEV, generator=g)
        U = torch.randn(T, r, device=DEV, generator=g)
        dU = torch.randn(T, r, device=DEV, generator=g)
        dA = o.lora_grad(X, dU, "rc", E, tpe, offs)
        dB = o.lora_grad(G, U, "cr", E, tpe, offs, scale=0.5)
        assert torch.equal(dA, o.lora_grad(X, dU, "rc", E, tpe, offs))
        assert torch.equal(dB, o.lora_grad(G, U, "cr", E, tpe, offs, scale=0.5))
        rdA = torch.zeros(E, r, K, dtype=torch.float64, device=DEV)
        rdB = torch.zeros(E, N, r, dtype=torch.float64, device=DEV)
        for e, (lo, hi) in enumerate(segs):
            rdA[e] = dU[lo:hi].double().T @ X[lo:hi].double()
            rdB[e] = 0.5 * G[lo:hi].double().T @ U[lo:hi].double()
        check(f"long {counts} dA", dA, rdA, ADAPTER_TOL)
        check(f"long {counts} dB", dB, rdB, ADAPTER_TOL)


# ---- 5. tables that leave [0, T), through the C ABI with guard rows ------------------------------------------------

def test_table_clipping_and_guard_rows():
    """All three kernels with a table whose ranges leave [0, T): results equal the clipped reference; the rows after T
    of every input hold NaN (never read: a read would poison the sums) and of every output a sentinel (never written)."""
    lib = fq()._native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    T, C, r, G, s = 60, 130, 16, 8, 1.25
    tpe = torch.tensor([8, 6, 10, 999, 5, 3], dtype=torch.int32, device=DEV)
    offs = torch.tensor([-4, 4, 12, 30, T + 3, 25], dtype=torch.int32, device=DEV)
    E = tpe.numel()
    g = torch.Generator(device=DEV).manual_seed(80)

    def guarded(cols, fill):
        t = torch.full((T + G, cols), fill, device=DEV)
        t[:T] = torch.randn(T, cols, device=DEV, generator=g)
        return t

    X, V, IN = guarded(C, float("nan")), guarded(r, float("nan")), guarded(C, float("nan"))
    A = torch.randn(E, r, C, device=DEV, generator=g) * 0.1              # rc
    B = torch.randn(E, C, r, device=DEV, generator=g) * 0.1              # cr
    out_s = torch.full((T + G, r), -7.5, device=DEV)
    out_e = torch.full((T + G, C), -7.5, device=DEV)
    D = torch.full((E, r, C), -7.5, device=DEV)
    assert lib.fql_lora_shrink_f32(X.data_ptr(), A.data_ptr(), 0, tpe.data_ptr(), offs.data_ptr(), out_s.data_ptr(),
                                   E, T, C, r, ctypes.c_float(s), stream) == 0
    assert lib.fql_lora_expand_f32(V.data_ptr(), B.data_ptr(), 1, tpe.data_ptr(), offs.data_ptr(), IN.data_ptr(),
                                   out_e.data_ptr(), E, T, C, r, ctypes.c_float(s), stream) == 0
    assert lib.fql_lora_grad_f32(X.data_ptr(), V.data_ptr(), tpe.data_ptr(), offs.data_ptr(), D.data_ptr(), 0, E, T,
                                 C, r, ctypes.c_float(s), stream) == 0
    torch.cuda.synchronize()
    rs = torch.zeros(T, r, dtype=torch.float64, device=DEV)
    re = IN[:T].double().clone()
    rD = torch.zeros(E, r, C, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe, offs, T)):
        rs[lo:hi] = s * X[lo:hi].double() @ A[e].double().T
        re[lo:hi] += s * V[lo:hi].double() @ B[e].double().T
        rD[e] = s * V[lo:hi].double().T @ X[lo:hi].double()
    check("clip shrink", out_s[:T], rs, ADAPTER_TOL)
    check("clip expand", out_e[:T], re, ADAPTER_TOL)
    check("clip grad", D, rD, ADAPTER_TOL)
    assert (out_s[T:] == -7.5).all() and (out_e[T:] == -7.5).all()
    assert (D[4] == 0).all()                                 # the expert wholly past T: zeros


# ---- 6. expand edge cases, at every vector width -----------------------------------------------------------------

@pytest.mark.parametrize("C", [33, 130, 256])
def test_expand_edge_cases(C):
    o = ops()
    r = 8
    g = torch.Generator(device=DEV).manual_seed(90 + C)
    tpe, offs, T = expert_table([9, 0, 30, 17], gaps=[2, 0, 1, 4], tail=3)
    E = tpe.numel()
    V = torch.randn(T, r, device=DEV, generator=g)
    W = torch.randn(E, C, r, device=DEV, generator=g)
    inp = torch.randn(T, C, device=DEV, generator=g)
    oop = o.lora_expand(V, W, "cr", tpe, offs, scale=1.5, input=inp)
    inplace = inp.clone()
    o.lora_expand(V, W, "cr", tpe, offs, scale=1.5, input=inplace, out=inplace)
    assert torch.equal(oop, inplace)
    ref = inp.double().clone()
    for e, (lo, hi) in enumerate(clipped_ranges(tpe, offs, T)):
        ref[lo:hi] += 1.5 * V[lo:hi].double() @ W[e].double().T
    check(f"expand C={C}", oop, ref, ADAPTER_TOL)
    fresh = o.lora_expand(V, W, "cr", tpe, offs, scale=1.5, out=torch.empty(T, C, device=DEV))
    assert torch.equal(fresh, o.lora_expand(V, W, "cr", tpe, offs, scale=1.5, input=torch.zeros(T, C, device=DEV)))
    assert torch.equal(o.lora_expand(V, W, "cr", tpe, offs, scale=0.0, input=inp), inp)
    neg = o.lora_expand(V, W, "cr", tpe, offs, scale=-1.5, out=torch.empty(T, C, device=DEV))
    assert torch.equal(neg, -fresh)
