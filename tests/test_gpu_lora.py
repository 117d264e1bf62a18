"""Low-rank adapters on the INT4 layers on the GPU (csrc/fql_lora.h, ops.linear_lora_forward / moe_lora_forward) against
float64 torch on the dequantised weights, plus the bitwise promises of include/fql_int4.h."""
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import EXACT_REL_FRO, FAST_REL_FRO, rel_fro, tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANKS = [4, 8, 16, 32, 64]


def fq():
    import fused_int4_amd
    return fused_int4_amd


def ops():
    from fused_int4_amd import ops as o
    return o


def w64(packed, scales, zps):
    return fq().dequantize_weights(packed.cpu(), scales.cpu(), zps.cpu()).double()


def linear_ref(x, W, A, B, s, gy, bias=None):
    """float64 forward and gradients of y = x W^T (+ b) + s (x A^T) B^T."""
    x64, A64, B64 = (t.detach().cpu().double().requires_grad_() for t in (x, A, B))
    y = x64 @ W.t() + s * (x64 @ A64.t()) @ B64.t()
    if bias is not None:
        y = y + bias.detach().cpu().double()
    y.backward(gy.cpu().double())
    return y.detach(), x64.grad, A64.grad, B64.grad


def lora_layer(N, K, r, seed, bias=False, group_size=None, precision="default", alpha=None):
    torch.manual_seed(seed)
    base = fq().QuantizedLinear.from_linear(torch.nn.Linear(K, N, bias=bias), precision=precision,
                                            group_size=group_size)
    m = fq().LoRAQuantizedLinear.from_quantized(base, r, alpha)
    with torch.no_grad():
        m.lora_B.normal_(0, 0.1)
    return m.to(DEV)


def check_linear(m, B, K, base_tol, seed=1):
    torch.manual_seed(seed)
    x = torch.randn(B, K, device=DEV, requires_grad=True)
    gy = torch.randn(B, m.out_features, device=DEV)
    y = m(x)
    y.backward(gy)
    W = w64(m.packed_weights, m.scales, m.zero_points)
    y64, gx64, gA64, gB64 = linear_ref(x, W, m.lora_A, m.lora_B, m.scaling, gy, m.bias)
    t = tol(base_tol)
    assert rel_fro(y.detach().cpu().numpy(), y64.numpy()) < t
    assert rel_fro(x.grad.cpu().numpy(), gx64.numpy()) < t
    assert rel_fro(m.lora_A.grad.cpu().numpy(), gA64.numpy()) < t
    assert rel_fro(m.lora_B.grad.cpu().numpy(), gB64.numpy()) < t


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("N,K", [(96, 64), (1000, 130), (4096, 4096)])
def test_linear_lora(r, B, N, K):
    check_linear(lora_layer(N, K, r, seed=N + K + r, alpha=2 * r), B, K, EXACT_REL_FRO)


def test_linear_lora_fast_base():
    check_linear(lora_layer(1000, 512, 16, seed=5, precision="fast"), 64, 512, FAST_REL_FRO)


def test_linear_lora_per_group_base():
    check_linear(lora_layer(384, 256, 8, seed=6, group_size=64), 48, 256, EXACT_REL_FRO)


def test_linear_lora_1d_input():
    m = lora_layer(96, 64, 4, seed=7)
    x = torch.randn(64, device=DEV)
    assert torch.equal(m(x), m(x.unsqueeze(0))[0])


def test_bias_gradient():
    m = lora_layer(200, 128, 8, seed=8, bias=True)
    m.bias.requires_grad_(True)
    x = torch.randn(33, 128, device=DEV, requires_grad=True)
    gy = torch.randn(33, 200, device=DEV)
    m(x).backward(gy)
    assert m.bias.grad is not None
    assert rel_fro(m.bias.grad.cpu().numpy(), gy.sum(0).cpu().double().numpy()) < 1e-6


# ---- grouped ------------------------------------------------------------------------------------------------------

def table(counts, gaps=None, seed=0):
    """Ragged expert table with optional uncovered rows between / after the ranges: (tpe, offs, T, covered mask)."""
    offs, pos = [], 0
    gaps = gaps or [0] * len(counts)
    for c, g in zip(counts, gaps):
        pos += g
        offs.append(pos)
        pos += c
    T = pos + 3                                                  # 3 trailing rows no expert covers
    covered = torch.zeros(T, dtype=torch.bool)
    for o, c in zip(offs, counts):
        covered[o:o + c] = True
    return (torch.tensor(counts, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32), T, covered)


def moe_layer(E, N, K, r, seed):
    torch.manual_seed(seed)
    base = fq().MoEINT4.from_weights([torch.randn(N, K) * 0.05 for _ in range(E)])
    m = fq().LoRAMoEINT4.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        m.lora_B.normal_(0, 0.1)
    return m.to(DEV)


def moe_ref(m, x, tpe, offs, gy):
    W = torch.stack([w64(m.packed_weights[e], m.scales[e], m.zero_points[e]) for e in range(m.num_experts)])
    x64, A64, B64 = (t.detach().cpu().double().requires_grad_() for t in (x, m.lora_A, m.lora_B))
    rows = []
    y = torch.zeros(x.shape[0], m.ffn_dim, dtype=torch.float64)
    for e in range(m.num_experts):
        o, c = int(offs[e]), int(tpe[e])
        if c:
            xe = x64[o:o + c]
            rows.append((o, c, xe @ W[e].t() + m.scaling * (xe @ A64[e].t()) @ B64[e].t()))
    for o, c, ye in rows:
        y = y.index_put((torch.arange(o, o + c),), ye)
    y.backward(gy.cpu().double())
    return y.detach(), x64.grad, A64.grad, B64.grad


GROUPED = [
    (5, 96, 64, [7, 0, 33, 1, 20], [0, 2, 0, 5, 0]),
    (8, 1000, 256, [128, 0, 64, 3, 200, 17, 0, 90], None),
]


def check_moe(m, counts, gaps, seed=2):
    tpe, offs, T, covered = table(counts, gaps)
    torch.manual_seed(seed)
    x = torch.randn(T, m.hidden_dim, device=DEV, requires_grad=True)
    gy = torch.randn(T, m.ffn_dim, device=DEV)
    y = m(x, None, tpe.to(DEV), offs.to(DEV))
    y.backward(gy)
    y64, gx64, gA64, gB64 = moe_ref(m, x, tpe, offs, gy)
    t = tol(EXACT_REL_FRO)
    assert rel_fro(y.detach().cpu().numpy(), y64.numpy()) < t
    assert rel_fro(x.grad.cpu().numpy(), gx64.numpy()) < t
    assert rel_fro(m.lora_A.grad.cpu().numpy(), gA64.numpy()) < t
    assert rel_fro(m.lora_B.grad.cpu().numpy(), gB64.numpy()) < t
    unc = ~covered
    assert (y.detach().cpu()[unc] == 0).all() and (x.grad.cpu()[unc] == 0).all()
    for e, c in enumerate(counts):
        if c == 0:
            assert (m.lora_A.grad[e] == 0).all() and (m.lora_B.grad[e] == 0).all()


@pytest.mark.parametrize("r", RANKS)
def test_moe_lora_ranks(r):
    E, N, K, counts, gaps = GROUPED[0]
    check_moe(moe_layer(E, N, K, r, seed=r), counts, gaps)


@pytest.mark.parametrize("E,N,K,counts,gaps", GROUPED[1:])
def test_moe_lora_shapes(E, N, K, counts, gaps):
    check_moe(moe_layer(E, N, K, 16, seed=E), counts, gaps)


def test_moe_lora_130_experts():
    g = torch.Generator().manual_seed(3)
    counts = torch.randint(0, 5, (130,), generator=g).tolist()
    gaps = torch.randint(0, 2, (130,), generator=g).tolist()
    check_moe(moe_layer(130, 64, 130, 8, seed=9), counts, gaps)


def test_moe_lora_fast_base():
    E, N, K, counts, gaps = GROUPED[0]
    m = moe_layer(E, N, K, 16, seed=11)
    m.precision = "fast"
    tpe, offs, T, _ = table(counts, gaps)
    x = torch.randn(T, K, device=DEV, requires_grad=True)
    gy = torch.randn(T, N, device=DEV)
    y = m(x, None, tpe.to(DEV), offs.to(DEV))
    y.backward(gy)
    y64, gx64, gA64, gB64 = moe_ref(m, x, tpe, offs, gy)
    assert rel_fro(y.detach().cpu().numpy(), y64.numpy()) < tol(FAST_REL_FRO)
    assert rel_fro(x.grad.cpu().numpy(), gx64.numpy()) < tol(FAST_REL_FRO)
    assert rel_fro(m.lora_B.grad.cpu().numpy(), gB64.numpy()) < tol(FAST_REL_FRO)


# ---- bitwise ------------------------------------------------------------------------------------------------------

def run_moe(m, x, tpe, offs, gy):
    for p in m.parameters():
        p.grad = None
    xx = x.detach().clone().requires_grad_()
    y = m(xx, None, tpe, offs)
    y.backward(gy)
    return y.detach(), xx.grad, m.lora_A.grad.clone(), m.lora_B.grad.clone()


def test_two_runs_are_bitwise_equal():
    E, N, K, counts, gaps = GROUPED[1]
    m = moe_layer(E, N, K, 16, seed=12)
    tpe, offs, T, _ = table(counts, gaps)
    x = torch.randn(T, K, device=DEV)
    gy = torch.randn(T, N, device=DEV)
    a = run_moe(m, x, tpe.to(DEV), offs.to(DEV), gy)
    b = run_moe(m, x, tpe.to(DEV), offs.to(DEV), gy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("K,N", [(130, 96), (256, 1000)])
def test_grouped_equals_per_expert(r, K, N):
    """Adapter terms of the grouped call == the E = 1 call on each expert's rows, bit for bit."""
    o = ops()
    counts, gaps = [7, 0, 33, 1, 20, 64], [0, 2, 0, 5, 0, 1]
    tpe, offs, T, _ = table(counts, gaps)
    E = len(counts)
    torch.manual_seed(r + K)
    X = torch.randn(T, K, device=DEV)
    G = torch.randn(T, N, device=DEV)
    A = torch.randn(E, r, K, device=DEV) * 0.1
    B = torch.randn(E, N, r, device=DEV) * 0.1
    t, f = tpe.to(DEV), offs.to(DEV)
    U = o.lora_shrink(X, A, "rc", t, f)
    delta = o.lora_expand(U, B, "cr", t, f, scale=2.0, out=torch.empty(T, N, device=DEV))
    dU = o.lora_shrink(G, B, "cr", t, f, scale=2.0)
    dX = o.lora_expand(dU, A, "rc", t, f, out=torch.empty(T, K, device=DEV))
    dA = o.lora_grad(X, dU, "rc", E, t, f)
    dB = o.lora_grad(G, U, "cr", E, t, f, scale=2.0)
    for e in range(E):
        lo, c = int(offs[e]), int(tpe[e])
        if c == 0:
            assert (dA[e] == 0).all() and (dB[e] == 0).all()
            continue
        Xe, Ge = X[lo:lo + c].contiguous(), G[lo:lo + c].contiguous()
        Ue = o.lora_shrink(Xe, A[e], "rc")
        assert torch.equal(U[lo:lo + c], Ue)
        assert torch.equal(delta[lo:lo + c], o.lora_expand(Ue, B[e], "cr", scale=2.0, out=torch.empty(c, N, device=DEV)))
        dUe = o.lora_shrink(Ge, B[e], "cr", scale=2.0)
        assert torch.equal(dU[lo:lo + c], dUe)
        assert torch.equal(dX[lo:lo + c], o.lora_expand(dUe, A[e], "rc", out=torch.empty(c, K, device=DEV)))
        assert torch.equal(dA[e], o.lora_grad(Xe, dUe, "rc")[0])
        assert torch.equal(dB[e], o.lora_grad(Ge, Ue, "cr", scale=2.0)[0])


def test_zero_B_equals_base_bitwise():
    torch.manual_seed(13)
    base = fq().QuantizedLinear.from_linear(torch.nn.Linear(130, 1000, bias=True)).to(DEV)
    m = fq().LoRAQuantizedLinear.from_quantized(base, 16)
    x = torch.randn(64, 130, device=DEV)
    with torch.no_grad():
        assert torch.equal(m(x), base(x))
    xg = x.clone().requires_grad_()
    xb = x.clone().requires_grad_()
    ym, yb = m(xg), base(xb)
    assert torch.equal(ym.detach(), yb.detach())
    gy = torch.randn_like(ym)
    ym.backward(gy)
    yb.backward(gy)
    assert torch.equal(xg.grad, xb.grad)

    E, N, K, counts, gaps = GROUPED[0]
    torch.manual_seed(14)
    moe_base = fq().MoEINT4.from_weights([torch.randn(N, K) * 0.05 for _ in range(E)]).to(DEV)
    moe = fq().LoRAMoEINT4.from_quantized(moe_base, 8)
    tpe, offs, T, _ = table(counts, gaps)
    t, f = tpe.to(DEV), offs.to(DEV)
    x = torch.randn(T, K, device=DEV)
    with torch.no_grad():
        assert torch.equal(moe(x, None, t, f), moe_base(x, None, t, f))
    xg = x.clone().requires_grad_()
    xb = x.clone().requires_grad_()
    ym, yb = moe(xg, None, t, f), moe_base(xb, None, t, f)
    assert torch.equal(ym.detach(), yb.detach())


def test_no_grad_saves_nothing():
    m = lora_layer(96, 64, 4, seed=15)
    with torch.no_grad():
        y = m(torch.randn(8, 64, device=DEV))
    assert y.grad_fn is None


def test_moe_lora_graph_capture_replays_same_bits():
    E, N, K, counts, gaps = GROUPED[1]
    m = moe_layer(E, N, K, 16, seed=16)
    tpe, offs, T, _ = table(counts, gaps)
    t, f = tpe.to(DEV), offs.to(DEV)
    x = torch.randn(T, K, device=DEV)
    with torch.no_grad():
        eager = m(x, None, t, f)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m(x, None, t, f)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(x, None, t, f)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_training_learns_a_planted_delta():
    """teacher = base + s B* A* per expert; AdamW on the adapters alone brings the loss down >= 10x in 100 steps."""
    torch.manual_seed(17)
    E, K, N, r = 4, 128, 64, 8
    base = fq().MoEINT4.from_weights([torch.randn(N, K) * 0.05 for _ in range(E)]).to(DEV)
    student = fq().LoRAMoEINT4.from_quantized(base, r, alpha=2 * r)
    teacher = fq().LoRAMoEINT4.from_quantized(base, r, alpha=2 * r)
    with torch.no_grad():
        teacher.lora_A.copy_(torch.randn(E, r, K) / K ** 0.5)
        teacher.lora_B.copy_(torch.randn(E, N, r) / r ** 0.5)
    counts = torch.tensor([64, 64, 64, 64], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, 64, 128, 192], dtype=torch.int32, device=DEV)
    x = torch.randn(256, K, device=DEV)
    with torch.no_grad():
        target = teacher(x, None, counts, offs)
    opt = torch.optim.AdamW(student.parameters(), lr=1e-2, weight_decay=0.0)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        loss = (student(x, None, counts, offs) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[0] / losses[-1] >= 10, (losses[0], losses[-1])
    assert torch.equal(student.packed_weights, base.packed_weights)
