"""Input / routing-weight gradients of the INT4 layers on the GPU (csrc/fql_bwd.h, fql_combine_bwd_f32) against float64
numpy oracles: dequantise in f64, then dY @ W."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import EXACT_REL_FRO, FAST_REL_FRO, FMA_REL_FRO, INT8_REL_FRO, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"default": EXACT_REL_FRO, "exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "int8": INT8_REL_FRO}


def fq():
    import fused_int4_amd
    return fused_int4_amd


def w64(packed, scales, zps):
    """f64 dequantisation [..., N, K] of per-row or per-group weights."""
    p = packed.cpu().numpy()
    q = np.empty(p.shape[:-1] + (2 * p.shape[-1],), np.float64)
    q[..., 0::2] = p & 15
    q[..., 1::2] = p >> 4
    s = scales.cpu().double().numpy()
    z = zps.cpu().double().numpy()
    if s.ndim == q.ndim:                                     # per group along K
        G = s.shape[-1]
        qg = q.reshape(q.shape[:-1] + (G, -1))
        return ((qg - z[..., None]) * s[..., None]).reshape(q.shape)
    return (q - z[..., None]) * s[..., None]


def quantized(N, K, seed=0, E=None):
    torch.manual_seed(seed)
    if E is None:
        return fq().quantize_weights(torch.randn(N, K))
    qs = [fq().quantize_weights(torch.randn(N, K) * 0.05) for _ in range(E)]
    return tuple(torch.stack([q[i] for q in qs]) for i in range(3))


@pytest.mark.parametrize("B", [1, 3, 64, 257])
@pytest.mark.parametrize("N,K", [(96, 64), (1000, 130), (4096, 4096), (96, 4096), (1000, 64)])
def test_linear_input_grad_exact(B, N, K):
    layer = fq().QuantizedLinear(K, N)
    packed, scales, zps = quantized(N, K, seed=B + N + K)
    layer.packed_weights, layer.scales, layer.zero_points = packed, scales, zps
    layer = layer.to(DEV)
    torch.manual_seed(1)
    x = torch.randn(B, K, device=DEV, requires_grad=True)
    gy = torch.randn(B, N)
    layer(x).backward(gy.to(DEV))
    ref = gy.double().numpy() @ w64(packed, scales, zps)
    assert rel_fro(x.grad.cpu().numpy(), ref) < EXACT_REL_FRO


@pytest.mark.parametrize("precision", ["fast", "int8", "exact"])
def test_linear_input_grad_precisions(precision):
    N, K, B = 1000, 4096, 64
    packed, scales, zps = quantized(N, K, seed=3)
    torch.manual_seed(2)
    x = torch.randn(B, K, device=DEV, requires_grad=True)
    gy = torch.randn(B, N)
    out = fq().ops.linear_forward(x, packed.to(DEV), scales.to(DEV), zps.to(DEV), precision=precision)
    out.backward(gy.to(DEV))
    ref = gy.double().numpy() @ w64(packed, scales, zps)
    assert rel_fro(x.grad.cpu().numpy(), ref) < TOL[precision]


def test_lora_adapter_gets_cpu_gradient():
    K, N, B, r = 256, 384, 48, 8
    torch.manual_seed(4)
    base = torch.nn.Linear(K, N, bias=False)
    q_cpu = fq().QuantizedLinear.from_linear(base)
    q_gpu = fq().QuantizedLinear.from_linear(base).to(DEV)
    lora = torch.nn.Linear(K, K, bias=False)
    lora_gpu = torch.nn.Linear(K, K, bias=False).to(DEV)
    lora_gpu.load_state_dict(lora.state_dict())
    x = torch.randn(B, K)
    q_cpu(x + lora(x)).square().sum().backward()
    q_gpu(x.to(DEV) + lora_gpu(x.to(DEV))).square().sum().backward()
    assert lora_gpu.weight.grad is not None
    assert rel_fro(lora_gpu.weight.grad.cpu().numpy(), lora.weight.grad.numpy()) < 1e-5


def test_integer_data_bit_exact():
    """Integer dY, power-of-two scales, integral zero points: the result is an exact integer combination, so it must
    match int64 arithmetic bit for bit (this also pins the transposed-read lane mapping)."""
    rng = np.random.default_rng(5)
    for (B, N, K) in [(64, 1000, 4096), (33, 257, 130), (3, 96, 64)]:
        q = rng.integers(0, 16, size=(N, K))
        z = rng.integers(0, 16, size=N).astype(np.float32)
        s = (2.0 ** rng.integers(-3, 2, size=N)).astype(np.float32)
        gy = rng.integers(-15, 16, size=(B, N)).astype(np.float32)
        packed = torch.from_numpy((q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8))
        got = fq().ops.linear_backward_input(torch.from_numpy(gy).to(DEV), packed.to(DEV), torch.from_numpy(s).to(DEV),
                                             torch.from_numpy(z).to(DEV)).cpu().numpy()
        # exact in int64 units of 2^-3
        ref = (gy.astype(np.int64) * (s * 8).astype(np.int64)[None, :]) @ (q - z.astype(np.int64)[:, None])
        assert np.array_equal(got, (ref / 8.0).astype(np.float32)), (B, N, K)


def test_non_integer_zero_points_and_heavy_tails():
    N, K, B = 1000, 512, 64
    packed, scales, zps = quantized(N, K, seed=6)
    zps = zps + torch.linspace(-0.4, 0.4, N)                 # fractional zero points
    torch.manual_seed(7)
    gy = torch.randn(B, N)
    gy[:, 17] *= 3e4                                         # outlier columns: heavy-tailed gradient rows
    gy[::3, 500] *= -1e5
    got = fq().ops.linear_backward_input(gy.to(DEV), packed.to(DEV), scales.to(DEV), zps.to(DEV)).cpu().numpy()
    ref = gy.double().numpy() @ w64(packed, scales, zps)
    assert rel_fro(got, ref) < EXACT_REL_FRO


def _table(counts):
    tpe = torch.tensor(counts, dtype=torch.int32)
    offs = torch.cumsum(tpe, 0, dtype=torch.int32) - tpe
    return tpe, offs


@pytest.mark.parametrize("counts,uncovered", [([40, 0, 33, 200, 1], 5), ([7] * 70, 0), ([0, 0, 130], 3)])
def test_grouped_backward(counts, uncovered):
    E, N, K = len(counts), 160, 192
    P, S, Z = quantized(N, K, seed=E, E=E)
    tpe, offs = _table(counts)
    T = int(tpe.sum()) + uncovered
    torch.manual_seed(8)
    gy = torch.randn(T, N)
    args = (P.to(DEV), S.to(DEV), Z.to(DEV), gy.to(DEV), tpe.to(DEV), offs.to(DEV))
    got = fq().ops.moe_backward_input(*args)
    again = fq().ops.moe_backward_input(*args)
    assert torch.equal(got, again)                           # deterministic
    got = got.cpu()
    W = w64(P, S, Z)
    assert (got[T - uncovered:] == 0).all()
    for e in range(E):
        lo, c = int(offs[e]), int(tpe[e])
        if c == 0:
            continue
        ref = gy[lo:lo + c].double().numpy() @ W[e]
        assert rel_fro(got[lo:lo + c].numpy(), ref) < EXACT_REL_FRO
        lin = fq().ops.linear_backward_input(gy[lo:lo + c].to(DEV), P[e].to(DEV), S[e].to(DEV), Z[e].to(DEV)).cpu()
        assert torch.equal(got[lo:lo + c], lin), e           # bitwise equal to the linear backward on that expert


def test_moe_modules_backward():
    E, N, K = 4, 256, 128
    P, S, Z = quantized(N, K, seed=9, E=E)
    m = fq().MoEINT4(E, K, N)
    m.packed_weights, m.scales, m.zero_points = P, S, Z
    m = m.to(DEV)
    tpe, offs = _table([10, 0, 50, 4])
    x = torch.randn(64, K, device=DEV, requires_grad=True)
    gy = torch.randn(64, N)
    m(x, None, tpe.to(DEV), offs.to(DEV)).backward(gy.to(DEV))
    W = w64(P, S, Z)
    ref = np.zeros((64, K))
    for e, (lo, c) in enumerate(zip(offs.tolist(), tpe.tolist())):
        ref[lo:lo + c] = gy[lo:lo + c].double().numpy() @ W[e]
    assert rel_fro(x.grad.cpu().numpy(), ref) < EXACT_REL_FRO

    torch.manual_seed(10)
    ws = [torch.randn(N, K) * 0.05 for _ in range(E)]
    qm = fq().QuantizedMoE.from_fp16_weights([w.half() for w in ws]).to(DEV)
    for dtypes in ([torch.float16] * E, [torch.float32, torch.bfloat16, torch.float16, torch.float32]):
        xs = [torch.randn(c, K, device=DEV, dtype=dt, requires_grad=True) for c, dt in zip([5, 0, 40, 9], dtypes)]
        outs = qm(xs)
        sum(o.float().sum() for o in outs).backward()
        for x, e in zip(xs, range(E)):
            if x.shape[0] == 0:
                continue
            Wq = w64(*[getattr(qm.experts[e], n) for n in ("packed_weights", "scales", "zero_points")])
            ref = np.ones((x.shape[0], N)) @ Wq
            assert rel_fro(x.grad.float().cpu().numpy(), ref) < 1e-2     # (16-bit inputs and gradients)


@pytest.mark.parametrize("top_k", [1, 2, 8])
def test_combine_backward(top_k):
    from fused_int4_amd import routing
    T, N, E = 50, 300, 16
    torch.manual_seed(11 + top_k)
    idx = torch.stack([torch.randperm(E)[:top_k] for _ in range(T)]).to(DEV)
    perm = torch.argsort(idx.reshape(-1), stable=True)
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(perm.numel(), device=DEV)
    y = torch.randn(T * top_k, N, device=DEV, requires_grad=True)
    w = torch.rand(T, top_k, device=DEV, requires_grad=True)
    go = torch.randn(T, N, device=DEV)
    routing.combine_grouped(y, w, inverse, top_k).backward(go)
    for dt in (torch.float32, torch.float64):          # torch's formulation, in float32 and as the float64 oracle
        y2 = y.detach().to(dt).requires_grad_()
        w2 = w.detach().to(dt).requires_grad_()
        ref = (y2.index_select(0, inverse).view(T, top_k, N) * w2.unsqueeze(-1)).sum(1)
        ref.backward(go.to(dt))
        assert (y.grad.to(dt) - y2.grad).abs().max().item() <= 1e-6 * y2.grad.abs().max().item()
        assert (w.grad.to(dt) - w2.grad).abs().max().item() <= 1e-6 * w2.grad.abs().max().item()


def test_gated_ffn_backward():
    E, H, F = 3, 128, 192
    torch.manual_seed(12)
    gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
    up = [torch.randn(F, H) * 0.1 for _ in range(E)]
    down = [torch.randn(H, F) * 0.1 for _ in range(E)]
    m = fq().QuantizedMoEFFN.from_weights(gate, up, down).to(DEV)
    tpe, offs = _table([20, 0, 30])
    x = torch.randn(50, H, dtype=torch.float64)
    gy = torch.randn(50, H, dtype=torch.float64)
    xg = x.float().to(DEV).requires_grad_()
    m(xg, tpe.to(DEV), offs.to(DEV)).backward(gy.float().to(DEV))
    Wgu = torch.from_numpy(w64(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points))
    Wd = torch.from_numpy(w64(m.down_packed, m.down_scales, m.down_zero_points))
    ref = torch.zeros(50, H, dtype=torch.float64)
    for e, (lo, c) in enumerate(zip(offs.tolist(), tpe.tolist())):
        if c == 0:
            continue
        xe = x[lo:lo + c].clone().requires_grad_()
        gu = xe @ Wgu[e].T
        h = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
        (h @ Wd[e].T).backward(gy[lo:lo + c])
        ref[lo:lo + c] = xe.grad
    assert rel_fro(xg.grad.cpu().numpy(), ref.numpy()) < 2e-5


def test_per_group_linear_backward():
    N, K, B = 300, 256, 40
    torch.manual_seed(13)
    lin = torch.nn.Linear(K, N, bias=False)
    layer = fq().QuantizedLinear.from_linear(lin, group_size=64).to(DEV)
    x = torch.randn(B, K, device=DEV, requires_grad=True)
    gy = torch.randn(B, N)
    layer(x).backward(gy.to(DEV))
    ref = gy.double().numpy() @ w64(layer.packed_weights, layer.scales, layer.zero_points)
    assert rel_fro(x.grad.cpu().numpy(), ref) < FMA_REL_FRO


def _same_under_grad(fn, *args):
    with torch.no_grad():
        a = fn(*args)
    b = fn(*[t.clone().requires_grad_() if torch.is_tensor(t) and t.is_floating_point() and t.dim() == 2 and i == 0
             else t for i, t in enumerate(args)])
    assert b.grad_fn is not None
    assert torch.equal(a, b.detach())


def test_forward_bitwise_unchanged_under_grad():
    N, K = 1000, 512
    ops = fq().ops
    packed, scales, zps = [t.to(DEV) for t in quantized(N, K, seed=14)]
    for B in (2, 64):
        x = torch.randn(B, K, device=DEV)
        _same_under_grad(lambda x_: ops.linear_forward(x_, packed, scales, zps), x)
        _same_under_grad(lambda x_: ops.linear_forward_any(x_, packed, scales, zps), x.bfloat16())
    P, S, Z = [t.to(DEV) for t in quantized(N, K, seed=15, E=3)]
    tpe, offs = _table([30, 0, 50])
    tpe, offs = tpe.to(DEV), offs.to(DEV)
    x = torch.randn(80, K, device=DEV)
    _same_under_grad(lambda x_: ops.moe_forward(P, S, Z, x_, None, tpe, offs), x)
    _same_under_grad(lambda x_: ops.moe_forward_any(P, S, Z, x_, None, tpe, offs), x.half())
    y = torch.randn(40 * 2, N, device=DEV)
    pos = torch.randperm(80, device=DEV).to(torch.int32)
    w = torch.rand(40, 2, device=DEV)
    _same_under_grad(lambda y_: ops.combine(y_, pos, w), y)


def test_forward_only_ops_refuse_grad():
    """The GPU ops without a backward, and the expert-parallel path built on them, raise instead of cutting the graph."""
    from fused_int4_amd.ep import ExpertParallelMoE
    E, N, K = 4, 64, 64
    P, S, Z = [t.to(DEV) for t in quantized(N, K, seed=18, E=E)]
    x = torch.randn(16, K, device=DEV)
    idx = torch.randint(0, E, (16, 2), device=DEV)
    w = torch.rand(16, 2, device=DEV)
    ep = ExpertParallelMoE(E, P, S, Z)
    for xi, wi in ((x.clone().requires_grad_(), w), (x, w.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="no backward"):
            ep(xi, idx, wi)
    with torch.no_grad():
        assert ep(x.clone().requires_grad_(), idx, w).shape == (16, N)
    tpe, offs = _table([4, 4, 4, 4])
    rows = torch.arange(16, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="no backward"):
        fq().ops.moe_gather_forward(P, S, Z, x.clone().requires_grad_(), rows, tpe.to(DEV), offs.to(DEV))


def test_adjoint_identity():
    N = K = 4096
    packed, scales, zps = quantized(N, K, seed=15)
    torch.manual_seed(16)
    x = torch.randn(1, K, dtype=torch.float64)
    y = torch.randn(64, N)
    W = w64(packed, scales, zps)
    wx = W @ x.numpy()[0]
    wty = fq().ops.linear_backward_input(y.to(DEV), packed.to(DEV), scales.to(DEV), zps.to(DEV)).double().cpu().numpy()
    lhs = y.double().numpy() @ wx
    rhs = wty @ x.numpy()[0]
    assert np.allclose(lhs, rhs, rtol=1e-5, atol=1e-5 * np.abs(lhs).max())


def test_moe_backward_memory():
    E, K, N, T = 8, 4096, 11008, 1024
    g = torch.Generator(device=DEV).manual_seed(17)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    S = torch.rand(E, N, device=DEV, generator=g) * 0.01
    Z = torch.full((E, N), 8.0, device=DEV)
    tpe, offs = _table([T // E] * E)
    x = torch.randn(T, K, device=DEV, requires_grad=True)
    out = fq().ops.moe_forward(P, S, Z, x, None, tpe.to(DEV), offs.to(DEV))
    gy = torch.randn_like(out)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.backward(gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    # the fused backward holds its limb workspace and grad_in, nothing else of size: one expert's float32 weights alone
    # (N * K * 4 = 180 MB) would break both bounds
    ws = fq()._native.lib().fql_moe_bwd_workspace_bytes(E, T, K, N, 0)
    assert peak <= ws + T * K * 4 + (8 << 20), (peak, ws)
    assert peak < E * N * K * 4 / 8, peak
