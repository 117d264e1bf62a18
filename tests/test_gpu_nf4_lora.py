"""The adapter stage of the two NF4 tile kernels on the GPU (csrc/fql_gemm_lut4.h, csrc/fql_gemm_lut4_bwd.h; DESIGN.md section
46), at tests/test_gpu_nf4.py's shapes and every rank: rank 4 is the partial step, 32 the full pair of images, 64 the second
pair; T = 257 is the second row tile with one live row.  References are float64, built from W by the definition."""
import pytest
import torch

from test_gpu_nf4 import DEV, DTYPES, KB, NS, TS, U, _both, _rows, _weights, fq

pytestmark = pytest.mark.gpu
TM = max(TS)
SHAPES = lambda f: pytest.mark.parametrize("dt", DTYPES)(pytest.mark.parametrize("N", NS)(pytest.mark.parametrize("K,block", KB)(f)))


def _adapters(K, N, r, exact, seed):
    """(v [TM, r], B [N, r], dv [TM, r], A [r, K]) float32: integers, or Gaussians that size the adapter term like the base term."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return ri(-4, 4, TM, r), ri(-2, 2, N, r), ri(-4, 4, TM, r), ri(-2, 2, r, K)
    rn = lambda *s: torch.randn(*s, generator=g)
    return rn(TM, r), rn(N, r) * 0.05 * (K / r) ** 0.5, rn(TM, r), rn(r, K) * 0.05 * (N / r) ** 0.5


def _fused(codes, absmax, book, block, x, v, B, gy, dv, A, bias, dt):
    """(out, dx) of the two fused ops on the GPU, as CPU tensors."""
    ops, d = fq().ops, lambda t: None if t is None else t.to(DEV)
    out = ops.linear_forward_lut4_lora(d(codes), d(absmax), d(x.to(dt)), d(v), d(B), d(book), block, bias=d(bias))
    dx = ops.linear_backward_input_lut4_lora(d(codes), d(absmax), d(gy.to(dt)), d(dv), d(A), d(book), block, out_dtype=dt)
    return out.cpu(), dx.cpu()


@SHAPES
def test_exact_integers_bit_for_bit(K, block, N, dt):
    codes, absmax, book, W = _weights(K, block, N, True, 1)
    x, gy, bias = _rows(TM, K, True, 2), _rows(TM, N, True, 3), torch.arange(N, dtype=torch.float32) - 3
    for r in fq().ops.LORA_RANKS:
        v, B, dv, A = (t.double() for t in _adapters(K, N, r, True, 20 + r))
        ref, dref = x.double() @ W.T + v @ B.T + bias.double(), gy.double() @ W + dv @ A
        mags = x.double().abs() @ W.abs().T + v.abs() @ B.abs().T + bias.abs(), gy.double().abs() @ W.abs() + dv.abs() @ A.abs()
        for rr, m in zip((ref, dref), mags):                   # multiples of 2^-2 whose absolute sum stays far below 2^24
            assert bool((rr * 4 == (rr * 4).round()).all()) and float(m.max()) * 4 < 2 ** 24
        for T in TS:
            out, dx = _fused(codes, absmax, book, block, x[:T], v[:T].float(), B.float(), gy[:T], dv[:T].float(), A.float(), bias, dt)
            assert torch.equal(out, ref[:T].float().to(dt)), (r, T, "forward")   # (the exact value, rounded once)
            assert torch.equal(dx, dref[:T].float().to(dt)), (r, T, "input gradient")


@SHAPES
def test_gaussian_zero_matrix_is_the_base_op_and_the_float32_bound(K, block, N, dt):
    """B = 0 / A = 0: the base ops' bits.  Otherwise |got - ref| <= L 2^-23 sum |products| (a float32 sum of L exact terms in any
    order), L = K + r + 1 forward (the bias), N + r input gradient; + 2^-8 |ref| for bfloat16.  ref: float64 on the rounded operands."""
    codes, absmax, _, W = _weights(K, block, N, False, 8)
    b16 = lambda t: t.bfloat16().double()
    x, gy, bias = b16(_rows(TM, K, False, 9)), b16(_rows(TM, N, False, 10)), torch.randn(N, generator=torch.Generator().manual_seed(11))
    base = {T: _both(codes, absmax, None, block, x[:T].float(), gy[:T].float(), bias, dt) for T in TS}
    worst = 0.0
    for r in fq().ops.LORA_RANKS:
        v, B, dv, A = _adapters(K, N, r, False, 40 + r)
        ref, dref = x @ W.T + b16(v) @ b16(B).T + bias.double(), gy @ W + b16(dv) @ b16(A)
        bound = (K + r + 1) * U * (x.abs() @ W.abs().T + b16(v).abs() @ b16(B).abs().T + bias.double().abs())
        dbound = (N + r) * U * (gy.abs() @ W.abs() + b16(dv).abs() @ b16(A).abs())
        if dt == torch.bfloat16:
            bound, dbound = bound + 2.0 ** -8 * ref.abs(), dbound + 2.0 ** -8 * dref.abs()
        for T in TS:
            run = lambda B, A: _fused(codes, absmax, None, block, x[:T].float(), v[:T], B, gy[:T].float(), dv[:T], A, bias, dt)
            zero = run(B * 0, A * 0)
            assert torch.equal(zero[0], base[T][0]) and torch.equal(zero[1], base[T][1]), (r, T)
            for got, rr, b in zip(run(B, A), (ref[:T], dref[:T]), (bound[:T], dbound[:T])):
                ratio = float(((got.double() - rr).abs() / b.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert bool(((got.double() - rr).abs() <= b).all()), (r, T, ratio)
    print(f"K={K} N={N} {dt}: largest |err| / bound = {worst:.4f}")


def test_non_finite_shrunk_rows_and_rerun():
    K, block, N, T, r = 192, 64, 136, 65, 16
    codes, absmax, _, _ = _weights(K, block, N, False, 12)
    x, gy = _rows(T, K, False, 13), _rows(T, N, False, 14)
    v, B, dv, A = _adapters(K, N, r, False, 15)
    run = lambda v, dv: _fused(codes, absmax, None, block, x, v[:T], B, gy, dv[:T], A, None, torch.float32)
    clean, again = run(v, dv), run(v, dv)
    assert torch.equal(clean[0], again[0]) and torch.equal(clean[1], again[1])
    vb, dvb = v.clone(), dv.clone()
    vb[3, 5], vb[40, 15], dvb[3, 0], dvb[40, 9] = float("inf"), float("nan"), float("nan"), float("-inf")
    bad = torch.zeros(T, dtype=torch.bool).index_fill_(0, torch.tensor([3, 40]), True)
    for got, ok in zip(run(vb, dvb), clean):
        assert bool(got[bad].isnan().all()) and torch.equal(got[~bad], ok[~bad])


@pytest.mark.parametrize("dt", DTYPES)
def test_odd_addresses_exact_sizes_and_stale_results(dt):
    """test_gpu_nf4's pool: every operand sized exactly between guard bands; v, dv, B and A at addresses that are multiples
    of 4 only (the element-load path).  The results start as NaN patterns and the bands must not change."""
    K, block, N, T, r = 192, 64, 40, 33, 8
    codes, absmax, _, _ = _weights(K, block, N, False, 16)
    x, gy, bias = _rows(T, K, False, 17).to(dt), _rows(T, N, False, 18).to(dt), torch.randn(N)
    v, B, dv, A = _adapters(K, N, r, False, 19)
    v, dv = v[:T].contiguous(), dv[:T].contiguous()
    want = _fused(codes, absmax, None, block, x, v, B, gy, dv, A, bias, dt)
    es, off = x.element_size(), [0]
    pool = torch.full((1 << 17,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFF: NaN in every float type)

    def place(t, align):
        start = (off[0] + 64 + 15) // 16 * 16 + (align if align < 16 else 0)  # 16 n + align: no more aligned than `align`
        off[0] = start + t.numel() * t.element_size()
        view = pool[start:off[0]].view(t.dtype).view(t.shape)
        view.copy_(t)
        return view
    fwd = [place(t, al) for t, al in ((codes, 16), (absmax, 4), (x, es), (v, 4), (B, 4), (bias, 4))]
    bwd = [place(t, al) for t, al in ((gy, es), (dv, 4), (A, 4))]
    out, dx = place(torch.full((T, N), float("nan"), dtype=dt), es), place(torch.full((T, K), float("nan"), dtype=dt), es)
    before = pool.clone()
    L, _native, I = fq()._native.lib(), fq()._native, {torch.float32: 0, torch.bfloat16: 2}[dt]
    st = torch.cuda.current_stream().cuda_stream
    c, a, xs, vs, Bs, b, gs, dvs, As, o, dxp = (t.data_ptr() for t in fwd + bwd + [out, dx])
    _native.check(L.fql_linear_lut4_lora_fwd(c, a, None, block, xs, I, vs, Bs, r, b, o, I, T, K, N, st), "fwd")
    _native.check(L.fql_linear_lut4_lora_bwd_input(c, a, None, block, gs, I, dvs, As, r, dxp, I, T, K, N, st), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want[0]) and torch.equal(dx.cpu(), want[1])
    out.fill_(float("nan")), dx.fill_(float("nan"))
    assert torch.equal(pool, before)                                          # nothing outside the two results was written


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_layer_against_the_ops_and_autograd(dt):
    K, N, T, r, alpha = 192, 136, 65, 8, 24.0
    s, ops = alpha / r, fq().ops
    g = torch.manual_seed(21)                                                 # (the default generator: nn.Linear's draws too)
    base = fq().NF4Linear.from_linear(torch.nn.Linear(K, N), input_grad=True).to(DEV)
    lora = fq().LoRANF4Linear.from_layer(base, rank=r, alpha=alpha, fused=True)
    pytest.raises(ValueError, fq().LoRANF4Linear, K, N, r, fused=True, split_k=True)
    buffers = {k: t.clone() for k, t in base.named_buffers()}
    x, gy = torch.randn(T, K, generator=g).bfloat16().float(), torch.randn(T, N, generator=g).bfloat16().float()
    xg, gyd = x.to(DEV, dt).requires_grad_(True), gy.to(DEV, dt)
    with torch.no_grad():
        assert torch.equal(lora(xg), base(xg))                                # lora_B = 0: NF4Linear's bits
        lora.lora_B.copy_(torch.randn(N, r, generator=g) * 0.1)
    y = lora(xg)
    y.backward(gyd)
    w, xd, A, B = (base.codes, base.absmax), xg.detach(), lora.lora_A.detach(), lora.lora_B.detach()
    v, dv = ops.lora_shrink(xd, A, "rc", scale=s), ops.lora_shrink(gyd, B, "cr", scale=s)
    hand = (ops.linear_forward_lut4_lora(*w, xd, v, B, base.code_book, 64, bias=base.bias, out_dtype=dt),
            ops.linear_backward_input_lut4_lora(*w, gyd, dv, A, base.code_book, 64, out_dtype=dt),
            ops.lora_grad(xd, dv, "rc")[0], ops.lora_grad(gyd, v, "cr")[0])
    got = (y, xg.grad, lora.lora_A.grad, lora.lora_B.grad)
    assert all(torch.equal(a.detach(), b) for a, b in zip(got, hand))         # the hand composition of the four ops, bit for bit
    # float64 autograd on the dequantised weights: test_gpu_nf4's float32 bound, plus the two adapter factors' bfloat16 roundings
    W = fq().dequantize_lut4(base.codes.cpu(), base.absmax.cpu()).double()
    x64, A64, B64 = x.double().requires_grad_(True), A.cpu().double().requires_grad_(True), B.cpu().double().requires_grad_(True)
    bias, gd = base.bias.cpu().double(), gy.double()
    ref = x64 @ W.T + bias + s * (x64 @ A64.T) @ B64.T
    ref.backward(gd)
    aW, aA, aB, ax, ag = W.abs(), A64.detach().abs(), B64.detach().abs(), x.double().abs(), gd.abs()
    mu, mg, h = s * (ax @ aA.T), s * (ag @ aB), 2.0 ** -8 + 2.0 ** -18
    checks = [(ref, K + r + 2, ax @ aW.T + bias.abs() + mu @ aB.T, h * (mu @ aB.T)), (x64.grad, N + r + 2, ag @ aW + mg @ aA, h * (mg @ aA)),
              (A64.grad, N + T + 1, mg.T @ ax, 0), (B64.grad, K + T + 1, ag.T @ mu, 0)]
    for a, (rr, terms, mags, extra) in zip(got, checks):
        bound = terms * U * mags + extra + (2.0 ** -8 * rr.detach().abs() if a.dtype == torch.bfloat16 else 0)
        err = (a.detach().cpu().double() - rr.detach()).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
    for k, t in base.named_buffers():
        assert torch.equal(t, buffers[k]), k                                  # the NF4 buffers are frozen
