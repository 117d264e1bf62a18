"""4-bit code-book (NF4) weights on the GPU (csrc/fql_gemm_lut4.h, csrc/fql_gemm_lut4_bwd.h): both
kernels against a float64 reference built from W by the definition (float32 multiply, ``.bfloat16()``, then float64).
K: one stage pair, an odd number of 64-k pairs, block = 128 (a scale shared by several stages); N: a partial tile and a crossing
of 128; T: one past each row-tile boundary (32, 64 and the tall tile's 256)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = [(64, 64), (192, 64), (256, 128)]
NS = [8, 40, 136]
TS = [1, 33, 65, 257]
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -23


def fq():
    import fused_int4_amd
    return fused_int4_amd


def _weights(K, block, N, exact, seed):
    """(codes, absmax, code_book, W float64 by the definition) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        book = torch.arange(-8, 8, dtype=torch.float32)
        c = torch.randint(0, 16, (N, K // 2, 2), generator=g, dtype=torch.uint8)
        codes = (c[..., 0] << 4) | c[..., 1]
        absmax = torch.ldexp(torch.ones(N, K // block), torch.randint(-2, 3, (N, K // block), generator=g))
    else:
        book = torch.tensor(fq().NF4_CODE_BOOK, dtype=torch.float32)
        codes, absmax = fq().quantize_lut4(torch.randn(N, K, generator=g) * 0.05, block=block)
    idx = torch.stack([codes >> 4, codes & 15], dim=-1).reshape(N, K).long()
    W = (book[idx] * absmax.repeat_interleave(block, dim=1)).bfloat16().double()
    return codes, absmax, book, W


def _rows(T, C, exact, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (T, C), generator=g).float() if exact else torch.randn(T, C, generator=g)


def _both(codes, absmax, book, block, x, gy, bias, dt, out_dtype=None):
    """(out, dx) of the two ops on the GPU, as CPU tensors."""
    ops, d = fq().ops, lambda t: None if t is None else t.to(DEV)
    out = ops.linear_forward_lut4(d(codes), d(absmax), d(x.to(dt)), d(book), block, bias=d(bias), out_dtype=out_dtype)
    dx = ops.linear_backward_input_lut4(d(codes), d(absmax), d(gy.to(dt)), d(book), block, out_dtype=out_dtype or dt)
    return out.cpu(), dx.cpu()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_exact_integers_bit_for_bit(K, block, N, dt):
    codes, absmax, book, W = _weights(K, block, N, True, 1)
    x, gy, bias = _rows(max(TS), K, True, 2), _rows(max(TS), N, True, 3), torch.arange(N, dtype=torch.float32) - 3
    ref, dref = x.double() @ W.T + bias.double(), gy.double() @ W
    for r, m in ((ref, x.double().abs() @ W.abs().T + bias.abs()), (dref, gy.double().abs() @ W.abs())):
        assert bool((r * 4 == (r * 4).round()).all()) and float(m.max()) * 4 < 2 ** 24   # multiples of 2^-2, far below 2^24
    for T in TS:
        out, dx = _both(codes, absmax, book, block, x[:T], gy[:T], bias, dt)
        assert out.dtype == dt and dx.dtype == dt
        assert torch.equal(out, ref[:T].float().to(dt)), (T, "forward")       # (the exact value, rounded once)
        assert torch.equal(dx, dref[:T].float().to(dt)), (T, "input gradient")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_nf4_gaussian_within_the_float32_bound(K, block, N, dt):
    """|got - ref| <= L 2^-23 sum |products| (a float32 sum of L exact products in any order), + 2^-8 |ref| for a bfloat16 result."""
    codes, absmax, _, W = _weights(K, block, N, False, 4)
    x, gy = _rows(max(TS), K, False, 5).bfloat16().double(), _rows(max(TS), N, False, 6).bfloat16().double()
    ref, dref = x @ W.T, gy @ W
    bound, dbound = K * U * (x.abs() @ W.abs().T), N * U * (gy.abs() @ W.abs())
    if dt == torch.bfloat16:
        bound, dbound = bound + 2.0 ** -8 * ref.abs(), dbound + 2.0 ** -8 * dref.abs()
    worst = 0.0
    for T in TS:
        out, dx = _both(codes, absmax, None, block, x[:T].float(), gy[:T].float(), None, dt)
        for got, r, b in ((out, ref[:T], bound[:T]), (dx, dref[:T], dbound[:T])):
            ratio = float(((got.double() - r).abs() / b.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool(((got.double() - r).abs() <= b).all()), (T, ratio)
    print(f"K={K} N={N} {dt}: largest |err| / bound = {worst:.4f}")


def test_row_permutation_rerun_and_non_finite_rows():
    K, block, N, T = 192, 64, 136, 65
    codes, absmax, _, _ = _weights(K, block, N, False, 7)
    x, gy = _rows(T, K, False, 8), _rows(T, N, False, 9)
    out, dx = _both(codes, absmax, None, block, x, gy, None, torch.float32)
    again = _both(codes, absmax, None, block, x, gy, None, torch.float32)
    assert torch.equal(out, again[0]) and torch.equal(dx, again[1])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(10))
    pout, pdx = _both(codes[perm], absmax[perm], None, block, x, gy, None, torch.float32)
    assert torch.equal(pout, out[:, perm])                                    # columns follow their weight rows, bit for bit
    xb, gb = x.clone(), gy.clone()
    xb[3, 100], xb[40, 191], gb[3, 135], gb[40, 0] = float("inf"), float("nan"), float("nan"), float("-inf")
    bout, bdx = _both(codes, absmax, None, block, xb, gb, None, torch.float32)
    bad = torch.zeros(T, dtype=torch.bool)
    bad[[3, 40]] = True
    for got, clean in ((bout, out), (bdx, dx)):
        assert bool(got[bad].isnan().all()) and torch.equal(got[~bad], clean[~bad])


@pytest.mark.parametrize("dt", DTYPES)
def test_odd_addresses_exact_sizes_and_stale_results(dt):
    """N = 40: every operand sits in one pool at an address that is a multiple of its element only (the codes: of 16, as
    the ABI asks), sized exactly, between guard bands; the results start as NaN patterns and the bands must not change."""
    K, block, N, T = 192, 64, 40, 33
    codes, absmax, _, _ = _weights(K, block, N, False, 11)
    x, gy, bias = _rows(T, K, False, 12).to(dt), _rows(T, N, False, 13).to(dt), torch.randn(N)
    want = _both(codes, absmax, None, block, x, gy, bias, dt)
    es = x.element_size()
    pool = torch.full((1 << 17,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFF: NaN in every float type)
    off = [0]

    def place(t, align):
        start = (off[0] + 64 + 15) // 16 * 16 + (align if align < 16 else 0)  # 16 n + align: no more aligned than `align`
        off[0] = start + t.numel() * t.element_size()
        view = pool[start:off[0]].view(t.dtype).view(t.shape)
        view.copy_(t)
        return view
    c, a, b = place(codes, 16), place(absmax, 4), place(bias, 4)
    xs, gs = place(x, es), place(gy, es)
    out, dx = place(torch.full((T, N), float("nan"), dtype=dt), es), place(torch.full((T, K), float("nan"), dtype=dt), es)
    before = pool.clone()
    L, _native, I = fq()._native.lib(), fq()._native, {torch.float32: 0, torch.bfloat16: 2}[dt]
    st = torch.cuda.current_stream().cuda_stream
    _native.check(L.fql_linear_lut4_fwd(c.data_ptr(), a.data_ptr(), None, block, xs.data_ptr(), I, b.data_ptr(), out.data_ptr(), I,
                                        T, K, N, st), "fwd")
    _native.check(L.fql_linear_lut4_bwd_input(c.data_ptr(), a.data_ptr(), None, block, gs.data_ptr(), I, dx.data_ptr(), I, T, K, N,
                                              st), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want[0]) and torch.equal(dx.cpu(), want[1])
    out.fill_(float("nan")), dx.fill_(float("nan"))
    assert torch.equal(pool, before)                                          # nothing outside the two results was written


@pytest.mark.parametrize("dt", DTYPES)
def test_layers_against_autograd_on_the_dequantised_weights(dt):
    K, N, T, r, alpha = 192, 136, 65, 8, 24.0
    s = alpha / r
    g = torch.Generator().manual_seed(14)
    torch.manual_seed(14)
    lin = torch.nn.Linear(K, N)
    base = fq().NF4Linear.from_linear(lin, input_grad=True).to(DEV)
    lora = fq().LoRANF4Linear.from_layer(base, rank=r, alpha=alpha)
    x = torch.randn(T, K, generator=g).bfloat16().float()                     # (bfloat16 values: no straight-through gap)
    gy = torch.randn(T, N, generator=g).bfloat16().float()
    xg = x.to(DEV, dt).requires_grad_(True)
    y0 = base(xg)
    with torch.no_grad():
        assert torch.equal(lora(xg), y0)                                      # lora_B = 0: NF4Linear's bits
        lora.lora_B.copy_(torch.randn(N, r, generator=g) * 0.1)
    y0.backward(gy.to(DEV, dt))
    gx0, xg.grad = xg.grad, None
    y1 = lora(xg)
    y1.backward(gy.to(DEV, dt))
    # the restatement, float64 autograd, with the bound's sums of magnitudes beside it
    W = fq().dequantize_lut4(base.codes.cpu(), base.absmax.cpu()).double()
    xd = x.double().requires_grad_(True)
    A, B = lora.lora_A.detach().cpu().double().requires_grad_(True), lora.lora_B.detach().cpu().double().requires_grad_(True)
    bias, gd = base.bias.cpu().double(), gy.double()
    ref0 = xd @ W.T + bias
    ref1 = ref0 + s * (xd @ A.T) @ B.T
    ref1.backward(gd)
    aW, aA, aB, ax, ag = W.abs(), A.detach().abs(), B.detach().abs(), x.double().abs(), gd.abs()
    m0, mu = ax @ aW.T + bias.abs(), s * (ax @ aA.T)
    checks = [(y0, ref0, K + 1, m0), (gx0, gd @ W, N, ag @ aW), (y1, ref1, K + r + 2, m0 + mu @ aB.T),
              (xg.grad, xd.grad, N + r + 2, ag @ aW + s * (ag @ aB) @ aA),
              (lora.lora_A.grad, A.grad, N + T + 1, s * (ag @ aB).T @ ax), (lora.lora_B.grad, B.grad, K + T + 1, ag.T @ mu)]
    for got, ref, terms, mags in checks:
        bound = terms * U * mags + (2.0 ** -8 * ref.detach().abs() if got.dtype == torch.bfloat16 else 0)
        err = (got.detach().cpu().double() - ref.detach()).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
