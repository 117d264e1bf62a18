"""The split-K decode form of the 4-bit code-book (NF4) forward on the GPU (csrc/fql_gemm_lut4_decode.h)
against a float64 reference built from W by the definition.  K: one pair (empty slices for S > 1), three pairs (uneven
slices), ten pairs under block = 128 (an absmax shared by two pairs; the ring of four slots wraps more than once at S = 1);
N: a partial 32-column tile, the scalar store path, two tiles with 16-byte stores; T: one row, one short of and one past a
row block (the threshold is raised to 64 here so that 33 rows take a second block); S: 1, 2, 4, 16 forced and the policy's."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = [(64, 64), (192, 64), (640, 128)]
NS = [8, 33, 72]
TS = [1, 31, 33]
SS = [1, 2, 4, 16, 0]                                                        # (0: the policy's S(K, N))
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -23
WS_ERR = -4


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


@contextlib.contextmanager
def _forced(slices, max_rows=64):
    lib = fq()._native.lib()
    old = lib.fql_tune_set_lut4_linear_decode_max_rows(max_rows), lib.fql_tune_set_lut4_linear_slices(slices)
    try:
        yield lib
    finally:
        lib.fql_tune_set_lut4_linear_decode_max_rows(old[0]), lib.fql_tune_set_lut4_linear_slices(old[1])


def _split(codes, absmax, book, block, x, bias, S, split_k=True, **kw):
    d = lambda t: None if t is None else t.to(DEV)
    with _forced(S) as lib:
        T, K, N = x.shape[0], x.shape[1], codes.shape[0]
        if split_k and T <= 64:                                               # (the form the call is about to take)
            assert lib.fql_tune_lut4_linear_kernel(T, K, N) & 255 == 2 and (S == 0 or lib.fql_tune_lut4_linear_kernel(T, K, N) >> 8 == S)
        return fq().ops.linear_forward_lut4(d(codes), d(absmax), d(x), d(book), block, bias=d(bias), split_k=split_k, **kw).cpu()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_exact_integers_bit_for_bit_at_every_slice_count(K, block, N, dt):
    codes, absmax, book, W = _weights(K, block, N, True, 1)
    x, bias = _rows(max(TS), K, True, 2), torch.arange(N, dtype=torch.float32) - 3
    ref, m = x.double() @ W.T + bias.double(), x.double().abs() @ W.abs().T + bias.abs()
    assert bool((ref * 4 == (ref * 4).round()).all()) and float(m.max()) * 4 < 2 ** 24   # multiples of 2^-2, far below 2^24
    for T in TS:
        for S in SS:
            out = _split(codes, absmax, book, block, x[:T].to(dt), bias, S)
            assert out.dtype == dt and torch.equal(out, ref[:T].float().to(dt)), (T, S)  # (the exact value, rounded once)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_nf4_gaussian_within_the_float32_bound(K, block, N, dt):
    """|got - ref| <= K 2^-23 sum |x W| (a float32 sum of K exact products in any order: a split sum is one), + 2^-8 |ref| for
    a bfloat16 result."""
    codes, absmax, _, W = _weights(K, block, N, False, 4)
    x = _rows(max(TS), K, False, 5).bfloat16().double()
    ref = x @ W.T
    bound = K * U * (x.abs() @ W.abs().T) + (2.0 ** -8 * ref.abs() if dt == torch.bfloat16 else 0)
    worst = 0.0
    for T in TS:
        for S in SS:
            err = (_split(codes, absmax, None, block, x[:T].to(dt), None, S).double() - ref[:T]).abs()
            ratio = float((err / bound[:T].clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound[:T]).all()), (T, S, ratio)
    print(f"K={K} N={N} {dt}: largest |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("S", [0, 4])
def test_batch_invariance_rerun_and_row_permutation(S):
    K, block, N, T = 192, 64, 72, 33
    codes, absmax, _, _ = _weights(K, block, N, False, 7)
    x, bias = _rows(T, K, False, 8), torch.randn(N, generator=torch.Generator().manual_seed(9))
    out = _split(codes, absmax, None, block, x, bias, S)
    assert torch.equal(out, _split(codes, absmax, None, block, x, bias, S))   # run to run
    for t in (0, 31, 32):                                                     # a row alone: the bits it has in the batch
        assert torch.equal(_split(codes, absmax, None, block, x[t:t + 1], bias, S)[0], out[t]), t
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(10))
    assert torch.equal(_split(codes[perm], absmax[perm], None, block, x, bias[perm], S), out[:, perm])


@pytest.mark.parametrize("dt", DTYPES)
def test_non_finite_rows_in_different_slices(dt):
    """S = 2 on three pairs: slice 0 is k < 128, slice 1 the rest.  An inf in slice 0 of row 3 and a NaN in slice 1 of row 32
    (the second row block) make exactly those rows NaN."""
    K, block, N, T = 192, 64, 72, 33
    codes, absmax, _, _ = _weights(K, block, N, False, 11)
    x = _rows(T, K, False, 12).to(dt)
    clean = _split(codes, absmax, None, block, x, None, 2)
    xb = x.clone()
    xb[3, 10], xb[32, 191] = float("inf"), float("nan")
    got = _split(codes, absmax, None, block, xb, None, 2)
    bad = torch.zeros(T, dtype=torch.bool)
    bad[[3, 32]] = True
    assert bool(got[bad].isnan().all()) and torch.equal(got[~bad], clean[~bad])


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("dt", DTYPES)
def test_odd_addresses_exact_sizes_and_guard_bands(dt, S):
    """N = 33: every operand sits in one 0xFF pool at an address that is a multiple of its element only (the codes and the
    workspace: of 16, as the ABI asks), sized exactly, between guard bands; nothing but out and the workspace may change."""
    K, block, N, T = 192, 64, 33, 33
    codes, absmax, _, _ = _weights(K, block, N, False, 13)
    x, bias = _rows(T, K, False, 14).to(dt), torch.randn(N, generator=torch.Generator().manual_seed(15))
    want = _split(codes, absmax, None, block, x, bias, S)
    es = x.element_size()
    pool = torch.full((1 << 18,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFF: NaN in every float type)
    off = [0]

    def place(t, align):
        start = (off[0] + 64 + 15) // 16 * 16 + (align if align < 16 else 0)  # 16 n + align: no more aligned than `align`
        off[0] = start + t.numel() * t.element_size()
        view = pool[start:off[0]].view(t.dtype).view(t.shape)
        view.copy_(t)
        return view
    with _forced(S) as L:
        ws_bytes = L.fql_linear_lut4_split_workspace_bytes(T, K, N)
        assert ws_bytes == 16 * 4 * T * N
        c, a, b, xs = place(codes, 16), place(absmax, 4), place(bias, 4), place(x, es)
        out, ws = place(torch.full((T, N), float("nan"), dtype=dt), es), place(torch.full((ws_bytes,), 0xFF, dtype=torch.uint8), 16)
        before = pool.clone()
        I, st = {torch.float32: 0, torch.bfloat16: 2}[dt], torch.cuda.current_stream().cuda_stream
        args = (c.data_ptr(), a.data_ptr(), None, block, xs.data_ptr(), I, b.data_ptr(), out.data_ptr(), I, T, K, N)
        assert L.fql_linear_lut4_split_fwd(*args, ws.data_ptr(), ws_bytes - 1, st) == WS_ERR      # refused without a launch
        assert L.fql_linear_lut4_split_fwd(*args, None, ws_bytes, st) == WS_ERR
        torch.cuda.synchronize()
        assert torch.equal(pool, before)
        fq()._native.check(L.fql_linear_lut4_split_fwd(*args, ws.data_ptr(), ws_bytes, st), "split")
        torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert bool((ws[S * 4 * T * N:] == 0xFF).all())                           # only partial[0 .. S) of the workspace is written
    out.fill_(float("nan")), ws.fill_(0xFF)
    assert torch.equal(pool, before)                                          # nothing outside out and the workspace was written


@pytest.mark.parametrize("dt", DTYPES)
def test_above_the_threshold_default_and_layers(dt):
    K, block, N = 192, 64, 72
    codes, absmax, _, _ = _weights(K, block, N, False, 16)
    x, bias = _rows(65, K, False, 17).to(dt), torch.randn(N, generator=torch.Generator().manual_seed(18))
    tile = _split(codes, absmax, None, block, x, bias, 0, split_k=False)
    assert fq()._native.lib().fql_tune_lut4_linear_kernel(65, K, N) == 1 << 8          # 65 rows: the tile kernel at any setting here
    assert torch.equal(_split(codes, absmax, None, block, x, bias, 0, split_k=True), tile)
    one = fq().ops.linear_forward_lut4(codes.to(DEV), absmax.to(DEV), x[:1].to(DEV), None, block, bias=bias.to(DEV), split_k=True)
    assert torch.equal(fq().ops.linear_forward_lut4(codes.to(DEV), absmax.to(DEV), x[:1].to(DEV), None, block, bias=bias.to(DEV)).cpu(),
                       tile[:1])                                             # the default is the parent's path
    base = fq().NF4Linear.from_bnb(codes, absmax, block, bias=bias, split_k=True).to(DEV)
    lora = fq().LoRANF4Linear.from_layer(base, rank=8)
    assert base.split_k and lora.split_k and "split_k=True" in repr(base) and "split_k" not in repr(fq().NF4Linear(K, N))
    with torch.no_grad():
        assert torch.equal(base(x[:1].to(DEV)), one) and torch.equal(lora(x[:1].to(DEV)), one)     # lora_B = 0: the op's bits
