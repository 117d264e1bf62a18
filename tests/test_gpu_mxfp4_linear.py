"""The dense MXFP4 linear layer on the GPU: ops.linear_forward_mxfp4 / ops.linear_gated_forward_mxfp4 /
ops.linear_backward_input_mxfp4, the split-K decode form behind them (csrc/fql_gemm_mx4_linear.h) and MXFP4Linear.

Shapes: K in {32, 96, 288, 544, 1024}, i.e. P = K / 64 = 0 whole pairs with the odd block alone, then 1 + odd, 4 + odd,
8 + odd, and 16 without an odd block; N in {8, 40, 136} (below 32, across 32, a fifth wave); T in {1, 2, 33, 70} (a second
row block, a third).  Every S in {1, 2, 4, 8, 16} is forced through the tuning hook on every shape, so slices with nothing
to do (S > P) run as well; the library's own S(K, N) is 1, 1, 4, 8, 16 on the five K.  The split range is opened to 128 rows
by the hook for the tests that compare batch sizes; the library's default decides nothing here.

MEASURED (MI355X; printed with -s):
  * float32 result against the float64 product of the bfloat16-rounded operands, relative Frobenius error, the split form
    at the policy's S and at S = 16: see GAUSSIAN_MEASURED below; the bound is test_gpu_mxfp4.py's SAME_INPUT_BOUND (2.64e-7,
    asserted there up to 288 terms) times K / 288 above 288 terms, plus 2^-9 for a 16-bit result.
  * x.grad of the layer against float64 autograd on the dequantised weights: LAYER_GRAD_MEASURED below; asserted at 4 x that,
    capped at 2^-6 (DESIGN.md section 26's rule).
"""
import functools

import pytest
import torch

import test_gpu_mxfp4 as fwd_t
from glu_reference import ALPHA, LIMIT, act_kw
from helpers import NAN, SENT, Guarded, assert_guards_intact, fq, guarded_like, misaligned, ops, rel_fro_dev, same_bits
from test_gpu_mxfp4 import BF16_OUT, SAME_INPUT_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
KS, NS, TS = [32, 96, 288, 544, 1024], [8, 40, 136], [1, 2, 33, 70]
SLICES = (1, 2, 4, 8, 16)
POLICY = {32: 1, 96: 1, 288: 4, 544: 8, 1024: 16}      # S(K, N) for N <= 136: 16, capped at max(1, K / 64)
T_ALL = max(TS)
INT_MAX = 2 ** 31 - 1
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
PREFILLS = (0x00, 0xFF, 0x7F)

# relative Frobenius error of the float32 result of the split form against the float64 product of the same rounded
# operands: the largest value printed on an MI355X over the fifteen shapes, both row types, the policy's S and S = 16
GAUSSIAN_MEASURED = 5.775e-8       # (K = 1024, N = 40, S = 16; the bound there is 2.64e-7 x 1024 / 288 = 9.39e-7)
# x.grad of MXFP4Linear(input_grad=True) against float64 autograd on the dequantised weights, the largest value printed on
# an MI355X per activation type.  The error is one rounding to bfloat16: of gy in the float32 layer's backward, of x.grad
# itself in the bfloat16 layer (whose gy is bfloat16 already)
LAYER_GRAD_MEASURED = {torch.float32: 1.700e-3, torch.bfloat16: 1.665e-3}      # (K = 1024, N = 136; K = 288, N = 40)
GRAD_CAP = 2.0 ** -6


def gaussian_bound(K, dout=torch.float32):
    return SAME_INPUT_BOUND * max(1.0, K / 288.0) + (0.0 if dout == torch.float32 else BF16_OUT)


def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def hooks():
    """(set_rows, set_slices) of the split form with the split range opened to 128 rows; the library's values come back."""
    L = lib()
    rows, slices = L.fql_tune_set_mx4_linear_decode_max_rows(128), L.fql_tune_set_mx4_linear_slices(0)
    dec = L.fql_tune_set_mx4_decode_max_rows(-1)
    try:
        yield L.fql_tune_set_mx4_linear_decode_max_rows, L.fql_tune_set_mx4_linear_slices
    finally:
        L.fql_tune_set_mx4_linear_decode_max_rows(rows)
        L.fql_tune_set_mx4_linear_slices(slices)
        L.fql_tune_set_mx4_decode_max_rows(dec)


@functools.lru_cache(maxsize=None)
def problem(K, N, integer=False, lo=125, hi=129, seed=0):
    """One matrix [N, K] of random element codes and scale codes in [lo, hi], T_ALL rows (randn, or integers in [-4, 4]) and
    a bias [N].  The scale codes span 2^4 and not test_gpu_mxfp4.py's 2^60: the 2^-9 allowed for a 16-bit result is a bound
    on an r.m.s. (one rounding to bfloat16 is up to 2^-8 of an element and 2^-8 / sqrt(6) = 1.6e-3 r.m.s. over a binade), so
    it holds where many outputs carry the norm, not where the one weight row with the largest scale does (70 outputs at
    N = 8: measured 2.05e-3 on the kernels that existed before this file, at K = 96).  ``ref`` / ``ref_b``: float64, the
    product of the bfloat16-rounded rows and the exactly dequantised weights (+ bias).  Computed once per shape and shared;
    nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(7000 * K + N + seed)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.uint8)
    blocks = fwd_t.pack(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    x = torch.randint(-4, 5, (T_ALL, K), generator=g).float() if integer else torch.randn(T_ALL, K, generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g).float() if integer else torch.randn(N, generator=g)
    ref = x.bfloat16().double() @ W.T
    return dict(K=K, N=N, codes=codes, blocks=blocks.to(DEV), scales=scales.to(DEV), x=x.to(DEV), bias=bias.to(DEV), ref=ref,
                ref_b=ref + bias.double(), W=W)


def run(p, x=None, bias=False, out_dtype=None, split_k=True, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"])
    a.update(over)
    return ops().linear_forward_mxfp4(a["blocks"], a["scales"], p["x"] if x is None else x,
                                      bias=p["bias"] if bias is True else (None if bias is False else bias), out_dtype=out_dtype,
                                      split_k=split_k)


def kernel_of(T, K, N):
    v = lib().fql_tune_mx4_linear_kernel(T, K, N)
    return v >> 8, v & 0xFF


# ---- 1. the slicing and the lane map, exactly

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din, hooks):
    """Integer rows in [-4, 4], random codes, scale codes in [125, 129]: every product is a multiple of 2^-3 and every
    partial sum is below 2^17, so any float32 order gives the integer reference bit for bit.  The data is asymmetric: a
    slice that takes the wrong pairs, a dropped or doubled odd block or a partial row stored under the wrong t fails."""
    _, set_slices = hooks
    p = problem(K, N, integer=True)
    assert float(p["ref_b"].abs().max()) < 2 ** 17 and float(p["ref"].abs().max()) < 2 ** 17
    for S in (0,) + SLICES:                                                  # 0: the library's policy
        set_slices(S)
        for T in TS:
            want_S = POLICY[K] if S == 0 else S
            assert kernel_of(T, K, N) == (want_S, 2 if want_S > 1 else 1), (S, T)
            x = p["x"][:T].to(din)
            for bias in (False, True):
                ref = (p["ref_b"] if bias else p["ref"])[:T]
                got = run(p, x, bias=bias, out_dtype=torch.float32)
                assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, S, T, bias)
            got16 = run(p, x, bias=True, out_dtype=torch.bfloat16)           # one rounding of the exact value
            assert same_bits(got16.cpu(), p["ref_b"][:T].float().bfloat16()), (K, N, S, T)
    set_slices(16)
    got16 = run(p, p["x"][:33].to(din), bias=True, out_dtype=torch.float16)
    assert same_bits(got16.cpu(), p["ref_b"][:33].float().half())


# ---- 2. split_k=False is the grouped op on the one-expert view

@pytest.mark.parametrize("form", [0, INT_MAX], ids=["tile", "decode"])
@pytest.mark.parametrize("K,N", [(96, 40), (544, 136)])
def test_without_split_k_it_is_the_grouped_op(K, N, form, hooks):
    set_rows, set_slices = hooks
    set_slices(16)                                                           # (must not matter)
    lib().fql_tune_set_mx4_decode_max_rows(form)
    p = problem(K, N)
    g = torch.Generator().manual_seed(11)
    gate_up = torch.randn(T_ALL, 2 * K, generator=g).to(DEV)
    for T in (2, 70):
        tpe, offs = torch.tensor([T], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for din in (torch.float32, torch.bfloat16):
            for dout in (torch.float32, torch.float16, torch.bfloat16):
                x = p["x"][:T].to(din)
                got = run(p, x, bias=True, out_dtype=dout, split_k=False)
                want = ops().moe_forward_mxfp4(p["blocks"][None], p["scales"][None], x, tpe, offs, bias=p["bias"][None], out_dtype=dout)
                assert same_bits(got, want), (T, din, dout)
                assert same_bits(got, ops().moe_forward_mxfp4(p["blocks"][None], p["scales"][None], x, None, None,
                                                              bias=p["bias"][None], out_dtype=dout))          # no table
                gu = gate_up[:T].to(din)
                got = ops().linear_gated_forward_mxfp4(p["blocks"], p["scales"], gu, bias=p["bias"], out_dtype=dout, split_k=False,
                                                       **act_kw("swiglu_clamp"))
                want = ops().moe_gated_forward_mxfp4(p["blocks"][None], p["scales"][None], gu, tpe, offs, bias=p["bias"][None],
                                                     out_dtype=dout, **act_kw("swiglu_clamp"))
                assert same_bits(got, want), (T, din, dout)


# ---- 3. random inputs

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_inputs_against_the_same_rounded_inputs(K, N, hooks):
    _, set_slices = hooks
    p = problem(K, N)
    for S in (0, 16):
        set_slices(S)
        for din in (torch.float32, torch.bfloat16):
            x = p["x"].to(din)
            for bias in (False, True):
                ref = p["ref_b"] if bias else p["ref"]
                e32 = rel_fro_dev(run(p, x, bias=bias, out_dtype=torch.float32), ref)
                e16 = rel_fro_dev(run(p, x, bias=bias, out_dtype=torch.bfloat16), ref)
                print(f"mxfp4 linear K={K} N={N} S={S or POLICY[K]} in={din} bias={bias}: rel_fro f32 out {e32:.3e} "
                      f"(bound {gaussian_bound(K):.2e}), bf16 out {e16:.3e} (bound {gaussian_bound(K, torch.bfloat16):.3e})")
                assert e32 <= gaussian_bound(K)
                assert e16 <= gaussian_bound(K, torch.bfloat16)


# ---- 4. a row's bits do not depend on the batch; run to run

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_batch_invariance_and_determinism(K, N, hooks):
    _, set_slices = hooks
    p = problem(K, N)
    perm = torch.randperm(T_ALL, generator=torch.Generator().manual_seed(5)).to(DEV)
    for S in (0, 16):
        set_slices(S)
        for din, dout in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
            x = p["x"].to(din)
            full = run(p, x, bias=True, out_dtype=dout)
            assert same_bits(full, run(p, x, bias=True, out_dtype=dout))                        # two runs
            for t in (0, 1, 31, 32, 63, 64, 69):
                one = run(p, x[t:t + 1], bias=True, out_dtype=dout)
                assert same_bits(one[0], full[t]), (S, din, t)
            assert same_bits(run(p, x[:33], bias=True, out_dtype=dout), full[:33])
            shuffled = run(p, x[perm].contiguous(), bias=True, out_dtype=dout)
            assert same_bits(shuffled, full[perm].contiguous()), (S, din)


# ---- 5. the non-finite rules

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [0, 4])
def test_a_non_finite_element_makes_exactly_its_row_nan(S, din, hooks):
    """K = 544: eight pairs and the odd block.  S = 4 gives slices of two pairs (the odd block with the last), the policy's
    S = 8 one pair each.  An Inf and a NaN in the first, a middle and the last slice's part of a row, and in the odd block:
    only that slice's partial row is NaN, and the sum makes exactly that output row NaN."""
    _, set_slices = hooks
    set_slices(S)
    K, N, T = 544, 40, 33
    p = problem(K, N)
    clean = run(p, p["x"][:T].to(din), bias=True, out_dtype=torch.float32)
    assert bool(torch.isfinite(clean).all())
    for k in (5, 2 * 64 + 7, 7 * 64 + 3, 512 + 9):                           # first, a middle, the last slice; the odd block
        for t in (0, 17, 32):
            for bad in (float("inf"), float("-inf"), NAN):
                x = p["x"][:T].to(din).clone()
                x[t, k] = bad
                got = run(p, x, bias=True, out_dtype=torch.float32)
                assert bool(torch.isnan(got[t]).all()), (k, t, bad)
                keep = torch.arange(T, device=DEV) != t
                assert same_bits(got[keep], clean[keep]), (k, t, bad)


@pytest.mark.parametrize("S", [0, 4, 16])
def test_scale_codes(S, hooks):
    """Scale code 255 makes exactly its weight row's outputs NaN, on every row (zero rows included); codes 0 and 1 are
    weights below 2^-126 (flushed or not, they change no float32 sum here); code 254 with |code| >= 4 is an infinite weight."""
    _, set_slices = hooks
    set_slices(S)
    K, N, T = 544, 40, 33
    p = problem(K, N, integer=True)
    x = p["x"][:T].clone()
    x[3] = 0                                                                 # NaN * 0 is NaN as well
    x[:, 512 + 4] = 1.0
    clean = run(p, x, out_dtype=torch.float32)
    others = torch.arange(N, device=DEV) != 5
    for b in (0, 6, 15, 16):                                                 # first slice, a middle one, the last pair, the odd block
        sc = p["scales"].clone()
        sc[5, b] = 255
        got = run(p, x, out_dtype=torch.float32, scales=sc)
        assert bool(torch.isnan(got[:, 5]).all()), b
        assert same_bits(got[:, others], clean[:, others]), b
        codes = p["codes"].clone()
        codes[5, 32 * b:32 * b + 32] = 0
        zeroed = run(p, x, out_dtype=torch.float32, blocks=fwd_t.pack(codes).to(DEV))
        for tiny in (0, 1):
            sc[5, b] = tiny
            got = run(p, x, out_dtype=torch.float32, scales=sc)
            assert same_bits(got[:, others], clean[:, others]), (b, tiny)
            assert float((got[:, 5] - zeroed[:, 5]).abs().max()) <= 2.0 ** -110, (b, tiny)
        sc[5, b] = 254
        codes[5, 32 * b:32 * b + 32] = 7                                     # 6 * 2^127
        got = run(p, x, out_dtype=torch.float32, scales=sc, blocks=fwd_t.pack(codes).to(DEV))
        assert not bool(torch.isfinite(got[:, 5]).any()), b
        assert same_bits(got[:, others], clean[:, others]), b
    sc = p["scales"].clone()
    sc[5, 16] = 254                                                          # 0.5 * 2^127 = 2^126 is a float32: one such weight
    codes = p["codes"].clone()
    codes[5, 512:544] = 0
    codes[5, 512 + 4] = 1
    got = run(p, x, out_dtype=torch.float32, scales=sc, blocks=fwd_t.pack(codes).to(DEV))
    # (2^126 plus the row's other 2^17 at most: the float32 next to 2^126, whichever way the matrix core's adder rounds)
    assert float((got[:, 5].double() / 2.0 ** 126 - 1).abs().max()) <= 2.0 ** -22, got[:4, 5]
    assert same_bits(got[:, others], clean[:, others])


# ---- 6. the gated entry

def own_hidden(gate_up, kind):
    """The grouped gated op's own h [T, K] bfloat16: the op on unit weights (code 2 = 1.0 on the diagonal, scale code 127)
    returns h[t][n] * 1 plus exact zeros."""
    T, K = gate_up.shape[0], gate_up.shape[1] // 2
    codes = torch.zeros(1, K, K, dtype=torch.uint8)
    codes[:, torch.arange(K), torch.arange(K)] = 2
    blocks, scales = fwd_t.pack(codes).to(DEV), torch.full((1, K, K // 32), 127, dtype=torch.uint8, device=DEV)
    tpe, offs = torch.tensor([T], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    h = ops().moe_gated_forward_mxfp4(blocks, scales, gate_up, tpe, offs, out_dtype=torch.float32, **act_kw(kind))
    assert torch.equal(h, h.bfloat16().float())
    return h.bfloat16()


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_gated_is_the_plain_op_on_its_own_hidden_rows(kind, din, hooks):
    _, set_slices = hooks
    set_slices(4)
    K, N = 288, 40
    p = problem(K, N)
    g = torch.Generator().manual_seed(13)
    for T in (2, 33):
        gate_up = torch.randn(T, 2 * K, generator=g).to(DEV).to(din)
        h = own_hidden(gate_up, kind)
        assert kernel_of(T, K, N) == (4, 2)
        for dout in (torch.float32, torch.bfloat16):
            want = run(p, h, bias=True, out_dtype=dout)
            got = ops().linear_gated_forward_mxfp4(p["blocks"], p["scales"], gate_up, bias=p["bias"], out_dtype=dout, **act_kw(kind))
            assert same_bits(got, want), (kind, T, dout)


# ---- 7. the footprint

@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_entries_stay_inside_their_buffers(dout, gated, hooks):
    """T = 33, N = 40, K = 288 at S = 16 (twelve slices have nothing to do and store zeros): out and the workspace are the
    interiors of guarded buffers, out 4 bytes off a 16-byte boundary and prefilled with SENT, the rows' base misaligned.
    Only [T, N] changes and all of it does; a store past T or N in a partial or in out lands in a guard or in SENT.  The
    workspace is prefilled with stale bytes, 0xFF being NaN as float32 and as bfloat16: the result does not change."""
    _, set_slices = hooks
    set_slices(16)
    T, N, K = 33, 40, 288
    p = problem(K, N)
    L = lib()
    if gated:
        g = torch.Generator().manual_seed(3)
        rows = misaligned(torch.randn(T, 2 * K, generator=g).to(DEV), 1)
        want = ops().linear_gated_forward_mxfp4(p["blocks"], p["scales"], rows, bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp"))
    else:
        rows = misaligned(p["x"][:T], 1)
        want = run(p, rows, bias=True, out_dtype=dout)
    assert rows.data_ptr() % 16 == 4 and kernel_of(T, K, N) == (16, 2)
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    nbytes = L.fql_linear_mx4_workspace_bytes(T, K, N, int(gated), 1)
    assert nbytes == ((T * K * 2 + 15) // 16 * 16 if gated else 0) + 64 * T * N
    ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
    st = torch.cuda.current_stream().cuda_stream
    for fill in PREFILLS:
        ws.bytes().fill_(fill)
        out.view(dout, T, N).fill_(SENT)
        if gated:
            rc = L.fql_linear_mx4_glu_fwd(bl.ptr, sc.ptr, rows.data_ptr(), 0, bias.ptr, out.ptr, DT[dout], T, K, N,
                                          ACT["swiglu_clamp"], ALPHA, LIMIT, 1, ws.ptr, nbytes, st)
        else:
            rc = L.fql_linear_mx4_fwd(bl.ptr, sc.ptr, rows.data_ptr(), 0, bias.ptr, out.ptr, DT[dout], T, K, N, 1, ws.ptr, nbytes, st)
        assert rc == 0
        assert_guards_intact(bl, sc, bias, out, ws, what=f"mx4 linear gated={gated} {dout} workspace {fill:#04x}")
        got = out.view(dout, T, N)
        assert int((got == SENT).sum()) == 0, hex(fill)                      # every element is written
        assert same_bits(got, want), hex(fill)
        # the partial sums, 16 slices of [T][N] behind h: P = 4 pairs in slices 0 .. 3, the odd block in slice 15, and the
        # eleven slices between them have nothing to do and store zeros over whatever was there
        part = ws.bytes()[nbytes - 64 * T * N:].view(torch.float32).view(16, T, N)
        assert bool(torch.isfinite(part).all()) and torch.count_nonzero(part[4:15]) == 0, hex(fill)
        assert all(int(torch.count_nonzero(part[s])) > 0 for s in (0, 1, 2, 3, 15)), hex(fill)


# ---- 8. the layer

def grad_bound(measured):
    return min(4 * measured, GRAD_CAP)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(288, 40), (1024, 136)])
def test_layer_forward_and_input_gradient(K, N, dt, hooks):
    p = problem(K, N)
    m = fq().MXFP4Linear.from_mxfp4(p["blocks"].cpu(), p["scales"].cpu(), bias=p["bias"].cpu(), input_grad=True)
    x_cpu = p["x"].cpu().reshape(2, T_ALL // 2, K)[:, :16].contiguous().to(dt)       # [2, 16, K]: inside the split range
    want = m(x_cpu)
    m = m.to(DEV)
    assert sorted(m.state_dict()) == ["bias", "blocks", "scales"]
    with torch.no_grad():
        got = m(x_cpu.to(DEV))
    assert got.shape == (2, 16, N) and got.dtype == dt
    err = rel_fro_dev(got, want)
    print(f"MXFP4Linear K={K} N={N} {dt}: GPU against the CPU forward, rel_fro {err:.3e} (bound {gaussian_bound(K, dt):.3e})")
    assert err <= gaussian_bound(K, dt)
    assert same_bits(m(x_cpu[0, 3].to(DEV)), got[0, 3])                                # 1-D input, and the batch does not matter
    # the input gradient
    x = x_cpu.to(DEV).clone().requires_grad_(True)
    gy = torch.randn(2, 16, N, generator=torch.Generator().manual_seed(17)).to(DEV).to(dt)
    y = m(x)
    assert same_bits(y.detach(), got)
    y.backward(gy)
    assert x.grad.dtype == dt and x.grad.shape == x.shape
    direct = ops().moe_backward_input_mxfp4(p["blocks"][None], p["scales"][None], gy.reshape(-1, N), None, None, out_dtype=dt)
    assert torch.equal(x.grad.reshape(-1, K), direct)
    assert torch.equal(direct, ops().linear_backward_input_mxfp4(p["blocks"], p["scales"], gy.reshape(-1, N), out_dtype=dt))
    x64 = x_cpu.double().requires_grad_(True)
    (x64 @ p["W"].T + p["bias"].cpu().double()).backward(gy.cpu().double())
    gerr = rel_fro_dev(x.grad, x64.grad)
    print(f"MXFP4Linear K={K} N={N} {dt}: x.grad against float64 autograd, rel_fro {gerr:.3e} "
          f"(bound {grad_bound(LAYER_GRAD_MEASURED[dt]):.3e})")
    assert gerr <= grad_bound(LAYER_GRAD_MEASURED[dt])
    plain = fq().MXFP4Linear.from_mxfp4(p["blocks"], p["scales"])
    with pytest.raises(RuntimeError, match="inference-only"):
        plain(x)


@pytest.mark.parametrize("precision", ["fp8", "fp6", "fp4"])
def test_block_scaled_layers_are_the_grouped_ops(precision, hooks):
    K, N, T = 288, 40, 33
    p = problem(K, N)
    m = fq().MXFP4Linear.from_mxfp4(p["blocks"], p["scales"], bias=p["bias"], precision=precision)
    g = torch.Generator().manual_seed(19)
    gate_up = torch.randn(T, 2 * K, generator=g).to(DEV)
    for dt in (torch.float32, torch.bfloat16):
        x = p["x"][:T].to(dt)
        want = ops().moe_forward_mxfp4(p["blocks"][None], p["scales"][None], x, None, None, bias=p["bias"][None], out_dtype=dt,
                                       precision=precision)
        with torch.no_grad():
            assert same_bits(m(x), want), dt
        got = ops().linear_gated_forward_mxfp4(p["blocks"], p["scales"], gate_up.to(dt), bias=p["bias"], precision=precision,
                                               **act_kw("gelu_tanh"))
        want = ops().moe_gated_forward_mxfp4(p["blocks"][None], p["scales"][None], gate_up.to(dt), None, None,
                                             bias=p["bias"][None], precision=precision, **act_kw("gelu_tanh"))
        assert same_bits(got, want), dt
