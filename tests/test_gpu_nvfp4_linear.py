"""The split-K decode form of the dense NVFP4 linear layer on the GPU (csrc/fql_gemm_nvfp4_linear.h):
ops.linear_forward_nvfp4 / ops.linear_gated_forward_nvfp4 with split_k=True and NVFP4Linear(split_k=True).

K in {32, 96, 288, 544, 1024}: the odd piece alone, one pair + odd, fewer pairs than the ring of four (+ odd), two rings'
worth + odd, several ring rounds; N in {8, 40, 136}; T in {1, 33}, the split range opened to 64 rows by the hook.  The
library's own S(K, N) is 1, 1, 4, 8, 16 on the five K.  Scale bytes 0x30 .. 0x47 throughout (test_gpu_mxfp4_linear.py's
problem() says why a 2^60 range of scales breaks an r.m.s. bound on a bfloat16 result)."""
import functools

import pytest
import torch

from glu_reference import act_kw
from helpers import NAN, SENT, Guarded, assert_guards_intact, fq, guarded_like, misaligned, ops, rel_fro_dev, same_bits
from test_gpu_mxfp4 import SAME_INPUT_BOUND
from test_gpu_nvfp4 import NARROW, lib, pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS, NS, TS, T_ALL = [32, 96, 288, 544, 1024], [8, 40, 136], [1, 33], 33
SLICES = (1, 2, 4, 8, 16)
POLICY = {32: 1, 96: 1, 288: 4, 544: 8, 1024: 16}      # S(K, N) for N <= 136: 16, capped at max(1, K / 64)
INT_MAX = 2 ** 31 - 1
GS = 0.25
# relative Frobenius error of the float32 result against the float64 product of the same rounded operands, the largest of the
# first run on an MI355X; asserted at 4 x it (the margin for Gaussian draws) and below DESIGN.md section 25's bound scaled to K
GAUSSIAN_MEASURED = 7.061e-8        # (K = 1024, N = 8, S = 16; the bound there is 4 x it = 2.82e-7, under 9.39e-7)
# one rounding to bfloat16 (8 significant bits) is at most 2^-8 of the element, so of the norm.  (2^-9 is an r.m.s. figure
# for many outputs; at 33 x 8 the grouped decode kernel, S = 1, gives 1.98e-3 at K = 96.)
BF16_OUT = 2.0 ** -8

def gaussian_bound(K, dout=torch.float32):
    return min(4 * GAUSSIAN_MEASURED, SAME_INPUT_BOUND * max(1.0, K / 288.0)) + (0.0 if dout == torch.float32 else BF16_OUT)

@pytest.fixture
def hooks():
    L = lib()
    old = L.fql_tune_set_nvfp4_linear_decode_max_rows(64), L.fql_tune_set_nvfp4_linear_slices(0), L.fql_tune_set_nvfp4_decode_max_rows(-1)
    yield L.fql_tune_set_nvfp4_linear_decode_max_rows, L.fql_tune_set_nvfp4_linear_slices
    L.fql_tune_set_nvfp4_linear_decode_max_rows(old[0]), L.fql_tune_set_nvfp4_linear_slices(old[1]), L.fql_tune_set_nvfp4_decode_max_rows(old[2])

def reference(x, blocks, scales, bias):
    from fused_int4_amd.quantize import dequantize_nvfp4
    return (x.cpu().bfloat16().double() @ dequantize_nvfp4(blocks.cpu(), scales.cpu()).double().T) * GS + bias.cpu().double()

@functools.lru_cache(maxsize=None)
def problem(K, N, integer=False):
    """Random codes, scale bytes in NARROW, 33 rows (randn, or integers in [-4, 4] and an integer bias); shared, read-only."""
    g = torch.Generator().manual_seed(4300 * K + N)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(NARROW[0], NARROW[1] + 1, (N, K // 16), generator=g, dtype=torch.uint8)
    x = torch.randint(-4, 5, (T_ALL, K), generator=g).float() if integer else torch.randn(T_ALL, K, generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g).float() if integer else torch.randn(N, generator=g)
    p = dict(K=K, N=N, codes=codes, blocks=pack(codes).to(DEV), scales=scales.to(DEV), x=x.to(DEV), bias=bias.to(DEV),
             gs=torch.tensor([GS], device=DEV))
    p["ref"] = reference(x, p["blocks"], scales, bias)
    return p

def run(p, x=None, out_dtype=None, split_k=True, **over):
    a = dict(p, **over)
    return ops().linear_forward_nvfp4(a["blocks"], a["scales"], a["gs"], p["x"] if x is None else x, bias=a["bias"],
                                      out_dtype=out_dtype, split_k=split_k)

def kernel_of(T, K, N):
    v = lib().fql_tune_nvfp4_linear_kernel(T, K, N)
    return v >> 8, v & 0xFF

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din, hooks):
    """Products are multiples of 2^-5, sums below 2^16: every float32 order gives the float64 product bit for bit."""
    _, set_slices = hooks
    p = problem(K, N, integer=True)
    assert (float(p["ref"].abs().max()) + 8) / GS < 2 ** 16
    for S in SLICES:
        set_slices(S)
        for T in TS:
            assert kernel_of(T, K, N) == (S, 2 if S > 1 else 1), (S, T)
            x = p["x"][:T].to(din)
            got = run(p, x, out_dtype=torch.float32)
            assert torch.equal(got.cpu().double(), p["ref"][:T]), (S, T)
            assert same_bits(run(p, x, out_dtype=torch.bfloat16).cpu(), p["ref"][:T].float().bfloat16()), (S, T)

@pytest.mark.parametrize("form", [0, INT_MAX], ids=["tile", "decode"])
@pytest.mark.parametrize("K,N", [(96, 40), (544, 136)])
def test_forced_one_slice_and_split_k_false_are_the_grouped_op(K, N, form, hooks):
    _, set_slices = hooks
    lib().fql_tune_set_nvfp4_decode_max_rows(form)
    p = problem(K, N)
    for T in TS:
        for dt in (torch.float32, torch.bfloat16):
            x = p["x"][:T].to(dt)
            want = ops().moe_forward_nvfp4(p["blocks"][None], p["scales"][None], p["gs"], x, None, None, bias=p["bias"][None])
            set_slices(1)
            assert same_bits(run(p, x), want), (T, dt)
            set_slices(16)                                                   # (must not matter without split_k)
            assert same_bits(run(p, x, split_k=False), want), (T, dt)

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gaussian_data_batch_invariance_and_determinism(K, N, hooks):
    _, set_slices = hooks
    p = problem(K, N)
    perm = torch.randperm(T_ALL, generator=torch.Generator().manual_seed(5)).to(DEV)
    for S in (0, 16):
        set_slices(S)
        for dt in (torch.float32, torch.bfloat16):
            x = p["x"].to(dt)
            e32 = rel_fro_dev(run(p, x, out_dtype=torch.float32), p["ref"])
            e16 = rel_fro_dev(run(p, x, out_dtype=torch.bfloat16), p["ref"])
            print(f"nvfp4 linear K={K} N={N} S={S or POLICY[K]} in={dt}: rel_fro f32 out {e32:.3e} (bound "
                  f"{gaussian_bound(K):.2e}), bf16 out {e16:.3e} (bound {gaussian_bound(K, torch.bfloat16):.3e})")
            assert e32 <= gaussian_bound(K) and e16 <= gaussian_bound(K, torch.bfloat16)
            full = run(p, x)
            assert same_bits(full, run(p, x))                                # a rerun
            for t in (0, 17, 31, 32):
                assert same_bits(run(p, x[t:t + 1])[0], full[t]), (S, dt, t)
            assert same_bits(run(p, x[perm].contiguous()), full[perm].contiguous()), (S, dt)

@pytest.mark.parametrize("S", [0, 4])
def test_non_finite_rules_and_negative_scale_bytes(S, hooks):
    """K = 544: eight pairs and the odd piece (scale blocks 32, 33).  The bytes go into the second 16-block of a piece."""
    _, set_slices = hooks
    set_slices(S)
    K, N, T = 544, 40, 33
    p = problem(K, N, integer=True)
    x = p["x"].clone()
    x[3] = 0
    clean = run(p, x, out_dtype=torch.float32)
    for k in (5, 3 * 64 + 21, 512 + 9):
        for t, bad in ((0, float("inf")), (17, NAN), (32, float("-inf"))):
            xb = x.clone()
            xb[t, k] = bad
            got = run(p, xb, out_dtype=torch.float32)
            keep = torch.arange(T, device=DEV) != t
            assert bool(torch.isnan(got[t]).all()) and same_bits(got[keep], clean[keep]), (k, t)
    others = torch.arange(N, device=DEV) != 5
    for b in (1, 4 * 5 + 3, 33):
        for byte in (0x7F, 0xFF):
            sc = p["scales"].clone()
            sc[5, b] = byte
            got = run(p, x, out_dtype=torch.float32, scales=sc)
            assert bool(torch.isnan(got[:, 5]).all()) and same_bits(got[:, others], clean[:, others]), (b, byte)
        sc = p["scales"].clone()
        sc[5, b] |= 0x80
        got = run(p, x, out_dtype=torch.float32, scales=sc)
        assert torch.equal(got.cpu().double(), reference(x, p["blocks"], sc, p["bias"])), b
        assert not torch.equal(got[:, 5], clean[:, 5])

@pytest.mark.parametrize("kind", ["silu", "gelu_tanh", "swiglu_clamp"])
def test_gated_is_the_plain_op_on_its_own_hidden_rows(kind, hooks):
    """h from the grouped gated op on unit weights (code 2 = 1.0 on the diagonal under the byte 0x38): exact."""
    _, set_slices = hooks
    set_slices(4)
    K, N, T = 288, 40, 33
    p = problem(K, N)
    gate_up = torch.randn(T, 2 * K, generator=torch.Generator().manual_seed(13)).to(DEV)
    eye = torch.zeros(1, K, K, dtype=torch.uint8)
    eye[:, torch.arange(K), torch.arange(K)] = 2
    h = ops().moe_gated_forward_nvfp4(pack(eye).to(DEV), torch.full((1, K, K // 16), 0x38, dtype=torch.uint8, device=DEV), None,
                                      gate_up, None, None, out_dtype=torch.float32, **act_kw(kind))
    assert torch.equal(h, h.bfloat16().float()) and kernel_of(T, K, N) == (4, 2)
    for dout in (torch.float32, torch.bfloat16):
        got = ops().linear_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], gate_up, bias=p["bias"], out_dtype=dout,
                                               split_k=True, **act_kw(kind))
        assert same_bits(got, run(p, h.bfloat16(), out_dtype=dout)), (kind, dout)

@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_entry_stays_inside_its_buffers(dout, hooks):
    """S = 16 (eleven slices store zeros), guarded buffers, a misaligned row base (the element-load form), a stale workspace."""
    _, set_slices = hooks
    set_slices(16)
    T, N, K = 33, 40, 288
    p = problem(K, N)
    L = lib()
    rows = misaligned(p["x"], 1)
    want = run(p, rows, out_dtype=dout)
    assert rows.data_ptr() % 16 == 4 and kernel_of(T, K, N) == (16, 2)
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    out = Guarded("out", T * N * (4 if dout == torch.float32 else 2), dout, SENT, offset=4)
    nbytes = L.fql_linear_nvfp4_split_workspace_bytes(T, K, N, 0)
    ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
    for fill in (0xFF, 0x7F):
        ws.bytes().fill_(fill)
        out.view(dout, T, N).fill_(SENT)
        rc = L.fql_linear_nvfp4_split_fwd(bl.ptr, sc.ptr, p["gs"].data_ptr(), rows.data_ptr(), 0, bias.ptr, out.ptr, 0 if dout == torch.float32 else 2, T, K, N,
                                          ws.ptr, nbytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and nbytes == 64 * T * N
        assert_guards_intact(bl, sc, bias, out, ws, what=f"nvfp4 linear split {dout} workspace {fill:#04x}")
        got = out.view(dout, T, N)
        assert int((got == SENT).sum()) == 0 and same_bits(got, want), hex(fill)
        part = ws.bytes().view(torch.float32).view(16, T, N)                 # pairs in slices 0 .. 3, the odd piece in slice 15
        assert bool(torch.isfinite(part).all()) and torch.count_nonzero(part[4:15]) == 0, hex(fill)
        assert all(int(torch.count_nonzero(part[s])) > 0 for s in (0, 1, 2, 3, 15)), hex(fill)

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_forward_is_the_op_and_the_input_gradient_is_unchanged(dt, hooks):
    K, N = 288, 40
    p = problem(K, N)
    make = lambda **kw: fq().NVFP4Linear.from_nvfp4(p["blocks"], p["scales"], p["gs"], bias=p["bias"], input_grad=True, **kw)
    m, plain = make(split_k=True), make()
    x = p["x"][:32].reshape(2, 16, K).to(dt)
    grads = []
    for layer, split in ((m, True), (plain, False)):
        xg = x.clone().requires_grad_(True)
        y = layer(xg)
        assert same_bits(y.detach().reshape(32, N), run(p, x.reshape(32, K), split_k=split))
        y.backward(torch.ones_like(y))
        grads.append(xg.grad)
    assert kernel_of(32, K, N) == (4, 2) and same_bits(grads[0], grads[1])
