"""The input gradient of the NVFP4 weights on the GPU: ops.moe_backward_input_nvfp4 / ops.linear_backward_input_nvfp4
(csrc/fql_gemm_nvfp4_bwd.h), NVFP4MoEFFN(input_grad=True), NVFP4Linear(input_grad=True) and QuantizedSparseMoEBlock with such
experts under grad mode.

N is the contraction here.  N in {8, 40, 136, 201}: half of a 16-n step, a partial first stage, two stages plus an 8-n tail,
an odd N on the element-load path; N in {64, 128}: exactly one and exactly two 64-n stages, the two sizes at which
``n0 + BN < N`` and ``n0 + 2 * BN < N`` of nv4_bwd_kernel change value with no partial stage behind them (at 64 the second
Stage is never read and nothing is stored behind the one contraction).  K in {32, 96, 288}: one 32-k piece (two scale blocks),
a partial 128-k tile, a third k tile of one piece; K in {128, 384}: one and three WHOLE 128-k output tiles (no piece of the
last tile is absent).  The table is test_gpu_nvfp4.py's ([0, 1, 33, 70] rows plus 2 uncovered), and E = 1 with one row and no
table.  The weights, scale bytes and global scales come from test_gpu_nvfp4.problem (the scale bytes are drawn per
16-block: the two halves of a staging thread's 32-k piece differ).

The reference is float64 on the CPU: bf16(dY) @ W_e with W_e = dequantize_nvfp4 WITHOUT the global scale, rounded to float32,
then the one float32 step * global_scale[e].

MEASURED (MI355X; printed by the tests with -s) and the bounds:
  * float32 dX on Gaussian dY, scale bytes over the whole finite range and both signs, against that reference, relative
    Frobenius error: 1.4e-8 .. 9.9e-8 over the thirty shapes and both dY types (SAME_INPUT_MEASURED_BWD: 9.912e-8 at K = 288,
    N = 201, float32 dY; K in {128, 384} and N in {64, 128} measure 2.8e-8 .. 9.8e-8); the bound asserted is the forward's
    own SAME_INPUT_BOUND = 3.92e-7, imported (the same instruction, the same accumulation, a contraction no longer than its 288).
  * a bfloat16 dX adds its one rounding, 2^-9 (a bound on every finite normal element, hence on the norm): measured
    1.59e-3 .. 1.68e-3; a float16 dX 2^-11, taken on scale bytes 0x30 .. 0x47 (the whole range leaves float16's): measured
    2.05e-4 (K = 96, N = 40) and 2.08e-4 (K = 288, N = 201).
  * against the UN-rounded float32 dY the error is the format's own (2^-9 an element): 1.46e-3 .. 1.73e-3, printed, not
    asserted.
  * the layer's and the block's gradients against float64 autograd on the dequantised weights x global scale
    (straight-through across the bfloat16 roundings of x and h): LAYER_MEASURED / BLOCK_MEASURED below (float32 layer:
    x 2.356e-3, gate_up_bias 1.499e-3, down_bias 7.0e-8; bfloat16 layer: x 3.154e-3, gate_up_bias 2.492e-3, down_bias 0;
    block: forward 8.9e-8, x 2.164e-3, gate.weight 1.26e-7, gate.bias 2.96e-7); asserted at 4 x the largest, capped at 2^-6
    (the error is the backward's own 2^-9 operand roundings; a lost GEMM is of order 1).
  * NVFP4Linear's x.grad against the float64 definition: 0 (a [15, 40] gradient; asserted at SAME_INPUT_BOUND).
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden_autograd
from helpers import (NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, hostile_table, ops, rel_fro_dev,
                     same_bits, uncovered_mask)
from test_gpu_nvfp4 import BF16_OUT, NARROW, SAME_INPUT_BOUND, ffn_weights, global_scales, pack
from test_gpu_nvfp4 import problem as weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 96, 128, 288, 384], [8, 40, 64, 128, 136, 201]
F16_OUT = 2.0 ** -11

# relative Frobenius error of the float32 dX against the reference above: the largest value the tests printed on an MI355X
SAME_INPUT_MEASURED_BWD = 9.912e-8  # (K = 288, N = 201, float32 dY; 1.4e-8 .. 9.9e-8 over the thirty shapes)
assert SAME_INPUT_MEASURED_BWD <= SAME_INPUT_BOUND
# relative Frobenius error of x.grad / the bias gradients (layer) and of x.grad / gate.weight.grad / gate.bias.grad (block)
# against the float64 reference, the largest value printed on an MI355X per activation type
LAYER_MEASURED = {torch.float32: 2.356e-3, torch.bfloat16: 3.154e-3}      # (x.grad in both; the bias gradients are below it)
BLOCK_MEASURED = 2.164e-3                                                  # (x.grad; the gate's two are 3.0e-7 at most)
GRAD_CAP = 2.0 ** -6               # a lost GEMM or a wrong operand is of order 1


def grad_bound(measured):
    return min(4.0 * measured, GRAD_CAP)


def lib():
    from fused_int4_amd import _native
    return _native.lib()


def reference(gy, W, gs, ranges, T):
    """(ref, acc) float64 [T, K]: acc = bf16(dY) @ W_e on the rows of expert e, ref = fl32(fl32(acc) * gs[e]); zero on the
    rows no expert covers."""
    K = W.shape[2]
    gr = gy.bfloat16().double()
    ref, acc = torch.zeros(T, K, dtype=torch.float64), torch.zeros(T, K, dtype=torch.float64)
    for e, (lo, hi) in enumerate(ranges):
        if hi > lo:
            acc[lo:hi] = gr[lo:hi] @ W[e]
            ref[lo:hi] = (acc[lo:hi].float() * gs[e]).double()
    return ref, acc


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, scale_range=None, integer=False):
    """test_gpu_nvfp4.problem's weights (random codes; scale bytes over the whole finite range and both signs, or in
    ``scale_range``, drawn per 16-block; a power-of-two global scale per expert) with a gradient dY [T, N]: randn, or
    (``integer``) integers in [-4, 4].  ``ref_raw``: the reference on the un-rounded dY.  Computed once; nobody writes to it."""
    w = weights(K, N, counts=counts, tail=tail, scale_range=scale_range, integer=integer)
    g = torch.Generator().manual_seed(7000 * K + N)
    T, E = w["T"], w["E"]
    gy = torch.randint(-4, 5, (T, N), generator=g).float() if integer else torch.randn(T, N, generator=g)
    tpe, offs = w["tpe"].cpu(), w["offs"].cpu()
    ranges = [(o, o + c) for c, o in zip(tpe.tolist(), offs.tolist())]
    gs = w["gs"].cpu()
    ref, acc = reference(gy, w["W"], gs, ranges, T)
    ref_raw = torch.zeros_like(ref)
    for e, (lo, hi) in enumerate(ranges):
        ref_raw[lo:hi] = (gy[lo:hi].double() @ w["W"][e]) * float(gs[e])
    return dict(E=E, T=T, K=K, N=N, blocks=w["blocks"], scales=w["scales"], gs=w["gs"], gy=gy.to(DEV), tpe=w["tpe"],
                offs=w["offs"], ref=ref, acc=acc, ref_raw=ref_raw, W=w["W"], counts=list(counts), ranges=ranges)


def run(p, gy=None, out_dtype=None, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], gs=p["gs"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_backward_input_nvfp4(a["blocks"], a["scales"], a["gs"], p["gy"] if gy is None else gy, a["tpe"], a["offs"],
                                          out_dtype=out_dtype)


# ---- 1. the lane map of the transposed read and the scale of each rotated dword, exactly

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din):
    """Integer gradients in [-4, 4], random codes, scale bytes 0x30 .. 0x47 (0.5 .. 3.75), a different power-of-two global
    scale per expert: every product is a multiple of 2^-5, |W| <= 6 x 3.75 = 22.5 and |sum| <= 201 x 4 x 22.5 = 18090 < 2^15,
    below 2^20 units: the float32 dX is the float64 reference bit for bit in any order, the bfloat16 dX its one rounding.
    The scale bytes are drawn per 16-block, so a scale applied to the wrong half of a rotated piece fails, as does a wrong
    transposed-read lane, an unswizzled chunk or a neighbour's global scale."""
    p = problem(K, N, scale_range=NARROW, integer=True)
    ref, acc = p["ref"], p["acc"]
    assert float(acc.abs().max()) < 2 ** 15 and bool((acc * 32 == (acc * 32).round()).all())
    assert bool((p["scales"][:, :, 0::2] != p["scales"][:, :, 1::2]).any())            # a piece's two halves differ
    got = run(p, p["gy"].to(din))
    assert got.dtype == torch.float32 and tuple(got.shape) == (p["T"], K)              # the default out_dtype
    assert torch.equal(got.cpu().double(), ref), (K, N)
    assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                               # uncovered rows: exactly zero
    got16 = run(p, p["gy"].to(din), out_dtype=torch.bfloat16)                          # one rounding of the exact value
    assert same_bits(got16.cpu(), ref.float().bfloat16())
    assert torch.count_nonzero(got16[p["T"] - TAIL:]) == 0
    none = run(p, p["gy"].to(din), gs=None)                                            # no global scale: acc itself
    assert torch.equal(none.cpu().double(), acc)


def test_exact_one_expert_one_row_no_table():
    p = problem(96, 40, counts=(1,), tail=0, scale_range=NARROW, integer=True)
    assert torch.equal(run(p).cpu().double(), p["ref"])
    assert torch.equal(run(p, tpe=None, offs=None).cpu().double(), p["ref"])
    dense = ops().linear_backward_input_nvfp4(p["blocks"][0], p["scales"][0], p["gs"], p["gy"])
    assert torch.equal(dense.cpu().double(), p["ref"])


# ---- 2. random gradients

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_gradients_against_the_same_rounded_gradients(K, N):
    p = problem(K, N)
    for din in (torch.float32, torch.bfloat16):
        gy = p["gy"].to(din)
        e32 = rel_fro_dev(run(p, gy), p["ref"])
        e16 = rel_fro_dev(run(p, gy, out_dtype=torch.bfloat16), p["ref"])
        print(f"nvfp4 bwd K={K} N={N} in={din}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.2e}), "
              f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
        assert e32 <= SAME_INPUT_BOUND
        assert e16 <= SAME_INPUT_BOUND + BF16_OUT
    # the format's own error: against the gradients before their rounding to bfloat16 (recorded, not asserted)
    print(f"nvfp4 bwd K={K} N={N}: rel_fro against un-rounded float32 gradients {rel_fro_dev(run(p), p['ref_raw']):.3e}")


@pytest.mark.parametrize("K,N", [(96, 40), (288, 201)])
def test_float16_output(K, N):
    q = problem(K, N, scale_range=NARROW)                                              # (inside float16's range)
    assert float(q["ref"].abs().max()) < 65504
    got = run(q, out_dtype=torch.float16)
    err = rel_fro_dev(got, q["ref"])
    print(f"nvfp4 bwd float16 out K={K} N={N}: rel_fro {err:.3e} (bound {SAME_INPUT_BOUND + F16_OUT:.3e})")
    assert got.dtype == torch.float16 and err <= SAME_INPUT_BOUND + F16_OUT


# ---- 3. independence, bit for bit

@pytest.mark.parametrize("K,N", [(288, 136), (96, 201), (128, 64), (384, 128)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N):
    p = problem(K, N)
    got = run(p)
    assert same_bits(got, run(p))                                                      # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_backward_input_nvfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gs"][e:e + 1],
                                             p["gy"][o:o + c].contiguous(), torch.tensor([c], dtype=torch.int32, device=DEV),
                                             torch.zeros(1, dtype=torch.int32, device=DEV))
        assert same_bits(one, got[o:o + c]), e
        bare = ops().moe_backward_input_nvfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gs"][e:e + 1],
                                              p["gy"][o:o + c].contiguous(), None, None)   # E = 1 without the table
        assert same_bits(bare, one), e
        dense = ops().linear_backward_input_nvfp4(p["blocks"][e], p["scales"][e], p["gs"][e:e + 1], p["gy"][o:o + c].contiguous())
        assert same_bits(dense, one), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_backward_input_nvfp4(p["blocks"][perm], p["scales"][perm], p["gs"][perm], p["gy"], p["tpe"][perm],
                                           p["offs"][perm])
    assert same_bits(again, got)


@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_no_global_scale_equals_ones(dout):
    p = problem(288, 136)
    assert same_bits(run(p, gs=None, out_dtype=dout), run(p, gs=torch.ones_like(p["gs"]), out_dtype=dout))


# ---- 4. non-finite values and refusals

@pytest.mark.parametrize("byte", [0x7F, 0xFF])
def test_nan_scale_byte_is_nan_in_exactly_the_16_k_of_its_block(byte):
    """The byte sits in the SECOND 16-block of a staging piece (k 48 .. 63 of piece 1): the first half of that piece and
    every other column stay the bits they were."""
    p = problem(96, 40)
    scales = p["scales"].clone()
    e, n, b = 2, 17, 3
    scales[e, n, b] = byte
    got, want = run(p, scales=scales), run(p)
    o, c = p["offs"].tolist()[e], p["counts"][e]
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[o:o + c, 16 * b:16 * b + 16] = True
    assert torch.equal(nan, expect)
    assert torch.equal(got[~expect], want[~expect])


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_inf_and_nan_gradients_are_nan_across_exactly_their_rows(din):
    p = problem(288, 136)
    gy = p["gy"].to(din).clone()
    t_inf = p["offs"].tolist()[3] + 40                                                 # a row of the second 32-row wave
    t_nan = p["offs"].tolist()[2] + 5
    gy[t_inf, 101] = float("inf")
    gy[t_nan, 7] = NAN
    got, want = run(p, gy), run(p, p["gy"].to(din))
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[t_inf] = True
    expect[t_nan] = True
    assert torch.equal(nan, expect)
    assert same_bits(got[~expect], want[~expect])


def test_negative_scale_byte_negates_its_contribution_exactly():
    """Integer data (every sum exact): flipping the sign bit of every scale byte of one 16-block column of expert e negates
    dX on those 16 k for its rows, and nothing else moves."""
    p = problem(96, 40, scale_range=NARROW, integer=True)
    e, b = 3, 3
    scales = p["scales"].clone()
    scales[e, :, b] |= 0x80
    got, want = run(p, scales=scales), run(p)
    o, c = p["offs"].tolist()[e], p["counts"][e]
    flipped = want.clone()
    flipped[o:o + c, 16 * b:16 * b + 16] *= -1.0
    assert torch.equal(got, flipped) and bool((want[o:o + c, 16 * b:16 * b + 16] != 0).any())


def test_empty_contraction_is_zeros_and_float16_is_refused():
    p = problem(96, 40)
    T, K = p["T"], p["K"]
    got = ops().moe_backward_input_nvfp4(p["blocks"][:, :0], p["scales"][:, :0], p["gs"], p["gy"][:, :0], p["tpe"], p["offs"])
    assert tuple(got.shape) == (T, K) and got.dtype == torch.float32 and torch.count_nonzero(got) == 0
    assert tuple(run(p, p["gy"][:0]).shape) == (0, K)
    with pytest.raises(RuntimeError, match="float16"):
        run(p, p["gy"].half())
    with pytest.raises(RuntimeError, match=r"\[T, N\]"):
        run(p, p["gy"][:, :-1])
    with pytest.raises(RuntimeError, match="CUDA"):
        run(p, blocks=p["blocks"].cpu())


# ---- 5. footprint

@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(96, 40), (96, 201), (288, 40), (288, 201), (128, 64)])
def test_entry_stays_inside_its_buffers(K, N, din, dout):
    """Every pointer is the interior of a guarded buffer; grad_in sits 4 bytes off a 16-byte boundary inside SENT and
    grad_out 4 bytes off one inside NaN; the scale bytes start at an odd address and end exactly at their last byte in
    front of 0xFF (a NaN scale): the two-byte scale load must not reach past [E][N][K / 16]; global_scale is followed by
    NaN.  Only [T, K] changes, the guards stay, uncovered rows are zero, the bits are the public op's and no NaN (no guard
    element served as an operand)."""
    p = problem(K, N, scale_range=NARROW)
    E, T = p["E"], p["T"]
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    gs = guarded_like("global_scale", p["gs"], NAN)
    gy = guarded_like("grad_out", p["gy"].to(din), NAN, offset=4)               # (both element types: vector and element loads)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("grad_in", T * K * esz, dout, SENT, offset=4)
    out.view(dout, T, K).fill_(SENT)
    assert out.ptr % 16 == 4 and gy.ptr % 16 == 4 and sc.ptr % 2 == 1
    rc = lib().fql_moe_nvfp4_bwd_input(bl.ptr, sc.ptr, gs.ptr, gy.ptr, DT[din], cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert_guards_intact(bl, sc, gs, gy, cnt, off, out, what=f"nvfp4 bwd K={K} N={N} {din}->{dout}")
    got = out.view(dout, T, K)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, run(p, p["gy"].to(din), out_dtype=dout))
    assert not bool(torch.isnan(got.float()).any())


# ---- 6. hostile expert tables

@functools.lru_cache(maxsize=None)
def table_problem(table, K=96, N=40):
    """The integer recipe on one of helpers.hostile_table's tables; the rows no expert covers are NaN in the gradient."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    tpe, offs, T, ranges = hostile_table(table)
    E = tpe.numel()
    g = torch.Generator().manual_seed(E + T)
    blocks = pack(torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8))
    scales = torch.randint(NARROW[0], NARROW[1] + 1, (E, N, K // 16), generator=g, dtype=torch.uint8)
    W = dequantize_nvfp4(blocks, scales).double()
    gs = global_scales(E)
    gy = torch.randint(-4, 5, (T, N), generator=g).float()
    ref, acc = reference(gy, W, gs, ranges, T)
    assert float(acc.abs().max()) < 2 ** 15
    unc = uncovered_mask(ranges, T)
    gy[unc] = NAN
    return dict(T=T, unc=unc, ref=ref, args=(blocks.to(DEV), scales.to(DEV), gs.to(DEV), gy.to(DEV), tpe.to(DEV), offs.to(DEV)))


@pytest.mark.parametrize("table", ["e65", "e130-descending", "clipped", "all-empty"])
def test_hostile_tables_exactly(table):
    p = table_problem(table)
    for dout in (torch.float32, torch.bfloat16):
        got = ops().moe_backward_input_nvfp4(*p["args"], out_dtype=dout)
        assert same_bits(got.cpu(), p["ref"].float().to(dout)), (table, dout)
        assert torch.count_nonzero(got.cpu()[p["unc"]]) == 0


# ---- 7. layers and block

E_L, H_L, F_L = 4, 64, 96
KIND = "swiglu_clamp"


def ste(v):
    """v with a straight-through rounding to bfloat16 (float64 graph)."""
    return v + (v.detach().float().bfloat16().double() - v.detach())


def dequantized(m):
    """(W_gate_up, W_down) float64 [E, N, K] of layer ``m``: dequantize_nvfp4 x the global scale."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    Wgu = dequantize_nvfp4(m.gate_up_blocks.cpu(), m.gate_up_scales.cpu()).double() * m.gate_up_global.cpu().double()[:, None, None]
    Wd = dequantize_nvfp4(m.down_blocks.cpu(), m.down_scales.cpu()).double() * m.down_global.cpu().double()[:, None, None]
    return Wgu, Wd


def expert_rows64(Wgu, Wd, bgu, bd, rows, counts, offsets):
    """The experts' output [T, H] in float64 (a graph): rows [o, o + c) belong to expert e (ascending, disjoint), the
    others are zero; x and h pass a straight-through rounding to bfloat16."""
    F, H = Wd.shape[2], Wd.shape[1]
    pieces, pos = [], 0
    for e, (c, o) in enumerate(zip(counts, offsets)):
        if c == 0:
            continue
        assert o >= pos
        pieces.append(torch.zeros(o - pos, H, dtype=torch.float64))
        gu = ste(rows[o:o + c]) @ Wgu[e].T + bgu[e]
        h = hidden_autograd(KIND, gu[:, :F], gu[:, F:], ALPHA, LIMIT)
        pieces.append(ste(h) @ Wd[e].T + bd[e])
        pos = o + c
    pieces.append(torch.zeros(rows.shape[0] - pos, H, dtype=torch.float64))
    return torch.cat(pieces)


def make_layer(dt, input_grad=True, seed=5, E=E_L, F=F_L):
    w = ffn_weights(E, H_L, F, seed=seed)
    return fq().NVFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                         down_bias=w["down_bias"], activation_dtype=dt, input_grad=input_grad,
                                         **act_kw(KIND)).to(DEV)


def hand_backward(m, x, gy, tpe, offs):
    """(dx, dgu): the layer's backward composed by hand from the four ops, every tensor in x's type."""
    dt = x.dtype
    gate_up = ops().moe_forward_nvfp4(m.gate_up_blocks, m.gate_up_scales, m.gate_up_global, x.detach(), tpe, offs,
                                      bias=m.gate_up_bias.detach(), out_dtype=dt)
    dh = ops().moe_backward_input_nvfp4(m.down_blocks, m.down_scales, m.down_global, gy, tpe, offs, out_dtype=dt)
    dgu = ops().glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
    return ops().moe_backward_input_nvfp4(m.gate_up_blocks, m.gate_up_scales, m.gate_up_global, dgu, tpe, offs, out_dtype=dt), dgu


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_gradients_are_the_ops_composed_and_match_float64_autograd(dt):
    m = make_layer(dt)
    assert not torch.equal(m.gate_up_global, torch.ones_like(m.gate_up_global))        # (the global scales are in play)
    m.gate_up_bias.requires_grad_(True)
    m.down_bias.requires_grad_(True)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(T, H_L, generator=g).to(DEV).to(dt).requires_grad_(True)
    gy = torch.randn(T, H_L, generator=g).to(DEV).to(dt)
    with torch.no_grad():
        want_y = m(x.detach(), tpe, offs)
    y = m(x, tpe, offs)
    assert y.dtype == dt and y.requires_grad and same_bits(y.detach(), want_y)         # the forward's bits do not change
    y.backward(gy)
    # (a) the hand composition, bit for bit
    dx, dgu = hand_backward(m, x, gy, tpe, offs)
    assert x.grad.dtype == dt and same_bits(x.grad, dx)
    assert same_bits(m.gate_up_bias.grad, ops().moe_bias_grad(dgu, E_L, tpe, offs))
    assert same_bits(m.down_bias.grad, ops().moe_bias_grad(gy, E_L, tpe, offs))
    assert torch.count_nonzero(x.grad[T - 2:]) == 0                                    # rows no expert covers
    # (b) float64 autograd on the dequantised weights x global scale
    Wgu, Wd = dequantized(m)
    x64 = x.detach().cpu().double().requires_grad_(True)
    bgu = m.gate_up_bias.detach().cpu().double().requires_grad_(True)
    bd = m.down_bias.detach().cpu().double().requires_grad_(True)
    expert_rows64(Wgu, Wd, bgu, bd, x64, tpe.tolist(), offs.tolist()).backward(gy.detach().cpu().double())
    errs = dict(x=rel_fro_dev(x.grad, x64.grad), gate_up_bias=rel_fro_dev(m.gate_up_bias.grad, bgu.grad),
                down_bias=rel_fro_dev(m.down_bias.grad, bd.grad))
    bound = grad_bound(LAYER_MEASURED[dt])
    print(f"nvfp4 layer {dt}: rel_fro of the gradients against float64 autograd "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {bound:.3e})")
    for k, v in errs.items():
        assert v <= bound, k


def test_a_frozen_bias_gets_no_gradient_and_input_grad_false_still_raises():
    m = make_layer(torch.float32)
    m.down_bias.requires_grad_(True)                                                   # gate_up_bias stays frozen
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(T, H_L, generator=g).to(DEV)
    gy = torch.randn(T, H_L, generator=g).to(DEV)
    y = m(x, tpe, offs)                                                                # the input wants none: a bias alone
    assert y.requires_grad
    y.backward(gy)
    assert m.gate_up_bias.grad is None and x.grad is None
    assert same_bits(m.down_bias.grad, ops().moe_bias_grad(gy, E_L, tpe, offs))
    m.down_bias.requires_grad_(False)
    assert not m(x, tpe, offs).requires_grad                                           # nothing wants a gradient: the plain ops
    frozen = make_layer(torch.float32, input_grad=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        frozen(x.clone().requires_grad_(True), tpe, offs)


def test_linear_layer_input_gradient_on_3d_input_with_a_bias():
    lin = torch.nn.Linear(96, 40)
    m = fq().NVFP4Linear.from_linear(lin, input_grad=True).to(DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 5, 96, generator=g).to(DEV).requires_grad_(True)
    gy = torch.randn(3, 5, 40, generator=g).to(DEV)
    with torch.no_grad():
        want_y = m(x.detach())
    y = m(x)
    assert y.shape == (3, 5, 40) and y.requires_grad and same_bits(y.detach(), want_y)
    y.backward(gy)
    want = ops().linear_backward_input_nvfp4(m.blocks, m.scales, m.global_scale, gy.reshape(15, 40))
    assert x.grad.shape == (3, 5, 96) and same_bits(x.grad.reshape(15, 96), want)
    from fused_int4_amd.quantize import dequantize_nvfp4
    W = dequantize_nvfp4(m.blocks.cpu(), m.scales.cpu()).double()
    ref = ((gy.reshape(15, 40).cpu().bfloat16().double() @ W).float() * m.global_scale.cpu()).double()
    err = rel_fro_dev(want, ref)
    print(f"nvfp4 linear layer: rel_fro of x.grad against the float64 definition {err:.3e} (bound {SAME_INPUT_BOUND:.1e})")
    assert err <= SAME_INPUT_BOUND
    xb = x.detach().bfloat16().requires_grad_(True)
    m(xb).backward(gy.bfloat16())
    assert xb.grad.dtype == torch.bfloat16
    assert same_bits(xb.grad.reshape(15, 96), ops().linear_backward_input_nvfp4(m.blocks, m.scales, m.global_scale,
                                                                                gy.bfloat16().reshape(15, 40),
                                                                                out_dtype=torch.bfloat16))
    plain = fq().NVFP4Linear.from_linear(lin).to(DEV)
    with pytest.raises(RuntimeError, match="inference-only"):
        plain(x.detach().requires_grad_(True))


class _HandFFN(torch.autograd.Function):
    """The experts' node written out: the layer's own forward, and hand_backward's four ops as the backward."""

    @staticmethod
    def forward(ctx, rows, tpe, offs, m):
        ctx.save_for_backward(rows, tpe, offs)
        ctx.m = m
        with torch.no_grad():
            return m(rows.detach(), tpe, offs)

    @staticmethod
    def backward(ctx, gy):
        rows, tpe, offs = ctx.saved_tensors
        return hand_backward(ctx.m, rows, gy.contiguous(), tpe, offs)[0], None, None, None


def composed_block(blk, x):
    """QuantizedSparseMoEBlock.forward written out with the public ops, the two expert layers replaced by _HandFFN."""
    x2 = x.reshape(-1, blk.hidden_dim)
    logits = blk.router_logits(x2)
    weights, indices, *_ = ops().router_score_topk(logits, blk.top_k, blk.scoring, blk.selection_bias, blk.n_group,
                                                   blk.topk_group, blk.group_top, blk.renormalize, blk.routed_scaling_factor,
                                                   return_scores=True)
    tpe, offs, token_of_sorted, pos_of_slot = ops().route_plan(indices, blk.num_experts)
    rows = ops().dispatch_rows(x2, token_of_sorted, pos_of_slot, blk.top_k)
    y = _HandFFN.apply(rows, tpe, offs, blk.experts)
    T = x2.shape[0]
    s = _HandFFN.apply(x2, torch.full((1,), T, dtype=torch.int32, device=x2.device),
                       torch.zeros(1, dtype=torch.int32, device=x2.device), blk.shared_experts)
    return ops().combine_any(y, pos_of_slot, weights, addend=s, addend_weight=None, out_dtype=x.dtype).reshape(x.shape)


def test_block_trains_through_nvfp4_experts_and_a_shared_expert():
    """E = 4, top-2, H = 64, F = 96, swiglu_clamp, expert and router biases, an NVFP4 shared expert, T = 50, under grad
    mode.  x.grad and the gate's gradients equal the written-out composition bit for bit; the reference is float64 autograd
    of a torch block on the dequantised weights x global scale, on the block's own indices."""
    T, top_k = 50, 2
    experts, shared = make_layer(torch.float32, seed=9), make_layer(torch.float32, seed=10, E=1, F=32)
    torch.manual_seed(13)                                                              # (the gate's initial weights)
    blk = fq().QuantizedSparseMoEBlock(E_L, H_L, F_L, top_k=top_k, experts=experts, shared_experts=shared, router_bias=True).to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H_L, generator=g).to(DEV).requires_grad_(True)
    gout = torch.randn(T, H_L, generator=g).to(DEV)
    with torch.no_grad():
        blk.gate.bias.copy_((torch.randn(E_L, generator=g) * 0.1).to(DEV))
        want_out, _ = blk(x.detach())
    out, logits = blk(x)
    assert same_bits(out.detach(), want_out)                                           # the forward's bits do not change
    indices = blk.routing[2].cpu().long()
    out.backward(gout)
    grads = dict(x=x.grad, gate_weight=blk.gate.weight.grad, gate_bias=blk.gate.bias.grad)
    for k, v in grads.items():
        assert v is not None and bool(torch.isfinite(v).all()), k
    # (a) the composition, bit for bit
    xc = x.detach().clone().requires_grad_(True)
    blk.gate.weight.grad, blk.gate.bias.grad = None, None
    outc = composed_block(blk, xc)
    assert same_bits(outc.detach(), want_out)
    outc.backward(gout)
    assert same_bits(xc.grad, grads["x"])
    assert same_bits(blk.gate.weight.grad, grads["gate_weight"]) and same_bits(blk.gate.bias.grad, grads["gate_bias"])
    # (b) float64 autograd
    Wgu, Wd = dequantized(experts)
    Sgu, Sd = dequantized(shared)
    bgu, bd = experts.gate_up_bias.detach().cpu().double(), experts.down_bias.detach().cpu().double()
    sbgu, sbd = shared.gate_up_bias.detach().cpu().double(), shared.down_bias.detach().cpu().double()
    x64 = x.detach().cpu().double().requires_grad_(True)
    Wg = blk.gate.weight.detach().cpu().double().requires_grad_(True)
    bg = blk.gate.bias.detach().cpu().double().requires_grad_(True)
    probs = torch.softmax(x64 @ Wg.T + bg, dim=-1)
    w = probs.gather(1, indices)
    w = w / w.sum(dim=-1, keepdim=True)                                                # renormalize=True (Mixtral)
    ref = expert_rows64(Sgu, Sd, sbgu, sbd, x64, [T], [0])                             # the shared expert: every token, weight 1
    for j in range(top_k):
        order = torch.argsort(indices[:, j], stable=True)
        counts = torch.bincount(indices[:, j], minlength=E_L).tolist()
        offsets = [sum(counts[:e]) for e in range(E_L)]
        y = expert_rows64(Wgu, Wd, bgu, bd, x64[order], counts, offsets)
        ref = ref + torch.zeros_like(ref).index_add(0, order, y * w[order, j:j + 1])
    err_out = rel_fro_dev(out.detach(), ref.detach())
    ref.backward(gout.cpu().double())
    errs = dict(x=rel_fro_dev(grads["x"], x64.grad), gate_weight=rel_fro_dev(grads["gate_weight"], Wg.grad),
                gate_bias=rel_fro_dev(grads["gate_bias"], bg.grad))
    bound = grad_bound(BLOCK_MEASURED)
    print(f"nvfp4 block under grad: forward rel_fro {err_out:.3e}; gradients against float64 autograd "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {bound:.3e})")
    for k, v in errs.items():
        assert v <= bound, k


def test_graph_capture_of_the_backward_and_replay_under_a_changed_table():
    """One capture of the op at T = 5 (warmed up on a side stream), one replay after the table's contents and the gradient
    changed in place: the replay is the eager result of the new state, bit for bit, and not the captured one's."""
    p = problem(96, 40)
    g = torch.Generator().manual_seed(17)
    gy = torch.randn(5, 40, generator=g).to(DEV)
    tpe = torch.tensor([2, 0, 1, 2], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, 2, 2, 3], dtype=torch.int32, device=DEV)
    call = lambda: ops().moe_backward_input_nvfp4(p["blocks"], p["scales"], p["gs"], gy, tpe, offs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call()
    first = call().clone()
    tpe.copy_(torch.tensor([0, 3, 1, 0], dtype=torch.int32, device=DEV))               # one row is left uncovered
    offs.copy_(torch.tensor([0, 1, 0, 4], dtype=torch.int32, device=DEV))
    gy.copy_(torch.randn(5, 40, generator=g).to(DEV))
    out.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    eager = call()
    assert same_bits(out, eager) and not same_bits(eager, first)
    assert torch.count_nonzero(eager[4]) == 0 and torch.count_nonzero(eager[:4]) > 0
