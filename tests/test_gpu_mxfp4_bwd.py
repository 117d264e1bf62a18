"""The input gradient of the MXFP4 expert weights on the GPU: ops.moe_backward_input_mxfp4 (csrc/fql_gemm_mx4_bwd.h),
MXFP4MoEFFN(input_grad=True) and QuantizedSparseMoEBlock with such experts under grad mode.

N is the contraction here.  N in {8, 40, 136, 201}: half of a 16-n step, a partial first stage, two stages plus an 8-n tail,
an odd N on the element-load path.  K in {32, 96, 288}: one 32-k piece, a partial 128-k tile, a third k tile of one piece.
The table is test_gpu_mxfp4.py's ([0, 1, 33, 70] rows plus 2 uncovered), and E = 1 with one row and no table.

MEASURED (MI355X; printed by the tests with -s) and the bounds:
  * float32 dX against the float64 product of the SAME bfloat16-rounded dY and the exactly dequantised weights, relative
    Frobenius error: 2.8e-8 .. 9.4e-8 over the twelve shapes (the largest, 9.367e-8, at K = 32, N = 201; the same for float32
    and bfloat16 dY); the bound asserted is the forward's own SAME_INPUT_BOUND = 2.64e-7 (the same instruction, the same
    accumulation, a contraction no longer than its 288).
  * a bfloat16 dX adds its one rounding (2^-9): measured 1.52e-3 .. 1.71e-3; a float16 one 2^-11: measured 2.1e-4.
  * against the UN-rounded float32 dY the error is the format's own (2^-9 an element): 1.57e-3 .. 1.94e-3, printed, not
    asserted.
  * the layer's and the block's gradients against float64 autograd on the dequantised weights (straight-through across
    the bfloat16 roundings of x and h): LAYER_MEASURED / BLOCK_MEASURED below (float32 layer: x 2.513e-3, gate_up_bias
    1.543e-3, down_bias 7.0e-8; bfloat16 layer: x 3.275e-3, gate_up_bias 2.386e-3, down_bias 0; block: x 2.202e-3,
    gate.weight 9.9e-8, gate.bias 1.41e-7); asserted at 4 x the largest, capped at 2^-6.
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden_autograd
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits
from test_gpu_mxfp4 import BF16_OUT, SAME_INPUT_BOUND, ffn_weights, pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 96, 288], [8, 40, 136, 201]
assert SAME_INPUT_BOUND == 4 * 6.6e-8

SAME_INPUT_MEASURED_BWD = 9.367e-8  # (K = 32, N = 201; 2.8e-8 .. 9.4e-8 over the twelve shapes)
assert SAME_INPUT_MEASURED_BWD <= SAME_INPUT_BOUND
# relative Frobenius error of x.grad / the bias gradients (layer) and of x.grad / gate.weight.grad / gate.bias.grad (block)
# against the float64 reference, the largest value printed on an MI355X per activation type; the error is the backward's
# own operand roundings to bfloat16 (gy and dgu, 2^-9 an element), in the bfloat16 layer also those of gate_up, dh and dgu
LAYER_MEASURED = {torch.float32: 2.513e-3, torch.bfloat16: 3.275e-3}      # (x.grad in both; the bias gradients are below it)
BLOCK_MEASURED = 2.202e-3                                                  # (x.grad; the gate's two are 1.4e-7 at most)
GRAD_CAP = 2.0 ** -6               # a lost GEMM or a wrong operand is of order 1


def grad_bound(measured):
    return min(4.0 * measured, GRAD_CAP)


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, lo=97, hi=157, integer=False, seed=0):
    """test_gpu_mxfp4.problem's construction for the transposed product: random element codes and scale codes in [lo, hi],
    dY randn or (``integer``) integers in [-4, 4].  ``ref``: float64, bf16(dY) @ W_e on the rows of expert e, zero on the
    rows no expert covers; ``ref_raw``: the same on the un-rounded dY.  Computed once per shape; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(1000 * K + N + seed)
    E = len(counts)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    gy = torch.randint(-4, 5, (T, N), generator=g).float() if integer else torch.randn(T, N, generator=g)
    gr = gy.bfloat16().double()
    ref, ref_raw = torch.zeros(T, K, dtype=torch.float64), torch.zeros(T, K, dtype=torch.float64)
    for e, (c, o) in enumerate(zip(tpe.tolist(), offs.tolist())):
        ref[o:o + c] = gr[o:o + c] @ W[e]
        ref_raw[o:o + c] = gy[o:o + c].double() @ W[e]
    return dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), gy=gy.to(DEV), tpe=tpe.to(DEV),
                offs=offs.to(DEV), ref=ref, ref_raw=ref_raw, W=W, counts=list(counts))


def run(p, gy=None, out_dtype=None, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_backward_input_mxfp4(a["blocks"], a["scales"], p["gy"] if gy is None else gy, a["tpe"], a["offs"],
                                          out_dtype=out_dtype)


# ---- the lane map of the transposed read, exactly

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din):
    """Integer gradients in [-4, 4], random codes, scale codes in [125, 129]: every product is a multiple of 2^-3 and
    |sum| <= 201 * 96 < 2^15, so the float32 dX is the integer reference bit for bit whatever the order.  The weights are
    asymmetric: a swapped operand, a wrong transposed-read lane, an unswizzled chunk or a scale on the wrong block fails."""
    p = problem(K, N, lo=125, hi=129, integer=True)
    ref = p["ref"]
    assert float(ref.abs().max()) < 2 ** 15 and bool((ref * 8 == (ref * 8).round()).all())
    got = run(p, p["gy"].to(din))
    assert got.dtype == torch.float32 and tuple(got.shape) == (p["T"], K)              # the default out_dtype
    assert torch.equal(got.cpu().double(), ref), (K, N)
    assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                               # uncovered rows: exactly zero
    got16 = run(p, p["gy"].to(din), out_dtype=torch.bfloat16)                          # one rounding of the exact value
    assert same_bits(got16.cpu(), ref.float().bfloat16())
    assert torch.count_nonzero(got16[p["T"] - TAIL:]) == 0


def test_exact_one_expert_one_row_no_table():
    p = problem(96, 40, counts=(1,), tail=0, lo=125, hi=129, integer=True)
    assert torch.equal(run(p).cpu().double(), p["ref"])
    assert torch.equal(run(p, tpe=None, offs=None).cpu().double(), p["ref"])


def test_empty_contraction_is_zeros_and_float16_is_refused():
    p = problem(96, 40)
    T, K = p["T"], p["K"]
    got = ops().moe_backward_input_mxfp4(p["blocks"][:, :0], p["scales"][:, :0], p["gy"][:, :0], p["tpe"], p["offs"])
    assert tuple(got.shape) == (T, K) and got.dtype == torch.float32 and torch.count_nonzero(got) == 0
    assert tuple(run(p, p["gy"][:0]).shape) == (0, K)
    with pytest.raises(RuntimeError, match="float16"):
        run(p, p["gy"].half())
    with pytest.raises(RuntimeError, match=r"\[T, N\]"):
        run(p, p["gy"][:, :-1])
    with pytest.raises(RuntimeError, match="CUDA"):
        run(p, blocks=p["blocks"].cpu())


# ---- random gradients

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_gradients_against_the_same_rounded_gradients(K, N):
    p = problem(K, N)
    for din in (torch.float32, torch.bfloat16):
        gy = p["gy"].to(din)
        e32 = rel_fro_dev(run(p, gy), p["ref"])
        e16 = rel_fro_dev(run(p, gy, out_dtype=torch.bfloat16), p["ref"])
        print(f"mxfp4 bwd K={K} N={N} in={din}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.2e}), "
              f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
        assert e32 <= SAME_INPUT_BOUND
        assert e16 <= SAME_INPUT_BOUND + BF16_OUT
    # the format's own error: against the gradients before their rounding to bfloat16 (recorded, not asserted)
    print(f"mxfp4 bwd K={K} N={N}: rel_fro against un-rounded float32 gradients {rel_fro_dev(run(p), p['ref_raw']):.3e}")


def test_float16_output():
    q = problem(32, 8, lo=125, hi=129)                                                 # (inside float16's range)
    got = run(q, out_dtype=torch.float16)
    err = rel_fro_dev(got, q["ref"])
    print(f"mxfp4 bwd float16 out: rel_fro {err:.3e} (bound {SAME_INPUT_BOUND + 2.0 ** -11:.3e})")
    assert got.dtype == torch.float16 and err <= SAME_INPUT_BOUND + 2.0 ** -11


# ---- independence, bit for bit

@pytest.mark.parametrize("K,N", [(288, 136), (96, 201)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N):
    p = problem(K, N)
    got = run(p)
    assert same_bits(got, run(p))                                                      # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_backward_input_mxfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gy"][o:o + c].contiguous(),
                                             torch.tensor([c], dtype=torch.int32, device=DEV),
                                             torch.zeros(1, dtype=torch.int32, device=DEV))
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_backward_input_mxfp4(p["blocks"][perm], p["scales"][perm], p["gy"], p["tpe"][perm], p["offs"][perm])
    assert same_bits(again, got)


# ---- non-finite values

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


def test_scale_code_255_is_nan_in_exactly_the_32_k_of_its_block():
    p = problem(96, 40)
    scales = p["scales"].clone()
    e, n, b = 2, 17, 1
    scales[e, n, b] = 255
    got, want = run(p, scales=scales), run(p)
    o, c = p["offs"].tolist()[e], p["counts"][e]
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[o:o + c, 32 * b:32 * b + 32] = True
    assert torch.equal(nan, expect)
    assert torch.equal(got[~expect], want[~expect])


# ---- footprint

@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [40, 201])
def test_entry_stays_inside_its_buffers(N, dout):
    """Every pointer is the interior of a guarded buffer; grad_in sits 4 bytes off a 16-byte boundary inside SENT and
    grad_out 4 bytes off one inside NaN.  Only [T, K] changes, the guards stay, uncovered rows are zero and the bits are
    the public op's."""
    from fused_int4_amd import _native
    lib = _native.lib()
    K = 96
    p = problem(K, N)
    E, T = p["E"], p["T"]
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    gy = guarded_like("grad_out", p["gy"], NAN, offset=4)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("grad_in", T * K * esz, dout, SENT, offset=4)
    out.view(dout, T, K).fill_(SENT)
    assert out.ptr % 16 == 4 and gy.ptr % 16 == 4
    rc = lib.fql_moe_mx4_bwd_input(bl.ptr, sc.ptr, gy.ptr, 0, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert_guards_intact(bl, sc, gy, cnt, off, out, what=f"mx4 bwd N={N} {dout}")
    got = out.view(dout, T, K)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, run(p, out_dtype=dout))


# ---- the layer

E_L, H_L, F_L = 4, 64, 96
KIND = "swiglu_clamp"


def ste(v):
    """v with a straight-through rounding to bfloat16 (float64 graph)."""
    return v + (v.detach().float().bfloat16().double() - v.detach())


def layer_reference(m, x, gy, tpe, offs):
    """float64 autograd on the dequantised weights of layer ``m``: (x.grad, gate_up_bias.grad, down_bias.grad)."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    Wgu = dequantize_mxfp4(m.gate_up_blocks.cpu(), m.gate_up_scales.cpu()).double()
    Wd = dequantize_mxfp4(m.down_blocks.cpu(), m.down_scales.cpu()).double()
    x64 = x.detach().cpu().double().requires_grad_(True)
    bgu = m.gate_up_bias.detach().cpu().double().requires_grad_(True)
    bd = m.down_bias.detach().cpu().double().requires_grad_(True)
    y = expert_rows64(Wgu, Wd, bgu, bd, x64, tpe.tolist(), offs.tolist())
    y.backward(gy.detach().cpu().double())
    return x64.grad, bgu.grad, bd.grad


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


def make_layer(dt, input_grad=True, seed=5):
    w = ffn_weights(E_L, H_L, F_L, seed=seed)
    return fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                         down_bias=w["down_bias"], activation_dtype=dt, input_grad=input_grad,
                                         **act_kw(KIND)).to(DEV)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_gradients_are_the_ops_composed_and_match_float64_autograd(dt):
    m = make_layer(dt)
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
    gate_up = ops().moe_forward_mxfp4(m.gate_up_blocks, m.gate_up_scales, x.detach(), tpe, offs,
                                      bias=m.gate_up_bias.detach(), out_dtype=dt)
    dh = ops().moe_backward_input_mxfp4(m.down_blocks, m.down_scales, gy, tpe, offs, out_dtype=dt)
    dgu = ops().glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
    dx = ops().moe_backward_input_mxfp4(m.gate_up_blocks, m.gate_up_scales, dgu, tpe, offs, out_dtype=dt)
    assert x.grad.dtype == dt and same_bits(x.grad, dx)
    assert same_bits(m.gate_up_bias.grad, ops().moe_bias_grad(dgu, E_L, tpe, offs))
    assert same_bits(m.down_bias.grad, ops().moe_bias_grad(gy, E_L, tpe, offs))
    assert torch.count_nonzero(x.grad[T - 2:]) == 0                                    # rows no expert covers
    # (b) float64 autograd on the dequantised weights
    rx, rbgu, rbd = layer_reference(m, x, gy, tpe, offs)
    errs = dict(x=rel_fro_dev(x.grad, rx), gate_up_bias=rel_fro_dev(m.gate_up_bias.grad, rbgu),
                down_bias=rel_fro_dev(m.down_bias.grad, rbd))
    bound = grad_bound(LAYER_MEASURED[dt])
    print(f"mxfp4 layer {dt}: rel_fro of the gradients against float64 autograd "
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
    xg = x.clone().requires_grad_(True)
    m(xg, tpe, offs).backward(gy)
    assert xg.grad is not None and m.gate_up_bias.grad is None
    frozen = make_layer(torch.float32, input_grad=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        frozen(x.clone().requires_grad_(True), tpe, offs)


# ---- the block

def test_block_trains_through_mxfp4_experts():
    """E = 4, top-2, H = 64, F = 96, swiglu_clamp, expert and router biases, T = 50, under grad mode.  Reference: float64
    autograd of a torch block on the dequantised weights, on the block's own indices."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    T, top_k = 50, 2
    experts = make_layer(torch.float32, seed=9)
    torch.manual_seed(13)                                                              # (the gate's initial weights)
    blk = fq().QuantizedSparseMoEBlock(E_L, H_L, F_L, top_k=top_k, experts=experts, router_bias=True).to(DEV)
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

    Wgu = dequantize_mxfp4(experts.gate_up_blocks.cpu(), experts.gate_up_scales.cpu()).double()
    Wd = dequantize_mxfp4(experts.down_blocks.cpu(), experts.down_scales.cpu()).double()
    bgu, bd = experts.gate_up_bias.detach().cpu().double(), experts.down_bias.detach().cpu().double()
    x64 = x.detach().cpu().double().requires_grad_(True)
    Wg = blk.gate.weight.detach().cpu().double().requires_grad_(True)
    bg = blk.gate.bias.detach().cpu().double().requires_grad_(True)
    probs = torch.softmax(x64 @ Wg.T + bg, dim=-1)
    w = probs.gather(1, indices)
    w = w / w.sum(dim=-1, keepdim=True)                                                # renormalize=True (Mixtral)
    ref = torch.zeros(T, H_L, dtype=torch.float64)
    for j in range(top_k):
        order = torch.argsort(indices[:, j], stable=True)
        counts = torch.bincount(indices[:, j], minlength=E_L).tolist()
        offsets = [sum(counts[:e]) for e in range(E_L)]
        y = expert_rows64(Wgu, Wd, bgu, bd, x64[order], counts, offsets)
        ref = ref + torch.zeros_like(ref).index_add(0, order, y * w[order, j:j + 1])
    err_out = rel_fro_dev(out.detach(), ref.detach())
    ref.backward(gout.cpu().double())
    errs = dict(x=rel_fro_dev(x.grad, x64.grad), gate_weight=rel_fro_dev(blk.gate.weight.grad, Wg.grad),
                gate_bias=rel_fro_dev(blk.gate.bias.grad, bg.grad))
    bound = grad_bound(BLOCK_MEASURED)
    print(f"mxfp4 block under grad: forward rel_fro {err_out:.3e}; gradients against float64 autograd "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {bound:.3e})")
    for k, v in errs.items():
        assert v <= bound, k
