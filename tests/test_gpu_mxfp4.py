"""OCP MXFP4 expert weights on the GPU: ops.moe_forward_mxfp4 / ops.moe_gated_forward_mxfp4 (csrc/fql_gemm_mx4.h), the
layer MXFP4MoEFFN and QuantizedSparseMoEBlock(experts=MXFP4MoEFFN).

The shapes are the smallest at which the kernel can go wrong: K in {32, 96, 288} (one scale block; a last stage of 32 k
behind a full one; several stages and a tail), N in {8, 40, 136} (less than one 32-column fragment; a partial second
fragment; a second 128-column workgroup), a table of [0, 1, 33, 70] rows plus 2 uncovered (an empty expert, one row, a
second 32-row wave, a second 64-row workgroup) and E = 1 with one row.

MEASURED (MI355X; printed by the tests with -s) and the bounds derived from them:
  * float32 result against the float64 product of the SAME bfloat16-rounded activations and the exactly dequantised
    weights, relative Frobenius error: see SAME_INPUT_MEASURED below; the bound is 4 x that (the margin allows for the
    matrix core's internal adder, which is not an fmaf chain) and must stay below 2^-9.
  * a bfloat16 result adds its one rounding: at most half an ulp, 2^-9 relative, per element (measured 1.5e-3 .. 1.75e-3).
  * against the UN-rounded float32 activations the error is the format's own (bfloat16 activations, 2^-9 per element):
    measured 1.4e-3 .. 2.0e-3 and printed, not asserted.
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 96, 288], [8, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes (tests/test_gpu_footprint.py); 0xFF is a NaN as bfloat16

# relative Frobenius error of the float32 result against the float64 product of the same rounded inputs: the largest value
# the tests below printed on an MI355X, and the bound the tests assert (4 x, below 2^-9 as the contract demands)
SAME_INPUT_MEASURED = 6.6e-8      # (K = 288, N = 40; 0 .. 6.6e-8 over the nine shapes)
SAME_INPUT_BOUND = 4 * SAME_INPUT_MEASURED
# the gated op against the float64 product of the bfloat16-rounded float64 h: the device's float32 h lands on the other
# side of a bfloat16 rounding boundary for a few elements (one ulp = 2^-8 of that element), which dominates
GATED_MEASURED = 3.5e-5           # (gelu_tanh, F = 96, bfloat16 rows; 6e-9 .. 3.4e-5 over the cases; the block: 5.3e-8)
GATED_BOUND = 4 * GATED_MEASURED
BF16_OUT = 2.0 ** -9               # one rounding of the result to bfloat16: half an ulp
assert SAME_INPUT_BOUND < 2.0 ** -9 and GATED_BOUND < 2.0 ** -9


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, lo=97, hi=157, integer=False, seed=0):
    """Random element codes and per-(row, block) scale codes in [lo, hi]; activations randn, or (``integer``) integers in
    [-4, 4].  ``ref``: float64, the product of the bfloat16-rounded activations and the exactly dequantised weights (+ the
    bias in ``ref_b``), zero on the rows no expert covers.  Computed once per shape and shared; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(1000 * K + N + seed)
    E = len(counts)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    x = torch.randint(-4, 5, (T, K), generator=g).float() if integer else torch.randn(T, K, generator=g)
    bias = torch.randint(-8, 9, (E, N), generator=g).float() if integer else torch.randn(E, N, generator=g)
    xr = x.bfloat16().double()
    ref, ref_b, ref_raw = torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64)
    for e, (c, o) in enumerate(zip(tpe.tolist(), offs.tolist())):
        ref[o:o + c] = xr[o:o + c] @ W[e].T
        ref_b[o:o + c] = ref[o:o + c] + bias[e].double()
        ref_raw[o:o + c] = x[o:o + c].double() @ W[e].T
    return dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), x=x.to(DEV), bias=bias.to(DEV),
                tpe=tpe.to(DEV), offs=offs.to(DEV), ref=ref, ref_b=ref_b, ref_raw=ref_raw, W=W, counts=list(counts))


def run(p, x=None, bias=False, out_dtype=None, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4(a["blocks"], a["scales"], p["x"] if x is None else x, a["tpe"], a["offs"],
                                   bias=p["bias"] if bias is True else (None if bias is False else bias), out_dtype=out_dtype)


# ---- the lane map, exactly

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din):
    """Integer activations in [-4, 4], random codes, scale codes in [125, 129]: every product is a multiple of 2^-3 and
    every partial sum is below 2^15, so the float32 result is the integer reference bit for bit whatever the order.  The
    weight matrix is asymmetric: a swapped row / column, a wrong k slot or a scale on the wrong block fails."""
    p = problem(K, N, lo=125, hi=129, integer=True)
    for bias in (False, True):
        ref = p["ref_b"] if bias else p["ref"]
        assert float(ref.abs().max()) < 2 ** 15
        got = run(p, p["x"].to(din), bias=bias, out_dtype=torch.float32)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                         # uncovered rows: exactly zero
        got16 = run(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16)          # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())


def test_exact_one_expert_one_row():
    p = problem(96, 40, counts=(1,), tail=0, lo=125, hi=129, integer=True)
    assert torch.equal(run(p, out_dtype=torch.float32).cpu().double(), p["ref"])


# ---- random inputs

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_inputs_against_the_same_rounded_inputs(K, N):
    p = problem(K, N)
    for din in (torch.float32, torch.bfloat16):
        x = p["x"] if din == torch.float32 else p["x"].bfloat16()
        for bias in (False, True):
            ref = p["ref_b"] if bias else p["ref"]
            e32 = rel_fro_dev(run(p, x, bias=bias, out_dtype=torch.float32), ref)
            e16 = rel_fro_dev(run(p, x, bias=bias, out_dtype=torch.bfloat16), ref)
            print(f"mxfp4 K={K} N={N} in={din} bias={bias}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.1e}), "
                  f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
            assert e32 <= SAME_INPUT_BOUND
            assert e16 <= SAME_INPUT_BOUND + BF16_OUT
    # the format's own error: against the activations before their rounding to bfloat16 (recorded, not asserted)
    print(f"mxfp4 K={K} N={N}: rel_fro against un-rounded float32 activations "
          f"{rel_fro_dev(run(p, out_dtype=torch.float32), p['ref_raw']):.3e}")


def test_float16_is_refused_and_out_dtype_follows_the_input():
    p = problem(32, 8)
    with pytest.raises(RuntimeError, match="float16"):
        run(p, p["x"].half())
    assert run(p).dtype == torch.float32 and run(p, p["x"].bfloat16()).dtype == torch.bfloat16
    q = problem(32, 8, lo=125, hi=129)                                               # (inside float16's range)
    got = run(q, out_dtype=torch.float16)                                            # (store_out4 gives it for free)
    assert got.dtype == torch.float16 and rel_fro_dev(got, q["ref"]) <= SAME_INPUT_BOUND + 2.0 ** -11
    with pytest.raises(RuntimeError, match="forward-only"):
        run(p, p["x"].clone().requires_grad_(True))


# ---- independence, bit for bit

@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N):
    p = problem(K, N)
    got = run(p, bias=True)
    assert same_bits(got, run(p, bias=True))                                         # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_forward_mxfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["x"][o:o + c].contiguous(),
                                      torch.tensor([c], dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int32, device=DEV), bias=p["bias"][e:e + 1])
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_forward_mxfp4(p["blocks"][perm], p["scales"][perm], p["x"], p["tpe"][perm], p["offs"][perm],
                                    bias=p["bias"][perm])
    assert same_bits(again, got)


# ---- non-finite values

def test_scale_code_255_is_nan_in_exactly_that_weight_row():
    p = problem(96, 40)
    scales = p["scales"].clone()
    e, n = 2, 17
    scales[e, n, 1] = 255
    got = run(p, scales=scales)
    want = run(p)
    o, c = p["offs"].tolist()[e], p["counts"][e]
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[o:o + c, n] = True
    assert torch.equal(nan, expect)
    assert torch.equal(got[~expect], want[~expect])


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_inf_activation_is_nan_across_exactly_its_row(din):
    p = problem(288, 136)
    x = p["x"].to(din).clone()
    t = p["offs"].tolist()[3] + 40                                                   # a row of the second 32-row wave
    x[t, 201] = float("inf")
    got, want = run(p, x), run(p, p["x"].to(din))
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[t] = True
    assert torch.equal(nan, expect)
    assert same_bits(got[~expect], want[~expect])


# ---- the gated op

@functools.lru_cache(maxsize=None)
def gated_problem(F, kind, N=40):
    p = dict(problem(F, N, seed=7))
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = torch.randn(p["T"], 2 * F, generator=g) * 2.0
    refs = {}
    for din in (torch.float32, torch.bfloat16):
        h = hidden64(kind, gate_up.to(din), ALPHA, LIMIT).bfloat16().double()        # the bf16-rounded reference h
        ref = torch.zeros(p["T"], N, dtype=torch.float64)
        for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
            ref[o:o + c] = h[o:o + c] @ p["W"][e].T + p["bias"][e].cpu().double()
        refs[din] = ref
    p.update(gate_up=gate_up.to(DEV), refs=refs)
    return p


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96])
def test_gated_op_against_the_rounded_reference_h(F, kind):
    p = gated_problem(F, kind)
    for din in (torch.float32, torch.bfloat16):
        gu = p["gate_up"].to(din)
        got = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gu, p["tpe"], p["offs"], bias=p["bias"],
                                            out_dtype=torch.float32, **act_kw(kind))
        err = rel_fro_dev(got, p["refs"][din])
        print(f"mxfp4 gated F={F} {kind} in={din}: rel_fro {err:.3e} (bound {GATED_BOUND:.1e})")
        assert err <= GATED_BOUND
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
        assert same_bits(got, ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gu, p["tpe"], p["offs"], bias=p["bias"],
                                                            out_dtype=torch.float32, **act_kw(kind)))


# ---- layer and block

def ffn_weights(E, H, F, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    return dict(gate=mk(F, H), up=mk(F, H), down=mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H))


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_is_the_two_ops_composed(dt):
    E, H, F = 4, 64, 96
    w = ffn_weights(E, H, F)
    m = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                      down_bias=w["down_bias"], activation_dtype=dt, **act_kw("swiglu_clamp")).to(DEV)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H, device=DEV).to(dt or torch.float32)
    got = m(x, tpe, offs)
    gate_up = ops().moe_forward_mxfp4(m.gate_up_blocks, m.gate_up_scales, x, tpe, offs, bias=m.gate_up_bias.detach())
    want = ops().moe_gated_forward_mxfp4(m.down_blocks, m.down_scales, gate_up, tpe, offs, bias=m.down_bias.detach(),
                                         **act_kw("swiglu_clamp"))
    assert got.dtype == x.dtype and same_bits(got, want)
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True), tpe, offs)


def test_block_with_mxfp4_experts_against_torch():
    """E = 4, top-2, H = 64, F = 96, swiglu_clamp, expert and router biases, under no_grad.  Reference: a torch block on the
    dequantised weights with bfloat16-rounded operands (x and h), the routing taken from the block's own router."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    E, H, F, T = 4, 64, 96, 50
    w = ffn_weights(E, H, F, seed=9)
    experts = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                            down_bias=w["down_bias"], **act_kw("swiglu_clamp"))
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=experts, router_bias=True).to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H, generator=g).to(DEV)
    with torch.no_grad():
        blk.gate.bias.copy_(torch.randn(E, generator=g) * 0.1)
        out, logits = blk(x)
        weights, indices = ops().router_topk(logits, 2)
    Wgu = dequantize_mxfp4(experts.gate_up_blocks.cpu(), experts.gate_up_scales.cpu()).double()
    Wd = dequantize_mxfp4(experts.down_blocks.cpu(), experts.down_scales.cpu()).double()
    xr = x.cpu().bfloat16().double()
    ref = torch.zeros(T, H, dtype=torch.float64)
    for t in range(T):
        for j in range(2):
            e = int(indices[t, j])
            gu = (Wgu[e] @ xr[t] + experts.gate_up_bias[e].cpu().double()).float()          # the layer keeps gate_up in float32
            h = hidden64("swiglu_clamp", gu[None], ALPHA, LIMIT).bfloat16().double()[0]
            ref[t] += float(weights[t, j]) * (Wd[e] @ h + experts.down_bias[e].cpu().double())
    err = rel_fro_dev(out, ref)
    print(f"mxfp4 block: rel_fro {err:.3e} (bound {GATED_BOUND:.1e})")
    assert err <= GATED_BOUND
    with pytest.raises(RuntimeError, match="inference-only"):
        blk(x.clone().requires_grad_(True))


# ---- footprint

@pytest.mark.parametrize("gated", [False, True], ids=["plain", "glu"])
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [40, 201])
def test_entries_stay_inside_their_buffers(N, dout, gated):
    """Every pointer is the interior of a guarded buffer; out sits 4 bytes off a 16-byte boundary inside SENT.  Only
    [T, N] changes, the guards stay, uncovered rows are zero and the bits are the public op's.  The gated entry runs once
    per stale workspace content (PREFILLS) and must return those bits each time."""
    from fused_int4_amd import _native
    lib = _native.lib()
    K = 96
    p = problem(K, N)
    E, T = p["E"], p["T"]
    if gated:
        g = torch.Generator().manual_seed(3)
        rows = torch.randn(T, 2 * K, generator=g).to(DEV)
    else:
        rows = p["x"]
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    rw, bias = guarded_like("rows", rows, NAN, offset=16), guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert out.ptr % 16 == 4
    nbytes = lib.fql_moe_mx4_workspace_bytes(E, T, K, N, int(gated))
    st = torch.cuda.current_stream().cuda_stream
    if gated:
        assert nbytes == (T * K * 2 + 15) // 16 * 16
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        want = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], rows, p["tpe"], p["offs"], bias=p["bias"],
                                             out_dtype=dout, **act_kw("swiglu_clamp"))
        bufs = (bl, sc, rw, bias, cnt, off, out, ws)
        for fill in PREFILLS:                      # what an earlier launch may have left in the workspace: the same bits
            ws.bytes().fill_(fill)
            out.view(dout, T, N).fill_(SENT)
            rc = lib.fql_moe_mx4_glu_fwd(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                         ACT["swiglu_clamp"], ALPHA, LIMIT, ws.ptr, nbytes, st)
            assert rc == 0
            assert_guards_intact(*bufs, what=f"mx4 fwd gated N={N} {dout} workspace {fill:#04x}")
            assert torch.count_nonzero(out.view(dout, T, N)[T - TAIL:]) == 0, hex(fill)
            assert same_bits(out.view(dout, T, N), want), hex(fill)
    else:
        assert nbytes == 0
        rc = lib.fql_moe_mx4_fwd(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N, None, 0, st)
        want = run(p, bias=True, out_dtype=dout)
        bufs = (bl, sc, rw, bias, cnt, off, out)
    assert rc == 0
    assert_guards_intact(*bufs, what=f"mx4 fwd gated={gated} N={N} {dout}")
    got = out.view(dout, T, N)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, want)
