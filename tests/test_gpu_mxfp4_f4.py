"""MXFP4 expert weights over MXFP4 rows on the GPU (W4A4): ops.quantize_rows_mxfp4, ops.moe_forward_mxfp4_fp4 and
``precision="fp4"`` of ops.moe_forward_mxfp4 / ops.moe_gated_forward_mxfp4 (csrc/fql_gemm_mx4_scaled.h:
v_mfma_scale_f32_32x32x64_f8f6f4 with both operands e2m1 and their E8M0 scales), the layer MXFP4MoEFFN(precision="fp4") and
the sparse block on it.  The reference for the rule is quantize.quantize_mxfp4 / dequantize_mxfp4 with float64 products.

Shapes: K in {32, 96, 256, 288} = 1, 3, 8 and 9 scale blocks (half an instruction; a half-filled second instruction; two
whole 128-k stages; two stages and a tail of one block), N in {8, 40, 136} (less than one 32-column fragment; a partial
second fragment; a second 128-column workgroup), a table of [0, 1, 33, 70] rows plus 2 uncovered (an empty expert, one
row, a second 32-row wave, a second 64-row workgroup).

MEASURED (MI355X; printed by the tests with -s):
  * float32 result against the float64 product of the SAME MXFP4 values on both sides: SAME_INPUT_MEASURED, asserted at the
    fp8 path's own bound SAME_INPUT_BOUND = 3.0e-5 (the same instruction in the same order; every product is exact); a
    bfloat16 result adds its one rounding, 2^-9.  The measurement is far below the fp8 path's 7.5e-6: a product of two
    e2m1 values has at most 4 significant bits, so the instruction's sums lose next to nothing.
  * against the UN-quantised float32 rows the error is the MXFP4 format's own: FORMAT_MEASURED; asserted only to lie in
    [5e-2, 2e-1] (computed on the host beforehand: 1.11e-1 to 1.16e-1).
  * the sparse block against torch with both GEMMs' rows quantised by quantize_mxfp4: BLOCK_MEASURED, asserted at 4 x and
    never above 1e-2 (a tenth of the format's own error).
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import (NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 96, 256, 288], [8, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes (tests/test_gpu_footprint.py); 0xFF is a NaN as an E8M0 scale

SAME_INPUT_BOUND = 3.0e-5         # the fp8 path's asserted bound (tests/test_gpu_mxfp4_f8.py), as it stands
SAME_INPUT_MEASURED = 3.5e-8      # (K = 256, N = 8; 0 at K = 32, where one block is one exact sum, .. 3.5e-8 over the twelve shapes)
FORMAT_MEASURED = 1.26e-1         # (K = 32, N = 40; 9.2e-2 .. 1.26e-1 over the twelve shapes)
FORMAT_RANGE = (5e-2, 2e-1)
BF16_OUT = 2.0 ** -9              # one rounding of the result to bfloat16: half an ulp
# the block: the device's float32 gate_up differs from the reference's by the first GEMM's accumulation error (1e-8), and
# with the seeded gate and input no element of h falls on the other e2m1 neighbour (one grid step would be up to half of
# that element: 1e-3 on the whole): what is left is accumulation and the float32 roundings of gate_up and out
BLOCK_MEASURED = 4.6e-8
BLOCK_BOUND = 4 * BLOCK_MEASURED
assert BLOCK_BOUND <= 1e-2
GATED_CODE_CAP, GATED_SCALE_CAP = 0.002, 0.01


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


def unpack(blocks):
    return torch.stack([blocks & 15, blocks >> 4], dim=-1).reshape(*blocks.shape[:-1], blocks.shape[-1] * 2)


def q_host(x):
    """quantize.quantize_mxfp4 of a tensor (widened to float32 on the host) -> (blocks, scales, their float64 values)."""
    from fused_int4_amd.quantize import dequantize_mxfp4, quantize_mxfp4
    b, s = quantize_mxfp4(x.detach().cpu().float())
    return b, s, dequantize_mxfp4(b, s).double()


def grouped64(rows64, W, bias, counts, offs):
    """float64 [T, N]: rows64 @ W[e].T (+ bias[e]) over the rows of expert e, zero elsewhere."""
    ref = torch.zeros(rows64.shape[0], W.shape[1], dtype=torch.float64)
    for e, (c, o) in enumerate(zip(counts, offs)):
        ref[o:o + c] = rows64[o:o + c] @ W[e].T
        if bias is not None:
            ref[o:o + c] += bias[e].double()
    return ref


@functools.lru_cache(maxsize=None)
def problem(K, N, lo=97, hi=157, kind="randn", seed=0):
    """Random weight codes over all 16 values and a scale code in [lo, hi] for every (row, block).  ``kind``: "randn" rows;
    "codes": rows that are MXFP4 already, random codes with a scale code in [lo, hi]; "grid": float rows of e2m1 grid
    values times 2^j per block, j in [-1, 1], with a +-4 or +-6 in every block.  Computed once per shape and shared; nobody
    writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(1000 * K + N + seed)
    E = len(COUNTS)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    tpe, offs, T = expert_table(COUNTS, tail=TAIL, device="cpu")
    p = dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), tpe=tpe.to(DEV), offs=offs.to(DEV), W=W,
             counts=list(COUNTS), offs_l=offs.tolist())
    if kind == "randn":
        x = torch.randn(T, K, generator=g)
        bias = torch.randn(E, N, generator=g)
    else:
        xc = torch.randint(0, 16, (T, K), generator=g, dtype=torch.uint8)
        if kind == "codes":
            xs = torch.randint(lo, hi + 1, (T, K // 32), generator=g, dtype=torch.uint8)
        else:
            where = torch.randint(0, 32, (T, K // 32), generator=g) + 32 * torch.arange(K // 32)
            anchor = torch.randint(6, 8, (T, K // 32), generator=g) + 8 * torch.randint(0, 2, (T, K // 32), generator=g)
            xc.scatter_(1, where, anchor.to(torch.uint8))
            xs = torch.randint(126, 129, (T, K // 32), generator=g, dtype=torch.uint8)
        xb = pack(xc)
        x = dequantize_mxfp4(xb, xs)
        p.update(xb=xb.to(DEV), xs=xs.to(DEV))
        bias = torch.randint(-8, 9, (E, N), generator=g).float()
    p.update(x=x.to(DEV), x_cpu=x, bias=bias.to(DEV), bias_cpu=bias)
    return p


def ref64(p, rows64, bias):
    return grouped64(rows64, p["W"], p["bias_cpu"] if bias else None, p["counts"], p["offs_l"])


def run4(p, xb, xs, bias=False, out_dtype=torch.float32, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4_fp4(a["blocks"], a["scales"], xb, xs, a["tpe"], a["offs"],
                                       bias=p["bias"] if bias else None, out_dtype=out_dtype)


def runq(p, x, bias=False, out_dtype=torch.float32, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4(a["blocks"], a["scales"], x, a["tpe"], a["offs"], bias=p["bias"] if bias else None,
                                   out_dtype=out_dtype, precision="fp4")


# ---- 1. the quantiser is the host rule, bit for bit

def assert_is_host_rule(x_dev):
    b, s, _ = q_host(x_dev)
    gb, gs = ops().quantize_rows_mxfp4(x_dev)
    assert gb.dtype == torch.uint8 and gs.dtype == torch.uint8 and gb.shape == b.shape and gs.shape == s.shape
    assert torch.equal(gs.cpu(), s), (gs.cpu() != s).nonzero()[:4]
    assert torch.equal(gb.cpu(), b), (gb.cpu() != b).nonzero()[:4]
    return gb, gs


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_quantiser_is_the_host_rule_on_random_rows(K, din):
    g = torch.Generator().manual_seed(K)
    T = 106
    x = torch.randn(T, K // 32, 32, generator=g) * torch.exp2(torch.randint(-29, 32, (T, K // 32, 1), generator=g).float())
    _, gs = assert_is_host_rule(x.reshape(T, K).to(din).to(DEV))
    assert int(gs.min()) <= 100 and int(gs.max()) >= 154                             # the scale codes span about [97, 157]


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantiser_is_the_host_rule_on_crafted_blocks(din):
    """One block a row, K = 32, for 2^shared in {2^-20, 1, 2^13}: every tie of the grid in both signs beside a 4.0 anchor;
    saturation (6.5, 7, 7.75); tiny negatives (code 8); an all-zero block; float32 subnormals (scale code 0)."""
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    rows = []
    for sh in (-20, 0, 13):
        a = torch.zeros(32)
        a[:7], a[7:14], a[14] = ties, -ties, 4.0
        a[15:20] = torch.tensor([0.125, -0.125, 0.1875, -0.3125, 0.8125])
        sat = torch.zeros(32)
        sat[:6] = torch.tensor([6.5, -6.5, 7.0, -7.0, 7.75, -7.5])
        sat[6:10] = torch.tensor([5.5, -5.0, 6.0, -4.5])
        tiny = torch.full((32,), -2.0 ** -10)
        tiny[3], tiny[4] = 6.0, -0.0
        rows += [torch.ldexp(r, torch.tensor(sh)) for r in (a, sat, tiny)]
    rows.append(torch.zeros(32))
    neg0 = torch.zeros(32)
    neg0[5] = -0.0
    rows.append(neg0)
    sub = torch.arange(32).float() * 2.0 ** -133 * torch.where(torch.arange(32) % 3 == 0, -1.0, 1.0)   # (bfloat16 holds these too)
    rows += [sub, sub * 4, torch.ldexp(torch.arange(32).float(), torch.tensor(-149))]
    x = torch.stack(rows).to(din)
    assert torch.equal(x.float()[:-1], torch.stack(rows)[:-1])                       # (all but the last row are bfloat16 values)
    gb, gs = assert_is_host_rule(x.to(DEV))
    gs, codes = gs.cpu()[:, 0], unpack(gb.cpu())
    assert gs[0] == 127 - 20 and gs[3] == 127 and gs[6] == 127 + 13                  # anchor 4 = 2^2: shared = the exponent
    assert codes[3, :15].tolist() == [0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 6]   # ties go to the even neighbour
    assert codes[4, :6].tolist() == [7, 15, 7, 15, 7, 15]                            # saturated at +-6
    assert codes[5, 0] == 8 and codes[5, 4] == 8                                     # a negative that rounds to zero keeps its sign
    assert gs[9] == 127 and int(codes[9].sum()) == 0 and gs[10] == 127 and codes[10, 5] == 8
    assert gs[11] == 0 and gs[12] == 0                                               # float32 subnormals: shared clamps at -127
    if din == torch.float32:
        assert gs[13] == 0


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantiser_marks_a_non_finite_block_and_only_it(din):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(9, 96, generator=g).to(din)
    clean = x.clone()
    bad = {(2, 1): float("inf"), (5, 0): NAN, (7, 2): float("-inf")}
    for (t, blk), v in bad.items():
        x[t, 32 * blk + 7] = v
        clean[t, 32 * blk + 7] = 0
    b, s, _ = q_host(clean)
    for (t, blk) in bad:
        b[t, 16 * blk:16 * blk + 16] = 0
        s[t, blk] = 255
    gb, gs = ops().quantize_rows_mxfp4(x.to(DEV))
    assert torch.equal(gs.cpu(), s) and torch.equal(gb.cpu(), b)


# ---- 2. the B lane map, the nibble order and the B scale's block, exactly

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_grid_data_mxfp4_rows_in(K, N):
    """Random codes over all 16 values on both sides, scale codes in [126, 128] on both sides: every product is a multiple
    of 2^-4 and every sum is below 2^16 (36 x 4 x 288), so the float32 result is the float64 reference bit for bit whatever
    the adder does.  The data is asymmetric: a swapped row or column, a wrong k slot, the nibbles in the other order or
    a scale on the wrong block fails."""
    p = problem(K, N, lo=126, hi=128, kind="codes")
    for bias in (False, True):
        ref = ref64(p, p["x_cpu"].double(), bias)
        assert float(ref.abs().max()) < 2 ** 16
        got = run4(p, p["xb"], p["xs"], bias=bias)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                         # uncovered rows: exactly zero
        got16 = run4(p, p["xb"], p["xs"], bias=bias, out_dtype=torch.bfloat16)       # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())


# ---- 3. exact through the quantiser

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_through_the_quantiser(K, N, din):
    """e2m1 grid values times 2^j per block, j in [-1, 1], a +-4 or +-6 in every block: the quantiser reproduces the rows
    exactly; weight scale codes in [126, 128].  The result is the float64 product of the original rows bit for bit."""
    p = problem(K, N, lo=126, hi=128, kind="grid")
    assert torch.equal(p["x_cpu"].to(din).float(), p["x_cpu"])
    for bias in (False, True):
        ref = ref64(p, p["x_cpu"].double(), bias)
        assert float(ref.abs().max()) < 2 ** 16
        got = runq(p, p["x"].to(din), bias=bias)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0


# ---- 4. random rows

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_inputs_against_the_same_mxfp4_values(K, N):
    p = problem(K, N)
    b, s, vals = q_host(p["x"])
    xb, xs = b.to(DEV), s.to(DEV)
    for bias in (False, True):
        ref = ref64(p, vals, bias)
        e32 = rel_fro_dev(run4(p, xb, xs, bias=bias), ref)
        e16 = rel_fro_dev(run4(p, xb, xs, bias=bias, out_dtype=torch.bfloat16), ref)
        print(f"mxfp4-f4 K={K} N={N} bias={bias}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.1e}), "
              f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
        assert e32 <= SAME_INPUT_BOUND
        assert e16 <= SAME_INPUT_BOUND + BF16_OUT
    # the format's own error: against the rows before their quantisation
    got = runq(p, p["x"])
    assert same_bits(got, run4(p, xb, xs))                                           # (the fused quantiser is the host rule)
    fmt = rel_fro_dev(got, ref64(p, p["x_cpu"].double(), False))
    print(f"mxfp4-f4 K={K} N={N}: rel_fro against un-quantised float32 rows {fmt:.3e} (measured up to {FORMAT_MEASURED:.2e})")
    assert FORMAT_RANGE[0] <= fmt <= FORMAT_RANGE[1]


# ---- 5. the gated form

def step_index(codes):
    """Signed position on the e2m1 grid: +-(code & 7)."""
    mag = (codes & 7).to(torch.int32)
    return torch.where(codes >= 8, -mag, mag)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96])
def test_gated_op_is_the_quantiser_then_the_gemm(F, kind):
    p = problem(F, 40, seed=7)
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = (torch.randn(p["T"], 2 * F, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        gu = gate_up.to(din)
        got = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gu, p["tpe"], p["offs"], bias=p["bias"],
                                            out_dtype=torch.float32, precision="fp4", **act_kw(kind))
        hb, hs = ops().quantize_rows_mxfp4(gu, **act_kw(kind))
        assert hb.shape == (p["T"], F // 2) and hs.shape == (p["T"], F // 32)
        assert same_bits(got, run4(p, hb, hs, bias=True))
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
        # the gated quantiser against quantize_mxfp4 of the float64 h
        b, s, _ = q_host(hidden64(kind, gu.cpu(), ALPHA, LIMIT))
        c_dev, c_ref = unpack(hb.cpu()), unpack(b)
        d_scale = hs.cpu() != s
        d_code = c_dev != c_ref
        print(f"mxfp4-f4 gated F={F} {kind} in={din}: {int(d_code.sum())} of {d_code.numel()} codes and "
              f"{int(d_scale.sum())} of {d_scale.numel()} scale bytes differ from the float64 h")
        assert d_code.float().mean() <= GATED_CODE_CAP and d_scale.float().mean() <= GATED_SCALE_CAP
        same_scale = (~d_scale).repeat_interleave(32, dim=1)
        off = d_code & same_scale
        assert bool(((step_index(c_dev) - step_index(c_ref)).abs()[off] == 1).all())


# ---- 6. independence, bit for bit

@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N):
    p = problem(K, N)
    got = runq(p, p["x"], bias=True)
    assert same_bits(got, runq(p, p["x"], bias=True))                                # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs_l"])):
        if c == 0:
            continue
        one = ops().moe_forward_mxfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["x"][o:o + c].contiguous(),
                                      torch.tensor([c], dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int32, device=DEV), bias=p["bias"][e:e + 1], precision="fp4")
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_forward_mxfp4(p["blocks"][perm], p["scales"][perm], p["x"], p["tpe"][perm], p["offs"][perm],
                                    bias=p["bias"][perm], precision="fp4")
    assert same_bits(again, got)


# ---- 7. non-finite values

def test_scale_code_255_is_nan_in_exactly_that_weight_row():
    p = problem(96, 40)
    scales = p["scales"].clone()
    e, n = 2, 17
    scales[e, n, 1] = 255
    got, want = runq(p, p["x"], scales=scales), runq(p, p["x"])
    o, c = p["offs_l"][e], p["counts"][e]
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[o:o + c, n] = True
    assert torch.equal(nan, expect)
    assert torch.equal(got[~expect], want[~expect])


@pytest.mark.parametrize("what", ["scale_byte", "inf_row", "nan_row", "nan_row_bf16", "inf_row_bf16"])
def test_non_finite_rows_are_nan_across_exactly_their_row(what):
    p = problem(288, 136)
    t = p["offs_l"][3] + 40                                                          # a row of the second 32-row wave
    if what == "scale_byte":
        b, s, _ = q_host(p["x"])
        xb, xs = b.to(DEV), s.to(DEV)
        bad = xs.clone()
        bad[t, 6] = 255
        got, want = run4(p, xb, bad), run4(p, xb, xs)
    else:
        din = torch.bfloat16 if what.endswith("bf16") else torch.float32
        x = p["x"].to(din).clone()
        x[t, 201] = NAN if what.startswith("nan") else float("inf")
        got, want = runq(p, x), runq(p, p["x"].to(din))
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[t] = True
    assert torch.equal(nan, expect)
    assert same_bits(got[~expect], want[~expect])


# ---- 8. layer and block

def ffn_weights(E, H, F, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    return dict(gate=mk(F, H), up=mk(F, H), down=mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_is_the_two_ops_composed_and_the_default_is_unchanged(dt, with_bias):
    E, H, F = 4, 64, 96
    w = ffn_weights(E, H, F)
    biases = dict(gate_bias=w["gate_bias"], up_bias=w["up_bias"], down_bias=w["down_bias"]) if with_bias else {}
    make = lambda **kw: fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], activation_dtype=dt, **biases,
                                                      **act_kw("swiglu_clamp"), **kw).to(DEV)
    m, base = make(precision="fp4"), make()
    assert list(m.state_dict()) == list(base.state_dict())
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(2)).to(DEV).to(dt or torch.float32)
    b_gu, b_d = (m.gate_up_bias.detach(), m.down_bias.detach()) if with_bias else (None, None)
    got = m(x, tpe, offs)
    gate_up = ops().moe_forward_mxfp4(m.gate_up_blocks, m.gate_up_scales, x, tpe, offs, bias=b_gu, precision="fp4")
    want = ops().moe_gated_forward_mxfp4(m.down_blocks, m.down_scales, gate_up, tpe, offs, bias=b_d, precision="fp4",
                                         **act_kw("swiglu_clamp"))
    assert got.dtype == x.dtype and same_bits(got, want)
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True), tpe, offs)
    # the default layer: the ops without the keyword, bit for bit
    gate_up = ops().moe_forward_mxfp4(base.gate_up_blocks, base.gate_up_scales, x, tpe, offs, bias=b_gu)
    want = ops().moe_gated_forward_mxfp4(base.down_blocks, base.down_scales, gate_up, tpe, offs, bias=b_d,
                                         **act_kw("swiglu_clamp"))
    assert same_bits(base(x, tpe, offs), want)
    assert not same_bits(got, want)                                                  # (the two modes are different numbers)


def test_block_with_fp4_mxfp4_experts_against_torch():
    """E = 4, top-2, H = 64, F = 96, swiglu_clamp, expert and router biases, seeded gate, under no_grad.  Reference: a torch
    block on the dequantised weights with the rows of both GEMMs (x, then h) quantised by quantize_mxfp4, the routing taken
    from the block's own router."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    E, H, F, T = 4, 64, 96, 50
    w = ffn_weights(E, H, F, seed=9)
    experts = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                            down_bias=w["down_bias"], precision="fp4", **act_kw("swiglu_clamp"))
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=experts, router_bias=True).to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H, generator=g).to(DEV)
    with torch.no_grad():
        blk.gate.bias.copy_(torch.randn(E, generator=g) * 0.1)
        blk.gate.weight.copy_((torch.randn(E, H, generator=g) * 0.1).to(DEV))
        out, logits = blk(x)
        weights, indices = ops().router_topk(logits, 2)
    Wgu = dequantize_mxfp4(experts.gate_up_blocks.cpu(), experts.gate_up_scales.cpu()).double()
    Wd = dequantize_mxfp4(experts.down_blocks.cpu(), experts.down_scales.cpu()).double()
    xq = q_host(x)[2]
    ref = torch.zeros(T, H, dtype=torch.float64)
    for t in range(T):
        for j in range(2):
            e = int(indices[t, j])
            gu = (Wgu[e] @ xq[t] + experts.gate_up_bias[e].cpu().double()).float()          # the layer keeps gate_up in float32
            h = q_host(hidden64("swiglu_clamp", gu[None], ALPHA, LIMIT))[2][0]
            ref[t] += float(weights[t, j]) * (Wd[e] @ h + experts.down_bias[e].cpu().double())
    err = rel_fro_dev(out, ref)
    print(f"mxfp4-f4 block: rel_fro {err:.3e} (bound {BLOCK_BOUND:.1e})")
    assert err <= BLOCK_BOUND
    with pytest.raises(RuntimeError, match="inference-only"):
        blk(x.clone().requires_grad_(True))


# ---- 9. footprint

@pytest.mark.parametrize("entry", ["f4", "q4", "glu_q4"])
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [40, 201])
def test_entries_stay_inside_their_buffers(N, dout, entry):
    """Every pointer is the interior of a guarded buffer; out sits 4 bytes off a 16-byte boundary inside SENT and the
    workspace has exactly the reported size.  Only [T, N] (and the workspace, but not its padding) changes, the guards stay,
    the operands are unchanged, uncovered rows are zero and the bits are the public op's.  The two entries with a workspace
    run on 0x5A and then once per stale workspace content of PREFILLS, with the same bits and the same workspace each time."""
    from fused_int4_amd import _native
    lib = _native.lib()
    K = 96
    p = problem(K, N)
    E, T = p["E"], p["T"]
    st = torch.cuda.current_stream().cuda_stream
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert out.ptr % 16 == 4
    mode = {"f4": 0, "q4": 1, "glu_q4": 2}[entry]
    nbytes = lib.fql_moe_mx4_f4_workspace_bytes(E, T, K, N, mode)
    if entry == "f4":
        assert nbytes == 0
        b, s, _ = q_host(p["x"])
        xb, xs = b.to(DEV), s.to(DEV)
        rw = guarded_like("in_blocks", xb, 0xFF, offset=16)                          # (a guard byte that is used: -1.5 twice)
        sg = guarded_like("in_scales", xs, 0xFF, offset=1)                           # (... a NaN scale)
        rc = lib.fql_moe_mx4_fwd_f4(bl.ptr, sc.ptr, rw.ptr, sg.ptr, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                    None, 0, st)
        want = run4(p, xb, xs, bias=True, out_dtype=dout)
        bufs, ops_in = (bl, sc, rw, sg, bias, cnt, off, out), ((rw, xb), (sg, xs))
    else:
        used_b, used_s = T * K // 2, T * K // 32
        assert nbytes == (used_b + 15) // 16 * 16 + (used_s + 15) // 16 * 16 and used_s % 16 != 0
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        ws.bytes().fill_(0x5A)
        row_off = 16 if N == 40 else 4                                               # the 16-byte loads / the element loads
        if entry == "q4":
            rows = p["x"]
            rw = guarded_like("rows", rows, NAN, offset=row_off)
            call = lambda: lib.fql_moe_mx4_fwd_q4(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                                  ws.ptr, nbytes, st)
            rc = call()
            want = runq(p, rows, bias=True, out_dtype=dout)
            hb, hs = ops().quantize_rows_mxfp4(rows)
        else:
            g = torch.Generator().manual_seed(3)
            rows = torch.randn(T, 2 * K, generator=g).to(DEV)
            rw = guarded_like("rows", rows, NAN, offset=row_off)
            call = lambda: lib.fql_moe_mx4_glu_fwd_q4(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                                      ACT["swiglu_clamp"], ALPHA, LIMIT, ws.ptr, nbytes, st)
            rc = call()
            want = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], rows, p["tpe"], p["offs"], bias=p["bias"],
                                                 out_dtype=dout, precision="fp4", **act_kw("swiglu_clamp"))
            hb, hs = ops().quantize_rows_mxfp4(rows, **act_kw("swiglu_clamp"))
        bufs, ops_in = (bl, sc, rw, bias, cnt, off, out, ws), ((rw, rows),)
    assert rc == 0
    assert_guards_intact(*bufs, what=f"mx4 f4 {entry} N={N} {dout}")
    if entry != "f4":                                                                # the workspace: the rows, their scales, padding
        w = ws.bytes()
        first = (used_b + 15) // 16 * 16
        assert torch.equal(w[:used_b], hb.flatten()) and torch.equal(w[first:first + used_s], hs.flatten())
        assert bool((w[used_b:first] == 0x5A).all()) and bool((w[first + used_s:] == 0x5A).all())
    for buf, t in ((bl, p["blocks"]), (sc, p["scales"]), (bias, p["bias"]), (cnt, p["tpe"]), (off, p["offs"])) + ops_in:
        # (the operands are unchanged)
        assert torch.equal(buf.view(t.dtype, *t.shape), t), buf.name
    got = out.view(dout, T, N)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, want)
    if entry != "f4":                               # what an earlier launch may have left in the workspace: the same bits
        for fill in PREFILLS:
            w.fill_(fill)
            got.fill_(SENT)
            assert call() == 0
            assert_guards_intact(*bufs, what=f"mx4 f4 {entry} N={N} {dout} workspace {fill:#04x}")
            assert torch.equal(w[:used_b], hb.flatten()) and torch.equal(w[first:first + used_s], hs.flatten()), hex(fill)
            assert bool((w[used_b:first] == fill).all()) and bool((w[first + used_s:] == fill).all()), hex(fill)
            assert torch.count_nonzero(got[T - TAIL:]) == 0, hex(fill)
            assert same_bits(got, want), hex(fill)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantize_rows_stays_inside_its_buffers(din, gated):
    """The quantiser's two outputs, [T][K/2] and [T][K/32], are written in full and nothing around them; rows 16-byte
    aligned (the wide loads) and 4 bytes off (the element loads)."""
    from fused_int4_amd import _native
    lib = _native.lib()
    T, K = 37, 96
    st = torch.cuda.current_stream().cuda_stream
    rows = torch.randn(T, (2 if gated else 1) * K, generator=torch.Generator().manual_seed(6)).to(din).to(DEV)
    kw = act_kw("gelu_tanh") if gated else {}
    wb, wsc = ops().quantize_rows_mxfp4(rows, **kw)
    for row_off in (16, 4):
        rw = guarded_like("rows", rows, NAN, offset=row_off)
        ob = Guarded("out_blocks", T * K // 2, torch.uint8, 0x5A, offset=16)
        osc = Guarded("out_scales", T * K // 32, torch.uint8, 0x5A, offset=1)
        rc = lib.fql_mx4_quantize_rows(rw.ptr, DT[din], int(gated), ACT["gelu_tanh"], ALPHA, LIMIT, ob.ptr, osc.ptr, T, K, st)
        assert rc == 0
        assert_guards_intact(rw, ob, osc, what=f"mx4 quantize_rows {din} gated={gated} offset {row_off}")
        assert torch.equal(rw.view(rows.dtype, *rows.shape), rows)
        assert torch.equal(ob.view(torch.uint8, T, K // 2), wb) and torch.equal(osc.view(torch.uint8, T, K // 32), wsc)
