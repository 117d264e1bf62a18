"""MXFP4 expert weights over MXFP6 rows on the GPU: ops.quantize_rows_mxfp6, ops.moe_forward_mxfp4_fp6 and
``precision="fp6"`` of ops.moe_forward_mxfp4 / ops.moe_gated_forward_mxfp4 (csrc/fql_gemm_mx4_scaled.h and its decode form
csrc/fql_gemm_mx4_sdecode.h with ROWS = 3: v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 weights against e2m3 rows, each with
its E8M0 scales), the layer MXFP4MoEFFN(precision="fp6") and the sparse block on it.  The reference for the rule is
quantize.quantize_mxfp6 / dequantize_mxfp6 with float64 products.  fql_tune_set_mx4_f6_decode_max_rows forces either kernel.

Shapes: K in {32, 96, 256, 288} = 1, 3, 8 and 9 scale blocks (half an instruction; a half-filled second instruction; two
whole 128-k stages; two stages and a tail of one block; rows of 24, 72, 192 and 216 bytes: 8-, 8-, 16- and 8-byte aligned),
N in {8, 40, 136} (less than one 32-column fragment; a partial second fragment; a second 128-column workgroup), a table of
[0, 1, 33, 70] rows plus 2 uncovered (an empty expert, one row, a second 32-row wave, a second 64-row workgroup).

MEASURED (MI355X; printed by the tests with -s):
  * float32 result against the float64 product of the SAME values on both sides: SAME_INPUT_MEASURED, asserted at the fp8
    path's own bound SAME_INPUT_BOUND = 3.0e-5 as it stands (the same instruction in the same order; every product of an
    e2m1 and an e2m3 value is exact); a bfloat16 result adds its one rounding, 2^-9.
  * against the UN-quantised float32 rows the error is the MXFP6 format's own: FORMAT_MEASURED; asserted only to lie in
    FORMAT_RANGE, fixed beforehand on the host from quantize_mxfp6 over the twelve shapes (FORMAT_HOST) with a factor of 1.5
    either way for what the accumulation and another draw could add; the upper end stays below the fp4 mode's 9e-2.
  * the sparse block against torch with both GEMMs' rows quantised by quantize_mxfp6: BLOCK_MEASURED, asserted at 4 x and
    never above 1e-2.
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import (NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_MAX = 2 ** 31 - 1
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 96, 256, 288], [8, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
FORMS = ["tile", "decode"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes (tests/test_gpu_footprint.py); 0xFF is a NaN as an E8M0 scale

SAME_INPUT_BOUND = 3.0e-5         # the fp8 path's asserted bound (tests/test_gpu_mxfp4_f8.py), as it stands
SAME_INPUT_MEASURED = 3.3e-8      # (0 at K = 32, where one block is one exact sum, .. 3.3e-8 over the twelve shapes; bf16 out 1.28e-3 .. 1.89e-3)
FORMAT_HOST = (2.6e-2, 3.7e-2)    # quantize_mxfp6 on the host, float64 products: 2.64e-2 (K = 96, N = 8) .. 3.67e-2 (K = 32, N = 8)
FORMAT_RANGE = (FORMAT_HOST[0] / 1.5, FORMAT_HOST[1] * 1.5)
assert FORMAT_RANGE[1] < 9e-2
FORMAT_MEASURED = 3.68e-2         # (K = 32, N = 8; 2.64e-2 .. 3.68e-2 over the twelve shapes: the host's figures to three digits)
BF16_OUT = 2.0 ** -9              # one rounding of the result to bfloat16: half an ulp
# the block: as in the fp4 test, the device's float32 gate_up differs from the reference's by the first GEMM's accumulation
# error, and with the seeded gate and input no element of h falls on the other e2m3 neighbour: what is left is accumulation
# and the float32 roundings of gate_up and out
BLOCK_MEASURED = 4.3e-8
BLOCK_BOUND = 4 * BLOCK_MEASURED
assert BLOCK_BOUND <= 1e-2
GATED_CODE_CAP, GATED_SCALE_CAP = 0.002, 0.01

E2M3_OF_INT = [0, 8, 16, 20, 24, 26, 28, 30]                        # e2m3 code of |v| for the integers 0 .. 7


def lib():
    from fused_int4_amd import _native
    return _native.lib()


def Q():
    from fused_int4_amd import quantize
    return quantize


@pytest.fixture
def force():
    """force("decode" | "tile" | "default"); the library's own threshold comes back afterwards."""
    setter = lib().fql_tune_set_mx4_f6_decode_max_rows
    default = setter(-1)                                            # (a negative value changes nothing)

    def use(which):
        setter({"decode": INT_MAX, "tile": 0, "default": default}[which])
        assert lib().fql_tune_mx4_f6_kernel(4, 106, 96, 40) == {"decode": 1, "tile": 0}.get(which, int(106 <= default))
    try:
        yield use
    finally:
        setter(default)


def pack4(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


def q_host(x):
    """quantize.quantize_mxfp6 of a tensor (widened to float32 on the host) -> (codes, scales, their float64 values)."""
    c, s = Q().quantize_mxfp6(x.detach().cpu().float())
    return c, s, Q().dequantize_mxfp6(c, s).double()


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
    "codes": rows that are MXFP6 already, random codes over all 64 values with a scale code in [125, 129] ("codes_wide": in
    [lo, hi], as the weights); "integer": MXFP6
    rows of integers in [-7, 7], every k drawn on its own, with scale codes in [126, 128].  Computed once per shape and
    shared; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(1000 * K + N + seed)
    E = len(COUNTS)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack4(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    tpe, offs, T = expert_table(COUNTS, tail=TAIL, device="cpu")
    p = dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), tpe=tpe.to(DEV), offs=offs.to(DEV), W=W,
             counts=list(COUNTS), offs_l=offs.tolist())
    if kind == "randn":
        x = torch.randn(T, K, generator=g)
        bias = torch.randn(E, N, generator=g)
    else:
        if kind in ("codes", "codes_wide"):
            xc = torch.randint(0, 64, (T, K), generator=g, dtype=torch.uint8)
            xlo, xhi = (lo, hi) if kind == "codes_wide" else (125, 129)
            xs = torch.randint(xlo, xhi + 1, (T, K // 32), generator=g, dtype=torch.uint8)
        else:
            mag = torch.randint(0, 8, (T, K), generator=g)
            xc = (torch.tensor(E2M3_OF_INT)[mag] + 32 * torch.randint(0, 2, (T, K), generator=g)).to(torch.uint8)
            xs = torch.randint(126, 129, (T, K // 32), generator=g, dtype=torch.uint8)
        xb = Q().pack_mxfp6(xc)
        x = Q().dequantize_mxfp6(xb, xs)
        if kind == "integer":
            unit = torch.exp2(xs.float() - 127).repeat_interleave(32, dim=1)
            assert torch.equal(x.abs(), mag.float() * unit)
        p.update(xb=xb.to(DEV), xs=xs.to(DEV))
        bias = torch.randint(-8, 9, (E, N), generator=g).float()
    p.update(x=x.to(DEV), x_cpu=x, bias=bias.to(DEV), bias_cpu=bias)
    return p


def ref64(p, rows64, bias):
    return grouped64(rows64, p["W"], p["bias_cpu"] if bias else None, p["counts"], p["offs_l"])


def run6(p, xb, xs, bias=False, out_dtype=torch.float32, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4_fp6(a["blocks"], a["scales"], xb, xs, a["tpe"], a["offs"],
                                       bias=p["bias"] if bias else None, out_dtype=out_dtype)


def runq(p, x, bias=False, out_dtype=torch.float32, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4(a["blocks"], a["scales"], x, a["tpe"], a["offs"], bias=p["bias"] if bias else None,
                                   out_dtype=out_dtype, precision="fp6")


def rung(p, gate_up, kind, bias=True, out_dtype=torch.float32):
    return ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gate_up, p["tpe"], p["offs"], bias=p["bias"] if bias else None,
                                         out_dtype=out_dtype, precision="fp6", **act_kw(kind))


# ---- 1. exact: the lane map, the field order and the scale's block

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_rows(K, N, form, force):
    """Integer e2m3 rows in [-7, 7] with scale codes 126 .. 128, every k drawn on its own; random weight codes with scale
    codes in [125, 129]: every product is a multiple of 2^-4 and every sum stays below 288 x 6 x 7 x 2 x 4 < 2^17, far
    below 2^24 x 2^-4, so the float32 result is the float64 reference bit for bit whatever the adder does.  A swapped row or
    column, a wrong k slot, another field order inside the 24 bytes or a scale on the wrong block fails."""
    p = problem(K, N, lo=125, hi=129, kind="integer")
    force(form)
    for bias in (False, True):
        ref = ref64(p, p["x_cpu"].double(), bias)
        assert float(ref.abs().max()) < 2 ** 17
        got = run6(p, p["xb"], p["xs"], bias=bias)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias, form)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                         # uncovered rows: exactly zero
        got16 = run6(p, p["xb"], p["xs"], bias=bias, out_dtype=torch.bfloat16)       # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())


# ---- 2. random codes against the float64 product of the same values

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_codes_against_the_same_values(K, N):
    """The float32 result with scale codes in [97, 157] on BOTH sides; the bfloat16 result with the rows' scale codes in
    [125, 129].  2^-9 is not the worst case of one rounding to bfloat16 (that is 2^-8, for a value just above a power of
    two) but a bound on its root mean square over many outputs of comparable size, 2^-8 / sqrt(7) = 1.5e-3 for mantissas
    spread over a binade: with row scales 2^60 apart a handful of rows carry the whole norm and the figure is theirs alone
    (2.4e-3 was seen at K = 96, N = 8), so that check runs where the 104 rows of the table weigh about the same."""
    wide = problem(K, N, kind="codes_wide")
    for bias in (False, True):
        e32 = rel_fro_dev(run6(wide, wide["xb"], wide["xs"], bias=bias), ref64(wide, wide["x_cpu"].double(), bias))
        print(f"mxfp4-f6 K={K} N={N} bias={bias}: rel_fro f32 out, scale codes 97 .. 157 on both sides {e32:.3e} (bound {SAME_INPUT_BOUND:.1e})")
        assert e32 <= SAME_INPUT_BOUND
    p = problem(K, N, kind="codes")
    for bias in (False, True):
        ref = ref64(p, p["x_cpu"].double(), bias)
        e32 = rel_fro_dev(run6(p, p["xb"], p["xs"], bias=bias), ref)
        e16 = rel_fro_dev(run6(p, p["xb"], p["xs"], bias=bias, out_dtype=torch.bfloat16), ref)
        print(f"mxfp4-f6 K={K} N={N} bias={bias}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.1e}), "
              f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
        assert e32 <= SAME_INPUT_BOUND
        assert e16 <= SAME_INPUT_BOUND + BF16_OUT


# ---- 3. the quantiser on the device is the host rule, bit for bit

def assert_is_host_rule(x_dev):
    c, s, _ = q_host(x_dev)
    gc, gs = ops().quantize_rows_mxfp6(x_dev)
    assert gc.dtype == torch.uint8 and gs.dtype == torch.uint8 and gc.shape == c.shape and gs.shape == s.shape
    assert torch.equal(gs.cpu(), s), (gs.cpu() != s).nonzero()[:4]
    assert torch.equal(gc.cpu(), c), (gc.cpu() != c).nonzero()[:4]
    return gc, gs


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
    """One block a row, K = 32, for 2^shared in {2^-20, 1, 2^13}: all 32 grid magnitudes in both signs; every tie of the three
    steps in both signs beside a 4.0 anchor; saturation (7.625, 7.75, 7.875); tiny negatives (code 32); an all-zero block;
    float32 subnormals (scale code 0)."""
    grid = torch.tensor([abs(v) for v in Q().MXFP6_VALUES[:32]])
    ties = torch.tensor([0.0625, 0.1875, 0.9375, 1.0625, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 7.25])
    rows = []
    for sh in (-20, 0, 13):
        a = torch.zeros(32)
        a[:11], a[11:22], a[22] = ties, -ties, 4.0
        sat = torch.zeros(32)
        sat[:8] = torch.tensor([7.625, -7.625, 7.75, -7.75, 7.875, -7.875, 7.5, -7.0])
        tiny = torch.full((32,), -2.0 ** -10)
        tiny[3], tiny[4] = 6.0, -0.0
        rows += [torch.ldexp(r, torch.tensor(sh)) for r in (grid, -grid, a, sat, tiny)]
    rows.append(torch.zeros(32))
    neg0 = torch.zeros(32)
    neg0[5] = -0.0
    rows.append(neg0)
    sub = torch.arange(32).float() * 2.0 ** -133 * torch.where(torch.arange(32) % 3 == 0, -1.0, 1.0)   # (bfloat16 holds these too)
    rows += [sub, sub * 4, torch.ldexp(torch.arange(32).float(), torch.tensor(-149))]
    x = torch.stack(rows).to(din)
    assert torch.equal(x.float()[:-1], torch.stack(rows)[:-1])                       # (all but the last row are bfloat16 values)
    gc, gs = assert_is_host_rule(x.to(DEV))
    gs, codes = gs.cpu()[:, 0], Q().unpack_mxfp6(gc.cpu())
    assert gs[0] == 127 - 20 and gs[5] == 127 and gs[10] == 127 + 13                 # 7.5 / anchor 4: shared = the exponent - 2
    assert codes[5].tolist() == list(range(32)) and codes[6].tolist() == list(range(32, 64))           # the grid is itself, -0 included
    assert codes[7, :11].tolist() == [0, 2, 8, 8, 16, 16, 18, 24, 24, 26, 30]        # ties go to the even neighbour
    assert codes[8, :8].tolist() == [31, 63, 31, 63, 31, 63, 31, 62]                 # 7.75 is a tie that goes up and saturates at 7.5
    assert codes[9, 0] == 32 and codes[9, 4] == 32                                   # a negative that rounds to zero keeps its sign
    assert gs[15] == 127 and int(codes[15].sum()) == 0 and gs[16] == 127 and codes[16, 5] == 32
    assert gs[17] == 0 and gs[18] == 0                                               # float32 subnormals: shared clamps at -127
    if din == torch.float32:
        assert gs[19] == 0


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantiser_marks_a_non_finite_block_and_only_it(din):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(9, 96, generator=g).to(din)
    clean = x.clone()
    bad = {(2, 1): float("inf"), (5, 0): NAN, (7, 2): float("-inf")}
    for (t, blk), v in bad.items():
        x[t, 32 * blk + 7] = v
        clean[t, 32 * blk + 7] = 0
    c, s, _ = q_host(clean)
    for (t, blk) in bad:
        c[t, 24 * blk:24 * blk + 24] = 0
        s[t, blk] = 255
    gc, gs = ops().quantize_rows_mxfp6(x.to(DEV))
    assert torch.equal(gs.cpu(), s) and torch.equal(gc.cpu(), c)


# ---- 4. random rows through the fused quantiser, and the format's own error

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_precision_fp6_is_the_quantiser_then_the_gemm_and_the_format_error(K, N):
    p = problem(K, N)
    for din in (torch.float32, torch.bfloat16):
        x = p["x"].to(din)
        c, s, _ = q_host(x)
        for bias in (False, True):
            assert same_bits(runq(p, x, bias=bias), run6(p, c.to(DEV), s.to(DEV), bias=bias)), (K, N, din, bias)
    got = runq(p, p["x"])
    fmt = rel_fro_dev(got, ref64(p, p["x_cpu"].double(), False))
    print(f"mxfp4-f6 K={K} N={N}: rel_fro against un-quantised float32 rows {fmt:.3e} (host {FORMAT_HOST[0]:.2e} .. {FORMAT_HOST[1]:.2e})")
    assert FORMAT_RANGE[0] <= fmt <= FORMAT_RANGE[1]


# ---- 5. the gated form

def step_index(codes):
    """Signed position on the e2m3 grid: +-(code & 31)."""
    mag = (codes & 31).to(torch.int32)
    return torch.where(codes >= 32, -mag, mag)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96])
def test_gated_op_is_the_quantiser_then_the_gemm(F, kind):
    p = problem(F, 40, seed=7)
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = (torch.randn(p["T"], 2 * F, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        gu = gate_up.to(din)
        got = rung(p, gu, kind)
        hc, hs = ops().quantize_rows_mxfp6(gu, **act_kw(kind))
        assert hc.shape == (p["T"], F // 4 * 3) and hs.shape == (p["T"], F // 32)
        assert same_bits(got, run6(p, hc, hs, bias=True))
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
        # the gated quantiser against quantize_mxfp6 of the float64 h
        c, s, _ = q_host(hidden64(kind, gu.cpu(), ALPHA, LIMIT))
        c_dev, c_ref = Q().unpack_mxfp6(hc.cpu()), Q().unpack_mxfp6(c)
        d_scale = hs.cpu() != s
        d_code = c_dev != c_ref
        print(f"mxfp4-f6 gated F={F} {kind} in={din}: {int(d_code.sum())} of {d_code.numel()} codes and "
              f"{int(d_scale.sum())} of {d_scale.numel()} scale bytes differ from the float64 h")
        assert d_code.float().mean() <= GATED_CODE_CAP and d_scale.float().mean() <= GATED_SCALE_CAP
        same_scale = (~d_scale).repeat_interleave(32, dim=1)
        off = d_code & same_scale
        assert bool(((step_index(c_dev) - step_index(c_ref)).abs()[off] == 1).all())


# ---- 6. tile against decode, bit for bit

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_tile_and_decode_return_the_same_bits(K, N, force):
    p = problem(K, N)
    c, s, _ = q_host(p["x"])
    xb, xs = c.to(DEV), s.to(DEV)
    outs = {}
    for form in FORMS:
        force(form)
        outs[form] = [run6(p, xb, xs, bias=bias, out_dtype=dt) for dt in DT for bias in (False, True)]
        outs[form].append(runq(p, p["x"].bfloat16(), bias=True))
    for a, b in zip(outs["tile"], outs["decode"]):
        assert same_bits(a, b), (K, N, a.dtype)
    assert bool(torch.isfinite(outs["tile"][0]).all()) and float(outs["tile"][0].abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_tile_and_decode_agree_on_the_gated_op(kind, force):
    p = problem(96, 40, seed=7)
    gate_up = (torch.randn(p["T"], 192, generator=torch.Generator().manual_seed(5)) * 2.0).to(DEV)
    force("tile")
    a = [rung(p, gate_up, kind), rung(p, gate_up.bfloat16(), kind, out_dtype=torch.bfloat16)]
    force("decode")
    b = [rung(p, gate_up, kind), rung(p, gate_up.bfloat16(), kind, out_dtype=torch.bfloat16)]
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_scale_codes_255_0_and_254_on_either_side(K, N, force):
    """Scale code 255 in one weight block: NaN in exactly that weight row for the rows of its expert; in one row block:
    NaN across exactly that row; codes 0 and 254 are 2^-127 and 2^127 (whatever their sums overflow to, it is the same in both
    forms and stays in their own weight rows and rows), checked exactly on one product alone."""
    p = problem(K, N)
    c, s, _ = q_host(p["x"])
    xb, xs = c.to(DEV), s.to(DEV)
    e, n, blk = 2, 5, K // 32 - 1
    t = p["offs_l"][3] + 40                                                          # a row of the second 32-row wave
    o, cnt = p["offs_l"][e], p["counts"][e]
    wsc = p["scales"].clone()
    wsc[e, n, blk] = 255
    xsc = xs.clone()
    xsc[t, blk] = 255
    ext_w, ext_x = p["scales"].clone(), xs.clone()
    ext_w[e, 1, 0], ext_w[e, 2, blk] = 0, 254
    ext_x[t, 0], ext_x[t + 1, blk] = 0, 254
    res = {}
    for form in FORMS:
        force(form)
        res[form] = (run6(p, xb, xs), run6(p, xb, xs, scales=wsc), run6(p, xb, xsc), run6(p, xb, ext_x, scales=ext_w))
    want, w255, x255, ext = res["tile"]
    for a, b in zip(res["tile"], res["decode"]):
        assert same_bits(a, b)
    expect = torch.zeros_like(want, dtype=torch.bool)
    expect[o:o + cnt, n] = True
    assert torch.equal(torch.isnan(w255), expect) and torch.equal(w255[~expect], want[~expect])
    expect = torch.zeros_like(want, dtype=torch.bool)
    expect[t] = True
    assert torch.equal(torch.isnan(x255), expect) and torch.equal(x255[~expect], want[~expect])
    untouched = torch.ones_like(want, dtype=torch.bool)
    untouched[o:o + cnt, 1:3] = False
    untouched[t:t + 2] = False
    assert torch.equal(ext[untouched], want[untouched])
    # one product alone under codes 0 and 254: 1.0 x 1.0 x 2^-127 x 2^0 is the float32 subnormal, x 2^127 is 2^127
    one_w = torch.zeros(1, 1, 16, dtype=torch.uint8, device=DEV)
    one_w[0, 0, 0] = 2                                                               # e2m1 1.0 at k = 0
    one_x = Q().pack_mxfp6(torch.tensor([[8] + [0] * 31], dtype=torch.uint8)).to(DEV)   # e2m3 1.0 at k = 0
    tab = (torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    for form in FORMS:
        force(form)
        for code, bits in ((0, 0x00400000), (254, 0x7F000000)):
            for side in ("weights", "rows"):
                ws_ = torch.tensor([[[code if side == "weights" else 127]]], dtype=torch.uint8, device=DEV)
                xs_ = torch.tensor([[code if side == "rows" else 127]], dtype=torch.uint8, device=DEV)
                v = ops().moe_forward_mxfp4_fp6(one_w, ws_, one_x, xs_, *tab)
                assert int(v.view(torch.int32)) == bits, (form, code, side)


# ---- 7. independence and footprint

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N, form, force):
    p = problem(K, N)
    force(form)
    got = runq(p, p["x"], bias=True)
    assert same_bits(got, runq(p, p["x"], bias=True))                                # two runs agree
    assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
    for e, (c, o) in enumerate(zip(p["counts"], p["offs_l"])):
        if c == 0:
            continue
        one = ops().moe_forward_mxfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["x"][o:o + c].contiguous(),
                                      torch.tensor([c], dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int32, device=DEV), bias=p["bias"][e:e + 1], precision="fp6")
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_forward_mxfp4(p["blocks"][perm], p["scales"][perm], p["x"], p["tpe"][perm], p["offs"][perm],
                                    bias=p["bias"][perm], precision="fp6")
    assert same_bits(again, got)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ["f6", "q6", "glu_q6"])
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [40, 201])
def test_entries_stay_inside_their_buffers(N, dout, entry, form, force):
    """Every pointer is the interior of a guarded buffer; out sits 4 bytes off a 16-byte boundary inside SENT and the
    workspace has exactly the reported size; in_codes sits 8 bytes off a 16-byte boundary (N = 201) or on one, and at K = 96
    every odd row is 8-byte aligned only.  Only [T, N] (and the workspace, but not its padding) changes, the guards stay, the
    operands are unchanged, uncovered rows are zero and the bits are the public op's.  The two entries with a workspace run
    on 0x5A and then once per stale workspace content of PREFILLS, with the same bits and the same workspace each time."""
    K = 96
    p = problem(K, N)
    E, T = p["E"], p["T"]
    force(form)
    st = torch.cuda.current_stream().cuda_stream
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert out.ptr % 16 == 4
    mode = {"f6": 0, "q6": 1, "glu_q6": 2}[entry]
    nbytes = lib().fql_moe_mx4_f6_workspace_bytes(E, T, K, N, mode)
    if entry == "f6":
        assert nbytes == 0
        c, s, _ = q_host(p["x"])
        xb, xs = c.to(DEV), s.to(DEV)
        rw = guarded_like("in_codes", xb, 0xFF, offset=16 if N == 40 else 8)         # (a guard byte that is used: -7.5s)
        assert rw.ptr % 16 == (0 if N == 40 else 8)
        sg = guarded_like("in_scales", xs, 0xFF, offset=1)                           # (... a NaN scale)
        rc = lib().fql_moe_mx4_fwd_f6(bl.ptr, sc.ptr, rw.ptr, sg.ptr, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                      None, 0, st)
        want = run6(p, xb, xs, bias=True, out_dtype=dout)
        bufs, ops_in = (bl, sc, rw, sg, bias, cnt, off, out), ((rw, xb), (sg, xs))
    else:
        used_b, used_s = T * K * 3 // 4, T * K // 32
        assert nbytes == (used_b + 15) // 16 * 16 + (used_s + 15) // 16 * 16 and used_s % 16 != 0
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        ws.bytes().fill_(0x5A)
        row_off = 16 if N == 40 else 4                                               # the 16-byte loads / the element loads
        if entry == "q6":
            rows = p["x"]
            rw = guarded_like("rows", rows, NAN, offset=row_off)
            call = lambda: lib().fql_moe_mx4_fwd_q6(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K,
                                                    N, ws.ptr, nbytes, st)
            rc = call()
            want = runq(p, rows, bias=True, out_dtype=dout)
            hb, hs = ops().quantize_rows_mxfp6(rows)
        else:
            g = torch.Generator().manual_seed(3)
            rows = torch.randn(T, 2 * K, generator=g).to(DEV)
            rw = guarded_like("rows", rows, NAN, offset=row_off)
            call = lambda: lib().fql_moe_mx4_glu_fwd_q6(bl.ptr, sc.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T,
                                                        K, N, ACT["swiglu_clamp"], ALPHA, LIMIT, ws.ptr, nbytes, st)
            rc = call()
            want = rung(p, rows, "swiglu_clamp", out_dtype=dout)
            hb, hs = ops().quantize_rows_mxfp6(rows, **act_kw("swiglu_clamp"))
        bufs, ops_in = (bl, sc, rw, bias, cnt, off, out, ws), ((rw, rows),)
    assert rc == 0
    assert_guards_intact(*bufs, what=f"mx4 f6 {entry} N={N} {dout} {form}")
    if entry != "f6":                                                                # the workspace: the rows, their scales, padding
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
    if entry != "f6":                               # what an earlier launch may have left in the workspace: the same bits
        for fill in PREFILLS:
            w.fill_(fill)
            got.fill_(SENT)
            assert call() == 0
            assert_guards_intact(*bufs, what=f"mx4 f6 {entry} N={N} {dout} {form} workspace {fill:#04x}")
            assert torch.equal(w[:used_b], hb.flatten()) and torch.equal(w[first:first + used_s], hs.flatten()), hex(fill)
            assert bool((w[used_b:first] == fill).all()) and bool((w[first + used_s:] == fill).all()), hex(fill)
            assert torch.count_nonzero(got[T - TAIL:]) == 0, hex(fill)
            assert same_bits(got, want), hex(fill)


def test_op_takes_rows_whose_base_is_8_byte_aligned_only(force):
    """in_codes as a view 8 bytes into a 16-byte aligned allocation: passed as it is (not copied), the same bits."""
    p = problem(96, 40)
    c, s, _ = q_host(p["x"])
    xb, xs = c.to(DEV), s.to(DEV)
    raw = torch.zeros(xb.numel() + 8, dtype=torch.uint8, device=DEV)
    view = raw[8:].view(xb.shape)
    view.copy_(xb)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    for form in FORMS:
        force(form)
        assert same_bits(run6(p, view, xs, bias=True), run6(p, xb, xs, bias=True)), form


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantize_rows_stays_inside_its_buffers(din, gated):
    """The quantiser's two outputs, [T][3K/4] and [T][K/32], are written in full and nothing around them; rows 16-byte
    aligned (the wide loads) and 4 bytes off (the element loads)."""
    T, K = 37, 96
    st = torch.cuda.current_stream().cuda_stream
    rows = torch.randn(T, (2 if gated else 1) * K, generator=torch.Generator().manual_seed(6)).to(din).to(DEV)
    kw = act_kw("gelu_tanh") if gated else {}
    wc, wsc = ops().quantize_rows_mxfp6(rows, **kw)
    for row_off in (16, 4):
        rw = guarded_like("rows", rows, NAN, offset=row_off)
        oc = Guarded("out_codes", T * K * 3 // 4, torch.uint8, 0x5A, offset=16)
        osc = Guarded("out_scales", T * K // 32, torch.uint8, 0x5A, offset=1)
        rc = lib().fql_mx6_quantize_rows(rw.ptr, DT[din], int(gated), ACT["gelu_tanh"], ALPHA, LIMIT, oc.ptr, osc.ptr, T, K, st)
        assert rc == 0
        assert_guards_intact(rw, oc, osc, what=f"mx6 quantize_rows {din} gated={gated} offset {row_off}")
        assert torch.equal(rw.view(rows.dtype, *rows.shape), rows)
        assert torch.equal(oc.view(torch.uint8, T, K * 3 // 4), wc) and torch.equal(osc.view(torch.uint8, T, K // 32), wsc)


def test_graph_replay_reuses_a_stale_workspace(force):
    """The op captured once (the decode kernel behind its pre-pass, whose workspace the graph's pool keeps), replayed after
    the rows and the table have changed in place: the bits of an eager call on the new contents by the other kernel."""
    p = problem(96, 40)
    T = p["T"]
    x, tpe, offs = p["x"].clone(), p["tpe"].clone(), p["offs"].clone()
    call = lambda x, tpe, offs: ops().moe_forward_mxfp4(p["blocks"], p["scales"], x, tpe, offs, bias=p["bias"], precision="fp6")
    force("decode")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            call(x, tpe, offs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call(x, tpe, offs)
    graph.replay()
    torch.cuda.synchronize()
    force("tile")
    assert same_bits(out, call(x, tpe, offs))
    t2, o2, _ = expert_table([40, 30, 0, 32], tail=4)
    x.copy_(torch.randn(T, 96, generator=torch.Generator().manual_seed(77)).to(DEV) * 3.0)
    tpe.copy_(t2)
    offs.copy_(o2)
    want = call(x, tpe, offs)                                        # eager, the tile kernel, the new contents
    graph.replay()                                                   # (the workspace still holds the first rows' codes)
    torch.cuda.synchronize()
    assert same_bits(out, want)
    assert torch.count_nonzero(out[T - 4:]) == 0 and float(out[:T - 4].abs().max()) > 0


# ---- 8. layer and block

def ffn_weights(E, H, F, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    return dict(gate=mk(F, H), up=mk(F, H), down=mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_is_the_two_ops_composed(dt, with_bias):
    E, H, F = 4, 64, 96
    w = ffn_weights(E, H, F)
    biases = dict(gate_bias=w["gate_bias"], up_bias=w["up_bias"], down_bias=w["down_bias"]) if with_bias else {}
    make = lambda **kw: fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], activation_dtype=dt, **biases,
                                                      **act_kw("swiglu_clamp"), **kw).to(DEV)
    m, base = make(precision="fp6"), make()
    assert list(m.state_dict()) == list(base.state_dict())
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(2)).to(DEV).to(dt or torch.float32)
    b_gu, b_d = (m.gate_up_bias.detach(), m.down_bias.detach()) if with_bias else (None, None)
    got = m(x, tpe, offs)
    gate_up = ops().moe_forward_mxfp4(m.gate_up_blocks, m.gate_up_scales, x, tpe, offs, bias=b_gu, precision="fp6")
    want = ops().moe_gated_forward_mxfp4(m.down_blocks, m.down_scales, gate_up, tpe, offs, bias=b_d, precision="fp6",
                                         **act_kw("swiglu_clamp"))
    assert got.dtype == x.dtype and same_bits(got, want)
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True), tpe, offs)
    assert not same_bits(got, base(x, tpe, offs))                                    # (the two modes are different numbers)


def test_block_with_fp6_mxfp4_experts_against_torch():
    """E = 4, top-2, H = 64, F = 96, swiglu_clamp, expert and router biases, seeded gate, under no_grad.  Reference: a torch
    block on the dequantised weights with the rows of both GEMMs (x, then h) quantised by quantize_mxfp6, the routing taken
    from the block's own router."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    E, H, F, T = 4, 64, 96, 50
    w = ffn_weights(E, H, F, seed=9)
    experts = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                            down_bias=w["down_bias"], precision="fp6", **act_kw("swiglu_clamp"))
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
    print(f"mxfp4-f6 block: rel_fro {err:.3e} (bound {BLOCK_BOUND:.1e})")
    assert err <= BLOCK_BOUND
    with pytest.raises(RuntimeError, match="inference-only"):
        blk(x.clone().requires_grad_(True))
