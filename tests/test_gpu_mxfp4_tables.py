"""The grouped MXFP4 kernels on many experts and on hostile expert tables, on the GPU.  Every grouped MXFP4 kernel
(mx4_kernel, mx4_decode_kernel, mx4_scaled_kernel<ROWS> and mx4_sdecode_kernel<ROWS> for e4m3, MXFP4 and MXFP6 rows,
mx4_bwd_kernel) starts with mx4_group_begin (csrc/fql_mx4_common.h): expert_range reads and clips the expert's rows, the
workgroup decides whether it has work, and the z-slice past the experts runs act_zero_uncovered, which scans the table 64
experts at a time (expert_chunk, with carries between chunks) and zeroes the rows no expert owns.  The sibling files feed
that preamble one ascending table of at most five experts each; this file feeds it the tables below, through every
kernel and both forms of each forward (fql_tune_set_mx4_decode_max_rows, fql_tune_set_mx4_scaled_decode_max_rows,
fql_tune_set_mx4_f6_decode_max_rows), against helpers.clipped_ranges: the contract of include/fql_int4.h, "ranges are
clipped to [0, T]; they must not overlap; rows no expert covers are zero".  Overlapping ranges are outside the contract
and are not tested; every table is asserted not to overlap when it is built (helpers.hostile_table).

The tables (a dot is a row no expert covers):
  * e65: 65 experts, [. . e0:1 e63:33 . . e64:3 .].  Expert 64 is the only lane of the second scan chunk: a scan that
    stops after one chunk zeroes its rows, a kernel that takes a chunk's lane for the expert misses it.
  * e130-descending: 130 experts of one row, expert e on row T - 2 - e: three chunks, the last one partial, offsets that
    descend (nothing may assume a sorted table), one uncovered row at each end.
  * e128-decode: T = 8, eight experts spread over both chunks own one row each, 120 are empty: a decode step of a
    128-expert model, the shape the 8-row decode thresholds were set for.  Also run with no threshold forced.
  * clipped: T = 40 with (offset, count) = (-3, 5) -> [0, 2); (2, 0), (10, -4), (50, 3), (INT_MAX, INT_MAX) and
    (INT_MIN, INT_MAX) -> empty; (30, 999) -> [30, 40).  Rows 2 .. 29 are uncovered.  The sums overflow 32 bits.
  * gaps-descending: counts [33, 0, 70, 1] laid out from the last expert to the first with 3 uncovered rows in front,
    5 between neighbours and 2 behind: the 70-row expert starts at row 9 (no multiple of 32 or 64) and crosses a wave and
    a workgroup boundary inside its own range.
  * all-empty: three empty experts over 5 rows: the result is all-zero bits.
  * one-expert-inside: one expert on [1, T - 1) of T = 35: E = 1 WITH a table that does not cover everything.

Shapes: K = 96, N = 40 for all (three scale blocks: a half-filled tail instruction; a partial second 32-column
fragment); e65 and gaps-descending also at K = 288, N = 136 (two stages plus a tail block; a second 128-column
workgroup).

One operand set makes every kernel exact.  Weights: random e2m1 codes over all 16 values with scale codes in [125, 129].
Rows: values of the signed e2m1 grid {0, 1, 2, 3, 4, 6} times 2^(s - 127) with s in [126, 128] drawn per block of 32:
exactly bfloat16 values, MXFP4 rows (e2m1 codes, scale s), MXFP6 rows (e2m3 codes, scale s) and, divided by a per-row
act_scale drawn from {0.5, 1, 2}, e4m3 bytes (all asserted on the host).  Bias: integers in [-8, 8].  Every product is a
multiple of 2^-4 (2^-5 for the e4m3 bytes, whose sums are at most twice as large) and every sum stays below
288 x 24 x 12 < 2^17 (asserted), so every partial sum is exact in float32 (2^18 / 2^-5 = 2^23 < 2^24) and the result is the
float64 reference bit for bit whatever the adder does; a bfloat16 result is one rounding of it.  The backward uses the
same grid for grad_out (an exponent per element), and its sums over N <= 136 stay below 2^16 (asserted).

The fused adapter entries (ops.moe_forward_mxfp4_lora / moe_gated_forward_mxfp4_lora / moe_backward_input_mxfp4_lora: the
LORA stage of mx4_kernel and mx4_bwd_kernel) index the shrunk rows v[t] and the adapter matrix B[e] / A[e] by the same
clamped row and expert as the base product, so they run through the same tables with the same operand set enlarged: v
and dv [T, r] integers in [-4, 4], B [E, N, r] and A [E, r, K] integers in [-2, 2], r = 4 at K = 96 (less than one 16-j
step) and 64 at K = 288 (all four).  The adapter adds at most 64 x 4 x 2 = 2^9 to a sum, which keeps the sums below
2^17 and 2^16 (asserted on the enlarged references).

Input rows no expert covers are NaN in every operand (float rows, the shrunk rows v and dv, scale code 255, NaN act_scale and NaN e4m3 bytes).
By the code, a lane past an expert's count re-reads that expert's last row (row_lo + cnt - 1: the clamp of tx / ty / t
in all five kernels), so an uncovered row is never an operand of a covered one; a kernel that read "the next row"
instead would put a NaN into a covered row here.  Uncovered output rows are checked as bits (-0.0 or a NaN payload is
not zero).  After every call the two table tensors equal their host copies."""
import functools

import pytest
import torch

from glu_reference import act_kw
from helpers import HOSTILE_TABLES, NAN, bits, hostile_table, ops, same_bits, uncovered_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_MAX = 2 ** 31 - 1
PRECISIONS = ["bf16", "fp8", "fp4", "fp6"]
FORMS = ["tile", "decode"]
CASES = [(t, 96, 40) for t in HOSTILE_TABLES] + [(t, 288, 136) for t in ("e65", "gaps-descending")]
CASE_IDS = [f"{t}-K{K}-N{N}" for t, K, N in CASES]
GRID = [0, 1, 2, 3, 4, 6]
LORA_RANK = {96: 4, 288: 64}                                           # the adapters' rank at each K of CASES
E2M1_CODE, E2M3_CODE = [0, 2, 4, 5, 6, 7], [0, 8, 16, 20, 24, 28]      # the codes of GRID's magnitudes


def lib():
    from fused_int4_amd import _native
    return _native.lib()


def setters():
    L = lib()
    return {"bf16": L.fql_tune_set_mx4_decode_max_rows, "fp8": lambda r: L.fql_tune_set_mx4_scaled_decode_max_rows(1, r),
            "fp4": lambda r: L.fql_tune_set_mx4_scaled_decode_max_rows(2, r), "fp6": L.fql_tune_set_mx4_f6_decode_max_rows}


def reported(precision, p):
    """1: the library takes the decode kernel of ``precision`` for the problem's shape, 0: the tile kernel."""
    L, shape = lib(), (p["E"], p["T"], p["K"], p["N"])
    if precision == "bf16":
        return L.fql_tune_mx4_kernel(*shape)
    if precision == "fp6":
        return L.fql_tune_mx4_f6_kernel(*shape)
    return L.fql_tune_mx4_scaled_kernel({"fp8": 1, "fp4": 2}[precision], *shape)


@pytest.fixture
def force():
    """force(precision, "decode" | "tile"); the library's own thresholds come back afterwards."""
    s = setters()
    default = {k: f(-1) for k, f in s.items()}                      # (a negative value changes nothing)

    def use(precision, form):
        s[precision]({"decode": INT_MAX, "tile": 0}[form])
    try:
        yield use
    finally:
        for k, f in s.items():
            f(default[k])


def grid_values(g, shape, exps):
    """Signed values of GRID times 2^exps (broadcast) -> (float32 values, index into GRID, sign bit)."""
    idx = torch.randint(0, 6, shape, generator=g)
    neg = torch.randint(0, 2, shape, generator=g)
    v = torch.tensor(GRID, dtype=torch.float32)[idx] * torch.exp2(exps)
    return torch.where(neg == 1, -v, v), idx, neg


@functools.lru_cache(maxsize=None)
def problem(table, K, N):
    """The operands of the docstring for one table and shape, with the float64 references ``ref`` / ``ref_b`` (with the
    bias) [T, N] and ``ref_bwd`` [T, K], zero outside every clipped range.  Computed once and shared; nobody writes to it."""
    from fused_int4_amd import quantize as Q
    tpe, offs, T, ranges = hostile_table(table)
    E = len(ranges)
    g = torch.Generator().manual_seed(100003 * HOSTILE_TABLES.index(table) + 1000 * K + N)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(125, 130, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = Q.pack_nibbles(codes)
    W = Q.dequantize_mxfp4(blocks, scales).double()
    bias = torch.randint(-8, 9, (E, N), generator=g).float()
    unc = uncovered_mask(ranges, T)
    # the rows, once per format
    xs = torch.randint(126, 129, (T, K // 32), generator=g, dtype=torch.uint8)
    x, idx, neg = grid_values(g, (T, K), (xs.float() - 127).repeat_interleave(32, dim=1))
    xb4 = Q.pack_nibbles((torch.tensor(E2M1_CODE)[idx] + 8 * neg).to(torch.uint8))
    xb6 = Q.pack_mxfp6((torch.tensor(E2M3_CODE)[idx] + 32 * neg).to(torch.uint8))
    a8 = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (T,), generator=g)]
    x8 = (x / a8[:, None]).to(torch.float8_e4m3fn)
    assert torch.equal(x.bfloat16().float(), x)
    assert torch.equal(Q.dequantize_mxfp4(xb4, xs), x) and torch.equal(Q.dequantize_mxfp6(xb6, xs), x)
    assert torch.equal(x8.float() * a8[:, None], x)
    grad, _, _ = grid_values(g, (T, N), torch.randint(-1, 2, (T, N), generator=g).float())
    assert torch.equal(grad.bfloat16().float(), grad)
    xr = torch.randn(T, K, generator=g)                                 # seeded random rows: the quantise-then-GEMM ops
    gate_up = torch.randn(T, 2 * K, generator=g) * 2.0
    # the float64 references, from the clean rows of every range
    ref, ref_b, ref_bwd = (torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64),
                           torch.zeros(T, K, dtype=torch.float64))
    for e, (lo, hi) in enumerate(ranges):
        ref[lo:hi] = x[lo:hi].double() @ W[e].T
        ref_b[lo:hi] = ref[lo:hi] + bias[e].double()
        ref_bwd[lo:hi] = grad[lo:hi].double() @ W[e]
    assert float(ref.abs().max()) < 2 ** 17 and float(ref_b.abs().max()) < 2 ** 17 and float(ref_bwd.abs().max()) < 2 ** 16
    assert torch.equal(ref * 16, (ref * 16).round()) and torch.equal(ref_bwd * 16, (ref_bwd * 16).round())
    # the adapter operands (a generator of their own: the operands above keep their values) and the enlarged references
    r = LORA_RANK[K]
    ga = torch.Generator().manual_seed(100003 * HOSTILE_TABLES.index(table) + 1000 * K + N + 500009)
    v, dv = torch.randint(-4, 5, (T, r), generator=ga).float(), torch.randint(-4, 5, (T, r), generator=ga).float()
    B, A = torch.randint(-2, 3, (E, N, r), generator=ga).float(), torch.randint(-2, 3, (E, r, K), generator=ga).float()
    ref_lora, ref_lora_bwd = ref.clone(), ref_bwd.clone()
    for e, (lo, hi) in enumerate(ranges):
        ref_lora[lo:hi] += v[lo:hi].double() @ B[e].double().T
        ref_lora_bwd[lo:hi] += dv[lo:hi].double() @ A[e].double()
    ref_lora_b = ref_lora + (ref_b - ref)
    assert max(float(ref_lora.abs().max()), float(ref_lora_b.abs().max())) < 2 ** 17 and float(ref_lora_bwd.abs().max()) < 2 ** 16
    assert bool(unc.all()) or not (torch.equal(ref_lora, ref) or torch.equal(ref_lora_bwd, ref_bwd))   # (the adapter matters)
    # the rows no expert covers are NaN in every operand
    xs_nan, x8b = xs.clone(), x8.view(torch.uint8).clone()
    for t in (x, grad, xr, gate_up, a8, v, dv):
        t[unc] = NAN
    xs_nan[unc] = 255
    x8b[unc] = 0x7F
    dev = lambda *ts: [t.to(DEV) for t in ts]
    p = dict(table=table, E=E, T=T, K=K, N=N, r=r, ranges=ranges, unc=unc, tpe_cpu=tpe, offs_cpu=offs, ref=ref, ref_b=ref_b,
             ref_bwd=ref_bwd, ref_lora=ref_lora, ref_lora_b=ref_lora_b, ref_lora_bwd=ref_lora_bwd)
    for name, t in zip(("tpe", "offs", "blocks", "scales", "bias", "x", "xb4", "xb6", "xs", "x8", "a8", "grad", "xr", "gate_up",
                        "v", "dv", "B", "A"),
                       dev(tpe, offs, blocks, scales, bias, x, xb4, xb6, xs_nan, x8b, a8, grad, xr, gate_up, v, dv, B, A)):
        p[name] = t
    return p


def table_intact(p):
    """The two table tensors still hold what the host built."""
    return torch.equal(p["tpe"].cpu(), p["tpe_cpu"]) and torch.equal(p["offs"].cpu(), p["offs_cpu"])


def uncovered_all_zero_bits(p, got):
    """Through an integer view: -0.0 and NaN payloads are not zero."""
    return got.shape[0] == p["T"] and int(torch.count_nonzero(bits(got.cpu())[p["unc"]])) == 0


def assert_is_reference(p, got, ref, what):
    assert table_intact(p), what
    if got.dtype == torch.float32:
        assert torch.equal(got.cpu().double(), ref), what
    else:
        assert same_bits(got.cpu(), ref.float().bfloat16()), what                # one rounding of the exact value
    assert uncovered_all_zero_bits(p, got), what
    if p["table"] == "all-empty":
        assert int(torch.count_nonzero(bits(got.cpu()))) == 0, what


def run_pre(precision, p, bias, out_dtype, rows_dtype=torch.float32):
    """The plain bfloat16 entry, or the pre-quantised entry of ``precision``, on the exact operands."""
    o = ops()
    w, t, kw = (p["blocks"], p["scales"]), (p["tpe"], p["offs"]), dict(bias=p["bias"] if bias else None, out_dtype=out_dtype)
    if precision == "bf16":
        return o.moe_forward_mxfp4(*w, p["x"].to(rows_dtype), *t, **kw)
    if precision == "fp8":
        return o.moe_forward_mxfp4_fp8(*w, p["x8"], p["a8"], *t, **kw)
    if precision == "fp4":
        return o.moe_forward_mxfp4_fp4(*w, p["xb4"], p["xs"], *t, **kw)
    return o.moe_forward_mxfp4_fp6(*w, p["xb6"], p["xs"], *t, **kw)


def check_exact(p, precision):
    for rows_dtype in ((torch.float32, torch.bfloat16) if precision == "bf16" else (None,)):
        for bias in (False, True):
            for out_dtype in (torch.float32, torch.bfloat16):
                got = run_pre(precision, p, bias, out_dtype, rows_dtype)
                assert got.dtype == out_dtype and got.shape == (p["T"], p["N"])
                assert_is_reference(p, got, p["ref_b"] if bias else p["ref"], (p["table"], precision, rows_dtype, bias, out_dtype))


@functools.lru_cache(maxsize=None)
def whole_table(rows):
    """A table of one expert that covers all of ``rows`` rows."""
    return torch.tensor([rows], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


def quantising_ops(precision):
    """(name, rows' key, op(blocks, scales, rows, tpe, offs, bias)) of the quantise-then-GEMM ops of ``precision``."""
    o = ops()
    out = [("gated", "gate_up", lambda b, s, r, t, f, bias: o.moe_gated_forward_mxfp4(b, s, r, t, f, bias=bias, precision=precision,
                                                                                     **act_kw("swiglu_clamp")))]
    if precision != "bf16":                                          # (the plain bfloat16 entry is checked exactly instead)
        out.append(("plain", "xr", lambda b, s, r, t, f, bias: o.moe_forward_mxfp4(b, s, r, t, f, bias=bias, precision=precision)))
    return out


def check_grouped_is_one_expert_calls(p, precision):
    """On seeded random rows (NaN where no expert covers): the grouped call has the bits of one call per expert on that
    expert's clipped slice, scattered into zeros."""
    for name, key, op in quantising_ops(precision):
        got = op(p["blocks"], p["scales"], p[key], p["tpe"], p["offs"], p["bias"])
        assert table_intact(p), (name, precision)
        assert got.dtype == torch.float32 and got.shape == (p["T"], p["N"])
        want = torch.zeros_like(got)
        for e, (lo, hi) in enumerate(p["ranges"]):
            if hi > lo:
                want[lo:hi] = op(p["blocks"][e:e + 1], p["scales"][e:e + 1], p[key][lo:hi].contiguous(), *whole_table(hi - lo),
                                 p["bias"][e:e + 1])
        assert bool(torch.isfinite(want).all()), (name, precision)                   # (the slices hold no uncovered row)
        assert same_bits(got, want), (p["table"], name, precision, (bits(got) != bits(want)).nonzero()[:4].tolist())
        assert uncovered_all_zero_bits(p, got), (name, precision)
        if bool((~p["unc"]).any()):
            assert float(got.abs().max()) > 0


# ---- 0. the tables are the ones the docstring describes

def test_tables_are_as_described():
    rows = lambda name: uncovered_mask(hostile_table(name)[3], hostile_table(name)[2]).nonzero().flatten().tolist()
    tpe, offs, T, ranges = hostile_table("e65")
    assert len(ranges) == 65 and T == 42 and rows("e65") == [0, 1, 36, 37, 41]
    assert (ranges[0], ranges[63], ranges[64]) == ((2, 3), (3, 36), (38, 41)) and int(tpe.count_nonzero()) == 3
    tpe, offs, T, ranges = hostile_table("e130-descending")
    assert len(ranges) == 130 and rows("e130-descending") == [0, T - 1]
    assert ranges == [(T - 2 - e, T - 1 - e) for e in range(130)] and bool((offs[1:] < offs[:-1]).all())
    tpe, offs, T, ranges = hostile_table("e128-decode")
    owners = [e for e, (lo, hi) in enumerate(ranges) if hi > lo]
    assert len(ranges) == 128 and T == 8 and rows("e128-decode") == [] and len(owners) == 8
    assert min(owners) < 64 <= max(owners) and sorted(ranges[e][0] for e in owners) == list(range(8))
    tpe, offs, T, ranges = hostile_table("clipped")
    assert T == 40 and [r for r in ranges if r[1] > r[0]] == [(0, 2), (30, 40)] and rows("clipped") == list(range(2, 30))
    assert [r[1] > r[0] for r in ranges] == [True, False, False, True, False, False, False]
    tpe, offs, T, ranges = hostile_table("gaps-descending")
    assert tpe.tolist() == [33, 0, 70, 1] and bool((offs[1:] < offs[:-1]).all()) and ranges[2] == (9, 79) and T == 124
    assert rows("gaps-descending") == [0, 1, 2] + list(range(4, 9)) + list(range(79, 89)) + [122, 123]
    assert rows("all-empty") == list(range(5)) and len(hostile_table("all-empty")[3]) == 3
    assert hostile_table("one-expert-inside")[3] == [(1, 34)] and rows("one-expert-inside") == [0, 34]


# ---- 1. the plain and the pre-quantised entries against float64, exactly

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_forward_is_the_float64_reference(table, K, N, precision, form, force):
    """ops.moe_forward_mxfp4 (float32 and bfloat16 rows), ops.moe_forward_mxfp4_fp8 / _fp4 / _fp6, with and without bias, a
    float32 and a bfloat16 result, under the tile and under the decode kernel."""
    p = problem(table, K, N)
    force(precision, form)
    assert reported(precision, p) == FORMS.index(form)
    check_exact(p, precision)


@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_backward_is_the_float64_reference(table, K, N):
    """ops.moe_backward_input_mxfp4 (one kernel form): grad_in [T, K] from float32 and bfloat16 gradient rows."""
    p = problem(table, K, N)
    for rows_dtype in (torch.float32, torch.bfloat16):
        for out_dtype in (torch.float32, torch.bfloat16):
            got = ops().moe_backward_input_mxfp4(p["blocks"], p["scales"], p["grad"].to(rows_dtype), p["tpe"], p["offs"],
                                                 out_dtype=out_dtype)
            assert got.dtype == out_dtype and got.shape == (p["T"], K)
            assert_is_reference(p, got, p["ref_bwd"], (table, "bwd", rows_dtype, out_dtype))


# ---- 2. the quantise-then-GEMM ops: the grouped call is the one-expert calls, bit for bit

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_grouped_equals_one_expert_calls(table, K, N, precision, form, force):
    """ops.moe_forward_mxfp4(precision="fp8" | "fp6" | "fp4") and ops.moe_gated_forward_mxfp4 (swiglu_clamp) in all four
    precisions, the grouped call and the one-expert calls under the same kernel form."""
    p = problem(table, K, N)
    force(precision, form)
    check_grouped_is_one_expert_calls(p, precision)


# ---- 3. the fused adapter entries: v[t] and B[e] / A[e] under the same clamped row and expert

@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_lora_forward_and_backward_are_the_float64_reference(table, K, N):
    """ops.moe_forward_mxfp4_lora (with and without bias) and ops.moe_backward_input_mxfp4_lora on the exact operands, from
    float32 and bfloat16 rows, a float32 and a bfloat16 result: the float32 result is the float64 reference bit for bit, a
    bfloat16 result one rounding of it, uncovered rows are zero bits although their x, v and dv are NaN, and the table
    tensors are unchanged."""
    p = problem(table, K, N)
    w, t = (p["blocks"], p["scales"]), (p["tpe"], p["offs"])
    for rows_dtype in (torch.float32, torch.bfloat16):
        for out_dtype in (torch.float32, torch.bfloat16):
            for bias in (False, True):
                got = ops().moe_forward_mxfp4_lora(*w, p["x"].to(rows_dtype), p["v"], p["B"], *t, bias=p["bias"] if bias else None,
                                                   out_dtype=out_dtype)
                assert got.dtype == out_dtype and got.shape == (p["T"], N)
                assert_is_reference(p, got, p["ref_lora_b"] if bias else p["ref_lora"], (table, "lora fwd", rows_dtype, bias, out_dtype))
            got = ops().moe_backward_input_mxfp4_lora(*w, p["grad"].to(rows_dtype), p["dv"], p["A"], *t, out_dtype=out_dtype)
            assert got.dtype == out_dtype and got.shape == (p["T"], K)
            assert_is_reference(p, got, p["ref_lora_bwd"], (table, "lora bwd", rows_dtype, out_dtype))


@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_lora_grouped_equals_one_expert_calls(table, K, N):
    """The three adapter entries (the gated one on the seeded random gate | up rows, swiglu_clamp): the grouped call has the
    bits of one call per expert on that expert's clipped slice of the rows and of v / dv with that expert's B / A,
    scattered into zeros."""
    p = problem(table, K, N)
    o = ops()
    entries = [("fwd", "x", "v", "B", lambda b, s, r, v, m, t, f, bias: o.moe_forward_mxfp4_lora(b, s, r, v, m, t, f, bias=bias,
                                                                                              out_dtype=torch.float32)),
               ("gated", "gate_up", "v", "B", lambda b, s, r, v, m, t, f, bias: o.moe_gated_forward_mxfp4_lora(
                   b, s, r, v, m, t, f, bias=bias, out_dtype=torch.float32, **act_kw("swiglu_clamp"))),
               ("bwd", "grad", "dv", "A", lambda b, s, r, v, m, t, f, bias: o.moe_backward_input_mxfp4_lora(b, s, r, v, m, t, f))]
    for name, rows, vk, mk, op in entries:
        got = op(p["blocks"], p["scales"], p[rows], p[vk], p[mk], p["tpe"], p["offs"], p["bias"])
        assert table_intact(p), name
        assert got.dtype == torch.float32 and got.shape == (p["T"], K if name == "bwd" else N)
        want = torch.zeros_like(got)
        for e, (lo, hi) in enumerate(p["ranges"]):
            if hi > lo:
                want[lo:hi] = op(p["blocks"][e:e + 1], p["scales"][e:e + 1], p[rows][lo:hi].contiguous(), p[vk][lo:hi].contiguous(),
                                 p[mk][e:e + 1], *whole_table(hi - lo), p["bias"][e:e + 1])
        assert bool(torch.isfinite(want).all()), name                                # (the slices hold no uncovered row)
        assert same_bits(got, want), (table, name, (bits(got) != bits(want)).nonzero()[:4].tolist())
        assert uncovered_all_zero_bits(p, got), name
        if bool((~p["unc"]).any()):
            assert float(got.abs().max()) > 0


# ---- 4. a decode step of a 128-expert model under the library's own thresholds

@pytest.mark.parametrize("precision", PRECISIONS)
def test_e128_decode_step_under_the_default_dispatch(precision):
    """T = 8 rows over 128 experts with no threshold forced: the library reports the decode kernel in every precision, and
    both checks hold through the dispatcher as a caller gets it."""
    p = problem("e128-decode", 96, 40)
    assert setters()[precision](-1) >= p["T"]                        # (the threshold a clean process has)
    assert reported(precision, p) == 1
    check_exact(p, precision)
    check_grouped_is_one_expert_calls(p, precision)
