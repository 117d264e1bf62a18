"""The grouped NVFP4 kernels on many experts and on hostile expert tables, on the GPU: tests/test_gpu_mxfp4_tables.py for
nv4_kernel, nv4_decode_kernel (csrc/fql_gemm_nvfp4.h) and nv4_bwd_kernel (csrc/fql_gemm_nvfp4_bwd.h).  All three start with
mx4_group_begin (csrc/fql_mx4_common.h) as the MXFP4 kernels do, and add per-expert operands of their own: the scale bytes
[E][N][K / 16] and global_scale[E], both indexed by blockIdx.z.  The feature files run four of the seven tables of
helpers.HOSTILE_TABLES at one shape through the plain forward and the backward; here all seven, and the two larger
cases, go through the plain forward and the gated forward under both kernel forms and through the backward: that file's
CASES (its docstring describes the tables), its ``table_intact``, and helpers.clipped_ranges for what the contract of
include/fql_int4.h says: "ranges are clipped to [0, T]; they must not overlap; rows no expert covers are zero".

The operands are the integer recipe of test_gpu_nvfp4.table_problem (test_gpu_nvfp4_bwd.table_problem for the gradient):
integer rows in [-4, 4], random e2m1 codes, scale bytes 0x30 .. 0x47 (0.5 .. 3.75), a power-of-two global scale that
differs between neighbouring experts, an integer bias.  Every product is a multiple of 2^-5 and every sum stays below 2^16
(2^15 in the backward; both asserted where the problems are built), so the float32 result is the float64 reference bit for
bit whatever the adder does, and a bfloat16 result is one rounding of it.  A global scale or a scale row taken under the
wrong expert (a scan chunk's lane instead of the expert, a clamp to the wrong neighbour) changes the result by a power of
two or by another random row.  The rows no expert covers are NaN in every input; uncovered output rows are checked as bits.
The gated entry has no exact recipe (its h is rounded to bfloat16): Gaussian gate | up rows against the float64 product of
the bfloat16-rounded float64 h at test_gpu_nvfp4.GATED_BOUND, as that file's gated test; the rows are first moved off
the points where that rounding is not defined at float32's resolution (near_a_bfloat16_tie).  After every call the two table
tensors equal their host copies.

The fused adapter entries (ops.moe_forward_nvfp4_lora / moe_gated_forward_nvfp4_lora / moe_backward_input_nvfp4_lora: the LORA
stage of nv4_kernel and nv4_bwd_kernel) index the shrunk rows v[t] / dv[t] by the absolute row and B[e] / A[e] by the expert,
next to the base kernels' own indexing, so they run through the same nine cases with the operand set enlarged as in
tests/test_gpu_mxfp4_tables.py: v and dv [T, r] integers in [-4, 4] (NaN on the rows no expert covers), B [E, N, r] and
A [E, r, K] integers in [-2, 2], r = that file's LORA_RANK (4 at K = 96, 64 at K = 288).  The global scale applies to the
weight term only: S = acc * g_e + sum_j v[t][j] B[e][n][j].  A weight term is a multiple of g_e * 2^-5 and every other term
an integer; the sum of the absolute values of all terms of one output is asserted below 2^24 of that unit where the
problem is built, so the float32 result is the float64 reference bit for bit."""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import NAN, bits, ops, rel_fro_dev, same_bits
from test_gpu_mxfp4_tables import CASE_IDS, CASES, LORA_RANK, table_intact, uncovered_all_zero_bits, whole_table
from test_gpu_nvfp4 import FORMS, GATED_BOUND, epilogue, force, lib, table_problem  # noqa: F401  (force: the fixture)
from test_gpu_nvfp4_bwd import table_problem as bwd_table_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
KIND = "swiglu_clamp"


TIE_MARGIN = 2.0 ** -20            # 16 float32 ulps, relative


def near_a_bfloat16_tie(h64):
    """bool, h64's shape: the float64 h lies within TIE_MARGIN (relative) of the midpoint of two neighbouring bfloat16
    values.  There the reference's rounding of h to bfloat16 is not defined at the resolution of the float32 h the op
    forms: a float32 h one ulp away rounds to the other neighbour, which moves that row of the result by 2^-8 of the
    element (on the e65 table, with 3552 elements of h, one such element at 0.9 float32 ulps from a midpoint put the whole
    comparison at 1.8e-4).  The rows are moved off such points from the reference alone, before any kernel runs, so that
    GATED_BOUND keeps its meaning: an h that is off by more than a few float32 ulps still lands on the wrong side
    somewhere and fails."""
    a = h64.abs().double()
    ulp = torch.exp2(torch.floor(torch.log2(a.clamp(min=2.0 ** -126))) - 7)          # the spacing of bfloat16 at |h|
    frac = torch.remainder(a / ulp, 1.0)
    return ((frac - 0.5).abs() * ulp <= TIE_MARGIN * a) & (a > 0)


@functools.lru_cache(maxsize=None)
def problem(table, K, N):
    """test_gpu_nvfp4.table_problem and test_gpu_nvfp4_bwd.table_problem of one case (the same weights: asserted), with
    Gaussian gate | up rows [T, 2 K] (NaN where no expert covers; an up value whose h lies near_a_bfloat16_tie, from
    float32 or bfloat16 rows, is multiplied by 1 + 2^-6 until none does) and their reference per row type (h is formed
    from the rows as the op gets them).  Computed once; nobody writes to it."""
    p, b = dict(table_problem(table, K, N)), bwd_table_problem(table, K, N)
    assert all(torch.equal(u, v) for u, v in zip(p["args"][:3], b["args"][:3])) and torch.equal(p["unc"], b["unc"])
    blocks, scales, gs, x, tpe, offs = p["args"]
    g = torch.Generator().manual_seed(7919 * p["T"] + K + N)
    gate_up = torch.randn(p["T"], 2 * K, generator=g) * 2.0
    for _ in range(8):                               # (see near_a_bfloat16_tie: one pass is enough at these sizes)
        near = (near_a_bfloat16_tie(hidden64(KIND, gate_up, ALPHA, LIMIT))
                | near_a_bfloat16_tie(hidden64(KIND, gate_up.bfloat16(), ALPHA, LIMIT)))
        if not bool(near.any()):
            break
        gate_up[:, K:][near] *= 1.0 + 2.0 ** -6
    assert not bool(near.any())
    ref_glu = {}
    for din in (torch.float32, torch.bfloat16):
        h = hidden64(KIND, gate_up.to(din), ALPHA, LIMIT).bfloat16().double()       # the bf16-rounded reference h
        ref_glu[din] = torch.zeros(p["T"], N, dtype=torch.float64)
        for e, (lo, hi) in enumerate(p["ranges"]):
            if hi > lo:
                ref_glu[din][lo:hi] = epilogue(h[lo:hi] @ p["W"][e].T, gs[e].cpu(), p["bias"][e].cpu())
    gate_up[p["unc"]] = NAN
    p.update(blocks=blocks, scales=scales, gs=gs, x=x, tpe=tpe, offs=offs, gy=b["args"][3], ref_bwd=b["ref"],
             gate_up=gate_up.to(DEV), ref_glu=ref_glu)
    p.update(lora_operands(p, table))
    return p


def lora_operands(p, table):
    """The adapter operands of one case (a generator of their own) on the device and the float64 references ``ref_lora`` /
    ``ref_lora_b`` [T, N] and ``ref_lora_bwd`` [T, K]: acc * g_e + the adapter term (+ bias), zero outside every clipped
    range, with the exactness condition of the module docstring asserted."""
    T, E, K, N, r = p["T"], p["E"], p["K"], p["N"], LORA_RANK[p["K"]]
    ga = torch.Generator().manual_seed(7919 * T + K + N + 500009 + len(table))
    v, dv = torch.randint(-4, 5, (T, r), generator=ga).float(), torch.randint(-4, 5, (T, r), generator=ga).float()
    B, A = torch.randint(-2, 3, (E, N, r), generator=ga).float(), torch.randint(-2, 3, (E, r, K), generator=ga).float()
    x, gy, gs, bias = p["x"].cpu().double(), p["gy"].cpu().double(), p["gs"].cpu().double(), p["bias"].cpu().double()
    assert all(float(a) != float(b) for a, b in zip(gs[:-1], gs[1:]))                # neighbours differ
    assert torch.equal(torch.log2(gs), torch.log2(gs).round())                       # powers of two
    ref, ref_b, ref_bwd = (torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64),
                           torch.zeros(T, K, dtype=torch.float64))
    moved = moved_bwd = False
    for e, (lo, hi) in enumerate(p["ranges"]):
        if hi <= lo:
            continue
        W, g, limit = p["W"][e], float(gs[e]), 2.0 ** 24 * min(float(gs[e]) * 2.0 ** -5, 1.0)
        add, add_bwd = v[lo:hi].double() @ B[e].double().T, dv[lo:hi].double() @ A[e].double()
        ref[lo:hi] = (x[lo:hi] @ W.T) * g + add
        ref_b[lo:hi] = ref[lo:hi] + bias[e]
        ref_bwd[lo:hi] = (gy[lo:hi] @ W) * g + add_bwd
        mass = (x[lo:hi].abs() @ W.abs().T) * g + v[lo:hi].double().abs() @ B[e].double().abs().T + bias[e].abs()
        mass_bwd = (gy[lo:hi].abs() @ W.abs()) * g + dv[lo:hi].double().abs() @ A[e].double().abs()
        assert float(mass.max()) < limit and float(mass_bwd.max()) < limit
        moved, moved_bwd = moved or bool(add.count_nonzero()), moved_bwd or bool(add_bwd.count_nonzero())
    assert bool(torch.isfinite(ref_b).all()) and bool(torch.isfinite(ref_bwd).all())
    assert bool(p["unc"].all()) or (moved and moved_bwd)                             # (the adapter matters)
    v[p["unc"]] = NAN
    dv[p["unc"]] = NAN
    return dict(r=r, v=v.to(DEV), dv=dv.to(DEV), B=B.to(DEV), A=A.to(DEV), ref_lora=ref, ref_lora_b=ref_b, ref_lora_bwd=ref_bwd)


def assert_is_reference(p, got, ref, what):
    assert table_intact(p), what
    assert got.shape == ref.shape and same_bits(got.cpu(), ref.float().to(got.dtype)), what   # (bfloat16: one rounding)
    assert uncovered_all_zero_bits(p, got), what
    if p["table"] == "all-empty":
        assert int(torch.count_nonzero(bits(got.cpu()))) == 0, what


def plain(p, rows, bias=True, out_dtype=torch.float32, experts=slice(None), table=None):
    tpe, offs = table or (p["tpe"], p["offs"])
    return ops().moe_forward_nvfp4(p["blocks"][experts], p["scales"][experts], p["gs"][experts], rows, tpe, offs,
                                   bias=p["bias"][experts] if bias else None, out_dtype=out_dtype)


def gated(p, rows, out_dtype=torch.float32, experts=slice(None), table=None):
    tpe, offs = table or (p["tpe"], p["offs"])
    return ops().moe_gated_forward_nvfp4(p["blocks"][experts], p["scales"][experts], p["gs"][experts], rows, tpe, offs,
                                         bias=p["bias"][experts], out_dtype=out_dtype, **act_kw(KIND))


def backward(p, rows, out_dtype=torch.float32, experts=slice(None), table=None):
    tpe, offs = table or (p["tpe"], p["offs"])
    return ops().moe_backward_input_nvfp4(p["blocks"][experts], p["scales"][experts], p["gs"][experts], rows, tpe, offs,
                                          out_dtype=out_dtype)


def check_forward_exact(p):
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            got = plain(p, p["x"].to(din), out_dtype=dout)
            assert got.dtype == dout
            assert_is_reference(p, got, p["ref_b"], (p["table"], din, dout))


def check_grouped_is_one_expert_calls(p, op, rows, what):
    """The grouped call has the bits of one call per expert on that expert's clipped slice, scattered into zeros."""
    got = op(p, rows)
    assert table_intact(p), what
    want = torch.zeros_like(got)
    for e, (lo, hi) in enumerate(p["ranges"]):
        if hi > lo:
            want[lo:hi] = op(p, rows[lo:hi].contiguous(), experts=slice(e, e + 1), table=whole_table(hi - lo))
    assert bool(torch.isfinite(want).all()), what                                    # (the slices hold no uncovered row)
    assert same_bits(got, want), (p["table"], what, (bits(got) != bits(want)).nonzero()[:4].tolist())
    assert uncovered_all_zero_bits(p, got), what
    if bool((~p["unc"]).any()):
        assert float(got.abs().max()) > 0


# ---- 1. the plain forward against float64, exactly

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_forward_is_the_float64_reference(table, K, N, form, force):
    """ops.moe_forward_nvfp4 with the global scales and the bias, float32 and bfloat16 rows, a float32 and a bfloat16
    result, under the tile and under the decode kernel."""
    force(form)
    p = problem(table, K, N)
    assert lib().fql_tune_nvfp4_kernel(p["E"], p["T"], K, N) == FORMS.index(form)
    check_forward_exact(p)


# ---- 2. the gated forward against the bfloat16-rounded float64 h

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_gated_forward_against_the_rounded_reference_h(table, K, N, form, force):
    force(form)
    p = problem(table, K, N)
    for din in (torch.float32, torch.bfloat16):
        ref = p["ref_glu"][din]
        got = gated(p, p["gate_up"].to(din))
        assert table_intact(p) and got.dtype == torch.float32 and got.shape == (p["T"], N)
        err = rel_fro_dev(got, ref)
        print(f"nvfp4 tables gated {form} {table} K={K} N={N} in={din}: rel_fro {err:.3e} (bound {GATED_BOUND:.1e})")
        assert err <= GATED_BOUND
        assert uncovered_all_zero_bits(p, got)
        if table == "all-empty":
            assert int(torch.count_nonzero(bits(got.cpu()))) == 0


# ---- 3. the backward against float64, exactly

@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_backward_is_the_float64_reference(table, K, N):
    """ops.moe_backward_input_nvfp4 (one kernel form): grad_in [T, K] from float32 and bfloat16 gradient rows."""
    p = problem(table, K, N)
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            got = backward(p, p["gy"].to(din), out_dtype=dout)
            assert got.dtype == dout
            assert_is_reference(p, got, p["ref_bwd"], (table, "bwd", din, dout))


# ---- 4. the grouped call is the one-expert calls, bit for bit

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_grouped_forward_equals_one_expert_calls(table, K, N, form, force):
    """The plain forward on the integer rows and the gated forward on the Gaussian gate | up rows, the grouped call and the
    one-expert calls under the same kernel form."""
    force(form)
    p = problem(table, K, N)
    check_grouped_is_one_expert_calls(p, plain, p["x"], "plain")
    check_grouped_is_one_expert_calls(p, gated, p["gate_up"], "gated")


@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_grouped_backward_equals_one_expert_calls(table, K, N):
    p = problem(table, K, N)
    check_grouped_is_one_expert_calls(p, backward, p["gy"], "bwd")


# ---- 5. the fused adapter entries: v[t] and B[e] / A[e] beside the base kernels' own indexing

@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_lora_forward_and_backward_are_the_float64_reference(table, K, N):
    """ops.moe_forward_nvfp4_lora (with and without bias) and ops.moe_backward_input_nvfp4_lora on the exact operands, from
    float32 and bfloat16 rows, a float32 and a bfloat16 result: the float32 result is the float64 reference bit for bit, a
    bfloat16 result one rounding of it, uncovered rows are zero bits although their x, dY, v and dv are NaN, and the table
    tensors are unchanged.  The global scale differs between neighbouring experts and scales the weight term only."""
    p = problem(table, K, N)
    w, t = (p["blocks"], p["scales"], p["gs"]), (p["tpe"], p["offs"])
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            for bias in (False, True):
                got = ops().moe_forward_nvfp4_lora(*w, p["x"].to(din), p["v"], p["B"], *t, bias=p["bias"] if bias else None,
                                                   out_dtype=dout)
                assert got.dtype == dout
                assert_is_reference(p, got, p["ref_lora_b"] if bias else p["ref_lora"], (table, "lora fwd", din, bias, dout))
            got = ops().moe_backward_input_nvfp4_lora(*w, p["gy"].to(din), p["dv"], p["A"], *t, out_dtype=dout)
            assert got.dtype == dout
            assert_is_reference(p, got, p["ref_lora_bwd"], (table, "lora bwd", din, dout))


@pytest.mark.parametrize("table,K,N", CASES, ids=CASE_IDS)
def test_lora_grouped_equals_one_expert_calls(table, K, N):
    """The three adapter entries (the gated one on the Gaussian gate | up rows, swiglu_clamp): the grouped call has the bits
    of one call per expert on that expert's clipped slice of the rows and of v / dv with that expert's B / A and global
    scale, scattered into zeros."""
    p = problem(table, K, N)
    o = ops()
    entries = [("fwd", "x", "v", "B", lambda w, r, v, m, t, bias: o.moe_forward_nvfp4_lora(*w, r, v, m, *t, bias=bias,
                                                                                        out_dtype=torch.float32)),
               ("gated", "gate_up", "v", "B", lambda w, r, v, m, t, bias: o.moe_gated_forward_nvfp4_lora(
                   *w, r, v, m, *t, bias=bias, out_dtype=torch.float32, **act_kw(KIND))),
               ("bwd", "gy", "dv", "A", lambda w, r, v, m, t, bias: o.moe_backward_input_nvfp4_lora(*w, r, v, m, *t))]
    for name, rows, vk, mk, op in entries:
        got = op((p["blocks"], p["scales"], p["gs"]), p[rows], p[vk], p[mk], (p["tpe"], p["offs"]), p["bias"])
        assert table_intact(p), name
        assert got.dtype == torch.float32 and got.shape == (p["T"], K if name == "bwd" else N)
        want = torch.zeros_like(got)
        for e, (lo, hi) in enumerate(p["ranges"]):
            if hi > lo:
                want[lo:hi] = op((p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gs"][e:e + 1]), p[rows][lo:hi].contiguous(),
                                 p[vk][lo:hi].contiguous(), p[mk][e:e + 1], whole_table(hi - lo), p["bias"][e:e + 1])
        assert bool(torch.isfinite(want).all()), name                                # (the slices hold no uncovered row)
        assert same_bits(got, want), (table, name, (bits(got) != bits(want)).nonzero()[:4].tolist())
        assert uncovered_all_zero_bits(p, got), name
        if bool((~p["unc"]).any()):
            assert float(got.abs().max()) > 0


# ---- 6. a decode step of a 128-expert model under the library's own threshold

def test_e128_decode_step_under_the_default_dispatch():
    """T = 8 rows over 128 experts with no threshold forced: the library reports the decode kernel, and the checks hold
    through the dispatcher as a caller gets it."""
    p = problem("e128-decode", 96, 40)
    assert lib().fql_tune_set_nvfp4_decode_max_rows(-1) >= p["T"]                    # (the threshold a clean process has)
    assert lib().fql_tune_nvfp4_kernel(p["E"], p["T"], p["K"], p["N"]) == 1
    check_forward_exact(p)
    check_grouped_is_one_expert_calls(p, plain, p["x"], "plain")
    check_grouped_is_one_expert_calls(p, gated, p["gate_up"], "gated")
