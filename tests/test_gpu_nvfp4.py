"""NVFP4 weights on the GPU: ops.moe_forward_nvfp4 / moe_gated_forward_nvfp4 / linear_forward_nvfp4 /
linear_gated_forward_nvfp4 (csrc/fql_gemm_nvfp4.h), the layers NVFP4MoEFFN and NVFP4Linear and
QuantizedSparseMoEBlock(experts=NVFP4MoEFFN).

K in {32, 96, 288} are those of tests/test_gpu_mxfp4.py, for the reasons given there (one 16-byte piece, i.e. two scale
blocks; a last stage of 32 k behind a full one; several stages and a tail); N in {8, 40, 136}, a table of [0, 1, 33, 70]
rows plus 2 uncovered, and E = 1 with one row.  Both kernels (the 64 x 128 tile and the one-wave decode kernel) are forced
in turn through fql_tune_set_nvfp4_decode_max_rows.  K in {64, 128, 608, 1248} are there for what those three leave out:

  * the tile kernel (a stage is 64 k): K = 64 is one whole stage (s1 is never read and nothing is stored behind the one
    contraction), K = 128 exactly two stages; the three K above are odd multiples of 32 and always end in a half stage.
  * the decode kernel's load ring (nv4_decode_body; a slot is one pair = 64 k; 8 slots for bfloat16 rows, 4 for float32
    rows, FQL_MX4_DECODE_DEPTH = 8): a trip of ``for (; j + DEPTH <= pairs; ...)`` consumes DEPTH slots and refills each with
    pair j + i + DEPTH, clamped to the last pair; the drain loop consumes what is left; K % 64 == 32 adds the odd piece
    (``odd``).  "consumed refills" are refilled slots that a later trip or the drain loop consumes, with their ``sc``:

        K     pairs  odd |  bfloat16 rows: trips, drained, consumed refills |  float32 rows: trips, drained, consumed refills
        32      0    yes |        0        0        0                        |        0        0        0
        64      1    no  |        0        1        0                        |        0        1        0
        96      1    yes |        0        1        0                        |        0        1        0
        128     2    no  |        0        2        0                        |        0        2        0
        288     4    yes |        0        4        0                        |        1        0        0  (refills clamped, unused)
        608     9    yes |        1        1        1                        |        2        1        5
        1248   19    yes |        2        3       11                        |        4        3       15

    The gated entry always feeds the kernels bfloat16 h rows from its workspace: F = 608 is its one trip and its consumed
    refill.  Rows whose base is not 16-byte aligned take nv4_decode_body<IN, OUT, false, 1, 1> (a ring of one slot: ``pairs``
    trips, nothing drained) and the element loads of nv4_kernel (vec_x == false): test_rows_one_element_off_a_16_byte_boundary
    and half of the footprint cases.

The reference is float64 on the CPU: the product of the bfloat16-rounded rows and ``dequantize_nvfp4`` WITHOUT the global
scale, rounded to float32, then the two float32 epilogue steps (* global_scale[e], + bias[e]).

MEASURED (MI355X; printed by the tests with -s) and the bounds derived from them:
  * float32 result on Gaussian rows, scale bytes over the whole finite range, relative Frobenius error against that
    reference: SAME_INPUT_MEASURED below; the bound is 4 x that (the matrix core's adder is not an fmaf chain) and must
    stay below 2^-9.
  * a bfloat16 result adds its one rounding, 2^-9 (measured 1.5e-3 .. 1.8e-3).  That comparison draws the scale bytes from 0x30 .. 0x47: with the whole
    range one weight row carries the norm, and 2^-9 is an r.m.s. bound over many elements, not a bound on one.
  * the gated entry against the float64 product of the bfloat16-rounded float64 h: GATED_MEASURED, x 4, below 2^-9, for
    F <= 288 (F = 128 measured 5.4e-8 .. 8.7e-6, inside it).  F = 608 has GATED_DEEP_MEASURED of its own, x 4, below 2^-9:
    everything but gelu_tanh on bfloat16 rows measures 1.1e-7 .. 1.6e-6 there; gelu_tanh on bfloat16 rows 6.9e-5.  The
    cause is the reference, not the sum: where the gate is above about 3.5 the float32 sigmoid is exactly 1, h is the
    exact 16-bit product of two bfloat16 values, one in 256 of those is a tie of the rounding to bfloat16 and goes to
    even, while the float64 h lies just below the tie and goes down; each such element moves its row by 2^-8 of the
    element, and a longer row has more of them (and larger ones: they sit where the gate is large).
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import (NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, hostile_table, misaligned, ops,
                     rel_fro_dev, same_bits, uncovered_mask)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
COUNTS, TAIL = [0, 1, 33, 70], 2
KS, NS = [32, 64, 96, 128, 288, 608, 1248], [8, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
FORMS = ["tile", "decode"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes; 0xFF is a NaN as bfloat16
INT_MAX = 2 ** 31 - 1
NARROW = (0x30, 0x47)             # the e4m3 values 0.5 .. 3.75, all three mantissa bits in use

# relative Frobenius error of the float32 result against the reference above: the largest value the tests below printed on
# an MI355X, and the bound the tests assert (4 x, below 2^-9 as the contract demands)
SAME_INPUT_MEASURED = 9.8e-8       # (K = 288, N = 136; 0 .. 9.8e-8 over the nine shapes of K <= 288 it was taken on, the same
#                                    from both kernels; measured over all 21 shapes since: K = 64 3.7e-8 .. 5.1e-8, K = 128
#                                    6.1e-8 .. 6.7e-8, K = 608 1.34e-7 .. 1.45e-7, K = 1248 1.81e-7 .. 1.95e-7 (N = 40): all
#                                    under the bound, which therefore stays)
SAME_INPUT_BOUND = 4 * SAME_INPUT_MEASURED
# the gated op: the device's float32 h lands on the other side of a bfloat16 rounding boundary for a few elements
GATED_MEASURED = 1.7e-5            # (gelu_tanh, F = 96, bfloat16 rows; 1.9e-8 .. 1.7e-5 over the cases; the block: 6.5e-8)
GATED_BOUND = 4 * GATED_MEASURED
GATED_DEEP_MEASURED = 6.907e-5     # (F > 288; gelu_tanh, F = 608, bfloat16 rows, both kernels; the other F = 608 cases: 1.1e-7 .. 1.6e-6)
GATED_DEEP_BOUND = 4 * GATED_DEEP_MEASURED
BF16_OUT = 2.0 ** -9               # one rounding of the result to bfloat16: half an ulp
assert SAME_INPUT_BOUND < 2.0 ** -9 and GATED_BOUND < 2.0 ** -9 and GATED_DEEP_BOUND < 2.0 ** -9


def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def force():
    """``force(form)`` pins the tile or the decode kernel for every T; the library's threshold is put back afterwards."""
    old = lib().fql_tune_set_nvfp4_decode_max_rows(-1)

    def use(form):
        lib().fql_tune_set_nvfp4_decode_max_rows(INT_MAX if form == "decode" else 0)
        assert lib().fql_tune_nvfp4_kernel(4, 5, 96, 40) == (1 if form == "decode" else 0)
    yield use
    lib().fql_tune_set_nvfp4_decode_max_rows(old)


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


def finite_scale_bytes(shape, g):
    """Random e4m3 bytes over the whole finite range, both signs: everything but 0x7F and 0xFF."""
    b = torch.randint(0, 0x7F, shape, generator=g, dtype=torch.uint8)
    return b | (torch.randint(0, 2, shape, generator=g, dtype=torch.uint8) << 7)


def global_scales(E):
    """A different power of two per expert, in 2^-3 .. 2^2 (cycling past six experts)."""
    return torch.tensor([2.0 ** ((5 * e + 1) % 6 - 3) for e in range(E)], dtype=torch.float32)


def epilogue(acc64, gs, bias=None):
    """The two float32 steps of the contract on a float64 sum: fl32(fl32(acc * gs) + bias), returned as float64."""
    v = acc64.float() * gs
    if bias is not None:
        v = v + bias
    return v.double()


def reference(x, W, gs, bias, ranges, T):
    """(ref, ref_b, acc) float64 [T, N]: zero on the rows no expert covers."""
    N = W.shape[1]
    xr = x.bfloat16().double()
    ref, ref_b, acc = (torch.zeros(T, N, dtype=torch.float64) for _ in range(3))
    for e, (lo, hi) in enumerate(ranges):
        if hi > lo:
            acc[lo:hi] = xr[lo:hi] @ W[e].T
            ref[lo:hi] = epilogue(acc[lo:hi], gs[e])
            ref_b[lo:hi] = epilogue(acc[lo:hi], gs[e], bias[e])
    return ref, ref_b, acc


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, scale_range=None, integer=False, seed=0):
    """Random element codes; scale bytes over the whole finite range or (``scale_range``) in [lo, hi]; rows randn, or
    (``integer``) integers in [-4, 4] with an integer bias.  Computed once per shape and shared; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    g = torch.Generator().manual_seed(1000 * K + N + seed)
    E = len(counts)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    if scale_range is None:
        scales = finite_scale_bytes((E, N, K // 16), g)
    else:
        scales = torch.randint(scale_range[0], scale_range[1] + 1, (E, N, K // 16), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    W = dequantize_nvfp4(blocks, scales).double()
    gs = global_scales(E)
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    x = torch.randint(-4, 5, (T, K), generator=g).float() if integer else torch.randn(T, K, generator=g)
    bias = torch.randint(-8, 9, (E, N), generator=g).float() if integer else torch.randn(E, N, generator=g)
    ranges = [(o, o + c) for c, o in zip(tpe.tolist(), offs.tolist())]
    ref, ref_b, acc = reference(x, W, gs, bias, ranges, T)
    return dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), gs=gs.to(DEV), x=x.to(DEV), bias=bias.to(DEV),
                tpe=tpe.to(DEV), offs=offs.to(DEV), ref=ref, ref_b=ref_b, acc=acc, W=W, counts=list(counts))


def run(p, x=None, bias=False, out_dtype=None, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], gs=p["gs"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_nvfp4(a["blocks"], a["scales"], a["gs"], p["x"] if x is None else x, a["tpe"], a["offs"],
                                   bias=p["bias"] if bias is True else (None if bias is False else bias), out_dtype=out_dtype)


# ---- the lane map, exactly

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_exact_on_integer_data(K, N, din, form, force):
    """Integer rows in [-4, 4], random codes, scale bytes 0x30 .. 0x47 (0.5 .. 3.75), a power-of-two global scale per
    expert, an integer bias: every product is a multiple of 2^-5 and every sum stays below 2^16 (asserted; the worst case
    at K = 1248 is 4 x 22.5 x 1248 < 2^17, 22 bits), so float32 is exact in any order and so are the two epilogue steps.
    A scale on the wrong half of a 16-byte piece, a swapped block or a neighbouring expert's global scale fails."""
    force(form)
    p = problem(K, N, scale_range=NARROW, integer=True)
    assert float(p["acc"].abs().max()) < 2 ** 16
    for bias in (False, True):
        ref = p["ref_b"] if bias else p["ref"]
        got = run(p, p["x"].to(din), bias=bias, out_dtype=torch.float32)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                         # uncovered rows: exactly zero
        got16 = run(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16)          # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())
    none = run(p, p["x"].to(din), out_dtype=torch.float32, gs=None)                  # no global scale, no bias: acc itself
    assert torch.equal(none.cpu().double(), p["acc"])


@pytest.mark.parametrize("form", FORMS)
def test_exact_one_expert_one_row(form, force):
    force(form)
    p = problem(96, 40, counts=(1,), tail=0, scale_range=NARROW, integer=True)
    assert torch.equal(run(p, out_dtype=torch.float32).cpu().double(), p["ref"])
    assert torch.equal(run(p, out_dtype=torch.float32, tpe=None, offs=None).cpu().double(), p["ref"])   # no table: one segment
    dense = ops().linear_forward_nvfp4(p["blocks"][0], p["scales"][0], p["gs"], p["x"], bias=p["bias"][0])
    assert torch.equal(dense.cpu().double(), p["ref_b"])


# ---- decode and tile: the same bits

def gate_up_rows(T, F, seed):
    return (torch.randn(T, 2 * F, generator=torch.Generator().manual_seed(seed)) * 2.0).to(DEV)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_decode_and_tile_give_the_same_bits(K, N, force):
    """Gaussian rows, scale bytes over the whole finite range: every element of the decode kernel's result is the tile
    kernel's, plain and gated, float32 and bfloat16 rows and results."""
    p = problem(K, N)
    gu = gate_up_rows(p["T"], K, K + N)
    got = {}
    for form in FORMS:
        force(form)
        res = []
        for din in (torch.float32, torch.bfloat16):
            for dout in (torch.float32, torch.bfloat16):
                res.append(run(p, p["x"].to(din), bias=True, out_dtype=dout))
                res.append(ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], gu.to(din), p["tpe"], p["offs"],
                                                         bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp")))
        res.append(run(p, gs=None))
        got[form] = res
    for i, (a, b) in enumerate(zip(got["tile"], got["decode"])):
        assert same_bits(a, b), (K, N, i)


# ---- random inputs

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_inputs_against_the_same_rounded_inputs(K, N, form, force):
    force(form)
    p, q = problem(K, N), problem(K, N, scale_range=NARROW, seed=3)
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            x = p["x"] if din == torch.float32 else p["x"].bfloat16()
            e32 = rel_fro_dev(run(p, x, bias=bias, out_dtype=torch.float32), p["ref_b"] if bias else p["ref"])
            x = q["x"] if din == torch.float32 else q["x"].bfloat16()
            e16 = rel_fro_dev(run(q, x, bias=bias, out_dtype=torch.bfloat16), q["ref_b"] if bias else q["ref"])
            print(f"nvfp4 {form} K={K} N={N} in={din} bias={bias}: rel_fro f32 out {e32:.3e} (bound {SAME_INPUT_BOUND:.1e}), "
                  f"bf16 out {e16:.3e} (bound {SAME_INPUT_BOUND + BF16_OUT:.3e})")
            assert e32 <= SAME_INPUT_BOUND
            assert e16 <= SAME_INPUT_BOUND + BF16_OUT


def test_float16_is_refused_and_out_dtype_follows_the_input():
    p = problem(32, 8)
    with pytest.raises(RuntimeError, match="float16"):
        run(p, p["x"].half())
    assert run(p).dtype == torch.float32 and run(p, p["x"].bfloat16()).dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="forward-only"):
        run(p, p["x"].clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="global_scale"):
        run(p, gs=p["gs"][:2])
    with pytest.raises(RuntimeError, match="K/16"):
        run(p, scales=p["scales"][:, :, :1])


# ---- independence, bit for bit

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_grouped_equals_one_expert_calls_permutation_and_rerun(K, N, form, force):
    force(form)
    p = problem(K, N)
    got = run(p, bias=True)
    assert same_bits(got, run(p, bias=True))                                         # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_forward_nvfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gs"][e:e + 1], p["x"][o:o + c].contiguous(),
                                      torch.tensor([c], dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int32, device=DEV), bias=p["bias"][e:e + 1])
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    again = ops().moe_forward_nvfp4(p["blocks"][perm], p["scales"][perm], p["gs"][perm], p["x"], p["tpe"][perm], p["offs"][perm],
                                    bias=p["bias"][perm])
    assert same_bits(again, got)


# ---- non-finite values and the sign of a scale

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("byte", [0x7F, 0xFF])
def test_nan_scale_byte_is_nan_in_exactly_that_weight_row(byte, form, force):
    """The byte sits in the SECOND 16-block of a 16-byte piece (block 3 = k 48 .. 63 of K = 96)."""
    force(form)
    p = problem(96, 40)
    scales = p["scales"].clone()
    e, n = 2, 17
    scales[e, n, 3] = byte
    got = run(p, scales=scales)
    want = run(p)
    o, c = p["offs"].tolist()[e], p["counts"][e]
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[o:o + c, n] = True
    assert torch.equal(nan, expect)
    assert torch.equal(got[~expect], want[~expect])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_non_finite_activation_is_nan_across_exactly_its_row(din, form, force):
    force(form)
    p = problem(288, 136)
    want = run(p, p["x"].to(din))
    for value in (float("inf"), float("nan")):
        x = p["x"].to(din).clone()
        t = p["offs"].tolist()[3] + 40                                               # a row of the second 32-row wave
        x[t, 201] = value
        got = run(p, x)
        nan = torch.isnan(got)
        expect = torch.zeros_like(nan)
        expect[t] = True
        assert torch.equal(nan, expect)
        assert same_bits(got[~expect], want[~expect])


@pytest.mark.parametrize("form", FORMS)
def test_negative_scale_byte_negates_its_contribution(form, force):
    """Integer data: the sign bit set in scale block 3 of every weight row of expert 3 turns
    out = gs * (rest + part) + bias into gs * (rest - part) + bias, exactly."""
    force(form)
    p = problem(96, 40, scale_range=NARROW, integer=True)
    e, j = 3, 3
    scales = p["scales"].clone()
    scales[e, :, j] |= 0x80
    o, c = p["offs"].tolist()[e], p["counts"][e]
    part = p["x"].cpu().double()[o:o + c, 16 * j:16 * j + 16] @ p["W"][e][:, 16 * j:16 * j + 16].T
    want = p["ref_b"].clone()
    want[o:o + c] = epilogue(p["acc"][o:o + c] - 2 * part, p["gs"][e].cpu(), p["bias"][e].cpu())
    got = run(p, bias=True, scales=scales)
    assert torch.equal(got.cpu().double(), want)
    assert not torch.equal(want, p["ref_b"])


# ---- the gated op

@functools.lru_cache(maxsize=None)
def gated_problem(F, kind, N=40):
    p = dict(problem(F, N, scale_range=NARROW, seed=7))
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = torch.randn(p["T"], 2 * F, generator=g) * 2.0
    refs = {}
    for din in (torch.float32, torch.bfloat16):
        h = hidden64(kind, gate_up.to(din), ALPHA, LIMIT).bfloat16().double()        # the bf16-rounded reference h
        ref = torch.zeros(p["T"], N, dtype=torch.float64)
        for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
            ref[o:o + c] = epilogue(h[o:o + c] @ p["W"][e].T, p["gs"][e].cpu(), p["bias"][e].cpu())
        refs[din] = ref
    p.update(gate_up=gate_up.to(DEV), refs=refs)
    return p


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96, 128, 608])
def test_gated_op_against_the_rounded_reference_h(F, kind, form, force):
    force(form)
    p = gated_problem(F, kind)
    bound = GATED_BOUND if F <= 288 else GATED_DEEP_BOUND
    for din in (torch.float32, torch.bfloat16):
        gu = p["gate_up"].to(din)
        call = lambda: ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], gu, p["tpe"], p["offs"], bias=p["bias"],
                                                     out_dtype=torch.float32, **act_kw(kind))
        got = call()
        err = rel_fro_dev(got, p["refs"][din])
        print(f"nvfp4 gated {form} F={F} {kind} in={din}: rel_fro {err:.3e} (bound {bound:.1e})")
        assert err <= bound
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
        assert same_bits(got, call())
    # the dense entry on expert 3's matrix and rows: the grouped launchers with E = 1
    dense32 = ops().linear_gated_forward_nvfp4(p["blocks"][3], p["scales"][3], p["gs"][3:4], p["gate_up"][-72:-2].contiguous(),
                                               bias=p["bias"][3], out_dtype=torch.float32, **act_kw(kind))
    want32 = ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], p["gate_up"], p["tpe"], p["offs"], bias=p["bias"],
                                           out_dtype=torch.float32, **act_kw(kind))[-72:-2]
    assert same_bits(dense32, want32.contiguous())


# ---- rows whose base is not 16-byte aligned

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "glu"])
@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(96, 40), (608, 37)])
def test_rows_one_element_off_a_16_byte_boundary(K, N, din, gated, form, force):
    """helpers.misaligned puts the rows one element past a 16-byte boundary: nv4_kernel then loads them element by element
    (vec_x == false) and the decode kernel runs nv4_decode_body<IN, OUT, false, 1, 1>, a ring of one slot; the gated entry
    hands such rows to its pre-pass.  The result is the result on an aligned copy bit for bit, and with the integer recipe
    the plain one is the float64 reference: an element load that takes a neighbour (k ^ 1, say) fails both."""
    force(form)
    p = problem(K, N, scale_range=NARROW, integer=True)
    T = p["T"]
    if gated:
        rows = gate_up_rows(T, K, K + N + 1).to(din)
        call = lambda r, dout: ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], r, p["tpe"], p["offs"],
                                                             bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp"))
    else:
        rows = p["x"].to(din)
        call = lambda r, dout: run(p, r, bias=True, out_dtype=dout)
    off = misaligned(rows, 1)
    assert rows.data_ptr() % 16 == 0 and off.data_ptr() % 16 == rows.element_size() and same_bits(off, rows)
    for dout in (torch.float32, torch.bfloat16):
        got, want = call(off, dout), call(rows, dout)
        assert same_bits(got, want), (K, N, din, dout, (got != want).nonzero()[:4].tolist())
        assert torch.count_nonzero(got[T - TAIL:]) == 0
        if not gated:
            ref = p["ref_b"] if dout == torch.float32 else p["ref_b"].float().bfloat16()
            assert torch.equal(got.cpu().double(), ref.double()), (K, N, din, dout)


# ---- footprint

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "glu"])
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(96, 40), (96, 201), (64, 40), (64, 201), (608, 40), (608, 201)],
                         ids=["40", "201", "K64-40", "K64-201", "K608-40", "K608-201"])      # (K = 96 keeps the ids it had)
def test_entries_stay_inside_their_buffers(K, N, dout, gated, form, force):
    """Every pointer is the interior of a guarded buffer; out sits 4 bytes off a 16-byte boundary inside SENT, and the
    scale bytes start at an odd address and end exactly at their last byte in front of 0xFF (a NaN scale): the two-byte
    scale load must not reach past [E][N][K / 16], neither in the ring's tail (K = 96, 608) nor in a ring slot clamped to
    the last pair (the refills at K = 608; every slot but the first at K = 64).  In half of the cases (bfloat16 out at
    N = 40, float32 out at N = 201) the rows start one element past a 16-byte boundary: the element-load paths.  Only [T, N] changes, the guards stay,
    uncovered rows are zero and the bits are the public op's.  The gated entry runs once per stale workspace content and
    must return those bits each time."""
    force(form)
    p = problem(K, N)
    E, T = p["E"], p["T"]
    rows = gate_up_rows(T, K, 3) if gated else p["x"]
    rows_offset = rows.element_size() if (dout == torch.bfloat16) == (N == 40) else 16
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    gs = guarded_like("global_scale", p["gs"], NAN)
    rw, bias = guarded_like("rows", rows, NAN, offset=rows_offset), guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    esz = 4 if dout == torch.float32 else 2
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert out.ptr % 16 == 4 and sc.ptr % 2 == 1 and rw.ptr % 16 == rows_offset % 16
    nbytes = lib().fql_moe_nvfp4_workspace_bytes(E, T, K, N, int(gated))
    st = torch.cuda.current_stream().cuda_stream
    if gated:
        assert nbytes == (T * K * 2 + 15) // 16 * 16
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        want = ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], rows, p["tpe"], p["offs"], bias=p["bias"],
                                             out_dtype=dout, **act_kw("swiglu_clamp"))
        bufs = (bl, sc, gs, rw, bias, cnt, off, out, ws)
        for fill in PREFILLS:                      # what an earlier launch may have left in the workspace: the same bits
            ws.bytes().fill_(fill)
            out.view(dout, T, N).fill_(SENT)
            rc = lib().fql_moe_nvfp4_glu_fwd(bl.ptr, sc.ptr, gs.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T,
                                             K, N, ACT["swiglu_clamp"], ALPHA, LIMIT, ws.ptr, nbytes, st)
            assert rc == 0
            assert_guards_intact(*bufs, what=f"nvfp4 fwd gated N={N} {dout} workspace {fill:#04x}")
            assert torch.count_nonzero(out.view(dout, T, N)[T - TAIL:]) == 0, hex(fill)
            assert same_bits(out.view(dout, T, N), want), hex(fill)
    else:
        assert nbytes == 0
        rc = lib().fql_moe_nvfp4_fwd(bl.ptr, sc.ptr, gs.ptr, rw.ptr, 0, bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                     None, 0, st)
        want = run(p, bias=True, out_dtype=dout)
        bufs = (bl, sc, gs, rw, bias, cnt, off, out)
    assert rc == 0
    assert_guards_intact(*bufs, what=f"nvfp4 fwd gated={gated} N={N} {dout} {form}")
    got = out.view(dout, T, N)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, want)
    assert not bool(torch.isnan(got.float()).any())                                  # (no guard byte served as a scale)


# ---- hostile expert tables

@functools.lru_cache(maxsize=None)
def table_problem(table, K=96, N=40):
    """The integer recipe on one of helpers.hostile_table's tables; the rows no expert covers are NaN in the input."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    tpe, offs, T, ranges = hostile_table(table)
    E = tpe.numel()
    g = torch.Generator().manual_seed(E + T)
    blocks = pack(torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8))
    scales = torch.randint(NARROW[0], NARROW[1] + 1, (E, N, K // 16), generator=g, dtype=torch.uint8)
    W = dequantize_nvfp4(blocks, scales).double()
    gs = global_scales(E)
    x = torch.randint(-4, 5, (T, K), generator=g).float()
    bias = torch.randint(-8, 9, (E, N), generator=g).float()
    unc = uncovered_mask(ranges, T)
    x[unc] = NAN
    _, ref_b, acc = reference(x, W, gs, bias, ranges, T)
    assert float(acc.abs().max()) < 2 ** 16
    return dict(T=T, unc=unc, ref_b=ref_b, args=(blocks.to(DEV), scales.to(DEV), gs.to(DEV), x.to(DEV), tpe.to(DEV), offs.to(DEV)),
                bias=bias.to(DEV), table=table, E=E, K=K, N=N, W=W, ranges=ranges, tpe_cpu=tpe, offs_cpu=offs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("table", ["e65", "e130-descending", "clipped", "all-empty"])
def test_hostile_tables_exactly(table, form, force):
    force(form)
    p = table_problem(table)
    for dout in (torch.float32, torch.bfloat16):
        got = ops().moe_forward_nvfp4(*p["args"], bias=p["bias"], out_dtype=dout)
        assert same_bits(got.cpu(), p["ref_b"].float().to(dout)), (table, dout)
        assert torch.count_nonzero(got.cpu()[p["unc"]]) == 0


# ---- layers and block

def ffn_weights(E, H, F, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    return dict(gate=mk(F, H), up=mk(F, H), down=mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H))


def test_linear_layer_on_3d_input_with_a_bias():
    lin = torch.nn.Linear(96, 40)
    m = fq().NVFP4Linear.from_linear(lin)
    x = torch.randn(3, 5, 96, generator=torch.Generator().manual_seed(2))
    from fused_int4_amd.quantize import dequantize_nvfp4
    ref = epilogue(x.reshape(15, 96).bfloat16().double() @ dequantize_nvfp4(m.blocks, m.scales).double().T, m.global_scale, m.bias)
    m = m.to(DEV)
    got = m(x.to(DEV))
    want = ops().linear_forward_nvfp4(m.blocks, m.scales, m.global_scale, x.to(DEV).reshape(15, 96), bias=m.bias)
    assert got.shape == (3, 5, 40) and same_bits(got.reshape(15, 40), want)
    err = rel_fro_dev(got.reshape(15, 40), ref)
    print(f"nvfp4 linear layer: rel_fro against the float64 definition {err:.3e} (bound {SAME_INPUT_BOUND:.1e})")
    assert err <= SAME_INPUT_BOUND
    grouped = ops().moe_forward_nvfp4(m.blocks[None], m.scales[None], m.global_scale, x.to(DEV).reshape(15, 96), None, None,
                                      bias=m.bias[None])
    assert same_bits(grouped, want)
    assert m(x.to(DEV).bfloat16()).dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.to(DEV).requires_grad_(True))


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_ffn_layer_is_the_two_ops_composed(dt):
    E, H, F = 4, 64, 96
    w = ffn_weights(E, H, F)
    m = fq().NVFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                      down_bias=w["down_bias"], activation_dtype=dt, **act_kw("swiglu_clamp")).to(DEV)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H, device=DEV).to(dt or torch.float32)
    got = m(x, tpe, offs)
    gate_up = ops().moe_forward_nvfp4(m.gate_up_blocks, m.gate_up_scales, m.gate_up_global, x, tpe, offs, bias=m.gate_up_bias.detach())
    want = ops().moe_gated_forward_nvfp4(m.down_blocks, m.down_scales, m.down_global, gate_up, tpe, offs,
                                         bias=m.down_bias.detach(), **act_kw("swiglu_clamp"))
    assert got.dtype == x.dtype and same_bits(got, want)
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True), tpe, offs)


def nvfp4_block(seed=9):
    E, H, F = 4, 64, 96
    w = ffn_weights(E, H, F, seed=seed)
    experts = fq().NVFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                            down_bias=w["down_bias"], **act_kw("swiglu_clamp"))
    return fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=experts, router_bias=True).to(DEV), experts


def block_reference(blk, experts, x, logits):
    """A torch block on the dequantised weights with bfloat16-rounded operands (x and h), the routing taken from the
    block's own router, the global scales applied as the kernels do (float32, before the bias)."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    weights, indices = ops().router_topk(logits, 2)
    Wgu = dequantize_nvfp4(experts.gate_up_blocks.cpu(), experts.gate_up_scales.cpu()).double()
    Wd = dequantize_nvfp4(experts.down_blocks.cpu(), experts.down_scales.cpu()).double()
    ggu, gd = experts.gate_up_global.cpu(), experts.down_global.cpu()
    xr = x.cpu().bfloat16().double()
    ref = torch.zeros(x.shape[0], x.shape[1], dtype=torch.float64)
    for t in range(x.shape[0]):
        for j in range(2):
            e = int(indices[t, j])
            gu = epilogue(Wgu[e] @ xr[t], ggu[e], experts.gate_up_bias[e].cpu()).float()     # the layer keeps gate_up in float32
            h = hidden64("swiglu_clamp", gu[None], ALPHA, LIMIT).bfloat16().double()[0]
            ref[t] += float(weights[t, j]) * epilogue(Wd[e] @ h, gd[e], experts.down_bias[e].cpu())
    return ref


def test_block_with_nvfp4_experts_against_torch():
    blk, experts = nvfp4_block()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(50, 64, generator=g).to(DEV)
    with torch.no_grad():
        blk.gate.bias.copy_(torch.randn(4, generator=g) * 0.1)
        out, logits = blk(x)
        err = rel_fro_dev(out, block_reference(blk, experts, x, logits))
    print(f"nvfp4 block: rel_fro {err:.3e} (bound {GATED_BOUND:.1e})")
    assert err <= GATED_BOUND
    with pytest.raises(RuntimeError, match="inference-only"):
        blk(x.clone().requires_grad_(True))


def test_block_graph_capture_and_replay_under_changed_routing():
    """One capture of the block at T = 5 (warmed up on a side stream), one replay after the tokens and the router bias
    changed in place: the replay is the eager result of the new state, bit for bit, and not the captured one's."""
    blk, _ = nvfp4_block(seed=13)
    g = torch.Generator().manual_seed(17)
    static_x = torch.randn(5, 64, generator=g).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        for _ in range(2):
            blk(static_x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=s):
        out, logits = blk(static_x)
    with torch.no_grad():
        first = blk(static_x.clone())[0].clone()
        static_x.copy_(torch.randn(5, 64, generator=g).to(DEV))
        blk.gate.bias.copy_(torch.tensor([3.0, -3.0, 0.5, 2.0], device=DEV))
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_logits = blk(static_x.clone())
    assert same_bits(out, eager) and same_bits(logits, eager_logits)
    assert not same_bits(eager, first)
