"""The decode kernels of the fp8-row and MXFP4-row precisions of the MXFP4 experts (csrc/fql_gemm_mx4_sdecode.h) on the GPU.
The six entries pick the kernel from T; here fql_tune_set_mx4_scaled_decode_max_rows forces either kernel per mode.

The contract is that the decode kernel returns THE SAME BITS as the tile kernel of its mode (mx4_scaled_kernel<1 | 2, OUT>),
so the main tests compare the two; the exactness tests stand without the tile kernel, so a mistake the two share cannot
hide.

The shapes are the smallest at which this kernel can go wrong: K in {32, 64, 96, 608} (half an instruction: only the lower
lane half has a block; one whole instruction; an odd tail behind a whole one; 19 blocks for a ring of 8 slots of 64 k: one
round of the loop that refills the ring, one slot of its remainder and the odd tail), N in {8, 37, 40, 136} (under one
32-row fragment; N % 4 != 0: element stores; a partial second wave; past 128), a table of [0, 1, 5, 32, 33] rows plus 2
uncovered (an empty expert, one row, a few rows, a full row block, a second row block) and E = 1 with one row and no
table through the C entries."""
import functools

import pytest
import torch

from glu_reference import act_kw
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_MAX = 2 ** 31 - 1
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
FP8, FP4 = 1, 2                    # the hooks' modes
MODES = [FP8, FP4]
MODE_IDS = ["fp8", "fp4"]
PRECISION = {FP8: "fp8", FP4: "fp4"}
COUNTS, TAIL = [0, 1, 5, 32, 33], 2
KS, NS = [32, 64, 96, 608], [8, 37, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes (tests/test_gpu_footprint.py); 0xFF is a NaN e4m3 byte and E8M0 code
# relative Frobenius error of the float32 result against the float64 product of the same quantised values: the bound
# tests/test_gpu_mxfp4_f8.py asserts for this arithmetic (SAME_INPUT_BOUND = 4 x the 7.5e-6 it measured), which
# tests/test_gpu_mxfp4_f4.py asserts as it stands for the MXFP4 rows (the same instruction in the same order); the bits
# are the tile kernels', so are the bounds
SAME_INPUT_BOUND = {FP8: 3.0e-5, FP4: 3.0e-5}


def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def force():
    """force(mode, "decode" | "tile" | "default"); the library's own thresholds come back afterwards."""
    setter = lib().fql_tune_set_mx4_scaled_decode_max_rows
    default = {m: setter(m, -1) for m in MODES}                     # (a negative value changes nothing)

    def use(mode, which):
        setter(mode, {"decode": INT_MAX, "tile": 0, "default": default[mode]}[which])
    try:
        yield use
    finally:
        for m in MODES:
            setter(m, default[m])


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


E2M1_OF_INT = {0: 0, 1: 2, 2: 4, 3: 5, 4: 6, 6: 7}                  # e2m1 code of |v| for the integers of the grid


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, lo=97, hi=157, integer=False, seed=0):
    """Random weight codes and per-(row, block) scale codes in [lo, hi]; rows randn, or (``integer``) two sets of exact
    rows: ``x8`` integers in [-4, 4] as e4m3 bytes and ``xb`` / ``xs`` e2m1 integers {0, +-1, +-2, +-3, +-4, +-6} with scale
    code 127, with their float64 references ``ref8`` / ``ref4`` (``_b``: with the integer bias), zero on the rows no expert
    covers.  Computed once per shape and shared; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(7919 * K + N + seed)
    E = len(counts)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    p = dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), tpe=tpe.to(DEV), offs=offs.to(DEV),
             counts=list(counts), offs_l=offs.tolist())
    if not integer:
        x = torch.randn(T, K, generator=g)
        bias = torch.randn(E, N, generator=g)
        p.update(x=x.to(DEV), bias=bias.to(DEV), W=dequantize_mxfp4(blocks, scales).double(), bias_cpu=bias)
        return p
    W = dequantize_mxfp4(blocks, scales).double()
    bias = torch.randint(-8, 9, (E, N), generator=g).float()
    xi = torch.randint(-4, 5, (T, K), generator=g).float()
    x8 = xi.to(torch.float8_e4m3fn)
    assert torch.equal(x8.float(), xi)                              # small integers are e4m3 values
    mag = torch.tensor([0, 1, 2, 3, 4, 6])[torch.randint(0, 6, (T, K), generator=g)]
    neg = torch.randint(0, 2, (T, K), generator=g)
    xc = (torch.tensor([E2M1_OF_INT.get(i, 0) for i in range(7)])[mag] + 8 * neg).to(torch.uint8)
    xb, xs = pack(xc), torch.full((T, K // 32), 127, dtype=torch.uint8)
    xg = dequantize_mxfp4(xb, xs)
    assert torch.equal(xg.abs(), mag.float()) and torch.equal(xg < 0, (neg == 1) & (mag > 0))

    def ref(rows, with_bias):
        out = torch.zeros(T, N, dtype=torch.float64)
        for e, (c, o) in enumerate(zip(tpe.tolist(), offs.tolist())):
            out[o:o + c] = rows[o:o + c].double() @ W[e].T + (bias[e].double() if with_bias else 0.0)
        return out
    p.update(bias=bias.to(DEV), x8=x8.view(torch.uint8).to(DEV), xb=xb.to(DEV), xs=xs.to(DEV), ref8=ref(xi, False),
             ref8_b=ref(xi, True), ref4=ref(xg, False), ref4_b=ref(xg, True))
    return p


def ref64(p, rows64, bias):
    out = torch.zeros(p["T"], p["N"], dtype=torch.float64)
    for e, (c, o) in enumerate(zip(p["counts"], p["offs_l"])):
        out[o:o + c] = rows64[o:o + c] @ p["W"][e].T + (p["bias_cpu"][e].double() if bias else 0.0)
    return out


def quantised(mode, x):
    """The rows as the pre-quantised entry of ``mode`` takes them: (e4m3 bytes, act_scale) or (blocks, scales)."""
    if mode == FP8:                                                 # (on the host: any e4m3 bytes will do here)
        x8, scale = ops().quantize_activations_fp8(x.cpu())
        return x8.view(torch.uint8).to(DEV), scale.to(DEV)
    return ops().quantize_rows_mxfp4(x)


def values64(mode, a, b):
    """The float64 values a pair of ``quantised`` stands for (on the host)."""
    if mode == FP8:
        return a.cpu().view(torch.float8_e4m3fn).float().double() * b.double().cpu()[:, None]
    from fused_int4_amd.quantize import dequantize_mxfp4
    return dequantize_mxfp4(a.cpu(), b.cpu()).double()


def run_pre(mode, p, a, b, bias=False, out_dtype=torch.float32, **over):
    """The pre-quantised entry of ``mode`` (ops.moe_forward_mxfp4_fp8 / ops.moe_forward_mxfp4_fp4)."""
    w = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    w.update(over)
    op = ops().moe_forward_mxfp4_fp8 if mode == FP8 else ops().moe_forward_mxfp4_fp4
    return op(w["blocks"], w["scales"], a, b, w["tpe"], w["offs"],
              bias=p["bias"] if bias is True else (None if bias is False else bias), out_dtype=out_dtype)


def run_q(mode, p, x, bias=False, out_dtype=None):
    """The quantising entry of ``mode`` (ops.moe_forward_mxfp4 with ``precision=``)."""
    return ops().moe_forward_mxfp4(p["blocks"], p["scales"], x, p["tpe"], p["offs"], bias=p["bias"] if bias else None,
                                   out_dtype=out_dtype, precision=PRECISION[mode])


def both(force, mode, call):
    """The same call under the tile kernel and under the decode kernel of ``mode``."""
    force(mode, "tile")
    want = call()
    force(mode, "decode")
    return call(), want


def c_pre(mode, p, a, b, dout, bias=True, table=True, a_ptr=None):
    """The pre-quantised C entry itself: E = 1 without a table, or rows at an address of the caller's choice."""
    out = torch.empty(p["T"], p["N"], dtype=dout, device=DEV)
    fn = lib().fql_moe_mx4_fwd_f8 if mode == FP8 else lib().fql_moe_mx4_fwd_f4
    rc = fn(p["blocks"].data_ptr(), p["scales"].data_ptr(), a.data_ptr() if a_ptr is None else a_ptr,
            None if b is None else b.data_ptr(), p["bias"].data_ptr() if bias else None,
            p["tpe"].data_ptr() if table else None, p["offs"].data_ptr() if table else None, out.data_ptr(), DT[dout],
            p["E"] if table else 1, p["T"], p["K"], p["N"], None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return out


# ---- 1. the same bits as the tile kernel

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_same_bits_as_the_tile_kernel(force, K, N, mode):
    p = problem(K, N)
    a, b = quantised(mode, p["x"])
    for dout in (torch.float32, torch.bfloat16, torch.float16):
        for bias in (False, True):
            got, want = both(force, mode, lambda: run_pre(mode, p, a, b, bias=bias, out_dtype=dout))
            assert same_bits(got, want), (K, N, "pre", dout, bias)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
            for din in (torch.float32, torch.bfloat16):
                x = p["x"].to(din)
                got, want = both(force, mode, lambda: run_q(mode, p, x, bias=bias, out_dtype=dout))
                assert same_bits(got, want), (K, N, din, dout, bias)
    force(mode, "decode")
    assert lib().fql_tune_mx4_scaled_kernel(mode, p["E"], p["T"], K, N) == 1
    force(mode, "tile")
    assert lib().fql_tune_mx4_scaled_kernel(mode, p["E"], p["T"], K, N) == 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96])
def test_gated_op_same_bits(force, F, kind, mode):
    p = problem(F, 40, seed=7)
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = (torch.randn(p["T"], 2 * F, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            got, want = both(force, mode, lambda: ops().moe_gated_forward_mxfp4(
                p["blocks"], p["scales"], gate_up.to(din), p["tpe"], p["offs"], bias=p["bias"], out_dtype=dout,
                precision=PRECISION[mode], **act_kw(kind)))
            assert same_bits(got, want), (F, kind, din, dout)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K,N", [(96, 40), (608, 37)])
def test_edge_weight_scale_codes_same_bits(force, K, N, mode):
    """Weight scale codes 0, 1, 254 and 255 next to ordinary ones: tiny weights, huge weights and a NaN block."""
    p = problem(K, N)
    scales = p["scales"].clone()
    for i, code in enumerate((0, 1, 254, 255, 0, 255)):
        scales[2 + i % 3, (5 * i + 3) % N, i % (K // 32)] = code
    assert {0, 1, 254, 255} <= set(scales.unique().tolist())
    a, b = quantised(mode, p["x"])
    got, want = both(force, mode, lambda: run_pre(mode, p, a, b, bias=True, scales=scales))
    assert same_bits(got, want), (K, N)
    assert bool(torch.isnan(got).any()) and not bool(torch.isnan(got).all())
    for din in (torch.float32, torch.bfloat16):
        w = dict(p, scales=scales)
        got, want = both(force, mode, lambda: run_q(mode, w, p["x"].to(din), bias=True))
        assert same_bits(got, want), (K, N, din)
        assert bool(torch.isnan(got).any()) and not bool(torch.isnan(got).all())


def test_fp8_nan_bytes_nan_scale_and_rows_off_a_16_byte_boundary(force):
    """e4m3 NaN bytes 0x7F and 0xFF in two rows and a NaN act_scale in a third: exactly those rows are NaN, the others have
    the clean run's bits, and the decode kernel agrees with the tile kernel bit for bit; then the same rows one byte past a
    16-byte boundary (the byte loads of both kernels) through the C entry."""
    p = problem(608, 136)
    offs = p["offs_l"]
    x8, act = quantised(FP8, p["x"])
    clean = both(force, FP8, lambda: run_pre(FP8, p, x8, act, bias=True))
    assert same_bits(*clean)
    x8, act = x8.clone(), act.clone()
    t_7f, t_ff, t_as = offs[4] + 32, offs[2] + 3, offs[3] + 31      # the second row block's only row; one of a few; a block's last
    x8[t_7f, 601] = 0x7F                                            # (k = 601: the upper lane half's bytes of the odd tail)
    x8[t_ff, 64] = 0xFF
    act[t_as] = NAN
    got, want = both(force, FP8, lambda: run_pre(FP8, p, x8, act, bias=True))
    assert same_bits(got, want)
    expect = torch.zeros_like(got, dtype=torch.bool)
    expect[[t_7f, t_ff, t_as]] = True
    assert torch.equal(torch.isnan(got), expect)
    assert same_bits(got[~expect], clean[0][~expect])
    rows = guarded_like("rows", x8, 0x7F, offset=1)                 # (a guard byte that is used is a NaN)
    assert rows.ptr % 16 == 1
    for dout in (torch.float32, torch.bfloat16):
        force(FP8, "tile")
        want = c_pre(FP8, p, x8, act, dout)
        assert same_bits(want, c_pre(FP8, p, x8, act, dout, a_ptr=rows.ptr))
        force(FP8, "decode")
        assert same_bits(c_pre(FP8, p, x8, act, dout, a_ptr=rows.ptr), want)
        assert same_bits(c_pre(FP8, p, x8, act, dout), want)
    assert_guards_intact(rows, what="e4m3 rows one byte past a 16-byte boundary")


def test_fp4_row_scale_codes_0_254_and_255(force):
    """Row scale codes 0 and 254 (2^-127 and 2^127; the 254 block keeps one nonzero code, so its sums hold one infinite
    term at most and no NaN) and 255 in two rows: exactly the 255 rows are NaN, the others have the clean run's bits
    where their own bytes did not change, and the decode kernel agrees with the tile kernel bit for bit."""
    p = problem(608, 136)
    offs = p["offs_l"]
    xb, xs = quantised(FP4, p["x"])
    clean = both(force, FP4, lambda: run_pre(FP4, p, xb, xs, bias=True))
    assert same_bits(*clean)
    xb, xs = xb.clone(), xs.clone()
    t_0, t_254, t_255a, t_255b = offs[3] + 7, offs[3] + 8, offs[4] + 32, offs[2] + 3
    xs[t_0, 5] = 0
    xs[t_254, 18] = 254                                             # (block 18: the odd tail's)
    xb[t_254, 16 * 18:16 * 19] = 0
    xb[t_254, 16 * 18 + 3] = 0x70                                   # one code: +6
    xs[t_255a, 18] = 255
    xs[t_255b, 1] = 255                                             # (the upper lane half of the first instruction)
    got, want = both(force, FP4, lambda: run_pre(FP4, p, xb, xs, bias=True))
    assert same_bits(got, want)
    expect = torch.zeros_like(got, dtype=torch.bool)
    expect[[t_255a, t_255b]] = True
    assert torch.equal(torch.isnan(got), expect)
    assert bool(torch.isinf(got[t_254]).any())
    same = ~expect
    same[[t_0, t_254]] = False
    assert same_bits(got[same], clean[0][same])


# ---- 2. exactness, without the tile kernel

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_decode_kernel_is_exact_on_integer_data(force, K, N, mode):
    """fp8: integers in [-4, 4] as e4m3 bytes; fp4: e2m1 integers {0, +-1, +-2, +-3, +-4, +-6} with row scale code 127;
    random weight codes with scale codes in [125, 129].  Every product is a multiple of 2^-3 and every sum is below 2^15
    (asserted), far inside the 2^21 up to which float32 holds multiples of 2^-3, so the float32 result is the float64
    reference bit for bit whatever the order.  The data is asymmetric: a swapped lane half, a wrong k slot or a scale on
    the wrong block fails."""
    p = problem(K, N, lo=125, hi=129, integer=True)
    a, b = (p["x8"], None) if mode == FP8 else (p["xb"], p["xs"])
    name = "ref8" if mode == FP8 else "ref4"
    force(mode, "decode")
    for bias in (False, True):
        ref = p[name + "_b"] if bias else p[name]
        assert float(ref.abs().max()) < 2 ** 15
        assert torch.equal(ref * 8, (ref * 8).round())
        got = run_pre(mode, p, a, b, bias=bias)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                     # uncovered rows: exactly zero
        got16 = run_pre(mode, p, a, b, bias=bias, out_dtype=torch.bfloat16)      # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())
    if mode == FP8:                                                              # a power-of-two act_scale: still exact
        act = torch.full((p["T"],), 0.25, device=DEV)
        assert torch.equal(run_pre(mode, p, a, act, bias=False).cpu().double(), p["ref8"] * 0.25)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K,N", [(32, 8), (96, 40), (608, 37)])
def test_one_expert_one_row_no_table(force, K, N, mode):
    p = problem(K, N, counts=(1,), tail=0, lo=125, hi=129, integer=True)
    a, b = (p["x8"], None) if mode == FP8 else (p["xb"], p["xs"])
    force(mode, "decode")
    got = c_pre(mode, p, a, b, torch.float32, table=False)
    assert torch.equal(got.cpu().double(), p["ref8_b" if mode == FP8 else "ref4_b"])
    force(mode, "tile")
    assert same_bits(c_pre(mode, p, a, b, torch.float32, table=False), got)
    q = problem(K, N, counts=(1,), tail=0)
    a, b = quantised(mode, q["x"])
    force(mode, "decode")
    got = c_pre(mode, q, a, b, torch.bfloat16, table=False)
    force(mode, "tile")
    assert same_bits(c_pre(mode, q, a, b, torch.bfloat16, table=False), got)


# ---- 3. independence, bit for bit

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K,N", [(608, 136), (96, 40)])
def test_decode_grouped_equals_one_expert_calls_permutation_and_rerun(force, K, N, mode):
    p = problem(K, N)
    a, b = quantised(mode, p["x"])
    force(mode, "decode")
    got = run_pre(mode, p, a, b, bias=True)
    assert same_bits(got, run_pre(mode, p, a, b, bias=True))                     # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs_l"])):
        if c == 0:
            continue
        one = run_pre(mode, p, a[o:o + c].contiguous(), b[o:o + c].contiguous(), bias=p["bias"][e:e + 1],
                      blocks=p["blocks"][e:e + 1], scales=p["scales"][e:e + 1],
                      tpe=torch.tensor([c], dtype=torch.int32, device=DEV), offs=torch.zeros(1, dtype=torch.int32, device=DEV))
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    again = run_pre(mode, p, a, b, bias=p["bias"][perm], blocks=p["blocks"][perm], scales=p["scales"][perm],
                    tpe=p["tpe"][perm], offs=p["offs"][perm])
    assert same_bits(again, got)


# ---- 4. guard bands

ENTRIES = ["f8", "q8", "glu_q8", "f4", "q4", "glu_q4"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(96, 37), (608, 136)])
def test_decode_kernel_stays_inside_its_buffers(force, K, N, dout, entry):
    """Every pointer is the interior of a guarded buffer.  The rows start one element past a 256-byte boundary (the element
    loads; the packed MXFP4 rows keep the 16 bytes the library asks for) and so does out (the element stores); blocks
    keeps its 16 bytes.  Only [T, N] (and the workspace) changes, the guards stay, uncovered rows are zero and the bits are
    the public op's under the tile kernel.  The entries with a workspace then run once per stale workspace content
    (PREFILLS) and must return those bits each time."""
    mode = FP8 if entry.endswith("8") else FP4
    gated, quantising = entry.startswith("glu"), "q" in entry
    L = lib()
    p = problem(K, N)
    E, T = p["E"], p["T"]
    assert T == 73
    esz = torch.empty((), dtype=dout).element_size()
    st = torch.cuda.current_stream().cuda_stream
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    out = Guarded("out", T * N * esz, dout, SENT, offset=esz)
    out.view(dout, T, N).fill_(SENT)
    assert out.ptr % 16 == esz
    tail = (bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N)
    wsq = L.fql_moe_mx4_f8_workspace_bytes if mode == FP8 else L.fql_moe_mx4_f4_workspace_bytes
    force(mode, "tile")
    if not quantising:
        a, b = quantised(mode, p["x"])
        want = run_pre(mode, p, a, b, bias=True, out_dtype=dout)
        if mode == FP8:
            rw, sg = guarded_like("rows", a, 0x7F, offset=1), guarded_like("act_scale", b, NAN)
            assert rw.ptr % 16 == 1
            call = lambda: L.fql_moe_mx4_fwd_f8(bl.ptr, sc.ptr, rw.ptr, sg.ptr, *tail, None, 0, st)
        else:
            rw, sg = guarded_like("in_blocks", a, 0xFF, offset=16), guarded_like("in_scales", b, 0xFF, offset=1)
            call = lambda: L.fql_moe_mx4_fwd_f4(bl.ptr, sc.ptr, rw.ptr, sg.ptr, *tail, None, 0, st)
        bufs, ws = (bl, sc, rw, sg, bias, cnt, off, out), None
    else:
        if gated:
            g = torch.Generator().manual_seed(3)
            rows = torch.randn(T, 2 * K, generator=g).to(DEV)
            want = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], rows, p["tpe"], p["offs"], bias=p["bias"],
                                                 out_dtype=dout, precision=PRECISION[mode], **act_kw("swiglu_clamp"))
        else:
            rows = p["x"]
            want = run_q(mode, p, rows, bias=True, out_dtype=dout)
        nbytes = wsq(E, T, K, N, 2 if gated else 1)
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        rw = guarded_like("rows", rows, NAN, offset=4)
        assert rw.ptr % 16 == 4
        name = f"fql_moe_mx4_{'glu_' if gated else ''}fwd_q{8 if mode == FP8 else 4}"
        act = (2, 1.702, 7.0) if gated else ()
        call = lambda: getattr(L, name)(bl.ptr, sc.ptr, rw.ptr, 0, *tail, *act, ws.ptr, nbytes, st)
        bufs = (bl, sc, rw, bias, cnt, off, out, ws)
    force(mode, "decode")
    assert L.fql_tune_mx4_scaled_kernel(mode, E, T, K, N) == 1
    got = out.view(dout, T, N)
    for fill in (None,) + (PREFILLS if ws is not None else ()):
        if fill is not None:                        # what an earlier launch may have left in the workspace: the same bits
            ws.bytes().fill_(fill)
            got.fill_(SENT)
        assert call() == 0
        assert_guards_intact(*bufs, what=f"mx4 scaled decode {entry} K={K} N={N} {dout} workspace {fill}")
        assert torch.count_nonzero(got[T - TAIL:]) == 0, fill
        assert same_bits(got, want), fill


# ---- 5. the dispatch, end to end

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_layer_in_the_block_takes_the_kernel_the_library_reports(force, mode):
    """E = 4, H = 64, F = 96 with biases inside QuantizedSparseMoEBlock, top-2, 3 tokens, under no_grad: 6 routed rows."""
    E, H, F, T, TOPK = 4, 64, 96, 3, 2
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    experts = fq().MXFP4MoEFFN.from_weights(mk(F, H), mk(F, H), mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H),
                                            precision=PRECISION[mode], **act_kw("swiglu_clamp"))
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=TOPK, experts=experts, router_bias=True).to(DEV)
    x = torch.randn(T, H, generator=g).to(DEV)
    default = lib().fql_tune_set_mx4_scaled_decode_max_rows(mode, -1)
    rows = T * TOPK
    for K, N in ((H, 2 * F), (F, H)):                                # the layer's two calls
        assert lib().fql_tune_mx4_scaled_kernel(mode, E, rows, K, N) == (1 if rows <= default else 0)
    outs = {}
    with torch.no_grad():
        for which in ("default", "tile", "decode"):
            force(mode, which)
            outs[which] = blk(x)[0]
    assert same_bits(outs["default"], outs["tile"])
    assert same_bits(outs["decode"], outs["tile"])
    assert bool(torch.isfinite(outs["tile"]).all()) and float(outs["tile"].abs().max()) > 0


# ---- 6. graph replay

def capture(call, static):
    """Warm ``call(*static)`` up twice on a side stream, capture it once on that stream (tests/test_gpu_graph_replay.py)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            call(*static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call(*static)
    return graph, out


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_captured_decode_call_replays_on_a_rewritten_table_and_rows(force, mode):
    """One call (the quantising pre-pass and the decode kernel: one launch chain, no parallel branches) captured with the
    decode kernel forced, replayed after the table and the rows were rewritten in place, against an eager tile-kernel call
    on the new contents."""
    K, N = 608, 136
    p = problem(K, N)
    T = p["T"]
    x, tpe, offs = p["x"].clone(), p["tpe"].clone(), p["offs"].clone()
    call = lambda x, tpe, offs: ops().moe_forward_mxfp4(p["blocks"], p["scales"], x, tpe, offs, bias=p["bias"],
                                                        precision=PRECISION[mode])
    force(mode, "decode")
    graph, out = capture(call, (x, tpe, offs))
    graph.replay()
    torch.cuda.synchronize()
    force(mode, "tile")
    assert same_bits(out, call(x, tpe, offs))
    t2, o2, total = expert_table([33, 2, 0, 30, 4], tail=4, device="cpu")
    assert total == T
    g = torch.Generator().manual_seed(99)
    x.copy_(torch.randn(T, K, generator=g))
    tpe.copy_(t2)
    offs.copy_(o2)
    want = call(x, tpe, offs)                                        # eager, the tile kernel, the new contents
    force(mode, "decode")                                            # (the graph holds its kernel whatever the threshold says now)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want)
    assert torch.count_nonzero(out[T - 4:]) == 0 and float(out[:T - 4].abs().max()) > 0


# ---- 7. the tolerance the bits inherit

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_decode_kernel_within_the_bound_of_this_arithmetic(force, mode):
    p = problem(608, 40)
    a, b = quantised(mode, p["x"])
    vals = values64(mode, a, b)
    force(mode, "decode")
    for bias in (False, True):
        err = rel_fro_dev(run_pre(mode, p, a, b, bias=bias), ref64(p, vals, bias))
        print(f"mxfp4 {PRECISION[mode]} decode K=608 N=40 bias={bias}: rel_fro {err:.3e} (bound {SAME_INPUT_BOUND[mode]:.2e})")
        assert err <= SAME_INPUT_BOUND[mode]
