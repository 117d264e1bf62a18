"""The decode kernel of the bfloat16 MXFP4 forward (csrc/fql_gemm_mx4_decode.h) on the GPU.  ops.moe_forward_mxfp4 and
ops.moe_gated_forward_mxfp4 pick it from T; here fql_tune_set_mx4_decode_max_rows forces either kernel.

The contract is that the decode kernel returns THE SAME BITS as the tile kernel (mx4_kernel), so the main test compares
the two; the exactness test stands without the tile kernel, so a mistake the two share cannot hide.

The shapes are the smallest at which this kernel can go wrong: K in {32, 96, 288} (one scale block: only one lane half
has a piece; three blocks: an odd tail behind a pair; nine blocks: deeper than the load ring, with an odd tail), N in
{8, 37, 40, 136} (under one 32-row fragment; N % 4 != 0: element stores; a partial second wave; past 128), a table of
[0, 1, 5, 32, 33] rows plus 2 uncovered (an empty expert, one row, a few rows, a full row block, a second row block) and
E = 1 with one row and no table."""
import functools

import pytest
import torch

from glu_reference import act_kw
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_MAX = 2 ** 31 - 1
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
COUNTS, TAIL = [0, 1, 5, 32, 33], 2
KS, NS = [32, 96, 288], [8, 37, 40, 136]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
PREFILLS = (0x00, 0xFF, 0x7F)     # stale workspace bytes (tests/test_gpu_footprint.py); 0xFF is a NaN as bfloat16
# relative Frobenius error of the float32 result against the float64 product of the same rounded inputs: the bound
# tests/test_gpu_mxfp4.py asserts for this arithmetic (4 x the 6.6e-8 it measured); the bits are the same, so is the bound
SAME_INPUT_BOUND = 2.64e-7


def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def force():
    """force("decode") / force("tile") / force("default"); the library's own threshold comes back afterwards."""
    default = lib().fql_tune_set_mx4_decode_max_rows(-1)            # (a negative value changes nothing)

    def use(which):
        lib().fql_tune_set_mx4_decode_max_rows({"decode": INT_MAX, "tile": 0, "default": default}[which])
    try:
        yield use
    finally:
        lib().fql_tune_set_mx4_decode_max_rows(default)


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


@functools.lru_cache(maxsize=None)
def problem(K, N, counts=tuple(COUNTS), tail=TAIL, lo=97, hi=157, integer=False, seed=0):
    """Random element codes and per-(row, block) scale codes in [lo, hi]; activations randn, or (``integer``) integers in
    [-4, 4].  ``ref`` / ``ref_b``: float64, the product of the bfloat16-rounded activations and the exactly dequantised
    weights (+ the bias), zero on the rows no expert covers.  Computed once per shape and shared; nobody writes to it."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    g = torch.Generator().manual_seed(7919 * K + N + seed)
    E = len(counts)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)
    blocks = pack(codes)
    W = dequantize_mxfp4(blocks, scales).double()
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    x = torch.randint(-4, 5, (T, K), generator=g).float() if integer else torch.randn(T, K, generator=g)
    bias = torch.randint(-8, 9, (E, N), generator=g).float() if integer else torch.randn(E, N, generator=g)
    xr = x.bfloat16().double()
    ref, ref_b = torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64)
    for e, (c, o) in enumerate(zip(tpe.tolist(), offs.tolist())):
        ref[o:o + c] = xr[o:o + c] @ W[e].T
        ref_b[o:o + c] = ref[o:o + c] + bias[e].double()
    return dict(E=E, T=T, K=K, N=N, blocks=blocks.to(DEV), scales=scales.to(DEV), x=x.to(DEV), bias=bias.to(DEV),
                tpe=tpe.to(DEV), offs=offs.to(DEV), ref=ref, ref_b=ref_b, counts=list(counts))


def run(p, x=None, bias=False, out_dtype=None, **over):
    a = dict(blocks=p["blocks"], scales=p["scales"], tpe=p["tpe"], offs=p["offs"])
    a.update(over)
    return ops().moe_forward_mxfp4(a["blocks"], a["scales"], p["x"] if x is None else x, a["tpe"], a["offs"],
                                   bias=p["bias"] if bias is True else (None if bias is False else bias), out_dtype=out_dtype)


def both(force, call):
    """The same call under the tile kernel and under the decode kernel."""
    force("tile")
    want = call()
    force("decode")
    return call(), want


def no_table(p, din, dout, bias=True):
    """E = 1, no table: the C entry itself (the public op always passes one)."""
    x = p["x"].to(din).contiguous()
    out = torch.empty(p["T"], p["N"], dtype=dout, device=DEV)
    rc = lib().fql_moe_mx4_fwd(p["blocks"].data_ptr(), p["scales"].data_ptr(), x.data_ptr(), DT[din],
                               p["bias"].data_ptr() if bias else None, None, None, out.data_ptr(), DT[dout], 1, p["T"], p["K"],
                               p["N"], None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return out


# ---- 1. the same bits as the tile kernel

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_same_bits_as_the_tile_kernel(force, K, N):
    p = problem(K, N)
    assert lib().fql_tune_mx4_kernel(p["E"], p["T"], K, N) in (0, 1)
    for din in (torch.float32, torch.bfloat16):
        x = p["x"].to(din)
        for dout in (torch.float32, torch.bfloat16, torch.float16):
            for bias in (False, True):
                got, want = both(force, lambda: run(p, x, bias=bias, out_dtype=dout))
                assert same_bits(got, want), (K, N, din, dout, bias)
    force("decode")
    assert lib().fql_tune_mx4_kernel(p["E"], p["T"], K, N) == 1
    force("tile")
    assert lib().fql_tune_mx4_kernel(p["E"], p["T"], K, N) == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [32, 96])
def test_gated_op_same_bits(force, F, kind):
    p = problem(F, 40, seed=7)
    g = torch.Generator().manual_seed(F + len(kind))
    gate_up = (torch.randn(p["T"], 2 * F, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            got, want = both(force, lambda: ops().moe_gated_forward_mxfp4(
                p["blocks"], p["scales"], gate_up.to(din), p["tpe"], p["offs"], bias=p["bias"], out_dtype=dout, **act_kw(kind)))
            assert same_bits(got, want), (F, kind, din, dout)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0


@pytest.mark.parametrize("K,N", [(96, 40), (288, 37)])
def test_edge_scale_codes_same_bits(force, K, N):
    """Scale codes 0, 1, 254 and 255 next to ordinary ones: flushed weights, infinite weights and a NaN block."""
    p = problem(K, N)
    scales = p["scales"].clone()
    for i, code in enumerate((0, 1, 254, 255, 0, 255)):
        scales[2 + i % 3, (5 * i + 3) % N, i % (K // 32)] = code
    assert {0, 1, 254, 255} <= set(scales.unique().tolist())
    for din in (torch.float32, torch.bfloat16):
        got, want = both(force, lambda: run(p, p["x"].to(din), bias=True, out_dtype=torch.float32, scales=scales))
        assert same_bits(got, want), (K, N, din)
        assert bool(torch.isnan(got).any()) and not bool(torch.isnan(got).all())


@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_inf_and_nan_rows_same_bits(force, din):
    p = problem(288, 136)
    offs = p["offs"].tolist()
    x = p["x"].to(din).clone()
    t_inf, t_nan = offs[4] + 32, offs[2] + 3                        # the second row block's only row; one of a few rows
    x[t_inf, 201] = float("inf")                                    # (k = 201: the upper lane half of its step)
    x[t_nan, 64] = NAN
    got, want = both(force, lambda: run(p, x, bias=True))
    assert same_bits(got, want)
    expect = torch.zeros_like(got, dtype=torch.bool)
    expect[t_inf] = True
    expect[t_nan] = True
    assert torch.equal(torch.isnan(got), expect)
    clean = run(p, p["x"].to(din), bias=True)
    assert same_bits(got[~expect], clean[~expect])


# ---- 2. exactness, without the tile kernel

@pytest.mark.parametrize("din", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_decode_kernel_is_exact_on_integer_data(force, K, N, din):
    """Integer activations in [-4, 4], random codes, scale codes in [125, 129]: every product is a multiple of 2^-3 and
    every partial sum is below 2^15, so the float32 result is the integer reference bit for bit whatever the order.  The
    weight matrix is asymmetric: a swapped lane half, a wrong k slot or a scale on the wrong block fails."""
    p = problem(K, N, lo=125, hi=129, integer=True)
    force("decode")
    for bias in (False, True):
        ref = p["ref_b"] if bias else p["ref"]
        assert float(ref.abs().max()) < 2 ** 15
        got = run(p, p["x"].to(din), bias=bias, out_dtype=torch.float32)
        assert torch.equal(got.cpu().double(), ref), (K, N, bias)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                     # uncovered rows: exactly zero
        got16 = run(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16)      # one rounding of the exact value
        assert same_bits(got16.cpu(), ref.float().bfloat16())


@pytest.mark.parametrize("K,N", [(32, 8), (96, 40), (288, 37)])
def test_one_expert_one_row_no_table(force, K, N):
    p = problem(K, N, counts=(1,), tail=0, lo=125, hi=129, integer=True)
    force("decode")
    got = no_table(p, torch.float32, torch.float32)
    assert torch.equal(got.cpu().double(), p["ref_b"])
    force("tile")
    assert same_bits(no_table(p, torch.float32, torch.float32), got)
    q = problem(K, N, counts=(1,), tail=0)
    for din in (torch.float32, torch.bfloat16):
        force("decode")
        got = no_table(q, din, torch.bfloat16)
        force("tile")
        assert same_bits(no_table(q, din, torch.bfloat16), got)


# ---- 3. independence, bit for bit

@pytest.mark.parametrize("K,N", [(288, 136), (96, 40)])
def test_decode_grouped_equals_one_expert_calls_permutation_and_rerun(force, K, N):
    p = problem(K, N)
    force("decode")
    got = run(p, bias=True)
    assert same_bits(got, run(p, bias=True))                                     # two runs agree
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_forward_mxfp4(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["x"][o:o + c].contiguous(),
                                      torch.tensor([c], dtype=torch.int32, device=DEV),
                                      torch.zeros(1, dtype=torch.int32, device=DEV), bias=p["bias"][e:e + 1])
        assert same_bits(one, got[o:o + c]), e
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    again = ops().moe_forward_mxfp4(p["blocks"][perm], p["scales"][perm], p["x"], p["tpe"][perm], p["offs"][perm],
                                    bias=p["bias"][perm])
    assert same_bits(again, got)


# ---- 4. guard bands

@pytest.mark.parametrize("gated", [False, True], ids=["plain", "glu"])
@pytest.mark.parametrize("din,dout", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                      (torch.float32, torch.float16)], ids=["f32", "bf16", "f32-f16"])
@pytest.mark.parametrize("K,N", [(96, 37), (288, 136)])
def test_decode_kernel_stays_inside_its_buffers(force, K, N, din, dout, gated):
    """Every pointer is the interior of a guarded buffer.  The rows start one element past a 256-byte boundary (the
    element loads) and so does out (the element stores); blocks keeps the 16 bytes the library asks for.  Only [T, N]
    changes, the guards stay, uncovered rows are zero and the bits are the public op's under the tile kernel.  The gated
    entry then runs once per stale workspace content (PREFILLS) and must return those bits each time."""
    p = problem(K, N)
    E, T = p["E"], p["T"]
    assert T == 73
    if gated:
        g = torch.Generator().manual_seed(3)
        rows = torch.randn(T, 2 * K, generator=g).to(DEV).to(din)
    else:
        rows = p["x"].to(din)
    esz_in, esz = rows.element_size(), torch.empty((), dtype=dout).element_size()
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    rw, bias = guarded_like("rows", rows, NAN, offset=esz_in), guarded_like("bias", p["bias"], NAN)
    cnt, off = guarded_like("tokens_per_expert", p["tpe"], 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    out = Guarded("out", T * N * esz, dout, SENT, offset=esz)
    out.view(dout, T, N).fill_(SENT)
    assert rw.ptr % 16 == esz_in and out.ptr % 16 == esz
    nbytes = lib().fql_moe_mx4_workspace_bytes(E, T, K, N, int(gated))
    st = torch.cuda.current_stream().cuda_stream
    force("tile")
    if gated:
        want = ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], rows, p["tpe"], p["offs"], bias=p["bias"],
                                             out_dtype=dout, **act_kw("swiglu_clamp"))
    else:
        want = run(p, rows, bias=True, out_dtype=dout)
    force("decode")
    assert lib().fql_tune_mx4_kernel(E, T, K, N) == 1
    if gated:
        ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
        rc = lib().fql_moe_mx4_glu_fwd(bl.ptr, sc.ptr, rw.ptr, DT[din], bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                       2, 1.702, 7.0, ws.ptr, nbytes, st)
        bufs = (bl, sc, rw, bias, cnt, off, out, ws)
    else:
        rc = lib().fql_moe_mx4_fwd(bl.ptr, sc.ptr, rw.ptr, DT[din], bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                   None, 0, st)
        bufs = (bl, sc, rw, bias, cnt, off, out)
    assert rc == 0
    assert_guards_intact(*bufs, what=f"mx4 decode gated={gated} K={K} N={N} {din} {dout}")
    got = out.view(dout, T, N)
    assert torch.count_nonzero(got[T - TAIL:]) == 0
    assert same_bits(got, want)
    if gated:                                       # what an earlier launch may have left in the workspace: the same bits
        for fill in PREFILLS:
            ws.bytes().fill_(fill)
            got.fill_(SENT)
            rc = lib().fql_moe_mx4_glu_fwd(bl.ptr, sc.ptr, rw.ptr, DT[din], bias.ptr, cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K,
                                           N, 2, 1.702, 7.0, ws.ptr, nbytes, st)
            assert rc == 0
            assert_guards_intact(*bufs, what=f"mx4 decode gated K={K} N={N} {din} {dout} workspace {fill:#04x}")
            assert torch.count_nonzero(got[T - TAIL:]) == 0, hex(fill)
            assert same_bits(got, want), hex(fill)


# ---- 5. the dispatch, end to end

def test_layer_in_the_block_takes_the_kernel_the_library_reports(force):
    """E = 4, H = 64, F = 96 with biases inside QuantizedSparseMoEBlock, top-2, 3 tokens, under no_grad: 6 routed rows."""
    E, H, F, T, TOPK = 4, 64, 96, 3, 2
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: [torch.randn(*s, generator=g) * 0.2 for _ in range(E)]
    experts = fq().MXFP4MoEFFN.from_weights(mk(F, H), mk(F, H), mk(H, F), gate_bias=mk(F), up_bias=mk(F), down_bias=mk(H),
                                            **act_kw("swiglu_clamp"))
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=TOPK, experts=experts, router_bias=True).to(DEV)
    x = torch.randn(T, H, generator=g).to(DEV)
    default = lib().fql_tune_set_mx4_decode_max_rows(-1)
    rows = T * TOPK
    for K, N in ((H, 2 * F), (F, H)):                                # the layer's two calls
        assert lib().fql_tune_mx4_kernel(E, rows, K, N) == (1 if rows <= default else 0)
    outs = {}
    with torch.no_grad():
        for which in ("default", "tile", "decode"):
            force(which)
            outs[which] = blk(x)[0]
    assert same_bits(outs["default"], outs["tile"])
    assert same_bits(outs["decode"], outs["tile"])
    assert bool(torch.isfinite(outs["tile"]).all()) and float(outs["tile"].abs().max()) > 0


# ---- 6. the tolerance the bits inherit

def test_decode_kernel_within_the_bound_of_this_arithmetic(force):
    p = problem(288, 40)
    force("decode")
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            err = rel_fro_dev(run(p, p["x"].to(din), bias=bias, out_dtype=torch.float32), p["ref_b"] if bias else p["ref"])
            print(f"mxfp4 decode K=288 N=40 in={din} bias={bias}: rel_fro {err:.3e} (bound {SAME_INPUT_BOUND:.2e})")
            assert err <= SAME_INPUT_BOUND
