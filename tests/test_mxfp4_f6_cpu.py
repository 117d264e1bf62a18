"""MXFP4 expert weights over MXFP6 rows (e2m3 elements with E8M0 block scales), the part that needs no GPU: the host
quantiser ``quantize.quantize_mxfp6`` / ``dequantize_mxfp6`` and the pack / unpack helpers, the C ABI of FQL_VERSION 400
(fql_moe_mx4_fwd_f6 / fql_moe_mx4_fwd_q6 / fql_moe_mx4_glu_fwd_q6 / fql_mx6_quantize_rows and the workspace query: declared,
exported and validated in fql_moe_mx4_fwd's order before any HIP call -- every call below is invalid, empty or stops at the
workspace check, so none launches), the tuning hooks of its decode threshold, ``precision="fp6"`` of MXFP4MoEFFN and what
the ops refuse on the host."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_mx4_f6_workspace_bytes", "fql_moe_mx4_fwd_f6", "fql_moe_mx4_fwd_q6", "fql_moe_mx4_glu_fwd_q6",
       "fql_mx6_quantize_rows")
HOOKS = ("fql_tune_set_mx4_f6_decode_max_rows", "fql_tune_mx4_f6_kernel")
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
SILU, GELU, CLAMP = 0, 1, 2
NAN = float("nan")
INT_MAX = 2 ** 31 - 1
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 8
P_8 = ctypes.c_void_p(24)      # 8-byte aligned, not 16


def r16(n):
    return (n + 15) // 16 * 16


def Q():
    from fused_int4_amd import quantize
    return quantize


# ---- the host quantiser

def e2m3(c):
    e, m = (c >> 3) & 3, c & 7
    v = m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)
    return -v if c & 32 else v


def test_exported_from_the_package():
    import fused_int4_amd
    for name in ("quantize_mxfp6", "dequantize_mxfp6"):
        assert name in fused_int4_amd.__all__ and getattr(fused_int4_amd, name) is getattr(Q(), name)
    for name in ("pack_mxfp6", "unpack_mxfp6", "quantize_mxfp6", "dequantize_mxfp6", "MXFP6_VALUES"):
        assert name in Q().__all__


def test_table_is_e2m3():
    assert [e2m3(c) for c in range(64)] == list(Q().MXFP6_VALUES)
    assert Q().MXFP6_VALUES[31] == 7.5 and Q().MXFP6_VALUES[8] == 1.0 and Q().MXFP6_VALUES[1] == 0.125
    assert len({abs(v) for v in Q().MXFP6_VALUES}) == 32


def test_pack_unpack_of_a_block_whose_elements_are_all_distinct():
    codes = torch.tensor([(7 * i + 3) % 64 for i in range(32)] + list(range(63, 31, -1)), dtype=torch.uint8).reshape(1, 64)
    assert len(set(codes[0, :32].tolist())) == 32 and len(set(codes[0, 32:].tolist())) == 32
    packed = Q().pack_mxfp6(codes)
    assert packed.shape == (1, 48) and packed.dtype == torch.uint8
    for b in range(2):                                                       # the public layout: one little-endian 192-bit integer
        big = int.from_bytes(bytes(packed[0, 24 * b:24 * b + 24].tolist()), "little")
        assert [(big >> (6 * i)) & 63 for i in range(32)] == codes[0, 32 * b:32 * b + 32].tolist()
    assert torch.equal(Q().unpack_mxfp6(packed), codes)
    with pytest.raises(ValueError):
        Q().pack_mxfp6(torch.zeros(1, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        Q().unpack_mxfp6(torch.zeros(1, 16, dtype=torch.uint8))


@pytest.mark.parametrize("shift", [-126, -20, 0, 3, 100])
def test_all_64_codes_round_trip(shift):
    """A block that holds 7.5 has shared = shift: every code comes back as itself, -0 (code 32) included."""
    codes = torch.arange(64, dtype=torch.uint8).reshape(2, 32)              # (codes 31 and 63: both blocks hold the largest value)
    x = torch.tensor([e2m3(int(c)) for c in codes.reshape(-1)], dtype=torch.float64).reshape(1, 64) * 2.0 ** shift
    packed, scales = Q().quantize_mxfp6(x)
    assert scales.tolist() == [[shift + 127, shift + 127]]
    assert torch.equal(Q().unpack_mxfp6(packed), codes.reshape(1, 64))
    back = Q().dequantize_mxfp6(packed, scales)
    assert back.dtype == torch.float32 and torch.equal(back.double(), x)
    assert torch.equal(torch.signbit(back), torch.signbit(x))


def test_ties_go_to_even_and_saturate():
    # the block's maximum 7.0 fixes shared = 0; the rest are exact ties of the three steps and values past 7.5
    vals = [7.0, 0.0625, 0.1875, 1.0625, 1.1875, 2.125, 2.375, 4.25, 4.75, 7.25, 7.75, 7.9, -7.75, -0.0625, -0.01, 0.0626]
    want = [7.0, 0.0, 0.25, 1.0, 1.25, 2.0, 2.5, 4.0, 5.0, 7.0, 7.5, 7.5, -7.5, -0.0, -0.0, 0.125]
    x = torch.tensor(vals + [0.0] * 16, dtype=torch.float64).reshape(1, 32)
    packed, scales = Q().quantize_mxfp6(x)
    assert scales.tolist() == [[127]]
    got = Q().dequantize_mxfp6(packed, scales)[0, :16].tolist()
    assert got == want
    codes = Q().unpack_mxfp6(packed)[0]
    assert codes[13] == 32 and codes[14] == 32                               # a negative value that rounds to zero keeps its sign
    assert codes[10] == 31 and codes[12] == 63


def test_zero_block_and_clamping_at_both_ends_of_e8m0():
    x = torch.zeros(1, 96, dtype=torch.float64)
    x[0, 32] = 2.0 ** -140                                                   # shared would be -142: clamped to -127
    x[0, 33] = -(2.0 ** -127)
    x[0, 64] = 1.5 * 2.0 ** 1000                                             # (float64 only) shared would be 998: clamped to 127
    packed, scales = Q().quantize_mxfp6(x)
    assert scales.tolist() == [[127, 0, 254]]
    codes = Q().unpack_mxfp6(packed)[0]
    assert not codes[:32].any()
    assert codes[32] == 0 and codes[33] == 32 + 8                            # 2^-140 / 2^-127 rounds to 0; -2^-127 is -1.0
    assert codes[64] == 31                                                   # saturated
    f = torch.zeros(1, 32)
    f[0, 0] = torch.finfo(torch.float32).max                                 # the largest float32: exponent 127, shared 125
    assert Q().quantize_mxfp6(f)[1].tolist() == [[252]]


def test_non_finite_input_raises_and_shapes_are_checked():
    for bad in (float("inf"), float("-inf"), NAN):
        x = torch.zeros(2, 32)
        x[1, 7] = bad
        with pytest.raises(ValueError, match="finite"):
            Q().quantize_mxfp6(x)
    with pytest.raises(ValueError):
        Q().quantize_mxfp6(torch.zeros(2, 48))
    with pytest.raises(ValueError):
        Q().dequantize_mxfp6(torch.zeros(2, 24, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))
    c, s = Q().quantize_mxfp6(torch.randn(3, 5, 64))
    assert c.shape == (3, 5, 48) and s.shape == (3, 5, 2)


def test_format_error_of_gaussian_rows():
    """The figure the mode is built on: e2m3 rows with E8M0 block scales lose about 2.8e-2 of Gaussian rows."""
    x = torch.randn(64, 2880, generator=torch.Generator().manual_seed(0))
    err = float((Q().dequantize_mxfp6(*Q().quantize_mxfp6(x)).double() - x.double()).norm() / x.double().norm())
    assert 2.4e-2 < err < 3.2e-2, err


# ---- the C ABI

@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _f6(lib, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P_8, xsc=P_BYTE, bias=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_fwd_f6(bl, sc, x, xsc, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _q6(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_fwd_q6(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _glu(lib, act=CLAMP, alpha=1.702, limit=7.0, di=F32, do=F32, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P,
         offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_glu_fwd_q6(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, act, alpha, limit, ws, nbytes, None)


def _qr(lib, di=F32, gated=0, act=SILU, alpha=1.702, limit=7.0, x=P, ob=P2, osc=P_BYTE, T=8, K=64):
    return lib.fql_mx6_quantize_rows(x, di, gated, act, alpha, limit, ob, osc, T, K, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    with open(os.path.join(ROOT, "include", "fql_int4_tune.h")) as f:
        tune = f.read()
    for name in HOOKS:
        assert name + "(" in tune and hasattr(raw, name) and name in _native.exported_symbols(), name
    assert lib.fql_version() >= 400


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    '#include "fql_int4_tune.h"\n'
                    "size_t (*w)(int, int, int, int, int) = fql_moe_mx4_f6_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const uint8_t *, const uint8_t *, const uint8_t *, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_mx4_fwd_f6;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_mx4_fwd_q6;\n"
                    "int (*c)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, float, float, void *, size_t, void *)\n"
                    "    = fql_moe_mx4_glu_fwd_q6;\n"
                    "int (*d)(const void *, int, int, int, float, float, uint8_t *, uint8_t *, int, int, void *)\n"
                    "    = fql_mx6_quantize_rows;\n"
                    "int (*e)(int) = fql_tune_set_mx4_f6_decode_max_rows;\n"
                    "int (*g)(int, int, int, int) = fql_tune_mx4_f6_kernel;\n"
                    "int version_is_400[FQL_VERSION >= 400 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_workspace_query(lib):
    w = lib.fql_moe_mx4_f6_workspace_bytes
    for shape in ((3, 51, 96, 136), (1, 1, 32, 1), (4, 1024, 2880, 2880), (2, 7, 288, 40)):
        E, T, K, N = shape
        assert w(E, T, K, N, 0) == 0                                         # rows already MXFP6: nothing is staged
        for mode in (1, 2):                                                  # the codes [T][3K/4], then their scales [T][K/32]
            assert w(E, T, K, N, mode) == r16(T * K * 3 // 4) + r16(T * K // 32)
            assert w(E, T, K, N, mode) % 16 == 0
        assert w(E, T, K, N, 3) == 0
    assert w(3, 0, 96, 136, 1) == 0 and w(3, 51, 0, 136, 2) == 0
    assert w(1, 4194240, 4096, 1, 1) == r16(4194240 * 3072) + r16(4194240 * 128)     # past 2^32: size_t arithmetic


@pytest.mark.parametrize("call", [_f6, _q6, _glu], ids=["f6", "q6", "glu_q6"])
def test_argument_errors_in_order_with_every_pointer_null(lib, call):
    """Every pointer NULL: what comes back is decided by the integers alone, in fql_moe_mx4_fwd's order."""
    null = dict(bl=None, sc=None, x=None, bias=None, tpe=None, offs=None, out=None)
    if call is _f6:
        null["xsc"] = None
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert call(lib, **null, **kw) == SHAPE, kw
    assert call(lib, **null, K=65) == ODD_K
    assert call(lib, **null, K=65, E=0) == SHAPE                             # the dimensions before odd K
    for K in (16, 48, 80, 2):
        assert call(lib, **null, K=K) == SHAPE, K                            # K % 32: one scale per 32 inputs
    assert call(lib, **null, K=33, do=3) == ODD_K                            # odd K before the types
    assert call(lib, **null, K=48, do=3) == SHAPE                            # ... and K % 32 too
    assert call(lib, **null, do=3) == DTYPE and call(lib, **null, do=-1) == DTYPE
    if call is not _f6:
        assert call(lib, **null, di=F16) == DTYPE                            # float16 rows are refused, not rounded
        assert call(lib, **null, di=3) == DTYPE and call(lib, **null, K=33, di=F16) == ODD_K
        assert call(lib, **null, T=0, di=F16) == DTYPE                       # the types before the empty call
    assert call(lib, **null, T=0) == OK and call(lib, **null, N=0) == OK     # the empty call before the pointers
    assert call(lib, **null) == NULLP


@pytest.mark.parametrize("call", [_f6, _q6, _glu], ids=["f6", "q6", "glu_q6"])
def test_pointer_table_and_alignment_errors(lib, call):
    for kw in (dict(bl=None), dict(sc=None), dict(x=None), dict(out=None), dict(tpe=None), dict(offs=None)):
        assert call(lib, **kw) == NULLP, kw
    assert call(lib, tpe=None, offs=None) == SHAPE                           # no table: one segment, E == 1 only
    assert call(lib, E=65535) == SHAPE and call(lib, T=4194241) == SHAPE
    assert call(lib, bl=P_WORD) == ALIGN                                     # blocks: 16 bytes
    assert call(lib, do=F16, out=P_BYTE) == ALIGN and call(lib, do=F32, out=P_HALF) == ALIGN
    assert call(lib, bias=P_HALF) == ALIGN
    if call is _f6:
        assert call(lib, xsc=None) == NULLP                                  # the rows' scales are an operand
        assert call(lib, xsc=None, tpe=None, offs=None) == NULLP             # ... checked with the pointers, before the table
        assert call(lib, x=P_WORD) == ALIGN and call(lib, x=P_BYTE) == ALIGN # in_codes: 8 bytes (in_scales_e8m0: none,
        assert call(lib, x=P_WORD, xsc=P_BYTE) == ALIGN                      # the default above is an odd address)
    else:
        assert call(lib, di=BF16, x=P_BYTE) == ALIGN and call(lib, di=F32, x=P_HALF) == ALIGN
        need = r16(8 * 64 * 3 // 4) + r16(8 * 64 // 32)
        assert call(lib) == WS                                               # everything else is fine: the workspace is last
        assert call(lib, ws=ctypes.c_void_p(24), nbytes=1 << 20) == WS       # misaligned
        assert call(lib, ws=P, nbytes=need - 16) == WS                       # short
        assert call(lib, bias=None) == WS and call(lib, tpe=None, offs=None, E=1) == WS      # both optional


def test_gated_activation_errors(lib):
    assert _glu(lib, act=3) == SHAPE and _glu(lib, act=-1) == SHAPE
    for kw in (dict(alpha=NAN), dict(limit=NAN), dict(limit=0.0), dict(limit=-1.0), dict(alpha=float("inf"))):
        assert _glu(lib, act=CLAMP, **kw) == SHAPE, kw
        assert _glu(lib, act=GELU, **kw) == SHAPE, kw
        assert _glu(lib, act=SILU, T=0, **kw) == OK, kw                      # silu ignores its two floats
        assert _qr(lib, gated=1, act=CLAMP, **kw) == SHAPE, kw
        assert _qr(lib, gated=0, act=CLAMP, T=0, **kw) == OK, kw             # not gated: the activation is not looked at
    assert _glu(lib, act=3, K=65) == SHAPE                                   # the activation before odd K
    assert _qr(lib, gated=1, act=3) == SHAPE and _qr(lib, gated=0, act=3, T=0) == OK


def test_quantize_rows_errors_in_order(lib):
    null = dict(x=None, ob=None, osc=None)
    for kw in (dict(T=-1), dict(K=0), dict(K=-32)):
        assert _qr(lib, **null, **kw) == SHAPE, kw
    assert _qr(lib, **null, K=65) == ODD_K and _qr(lib, **null, K=48) == SHAPE
    assert _qr(lib, **null, di=F16) == DTYPE and _qr(lib, **null, di=3) == DTYPE
    assert _qr(lib, **null, K=33, di=F16) == ODD_K and _qr(lib, **null, T=0, di=F16) == DTYPE
    assert _qr(lib, **null, T=0) == OK
    assert _qr(lib, **null) == NULLP
    for kw in (dict(x=None), dict(ob=None), dict(osc=None)):
        assert _qr(lib, **kw) == NULLP, kw
    assert _qr(lib, T=4194241) == SHAPE
    assert _qr(lib, ob=P_WORD) == ALIGN and _qr(lib, ob=P_8) == ALIGN        # out_codes: 16 bytes
    assert _qr(lib, di=F32, x=P_HALF) == ALIGN and _qr(lib, di=BF16, x=P_BYTE) == ALIGN


# ---- the tuning hooks

@pytest.fixture()
def threshold(lib):
    setter = lib.fql_tune_set_mx4_f6_decode_max_rows
    default = setter(-1)                                                     # (a negative value changes nothing)
    yield setter
    setter(default)


def test_hooks_set_report_and_refuse_a_negative_value(lib, threshold):
    k = lib.fql_tune_mx4_f6_kernel
    default = threshold(-1)
    assert default >= 0 and threshold(-1) == default and threshold(-7) == default
    assert threshold(5) == default and threshold(-1) == 5
    assert [k(32, T, 2880, 5760) for T in (1, 5, 6, 1024)] == [1, 1, 0, 0]
    assert k(1, 5, 32, 1) == 1 and k(1, 6, 32, 1) == 0                       # a function of T alone
    assert threshold(0) == 5 and [k(32, T, 2880, 5760) for T in (0, 1, 4)] == [0, 0, 0]
    assert threshold(INT_MAX) == 0 and k(32, 1024, 2880, 5760) == 1 and k(32, 0, 2880, 5760) == 0
    assert k(1, 32 * 65535, 32, 1) == 1 and k(1, 32 * 65535 + 1, 32, 1) == 0         # (the decode kernel's grid)
    assert threshold(-1) == INT_MAX


def test_threshold_is_its_own_and_mode_3_of_the_scaled_pair_is_still_unknown(lib, threshold):
    scaled, bf = lib.fql_tune_set_mx4_scaled_decode_max_rows, lib.fql_tune_set_mx4_decode_max_rows
    before = (scaled(1, -1), scaled(2, -1), bf(-1))
    threshold(77)
    assert (scaled(1, -1), scaled(2, -1), bf(-1)) == before
    assert scaled(3, 5) == -1 and scaled(3, -1) == -1
    assert lib.fql_tune_mx4_scaled_kernel(3, 32, 4, 2880, 5760) == -1
    assert threshold(-1) == 77                                               # ... and mode 3 did not reach it


# ---- the layer and the ops

E, H, F = 3, 64, 96


def fq():
    import fused_int4_amd
    return fused_int4_amd


def test_precision_is_configuration_not_state():
    base = fq().MXFP4MoEFFN(E, H, F)
    m = fq().MXFP4MoEFFN(E, H, F, precision="fp6")
    assert base.precision == "bf16" and m.precision == "fp6"
    assert list(m.state_dict()) == list(base.state_dict())
    b = fq().MXFP4MoEFFN(E, H, F, precision="fp6", expert_bias=True, activation="swiglu_clamp")
    assert list(b.state_dict()) == list(fq().MXFP4MoEFFN(E, H, F, expert_bias=True).state_dict())
    assert "precision=fp6" in repr(m) and "fp6" not in repr(base)
    m.load_state_dict(base.state_dict())                                     # either way round
    base.load_state_dict(m.state_dict())


def test_fp6_has_no_backward_and_unknown_precisions_name_all_four():
    with pytest.raises(ValueError, match="input_grad"):
        fq().MXFP4MoEFFN(E, H, F, precision="fp6", input_grad=True)
    with pytest.raises(ValueError, match="precision") as err:
        fq().MXFP4MoEFFN(E, H, F, precision="nope")
    assert all(mode in str(err.value) for mode in ("bf16", "fp8", "fp6", "fp4"))


def test_precision_passes_through_the_constructors():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    m = fq().MXFP4MoEFFN.from_mxfp4(r(E, 2 * F, H // 2), r(E, 2 * F, H // 32), r(E, H, F // 2), r(E, H, F // 32), precision="fp6")
    assert m.precision == "fp6"
    w = lambda *s: [torch.randn(*s, generator=g) for _ in range(E)]
    assert fq().MXFP4MoEFFN.from_weights(w(F, H), w(F, H), w(H, F), precision="fp6").precision == "fp6"
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_weights(w(F, H), w(F, H), w(H, F), precision="fp6", input_grad=True)
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=m)
    assert blk.experts is m and sorted(blk.state_dict()) == sorted(
        ["gate.weight"] + ["experts." + k for k in fq().MXFP4MoEFFN(E, H, F).state_dict()])


def test_ops_refuse_cpu_tensors_float16_rows_and_unknown_precisions():
    from fused_int4_amd import ops
    blocks, scales = torch.zeros(2, 8, 32, dtype=torch.uint8), torch.full((2, 8, 2), 127, dtype=torch.uint8)
    tpe, offs = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_forward_mxfp4(blocks, scales, torch.zeros(4, 64), tpe, offs, precision="fp6")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_gated_forward_mxfp4(blocks, scales, torch.zeros(4, 128), tpe, offs, precision="fp6")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_forward_mxfp4_fp6(blocks, scales, torch.zeros(4, 48, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8),
                                  tpe, offs)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.moe_forward_mxfp4_fp6(blocks, scales, torch.zeros(4, 48), torch.zeros(4, 2, dtype=torch.uint8), tpe, offs)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.quantize_rows_mxfp6(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="float16"):
        ops.quantize_rows_mxfp6(torch.zeros(4, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="activation"):
        ops.quantize_rows_mxfp6(torch.zeros(4, 64), activation="relu")
    for call, width in ((ops.moe_forward_mxfp4, 64), (ops.moe_gated_forward_mxfp4, 128)):
        with pytest.raises(RuntimeError, match="float16"):                   # (refused on the type, before the device)
            call(blocks, scales, torch.zeros(4, width, dtype=torch.float16), tpe, offs, precision="fp6")
        with pytest.raises(ValueError, match="precision") as err:
            call(blocks, scales, torch.zeros(4, width), tpe, offs, precision="int8")
        assert all(mode in str(err.value) for mode in ("bf16", "fp8", "fp6", "fp4"))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.moe_forward_mxfp4(blocks, scales, torch.zeros(4, 64, requires_grad=True), tpe, offs, precision="fp6")
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.quantize_rows_mxfp6(torch.zeros(4, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.moe_forward_mxfp4_fp6(blocks, scales, torch.zeros(4, 48, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8),
                                  tpe, offs, bias=torch.zeros(2, 8, requires_grad=True))
