"""MXFP4 expert weights over MXFP4 rows (both operands e2m1 on the block-scaled matrix cores), the part that needs no GPU:
the C ABI of FQL_VERSION 370 (fql_moe_mx4_fwd_f4 / fql_moe_mx4_fwd_q4 / fql_moe_mx4_glu_fwd_q4 / fql_mx4_quantize_rows and the
workspace query: declared, exported and validated in fql_moe_mx4_fwd's order before any HIP call -- every call below is
invalid, empty or stops at the workspace check, so none launches), ``precision="fp4"`` of MXFP4MoEFFN and what the ops
refuse on the host."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_mx4_f4_workspace_bytes", "fql_moe_mx4_fwd_f4", "fql_moe_mx4_fwd_q4", "fql_moe_mx4_glu_fwd_q4",
       "fql_mx4_quantize_rows")
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
SILU, GELU, CLAMP = 0, 1, 2
NAN = float("nan")
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 16


def r16(n):
    return (n + 15) // 16 * 16


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _f4(lib, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, xsc=P_BYTE, bias=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_fwd_f4(bl, sc, x, xsc, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _q4(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_fwd_q4(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _glu(lib, act=CLAMP, alpha=1.702, limit=7.0, di=F32, do=F32, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P,
         offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_glu_fwd_q4(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, act, alpha, limit, ws, nbytes, None)


def _qr(lib, di=F32, gated=0, act=SILU, alpha=1.702, limit=7.0, x=P, ob=P2, osc=P_BYTE, T=8, K=64):
    return lib.fql_mx4_quantize_rows(x, di, gated, act, alpha, limit, ob, osc, T, K, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 370


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "size_t (*w)(int, int, int, int, int) = fql_moe_mx4_f4_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const uint8_t *, const uint8_t *, const uint8_t *, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_mx4_fwd_f4;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_mx4_fwd_q4;\n"
                    "int (*c)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, float, float, void *, size_t, void *)\n"
                    "    = fql_moe_mx4_glu_fwd_q4;\n"
                    "int (*d)(const void *, int, int, int, float, float, uint8_t *, uint8_t *, int, int, void *)\n"
                    "    = fql_mx4_quantize_rows;\n"
                    "int version_is_370[FQL_VERSION >= 370 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_workspace_query(lib):
    w = lib.fql_moe_mx4_f4_workspace_bytes
    for shape in ((3, 51, 96, 136), (1, 1, 32, 1), (4, 1024, 2880, 2880), (2, 7, 288, 40)):
        E, T, K, N = shape
        assert w(E, T, K, N, 0) == 0                                         # rows already MXFP4: nothing is staged
        for mode in (1, 2):                                                  # the packed rows [T][K/2], then their scales [T][K/32]
            assert w(E, T, K, N, mode) == r16(T * K // 2) + r16(T * K // 32)
            assert w(E, T, K, N, mode) % 16 == 0
        assert w(E, T, K, N, 3) == 0
    assert w(3, 0, 96, 136, 1) == 0 and w(3, 51, 0, 136, 2) == 0


@pytest.mark.parametrize("call", [_f4, _q4, _glu], ids=["f4", "q4", "glu_q4"])
def test_argument_errors_in_order_with_every_pointer_null(lib, call):
    """Every pointer NULL: what comes back is decided by the integers alone, in fql_moe_mx4_fwd's order."""
    null = dict(bl=None, sc=None, x=None, bias=None, tpe=None, offs=None, out=None)
    if call is _f4:
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
    if call is not _f4:
        assert call(lib, **null, di=F16) == DTYPE                            # float16 rows are refused, not rounded
        assert call(lib, **null, di=3) == DTYPE and call(lib, **null, K=33, di=F16) == ODD_K
        assert call(lib, **null, T=0, di=F16) == DTYPE                       # the types before the empty call
    assert call(lib, **null, T=0) == OK and call(lib, **null, N=0) == OK     # the empty call before the pointers
    assert call(lib, **null) == NULLP


@pytest.mark.parametrize("call", [_f4, _q4, _glu], ids=["f4", "q4", "glu_q4"])
def test_pointer_table_and_alignment_errors(lib, call):
    for kw in (dict(bl=None), dict(sc=None), dict(x=None), dict(out=None), dict(tpe=None), dict(offs=None)):
        assert call(lib, **kw) == NULLP, kw
    assert call(lib, tpe=None, offs=None) == SHAPE                           # no table: one segment, E == 1 only
    assert call(lib, E=65535) == SHAPE and call(lib, T=4194241) == SHAPE
    assert call(lib, bl=P_WORD) == ALIGN                                     # blocks: 16 bytes
    assert call(lib, do=F16, out=P_BYTE) == ALIGN and call(lib, do=F32, out=P_HALF) == ALIGN
    assert call(lib, bias=P_HALF) == ALIGN
    if call is _f4:
        assert call(lib, xsc=None) == NULLP                                  # the rows' scales are an operand
        assert call(lib, xsc=None, tpe=None, offs=None) == NULLP             # ... checked with the pointers, before the table
        assert call(lib, x=P_WORD) == ALIGN and call(lib, x=P_BYTE) == ALIGN # in_blocks: 16 bytes (in_scales_e8m0: none,
        assert call(lib, x=P_WORD, xsc=P_BYTE) == ALIGN                      # the default above is an odd address)
    else:
        assert call(lib, di=BF16, x=P_BYTE) == ALIGN and call(lib, di=F32, x=P_HALF) == ALIGN
        need = r16(8 * 64 // 2) + r16(8 * 64 // 32)
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
    assert _qr(lib, ob=P_WORD) == ALIGN                                      # out_blocks: 16 bytes
    assert _qr(lib, di=F32, x=P_HALF) == ALIGN and _qr(lib, di=BF16, x=P_BYTE) == ALIGN


# ---- the layer and the ops

E, H, F = 3, 64, 96


def fq():
    import fused_int4_amd
    return fused_int4_amd


def test_precision_is_configuration_not_state():
    base = fq().MXFP4MoEFFN(E, H, F)
    m = fq().MXFP4MoEFFN(E, H, F, precision="fp4")
    assert base.precision == "bf16" and m.precision == "fp4"
    assert list(m.state_dict()) == list(base.state_dict())
    b = fq().MXFP4MoEFFN(E, H, F, precision="fp4", expert_bias=True, activation="swiglu_clamp")
    assert list(b.state_dict()) == list(fq().MXFP4MoEFFN(E, H, F, expert_bias=True).state_dict())
    assert "precision=fp4" in repr(m) and "fp4" not in repr(base).replace("mxfp4", "")
    assert "precision=fp8" in repr(fq().MXFP4MoEFFN(E, H, F, precision="fp8"))
    m.load_state_dict(base.state_dict())                                     # either way round
    base.load_state_dict(m.state_dict())


def test_fp4_has_no_backward_and_unknown_precisions_raise():
    with pytest.raises(ValueError, match="input_grad"):
        fq().MXFP4MoEFFN(E, H, F, precision="fp4", input_grad=True)
    with pytest.raises(ValueError, match="precision") as err:
        fq().MXFP4MoEFFN(E, H, F, precision="nope")
    assert all(mode in str(err.value) for mode in ("bf16", "fp8", "fp4"))
    assert fq().MXFP4MoEFFN(E, H, F, precision="bf16", input_grad=True).input_grad


def test_precision_passes_through_the_constructors():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    m = fq().MXFP4MoEFFN.from_mxfp4(r(E, 2 * F, H // 2), r(E, 2 * F, H // 32), r(E, H, F // 2), r(E, H, F // 32), precision="fp4")
    assert m.precision == "fp4"
    w = lambda *s: [torch.randn(*s, generator=g) for _ in range(E)]
    assert fq().MXFP4MoEFFN.from_weights(w(F, H), w(F, H), w(H, F), precision="fp4").precision == "fp4"
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_weights(w(F, H), w(F, H), w(H, F), precision="fp4", input_grad=True)
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=m)
    assert blk.experts is m and sorted(blk.state_dict()) == sorted(
        ["gate.weight"] + ["experts." + k for k in fq().MXFP4MoEFFN(E, H, F).state_dict()])


def test_ops_refuse_cpu_tensors_float16_rows_and_unknown_precisions():
    from fused_int4_amd import ops
    blocks, scales = torch.zeros(2, 8, 32, dtype=torch.uint8), torch.full((2, 8, 2), 127, dtype=torch.uint8)
    tpe, offs = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_forward_mxfp4(blocks, scales, torch.zeros(4, 64), tpe, offs, precision="fp4")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_gated_forward_mxfp4(blocks, scales, torch.zeros(4, 128), tpe, offs, precision="fp4")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.moe_forward_mxfp4_fp4(blocks, scales, torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8),
                                  tpe, offs)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.moe_forward_mxfp4_fp4(blocks, scales, torch.zeros(4, 32), torch.zeros(4, 2, dtype=torch.uint8), tpe, offs)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.quantize_rows_mxfp4(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="float16"):
        ops.quantize_rows_mxfp4(torch.zeros(4, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="activation"):
        ops.quantize_rows_mxfp4(torch.zeros(4, 64), activation="relu")
    for call, width in ((ops.moe_forward_mxfp4, 64), (ops.moe_gated_forward_mxfp4, 128)):
        with pytest.raises(RuntimeError, match="float16"):                   # (refused on the type, before the device)
            call(blocks, scales, torch.zeros(4, width, dtype=torch.float16), tpe, offs, precision="fp4")
        with pytest.raises(ValueError, match="precision") as err:
            call(blocks, scales, torch.zeros(4, width), tpe, offs, precision="int8")
        assert all(mode in str(err.value) for mode in ("bf16", "fp8", "fp4"))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.moe_forward_mxfp4(blocks, scales, torch.zeros(4, 64, requires_grad=True), tpe, offs, precision="fp4")
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.quantize_rows_mxfp4(torch.zeros(4, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.moe_forward_mxfp4_fp4(blocks, scales, torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8),
                                  tpe, offs, bias=torch.zeros(2, 8, requires_grad=True))
