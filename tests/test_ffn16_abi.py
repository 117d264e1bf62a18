"""C ABI of the typed gated-FFN entry points (include/fql_int4.h: fql_moe_gated_fwd, fql_lora_gated_shrink,
fql_lora_gated_grad, fql_swiglu_bwd): declared, exported, and validated in the documented order before any HIP call.
Every call below is invalid or empty, so none launches (there is no GPU in the CPU test tier)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_gated_fwd", "fql_lora_gated_shrink", "fql_lora_gated_grad", "fql_swiglu_bwd")
OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
RC, CR = 0, 1
FP8 = 8
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
TYPES = [F32, F16, BF16]


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, gu=P, tpe=P, offs=P, out=P2, ws=None,
         nbytes=0):
    return lib.fql_moe_gated_fwd(pk, sc, zp, gu, di, tpe, offs, out, do, E, T, K, N, prec, ws, nbytes, None)


def _shrink(lib, dt=BF16, E=2, T=8, C=64, r=16, lay=RC, gu=P, w=P, tpe=P, offs=P, out=P):
    return lib.fql_lora_gated_shrink(gu, dt, w, lay, tpe, offs, out, E, T, C, r, 1.0, None)


def _grad(lib, dt=F16, E=2, T=8, C=64, r=16, lay=RC, gu=P, v=P, tpe=P, offs=P, d=P):
    return lib.fql_lora_gated_grad(gu, dt, v, tpe, offs, d, lay, E, T, C, r, 1.0, None)


def _swiglu(lib, dg=BF16, dd=BF16, do=BF16, T=8, F=64, gu=P, dh=P, out=P2):
    return lib.fql_swiglu_bwd(gu, dg, dh, dd, out, do, T, F, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 260


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, void *, size_t, void *) = fql_moe_gated_fwd;\n"
                    "int (*b)(const void *, int, const void *, int, void *, int, int, int, void *) = fql_swiglu_bwd;\n"
                    "int version_is_260[FQL_VERSION >= 260 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


# ---- fql_moe_gated_fwd: BAD_PRECISION, BAD_SHAPE, ODD_K, DTYPE, the empty call, NULL_POINTER, the table, ALIGNMENT, WORKSPACE

def test_gated_fwd_order(lib):
    assert _fwd(lib, prec=5) == PREC
    assert _fwd(lib, prec=FP8) == PREC                           # no gated forward in fp8
    assert _fwd(lib, prec=FP8, di=9, T=-1) == PREC
    assert _fwd(lib, T=-1) == SHAPE
    assert _fwd(lib, E=0, di=9) == SHAPE
    assert _fwd(lib, K=0) == SHAPE
    assert _fwd(lib, K=65, di=9) == ODD_K
    assert _fwd(lib, di=9) == DTYPE
    assert _fwd(lib, do=3) == DTYPE
    assert _fwd(lib, di=-1, T=0) == DTYPE                        # before the empty-call shortcut
    assert _fwd(lib, do=3, gu=None, out=None) == DTYPE           # before the pointers
    assert _fwd(lib, T=0, pk=None, sc=None, zp=None, gu=None, out=None, tpe=None, offs=None) == OK
    assert _fwd(lib, N=0, gu=None) == OK
    for kw in ("pk", "sc", "zp", "gu", "out"):
        assert _fwd(lib, **{kw: None}) == NULLP, kw
    assert _fwd(lib, tpe=None) == NULLP
    assert _fwd(lib, offs=None) == NULLP
    assert _fwd(lib, E=2, tpe=None, offs=None) == SHAPE          # no table: one expert only
    assert _fwd(lib, E=70000) == SHAPE
    assert _fwd(lib, K=66) == ALIGN                              # MFMA path only: K % 32 == 0
    assert _fwd(lib, pk=P_ODD) == ALIGN
    assert _fwd(lib, gu=P_BYTE) == ALIGN
    assert _fwd(lib) == WS
    assert _fwd(lib, ws=ctypes.c_void_p(24), nbytes=1 << 30) == WS
    assert _fwd(lib, E=1, tpe=None, offs=None) == WS             # the dense form gets as far


@pytest.mark.parametrize("di", TYPES)
@pytest.mark.parametrize("do", TYPES)
def test_gated_fwd_every_pair_reaches_the_workspace_check(lib, di, do):
    assert _fwd(lib, di=di, do=do) == WS
    assert _fwd(lib, di=di, do=do, prec=FP8) == PREC
    assert _fwd(lib, di=di, do=do, K=65) == ODD_K


# ---- gated shrink / grad: BAD_SHAPE, DTYPE, the empty call, NULL_POINTER, ALIGNMENT

@pytest.mark.parametrize("call", [_shrink, _grad])
def test_gated_adapter_order(lib, call):
    assert call(lib, r=12) == SHAPE
    assert call(lib, lay=2) == SHAPE
    assert call(lib, T=-1) == SHAPE
    assert call(lib, E=70000) == SHAPE
    assert call(lib, T=1 << 19, C=1 << 11) == SHAPE             # 2 T C = 2^31: the gated operand's own limit
    assert call(lib, r=12, dt=7, tpe=None) == SHAPE
    for bad in (3, -1, 8):
        assert call(lib, dt=bad) == DTYPE
        assert call(lib, dt=bad, T=0) == DTYPE                   # before the empty-call shortcut
        assert call(lib, dt=bad, gu=None) == DTYPE               # before the pointers
    for dt in TYPES:
        assert call(lib, dt=dt, T=0, gu=None, tpe=None, offs=None) == OK
        assert call(lib, dt=dt, gu=None) == NULLP
        assert call(lib, dt=dt, tpe=None) == NULLP
        assert call(lib, dt=dt, offs=None) == NULLP
        assert call(lib, dt=dt, E=2, tpe=None, offs=None) == NULLP   # E / table mismatch


@pytest.mark.parametrize("dt", TYPES)
def test_gated_adapter_pointers_and_alignment(lib, dt):
    for kw in ("gu", "w", "out"):
        assert _shrink(lib, dt=dt, **{kw: None}) == NULLP, kw
    for kw in ("gu", "v", "d"):
        assert _grad(lib, dt=dt, **{kw: None}) == NULLP, kw
    assert _shrink(lib, dt=dt, w=P_ODD) == ALIGN
    assert _grad(lib, dt=dt, v=P_ODD) == ALIGN
    assert _grad(lib, dt=dt, d=P_ODD) == ALIGN
    assert _shrink(lib, dt=dt, w=P_ODD, gu=None) == NULLP        # pointers before alignment
    assert _grad(lib, dt=dt, C=0, gu=None, v=None, d=None) == OK
    assert _grad(lib, dt=dt, E=0, gu=None, v=None, d=None, tpe=None, offs=None) == OK
    if dt != F32:
        assert _shrink(lib, dt=dt, gu=P_BYTE) == ALIGN
        assert _grad(lib, dt=dt, gu=P_BYTE) == ALIGN


# ---- fql_swiglu_bwd: BAD_SHAPE, DTYPE, the empty call, NULL_POINTER, in place, ALIGNMENT

def test_swiglu_bwd_order(lib):
    assert _swiglu(lib, T=-1) == SHAPE
    assert _swiglu(lib, F=-1, dg=9) == SHAPE
    assert _swiglu(lib, T=1 << 20, F=1 << 10) == SHAPE
    for kw in ("dg", "dd", "do"):
        assert _swiglu(lib, **{kw: 5}) == DTYPE, kw
        assert _swiglu(lib, T=0, **{kw: -1}) == DTYPE, kw        # before the empty-call shortcut
        assert _swiglu(lib, gu=None, **{kw: 3}) == DTYPE, kw     # before the pointers
    assert _swiglu(lib, gu=P_BYTE) == ALIGN
    assert _swiglu(lib, dh=P_BYTE) == ALIGN
    assert _swiglu(lib, out=P_BYTE) == ALIGN


@pytest.mark.parametrize("dg", TYPES)
@pytest.mark.parametrize("dd", TYPES)
@pytest.mark.parametrize("do", TYPES)
def test_swiglu_bwd_every_triple(lib, dg, dd, do):
    assert _swiglu(lib, dg, dd, do, T=0, gu=None, dh=None, out=None) == OK
    assert _swiglu(lib, dg, dd, do, F=0, gu=None, dh=None, out=None) == OK
    for kw in ("gu", "dh", "out"):
        assert _swiglu(lib, dg, dd, do, **{kw: None}) == NULLP, kw
    assert _swiglu(lib, dg, dd, do, gu=P, out=P) == SHAPE        # not in place
