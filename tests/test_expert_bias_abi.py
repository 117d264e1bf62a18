"""C ABI of the per-expert biases of the grouped GEMM (include/fql_int4.h, FQL_VERSION 310: fql_moe_bias_fwd,
fql_moe_glu_bias_fwd, fql_moe_bias_grad): declared, exported, and validated in the documented order before any HIP call.
Every call below is invalid or empty, so none launches (there is no GPU in the CPU test tier)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_bias_fwd", "fql_moe_glu_bias_fwd", "fql_moe_bias_grad")
OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
FP8 = 8
SILU, GELU, CLAMP = 0, 1, 2
NAN = float("nan")
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
TYPES = [F32, F16, BF16]


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=F32, do=F32, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, x=P, tpe=P, offs=P, bias=P, out=P2, ws=None,
         nbytes=0):
    return lib.fql_moe_bias_fwd(pk, sc, zp, x, di, tpe, offs, bias, out, do, E, T, K, N, prec, ws, nbytes, None)


def _plain(lib, di=F32, do=F32, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, x=P, tpe=P, offs=P, out=P2, ws=None,
           nbytes=0):
    return lib.fql_moe_fwd(pk, sc, zp, x, di, tpe, offs, out, do, E, T, K, N, prec, ws, nbytes, None)


def _glu(lib, act=CLAMP, alpha=1.702, limit=7.0, di=BF16, do=BF16, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, gu=P,
         tpe=P, offs=P, bias=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_glu_bias_fwd(pk, sc, zp, gu, di, tpe, offs, bias, out, do, E, T, K, N, prec, act, alpha, limit, ws,
                                    nbytes, None)


def _glu_plain(lib, act=CLAMP, alpha=1.702, limit=7.0, di=BF16, do=BF16, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P,
               gu=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_glu_fwd(pk, sc, zp, gu, di, tpe, offs, out, do, E, T, K, N, prec, act, alpha, limit, ws, nbytes, None)


def _grad(lib, dt=F32, E=2, T=8, N=96, g=P, tpe=P, offs=P, out=P2):
    return lib.fql_moe_bias_grad(g, dt, tpe, offs, out, E, T, N, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 310


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, const float *, void *, int, int, int, int, int, int, void *, size_t, void *)\n"
                    "    = fql_moe_bias_fwd;\n"
                    "int (*b)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, const float *, void *, int, int, int, int, int, int, int, float, float,\n"
                    "         void *, size_t, void *) = fql_moe_glu_bias_fwd;\n"
                    "int (*c)(const void *, int, const int32_t *, const int32_t *, float *, int, int, int, void *)\n"
                    "    = fql_moe_bias_grad;\n"
                    "int version_is_310[FQL_VERSION >= 310 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


# ---- fql_moe_bias_fwd: the rows of fql_moe_fwd, with and without the bias

ROWS = [dict(prec=5), dict(T=-1), dict(K=65), dict(T=0), dict(N=0), dict(out=None), dict(pk=None), dict(x=None),
        dict(tpe=None), dict(offs=None), dict(E=70000), dict(),                            # () gets to the workspace check
        dict(ws=ctypes.c_void_p(24), nbytes=1 << 30)]


@pytest.mark.parametrize("di,do", [(F32, F32), (F16, F16), (BF16, F32), (F32, BF16)])
def test_bias_fwd_answers_as_moe_fwd(lib, di, do):
    for kw in ROWS:
        want = _plain(lib, di=di, do=do, **kw)
        assert _fwd(lib, di=di, do=do, bias=None, **kw) == want, kw          # NULL bias: the call IS fql_moe_fwd
        assert _fwd(lib, di=di, do=do, **kw) == want, kw                     # with a bias: the same checks, the same order
    assert _fwd(lib, di=di, do=do) == WS
    assert _fwd(lib, di=9, do=do) == _plain(lib, di=9, do=do) == DTYPE


def test_bias_fwd_empty_contraction(lib):
    # E == 0 or K == 0: the float32 call writes zeros; with a bias there is nothing worth a kernel (as fql_linear_bias_fwd_f32)
    assert _fwd(lib, K=0) == SHAPE
    assert _fwd(lib, E=0) == SHAPE
    assert _fwd(lib, K=0, T=0) == OK                                         # the empty call comes first
    for di, do in ((F16, F16), (BF16, F32)):
        assert _fwd(lib, di=di, do=do, K=0) == SHAPE
        assert _fwd(lib, di=di, do=do, E=0) == SHAPE


def test_bias_fwd_16bit_off_the_mfma_path(lib):
    assert _fwd(lib, di=F16, do=F16, K=34) == DTYPE                          # K % 32 != 0: no 16-bit I/O there
    assert _fwd(lib, di=BF16, do=F32, pk=P_ODD) == DTYPE
    assert _plain(lib, di=F16, do=F16, K=34) == DTYPE


# ---- fql_moe_glu_bias_fwd: the rows of fql_moe_glu_fwd for every kind

@pytest.mark.parametrize("act", [SILU, GELU, CLAMP])
def test_glu_bias_fwd_order(lib, act):
    f = lambda **kw: _glu(lib, act=act, **kw)
    assert f(prec=5) == PREC
    assert f(prec=FP8) == PREC
    assert f(T=-1) == SHAPE
    assert f(E=0, di=9) == SHAPE
    assert f(K=0) == SHAPE
    assert f(K=65, di=9) == ODD_K
    assert f(di=9) == DTYPE
    assert f(do=3) == DTYPE
    assert f(di=-1, T=0) == DTYPE
    assert f(T=0, pk=None, sc=None, zp=None, gu=None, out=None, tpe=None, offs=None) == OK
    assert f(N=0, gu=None) == OK
    for kw in ("pk", "sc", "zp", "gu", "out"):
        assert f(**{kw: None}) == NULLP, kw
    assert f(tpe=None) == NULLP
    assert f(offs=None) == NULLP
    assert f(E=2, tpe=None, offs=None) == SHAPE
    assert f(E=70000) == SHAPE
    assert f(K=66) == ALIGN
    assert f(pk=P_ODD) == ALIGN
    assert f(gu=P_BYTE) == ALIGN
    assert f() == WS
    assert f(E=1, tpe=None, offs=None) == WS                                 # the dense form gets as far
    for di in TYPES:
        for do in TYPES:
            assert f(di=di, do=do) == WS
    # NULL bias: the call IS fql_moe_glu_fwd
    for kw in (dict(prec=5), dict(T=-1), dict(K=65), dict(di=9), dict(T=0), dict(gu=None), dict(tpe=None), dict(K=66), dict()):
        assert f(bias=None, **kw) == _glu_plain(lib, act=act, **kw), kw


def test_glu_bias_fwd_activation_arguments(lib):
    nulls = dict(pk=None, sc=None, zp=None, gu=None, tpe=None, offs=None, out=None)
    for act in (-1, 3, 7):
        assert _glu(lib, act=act, **nulls) == SHAPE
    for kind in (GELU, CLAMP):
        assert _glu(lib, act=kind, alpha=NAN, **nulls) == SHAPE
        assert _glu(lib, act=kind, limit=0.0, **nulls) == SHAPE
        assert _glu(lib, act=kind, limit=-1.0, T=0, **nulls) == SHAPE
    assert _glu(lib, act=SILU, alpha=NAN, limit=-1.0, **nulls) == NULLP      # silu ignores the two floats


# ---- fql_moe_bias_grad

def test_bias_grad_order(lib):
    f = lambda **kw: _grad(lib, **kw)
    assert f(E=-1) == SHAPE
    assert f(T=-1, dt=9) == SHAPE
    assert f(N=-1) == SHAPE
    assert f(E=70000) == SHAPE
    assert f(N=(1 << 31) - 1) == SHAPE
    for bad in (3, -1, 8):
        assert f(dt=bad) == DTYPE
        assert f(dt=bad, E=0) == DTYPE                                       # before the empty-call shortcut
        assert f(dt=bad, g=None, out=None) == DTYPE                          # before the pointers
    for dt in TYPES:
        assert f(dt=dt, E=0, g=None, out=None, tpe=None, offs=None) == OK
        assert f(dt=dt, N=0, g=None, out=None) == OK
        assert f(dt=dt, out=None) == NULLP
        assert f(dt=dt, g=None) == NULLP
        assert f(dt=dt, tpe=None) == NULLP
        assert f(dt=dt, offs=None) == NULLP
        assert f(dt=dt, E=2, tpe=None, offs=None) == SHAPE                   # no table: one expert only
        assert f(dt=dt, out=P_HALF) == ALIGN
        assert f(dt=dt, g=P_BYTE) == ALIGN
        assert f(dt=dt, g=P_BYTE, out=None) == NULLP                         # pointers before alignment
    assert f(dt=F32, g=P_HALF) == ALIGN
