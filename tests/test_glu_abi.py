"""C ABI of the activation kinds of the gated FFN experts (include/fql_int4.h, FQL_VERSION 300: fql_moe_glu_fwd,
fql_lora_glu_shrink, fql_lora_glu_grad, fql_glu_bwd): declared, exported, and validated in the documented order before
any HIP call.  Every call below is invalid or empty, so none launches (there is no GPU in the CPU test tier)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_glu_fwd", "fql_lora_glu_shrink", "fql_lora_glu_grad", "fql_glu_bwd")
OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
RC, CR = 0, 1
FP8 = 8
SILU, GELU, CLAMP = 0, 1, 2
KINDS = [SILU, GELU, CLAMP]
NEW_KINDS = [GELU, CLAMP]
INF, NAN = float("inf"), float("nan")
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
TYPES = [F32, F16, BF16]


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, act=GELU, alpha=1.702, limit=7.0, di=BF16, do=BF16, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, gu=P,
         tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_glu_fwd(pk, sc, zp, gu, di, tpe, offs, out, do, E, T, K, N, prec, act, alpha, limit, ws, nbytes,
                               None)


def _shrink(lib, act=GELU, alpha=1.702, limit=7.0, dt=BF16, E=2, T=8, C=64, r=16, lay=RC, gu=P, w=P, tpe=P, offs=P,
            out=P):
    return lib.fql_lora_glu_shrink(gu, dt, w, lay, tpe, offs, out, E, T, C, r, 1.0, act, alpha, limit, None)


def _grad(lib, act=GELU, alpha=1.702, limit=7.0, dt=F16, E=2, T=8, C=64, r=16, lay=RC, gu=P, v=P, tpe=P, offs=P, d=P):
    return lib.fql_lora_glu_grad(gu, dt, v, tpe, offs, d, lay, E, T, C, r, 1.0, act, alpha, limit, None)


def _bwd(lib, act=GELU, alpha=1.702, limit=7.0, dg=BF16, dd=BF16, do=BF16, T=8, F=64, gu=P, dh=P, out=P2):
    return lib.fql_glu_bwd(gu, dg, dh, dd, out, do, T, F, act, alpha, limit, None)


CALLS = [_fwd, _shrink, _grad, _bwd]


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 300
    assert (_native.ACT_SILU, _native.ACT_GELU_TANH, _native.ACT_SWIGLU_CLAMP) == (0, 1, 2)


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, int, float, float, void *, size_t,\n"
                    "         void *) = fql_moe_glu_fwd;\n"
                    "int (*b)(const void *, int, const float *, int, const int32_t *, const int32_t *, float *, int, int,\n"
                    "         int, int, float, int, float, float, void *) = fql_lora_glu_shrink;\n"
                    "int (*c)(const void *, int, const float *, const int32_t *, const int32_t *, float *, int, int, int,\n"
                    "         int, int, float, int, float, float, void *) = fql_lora_glu_grad;\n"
                    "int (*d)(const void *, int, const void *, int, void *, int, int, int, int, float, float, void *)\n"
                    "    = fql_glu_bwd;\n"
                    "int version_is_300[FQL_VERSION >= 300 ? 1 : -1];\n"
                    "int kinds[(FQL_ACT_SILU == 0 && FQL_ACT_GELU_TANH == 1 && FQL_ACT_SWIGLU_CLAMP == 2) ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


# ---- the activation arguments: FQL_ERR_BAD_SHAPE with every pointer NULL, so before any pointer is looked at

NULLS = {_fwd: dict(pk=None, sc=None, zp=None, gu=None, tpe=None, offs=None, out=None),
         _shrink: dict(gu=None, w=None, tpe=None, offs=None, out=None),
         _grad: dict(gu=None, v=None, tpe=None, offs=None, d=None),
         _bwd: dict(gu=None, dh=None, out=None)}


@pytest.mark.parametrize("call", CALLS)
def test_bad_activation_arguments(lib, call):
    nulls = NULLS[call]
    for act in (-1, 3, 7, 1 << 20):
        assert call(lib, act=act, **nulls) == SHAPE, act
    for kind in NEW_KINDS:
        for alpha in (INF, -INF, NAN):
            assert call(lib, act=kind, alpha=alpha, **nulls) == SHAPE, (kind, alpha)
        for limit in (0.0, -0.0, -1.0, INF, -INF, NAN):
            assert call(lib, act=kind, limit=limit, **nulls) == SHAPE, (kind, limit)
        assert call(lib, act=kind, alpha=-2.0, limit=1e-3, **nulls) == NULLP     # a negative alpha is allowed
    # silu ignores the two floats: the sibling's answer
    assert call(lib, act=SILU, alpha=NAN, limit=-1.0, **nulls) == NULLP


def test_bad_activation_sits_in_the_first_bad_shape_clause(lib):
    # fql_moe_glu_fwd: behind BAD_PRECISION, in front of ODD_K, DTYPE, the empty call and the pointers
    assert _fwd(lib, act=9, prec=5) == PREC
    assert _fwd(lib, act=9, prec=FP8) == PREC
    assert _fwd(lib, act=9, K=65) == SHAPE
    assert _fwd(lib, act=9, di=9) == SHAPE
    assert _fwd(lib, limit=0.0, T=0) == SHAPE
    # adapters and backward: in front of DTYPE and the empty call
    for call in (_shrink, _grad):
        assert call(lib, act=9, dt=7) == SHAPE
        assert call(lib, alpha=NAN, T=0) == SHAPE
    assert _bwd(lib, act=9, dg=7) == SHAPE
    assert _bwd(lib, limit=-1.0, T=0) == SHAPE


# ---- the siblings' rows, through the new entry points, for every kind (silu is forwarded)

@pytest.mark.parametrize("act", KINDS)
def test_glu_fwd_order(lib, act):
    f = lambda **kw: _fwd(lib, act=act, **kw)
    assert f(prec=5) == PREC
    assert f(prec=FP8) == PREC                                   # no gated forward in fp8
    assert f(prec=FP8, di=9, T=-1) == PREC
    assert f(T=-1) == SHAPE
    assert f(E=0, di=9) == SHAPE
    assert f(K=0) == SHAPE
    assert f(K=65, di=9) == ODD_K
    assert f(di=9) == DTYPE
    assert f(do=3) == DTYPE
    assert f(di=-1, T=0) == DTYPE                                # before the empty-call shortcut
    assert f(do=3, gu=None, out=None) == DTYPE                   # before the pointers
    assert f(T=0, pk=None, sc=None, zp=None, gu=None, out=None, tpe=None, offs=None) == OK
    assert f(N=0, gu=None) == OK
    for kw in ("pk", "sc", "zp", "gu", "out"):
        assert f(**{kw: None}) == NULLP, kw
    assert f(tpe=None) == NULLP
    assert f(offs=None) == NULLP
    assert f(E=2, tpe=None, offs=None) == SHAPE                  # no table: one expert only
    assert f(E=70000) == SHAPE
    assert f(K=66) == ALIGN                                      # MFMA path only: K % 32 == 0
    assert f(pk=P_ODD) == ALIGN
    assert f(gu=P_BYTE) == ALIGN
    assert f() == WS
    assert f(ws=ctypes.c_void_p(24), nbytes=1 << 30) == WS
    assert f(E=1, tpe=None, offs=None) == WS                     # the dense form gets as far
    for di in TYPES:
        for do in TYPES:
            assert f(di=di, do=do) == WS
            assert f(di=di, do=do, prec=FP8) == PREC


@pytest.mark.parametrize("act", KINDS)
@pytest.mark.parametrize("call", [_shrink, _grad])
def test_glu_adapter_order(lib, call, act):
    f = lambda **kw: call(lib, act=act, **kw)
    assert f(r=12) == SHAPE
    assert f(lay=2) == SHAPE
    assert f(T=-1) == SHAPE
    assert f(E=70000) == SHAPE
    assert f(T=1 << 19, C=1 << 11) == SHAPE                      # 2 T C = 2^31: the gated operand's own limit
    assert f(r=12, dt=7, tpe=None) == SHAPE
    for bad in (3, -1, 8):
        assert f(dt=bad) == DTYPE
        assert f(dt=bad, T=0) == DTYPE                           # before the empty-call shortcut
        assert f(dt=bad, gu=None) == DTYPE                       # before the pointers
    for dt in TYPES:
        assert f(dt=dt, T=0, gu=None, tpe=None, offs=None) == OK
        assert f(dt=dt, gu=None) == NULLP
        assert f(dt=dt, tpe=None) == NULLP
        assert f(dt=dt, offs=None) == NULLP
        assert f(dt=dt, E=2, tpe=None, offs=None) == NULLP       # E / table mismatch


@pytest.mark.parametrize("act", KINDS)
@pytest.mark.parametrize("dt", TYPES)
def test_glu_adapter_pointers_and_alignment(lib, dt, act):
    s = lambda **kw: _shrink(lib, act=act, dt=dt, **kw)
    g = lambda **kw: _grad(lib, act=act, dt=dt, **kw)
    for kw in ("gu", "w", "out"):
        assert s(**{kw: None}) == NULLP, kw
    for kw in ("gu", "v", "d"):
        assert g(**{kw: None}) == NULLP, kw
    assert s(w=P_ODD) == ALIGN
    assert g(v=P_ODD) == ALIGN
    assert g(d=P_ODD) == ALIGN
    assert s(w=P_ODD, gu=None) == NULLP                          # pointers before alignment
    assert g(C=0, gu=None, v=None, d=None) == OK
    assert g(E=0, gu=None, v=None, d=None, tpe=None, offs=None) == OK
    if dt != F32:
        assert s(gu=P_BYTE) == ALIGN
        assert g(gu=P_BYTE) == ALIGN


@pytest.mark.parametrize("act", KINDS)
def test_glu_bwd_order(lib, act):
    f = lambda **kw: _bwd(lib, act=act, **kw)
    assert f(T=-1) == SHAPE
    assert f(F=-1, dg=9) == SHAPE
    assert f(T=1 << 20, F=1 << 10) == SHAPE
    for kw in ("dg", "dd", "do"):
        assert f(**{kw: 5}) == DTYPE, kw
        assert f(T=0, **{kw: -1}) == DTYPE, kw                   # before the empty-call shortcut
        assert f(gu=None, **{kw: 3}) == DTYPE, kw                # before the pointers
    assert f(gu=P_BYTE) == ALIGN
    assert f(dh=P_BYTE) == ALIGN
    assert f(out=P_BYTE) == ALIGN
    for dg in TYPES:
        for dd in TYPES:
            for do in TYPES:
                t = dict(dg=dg, dd=dd, do=do)
                assert f(T=0, gu=None, dh=None, out=None, **t) == OK
                assert f(F=0, gu=None, dh=None, out=None, **t) == OK
                for kw in ("gu", "dh", "out"):
                    assert f(**{kw: None}, **t) == NULLP, kw
                assert f(gu=P, out=P, **t) == SHAPE              # not in place
