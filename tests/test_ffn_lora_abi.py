"""C ABI of the gated-FFN adapter entry points (include/fql_int4.h: fql_lora_gated_shrink_f32, fql_lora_gated_grad_f32,
fql_swiglu_bwd_f32): declared, exported, validated before any HIP call.  No compute call is made here (there is no GPU
in the CPU test tier)."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_lora_gated_shrink_f32", "fql_lora_gated_grad_f32", "fql_swiglu_bwd_f32")
OK, NULLP, SHAPE, ALIGN = 0, -1, -2, -7
RC, CR = 0, 1
P = ctypes.c_void_p(16)        # never dereferenced: every call below fails validation (or is empty) before a launch
P2 = ctypes.c_void_p(32)
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _shrink(lib, E=2, T=8, C=64, r=16, lay=RC, x=P, w=P, tpe=P, offs=P, out=P):
    return lib.fql_lora_gated_shrink_f32(x, w, lay, tpe, offs, out, E, T, C, r, 1.0, None)


def _grad(lib, E=2, T=8, C=64, r=16, lay=RC, p=P, v=P, tpe=P, offs=P, d=P):
    return lib.fql_lora_gated_grad_f32(p, v, tpe, offs, d, lay, E, T, C, r, 1.0, None)


def _swiglu(lib, T=8, F=64, gu=P, dh=P, out=P2):
    return lib.fql_swiglu_bwd_f32(gu, dh, out, T, F, None)


CALLS = (_shrink, _grad)


def test_declared_and_exported(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 240


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("r", [0, 1, 12, 24, 128, -16])
def test_bad_rank(lib, call, r):
    assert call(lib, r=r) == SHAPE


@pytest.mark.parametrize("call", CALLS)
def test_bad_layout(lib, call):
    assert call(lib, lay=2) == SHAPE
    assert call(lib, lay=-1) == SHAPE


@pytest.mark.parametrize("call", CALLS)
def test_bad_sizes(lib, call):
    assert call(lib, E=-1) == SHAPE
    assert call(lib, T=-1) == SHAPE
    assert call(lib, C=-4) == SHAPE
    assert call(lib, E=70000) == SHAPE
    assert call(lib, T=1 << 20, C=1 << 12) == SHAPE            # T * C = 2^32: past 31 bits
    assert call(lib, T=1 << 19, C=1 << 11) == SHAPE            # T * C = 2^30 fits, the [T][2C] operand (2^31) does not
    first = "x" if call is _shrink else "p"
    assert call(lib, T=1 << 19, C=1 << 10, **{first: None}) == NULLP      # 2 T C = 2^30 passes the size check
    assert call(lib, E=1024, C=1 << 16, r=64) == SHAPE         # E * C * r past 31 bits


@pytest.mark.parametrize("call", CALLS)
def test_rank_is_checked_before_pointers(lib, call):
    assert call(lib, r=12, tpe=None, offs=None) == SHAPE


def test_null_pointers(lib):
    for kw in ("x", "w", "out"):
        assert _shrink(lib, **{kw: None}) == NULLP, kw
    for kw in ("p", "v", "d"):
        assert _grad(lib, **{kw: None}) == NULLP, kw
    for call in CALLS:
        assert call(lib, tpe=None) == NULLP                   # one table pointer without the other
        assert call(lib, offs=None) == NULLP
        assert call(lib, E=2, tpe=None, offs=None) == NULLP   # no table needs E == 1


def test_alignment(lib):
    assert _shrink(lib, w=P_ODD) == ALIGN
    assert _grad(lib, v=P_ODD) == ALIGN
    assert _grad(lib, d=P_ODD) == ALIGN


def test_empty_is_a_no_op(lib):
    assert _shrink(lib, T=0, tpe=None, offs=None, x=None, w=None, out=None) == OK
    assert _grad(lib, T=0, tpe=None, offs=None, p=None, v=None, d=None) == OK
    assert _grad(lib, C=0, p=None, v=None, d=None) == OK
    assert _grad(lib, E=0, p=None, v=None, d=None, tpe=None, offs=None) == OK


def test_swiglu_bwd_validation(lib):
    assert _swiglu(lib, T=-1) == SHAPE
    assert _swiglu(lib, F=-1) == SHAPE
    assert _swiglu(lib, T=1 << 19, F=1 << 11) == SHAPE          # 2 * T * F = 2^31: past 31 bits
    assert _swiglu(lib, T=-1, gu=None, dh=None, out=None) == SHAPE      # shape checks come first
    for kw in ("gu", "dh", "out"):
        assert _swiglu(lib, **{kw: None}) == NULLP, kw
    assert _swiglu(lib, out=P) == SHAPE                         # dgate_up == gate_up: not in place
    assert _swiglu(lib, T=0, gu=None, dh=None, out=None) == OK
    assert _swiglu(lib, F=0, gu=None, dh=None, out=None) == OK
