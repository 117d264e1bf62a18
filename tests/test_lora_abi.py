"""C ABI of the low-rank adapter entry points (include/fql_int4.h, fql_lora_*): declared, exported, validated before any
HIP call.  No compute call is made here (there is no GPU in the CPU test tier)."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

LORA = ("fql_lora_shrink_f32", "fql_lora_expand_f32", "fql_lora_grad_f32")
OK, NULLP, SHAPE, ALIGN = 0, -1, -2, -7
RC, CR = 0, 1
P = ctypes.c_void_p(16)        # never dereferenced: every call below fails validation (or is empty) before a launch
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _shrink(lib, E=2, T=8, C=64, r=16, lay=RC, x=P, w=P, tpe=P, offs=P, out=P):
    return lib.fql_lora_shrink_f32(x, w, lay, tpe, offs, out, E, T, C, r, 1.0, None)


def _expand(lib, E=2, T=8, C=64, r=16, lay=CR, v=P, w=P, tpe=P, offs=P, inp=P, out=P):
    return lib.fql_lora_expand_f32(v, w, lay, tpe, offs, inp, out, E, T, C, r, 1.0, None)


def _grad(lib, E=2, T=8, C=64, r=16, lay=CR, p=P, v=P, tpe=P, offs=P, d=P):
    return lib.fql_lora_grad_f32(p, v, tpe, offs, d, lay, E, T, C, r, 1.0, None)


CALLS = (_shrink, _expand, _grad)


def test_declared_and_exported(lib):
    import test_c_abi
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in LORA:
        assert name in names, name
        assert hasattr(raw, name), name
    assert lib.fql_version() >= 230


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
    assert call(lib, E=1024, C=1 << 16, r=64) == SHAPE         # E * C * r past 31 bits


@pytest.mark.parametrize("call", CALLS)
def test_rank_is_checked_before_pointers(lib, call):
    assert call(lib, r=12, tpe=None, offs=None) == SHAPE


def test_null_pointers(lib):
    for kw in ("x", "w", "out"):
        assert _shrink(lib, **{kw: None}) == NULLP, kw
    for kw in ("v", "w", "out"):
        assert _expand(lib, **{kw: None}) == NULLP, kw
    for kw in ("p", "v", "d"):
        assert _grad(lib, **{kw: None}) == NULLP, kw
    for call in CALLS:
        assert call(lib, tpe=None) == NULLP                   # one table pointer without the other
        assert call(lib, offs=None) == NULLP
        assert call(lib, E=2, tpe=None, offs=None) == NULLP   # no table needs E == 1


def test_alignment(lib):
    assert _shrink(lib, w=P_ODD) == ALIGN
    assert _expand(lib, w=P_ODD) == ALIGN
    assert _grad(lib, v=P_ODD) == ALIGN
    assert _grad(lib, d=P_ODD) == ALIGN


def test_empty_is_a_no_op(lib):
    for call in CALLS:
        assert call(lib, T=0, tpe=None, offs=None, **{k: None for k in _ptr_names(call)}) == OK
    assert _expand(lib, C=0, v=None, w=None, inp=None, out=None) == OK
    assert _grad(lib, C=0, p=None, v=None, d=None) == OK
    assert _grad(lib, E=0, p=None, v=None, d=None, tpe=None, offs=None) == OK


def _ptr_names(call):
    return {_shrink: ("x", "w", "out"), _expand: ("v", "w", "inp", "out"), _grad: ("p", "v", "d")}[call]
