"""C ABI of the typed (float32 / float16 / bfloat16) adapter and input-gradient entry points (include/fql_int4.h:
fql_lora_shrink / _expand / _grad, fql_linear_bwd_input / fql_moe_bwd_input): declared, exported, and validated in the
documented order before any HIP call.  Every call below is invalid or empty, so none launches (there is no GPU in the
CPU test tier)."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_lora_shrink", "fql_lora_expand", "fql_lora_grad", "fql_linear_bwd_input", "fql_moe_bwd_input")
OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
RC, CR = 0, 1
MAX_N = 132104
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_ODD = ctypes.c_void_p(20)    # 4-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _shrink(lib, dt=BF16, E=2, T=8, C=64, r=16, lay=RC, x=P, w=P, tpe=P, offs=P, out=P):
    return lib.fql_lora_shrink(x, dt, w, lay, tpe, offs, out, E, T, C, r, 1.0, None)


def _expand(lib, di=F32, do=BF16, E=2, T=8, C=64, r=16, lay=CR, v=P, w=P, tpe=P, offs=P, inp=P, out=P2):
    return lib.fql_lora_expand(v, w, lay, tpe, offs, inp, di, out, do, E, T, C, r, 1.0, None)


def _grad(lib, dt=F16, E=2, T=8, C=64, r=16, lay=CR, p=P, v=P, tpe=P, offs=P, d=P):
    return lib.fql_lora_grad(p, dt, v, tpe, offs, d, lay, E, T, C, r, 1.0, None)


def _lin(lib, di=BF16, do=BF16, B=4, K=64, N=96, prec=0, go=P, pk=P, sc=P, zp=P, gi=P, ws=None, nbytes=0):
    return lib.fql_linear_bwd_input(go, di, pk, sc, zp, gi, do, B, K, N, prec, ws, nbytes, None)


def _moe(lib, di=F16, do=F32, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, go=P, tpe=P, offs=P, gi=P, ws=None,
         nbytes=0):
    return lib.fql_moe_bwd_input(pk, sc, zp, go, di, tpe, offs, gi, do, E, T, K, N, prec, ws, nbytes, None)


LORA_CALLS = (_shrink, _expand, _grad)


def test_declared_and_exported(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 250


# ---- adapters: BAD_SHAPE, then DTYPE, then the empty call, NULL_POINTER, ALIGNMENT

@pytest.mark.parametrize("call", LORA_CALLS)
def test_lora_shape_errors_come_first(lib, call):
    assert call(lib, r=12) == SHAPE
    assert call(lib, lay=2) == SHAPE
    assert call(lib, T=-1) == SHAPE
    assert call(lib, E=70000) == SHAPE
    assert call(lib, T=1 << 20, C=1 << 12) == SHAPE
    # ... before the element type and before the pointers
    kw = {"do": 7} if call is _expand else {"dt": 7}
    assert call(lib, r=12, tpe=None, offs=None, **kw) == SHAPE


@pytest.mark.parametrize("bad", [3, -1, 8, 100])
def test_lora_unknown_dtype(lib, bad):
    assert _shrink(lib, dt=bad) == DTYPE
    assert _grad(lib, dt=bad) == DTYPE
    assert _expand(lib, do=bad) == DTYPE
    assert _expand(lib, di=bad) == DTYPE
    assert _expand(lib, di=bad, inp=None, w=None) == NULLP     # in_dtype is ignored without an `in`
    # the element type is checked before the empty-call shortcut and before the pointers
    assert _shrink(lib, dt=bad, T=0) == DTYPE
    assert _grad(lib, dt=bad, p=None) == DTYPE
    assert _expand(lib, do=bad, v=None) == DTYPE


def test_expand_in_place_needs_one_dtype(lib):
    assert _expand(lib, di=F32, do=BF16, inp=P, out=P) == DTYPE
    assert _expand(lib, di=F16, do=BF16, inp=P, out=P) == DTYPE
    assert _expand(lib, di=BF16, do=F32, inp=P, out=P) == DTYPE
    assert _expand(lib, di=F32, do=BF16, inp=P, out=P, T=0) == DTYPE      # before the empty-call shortcut
    assert _expand(lib, di=BF16, do=BF16, inp=P, out=P, w=None) == NULLP  # same type: allowed, goes on to the pointers
    assert _expand(lib, di=F32, do=F32, inp=P, out=P, w=None) == NULLP


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_lora_null_pointers_and_tables(lib, dt):
    for kw in ("x", "w", "out"):
        assert _shrink(lib, dt=dt, **{kw: None}) == NULLP, kw
    for kw in ("p", "v", "d"):
        assert _grad(lib, dt=dt, **{kw: None}) == NULLP, kw
    for kw in ("v", "w", "out"):
        assert _expand(lib, di=dt, do=BF16, **{kw: None}) == NULLP, kw
        assert _expand(lib, di=F16, do=dt, **{kw: None}) == NULLP, kw
    for call, kw in ((_shrink, {"dt": dt}), (_grad, {"dt": dt}), (_expand, {"di": dt})):
        assert call(lib, tpe=None, **kw) == NULLP
        assert call(lib, offs=None, **kw) == NULLP
        assert call(lib, E=2, tpe=None, offs=None, **kw) == NULLP


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_lora_alignment(lib, dt):
    assert _shrink(lib, dt=dt, w=P_ODD) == ALIGN
    assert _expand(lib, di=dt, w=P_ODD) == ALIGN
    assert _grad(lib, dt=dt, v=P_ODD) == ALIGN
    assert _grad(lib, dt=dt, d=P_ODD) == ALIGN
    assert _shrink(lib, dt=dt, w=P_ODD, x=None) == NULLP        # pointers before alignment


def test_16bit_operand_must_be_element_aligned(lib):
    for dt in (F16, BF16):
        assert _shrink(lib, dt=dt, x=P_BYTE) == ALIGN
        assert _grad(lib, dt=dt, p=P_BYTE) == ALIGN
        assert _expand(lib, di=dt, do=F32, inp=P_BYTE) == ALIGN
        assert _expand(lib, di=F32, do=dt, out=P_BYTE) == ALIGN


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_lora_empty_is_a_no_op(lib, dt):
    none3 = {"tpe": None, "offs": None}
    assert _shrink(lib, dt=dt, T=0, x=None, w=None, out=None, **none3) == OK
    assert _grad(lib, dt=dt, T=0, p=None, v=None, d=None, **none3) == OK
    assert _grad(lib, dt=dt, C=0, p=None, v=None, d=None) == OK
    assert _grad(lib, dt=dt, E=0, p=None, v=None, d=None, **none3) == OK
    assert _expand(lib, di=dt, do=BF16, T=0, v=None, w=None, inp=None, out=None, **none3) == OK
    assert _expand(lib, di=F16, do=dt, C=0, v=None, w=None, inp=None, out=None) == OK


# ---- input gradients: BAD_PRECISION, BAD_SHAPE, ODD_K, then DTYPE, then the empty call, NULL_POINTER, WORKSPACE

@pytest.mark.parametrize("call", [_lin, _moe])
def test_bwd_order(lib, call):
    rows = "B" if call is _lin else "T"
    assert call(lib, prec=5) == PREC
    assert call(lib, prec=5, di=9) == PREC
    assert call(lib, **{rows: -1}) == SHAPE
    assert call(lib, N=-3, do=9) == SHAPE
    assert call(lib, K=65, di=9) == ODD_K
    assert call(lib, N=MAX_N + 1, di=9) == SHAPE
    assert call(lib, di=9) == DTYPE
    assert call(lib, do=3) == DTYPE
    assert call(lib, di=-1, **{rows: 0}) == DTYPE               # before the empty-call shortcut
    assert call(lib, do=3, go=None, gi=None) == DTYPE           # before the pointers
    for kw in ("go", "pk", "sc", "zp", "gi"):
        assert call(lib, **{kw: None}) == NULLP, kw
    assert call(lib) == WS
    assert call(lib, ws=ctypes.c_void_p(24), nbytes=1 << 30) == WS
    assert call(lib, **{rows: 0}, go=None, pk=None, sc=None, zp=None, gi=None) == OK


def test_moe_bwd_table_pointers(lib):
    assert _moe(lib, tpe=None) == NULLP
    assert _moe(lib, offs=None) == NULLP
    assert _moe(lib, E=70000) == SHAPE


@pytest.mark.parametrize("di", [F32, F16, BF16])
@pytest.mark.parametrize("do", [F32, F16, BF16])
def test_bwd_every_pair_reaches_the_workspace_check(lib, di, do):
    assert _lin(lib, di=di, do=do) == WS
    assert _moe(lib, di=di, do=do) == WS
