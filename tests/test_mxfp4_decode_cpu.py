"""The decode kernel of the bfloat16 MXFP4 forward (FQL_VERSION 380), the part that needs no GPU: the two tuning hooks
are declared in include/fql_int4_tune.h and exported, the choice between the two kernels is a function of T alone, and the
entries' return codes do not depend on it (every call below is invalid or empty: none launches)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HOOKS = ("fql_tune_set_mx4_decode_max_rows", "fql_tune_mx4_kernel")
INT_MAX = 2 ** 31 - 1
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def threshold(lib):
    """Sets the threshold for a test; the value the library was built with comes back afterwards."""
    default = lib.fql_tune_set_mx4_decode_max_rows(-1)         # (a negative value changes nothing)
    try:
        yield lib.fql_tune_set_mx4_decode_max_rows
    finally:
        lib.fql_tune_set_mx4_decode_max_rows(default)
    assert lib.fql_tune_set_mx4_decode_max_rows(-1) == default


def test_hooks_are_declared_in_the_tuning_header_and_exported(lib):
    from fused_int4_amd import _native
    txt = open(os.path.join(ROOT, "include", "fql_int4_tune.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    boundary = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fql_int4.h")).read(), flags=re.S)
    raw = ctypes.CDLL(lib._name)
    for name in HOOKS:
        assert re.search(r"FQL_API\s+int\s+" + name + r"\s*\(", txt), name
        assert name not in boundary, name                      # tools and tests only: not part of the drop-in boundary
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 380


def test_setter_returns_the_previous_value_and_round_trips(lib, threshold):
    default = threshold(17)
    assert 0 <= default
    assert threshold(64) == 17
    assert threshold(0) == 64
    assert threshold(INT_MAX) == 0
    assert threshold(-5) == INT_MAX and threshold(-1) == INT_MAX   # refused, nothing changed
    assert threshold(default) == INT_MAX
    assert threshold(default) == default


def test_choice_is_a_function_of_t_alone(lib, threshold):
    k = lib.fql_tune_mx4_kernel
    threshold(0)
    for T in (0, 1, 4, 32, 33, 128, 4096, 4194240, INT_MAX):
        assert k(32, T, 2880, 5760) == 0, T                     # threshold 0: always the tile kernel
    threshold(64)
    assert k(32, 64, 2880, 5760) == 1 and k(32, 65, 2880, 5760) == 0
    assert k(32, 1, 2880, 5760) == 1 and k(32, 0, 2880, 5760) == 0
    for E, K, N in ((1, 32, 8), (128, 288, 136), (65534, 2880, 1)):
        assert k(E, 64, K, N) == 1 and k(E, 65, K, N) == 0       # ... of T alone
    threshold(INT_MAX)
    assert k(32, 65, 2880, 5760) == 1
    assert k(32, 32 * 65535, 2880, 5760) == 1                    # the last T whose row blocks fit the grid's y
    assert k(32, 32 * 65535 + 1, 2880, 5760) == 0
    assert k(32, 4194240, 2880, 5760) == 0                       # (the largest T the entries accept)
    assert k(32, 0, 2880, 5760) == 0


def _fwd(lib, **kw):
    a = dict(di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P, offs=P, out=P2)
    a.update(kw)
    return lib.fql_moe_mx4_fwd(a["bl"], a["sc"], a["x"], a["di"], a["bias"], a["tpe"], a["offs"], a["out"], a["do"], a["E"],
                               a["T"], a["K"], a["N"], None, 0, None)


def _glu(lib, **kw):
    a = dict(di=F32, do=F32, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P, offs=P, out=P2, act=2, alpha=1.702, limit=7.0)
    a.update(kw)
    return lib.fql_moe_mx4_glu_fwd(a["bl"], a["sc"], a["x"], a["di"], a["bias"], a["tpe"], a["offs"], a["out"], a["do"], a["E"],
                                   a["T"], a["K"], a["N"], a["act"], a["alpha"], a["limit"], None, 0, None)


NONE = dict(bl=None, sc=None, x=None, bias=None, tpe=None, offs=None, out=None)


@pytest.mark.parametrize("rows", [0, INT_MAX], ids=["tile", "decode"])
@pytest.mark.parametrize("call", [_fwd, _glu], ids=["fwd", "glu"])
def test_return_codes_do_not_depend_on_the_threshold(lib, threshold, call, rows):
    """The codes tests/test_mxfp4_cpu.py pins, with every pointer NULL and at both ends of the threshold."""
    threshold(rows)
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert call(lib, **NONE, **kw) == SHAPE, kw
    assert call(lib, **NONE, K=65) == ODD_K
    assert call(lib, **NONE, K=65, E=0) == SHAPE
    for K in (16, 48, 80, 2):
        assert call(lib, **NONE, K=K) == SHAPE, K
    assert call(lib, **NONE, K=33, di=F16) == ODD_K
    assert call(lib, **NONE, di=F16) == DTYPE and call(lib, **NONE, di=3) == DTYPE and call(lib, **NONE, do=3) == DTYPE
    assert call(lib, **NONE, T=0) == OK and call(lib, **NONE, N=0) == OK
    assert call(lib, **NONE, T=0, di=F16) == DTYPE
    assert call(lib, **NONE) == NULLP
    for name in ("bl", "sc", "x", "out", "tpe", "offs"):
        assert call(lib, **{name: None}) == NULLP, name
    assert call(lib, tpe=None, offs=None) == SHAPE               # no table: E == 1 only
    assert call(lib, E=65535) == SHAPE and call(lib, T=4194241) == SHAPE
    assert call(lib, bl=ctypes.c_void_p(20)) == ALIGN and call(lib, bias=ctypes.c_void_p(18)) == ALIGN
    if call is _glu:
        assert call(lib, act=3) == SHAPE and call(lib, limit=0.0) == SHAPE
        assert call(lib) == WS and call(lib, bias=None) == WS    # everything else is fine: the workspace is last
