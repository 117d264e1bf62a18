"""The decode kernels of the fp8-row and MXFP4-row precisions of the MXFP4 experts (FQL_VERSION 390), the part that needs
no GPU: the two tuning hooks are declared in include/fql_int4_tune.h and exported, each mode has a threshold of its own that
neither the other mode's nor the bfloat16 path's setter moves, the choice between the two kernels is a function of T alone,
and the six entries' return codes do not depend on it (every call below is invalid or empty: none launches)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HOOKS = ("fql_tune_set_mx4_scaled_decode_max_rows", "fql_tune_mx4_scaled_kernel")
INT_MAX = 2 ** 31 - 1
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
FP8, FP4 = 1, 2                # the hooks' modes
MODES = [FP8, FP4]
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def threshold(lib):
    """threshold(mode, rows) sets a mode's threshold for a test; the values the library was built with, the bfloat16 path's
    included, come back afterwards."""
    setter = lib.fql_tune_set_mx4_scaled_decode_max_rows
    defaults = {m: setter(m, -1) for m in MODES}                # (a negative value changes nothing)
    bf16 = lib.fql_tune_set_mx4_decode_max_rows(-1)
    try:
        yield setter
    finally:
        for m in MODES:
            setter(m, defaults[m])
        lib.fql_tune_set_mx4_decode_max_rows(bf16)
    assert {m: setter(m, -1) for m in MODES} == defaults
    assert lib.fql_tune_set_mx4_decode_max_rows(-1) == bf16


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
    assert lib.fql_version() >= 390
    m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", boundary)
    assert m and int(m.group(1)) == lib.fql_version()


@pytest.mark.parametrize("mode", MODES, ids=["fp8", "fp4"])
def test_setter_returns_the_previous_value_and_round_trips(lib, threshold, mode):
    default = threshold(mode, 17)
    assert 0 <= default
    assert threshold(mode, 64) == 17
    assert threshold(mode, 0) == 64
    assert threshold(mode, INT_MAX) == 0
    assert threshold(mode, -5) == INT_MAX and threshold(mode, -1) == INT_MAX   # refused, nothing changed
    assert threshold(mode, default) == INT_MAX
    assert threshold(mode, default) == default


def test_modes_are_independent_of_each_other_and_of_the_bfloat16_threshold(lib, threshold):
    k, kb = lib.fql_tune_mx4_scaled_kernel, lib.fql_tune_mx4_kernel
    bf = lib.fql_tune_set_mx4_decode_max_rows
    threshold(FP8, 11)
    threshold(FP4, 23)
    bf(37)
    assert threshold(FP8, -1) == 11 and threshold(FP4, -1) == 23 and bf(-1) == 37
    for T, want in ((11, (1, 1, 1)), (12, (0, 1, 1)), (23, (0, 1, 1)), (24, (0, 0, 1)), (37, (0, 0, 1)), (38, (0, 0, 0))):
        assert (k(FP8, 32, T, 2880, 5760), k(FP4, 32, T, 2880, 5760), kb(32, T, 2880, 5760)) == want, T
    threshold(FP8, INT_MAX)                                     # one moves, the other two stay
    assert threshold(FP4, -1) == 23 and bf(-1) == 37
    threshold(FP4, 0)
    assert threshold(FP8, -1) == INT_MAX and bf(-1) == 37
    bf(0)                                                       # ... and the reverse
    assert threshold(FP8, -1) == INT_MAX and threshold(FP4, -1) == 0
    assert k(FP8, 32, 4096, 2880, 5760) == 1 and k(FP4, 32, 1, 2880, 5760) == 0 and kb(32, 1, 2880, 5760) == 0


def test_an_unknown_mode_returns_minus_one_and_changes_nothing(lib, threshold):
    threshold(FP8, 5)
    threshold(FP4, 9)
    bf16 = lib.fql_tune_set_mx4_decode_max_rows(-1)
    for mode in (0, 3, -1, 255, INT_MAX):
        assert threshold(mode, 77) == -1, mode
        assert threshold(mode, -1) == -1, mode
        assert lib.fql_tune_mx4_scaled_kernel(mode, 32, 4, 2880, 5760) == -1, mode
    assert threshold(FP8, -1) == 5 and threshold(FP4, -1) == 9
    assert lib.fql_tune_set_mx4_decode_max_rows(-1) == bf16


@pytest.mark.parametrize("mode", MODES, ids=["fp8", "fp4"])
def test_choice_is_a_function_of_t_alone(lib, threshold, mode):
    k = lambda *a: lib.fql_tune_mx4_scaled_kernel(mode, *a)
    threshold(mode, 0)
    for T in (0, 1, 4, 32, 33, 128, 4096, 4194240, INT_MAX):
        assert k(32, T, 2880, 5760) == 0, T                     # threshold 0: always the tile kernel
    threshold(mode, 64)
    assert k(32, 64, 2880, 5760) == 1 and k(32, 65, 2880, 5760) == 0
    assert k(32, 1, 2880, 5760) == 1 and k(32, 0, 2880, 5760) == 0
    for E, K, N in ((1, 32, 8), (128, 288, 136), (65534, 2880, 1)):
        assert k(E, 64, K, N) == 1 and k(E, 65, K, N) == 0       # ... of T alone
    threshold(mode, INT_MAX)
    assert k(32, 65, 2880, 5760) == 1
    assert k(32, 32 * 65535, 2880, 5760) == 1                    # the last T whose row blocks fit the grid's y
    assert k(32, 32 * 65535 + 1, 2880, 5760) == 0
    assert k(32, 4194240, 2880, 5760) == 0                       # (the largest T the entries accept)
    assert k(32, 0, 2880, 5760) == 0
    for E, K, N in ((1, 32, 8), (128, 288, 136), (65534, 2880, 1)):
        assert k(E, 32 * 65535, K, N) == 1 and k(E, 32 * 65535 + 1, K, N) == 0


# ---- the six entries: (name, mode, rows given as floats?, gated?)
ENTRIES = [("fql_moe_mx4_fwd_f8", FP8, False, False), ("fql_moe_mx4_fwd_q8", FP8, True, False),
           ("fql_moe_mx4_glu_fwd_q8", FP8, True, True), ("fql_moe_mx4_fwd_f4", FP4, False, False),
           ("fql_moe_mx4_fwd_q4", FP4, True, False), ("fql_moe_mx4_glu_fwd_q4", FP4, True, True)]
NONE = dict(bl=None, sc=None, x=None, xs=None, bias=None, tpe=None, offs=None, out=None)


def call(lib, entry, **kw):
    name, _, quantising, gated = entry
    a = dict(di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, xs=P, bias=P, tpe=P, offs=P, out=P2, act=2, alpha=1.702,
             limit=7.0, ws=None, wsb=0)
    a.update(kw)
    fn = getattr(lib, name)
    tail = (a["bias"], a["tpe"], a["offs"], a["out"], a["do"], a["E"], a["T"], a["K"], a["N"])
    if not quantising:                                             # rows as bytes + their scales (act_scale / in_scales)
        return fn(a["bl"], a["sc"], a["x"], a["xs"], *tail, a["ws"], a["wsb"], None)
    if gated:
        return fn(a["bl"], a["sc"], a["x"], a["di"], *tail, a["act"], a["alpha"], a["limit"], a["ws"], a["wsb"], None)
    return fn(a["bl"], a["sc"], a["x"], a["di"], *tail, a["ws"], a["wsb"], None)


def key(kw):
    return tuple((k, getattr(v, "value", v)) for k, v in kw.items())


def codes(lib, entry):
    """The return codes of the entry on a fixed list of invalid and empty calls; none of them reaches a launch."""
    _, mode, quantising, gated = entry
    got = []
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1), dict(K=65), dict(K=65, E=0), dict(K=16), dict(K=48),
               dict(K=80), dict(K=2), dict(K=33, di=F16), dict(di=F16), dict(di=3), dict(do=3), dict(T=0), dict(N=0),
               dict(T=0, do=3), dict(), dict(T=1), dict(T=32 * 65535), dict(T=4194240), dict(T=4194241)):
        got.append(("none", key(kw), call(lib, entry, **NONE, **kw)))
    for name in ("bl", "sc", "x", "out", "tpe", "offs") + (() if quantising or mode == FP8 else ("xs",)):
        got.append((name, (), call(lib, entry, **{name: None})))
    for kw in (dict(tpe=None, offs=None), dict(E=65535), dict(T=4194241), dict(bl=ctypes.c_void_p(20)),
               dict(bias=ctypes.c_void_p(18)), dict(out=ctypes.c_void_p(33), do=F32)):
        got.append(("some", key(kw), call(lib, entry, **kw)))
    if not quantising:
        got.append(("rows", (), call(lib, entry, xs=ctypes.c_void_p(18) if mode == FP8 else P, x=P if mode == FP8 else ctypes.c_void_p(24))))
    if gated:
        got.append(("act", (), call(lib, entry, act=3)))
        got.append(("limit", (), call(lib, entry, limit=0.0)))
    if quantising:                                                 # everything else is fine: the workspace is last
        for kw in (dict(), dict(bias=None), dict(T=1), dict(T=33), dict(ws=ctypes.c_void_p(24), wsb=1 << 20), dict(ws=P, wsb=16)):
            got.append(("ws", key(kw), call(lib, entry, **kw)))
    return got


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0][12:] for e in ENTRIES])
def test_return_codes_do_not_depend_on_the_threshold(lib, threshold, entry):
    _, mode, quantising, gated = entry
    threshold(mode, 0)
    tile = codes(lib, entry)
    threshold(mode, INT_MAX)
    decode = codes(lib, entry)
    assert tile == decode
    by = {(a, b): rc for a, b, rc in tile}
    assert all(rc != OK for (a, b), rc in by.items() if not (a == "none" and dict(b).keys() <= {"T", "N"} and 0 in dict(b).values()))
    # the codes mx4_check documents, pinned at a few points
    assert by[("none", (("E", 0),))] == SHAPE and by[("none", (("K", 65),))] == ODD_K and by[("none", (("K", 48),))] == SHAPE
    assert by[("none", (("do", 3),))] == DTYPE
    assert by[("none", (("T", 0),))] == OK and by[("none", (("N", 0),))] == OK and by[("none", (("T", 0), ("do", 3)))] == DTYPE
    assert by[("none", ())] == NULLP and by[("none", (("T", 32 * 65535),))] == NULLP and by[("none", (("T", 4194241),))] == NULLP
    assert by[("bl", ())] == NULLP and by[("tpe", ())] == NULLP
    assert by[("some", (("tpe", None), ("offs", None)))] == SHAPE and by[("some", (("E", 65535),))] == SHAPE
    assert by[("some", (("T", 4194241),))] == SHAPE
    assert by[("none", (("di", F16),))] == (DTYPE if quantising else NULLP)     # (byte rows: in_dtype is not looked at)
    assert by[("rows", ())] == ALIGN if not quantising else True
    if gated:
        assert by[("act", ())] == SHAPE and by[("limit", ())] == SHAPE
    if quantising:
        assert all(rc == WS for (a, b), rc in by.items() if a == "ws")
