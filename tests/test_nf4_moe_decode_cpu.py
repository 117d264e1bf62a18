"""The decode forms of the grouped NF4 experts without a GPU (FQL_VERSION 510): the three split entries
and the five hooks are declared, exported and bound; the split entries validate in lut4_check's order, then the sliced grid's
bound on E, then the workspace, before any HIP call (host pointers that are never dereferenced); the hooks' rules; the ops'
operand errors come before their device check with ``split_k=True``."""
import os
import re

import pytest
import torch

from conftest import ROOT
from test_nf4_cpu import ALIGN, BF16, DTYPE, F16, NULLP, ODD_K, OK, P, P2, P_WORD, SHAPE, fq, lib  # noqa: F401

WS = -4
SETTERS = ("fql_tune_set_lut4_group_decode_max_rows", "fql_tune_set_lut4_group_split_max_rows", "fql_tune_set_lut4_group_slices")


@pytest.fixture
def hooks(lib):
    """The three grouped hooks, put back afterwards (a negative value changes nothing and returns the current one)."""
    old = [getattr(lib, n)(-1) for n in SETTERS]
    yield lib
    for n, v in zip(SETTERS, old):
        getattr(lib, n)(v)


def _split(lib, di=BF16, do=BF16, E=3, T=8, K=128, N=40, block=64, c=P, a=P, x=P, o=P2, tpe=P, offs=P, gated=None, ws=P,
           ws_bytes=1 << 40):
    head = (c, a, None, block, x, di, None, tpe, offs, o, do, E, T, K, N)
    if gated is None:
        return lib.fql_moe_lut4_split_fwd(*head, ws, ws_bytes, None)
    return lib.fql_moe_lut4_glu_split_fwd(*head, *gated, ws, ws_bytes, None)


def test_symbols_version_and_check_order(hooks):
    import test_c_abi
    from fused_int4_amd import _native
    lib = hooks
    for name, nargs in (("fql_moe_lut4_split_fwd", 18), ("fql_moe_lut4_glu_split_fwd", 21), ("fql_moe_lut4_split_workspace_bytes", 5),
                        ("fql_tune_set_lut4_group_decode_max_rows", 1), ("fql_tune_lut4_group_kernel", 1),
                        ("fql_tune_set_lut4_group_split_max_rows", 1), ("fql_tune_set_lut4_group_slices", 1),
                        ("fql_tune_lut4_group_split_kernel", 3)):
        assert name in test_c_abi.declared_symbols() and name in _native.exported_symbols(), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        header = int(re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.fql_version() >= 510 and lib.fql_version() == header
    lib.fql_tune_set_lut4_group_split_max_rows(64)
    null = dict(c=None, a=None, x=None, o=None, tpe=None, offs=None, ws=None)
    silu = (0, 0.0, 0.0)
    for gated in (None, silu):
        call = lambda **kw: _split(lib, gated=gated, **kw)
        assert call(E=0, K=65, block=48, di=F16, **null) == SHAPE             # each step repairs the failure before it
        assert call(K=65, block=48, di=F16, **null) == ODD_K
        assert call(K=96, block=48, di=F16, **null) == SHAPE
        assert call(block=32, di=F16, **null) == SHAPE
        assert call(di=F16, **null) == DTYPE
        assert call(T=0, **null) == OK
        assert call(**null) == NULLP
        assert call(offs=None, ws=None) == NULLP
        assert call(tpe=None, offs=None, ws=None) == SHAPE
        assert call(E=65535, ws=None) == SHAPE
        assert call(T=65535 * 128 + 1, ws=None) == SHAPE
        assert call(E=4096, c=P_WORD, ws=None) == ALIGN                        # the alignment before the sliced grid's bound
        assert call(E=4096, ws=None) == SHAPE                                  # z = E * 16 > 65535, before the workspace
        assert call(E=4095, ws=None) == WS
        need = lib.fql_moe_lut4_split_workspace_bytes(3, 8, 128, 40, int(gated is not None))
        assert need == (8 * 128 * 2 if gated else 0) + 16 * 8 * 40 * 4
        for kw in (dict(ws=None), dict(ws=P_WORD), dict(ws_bytes=need - 1)):
            assert call(**kw) == WS, kw
    assert _split(lib, gated=(99, 0.0, 0.0), **null) == SHAPE
    # past the row threshold the split entry is the plain one: no partial sums, no bound on E beyond the plain entry's
    assert lib.fql_moe_lut4_split_workspace_bytes(3, 65, 128, 40, 0) == 0
    assert lib.fql_moe_lut4_split_workspace_bytes(3, 65, 128, 40, 1) == lib.fql_moe_lut4_workspace_bytes(3, 65, 128, 40, 1) == 65 * 128 * 2
    assert _split(lib, T=65, gated=silu, ws=None) == WS and _split(lib, T=65, gated=silu, ws_bytes=65 * 128 * 2 - 1) == WS


def test_hooks_follow_the_rule_and_leave_the_dense_families_alone(hooks):
    lib = hooks
    dense = lambda: [f(T, K, N) for f in (lib.fql_tune_lut4_linear_kernel, lib.fql_tune_nvfp4_linear_kernel, lib.fql_tune_mx4_linear_kernel)
                     for T, K, N in ((1, 4096, 4096), (16, 11008, 4096), (300, 4096, 11008))]
    before = dense()
    rows = lambda T, m: 0 < T <= m and (T - 1) // 32 + 1 <= 65535
    shapes = [(1, 64, 40), (7, 320, 37), (8, 4096, 4096), (9, 11008, 4096), (2 ** 31 - 1, 4096, 28672)]
    for m in (0, 8, 2 ** 31 - 1):
        lib.fql_tune_set_lut4_group_decode_max_rows(m)
        assert lib.fql_tune_set_lut4_group_decode_max_rows(-1) == m            # the old value back; a negative one changes nothing
        for T, K, N in shapes:
            assert lib.fql_tune_lut4_group_kernel(T) == int(rows(T, m))
    lib.fql_tune_set_lut4_group_decode_max_rows(8)
    for sm in (0, 8):
        lib.fql_tune_set_lut4_group_split_max_rows(sm)
        assert lib.fql_tune_set_lut4_group_split_max_rows(-3) == sm
        for forced in (0, 1, 2, 4, 8, 16):
            lib.fql_tune_set_lut4_group_slices(forced)
            for bad in (-1, 3, 5, 17, 32):
                assert lib.fql_tune_set_lut4_group_slices(bad) == forced        # illegal: ignored
            for T, K, N in shapes:
                code = lib.fql_tune_lut4_group_split_kernel(T, K, N)
                if not rows(T, sm):
                    assert code == (1 << 8) | int(rows(T, 8))                  # the plain entry's kernel
                    continue
                S, kind = code >> 8, code & 255
                assert kind == 2 and S in (1, 2, 4, 8, 16)
                if forced:
                    assert S == forced
                else:                                                          # S(K, N): no empty slice, and T has no say
                    assert S <= max(1, K // 64) and code == lib.fql_tune_lut4_group_split_kernel(1, K, N)
    assert dense() == before


def test_ops_check_operands_before_devices_with_split_k():
    ops = fq().ops
    c, a = torch.zeros(3, 40, 64, dtype=torch.uint8), torch.ones(3, 40, 2)
    x, gu, tab = torch.zeros(6, 128), torch.zeros(6, 256), torch.zeros(3, dtype=torch.int32)
    for op, rows in ((ops.moe_forward_lut4, x), (ops.moe_gated_forward_lut4, gu)):
        with pytest.raises(RuntimeError, match="float16 is refused"):
            op(c, a, rows.half(), tab, tab, split_k=True)
        with pytest.raises(RuntimeError, match="absmax must be"):
            op(c, a[:, :, :1], rows, tab, tab, split_k=True)
        with pytest.raises(RuntimeError, match="columns"):
            op(c, a, rows[:, :-1], tab, tab, split_k=True)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            op(c, a, rows, tab, tab, split_k=True)
    F4 = fq().NF4MoEFFN
    assert F4(2, 64, 64, split_k=True).split_k and not F4(2, 64, 64).split_k and "split_k=True" in repr(F4(2, 64, 64, split_k=True))
    with pytest.raises(ValueError, match="split_k"):
        F4(2, 64, 64, split_k=True, input_grad=True)
