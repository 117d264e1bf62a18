"""The split entry of the 4-bit code-book (NF4) forward without a GPU (FQL_VERSION 480): declared, exported, bound, and
validated in fql_linear_lut4_fwd's order with the workspace check last, before any HIP call (every call below is invalid or
empty, with host pointers that are never dereferenced); the policy hooks; the op's argument errors before its device check."""
import ctypes

import pytest
import torch

from test_nf4_cpu import ALIGN, BF16, DTYPE, F16, NULLP, ODD_K, OK, P, P2, P_WORD, SHAPE, fq, lib  # noqa: F401

WS = -4


def _split(lib, di=BF16, do=BF16, T=8, K=128, N=40, block=64, c=P, a=P, x=P, o=P2, ws=P, ws_bytes=1 << 30):
    return lib.fql_linear_lut4_split_fwd(c, a, None, block, x, di, None, o, do, T, K, N, ws, ws_bytes, None)


def test_split_entry_abi_and_check_order(lib):
    import test_c_abi
    from fused_int4_amd import _native
    for name, nargs in (("fql_linear_lut4_split_fwd", 15), ("fql_linear_lut4_split_workspace_bytes", 3)):
        assert name in test_c_abi.declared_symbols() and name in _native.exported_symbols()
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.fql_version() >= 480
    null = dict(c=None, a=None, x=None, o=None, ws=None)
    assert _split(lib, T=-1, K=65, block=48, di=F16, **null) == SHAPE         # each step repairs the failure before it
    assert _split(lib, K=65, block=48, di=F16, **null) == ODD_K
    assert _split(lib, K=96, block=48, di=F16, **null) == SHAPE
    assert _split(lib, block=32, di=F16, **null) == SHAPE
    assert _split(lib, di=F16, **null) == DTYPE
    assert _split(lib, T=0, **null) == OK
    assert _split(lib, **null) == NULLP
    assert _split(lib, c=P_WORD, ws=None) == ALIGN                            # the alignment before the workspace
    need = lib.fql_linear_lut4_split_workspace_bytes(8, 128, 40)
    assert need == 16 * 4 * 8 * 40
    for kw in (dict(ws=None), dict(ws=P_WORD), dict(ws_bytes=need - 1)):
        assert _split(lib, **kw) == WS, kw


def test_policy_hooks(lib):
    rows = lib.fql_tune_set_lut4_linear_decode_max_rows(-1)                   # (a negative value changes nothing)
    assert lib.fql_tune_set_lut4_linear_decode_max_rows(-1) == rows
    S = lib.fql_tune_lut4_linear_kernel(1, 4096, 4096) >> 8
    if rows > 0:
        assert lib.fql_tune_lut4_linear_kernel(1, 4096, 4096) & 255 == 2 and S in (1, 2, 4, 8, 16)
        assert lib.fql_tune_lut4_linear_kernel(1, 64, 8) == (1 << 8) | 2      # one pair: never more than one slice
        assert lib.fql_tune_lut4_linear_kernel(rows, 4096, 4096) == lib.fql_tune_lut4_linear_kernel(1, 4096, 4096)   # S(K, N), not of T
    assert lib.fql_tune_lut4_linear_kernel(rows + 1, 4096, 4096) == 1 << 8
    assert lib.fql_linear_lut4_split_workspace_bytes(rows + 1, 4096, 4096) == 0
    assert lib.fql_tune_set_lut4_linear_slices(3) == 0 and lib.fql_tune_set_lut4_linear_slices(4) == 0
    try:
        assert rows == 0 or lib.fql_tune_lut4_linear_kernel(1, 64, 8) == (4 << 8) | 2
    finally:
        assert lib.fql_tune_set_lut4_linear_slices(0) == 4


def test_op_checks_types_and_shapes_before_devices_with_split_k():
    ops = fq().ops
    c, a, x = torch.zeros(40, 64, dtype=torch.uint8), torch.ones(40, 2), torch.zeros(6, 128)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        ops.linear_forward_lut4(c, a, x.half(), split_k=True)
    with pytest.raises(RuntimeError, match="block"):
        ops.linear_forward_lut4(c, a, x, block=96, split_k=True)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.linear_forward_lut4(c, a, x, split_k=True)
    m = fq().NF4Linear(128, 8, split_k=True)
    assert m.split_k and "split_k=True" in repr(m) and list(m.state_dict()) == ["codes", "absmax", "code_book"]
    assert torch.equal(m(x), torch.zeros(6, 8))                               # the CPU forward is the definition either way
