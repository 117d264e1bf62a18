"""C ABI of the backward entry points (include/fql_int4.h): declared, exported, validated before any HIP call.
No compute call is made here (there is no GPU in the CPU test tier)."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

BWD = ("fql_linear_bwd_workspace_bytes", "fql_linear_bwd_input_f32", "fql_moe_bwd_workspace_bytes",
       "fql_moe_bwd_input_f32", "fql_combine_bwd_f32")
OK, NULLP, SHAPE, ODD_K, WS, PREC = 0, -1, -2, -3, -4, -6
MAX_N = 132104
P = ctypes.c_void_p(16)        # never dereferenced: every call below fails validation (or is empty) before a launch


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def test_declared_and_exported(lib):
    import test_c_abi
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in BWD:
        assert name in names, name
        assert hasattr(raw, name), name
    assert lib.fql_version() >= 220


def _lin(lib, B=4, K=64, N=96, prec=0, go=P, pk=P, sc=P, zp=P, gi=P, ws=None, nbytes=0):
    return lib.fql_linear_bwd_input_f32(go, pk, sc, zp, gi, B, K, N, prec, ws, nbytes, None)


def _moe(lib, E=2, T=8, K=64, N=96, prec=0, pk=P, sc=P, zp=P, go=P, tpe=P, offs=P, gi=P, ws=None, nbytes=0):
    return lib.fql_moe_bwd_input_f32(pk, sc, zp, go, tpe, offs, gi, E, T, K, N, prec, ws, nbytes, None)


def test_linear_validation(lib):
    assert _lin(lib, K=65) == ODD_K
    assert _lin(lib, B=-1) == SHAPE
    assert _lin(lib, N=-3) == SHAPE
    assert _lin(lib, prec=5) == PREC
    assert _lin(lib, N=MAX_N + 1) == SHAPE
    for kw in ("go", "pk", "sc", "zp", "gi"):
        assert _lin(lib, **{kw: None}) == NULLP, kw
    assert _lin(lib) == WS                                  # no workspace
    assert _lin(lib, ws=ctypes.c_void_p(24), nbytes=1 << 30) == WS    # misaligned workspace


def test_moe_validation(lib):
    assert _moe(lib, K=7) == ODD_K
    assert _moe(lib, E=-1) == SHAPE
    assert _moe(lib, T=-1) == SHAPE
    assert _moe(lib, E=70000) == SHAPE
    assert _moe(lib, prec=4) == PREC
    assert _moe(lib, N=MAX_N + 1) == SHAPE
    for kw in ("pk", "sc", "zp", "go", "tpe", "offs", "gi"):
        assert _moe(lib, **{kw: None}) == NULLP, kw
    assert _moe(lib) == WS


def test_empty_batch_is_a_no_op(lib):
    assert _lin(lib, B=0, go=None, pk=None, sc=None, zp=None, gi=None) == OK
    assert _moe(lib, T=0, go=None, pk=None, sc=None, zp=None, gi=None, tpe=None, offs=None) == OK
    assert lib.fql_combine_bwd_f32(None, None, P, None, None, None, 0, 2, 64, 0, None) == OK


def test_combine_validation(lib):
    assert lib.fql_combine_bwd_f32(P, P, P, P, P, P, 4, 0, 64, 8, None) == SHAPE      # top_k
    assert lib.fql_combine_bwd_f32(P, P, P, P, P, P, -1, 2, 64, 8, None) == SHAPE
    assert lib.fql_combine_bwd_f32(P, P, P, P, P, P, 4, 2, 64, 0, None) == SHAPE      # no rows to point at
    assert lib.fql_combine_bwd_f32(P, P, None, P, P, P, 4, 2, 64, 8, None) == NULLP
    assert lib.fql_combine_bwd_f32(None, P, P, P, P, P, 4, 2, 64, 8, None) == NULLP
    assert lib.fql_combine_bwd_f32(P, P, P, P, None, P, 4, 2, 64, 8, None) == NULLP


@pytest.mark.parametrize("B,K,N", [(1, 64, 96), (64, 4096, 1000), (257, 130, 4096)])
def test_workspace_monotone_in_limbs(lib, B, K, N):
    by_limbs = [lib.fql_linear_bwd_workspace_bytes(B, K, N, p) for p in (1, 2, 3)]
    assert 0 < by_limbs[0] < by_limbs[1] < by_limbs[2]
    assert lib.fql_linear_bwd_workspace_bytes(B, K, N, 0) == by_limbs[2]      # default = 3 limbs
    assert lib.fql_linear_bwd_workspace_bytes(B, K, N, 8) == by_limbs[0]      # fp8 layers: 1 limb
    moe = [lib.fql_moe_bwd_workspace_bytes(4, B, K, N, p) for p in (1, 2, 3)]
    assert 0 < moe[0] < moe[1] < moe[2]
    assert lib.fql_linear_bwd_workspace_bytes(B, K, MAX_N + 1, 3) == 0
    assert lib.fql_linear_bwd_workspace_bytes(B, K, N, 5) == 0
