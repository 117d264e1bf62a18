"""The split-K decode form of the dense NVFP4 linear layer (FQL_VERSION 460) without a GPU: the C ABI of the three entries and
the three hooks (every call is invalid, empty or stops at the workspace check; host pointers are never dereferenced), the
workspace arithmetic, the policy as the reporting hook shows it, and the defaults of the ops and the layer."""
import ctypes
import inspect

import pytest
import torch

NEW = ("fql_linear_nvfp4_split_workspace_bytes", "fql_linear_nvfp4_split_fwd", "fql_linear_nvfp4_glu_split_fwd")
HOOKS = ("fql_tune_set_nvfp4_linear_decode_max_rows", "fql_tune_set_nvfp4_linear_slices", "fql_tune_nvfp4_linear_kernel")
INT_MAX, T_MAX = 2 ** 31 - 1, 4194240                                     # T_MAX: the largest T mx4_check admits
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
P, P2, P_HALF, P_WORD = (ctypes.c_void_p(v) for v in (16, 32, 18, 20))    # never dereferenced
NONE = dict(bl=None, sc=None, x=None, bias=None, out=None)

@pytest.fixture
def lib():
    """The library; the two settings of the hooks come back afterwards."""
    import fused_int4_amd
    L = fused_int4_amd._native.lib()
    old = L.fql_tune_set_nvfp4_linear_decode_max_rows(-1), L.fql_tune_set_nvfp4_linear_slices(-1)
    yield L
    L.fql_tune_set_nvfp4_linear_decode_max_rows(old[0]), L.fql_tune_set_nvfp4_linear_slices(old[1])

def _fwd(lib, di=BF16, do=BF16, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, out=P2, ws=None, nbytes=0):
    return lib.fql_linear_nvfp4_split_fwd(bl, sc, gs, x, di, bias, out, do, T, K, N, ws, nbytes, None)

def _glu(lib, di=F32, do=F32, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, out=P2, ws=None, nbytes=0, act=2, alpha=1.702, limit=7.0):
    return lib.fql_linear_nvfp4_glu_split_fwd(bl, sc, gs, x, di, bias, out, do, T, K, N, act, alpha, limit, ws, nbytes, None)

@pytest.mark.parametrize("entry", [_fwd, _glu], ids=["fwd", "glu"])
def test_symbols_version_and_return_codes_in_the_documented_order(lib, entry):
    """mx4_check's order with E = 1, every check in front of any HIP call, the workspace last."""
    import test_c_abi
    from fused_int4_amd import _native
    assert lib.fql_version() >= 460 and all(n in test_c_abi.declared_symbols() for n in NEW)
    assert all(hasattr(ctypes.CDLL(lib._name), n) and n in _native.exported_symbols() for n in NEW + HOOKS)
    call = lambda **kw: entry(lib, **kw)
    assert [call(**NONE, **kw) for kw in (dict(T=-1), dict(K=0), dict(N=-1), dict(K=48), dict(K=65, T=-1))] == [SHAPE] * 5
    assert call(**NONE, K=65) == ODD_K and call(**NONE, K=33, di=F16) == ODD_K
    assert call(**NONE, di=F16) == DTYPE and call(**NONE, do=3) == DTYPE and call(**NONE, T=0, di=F16) == DTYPE
    assert call(**NONE, T=0) == OK and call(**NONE, N=0) == OK and call(**NONE) == NULLP
    assert [call(**{name: None}) for name in ("bl", "sc", "x", "out")] == [NULLP] * 4
    assert call(T=T_MAX + 1) == SHAPE and call(T=T_MAX + 1, bl=None) == NULLP
    assert call(bl=P_WORD) == ALIGN and call(bias=P_HALF) == ALIGN and call(gs=P_HALF) == ALIGN
    if entry is _glu:
        assert call(act=3) == SHAPE and call(limit=0.0) == SHAPE and call(act=3, K=65) == SHAPE
    need = lib.fql_linear_nvfp4_split_workspace_bytes(8, 64, 96, int(entry is _glu))
    assert need > 0 and call() == WS and call(bias=None, gs=None) == WS   # everything else is fine: the workspace is last
    assert call(ws=P, nbytes=need - 1) == WS and call(ws=P_WORD, nbytes=need) == WS and call(ws=None, nbytes=need) == WS
    assert call(ws=P, nbytes=need, bl=P_WORD) == ALIGN                    # ... and behind every other check

def test_workspace_bytes(lib):
    w, plain, rows = lib.fql_linear_nvfp4_split_workspace_bytes, lib.fql_linear_nvfp4_workspace_bytes, lib.fql_tune_set_nvfp4_linear_decode_max_rows
    rows(64)
    for T, K, N in ((1, 32, 8), (33, 96, 40), (64, 1024, 136)):
        h = (2 * T * K + 15) // 16 * 16
        assert plain(T, K, N, 1) == h == lib.fql_moe_nvfp4_workspace_bytes(1, T, K, N, 1) and plain(T, K, N, 0) == 0
        assert w(T, K, N, 0) == 64 * T * N and w(T, K, N, 1) == h + 64 * T * N           # 16 slices of [T][N] float32
    assert w(65, 64, 96, 0) == 0 and w(65, 64, 96, 1) == plain(65, 64, 96, 1)            # above the threshold: no partials
    assert w(0, 64, 96, 1) == 0 and w(-1, 64, 96, 1) == 0 and w(8, 64, 0, 0) == 0
    rows(0)
    assert w(1, 64, 96, 0) == 0
    rows(INT_MAX)                                                                        # size_t arithmetic near INT_MAX
    assert w(T_MAX, 32, INT_MAX, 0) == 64 * T_MAX * INT_MAX
    assert w(T_MAX, INT_MAX - 31, INT_MAX, 1) == (2 * T_MAX * (INT_MAX - 31) + 15) // 16 * 16 + 64 * T_MAX * INT_MAX < 2 ** 64

def test_hooks_and_the_reported_policy(lib):
    rows, slices = lib.fql_tune_set_nvfp4_linear_decode_max_rows, lib.fql_tune_set_nvfp4_linear_slices
    k, dec = lib.fql_tune_nvfp4_linear_kernel, lib.fql_tune_nvfp4_kernel
    assert rows(64) >= 0 and rows(-5) == 64 and slices(0) in (0, 1, 2, 4, 8, 16)
    assert [slices(bad) for bad in (3, 32, -1, 12, INT_MAX)] == [0] * 5                  # refused, nothing changed
    for K in (32, 96, 288, 544, 1024, 2880, 4096, 8192, 28672):
        for N in (1, 8, 40, 136, 2880, 5120, 8192, 28672, 65536):
            got = {k(T, K, N) for T in (1, 2, 33, 64)}
            assert len(got) == 1, (K, N)                                                 # S is a function of (K, N), never of T
            S, form = got.pop() >> 8, k(1, K, N) & 0xFF
            assert S in (1, 2, 4, 8, 16) and S <= max(1, K // 64) and form == (2 if S > 1 else dec(1, 1, K, N)), (K, N, S)
            assert k(65, K, N) == (1 << 8) | dec(1, 65, K, N) and k(0, K, N) >> 8 == 1
    assert [k(1, K, 40) >> 8 for K in (32, 96, 288, 544, 1024)] == [1, 1, 4, 8, 16]
    # the measured shapes
    assert [k(1, K, N) >> 8 for K, N in ((2880, 5120), (4096, 2880), (8192, 8192), (8192, 28672), (28672, 8192))] == [8, 8, 4, 1, 4]
    for S in (1, 2, 4, 8, 16):                                                           # forced: every shape, S above P too
        assert slices(S) in (0, 1, 2, 4, 8) and k(1, 32, 8) >> 8 == S and k(65, 32, 8) >> 8 == 1
    slices(0), rows(0)
    assert k(1, 1024, 40) >> 8 == 1

def test_defaults_and_the_cpu_forward():
    import fused_int4_amd as fq
    from fused_int4_amd.quantize import dequantize_nvfp4, quantize_nvfp4
    for op in (fq.ops.linear_forward_nvfp4, fq.ops.linear_gated_forward_nvfp4):
        assert inspect.signature(op).parameters["split_k"].default is False
    g = torch.Generator().manual_seed(0)
    blocks, scales, gs = quantize_nvfp4(torch.randn(40, 96, generator=g) * 0.1)
    plain, m = fq.NVFP4Linear.from_nvfp4(blocks, scales, gs), fq.NVFP4Linear.from_nvfp4(blocks, scales, gs, split_k=True)
    assert plain.split_k is False and m.split_k is True and fq.NVFP4Linear.from_linear(torch.nn.Linear(32, 8), split_k=True).split_k
    assert "split_k" not in repr(plain) and "split_k=True" in repr(m) and sorted(m.state_dict()) == sorted(plain.state_dict())
    x = torch.randn(5, 96, generator=g)
    want = (x.bfloat16().float() @ dequantize_nvfp4(blocks, scales).T) * torch.as_tensor(gs, dtype=torch.float32)
    assert torch.equal(m(x), want) and torch.equal(plain(x), want)
