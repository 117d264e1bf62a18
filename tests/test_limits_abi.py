"""The host-side size limits of the C ABI (include/fql_int4.h): at the first refused value an entry
returns its documented code; one below, it passes on to the next check in its documented order.  Every call below is
refused before any HIP call (a NULL workspace, a NULL or misaligned pointer is what the next check trips over), so
nothing launches: there is no GPU in the CPU test tier.  The pattern is tests/test_expert_bias_abi.py's."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
INT8, FAST, EXACT, FP8 = 1, 2, 3, 8
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
B31 = 1 << 31


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def first_refused(ok, lo, hi):
    """The smallest value in (lo, hi] that ``ok`` refuses: ok(lo) holds, ok(hi) does not, ok is monotone."""
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return hi


# ---- mfma_addressable, seen through fql_native_dtype_supported and through the entries that refuse

def supported(lib, T, E, K, N, prec, grouped=1):
    return lib.fql_native_dtype_supported(T, E, K, N, prec, P, grouped) == 1


def limb_bytes(T, E, K, L, sets):
    """include/fql_int4.h: sets * limbs * (K padded to 256) / 256 * row_blocks(T, E) * 8192, row_blocks = (T + 32 E + 159) / 32."""
    return sets * L * ((K + 255) // 256) * ((T + 32 * E + 128 + 31) // 32) * 8192


@pytest.mark.parametrize("prec,L,sets", [(EXACT, 3, 2), (FAST, 2, 2), (INT8, 1, 1), (FP8, 1, 1)])
@pytest.mark.parametrize("E,K", [(1, 32), (4, 32), (8, 544)])
def test_row_limit_is_the_limb_buffer_below_2_31_bytes(lib, prec, L, sets, E, K):
    T = first_refused(lambda t: supported(lib, t, E, K, 136, prec), 1, B31 - 1)
    assert limb_bytes(T - 1, E, K, L, sets) < B31 <= limb_bytes(T, E, K, L, sets)
    assert lib.fql_act_limb_bytes(T - 1, E, K, prec) == limb_bytes(T - 1, E, K, L, sets)
    assert lib.fql_act_limb_bytes(T, E, K, prec) == limb_bytes(T, E, K, L, sets)


@pytest.mark.parametrize("K", [512, 4096, 8192])
def test_column_limit_has_a_margin_of_256_rows(lib, K):
    """(N + 256) * K / 2 < 2^31: the tile kernels form weight offsets of rows up to one tile past N in 32 bits."""
    for grouped in (0, 1):
        N = first_refused(lambda n: supported(lib, 64, 1, K, n, EXACT, grouped), 1, B31 // (K // 2))
        assert (N - 1 + 256) * (K // 2) < B31 <= (N + 256) * (K // 2)


def test_expert_count_enters_the_row_limit(lib):
    E = first_refused(lambda e: supported(lib, 225, e, 256, 776, EXACT), 1, 65535)
    assert limb_bytes(225, E - 1, 256, 3, 2) < B31 <= limb_bytes(225, E, 256, 3, 2)
    assert supported(lib, 225, 65535, 512, 264, INT8)          # one byte plane: the grid's 65535 experts fit


def moe_typed(lib, T, N, K=32, E=4, prec=EXACT, di=BF16, do=BF16):
    return lib.fql_moe_fwd(P, P, P, P, di, P, P, P2, do, E, T, K, N, prec, None, 0, None)


def linear_typed(lib, B, N, K=32, prec=EXACT):
    return lib.fql_linear_fwd(P, BF16, P, P, P, P2, BF16, B, K, N, prec, None, 0, None)


def test_entries_refuse_past_the_row_limit_and_go_on_below_it(lib):
    """One row too many: the 16-bit entries answer FQL_ERR_DTYPE, the gather / row-weight / gated / fp8 ones
    FQL_ERR_ALIGNMENT, the tuning hook FQL_ERR_BAD_SHAPE.  One row fewer: each gets to its workspace check (NULL here)."""
    E, K, N = 4, 32, 136
    for prec in (EXACT, FAST, INT8):
        T = first_refused(lambda t: supported(lib, t, E, K, N, prec), 1, B31 - 1)
        for t, typed, other in ((T, DTYPE, ALIGN), (T - 1, WS, WS)):
            assert moe_typed(lib, t, N, K, E, prec) == typed
            assert lib.fql_moe_bias_fwd(P, P, P, P, BF16, P, P, P, P2, F32, E, t, K, N, prec, None, 0, None) == typed
            assert lib.fql_moe_gather_fwd_f32(P, P, P, P, P, 7, P, P, P2, E, t, K, N, prec, None, 0, None) == other
            assert lib.fql_moe_gather_scaled_fwd_f32(P, P, P, P, P, 7, P, P, P, P2, E, t, K, N, prec, None, 0, None) == other
            assert lib.fql_moe_gated_fwd_f32(P, P, P, P, P, P, P2, E, t, K, N, prec, None, 0, None) == other
            assert lib.fql_moe_gated_fwd(P, P, P, P, BF16, P, P, P2, BF16, E, t, K, N, prec, None, 0, None) == other
            assert lib.fql_moe_glu_fwd(P, P, P, P, BF16, P, P, P2, BF16, E, t, K, N, prec, 1, 1.702, 7.0, None, 0, None) == other
    T = first_refused(lambda t: supported(lib, t, E, K, N, FP8), 1, B31 - 1)
    for t, want in ((T, ALIGN), (T - 1, WS)):
        assert lib.fql_moe_fwd_f32(P, P, P, P, P, P, P2, E, t, K, N, FP8, None, 0, None) == want
        assert lib.fql_moe_fwd_f8(P, P, P, P, P, P, P, P2, F32, E, t, K, N, None, 0, None) == want
    # a single group of rows: the linear entries (rows above the GEMV's 4)
    T = first_refused(lambda t: supported(lib, t, 1, K, N, EXACT, 0), 5, B31 - 1)
    assert linear_typed(lib, T, N) == DTYPE and linear_typed(lib, T - 1, N) == WS
    assert lib.fql_linear_fwd_f8(P, P, P, P, P, P2, F32, T - 1, K, N, None, 0, None) == WS      # (fp8's limit lies higher)


def test_entries_refuse_past_the_column_limit_and_go_on_below_it(lib):
    K = 4096
    N = first_refused(lambda n: supported(lib, 64, 1, K, n, EXACT), 1, B31 // (K // 2))
    for n, typed, other in ((N, DTYPE, ALIGN), (N - 1, WS, WS)):
        assert moe_typed(lib, 64, n, K, 1) == typed
        assert linear_typed(lib, 64, n, K) == typed
        assert lib.fql_moe_gated_fwd_f32(P, P, P, P, P, P, P2, 1, 64, K, n, EXACT, None, 0, None) == other
        assert lib.fql_moe_fwd_f32(P, P, P, P, P, P, P2, 1, 64, K, n, FP8, None, 0, None) == other
    tune = lib.fql_tune_gemm_i8_f32                            # (the hook has no check left below the limit: it launches)
    tune.restype = ctypes.c_int
    tune.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    assert tune(0, P, P, P, P, P, P, P, P, P2, 1, 64, K, N, EXACT, None, None, 0) == SHAPE


def test_expert_count_of_the_grid(lib):
    """65535 experts (grid.y / grid.z) for the INT4 entries, 65534 for the kernels with one more slice for the uncovered
    rows (MXFP4, the per-group input gradient)."""
    K, N, T = 64, 96, 8
    assert lib.fql_moe_fwd_f32(P, P, P, P, P, P, P2, 65536, T, K, N, INT8, None, 0, None) == SHAPE
    assert lib.fql_moe_fwd_f32(P, P, P, P, P, P, P2, 65535, T, K, N, INT8, None, 0, None) == WS
    assert moe_typed(lib, T, N, K, 65536, INT8) == SHAPE and moe_typed(lib, T, N, K, 65535, INT8) == WS
    assert lib.fql_moe_gated_fwd_f32(P, P, P, P, P, P, P2, 65536, T, K, N, INT8, None, 0, None) == SHAPE
    assert lib.fql_moe_gated_fwd_f32(P, P, P, P, P, P, P2, 65535, T, K, N, INT8, None, 0, None) == WS
    assert lib.fql_moe_mx4_fwd(P, P, P, F32, None, P, P, P2, F32, 65535, T, K, N, None, 0, None) == SHAPE
    assert lib.fql_moe_mx4_fwd(P_BYTE, P, P, F32, None, P, P, P2, F32, 65534, T, K, N, None, 0, None) == ALIGN
    assert lib.fql_moe_bias_grad(P, F32, P, P, P2, 65536, T, N, None) == SHAPE
    assert lib.fql_moe_bias_grad(P_BYTE, F32, P, P, P2, 65535, T, N, None) == ALIGN


# ---- the input gradient: it refuses, it has no generic kernel to fall back to

@pytest.mark.parametrize("prec,L,sets", [(EXACT, 3, 2), (FAST, 2, 2), (INT8, 1, 1)])
def test_backward_limits(lib, prec, L, sets):
    E, K, N = 4, 64, 136                                      # the gradient's limbs run along N (padded to 256)
    ok = lambda t: lib.fql_moe_bwd_workspace_bytes(E, t, K, N, prec) > 0
    T = first_refused(ok, 1, B31 - 1)
    assert limb_bytes(T - 1, E, N, L, sets) < B31 <= limb_bytes(T, E, N, L, sets)
    bwd = lambda t, n=N, k=K, e=E: lib.fql_moe_bwd_input_f32(P, P, P, P, P, P, P2, e, t, k, n, prec, None, 0, None)
    assert bwd(T) == SHAPE and bwd(T - 1) == WS
    assert lib.fql_moe_bwd_input(P, P, P, P, BF16, P, P, P2, BF16, E, T, K, N, prec, None, 0, None) == SHAPE
    assert lib.fql_moe_bwd_input(P, P, P, P, BF16, P, P, P2, BF16, E, T - 1, K, N, prec, None, 0, None) == WS
    # weights: N * K / 2 < 2^31 bytes, N <= 132104 (int32 accumulation), E <= 65535
    assert bwd(8, n=132105) == SHAPE and bwd(8, n=132104) == WS
    assert bwd(8, n=132104, k=32514) == SHAPE and bwd(8, n=132104, k=32512) == WS
    assert 132104 * (32512 // 2) < B31 <= 132104 * (32514 // 2)
    assert bwd(8, e=65536) == SHAPE


# ---- adapters, gated backward, bias gradient: element counts below 2^31

def test_lora_element_counts(lib):
    shrink = lambda E, T, C, r: lib.fql_lora_shrink(None, F32, None, 0, None, None, None, E, T, C, r, 1.0, None)
    expand = lambda E, T, C, r: lib.fql_lora_expand(None, None, 1, None, None, None, F32, None, F32, E, T, C, r, 1.0, None)
    grad = lambda E, T, C, r: lib.fql_lora_grad(None, F32, None, None, None, None, 1, E, T, C, r, 1.0, None)
    gated = lambda E, T, C, r: lib.fql_lora_gated_shrink(None, F32, None, 0, None, None, None, E, T, C, r, 1.0, None)
    for f in (shrink, expand, grad):
        assert f(1, 1 << 21, 1 << 10, 8) == SHAPE                            # T * C = 2^31
        assert f(1, (1 << 21) - 1, 1 << 10, 8) == NULLP                      # one row fewer: on to the pointers
        assert f(1, 1 << 25, 8, 64) == SHAPE                                 # T * r = 2^31
        assert f(1, (1 << 25) - 1, 8, 64) == NULLP
        assert f(1 << 15, 8, 1 << 10, 64) == SHAPE                           # E * C * r = 2^31
        assert f((1 << 15) - 1, 8, 1 << 10, 64) == NULLP
        assert f(65536, 8, 8, 8) == SHAPE
    assert gated(1, 1 << 20, 1 << 10, 8) == SHAPE                            # 2 * T * C = 2^31
    assert gated(1, (1 << 20) - 1, 1 << 10, 8) == NULLP


def test_gated_backward_element_count(lib):
    for dt in (F32, BF16):
        assert lib.fql_swiglu_bwd(None, dt, None, dt, None, dt, 1 << 20, 1 << 10, None) == SHAPE     # 2 T F = 2^31
        assert lib.fql_swiglu_bwd(None, dt, None, dt, None, dt, (1 << 20) - 1, 1 << 10, None) == NULLP
        assert lib.fql_glu_bwd(None, dt, None, dt, None, dt, 1 << 20, 1 << 10, 1, 1.702, 7.0, None) == SHAPE
        assert lib.fql_glu_bwd(None, dt, None, dt, None, dt, (1 << 20) - 1, 1 << 10, 1, 1.702, 7.0, None) == NULLP
    assert lib.fql_swiglu_bwd_f32(None, None, None, 1 << 20, 1 << 10, None) == SHAPE
    assert lib.fql_swiglu_bwd_f32(None, None, None, (1 << 20) - 1, 1 << 10, None) == NULLP


def test_bias_grad_width(lib):
    assert lib.fql_moe_bias_grad(P, F32, P, P, P2, 2, 8, 0x7FFFFF01, None) == SHAPE
    assert lib.fql_moe_bias_grad(P_BYTE, F32, P, P, P2, 2, 8, 0x7FFFFF00, None) == ALIGN


# ---- combine: tokens on grid.y

def test_combine_token_count(lib):
    for fn in (lib.fql_combine, lib.fql_combine_sparse):
        assert fn(P, F32, P, P, None, None, P2, F32, 65536, 2, 64, 100, None) == SHAPE
        assert fn(P_BYTE, F32, P, P, None, None, P2, F32, 65535, 2, 64, 100, None) == ALIGN
    assert lib.fql_combine_f32(P, P, P, P2, 65536, 2, 64, 100, None) == SHAPE


# ---- MXFP4: the grid limits (mx4_check, csrc/fql_mx4.hip), every entry

def mx4_entries(lib):
    yield "bf16", lambda b, E, T, K, N: lib.fql_moe_mx4_fwd(b, P, P, F32, None, P, P, P2, F32, E, T, K, N, None, 0, None)
    yield "glu", lambda b, E, T, K, N: lib.fql_moe_mx4_glu_fwd(b, P, P, F32, None, P, P, P2, F32, E, T, K, N, 0, 1.702, 7.0,
                                                                 None, 0, None)
    yield "f8", lambda b, E, T, K, N: lib.fql_moe_mx4_fwd_f8(b, P, P, P, None, P, P, P2, F32, E, T, K, N, None, 0, None)
    yield "q8", lambda b, E, T, K, N: lib.fql_moe_mx4_fwd_q8(b, P, P, F32, None, P, P, P2, F32, E, T, K, N, None, 0, None)
    yield "f4", lambda b, E, T, K, N: lib.fql_moe_mx4_fwd_f4(b, P, P, P, None, P, P, P2, F32, E, T, K, N, None, 0, None)
    yield "q4", lambda b, E, T, K, N: lib.fql_moe_mx4_fwd_q4(b, P, P, F32, None, P, P, P2, F32, E, T, K, N, None, 0, None)


def test_mxfp4_grid_limits(lib):
    K, N = 64, 96
    rows = 64 * 65535                                         # 65535 row tiles of 64 on grid.y
    for name, f in mx4_entries(lib):
        assert f(P, 65535, 8, K, N) == SHAPE, name                           # the experts and the coverage slice on grid.z
        assert f(P_BYTE, 65534, 8, K, N) == ALIGN, name                      # one fewer: on to the alignment of the blocks
        assert f(P, 4, rows + 1, K, N) == SHAPE, name
        assert f(P_BYTE, 4, rows, K, N) == ALIGN, name
    assert lib.fql_moe_mx4_bwd_input(P, P, P, F32, P, P, P2, F32, 65535, 8, K, N, None) == SHAPE


# ---- the routing kernels: experts in LDS / lanes, slots of a token in the first lanes of its group

def test_router_expert_and_slot_counts(lib):
    """E <= 128 (ROUTER_MAX_EXPERTS), top_k <= 8 (ROUTER_MAX_TOPK), for the plain and the scored pair; one below, the call
    goes on to its pointers."""
    fwd = lambda E, k: lib.fql_router_topk_fwd(None, F32, 8, E, k, 1, None, None, None, None)
    bwd = lambda E, k: lib.fql_router_topk_bwd(None, F32, None, None, None, None, 8, E, k, 1, None)
    sfwd = lambda E, k: lib.fql_router_score_topk_fwd(None, F32, 8, E, k, 1, None, 1, 1, 1, 1, 1.0, None, None, None, None)
    sbwd = lambda E, k: lib.fql_router_score_topk_bwd(None, F32, None, None, None, None, 8, E, k, 1, 1, 1.0, None)
    for f in (fwd, bwd, sfwd, sbwd):
        assert f(129, 4) == SHAPE and f(128, 4) == NULLP
        assert f(128, 9) == SHAPE and f(128, 8) == NULLP
    assert lib.fql_router_score_topk_fwd(None, F32, 8, 128, 4, 1, None, 9, 1, 1, 1, 1.0, None, None, None, None) == SHAPE   # groups <= 8
    assert lib.fql_router_score_topk_fwd(None, F32, 8, 128, 4, 1, None, 8, 8, 1, 1, 1.0, None, None, None, None) == NULLP


def test_route_plan_and_regroup_limits(lib):
    """The plan kernels keep one counter per (thread, expert) in LDS: E <= 128; the regroup index G x EL <= 8192."""
    assert lib.fql_route_plan_i32(P, 16, 2, 129, P, P, P, P, None) == SHAPE
    assert lib.fql_route_plan_i32(P, 16, 2, 128, None, P, P, P, None) == NULLP
    assert lib.fql_route_plan_capped_i32(P, 16, 2, 129, None, 0, P, P, P, P, P, None) == SHAPE
    assert lib.fql_route_plan_capped_i32(P, 16, 2, 128, None, 0, None, P, P, P, P, None) == NULLP
    assert lib.fql_regroup_index_i32(P, 64, 129, P, P, P, P, None) == SHAPE              # 8256 entries
    assert lib.fql_regroup_index_i32(None, 64, 128, P, P, P, P, None) == NULLP            # 8192: on to the pointers


def test_per_group_expert_counts(lib):
    """Per-group weights: 65535 experts forward (grid.y / .z), 65534 for the input gradient (one more z-slice zeroes the
    rows no expert covers); one below, the next check (a misaligned scale pointer) answers."""
    K, N, T, G = 64, 96, 8, 32
    P_ODD = ctypes.c_void_p(18)
    bwd = lambda E, s=P: lib.fql_moe_group_bwd_input(P, s, P, P, F32, P, P, P2, F32, E, T, K, N, G, None, 0, None)
    assert bwd(65535) == SHAPE and bwd(65534, P_ODD) == ALIGN
    fwd = lambda E, x=P: lib.fql_moe_group_fwd_f32(x, P, P, P, P, P, P2, E, T, K, N, G, None)
    assert fwd(65536) == SHAPE and fwd(65535, None) == NULLP
    typed = lambda E: lib.fql_moe_group_fwd(P, P, P, P, BF16, P, P, None, P2, BF16, E, T, K, N, G, EXACT, None, 0, None)
    assert typed(65536) == SHAPE
