"""Return codes of the C dispatcher (csrc/fql_int4.hip) that are decided before its first HIP call.

A written-out table: (entry point, arguments, expected code).  The expected codes are read off the order of the checks in
each entry point; that order is part of the contract, so a refactor of the dispatcher must leave
every row as it is.  Every pointer is NULL here: no row hands the library memory a kernel could touch if a refusal
were lost.  Refusals that need real operands (alignment, the expert-table pair, workspace size, ...) are in the GPU
tier, tests/test_gpu_dispatch_contract.py."""
import ctypes

import pytest

OK, NULLP, SHAPE, ODD_K, WORKSPACE, LAUNCH, PRECISION, ALIGNMENT, DTYPE = 0, -1, -2, -3, -4, -5, -6, -7, -8
DEF, I8, FAST, EXACT, FP8, BADP = 0, 1, 2, 3, 8, 9
F32, F16, BF16, BADT = 0, 1, 2, 3
N_ = None                      # a NULL pointer

_c_int, _c_vp, _c_sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_TUNE = {
    "fql_tune_gemm_i8_f32": (_c_int, [_c_int] + [_c_vp] * 9 + [_c_int] * 5 + [_c_vp, _c_vp, _c_sz]),
    "fql_tune_gemm_i8": (_c_int, [_c_int] + [_c_vp] * 9 + [_c_int, _c_vp, _c_vp] + [_c_int] * 5 + [_c_vp, _c_vp, _c_sz]),
    "fql_tune_num_configs": (_c_int, []),
    "fql_tune_num_rows32_configs": (_c_int, []),
    "fql_tune_num_rows16_configs": (_c_int, []),
    "fql_tune_num_w4_configs": (_c_int, []),
    "fql_tune_is_config": (_c_int, [_c_int, _c_int]),
    "fql_tune_chosen_cfg": (_c_int, [_c_int] * 6),
}


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    handle = _native.lib()
    for name, (res, args) in _TUNE.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


WS = (N_, 0, N_)               # workspace, workspace_bytes, stream

ROWS = [
    # ---- fql_linear_fwd_f32(x, packed, scales, zps, out, B, K, N, precision, workspace, bytes, stream)
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 4, 1, BADP) + WS, PRECISION),
    ("fql_linear_fwd_f32", (N_,) * 5 + (-1, 3, 1, BADP) + WS, PRECISION),        # precision before shape and odd K
    ("fql_linear_fwd_f32", (N_,) * 5 + (-1, 4, 1, DEF) + WS, SHAPE),
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, -2, 1, DEF) + WS, SHAPE),
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 4, -1, DEF) + WS, SHAPE),
    ("fql_linear_fwd_f32", (N_,) * 5 + (-1, 3, 1, DEF) + WS, SHAPE),             # shape before odd K
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 3, 1, DEF) + WS, ODD_K),
    ("fql_linear_fwd_f32", (N_,) * 5 + (0, 3, 1, DEF) + WS, ODD_K),              # odd K before the empty batch
    ("fql_linear_fwd_f32", (N_,) * 5 + (0, 4, 1, DEF) + WS, OK),
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 4, 0, FP8) + WS, OK),
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 4, 1, DEF) + WS, NULLP),
    ("fql_linear_fwd_f32", (N_,) * 5 + (1, 0, 1, DEF) + WS, NULLP),              # K == 0: pointers first
    ("fql_linear_fwd_f32", (N_,) * 5 + (8, 64, 16, FP8) + WS, NULLP),
    # ---- fql_linear_bias_fwd_f32(x, packed, scales, zps, bias, out, B, K, N, precision, ...)
    ("fql_linear_bias_fwd_f32", (N_,) * 6 + (1, 4, 1, BADP) + WS, PRECISION),
    ("fql_linear_bias_fwd_f32", (N_,) * 6 + (1, 4, -1, I8) + WS, SHAPE),
    ("fql_linear_bias_fwd_f32", (N_,) * 6 + (1, 5, 1, FAST) + WS, ODD_K),
    ("fql_linear_bias_fwd_f32", (N_,) * 6 + (0, 4, 1, EXACT) + WS, OK),
    ("fql_linear_bias_fwd_f32", (N_,) * 6 + (3, 4, 1, DEF) + WS, NULLP),
    # ---- fql_moe_fwd_f32(packed, scales, zps, inputs, tpe, offs, out, E, T, K, N, precision, ...)
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, BADP) + WS, PRECISION),
    ("fql_moe_fwd_f32", (N_,) * 7 + (-1, 8, 64, 16, DEF) + WS, SHAPE),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, -1, 64, 16, DEF) + WS, SHAPE),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, -2, 16, DEF) + WS, SHAPE),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, 64, -1, DEF) + WS, SHAPE),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, 63, 16, DEF) + WS, ODD_K),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 0, 63, 16, DEF) + WS, ODD_K),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 0, 64, 16, DEF) + WS, OK),
    ("fql_moe_fwd_f32", (N_,) * 7 + (0, 8, 0, 0, FP8) + WS, OK),
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, DEF) + WS, NULLP),
    ("fql_moe_fwd_f32", (N_,) * 7 + (0, 8, 64, 16, DEF) + WS, NULLP),             # E == 0 with no `out`: the pointer first
    ("fql_moe_fwd_f32", (N_,) * 7 + (2, 8, 0, 16, DEF) + WS, NULLP),
    # ---- fql_moe_gather_fwd_f32(packed, scales, zps, tokens, row_index, n_tokens, tpe, offs, out, E, T, K, N, precision, ...)
    ("fql_moe_gather_fwd_f32", (N_,) * 5 + (4,) + (N_,) * 3 + (2, 8, 64, 16, DEF) + WS, NULLP),
    ("fql_moe_gather_fwd_f32", (N_,) * 5 + (4,) + (N_,) * 3 + (-2, 8, 63, 16, BADP) + WS, NULLP),   # row_index before everything
    # ---- fql_moe_gather_scaled_fwd_f32(packed, scales, zps, tokens, row_index, n_tokens, row_weight, tpe, offs, out, E, ...)
    ("fql_moe_gather_scaled_fwd_f32", (N_,) * 5 + (4,) + (N_,) * 4 + (2, 8, 64, 16, DEF) + WS, NULLP),
    ("fql_moe_gather_scaled_fwd_f32", (N_,) * 5 + (4,) + (N_,) * 4 + (2, 8, 64, 16, FP8) + WS, NULLP),
    # ---- fql_native_dtype_supported(rows, E, K, N, precision, packed, grouped): 1 or 0
    ("fql_native_dtype_supported", (8, 1, 64, 16, BADP, N_, 0), 0),
    ("fql_native_dtype_supported", (0, 1, 64, 16, DEF, N_, 0), 0),
    ("fql_native_dtype_supported", (8, 0, 64, 16, DEF, N_, 1), 0),
    ("fql_native_dtype_supported", (2, 1, 64, 16, DEF, N_, 0), 0),                # a GEMV shape
    ("fql_native_dtype_supported", (2, 1, 64, 16, DEF, N_, 1), 1),                # ... but not a grouped call
    ("fql_native_dtype_supported", (3, 1, 64, 16, DEF, N_, 0), 1),
    ("fql_native_dtype_supported", (8, 2, 34, 16, DEF, N_, 1), 0),                # K % 32
    ("fql_native_dtype_supported", (8, 2, 64, 16, FP8, N_, 1), 1),
    # ---- fql_linear_fwd(x, in_dtype, packed, scales, zps, out, out_dtype, B, K, N, precision, ...)
    ("fql_linear_fwd", (N_, F32, N_, N_, N_, N_, F32, 1, 3, 1, DEF) + WS, ODD_K),                   # forwards to the _f32 form
    ("fql_linear_fwd", (N_, F32, N_, N_, N_, N_, F32, -1, 3, 1, BADP) + WS, PRECISION),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, F32, 8, 64, 16, BADP) + WS, PRECISION),
    ("fql_linear_fwd", (N_, BADT, N_, N_, N_, N_, F32, -1, 64, 16, BADP) + WS, PRECISION),          # precision before dtype
    ("fql_linear_fwd", (N_, BADT, N_, N_, N_, N_, F32, -1, 63, 16, DEF) + WS, DTYPE),               # dtype before shape
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, -1, 8, 64, 16, DEF) + WS, DTYPE),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, -1, 63, 16, DEF) + WS, SHAPE),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 8, -64, 16, DEF) + WS, SHAPE),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 8, 64, -1, DEF) + WS, SHAPE),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 0, 63, 16, DEF) + WS, ODD_K),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 0, 64, 16, DEF) + WS, OK),
    ("fql_linear_fwd", (N_, F32, N_, N_, N_, N_, F16, 8, 64, 0, FP8) + WS, OK),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 8, 64, 16, DEF) + WS, NULLP),
    ("fql_linear_fwd", (N_, F16, N_, N_, N_, N_, BF16, 8, 0, 16, DEF) + WS, NULLP),                 # the typed form has no K == 0 path
    # ---- fql_linear_bias_fwd(x, in_dtype, packed, scales, zps, bias, out, out_dtype, B, K, N, precision, ...)
    ("fql_linear_bias_fwd", (N_, F32, N_, N_, N_, N_, N_, F32, 1, 4, 1, DEF) + WS, NULLP),
    ("fql_linear_bias_fwd", (N_, BF16, N_, N_, N_, N_, N_, F32, 1, 4, 1, BADP) + WS, PRECISION),
    ("fql_linear_bias_fwd", (N_, BF16, N_, N_, N_, N_, N_, BADT, 1, 4, 1, DEF) + WS, DTYPE),
    ("fql_linear_bias_fwd", (N_, BF16, N_, N_, N_, N_, N_, F32, 1, 5, 1, DEF) + WS, ODD_K),
    ("fql_linear_bias_fwd", (N_, BF16, N_, N_, N_, N_, N_, F32, 1, 4, 1, DEF) + WS, NULLP),
    # ---- fql_moe_fwd(packed, scales, zps, inputs, in_dtype, tpe, offs, out, out_dtype, E, T, K, N, precision, ...)
    ("fql_moe_fwd", (N_,) * 4 + (F32, N_, N_, N_, F32, 0, 8, 64, 16, DEF) + WS, NULLP),             # forwards: E == 0 is no shape error there
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 0, 8, 64, 16, BADP) + WS, PRECISION),
    ("fql_moe_fwd", (N_,) * 4 + (BADT, N_, N_, N_, F32, 0, 8, 63, 16, DEF) + WS, DTYPE),            # dtype before shape
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, BADT, 2, 8, 64, 16, DEF) + WS, DTYPE),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 0, 8, 63, 16, DEF) + WS, SHAPE),             # the typed form refuses E == 0
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, 8, 0, 16, DEF) + WS, SHAPE),              # ... and K == 0
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, -1, 64, 16, DEF) + WS, SHAPE),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, 8, 64, -1, DEF) + WS, SHAPE),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, 0, 63, 16, DEF) + WS, ODD_K),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, 0, 64, 16, DEF) + WS, OK),
    ("fql_moe_fwd", (N_,) * 4 + (F32, N_, N_, N_, BF16, 2, 8, 64, 0, FP8) + WS, OK),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 2, 8, 64, 16, DEF) + WS, NULLP),
    ("fql_moe_fwd", (N_,) * 4 + (F16, N_, N_, N_, F32, 70000, 8, 64, 16, DEF) + WS, NULLP),         # pointers before E > 65535
    # ---- fql_moe_fwd_f8(packed, scales, zps, inputs, act_scales, tpe, offs, out, out_dtype, E, T, K, N, ...)
    ("fql_moe_fwd_f8", (N_,) * 8 + (F32, 2, 8, 64, 16) + WS, NULLP),
    ("fql_moe_fwd_f8", (N_,) * 8 + (BADT, -2, 8, 63, 16) + WS, NULLP),                              # the table before everything
    # ---- fql_linear_fwd_f8(x, act_scales, packed, scales, zps, out, out_dtype, B, K, N, ...)
    ("fql_linear_fwd_f8", (N_,) * 6 + (BADT, -1, 63, 16) + WS, DTYPE),
    ("fql_linear_fwd_f8", (N_,) * 6 + (F16, -1, 63, 16) + WS, SHAPE),
    ("fql_linear_fwd_f8", (N_,) * 6 + (F16, 8, 0, 16) + WS, SHAPE),
    ("fql_linear_fwd_f8", (N_,) * 6 + (F16, 8, 64, -16) + WS, SHAPE),
    ("fql_linear_fwd_f8", (N_,) * 6 + (F32, 0, 63, 16) + WS, ODD_K),
    ("fql_linear_fwd_f8", (N_,) * 6 + (F32, 0, 64, 16) + WS, OK),
    ("fql_linear_fwd_f8", (N_,) * 6 + (BF16, 8, 64, 0) + WS, OK),
    ("fql_linear_fwd_f8", (N_,) * 6 + (BF16, 8, 64, 16) + WS, NULLP),
    # ---- fql_linear_group_fwd_f32(x, packed, scales, zps, bias, out, B, K, N, group, stream)
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (-1, 63, 16, 0, N_), SHAPE),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, -64, 16, 32, N_), SHAPE),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 64, -1, 32, N_), SHAPE),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 63, 16, 0, N_), ODD_K),                            # odd K before the group checks
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (0, 64, 16, 0, N_), SHAPE),                            # the group before the empty batch
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 64, 16, -32, N_), SHAPE),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 66, 16, 33, N_), SHAPE),                           # odd group
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 64, 16, 24, N_), SHAPE),                           # does not tile K
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (0, 64, 16, 32, N_), OK),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 64, 0, 32, N_), OK),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 64, 16, 32, N_), NULLP),
    ("fql_linear_group_fwd_f32", (N_,) * 6 + (8, 0, 16, 32, N_), NULLP),
    # ---- fql_moe_group_fwd_f32(packed, scales, zps, inputs, tpe, offs, out, E, T, K, N, group, stream)
    ("fql_moe_group_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, 32, N_), NULLP),
    ("fql_moe_group_fwd_f32", (N_,) * 7 + (-2, 8, 63, 16, 0, N_), NULLP),                           # the table before everything
    # ---- fql_linear_group_ws_fwd_f32(x, packed, scales, zps, bias, out, B, K, N, group, precision, ...)
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (-1, 63, 16, 0, BADP) + WS, PRECISION),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 64, 16, 32, FP8) + WS, PRECISION),              # no fp8 form
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (-1, 63, 16, 0, DEF) + WS, SHAPE),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 63, 16, 0, DEF) + WS, SHAPE),                   # here the group comes before odd K
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 63, 16, 2, DEF) + WS, SHAPE),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 63, 16, 63, DEF) + WS, ODD_K),                  # (through the float32 path's checks)
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 64, 16, 24, DEF) + WS, SHAPE),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (0, 0, 16, 0, DEF) + WS, OK),                       # K == 0: any group goes
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 0, 16, -4, DEF) + WS, NULLP),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 0, 16, 3, DEF) + WS, SHAPE),                    # ... but a positive one must be even
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (0, 64, 16, 32, I8) + WS, OK),
    ("fql_linear_group_ws_fwd_f32", (N_,) * 6 + (8, 64, 16, 32, FAST) + WS, NULLP),
    # ---- fql_moe_group_ws_fwd_f32(packed, scales, zps, inputs, tpe, offs, out, E, T, K, N, group, precision, ...)
    ("fql_moe_group_ws_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, 32, DEF) + WS, NULLP),
    ("fql_moe_group_ws_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, 32, BADP) + WS, NULLP),                 # the table before everything
    # ---- fql_moe_gated_fwd_f32(packed, scales, zps, gate_up, tpe, offs, out, E, T, K, N, precision, ...)
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (0, 8, 63, 16, BADP) + WS, PRECISION),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, FP8) + WS, PRECISION),                     # no gated fp8 form
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (0, 8, 63, 16, DEF) + WS, SHAPE),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, -8, 64, 16, DEF) + WS, SHAPE),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 8, 0, 16, DEF) + WS, SHAPE),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 8, 64, -16, DEF) + WS, SHAPE),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 0, 63, 16, DEF) + WS, ODD_K),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 0, 64, 16, DEF) + WS, OK),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 8, 64, 0, I8) + WS, OK),
    ("fql_moe_gated_fwd_f32", (N_,) * 7 + (2, 8, 64, 16, DEF) + WS, NULLP),
    # ---- fql_moe_gated_fwd(packed, scales, zps, gate_up, in_dtype, tpe, offs, out, out_dtype, E, T, K, N, precision, ...)
    ("fql_moe_gated_fwd", (N_,) * 4 + (F32, N_, N_, N_, F32, 2, 8, 64, 16, FP8) + WS, PRECISION),   # forwards to the _f32 form
    ("fql_moe_gated_fwd", (N_,) * 4 + (BADT, N_, N_, N_, F32, 0, 8, 63, 16, BADP) + WS, PRECISION),
    ("fql_moe_gated_fwd", (N_,) * 4 + (F16, N_, N_, N_, F16, 2, 8, 64, 16, FP8) + WS, PRECISION),
    ("fql_moe_gated_fwd", (N_,) * 4 + (BADT, N_, N_, N_, F32, 0, 8, 63, 16, DEF) + WS, SHAPE),      # here shape and odd K come before dtype
    ("fql_moe_gated_fwd", (N_,) * 4 + (BADT, N_, N_, N_, F32, 2, 8, 63, 16, DEF) + WS, ODD_K),
    ("fql_moe_gated_fwd", (N_,) * 4 + (BADT, N_, N_, N_, F32, 2, 0, 64, 16, DEF) + WS, DTYPE),      # ... and dtype before the empty call
    ("fql_moe_gated_fwd", (N_,) * 4 + (F16, N_, N_, N_, BADT, 2, 8, 64, 16, DEF) + WS, DTYPE),
    ("fql_moe_gated_fwd", (N_,) * 4 + (F16, N_, N_, N_, F16, 2, 0, 64, 16, DEF) + WS, OK),
    ("fql_moe_gated_fwd", (N_,) * 4 + (BF16, N_, N_, N_, F32, 2, 8, 64, 0, DEF) + WS, OK),
    ("fql_moe_gated_fwd", (N_,) * 4 + (BF16, N_, N_, N_, BF16, 2, 8, 64, 16, DEF) + WS, NULLP),
    # ---- fql_route_plan_i32(expert_of_slot, n_slots, top_k, E, counts, offsets, token_of_sorted, pos_of_slot, stream)
    ("fql_route_plan_i32", (N_, -1, 2, 4) + (N_,) * 5, SHAPE),
    ("fql_route_plan_i32", (N_, 8, 0, 4) + (N_,) * 5, SHAPE),
    ("fql_route_plan_i32", (N_, 8, 2, 0) + (N_,) * 5, SHAPE),
    ("fql_route_plan_i32", (N_, 8, 2, 129) + (N_,) * 5, SHAPE),
    ("fql_route_plan_i32", (N_, 8, 2, 128) + (N_,) * 5, NULLP),
    ("fql_route_plan_i32", (N_, 0, 2, 4) + (N_,) * 5, NULLP),                                       # counts / offsets are written even for no slots
    # ---- fql_combine_f32(y, pos_of_slot, weights, out, T, top_k, N, R, stream)
    ("fql_combine_f32", (N_,) * 4 + (-1, 2, 16, 8, N_), SHAPE),
    ("fql_combine_f32", (N_,) * 4 + (4, 0, 16, 8, N_), SHAPE),
    ("fql_combine_f32", (N_,) * 4 + (4, 2, -16, 8, N_), SHAPE),
    ("fql_combine_f32", (N_,) * 4 + (4, 2, 16, -8, N_), SHAPE),
    ("fql_combine_f32", (N_,) * 4 + (0, 2, 16, 0, N_), OK),
    ("fql_combine_f32", (N_,) * 4 + (4, 2, 0, 8, N_), OK),
    ("fql_combine_f32", (N_,) * 4 + (4, 2, 16, 8, N_), NULLP),
    ("fql_combine_f32", (N_,) * 4 + (70000, 2, 16, 8, N_), NULLP),                                  # pointers before T > 65535
    # ---- fql_combine_bwd_f32(grad_out, y, pos_of_slot, weights, grad_y, grad_weights, T, top_k, N, rows, stream)
    ("fql_combine_bwd_f32", (N_,) * 6 + (-1, 2, 16, 8, N_), SHAPE),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 0, 16, 8, N_), SHAPE),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 2, -1, 8, N_), SHAPE),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 2, 16, -8, N_), SHAPE),
    ("fql_combine_bwd_f32", (N_,) * 6 + (0, 2, 16, 0, N_), OK),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 2, 16, 0, N_), SHAPE),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 2, 16, 8, N_), NULLP),
    ("fql_combine_bwd_f32", (N_,) * 6 + (4, 2, 0, 8, N_), NULLP),                                   # pos_of_slot before the N == 0 shortcut
    # ---- fql_regroup_index_i32(recv_counts, G, EL, tokens_per_expert, input_offsets, gather, scatter, stream)
    ("fql_regroup_index_i32", (N_, 0, 4) + (N_,) * 5, SHAPE),
    ("fql_regroup_index_i32", (N_, 2, 0) + (N_,) * 5, SHAPE),
    ("fql_regroup_index_i32", (N_, 128, 65) + (N_,) * 5, SHAPE),
    ("fql_regroup_index_i32", (N_, 128, 64) + (N_,) * 5, NULLP),
    # ---- fql_unpack_u8(packed, q, nbytes, stream)
    ("fql_unpack_u8", (N_, N_, 0, N_), OK),
    ("fql_unpack_u8", (N_, N_, 16, N_), NULLP),
    # ---- fql_dequantize_f32(packed, scales, zps, w, N, K, stream)
    ("fql_dequantize_f32", (N_,) * 4 + (-1, 63, N_), SHAPE),
    ("fql_dequantize_f32", (N_,) * 4 + (16, -64, N_), SHAPE),
    ("fql_dequantize_f32", (N_,) * 4 + (0, 63, N_), ODD_K),
    ("fql_dequantize_f32", (N_,) * 4 + (0, 64, N_), OK),
    ("fql_dequantize_f32", (N_,) * 4 + (16, 0, N_), OK),
    ("fql_dequantize_f32", (N_,) * 4 + (16, 64, N_), NULLP),
    # ---- fql_quantize_rows_f32(w, packed, scales, zps, N, K, stream)
    ("fql_quantize_rows_f32", (N_,) * 4 + (-1, 63, N_), SHAPE),
    ("fql_quantize_rows_f32", (N_,) * 4 + (16, -2, N_), SHAPE),
    ("fql_quantize_rows_f32", (N_,) * 4 + (0, 63, N_), ODD_K),
    ("fql_quantize_rows_f32", (N_,) * 4 + (0, 64, N_), OK),
    ("fql_quantize_rows_f32", (N_,) * 4 + (16, 0, N_), OK),
    ("fql_quantize_rows_f32", (N_,) * 4 + (16, 64, N_), NULLP),
    # ---- fql_quantize_tensor_f32(w, packed, scales, zps, scratch, N, K, stream)
    ("fql_quantize_tensor_f32", (N_,) * 5 + (-1, 63, N_), SHAPE),
    ("fql_quantize_tensor_f32", (N_,) * 5 + (16, -2, N_), SHAPE),
    ("fql_quantize_tensor_f32", (N_,) * 5 + (16, 63, N_), ODD_K),
    ("fql_quantize_tensor_f32", (N_,) * 5 + (0, 64, N_), OK),
    ("fql_quantize_tensor_f32", (N_,) * 5 + (16, 0, N_), OK),
    ("fql_quantize_tensor_f32", (N_,) * 5 + (16, 64, N_), NULLP),
    # ---- fql_act_quant_f32(x, limbs, delta, rowsum, tpe, offs, E, T, K, precision, stream)
    ("fql_act_quant_f32", (N_,) * 6 + (0, -1, 0, BADP, N_), PRECISION),
    ("fql_act_quant_f32", (N_,) * 6 + (2, -1, 64, DEF, N_), SHAPE),
    ("fql_act_quant_f32", (N_,) * 6 + (2, 0, 0, DEF, N_), SHAPE),                                   # K <= 0 before the empty call
    ("fql_act_quant_f32", (N_,) * 6 + (0, 0, 64, DEF, N_), SHAPE),
    ("fql_act_quant_f32", (N_,) * 6 + (2, 0, 63, FP8, N_), OK),                                     # (any K: odd is fine for activations)
    ("fql_act_quant_f32", (N_,) * 6 + (2, 8, 64, DEF, N_), NULLP),
    # ---- fql_gemm_i8_f32(limbs, delta, rowsum, packed, scales, zps, tpe, offs, out, E, T, K, N, precision, stream, scratch, bytes)
    ("fql_gemm_i8_f32", (N_,) * 9 + (0, 8, 63, 16, BADP, N_, N_, 0), PRECISION),
    ("fql_gemm_i8_f32", (N_,) * 9 + (0, 8, 63, 16, DEF, N_, N_, 0), SHAPE),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, -8, 64, 16, DEF, N_, N_, 0), SHAPE),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 8, 0, 16, DEF, N_, N_, 0), SHAPE),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 8, 64, -1, DEF, N_, N_, 0), SHAPE),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 0, 63, 16, DEF, N_, N_, 0), ODD_K),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 0, 64, 16, FP8, N_, N_, 0), OK),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 8, 64, 0, DEF, N_, N_, 0), OK),
    ("fql_gemm_i8_f32", (N_,) * 9 + (2, 8, 64, 16, DEF, N_, N_, 0), NULLP),
    # ---- fql_tune_gemm_i8_f32(cfg, <the same>): the configuration id is checked first, against the precision's limb count
    ("fql_tune_gemm_i8_f32", (-1,) + (N_,) * 9 + (2, 8, 64, 16, DEF, N_, N_, 0), SHAPE),
    ("fql_tune_gemm_i8_f32", (4,) + (N_,) * 9 + (2, 0, 64, 16, DEF, N_, N_, 0), SHAPE),              # an id no limb count is built for
    ("fql_tune_gemm_i8_f32", (0,) + (N_,) * 9 + (2, 0, 64, 16, I8, N_, N_, 0), SHAPE),               # 3 limbs only
    ("fql_tune_gemm_i8_f32", (300,) + (N_,) * 9 + (2, 0, 64, 16, FAST, N_, N_, 0), SHAPE),
    ("fql_tune_gemm_i8_f32", (100,) + (N_,) * 9 + (2, 0, 64, 16, FP8, N_, N_, 0), SHAPE),            # fp8: wide ids only
    ("fql_tune_gemm_i8_f32", (18,) + (N_,) * 9 + (2, 0, 64, 16, BADP, N_, N_, 0), SHAPE),
    ("fql_tune_gemm_i8_f32", (100,) + (N_,) * 9 + (2, 0, 64, 16, BADP, N_, N_, 0), PRECISION),
    ("fql_tune_gemm_i8_f32", (0,) + (N_,) * 9 + (2, 0, 63, 16, DEF, N_, N_, 0), ODD_K),
    ("fql_tune_gemm_i8_f32", (301,) + (N_,) * 9 + (2, 0, 64, 16, EXACT, N_, N_, 0), OK),
    ("fql_tune_gemm_i8_f32", (5,) + (N_,) * 9 + (2, 8, 64, 0, FP8, N_, N_, 0), OK),
    ("fql_tune_gemm_i8_f32", (223,) + (N_,) * 9 + (2, 8, 64, 16, FAST, N_, N_, 0), NULLP),
    # ---- fql_tune_gemm_i8(cfg, limbs, delta, rowsum, packed, scales, zps, tpe, offs, out, out_dtype, bias, row_weight, E, ...)
    ("fql_tune_gemm_i8", (10,) + (N_,) * 9 + (BADT, N_, N_, 2, 8, 64, 16, FAST, N_, N_, 0), SHAPE),
    ("fql_tune_gemm_i8", (11,) + (N_,) * 9 + (BADT, N_, N_, 0, 8, 63, 16, FAST, N_, N_, 0), DTYPE),  # dtype before shape
    ("fql_tune_gemm_i8", (11,) + (N_,) * 9 + (F16, N_, N_, 0, 8, 63, 16, FAST, N_, N_, 0), SHAPE),
    ("fql_tune_gemm_i8", (12,) + (N_,) * 9 + (BF16, N_, N_, 2, 0, 64, 16, FP8, N_, N_, 0), OK),
    ("fql_tune_gemm_i8", (208,) + (N_,) * 9 + (BF16, N_, N_, 2, 8, 64, 16, I8, N_, N_, 0), NULLP),
    # ---- size queries: 0 is the refusal
    ("fql_act_padded_k", (0,), 0),
    ("fql_act_padded_k", (-5,), 0),
    ("fql_act_padded_k", (1,), 256),
    ("fql_act_padded_k", (257,), 512),
    ("fql_linear_workspace_bytes", (8, 64, 16, BADP), 0),
    ("fql_linear_workspace_bytes", (2, 64, 16, DEF), 0),                                             # GEMV shapes use none
    ("fql_linear_workspace_bytes", (0, 64, 16, FP8), 0),
    ("fql_linear_workspace_bytes", (8, 0, 16, DEF), 0),
    ("fql_linear_workspace_bytes", (8, 34, 16, DEF), 0),
    ("fql_moe_workspace_bytes", (2, 8, 64, 16, BADP), 0),
    ("fql_moe_workspace_bytes", (2, 0, 64, 16, DEF), 0),
    ("fql_moe_workspace_bytes", (0, 8, 64, 16, DEF), 0),
    ("fql_moe_workspace_bytes", (2, 8, 0, 16, DEF), 0),
    ("fql_moe_workspace_bytes", (2, 8, 34, 16, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 64, 16, 32, BADP), 0),
    ("fql_group_workspace_bytes", (2, 8, 64, 16, 32, FP8), 0),
    ("fql_group_workspace_bytes", (0, 8, 64, 16, 32, DEF), 0),
    ("fql_group_workspace_bytes", (2, 0, 64, 16, 32, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 0, 16, 32, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 64, 0, 32, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 64, 16, 0, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 64, 16, 24, DEF), 0),
    ("fql_group_workspace_bytes", (2, 8, 68, 16, 34, DEF), 0),                                       # K % 32
    ("fql_act_limb_bytes", (8, 2, 64, BADP), 0),
    ("fql_act_limb_bytes", (0, 2, 64, DEF), 0),
    ("fql_act_limb_bytes", (8, 0, 64, DEF), 0),
    ("fql_act_limb_bytes", (8, 2, 0, DEF), 0),
    ("fql_act_limb_bytes", (8, 2, 64, I8), 1 * 1 * 7 * 8192),                                        # (8 + 32 * 2 + 159) / 32 = 7 row blocks
    ("fql_act_limb_bytes", (8, 2, 64, FP8), 1 * 1 * 7 * 8192),
    ("fql_act_limb_bytes", (8, 2, 257, DEF), 2 * 3 * 2 * 7 * 8192),                                  # residual set, 3 limbs, 2 k-blocks
    ("fql_gemm_scratch_bytes", (BADP,), 0),
    ("fql_gemm_scratch_bytes", (I8,), 0),
    ("fql_gemm_scratch_bytes", (FP8,), 0),
    # ---- tuning queries
    ("fql_tune_num_configs", (), 18),
    ("fql_tune_num_rows32_configs", (), 8),
    ("fql_tune_num_rows16_configs", (), 9),
    ("fql_tune_num_w4_configs", (), 2),
    ("fql_tune_is_config", (1, BADP), 0),
    ("fql_tune_chosen_cfg", (BADP, 8, 1024, 4096, 11008, 1), -1),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{i}-{ROWS[i][0]}")
def test_return_code(lib, row):
    name, args, expected = ROWS[row]
    assert getattr(lib, name)(*args) == expected, (name, args)


def test_error_strings(lib):
    for code in range(0, -9, -1):
        assert lib.fql_error_string(code) not in (None, b"unknown error code"), code
    assert lib.fql_error_string(1) == b"unknown error code"
    assert lib.fql_error_string(-9) == b"unknown error code"


# The tile configurations that exist, per precision: wide ids (fql_gemm_i8.h) built for that limb count, every id of the
# 32-row, 16-row and 4-wave 16-row families, the one-wave-per-SIMD pair at 3 limbs.  fp8: its seven wide ids alone.
FAMILIES = set(range(100, 108)) | set(range(200, 209)) | set(range(220, 224))
CONFIGS = {
    DEF: {0, 1, 7, 8, 9, 13, 300, 301} | FAMILIES,
    EXACT: {0, 1, 7, 8, 9, 13, 300, 301} | FAMILIES,
    FAST: {1, 2, 3, 7, 8, 11, 13} | FAMILIES,
    I8: {1, 2, 7, 8, 11, 12, 13} | FAMILIES,
    FP8: {1, 5, 6, 7, 8, 11, 12},
}


@pytest.mark.parametrize("precision", sorted(CONFIGS))
def test_configuration_ids(lib, precision):
    got = {c for c in range(-2, 400) if lib.fql_tune_is_config(c, precision)}
    assert got == CONFIGS[precision]
