"""Return codes of the C dispatcher (csrc/fql_int4.hip) that need real operands: the GPU tier of
tests/test_dispatch_contract.py.  Alignment refusals, the expert-table pair, the row weight that is not the plane behind
delta, workspace NULL / misaligned / too small, fp8 on a GEMV shape, 16-bit I/O off the matrix-core path.

Every row is refused before a launch, and every pointer is a real device buffer large enough for the call it describes
(the 70000-expert rows get 70000-entry tables of zeros), so a lost refusal would compute, not fault.  Shapes: E 2, T 8,
K 64, N 16; K 34 for the shape no matrix-core kernel takes; B 2 / 3 / 5 around the GEMV threshold."""
import ctypes

import pytest
import torch

from test_dispatch_contract import (ALIGNMENT, BF16, DEF, DTYPE, EXACT, F16, F32, FP8, I8, NULLP, OK, PRECISION, SHAPE,
                                    WORKSPACE, _TUNE)

pytestmark = pytest.mark.gpu
E, T, K, N = 2, 8, 64, 16
BIG_E = 70000
N_ = None


@pytest.fixture(scope="module")
def b():
    """Device buffers as integer addresses (and what keeps them alive)."""
    from fused_int4_amd import _native
    lib = _native.lib()
    for name, (res, args) in _TUNE.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    dev = "cuda"
    torch.manual_seed(0)
    need = max(lib.fql_moe_workspace_bytes(E, T, K, N, DEF), lib.fql_moe_workspace_bytes(E, T, K, N, FP8),
               lib.fql_linear_workspace_bytes(5, K, N, DEF))
    keep = dict(
        x=torch.rand(T, 2 * K, device=dev),                                  # [T][K] rows, or [T][2K] gate|up
        x16=torch.rand(T, 2 * K + 8, device=dev).to(torch.bfloat16),
        x8=torch.randint(0, 256, (T * K + 64,), dtype=torch.uint8, device=dev),
        asc=torch.rand(T, device=dev),
        P=torch.randint(0, 256, (E * N * K // 2 + 64,), dtype=torch.uint8, device=dev),
        S=torch.rand(E, N, device=dev) + 0.5, Z=torch.rand(E, N, device=dev), bias=torch.rand(E, N, device=dev),
        out=torch.zeros(T, N, device=dev),
        tpe=torch.tensor([5, 3], dtype=torch.int32, device=dev), offs=torch.tensor([0, 5], dtype=torch.int32, device=dev),
        tpe_big=torch.zeros(BIG_E, dtype=torch.int32, device=dev), offs_big=torch.zeros(BIG_E, dtype=torch.int32, device=dev),
        ri=torch.arange(T, dtype=torch.int32, device=dev), rw=torch.rand(T, device=dev),
        ws=torch.zeros(need + 64, dtype=torch.uint8, device=dev),
        limbs=torch.zeros((1 << 17) + 64, dtype=torch.int8, device=dev), delta=torch.rand(3, T, device=dev),
        rowsum=torch.zeros(2, 3, T, dtype=torch.int32, device=dev),
        slots=torch.zeros(T, dtype=torch.int32, device=dev),
    )
    d = {k: v.data_ptr() for k, v in keep.items()}
    assert d["ws"] % 16 == 0 and d["P"] % 16 == 0 and d["limbs"] % 16 == 0
    d.update(lib=lib, keep=keep, need=need)
    torch.cuda.synchronize()
    return d


def W(b, off=0, short=0):
    """workspace, workspace_bytes, stream"""
    return (b["ws"] + off, b["need"] - short, N_)


WEIGHTS = lambda b, off=0: (b["P"] + off, b["S"], b["Z"])                       # noqa: E731

ROWS = [
    # ---- fql_linear_fwd_f32(x, packed, scales, zps, out, B, K, N, precision, ...): fp8 exists on the matrix-core path only
    ("linear/f8-gemv", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 2, K, N, FP8, *W(b))), PRECISION),
    ("linear/f8-K34", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, 34, N, FP8, *W(b))), PRECISION),
    ("linear/f8-weights-align", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b, 8), b["out"], 5, K, N, FP8, *W(b))), PRECISION),
    ("linear/f8-B3-no-ws", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 3, K, N, FP8, N_, 0, N_)), WORKSPACE),
    ("linear/f8-B5-no-ws", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, K, N, FP8, N_, 0, N_)), WORKSPACE),
    ("linear/f8-ws-small", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, K, N, FP8, b["ws"], 64, N_)), WORKSPACE),
    ("linear/B5-no-ws", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, K, N, DEF, N_, 0, N_)), WORKSPACE),
    ("linear/B5-ws-align", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, K, N, DEF, *W(b, 8))), WORKSPACE),
    ("linear/B5-ws-small", lambda b: ("fql_linear_fwd_f32", (b["x"], *WEIGHTS(b), b["out"], 5, K, N, DEF, b["ws"], 64, N_)), WORKSPACE),
    ("linear/K0-bias", lambda b: ("fql_linear_bias_fwd_f32", (b["x"], *WEIGHTS(b), b["bias"], b["out"], 5, 0, N, DEF, *W(b))), SHAPE),
    # ---- fql_linear_fwd(x, in_dtype, packed, scales, zps, out, out_dtype, B, K, N, precision, ...): 16-bit I/O, same path only
    ("linear16/gemv", lambda b: ("fql_linear_fwd", (b["x16"], BF16, *WEIGHTS(b), b["out"], F32, 2, K, N, DEF, *W(b))), DTYPE),
    ("linear16/K34", lambda b: ("fql_linear_fwd", (b["x16"], BF16, *WEIGHTS(b), b["out"], F32, 5, 34, N, DEF, *W(b))), DTYPE),
    ("linear16/weights-align", lambda b: ("fql_linear_fwd", (b["x"], F32, *WEIGHTS(b, 4), b["out"], F16, 5, K, N, DEF, *W(b))), DTYPE),
    ("linear16/B3-no-ws", lambda b: ("fql_linear_fwd", (b["x16"], BF16, *WEIGHTS(b), b["out"], F32, 3, K, N, DEF, N_, 0, N_)), WORKSPACE),
    ("linear16/ws-small", lambda b: ("fql_linear_bias_fwd", (b["x16"], BF16, *WEIGHTS(b), b["bias"], b["out"], F32, 5, K, N, DEF, *W(b, 0, b["need"] - 64))), WORKSPACE),
    # ---- fql_moe_fwd_f32(packed, scales, zps, inputs, tpe, offs, out, E, T, K, N, precision, ...)
    ("moe/null-weights", lambda b: ("fql_moe_fwd_f32", (N_, b["S"], b["Z"], b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, *W(b))), NULLP),
    ("moe/null-table", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], N_, b["out"], E, T, K, N, DEF, *W(b))), NULLP),
    ("moe/E-big", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe_big"], b["offs_big"], b["out"], BIG_E, T, K, N, DEF, *W(b))), SHAPE),
    ("moe/no-ws", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, N_, 0, N_)), WORKSPACE),
    ("moe/ws-align", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, I8, *W(b, 4))), WORKSPACE),
    ("moe/ws-small", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF,
                                                    b["ws"], b["lib"].fql_moe_workspace_bytes(E, T, K, N, DEF) - 1, N_)), WORKSPACE),
    ("moe/f8-K34", lambda b: ("fql_moe_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, 34, N, FP8, *W(b))), ALIGNMENT),
    # ---- fql_moe_gather_fwd_f32(packed, scales, zps, tokens, row_index, n_tokens, tpe, offs, out, E, T, K, N, precision, ...)
    ("gather/n-src", lambda b: ("fql_moe_gather_fwd_f32", (*WEIGHTS(b), b["x"], b["ri"], 0, b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, *W(b))), SHAPE),
    ("gather/K34", lambda b: ("fql_moe_gather_fwd_f32", (*WEIGHTS(b), b["x"], b["ri"], T, b["tpe"], b["offs"], b["out"], E, T, 34, N, DEF, *W(b))), ALIGNMENT),
    ("gather/weights-align", lambda b: ("fql_moe_gather_fwd_f32", (*WEIGHTS(b, 8), b["x"], b["ri"], T, b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, *W(b))), ALIGNMENT),
    # ---- fql_moe_gather_scaled_fwd_f32(packed, scales, zps, tokens, row_index, n_tokens, row_weight, tpe, offs, out, E, ...)
    ("scaled/null-weight", lambda b: ("fql_moe_gather_scaled_fwd_f32", (*WEIGHTS(b), b["x"], b["ri"], T, N_, b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, *W(b))), NULLP),
    ("scaled/f8", lambda b: ("fql_moe_gather_scaled_fwd_f32", (*WEIGHTS(b), b["x"], b["ri"], T, b["rw"], b["tpe"], b["offs"], b["out"], E, T, K, N, FP8, *W(b))), PRECISION),
    ("scaled/K34", lambda b: ("fql_moe_gather_scaled_fwd_f32", (*WEIGHTS(b), b["x"], b["ri"], T, b["rw"], b["tpe"], b["offs"], b["out"], E, T, 34, N, DEF, *W(b))), ALIGNMENT),
    # ---- fql_moe_fwd(packed, scales, zps, inputs, in_dtype, tpe, offs, out, out_dtype, E, T, K, N, precision, ...)
    ("moe16/E-big", lambda b: ("fql_moe_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe_big"], b["offs_big"], b["out"], F32, BIG_E, T, K, N, DEF, *W(b))), SHAPE),
    ("moe16/K34", lambda b: ("fql_moe_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe"], b["offs"], b["out"], F32, E, T, 34, N, DEF, *W(b))), DTYPE),
    ("moe16/weights-align", lambda b: ("fql_moe_fwd", (*WEIGHTS(b, 2), b["x16"], BF16, b["tpe"], b["offs"], b["out"], F32, E, T, K, N, DEF, *W(b))), DTYPE),
    ("moe16/no-ws", lambda b: ("fql_moe_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe"], b["offs"], b["out"], F32, E, T, K, N, DEF, N_, 0, N_)), WORKSPACE),
    # ---- fql_moe_fwd_f8(packed, scales, zps, inputs, act_scales, tpe, offs, out, out_dtype, E, T, K, N, ...) / fql_linear_fwd_f8
    ("f8/null-offs", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe"], N_, b["out"], F32, E, T, K, N, *W(b))), NULLP),
    ("f8/null-x", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), N_, b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, K, N, *W(b))), NULLP),
    ("f8/E-big", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe_big"], b["offs_big"], b["out"], F32, BIG_E, T, K, N, *W(b))), SHAPE),
    ("f8/K34", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, 34, N, *W(b))), ALIGNMENT),
    ("f8/weights-align", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b, 8), b["x8"], b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, K, N, *W(b))), ALIGNMENT),
    ("f8/no-ws", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, K, N, N_, 0, N_)), WORKSPACE),
    ("f8/ws-align", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, K, N, *W(b, 8))), WORKSPACE),
    ("f8/ws-small", lambda b: ("fql_moe_fwd_f8", (*WEIGHTS(b), b["x8"], b["asc"], b["tpe"], b["offs"], b["out"], F32, E, T, K, N,
                                                  b["ws"], b["lib"].fql_moe_workspace_bytes(E, T, K, N, FP8) - 1, N_)), WORKSPACE),
    ("f8-linear/K34", lambda b: ("fql_linear_fwd_f8", (b["x8"], b["asc"], *WEIGHTS(b), b["out"], F32, 5, 34, N, *W(b))), ALIGNMENT),
    ("f8-linear/no-ws", lambda b: ("fql_linear_fwd_f8", (b["x8"], b["asc"], *WEIGHTS(b), b["out"], F32, 2, K, N, N_, 0, N_)), WORKSPACE),
    # ---- fql_moe_group_fwd_f32(packed, scales, zps, inputs, tpe, offs, out, E, T, K, N, group, stream) and its workspace form
    ("group/null-offs", lambda b: ("fql_moe_group_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], N_, b["out"], E, T, K, N, 32, N_)), NULLP),
    ("group/E-big", lambda b: ("fql_moe_group_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe_big"], b["offs_big"], b["out"], BIG_E, T, K, N, 32, N_)), SHAPE),
    ("group-ws/E-big", lambda b: ("fql_moe_group_ws_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe_big"], b["offs_big"], b["out"], BIG_E, T, K, N, 32, DEF, *W(b))), SHAPE),
    # ---- fql_moe_gated_fwd_f32(packed, scales, zps, gate_up, tpe, offs, out, E, T, K, N, precision, ...)
    ("gated/pair-offs", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], N_, b["out"], E, T, K, N, DEF, *W(b))), NULLP),
    ("gated/pair-tpe", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], N_, b["offs"], b["out"], E, T, K, N, DEF, *W(b))), NULLP),
    ("gated/no-table-E2", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], N_, N_, b["out"], E, T, K, N, DEF, *W(b))), SHAPE),
    ("gated/E-big", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe_big"], b["offs_big"], b["out"], BIG_E, T, K, N, DEF, *W(b))), SHAPE),
    ("gated/K34", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, 34, N, DEF, *W(b))), ALIGNMENT),
    ("gated/weights-align", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b, 8), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, *W(b))), ALIGNMENT),
    ("gated/no-ws", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, N_, 0, N_)), WORKSPACE),
    ("gated/ws-small", lambda b: ("fql_moe_gated_fwd_f32", (*WEIGHTS(b), b["x"], b["tpe"], b["offs"], b["out"], E, T, K, N, DEF,
                                                            b["ws"], b["lib"].fql_moe_workspace_bytes(E, T, K, N, DEF) - 1, N_)), WORKSPACE),
    # ---- fql_moe_gated_fwd(packed, scales, zps, gate_up, in_dtype, tpe, offs, out, out_dtype, E, T, K, N, precision, ...)
    ("gated16/pair", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe"], N_, b["out"], F32, E, T, K, N, DEF, *W(b))), NULLP),
    ("gated16/no-table-E2", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"], BF16, N_, N_, b["out"], F32, E, T, K, N, DEF, *W(b))), SHAPE),
    ("gated16/E-big", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe_big"], b["offs_big"], b["out"], F32, BIG_E, T, K, N, DEF, *W(b))), SHAPE),
    ("gated16/K34", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"], BF16, b["tpe"], b["offs"], b["out"], F32, E, T, 34, N, DEF, *W(b))), ALIGNMENT),
    ("gated16/x-align", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"] + 1, BF16, b["tpe"], b["offs"], b["out"], F32, E, T, K, N, DEF, *W(b))), ALIGNMENT),
    ("gated16/no-ws", lambda b: ("fql_moe_gated_fwd", (*WEIGHTS(b), b["x16"], F16, b["tpe"], b["offs"], b["out"], F32, E, T, K, N, DEF, N_, 0, N_)), WORKSPACE),
    # ---- fql_act_quant_f32(x, limbs, delta, rowsum, tpe, offs, E, T, K, precision, stream)
    ("act/pair", lambda b: ("fql_act_quant_f32", (b["x"], b["limbs"], b["delta"], b["rowsum"], b["tpe"], N_, E, T, K, DEF, N_)), NULLP),
    ("act/no-table-E2", lambda b: ("fql_act_quant_f32", (b["x"], b["limbs"], b["delta"], b["rowsum"], N_, N_, E, T, K, DEF, N_)), SHAPE),
    ("act/limbs-align", lambda b: ("fql_act_quant_f32", (b["x"], b["limbs"] + 8, b["delta"], b["rowsum"], b["tpe"], b["offs"], E, T, K, DEF, N_)), ALIGNMENT),
    # ---- fql_gemm_i8_f32(limbs, delta, rowsum, packed, scales, zps, tpe, offs, out, E, T, K, N, precision, stream, scratch, bytes)
    ("gemm/pair", lambda b: ("fql_gemm_i8_f32", (b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), N_, b["offs"], b["out"], E, T, K, N, DEF, N_, N_, 0)), NULLP),
    ("gemm/no-table-E2", lambda b: ("fql_gemm_i8_f32", (b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), N_, N_, b["out"], E, T, K, N, DEF, N_, N_, 0)), SHAPE),
    ("gemm/K34", lambda b: ("fql_gemm_i8_f32", (b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), b["tpe"], b["offs"], b["out"], E, T, 34, N, DEF, N_, N_, 0)), ALIGNMENT),
    ("gemm/weights-align", lambda b: ("fql_gemm_i8_f32", (b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b, 8), b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, N_, N_, 0)), ALIGNMENT),
    ("gemm/limbs-align", lambda b: ("fql_gemm_i8_f32", (b["limbs"] + 4, b["delta"], b["rowsum"], *WEIGHTS(b), b["tpe"], b["offs"], b["out"], E, T, K, N, DEF, N_, N_, 0)), ALIGNMENT),
    # ---- fql_tune_gemm_i8(cfg, limbs, delta, rowsum, packed, scales, zps, tpe, offs, out, out_dtype, bias, row_weight, E, ...):
    #      the row weight must BE the plane behind delta's sets (2 at 3 limbs, 1 at one limb)
    ("tune/row-weight-elsewhere", lambda b: ("fql_tune_gemm_i8", (0, b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), b["tpe"], b["offs"], b["out"], F32,
                                                                  N_, b["rw"], E, T, K, N, EXACT, N_, N_, 0)), ALIGNMENT),
    ("tune/row-weight-plane-of-3-limbs", lambda b: ("fql_tune_gemm_i8", (1, b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), b["tpe"], b["offs"], b["out"], F32,
                                                                         N_, b["delta"] + 2 * T * 4, E, T, K, N, I8, N_, N_, 0)), ALIGNMENT),
    ("tune/cfg-of-other-limbs", lambda b: ("fql_tune_gemm_i8", (12, b["limbs"], b["delta"], b["rowsum"], *WEIGHTS(b), b["tpe"], b["offs"], b["out"], F32,
                                                                N_, N_, E, T, K, N, DEF, N_, N_, 0)), SHAPE),
    # ---- fql_route_plan_i32(expert_of_slot, n_slots, top_k, E, counts, offsets, token_of_sorted, pos_of_slot, stream)
    ("route/null-slots", lambda b: ("fql_route_plan_i32", (N_, T, 2, E, b["tpe"], b["offs"], b["slots"], b["slots"], N_)), NULLP),
    # ---- fql_combine_bwd_f32(grad_out, y, pos_of_slot, weights, grad_y, grad_weights, T, top_k, N, rows, stream)
    ("combine-bwd/null-grad", lambda b: ("fql_combine_bwd_f32", (N_, N_, b["slots"], N_, b["out"], N_, 4, 2, N, T, N_)), NULLP),
    ("combine-bwd/null-y", lambda b: ("fql_combine_bwd_f32", (b["x"], N_, b["slots"], N_, b["out"], b["rw"], 4, 2, N, T, N_)), NULLP),
    ("combine-bwd/nothing-to-do", lambda b: ("fql_combine_bwd_f32", (N_, N_, b["slots"], N_, N_, N_, 4, 2, 0, T, N_)), OK),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_return_code(b, row):
    _, make, expected = ROWS[row]
    name, args = make(b)
    fn = getattr(b["lib"], name)
    with torch.cuda.device(0):
        assert fn(*args) == expected, name
