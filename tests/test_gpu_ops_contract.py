"""What the operator boundary (ops.py) refuses: one row per (op, bad call, exception type, message regex).

``test_refusals`` is the characterisation of the boundary: every row raised the same way before the shared checkers
(``_expert_table``, ``_check_weights``, ``_check_group_weights``, ``_check_bias``) replaced the pasted ones, so the table
can be run unchanged on an older checkout (``-k refusals``).  ``test_closed_doors`` is the second group: tensors that
used to reach a kernel unchecked (a CPU tensor became a host pointer).  Never run that group on a checkout without the
shared checkers.

Shapes are a few rows; no row launches a kernel (every call raises before its launch)."""
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import ops

pytestmark = pytest.mark.gpu
T, K, N, E, R = 8, 64, 16, 2, 4
H, F = 64, 32                                # gated FFN: hidden and ffn dims
f16, f64, i32 = torch.float16, torch.float64, torch.int32


@pytest.fixture(scope="module")
def g():
    """The good arguments, on the GPU; a row replaces one of them."""
    torch.manual_seed(0)
    dev = "cuda"
    u8 = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device=dev)       # noqa: E731
    f = lambda *s: torch.rand(s, device=dev) + 0.5                                 # noqa: E731
    d = dict(
        x=f(T, K), P=u8(N, K // 2), s=f(N), z=f(N), bias=f(N),
        P3=u8(E, N, K // 2), S=f(E, N), Z=f(E, N), Sg=f(E, N, 2), Zg=f(E, N, 2), sg=f(N, 2), zg=f(N, 2),
        tpe=torch.tensor([5, 3], dtype=i32, device=dev), offs=torch.tensor([0, 5], dtype=i32, device=dev),
        tpe3=torch.tensor([5, 3, 0], dtype=i32, device=dev), tpe1=torch.tensor([8], dtype=i32, device=dev),
        ri=torch.arange(T, dtype=i32, device=dev), rw=f(T), gu=f(T, 2 * K), gy=f(T, N),
        x8=u8(T, K), asc=f(T), A=f(E, R, K), B=f(E, N, R), A1=f(R, K), B1=f(N, R), v=f(T, R), A5=f(E, 5, K),
        y=f(T, N), pos=torch.arange(T, dtype=i32, device=dev), w=f(T // 2, 2), dh=f(T, K), gy4=f(T // 2, N),
        # gated FFN layer
        gup=u8(E, 2 * F, H // 2), gus=f(E, 2 * F), guz=f(E, 2 * F), dp=u8(E, H, F // 2), ds=f(E, H), dz=f(E, H),
        Agu=f(E, R, H), Bgu=f(E, 2 * F, R), Ad=f(E, R, F), Bd=f(E, H, R),
        # phase-1 outputs of act_quant at precision "exact": 2 sets, 3 limbs
        limbs=torch.zeros(1 << 16, dtype=torch.int8, device=dev), delta=f(2, T),
        rowsum=torch.zeros(2, 3, T, dtype=i32, device=dev),
    )
    return d


def ffn(g, o, **kw):
    a = dict(gup=g["gup"], gus=g["gus"], guz=g["guz"], dp=g["dp"], ds=g["ds"], dz=g["dz"], x=g["x"], Agu=g["Agu"],
             Bgu=g["Bgu"], Ad=g["Ad"], Bd=g["Bd"], tpe=g["tpe"], offs=g["offs"], precision="default",
             activation_dtype=None)
    a.update(kw)
    return o.moe_ffn_lora_forward(a["gup"], a["gus"], a["guz"], a["dp"], a["ds"], a["dz"], a["x"], a["Agu"], a["Bgu"],
                                  a["Ad"], a["Bd"], 2.0, a["tpe"], a["offs"], precision=a["precision"],
                                  activation_dtype=a["activation_dtype"])


RT, VE = RuntimeError, ValueError
TABLE = "tokens_per_expert|input_offsets"
REFUSALS = [
    # ---- linear_forward: the reference's checks, in its words
    ("linear/cpu", lambda g, o: o.linear_forward(g["x"].cpu(), g["P"], g["s"], g["z"]), RT, "input must be a CUDA tensor"),
    ("linear/dtype", lambda g, o: o.linear_forward(g["x"].half(), g["P"], g["s"], g["z"]), RT, "input must be float32"),
    ("linear/packed-dtype", lambda g, o: o.linear_forward(g["x"], g["P"].float(), g["s"], g["z"]), RT, "packed_weights must be uint8"),
    ("linear/scales-dtype", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"].half(), g["z"]), RT, "scales must be float32"),
    ("linear/zps-dtype", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"], g["z"].half()), RT, "zero_points must be float32"),
    ("linear/noncontig", lambda g, o: o.linear_forward(g["x"].t(), g["P"], g["s"], g["z"]), RT, "input must be contiguous"),
    ("linear/rank", lambda g, o: o.linear_forward(g["x"][None], g["P"], g["s"], g["z"]), RT, "input must be 1-D or 2-D"),
    ("linear/K", lambda g, o: o.linear_forward(g["x"][:, :32].contiguous(), g["P"], g["s"], g["z"]), RT, "packed_weights dim 1 must be input_dim / 2"),
    ("linear/scales-len", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"][:N - 1], g["z"]), RT, "output_dim elements"),
    ("linear/bias-len", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"], g["z"], bias=g["bias"][:N - 1]), RT, "bias"),
    ("linear/bias-dtype", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"], g["z"], bias=g["bias"].half()), RT, "bias"),
    ("linear/precision", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"], g["z"], precision="bf16"), VE, "precision"),
    ("linear-group/shape", lambda g, o: o.linear_forward(g["x"], g["P"], g["sg"], g["zg"][:, :1]), RT, "per-group scales"),
    ("linear-group/odd", lambda g, o: o.linear_forward(g["x"], g["P"], g["s"][:, None].expand(N, K), g["z"][:, None].expand(N, K)), RT, "group_size must be even"),
    ("linear-group/bias-len", lambda g, o: o.linear_forward(g["x"], g["P"], g["sg"], g["zg"], bias=g["bias"][:N - 1]), RT, "bias"),
    # ---- linear_forward_any
    ("linear_any/dtype", lambda g, o: o.linear_forward_any(g["x"].to(i32), g["P"], g["s"], g["z"]), RT, "float32, float16 or bfloat16"),
    ("linear_any/out_dtype", lambda g, o: o.linear_forward_any(g["x"], g["P"], g["s"], g["z"], out_dtype=f64), RT, "float32, float16 or bfloat16"),
    ("linear_any/K", lambda g, o: o.linear_forward_any(g["x"][:, :32].half(), g["P"], g["s"], g["z"]), RT, "packed_weights dim 1"),
    ("linear_any/rank", lambda g, o: o.linear_forward_any(g["x"].half()[None], g["P"], g["s"], g["z"]), RT, "input must be 1-D or 2-D"),
    ("linear_any/scales-len", lambda g, o: o.linear_forward_any(g["x"].half(), g["P"], g["s"][:N - 1], g["z"]), RT, "scales"),
    ("linear_any/bias-len", lambda g, o: o.linear_forward_any(g["x"].half(), g["P"], g["s"], g["z"], bias=g["bias"][:N - 1]), RT, "bias"),
    # ---- moe_forward / moe_forward_any
    ("moe/cpu", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"].cpu(), None, g["tpe"], g["offs"]), RT, "inputs"),
    ("moe/dtype", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"].half(), None, g["tpe"], g["offs"]), RT, "inputs must be float32"),
    ("moe/rank", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"][None], None, g["tpe"], g["offs"]), RT, "inputs"),
    ("moe/packed-rank", lambda g, o: o.moe_forward(g["P"], g["S"], g["Z"], g["x"], None, g["tpe"], g["offs"]), RT, "packed_weights"),
    ("moe/K", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"][:, :32].contiguous(), None, g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("moe/scales-shape", lambda g, o: o.moe_forward(g["P3"], g["S"][:, :N - 1], g["Z"], g["x"], None, g["tpe"], g["offs"]), RT, "scales"),
    ("moe/scales-dtype", lambda g, o: o.moe_forward(g["P3"], g["S"].half(), g["Z"], g["x"], None, g["tpe"], g["offs"]), RT, "scales"),
    ("moe/table+1", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe3"], g["offs"]), RT, TABLE),
    ("moe/table-1", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe"], g["offs"][:1]), RT, TABLE),
    ("moe/table-cpu", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe"].cpu(), g["offs"]), RT, "tokens_per_expert"),
    ("moe/precision", lambda g, o: o.moe_forward(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe"], g["offs"], precision=7), VE, "precision"),
    ("moe_any/dtype", lambda g, o: o.moe_forward_any(g["P3"], g["S"], g["Z"], g["x"].to(i32), None, g["tpe"], g["offs"]), RT, "float32, float16 or bfloat16"),
    ("moe_any/out_dtype", lambda g, o: o.moe_forward_any(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe"], g["offs"], out_dtype=f64), RT, "float32, float16 or bfloat16"),
    ("moe_any/K", lambda g, o: o.moe_forward_any(g["P3"], g["S"], g["Z"], g["x"][:, :32].half(), None, g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("moe_any/table+1", lambda g, o: o.moe_forward_any(g["P3"], g["S"], g["Z"], g["x"].half(), None, g["tpe3"], g["offs"]), RT, TABLE),
    ("moe_any/scales-shape", lambda g, o: o.moe_forward_any(g["P3"], g["S"][:, :N - 1], g["Z"], g["x"].half(), None, g["tpe"], g["offs"]), RT, "scales"),
    # ---- moe_group_forward
    ("moe_group/dtype", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"], g["x"].half(), g["tpe"], g["offs"]), RT, "inputs"),
    ("moe_group/rank", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"], g["x"][None], g["tpe"], g["offs"]), RT, "inputs"),
    ("moe_group/K", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"], g["x"][:, :32].contiguous(), g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("moe_group/scales-shape", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"][:, :, :1], g["x"], g["tpe"], g["offs"]), RT, "per-group scales"),
    ("moe_group/scales-dtype", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"].half(), g["Zg"], g["x"], g["tpe"], g["offs"]), RT, "scales"),
    ("moe_group/odd", lambda g, o: o.moe_group_forward(g["P3"], g["S"][:, :, None].expand(E, N, K), g["Z"][:, :, None].expand(E, N, K), g["x"], g["tpe"], g["offs"]), RT, "group_size must be even"),
    ("moe_group/table+1", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"], g["x"], g["tpe3"], g["offs"]), RT, TABLE),
    ("moe_group/table-1", lambda g, o: o.moe_group_forward(g["P3"], g["Sg"], g["Zg"], g["x"], g["tpe"], g["offs"][:1]), RT, TABLE),
    # ---- moe_gather_forward
    ("gather/dtype", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"].half(), g["ri"], g["tpe"], g["offs"]), RT, "tokens must be float32"),
    ("gather/rank", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"][None], g["ri"], g["tpe"], g["offs"]), RT, "tokens must be float32"),
    ("gather/K", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"][:, :32].contiguous(), g["ri"], g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("gather/K%32", lambda g, o: o.moe_gather_forward(g["P3"][:, :, :24], g["S"], g["Z"], g["x"][:, :48].contiguous(), g["ri"], g["tpe"], g["offs"]), RT, "% 32"),
    ("gather/scales-shape", lambda g, o: o.moe_gather_forward(g["P3"], g["S"][:, :N - 1], g["Z"], g["x"], g["ri"], g["tpe"], g["offs"]), RT, "scales"),
    ("gather/table+1", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"], g["ri"], g["tpe3"], g["offs"]), RT, TABLE),
    ("gather/table-1", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"], g["ri"], g["tpe"], g["offs"][:1]), RT, TABLE),
    ("gather/row_weight", lambda g, o: o.moe_gather_forward(g["P3"], g["S"], g["Z"], g["x"], g["ri"], g["tpe"], g["offs"], row_weight=g["rw"][:T - 1]), RT, "row_weight"),
    # ---- moe_gated_forward
    ("gated/dtype", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"].to(i32), g["tpe"], g["offs"]), RT, "gate_up"),
    ("gated/rank", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"][0], g["tpe"], g["offs"]), RT, "gate_up"),
    ("gated/K", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"][:, :K].contiguous(), g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("gated/K%32", lambda g, o: o.moe_gated_forward(g["P3"][:, :, :8], g["S"], g["Z"], g["gu"][:, :32].contiguous(), g["tpe"], g["offs"]), RT, "% 32"),
    ("gated/out_dtype", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"], g["tpe"], g["offs"], out_dtype=f64), RT, "out_dtype"),
    ("gated/table+1", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"], g["tpe3"], g["offs"]), RT, TABLE),
    ("gated/table-1", lambda g, o: o.moe_gated_forward(g["P3"], g["S"], g["Z"], g["gu"], g["tpe"], g["offs"][:1]), RT, TABLE),
    ("gated/scales-shape", lambda g, o: o.moe_gated_forward(g["P3"], g["S"][:, :N - 1], g["Z"], g["gu"], g["tpe"], g["offs"]), RT, "scales"),
    # ---- routing, quantisers, phase 1 / 2
    ("route_plan/rank", lambda g, o: o.route_plan(g["pos"], E), RT, "expert_indices"),
    ("route_plan/experts", lambda g, o: o.route_plan(g["pos"].view(T // 2, 2), 129), RT, "128 experts"),
    ("combine/dtype", lambda g, o: o.combine(g["y"].half(), g["pos"], g["w"]), RT, "y must be"),
    ("combine/rank", lambda g, o: o.combine(g["y"][0], g["pos"], g["w"]), RT, "y must be"),
    ("combine/top_k", lambda g, o: o.combine(g["y"], g["pos"], None), RT, "top_k"),
    ("combine/tokens", lambda g, o: o.combine(g["y"], torch.zeros(65536, dtype=i32, device="cuda"), torch.ones(65536, 1, device="cuda")), RT, "65535"),
    ("regroup/rank", lambda g, o: o.regroup_index(g["pos"], T), RT, "recv_counts"),
    ("quantize_rows/dtype", lambda g, o: o.quantize_rows(g["x"].half()), RT, "weight must be"),
    ("quantize_rows/rank", lambda g, o: o.quantize_rows(g["x"][None]), RT, "weight must be"),
    ("quantize_tensor/dtype", lambda g, o: o.quantize_tensor(g["x"].half()), RT, "weight must be"),
    ("quantize_tensor/rank", lambda g, o: o.quantize_tensor(g["x"][0]), RT, "weight must be"),
    ("unpack/dtype", lambda g, o: o.unpack_nibbles(g["x"]), RT, "packed must be"),
    ("dequantize/cpu", lambda g, o: o.dequantize_forward(g["P"].cpu(), g["s"], g["z"]), RT, "packed_weights"),
    ("act_quant/dtype", lambda g, o: o.act_quant(g["x"].half()), RT, "x must be"),
    ("act_quant/rank", lambda g, o: o.act_quant(g["x"][0]), RT, "x must be"),
    ("act_quant/precision", lambda g, o: o.act_quant(g["x"], precision="bf16"), VE, "precision"),
    ("gemm_i8/limb-count", lambda g, o: o.gemm_i8(g["limbs"], g["delta"], g["rowsum"], g["P"], g["s"], g["z"], precision="int8"), RT, "limb count"),
    ("gemm_i8/limbs-size", lambda g, o: o.gemm_i8(g["limbs"][:16], g["delta"], g["rowsum"], g["P"], g["s"], g["z"], precision="exact"), RT, "limbs"),
    ("tune_gemm_i8/out_dtype", lambda g, o: o.tune_gemm_i8(1, g["limbs"], g["delta"], g["rowsum"], g["P"], g["s"], g["z"], None, None, g["y"], 1, T, K, N, "exact", out_dtype=f16), RT, "out must be"),
    ("tune_gemm_i8/bias", lambda g, o: o.tune_gemm_i8(1, g["limbs"], g["delta"], g["rowsum"], g["P"], g["s"], g["z"], None, None, g["y"], 1, T, K, N, "exact", bias=g["bias"][:N - 1]), RT, "bias"),
    # ---- fp8 activations
    ("moe_fp8/dtype", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x"], None, g["tpe"], g["offs"]), RT, "float8_e4m3fn"),
    ("moe_fp8/rank", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"][0], None, g["tpe"], g["offs"]), RT, "inputs"),
    ("moe_fp8/K%32", lambda g, o: o.moe_forward_fp8(g["P3"][:, :, :24], g["S"], g["Z"], g["x8"][:, :48], None, g["tpe"], g["offs"]), RT, "% 32"),
    ("moe_fp8/K", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"][:, :32], None, g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("moe_fp8/act_scales", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"], g["asc"][:3], g["tpe"], g["offs"]), RT, "one element per row"),
    ("moe_fp8/out_dtype", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"], None, g["tpe"], g["offs"], out_dtype=f64), RT, "float32, float16 or bfloat16"),
    ("moe_fp8/scales-shape", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"][:, :N - 1], g["Z"], g["x8"], None, g["tpe"], g["offs"]), RT, "scales"),
    ("moe_fp8/table+1", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"], None, g["tpe3"], g["offs"]), RT, TABLE),
    ("moe_fp8/table-1", lambda g, o: o.moe_forward_fp8(g["P3"], g["S"], g["Z"], g["x8"], None, g["tpe"], g["offs"][:1]), RT, TABLE),
    ("linear_fp8/dtype", lambda g, o: o.linear_forward_fp8(g["x"], None, g["P"], g["s"], g["z"]), RT, "float8_e4m3fn"),
    ("linear_fp8/rank", lambda g, o: o.linear_forward_fp8(g["x8"][0], None, g["P"], g["s"], g["z"]), RT, "x_e4m3"),
    ("linear_fp8/K%32", lambda g, o: o.linear_forward_fp8(g["x8"][:, :48], None, g["P"][:, :24], g["s"], g["z"]), RT, "% 32"),
    ("linear_fp8/K", lambda g, o: o.linear_forward_fp8(g["x8"][:, :32], None, g["P"], g["s"], g["z"]), RT, "packed_weights dim 1"),
    ("linear_fp8/act_scales", lambda g, o: o.linear_forward_fp8(g["x8"], g["asc"][:3], g["P"], g["s"], g["z"]), RT, "one element per row"),
    ("linear_fp8/out_dtype", lambda g, o: o.linear_forward_fp8(g["x8"], None, g["P"], g["s"], g["z"], out_dtype=f64), RT, "float32, float16 or bfloat16"),
    ("linear_fp8/scales-len", lambda g, o: o.linear_forward_fp8(g["x8"], None, g["P"], g["s"][:N - 1], g["z"]), RT, "scales"),
    # ---- backward ops
    ("linear_bwd/dtype", lambda g, o: o.linear_backward_input(g["gy"].to(i32), g["P"], g["s"], g["z"]), RT, "grad_out"),
    ("linear_bwd/rank", lambda g, o: o.linear_backward_input(g["gy"][0], g["P"], g["s"], g["z"]), RT, "grad_out"),
    ("linear_bwd/N", lambda g, o: o.linear_backward_input(g["gy"][:, :N - 1].contiguous(), g["P"], g["s"], g["z"]), RT, "grad_out"),
    ("linear_bwd/scales-len", lambda g, o: o.linear_backward_input(g["gy"], g["P"], g["s"][:N - 1], g["z"]), RT, "scales"),
    ("linear_bwd/out_dtype", lambda g, o: o.linear_backward_input(g["gy"], g["P"], g["s"], g["z"], out_dtype=f64), RT, "out_dtype"),
    ("moe_bwd/dtype", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"].to(i32), g["tpe"], g["offs"]), RT, "grad_out"),
    ("moe_bwd/rank", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"][0], g["tpe"], g["offs"]), RT, "grad_out"),
    ("moe_bwd/N", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"][:, :N - 1].contiguous(), g["tpe"], g["offs"]), RT, "grad_out"),
    ("moe_bwd/scales-shape", lambda g, o: o.moe_backward_input(g["P3"], g["S"][:, :N - 1], g["Z"], g["gy"], g["tpe"], g["offs"]), RT, "scales"),
    ("moe_bwd/out_dtype", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"], g["tpe"], g["offs"], out_dtype=f64), RT, "out_dtype"),
    # ---- the two torch-only ops: whatever torch raises
    ("group_bwd/N", lambda g, o: o.group_backward_input(g["gy"][:, :N - 1].contiguous(), g["P"], g["sg"], g["zg"]), RT, "shapes|size"),
    ("quantize_fp8/rank", lambda g, o: o.quantize_activations_fp8(g["x"][0]), IndexError, "[Dd]imension"),
    # ---- LoRA kernels
    ("shrink/dtype", lambda g, o: o.lora_shrink(g["x"].to(i32), g["A"], "rc", g["tpe"], g["offs"]), RT, "input must be a"),
    ("shrink/rank", lambda g, o: o.lora_shrink(g["x"][0], g["A1"]), RT, "input must be a"),
    ("shrink/weight-dtype", lambda g, o: o.lora_shrink(g["x"], g["A"].half(), "rc", g["tpe"], g["offs"]), RT, "weight must be a float32"),
    ("shrink/K", lambda g, o: o.lora_shrink(g["x"][:, :32].contiguous(), g["A"], "rc", g["tpe"], g["offs"]), RT, "columns"),
    ("shrink/lora-rank", lambda g, o: o.lora_shrink(g["x"], g["A5"], "rc", g["tpe"], g["offs"]), RT, "LoRA rank"),
    ("shrink/layout", lambda g, o: o.lora_shrink(g["x"], g["A"], "xx", g["tpe"], g["offs"]), VE, "layout"),
    ("shrink/table+1", lambda g, o: o.lora_shrink(g["x"], g["A"], "rc", g["tpe3"], g["offs"]), RT, TABLE),
    ("shrink/table-1", lambda g, o: o.lora_shrink(g["x"], g["A"], "rc", g["tpe"], g["offs"][:1]), RT, TABLE),
    ("shrink/table-half", lambda g, o: o.lora_shrink(g["x"], g["A"], "rc", g["tpe"], None), RT, "given together"),
    ("shrink/table-none", lambda g, o: o.lora_shrink(g["x"], g["A"], "rc"), RT, "more than one expert"),
    ("shrink/table-cpu", lambda g, o: o.lora_shrink(g["x"], g["A"], "rc", g["tpe"], g["offs"].cpu()), RT, "input_offsets"),
    ("expand/v-dtype", lambda g, o: o.lora_expand(g["v"].half(), g["B"], "cr", g["tpe"], g["offs"], input=g["y"]), RT, "v must be a float32"),
    ("expand/v-columns", lambda g, o: o.lora_expand(g["x"], g["B"], "cr", g["tpe"], g["offs"], input=g["y"]), RT, "adapter rank"),
    ("expand/no-ref", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe"], g["offs"]), RT, "`input` or `out`"),
    ("expand/input-shape", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe"], g["offs"], input=g["y"][:T - 1]), RT, "input must be"),
    ("expand/C", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe"], g["offs"], input=g["x"]), RT, "columns"),
    ("expand/out_dtype", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe"], g["offs"], input=g["y"], out_dtype=f64), RT, "out_dtype"),
    ("expand/out-shape", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe"], g["offs"], input=g["y"], out=g["y"][:T - 1]), RT, "out must be"),
    ("expand/lora-rank", lambda g, o: o.lora_expand(g["v"], g["A5"], "rc", g["tpe"], g["offs"], input=g["x"]), RT, "LoRA rank"),
    ("expand/table+1", lambda g, o: o.lora_expand(g["v"], g["B"], "cr", g["tpe3"], g["offs"], input=g["y"]), RT, TABLE),
    ("grad/p-dtype", lambda g, o: o.lora_grad(g["x"].to(i32), g["v"], "rc", E, g["tpe"], g["offs"]), RT, "p must be a"),
    ("grad/v-dtype", lambda g, o: o.lora_grad(g["x"], g["v"].half(), "rc", E, g["tpe"], g["offs"]), RT, "v must be a float32"),
    ("grad/rows", lambda g, o: o.lora_grad(g["x"], g["v"][:T - 1], "rc", E, g["tpe"], g["offs"]), RT, "same number of rows"),
    ("grad/lora-rank", lambda g, o: o.lora_grad(g["x"], g["x"][:, :5].contiguous(), "rc", E, g["tpe"], g["offs"]), RT, "LoRA rank"),
    ("grad/layout", lambda g, o: o.lora_grad(g["x"], g["v"], "xx", E, g["tpe"], g["offs"]), VE, "layout"),
    ("grad/table+1", lambda g, o: o.lora_grad(g["x"], g["v"], "rc", E, g["tpe3"], g["offs"]), RT, TABLE),
    ("grad/table-1", lambda g, o: o.lora_grad(g["x"], g["v"], "rc", E, g["tpe"], g["offs"][:1]), RT, TABLE),
    ("grad/table-none", lambda g, o: o.lora_grad(g["x"], g["v"], "rc", E), RT, "more than one expert"),
    ("gated_shrink/dtype", lambda g, o: o.lora_gated_shrink(g["gu"].to(i32), g["A"], "rc", g["tpe"], g["offs"]), RT, "gate_up must be a"),
    ("gated_shrink/odd", lambda g, o: o.lora_gated_shrink(g["gu"][:, :2 * K - 1].contiguous(), g["A"], "rc", g["tpe"], g["offs"]), RT, r"gate_up must be \[T, 2C\]"),
    ("gated_shrink/K", lambda g, o: o.lora_gated_shrink(g["x"], g["A"], "rc", g["tpe"], g["offs"]), RT, "columns"),
    ("gated_shrink/lora-rank", lambda g, o: o.lora_gated_shrink(g["gu"], g["A5"], "rc", g["tpe"], g["offs"]), RT, "LoRA rank"),
    ("gated_shrink/table+1", lambda g, o: o.lora_gated_shrink(g["gu"], g["A"], "rc", g["tpe3"], g["offs"]), RT, TABLE),
    ("gated_shrink/table-none", lambda g, o: o.lora_gated_shrink(g["gu"], g["A"], "rc"), RT, "more than one expert"),
    ("gated_grad/dtype", lambda g, o: o.lora_gated_grad(g["gu"].to(i32), g["v"], "rc", E, g["tpe"], g["offs"]), RT, "gate_up must be a"),
    ("gated_grad/odd", lambda g, o: o.lora_gated_grad(g["gu"][:, :2 * K - 1].contiguous(), g["v"], "rc", E, g["tpe"], g["offs"]), RT, r"gate_up must be \[T, 2C\]"),
    ("gated_grad/v-dtype", lambda g, o: o.lora_gated_grad(g["gu"], g["v"].half(), "rc", E, g["tpe"], g["offs"]), RT, "v must be a float32"),
    ("gated_grad/rows", lambda g, o: o.lora_gated_grad(g["gu"], g["v"][:T - 1], "rc", E, g["tpe"], g["offs"]), RT, "same number of rows"),
    ("gated_grad/lora-rank", lambda g, o: o.lora_gated_grad(g["gu"], g["x"][:, :5].contiguous(), "rc", E, g["tpe"], g["offs"]), RT, "LoRA rank"),
    ("gated_grad/table-1", lambda g, o: o.lora_gated_grad(g["gu"], g["v"], "rc", E, g["tpe"][:1], g["offs"]), RT, TABLE),
    ("swiglu/dtype", lambda g, o: o.swiglu_backward(g["gu"].to(i32), g["dh"]), RT, "gate_up must be a"),
    ("swiglu/odd", lambda g, o: o.swiglu_backward(g["gu"][:, :2 * K - 1].contiguous(), g["dh"]), RT, r"gate_up must be \[T, 2C\]"),
    ("swiglu/dh-shape", lambda g, o: o.swiglu_backward(g["gu"], g["dh"][:, :K - 1].contiguous()), RT, "dh must be"),
    ("swiglu/dh-dtype", lambda g, o: o.swiglu_backward(g["gu"], g["dh"].to(i32)), RT, "dh must be a"),
    ("swiglu/out_dtype", lambda g, o: o.swiglu_backward(g["gu"], g["dh"], out_dtype=f64), RT, "out_dtype"),
    # ---- LoRA layers
    ("linear_lora/dtype", lambda g, o: o.linear_lora_forward(g["x"].to(i32), g["P"], g["s"], g["z"], g["A1"], g["B1"], 2.0), RT, "x must be a CUDA"),
    ("linear_lora/rank", lambda g, o: o.linear_lora_forward(g["x"][None], g["P"], g["s"], g["z"], g["A1"], g["B1"], 2.0), RT, "1-D or 2-D"),
    ("linear_lora/adapter-dtype", lambda g, o: o.linear_lora_forward(g["x"], g["P"], g["s"], g["z"], g["A1"].half(), g["B1"], 2.0), RT, "stay float32"),
    ("linear_lora/adapter-rank", lambda g, o: o.linear_lora_forward(g["x"], g["P"], g["s"], g["z"], g["A"], g["B"], 2.0), RT, "lora_A / lora_B must be"),
    ("linear_lora/adapter-K", lambda g, o: o.linear_lora_forward(g["x"], g["P"], g["s"], g["z"], g["A1"][:, :32], g["B1"], 2.0), RT, "lora_A must be"),
    ("linear_lora/lora-rank", lambda g, o: o.linear_lora_forward(g["x"], g["P"], g["s"], g["z"], g["A5"][0], g["B"][0, :, :1].expand(N, 5), 2.0), RT, "LoRA rank"),
    ("linear_lora/K", lambda g, o: o.linear_lora_forward(g["x"], g["P"][:, :16].contiguous(), g["s"], g["z"], g["A1"], g["B1"], 2.0), RT, "packed_weights dim 1"),
    ("linear_lora/bias-len", lambda g, o: o.linear_lora_forward(g["x"], g["P"], g["s"], g["z"], g["A1"], g["B1"], 2.0, bias=g["bias"][:N - 1]), RT, "bias"),
    ("moe_lora/dtype", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"].to(i32), g["A"], g["B"], 2.0, g["tpe"], g["offs"]), RT, "inputs must be a CUDA"),
    ("moe_lora/rank", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"][None], g["A"], g["B"], 2.0, g["tpe"], g["offs"]), RT, "inputs must be a CUDA"),
    ("moe_lora/packed-rank", lambda g, o: o.moe_lora_forward(g["P"], g["s"], g["z"], g["x"], g["A"], g["B"], 2.0, g["tpe"], g["offs"]), RT, "per-row INT4 weights"),
    ("moe_lora/adapter-dtype", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"], g["A"], g["B"].half(), 2.0, g["tpe"], g["offs"]), RT, "stay float32"),
    ("moe_lora/adapter-E", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"], g["A"][:1], g["B"], 2.0, g["tpe"], g["offs"]), RT, "lora_A must be"),
    ("moe_lora/lora-rank", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"], g["A5"], g["B"][:, :, :1].expand(E, N, 5), 2.0, g["tpe"], g["offs"]), RT, "LoRA rank"),
    ("moe_lora/K", lambda g, o: o.moe_lora_forward(g["P3"][:, :, :16], g["S"], g["Z"], g["x"], g["A"], g["B"], 2.0, g["tpe"], g["offs"]), RT, "packed_weights dim 2"),
    ("moe_lora/table+1", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"], g["A"], g["B"], 2.0, g["tpe3"], g["offs"]), RT, TABLE),
    ("moe_lora/table-1", lambda g, o: o.moe_lora_forward(g["P3"], g["S"], g["Z"], g["x"].half(), g["A"], g["B"], 2.0, g["tpe"], g["offs"][:1]), RT, TABLE),
    ("ffn_lora/dtype", lambda g, o: ffn(g, o, x=g["x"].half()), RT, "float32 only"),
    ("ffn_lora/activation_dtype", lambda g, o: ffn(g, o, activation_dtype=f16), RT, "activation_dtype"),
    ("ffn_lora/activation_dtype-int", lambda g, o: ffn(g, o, activation_dtype=torch.int8), VE, "activation_dtype"),
    ("ffn_lora/fp8", lambda g, o: ffn(g, o, x=g["x"].half(), activation_dtype=f16, precision="fp8"), RT, "fp8"),
    ("ffn_lora/packed-rank", lambda g, o: ffn(g, o, gup=g["gup"][0]), RT, "per-row INT4 weights"),
    ("ffn_lora/down-shape", lambda g, o: ffn(g, o, dp=g["dp"][:, :, :8]), RT, "down_packed"),
    ("ffn_lora/adapter-dtype", lambda g, o: ffn(g, o, Ad=g["Ad"].half()), RT, "stay float32"),
    ("ffn_lora/adapter-K", lambda g, o: ffn(g, o, Agu=g["Agu"][:, :, :32]), RT, "lora_A must be"),
    ("ffn_lora/lora-rank", lambda g, o: ffn(g, o, Agu=g["A5"], Bgu=g["Bgu"][:, :, :1].expand(E, 2 * F, 5)), RT, "LoRA rank"),
    ("ffn_lora/ranks-differ", lambda g, o: ffn(g, o, Ad=g["Ad"].repeat(1, 2, 1), Bd=g["Bd"].repeat(1, 1, 2)), RT, "same rank"),
    ("ffn_lora/table+1", lambda g, o: ffn(g, o, tpe=g["tpe3"]), RT, TABLE),
    ("ffn_lora/table-1", lambda g, o: ffn(g, o, x=g["x"].half(), activation_dtype=f16, offs=g["offs"][:1]), RT, TABLE),
    ("check_rows/dtype", lambda g, o: o.check_activation_rows(g["x"], "inputs", f16), RT, "activation_dtype"),
    ("activation_dtype_of", lambda g, o: o.activation_dtype_of(f64), VE, "activation_dtype"),
]


@pytest.mark.parametrize("call,exc,regex", [pytest.param(c, e, r, id=i) for i, c, e, r in REFUSALS])
def test_refusals(g, call, exc, regex):
    with torch.no_grad(), pytest.raises(exc, match=regex) as info:
        call(g, ops())
    assert type(info.value) is exc                 # the type itself, not a subclass (NativeLibraryError is a RuntimeError)


# ---- the doors the shared checkers closed: each argument of these ops as a CPU tensor (it used to reach the kernel as a
# host pointer or be copied to the device behind the caller's back), and an expert table of E - 1 elements where none
# was checked.  RuntimeError, before the native library is touched.
def _each(name, op, keys, names, **kw):
    """One row per argument: ``ops.<op>(*good)`` with the argument ``names[i]`` (``g[keys[i]]``) moved to the CPU."""
    def row(i):
        return lambda g, o: getattr(o, op)(*[g[k].cpu() if j == i else g[k] for j, k in enumerate(keys)], **kw)
    return [(f"{name}/{n}", row(i)) for i, n in enumerate(names)]


WEIGHTS = ["packed_weights", "scales", "zero_points"]
LIMBS = ["limbs", "delta", "rowsum"]
DOORS = (
    _each("linear_bwd", "linear_backward_input", ["gy", "P", "s", "z"], ["grad_out"] + WEIGHTS)
    + _each("moe_bwd", "moe_backward_input", ["P3", "S", "Z", "gy", "tpe", "offs"],
            WEIGHTS + ["grad_out", "tokens_per_expert", "input_offsets"])
    + _each("dequantize", "dequantize_forward", ["P", "s", "z"], WEIGHTS)
    + _each("combine", "combine", ["y", "pos", "w"], ["y", "pos_of_slot", "expert_weights"])
    + _each("combine_unweighted", "combine", ["y", "pos"], ["y", "pos_of_slot"], expert_weights=None, top_k=2)
    + _each("combine_bwd", "combine_backward", ["gy4", "y", "pos", "w"], ["grad_out", "y", "pos_of_slot", "expert_weights"])
    + _each("gemm_i8", "gemm_i8", ["limbs", "delta", "rowsum", "P", "s", "z"], LIMBS + WEIGHTS, precision="exact")
    + _each("gemm_i8_grouped", "gemm_i8", ["limbs", "delta", "rowsum", "P3", "S", "Z", "tpe", "offs"],
            LIMBS + WEIGHTS + ["tokens_per_expert", "input_offsets"], precision="exact")
    + [
        ("gemm_i8/out", lambda g, o: o.gemm_i8(g["limbs"], g["delta"], g["rowsum"], g["P"], g["s"], g["z"], precision="exact", out=g["y"].cpu())),
        ("act_quant/tokens_per_expert", lambda g, o: o.act_quant(g["x"], "exact", g["tpe"].cpu(), g["offs"])),
        ("act_quant/input_offsets", lambda g, o: o.act_quant(g["x"], "exact", g["tpe"], g["offs"].cpu())),
        # tables and scales whose sizes nothing compared
        ("moe_bwd/table-1", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"], g["tpe"][:1], g["offs"])),
        ("moe_bwd/table+1", lambda g, o: o.moe_backward_input(g["P3"], g["S"], g["Z"], g["gy"], g["tpe"], g["tpe3"])),
        ("gemm_i8/table-1", lambda g, o: o.gemm_i8(g["limbs"], g["delta"], g["rowsum"], g["P3"], g["S"], g["Z"], g["tpe"], g["offs"][:1], precision="exact")),
        ("gemm_i8/scales-len", lambda g, o: o.gemm_i8(g["limbs"], g["delta"], g["rowsum"], g["P"], g["s"][:N - 1], g["z"], precision="exact")),
        ("act_quant/table-1", lambda g, o: o.act_quant(g["x"], "exact", g["tpe"], g["offs"][:1])),
        ("dequantize/scales-len", lambda g, o: o.dequantize_forward(g["P"], g["s"][:N - 1], g["z"])),
        ("combine/pos-len", lambda g, o: o.combine(g["y"], g["pos"][:T - 1], g["w"])),
        ("combine_bwd/pos-len", lambda g, o: o.combine_backward(g["gy4"], g["y"], g["pos"][:T - 1], g["w"])),
    ])


@pytest.mark.parametrize("call", [pytest.param(c, id=i) for i, c in DOORS])
def test_closed_doors(g, monkeypatch, call):
    def touched():
        raise AssertionError("the native library was reached before the refusal")
    monkeypatch.setattr(ops()._native, "lib", touched)
    with torch.no_grad(), pytest.raises(RuntimeError) as info:
        call(g, ops())
    assert type(info.value) is RuntimeError
