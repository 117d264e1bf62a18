"""fused INT4 dequantize-linear / MoE expert GEMM for AMD Instinct MI355X (gfx950).

Drop-in for the Python surface of samy19980109/Fused-4-bit-Dequantize-Linear-CUDA-Kernel
(reference python/__init__.py:14-22 exports, plus the MoE modules the reference keeps in
python/moe_int4_module.py and benchmark/moe_grouped_gemm/).
"""
from .quantize import (quantize_weights, dequantize_weights, reference_quantized_linear, quantize_mxfp4,
                       dequantize_mxfp4, quantize_mxfp6, dequantize_mxfp6, quantize_nvfp4, dequantize_nvfp4,
                       nvfp4_scale_values)
from .module import QuantizedLinear
from .moe import MoEINT4, quantize_weights_moe, QuantizedMoE, QuantizedMoEExpert, QuantizedMoEFFN, QuantizedSparseMoEBlock, \
    MXFP4MoEFFN, NVFP4MoEFFN
from .mxfp4_linear import MXFP4Linear
from .nvfp4_linear import NVFP4Linear, LoRANVFP4Linear
from .lora import LoRAQuantizedLinear, LoRAMoEINT4, LoRAQuantizedMoEFFN, LoRAMXFP4MoEFFN, LoRANVFP4MoEFFN
from .routing import (RoutingResult, simulate_routing, balanced_routing, create_expert_inputs,
                      combine_expert_outputs, dispatch_grouped, dispatch_indices, combine_grouped)

__all__ = [
    "quantize_weights", "dequantize_weights", "reference_quantized_linear", "QuantizedLinear",
    "MoEINT4", "quantize_weights_moe", "QuantizedMoE", "QuantizedMoEExpert", "QuantizedMoEFFN",
    "RoutingResult", "simulate_routing", "balanced_routing", "create_expert_inputs",
    "combine_expert_outputs", "dispatch_grouped", "dispatch_indices", "combine_grouped",
    "LoRAQuantizedLinear", "LoRAMoEINT4", "LoRAQuantizedMoEFFN", "LoRAMXFP4MoEFFN", "QuantizedSparseMoEBlock",
    "quantize_mxfp4", "dequantize_mxfp4", "MXFP4MoEFFN", "quantize_mxfp6", "dequantize_mxfp6", "MXFP4Linear",
    "quantize_nvfp4", "dequantize_nvfp4", "nvfp4_scale_values", "NVFP4MoEFFN", "NVFP4Linear", "LoRANVFP4MoEFFN", "LoRANVFP4Linear",
]
