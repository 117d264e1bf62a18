"""Trainable low-rank adapters (LoRA) on the frozen INT4 layers: ``y = W_q x + (alpha / r) * B (A x)``.

``LoRAQuantizedLinear`` and ``LoRAMoEINT4`` keep the base layer's buffers (and state_dict keys) unchanged and add two
float32 parameters in PEFT's layout, ``lora_A`` [r, K] / [E, r, K] and ``lora_B`` [N, r] / [E, N, r].  They are the
module's only parameters, so an optimiser built from ``parameters()`` trains the adapters alone.  On the GPU the adapter
runs in the segmented kernels of csrc/fql_lora.h (ops.linear_lora_forward / ops.moe_lora_forward); on the CPU
``LoRAQuantizedLinear`` is plain torch.  INTEGRATION.md section 6 lists what is out of scope.

Both take float16 / bfloat16 activations on the GPU: the kernels read ``x`` and the incoming
gradient as they are and write ``y`` and ``x.grad`` in ``x``'s type, bit for bit the float32 module on ``x.float()``
rounded once; ``lora_A`` / ``lora_B`` and their gradients stay float32, and the node saves ``x`` in its own type.

``LoRAQuantizedMoEFFN`` puts an adapter on each projection of the gated experts of ``QuantizedMoEFFN``: one on the
stacked gate|up weight (one ``A`` shared by gate and up, a ``[2F, r]`` ``B``: PEFT's shape for a fused ``gate_up_proj``)
and one on the down weight (ops.moe_ffn_lora_forward).  Built with ``activation_dtype`` =
torch.float16 / torch.bfloat16 it runs on 16-bit activations and keeps ``gate_up`` in that type (INTEGRATION.md
section 9); by default it is the float32 layer.

``LoRAMXFP4MoEFFN`` is the same pair of adapters on the MXFP4 experts of ``MXFP4MoEFFN``, with the adapter term fused into
the bfloat16 GEMMs as one more contraction stage (ops.moe_ffn_lora_forward_mxfp4, INTEGRATION.md section 17, DESIGN.md
section 35).  ``LoRANVFP4MoEFFN`` is that layer on the NVFP4 experts of ``NVFP4MoEFFN`` (ops.moe_ffn_lora_forward_nvfp4,
INTEGRATION.md section 18); the dense ``LoRANVFP4Linear`` lives in nvfp4_linear.py.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .module import QuantizedLinear
from .moe import MoEINT4, MXFP4MoEFFN, NVFP4MoEFFN, QuantizedMoEFFN
from .ops import LORA_RANKS


def _check_rank(rank):
    if rank not in LORA_RANKS:
        raise ValueError(f"rank must be one of {LORA_RANKS}, got {rank!r}")


class LoRAQuantizedLinear(QuantizedLinear):
    def __init__(self, in_features: int, out_features: int, rank: int, alpha: float | None = None,
                 precision: str = "default", bias: bool = False, group_size: int | None = None):
        super().__init__(in_features, out_features, precision=precision, bias=bias, group_size=group_size)
        _check_rank(rank)
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        self.lora_A = nn.Parameter(torch.empty(rank, in_features, dtype=torch.float32))
        self.lora_B = nn.Parameter(torch.empty(out_features, rank, dtype=torch.float32))
        self.reset_lora_parameters()

    def reset_lora_parameters(self):
        """PEFT's initialisation: A kaiming-uniform (a = sqrt(5)), B zeros -- a fresh adapter adds nothing."""
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B)

    @classmethod
    def from_quantized(cls, layer: QuantizedLinear, rank: int, alpha: float | None = None) -> "LoRAQuantizedLinear":
        """Wrap an existing ``QuantizedLinear``; the new module shares its buffers (no copy)."""
        module = cls(layer.in_features, layer.out_features, rank, alpha, precision=layer.precision,
                     bias=layer.bias is not None, group_size=layer.group_size)
        module.packed_weights = layer.packed_weights
        module.scales = layer.scales
        module.zero_points = layer.zero_points
        if layer.bias is not None:
            module.bias = layer.bias
        dev = layer.packed_weights.device
        module.lora_A.data = module.lora_A.data.to(dev)
        module.lora_B.data = module.lora_B.data.to(dev)
        return module

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in ("lora_A", "lora_B")}

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            from . import ops
            return ops.linear_lora_forward(x, self.packed_weights, self.scales, self.zero_points, self.lora_A,
                                           self.lora_B, self.scaling, precision=self.precision, bias=self.bias)
        return super().forward(x) + self.scaling * ((x @ self.lora_A.t()) @ self.lora_B.t())

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, rank={self.rank}, alpha={self.alpha:g}"


class LoRAMoEINT4(MoEINT4):
    def __init__(self, num_experts, hidden_dim, ffn_dim, rank: int, alpha: float | None = None,
                 precision: str = "default"):
        super().__init__(num_experts, hidden_dim, ffn_dim, precision=precision)
        _check_rank(rank)
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        self.lora_A = nn.Parameter(torch.empty(num_experts, rank, hidden_dim, dtype=torch.float32))
        self.lora_B = nn.Parameter(torch.empty(num_experts, ffn_dim, rank, dtype=torch.float32))
        self.reset_lora_parameters()

    def reset_lora_parameters(self):
        """PEFT's initialisation per expert (fan-in = hidden_dim): A kaiming-uniform (a = sqrt(5)), B zeros."""
        with torch.no_grad():
            for e in range(self.num_experts):
                nn.init.kaiming_uniform_(self.lora_A[e], a=math.sqrt(5))
        nn.init.zeros_(self.lora_B)

    @classmethod
    def from_quantized(cls, layer: MoEINT4, rank: int, alpha: float | None = None) -> "LoRAMoEINT4":
        """Wrap an existing ``MoEINT4``; the new module shares its buffers (no copy)."""
        module = cls(layer.num_experts, layer.hidden_dim, layer.ffn_dim, rank, alpha, precision=layer.precision)
        module.packed_weights = layer.packed_weights
        module.scales = layer.scales
        module.zero_points = layer.zero_points
        dev = layer.packed_weights.device
        module.lora_A.data = module.lora_A.data.to(dev)
        module.lora_B.data = module.lora_B.data.to(dev)
        return module

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in ("lora_A", "lora_B")}

    def forward(self, inputs, expert_ids, tokens_per_expert, input_offsets):
        """inputs ``[T, K]`` float32 / float16 / bfloat16 on the GPU, rows grouped by expert -> ``[T, N]`` of the same
        type (GPU only, as MoEINT4)."""
        del expert_ids
        if not inputs.is_cuda:
            raise RuntimeError("LoRAMoEINT4 runs on the GPU only (inputs must be a CUDA tensor)")
        from . import ops
        return ops.moe_lora_forward(self.packed_weights, self.scales, self.zero_points, inputs, self.lora_A,
                                    self.lora_B, self.scaling, tokens_per_expert, input_offsets,
                                    precision=self.precision)

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, ffn_dim={self.ffn_dim}, "
                f"rank={self.rank}, alpha={self.alpha:g}")


_FFN_ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")


class LoRAQuantizedMoEFFN(QuantizedMoEFFN):
    """``down(silu(gate(x)) * up(x))`` per expert with ``gate_up = W_gu x + s B_gu (A_gu x)`` and
    ``y = W_d h + s B_d (A_d h)``, ``s = alpha / rank``.  The INT4 buffers are frozen; the four adapters are the only
    parameters (float32 whatever ``activation_dtype`` is).  With ``expert_bias=True`` the layer also has the two bias
    parameters of ``QuantizedMoEFFN`` (frozen until ``requires_grad_(True)``): ``gate_up = W_gu x + b_gu + s B_gu (A_gu x)``
    and ``y = W_d h + b_d + s B_d (A_d h)``.  ``group_size``: per-group INT4 scales, as ``QuantizedMoEFFN`` takes it."""

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, rank: int, alpha: float | None = None,
                 precision: str = "default", activation_dtype=None, activation: str = "silu",
                 activation_alpha: float = 1.702, activation_limit: float = 7.0, expert_bias: bool = False,
                 group_size=None):
        super().__init__(num_experts, hidden_dim, ffn_dim, precision=precision, activation_dtype=activation_dtype,
                         activation=activation, activation_alpha=activation_alpha, activation_limit=activation_limit,
                         expert_bias=expert_bias, group_size=group_size)
        _check_rank(rank)
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.gate_up_lora_A = nn.Parameter(torch.empty(E, rank, H, dtype=torch.float32))
        self.gate_up_lora_B = nn.Parameter(torch.empty(E, 2 * F, rank, dtype=torch.float32))
        self.down_lora_A = nn.Parameter(torch.empty(E, rank, F, dtype=torch.float32))
        self.down_lora_B = nn.Parameter(torch.empty(E, H, rank, dtype=torch.float32))
        self.reset_lora_parameters()

    def reset_lora_parameters(self):
        """PEFT's initialisation per expert (fan-in = hidden_dim / ffn_dim): A kaiming-uniform (a = sqrt(5)), B zeros."""
        with torch.no_grad():
            for e in range(self.num_experts):
                nn.init.kaiming_uniform_(self.gate_up_lora_A[e], a=math.sqrt(5))
                nn.init.kaiming_uniform_(self.down_lora_A[e], a=math.sqrt(5))
        nn.init.zeros_(self.gate_up_lora_B)
        nn.init.zeros_(self.down_lora_B)

    @classmethod
    def from_quantized(cls, layer: QuantizedMoEFFN, rank: int, alpha: float | None = None,
                       activation_dtype=None) -> "LoRAQuantizedMoEFFN":
        """Wrap an existing ``QuantizedMoEFFN``; the new module shares its buffers (no copy).  ``activation_dtype``
        None keeps the wrapped layer's.  The activation kind is the wrapped layer's, and so are its biases: the same
        parameters, in the ``requires_grad`` state they have."""
        if activation_dtype is None:
            activation_dtype = layer.activation_dtype
        module = cls(layer.num_experts, layer.hidden_dim, layer.ffn_dim, rank, alpha, precision=layer.precision,
                     activation_dtype=activation_dtype, activation=layer.activation,
                     activation_alpha=layer.activation_alpha, activation_limit=layer.activation_limit,
                     expert_bias=layer.expert_bias, group_size=layer.group_size)
        for name, buf in layer.named_buffers():
            setattr(module, name, buf)
        if layer.expert_bias:
            module.gate_up_bias, module.down_bias = layer.gate_up_bias, layer.down_bias
        dev = layer.gate_up_packed.device
        for name in _FFN_ADAPTERS:
            p = getattr(module, name)
            p.data = p.data.to(dev)
        return module

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in _FFN_ADAPTERS}

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 on the GPU, rows grouped by expert -> ``[T, H]`` float32 (GPU only); with
        ``activation_dtype`` both have that type."""
        if not inputs.is_cuda:
            raise RuntimeError("LoRAQuantizedMoEFFN runs on the GPU (the product path has no CPU fallback)")
        from . import ops
        return ops.moe_ffn_lora_forward(self.gate_up_packed, self.gate_up_scales, self.gate_up_zero_points,
                                        self.down_packed, self.down_scales, self.down_zero_points, inputs,
                                        self.gate_up_lora_A, self.gate_up_lora_B, self.down_lora_A, self.down_lora_B,
                                        self.scaling, tokens_per_expert, input_offsets, precision=self.precision,
                                        activation_dtype=self.activation_dtype, activation=self.activation,
                                        activation_alpha=self.activation_alpha,
                                        activation_limit=self.activation_limit, **self._bias_args())

    def _bias_args(self):
        """The biases as ``ops.moe_ffn_lora_forward`` takes them (nothing for a layer without ``expert_bias``)."""
        return {"gate_up_bias": self.gate_up_bias, "down_bias": self.down_bias} if self.expert_bias else {}

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, ffn_dim={self.ffn_dim}, "
                f"rank={self.rank}, alpha={self.alpha:g}") + self._activation_repr()


class LoRAMXFP4MoEFFN(MXFP4MoEFFN):
    """``MXFP4MoEFFN`` with a trainable low-rank adapter on each projection: ``gate_up = W_gu x + b_gu + s B_gu (A_gu x)``
    and ``y = W_d h + b_d + s B_d (A_d h)``, ``s = alpha / rank``.  The MXFP4 buffers are frozen and keep the checkpoint's
    encoding; the four float32 adapters (``LoRAQuantizedMoEFFN``'s names, shapes and PEFT initialisation) are the only
    parameters besides the biases of ``expert_bias=True`` (frozen until ``requires_grad_(True)``).  ``activation_dtype``
    None / float32 or bfloat16, every activation kind, as in the base layer.  The layer is differentiable in its input,
    the adapters and the biases (``ops.moe_ffn_lora_forward_mxfp4``); the adapter term rides in the two GEMMs as one more
    contraction stage, its operands rounded to bfloat16 as the rows are (the adapters' master copies stay float32).  A
    fresh layer (``B = 0``) returns ``MXFP4MoEFFN``'s bits.  ``precision`` other than ``"bf16"`` raises ``ValueError``: those
    modes have no backward."""

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, rank: int, alpha: float | None = None,
                 activation: str = "silu", activation_alpha: float = 1.702, activation_limit: float = 7.0,
                 expert_bias: bool = False, activation_dtype=None, precision: str = "bf16"):
        if precision != "bf16":
            raise ValueError(f"LoRAMXFP4MoEFFN runs in precision='bf16' only (got {precision!r}): the fp8 / fp6 / fp4 modes "
                             "have no backward")
        super().__init__(num_experts, hidden_dim, ffn_dim, activation=activation, activation_alpha=activation_alpha,
                         activation_limit=activation_limit, expert_bias=expert_bias, activation_dtype=activation_dtype,
                         input_grad=True, precision=precision)
        _check_rank(rank)
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.gate_up_lora_A = nn.Parameter(torch.empty(E, rank, H, dtype=torch.float32))
        self.gate_up_lora_B = nn.Parameter(torch.empty(E, 2 * F, rank, dtype=torch.float32))
        self.down_lora_A = nn.Parameter(torch.empty(E, rank, F, dtype=torch.float32))
        self.down_lora_B = nn.Parameter(torch.empty(E, H, rank, dtype=torch.float32))
        self.reset_lora_parameters()

    reset_lora_parameters = LoRAQuantizedMoEFFN.reset_lora_parameters

    @classmethod
    def from_mxfp4(cls, *args, **kwargs) -> "LoRAMXFP4MoEFFN":
        """``MXFP4MoEFFN.from_mxfp4`` with ``rank=`` (and ``alpha=``) among the keywords; the adapters are created on the
        device of the blocks."""
        module = super().from_mxfp4(*args, **kwargs)
        return module._adapters_to(module.gate_up_blocks.device)

    @classmethod
    def from_layer(cls, layer: MXFP4MoEFFN, rank: int, alpha: float | None = None) -> "LoRAMXFP4MoEFFN":
        """Wrap an existing ``MXFP4MoEFFN``; the new module shares its buffers (no copy) and its biases, the same
        parameters in the ``requires_grad`` state they have.  The activation kind and type are the wrapped layer's."""
        module = cls(layer.num_experts, layer.hidden_dim, layer.ffn_dim, rank, alpha, activation=layer.activation,
                     activation_alpha=layer.activation_alpha, activation_limit=layer.activation_limit,
                     expert_bias=layer.expert_bias, activation_dtype=layer.activation_dtype, precision=layer.precision)
        for name, buf in layer.named_buffers():
            setattr(module, name, buf)
        if layer.expert_bias:
            module.gate_up_bias, module.down_bias = layer.gate_up_bias, layer.down_bias
        return module._adapters_to(layer.gate_up_blocks.device)

    def _adapters_to(self, dev):
        for name in _FFN_ADAPTERS:
            p = getattr(self, name)
            p.data = p.data.to(dev)
        return self

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in _FFN_ADAPTERS}

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 (``activation_dtype=torch.bfloat16``: bfloat16) on the GPU, rows grouped by expert ->
        ``[T, H]`` of the same type."""
        if not inputs.is_cuda:
            raise RuntimeError("LoRAMXFP4MoEFFN runs on the GPU (the product path has no CPU fallback)")
        from . import ops
        b_gu, b_d = self.biases
        return ops.moe_ffn_lora_forward_mxfp4(self.gate_up_blocks, self.gate_up_scales, self.down_blocks, self.down_scales,
                                              inputs, self.gate_up_lora_A, self.gate_up_lora_B, self.down_lora_A,
                                              self.down_lora_B, self.scaling, tokens_per_expert, input_offsets,
                                              activation_dtype=self.activation_dtype, activation=self.activation,
                                              activation_alpha=self.activation_alpha,
                                              activation_limit=self.activation_limit, gate_up_bias=b_gu, down_bias=b_d)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, rank={self.rank}, alpha={self.alpha:g}"


class LoRANVFP4MoEFFN(NVFP4MoEFFN):
    """``NVFP4MoEFFN`` with a trainable low-rank adapter on each projection: ``gate_up = g_gu (W_gu x) + b_gu + s B_gu (A_gu x)``
    and ``y = g_d (W_d h) + b_d + s B_d (A_d h)``, ``s = alpha / rank``, ``g`` the per-expert global scales (they scale the
    weight term only).  The NVFP4 buffers are frozen and keep the checkpoint's encoding; the four float32 adapters
    (``LoRAQuantizedMoEFFN``'s names, shapes and PEFT initialisation) are the only parameters besides the biases of
    ``expert_bias=True`` (frozen until ``requires_grad_(True)``).  ``activation_dtype`` None / float32 or bfloat16, every
    activation kind, as in the base layer; ``input_grad`` is always on.  The layer is differentiable in its input, the
    adapters and the biases (``ops.moe_ffn_lora_forward_nvfp4``); the adapter term rides in the two GEMMs as one more
    contraction stage, its operands rounded to bfloat16 as the rows are (the adapters' master copies stay float32).  A
    fresh layer (``B = 0``) returns ``NVFP4MoEFFN``'s bits.  GPU only."""

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, rank: int, alpha: float | None = None,
                 activation: str = "silu", activation_alpha: float = 1.702, activation_limit: float = 7.0,
                 expert_bias: bool = False, activation_dtype=None, input_grad: bool = True):
        del input_grad                                                                 # (always on: the layer is for training)
        super().__init__(num_experts, hidden_dim, ffn_dim, activation=activation, activation_alpha=activation_alpha,
                         activation_limit=activation_limit, expert_bias=expert_bias, activation_dtype=activation_dtype,
                         input_grad=True)
        _check_rank(rank)
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.gate_up_lora_A = nn.Parameter(torch.empty(E, rank, H, dtype=torch.float32))
        self.gate_up_lora_B = nn.Parameter(torch.empty(E, 2 * F, rank, dtype=torch.float32))
        self.down_lora_A = nn.Parameter(torch.empty(E, rank, F, dtype=torch.float32))
        self.down_lora_B = nn.Parameter(torch.empty(E, H, rank, dtype=torch.float32))
        self.reset_lora_parameters()

    reset_lora_parameters = LoRAQuantizedMoEFFN.reset_lora_parameters
    _adapters_to = LoRAMXFP4MoEFFN._adapters_to
    adapter_state_dict = LoRAMXFP4MoEFFN.adapter_state_dict

    @classmethod
    def from_nvfp4(cls, *args, **kwargs) -> "LoRANVFP4MoEFFN":
        """``NVFP4MoEFFN.from_nvfp4`` with ``rank=`` (and ``alpha=``) among the keywords (``from_weights`` takes them the
        same way); the adapters are created on the device of the blocks."""
        module = super().from_nvfp4(*args, **kwargs)
        return module._adapters_to(module.gate_up_blocks.device)

    @classmethod
    def from_layer(cls, layer: NVFP4MoEFFN, rank: int, alpha: float | None = None) -> "LoRANVFP4MoEFFN":
        """Wrap an existing ``NVFP4MoEFFN``; the new module shares its buffers (no copy) and its biases, the same
        parameters in the ``requires_grad`` state they have.  The activation kind and type are the wrapped layer's."""
        module = cls(layer.num_experts, layer.hidden_dim, layer.ffn_dim, rank, alpha, activation=layer.activation,
                     activation_alpha=layer.activation_alpha, activation_limit=layer.activation_limit,
                     expert_bias=layer.expert_bias, activation_dtype=layer.activation_dtype)
        for name, buf in layer.named_buffers():
            setattr(module, name, buf)
        if layer.expert_bias:
            module.gate_up_bias, module.down_bias = layer.gate_up_bias, layer.down_bias
        return module._adapters_to(layer.gate_up_blocks.device)

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 (``activation_dtype=torch.bfloat16``: bfloat16) on the GPU, rows grouped by expert ->
        ``[T, H]`` of the same type."""
        if not inputs.is_cuda:
            raise RuntimeError("LoRANVFP4MoEFFN runs on the GPU (the product path has no CPU fallback)")
        from . import ops
        b_gu, b_d = self.biases
        return ops.moe_ffn_lora_forward_nvfp4(self.gate_up_blocks, self.gate_up_scales, self.gate_up_global, self.down_blocks,
                                              self.down_scales, self.down_global, inputs, self.gate_up_lora_A,
                                              self.gate_up_lora_B, self.down_lora_A, self.down_lora_B, self.scaling,
                                              tokens_per_expert, input_offsets, activation_dtype=self.activation_dtype,
                                              activation=self.activation, activation_alpha=self.activation_alpha,
                                              activation_limit=self.activation_limit, gate_up_bias=b_gu, down_bias=b_d)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, rank={self.rank}, alpha={self.alpha:g}"
