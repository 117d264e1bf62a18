"""``NVFP4Linear``: a dense ``nn.Linear`` on NVFP4 weights (the encoding of ModelOpt's ``-FP4`` / ``-NVFP4`` exports), frozen
(csrc/fql_gemm_nvfp4.h, csrc/fql_gemm_nvfp4_bwd.h; DESIGN.md sections 38 and 39), and ``LoRANVFP4Linear``, the same layer with
a trainable low-rank adapter fused into its two GEMMs."""
import math

import torch
import torch.nn as nn


class _NVFP4LinearFn(torch.autograd.Function):
    """``NVFP4Linear(input_grad=True)``: the forward's kernels, and ``ops.linear_backward_input_nvfp4`` for ``x.grad`` (the
    weights and the bias are frozen).  Straight-through across the forward's bfloat16 rounding of ``x``."""

    @staticmethod
    def forward(ctx, x2, m):
        ctx.m = m
        return m._rows(x2.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import ops
        m = ctx.m
        return ops.linear_backward_input_nvfp4(m.blocks, m.scales, m.global_scale, gy.contiguous(), out_dtype=gy.dtype), None


class NVFP4Linear(nn.Module):
    """``y = (x @ W.T) * global_scale (+ bias)`` on frozen NVFP4 weights, any leading dimensions as ``nn.Linear``.

    Buffers in the checkpoint's own encoding, never re-quantised: ``blocks`` uint8 [N, K/2] (two e2m1 codes a byte, even
    input in the low nibble), ``scales`` uint8 [N, K/16] (one e4m3fn scale byte per 16 consecutive inputs),
    ``global_scale`` float32 [1] (the per-tensor scale; it MULTIPLIES, as ModelOpt's ``weight_scale_2`` does --
    compressed-tensors stores the reciprocal, ``weight_global_scale``: invert it before ``from_nvfp4``) and, with
    ``bias=True``, a float32 ``bias`` [N].  K = ``in_features`` (a multiple of 32), N = ``out_features``.

    On the GPU the forward is ``ops.linear_forward_nvfp4``: inputs float32 (rounded once to bfloat16) or bfloat16 (float16
    is refused), ``W`` without the global scale exact in bfloat16, float32 sums, then ``* global_scale``, then ``+ bias``,
    two float32 steps, and the result in the inputs' type.  It is bit for bit ``ops.moe_forward_nvfp4`` on one expert;
    there is no split-K form.  On the CPU the forward is the definition,
    ``(bf16(x) @ dequantize_nvfp4(blocks, scales).T) * global_scale (+ bias)`` in float32.

    ``input_grad=False`` (the default) is inference only: a forward under grad mode on an input that requires grad raises
    ``RuntimeError``.  ``input_grad=True`` gives ``x.grad`` through ``ops.linear_backward_input_nvfp4`` (on the GPU only),
    straight-through across the bfloat16 rounding of ``x``.  It is configuration, not state: the
    state-dict keys are ``blocks``, ``scales``, ``global_scale`` (and ``bias``)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, input_grad: bool = False):
        super().__init__()
        if in_features <= 0 or in_features % 32 != 0 or out_features <= 0:
            raise ValueError("in_features must be a positive multiple of 32 and out_features positive")
        self.in_features, self.out_features = in_features, out_features
        self.input_grad = bool(input_grad)
        self.register_buffer("blocks", torch.zeros(out_features, in_features // 2, dtype=torch.uint8))
        self.register_buffer("scales", torch.full((out_features, in_features // 16), 0x38, dtype=torch.uint8))
        self.register_buffer("global_scale", torch.ones(1, dtype=torch.float32))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float32))
        else:
            self.register_buffer("bias", None)

    @classmethod
    def from_nvfp4(cls, blocks, scales, global_scale=None, bias=None, **kwargs) -> "NVFP4Linear":
        """The checkpoint's tensors as they are: ``blocks`` uint8 [N, K/2], ``scales`` uint8 [N, K/16] (a
        ``float8_e4m3fn`` tensor is viewed as its bytes), ``global_scale`` one float32 value or None for 1, ``bias`` [N]
        or None.  ``kwargs``: ``input_grad``."""
        if scales.dtype == torch.float8_e4m3fn:
            scales = scales.view(torch.uint8)
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("blocks and scales must be uint8")
        if blocks.dim() != 2 or scales.dim() != 2 or blocks.shape[1] % 16 or tuple(scales.shape) != (blocks.shape[0], blocks.shape[1] // 8):
            raise ValueError("blocks must be [N, K/2] with K % 32 == 0 and scales [N, K/16]")
        N, K = blocks.shape[0], 2 * blocks.shape[1]
        if bias is not None and tuple(bias.shape) != (N,):
            raise ValueError("bias must be [N]")
        if global_scale is not None:
            global_scale = torch.as_tensor(global_scale, dtype=torch.float32)
            if global_scale.numel() != 1:
                raise ValueError("global_scale must hold one value")
        m = cls(K, N, bias=bias is not None, **kwargs)
        m.blocks, m.scales = blocks.contiguous().clone(), scales.contiguous().clone()
        if global_scale is not None:
            m.global_scale = global_scale.detach().reshape(1).clone().to(blocks.device)
        if bias is not None:
            m.bias = bias.detach().float().contiguous().clone()
        return m

    @classmethod
    def from_linear(cls, linear: nn.Linear, **kwargs) -> "NVFP4Linear":
        """Quantise an ``nn.Linear`` with ``quantize.quantize_nvfp4``; its bias is kept (float32).  ``kwargs``:
        ``input_grad``."""
        from .quantize import quantize_nvfp4
        blocks, scales, gs = quantize_nvfp4(linear.weight.detach().float())
        return cls.from_nvfp4(blocks, scales, gs, bias=None if linear.bias is None else linear.bias.detach(), **kwargs)

    def _rows(self, x2):
        from . import ops
        return ops.linear_forward_nvfp4(self.blocks, self.scales, self.global_scale, x2, bias=self.bias, out_dtype=x2.dtype)

    def forward(self, x):
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("ops.linear_forward_nvfp4: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is "
                               "refused: rounding it to bfloat16 would lose three bits; cast it yourself)")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise RuntimeError(f"NVFP4Linear: the last dimension of the input must be in_features = {self.in_features}, got "
                               f"{list(x.shape)}")
        wants = torch.is_grad_enabled() and x.requires_grad
        if wants and not self.input_grad:
            raise RuntimeError("NVFP4Linear is inference-only: the NVFP4 format has no backward.  Run it under "
                               "torch.no_grad(), or on a detached input (or build the layer with input_grad=True)")
        lead = x.shape[:-1]
        if not x.is_cuda:
            from .quantize import dequantize_nvfp4
            if wants:
                raise RuntimeError("NVFP4Linear: the input gradient runs on the GPU only")
            y = (x.detach().bfloat16().float() @ dequantize_nvfp4(self.blocks, self.scales).T) * self.global_scale
            if self.bias is not None:
                y = y + self.bias
            return y.to(x.dtype)
        x2 = x.reshape(-1, self.in_features)
        y = _NVFP4LinearFn.apply(x2, self) if wants else self._rows(x2)
        return y.reshape(*lead, self.out_features)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, format=nvfp4"
                + (", input_grad=True" if self.input_grad else ""))


class LoRANVFP4Linear(NVFP4Linear):
    """``NVFP4Linear`` with a trainable low-rank adapter: ``y = (x @ W.T) * global_scale (+ bias) + s * (x @ lora_A.T) @
    lora_B.T``, ``s = alpha / rank``, any leading dimensions.  The NVFP4 buffers (and the bias) are frozen; ``lora_A`` [r, K]
    and ``lora_B`` [N, r] float32, ``LoRAQuantizedLinear``'s shapes and PEFT initialisation, are the only parameters, so the
    state-dict keys are the base layer's plus ``lora_A`` and ``lora_B``.  The adapter term rides in the forward GEMM and in
    the input gradient as one more contraction stage (``ops.linear_lora_forward_nvfp4``); a fresh layer (``B = 0``) returns
    ``NVFP4Linear``'s bits.  The adapter path runs on the GPU only."""

    def __init__(self, in_features: int, out_features: int, rank: int, alpha: float | None = None, bias: bool = False,
                 input_grad: bool = True):
        del input_grad                                                                 # (always on: the layer is for training)
        super().__init__(in_features, out_features, bias=bias, input_grad=True)
        from .ops import LORA_RANKS
        if rank not in LORA_RANKS:
            raise ValueError(f"rank must be one of {LORA_RANKS}, got {rank!r}")
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

    def _adapters_to(self, dev):
        self.lora_A.data, self.lora_B.data = self.lora_A.data.to(dev), self.lora_B.data.to(dev)
        return self

    @classmethod
    def from_nvfp4(cls, *args, **kwargs) -> "LoRANVFP4Linear":
        """``NVFP4Linear.from_nvfp4`` with ``rank=`` (and ``alpha=``) among the keywords (``from_linear`` takes them the
        same way); the adapters are created on the device of the blocks."""
        module = super().from_nvfp4(*args, **kwargs)
        return module._adapters_to(module.blocks.device)

    @classmethod
    def from_layer(cls, layer: NVFP4Linear, rank: int, alpha: float | None = None) -> "LoRANVFP4Linear":
        """Wrap an existing ``NVFP4Linear``; the new module shares its buffers (no copy)."""
        module = cls(layer.in_features, layer.out_features, rank, alpha, bias=layer.bias is not None)
        for name, buf in layer.named_buffers():
            setattr(module, name, buf)
        return module._adapters_to(layer.blocks.device)

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in ("lora_A", "lora_B")}

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("LoRANVFP4Linear runs on the GPU (the adapter path has no CPU fallback)")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise RuntimeError(f"LoRANVFP4Linear: the last dimension of the input must be in_features = {self.in_features}, "
                               f"got {list(x.shape)}")
        from . import ops
        y = ops.linear_lora_forward_nvfp4(x.reshape(-1, self.in_features), self.blocks, self.scales, self.global_scale,
                                          self.lora_A, self.lora_B, self.scaling, bias=self.bias)
        return y.reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, rank={self.rank}, alpha={self.alpha:g}"
