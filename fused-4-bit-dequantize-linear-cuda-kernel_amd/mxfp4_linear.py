"""``MXFP4Linear``: a dense ``nn.Linear`` on OCP MXFP4 weights (the encoding AMD's Quark "-MXFP4" checkpoints and gpt-oss
use), frozen, with a split-K decode kernel for small batches (csrc/fql_gemm_mx4_linear.h)."""
import torch
import torch.nn as nn

PRECISIONS = ("bf16", "fp8", "fp6", "fp4")


class _MXFP4LinearFn(torch.autograd.Function):
    """``MXFP4Linear(input_grad=True)``: the forward's kernels, and ``ops.linear_backward_input_mxfp4`` for ``x.grad`` (the
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
        return ops.linear_backward_input_mxfp4(m.blocks, m.scales, gy.contiguous(), out_dtype=gy.dtype), None


class MXFP4Linear(nn.Module):
    """``y = x @ W.T (+ bias)`` on frozen OCP MXFP4 weights, any leading dimensions as ``nn.Linear``.

    Buffers in the checkpoint's own encoding, never re-quantised: ``blocks`` uint8 [N, K/2] (two e2m1 codes a byte, even
    input in the low nibble), ``scales`` uint8 [N, K/32] (one E8M0 power-of-two scale per 32 consecutive inputs) and, with
    ``bias=True``, a float32 ``bias`` [N].  K = ``in_features`` (a multiple of 32), N = ``out_features``.

    On the GPU the forward is ``ops.linear_forward_mxfp4``: inputs float32 (rounded once to bfloat16) or bfloat16 (float16
    is refused), the weights exact in bfloat16, float32 sums, the result in the inputs' type.  ``split_k=True`` (the
    default) lets small batches take the split-K decode form: S slices of K side by side and a fixed-order float32 sum
    (a row's result does not depend on the batch, but is not the tile kernel's bit pattern: its bits may change as the
    batch crosses the library's threshold); ``split_k=False`` is bit for bit ``ops.moe_forward_mxfp4`` on one expert.  On
    the CPU the forward is the definition, ``bf16(x) @ dequantize_mxfp4(blocks, scales).T (+ bias)`` in float32.

    ``precision="fp8"`` / ``"fp6"`` / ``"fp4"`` quantise the rows as ``MXFP4MoEFFN`` does and run the block-scaled matrix
    cores; no split form, inference only (``input_grad=True`` with them raises ``ValueError``).

    ``input_grad=False`` (the default) is inference only: a forward under grad mode on an input that requires grad raises
    ``RuntimeError``.  ``input_grad=True`` gives ``x.grad`` through ``ops.linear_backward_input_mxfp4``, straight-through
    across the bfloat16 rounding of ``x``.  ``precision``, ``input_grad`` and ``split_k`` are
    configuration, not state: the state-dict keys are ``blocks``, ``scales`` (and ``bias``)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, precision: str = "bf16",
                 input_grad: bool = False, split_k: bool = True):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be 'bf16', 'fp8', 'fp6' or 'fp4', got {precision!r}")
        if precision != "bf16" and input_grad:
            raise ValueError(f"precision='{precision}' has no backward: it cannot be combined with input_grad=True")
        if in_features <= 0 or in_features % 32 != 0 or out_features <= 0:
            raise ValueError("in_features must be a positive multiple of 32 (one scale per 32 inputs) and out_features positive")
        self.in_features, self.out_features = in_features, out_features
        self.precision, self.input_grad, self.split_k = precision, bool(input_grad), bool(split_k)
        self.register_buffer("blocks", torch.zeros(out_features, in_features // 2, dtype=torch.uint8))
        self.register_buffer("scales", torch.full((out_features, in_features // 32), 127, dtype=torch.uint8))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float32))
        else:
            self.register_buffer("bias", None)

    @classmethod
    def from_mxfp4(cls, blocks, scales, bias=None, **kwargs) -> "MXFP4Linear":
        """The checkpoint's tensors as they are: ``blocks`` uint8 [N, K/2] (or [N, K/32, 16], flattened here), ``scales``
        uint8 [N, K/32], ``bias`` [N] or None.  ``kwargs``: ``precision``, ``input_grad``, ``split_k``."""
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("blocks and scales must be uint8")
        if blocks.dim() == 3 and blocks.shape[-1] == 16:
            blocks = blocks.reshape(blocks.shape[0], -1)
        if blocks.dim() != 2 or scales.dim() != 2 or blocks.shape[1] % 16 or tuple(scales.shape) != (blocks.shape[0], blocks.shape[1] // 16):
            raise ValueError("blocks must be [N, K/2] (or [N, K/32, 16]) and scales [N, K/32]")
        N, K = blocks.shape[0], 2 * blocks.shape[1]
        if bias is not None and tuple(bias.shape) != (N,):
            raise ValueError("bias must be [N]")
        m = cls(K, N, bias=bias is not None, **kwargs)
        m.blocks, m.scales = blocks.contiguous().clone(), scales.contiguous().clone()
        if bias is not None:
            m.bias = bias.detach().float().contiguous().clone()
        return m

    @classmethod
    def from_linear(cls, linear: nn.Linear, **kwargs) -> "MXFP4Linear":
        """Quantise an ``nn.Linear`` with ``quantize.quantize_mxfp4``; its bias is kept (float32)."""
        from .quantize import quantize_mxfp4
        blocks, scales = quantize_mxfp4(linear.weight.detach().float())
        return cls.from_mxfp4(blocks, scales, bias=None if linear.bias is None else linear.bias.detach(), **kwargs)

    def _rows(self, x2):
        from . import ops
        return ops.linear_forward_mxfp4(self.blocks, self.scales, x2, bias=self.bias, out_dtype=x2.dtype,
                                        precision=self.precision, split_k=self.split_k)

    def forward(self, x):
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("ops.linear_forward_mxfp4: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is "
                               "refused: rounding it to bfloat16 would lose three bits; cast it yourself)")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise RuntimeError(f"MXFP4Linear: the last dimension of the input must be in_features = {self.in_features}, got "
                               f"{list(x.shape)}")
        wants = torch.is_grad_enabled() and x.requires_grad
        if wants and not self.input_grad:
            raise RuntimeError("MXFP4Linear is inference-only: the MXFP4 format has no backward.  Run it under "
                               "torch.no_grad(), or on a detached input (or build the layer with input_grad=True)")
        lead = x.shape[:-1]
        if not x.is_cuda:
            from .quantize import dequantize_mxfp4
            if self.precision != "bf16":
                raise RuntimeError(f"MXFP4Linear: precision='{self.precision}' runs on the GPU only")
            if wants:
                raise RuntimeError("MXFP4Linear: the input gradient runs on the GPU only")
            y = x.detach().bfloat16().float() @ dequantize_mxfp4(self.blocks, self.scales).T
            if self.bias is not None:
                y = y + self.bias
            return y.to(x.dtype)
        x2 = x.reshape(-1, self.in_features)
        y = _MXFP4LinearFn.apply(x2, self) if wants else self._rows(x2)
        return y.reshape(*lead, self.out_features)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, format=mxfp4"
                + (f", precision={self.precision}" if self.precision != "bf16" else "")
                + (", input_grad=True" if self.input_grad else "") + ("" if self.split_k else ", split_k=False"))
