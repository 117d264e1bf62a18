"""``NF4Linear``: a dense ``nn.Linear`` on 4-bit code-book weights in bitsandbytes' own encoding (NF4 of QLoRA, Hugging Face
``load_in_4bit``, the ``*-bnb-4bit`` checkpoints), frozen (csrc/fql_gemm_lut4.h, csrc/fql_gemm_lut4_bwd.h; DESIGN.md section
44), and ``LoRANF4Linear``, the same layer with a trainable low-rank adapter, composed from the existing adapter ops or, with
``fused=True``, run as one more contraction stage of the two tile kernels."""
import math

import torch
import torch.nn as nn

from .quantize import NF4_CODE_BOOK


class _NF4LinearFn(torch.autograd.Function):
    """``NF4Linear(input_grad=True)``: the forward's kernel, and ``ops.linear_backward_input_lut4`` for ``x.grad`` (the
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
        return ops.linear_backward_input_lut4(m.codes, m.absmax, gy.contiguous(), m.code_book, m.block, out_dtype=gy.dtype), None


class NF4Linear(nn.Module):
    """``y = x @ W.T (+ bias)`` on frozen code-book weights, any leading dimensions as ``nn.Linear``;
    ``W[n, k] = bf16(code_book[c(n, k)] * absmax[n, k // block])``, what bitsandbytes' ``dequantize_4bit`` to bfloat16 gives.

    Buffers in bitsandbytes' own encoding, never re-quantised and never reordered: ``codes`` uint8 [N, K/2] (input ``2i`` in
    the HIGH nibble of byte ``i``), ``absmax`` float32 [N, K/block], ``code_book`` float32 [16] (the NF4 table unless given)
    and, with ``bias=True``, a float32 ``bias`` [N].  K = ``in_features`` (a multiple of 64 and of ``block``, a power of two
    >= 64), N = ``out_features``.  A double-quantised checkpoint's statistics become ``absmax`` once, at load, through
    ``quantize.bnb_nested_absmax``.

    On the GPU the forward is ``ops.linear_forward_lut4``: inputs float32 (rounded once to bfloat16) or bfloat16 (float16 is
    refused), float32 sums, then ``+ bias``, the result in the inputs' type.  On the CPU the forward is the definition,
    ``bf16(x) @ dequantize_lut4(codes, absmax).T (+ bias)`` in float32.

    ``input_grad=False`` (the default) is inference only: a forward under grad mode on an input that requires grad raises
    ``RuntimeError``.  ``input_grad=True`` gives ``x.grad`` through ``ops.linear_backward_input_lut4`` (on the GPU only),
    straight-through across the bfloat16 rounding of ``x``.  It is configuration, not state: the state-dict keys are
    ``codes``, ``absmax``, ``code_book`` (and ``bias``).

    ``split_k=True`` (configuration as well; the default is False and the tile kernel's bits) is for generation: up to the
    library's row threshold the forward is the split-K decode form of ``ops.linear_forward_lut4(split_k=True)``.  A row's
    bits then depend on its own row, the weights, K and N, not on the batch or the row's position, and are run-to-run
    identical; they are not the tile kernel's bits, so a row may change as the batch crosses the threshold."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, input_grad: bool = False, block: int = 64,
                 split_k: bool = False):
        super().__init__()
        if block < 64 or block & (block - 1):
            raise ValueError("block must be a power of two of at least 64")
        if in_features <= 0 or in_features % 64 != 0 or in_features % block != 0 or out_features <= 0:
            raise ValueError("in_features must be a positive multiple of 64 and of block, and out_features positive")
        self.in_features, self.out_features, self.block = in_features, out_features, block
        self.input_grad, self.split_k = bool(input_grad), bool(split_k)
        self.register_buffer("codes", torch.full((out_features, in_features // 2), 0x77, dtype=torch.uint8))   # (NF4's zero)
        self.register_buffer("absmax", torch.ones(out_features, in_features // block, dtype=torch.float32))
        self.register_buffer("code_book", torch.tensor(NF4_CODE_BOOK, dtype=torch.float32))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float32))
        else:
            self.register_buffer("bias", None)

    @classmethod
    def from_bnb(cls, codes, absmax, block: int = 64, code_book=None, bias=None, **kwargs) -> "NF4Linear":
        """bitsandbytes' tensors as they are: ``codes`` uint8 [N, K/2] and ``absmax`` float32 [N, K/block]; its packed
        ``[N*K/2, 1]`` / flat weight and flat ``[N*K/block]`` statistics are viewed, given ``out_features=`` among the
        keywords.  ``code_book`` 16 values or None for NF4, ``bias`` [N] or None.  ``kwargs``: ``input_grad``, ``split_k``."""
        N = kwargs.pop("out_features", None)
        if codes.dtype != torch.uint8 or absmax.dtype != torch.float32:
            raise ValueError("codes must be uint8 and absmax float32")
        if codes.dim() != 2 or codes.shape[1] == 1:
            if N is None and absmax.dim() == 2:
                N = absmax.shape[0]                                                    # (statistics already [N, K/block])
            if N is None or N <= 0 or codes.numel() % N:
                raise ValueError("a flat or [N*K/2, 1] codes tensor needs out_features= (a divisor of its size)")
            codes = codes.reshape(N, -1)
        N, K = codes.shape[0], 2 * codes.shape[1]
        if block < 64 or block & (block - 1) or K % 64 or K % block or absmax.numel() != N * (K // block):
            raise ValueError("codes must be [N, K/2] with K % 64 == 0 and absmax [N, K/block], block a power of two >= 64 dividing K")
        if bias is not None and tuple(bias.shape) != (N,):
            raise ValueError("bias must be [N]")
        m = cls(K, N, bias=bias is not None, block=block, **kwargs)
        m.codes, m.absmax = codes.contiguous().clone(), absmax.reshape(N, K // block).contiguous().clone()
        if code_book is not None:
            book = torch.as_tensor(code_book, dtype=torch.float32)
            if tuple(book.shape) != (16,):
                raise ValueError("code_book must hold 16 values")
            m.code_book = book.detach().clone().to(codes.device)
        else:
            m.code_book = m.code_book.to(codes.device)
        if bias is not None:
            m.bias = bias.detach().float().contiguous().clone()
        return m

    @classmethod
    def from_linear(cls, linear: nn.Linear, block: int = 64, code_book=None, **kwargs) -> "NF4Linear":
        """Quantise an ``nn.Linear`` with ``quantize.quantize_lut4``; its bias is kept (float32).  ``kwargs``: ``input_grad``, ``split_k``."""
        from .quantize import quantize_lut4
        codes, absmax = quantize_lut4(linear.weight.detach().float(), code_book, block)
        return cls.from_bnb(codes, absmax, block, code_book, bias=None if linear.bias is None else linear.bias.detach(), **kwargs)

    def _rows(self, x2):
        from . import ops
        return ops.linear_forward_lut4(self.codes, self.absmax, x2, self.code_book, self.block, bias=self.bias, out_dtype=x2.dtype,
                                       split_k=self.split_k)

    def forward(self, x):
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("ops.linear_forward_lut4: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is "
                               "refused: rounding it to bfloat16 would lose three bits; cast it yourself)")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise RuntimeError(f"NF4Linear: the last dimension of the input must be in_features = {self.in_features}, got "
                               f"{list(x.shape)}")
        wants = torch.is_grad_enabled() and x.requires_grad
        if wants and not self.input_grad:
            raise RuntimeError("NF4Linear is inference-only as built.  Run it under torch.no_grad(), or on a detached input "
                               "(or build the layer with input_grad=True)")
        lead = x.shape[:-1]
        if not x.is_cuda:
            from .quantize import dequantize_lut4
            if wants:
                raise RuntimeError("NF4Linear: the input gradient runs on the GPU only")
            y = x.detach().bfloat16().float() @ dequantize_lut4(self.codes, self.absmax, self.code_book, self.block).float().T
            if self.bias is not None:
                y = y + self.bias
            return y.to(x.dtype)
        x2 = x.reshape(-1, self.in_features)
        y = _NF4LinearFn.apply(x2, self) if wants else self._rows(x2)
        return y.reshape(*lead, self.out_features)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, format=lut4, "
                f"block={self.block}" + (", input_grad=True" if self.input_grad else "") + (", split_k=True" if self.split_k else ""))


class LoRANF4Linear(NF4Linear):
    """``NF4Linear`` with a trainable low-rank adapter (QLoRA): ``y = x @ W.T (+ bias) + s * (x @ lora_A.T) @ lora_B.T``,
    ``s = alpha / rank``, any leading dimensions.  The code-book buffers (and the bias) are frozen; ``lora_A`` [r, K] and
    ``lora_B`` [N, r] float32, PEFT's initialisation, are the only parameters, so the state-dict keys are the base layer's
    plus ``lora_A`` and ``lora_B``.  Composed from ``ops.linear_forward_lut4`` / ``linear_backward_input_lut4`` and
    ``ops.lora_shrink`` / ``lora_expand`` / ``lora_grad`` in one autograd node (``ops.linear_lora_forward_lut4``).  A fresh
    layer (``B = 0``) returns ``NF4Linear``'s bits.  The adapter path runs on the GPU only.

    ``fused=True`` (configuration, not state; the default is False and the composed route's bits) runs the adapter inside
    the tile kernels: ``v = s * x @ lora_A.T`` by ``ops.lora_shrink``, then ``ops.linear_forward_lut4_lora`` in one launch, and
    ``ops.linear_backward_input_lut4_lora`` for ``x.grad``; no float32 [T, N] or [T, K] tensor exists.  That route rounds
    ``v``, ``lora_B``, ``dv`` and ``lora_A`` once to bfloat16 on their way into the matrix cores.  It has no ``split_k`` form:
    the two together raise ``ValueError``."""

    def __init__(self, in_features: int, out_features: int, rank: int, alpha: float | None = None, bias: bool = False,
                 input_grad: bool = True, block: int = 64, split_k: bool = False, fused: bool = False):
        del input_grad                                                                 # (always on: the layer is for training)
        if fused and split_k:
            raise ValueError("fused=True runs the tile kernel's adapter stage; it has no split_k form")
        super().__init__(in_features, out_features, bias=bias, input_grad=True, block=block, split_k=split_k)
        self.fused = bool(fused)
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
    def from_bnb(cls, *args, **kwargs) -> "LoRANF4Linear":
        """``NF4Linear.from_bnb`` with ``rank=`` (and ``alpha=``, ``fused=``) among the keywords (``from_linear`` takes them
        the same way); the adapters are created on the device of the codes."""
        module = super().from_bnb(*args, **kwargs)
        return module._adapters_to(module.codes.device)

    @classmethod
    def from_layer(cls, layer: NF4Linear, rank: int, alpha: float | None = None, fused: bool = False) -> "LoRANF4Linear":
        """Wrap an existing ``NF4Linear``; the new module shares its buffers (no copy)."""
        module = cls(layer.in_features, layer.out_features, rank, alpha, bias=layer.bias is not None, block=layer.block,
                     split_k=layer.split_k, fused=fused)
        for name, buf in layer.named_buffers():
            setattr(module, name, buf)
        return module._adapters_to(layer.codes.device)

    def adapter_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if k in ("lora_A", "lora_B")}

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("LoRANF4Linear runs on the GPU (the adapter path has no CPU fallback)")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise RuntimeError(f"LoRANF4Linear: the last dimension of the input must be in_features = {self.in_features}, "
                               f"got {list(x.shape)}")
        from . import ops
        y = ops.linear_lora_forward_lut4(x.reshape(-1, self.in_features), self.codes, self.absmax, self.lora_A, self.lora_B,
                                         self.scaling, self.code_book, self.block, bias=self.bias, split_k=self.split_k,
                                         fused=self.fused)
        return y.reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, rank={self.rank}, alpha={self.alpha:g}" + (", fused=True" if self.fused else "")
