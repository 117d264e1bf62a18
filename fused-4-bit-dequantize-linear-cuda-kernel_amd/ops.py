"""Operator boundary: tensor checks + raw-pointer calls into libfql_int4.so.

``linear_forward`` mirrors ``fused_quant_linear_cuda.forward`` (reference
csrc/quantized_linear.cpp:22-28 and the checks of csrc/quantized_linear_kernel.cu:293-378);
``moe_forward`` mirrors ``moe_int4_cuda.forward`` (reference csrc/moe_int4_kernel.cu:93-141).
Outputs are allocated here with torch (``torch.empty``), launches go to torch's current
stream, nothing synchronises.  GPU tensors only -- a CPU tensor raises, exactly like the
reference's TORCH_CHECK(input.is_cuda()).

Every op is built from the same few steps (DESIGN.md "The operator boundary"): ``_expert_table`` converts and checks
the expert table, ``_check_weights`` / ``_check_group_weights`` / ``_check_mxfp4`` / ``_check_bias`` the weight operands, ``_on`` the
device of anything else, and every launch of a product op goes through ``_launch`` (the tuning hook ``tune_gemm_i8`` and
the size / capability queries call the library directly).
"""
from __future__ import annotations

import torch

from . import _native

_PRECISIONS = {"default": _native.PRECISION_DEFAULT, "exact": _native.PRECISION_EXACT,
               "fast": _native.PRECISION_FAST, "int8": _native.PRECISION_INT8, "fp8": _native.PRECISION_FP8,
               0: 0, 1: 1, 2: 2, 3: 3, 8: 8}
_DTYPES = {torch.float32: _native.DTYPE_F32, torch.float16: _native.DTYPE_F16, torch.bfloat16: _native.DTYPE_BF16}


def _planes(prec):
    """Byte planes of the activation workspace: 3 / 2 / 1 int8 limbs, or one plane of e4m3 values."""
    return {0: 3, 8: 1}.get(prec, prec)


def _precision(p):
    try:
        return _PRECISIONS[p]
    except KeyError:
        raise ValueError(f"precision must be 'default', 'exact', 'fast', 'int8' or 'fp8', got {p!r}") from None


ACTIVATIONS = ("silu", "gelu_tanh", "swiglu_clamp")
_ACTIVATIONS = {"silu": _native.ACT_SILU, "gelu_tanh": _native.ACT_GELU_TANH, "gelu_pytorch_tanh": _native.ACT_GELU_TANH,
                "swiglu_clamp": _native.ACT_SWIGLU_CLAMP}


def activation_of(activation="silu", activation_alpha=1.702, activation_limit=7.0):
    """The activation arguments of the gated FFN ops and layers as ``(kind, alpha, limit)``: ``kind`` one of
    ``ACTIVATIONS`` (``"gelu_pytorch_tanh"``, Hugging Face's name, is ``"gelu_tanh"``), ``alpha`` finite, ``limit``
    finite and > 0 (both used by ``"swiglu_clamp"`` only; the defaults are gpt-oss's)."""
    if not isinstance(activation, str) or activation not in _ACTIVATIONS:
        raise ValueError(f"activation must be 'silu', 'gelu_tanh' (alias 'gelu_pytorch_tanh') or 'swiglu_clamp', got "
                         f"{activation!r}")
    kind = "gelu_tanh" if activation == "gelu_pytorch_tanh" else activation
    try:
        alpha, limit = float(activation_alpha), float(activation_limit)
    except (TypeError, ValueError):
        raise ValueError("activation_alpha and activation_limit must be numbers") from None
    if alpha != alpha or alpha in (float("inf"), float("-inf")):
        raise ValueError(f"activation_alpha must be finite, got {activation_alpha!r}")
    if limit != limit or limit == float("inf") or not limit > 0.0:
        raise ValueError(f"activation_limit must be finite and > 0, got {activation_limit!r}")
    return kind, alpha, limit


def _stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# The shared steps of every op.  A wrong-shaped, wrong-typed, CPU or foreign-device tensor must become a Python error
# in one of the checkers, never an out-of-bounds read or a host pointer inside a kernel.
# ---------------------------------------------------------------------------------------------------------------------

def _launch(name, dev, *args, ws_bytes=None, after=()):
    """Call the library's ``name`` on torch's current stream of ``dev`` and raise under that name if it refuses.
    Tensors among ``args`` are passed as tensors (or None for NULL) and become pointers here, so everything a launch
    reads must outlive the launch by construction: this frame holds it until the call has returned.  ``ws_bytes`` (for
    the ops that have one) allocates the workspace and appends ``workspace, workspace_bytes``; then comes the stream, then
    ``after`` (plain values) for the one signature that goes on behind it."""
    fn = getattr(_native.lib(), name)
    idx = dev.index     # torch.cuda.device() and current_stream() resolve a torch.device in Python (1.7 us each), an int not
    with torch.cuda.device(idx):
        ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        if ws_bytes is not None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
            ptrs += (None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel())
        rc = fn(*ptrs, torch.cuda.current_stream(idx).cuda_stream, *after)
    _native.check(rc, name)


def _on(dev, **tensors):
    """Every named tensor (None passes) lives on the GPU ``dev``."""
    for name, t in tensors.items():
        if t is not None and (not t.is_cuda or t.device != dev):
            raise RuntimeError(f"{name} must be a CUDA tensor on the inputs' device")


def _expert_table(tokens_per_expert, input_offsets, E, dev, optional=False):
    """The device-side expert table as the kernels read it: ``(tokens_per_expert, input_offsets)``, int32 [E], contiguous,
    on ``dev`` (consumed there, no .item()).  ``optional``: both None gives (None, None), one segment of all rows
    (E == 1)."""
    if optional and (tokens_per_expert is None or input_offsets is None):
        if tokens_per_expert is not None or input_offsets is not None:
            raise RuntimeError("tokens_per_expert and input_offsets must be given together")
        if E != 1:
            raise RuntimeError("tokens_per_expert and input_offsets are required when there is more than one expert")
        return None, None
    for name, t in (("tokens_per_expert", tokens_per_expert), ("input_offsets", input_offsets)):
        if not t.is_cuda or t.device != dev:
            raise RuntimeError(f"{name} must be a CUDA tensor on the inputs' device")
        if t.numel() != E:
            raise RuntimeError("tokens_per_expert and input_offsets must have num_experts elements")
    return tokens_per_expert.to(dtype=torch.int32).contiguous(), input_offsets.to(dtype=torch.int32).contiguous()


def _check_packed(packed_weights, dev, K=None, grouped=False):
    """``packed_weights`` uint8 [N, K/2] (``grouped``: [E, N, K/2]) on ``dev``, K / 2 matching ``K`` when given.  Returns
    ``(E, N, K / 2)``."""
    if not packed_weights.is_cuda or packed_weights.device != dev:
        raise RuntimeError("packed_weights must be a CUDA tensor on the inputs' device")
    if packed_weights.dtype != torch.uint8 or packed_weights.dim() != (3 if grouped else 2):
        raise RuntimeError("packed_weights must be uint8 " + ("[num_experts, ffn_dim, hidden_dim/2]" if grouped
                                                              else "[output_dim, input_dim/2]"))
    N, packed_dim = packed_weights.shape[-2:]
    if K is not None and packed_dim * 2 != K:
        raise RuntimeError("packed_weights dim 2 must be hidden_dim / 2" if grouped
                           else "packed_weights dim 1 must be input_dim / 2")
    return (packed_weights.shape[0] if grouped else 1), N, packed_dim


def _check_weights(packed_weights, scales, zero_points, dev, K=None, grouped=False):
    """The per-row weight triple on ``dev``: ``packed_weights`` uint8 [N, K/2] with float32 ``scales`` / ``zero_points``
    of N elements, or (``grouped``) [E, N, K/2] with [E, N].  Returns ``(packed_weights, scales, zero_points, E, N, K)``,
    the tensors contiguous, E = 1 for one matrix."""
    E, N, packed_dim = _check_packed(packed_weights, dev, K, grouped)
    for name, t in (("scales", scales), ("zero_points", zero_points)):
        if not t.is_cuda or t.device != dev:
            raise RuntimeError(f"{name} must be a CUDA tensor on the inputs' device")
        if t.dtype != torch.float32 or (tuple(t.shape) != (E, N) if grouped else t.numel() != N):
            raise RuntimeError(f"{name} must be float32 " + ("[num_experts, ffn_dim]" if grouped
                                                             else "with output_dim elements"))
    return packed_weights.contiguous(), scales.contiguous(), zero_points.contiguous(), E, N, 2 * packed_dim


def _check_group_weights(packed_weights, scales, zero_points, dev, K):
    """The per-group weight triple on ``dev``: ``packed_weights`` uint8 [N, K/2] or [E, N, K/2], float32 ``scales`` /
    ``zero_points`` [N, K / group_size] or [E, N, K / group_size] with an even group size.  Returns
    ``(packed_weights, scales, zero_points, group_size)``, the tensors contiguous."""
    _on(dev, packed_weights=packed_weights, scales=scales, zero_points=zero_points)
    if packed_weights.dtype != torch.uint8:
        raise RuntimeError("packed_weights must be uint8")
    if scales.dtype != torch.float32 or zero_points.dtype != torch.float32:
        raise RuntimeError("scales and zero_points must be float32")
    if scales.dim() != packed_weights.dim() or scales.shape[:-1] != packed_weights.shape[:-1] \
            or zero_points.shape != scales.shape or scales.shape[-1] == 0 or K % scales.shape[-1] != 0:
        raise RuntimeError("per-group scales and zero_points must be [output_dim, input_dim / group_size] "
                           "([E, N, K / group_size] for experts)")
    group = K // scales.shape[-1]
    if group % 2 != 0:
        raise RuntimeError("group_size must be even")
    return packed_weights.contiguous(), scales.contiguous(), zero_points.contiguous(), group


def _expert_group(scales):
    """Whether the experts' ``scales`` are per group along K: [E, N, K / group_size] with more than one group."""
    return isinstance(scales, torch.Tensor) and scales.dim() == 3 and scales.shape[-1] > 1


def _expert_weights(packed_weights, scales, zero_points, dev, K=None):
    """The weight triple of the grouped ops: per row (``_check_weights(grouped=True)``) or, with 3-D ``scales``, per group
    along K (``_check_group_weights``).  A last dimension of 1 is per-row and is passed on as [E, N].  Returns
    ``(packed_weights, scales, zero_points, E, N, K, group_size)``, ``group_size`` None for per-row weights."""
    if _expert_group(scales):
        E, N, packed_dim = _check_packed(packed_weights, dev, K, grouped=True)
        return (*_check_group_weights(packed_weights, scales, zero_points, dev, 2 * packed_dim)[:3], E, N, 2 * packed_dim,
                2 * packed_dim // scales.shape[-1])
    if isinstance(scales, torch.Tensor) and scales.dim() == 3 and isinstance(zero_points, torch.Tensor) \
            and zero_points.dim() == 3 and zero_points.shape[-1] == 1:
        scales, zero_points = scales[..., 0], zero_points[..., 0]
    return (*_check_weights(packed_weights, scales, zero_points, dev, K, grouped=True), None)


def _moe_group_launch(packed_weights, scales, zero_points, rows, tpe, offs, bias, out_dtype, E, N, K, group, precision,
                      act=None):
    """The grouped GEMM on per-group weights: ``fql_moe_group_fwd`` on ``rows`` [T, K], or (``act``: the triple of
    ``activation_of``) ``fql_moe_group_glu_fwd`` on gate|up rows [T, 2K].  Rows and result in any of the three types; the
    library stages what its float32 kernels need (include/fql_int4.h), torch touches no [T, .] tensor here."""
    prec = _group_precision(precision)
    T, dev = rows.shape[0], rows.device
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    ws_bytes = _native.lib().fql_moe_group_typed_workspace_bytes(E, T, K, N, group, prec)
    if act is None:
        _launch("fql_moe_group_fwd", dev, packed_weights, scales, zero_points, rows.contiguous(), _DTYPES[rows.dtype], tpe,
                offs, bias, out, _DTYPES[out_dtype], E, T, K, N, group, prec, ws_bytes=ws_bytes)
    else:
        _launch("fql_moe_group_glu_fwd", dev, packed_weights, scales, zero_points, rows.contiguous(), _DTYPES[rows.dtype],
                tpe, offs, bias, out, _DTYPES[out_dtype], E, T, K, N, group, prec, _ACTIVATIONS[act[0]], act[1], act[2],
                ws_bytes=ws_bytes)
    return out


def _group_precision(precision):
    prec = _precision(precision)
    if prec == _native.PRECISION_FP8:
        raise RuntimeError("precision='fp8' is not available with per-group weights")
    return prec


def _check_bias(bias, N, dev, E=None):
    """``bias`` None, or float32 with N elements on ``dev`` (returned contiguous).  ``E``: the per-expert bias of a grouped
    GEMM, float32 [E, N]."""
    if bias is None:
        return None
    if E is not None:
        if not bias.is_cuda or bias.device != dev or bias.dtype != torch.float32 or tuple(bias.shape) != (E, N):
            raise RuntimeError("bias must be a float32 [num_experts, ffn_dim] tensor on the inputs' device")
        return bias.contiguous()
    if not bias.is_cuda or bias.device != dev or bias.dtype != torch.float32 or bias.numel() != N:
        raise RuntimeError("bias must be a float32 tensor with output_dim elements on the input's device")
    return bias.contiguous()


def linear_forward(input, packed_weights, scales, zero_points, precision="default", bias=None):
    """Fused 4-bit dequantize + linear forward.  input [K] or [B,K] float32 -> [N] or [B,N].
    ``bias`` [N] float32 (optional, not in the reference: python/module.py:84) is added in the kernels' epilogues.
    Under autograd (grad mode on, ``input`` or ``bias`` requiring grad) the input gradient runs on the GPU too."""
    if _wants_grad(input, bias):
        return _LinearFn.apply(input, packed_weights, scales, zero_points, bias, precision, None, False)
    squeeze = False
    if input.dim() == 1:                                   # :302-306
        input = input.unsqueeze(0)
        squeeze = True
    # device / layout / dtype checks, same order and wording as :311-335 (hence not _check_weights)
    if not input.is_cuda:
        raise RuntimeError("input must be a CUDA tensor")
    if not packed_weights.is_cuda:
        raise RuntimeError("packed_weights must be a CUDA tensor")
    if not scales.is_cuda:
        raise RuntimeError("scales must be a CUDA tensor")
    if not zero_points.is_cuda:
        raise RuntimeError("zero_points must be a CUDA tensor")
    if not input.is_contiguous():
        raise RuntimeError("input must be contiguous")
    if not packed_weights.is_contiguous():
        raise RuntimeError("packed_weights must be contiguous")
    if input.dtype != torch.float32:
        raise RuntimeError("input must be float32")
    if packed_weights.dtype != torch.uint8:
        raise RuntimeError("packed_weights must be uint8")
    if scales.dtype != torch.float32:
        raise RuntimeError("scales must be float32")
    if zero_points.dtype != torch.float32:
        raise RuntimeError("zero_points must be float32")
    if input.dim() != 2 or packed_weights.dim() != 2:
        raise RuntimeError("input must be 1-D or 2-D and packed_weights 2-D")
    B, K = input.shape
    N, packed_dim = packed_weights.shape
    if packed_dim != K // 2 or K % 2 != 0:
        raise RuntimeError("packed_weights dim 1 must be input_dim / 2")
    dev = input.device
    if _per_group(scales):                                  # per-group scales along K (float32 contraction: include/fql_int4.h)
        out = _linear_group_forward(input, packed_weights, scales, zero_points, bias, precision)
        return out.squeeze(0) if squeeze else out
    # not checked by the reference (silent UB there); checked here
    if scales.numel() != N or zero_points.numel() != N:
        raise RuntimeError("scales and zero_points must have output_dim elements")
    if packed_weights.device != dev or scales.device != dev or zero_points.device != dev:
        raise RuntimeError("all tensors must be on the same device")
    bias = _check_bias(bias, N, dev)
    prec = _precision(precision)
    out = torch.empty((B, N), dtype=torch.float32, device=dev)     # :338
    _launch("fql_linear_bias_fwd_f32", dev, input, packed_weights, scales.contiguous(), zero_points.contiguous(), bias,
            out, B, K, N, prec, ws_bytes=_native.lib().fql_linear_workspace_bytes(B, K, N, prec))
    return out.squeeze(0) if squeeze else out                      # :373-375


def _per_group(scales):
    return scales.dim() == 2 and scales.shape[1] > 1


def _linear_group_forward(input, packed_weights, scales, zero_points, bias, precision="default"):
    """Per-group scales along K (``scales`` / ``zero_points`` [N, K / group_size]): fql_linear_group_ws_fwd_f32."""
    B, K = input.shape
    N = packed_weights.shape[0]
    dev = input.device
    packed_weights, scales, zero_points, group = _check_group_weights(packed_weights, scales, zero_points, dev, K)
    bias = _check_bias(bias, N, dev)
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    prec = _precision(precision)
    _launch("fql_linear_group_ws_fwd_f32", dev, input.contiguous(), packed_weights, scales, zero_points, bias, out,
            B, K, N, group, prec, ws_bytes=_native.lib().fql_group_workspace_bytes(1, B, K, N, group, prec))
    return out


def moe_group_forward(packed_weights, scales, zero_points, inputs, tokens_per_expert, input_offsets, precision="default"):
    """Grouped per-expert INT4 GEMM with per-GROUP scales along K: ``scales`` / ``zero_points`` [E, N, K / group_size].
    Batches of 8+ rows per expert run on the INT8 matrix cores (limb accumulators folded in float32 per group), smaller
    ones on the float32 matrix-core / FMA kernels (include/fql_int4.h); rows no expert covers are zero."""
    _forward_only("moe_group_forward", inputs)
    if not inputs.is_cuda or inputs.dtype != torch.float32 or inputs.dim() != 2 or packed_weights.dim() != 3:
        raise RuntimeError("inputs must be a CUDA float32 [T, K] tensor and packed_weights [E, N, K/2]")
    E, N, K2 = packed_weights.shape
    T, K = inputs.shape
    if K != 2 * K2:
        raise RuntimeError("packed_weights dim 2 must be hidden_dim / 2")
    dev = inputs.device
    packed_weights, scales, zero_points, group = _check_group_weights(packed_weights, scales, zero_points, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    out = torch.empty((T, N), dtype=torch.float32, device=dev)
    prec = _precision(precision)
    _launch("fql_moe_group_ws_fwd_f32", dev, packed_weights, scales, zero_points, inputs.contiguous(), tpe, offs, out,
            E, T, K, N, group, prec, ws_bytes=_native.lib().fql_group_workspace_bytes(E, T, K, N, group, prec))
    return out


def moe_forward(packed_weights, scales, zero_points, inputs, expert_ids, tokens_per_expert,
                input_offsets, precision="default", bias=None):
    """Grouped per-expert INT4 GEMM over rows pre-grouped by expert.

    packed_weights [E,N,K/2] u8, scales/zero_points [E,N] f32 (or per group along K: [E,N,K/group_size], the layout
    of ``quantize_weights(group_size=)``), inputs [T,K] f32,
    tokens_per_expert / input_offsets [E] int32 on the device (consumed there, no .item()).
    ``expert_ids`` is accepted and ignored, as in the reference (csrc/moe_int4_kernel.cu:98).
    Returns [T,N] float32; rows covered by no expert are zero (reference: torch::zeros :109).
    ``bias`` [E,N] float32 (optional, not in the reference): expert e's bias is added to the rows of expert e in the
    kernels' epilogues; rows no expert covers stay zero.  Without it the call is what it always was.
    Under autograd (grad mode on, ``inputs`` or ``bias`` requiring grad) the input gradient runs on the GPU too, and the
    bias gradient is ``moe_bias_grad``.
    """
    del expert_ids
    if _wants_grad(inputs, bias):
        return _MoEFn.apply(inputs, packed_weights, scales, zero_points, tokens_per_expert, input_offsets, precision,
                            None, False, bias)
    if not inputs.is_cuda:
        raise RuntimeError("inputs must be a CUDA tensor")
    if inputs.dtype != torch.float32 or inputs.dim() != 2:
        raise RuntimeError("inputs must be float32 [total_tokens, hidden_dim]")
    T, K = inputs.shape
    dev = inputs.device
    packed_weights, scales, zero_points, E, N, _, group = _expert_weights(packed_weights, scales, zero_points, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    if group is not None:
        return _moe_group_launch(packed_weights, scales, zero_points, inputs, tpe, offs, bias, torch.float32, E, N, K,
                                 group, precision)
    prec = _precision(precision)
    out = torch.empty((T, N), dtype=torch.float32, device=dev)
    if bias is not None:
        _launch("fql_moe_bias_fwd", dev, packed_weights, scales, zero_points, inputs.contiguous(), _native.DTYPE_F32, tpe,
                offs, bias, out, _native.DTYPE_F32, E, T, K, N, prec,
                ws_bytes=_native.lib().fql_moe_workspace_bytes(E, T, K, N, prec))
        return out
    _launch("fql_moe_fwd_f32", dev, packed_weights, scales, zero_points, inputs.contiguous(), tpe, offs, out,
            E, T, K, N, prec, ws_bytes=_native.lib().fql_moe_workspace_bytes(E, T, K, N, prec))
    return out


def linear_forward_any(input, packed_weights, scales, zero_points, precision="default", out_dtype=None, bias=None):
    """``linear_forward`` for float32 / float16 / bfloat16 activations, output in ``out_dtype`` (default: the
    input's).  Equal bit for bit to ``linear_forward(input.float(), bias=bias).to(out_dtype)``; on the MFMA path the
    two conversion passes are fused into the kernels, elsewhere torch converts."""
    out_dtype = input.dtype if out_dtype is None else out_dtype
    if input.dtype not in _DTYPES or out_dtype not in _DTYPES:
        raise RuntimeError("activations and outputs must be float32, float16 or bfloat16")
    if _wants_grad(input, bias):
        return _LinearFn.apply(input, packed_weights, scales, zero_points, bias, precision, out_dtype, True)
    if input.dtype == torch.float32 and out_dtype == torch.float32:
        return linear_forward(input, packed_weights, scales, zero_points, precision=precision, bias=bias)
    x2 = input.unsqueeze(0) if input.dim() == 1 else input
    prec = _precision(precision)
    L = _native.lib()
    native = (x2.is_cuda and x2.dim() == 2 and x2.is_contiguous() and packed_weights.is_cuda
              and packed_weights.dtype == torch.uint8 and packed_weights.dim() == 2 and packed_weights.is_contiguous()
              and packed_weights.shape[1] * 2 == x2.shape[1]
              and L.fql_native_dtype_supported(x2.shape[0], 1, x2.shape[1], packed_weights.shape[0], prec,
                                               packed_weights.data_ptr(), 0) == 1)
    if not native:
        return linear_forward(input.float().contiguous(), packed_weights, scales, zero_points,
                              precision=precision, bias=bias).to(out_dtype)
    B, K = x2.shape
    dev = x2.device
    packed_weights, scales, zero_points, _, N, _ = _check_weights(packed_weights, scales, zero_points, dev, K)
    bias = _check_bias(bias, N, dev)
    out = torch.empty((B, N), dtype=out_dtype, device=dev)
    _launch("fql_linear_bias_fwd", dev, x2, _DTYPES[x2.dtype], packed_weights, scales, zero_points, bias, out,
            _DTYPES[out_dtype], B, K, N, prec, ws_bytes=L.fql_linear_workspace_bytes(B, K, N, prec))
    return out.squeeze(0) if input.dim() == 1 else out


def moe_forward_any(packed_weights, scales, zero_points, inputs, expert_ids, tokens_per_expert, input_offsets,
                    precision="default", out_dtype=None, bias=None):
    """``moe_forward`` for float32 / float16 / bfloat16 rows (the reference's MoE benches feed float16,
    benchmark/moe_grouped_gemm/moe_int4_module.py:161-165), output in ``out_dtype`` (default: the input's).
    Equal bit for bit to ``moe_forward(inputs.float(), bias=bias).to(out_dtype)``: a 16-bit result is rounded once, after
    the per-expert ``bias`` [E, N] float32 (optional)."""
    out_dtype = inputs.dtype if out_dtype is None else out_dtype
    if inputs.dtype not in _DTYPES or out_dtype not in _DTYPES:
        raise RuntimeError("activations and outputs must be float32, float16 or bfloat16")
    if _wants_grad(inputs, bias):
        return _MoEFn.apply(inputs, packed_weights, scales, zero_points, tokens_per_expert, input_offsets, precision,
                            out_dtype, True, bias)
    if inputs.dtype == torch.float32 and out_dtype == torch.float32:
        return moe_forward(packed_weights, scales, zero_points, inputs, expert_ids, tokens_per_expert, input_offsets,
                           precision=precision, bias=bias)
    if _expert_group(scales):                               # per-group weights: the library takes every type and shape
        if not inputs.is_cuda or inputs.dim() != 2:
            raise RuntimeError("inputs must be a CUDA [total_tokens, hidden_dim] tensor")
        T, K = inputs.shape
        dev = inputs.device
        packed_weights, scales, zero_points, E, N, _, group = _expert_weights(packed_weights, scales, zero_points, dev, K)
        tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
        return _moe_group_launch(packed_weights, scales, zero_points, inputs, tpe, offs, _check_bias(bias, N, dev, E),
                                 out_dtype, E, N, K, group, precision)
    prec = _precision(precision)
    L = _native.lib()
    ok = (inputs.is_cuda and inputs.dim() == 2 and packed_weights.is_cuda and packed_weights.dim() == 3
          and packed_weights.dtype == torch.uint8 and packed_weights.shape[2] * 2 == inputs.shape[1])
    native = ok and L.fql_native_dtype_supported(inputs.shape[0], packed_weights.shape[0], inputs.shape[1],
                                                 packed_weights.shape[1], prec, packed_weights.data_ptr(), 1) == 1
    if not native:
        return moe_forward(packed_weights, scales, zero_points, inputs.float().contiguous(), expert_ids,
                           tokens_per_expert, input_offsets, precision=precision, bias=bias).to(out_dtype)
    T, K = inputs.shape
    dev = inputs.device
    packed_weights, scales, zero_points, E, N, _, _ = _expert_weights(packed_weights, scales, zero_points, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    if bias is not None:
        _launch("fql_moe_bias_fwd", dev, packed_weights, scales, zero_points, inputs.contiguous(), _DTYPES[inputs.dtype],
                tpe, offs, bias, out, _DTYPES[out_dtype], E, T, K, N, prec,
                ws_bytes=L.fql_moe_workspace_bytes(E, T, K, N, prec))
        return out
    _launch("fql_moe_fwd", dev, packed_weights, scales, zero_points, inputs.contiguous(), _DTYPES[inputs.dtype], tpe,
            offs, out, _DTYPES[out_dtype], E, T, K, N, prec, ws_bytes=L.fql_moe_workspace_bytes(E, T, K, N, prec))
    return out


def moe_gather_forward(packed_weights, scales, zero_points, tokens, row_index, tokens_per_expert,
                       input_offsets, precision="default", row_weight=None):
    """Grouped per-expert INT4 GEMM with the dispatch gather fused in: grouped row t = tokens[row_index[t]].
    ``row_weight`` [T] float32 (optional): grouped row t of the result is multiplied by row_weight[t] in the GEMM epilogue
    (the routing weight of its (token, slot) pair), so that ``combine(y, pos, None)`` is a pure gather-add.

    ``tokens`` [n_tokens, K] float32 in token order, ``row_index`` [T] int32 (e.g. from
    ``routing.dispatch_indices``).  Returns the grouped outputs [T, N]; un-sort / combine with
    ``routing.combine_grouped``.  The [T, K] gathered activations are never materialised."""
    _forward_only("moe_gather_forward", tokens, row_weight)
    if not tokens.is_cuda:
        raise RuntimeError("tokens must be a CUDA tensor")
    if tokens.dtype != torch.float32 or tokens.dim() != 2:
        raise RuntimeError("tokens must be float32 [n_tokens, hidden_dim]")
    n_tokens, K = tokens.shape
    dev = tokens.device
    if not row_index.is_cuda:
        raise RuntimeError("row_index must be a CUDA tensor")
    packed_weights, scales, zero_points, E, N, _ = _check_weights(packed_weights, scales, zero_points, dev, K, grouped=True)
    if K % 32 != 0:
        raise RuntimeError("fused gather needs hidden_dim % 32 == 0")
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    T = row_index.numel()
    ri = row_index.to(device=dev, dtype=torch.int32).contiguous()
    if row_weight is not None:
        if not row_weight.is_cuda or row_weight.device != dev or row_weight.numel() != T:
            raise RuntimeError("row_weight must be a CUDA tensor with one element per grouped row")
        row_weight = row_weight.to(torch.float32).contiguous()
    prec = _precision(precision)
    ws_bytes = _native.lib().fql_moe_workspace_bytes(E, T, K, N, prec)
    out = torch.empty((T, N), dtype=torch.float32, device=dev)
    if row_weight is None:
        _launch("fql_moe_gather_fwd_f32", dev, packed_weights, scales, zero_points, tokens.contiguous(), ri, n_tokens,
                tpe, offs, out, E, T, K, N, prec, ws_bytes=ws_bytes)
        return out
    _launch("fql_moe_gather_scaled_fwd_f32", dev, packed_weights, scales, zero_points, tokens.contiguous(), ri, n_tokens,
            row_weight, tpe, offs, out, E, T, K, N, prec, ws_bytes=ws_bytes)
    return out


def moe_gated_forward(packed_weights, scales, zero_points, gate_up, tokens_per_expert, input_offsets,
                      precision="default", out_dtype=None, activation="silu", activation_alpha=1.702,
                      activation_limit=7.0, bias=None):
    """Second GEMM of a gated FFN expert with the activation fused into its pre-pass:
    ``out[t] = W_e @ (silu(gate_up[t, :K]) * gate_up[t, K:])``; ``gate_up`` [T, 2K] float32 / float16 / bfloat16 (the
    output of the fused gate|up projection), ``packed_weights`` [E, N, K/2].  The [T, K] hidden activation is never
    written.  The result has ``out_dtype`` (default: ``gate_up``'s type); a 16-bit ``gate_up`` is read as it is and a
    16-bit result is rounded once: bit for bit ``moe_gated_forward(gate_up.float()).to(out_dtype)``.
    ``activation``: ``"silu"``, ``"gelu_tanh"`` (GeGLU) or ``"swiglu_clamp"`` (gpt-oss, with ``activation_alpha`` and
    ``activation_limit``) in place of silu(g) * u (``activation_of``).
    ``bias`` [E, N] float32 (optional): expert e's bias is added to the rows of expert e in the GEMM's epilogue, before
    the one rounding of a 16-bit result; rows no expert covers stay zero.
    Per-group ``scales`` / ``zero_points`` [E, N, K / group_size] take ``fql_moe_group_glu_fwd``: h stays out of memory on
    the integer path only (K % 256 == 0, group_size % 64 == 0, 8+ rows per expert)."""
    _forward_only("moe_gated_forward", gate_up, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    if not gate_up.is_cuda or gate_up.dtype not in _DTYPES or gate_up.dim() != 2:
        raise RuntimeError("gate_up must be a CUDA float32 (or float16 / bfloat16) [T, 2K] tensor")
    out_dtype = gate_up.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    T, K2 = gate_up.shape
    K = K2 // 2
    dev = gate_up.device
    if K2 % 2 or K % 32:
        raise RuntimeError("gate_up must be [T, 2K] with K % 32 == 0")
    packed_weights, scales, zero_points, E, N, _, group = _expert_weights(packed_weights, scales, zero_points, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    if group is not None:
        return _moe_group_launch(packed_weights, scales, zero_points, gate_up, tpe, offs, bias, out_dtype, E, N, K, group,
                                 precision, act=(kind, act_alpha, act_limit))
    L = _native.lib()
    prec = _precision(precision)
    typed = gate_up.dtype != torch.float32 or out_dtype != torch.float32
    round_to = None
    if typed and T > 0 and L.fql_native_dtype_supported(T, E, K, N, prec, packed_weights.data_ptr(), 1) != 1:
        # off the 16-bit MFMA path: widen and round around the float32 call (the same contract)
        gate_up, round_to, out_dtype = gate_up.float(), out_dtype, torch.float32
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    if bias is not None:
        _launch("fql_moe_glu_bias_fwd", dev, packed_weights, scales, zero_points, gate_up.contiguous(),
                _DTYPES[gate_up.dtype], tpe, offs, bias, out, _DTYPES[out_dtype], E, T, K, N, prec, _ACTIVATIONS[kind],
                act_alpha, act_limit, ws_bytes=L.fql_moe_workspace_bytes(E, T, K, N, prec))
    elif kind == "silu":
        _launch("fql_moe_gated_fwd", dev, packed_weights, scales, zero_points, gate_up.contiguous(), _DTYPES[gate_up.dtype],
                tpe, offs, out, _DTYPES[out_dtype], E, T, K, N, prec, ws_bytes=L.fql_moe_workspace_bytes(E, T, K, N, prec))
    else:
        _launch("fql_moe_glu_fwd", dev, packed_weights, scales, zero_points, gate_up.contiguous(), _DTYPES[gate_up.dtype],
                tpe, offs, out, _DTYPES[out_dtype], E, T, K, N, prec, _ACTIVATIONS[kind], act_alpha, act_limit,
                ws_bytes=L.fql_moe_workspace_bytes(E, T, K, N, prec))
    return out if round_to is None else out.to(round_to)


def _check_mxfp4(blocks, scales, dev, K):
    """The MXFP4 weight pair on ``dev``: ``blocks`` uint8 [E, N, K/2] (two e2m1 codes a byte, even k in the low nibble)
    and ``scales`` uint8 [E, N, K/32] (E8M0), K matching the rows' and a multiple of 32.  Returns
    ``(blocks, scales, E, N)``, the tensors contiguous."""
    _on(dev, blocks=blocks, scales=scales)
    if blocks.dtype != torch.uint8 or blocks.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("blocks must be uint8 [num_experts, N, K/2] and scales uint8 [num_experts, N, K/32]")
    E, N, half = blocks.shape
    if K % 32 != 0 or half * 2 != K or tuple(scales.shape) != (E, N, K // 32):
        raise RuntimeError("blocks must be [num_experts, N, K/2] and scales [num_experts, N, K/32] with K % 32 == 0 the "
                           "rows' width")
    return blocks.contiguous(), scales.contiguous(), E, N


def _mxfp4_precision(precision):
    """``precision`` of the MXFP4 ops, validated: "bf16" (the default), "fp8", "fp6" or "fp4"."""
    if precision not in ("bf16", "fp8", "fp6", "fp4"):
        raise ValueError(f"precision must be 'bf16', 'fp8', 'fp6' or 'fp4' for MXFP4 weights, got {precision!r}")
    return precision


def _mxfp4_launch(name, blocks, scales, rows, K, tokens_per_expert, input_offsets, bias, out_dtype, gated, act=(),
                  precision="bf16"):
    if not rows.is_cuda or rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is refused: rounding "
                           "it to bfloat16 would lose three bits; cast it yourself)")
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    dev, T = rows.device, rows.shape[0]
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)   # (none: one expert, all rows)
    bias = _check_bias(bias, N, dev, E)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    L = _native.lib()
    if precision == "fp8":      # the quantising pre-pass, then the block-scaled fp4 x fp8 GEMM (csrc/fql_gemm_mx4_scaled.h)
        entry, ws = ("fql_moe_mx4_glu_fwd_q8" if gated else "fql_moe_mx4_fwd_q8",
                     L.fql_moe_mx4_f8_workspace_bytes(E, T, K, N, 2 if gated else 1))
    elif precision == "fp4":    # the MXFP4 quantiser, then the block-scaled fp4 x fp4 GEMM (csrc/fql_gemm_mx4_scaled.h)
        entry, ws = ("fql_moe_mx4_glu_fwd_q4" if gated else "fql_moe_mx4_fwd_q4",
                     L.fql_moe_mx4_f4_workspace_bytes(E, T, K, N, 2 if gated else 1))
    elif precision == "fp6":    # the MXFP6 quantiser, then the block-scaled fp4 x e2m3 GEMM (csrc/fql_gemm_mx4_scaled.h)
        entry, ws = ("fql_moe_mx4_glu_fwd_q6" if gated else "fql_moe_mx4_fwd_q6",
                     L.fql_moe_mx4_f6_workspace_bytes(E, T, K, N, 2 if gated else 1))
    else:
        entry, ws = "fql_moe_mx4_glu_fwd" if gated else "fql_moe_mx4_fwd", L.fql_moe_mx4_workspace_bytes(E, T, K, N, int(gated))
    _launch(entry, dev, blocks, scales, rows.contiguous(), _DTYPES[rows.dtype], bias, tpe, offs, out, _DTYPES[out_dtype],
            E, T, K, N, *act, ws_bytes=ws)
    return out


def moe_forward_mxfp4(blocks, scales, inputs, tokens_per_expert, input_offsets, bias=None, out_dtype=None, precision="bf16"):
    """The grouped GEMM on OCP MXFP4 expert weights: ``out[t] = W_e @ bf16(inputs[t]) (+ bias[e])`` over the rows of expert
    e.  ``blocks`` uint8 [E, N, K/2], ``scales`` uint8 [E, N, K/32] (``quantize.quantize_mxfp4``); ``inputs`` [T, K] float32
    (rounded once to bfloat16) or bfloat16; ``bias`` [E, N] float32 (optional), added before the one rounding to
    ``out_dtype`` (default: the inputs' type).  The weights are exact in bfloat16 and the contraction accumulates in
    float32 on the bfloat16 matrix cores; rows no expert covers are zero.  Forward only.
    Small batches (T up to the library's decode threshold) take a decode kernel that streams the weights once with one
    wave per 32 weight rows instead of the 64-row tile; the two return the same bits, so the result does not depend on T.
    Every precision has such a pair (each with a threshold of its own, set from a measurement), behind its pre-pass.

    ``precision="fp8"`` is the opt-in mode on the block-scaled FP4 matrix cores: the rows are quantised per row to OCP e4m3
    (``quantize_activations_fp8``'s rule, inside a fused pre-pass) and contracted with the packed weights and their E8M0
    scales as they are: ``out[t] = act_scale[t] * (W_e @ e4m3(inputs[t] / act_scale[t])) (+ bias[e])``.

    ``precision="fp4"`` (W4A4) quantises the rows to MXFP4 themselves, per block of 32 by ``quantize.quantize_mxfp4``'s rule
    (``quantize_rows_mxfp4``, inside a fused pre-pass), and contracts e2m1 with e2m1, each side with its E8M0 scales:
    ``out[t] = W_e @ mxfp4(inputs[t]) (+ bias[e])``.  The format error of the rows is about 1.1e-1 (relative Frobenius).

    ``precision="fp6"`` quantises the rows to MXFP6 (e2m3 elements, per block of 32 by ``quantize.quantize_mxfp6``'s rule:
    ``quantize_rows_mxfp6``, inside a fused pre-pass) and contracts e2m1 with e2m3 at the same matrix rate as ``"fp4"``:
    ``out[t] = W_e @ mxfp6(inputs[t]) (+ bias[e])``.  The format error of Gaussian rows is about 2.8e-2."""
    _forward_only("moe_forward_mxfp4", inputs, bias)
    precision = _mxfp4_precision(precision)
    K = inputs.shape[1] if inputs.dim() == 2 else 0
    return _mxfp4_launch("moe_forward_mxfp4", blocks, scales, inputs, K, tokens_per_expert, input_offsets, bias, out_dtype, False,
                         precision=precision)


def moe_gated_forward_mxfp4(blocks, scales, gate_up, tokens_per_expert, input_offsets, activation="silu",
                            activation_alpha=1.702, activation_limit=7.0, bias=None, out_dtype=None, precision="bf16"):
    """The down projection of a gated FFN expert on MXFP4 weights: ``out[t] = W_e @ bf16(act(gate_up[t, :K], gate_up[t, K:]))
    (+ bias[e])``, ``gate_up`` [T, 2K] float32 or bfloat16, ``blocks`` [E, N, K/2].  The activation (``activation_of``) is
    evaluated in float32 and rounded once to bfloat16 by a streaming pre-pass into the op's workspace: no [T, K] tensor is
    handed back.  Forward only.  Behind the pre-pass, small batches take the decode kernel of
    ``moe_forward_mxfp4`` with the same bits as the tile kernel, in every precision.

    ``precision="fp8"``: the float32 ``h = act(...)`` is quantised per row to e4m3 by the pre-pass instead (never stored as
    floats) and contracted on the block-scaled FP4 matrix cores, as in ``moe_forward_mxfp4``.  ``precision="fp4"``: ``h`` is
    evaluated once in float32 and quantised to MXFP4 per block of 32 (``quantize_rows_mxfp4(gate_up, activation=...)``);
    ``precision="fp6"``: the same with MXFP6 rows (``quantize_rows_mxfp6(gate_up, activation=...)``)."""
    _forward_only("moe_gated_forward_mxfp4", gate_up, bias)
    precision = _mxfp4_precision(precision)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    if gate_up.dim() != 2 or gate_up.shape[1] % 64 != 0:
        raise RuntimeError("gate_up must be [T, 2K] with K % 32 == 0")
    return _mxfp4_launch("moe_gated_forward_mxfp4", blocks, scales, gate_up, gate_up.shape[1] // 2, tokens_per_expert,
                         input_offsets, bias, out_dtype, True, act=(_ACTIVATIONS[kind], act_alpha, act_limit),
                         precision=precision)


def _mxfp4_linear_launch(name, blocks, scales, rows, cols, bias, out_dtype, gated, act, precision, split_k):
    """The two dense MXFP4 ops.  ``rows`` [T, cols] float32 / bfloat16, ``blocks`` [N, K/2], ``scales`` [N, K/32],
    ``bias`` [N] float32 or None.  Types and shapes first, then the devices: the argument errors read the same without a
    GPU."""
    precision = _mxfp4_precision(precision)
    if rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is refused: rounding "
                           "it to bfloat16 would lose three bits; cast it yourself)")
    if blocks.dtype != torch.uint8 or blocks.dim() != 2 or scales.dtype != torch.uint8 or scales.dim() != 2:
        raise RuntimeError("blocks must be uint8 [N, K/2] and scales uint8 [N, K/32]")
    N, K = blocks.shape[0], 2 * blocks.shape[1]
    if K % 32 != 0 or tuple(scales.shape) != (N, K // 32):
        raise RuntimeError("blocks must be [N, K/2] and scales [N, K/32] with K % 32 == 0")
    if rows.shape[1] != cols(K):
        raise RuntimeError(f"ops.{name}: the rows must have {cols(K)} columns for blocks {list(blocks.shape)}")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (N,)):
        raise RuntimeError("bias must be a float32 [N] tensor")
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    if not rows.is_cuda:
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA tensor")
    dev, T = rows.device, rows.shape[0]
    _on(dev, blocks=blocks, scales=scales, bias=bias)
    if precision != "bf16":     # the block-scaled precisions have no split form: the grouped op on the one-expert view
        return _mxfp4_launch(name, blocks[None], scales[None], rows, K, None, None, None if bias is None else bias[None],
                             out_dtype, gated, act=act, precision=precision)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    split = int(bool(split_k))
    _launch("fql_linear_mx4_glu_fwd" if gated else "fql_linear_mx4_fwd", dev, blocks.contiguous(), scales.contiguous(),
            rows.contiguous(), _DTYPES[rows.dtype], None if bias is None else bias.contiguous(), out, _DTYPES[out_dtype],
            T, K, N, *act, split, ws_bytes=_native.lib().fql_linear_mx4_workspace_bytes(T, K, N, int(gated), split))
    return out


def linear_forward_mxfp4(blocks, scales, x, bias=None, out_dtype=None, precision="bf16", split_k=True):
    """A dense linear layer on OCP MXFP4 weights: ``out[t] = W @ bf16(x[t]) (+ bias)``.  ``blocks`` uint8 [N, K/2] and
    ``scales`` uint8 [N, K/32] (``quantize.quantize_mxfp4``, or a checkpoint's tensors); ``x`` [T, K] float32 (rounded
    once to bfloat16) or bfloat16; ``bias`` [N] float32 (optional), added before the one rounding to ``out_dtype``
    (default: ``x``'s type).  Forward only (``linear_backward_input_mxfp4`` is the input gradient).

    ``split_k=False`` is ``moe_forward_mxfp4`` on the one-expert view ``blocks[None]`` without a table: the same kernels,
    the same bits.  ``split_k=True`` (the default) lets a small batch (T up to the library's threshold, on shapes for
    which the library's S(K, N) is above 1) run the decode kernel once per slice of K, S slices side by side, and sum the
    float32 partial results in a fixed order in a second launch: a dense matrix at a few rows has no other axis to fill
    the chip from.  A row's result then depends on its own row and the weights only, not on T or its position, and is
    the same run to run; it is not the tile kernel's bit pattern, so a row's bits may change as T crosses the threshold
    (both are within the float32 bound of the exact product).  INTEGRATION.md section 17.

    ``precision="fp8"``, ``"fp6"`` and ``"fp4"`` are ``moe_forward_mxfp4``'s block-scaled modes on the one-expert view;
    there is no split form there, and ``split_k`` is not looked at."""
    _forward_only("linear_forward_mxfp4", x, bias)
    return _mxfp4_linear_launch("linear_forward_mxfp4", blocks, scales, x, lambda K: K, bias, out_dtype, False, (), precision,
                                split_k)


def linear_gated_forward_mxfp4(blocks, scales, gate_up, activation="silu", activation_alpha=1.702, activation_limit=7.0,
                               bias=None, out_dtype=None, precision="bf16", split_k=True):
    """The down projection of a dense gated MLP on MXFP4 weights: ``out[t] = W @ bf16(act(gate_up[t, :K], gate_up[t, K:]))
    (+ bias)``, ``gate_up`` [T, 2K] float32 or bfloat16, ``blocks`` [N, K/2].  ``moe_gated_forward_mxfp4``'s streaming
    pre-pass into the op's workspace, then ``linear_forward_mxfp4``'s kernels on the bfloat16 ``h``, with the same
    ``split_k``.  The block-scaled precisions go through ``moe_gated_forward_mxfp4`` on the one-expert view: no split form
    there."""
    _forward_only("linear_gated_forward_mxfp4", gate_up, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    return _mxfp4_linear_launch("linear_gated_forward_mxfp4", blocks, scales, gate_up, lambda K: 2 * K, bias, out_dtype, True,
                                (_ACTIVATIONS[kind], act_alpha, act_limit), precision, split_k)


def linear_backward_input_mxfp4(blocks, scales, grad_out, out_dtype=None):
    """``grad_in[t] = bf16(grad_out[t]) @ W`` on dense MXFP4 weights ``blocks`` [N, K/2] / ``scales`` [N, K/32]:
    ``moe_backward_input_mxfp4`` on the one-expert view without a table.  ``grad_out`` [T, N] float32 or bfloat16 -> [T, K]
    ``out_dtype`` (default float32)."""
    if blocks.dim() != 2 or scales.dim() != 2:
        raise RuntimeError("blocks must be uint8 [N, K/2] and scales uint8 [N, K/32]")
    return moe_backward_input_mxfp4(blocks[None], scales[None], grad_out, None, None, out_dtype=out_dtype)


def _nvfp4_lora_operands(name, lora, T, w_shape):
    """The adapter operands of an NVFP4 adapter op, ``lora`` = (the shrunk rows [T, r] float32, the adapter matrix float32
    of ``w_shape(r)``): types and shapes, as ``_mxfp4_lora_launch`` checks them.  Returns the rank."""
    v, w = lora
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 2 or v.shape[0] != T:
        raise RuntimeError(f"ops.{name}: the shrunk rows must be a float32 [T, r] tensor with the rows' T")
    r = v.shape[1]
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != w_shape(r):
        raise RuntimeError(f"ops.{name}: the adapter matrix must be a float32 {list(w_shape(r))} tensor (the adapter "
                           "weights stay float32 whatever the activations' type)")
    return r


def _nvfp4_launch(name, blocks, scales, global_scale, rows, cols, tokens_per_expert, input_offsets, bias, out_dtype, gated,
                  act=(), dense=False, lora=None):
    """The four NVFP4 ops and, with ``lora`` = (v [T, r], lora_B [E, N, r] / dense [N, r]), their adapter forms (the ``_lora``
    entries: always the tile kernel; there is no gated dense one).  ``rows`` [T, cols(K)] float32 / bfloat16; grouped: ``blocks`` [E, N, K/2], ``scales`` [E, N, K/16],
    ``global_scale`` float32 [E] or None, ``bias`` [E, N]; ``dense``: ``blocks`` [N, K/2], ``scales`` [N, K/16],
    ``global_scale`` float32 with one element or None, ``bias`` [N], no table.  Types and shapes first, then the devices:
    the argument errors read the same without a GPU."""
    if rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is refused: rounding "
                           "it to bfloat16 would lose three bits; cast it yourself)")
    wd = 2 if dense else 3
    shape = "[N, K/2] and scales_e4m3 uint8 [N, K/16]" if dense else "[num_experts, N, K/2] and scales_e4m3 uint8 [num_experts, N, K/16]"
    if blocks.dtype != torch.uint8 or blocks.dim() != wd or scales.dtype != torch.uint8 or scales.dim() != wd:
        raise RuntimeError(f"blocks must be uint8 {shape}")
    E = 1 if dense else blocks.shape[0]
    N, K = blocks.shape[-2], 2 * blocks.shape[-1]
    if K % 32 != 0 or tuple(scales.shape) != tuple(blocks.shape[:-1]) + (K // 16,):
        raise RuntimeError(f"blocks must be uint8 {shape} with K % 32 == 0")
    if rows.shape[1] != cols(K):
        raise RuntimeError(f"ops.{name}: the rows must have {cols(K)} columns for blocks {list(blocks.shape)}")
    if global_scale is not None and (not isinstance(global_scale, torch.Tensor) or global_scale.dtype != torch.float32
                                     or global_scale.numel() != E or global_scale.dim() > 1):
        raise RuntimeError(f"global_scale must be a float32 tensor of {E} element(s) (one per expert), or None")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != ((N,) if dense else (E, N))):
        raise RuntimeError("bias must be a float32 [N] tensor" if dense else "bias must be a float32 [num_experts, N] tensor")
    T = rows.shape[0]
    extra, tag = (), ""
    if lora is not None:
        if dense and gated:
            raise RuntimeError(f"ops.{name}: the gated dense NVFP4 op has no adapter form")
        r = _nvfp4_lora_operands(name, lora, T, lambda r: (N, r) if dense else (E, N, r))
        tag = "_lora"
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    if not rows.is_cuda:
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA tensor")
    dev = rows.device
    _on(dev, blocks=blocks, scales_e4m3=scales, global_scale=global_scale, bias=bias)
    if lora is not None:
        _on(dev, lora_rows=lora[0], lora_weight=lora[1])
        extra = (lora[0].contiguous(), lora[1].contiguous(), r)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    L = _native.lib()
    gs = None if global_scale is None else global_scale.contiguous()
    b = None if bias is None else bias.contiguous()
    if dense:
        _launch(f"fql_linear_nvfp4_glu{tag}_fwd" if gated else f"fql_linear_nvfp4{tag}_fwd", dev, blocks.contiguous(),
                scales.contiguous(), gs, rows.contiguous(), _DTYPES[rows.dtype], *extra, b, out, _DTYPES[out_dtype], T, K, N, *act,
                ws_bytes=L.fql_linear_nvfp4_workspace_bytes(T, K, N, int(gated)))
        return out
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)   # (none: one expert, all rows)
    _launch(f"fql_moe_nvfp4_glu{tag}_fwd" if gated else f"fql_moe_nvfp4{tag}_fwd", dev, blocks.contiguous(), scales.contiguous(), gs,
            rows.contiguous(), _DTYPES[rows.dtype], *extra, b, tpe, offs, out, _DTYPES[out_dtype], E, T, K, N, *act,
            ws_bytes=L.fql_moe_nvfp4_workspace_bytes(E, T, K, N, int(gated)))
    return out


def moe_forward_nvfp4(blocks, scales_e4m3, global_scale, inputs, tokens_per_expert, input_offsets, bias=None, out_dtype=None):
    """The grouped GEMM on NVFP4 expert weights (ModelOpt's ``-FP4`` / ``-NVFP4`` exports):
    ``out[t] = (W_e @ bf16(inputs[t])) * global_scale[e] (+ bias[e])`` over the rows of expert e.  ``blocks`` uint8
    [E, N, K/2] (two e2m1 codes a byte, even k in the low nibble), ``scales_e4m3`` uint8 [E, N, K/16] (the e4m3fn value
    of the byte scales 16 consecutive inputs), ``global_scale`` float32 [E] or None for 1 (``quantize.quantize_nvfp4``, or
    a checkpoint's ``weight`` / ``weight_scale`` / ``weight_scale_2``).  ``global_scale`` MULTIPLIES, as ModelOpt's
    ``weight_scale_2`` does; compressed-tensors stores the reciprocal (``weight_global_scale``): invert it first.
    ``inputs`` [T, K] float32 (rounded once to bfloat16) or bfloat16, K % 32 == 0; ``bias`` [E, N] float32.  The weights
    without the global scale are exact in bfloat16; the sums are float32 on the bfloat16 matrix cores; the multiply by
    ``global_scale`` and the addition of the bias are two float32 steps, then one rounding to ``out_dtype`` (default:
    the inputs' type).  Rows no expert covers are zero; both table arguments may be None with one expert.  A small
    batch takes a decode kernel that returns the same bits as the tile kernel.  Forward only (INTEGRATION.md
    section 18)."""
    _forward_only("moe_forward_nvfp4", inputs, bias)
    return _nvfp4_launch("moe_forward_nvfp4", blocks, scales_e4m3, global_scale, inputs, lambda K: K, tokens_per_expert,
                         input_offsets, bias, out_dtype, False)


def moe_gated_forward_nvfp4(blocks, scales_e4m3, global_scale, gate_up, tokens_per_expert, input_offsets, activation="silu",
                            activation_alpha=1.702, activation_limit=7.0, bias=None, out_dtype=None):
    """The down projection of a gated FFN expert on NVFP4 weights: ``moe_forward_nvfp4`` on
    ``bf16(act(gate_up[t, :K], gate_up[t, K:]))``, ``gate_up`` [T, 2K] float32 or bfloat16, by ``moe_gated_forward_mxfp4``'s
    streaming pre-pass into the op's workspace.  Forward only."""
    _forward_only("moe_gated_forward_nvfp4", gate_up, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    return _nvfp4_launch("moe_gated_forward_nvfp4", blocks, scales_e4m3, global_scale, gate_up, lambda K: 2 * K,
                         tokens_per_expert, input_offsets, bias, out_dtype, True, (_ACTIVATIONS[kind], act_alpha, act_limit))


def linear_forward_nvfp4(blocks, scales_e4m3, global_scale, x, bias=None, out_dtype=None):
    """A dense linear layer on NVFP4 weights: ``out[t] = (W @ bf16(x[t])) * global_scale (+ bias)``.  ``blocks`` uint8
    [N, K/2], ``scales_e4m3`` uint8 [N, K/16], ``global_scale`` float32 with one element or None, ``bias`` [N] float32.
    Exactly ``moe_forward_nvfp4`` on the one-expert view without a table: the same kernels, the same bits.  There is no
    split-K form."""
    _forward_only("linear_forward_nvfp4", x, bias)
    return _nvfp4_launch("linear_forward_nvfp4", blocks, scales_e4m3, global_scale, x, lambda K: K, None, None, bias, out_dtype,
                         False, dense=True)


def linear_gated_forward_nvfp4(blocks, scales_e4m3, global_scale, gate_up, activation="silu", activation_alpha=1.702,
                               activation_limit=7.0, bias=None, out_dtype=None):
    """The down projection of a dense gated MLP on NVFP4 weights: ``linear_forward_nvfp4`` on
    ``bf16(act(gate_up[t, :K], gate_up[t, K:]))``, ``gate_up`` [T, 2K], by the streaming pre-pass of
    ``moe_gated_forward_nvfp4``."""
    _forward_only("linear_gated_forward_nvfp4", gate_up, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    return _nvfp4_launch("linear_gated_forward_nvfp4", blocks, scales_e4m3, global_scale, gate_up, lambda K: 2 * K, None, None,
                         bias, out_dtype, True, (_ACTIVATIONS[kind], act_alpha, act_limit), dense=True)


ROUTE_MAX_EXPERTS = 128


def route_plan(expert_indices, num_experts):
    """Stable sort of the (token, slot) pairs by expert in ONE launch (replaces argsort + bincount + cumsum +
    index ops of routing.py:117-149).  ``expert_indices`` [T, top_k] integer, on the GPU.  Returns int32 device
    tensors ``(tokens_per_expert [E], input_offsets [E], token_of_sorted [T*top_k], pos_of_slot [T*top_k])``."""
    if not expert_indices.is_cuda or expert_indices.dim() != 2:
        raise RuntimeError("expert_indices must be a CUDA [tokens, top_k] tensor")
    if num_experts > ROUTE_MAX_EXPERTS:
        raise RuntimeError(f"route_plan supports up to {ROUTE_MAX_EXPERTS} experts")
    dev = expert_indices.device
    T, top_k = expert_indices.shape
    flat = expert_indices.reshape(-1).to(torch.int32).contiguous()
    n = flat.numel()
    counts = torch.empty(num_experts, dtype=torch.int32, device=dev)
    offsets = torch.empty(num_experts, dtype=torch.int32, device=dev)
    token_of_sorted = torch.empty(n, dtype=torch.int32, device=dev)
    pos_of_slot = torch.empty(n, dtype=torch.int32, device=dev)
    _launch("fql_route_plan_i32", dev, flat, n, top_k, num_experts, counts, offsets, token_of_sorted, pos_of_slot)
    return counts, offsets, token_of_sorted, pos_of_slot


def route_plan_capped(expert_indices, num_experts, capacity=None, token_mask=None):
    """``route_plan`` with slots that go nowhere, in ONE launch: a token whose ``token_mask`` entry is False is not
    routed at all, and an expert keeps at most ``capacity`` slots (None: no limit), the earliest in token order (the
    "position" drop policy of GShard and Megatron-Core).  ``expert_indices`` [T, top_k] integer, ``token_mask`` [T] bool or
    uint8, both on the GPU.  Returns int32 device tensors ``(tokens_per_expert [E], input_offsets [E], token_of_sorted
    [T*top_k], pos_of_slot [T*top_k], demand [E])``: ``tokens_per_expert`` counts the KEPT slots, ``demand`` the slots the
    router chose among the unmasked tokens before any drop; the kept rows are compact and in expert order,
    ``token_of_sorted`` is 0 behind them and ``pos_of_slot`` is -1 for a slot that was dropped or masked (read it with the
    ``skip_dropped=True`` forms of ``dispatch_rows`` and ``combine_any``).  Nothing is read back to the host."""
    if not expert_indices.is_cuda or expert_indices.dim() != 2:
        raise RuntimeError("expert_indices must be a CUDA [tokens, top_k] tensor")
    if num_experts > ROUTE_MAX_EXPERTS:
        raise RuntimeError(f"route_plan_capped supports up to {ROUTE_MAX_EXPERTS} experts")
    dev = expert_indices.device
    T, top_k = expert_indices.shape
    if capacity is not None:
        try:
            whole = int(capacity) == capacity and 1 <= capacity <= 0x7fffffff
        except (TypeError, ValueError, OverflowError):         # a string, NaN, an infinity
            whole = False
        if not whole:
            raise RuntimeError(f"capacity must be an integer >= 1 (or None for no limit), got {capacity!r}")
    mask = None
    if token_mask is not None:
        if not isinstance(token_mask, torch.Tensor) or not token_mask.is_cuda or token_mask.device != dev:
            raise RuntimeError("token_mask must be a CUDA tensor on expert_indices' device")
        if token_mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("token_mask must be a bool or uint8 tensor")
        if token_mask.dim() != 1 or token_mask.numel() != T:
            raise RuntimeError("token_mask must be [tokens]")
        mask = token_mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    flat = expert_indices.reshape(-1).to(torch.int32).contiguous()
    n = flat.numel()
    demand = torch.empty(num_experts, dtype=torch.int32, device=dev)
    counts = torch.empty(num_experts, dtype=torch.int32, device=dev)
    offsets = torch.empty(num_experts, dtype=torch.int32, device=dev)
    token_of_sorted = torch.empty(n, dtype=torch.int32, device=dev)
    pos_of_slot = torch.empty(n, dtype=torch.int32, device=dev)
    _launch("fql_route_plan_capped_i32", dev, flat, n, top_k, num_experts, mask, 0 if capacity is None else int(capacity),
            demand, counts, offsets, token_of_sorted, pos_of_slot)
    return counts, offsets, token_of_sorted, pos_of_slot, demand


def combine(y, pos_of_slot, expert_weights, top_k=None):
    """out[t] = sum_k expert_weights[t, k] * y[pos_of_slot[t*top_k + k]] in one launch (routing.py:172-189), on float32
    rows: ``combine_any`` without an addend.  ``expert_weights=None`` (with ``top_k``): the rows already carry their
    weights -- a pure gather-add.  Under autograd the gradients to ``y`` and ``expert_weights`` come from one backward
    launch."""
    if not y.is_cuda or y.dtype != torch.float32 or y.dim() != 2:
        raise RuntimeError("y must be a CUDA float32 [rows, N] tensor")
    return combine_any(y, pos_of_slot, expert_weights, top_k)


def _combine_operands(y, pos_of_slot, expert_weights, top_k, addend, addend_weight):
    """``(T, top_k, pos int32, weights float32 or None, addend contiguous, addend_weight float32 [T] contiguous)`` of the
    combine and its backward, on ``y``'s device."""
    if not y.is_cuda or y.dtype not in _DTYPES or y.dim() != 2:
        raise RuntimeError("y must be a CUDA float32, float16 or bfloat16 [rows, N] tensor")
    if expert_weights is None:
        if not top_k:
            raise RuntimeError("top_k is needed when the rows carry their weights")
        T = pos_of_slot.numel() // top_k
    else:
        T, top_k = expert_weights.shape
    _on(y.device, y=y, pos_of_slot=pos_of_slot, expert_weights=expert_weights)
    if pos_of_slot.numel() < T * top_k:
        raise RuntimeError("pos_of_slot must have tokens * top_k elements")
    w = None if expert_weights is None else expert_weights.to(dtype=torch.float32).contiguous()
    pos = pos_of_slot.to(dtype=torch.int32).contiguous()
    _on(y.device, addend=addend, addend_weight=addend_weight)
    if addend is None:
        if addend_weight is not None:
            raise RuntimeError("addend_weight needs an addend")
        return T, top_k, pos, w, None, None
    if addend.dtype != y.dtype or tuple(addend.shape) != (T, y.shape[1]):
        raise RuntimeError("addend must be [tokens, N] of y's type")
    if addend_weight is not None and (addend_weight.dtype != torch.float32 or tuple(addend_weight.shape) != (T,)):
        raise RuntimeError("addend_weight must be float32 [tokens]")
    return T, top_k, pos, w, addend.contiguous(), None if addend_weight is None else addend_weight.contiguous()


def _combine_out_dtype(out_dtype, default):
    out_dtype = default if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    return out_dtype


def combine_any(y, pos_of_slot, expert_weights, top_k=None, addend=None, addend_weight=None, out_dtype=None,
                skip_dropped=False):
    """``combine`` with element types and an addend, in one launch: ``out[t] = sum_k expert_weights[t, k] *
    y[pos_of_slot[t*top_k + k]] + addend_weight[t] * addend[t]``.  ``y`` [R, N] float32 / float16 / bfloat16 is read as it
    is, the sum is float32 (the slot terms exactly ``combine``'s, the addend term last) and ``out`` [T, N] is rounded once
    to ``out_dtype`` (default ``y.dtype``): without an addend, bit for bit ``combine(y.float(), ...).to(out_dtype)``.
    ``addend`` [T, N] of ``y``'s type (a shared expert's output) and ``addend_weight`` [T] float32 are optional
    (``addend_weight=None``: 1).  Under autograd the gradients to ``y``, ``expert_weights``, ``addend`` and
    ``addend_weight`` come from one backward launch (``combine_any_backward``); ``y`` and ``addend`` are saved in their
    own type.  ``skip_dropped=True`` (the plan of ``route_plan_capped``): a slot with ``pos_of_slot < 0`` adds nothing
    (its row and its weight are not read) where the default clamps it to row 0; under autograd it gets a zero weight
    gradient and sends ``y`` nothing."""
    if _wants_grad(y, expert_weights, addend, addend_weight):
        if skip_dropped:
            return _CombineFn.apply(y, pos_of_slot, expert_weights, top_k, addend, addend_weight, out_dtype, True)
        return _CombineFn.apply(y, pos_of_slot, expert_weights, top_k, addend, addend_weight, out_dtype)
    T, top_k, pos, w, addend, aw = _combine_operands(y, pos_of_slot, expert_weights, top_k, addend, addend_weight)
    out_dtype = _combine_out_dtype(out_dtype, y.dtype)
    if T > 65535:
        raise RuntimeError("combine handles up to 65535 tokens per call")
    out = torch.empty((T, y.shape[1]), dtype=out_dtype, device=y.device)
    _launch("fql_combine_sparse" if skip_dropped else "fql_combine", y.device, y.contiguous(), _DTYPES[y.dtype], pos, w,
            addend, aw, out, _DTYPES[out_dtype], T, top_k, y.shape[1], y.shape[0])
    return out


ROUTER_MAX_TOPK = 8


def _router_operands(logits, top_k):
    """``(logits contiguous, T, E)`` of ``router_topk`` and its backward; the limits of csrc/fql_router.h raise here."""
    _on(logits.device, logits=logits)
    if logits.dim() != 2 or logits.dtype not in _DTYPES:
        raise RuntimeError("logits must be a float32, float16 or bfloat16 [tokens, num_experts] tensor")
    T, E = logits.shape
    if E < 1 or E > ROUTE_MAX_EXPERTS:
        raise RuntimeError(f"router_topk supports 1 to {ROUTE_MAX_EXPERTS} experts, got {E}")
    if not isinstance(top_k, int) or top_k < 1 or top_k > min(E, ROUTER_MAX_TOPK):
        raise RuntimeError(f"top_k must be an integer in [1, min(num_experts, {ROUTER_MAX_TOPK})], got {top_k!r}")
    return logits.contiguous(), T, E


def router_topk(logits, top_k, renormalize=True, return_probs=False):
    """The MoE router in ONE launch (replaces softmax -> topk -> sum -> div -> to(int32)): ``logits`` [T, E] float32 /
    float16 / bfloat16 on the GPU -> ``(weights [T, top_k] float32, indices [T, top_k] int32)``, plus ``probs`` [T, E]
    float32 (the full softmax, for a load-balancing loss) with ``return_probs``.  Selection is on the logits, ties to the
    lower expert id; ``renormalize`` divides the selected probabilities by their sum (Mixtral).  ``indices`` is what
    ``route_plan`` reads, ``weights`` what ``combine`` reads.  A row with a non-finite logit gets NaN weights and indices
    0 .. top_k-1.  Under autograd the gradients of ``weights`` and ``probs`` reach ``logits`` in one backward launch.
    This is ``router_score_topk`` at its defaults, which the library runs with the other routing rules compiled out."""
    return router_score_topk(logits, top_k, renormalize=renormalize, return_scores=return_probs)


def router_topk_backward(logits, indices, grad_weights, grad_probs, renormalize=True):
    """Gradient of ``router_topk`` to ``logits`` (in their type, rounded once) from the gradients of ``weights`` and / or
    ``probs`` (float32; either may be None), one launch, no atomics."""
    return router_score_topk_backward(logits, indices, grad_weights, grad_probs, renormalize=renormalize)


ROUTER_MAX_GROUPS = 8
_SCORINGS = {"softmax": 0, "sigmoid": 1}


def _router_score_settings(E, top_k, scoring, n_group=1, topk_group=1, group_top=1, scale=1.0):
    """``(scoring code, scale as a float)`` of ``router_score_topk`` and its backward; the limits of
    csrc/fql_router.h raise here."""
    try:
        code = _SCORINGS[scoring]
    except (KeyError, TypeError):
        raise ValueError(f"scoring must be 'softmax' or 'sigmoid', got {scoring!r}") from None
    if not all(isinstance(v, int) for v in (n_group, topk_group, group_top)):
        raise RuntimeError("n_group, topk_group and group_top must be integers")
    if n_group < 1 or n_group > ROUTER_MAX_GROUPS or E % n_group != 0:
        raise RuntimeError(f"n_group must be in [1, {ROUTER_MAX_GROUPS}] and divide num_experts ({E}), got {n_group}")
    if topk_group < 1 or topk_group > n_group or topk_group * (E // n_group) < top_k:
        raise RuntimeError(f"topk_group must be in [1, n_group] and its groups must hold top_k experts, got {topk_group}")
    if group_top not in (1, 2):
        raise RuntimeError(f"group_top must be 1 or 2, got {group_top}")
    scale = float(scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise RuntimeError("scale must be finite")
    return code, scale


def router_score_topk(logits, top_k, scoring="softmax", select_bias=None, n_group=1, topk_group=1, group_top=2,
                      renormalize=True, scale=1.0, return_scores=False):
    """``router_topk`` for the routing rules of DeepSeek-V2 / V3, GLM-4.5, Kimi-K2 and Llama-4, still ONE launch:
    ``scoring`` 'softmax' or 'sigmoid'; ``select_bias`` [E] float32 (``e_score_correction_bias``) is added to the scores
    for the selection only; the experts form ``n_group`` groups of which the ``topk_group`` best are searched, a group's
    score being the largest (``group_top=1``, DeepSeek-V2) or the sum of the two largest (``group_top=2``, DeepSeek-V3)
    biased scores; the weights are the unbiased scores of the chosen experts, divided by their sum (``renormalize``) and
    multiplied by ``scale`` (``routed_scaling_factor``).  Returns ``(weights [T, top_k] float32, indices [T, top_k]
    int32)``, plus ``scores`` [T, E] float32 with ``return_scores``.  Without a bias the selection is on the logits, ties
    to the lower expert id; experts outside the chosen groups are never selected.  With the defaults this is
    ``router_topk``.  Under autograd the gradients of ``weights`` and ``scores`` reach ``logits`` in one backward
    launch; the bias gets none."""
    if _wants_grad(logits):
        out = _RouterTopkFn.apply(logits, top_k, scoring, select_bias, n_group, topk_group, group_top,
                                  bool(renormalize), scale, bool(return_scores))
        return out if return_scores else out[:2]
    logits, T, E = _router_operands(logits, top_k)
    code, scale = _router_score_settings(E, top_k, scoring, n_group, topk_group, group_top, scale)
    dev = logits.device
    _on(dev, select_bias=select_bias)
    if select_bias is not None and (select_bias.dtype != torch.float32 or tuple(select_bias.shape) != (E,)):
        raise RuntimeError("select_bias must be a float32 [num_experts] tensor")
    bias = None if select_bias is None else select_bias.detach().contiguous()
    indices = torch.empty((T, top_k), dtype=torch.int32, device=dev)
    weights = torch.empty((T, top_k), dtype=torch.float32, device=dev)
    scores = torch.empty((T, E), dtype=torch.float32, device=dev) if return_scores else None
    _launch("fql_router_score_topk_fwd", dev, logits, _DTYPES[logits.dtype], T, E, top_k, code, bias, n_group, topk_group,
            group_top, int(bool(renormalize)), scale, indices, weights, scores)
    return (weights, indices, scores) if return_scores else (weights, indices)


def router_score_topk_backward(logits, indices, grad_weights, grad_scores, scoring="softmax", renormalize=True, scale=1.0):
    """Gradient of ``router_score_topk`` to ``logits`` (in their type, rounded once) from the gradients of ``weights``
    and / or ``scores`` (float32; either may be None), one launch, no atomics.  The groups and the bias do not enter:
    the ``indices`` say what was chosen."""
    top_k = indices.shape[1]
    logits, T, E = _router_operands(logits, top_k)
    code, scale = _router_score_settings(E, top_k, scoring, scale=scale)
    dev = logits.device
    _on(dev, indices=indices, grad_weights=grad_weights, grad_scores=grad_scores)
    if tuple(indices.shape) != (T, top_k) or (grad_weights is not None and tuple(grad_weights.shape) != (T, top_k)) \
            or (grad_scores is not None and tuple(grad_scores.shape) != (T, E)):
        raise RuntimeError("indices and grad_weights must be [tokens, top_k], grad_scores [tokens, num_experts]")
    gw = None if grad_weights is None else grad_weights.to(dtype=torch.float32).contiguous()
    gs = None if grad_scores is None else grad_scores.to(dtype=torch.float32).contiguous()
    grad_logits = torch.empty_like(logits)
    _launch("fql_router_score_topk_bwd", dev, logits, _DTYPES[logits.dtype], indices.to(dtype=torch.int32).contiguous(), gw,
            gs, grad_logits, T, E, top_k, code, int(bool(renormalize)), scale)
    return grad_logits


def dispatch_rows(x, token_of_sorted, pos_of_slot, top_k, skip_dropped=False):
    """The differentiable dispatch: ``x[token_of_sorted]`` ([T, H] -> [T * top_k, H], rows in expert order, from the plan
    of ``route_plan``).  Its backward is the pure gather-add form of ``combine`` over ``pos_of_slot`` (one launch, no
    atomics: ``x.grad`` is bit-reproducible, which ``index_add_`` is not), through ``combine_any``: a 16-bit gradient is
    read as it arrives, summed in float32 and rounded once to ``x``'s type.  ``skip_dropped=True`` (the plan of
    ``route_plan_capped``): the backward is the sparse gather-add, a slot with ``pos_of_slot < 0`` sends ``x`` nothing."""
    if _wants_grad(x):
        if skip_dropped:
            return _DispatchRowsFn.apply(x, token_of_sorted, pos_of_slot, top_k, True)
        return _DispatchRowsFn.apply(x, token_of_sorted, pos_of_slot, top_k)
    _on(x.device, x=x, token_of_sorted=token_of_sorted)
    return x.index_select(0, token_of_sorted)


def regroup_index(recv_counts, total_rows):
    """Expert-parallel receive side: ``recv_counts`` [G, EL] (rows per source rank and local expert, in arrival
    order), ``total_rows`` = their sum (the caller knows it on the host from the all-to-all split sizes) ->
    ``(tokens_per_expert [EL], input_offsets [EL], gather [R], scatter [R])`` int32 device tensors, one launch."""
    if not recv_counts.is_cuda or recv_counts.dim() != 2:
        raise RuntimeError("recv_counts must be a CUDA [ranks, local_experts] tensor")
    dev = recv_counts.device
    G, EL = recv_counts.shape
    tpe = torch.empty(EL, dtype=torch.int32, device=dev)
    offs = torch.empty(EL, dtype=torch.int32, device=dev)
    gather = torch.empty(max(total_rows, 1), dtype=torch.int32, device=dev)
    scatter = torch.empty(max(total_rows, 1), dtype=torch.int32, device=dev)
    _launch("fql_regroup_index_i32", dev, recv_counts.to(torch.int32).contiguous(), G, EL, tpe, offs, gather, scatter)
    return tpe, offs, gather[:total_rows], scatter[:total_rows]


def _quantize(weight_fp32, per_tensor):
    if not weight_fp32.is_cuda or weight_fp32.dtype != torch.float32 or weight_fp32.dim() != 2:
        raise RuntimeError("weight must be a CUDA float32 [N,K] tensor")
    w = weight_fp32.contiguous()
    N, K = w.shape
    packed = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    scales = torch.empty((N,), dtype=torch.float32, device=w.device)
    zps = torch.empty((N,), dtype=torch.float32, device=w.device)
    if per_tensor:                                          # + the scratch of the whole-tensor min / max reduction
        scratch = torch.empty((2 * N,), dtype=torch.float32, device=w.device)
        _launch("fql_quantize_tensor_f32", w.device, w, packed, scales, zps, scratch, N, K)
    else:
        _launch("fql_quantize_rows_f32", w.device, w, packed, scales, zps, N, K)
    return packed, scales, zps


def quantize_rows(weight_fp32):
    """GPU quantize_weights (python/quantize.py:38-124), bit-exact with the host arithmetic."""
    return _quantize(weight_fp32, per_tensor=False)


def quantize_tensor(weight_fp32):
    """GPU per-tensor quantiser of one expert (python/moe_int4_module.py:45-76): scale / zp broadcast to [N]."""
    return _quantize(weight_fp32, per_tensor=True)


def unpack_nibbles(packed):
    """q[..., 2j] = packed[..., j] & 15; q[..., 2j+1] = packed[..., j] >> 4 on the device."""
    if not packed.is_cuda or packed.dtype != torch.uint8:
        raise RuntimeError("packed must be a CUDA uint8 tensor")
    packed = packed.contiguous()
    q = torch.empty(packed.shape[:-1] + (packed.shape[-1] * 2,), dtype=torch.uint8, device=packed.device)
    _launch("fql_unpack_u8", packed.device, packed, q, packed.numel())
    return q


def dequantize_forward(packed_weights, scales, zero_points):
    """GPU dequantize_weights: [N,K/2] u8 -> [N,K] f32 (python/quantize.py:127-173)."""
    dev = packed_weights.device
    packed_weights, scales, zero_points, _, N, K = _check_weights(packed_weights, scales, zero_points, dev)
    w = torch.empty((N, K), dtype=torch.float32, device=dev)
    _launch("fql_dequantize_f32", dev, packed_weights, scales, zero_points, w, N, K)
    return w


def _sets(prec):
    """Limb sets of the two-phase buffers: 2 (main + residual of heavy-tailed rows) for 2 / 3 limbs, else 1."""
    return 2 if _planes(prec) >= 2 else 1


def act_quant(x, precision="default", tokens_per_expert=None, input_offsets=None, out=None):
    """Phase 1 of the MFMA path: float32 rows -> int8 limbs in MFMA-fragment order (+ delta, rowsum).
    Pass the device-side expert arrays for a grouped (MoE) layout, or neither for one group.
    Returns ``(limbs, delta [S, T], rowsum [S, limbs, T])`` with S = 2 sets for 2 / 3 limbs (set 1 = the residual of
    heavy-tailed rows, ``delta[1] == 0`` where a row has none) and S = 1 for int8 / fp8 (include/fql_int4.h)."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("x must be a CUDA float32 [T,K] tensor")
    x = x.contiguous()
    T, K = x.shape
    prec = _precision(precision)
    nl, ns = _planes(prec), _sets(prec)
    tpe, offs, E = None, None, 1
    if tokens_per_expert is not None:
        E = tokens_per_expert.numel()
        tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, x.device)
    if out is not None:                 # reuse the buffers of an earlier call with the same shapes (timing loops)
        limbs, delta, rowsum = out
    else:
        limbs = torch.zeros(_native.lib().fql_act_limb_bytes(T, E, K, prec), dtype=torch.int8, device=x.device)
        delta = torch.zeros((ns, T), dtype=torch.float32, device=x.device)
        rowsum = torch.zeros((ns, nl, T), dtype=torch.int32, device=x.device)
    _launch("fql_act_quant_f32", x.device, x, limbs, delta, rowsum, tpe, offs, E, T, K, prec)
    return limbs, delta, rowsum


_SCRATCH = {}


def gemm_scratch(prec, device):
    """The residual-pass scratch of phase 2: one cached buffer per (device, STREAM) -- its slots are indexed by workgroup and
    wave only, so two launches that overlap on different streams must not share one; contents never outlive a launch."""
    n = _native.lib().fql_gemm_scratch_bytes(prec)
    if n == 0:
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, n)
    if key not in _SCRATCH:
        _SCRATCH[key] = torch.empty(n, dtype=torch.uint8, device=device)
    return _SCRATCH[key]


def gemm_i8(limbs, delta, rowsum, packed_weights, scales, zero_points, tokens_per_expert=None,
            input_offsets=None, precision="default", out=None):
    """Phase 2 of the MFMA path: grouped INT4 x INT8-limb GEMM over pre-converted activations
    (``act_quant`` output, produced with the same expert arrays).  ``packed_weights`` [N,K/2] (one
    group) or [E,N,K/2] with device-side ``tokens_per_expert`` / ``input_offsets``."""
    dev = limbs.device
    _on(dev, limbs=limbs, delta=delta, rowsum=rowsum, out=out)
    T = delta.shape[-1]
    grouped = packed_weights.dim() == 3
    packed_weights, scales, zero_points, E, N, K = _check_weights(packed_weights, scales, zero_points, dev, grouped=grouped)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev) if grouped else (None, None)
    prec = _precision(precision)
    if _planes(prec) != rowsum.shape[-2] or _sets(prec) != delta.shape[0]:
        raise RuntimeError("limb count does not match precision")
    if limbs.numel() < _native.lib().fql_act_limb_bytes(T, E, K, prec):
        raise RuntimeError("limbs were not produced for this T, E, K")
    if out is None:
        out = torch.zeros((T, N), dtype=torch.float32, device=dev) if grouped else \
            torch.empty((T, N), dtype=torch.float32, device=dev)
    scratch = gemm_scratch(prec, dev)
    _launch("fql_gemm_i8_f32", dev, limbs, delta, rowsum, packed_weights, scales, zero_points, tpe, offs, out,
            E, T, K, N, prec, after=(None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel()))   # (cached)
    return out


def tune_gemm_i8(cfg, limbs, delta, rowsum, packed_weights, scales, zero_points, tokens_per_expert, input_offsets, out,
                 E, T, K, N, precision, out_dtype=None, bias=None, row_weight=None):
    """Phase 2 with an explicit tile configuration id (tuning / test hook, not part of the public header).
    With ``out_dtype`` (the element type of ``out``), ``bias`` [E, N] or ``row_weight`` [T] the call goes to the hook that
    reaches the whole epilogue: out = out_dtype(fl32(fl32(acc + bias) * row_weight)).  The kernels read a row's weight
    from the plane behind delta's sets (the pre-pass of the product path puts it there), so it is appended to a copy of
    ``delta`` here."""
    import ctypes
    prec = _precision(precision)
    dev = limbs.device
    scratch = gemm_scratch(prec, dev)
    head = [cfg, limbs.data_ptr(), None, rowsum.data_ptr(), packed_weights.data_ptr(), scales.data_ptr(),
            zero_points.data_ptr(), None if tokens_per_expert is None else tokens_per_expert.data_ptr(),
            None if input_offsets is None else input_offsets.data_ptr(), out.data_ptr()]
    tail = [E, T, K, N, prec, _stream_ptr(dev), None if scratch is None else scratch.data_ptr(),
            0 if scratch is None else scratch.numel()]
    tail_types = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    if out_dtype is None and bias is None and row_weight is None:
        fn = _native.lib().fql_tune_gemm_i8_f32
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 9 + tail_types
        head[2] = delta.data_ptr()
        with torch.cuda.device(dev):
            return fn(*head, *tail)
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out.dtype != out_dtype or out_dtype not in _DTYPES:
        raise RuntimeError("out must be a float32, float16 or bfloat16 tensor of element type out_dtype")
    for name, t, n in (("bias", bias, E * N), ("row_weight", row_weight, T)):
        if t is not None and (t.device != dev or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous float32 tensor of {n} elements on the limbs' device")
    rw_ptr = None
    if row_weight is not None:
        if delta.dim() != 2 or delta.shape != (_sets(prec), T):
            raise RuntimeError("delta must be [sets, T] as act_quant returns it")
        delta = torch.cat([delta, row_weight.reshape(1, T)])
        rw_ptr = delta[_sets(prec)].data_ptr()
    fn = _native.lib().fql_tune_gemm_i8
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + tail_types
    head[2] = delta.data_ptr()
    with torch.cuda.device(dev):
        return fn(*head, _DTYPES[out_dtype], None if bias is None else bias.data_ptr(), rw_ptr, *tail)


# ------------------------------------------------------------------------------------------------ fp8 activations
def _as_e4m3_bytes(t, name):
    if t.dtype == torch.uint8:
        return t
    if t.dtype == getattr(torch, "float8_e4m3fn", None):
        return t.view(torch.uint8)
    raise RuntimeError(f"{name} must be torch.float8_e4m3fn (or its uint8 bytes)")


def quantize_activations_fp8(x):
    """Per-row OCP e4m3 quantisation with torch ops (for callers that want to hold fp8 activations themselves):
    ``scale[t] = max|x[t]| / 448`` (1 for an all-zero row), ``x8 = (x / scale).to(torch.float8_e4m3fn)``.
    ``precision="fp8"`` on the float entry points does the same inside the fused pre-pass."""
    x = x.float()
    amax = x.abs().amax(dim=1)
    # tensor / tensor: a true float32 division (torch turns `/ 448.0` into a multiplication by the reciprocal, one ulp off)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    return (x / scale[:, None]).to(torch.float8_e4m3fn), scale


def _fp8_operands(x, act_scales, name, out_dtype, K_name):
    """``(x8 uint8 [rows, K] contiguous, act_scales float32 [rows] or None)`` of the two fp8 entry points."""
    x8 = _as_e4m3_bytes(x, name)
    if not x8.is_cuda or x8.dim() != 2:
        raise RuntimeError(f"{name} must be a CUDA [rows, {K_name}] tensor")
    if out_dtype not in _DTYPES:
        raise RuntimeError("outputs must be float32, float16 or bfloat16")
    if x8.shape[1] % 32 != 0:
        raise RuntimeError(f"the fp8 path needs {K_name} % 32 == 0")
    if act_scales is not None:
        if act_scales.numel() != x8.shape[0]:
            raise RuntimeError("act_scales must have one element per row")
        act_scales = act_scales.to(device=x8.device, dtype=torch.float32).contiguous()
    return x8.contiguous(), act_scales


def moe_forward_fp8(packed_weights, scales, zero_points, inputs_e4m3, act_scales, tokens_per_expert, input_offsets,
                    out_dtype=torch.float32):
    """Grouped per-expert INT4 GEMM over rows that are already fp8: ``inputs_e4m3`` [T, K] torch.float8_e4m3fn
    (or its uint8 bytes), ``act_scales`` [T] float32 or None.  One fp8 MFMA pass, float32 accumulation
    (BASELINE.json configs[4]).  Returns [T, N] in ``out_dtype``; rows no expert covers are zero."""
    _forward_only("moe_forward_fp8", inputs_e4m3, act_scales)
    x8, act_scales = _fp8_operands(inputs_e4m3, act_scales, "inputs_e4m3", out_dtype, "hidden_dim")
    T, K = x8.shape
    dev = x8.device
    packed_weights, scales, zero_points, E, N, _ = _check_weights(packed_weights, scales, zero_points, dev, K, grouped=True)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    _launch("fql_moe_fwd_f8", dev, packed_weights, scales, zero_points, x8, act_scales, tpe, offs, out, _DTYPES[out_dtype],
            E, T, K, N, ws_bytes=_native.lib().fql_moe_workspace_bytes(E, T, K, N, _native.PRECISION_FP8))
    return out


def moe_forward_mxfp4_fp8(blocks, scales, inputs_e4m3, act_scales, tokens_per_expert, input_offsets, bias=None,
                          out_dtype=torch.float32):
    """The grouped GEMM on OCP MXFP4 expert weights over rows that are already fp8, on the block-scaled FP4 matrix cores:
    ``out[t] = act_scales[t] * (W_e @ e4m3(inputs_e4m3[t])) (+ bias[e])``.  ``blocks`` / ``scales`` as ``moe_forward_mxfp4``
    takes them; ``inputs_e4m3`` [T, K] torch.float8_e4m3fn (or its uint8 bytes), ``act_scales`` [T] float32 or None (= 1);
    ``bias`` [E, N] float32 (optional).  Returns [T, N] in ``out_dtype``; rows no expert covers are zero.  Forward only
    (INTEGRATION.md section 17).  Small batches (T up to the library's fp8 decode threshold) take a one-wave decode
    kernel that returns the same bits as the tile kernel: the result does not depend on T."""
    _forward_only("moe_forward_mxfp4_fp8", inputs_e4m3, act_scales, bias)
    x8, act_scales = _fp8_operands(inputs_e4m3, act_scales, "inputs_e4m3", out_dtype, "hidden_dim")
    T, K = x8.shape
    dev = x8.device
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    _launch("fql_moe_mx4_fwd_f8", dev, blocks, scales, x8, act_scales, bias, tpe, offs, out, _DTYPES[out_dtype], E, T, K, N,
            ws_bytes=_native.lib().fql_moe_mx4_f8_workspace_bytes(E, T, K, N, 0))
    return out


def quantize_rows_mxfp4(rows, activation=None, activation_alpha=1.702, activation_limit=7.0):
    """Rows to MXFP4 on the GPU, the quantiser of ``precision="fp4"`` on its own: ``rows`` [T, K] float32 or bfloat16 (CUDA,
    K % 32 == 0) -> ``(blocks uint8 [T, K/2], scales uint8 [T, K/32])``, bit for bit ``quantize.quantize_mxfp4`` for every
    finite input.  A block that holds an inf or a NaN gets zero codes and scale code 255 (a NaN output row of the GEMM).
    With ``activation`` given, ``rows`` is ``gate_up`` [T, 2K] and what is quantised is ``h = act(gate_up[:, :K],
    gate_up[:, K:])`` (``activation_of``), evaluated once in float32.  Forward only."""
    _forward_only("quantize_rows_mxfp4", rows)
    gated = activation is not None
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit) if gated else ("silu", 0.0, 0.0)
    if not rows.is_cuda or rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("ops.quantize_rows_mxfp4: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is refused: "
                           "cast it yourself)")
    T, width = rows.shape
    if width % (64 if gated else 32) != 0 or width == 0:
        raise RuntimeError("gate_up must be [T, 2K] with K % 32 == 0" if gated else "rows must be [T, K] with K % 32 == 0")
    K = width // 2 if gated else width
    dev = rows.device
    blocks = torch.empty((T, K // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((T, K // 32), dtype=torch.uint8, device=dev)
    _launch("fql_mx4_quantize_rows", dev, rows.contiguous(), _DTYPES[rows.dtype], int(gated), _ACTIVATIONS[kind], act_alpha,
            act_limit, blocks, scales, T, K)
    return blocks, scales


def moe_forward_mxfp4_fp4(blocks, scales, in_blocks, in_scales, tokens_per_expert, input_offsets, bias=None,
                          out_dtype=torch.float32):
    """The grouped GEMM on OCP MXFP4 expert weights over rows that are already MXFP4 (W4A4), both operands e2m1 with their
    E8M0 block scales on the block-scaled FP4 matrix cores: ``out[t] = W_e @ X[t] (+ bias[e])``.  ``blocks`` / ``scales`` as
    ``moe_forward_mxfp4`` takes them; ``in_blocks`` uint8 [T, K/2] and ``in_scales`` uint8 [T, K/32] in the same layout
    (``quantize_rows_mxfp4`` or ``quantize.quantize_mxfp4``); ``bias`` [E, N] float32 (optional).  Returns [T, N] in
    ``out_dtype``; rows no expert covers are zero; an ``in_scales`` byte of 255 makes its row NaN.  Forward only
    (INTEGRATION.md section 17).  Small batches (T up to the library's fp4 decode threshold) take a one-wave decode
    kernel that returns the same bits as the tile kernel: the result does not depend on T."""
    _forward_only("moe_forward_mxfp4_fp4", bias)
    for name, t in (("in_blocks", in_blocks), ("in_scales", in_scales)):
        if not t.is_cuda or t.dim() != 2 or t.dtype != torch.uint8:
            raise RuntimeError(f"ops.moe_forward_mxfp4_fp4: {name} must be a CUDA uint8 2-D tensor")
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    T, K = in_blocks.shape[0], in_blocks.shape[1] * 2
    dev = in_blocks.device
    if K % 32 != 0 or in_scales.device != dev or tuple(in_scales.shape) != (T, K // 32):
        raise RuntimeError("in_blocks must be [T, K/2] and in_scales [T, K/32] with K % 32 == 0, on one device")
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    _launch("fql_moe_mx4_fwd_f4", dev, blocks, scales, in_blocks.contiguous(), in_scales.contiguous(), bias, tpe, offs, out,
            _DTYPES[out_dtype], E, T, K, N, ws_bytes=_native.lib().fql_moe_mx4_f4_workspace_bytes(E, T, K, N, 0))
    return out


def quantize_rows_mxfp6(rows, activation=None, activation_alpha=1.702, activation_limit=7.0):
    """Rows to MXFP6 (e2m3) on the GPU, the quantiser of ``precision="fp6"`` on its own: ``rows`` [T, K] float32 or bfloat16
    (CUDA, K % 32 == 0) -> ``(codes uint8 [T, 3K/4], scales uint8 [T, K/32])``, bit for bit ``quantize.quantize_mxfp6`` for
    every finite input.  A block that holds an inf or a NaN gets zero codes and scale code 255 (a NaN output row of the
    GEMM).  With ``activation`` given, ``rows`` is ``gate_up`` [T, 2K] and what is quantised is ``h = act(gate_up[:, :K],
    gate_up[:, K:])`` (``activation_of``), evaluated once in float32.  Forward only."""
    _forward_only("quantize_rows_mxfp6", rows)
    gated = activation is not None
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit) if gated else ("silu", 0.0, 0.0)
    if not rows.is_cuda or rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("ops.quantize_rows_mxfp6: the rows must be a CUDA float32 or bfloat16 2-D tensor (float16 is refused: "
                           "cast it yourself)")
    T, width = rows.shape
    if width % (64 if gated else 32) != 0 or width == 0:
        raise RuntimeError("gate_up must be [T, 2K] with K % 32 == 0" if gated else "rows must be [T, K] with K % 32 == 0")
    K = width // 2 if gated else width
    dev = rows.device
    codes = torch.empty((T, K // 4 * 3), dtype=torch.uint8, device=dev)
    scales = torch.empty((T, K // 32), dtype=torch.uint8, device=dev)
    _launch("fql_mx6_quantize_rows", dev, rows.contiguous(), _DTYPES[rows.dtype], int(gated), _ACTIVATIONS[kind], act_alpha,
            act_limit, codes, scales, T, K)
    return codes, scales


def moe_forward_mxfp4_fp6(blocks, scales, in_codes, in_scales, tokens_per_expert, input_offsets, bias=None,
                          out_dtype=torch.float32):
    """The grouped GEMM on OCP MXFP4 expert weights over rows that are already MXFP6 (e2m3 elements with E8M0 block scales)
    on the block-scaled matrix cores, at the FP4 rate: ``out[t] = W_e @ X[t] (+ bias[e])``.  ``blocks`` / ``scales`` as
    ``moe_forward_mxfp4`` takes them; ``in_codes`` uint8 [T, 3K/4] (``quantize.pack_mxfp6``'s layout) and ``in_scales`` uint8
    [T, K/32] (``quantize_rows_mxfp6`` or ``quantize.quantize_mxfp6``); ``bias`` [E, N] float32 (optional).  Returns [T, N]
    in ``out_dtype``; rows no expert covers are zero; an ``in_scales`` byte of 255 makes its row NaN.  ``in_codes`` must be
    8-byte aligned (a contiguous tensor that is not is copied).  Forward only.  Small batches
    (T up to the library's fp6 decode threshold) take a one-wave decode kernel that returns the same bits as the tile
    kernel: the result does not depend on T."""
    _forward_only("moe_forward_mxfp4_fp6", bias)
    for name, t in (("in_codes", in_codes), ("in_scales", in_scales)):
        if not t.is_cuda or t.dim() != 2 or t.dtype != torch.uint8:
            raise RuntimeError(f"ops.moe_forward_mxfp4_fp6: {name} must be a CUDA uint8 2-D tensor")
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    T = in_codes.shape[0]
    dev = in_codes.device
    if in_codes.shape[1] % 24 != 0 or in_scales.device != dev or tuple(in_scales.shape) != (T, in_codes.shape[1] // 24):
        raise RuntimeError("in_codes must be [T, 3K/4] and in_scales [T, K/32] with K % 32 == 0, on one device")
    K = in_codes.shape[1] // 3 * 4
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    bias = _check_bias(bias, N, dev, E)
    out = torch.empty((T, N), dtype=out_dtype, device=dev)
    in_codes = in_codes.contiguous()
    if in_codes.data_ptr() % 8 != 0:
        in_codes = in_codes.clone()
    _launch("fql_moe_mx4_fwd_f6", dev, blocks, scales, in_codes, in_scales.contiguous(), bias, tpe, offs, out,
            _DTYPES[out_dtype], E, T, K, N, ws_bytes=_native.lib().fql_moe_mx4_f6_workspace_bytes(E, T, K, N, 0))
    return out


def linear_forward_fp8(x_e4m3, act_scales, packed_weights, scales, zero_points, out_dtype=torch.float32):
    """Fused 4-bit dequantize + linear over fp8 rows: ``x_e4m3`` [B, K] torch.float8_e4m3fn (or uint8 bytes),
    ``act_scales`` [B] float32 or None -> [B, N] in ``out_dtype``."""
    _forward_only("linear_forward_fp8", x_e4m3, act_scales)
    x8, act_scales = _fp8_operands(x_e4m3, act_scales, "x_e4m3", out_dtype, "input_dim")
    B, K = x8.shape
    dev = x8.device
    packed_weights, scales, zero_points, _, N, _ = _check_weights(packed_weights, scales, zero_points, dev, K)
    out = torch.empty((B, N), dtype=out_dtype, device=dev)
    if B == 0:
        return out
    _launch("fql_linear_fwd_f8", dev, x8, act_scales, packed_weights, scales, zero_points, out, _DTYPES[out_dtype],
            B, K, N, ws_bytes=_native.lib().fql_linear_workspace_bytes(B, K, N, _native.PRECISION_FP8))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Backward (input and routing-weight gradients).  The weights are frozen buffers: no weight gradient is computed, and
# the backward is once-differentiable.  Inference is untouched: the autograd wrappers below are entered only when grad
# mode is on and an input requires grad, and their forward is the plain op (bit for bit the same values).
# ---------------------------------------------------------------------------------------------------------------------

def _grad_dtypes(grad_out, out_dtype, rows):
    if not grad_out.is_cuda or grad_out.dtype not in _DTYPES or grad_out.dim() != 2:
        raise RuntimeError(f"grad_out must be a CUDA float32, float16 or bfloat16 [{rows}, N] tensor")
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    return out_dtype


def linear_backward_input(grad_out, packed_weights, scales, zero_points, precision="default", out_dtype=None):
    """``grad_in = grad_out @ W`` for the per-row INT4 weights ``W = (q - zp) * s`` ([N, K]): the transposed INT4 GEMM
    of csrc/fql_bwd.h.  ``grad_out`` [B, N] float32 / float16 / bfloat16 on the GPU -> [B, K] ``out_dtype`` (default
    float32).  A 16-bit ``grad_out`` is read as it is and a 16-bit result is rounded once in the kernel: bit for bit
    ``linear_backward_input(grad_out.float()).to(out_dtype)`` with no float32 copy made."""
    out_dtype = _grad_dtypes(grad_out, out_dtype, "B")
    dev = grad_out.device
    packed_weights, scales, zero_points, _, N, K = _check_weights(packed_weights, scales, zero_points, dev)
    B = grad_out.shape[0]
    if grad_out.shape[1] != N:
        raise RuntimeError("grad_out must have output_dim columns")
    prec = _precision(precision)
    out = torch.empty((B, K), dtype=out_dtype, device=dev)
    _launch("fql_linear_bwd_input", dev, grad_out.contiguous(), _DTYPES[grad_out.dtype], packed_weights, scales,
            zero_points, out, _DTYPES[out_dtype], B, K, N, prec,
            ws_bytes=_native.lib().fql_linear_bwd_workspace_bytes(B, K, N, prec))
    return out


def moe_backward_input(packed_weights, scales, zero_points, grad_out, tokens_per_expert, input_offsets,
                       precision="default", out_dtype=None):
    """Grouped ``grad_in[t] = grad_out[t] @ W_e`` for the rows of each expert's range; rows no expert covers are zero.
    ``grad_out`` [T, N] float32 / float16 / bfloat16, ``packed_weights`` [E, N, K/2] -> [T, K] ``out_dtype`` (default
    float32); 16-bit types as in ``linear_backward_input``.  Per-group ``scales`` / ``zero_points``
    [E, N, K / group_size] take the float32 matrix-core kernel of csrc/fql_group_bwd.h (``precision`` does not enter it):
    a fixed summation order, so the grouped call equals the one-expert calls bit for bit."""
    out_dtype = _grad_dtypes(grad_out, out_dtype, "T")
    dev = grad_out.device
    packed_weights, scales, zero_points, E, N, K, group = _expert_weights(packed_weights, scales, zero_points, dev)
    T = grad_out.shape[0]
    if grad_out.shape[1] != N:
        raise RuntimeError("grad_out must be [T, ffn_dim]")
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev)
    out = torch.empty((T, K), dtype=out_dtype, device=dev)
    if group is not None:                                   # per-group weights: csrc/fql_group_bwd.h (float32 contraction)
        _group_precision(precision)
        _launch("fql_moe_group_bwd_input", dev, packed_weights, scales, zero_points, grad_out.contiguous(),
                _DTYPES[grad_out.dtype], tpe, offs, out, _DTYPES[out_dtype], E, T, K, N, group,
                ws_bytes=_native.lib().fql_moe_group_bwd_workspace_bytes(E, T, K, N, group))
        return out
    prec = _precision(precision)
    _launch("fql_moe_bwd_input", dev, packed_weights, scales, zero_points, grad_out.contiguous(), _DTYPES[grad_out.dtype],
            tpe, offs, out, _DTYPES[out_dtype], E, T, K, N, prec,
            ws_bytes=_native.lib().fql_moe_bwd_workspace_bytes(E, T, K, N, prec))
    return out


def moe_backward_input_mxfp4(blocks, scales, grad_out, tokens_per_expert, input_offsets, out_dtype=None):
    """Grouped ``grad_in[t] = bf16(grad_out[t]) @ W_e`` on OCP MXFP4 expert weights, for the rows of each expert's range;
    rows no expert covers are zero.  ``blocks`` uint8 [E, N, K/2] and ``scales`` uint8 [E, N, K/32] as
    ``moe_forward_mxfp4`` takes them; ``grad_out`` [T, N] float32 (rounded once to bfloat16) or bfloat16 -> [T, K]
    ``out_dtype`` (default float32), rounded once.  The transposed bfloat16 matrix-core GEMM of csrc/fql_gemm_mx4_bwd.h: the
    weights are exact, the accumulation is float32 in a fixed order, so the grouped call equals the one-expert calls bit
    for bit.  The table as ``moe_forward`` takes it, or none with one expert (all rows).  A non-finite element of a
    gradient row makes that whole row of the result NaN."""
    # (types and shapes first, then the devices: the argument errors read the same with or without a GPU)
    if grad_out.dim() != 2 or grad_out.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("ops.moe_backward_input_mxfp4: grad_out must be a float32 or bfloat16 [T, N] tensor (float16 is "
                           "refused: rounding it to bfloat16 would lose three bits; cast it yourself)")
    if blocks.dtype != torch.uint8 or blocks.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("blocks must be uint8 [num_experts, N, K/2] and scales uint8 [num_experts, N, K/32]")
    if grad_out.shape[1] != blocks.shape[1]:
        raise RuntimeError("grad_out must be [T, N] for blocks [num_experts, N, K/2]")
    out_dtype = _grad_dtypes(grad_out, out_dtype, "T")
    dev, T, K = grad_out.device, grad_out.shape[0], 2 * blocks.shape[2]
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    out = torch.empty((T, K), dtype=out_dtype, device=dev)
    _launch("fql_moe_mx4_bwd_input", dev, blocks, scales, grad_out.contiguous(), _DTYPES[grad_out.dtype], tpe, offs, out,
            _DTYPES[out_dtype], E, T, K, N)
    return out


def _nvfp4_backward_input(name, blocks, scales, global_scale, grad_out, tokens_per_expert, input_offsets, out_dtype, dense,
                          lora=None):
    """Both NVFP4 input gradients, ``_nvfp4_launch``'s order of checks: types and shapes first, then the devices.  With
    ``lora`` = (dv [T, r], lora_A [E, r, K] / dense [r, K]) their adapter forms."""
    if grad_out.dim() != 2 or grad_out.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ops.{name}: grad_out must be a float32 or bfloat16 [T, N] tensor (float16 is refused: rounding "
                           "it to bfloat16 would lose three bits; cast it yourself)")
    wd = 2 if dense else 3
    shape = "[N, K/2] and scales_e4m3 uint8 [N, K/16]" if dense else "[num_experts, N, K/2] and scales_e4m3 uint8 [num_experts, N, K/16]"
    if blocks.dtype != torch.uint8 or blocks.dim() != wd or scales.dtype != torch.uint8 or scales.dim() != wd:
        raise RuntimeError(f"blocks must be uint8 {shape}")
    E = 1 if dense else blocks.shape[0]
    N, K = blocks.shape[-2], 2 * blocks.shape[-1]
    if K % 32 != 0 or tuple(scales.shape) != tuple(blocks.shape[:-1]) + (K // 16,):
        raise RuntimeError(f"blocks must be uint8 {shape} with K % 32 == 0")
    if grad_out.shape[1] != N:
        raise RuntimeError(f"ops.{name}: grad_out must be [T, N] for blocks {list(blocks.shape)}")
    if global_scale is not None and (not isinstance(global_scale, torch.Tensor) or global_scale.dtype != torch.float32
                                     or global_scale.numel() != E or global_scale.dim() > 1):
        raise RuntimeError(f"global_scale must be a float32 tensor of {E} element(s) (one per expert), or None")
    T = grad_out.shape[0]
    if lora is not None:
        r = _nvfp4_lora_operands(name, lora, T, lambda r: (r, K) if dense else (E, r, K))
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    if not grad_out.is_cuda:
        raise RuntimeError(f"ops.{name}: grad_out must be a CUDA tensor")
    dev = grad_out.device
    _on(dev, blocks=blocks, scales_e4m3=scales, global_scale=global_scale)
    tpe, offs = (None, None) if dense else _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    out = torch.empty((T, K), dtype=out_dtype, device=dev)
    gs = None if global_scale is None else global_scale.contiguous()
    if lora is None:
        _launch("fql_moe_nvfp4_bwd_input", dev, blocks.contiguous(), scales.contiguous(), gs, grad_out.contiguous(),
                _DTYPES[grad_out.dtype], tpe, offs, out, _DTYPES[out_dtype], E, T, K, N)
        return out
    _on(dev, lora_rows=lora[0], lora_weight=lora[1])
    if T == 0:
        return out
    if N == 0:
        raise RuntimeError(f"ops.{name}: blocks with no rows (N == 0) have no adapter form")
    table, shape = ((), (T, K, N)) if dense else ((tpe, offs), (E, T, K, N))
    _launch("fql_linear_nvfp4_lora_bwd_input" if dense else "fql_moe_nvfp4_lora_bwd_input", dev, blocks.contiguous(),
            scales.contiguous(), gs, grad_out.contiguous(), _DTYPES[grad_out.dtype], lora[0].contiguous(), lora[1].contiguous(), r,
            *table, out, _DTYPES[out_dtype], *shape)
    return out


def moe_backward_input_nvfp4(blocks, scales_e4m3, global_scale, grad_out, tokens_per_expert, input_offsets, out_dtype=None):
    """Grouped ``grad_in[t] = (bf16(grad_out[t]) @ W_e) * global_scale[e]`` on NVFP4 expert weights, for the rows of each
    expert's range; rows no expert covers are zero.  ``blocks`` uint8 [E, N, K/2], ``scales_e4m3`` uint8 [E, N, K/16] and
    ``global_scale`` float32 [E] or None (1) as ``moe_forward_nvfp4`` takes them; ``grad_out`` [T, N] float32 (rounded once
    to bfloat16) or bfloat16 -> [T, K] ``out_dtype`` (default float32), rounded once.  The transposed bfloat16 matrix-core
    GEMM of csrc/fql_gemm_nvfp4_bwd.h: the weights without the global scale are exact, the accumulation is float32 in a
    fixed order, so the grouped call equals the one-expert calls bit for bit.  The table as ``moe_forward`` takes it, or
    none with one expert (all rows).  A non-finite element of a gradient row makes that whole row of the result NaN; a
    NaN scale byte makes its 16 columns NaN on the rows of its expert."""
    return _nvfp4_backward_input("moe_backward_input_nvfp4", blocks, scales_e4m3, global_scale, grad_out, tokens_per_expert,
                                 input_offsets, out_dtype, False)


def linear_backward_input_nvfp4(blocks, scales_e4m3, global_scale, grad_out, out_dtype=None):
    """``grad_in[t] = (bf16(grad_out[t]) @ W) * global_scale`` on dense NVFP4 weights ``blocks`` [N, K/2] / ``scales_e4m3``
    [N, K/16] / ``global_scale`` float32 with one element or None: ``moe_backward_input_nvfp4`` on the one-expert view
    without a table, the same kernel, the same bits.  ``grad_out`` [T, N] float32 or bfloat16 -> [T, K] ``out_dtype``
    (default float32)."""
    return _nvfp4_backward_input("linear_backward_input_nvfp4", blocks, scales_e4m3, global_scale, grad_out, None, None,
                                 out_dtype, True)


def moe_bias_grad(grad_rows, num_experts, tokens_per_expert=None, input_offsets=None):
    """Gradient of a per-expert bias: ``grad_bias[e] = sum of grad_rows[t] over the rows t of expert e`` -> [E, N] float32.
    ``grad_rows`` [T, N] float32 / float16 / bfloat16 (read as it is, widened exactly); the expert table as
    ``moe_forward`` takes it, or none with ``num_experts == 1`` (all rows).  One launch, float32 accumulation, no atomics:
    an expert's summation order depends on its row count alone, so the result is run-to-run identical and does not change
    when the table is permuted.  Experts without rows get zeros (csrc/fql_bias.hip)."""
    if not grad_rows.is_cuda or grad_rows.dtype not in _DTYPES or grad_rows.dim() != 2:
        raise RuntimeError("grad_rows must be a CUDA float32, float16 or bfloat16 [T, N] tensor")
    dev = grad_rows.device
    E = int(num_experts)
    if E < 0:
        raise RuntimeError("num_experts must not be negative")
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    T, N = grad_rows.shape
    out = torch.empty((E, N), dtype=torch.float32, device=dev)
    if E == 0 or N == 0:
        return out
    _launch("fql_moe_bias_grad", dev, grad_rows.contiguous(), _DTYPES[grad_rows.dtype], tpe, offs, out, E, T, N)
    return out


# rows of per-group weights dequantised at a time by the unfused backward (bounds its float32 transient to
# GROUP_BWD_CHUNK * K * 4 bytes)
GROUP_BWD_CHUNK = 1024


def group_backward_input(grad_out, packed_weights, scales, zero_points):
    """Per-group weights (``scales`` [N, K / group_size]): UNFUSED backward -- GPU dequantise of GROUP_BWD_CHUNK rows
    of W at a time, then a float32 ``torch.mm``.  The rank-1 zero-point fold of the fused kernel does not apply here."""
    from .quantize import dequantize_weights
    N = packed_weights.shape[0]
    gy = grad_out.contiguous()
    out = None
    for n0 in range(0, N, GROUP_BWD_CHUNK):
        n1 = min(N, n0 + GROUP_BWD_CHUNK)
        w = dequantize_weights(packed_weights[n0:n1].contiguous(), scales[n0:n1].contiguous(),
                               zero_points[n0:n1].contiguous())
        part = torch.mm(gy[:, n0:n1], w)
        out = part if out is None else out.add_(part)
    return out


def combine_backward(grad_out, y, pos_of_slot, expert_weights, top_k=None, need_weights=True):
    """Gradients of ``combine``: ``(grad_y [R, N], grad_weights [T, top_k] or None)`` in one launch, no atomics.
    Rows of ``y`` that no slot names get zero."""
    return combine_any_backward(grad_out.to(torch.float32), y, pos_of_slot, expert_weights, top_k,
                                need_weights=need_weights)[:2]


def combine_any_backward(grad_out, y, pos_of_slot, expert_weights, top_k=None, addend=None, addend_weight=None,
                         need_weights=True, need_addend=True, need_addend_weight=True, skip_dropped=False):
    """Gradients of ``combine_any`` in one launch, no atomics: ``(grad_y [R, N], grad_weights [T, top_k], grad_addend
    [T, N], grad_addend_weight [T])``, None for what does not exist or is not needed.  ``grad_out`` [T, N] float32 /
    float16 / bfloat16 is read as it is; ``grad_y`` and ``grad_addend`` have ``y``'s type (rounded once), the two weight
    gradients are float32.  Rows of ``y`` that no slot names get zero.  ``skip_dropped=True``: the backward of
    ``combine_any(..., skip_dropped=True)``; a slot with ``pos_of_slot < 0`` gets a zero weight gradient and names no row
    (``grad_y`` is allocated as zeros)."""
    T, top_k, pos, w, addend, aw = _combine_operands(y, pos_of_slot, expert_weights, top_k, addend, addend_weight)
    dev = y.device
    R, N = y.shape
    _on(dev, grad_out=grad_out)
    if grad_out.dtype not in _DTYPES or tuple(grad_out.shape) != (T, N):
        raise RuntimeError("grad_out must be a float32, float16 or bfloat16 [tokens, N] tensor")
    grad_y = (torch.empty if R == T * top_k and not skip_dropped else torch.zeros)((R, N), dtype=y.dtype, device=dev)
    grad_w = torch.empty((T, top_k), dtype=torch.float32, device=dev) if (need_weights and w is not None) else None
    grad_a = torch.empty((T, N), dtype=y.dtype, device=dev) if (need_addend and addend is not None) else None
    grad_aw = torch.empty(T, dtype=torch.float32, device=dev) if (need_addend_weight and aw is not None) else None
    _launch("fql_combine_sparse_bwd" if skip_dropped else "fql_combine_bwd", dev, grad_out.contiguous(),
            _DTYPES[grad_out.dtype], y.contiguous(), pos, w, addend, aw, _DTYPES[y.dtype], grad_y, grad_w, grad_a, grad_aw,
            T, top_k, N, R)
    return grad_y, grad_w, grad_a, grad_aw


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _forward_only(name, *tensors):
    """The ops without a backward refuse inputs that require grad (under grad mode): their output would carry no
    grad_fn, and everything upstream of them would silently get no gradient."""
    if _wants_grad(*tensors):
        raise RuntimeError(f"ops.{name} has no backward (forward-only); call it under torch.no_grad() or on detached "
                           "inputs.  The differentiable ops are linear_forward, linear_forward_any, moe_forward, "
                           "moe_forward_any, combine and combine_any (INTEGRATION.md section 5)")


class _LinearFn(torch.autograd.Function):
    """``linear_forward`` / ``linear_forward_any`` with an input gradient (fused, per-row weights) or the unfused
    per-group one.  Saves the weight buffers only."""

    @staticmethod
    def forward(ctx, x, packed, scales, zps, bias, precision, out_dtype, any_dtype):
        ctx.save_for_backward(packed, scales, zps)
        ctx.precision, ctx.x_dtype, ctx.x_dim = precision, x.dtype, x.dim()
        ctx.bias_grad = bias is not None and bias.requires_grad
        if any_dtype:
            return linear_forward_any(x, packed, scales, zps, precision=precision, out_dtype=out_dtype, bias=bias)
        return linear_forward(x, packed, scales, zps, precision=precision, bias=bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        packed, scales, zps = ctx.saved_tensors
        g2 = gy.reshape(-1, gy.shape[-1])
        if _per_group(scales):                                 # per-group weights: unfused, float32 in torch
            gx = group_backward_input(g2.to(torch.float32), packed, scales, zps).to(ctx.x_dtype)
        else:                                                  # gy in its own type, dX in x's: no cast pass
            gx = linear_backward_input(g2, packed, scales, zps, precision=ctx.precision, out_dtype=ctx.x_dtype)
        gx = gx.reshape(-1) if ctx.x_dim == 1 else gx
        gb = g2.sum(0, dtype=torch.float32) if ctx.bias_grad else None
        return gx, None, None, None, gb, None, None, None


class _MoEFn(torch.autograd.Function):
    """``moe_forward`` / ``moe_forward_any`` with the grouped input gradient and, for a per-expert ``bias`` that requires
    grad, its gradient (``moe_bias_grad`` of the incoming gradient).  Saves the weight buffers and the expert table only."""

    @staticmethod
    def forward(ctx, inputs, packed, scales, zps, tpe, offs, precision, out_dtype, any_dtype, bias=None):
        ctx.save_for_backward(packed, scales, zps, tpe, offs)
        ctx.precision, ctx.x_dtype = precision, inputs.dtype
        if any_dtype:
            return moe_forward_any(packed, scales, zps, inputs, None, tpe, offs, precision=precision, out_dtype=out_dtype,
                                   bias=bias)
        return moe_forward(packed, scales, zps, inputs, None, tpe, offs, precision=precision, bias=bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        packed, scales, zps, tpe, offs = ctx.saved_tensors
        gx = gb = None
        if ctx.needs_input_grad[0]:
            gx = moe_backward_input(packed, scales, zps, gy, tpe, offs, precision=ctx.precision, out_dtype=ctx.x_dtype)
        if len(ctx.needs_input_grad) > 9 and ctx.needs_input_grad[9]:
            gb = moe_bias_grad(_grad_rows(gy), packed.shape[0], tpe, offs)
        return gx, None, None, None, None, None, None, None, None, gb


class _CombineFn(torch.autograd.Function):
    """``combine`` / ``combine_any`` with the four gradients from one launch.  Saves ``y`` and ``addend`` in their own
    type."""

    @staticmethod
    def forward(ctx, y, pos_of_slot, expert_weights, top_k, addend, addend_weight, out_dtype, skip_dropped=False):
        ctx.save_for_backward(y, pos_of_slot, expert_weights, addend, addend_weight)
        ctx.top_k, ctx.skip_dropped = top_k, skip_dropped
        return combine_any(y, pos_of_slot, expert_weights, top_k, addend, addend_weight, out_dtype, skip_dropped)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        y, pos, w, addend, aw = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy, gw, ga, gaw = combine_any_backward(gout, y, pos, w, ctx.top_k, addend, aw, need_weights=need[2],
                                               need_addend=need[4], need_addend_weight=need[5],
                                               skip_dropped=ctx.skip_dropped)
        if gw is not None and w.dtype != torch.float32:
            gw = gw.to(w.dtype)
        return (gy if need[0] else None, None, gw, None, ga, gaw, None) + (None,) * (len(need) - 7)


class _RouterTopkFn(torch.autograd.Function):
    """``router_topk`` / ``router_score_topk`` with the gradient to the logits.  Saves the logits and the indices; the
    scores are recomputed."""

    @staticmethod
    def forward(ctx, logits, top_k, scoring, select_bias, n_group, topk_group, group_top, renormalize, scale, return_scores):
        out = router_score_topk(logits.detach(), top_k, scoring, select_bias, n_group, topk_group, group_top, renormalize,
                                scale, return_scores)
        ctx.save_for_backward(logits, out[1])
        ctx.scoring, ctx.renormalize, ctx.scale = scoring, renormalize, scale
        ctx.set_materialize_grads(False)                       # a gradient that does not exist arrives as None
        ctx.mark_non_differentiable(out[1])
        return out if return_scores else out + (None,)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_weights, _grad_indices, grad_scores):
        logits, indices = ctx.saved_tensors
        return (router_score_topk_backward(logits, indices, grad_weights, grad_scores, ctx.scoring, ctx.renormalize,
                                           ctx.scale),) + (None,) * 9


class _DispatchRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, token_of_sorted, pos_of_slot, top_k, skip_dropped=False):
        ctx.save_for_backward(pos_of_slot)
        ctx.top_k, ctx.x_dtype, ctx.skip_dropped = top_k, x.dtype, skip_dropped
        return dispatch_rows(x.detach(), token_of_sorted, pos_of_slot, top_k)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        pos_of_slot, = ctx.saved_tensors
        rest = (None,) * (len(ctx.needs_input_grad) - 1)
        if grad_rows.dtype not in _DTYPES or ctx.x_dtype not in _DTYPES:      # (a float64 x: through float32, as before)
            g32 = grad_rows.to(torch.float32)
            if ctx.skip_dropped:
                return (combine_any(g32, pos_of_slot, None, ctx.top_k, skip_dropped=True).to(ctx.x_dtype),) + rest
            return (combine(g32, pos_of_slot, None, ctx.top_k).to(ctx.x_dtype),) + rest
        return (combine_any(grad_rows, pos_of_slot, None, ctx.top_k, out_dtype=ctx.x_dtype,
                            skip_dropped=ctx.skip_dropped),) + rest


# ---------------------------------------------------------------------------------------------------------------------
# Low-rank adapters (LoRA) on the INT4 layers: y = W_q x + scaling * B (A x), with float32 lora_A [r, K] / [E, r, K] and
# lora_B [N, r] / [E, N, r] (PEFT's layout).  The segmented kernels of csrc/fql_lora.h run the adapter for every expert
# in one launch each, from the device-side expert table of the grouped GEMM.
# ---------------------------------------------------------------------------------------------------------------------

LORA_RANKS = (4, 8, 16, 32, 64)          # ranks the kernels are built for (csrc/fql_lora.hip)
_LORA_LAYOUTS = {"rc": _native.LORA_RC, "cr": _native.LORA_CR}


def _lora_layout(layout):
    try:
        return _LORA_LAYOUTS[layout]
    except KeyError:
        raise ValueError(f"layout must be 'rc' ([E, r, C]) or 'cr' ([E, C, r]), got {layout!r}") from None


def _lora_rows(t, name, dev, wide=False):
    """A [T, r] tensor (float32), or with ``wide`` a streamed [T, C] operand (float32, float16 or bfloat16)."""
    if not t.is_cuda or t.device != dev:
        raise RuntimeError(f"{name} must be a CUDA tensor on the inputs' device")
    if t.dim() != 2 or (t.dtype != torch.float32 and not (wide and t.dtype in _DTYPES)):
        kinds = "float32, float16 or bfloat16" if wide else "float32"
        raise RuntimeError(f"{name} must be a {kinds} 2-D tensor")
    return t.contiguous()


def _lora_weight(w, layout, C, dev, name="w"):
    """Adapter weight [r, C] / [C, r] (one segment) or [E, r, C] / [E, C, r] -> (contiguous 16-byte aligned tensor, E, r)."""
    if not w.is_cuda or w.device != dev:
        raise RuntimeError(f"{name} must be a CUDA tensor on the inputs' device")
    if w.dtype != torch.float32 or w.dim() not in (2, 3):
        raise RuntimeError(f"{name} must be a float32 [r, C] / [C, r] or [E, r, C] / [E, C, r] tensor")
    w3 = w.unsqueeze(0) if w.dim() == 2 else w
    E, a, b = w3.shape
    r, c = (a, b) if _lora_layout(layout) == _native.LORA_RC else (b, a)
    if c != C:
        raise RuntimeError(f"{name} has {c} columns where the activations have {C}")
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    w3 = w3.contiguous()
    if w3.data_ptr() % 16:
        w3 = w3.clone()
    return w3, E, r


def _gate_up_rows(gate_up, dev):
    g = _lora_rows(gate_up, "gate_up", dev, wide=True)
    if g.shape[1] % 2:
        raise RuntimeError("gate_up must be [T, 2C] (gate | up)")
    return g, g.shape[0], g.shape[1] // 2


def _lora_shrink(rows, weight, layout, tokens_per_expert, input_offsets, scale, gated, act=("silu", 0.0, 0.0)):
    """``lora_shrink`` (rows = input [T, C]) / ``lora_gated_shrink`` (rows = gate_up [T, 2C]; ``act``: what
    ``activation_of`` returned)."""
    dev = rows.device
    if gated:
        x, T, C = _gate_up_rows(rows, dev)
    else:
        x = _lora_rows(rows, "input", dev, wide=True)
        T, C = x.shape
    w, E, r = _lora_weight(weight, layout, C, dev, "weight")
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    out = torch.empty((T, r), dtype=torch.float32, device=dev)
    if T == 0:
        return out
    if C == 0:
        return out.zero_()
    if gated and act[0] != "silu":
        _launch("fql_lora_glu_shrink", dev, x, _DTYPES[x.dtype], w, _lora_layout(layout), tpe, offs, out, E, T, C, r,
                float(scale), _ACTIVATIONS[act[0]], act[1], act[2])
        return out
    _launch("fql_lora_gated_shrink" if gated else "fql_lora_shrink", dev, x, _DTYPES[x.dtype], w, _lora_layout(layout),
            tpe, offs, out, E, T, C, r, float(scale))
    return out


def _lora_grad(rows, v, layout, num_experts, tokens_per_expert, input_offsets, scale, gated, act=("silu", 0.0, 0.0)):
    """``lora_grad`` (rows = p [T, C]) / ``lora_gated_grad`` (rows = gate_up [T, 2C]; ``act``: what ``activation_of``
    returned)."""
    dev = rows.device
    name = "gate_up" if gated else "p"
    if gated:
        pp, T, C = _gate_up_rows(rows, dev)
    else:
        pp = _lora_rows(rows, name, dev, wide=True)
        T, C = pp.shape
    vv = _lora_rows(v, "v", dev)
    r = vv.shape[1]
    if vv.shape[0] != T:
        raise RuntimeError(f"{name} and v must have the same number of rows")
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    E = int(num_experts)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    lay = _lora_layout(layout)
    shape = (E, C, r) if lay == _native.LORA_CR else (E, r, C)
    if T == 0 or C == 0 or E == 0:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    d = torch.empty(shape, dtype=torch.float32, device=dev)
    if vv.data_ptr() % 16:
        vv = vv.clone()
    if gated and act[0] != "silu":
        _launch("fql_lora_glu_grad", dev, pp, _DTYPES[pp.dtype], vv, tpe, offs, d, lay, E, T, C, r, float(scale),
                _ACTIVATIONS[act[0]], act[1], act[2])
        return d
    _launch("fql_lora_gated_grad" if gated else "fql_lora_grad", dev, pp, _DTYPES[pp.dtype], vv, tpe, offs, d, lay,
            E, T, C, r, float(scale))
    return d


def lora_shrink(input, weight, layout="rc", tokens_per_expert=None, input_offsets=None, scale=1.0):
    """Segmented ``out[t] = scale * input[t] @ W_e^T`` -> [T, r] float32: ``weight`` [E, r, C] (``layout='rc'``, e.g.
    lora_A) or [E, C, r] (``'cr'``, e.g. lora_B), 2-D for one segment.  Rows no expert covers are zero.  ``input`` may
    be float16 / bfloat16: read as it is, bit for bit the call on ``input.float()``."""
    return _lora_shrink(input, weight, layout, tokens_per_expert, input_offsets, scale, gated=False)


def lora_expand(v, weight, layout="cr", tokens_per_expert=None, input_offsets=None, scale=1.0, input=None, out=None,
                out_dtype=None):
    """Segmented ``out[t] = input[t] + scale * v[t] @ W_e^T`` -> [T, C]: ``v`` [T, r] float32, ``weight`` [E, C, r]
    (``layout='cr'``, e.g. lora_B) or [E, r, C] (``'rc'``, e.g. lora_A).  ``input`` None starts from zero; ``out`` may be
    ``input`` (in place; it must then be contiguous).  Rows no expert covers get ``input`` (or zero).  ``input`` and
    ``out`` may each be float32, float16 or bfloat16 (in place: one type); without ``out=`` the result has ``out_dtype``
    (default: ``input``'s type, float32 without an input).  A 16-bit result is the float32 one rounded once."""
    dev = v.device
    vv = _lora_rows(v, "v", dev)
    T = vv.shape[0]
    ref = input if input is not None else out
    if ref is None:
        raise RuntimeError("lora_expand needs `input` or `out` to know the number of columns")
    C = ref.shape[-1]
    w, E, r = _lora_weight(weight, layout, C, dev, "weight")
    if vv.shape[1] != r:
        raise RuntimeError(f"v has {vv.shape[1]} columns where the adapter rank is {r}")
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    inp = None
    if input is not None:
        if tuple(input.shape) != (T, C):
            raise RuntimeError("input must be [T, C]")
        inp = input if (out is not None and input is out) else _lora_rows(input, "input", dev, wide=True)
    if out is None:
        if out_dtype is None:
            out_dtype = torch.float32 if inp is None else inp.dtype
        if out_dtype not in _DTYPES:
            raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
        out = torch.empty((T, C), dtype=out_dtype, device=dev)
    elif (not out.is_cuda or out.device != dev or out.dtype not in _DTYPES or tuple(out.shape) != (T, C)
          or not out.is_contiguous() or (out_dtype is not None and out_dtype != out.dtype)):
        raise RuntimeError("out must be a contiguous CUDA float32 / float16 / bfloat16 [T, C] tensor on the inputs' "
                           "device (of out_dtype, when that is given)")
    if T == 0 or C == 0:
        return out
    _launch("fql_lora_expand", dev, vv, w, _lora_layout(layout), tpe, offs, inp,
            _native.DTYPE_F32 if inp is None else _DTYPES[inp.dtype], out, _DTYPES[out.dtype], E, T, C, r, float(scale))
    return out


def lora_grad(p, v, layout, num_experts=1, tokens_per_expert=None, input_offsets=None, scale=1.0):
    """Segment reduction ``D_e = scale * sum_{t of e} p[t]^T v[t]`` per expert: ``p`` [T, C], ``v`` [T, r] ->
    [E, C, r] (``layout='cr'``: dB) or [E, r, C] (``'rc'``: dA), float32.  Experts without rows get zeros.  ``p`` may be
    float16 / bfloat16: read as it is, bit for bit the call on ``p.float()``."""
    return _lora_grad(p, v, layout, num_experts, tokens_per_expert, input_offsets, scale, gated=False)


def _lora_check_adapters(lora_A, lora_B, K, N, E):
    """lora_A [r, K] / lora_B [N, r] (E == 1: 2-D) or [E, r, K] / [E, N, r]: float32 CUDA."""
    for name, t in (("lora_A", lora_A), ("lora_B", lora_B)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be a float32 CUDA tensor: the adapter weights and their gradients stay "
                               "float32 whatever the activations' type (keep them out of a module-wide .half() / "
                               ".bfloat16(), or cast them back)")
    want_dim = 2 if E is None else 3
    if lora_A.dim() != want_dim or lora_B.dim() != want_dim:
        raise RuntimeError("lora_A / lora_B must be [r, K] / [N, r] for a linear layer, [E, r, K] / [E, N, r] for MoE")
    r = lora_A.shape[-2]
    if lora_A.shape[-1] != K or tuple(lora_B.shape[-2:]) != (N, r) or (E is not None and (lora_A.shape[0] != E
                                                                                        or lora_B.shape[0] != E)):
        raise RuntimeError(f"lora_A must be [{'E, ' if E else ''}r, {K}] and lora_B [{'E, ' if E else ''}{N}, r]")
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")


def _expand_into(v, weight, layout, base32, dtype, tpe=None, offs=None, scale=1.0):
    """``base32 + scale * v W`` in ``dtype``: in place on the float32 base, or one 16-bit write from it."""
    if dtype == torch.float32:
        return lora_expand(v, weight, layout, tpe, offs, scale=scale, input=base32, out=base32)
    return lora_expand(v, weight, layout, tpe, offs, scale=scale, input=base32, out_dtype=dtype)


def _linear_lora_apply(x2, packed, scales, zps, lora_A, lora_B, scaling, precision, bias):
    """Base forward to float32, U = x A^T, then y = base + scaling * U B^T in x's type.  Returns (y, U).
    16-bit x: the base GEMM and the shrink read x as it is and the expand writes y once -- one rounding, no float32
    copy of x (but on the unfused per-group branch, where torch widens x)."""
    y32 = linear_forward_any(x2.float() if _per_group(scales) else x2, packed, scales, zps, precision=precision,
                             out_dtype=torch.float32, bias=bias)
    u = lora_shrink(x2, lora_A, "rc")
    return _expand_into(u, lora_B, "cr", y32, x2.dtype, scale=scaling), u


def linear_lora_forward(x, packed, scales, zps, lora_A, lora_B, scaling, precision="default", bias=None):
    """INT4 linear plus a low-rank adapter: ``x @ W_q^T (+ bias) + scaling * (x @ lora_A^T) @ lora_B^T``, ``x`` [K]
    or [B, K] float32 / float16 / bfloat16, float32 ``lora_A`` [r, K] and ``lora_B`` [N, r]; the result has ``x``'s
    type.  Differentiable in ``x``, ``lora_A``, ``lora_B`` and ``bias`` (the INT4 weights are frozen); the backward
    reuses the fused input gradient of the base layer.  16-bit ``x``: bit for bit the float32 call on ``x.float()``
    with ``y`` and ``x.grad`` rounded once; the adapter gradients are float32."""
    if not x.is_cuda or x.dtype not in _DTYPES:
        raise RuntimeError("linear_lora_forward: x must be a CUDA float32, float16 or bfloat16 tensor")
    if x.dim() not in (1, 2):
        raise RuntimeError("x must be 1-D or 2-D")
    K = x.shape[-1]
    _lora_check_adapters(lora_A, lora_B, K, packed.shape[0], None)
    if _wants_grad(x, lora_A, lora_B, bias):
        return _LinearLoRAFn.apply(x, lora_A, lora_B, bias, packed, scales, zps, float(scaling), precision)
    x2 = x.unsqueeze(0) if x.dim() == 1 else x
    y, _ = _linear_lora_apply(x2, packed, scales, zps, lora_A, lora_B, float(scaling), precision, bias)
    return y.squeeze(0) if x.dim() == 1 else y


def moe_lora_forward(packed, scales, zps, inputs, lora_A, lora_B, scaling, tokens_per_expert, input_offsets,
                     precision="default"):
    """Grouped INT4 GEMM plus a per-expert low-rank adapter: for the rows t of expert e,
    ``y[t] = inputs[t] @ W_e^T + scaling * (inputs[t] @ lora_A[e]^T) @ lora_B[e]^T``; rows no expert covers are zero.
    ``lora_A`` [E, r, K], ``lora_B`` [E, N, r] float32.  Per-row INT4 weights only.  Differentiable in ``inputs``,
    ``lora_A`` and ``lora_B``.  ``inputs`` float32 / float16 / bfloat16, result in the same type (16-bit: as
    ``linear_lora_forward``)."""
    if not inputs.is_cuda or inputs.dtype not in _DTYPES or inputs.dim() != 2:
        raise RuntimeError("inputs must be a CUDA float32, float16 or bfloat16 [T, K] tensor")
    if packed.dim() != 3 or scales.dim() != 2:
        raise RuntimeError("moe_lora_forward takes per-row INT4 weights: packed [E, N, K/2], scales / zero_points [E, N]")
    E, N = packed.shape[0], packed.shape[1]
    _lora_check_adapters(lora_A, lora_B, inputs.shape[1], N, E)
    if _wants_grad(inputs, lora_A, lora_B):
        return _MoELoRAFn.apply(inputs, lora_A, lora_B, packed, scales, zps, tokens_per_expert, input_offsets,
                                float(scaling), precision)
    y, _ = _moe_lora_apply(packed, scales, zps, inputs, lora_A, lora_B, float(scaling), tokens_per_expert,
                           input_offsets, precision)
    return y


def _moe_lora_apply(packed, scales, zps, inputs, lora_A, lora_B, scaling, tpe, offs, precision):
    y32 = moe_forward_any(packed, scales, zps, inputs, None, tpe, offs, precision=precision, out_dtype=torch.float32)
    u = lora_shrink(inputs, lora_A, "rc", tpe, offs)
    return _expand_into(u, lora_B, "cr", y32, inputs.dtype, tpe, offs, scaling), u


class _LinearLoRAFn(torch.autograd.Function):
    """Base INT4 linear + adapter in one node.  Saves x (in its own type) and U = x A^T ([B, r] float32); nothing
    dequantised.  gy is read in its own type; a 16-bit dX is written once, by the expand, from the float32 base dX."""

    @staticmethod
    def forward(ctx, x, lora_A, lora_B, bias, packed, scales, zps, scaling, precision):
        x2 = (x.unsqueeze(0) if x.dim() == 1 else x).contiguous()
        y, u = _linear_lora_apply(x2, packed, scales, zps, lora_A, lora_B, scaling, precision, bias)
        ctx.save_for_backward(x2, u, lora_A, lora_B, packed, scales, zps)
        ctx.scaling, ctx.precision, ctx.x_dim = scaling, precision, x.dim()
        return y.squeeze(0) if x.dim() == 1 else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x2, u, lora_A, lora_B, packed, scales, zps = ctx.saved_tensors
        need_x, need_A, need_B, need_b = ctx.needs_input_grad[:4]
        g = _grad_rows(gy.reshape(-1, gy.shape[-1]))
        gx = gA = gB = gb = None
        if need_x or need_A:
            du = lora_shrink(g, lora_B, "cr", scale=ctx.scaling)                # dU = s G B
            if need_x:
                if _per_group(scales):                                          # unfused: torch widens gy here only
                    gx = group_backward_input(g.to(torch.float32), packed, scales, zps)
                else:
                    gx = linear_backward_input(g, packed, scales, zps, precision=ctx.precision)
                gx = _expand_into(du, lora_A, "rc", gx, x2.dtype)               # dX += dU A
                gx = gx.reshape(-1) if ctx.x_dim == 1 else gx
            if need_A:
                gA = lora_grad(x2, du, "rc")[0]                                  # dA = dU^T X
        if need_B:
            gB = lora_grad(g, u, "cr", scale=ctx.scaling)[0]                     # dB = s G^T U
        if need_b:
            gb = g.sum(0, dtype=torch.float32)
        return gx, gA, gB, gb, None, None, None, None, None


def _grad_rows(gy):
    """The incoming gradient as the kernels read it: contiguous, in its own type (float32 / float16 / bfloat16)."""
    if gy.dtype not in _DTYPES:
        raise RuntimeError("the gradient must be float32, float16 or bfloat16")
    return gy.contiguous()


class _MoELoRAFn(torch.autograd.Function):
    """Grouped INT4 GEMM + per-expert adapter in one node.  Saves inputs (in their own type), U ([T, r] float32) and the
    expert table."""

    @staticmethod
    def forward(ctx, inputs, lora_A, lora_B, packed, scales, zps, tpe, offs, scaling, precision):
        y, u = _moe_lora_apply(packed, scales, zps, inputs, lora_A, lora_B, scaling, tpe, offs, precision)
        ctx.save_for_backward(inputs.contiguous(), u, lora_A, lora_B, packed, scales, zps, tpe, offs)
        ctx.scaling, ctx.precision = scaling, precision
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, u, lora_A, lora_B, packed, scales, zps, tpe, offs = ctx.saved_tensors
        need_x, need_A, need_B = ctx.needs_input_grad[:3]
        E = packed.shape[0]
        g = _grad_rows(gy)
        gx = gA = gB = None
        if need_x or need_A:
            du = lora_shrink(g, lora_B, "cr", tpe, offs, scale=ctx.scaling)
            if need_x:
                gx = moe_backward_input(packed, scales, zps, g, tpe, offs, precision=ctx.precision)
                gx = _expand_into(du, lora_A, "rc", gx, x.dtype, tpe, offs)
            if need_A:
                gA = lora_grad(x, du, "rc", E, tpe, offs)
        if need_B:
            gB = lora_grad(g, u, "cr", E, tpe, offs, scale=ctx.scaling)
        return gx, gA, gB, None, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# Adapters on the gated FFN experts (QuantizedMoEFFN): y = W_d h + s B_d (A_d h), h = silu(g) * u, [g | u] = W_gu x +
# s B_gu (A_gu x).  h is never written: the down adapter's shrink and weight gradient form it from gate_up with the
# function the down GEMM's pre-pass uses (csrc/fql_common.h act_silu_mul), and the backward of the gate is one
# streaming kernel.
# ---------------------------------------------------------------------------------------------------------------------

def lora_gated_shrink(gate_up, weight, layout="rc", tokens_per_expert=None, input_offsets=None, scale=1.0,
                      activation="silu", activation_alpha=1.702, activation_limit=7.0):
    """``lora_shrink`` on the hidden activation of a gated FFN expert without materialising it:
    ``out[t] = scale * (silu(gate_up[t, :C]) * gate_up[t, C:]) @ W_e^T`` -> [T, r] float32; ``gate_up`` [T, 2C]
    float32, or float16 / bfloat16 read as it is: bit for bit the call on ``gate_up.float()``.  ``activation`` (and its
    two floats, ``activation_of``): the kind of h, the bits ``moe_gated_forward`` consumes for the same kind."""
    return _lora_shrink(gate_up, weight, layout, tokens_per_expert, input_offsets, scale, gated=True,
                        act=activation_of(activation, activation_alpha, activation_limit))


def lora_gated_grad(gate_up, v, layout, num_experts=1, tokens_per_expert=None, input_offsets=None, scale=1.0,
                    activation="silu", activation_alpha=1.702, activation_limit=7.0):
    """``lora_grad`` with ``p = silu(gate_up[:, :C]) * gate_up[:, C:]`` formed on the fly: ``gate_up`` [T, 2C],
    ``v`` [T, r] -> [E, C, r] (``layout='cr'``) or [E, r, C] (``'rc'``: dA of the down adapter), float32.  ``gate_up``
    may be float16 / bfloat16: read as it is, bit for bit the call on ``gate_up.float()``.  ``activation`` (and its two
    floats, ``activation_of``): the kind of p."""
    return _lora_grad(gate_up, v, layout, num_experts, tokens_per_expert, input_offsets, scale, gated=True,
                      act=activation_of(activation, activation_alpha, activation_limit))


def swiglu_backward(gate_up, dh, out_dtype=None):
    """Backward of ``h = silu(g) * u`` in one pass: ``gate_up`` [T, 2F] = [g | u] and ``dh`` [T, F] ->
    ``[dg | du]`` [T, 2F] with ``dg = dh * u * silu'(g)``, ``du = dh * silu(g)``.  Each of ``gate_up``, ``dh`` and the
    result (``out_dtype``, default ``gate_up``'s type) may be float32, float16 or bfloat16: float32 arithmetic on the
    widened values, bit for bit ``swiglu_backward(gate_up.float(), dh.float()).to(out_dtype)``."""
    return _glu_backward(gate_up, dh, out_dtype, ("silu", 0.0, 0.0))


def glu_backward(gate_up, dh, activation="silu", activation_alpha=1.702, activation_limit=7.0, out_dtype=None):
    """``swiglu_backward`` for any activation kind (``activation_of``): with ``h = g' * sigmoid(a) * u'``,
    ``dg = dh * u' * sig * (1 + g' a' (1 - sig))`` and ``du = dh * g' * sig``; ``"swiglu_clamp"`` passes no gradient
    where its clamp is active.  ``"silu"`` is ``swiglu_backward``, kernel for kernel.  Element types as there: bit for
    bit the call on the widened operands, a 16-bit result rounded once."""
    return _glu_backward(gate_up, dh, out_dtype, activation_of(activation, activation_alpha, activation_limit))


def _glu_backward(gate_up, dh, out_dtype, act):
    dev = gate_up.device
    g, T, F = _gate_up_rows(gate_up, dev)
    d = _lora_rows(dh, "dh", dev, wide=True)
    if tuple(d.shape) != (T, F):
        raise RuntimeError(f"dh must be [{T}, {F}] for gate_up [{T}, {2 * F}]")
    out_dtype = g.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    out = torch.empty((T, 2 * F), dtype=out_dtype, device=dev)
    if T == 0 or F == 0:
        return out
    if act[0] != "silu":
        _launch("fql_glu_bwd", dev, g, _DTYPES[g.dtype], d, _DTYPES[d.dtype], out, _DTYPES[out_dtype], T, F,
                _ACTIVATIONS[act[0]], act[1], act[2])
        return out
    _launch("fql_swiglu_bwd", dev, g, _DTYPES[g.dtype], d, _DTYPES[d.dtype], out, _DTYPES[out_dtype], T, F)
    return out


def activation_dtype_of(activation_dtype):
    """The ``activation_dtype`` argument of the gated FFN layers: None / float32 (the float32 layer) or a 16-bit type."""
    if activation_dtype is None or activation_dtype == torch.float32:
        return None
    if activation_dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"activation_dtype must be None, torch.float32, torch.float16 or torch.bfloat16, got "
                         f"{activation_dtype!r}")
    return activation_dtype


def check_activation_rows(t, name, dt):
    """A [T, .] tensor of a gated FFN layer built with a 16-bit ``activation_dtype``: that type, on the GPU, 2-D."""
    if not t.is_cuda or t.dim() != 2 or t.dtype != dt:
        raise RuntimeError(f"{name} must be a CUDA {dt} 2-D tensor: the layer was built with activation_dtype={dt}, so "
                           f"pass {name}.to({dt}) (or build the layer without activation_dtype for float32 "
                           f"activations); got {t.dtype}")


def moe_ffn_lora_forward(gate_up_packed, gate_up_scales, gate_up_zps, down_packed, down_scales, down_zps, inputs,
                         gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B, scaling, tokens_per_expert,
                         input_offsets, precision="default", activation_dtype=None, activation="silu",
                         activation_alpha=1.702, activation_limit=7.0, gate_up_bias=None, down_bias=None):
    """Gated INT4 FFN experts with a low-rank adapter on each projection: for the rows t of expert e,
    ``gu = W_gu x + s B_gu (A_gu x)``, ``h = silu(gu[:F]) * gu[F:]`` (never stored), ``y = W_d h + s B_d (A_d h)``; rows
    no expert covers are zero.  ``inputs`` [T, H] float32, stacked gate|up weights [E, 2F, H/2], down weights
    [E, H, F/2], ``gate_up_lora_A`` [E, r, H], ``gate_up_lora_B`` [E, 2F, r], ``down_lora_A`` [E, r, F],
    ``down_lora_B`` [E, H, r].  Scales / zero points per row [E, N] or per group [E, N, K / group_size].  Differentiable
    (once) in ``inputs`` and the four adapters.

    ``activation_dtype`` = torch.float16 / torch.bfloat16 is the memory-for-precision form: ``inputs`` and the incoming
    gradient have that type, ``gate_up`` is stored (and saved) in it, ``y`` and ``inputs.grad`` come back in it; the
    adapters and their gradients stay float32.  Five tensors are rounded, once each.

    ``activation`` (with ``activation_alpha``, ``activation_limit``; ``activation_of``) replaces silu(g) * u by
    another kind of h in the forward and in every gradient.

    ``gate_up_bias`` [E, 2F] / ``down_bias`` [E, H] float32 (each optional): per-expert biases of the two projections,
    ``gu = W_gu x + b_gu + s B_gu (A_gu x)`` and ``y = W_d h + b_d + s B_d (A_d h)``.  A bias is part of the base GEMM's
    float32 result (its epilogue) and the adapter term is added after it.  Differentiable in them too
    (``moe_bias_grad`` of dgu and of the incoming gradient), computed only for a bias that requires grad."""
    act = activation_of(activation, activation_alpha, activation_limit)
    dt = activation_dtype_of(activation_dtype)
    if dt is not None:
        check_activation_rows(inputs, "inputs", dt)
        if _precision(precision) == _native.PRECISION_FP8:
            raise RuntimeError("precision='fp8' has no gated forward and no backward: not available with a 16-bit "
                               "activation_dtype either")
    elif not inputs.is_cuda or inputs.dtype != torch.float32 or inputs.dim() != 2:
        raise RuntimeError("inputs must be a CUDA float32 [T, H] tensor: without activation_dtype the gated FFN adapters "
                           "are float32 only (pass activation_dtype=torch.float16 / torch.bfloat16 to run the layer on "
                           "16-bit activations; gate_up is then rounded to that type between the two projections)")
    if gate_up_packed.dim() != 3 or down_packed.dim() != 3:
        raise RuntimeError("moe_ffn_lora_forward takes per-row INT4 weights: packed [E, N, K/2], scales / zero_points "
                           "[E, N] (or per-group ones: [E, N, K / group_size])")
    E, F2, H = gate_up_packed.shape[0], gate_up_packed.shape[1], inputs.shape[1]
    if F2 % 2 or tuple(down_packed.shape) != (E, H, F2 // 4):
        raise RuntimeError("gate_up_packed must be [E, 2F, H/2] and down_packed [E, H, F/2]")
    _lora_check_adapters(gate_up_lora_A, gate_up_lora_B, H, F2, E)
    _lora_check_adapters(down_lora_A, down_lora_B, F2 // 2, H, E)
    if down_lora_A.shape[1] != gate_up_lora_A.shape[1]:
        raise RuntimeError("the gate_up and down adapters must have the same rank")
    weights = (gate_up_packed, gate_up_scales, gate_up_zps, down_packed, down_scales, down_zps)
    adapters = (gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B)
    biases = (_check_bias(gate_up_bias, F2, inputs.device, E), _check_bias(down_bias, H, inputs.device, E))
    if _wants_grad(inputs, *adapters, *biases):
        return _MoEFFNLoRAFn.apply(inputs, *adapters, *weights, tokens_per_expert, input_offsets, float(scaling),
                                   precision, dt, act, *biases)
    return _moe_ffn_lora_apply(weights, inputs, adapters, float(scaling), tokens_per_expert, input_offsets,
                               precision, act, biases)[0]


def _moe_ffn_lora_apply(weights, inputs, adapters, scaling, tpe, offs, precision, act=("silu", 1.702, 7.0),
                        biases=(None, None)):
    """Returns (y, gate_up, U_gu, U_d), y and gate_up in ``inputs``' type: each base GEMM reads its operand as it is and
    writes float32 (its per-expert bias, one of ``biases``, included), and the expand adds the adapter term to that in
    place (float32) or writes the sum once in the 16-bit type -- gate_up (rounding 1) and y (rounding 2)."""
    gup, gus, guz, dp, ds, dz = weights
    A_gu, B_gu, A_d, B_d = adapters
    dt = inputs.dtype
    gu32 = moe_forward_any(gup, gus, guz, inputs, None, tpe, offs, precision=precision, out_dtype=torch.float32,
                           bias=biases[0])
    u_gu = lora_shrink(inputs, A_gu, "rc", tpe, offs)
    gate_up = _expand_into(u_gu, B_gu, "cr", gu32, dt, tpe, offs, scaling)
    del gu32
    y32 = moe_gated_forward(dp, ds, dz, gate_up, tpe, offs, precision=precision, out_dtype=torch.float32,
                            activation=act[0], activation_alpha=act[1], activation_limit=act[2], bias=biases[1])
    u_d = _lora_shrink(gate_up, A_d, "rc", tpe, offs, 1.0, gated=True, act=act)
    return _expand_into(u_d, B_d, "cr", y32, dt, tpe, offs, scaling), gate_up, u_gu, u_d


class _MoEFFNLoRAFn(torch.autograd.Function):
    """The whole gated FFN block + its two adapters in one node.  Saves inputs [T, H], gate_up [T, 2F], U_gu and U_d
    ([T, r]), the tables and the parameters: nothing of shape [T, F].  With a 16-bit ``dt`` inputs and gate_up are saved
    in that type (U_gu, U_d float32): T (2H + 4F + 8r) bytes."""

    @staticmethod
    def forward(ctx, inputs, A_gu, B_gu, A_d, B_d, gup, gus, guz, dp, ds, dz, tpe, offs, scaling, precision, dt=None,
                act=("silu", 1.702, 7.0), b_gu=None, b_d=None):
        x = inputs.contiguous()
        y, gate_up, u_gu, u_d = _moe_ffn_lora_apply((gup, gus, guz, dp, ds, dz), x, (A_gu, B_gu, A_d, B_d), scaling,
                                                    tpe, offs, precision, act, (b_gu, b_d))
        ctx.save_for_backward(x, gate_up, u_gu, u_d, A_gu, B_gu, A_d, B_d, gup, gus, guz, dp, ds, dz, tpe, offs)
        ctx.scaling, ctx.precision, ctx.act_dtype, ctx.act = scaling, precision, dt, act
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        """Every kernel reads its operand in the type it has.  The base input gradients are float32; the expand adds the
        adapter term in place, or (16-bit ``dt``) writes dh (rounding 3) and dx (rounding 5) once in ``dt``, as
        swiglu_backward writes dgu (rounding 4).  Adapter gradients are float32."""
        x, gate_up, u_gu, u_d, A_gu, B_gu, A_d, B_d, gup, gus, guz, dp, ds, dz, tpe, offs = ctx.saved_tensors
        need_x, need_Agu, need_Bgu, need_Ad, need_Bd = ctx.needs_input_grad[:5]
        need_bgu, need_bd = (tuple(ctx.needs_input_grad[17:19]) + (False, False))[:2]      # the two per-expert biases
        E, s, prec = gup.shape[0], ctx.scaling, ctx.precision
        if ctx.act_dtype is not None:
            check_activation_rows(gy, "the incoming gradient", ctx.act_dtype)
            g, dt = gy.contiguous(), ctx.act_dtype
        else:
            g, dt = gy.to(torch.float32).contiguous(), torch.float32
        gx = gAgu = gBgu = gAd = gBd = gbgu = gbd = None
        if need_Bd:
            gBd = lora_grad(g, u_d, "cr", E, tpe, offs, scale=s)                         # dB_d = s dY^T U_d
        if need_bd:
            gbd = moe_bias_grad(g, E, tpe, offs)                                         # db_d = sum of dY per expert
        through = need_x or need_Agu or need_Bgu or need_bgu                            # anything upstream of h
        if through or need_Ad:
            du_d = lora_shrink(g, B_d, "cr", tpe, offs, scale=s)                         # dU_d = s dY B_d
            if need_Ad:
                gAd = _lora_grad(gate_up, du_d, "rc", E, tpe, offs, 1.0, gated=True, act=ctx.act)   # dA_d = dU_d^T h
        if through:
            dh = moe_backward_input(dp, ds, dz, g, tpe, offs, precision=prec)            # dh = dY W_d (float32)
            dh = _expand_into(du_d, A_d, "rc", dh, dt, tpe, offs)                        #      + dU_d A_d, in dt
            dgu = _glu_backward(gate_up, dh, dt, ctx.act)
            del dh
            if need_Bgu:
                gBgu = lora_grad(dgu, u_gu, "cr", E, tpe, offs, scale=s)                 # dB_gu = s dgu^T U_gu
            if need_bgu:
                gbgu = moe_bias_grad(dgu, E, tpe, offs)                                  # db_gu = sum of dgu per expert
            if need_x or need_Agu:
                du_gu = lora_shrink(dgu, B_gu, "cr", tpe, offs, scale=s)                 # dU_gu = s dgu B_gu
                if need_x:
                    gx = moe_backward_input(gup, gus, guz, dgu, tpe, offs, precision=prec)
                    gx = _expand_into(du_gu, A_gu, "rc", gx, dt, tpe, offs)              # dx = dgu W_gu + dU_gu A_gu
                if need_Agu:
                    gAgu = lora_grad(x, du_gu, "rc", E, tpe, offs)                       # dA_gu = dU_gu^T x
        return (gx, gAgu, gBgu, gAd, gBd) + (None,) * 12 + (gbgu, gbd)


# ---------------------------------------------------------------------------------------------------------------------
# Adapters on the MXFP4 experts (MXFP4MoEFFN), fused into the bfloat16 GEMMs: the adapter term is one more contraction
# stage of the tile kernel (csrc/fql_gemm_mx4.h, csrc/fql_gemm_mx4_bwd.h), so no float32 [T, C]
# base result is written for an expand pass to read back.  The shrunk rows carry the scale: v = s A x, dv = s dY B.
# ---------------------------------------------------------------------------------------------------------------------

def _mxfp4_lora_launch(name, entry, blocks, scales, rows, cols, v, w, w_shape, tokens_per_expert, input_offsets, bias,
                       out_dtype, K, act=(), gated=False):
    """The three adapter entries.  ``rows`` [T, cols] float32 / bfloat16, ``v`` [T, r] float32, ``w`` float32 of
    ``w_shape(E, r)``.  Types and shapes first, then the devices: the argument errors read the same without a GPU."""
    if rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ops.{name}: the rows must be a float32 or bfloat16 2-D tensor (float16 is refused: rounding it "
                           "to bfloat16 would lose three bits; cast it yourself)")
    if blocks.dtype != torch.uint8 or blocks.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("blocks must be uint8 [num_experts, N, K/2] and scales uint8 [num_experts, N, K/32]")
    if K % 32 != 0 or tuple(scales.shape) != (blocks.shape[0], blocks.shape[1], K // 32):
        raise RuntimeError("blocks must be [num_experts, N, K/2] and scales [num_experts, N, K/32] with K % 32 == 0")
    if rows.shape[1] != cols:
        raise RuntimeError(f"ops.{name}: the rows must have {cols} columns for blocks {list(blocks.shape)}")
    T, E = rows.shape[0], blocks.shape[0]
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[0] != T:
        raise RuntimeError(f"ops.{name}: the shrunk rows must be a float32 [T, r] tensor with the rows' T")
    r = v.shape[1]
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    if w.dtype != torch.float32 or tuple(w.shape) != w_shape(E, r):
        raise RuntimeError(f"ops.{name}: the adapter matrix must be a float32 {list(w_shape(E, r))} tensor (the adapter "
                           "weights stay float32 whatever the activations' type)")
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPES:
        raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
    if not rows.is_cuda:
        raise RuntimeError(f"ops.{name}: the rows must be a CUDA tensor")
    dev = rows.device
    blocks, scales, E, N = _check_mxfp4(blocks, scales, dev, K)
    _on(dev, lora_rows=v, lora_weight=w)
    tpe, offs = _expert_table(tokens_per_expert, input_offsets, E, dev, optional=True)
    out_cols = K if entry == "fql_moe_mx4_lora_bwd_input" else N
    out = torch.empty((T, out_cols), dtype=out_dtype, device=dev)
    if T == 0 or out_cols == 0:
        return out
    if entry == "fql_moe_mx4_lora_bwd_input":
        if N == 0:
            raise RuntimeError(f"ops.{name}: blocks with no rows (N == 0) have no adapter form")
        _launch(entry, dev, blocks, scales, rows.contiguous(), _DTYPES[rows.dtype], v.contiguous(), w.contiguous(), r, tpe,
                offs, out, _DTYPES[out_dtype], E, T, K, N)
        return out
    bias = _check_bias(bias, N, dev, E)
    _launch(entry, dev, blocks, scales, rows.contiguous(), _DTYPES[rows.dtype], v.contiguous(), w.contiguous(), r, bias, tpe,
            offs, out, _DTYPES[out_dtype], E, T, K, N, *act,
            ws_bytes=_native.lib().fql_moe_mx4_workspace_bytes(E, T, K, N, int(gated)))
    return out


def moe_forward_mxfp4_lora(blocks, scales, inputs, v, lora_B, tokens_per_expert, input_offsets, bias=None, out_dtype=None):
    """``moe_forward_mxfp4`` (bfloat16 precision) with a low-rank adapter fused in: for the rows t of expert e,
    ``out[t] = W_e @ bf16(inputs[t]) + bf16(lora_B[e]) @ bf16(v[t]) (+ bias[e])``, rounded once to ``out_dtype``.  ``v``
    [T, r] float32 are the shrunk rows with the scale in them (``lora_shrink(inputs, lora_A, scale=s)``), ``lora_B``
    [E, N, r] float32, r in ``LORA_RANKS``.  The adapter is one more contraction stage of the tile kernel
    (csrc/fql_gemm_mx4.h): the operands are rounded to bfloat16 on their way into LDS as ``inputs`` are, the order is
    fixed, and a row's result depends on its own rows of ``inputs`` and ``v`` and its expert's weights only.  With
    ``lora_B`` zero the result is ``moe_forward_mxfp4``'s bit for bit.  A non-finite ``v[t]`` makes row t NaN.  Always the
    tile kernel (no decode form).  Forward only: ``moe_ffn_lora_forward_mxfp4`` is the differentiable form."""
    _forward_only("moe_forward_mxfp4_lora", inputs, v, lora_B, bias)
    return _mxfp4_lora_launch("moe_forward_mxfp4_lora", "fql_moe_mx4_lora_fwd", blocks, scales, inputs, 2 * blocks.shape[-1],
                              v, lora_B, lambda E, r: (E, blocks.shape[1], r), tokens_per_expert, input_offsets, bias,
                              out_dtype, 2 * blocks.shape[-1])


def moe_gated_forward_mxfp4_lora(blocks, scales, gate_up, v, lora_B, tokens_per_expert, input_offsets, activation="silu",
                                 activation_alpha=1.702, activation_limit=7.0, bias=None, out_dtype=None):
    """``moe_gated_forward_mxfp4`` (bfloat16 precision) with the adapter stage of ``moe_forward_mxfp4_lora``:
    ``out[t] = W_e @ h[t] + bf16(lora_B[e]) @ bf16(v[t]) (+ bias[e])`` with ``h = bf16(act(gate_up[t, :K], gate_up[t, K:]))``
    from the same streaming pre-pass; ``v`` [T, r] float32 (``lora_gated_shrink(gate_up, lora_A, scale=s, ...)``),
    ``lora_B`` [E, N, r] float32."""
    _forward_only("moe_gated_forward_mxfp4_lora", gate_up, v, lora_B, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    return _mxfp4_lora_launch("moe_gated_forward_mxfp4_lora", "fql_moe_mx4_glu_lora_fwd", blocks, scales, gate_up,
                              4 * blocks.shape[-1], v, lora_B, lambda E, r: (E, blocks.shape[1], r), tokens_per_expert,
                              input_offsets, bias, out_dtype, 2 * blocks.shape[-1],
                              act=(_ACTIVATIONS[kind], act_alpha, act_limit), gated=True)


def moe_backward_input_mxfp4_lora(blocks, scales, grad_out, dv, lora_A, tokens_per_expert, input_offsets, out_dtype=None):
    """``moe_backward_input_mxfp4`` with the adapter's share fused in: ``grad_in[t] = bf16(grad_out[t]) @ W_e +
    bf16(dv[t]) @ bf16(lora_A[e])`` -> [T, K] ``out_dtype`` (default float32), rounded once.  ``dv`` [T, r] float32
    (``lora_shrink(grad_out, lora_B, "cr", scale=s)``), ``lora_A`` [E, r, K] float32.  One more contraction stage of the
    transposed kernel (csrc/fql_gemm_mx4_bwd.h); with ``lora_A`` zero the result is ``moe_backward_input_mxfp4``'s bit for
    bit, and a non-finite ``dv[t]`` makes row t NaN."""
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    return _mxfp4_lora_launch("moe_backward_input_mxfp4_lora", "fql_moe_mx4_lora_bwd_input", blocks, scales, grad_out,
                              blocks.shape[1] if blocks.dim() == 3 else -1, dv, lora_A,
                              lambda E, r: (E, r, 2 * blocks.shape[-1]), tokens_per_expert, input_offsets, None, out_dtype,
                              2 * blocks.shape[-1])


def _check_ffn_adapters(adapters, E, H, F2):
    """The four adapters of a gated FP4 FFN block: float32 [E, r, H], [E, 2F, r], [E, r, F], [E, H, r] of one rank."""
    names = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
    for name, t, shape in zip(names, adapters, ((E, H), (E, F2), (E, F2 // 2), (E, H))):
        if t.dtype != torch.float32 or t.dim() != 3:
            raise RuntimeError(f"{name} must be a float32 3-D tensor: the adapter weights and their gradients stay float32 "
                               "whatever the activations' type")
        got = (t.shape[0], t.shape[2] if name.endswith("A") else t.shape[1])
        if got != shape:
            raise RuntimeError("the adapters must be gate_up_lora_A [E, r, H], gate_up_lora_B [E, 2F, r], down_lora_A "
                               f"[E, r, F] and down_lora_B [E, H, r]; {name} is {list(t.shape)}")
    r = adapters[0].shape[1]
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    if adapters[1].shape[2] != r or adapters[2].shape[1] != r or adapters[3].shape[2] != r:
        raise RuntimeError("the gate_up and down adapters must have the same rank")


def moe_ffn_lora_forward_mxfp4(gate_up_blocks, gate_up_scales, down_blocks, down_scales, inputs, gate_up_lora_A,
                               gate_up_lora_B, down_lora_A, down_lora_B, scaling, tokens_per_expert, input_offsets,
                               activation_dtype=None, activation="silu", activation_alpha=1.702, activation_limit=7.0,
                               gate_up_bias=None, down_bias=None):
    """Gated FFN experts on MXFP4 weights with a low-rank adapter on each projection, fused into the GEMMs: for the rows t
    of expert e, ``gu = W_gu x + b_gu + B_gu v_gu`` with ``v_gu = s A_gu x``, ``h = act(gu)`` (never stored),
    ``y = W_d h + b_d + B_d v_d`` with ``v_d = s A_d h``.  ``inputs`` [T, H] float32, or bfloat16 with
    ``activation_dtype=torch.bfloat16`` (``gate_up`` is then kept in bfloat16 and ``y`` comes back in it); blocks / scales
    as ``MXFP4MoEFFN`` holds them; ``gate_up_lora_A`` [E, r, H], ``gate_up_lora_B`` [E, 2F, r], ``down_lora_A`` [E, r, F],
    ``down_lora_B`` [E, H, r] float32.  Differentiable (once) in ``inputs``, the four adapters and the two biases; the
    weights are frozen.  Every operand of a contraction is rounded once to bfloat16 and the gradient is straight-through
    across those roundings, as ``MXFP4MoEFFN(input_grad=True)``'s is.  No float32 [T, C] temporary exists with bfloat16
    activations, and nothing of shape [T, F] is saved."""
    act = activation_of(activation, activation_alpha, activation_limit)
    if activation_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError("activation_dtype must be None, torch.float32 or torch.bfloat16 (float16 rows are refused: "
                         "rounding them to bfloat16 would lose three bits)")
    dt = torch.float32 if activation_dtype is None else activation_dtype
    if inputs.dim() != 2 or inputs.dtype != dt:
        raise RuntimeError(f"inputs must be a 2-D {dt} tensor (activation_dtype), got {inputs.dtype}")
    for name, t in (("gate_up_blocks", gate_up_blocks), ("gate_up_scales", gate_up_scales), ("down_blocks", down_blocks),
                    ("down_scales", down_scales)):
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise RuntimeError(f"{name} must be a uint8 3-D tensor (MXFP4MoEFFN's buffers)")
    E, F2, H = gate_up_blocks.shape[0], gate_up_blocks.shape[1], inputs.shape[1]
    if F2 % 2 or gate_up_blocks.shape[2] * 2 != H or tuple(down_blocks.shape) != (E, H, F2 // 4):
        raise RuntimeError("gate_up_blocks must be [E, 2F, H/2] and down_blocks [E, H, F/2] for inputs [T, H]")
    _check_ffn_adapters((gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B), E, H, F2)
    if not inputs.is_cuda:
        raise RuntimeError("inputs must be a CUDA tensor (the product path has no CPU fallback)")
    adapters = (gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B)
    biases = (_check_bias(gate_up_bias, F2, inputs.device, E), _check_bias(down_bias, H, inputs.device, E))
    return _fp4_ffn_lora(_MXFP4FFNLoRAFn, _MXFP4_LORA_OPS, (gate_up_blocks, gate_up_scales), (down_blocks, down_scales), inputs,
                         adapters, biases, float(scaling), tokens_per_expert, input_offsets, act)


# The three adapter ops of a weight format by name (forward, gated forward, input gradient), looked up in this module when
# they run.  Each takes its format's weight operands first, then what the MXFP4 ops take.
_MXFP4_LORA_OPS = ("moe_forward_mxfp4_lora", "moe_gated_forward_mxfp4_lora", "moe_backward_input_mxfp4_lora")
_NVFP4_LORA_OPS = ("moe_forward_nvfp4_lora", "moe_gated_forward_nvfp4_lora", "moe_backward_input_nvfp4_lora")


def _fp4_ffn_lora(node, fmt, w_gu, w_d, inputs, adapters, biases, scaling, tpe, offs, act):
    """The gated FFN block with its adapters on the weights ``w_gu`` / ``w_d`` (tuples, the format's operands) through the
    ops ``fmt`` names: the autograd ``node`` when something wants a gradient, the plain launches otherwise."""
    if _wants_grad(inputs, *adapters, *biases):
        return node.apply(inputs, *adapters, *biases, w_gu, w_d, tpe, offs, scaling, act, fmt)
    return _fp4_ffn_lora_apply(fmt, w_gu, w_d, inputs, adapters, scaling, tpe, offs, act, biases)[0]


def _fp4_ffn_lora_apply(fmt, w_gu, w_d, inputs, adapters, scaling, tpe, offs, act, biases):
    """Returns (y, gate_up, v_gu, v_d), y and gate_up in ``inputs``' type.  Four launches and the gated pre-pass: the two
    shrinks (scale included) and the two GEMMs with their adapter stage."""
    forward, gated_forward = globals()[fmt[0]], globals()[fmt[1]]
    A_gu, B_gu, A_d, B_d = (a.detach() for a in adapters)
    b_gu, b_d = (None if b is None else b.detach() for b in biases)
    x, dt = inputs.detach(), inputs.dtype
    v_gu = lora_shrink(x, A_gu, "rc", tpe, offs, scale=scaling)
    gate_up = forward(*w_gu, x, v_gu, B_gu, tpe, offs, bias=b_gu, out_dtype=dt)
    v_d = _lora_shrink(gate_up, A_d, "rc", tpe, offs, scaling, gated=True, act=act)
    y = gated_forward(*w_d, gate_up, v_d, B_d, tpe, offs, activation=act[0], activation_alpha=act[1],
                      activation_limit=act[2], bias=b_d, out_dtype=dt)
    return y, gate_up, v_gu, v_d


class _FP4FFNLoRAFn(torch.autograd.Function):
    """The gated FP4 FFN block + its two adapters in one node, modelled on ``_MoEFFNLoRAFn`` and ``_MXFP4GatedFFNFn``.  The
    node is format-neutral: ``w_gu`` / ``w_d`` are each projection's weight operands as a tuple and ``fmt`` the table of op
    names (``_MXFP4_LORA_OPS`` or ``_NVFP4_LORA_OPS``); ``_MXFP4FFNLoRAFn`` and ``_NVFP4FFNLoRAFn`` below are this class.
    Saves inputs [T, H] and gate_up [T, 2F] in the layer's type, v_gu and v_d ([T, r] float32, the scale in them), the
    table and the parameters: nothing of shape [T, F].  Every [T, C] tensor of the backward (dh, dgu, dx) is written once,
    in the layer's type, by the kernel that forms it."""

    @staticmethod
    def forward(ctx, inputs, A_gu, B_gu, A_d, B_d, b_gu, b_d, w_gu, w_d, tpe, offs, scaling, act, fmt):
        x = inputs.contiguous()
        y, gate_up, v_gu, v_d = _fp4_ffn_lora_apply(fmt, w_gu, w_d, x, (A_gu, B_gu, A_d, B_d), scaling, tpe, offs, act,
                                                    (b_gu, b_d))
        ctx.save_for_backward(x, gate_up, v_gu, v_d, A_gu, B_gu, A_d, B_d, tpe, offs, *w_gu, *w_d)
        ctx.scaling, ctx.act, ctx.fmt, ctx.operands = scaling, act, fmt, len(w_gu)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, gate_up, v_gu, v_d, A_gu, B_gu, A_d, B_d, tpe, offs, *w = ctx.saved_tensors
        w_gu, w_d = w[:ctx.operands], w[ctx.operands:]
        backward_input = globals()[ctx.fmt[2]]
        need_x, need_Agu, need_Bgu, need_Ad, need_Bd, need_bgu, need_bd = ctx.needs_input_grad[:7]
        E, s, dt = A_gu.shape[0], ctx.scaling, gate_up.dtype
        check_activation_rows(gy, "the incoming gradient", dt)
        g = gy.contiguous()
        gx = gAgu = gBgu = gAd = gBd = gbgu = gbd = None
        if need_Bd:
            gBd = lora_grad(g, v_d, "cr", E, tpe, offs)                                  # dB_d = dY^T v_d (s is in v_d)
        if need_bd:
            gbd = moe_bias_grad(g, E, tpe, offs)                                         # db_d = sum of dY per expert
        through = need_x or need_Agu or need_Bgu or need_bgu                            # anything upstream of h
        if through or need_Ad:
            dv_d = lora_shrink(g, B_d, "cr", tpe, offs, scale=s)                         # dv_d = s dY B_d
            if need_Ad:
                gAd = _lora_grad(gate_up, dv_d, "rc", E, tpe, offs, 1.0, gated=True, act=ctx.act)   # dA_d = dv_d^T h
        if through:
            dh = backward_input(*w_d, g, dv_d, A_d, tpe, offs, out_dtype=dt)             # dh = dY W_d + dv_d A_d
            dgu = _glu_backward(gate_up, dh, dt, ctx.act)
            del dh
            if need_Bgu:
                gBgu = lora_grad(dgu, v_gu, "cr", E, tpe, offs)                          # dB_gu = dgu^T v_gu
            if need_bgu:
                gbgu = moe_bias_grad(dgu, E, tpe, offs)                                  # db_gu = sum of dgu per expert
            if need_x or need_Agu:
                dv_gu = lora_shrink(dgu, B_gu, "cr", tpe, offs, scale=s)                 # dv_gu = s dgu B_gu
                if need_x:
                    gx = backward_input(*w_gu, dgu, dv_gu, A_gu, tpe, offs, out_dtype=dt)
                if need_Agu:
                    gAgu = lora_grad(x, dv_gu, "rc", E, tpe, offs)                       # dA_gu = dv_gu^T x
        return (gx, gAgu, gBgu, gAd, gBd, gbgu, gbd) + (None,) * 7


_MXFP4FFNLoRAFn = _NVFP4FFNLoRAFn = _FP4FFNLoRAFn     # the node of either format: what differs is ``fmt`` and the weight tuples


# ---------------------------------------------------------------------------------------------------------------------
# Adapters on the NVFP4 weights (NVFP4MoEFFN, NVFP4Linear), fused into the two NVFP4 tile kernels as the MXFP4 ones are
# (csrc/fql_gemm_nvfp4.h, csrc/fql_gemm_nvfp4_bwd.h).  global_scale scales the weight term only.
# ---------------------------------------------------------------------------------------------------------------------

def moe_forward_nvfp4_lora(blocks, scales_e4m3, global_scale, inputs, v, lora_B, tokens_per_expert, input_offsets, bias=None,
                           out_dtype=None):
    """``moe_forward_nvfp4`` with a low-rank adapter fused in: for the rows t of expert e,
    ``out[t] = (W_e @ bf16(inputs[t])) * global_scale[e] + bf16(lora_B[e]) @ bf16(v[t]) (+ bias[e])``, rounded once to
    ``out_dtype``.  ``v`` [T, r] float32 are the shrunk rows with the scale in them (``lora_shrink(inputs, lora_A,
    scale=s)``), ``lora_B`` [E, N, r] float32, r in ``LORA_RANKS``.  The adapter is one more contraction stage of the tile
    kernel (csrc/fql_gemm_nvfp4.h).  ``global_scale`` multiplies the finished weight sum (one float32 rounding) BEFORE the
    adapter stage accumulates onto it, so it never touches the adapter term.  With ``lora_B`` zero the result equals
    ``moe_forward_nvfp4``'s for any ``global_scale`` and bias; the only possible difference is the sign of a zero when
    ``global_scale[e] < 0`` (the stage adds +0 to a -0).  A row's result depends on its own rows of ``inputs`` and ``v``
    and its expert's weights, ``lora_B`` and scale only.  A non-finite ``v[t]`` makes row t NaN.  Always the tile kernel
    (no decode form).  Forward only: ``moe_ffn_lora_forward_nvfp4`` is the differentiable form."""
    _forward_only("moe_forward_nvfp4_lora", inputs, v, lora_B, bias)
    return _nvfp4_launch("moe_forward_nvfp4_lora", blocks, scales_e4m3, global_scale, inputs, lambda K: K, tokens_per_expert,
                         input_offsets, bias, out_dtype, False, lora=(v, lora_B))


def moe_gated_forward_nvfp4_lora(blocks, scales_e4m3, global_scale, gate_up, v, lora_B, tokens_per_expert, input_offsets,
                                 activation="silu", activation_alpha=1.702, activation_limit=7.0, bias=None, out_dtype=None):
    """``moe_gated_forward_nvfp4`` with the adapter stage of ``moe_forward_nvfp4_lora``: the same op on
    ``h = bf16(act(gate_up[t, :K], gate_up[t, K:]))`` from the same streaming pre-pass; ``v`` [T, r] float32
    (``lora_gated_shrink(gate_up, lora_A, scale=s, ...)``), ``lora_B`` [E, N, r] float32."""
    _forward_only("moe_gated_forward_nvfp4_lora", gate_up, v, lora_B, bias)
    kind, act_alpha, act_limit = activation_of(activation, activation_alpha, activation_limit)
    return _nvfp4_launch("moe_gated_forward_nvfp4_lora", blocks, scales_e4m3, global_scale, gate_up, lambda K: 2 * K,
                         tokens_per_expert, input_offsets, bias, out_dtype, True, (_ACTIVATIONS[kind], act_alpha, act_limit),
                         lora=(v, lora_B))


def moe_backward_input_nvfp4_lora(blocks, scales_e4m3, global_scale, grad_out, dv, lora_A, tokens_per_expert, input_offsets,
                                  out_dtype=None):
    """``moe_backward_input_nvfp4`` with the adapter's share fused in: ``grad_in[t] = (bf16(grad_out[t]) @ W_e) *
    global_scale[e] + bf16(dv[t]) @ bf16(lora_A[e])`` -> [T, K] ``out_dtype`` (default float32), rounded once.  ``dv`` [T, r]
    float32 (``lora_shrink(grad_out, lora_B, "cr", scale=s)``), ``lora_A`` [E, r, K] float32.  One more contraction stage of
    the transposed kernel (csrc/fql_gemm_nvfp4_bwd.h); ``global_scale`` multiplies the weight sum in front of it.  With
    ``lora_A`` zero the result equals ``moe_backward_input_nvfp4``'s (but for the sign of a zero when ``global_scale[e] < 0``),
    and a non-finite ``dv[t]`` makes row t NaN."""
    return _nvfp4_backward_input("moe_backward_input_nvfp4_lora", blocks, scales_e4m3, global_scale, grad_out, tokens_per_expert,
                                 input_offsets, out_dtype, False, lora=(dv, lora_A))


def linear_forward_nvfp4_lora(blocks, scales_e4m3, global_scale, x, v, lora_B, bias=None, out_dtype=None):
    """``linear_forward_nvfp4`` with the adapter stage: ``out[t] = (W @ bf16(x[t])) * global_scale + bf16(lora_B) @ bf16(v[t])
    (+ bias)``; ``v`` [T, r] float32, ``lora_B`` [N, r] float32.  Exactly ``moe_forward_nvfp4_lora`` on the one-expert view
    without a table.  Forward only: ``linear_lora_forward_nvfp4`` is the differentiable form."""
    _forward_only("linear_forward_nvfp4_lora", x, v, lora_B, bias)
    return _nvfp4_launch("linear_forward_nvfp4_lora", blocks, scales_e4m3, global_scale, x, lambda K: K, None, None, bias,
                         out_dtype, False, dense=True, lora=(v, lora_B))


def linear_backward_input_nvfp4_lora(blocks, scales_e4m3, global_scale, grad_out, dv, lora_A, out_dtype=None):
    """``linear_backward_input_nvfp4`` with the adapter's share: ``grad_in[t] = (bf16(grad_out[t]) @ W) * global_scale +
    bf16(dv[t]) @ bf16(lora_A)``; ``dv`` [T, r] float32, ``lora_A`` [r, K] float32.  ``moe_backward_input_nvfp4_lora`` on the
    one-expert view without a table."""
    return _nvfp4_backward_input("linear_backward_input_nvfp4_lora", blocks, scales_e4m3, global_scale, grad_out, None, None,
                                 out_dtype, True, lora=(dv, lora_A))


def moe_ffn_lora_forward_nvfp4(gate_up_blocks, gate_up_scales, gate_up_global, down_blocks, down_scales, down_global, inputs,
                               gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B, scaling, tokens_per_expert,
                               input_offsets, activation_dtype=None, activation="silu", activation_alpha=1.702,
                               activation_limit=7.0, gate_up_bias=None, down_bias=None):
    """``moe_ffn_lora_forward_mxfp4`` on NVFP4 weights: ``gu = g_gu (W_gu x) + b_gu + B_gu v_gu`` with ``v_gu = s A_gu x``,
    ``h = act(gu)`` (never stored), ``y = g_d (W_d h) + b_d + B_d v_d`` with ``v_d = s A_d h``; blocks / scales / global
    scales as ``NVFP4MoEFFN`` holds them (``gate_up_global`` / ``down_global`` float32 [E] or None), the adapters and
    everything else as there.  Differentiable (once) in ``inputs``, the four adapters and the two biases; the weights are
    frozen and the gradient is straight-through across the bfloat16 roundings.  No float32 [T, C] temporary exists with
    bfloat16 activations, and nothing of shape [T, F] is saved."""
    act = activation_of(activation, activation_alpha, activation_limit)
    if activation_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError("activation_dtype must be None, torch.float32 or torch.bfloat16 (float16 rows are refused: "
                         "rounding them to bfloat16 would lose three bits)")
    dt = torch.float32 if activation_dtype is None else activation_dtype
    if inputs.dim() != 2 or inputs.dtype != dt:
        raise RuntimeError(f"inputs must be a 2-D {dt} tensor (activation_dtype), got {inputs.dtype}")
    for name, t in (("gate_up_blocks", gate_up_blocks), ("gate_up_scales", gate_up_scales), ("down_blocks", down_blocks),
                    ("down_scales", down_scales)):
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise RuntimeError(f"{name} must be a uint8 3-D tensor (NVFP4MoEFFN's buffers)")
    E, F2, H = gate_up_blocks.shape[0], gate_up_blocks.shape[1], inputs.shape[1]
    if F2 % 2 or gate_up_blocks.shape[2] * 2 != H or tuple(down_blocks.shape) != (E, H, F2 // 4):
        raise RuntimeError("gate_up_blocks must be [E, 2F, H/2] and down_blocks [E, H, F/2] for inputs [T, H]")
    adapters = (gate_up_lora_A, gate_up_lora_B, down_lora_A, down_lora_B)
    _check_ffn_adapters(adapters, E, H, F2)
    if not inputs.is_cuda:
        raise RuntimeError("inputs must be a CUDA tensor (the product path has no CPU fallback)")
    biases = (_check_bias(gate_up_bias, F2, inputs.device, E), _check_bias(down_bias, H, inputs.device, E))
    return _fp4_ffn_lora(_NVFP4FFNLoRAFn, _NVFP4_LORA_OPS, (gate_up_blocks, gate_up_scales, gate_up_global),
                         (down_blocks, down_scales, down_global), inputs, adapters, biases, float(scaling), tokens_per_expert,
                         input_offsets, act)


def linear_lora_forward_nvfp4(x, blocks, scales_e4m3, global_scale, lora_A, lora_B, scaling, bias=None):
    """A dense NVFP4 linear layer plus a low-rank adapter, fused: ``y = (bf16(x) @ W^T) * global_scale + bf16(v) @
    bf16(lora_B)^T (+ bias)`` with ``v = scaling * x @ lora_A^T``.  ``x`` [T, K] float32 or bfloat16, ``lora_A`` [r, K] and
    ``lora_B`` [N, r] float32; the result has ``x``'s type.  Differentiable (once) in ``x``, ``lora_A`` and ``lora_B``; the
    NVFP4 weights and the bias are frozen, and the gradient is straight-through across the bfloat16 roundings."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("ops.linear_lora_forward_nvfp4: x must be a float32 or bfloat16 [T, K] tensor (float16 is refused: "
                           "rounding it to bfloat16 would lose three bits; cast it yourself)")
    for name, t in (("lora_A", lora_A), ("lora_B", lora_B)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
            raise RuntimeError(f"{name} must be a float32 2-D tensor: lora_A [r, K] and lora_B [N, r]")
    r = lora_A.shape[0]
    if r not in LORA_RANKS:
        raise RuntimeError(f"LoRA rank must be one of {LORA_RANKS}, got {r}")
    if lora_A.shape[1] != x.shape[1] or lora_B.shape[1] != r or blocks.dim() != 2 or lora_B.shape[0] != blocks.shape[0]:
        raise RuntimeError(f"lora_A must be [r, {x.shape[1]}] and lora_B [N, r] for blocks [N, K/2]")
    if not x.is_cuda:
        raise RuntimeError("ops.linear_lora_forward_nvfp4: x must be a CUDA tensor (the adapter path has no CPU fallback)")
    if _wants_grad(x, lora_A, lora_B):
        return _NVFP4LinearLoRAFn.apply(x, lora_A, lora_B, blocks, scales_e4m3, global_scale, bias, float(scaling))
    return _nvfp4_linear_lora_apply(x, blocks, scales_e4m3, global_scale, lora_A, lora_B, float(scaling), bias)[0]


def _nvfp4_linear_lora_apply(x, blocks, scales, gs, lora_A, lora_B, scaling, bias):
    """(y, v): the shrink (scale included) and the GEMM with its adapter stage."""
    x = x.detach()
    v = lora_shrink(x, lora_A.detach(), "rc", scale=scaling)
    return linear_forward_nvfp4_lora(blocks, scales, gs, x, v, lora_B.detach(), bias=bias, out_dtype=x.dtype), v


class _NVFP4LinearLoRAFn(torch.autograd.Function):
    """Dense NVFP4 linear + adapter in one node.  Saves x (in its own type) and v = s x A^T ([T, r] float32)."""

    @staticmethod
    def forward(ctx, x, lora_A, lora_B, blocks, scales, gs, bias, scaling):
        x2 = x.contiguous()
        y, v = _nvfp4_linear_lora_apply(x2, blocks, scales, gs, lora_A, lora_B, scaling, bias)
        ctx.save_for_backward(x2, v, lora_A, lora_B, blocks, scales, gs)
        ctx.scaling = scaling
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x2, v, lora_A, lora_B, blocks, scales, gs = ctx.saved_tensors
        need_x, need_A, need_B = ctx.needs_input_grad[:3]
        check_activation_rows(gy, "the incoming gradient", x2.dtype)
        g = gy.contiguous()
        gx = gA = gB = None
        if need_B:
            gB = lora_grad(g, v, "cr")[0]                                                # dB = dY^T v (s is in v)
        if need_x or need_A:
            dv = lora_shrink(g, lora_B, "cr", scale=ctx.scaling)                         # dv = s dY B
            if need_A:
                gA = lora_grad(x2, dv, "rc")[0]                                          # dA = dv^T x
            if need_x:
                gx = linear_backward_input_nvfp4_lora(blocks, scales, gs, g, dv, lora_A, out_dtype=x2.dtype)   # dX = dY W g + dv A
        return gx, gA, gB, None, None, None, None, None
