"""Weight format: asymmetric per-row INT4 with two weights per byte.

Same public functions, argument meaning and results (bit-exact, pinned by tests/golden) as the
reference's ``python/quantize.py``:

  quantize_weights            python/quantize.py:38-124
  dequantize_weights          python/quantize.py:127-173
  reference_quantized_linear  python/quantize.py:176-202

Format: ``packed[n, j] = (q[n, 2j+1] << 4) | q[n, 2j]`` (uint8, ``[N, K/2]``),
``w[n, k] = (q[n, k] - zero_points[n]) * scales[n]`` with float32 ``scales``/``zero_points`` of
shape ``[N]``.  These run on whatever device the tensors live on; on a GPU,
``dequantize_weights`` uses the HIP kernel of the extension.

A second frozen format for the MoE experts, OCP MXFP4 (``quantize_mxfp4`` / ``dequantize_mxfp4``, pure torch): the same
byte layout with e2m1 codes in the nibbles and one E8M0 power-of-two scale byte per 32 consecutive inputs.  Activation rows
can also be OCP MXFP6 (``quantize_mxfp6`` / ``dequantize_mxfp6``): e2m3 codes, 32 of them in 24 bytes, the same scales.

A third frozen format, NVFP4 (``quantize_nvfp4`` / ``dequantize_nvfp4``, pure torch): the MXFP4 byte layout and code table
with one OCP e4m3 scale byte per 16 consecutive inputs and one float32 scale per tensor.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

__all__ = ["quantize_weights", "dequantize_weights", "reference_quantized_linear",
           "pack_nibbles", "unpack_nibbles", "quantize_mxfp4", "dequantize_mxfp4", "MXFP4_VALUES",
           "pack_mxfp6", "unpack_mxfp6", "quantize_mxfp6", "dequantize_mxfp6", "MXFP6_VALUES",
           "quantize_nvfp4", "dequantize_nvfp4", "nvfp4_scale_values", "NVFP4_BLOCK"]


def pack_nibbles(q: torch.Tensor) -> torch.Tensor:
    """[..., K] uint8 values in 0..15 -> [..., K/2] bytes, even index in the low nibble."""
    return (q[..., 1::2] << 4) | q[..., 0::2]


def unpack_nibbles(packed: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_nibbles` (python/quantize.py:152-163)."""
    if packed.is_cuda:
        from . import ops
        return ops.unpack_nibbles(packed)
    q = torch.empty(packed.shape[:-1] + (packed.shape[-1] * 2,), dtype=torch.uint8, device=packed.device)
    q[..., 0::2] = packed & 0x0F
    q[..., 1::2] = packed >> 4
    return q


def quantize_weights(weight_fp32: torch.Tensor, num_bits: int = 4, group_size: int | None = None):
    """``[N, K]`` float32 -> ``(packed [N, K/2] uint8, scales [N], zero_points [N])``.

    Per row: ``scale = (max - min) / qmax``; a constant row uses ``max(|v|, 1) / qmax``; scale is
    floored at 1e-8; ``zp = clamp(round(-min / scale), 0, qmax)``;
    ``q = clamp(round(w / scale + zp), 0, qmax)`` with round-half-to-even.

    ``group_size`` (not in the reference): the same rule applied to every run of ``group_size``
    consecutive k of a row -- ``scales`` / ``zero_points`` become ``[N, K / group_size]`` (the GPTQ / AWQ layout).
    """
    assert weight_fp32.ndim == 2, "Weight must be 2D [output_dim, input_dim]"
    assert weight_fp32.shape[1] % 2 == 0, "input_dim must be even for packing"
    if group_size is not None and group_size != weight_fp32.shape[1]:
        N, K = weight_fp32.shape
        assert group_size > 0 and group_size % 2 == 0 and K % group_size == 0, "group_size must be even and divide input_dim"
        G = K // group_size
        p, s, z = quantize_weights(weight_fp32.reshape(N * G, group_size).contiguous(), num_bits)
        return p.reshape(N, K // 2), s.reshape(N, G), z.reshape(N, G)
    if weight_fp32.is_cuda and num_bits == 4 and weight_fp32.dtype == torch.float32:
        from . import ops                       # HIP quantiser: bit-exact with the host path below
        return ops.quantize_rows(weight_fp32)
    qmax = (1 << num_bits) - 1
    lo, hi = torch.aminmax(weight_fp32, dim=1)
    span_scale = (hi - lo) / qmax
    flat_scale = hi.abs().clamp(min=1.0) / qmax                 # rows whose values are all equal
    scales = torch.where(hi == lo, flat_scale, span_scale).clamp(min=1e-8)
    zero_points = torch.round(-lo / scales).clamp(0, qmax)
    q = torch.round(weight_fp32 / scales[:, None] + zero_points[:, None]).clamp(0, qmax).to(torch.uint8)
    return pack_nibbles(q), scales, zero_points


def dequantize_weights(packed_uint8: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor):
    """``[N, K/2]`` packed bytes -> ``[N, K]`` float32: ``(q - zp) * scale``; ``scales`` / ``zero_points`` ``[N]``
    (per row, the reference's format) or ``[N, K / group_size]`` (per group along K)."""
    if scales.dim() == 2:                                   # per-group: the per-row rule on [N * G, group_size]
        N, G = scales.shape
        K = packed_uint8.shape[1] * 2
        w = dequantize_weights(packed_uint8.reshape(N * G, K // G // 2).contiguous(), scales.reshape(-1).contiguous(),
                               zero_points.reshape(-1).contiguous())
        return w.reshape(N, K)
    if packed_uint8.is_cuda:
        from . import ops
        return ops.dequantize_forward(packed_uint8, scales, zero_points)
    q = unpack_nibbles(packed_uint8).to(torch.float32)
    return (q - zero_points.unsqueeze(1)) * scales.unsqueeze(1)


def reference_quantized_linear(input: torch.Tensor, packed_weights: torch.Tensor,
                               scales: torch.Tensor, zero_points: torch.Tensor):
    """Un-fused formulation: materialise the float32 weights, then ``F.linear``.

    Part of the reference's public API (python/__init__.py:14-22).  It is what a CPU tensor gets
    from ``QuantizedLinear.forward`` (python/module.py:113-118); GPU tensors never come here --
    they go to the fused HIP kernels via :mod:`ops`.
    """
    return F.linear(input, dequantize_weights(packed_weights, scales, zero_points))


# ---- OCP MXFP4: e2m1 elements, two to a byte (even k in the low nibble), one E8M0 scale byte per 32 consecutive inputs

MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)
MXFP4_BLOCK = 32


def quantize_mxfp4(weight: torch.Tensor):
    """``[..., N, K]`` (K % 32 == 0) -> ``(blocks uint8 [..., N, K/2], scales uint8 [..., N, K/32])`` by the OCP MX rule:
    per block of 32 consecutive inputs ``shared = floor(log2(amax)) - 2`` (2 = e2m1's largest exponent), clamped to
    [-127, 127], scale code ``shared + 127``; the elements are ``x / 2^shared`` rounded to nearest even on the e2m1 grid
    and saturated to +-6, the sign kept (a negative value that rounds to zero is code 8).  An all-zero block gets scale
    code 127 and zero elements.  A non-finite weight raises ``ValueError``."""
    if weight.dim() < 2 or weight.shape[-1] % MXFP4_BLOCK != 0:
        raise ValueError("weight must be [..., N, K] with K % 32 == 0")
    if not bool(torch.isfinite(weight).all()):
        raise ValueError("quantize_mxfp4: the weights must be finite")
    K = weight.shape[-1]
    x = weight.detach().to(torch.float64).reshape(*weight.shape[:-1], K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = x.abs().amax(dim=-1, keepdim=True)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    shared = torch.where(amax == 0, torch.zeros_like(ex), ex - 1 - 2).clamp(-127, 127)
    v = torch.ldexp(x.abs(), -shared)                           # exact in float64
    q = torch.where(v < 2, torch.round(v * 2) / 2, torch.where(v < 4, torch.round(v), torch.round(v / 2) * 2)).clamp(max=6.0)
    mag = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4)).to(torch.uint8)
    codes = (mag | (torch.signbit(x).to(torch.uint8) << 3)).reshape(*weight.shape[:-1], K)
    scales = (shared + 127).to(torch.uint8).reshape(*weight.shape[:-1], K // MXFP4_BLOCK)
    return pack_nibbles(codes), scales


def mxfp4_scale_values(scales: torch.Tensor) -> torch.Tensor:
    """E8M0 codes (uint8) -> float32: ``2^(s - 127)`` for 0 .. 254 (code 0 is the float32 subnormal 2^-127), NaN for 255."""
    s = scales.to(torch.int32)
    bits = torch.where(s == 0, torch.full_like(s, 0x00400000), s << 23)
    bits = torch.where(s == 255, torch.full_like(s, 0x7FC00000), bits)
    return bits.view(torch.float32)


def dequantize_mxfp4(blocks: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``(blocks [..., N, K/2], scales [..., N, K/32])`` uint8 -> ``[..., N, K]`` float32: the 16-entry table times the
    block's scale.  Exact, up to float32's own range (scale code 254 with |code| >= 2 is infinite)."""
    if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError("blocks and scales must be uint8")
    K = blocks.shape[-1] * 2
    if K % MXFP4_BLOCK != 0 or tuple(scales.shape) != tuple(blocks.shape[:-1]) + (K // MXFP4_BLOCK,):
        raise ValueError("blocks must be [..., N, K/2] and scales [..., N, K/32]")
    codes = torch.stack([blocks & 0x0F, blocks >> 4], dim=-1).reshape(*blocks.shape[:-1], K)
    table = torch.tensor(MXFP4_VALUES, dtype=torch.float32, device=blocks.device)
    w = table[codes.long()].reshape(*blocks.shape[:-1], K // MXFP4_BLOCK, MXFP4_BLOCK)
    return (w * mxfp4_scale_values(scales).unsqueeze(-1)).reshape(*blocks.shape[:-1], K)


# ---- NVFP4: e2m1 elements in the MXFP4 byte layout, one OCP e4m3fn scale byte per 16 consecutive inputs, one float32
#      scale per tensor (ModelOpt's weight / weight_scale / weight_scale_2)

NVFP4_BLOCK = 16
_E2M1_MAX, _E4M3_MAX = 6.0, 448.0


def nvfp4_scale_values(scales: torch.Tensor) -> torch.Tensor:
    """e4m3fn bytes (uint8) -> float32, by the definition: sign, four exponent bits of bias 7, three mantissa bits;
    exponent field 0 is the subnormal ``m * 2^-9``; 0x7F and 0xFF are NaN; the largest value is 448."""
    if scales.dtype != torch.uint8:
        raise ValueError("scales must be uint8")
    s = scales.to(torch.int32)
    ex, m = (s >> 3) & 15, (s & 7).to(torch.float32)
    mag = torch.where(ex == 0, m * 2.0 ** -9, torch.ldexp(1.0 + m / 8.0, ex - 7))
    v = torch.where((s & 0x80) != 0, -mag, mag)
    return torch.where((s & 0x7F) == 0x7F, torch.full_like(v, float("nan")), v)


def _leading_scale(global_scale, lead, device):
    """``global_scale`` (None: 1) as a float32 tensor that broadcasts over ``[*lead, N, blocks, 16]``."""
    if global_scale is None:
        return torch.ones((), dtype=torch.float32, device=device)
    g = torch.as_tensor(global_scale, dtype=torch.float32, device=device)
    want = 1
    for d in lead:
        want *= d
    if g.numel() != want:
        raise ValueError(f"global_scale must hold one value per leading matrix ({want}), got {list(g.shape)}")
    return g.reshape(*lead, 1, 1, 1)


def quantize_nvfp4(weight: torch.Tensor, global_scale=None):
    """``[..., N, K]`` (K % 16 == 0) -> ``(blocks uint8 [..., N, K/2], scales uint8 [..., N, K/16], global_scale float32)``
    by ModelOpt's rule.  ``global_scale`` has one value per leading matrix (``[E]`` for ``[E, N, K]``, ``[1]`` for
    ``[N, K]``); when not given it is ``amax(|W|) / (6 * 448)`` of each matrix, and 1 for an all-zero one.  The block scale
    is ``block_amax / (6 * global_scale)`` in float32, clamped to 448 and then rounded to e4m3fn to nearest even (a cast of
    a value above 464 would give NaN: the clamp comes first).  The codes are ``w / (scale * global_scale)``, ``scale`` the
    rounded one, rounded to e2m1 by ``quantize_mxfp4``'s element rule; a zero block scale gives zero codes.
    ``global_scale`` multiplies, as ModelOpt's ``weight_scale_2`` does; compressed-tensors checkpoints store its
    reciprocal (``weight_global_scale``): invert it before handing it to this library."""
    if weight.dim() < 2 or weight.shape[-1] % NVFP4_BLOCK != 0:
        raise ValueError("weight must be [..., N, K] with K % 16 == 0")
    if not bool(torch.isfinite(weight).all()):
        raise ValueError("quantize_nvfp4: the weights must be finite")
    lead, K = tuple(weight.shape[:-2]), weight.shape[-1]
    w = weight.detach().to(torch.float32)
    if global_scale is None:
        amax = w.abs().amax(dim=(-2, -1)) if w.numel() else torch.zeros(lead)
        gs = torch.where(amax == 0, torch.ones_like(amax), amax / (_E2M1_MAX * _E4M3_MAX)).to(torch.float32)
    else:
        gs = torch.as_tensor(global_scale, dtype=torch.float32, device=w.device).reshape(lead)
        if not bool((torch.isfinite(gs) & (gs > 0)).all()):
            raise ValueError("quantize_nvfp4: global_scale must be finite and positive")
    x = w.reshape(*weight.shape[:-1], K // NVFP4_BLOCK, NVFP4_BLOCK)
    g = gs.reshape(*lead, 1, 1, 1)
    block_scale = (x.abs().amax(dim=-1, keepdim=True) / (_E2M1_MAX * g)).clamp(max=_E4M3_MAX)
    scales = block_scale.to(torch.float8_e4m3fn).view(torch.uint8)
    dq = nvfp4_scale_values(scales).to(torch.float64) * g.to(torch.float64)          # what a code is multiplied by
    v = torch.where(dq == 0, torch.zeros_like(dq), x.abs().to(torch.float64) / torch.where(dq == 0, torch.ones_like(dq), dq))
    q = torch.where(v < 2, torch.round(v * 2) / 2, torch.where(v < 4, torch.round(v), torch.round(v / 2) * 2)).clamp(max=6.0)
    mag = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4)).to(torch.uint8)
    sign = torch.where(dq == 0, torch.zeros_like(mag), torch.signbit(x).to(torch.uint8) << 3)
    codes = (mag | sign).reshape(*weight.shape[:-1], K)
    return pack_nibbles(codes), scales.reshape(*weight.shape[:-1], K // NVFP4_BLOCK), gs.reshape(-1) if lead else gs.reshape(1)


def dequantize_nvfp4(blocks: torch.Tensor, scales: torch.Tensor, global_scale=None) -> torch.Tensor:
    """``(blocks [..., N, K/2], scales [..., N, K/16])`` uint8 -> ``[..., N, K]`` float32: the 16-entry e2m1 table times
    the block's e4m3 scale (exact: at most six significant bits), then times ``global_scale`` (one value per leading
    matrix; None: 1, nothing more is rounded)."""
    if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError("blocks and scales must be uint8")
    K = blocks.shape[-1] * 2
    if blocks.dim() < 2 or K % NVFP4_BLOCK != 0 or tuple(scales.shape) != tuple(blocks.shape[:-1]) + (K // NVFP4_BLOCK,):
        raise ValueError("blocks must be [..., N, K/2] and scales [..., N, K/16]")
    codes = torch.stack([blocks & 0x0F, blocks >> 4], dim=-1).reshape(*blocks.shape[:-1], K)
    table = torch.tensor(MXFP4_VALUES, dtype=torch.float32, device=blocks.device)
    w = table[codes.long()].reshape(*blocks.shape[:-1], K // NVFP4_BLOCK, NVFP4_BLOCK) * nvfp4_scale_values(scales).unsqueeze(-1)
    if global_scale is not None:
        w = w * _leading_scale(global_scale, tuple(blocks.shape[:-2]), blocks.device)
    return w.reshape(*blocks.shape[:-1], K)


# ---- OCP MXFP6 (e2m3) rows: 32 six-bit codes in 24 bytes, one E8M0 scale byte per 32 consecutive inputs

# code = sign << 5 | exponent << 3 | mantissa, bias 1: subnormals m / 8, largest value 7.5, no inf or NaN
MXFP6_VALUES = tuple((-1.0 if c & 32 else 1.0) * ((c & 7) / 8 if (c >> 3) & 3 == 0 else (1 + (c & 7) / 8) * 2.0 ** (((c >> 3) & 3) - 1))
                     for c in range(64))


def pack_mxfp6(codes: torch.Tensor) -> torch.Tensor:
    """[..., K] uint8 codes in 0..63 (K % 32 == 0) -> [..., 3K/4] bytes: element i of block b is bits 6 i .. 6 i + 5 of the
    24 bytes at 24 b read as one little-endian integer.  Four codes fill three bytes."""
    if codes.dtype != torch.uint8 or codes.shape[-1] % MXFP4_BLOCK != 0:
        raise ValueError("codes must be uint8 [..., K] with K % 32 == 0")
    c = codes.reshape(*codes.shape[:-1], -1, 4).to(torch.int32)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = torch.stack([word & 255, (word >> 8) & 255, word >> 16], dim=-1).to(torch.uint8)
    return out.reshape(*codes.shape[:-1], codes.shape[-1] // 4 * 3)


def unpack_mxfp6(packed: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_mxfp6`: [..., 3K/4] bytes -> [..., K] uint8 codes."""
    if packed.dtype != torch.uint8 or packed.shape[-1] % 24 != 0:
        raise ValueError("packed must be uint8 [..., 3K/4] with K % 32 == 0")
    b = packed.reshape(*packed.shape[:-1], -1, 3).to(torch.int32)
    word = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    out = torch.stack([word & 63, (word >> 6) & 63, (word >> 12) & 63, word >> 18], dim=-1).to(torch.uint8)
    return out.reshape(*packed.shape[:-1], packed.shape[-1] // 3 * 4)


def quantize_mxfp6(x: torch.Tensor):
    """``[..., T, K]`` (K % 32 == 0) -> ``(codes uint8 [..., T, 3K/4], scales uint8 [..., T, K/32])`` by the OCP MX rule with
    e2m3 elements: per block of 32 consecutive inputs ``shared = floor(log2(amax)) - 2`` (2 = e2m3's largest exponent),
    clamped to [-127, 127], scale code ``shared + 127``; the elements are ``x / 2^shared`` rounded to nearest even on the
    e2m3 grid (steps of 1/8 below 2, 1/4 below 4, 1/2 above) and saturated to +-7.5, the sign kept (a negative value that
    rounds to zero is code 32).  An all-zero block gets scale code 127 and zero elements.  A non-finite input raises
    ``ValueError``.  Computed in float64."""
    if x.dim() < 2 or x.shape[-1] % MXFP4_BLOCK != 0:
        raise ValueError("x must be [..., T, K] with K % 32 == 0")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("quantize_mxfp6: the values must be finite")
    K = x.shape[-1]
    v64 = x.detach().to(torch.float64).reshape(*x.shape[:-1], K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = v64.abs().amax(dim=-1, keepdim=True)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    shared = torch.where(amax == 0, torch.zeros_like(ex), ex - 1 - 2).clamp(-127, 127)
    v = torch.ldexp(v64.abs(), -shared)                         # exact in float64
    q = torch.where(v < 2, torch.round(v * 8) / 8, torch.where(v < 4, torch.round(v * 4) / 4, torch.round(v * 2) / 2)).clamp(max=7.5)
    mag = torch.where(q < 2, q * 8, torch.where(q < 4, q * 4 + 8, q * 2 + 16)).to(torch.uint8)
    codes = (mag | (torch.signbit(v64).to(torch.uint8) << 5)).reshape(*x.shape[:-1], K)
    scales = (shared + 127).to(torch.uint8).reshape(*x.shape[:-1], K // MXFP4_BLOCK)
    return pack_mxfp6(codes), scales


def dequantize_mxfp6(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``(codes [..., T, 3K/4], scales [..., T, K/32])`` uint8 -> ``[..., T, K]`` float32: the 64-entry table times the
    block's scale.  Exact, up to float32's own range."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError("codes and scales must be uint8")
    if codes.shape[-1] % 24 != 0 or tuple(scales.shape) != tuple(codes.shape[:-1]) + (codes.shape[-1] // 24,):
        raise ValueError("codes must be [..., T, 3K/4] and scales [..., T, K/32]")
    K = codes.shape[-1] // 3 * 4
    table = torch.tensor(MXFP6_VALUES, dtype=torch.float32, device=codes.device)
    w = table[unpack_mxfp6(codes).long()].reshape(*codes.shape[:-1], K // MXFP4_BLOCK, MXFP4_BLOCK)
    return (w * mxfp4_scale_values(scales).unsqueeze(-1)).reshape(*codes.shape[:-1], K)
