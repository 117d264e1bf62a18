"""MoE modules over the grouped INT4 GEMM.

``MoEINT4`` / ``quantize_weights_moe``  -- surface of the reference's python/moe_int4_module.py:19-146
    (stacked ``[E, N, K/2]`` buffers, per-TENSOR scale / zero-point broadcast to ``[E, N]``,
    ``forward(inputs, expert_ids, tokens_per_expert, input_offsets)`` over rows pre-grouped by expert).
``QuantizedMoEExpert`` / ``QuantizedMoE`` -- surface of benchmark/moe_grouped_gemm/moe_int4_module.py:21-130
    (per-expert per-ROW quantisation, ``forward(List[Tensor]) -> List[Tensor]``).

Both run ONE fused launch sequence for all experts on the GPU (device-side offsets, no per-expert
launches or host syncs).  The reference's ``moe_int4_cuda`` kernel is defective; the
semantics implemented are the ones its wrapper documents and ``QuantizedMoE.forward`` computes.
"""
from __future__ import annotations

import math
from typing import List

import torch
import torch.nn as nn

from .quantize import quantize_weights, dequantize_weights, pack_nibbles

try:  # mirrors the reference's module-level availability flag (python/moe_int4_module.py:10-16)
    from . import _native
    _native.lib()
    CUDA_AVAILABLE = True
except Exception:  # library not built: MoEINT4.forward raises, as the reference does
    CUDA_AVAILABLE = False


def quantize_weights_moe(weights_list):
    """List of ``[N, K]`` (fp16/fp32) -> stacked ``(packed [E,N,K/2], scales [E,N], zero_points [E,N])``.

    Per expert, over the WHOLE tensor: ``scale = (max - min) / 15``, ``zp = clamp(round(-min/scale), 0, 15)``,
    ``q = clamp(round(w/scale + zp), 0, 15)`` (python/moe_int4_module.py:45-59).  As in the reference
    there is no guard for a constant tensor.
    """
    E = len(weights_list)
    N, K = weights_list[0].shape
    device = weights_list[0].device
    packed = torch.zeros(E, N, K // 2, dtype=torch.uint8, device=device)
    scales = torch.zeros(E, N, dtype=torch.float32, device=device)
    zero_points = torch.zeros(E, N, dtype=torch.float32, device=device)
    for e, w in enumerate(weights_list):
        w32 = w.float()
        if w32.is_cuda:                             # HIP quantiser: bit-exact with the host arithmetic below
            from . import ops
            packed[e], scales[e], zero_points[e] = ops.quantize_tensor(w32)
            continue
        lo, hi = torch.aminmax(w32)
        scale = ((hi - lo) / 15.0).item()
        zp = float(max(0, min(15, round((-lo / scale).item()))))
        scales[e] = scale
        zero_points[e] = zp
        q = torch.round(w32 / scale + zp).clamp(0, 15).to(torch.uint8)
        packed[e] = pack_nibbles(q)                 # one vectorised pack instead of a K/2-step loop
    return packed, scales, zero_points


class MoEINT4(nn.Module):
    def __init__(self, num_experts, hidden_dim, ffn_dim, precision: str = "default"):
        super().__init__()
        self.num_experts = num_experts
        self.hidden_dim = hidden_dim
        self.ffn_dim = ffn_dim
        self.packed_dim = hidden_dim // 2
        self.precision = precision
        self.register_buffer("packed_weights",
                             torch.zeros(num_experts, ffn_dim, self.packed_dim, dtype=torch.uint8))
        self.register_buffer("scales", torch.zeros(num_experts, ffn_dim, dtype=torch.float32))
        self.register_buffer("zero_points", torch.zeros(num_experts, ffn_dim, dtype=torch.float32))

    @classmethod
    def from_weights(cls, weights_list, precision: str = "default"):
        module = cls(len(weights_list), weights_list[0].shape[1], weights_list[0].shape[0], precision=precision)
        packed, scales, zero_points = quantize_weights_moe(weights_list)
        module.packed_weights = packed
        module.scales = scales
        module.zero_points = zero_points
        return module

    def forward(self, inputs, expert_ids, tokens_per_expert, input_offsets):
        """inputs ``[T, K]`` float32 with rows grouped by expert -> ``[T, N]`` float32."""
        if not CUDA_AVAILABLE:
            raise RuntimeError("CUDA kernel not available")
        from . import ops
        return ops.moe_forward(self.packed_weights, self.scales, self.zero_points, inputs, expert_ids,
                               tokens_per_expert, input_offsets, precision=self.precision)


class QuantizedMoEExpert(nn.Module):
    def __init__(self, in_features: int, out_features: int, precision: str = "default"):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.precision = precision
        self.register_buffer("packed_weights", torch.zeros(out_features, in_features // 2, dtype=torch.uint8))
        self.register_buffer("scales", torch.zeros(out_features, dtype=torch.float32))
        self.register_buffer("zero_points", torch.zeros(out_features, dtype=torch.float32))

    @classmethod
    def from_fp16(cls, weight: torch.Tensor, precision: str = "default") -> "QuantizedMoEExpert":
        assert weight.shape[1] % 2 == 0, "in_features must be even for INT4 packing"
        expert = cls(weight.shape[1], weight.shape[0], precision=precision)
        packed, scales, zero_points = quantize_weights(weight.float())
        expert.packed_weights = packed
        expert.scales = scales
        expert.zero_points = zero_points
        return expert

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape[0] == 0:      # reference quirk: always float16 (moe_int4_module.py:65-68)
            return torch.empty(0, self.out_features, device=x.device, dtype=torch.float16)
        if x.is_cuda:
            from . import ops
            return ops.linear_forward_any(x.contiguous(), self.packed_weights, self.scales, self.zero_points,
                                          precision=self.precision)          # in x's dtype (:70-72)
        w = dequantize_weights(self.packed_weights, self.scales, self.zero_points)
        return x @ w.T.to(x.dtype)

    @property
    def weight_memory_bytes(self) -> int:
        return self.packed_weights.numel() + 4 * self.scales.numel() + 4 * self.zero_points.numel()


class QuantizedMoE(nn.Module):
    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, precision: str = "default"):
        super().__init__()
        self.num_experts = num_experts
        self.hidden_dim = hidden_dim
        self.ffn_dim = ffn_dim
        self.precision = precision
        self.experts = nn.ModuleList([QuantizedMoEExpert(hidden_dim, ffn_dim, precision)
                                      for _ in range(num_experts)])
        self._stacked = None        # lazily built [E,N,K/2] view of the experts' buffers for the grouped launch

    @classmethod
    def from_fp16_weights(cls, weights: List[torch.Tensor], precision: str = "default") -> "QuantizedMoE":
        assert len(weights) > 0
        moe = cls(len(weights), weights[0].shape[1], weights[0].shape[0], precision=precision)
        for i, w in enumerate(weights):
            moe.experts[i] = QuantizedMoEExpert.from_fp16(w, precision=precision)
        return moe

    def _stack(self, device):
        """The experts' buffers as ONE [E, N, K/2] / [E, N] / [E, N] set for the grouped launch -- without a second copy of
        the weights: the stacked tensors become the storage and every expert's registered buffers are re-bound to views
        of them (state_dict keys, shapes and in-place loads are unchanged; ``.to()`` / a replaced expert break the
        views, which the next call detects by address and repairs).  Only when the module lives on another device than
        the inputs is a side copy kept, as before."""
        names = ("packed_weights", "scales", "zero_points")
        st = self._stacked
        if st is not None and st[0].device == device:
            views = all(getattr(e, n).data_ptr() == st[k][i].data_ptr() for i, e in enumerate(self.experts) for k, n in enumerate(names))
            if views:                                            # the experts' buffers ARE the stacked storage
                return st[:3]
            key = tuple((getattr(e, n).data_ptr(), getattr(e, n)._version) for e in self.experts for n in names)
            if st[3] == key:                                     # side copy of a module on another device, still current
                return st[:3]
        on_device = all(getattr(e, n).device == device for e in self.experts for n in names)
        stacked = tuple(torch.stack([getattr(e, n) for e in self.experts]).to(device) for n in names)
        key = None
        if on_device:
            for i, e in enumerate(self.experts):
                for k, n in enumerate(names):
                    e._buffers[n] = stacked[k][i]               # a view: the per-expert copy is released
        else:
            key = tuple((getattr(e, n).data_ptr(), getattr(e, n)._version) for e in self.experts for n in names)
        self._stacked = stacked + (key,)
        return stacked

    def forward(self, expert_inputs: List[torch.Tensor]) -> List[torch.Tensor]:
        """One tensor ``[m_e, K]`` per expert in, one ``[m_e, N]`` per expert out (in x's dtype;
        empty inputs give an empty float16 tensor, as the reference does)."""
        if len(expert_inputs) == 0 or not expert_inputs[0].is_cuda:
            return [expert(x) for expert, x in zip(self.experts, expert_inputs)]
        from . import ops
        dev = expert_inputs[0].device
        counts = [int(x.shape[0]) for x in expert_inputs]
        packed, scales, zps = self._stack(dev)
        dtypes = {x.dtype for x in expert_inputs}
        common = dtypes.pop() if len(dtypes) == 1 else torch.float32      # mixed dtypes: compute once in float32
        if common not in (torch.float32, torch.float16, torch.bfloat16):
            common = torch.float32
        grouped = torch.cat([x.to(common) for x in expert_inputs], dim=0).contiguous()
        tpe = torch.tensor(counts, dtype=torch.int32)
        offs = torch.cumsum(tpe, 0, dtype=torch.int32) - tpe
        out = ops.moe_forward_any(packed, scales, zps, grouped, None, tpe.to(dev, non_blocking=True),
                                  offs.to(dev, non_blocking=True), precision=self.precision) \
            if grouped.shape[0] else grouped.new_zeros((0, self.ffn_dim))
        outs, o = [], 0
        for x, c in zip(expert_inputs, counts):
            if c == 0:
                outs.append(torch.empty(0, self.ffn_dim, device=x.device, dtype=torch.float16))
            else:
                outs.append(out[o:o + c].to(x.dtype))
            o += c
        return outs

    @property
    def total_memory_bytes(self) -> int:
        return sum(e.weight_memory_bytes for e in self.experts)


class QuantizedMoEFFN(nn.Module):
    """Full gated FFN experts in INT4: ``down( silu(gate(x)) * up(x) )`` per expert, rows
    pre-grouped by expert.  The reference models only the up projection ("just the up projection for
    simplicity", benchmark/moe_grouped_gemm/config.py:50-52); this is the step either side of it in a
    Mixtral / DeepSeek block, built from the same kernels:

      * gate and up are ONE grouped GEMM over the stacked ``[E, 2F, H]`` weights (one pass over x),
      * silu(gate) * up is fused into the down GEMM's activation pre-pass (``fql_moe_gated_fwd_f32``),
        so the ``[T, F]`` hidden activation never exists in memory.

    Weights are quantised per output row with ``quantize_weights`` (per-row scale / zero point, as
    ``QuantizedMoEExpert.from_fp16`` does).

    ``activation_dtype`` (None / torch.float32: the float32 layer, unchanged) = torch.float16 / torch.bfloat16 runs the
    layer on 16-bit activations: inputs and the incoming gradient have that type, ``gate_up`` is written (and kept for
    the backward) in it, and the output and the input gradient come back in it.  That rounds ``gate_up`` between the two
    projections, which the float32 layer does not do: a memory-for-precision choice, so it is opt-in.

    ``activation`` chooses the function between the two projections: ``"silu"`` (SwiGLU, the default), ``"gelu_tanh"``
    (GeGLU, tanh form; Hugging Face's ``"gelu_pytorch_tanh"`` is accepted) or ``"swiglu_clamp"`` (gpt-oss:
    ``min(g, limit) * sigmoid(alpha * min(g, limit)) * (clamp(u, -limit, limit) + 1)`` with ``activation_alpha`` and
    ``activation_limit``).  It is configuration, not state: the state-dict keys and values are the same for every kind
    (INTEGRATION.md section 13).

    ``expert_bias=True`` (gpt-oss) adds a bias to both projections, ``gate_up = W_gu x + b_gu`` and ``y = W_d h + b_d``,
    each added in its GEMM's epilogue (on 16-bit activations before the one rounding): float32 ``nn.Parameter``s
    ``gate_up_bias`` [E, 2F] and ``down_bias`` [E, H], zeros with ``requires_grad=False`` -- a loaded checkpoint is frozen
    like the weights, ``requires_grad_(True)`` trains them (their gradient is ``ops.moe_bias_grad``, computed only
    then).  Rows no expert covers stay zero.  A layer built without it has the state-dict keys it always had
    (INTEGRATION.md section 14).

    ``group_size`` (None: per output row) quantises both projections per group of that many consecutive inputs, the
    layout of GPTQ / AWQ-style checkpoints (``quantize_weights(group_size=)``): the scale and zero-point buffers keep their
    names and become ``[E, 2F, H / group_size]`` and ``[E, H, F / group_size]``.  One value serves both projections; it
    must be even and divide ``hidden_dim`` and ``ffn_dim``.  A value that gives one group (``hidden_dim == ffn_dim ==
    group_size``) is the per-row layer.  Forward and backward run the per-group kernels;
    ``precision="fp8"`` is not available with it."""

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, precision: str = "default",
                 activation_dtype=None, activation: str = "silu", activation_alpha: float = 1.702,
                 activation_limit: float = 7.0, expert_bias: bool = False, group_size=None):
        super().__init__()
        assert hidden_dim % 32 == 0 and ffn_dim % 32 == 0, "hidden_dim and ffn_dim must be multiples of 32"
        self.num_experts, self.hidden_dim, self.ffn_dim, self.precision = num_experts, hidden_dim, ffn_dim, precision
        self.activation_dtype = _activation_dtype(activation_dtype, precision)
        from . import ops
        self.activation, self.activation_alpha, self.activation_limit = ops.activation_of(
            activation, activation_alpha, activation_limit)
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.group_size = gs = _group_size(group_size, H, F)
        if gs is not None and precision in ("fp8", 8):
            raise ValueError("precision='fp8' is not available with group_size")
        groups_gu, groups_d = ((), ()) if gs is None else ((H // gs,), (F // gs,))
        self.register_buffer("gate_up_packed", torch.zeros(E, 2 * F, H // 2, dtype=torch.uint8))
        self.register_buffer("gate_up_scales", torch.zeros(E, 2 * F, *groups_gu, dtype=torch.float32))
        self.register_buffer("gate_up_zero_points", torch.zeros(E, 2 * F, *groups_gu, dtype=torch.float32))
        self.register_buffer("down_packed", torch.zeros(E, H, F // 2, dtype=torch.uint8))
        self.register_buffer("down_scales", torch.zeros(E, H, *groups_d, dtype=torch.float32))
        self.register_buffer("down_zero_points", torch.zeros(E, H, *groups_d, dtype=torch.float32))
        self.expert_bias = bool(expert_bias)
        if self.expert_bias:                 # (no attribute at all otherwise: the state-dict keys stay those of before)
            self.gate_up_bias = nn.Parameter(torch.zeros(E, 2 * F, dtype=torch.float32), requires_grad=False)
            self.down_bias = nn.Parameter(torch.zeros(E, H, dtype=torch.float32), requires_grad=False)

    @classmethod
    def from_weights(cls, gate: List[torch.Tensor], up: List[torch.Tensor], down: List[torch.Tensor],
                     precision: str = "default", activation_dtype=None, activation: str = "silu",
                     activation_alpha: float = 1.702, activation_limit: float = 7.0, gate_bias=None, up_bias=None,
                     down_bias=None, group_size=None) -> "QuantizedMoEFFN":
        """``gate[e]``, ``up[e]``: ``[F, H]``; ``down[e]``: ``[H, F]`` (nn.Linear weight layout).  ``gate_bias[e]``,
        ``up_bias[e]``: ``[F]``; ``down_bias[e]``: ``[H]``: the per-expert biases, all three or none (then the layer has
        no bias parameters).  ``group_size``: quantise per group along the inputs (``quantize_weights(group_size=)``)."""
        E = len(gate)
        F, H = gate[0].shape
        given = [b is not None for b in (gate_bias, up_bias, down_bias)]
        if any(given) and not all(given):
            raise ValueError("gate_bias, up_bias and down_bias come together: pass all three or none")
        if all(given):
            for name, b, n in (("gate_bias", gate_bias, F), ("up_bias", up_bias, F), ("down_bias", down_bias, H)):
                if len(b) != E or any(tuple(t.shape) != (n,) for t in b):
                    raise ValueError(f"{name} must be a list of num_experts tensors of shape [{n}]")
        m = cls(E, H, F, precision, activation_dtype=activation_dtype, activation=activation,
                activation_alpha=activation_alpha, activation_limit=activation_limit, expert_bias=all(given),
                group_size=group_size)
        if all(given):
            dev = gate[0].device
            with torch.no_grad():
                m.gate_up_bias.data = torch.stack([torch.cat([g.float(), u.float()]) for g, u in zip(gate_bias, up_bias)]).to(dev)
                m.down_bias.data = torch.stack([d.float() for d in down_bias]).to(dev)
        gs = m.group_size                    # (a projection with one group comes back per row: the buffer's shape holds)
        gu = [quantize_weights(torch.cat([g.float(), u.float()], dim=0), group_size=gs) for g, u in zip(gate, up)]
        dn = [quantize_weights(d.float(), group_size=gs) for d in down]
        m.gate_up_packed = torch.stack([t[0] for t in gu])
        m.gate_up_scales = torch.stack([t[1] for t in gu]).reshape(m.gate_up_scales.shape)
        m.gate_up_zero_points = torch.stack([t[2] for t in gu]).reshape(m.gate_up_zero_points.shape)
        m.down_packed = torch.stack([t[0] for t in dn])
        m.down_scales = torch.stack([t[1] for t in dn]).reshape(m.down_scales.shape)
        m.down_zero_points = torch.stack([t[2] for t in dn]).reshape(m.down_zero_points.shape)
        return m

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 rows grouped by expert -> ``[T, H]`` float32 (``activation_dtype``: both in
        that type)."""
        if not inputs.is_cuda:
            raise RuntimeError("QuantizedMoEFFN runs on the GPU (the product path has no CPU fallback)")
        if self.activation_dtype is not None:
            from . import ops
            ops.check_activation_rows(inputs, "inputs", self.activation_dtype)
        b_gu, b_d = self.biases
        if torch.is_grad_enabled() and (inputs.requires_grad or (self.expert_bias and (b_gu.requires_grad
                                                                                      or b_d.requires_grad))):
            fn = _GatedFFNFn if self.activation_dtype is None else _GatedFFN16Fn
            return fn.apply(inputs, tokens_per_expert, input_offsets, self, b_gu, b_d)
        return _gated_ffn(self, inputs, tokens_per_expert, input_offsets)[0]

    @property
    def biases(self):
        """``(gate_up_bias, down_bias)``, or ``(None, None)`` for a layer built without ``expert_bias``."""
        return (self.gate_up_bias, self.down_bias) if self.expert_bias else (None, None)

    @property
    def total_memory_bytes(self) -> int:
        return (sum(b.numel() * b.element_size() for b in self.buffers())
                + sum(b.numel() * b.element_size() for b in self.biases if b is not None))

    @property
    def activation_args(self):
        """``(activation, activation_alpha, activation_limit)`` as the ops take them."""
        return self.activation, self.activation_alpha, self.activation_limit

    def _activation_repr(self) -> str:
        bias = ", expert_bias=True" if self.expert_bias else ""
        if self.group_size is not None:
            bias += f", group_size={self.group_size}"
        if self.activation == "silu":
            return bias
        s = f", activation={self.activation}"
        if self.activation == "swiglu_clamp":
            s += f", activation_alpha={self.activation_alpha:g}, activation_limit={self.activation_limit:g}"
        return s + bias

    def extra_repr(self) -> str:
        return self._activation_repr().lstrip(", ")


def _group_size(group_size, hidden_dim, ffn_dim):
    """The ``group_size`` argument of the gated FFN layers: None (per row), or an even divisor of both dimensions; the one
    value that gives a single group in both projections is per row too."""
    if group_size is None:
        return None
    if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size <= 0 or group_size % 2 != 0 \
            or hidden_dim % group_size != 0 or ffn_dim % group_size != 0:
        raise ValueError(f"group_size must be even and divide hidden_dim ({hidden_dim}) and ffn_dim ({ffn_dim}), got "
                         f"{group_size!r}")
    return None if group_size == hidden_dim == ffn_dim else group_size


def _activation_dtype(activation_dtype, precision):
    from . import ops
    dt = ops.activation_dtype_of(activation_dtype)
    if dt is not None and precision in ("fp8", 8):
        raise ValueError("precision='fp8' has no gated forward and no backward: it cannot be combined with a 16-bit "
                         "activation_dtype")
    return dt


def _gated_ffn(m, inputs, tpe, offs):
    """(y, gate_up) in the layer's activation type: the gate|up GEMM, then the down GEMM with silu(gate) * up fused into
    its pre-pass.  On 16-bit activations each GEMM reads its operand as it is and rounds its result once."""
    from . import ops
    dt = m.activation_dtype
    b_gu, b_d = m.biases                                    # (detached: a bias gradient is the autograd node's business)
    bias_gu = {} if b_gu is None else {"bias": b_gu.detach()}
    bias_d = {} if b_d is None else {"bias": b_d.detach()}
    if dt is None:                                          # the float32 layer takes float32 rows only
        gate_up = ops.moe_forward(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, inputs, None, tpe, offs,
                                  precision=m.precision, **bias_gu)
    else:
        gate_up = ops.moe_forward_any(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, inputs, None, tpe,
                                      offs, precision=m.precision, out_dtype=dt, **bias_gu)
    return ops.moe_gated_forward(m.down_packed, m.down_scales, m.down_zero_points, gate_up, tpe, offs,
                                 precision=m.precision, out_dtype=dt, activation=m.activation,
                                 activation_alpha=m.activation_alpha, activation_limit=m.activation_limit,
                                 **bias_d), gate_up


class _GatedFFNFn(torch.autograd.Function):
    """``QuantizedMoEFFN`` with the input gradient.  Keeps the ``gate_up`` tensor the forward materialises anyway; the
    backward is ``dh`` on the down weights, ``dg = dh * u * silu'(g)`` and ``du = dh * silu(g)`` (torch elementwise),
    then ``dx`` on the gate / up weights -- both GEMMs the fused kernel of csrc/fql_bwd.h.  ``b_gu`` / ``b_d`` are the
    layer's biases (None without ``expert_bias``): the forward reads them from ``m``, they are inputs so that autograd can
    ask for their gradients, ``ops.moe_bias_grad`` of dgu and of gy, launched only for a bias that requires grad."""

    @staticmethod
    def forward(ctx, inputs, tokens_per_expert, input_offsets, m, b_gu=None, b_d=None):
        out, gate_up = _gated_ffn(m, inputs, tokens_per_expert, input_offsets)
        ctx.save_for_backward(gate_up, tokens_per_expert, input_offsets)
        ctx.m = m
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import ops
        gate_up, tpe, offs = ctx.saved_tensors
        m = ctx.m
        K = gate_up.shape[1] // 2
        need_x, need_bgu, need_bd = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        gy = gy.to(torch.float32)
        gbd = ops.moe_bias_grad(gy, m.num_experts, tpe, offs) if need_bd else None
        if not (need_x or need_bgu):
            return None, None, None, None, None, gbd
        dh = ops.moe_backward_input(m.down_packed, m.down_scales, m.down_zero_points, gy, tpe, offs,
                                    precision=m.precision)
        if m.activation == "silu":
            g, u = gate_up[:, :K], gate_up[:, K:]
            sig = torch.sigmoid(g)
            dgu = torch.cat([dh * u * (sig * (1.0 + g * (1.0 - sig))), dh * (g * sig)], dim=1)
        else:                                                   # the other kinds: one streaming kernel
            dgu = ops.glu_backward(gate_up, dh, *m.activation_args)
        gbgu = ops.moe_bias_grad(dgu, m.num_experts, tpe, offs) if need_bgu else None
        dx = ops.moe_backward_input(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, dgu, tpe, offs,
                                    precision=m.precision) if need_x else None
        return dx, None, None, None, gbgu, gbd


class _GatedFFN16Fn(_GatedFFNFn):
    """``_GatedFFNFn`` on 16-bit activations (the same forward): keeps ``gate_up`` in the 16-bit type; the backward is
    ``dh`` on the down weights, ``ops.swiglu_backward`` and ``dx`` on the gate / up weights, each tensor written once in
    that type."""

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import ops
        gate_up, tpe, offs = ctx.saved_tensors
        m = ctx.m
        dt = m.activation_dtype
        ops.check_activation_rows(gy, "the incoming gradient", dt)
        need_x, need_bgu, need_bd = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        gbd = ops.moe_bias_grad(gy, m.num_experts, tpe, offs) if need_bd else None
        if not (need_x or need_bgu):
            return None, None, None, None, None, gbd
        dh = ops.moe_backward_input(m.down_packed, m.down_scales, m.down_zero_points, gy, tpe, offs,
                                    precision=m.precision, out_dtype=dt)
        dgu = ops.glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
        gbgu = ops.moe_bias_grad(dgu, m.num_experts, tpe, offs) if need_bgu else None
        dx = ops.moe_backward_input(m.gate_up_packed, m.gate_up_scales, m.gate_up_zero_points, dgu, tpe, offs,
                                    precision=m.precision, out_dtype=dt) if need_x else None
        return dx, None, None, None, gbgu, gbd


class _MXFP4GatedFFNFn(torch.autograd.Function):
    """``MXFP4MoEFFN(input_grad=True)`` with the input gradient, modelled on ``_GatedFFN16Fn``.  Keeps ``gate_up`` in the
    layer's type (float32 or bfloat16); the backward is ``dh`` on the down weights (``ops.moe_backward_input_mxfp4``),
    ``ops.glu_backward`` for every activation kind and ``dx`` on the gate / up weights, each tensor written once in that
    type.  ``b_gu`` / ``b_d`` are inputs so that autograd can ask for their gradients: ``ops.moe_bias_grad`` of dgu and of
    gy, launched only for a bias that requires grad."""

    @staticmethod
    def forward(ctx, inputs, tokens_per_expert, input_offsets, m, b_gu=None, b_d=None):
        out, gate_up = m._ffn(inputs, tokens_per_expert, input_offsets)
        ctx.save_for_backward(gate_up, tokens_per_expert, input_offsets)
        ctx.m = m
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import ops
        gate_up, tpe, offs = ctx.saved_tensors
        m = ctx.m
        dt = gate_up.dtype
        ops.check_activation_rows(gy, "the incoming gradient", dt)
        need_x, need_bgu, need_bd = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        gbd = ops.moe_bias_grad(gy, m.num_experts, tpe, offs) if need_bd else None
        if not (need_x or need_bgu):
            return None, None, None, None, None, gbd
        dh = ops.moe_backward_input_mxfp4(m.down_blocks, m.down_scales, gy, tpe, offs, out_dtype=dt)
        dgu = ops.glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
        gbgu = ops.moe_bias_grad(dgu, m.num_experts, tpe, offs) if need_bgu else None
        dx = ops.moe_backward_input_mxfp4(m.gate_up_blocks, m.gate_up_scales, dgu, tpe, offs, out_dtype=dt) \
            if need_x else None
        return dx, None, None, None, gbgu, gbd


class MXFP4MoEFFN(nn.Module):
    """Gated FFN experts on OCP MXFP4 weights (the format gpt-oss ships its experts in), frozen:
    ``down( act(gate(x), up(x)) )`` per expert, rows pre-grouped by expert, the same ``forward`` as ``QuantizedMoEFFN``.

    The weights are uint8 buffers in the checkpoint's own encoding, never re-quantised: ``gate_up_blocks`` [E, 2F, H/2] and
    ``down_blocks`` [E, H, F/2] hold two e2m1 codes a byte (even input in the low nibble), ``gate_up_scales`` [E, 2F, H/32]
    and ``down_scales`` [E, H, F/32] one E8M0 power-of-two scale per 32 consecutive inputs.  Rows 0 .. F-1 of ``gate_up``
    are the gate, F .. 2F-1 the up projection (``from_mxfp4(interleaved=True)`` converts gpt-oss's alternating order).
    ``expert_bias=True`` adds float32 ``gate_up_bias`` [E, 2F] and ``down_bias`` [E, H], as in ``QuantizedMoEFFN``.

    Both GEMMs are ``ops.moe_forward_mxfp4`` / ``ops.moe_gated_forward_mxfp4``: the weights are exact in bfloat16, the
    activations are rounded once to bfloat16 (float32 inputs) or read as they are (bfloat16), the sums are float32.
    ``activation_dtype=torch.bfloat16`` takes bfloat16 inputs, keeps ``gate_up`` in bfloat16 and returns bfloat16; the
    default takes float32 and keeps ``gate_up`` in float32.  A small batch (few routed rows: decode) takes the library's
    decode kernel for both GEMMs instead of the 64-row tile; it returns the same bits, so nothing else changes.  That
    holds in every ``precision``: ``"fp8"`` and ``"fp4"`` have a decode kernel of their own behind their pre-pass, each
    with a threshold set from a measurement.

    ``input_grad=False`` (the default) is inference only: a forward under grad mode on an input that requires grad raises
    ``RuntimeError``, and ``QuantizedSparseMoEBlock(experts=MXFP4MoEFFN(...))`` works under ``torch.no_grad()``.
    ``input_grad=True`` makes the layer differentiable in its input and, for biases that ``requires_grad``, in its biases
    (the weights stay frozen): under grad mode the forward (the same kernels, the same bits) keeps ``gate_up`` and the
    backward is ``dh = ops.moe_backward_input_mxfp4`` on the down weights, ``ops.glu_backward``, then ``dx`` on the gate /
    up weights, every tensor in the layer's activation type.  The gradient is straight-through across the forward's two
    bfloat16 roundings, of ``x`` and of ``h``: it is the gradient of the function without them, evaluated at the
    forward's values, and the backward rounds its own operands (``gy``, ``dgu``) once to bfloat16 in the same way.  The
    keyword is configuration, not state: the state-dict keys do not change.

    ``precision="fp8"`` (default ``"bf16"``) runs both GEMMs on the block-scaled FP4 matrix cores instead: the rows (``x``,
    then the float32 ``h``) are quantised per row to OCP e4m3 by a fused pre-pass and contracted with the packed weights
    and their E8M0 scales as they lie in the checkpoint (``ops.moe_forward_mxfp4(..., precision="fp8")``).  The mode is
    inference only: it has no backward, so ``input_grad=True`` with it raises ``ValueError``.  Configuration as well: the
    state-dict keys do not change.

    ``precision="fp4"`` (W4A4) quantises the rows to MXFP4 as well, per block of 32 by ``quantize.quantize_mxfp4``'s rule
    (``ops.quantize_rows_mxfp4``), and contracts e2m1 with e2m1: half the activation traffic of the fp8 mode again, at the
    format's price (about 1.1e-1 relative on the rows against 3e-2 for e4m3).  Inference only and configuration, as fp8.

    ``precision="fp6"`` quantises the rows to MXFP6 instead (e2m3 elements, per block of 32 by ``quantize.quantize_mxfp6``'s
    rule, ``ops.quantize_rows_mxfp6``) and contracts e2m1 with e2m3 at the matrix rate of the fp4 mode: three quarters of the
    fp8 mode's row bytes at about its error (2.8e-2 relative on Gaussian rows).  Inference only and configuration, as fp8."""

    group_size = None                        # (what the block reads: the scale blocks are the format's, not an option)

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, activation: str = "silu",
                 activation_alpha: float = 1.702, activation_limit: float = 7.0, expert_bias: bool = False,
                 activation_dtype=None, input_grad: bool = False, precision: str = "bf16"):
        super().__init__()
        if precision not in ("bf16", "fp8", "fp6", "fp4"):
            raise ValueError(f"precision must be 'bf16', 'fp8', 'fp6' or 'fp4', got {precision!r}")
        if precision != "bf16" and input_grad:
            raise ValueError(f"precision='{precision}' has no backward: it cannot be combined with input_grad=True")
        if hidden_dim % 32 != 0 or ffn_dim % 32 != 0 or hidden_dim <= 0 or ffn_dim <= 0:
            raise ValueError("hidden_dim and ffn_dim must be positive multiples of 32 (one scale per 32 inputs)")
        if activation_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("activation_dtype must be None, torch.float32 or torch.bfloat16 (float16 rows are refused: "
                             "rounding them to bfloat16 would lose three bits)")
        from . import ops
        self.num_experts, self.hidden_dim, self.ffn_dim = num_experts, hidden_dim, ffn_dim
        self.activation, self.activation_alpha, self.activation_limit = ops.activation_of(
            activation, activation_alpha, activation_limit)
        self.activation_dtype = None if activation_dtype == torch.float32 else activation_dtype
        self.input_grad = bool(input_grad)
        self.precision = precision
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.register_buffer("gate_up_blocks", torch.zeros(E, 2 * F, H // 2, dtype=torch.uint8))
        self.register_buffer("gate_up_scales", torch.full((E, 2 * F, H // 32), 127, dtype=torch.uint8))
        self.register_buffer("down_blocks", torch.zeros(E, H, F // 2, dtype=torch.uint8))
        self.register_buffer("down_scales", torch.full((E, H, F // 32), 127, dtype=torch.uint8))
        self.expert_bias = bool(expert_bias)
        if self.expert_bias:
            self.gate_up_bias = nn.Parameter(torch.zeros(E, 2 * F, dtype=torch.float32), requires_grad=False)
            self.down_bias = nn.Parameter(torch.zeros(E, H, dtype=torch.float32), requires_grad=False)

    @classmethod
    def from_mxfp4(cls, gate_up_blocks, gate_up_scales, down_blocks, down_scales, gate_up_bias=None, down_bias=None,
                   interleaved: bool = False, **kwargs) -> "MXFP4MoEFFN":
        """Tensors already in the format: ``gate_up_blocks`` [E, 2F, H/2] (or [E, 2F, H/32, 16], the checkpoint's block
        dimension, flattened here), ``gate_up_scales`` [E, 2F, H/32], ``down_blocks`` [E, H, F/2] (or [E, H, F/32, 16]),
        ``down_scales`` [E, H, F/32], all uint8; ``gate_up_bias`` [E, 2F] and ``down_bias`` [E, H] (both or none).
        ``interleaved=True``: rows 0, 2, 4, ... of ``gate_up`` are the gate and 1, 3, 5, ... the up projection (gpt-oss's
        order); they are de-interleaved once, the bias included.  ``kwargs``: the constructor's activation arguments,
        ``activation_dtype``, ``input_grad`` and ``precision``."""
        def flat(name, b, s):
            if b.dtype != torch.uint8 or s.dtype != torch.uint8:
                raise ValueError(f"{name}_blocks and {name}_scales must be uint8")
            if b.dim() == 4 and b.shape[-1] == 16:
                b = b.reshape(b.shape[0], b.shape[1], -1)
            if b.dim() != 3 or s.dim() != 3 or tuple(s.shape) != (b.shape[0], b.shape[1], b.shape[2] // 16) or b.shape[2] % 16:
                raise ValueError(f"{name}_blocks must be [E, N, K/2] (or [E, N, K/32, 16]) and {name}_scales [E, N, K/32]")
            return b, s
        gub, gus = flat("gate_up", gate_up_blocks, gate_up_scales)
        db, ds = flat("down", down_blocks, down_scales)
        E, F2, H = gub.shape[0], gub.shape[1], gub.shape[2] * 2
        if F2 % 2 or tuple(db.shape) != (E, H, F2 // 4):
            raise ValueError("gate_up must be [E, 2F, H/2] and down [E, H, F/2] of the same E, H and F")
        if (gate_up_bias is None) != (down_bias is None):
            raise ValueError("gate_up_bias and down_bias come together: pass both or none")
        if gate_up_bias is not None and (tuple(gate_up_bias.shape) != (E, F2) or tuple(down_bias.shape) != (E, H)):
            raise ValueError("gate_up_bias must be [E, 2F] and down_bias [E, H]")
        if interleaved:
            split = lambda t: torch.cat([t[:, 0::2], t[:, 1::2]], dim=1)
            gub, gus = split(gub), split(gus)
            gate_up_bias = None if gate_up_bias is None else split(gate_up_bias)
        m = cls(E, H, F2 // 2, expert_bias=gate_up_bias is not None, **kwargs)
        m.gate_up_blocks, m.gate_up_scales = gub.contiguous().clone(), gus.contiguous().clone()
        m.down_blocks, m.down_scales = db.contiguous().clone(), ds.contiguous().clone()
        if gate_up_bias is not None:
            with torch.no_grad():
                m.gate_up_bias.data = gate_up_bias.detach().float().contiguous().clone()
                m.down_bias.data = down_bias.detach().float().contiguous().clone()
        return m

    @classmethod
    def from_weights(cls, gate: List[torch.Tensor], up: List[torch.Tensor], down: List[torch.Tensor], gate_bias=None,
                     up_bias=None, down_bias=None, **kwargs) -> "MXFP4MoEFFN":
        """``gate[e]``, ``up[e]``: ``[F, H]``; ``down[e]``: ``[H, F]`` float weights, quantised with
        ``quantize.quantize_mxfp4``; the biases as ``QuantizedMoEFFN.from_weights`` takes them (all three or none)."""
        from .quantize import quantize_mxfp4
        given = [b is not None for b in (gate_bias, up_bias, down_bias)]
        if any(given) and not all(given):
            raise ValueError("gate_bias, up_bias and down_bias come together: pass all three or none")
        gub, gus = quantize_mxfp4(torch.stack([torch.cat([g.float(), u.float()], dim=0) for g, u in zip(gate, up)]))
        db, ds = quantize_mxfp4(torch.stack([d.float() for d in down]))
        b_gu = torch.stack([torch.cat([g.float(), u.float()]) for g, u in zip(gate_bias, up_bias)]) if all(given) else None
        b_d = torch.stack([d.float() for d in down_bias]) if all(given) else None
        return cls.from_mxfp4(gub, gus, db, ds, gate_up_bias=b_gu, down_bias=b_d, **kwargs)

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 (``activation_dtype=torch.bfloat16``: bfloat16) rows grouped by expert -> ``[T, H]`` of
        the same type."""
        if not inputs.is_cuda:
            raise RuntimeError("MXFP4MoEFFN runs on the GPU (the product path has no CPU fallback)")
        if not self.input_grad and torch.is_grad_enabled() and inputs.requires_grad:
            raise RuntimeError("MXFP4MoEFFN is inference-only: the MXFP4 format has no backward.  Run it under "
                               "torch.no_grad(), or on a detached input (or build the layer with input_grad=True)")
        dt = torch.float32 if self.activation_dtype is None else self.activation_dtype
        if inputs.dim() != 2 or inputs.dtype != dt:
            raise RuntimeError(f"MXFP4MoEFFN: inputs must be a 2-D {dt} tensor (the layer's activation_dtype), got "
                               f"{inputs.dtype}")
        b_gu, b_d = self.biases
        if self.input_grad and torch.is_grad_enabled() and (
                inputs.requires_grad or (b_gu is not None and (b_gu.requires_grad or b_d.requires_grad))):
            return _MXFP4GatedFFNFn.apply(inputs, tokens_per_expert, input_offsets, self, b_gu, b_d)
        return self._ffn(inputs, tokens_per_expert, input_offsets)[0]

    def _ffn(self, inputs, tokens_per_expert, input_offsets):
        """(y, gate_up) in the layer's activation type, on detached biases (their gradient is the autograd node's
        business)."""
        from . import ops
        dt = torch.float32 if self.activation_dtype is None else self.activation_dtype
        b_gu, b_d = self.biases
        b_gu, b_d = (None, None) if b_gu is None else (b_gu.detach(), b_d.detach())
        gate_up = ops.moe_forward_mxfp4(self.gate_up_blocks, self.gate_up_scales, inputs.detach(), tokens_per_expert,
                                        input_offsets, bias=b_gu, out_dtype=dt, precision=self.precision)
        return ops.moe_gated_forward_mxfp4(self.down_blocks, self.down_scales, gate_up, tokens_per_expert, input_offsets,
                                           activation=self.activation, activation_alpha=self.activation_alpha,
                                           activation_limit=self.activation_limit, bias=b_d, out_dtype=dt,
                                           precision=self.precision), gate_up

    @property
    def biases(self):
        """``(gate_up_bias, down_bias)``, or ``(None, None)`` for a layer built without ``expert_bias``."""
        return (self.gate_up_bias, self.down_bias) if self.expert_bias else (None, None)

    @property
    def total_memory_bytes(self) -> int:
        return (sum(b.numel() * b.element_size() for b in self.buffers())
                + sum(b.numel() * b.element_size() for b in self.biases if b is not None))

    @property
    def activation_args(self):
        """``(activation, activation_alpha, activation_limit)`` as the ops take them."""
        return self.activation, self.activation_alpha, self.activation_limit

    _activation_repr = QuantizedMoEFFN._activation_repr

    def extra_repr(self) -> str:
        return ("format=mxfp4" + self._activation_repr() + (", input_grad=True" if self.input_grad else "")
                + (f", precision={self.precision}" if self.precision != "bf16" else ""))


class _NVFP4GatedFFNFn(torch.autograd.Function):
    """``NVFP4MoEFFN(input_grad=True)`` with the input gradient, modelled on ``_MXFP4GatedFFNFn``: ``dh`` on the down weights
    (``ops.moe_backward_input_nvfp4``), ``ops.glu_backward`` for every activation kind and ``dx`` on the gate / up weights,
    each tensor written once in the layer's activation type; ``ops.moe_bias_grad`` only for a bias that requires grad."""

    @staticmethod
    def forward(ctx, inputs, tokens_per_expert, input_offsets, m, b_gu=None, b_d=None):
        out, gate_up = m._ffn(inputs, tokens_per_expert, input_offsets)
        ctx.save_for_backward(gate_up, tokens_per_expert, input_offsets)
        ctx.m = m
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from . import ops
        gate_up, tpe, offs = ctx.saved_tensors
        m = ctx.m
        dt = gate_up.dtype
        ops.check_activation_rows(gy, "the incoming gradient", dt)
        need_x, need_bgu, need_bd = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        gbd = ops.moe_bias_grad(gy, m.num_experts, tpe, offs) if need_bd else None
        if not (need_x or need_bgu):
            return None, None, None, None, None, gbd
        dh = ops.moe_backward_input_nvfp4(m.down_blocks, m.down_scales, m.down_global, gy, tpe, offs, out_dtype=dt)
        dgu = ops.glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
        gbgu = ops.moe_bias_grad(dgu, m.num_experts, tpe, offs) if need_bgu else None
        dx = ops.moe_backward_input_nvfp4(m.gate_up_blocks, m.gate_up_scales, m.gate_up_global, dgu, tpe, offs,
                                          out_dtype=dt) if need_x else None
        return dx, None, None, None, gbgu, gbd


class NVFP4MoEFFN(nn.Module):
    """Gated FFN experts on NVFP4 weights (the format of ModelOpt's ``-FP4`` / ``-NVFP4`` exports), frozen:
    ``down( act(gate(x), up(x)) )`` per expert, rows pre-grouped by expert, the same ``forward`` as ``MXFP4MoEFFN``.

    The buffers are the checkpoint's tensors, never re-quantised: ``gate_up_blocks`` uint8 [E, 2F, H/2] and ``down_blocks``
    [E, H, F/2] hold two e2m1 codes a byte (even input in the low nibble), ``gate_up_scales`` [E, 2F, H/16] and
    ``down_scales`` [E, H, F/16] one e4m3fn scale byte per 16 consecutive inputs, ``gate_up_global`` and ``down_global``
    float32 [E] the per-tensor scales.  The global scales MULTIPLY (ModelOpt's ``weight_scale_2``); compressed-tensors
    stores the reciprocal (``weight_global_scale``): invert it before ``from_nvfp4``.  Rows 0 .. F-1 of ``gate_up`` are the
    gate, F .. 2F-1 the up projection (``from_nvfp4(interleaved=True)`` converts an alternating order).
    ``expert_bias=True`` adds float32 ``gate_up_bias`` [E, 2F] and ``down_bias`` [E, H], as in ``MXFP4MoEFFN``.

    Both GEMMs are ``ops.moe_forward_nvfp4`` / ``ops.moe_gated_forward_nvfp4``: the weights are exact in bfloat16, the
    activations are rounded once to bfloat16 (float32 inputs) or read as they are (``activation_dtype=torch.bfloat16``),
    the sums are float32, and a small batch takes the decode kernel with the same bits.

    ``input_grad=False`` (the default) is inference only: a forward under grad mode on an input that requires grad raises
    ``RuntimeError``, as ``MXFP4MoEFFN(input_grad=False)`` does.  ``input_grad=True`` makes the layer differentiable in its
    input and, for biases that ``requires_grad``, in its biases (the weights stay frozen): under grad mode the forward (the
    same kernels, the same bits) keeps ``gate_up`` and the backward is ``dh = ops.moe_backward_input_nvfp4`` on the down
    weights, ``ops.glu_backward``, then ``dx`` on the gate / up weights, every tensor in the layer's activation type.  The
    gradient is straight-through across the forward's two bfloat16 roundings, as ``MXFP4MoEFFN``'s is.  The keyword is
    configuration, not state: the state-dict keys do not change."""

    group_size = None                        # (what the block reads: the scale blocks are the format's, not an option)
    precision = "bf16"

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, activation: str = "silu",
                 activation_alpha: float = 1.702, activation_limit: float = 7.0, expert_bias: bool = False,
                 activation_dtype=None, input_grad: bool = False):
        super().__init__()
        if hidden_dim % 32 != 0 or ffn_dim % 32 != 0 or hidden_dim <= 0 or ffn_dim <= 0 or num_experts <= 0:
            raise ValueError("hidden_dim and ffn_dim must be positive multiples of 32 and num_experts positive")
        if activation_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("activation_dtype must be None, torch.float32 or torch.bfloat16 (float16 rows are refused: "
                             "rounding them to bfloat16 would lose three bits)")
        from . import ops
        self.num_experts, self.hidden_dim, self.ffn_dim = num_experts, hidden_dim, ffn_dim
        self.activation, self.activation_alpha, self.activation_limit = ops.activation_of(
            activation, activation_alpha, activation_limit)
        self.activation_dtype = None if activation_dtype == torch.float32 else activation_dtype
        self.input_grad = bool(input_grad)
        E, H, F = num_experts, hidden_dim, ffn_dim
        self.register_buffer("gate_up_blocks", torch.zeros(E, 2 * F, H // 2, dtype=torch.uint8))
        self.register_buffer("gate_up_scales", torch.full((E, 2 * F, H // 16), 0x38, dtype=torch.uint8))
        self.register_buffer("gate_up_global", torch.ones(E, dtype=torch.float32))
        self.register_buffer("down_blocks", torch.zeros(E, H, F // 2, dtype=torch.uint8))
        self.register_buffer("down_scales", torch.full((E, H, F // 16), 0x38, dtype=torch.uint8))
        self.register_buffer("down_global", torch.ones(E, dtype=torch.float32))
        self.expert_bias = bool(expert_bias)
        if self.expert_bias:
            self.gate_up_bias = nn.Parameter(torch.zeros(E, 2 * F, dtype=torch.float32), requires_grad=False)
            self.down_bias = nn.Parameter(torch.zeros(E, H, dtype=torch.float32), requires_grad=False)

    @classmethod
    def from_nvfp4(cls, gate_up_blocks, gate_up_scales, gate_up_global, down_blocks, down_scales, down_global,
                   gate_up_bias=None, down_bias=None, interleaved: bool = False, **kwargs) -> "NVFP4MoEFFN":
        """Tensors already in the format: ``gate_up_blocks`` [E, 2F, H/2], ``gate_up_scales`` [E, 2F, H/16] and
        ``down_blocks`` [E, H, F/2], ``down_scales`` [E, H, F/16], all uint8 (a ``float8_e4m3fn`` scale tensor is viewed
        as its bytes); ``gate_up_global`` / ``down_global`` float32 [E], or None for ones; ``gate_up_bias`` [E, 2F] and
        ``down_bias`` [E, H] (both or none).  ``interleaved=True``: rows 0, 2, 4, ... of ``gate_up`` are the gate and
        1, 3, 5, ... the up projection; they are de-interleaved once, the bias included.  ``kwargs``: the constructor's
        activation arguments, ``activation_dtype`` and ``input_grad``."""
        def check(name, b, s, g):
            if s.dtype == torch.float8_e4m3fn:
                s = s.view(torch.uint8)
            if b.dtype != torch.uint8 or s.dtype != torch.uint8:
                raise ValueError(f"{name}_blocks and {name}_scales must be uint8")
            if b.dim() != 3 or s.dim() != 3 or b.shape[2] % 16 or tuple(s.shape) != (b.shape[0], b.shape[1], b.shape[2] // 8):
                raise ValueError(f"{name}_blocks must be [E, N, K/2] with K % 32 == 0 and {name}_scales [E, N, K/16]")
            if g is None:
                g = torch.ones(b.shape[0], dtype=torch.float32, device=b.device)
            if not isinstance(g, torch.Tensor) or g.numel() != b.shape[0]:
                raise ValueError(f"{name}_global must hold one float32 value per expert")
            return b, s, g.detach().to(torch.float32).reshape(-1)
        gub, gus, gug = check("gate_up", gate_up_blocks, gate_up_scales, gate_up_global)
        db, ds, dg = check("down", down_blocks, down_scales, down_global)
        E, F2, H = gub.shape[0], gub.shape[1], gub.shape[2] * 2
        if F2 % 2 or tuple(db.shape) != (E, H, F2 // 4):
            raise ValueError("gate_up must be [E, 2F, H/2] and down [E, H, F/2] of the same E, H and F")
        if (gate_up_bias is None) != (down_bias is None):
            raise ValueError("gate_up_bias and down_bias come together: pass both or none")
        if gate_up_bias is not None and (tuple(gate_up_bias.shape) != (E, F2) or tuple(down_bias.shape) != (E, H)):
            raise ValueError("gate_up_bias must be [E, 2F] and down_bias [E, H]")
        if interleaved:
            split = lambda t: torch.cat([t[:, 0::2], t[:, 1::2]], dim=1)
            gub, gus = split(gub), split(gus)
            gate_up_bias = None if gate_up_bias is None else split(gate_up_bias)
        m = cls(E, H, F2 // 2, expert_bias=gate_up_bias is not None, **kwargs)
        m.gate_up_blocks, m.gate_up_scales, m.gate_up_global = gub.contiguous().clone(), gus.contiguous().clone(), gug.clone()
        m.down_blocks, m.down_scales, m.down_global = db.contiguous().clone(), ds.contiguous().clone(), dg.clone()
        if gate_up_bias is not None:
            with torch.no_grad():
                m.gate_up_bias.data = gate_up_bias.detach().float().contiguous().clone()
                m.down_bias.data = down_bias.detach().float().contiguous().clone()
        return m

    @classmethod
    def from_weights(cls, gate: List[torch.Tensor], up: List[torch.Tensor], down: List[torch.Tensor], gate_bias=None,
                     up_bias=None, down_bias=None, **kwargs) -> "NVFP4MoEFFN":
        """``gate[e]``, ``up[e]``: ``[F, H]``; ``down[e]``: ``[H, F]`` float weights, quantised with
        ``quantize.quantize_nvfp4`` (one global scale per expert and projection); the biases as
        ``QuantizedMoEFFN.from_weights`` takes them (all three or none)."""
        from .quantize import quantize_nvfp4
        given = [b is not None for b in (gate_bias, up_bias, down_bias)]
        if any(given) and not all(given):
            raise ValueError("gate_bias, up_bias and down_bias come together: pass all three or none")
        gu = quantize_nvfp4(torch.stack([torch.cat([g.float(), u.float()], dim=0) for g, u in zip(gate, up)]))
        d = quantize_nvfp4(torch.stack([t.float() for t in down]))
        b_gu = torch.stack([torch.cat([g.float(), u.float()]) for g, u in zip(gate_bias, up_bias)]) if all(given) else None
        b_d = torch.stack([t.float() for t in down_bias]) if all(given) else None
        return cls.from_nvfp4(*gu, *d, gate_up_bias=b_gu, down_bias=b_d, **kwargs)

    def forward(self, inputs, tokens_per_expert, input_offsets):
        """inputs ``[T, H]`` float32 (``activation_dtype=torch.bfloat16``: bfloat16) rows grouped by expert -> ``[T, H]`` of
        the same type."""
        if not inputs.is_cuda:
            raise RuntimeError("NVFP4MoEFFN runs on the GPU (the product path has no CPU fallback)")
        if not self.input_grad and torch.is_grad_enabled() and inputs.requires_grad:
            raise RuntimeError("NVFP4MoEFFN is inference-only: the NVFP4 format has no backward.  Run it under "
                               "torch.no_grad(), or on a detached input (or build the layer with input_grad=True)")
        dt = torch.float32 if self.activation_dtype is None else self.activation_dtype
        if inputs.dim() != 2 or inputs.dtype != dt:
            raise RuntimeError(f"NVFP4MoEFFN: inputs must be a 2-D {dt} tensor (the layer's activation_dtype), got "
                               f"{inputs.dtype}")
        b_gu, b_d = self.biases
        if self.input_grad and torch.is_grad_enabled() and (
                inputs.requires_grad or (b_gu is not None and (b_gu.requires_grad or b_d.requires_grad))):
            return _NVFP4GatedFFNFn.apply(inputs, tokens_per_expert, input_offsets, self, b_gu, b_d)
        return self._ffn(inputs, tokens_per_expert, input_offsets)[0]

    def _ffn(self, inputs, tokens_per_expert, input_offsets):
        """(y, gate_up) in the layer's activation type, on detached biases (their gradient is the autograd node's
        business)."""
        from . import ops
        dt = torch.float32 if self.activation_dtype is None else self.activation_dtype
        b_gu, b_d = self.biases
        b_gu, b_d = (None, None) if b_gu is None else (b_gu.detach(), b_d.detach())
        gate_up = ops.moe_forward_nvfp4(self.gate_up_blocks, self.gate_up_scales, self.gate_up_global, inputs.detach(),
                                        tokens_per_expert, input_offsets, bias=b_gu, out_dtype=dt)
        return ops.moe_gated_forward_nvfp4(self.down_blocks, self.down_scales, self.down_global, gate_up, tokens_per_expert,
                                           input_offsets, activation=self.activation, activation_alpha=self.activation_alpha,
                                           activation_limit=self.activation_limit, bias=b_d, out_dtype=dt), gate_up

    biases = MXFP4MoEFFN.biases
    total_memory_bytes = MXFP4MoEFFN.total_memory_bytes
    activation_args = MXFP4MoEFFN.activation_args
    _activation_repr = QuantizedMoEFFN._activation_repr

    def extra_repr(self) -> str:
        return "format=nvfp4" + self._activation_repr() + (", input_grad=True" if self.input_grad else "")


class QuantizedSparseMoEBlock(nn.Module):
    """A Mixtral-style sparse MoE layer, hidden states in and hidden states out: a trainable float gate, the fused top-k
    router (``ops.router_topk``), the one-launch plan, a dispatch with a deterministic backward, the INT4 gated FFN
    experts and the one-launch combine.  ``forward`` returns ``(out, router_logits)`` as the Hugging Face Mixtral block
    does.  Nothing is read back to the host.

    ``gate`` is an ``nn.Linear(hidden_dim, num_experts, bias=False)``: float, trainable, not quantised, run by torch
    (its weight is cast to the activations' type when they differ).  ``experts`` is a ``QuantizedMoEFFN`` (built here
    when not given; a ``LoRAQuantizedMoEFFN`` may be passed in, or an ``MXFP4MoEFFN``: built with ``input_grad=True`` it trains the
    router and everything upstream under grad mode, without it the block runs under ``torch.no_grad()``; or an ``NVFP4MoEFFN``,
    with the same ``input_grad`` keyword and the same rule).  State-dict keys: ``gate.weight`` and ``experts.*``.
    The combine (``ops.combine_any``) reads the expert rows in their own type, sums in float32 and rounds the output once
    to the activations' type: no cast pass either side of it.

    A shared expert (DeepSeek-V2 / V3, GLM-4.5, Kimi-K2, Llama-4, Qwen-MoE) is a dense gated FFN that every token passes
    through: ``shared_ffn_dim > 0`` builds ``shared_experts = QuantizedMoEFFN(1, hidden_dim, shared_ffn_dim)``, or pass a
    ready one-expert module as ``shared_experts=`` (a ``LoRAQuantizedMoEFFN`` works).  It runs on the tokens as they are
    (no dispatch) and its output enters the combine as the addend, behind the routed terms and untouched by the routing
    weights and ``routed_scaling_factor``.  ``shared_expert_gate=True`` (Qwen2-MoE) adds a float, trainable
    ``shared_expert_gate = nn.Linear(hidden_dim, 1, bias=False)`` run by torch like ``gate``; the shared output is then
    weighted per token by ``sigmoid(z)``, ``z`` the layer's output widened to float32.  State-dict keys:
    ``shared_experts.*`` and ``shared_expert_gate.weight``, absent when the feature is off.

    The routing rule is Mixtral's by default.  ``scoring="sigmoid"``, ``n_group`` / ``topk_group`` / ``group_top``
    (group-limited selection), ``routed_scaling_factor`` and ``selection_bias=True`` (a float32 buffer
    ``gate.e_score_correction_bias`` [E] of zeros, added to the scores for the selection only and moved by
    ``update_selection_bias``) select the rules of DeepSeek-V2 / V3, GLM-4.5, Kimi-K2 and Llama-4 (INTEGRATION.md
    section 11).  The forward makes one ``ops.router_score_topk`` call either way: with all at their defaults that is
    ``ops.router_topk``, bit for bit and kernel for kernel, and the state-dict keys are unchanged.

    ``activation`` (with ``activation_alpha`` / ``activation_limit``) is handed to the experts and the shared expert the
    block builds.  A module passed in as ``experts`` / ``shared_experts`` keeps its own; an explicit block argument that
    contradicts it raises ``ValueError``.

    ``expert_bias`` (gpt-oss) is handed to the experts the block builds (``QuantizedMoEFFN(expert_bias=True)``: frozen
    float32 parameters ``experts.gate_up_bias`` / ``experts.down_bias``); a module passed in as ``experts`` keeps its
    own, and an explicit argument that contradicts it raises ``ValueError``.  The combine multiplies the routing weight
    into an expert's output after its bias.  ``router_bias=True`` makes ``gate`` an ``nn.Linear(..., bias=True)``
    (``gate.bias``, gpt-oss's ``router.bias``: float, trainable, run by torch, part of ``router_logits``).  Both off: the
    state-dict keys of before.

    ``capacity_factor`` (Switch, GShard, Megatron-Core's ``moe_expert_capacity_factor``) bounds the rows an expert takes in
    a call at ``ceil(capacity_factor * T * top_k / num_experts)``, ``T`` the token rows of the call; the overflow is
    dropped, earlier tokens win, and the routing weights are NOT renormalised after a drop.  ``forward(x, token_mask)``
    takes a mask of the real tokens: a masked (padding) token is not routed at all.  Either one switches the forward to
    ``ops.route_plan_capped`` and the ``skip_dropped`` dispatch and combine; with neither it is the forward of before, bit
    for bit and launch for launch.  The state dict is unchanged.

    ``group_size`` (per-group INT4 scales, ``QuantizedMoEFFN``'s) is handed to the experts and the shared expert the block
    builds; a module passed in keeps its own, and an explicit argument that contradicts it raises ``ValueError``
    (INTEGRATION.md section 16)."""

    def __init__(self, num_experts: int, hidden_dim: int, ffn_dim: int, top_k: int = 2, precision: str = "default",
                 activation_dtype=None, renormalize: bool = True, experts=None, scoring: str = "softmax",
                 n_group: int = 1, topk_group: int = 1, group_top: int = 2, routed_scaling_factor: float = 1.0,
                 selection_bias: bool = False, shared_ffn_dim: int = 0, shared_experts=None,
                 shared_expert_gate: bool = False, activation=None, activation_alpha=None, activation_limit=None,
                 expert_bias=None, router_bias: bool = False, capacity_factor=None, group_size=None):
        super().__init__()
        from . import ops
        # None: not given (a built expert takes the default, a passed-in one keeps its own)
        act_kw = {k: v for k, v in (("activation", activation), ("activation_alpha", activation_alpha),
                                    ("activation_limit", activation_limit)) if v is not None}
        want = ops.activation_of(**act_kw)

        def check_activation(name, module):
            have = dict(zip(("activation", "activation_alpha", "activation_limit"), module.activation_args))
            given = dict(zip(("activation", "activation_alpha", "activation_limit"), want))
            for k in act_kw:
                if k != "activation" and have["activation"] != "swiglu_clamp":
                    continue                                    # (the two floats belong to the clamped kind alone)
                if have[k] != given[k]:
                    raise ValueError(f"{k}={act_kw[k]!r} contradicts {name}, built with {k}={have[k]!r}: leave the "
                                     f"block's argument out, or build {name} with it")
            have_gs = getattr(module, "group_size", None)
            if group_size is not None and _group_size(group_size, module.hidden_dim, module.ffn_dim) != have_gs:
                raise ValueError(f"group_size={group_size!r} contradicts {name}, built with group_size={have_gs!r}: leave "
                                 f"the block's argument out, or build {name} with it")
        if num_experts < 1 or num_experts > ops.ROUTE_MAX_EXPERTS:
            raise ValueError(f"num_experts must be in [1, {ops.ROUTE_MAX_EXPERTS}], got {num_experts}")
        if top_k < 1 or top_k > min(num_experts, ops.ROUTER_MAX_TOPK):
            raise ValueError(f"top_k must be in [1, min(num_experts, {ops.ROUTER_MAX_TOPK})], got {top_k}")
        if scoring not in ("softmax", "sigmoid"):
            raise ValueError(f"scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
        if n_group < 1 or n_group > ops.ROUTER_MAX_GROUPS or num_experts % n_group != 0:
            raise ValueError(f"n_group must be in [1, {ops.ROUTER_MAX_GROUPS}] and divide num_experts, got {n_group}")
        if topk_group < 1 or topk_group > n_group or topk_group * (num_experts // n_group) < top_k:
            raise ValueError(f"topk_group must be in [1, n_group] and its groups must hold top_k experts, got {topk_group}")
        if group_top not in (1, 2):
            raise ValueError(f"group_top must be 1 or 2, got {group_top}")
        if not math.isfinite(routed_scaling_factor):
            raise ValueError("routed_scaling_factor must be finite")
        if capacity_factor is not None:
            try:
                capacity_factor = float(capacity_factor)
            except (TypeError, ValueError):
                raise ValueError(f"capacity_factor must be a number > 0 or None, got {capacity_factor!r}") from None
            if not math.isfinite(capacity_factor) or capacity_factor <= 0.0:
                raise ValueError(f"capacity_factor must be finite and > 0, got {capacity_factor!r}")
        if experts is None:
            experts = QuantizedMoEFFN(num_experts, hidden_dim, ffn_dim, precision=precision,
                                      activation_dtype=activation_dtype, expert_bias=bool(expert_bias),
                                      group_size=group_size, **act_kw)
        elif (experts.num_experts, experts.hidden_dim, experts.ffn_dim) != (num_experts, hidden_dim, ffn_dim):
            raise ValueError("experts must have the block's num_experts, hidden_dim and ffn_dim")
        else:
            check_activation("experts", experts)
            have_bias = bool(getattr(experts, "expert_bias", False))
            if expert_bias is not None and bool(expert_bias) != have_bias:      # None: not given, the module keeps its own
                raise ValueError(f"expert_bias={expert_bias!r} contradicts experts, built with expert_bias={have_bias!r}: "
                                 "leave the block's argument out, or build experts with it")
        if shared_ffn_dim < 0 or shared_ffn_dim % 32 != 0:
            raise ValueError(f"shared_ffn_dim must be a non-negative multiple of 32, got {shared_ffn_dim}")
        if shared_experts is not None:
            if (shared_experts.num_experts, shared_experts.hidden_dim) != (1, hidden_dim):
                raise ValueError("shared_experts must be one expert (num_experts == 1) of the block's hidden_dim")
            if shared_ffn_dim and shared_experts.ffn_dim != shared_ffn_dim:
                raise ValueError("shared_ffn_dim and shared_experts.ffn_dim differ")
            check_activation("shared_experts", shared_experts)
        elif shared_ffn_dim:
            shared_experts = QuantizedMoEFFN(1, hidden_dim, shared_ffn_dim, precision=precision,
                                             activation_dtype=activation_dtype, group_size=group_size, **act_kw)
        if shared_expert_gate and shared_experts is None:
            raise ValueError("shared_expert_gate=True needs a shared expert (shared_ffn_dim or shared_experts)")
        self.num_experts, self.hidden_dim, self.ffn_dim = num_experts, hidden_dim, ffn_dim
        self.top_k, self.renormalize = top_k, bool(renormalize)
        self.scoring, self.n_group, self.topk_group, self.group_top = scoring, n_group, topk_group, group_top
        self.routed_scaling_factor = float(routed_scaling_factor)
        self.gate = nn.Linear(hidden_dim, num_experts, bias=bool(router_bias))
        if selection_bias:                   # the checkpoint's name: gate.e_score_correction_bias
            self.gate.register_buffer("e_score_correction_bias", torch.zeros(num_experts, dtype=torch.float32))
        self.experts = experts
        if shared_experts is not None:       # (no attribute at all otherwise: the state-dict keys stay those of before)
            self.shared_experts = shared_experts
        if shared_expert_gate:
            self.shared_expert_gate = nn.Linear(hidden_dim, 1, bias=False)
        self.capacity_factor = capacity_factor
        self.routing = None                  # (probs / scores, tokens_per_expert, indices) of the last forward
        self.kept_per_expert = None          # the plan's counts of the last forward (after the drops; == routing[1] without)
        self._token_mask = None              # the flat mask of the last forward, for aux_loss

    @classmethod
    def from_weights(cls, gate_weight: torch.Tensor, gate: List[torch.Tensor], up: List[torch.Tensor],
                     down: List[torch.Tensor], top_k: int = 2, precision: str = "default", activation_dtype=None,
                     renormalize: bool = True, shared=None, shared_expert_gate_weight=None, activation: str = "silu",
                     activation_alpha: float = 1.702, activation_limit: float = 7.0, router_bias=None, gate_bias=None,
                     up_bias=None, down_bias=None, group_size=None, **routing) -> "QuantizedSparseMoEBlock":
        """``gate_weight`` [E, H] (the router); ``gate[e]``, ``up[e]`` [F, H] and ``down[e]`` [H, F] as
        ``QuantizedMoEFFN.from_weights`` takes them.  ``shared``: ``(gate [Fs, H], up [Fs, H], down [H, Fs])`` of the
        shared expert; ``shared_expert_gate_weight`` [1, H]: the weight of its sigmoid gate.  ``routing``: the
        constructor's ``scoring``, ``n_group``, ``topk_group``, ``group_top``, ``routed_scaling_factor``,
        ``selection_bias`` and ``capacity_factor``.  ``activation`` (and its two floats): the experts' and the shared expert's.
        ``router_bias`` [E]: the bias of the router (``gate.bias``); ``gate_bias[e]``, ``up_bias[e]`` [F] and
        ``down_bias[e]`` [H]: the experts' biases as ``QuantizedMoEFFN.from_weights`` takes them (all three or none).
        ``group_size``: per-group quantisation of the experts and the shared expert."""
        act = dict(activation=activation, activation_alpha=activation_alpha, activation_limit=activation_limit)
        experts = QuantizedMoEFFN.from_weights(gate, up, down, precision=precision, activation_dtype=activation_dtype,
                                               gate_bias=gate_bias, up_bias=up_bias, down_bias=down_bias,
                                               group_size=group_size, **act)
        E, H = gate_weight.shape
        if E != experts.num_experts or H != experts.hidden_dim:
            raise ValueError("gate_weight must be [num_experts, hidden_dim]")
        if router_bias is not None and tuple(router_bias.shape) != (E,):
            raise ValueError("router_bias must be [num_experts]")
        shared_experts = None
        if shared is not None:
            sg, su, sd = shared
            shared_experts = QuantizedMoEFFN.from_weights([sg], [su], [sd], precision=precision,
                                                          activation_dtype=activation_dtype, group_size=group_size, **act)
        if shared_expert_gate_weight is not None and tuple(shared_expert_gate_weight.shape) != (1, H):
            raise ValueError("shared_expert_gate_weight must be [1, hidden_dim]")
        m = cls(E, H, experts.ffn_dim, top_k=top_k, precision=precision, activation_dtype=activation_dtype,
                renormalize=renormalize, experts=experts, shared_experts=shared_experts,
                shared_expert_gate=shared_expert_gate_weight is not None, router_bias=router_bias is not None,
                group_size=group_size, **routing)
        with torch.no_grad():
            m.gate.weight.copy_(gate_weight.float())
            if router_bias is not None:
                m.gate.bias.copy_(router_bias.float())
            if shared_expert_gate_weight is not None:
                m.shared_expert_gate.weight.copy_(shared_expert_gate_weight.float())
        return m

    @property
    def selection_bias(self):
        """The buffer ``gate.e_score_correction_bias`` [E], or None for a block built without ``selection_bias``."""
        return getattr(self.gate, "e_score_correction_bias", None)

    @property
    def scored_routing(self) -> bool:
        """Whether any routing setting differs from Mixtral's (the router then runs its scored kernel variant)."""
        return (self.scoring != "softmax" or self.n_group != 1 or self.routed_scaling_factor != 1.0
                or self.selection_bias is not None)

    def update_selection_bias(self, rate: float) -> None:
        """The aux-loss-free balancing step on the counts of the last forward: ``b_e += rate * sign(mean(c) - c_e)``, an
        over-loaded expert's bias goes down and an under-loaded one's up.  A few torch ops, nothing read back."""
        bias = self.selection_bias
        if bias is None:
            raise RuntimeError("update_selection_bias needs a block built with selection_bias=True")
        if self.routing is None:
            raise RuntimeError("update_selection_bias needs a forward before it")
        with torch.no_grad():
            counts = self.routing[1].to(torch.float32)
            bias.add_(torch.sign(counts.mean() - counts), alpha=rate)

    def router_logits(self, x2: torch.Tensor) -> torch.Tensor:
        w, b = self.gate.weight, self.gate.bias
        if b is not None and b.dtype != x2.dtype:
            b = b.to(x2.dtype)
        return nn.functional.linear(x2, w if w.dtype == x2.dtype else w.to(x2.dtype), b)

    def shared_output(self, x2: torch.Tensor, x_gate=None):
        """``(s [T, H], aw [T] float32 or None)``: the shared expert on the tokens themselves (one segment of all rows, its
        table made on the device) and, with ``shared_expert_gate``, its per-token weight ``sigmoid(z)`` in float32, ``z``
        computed from ``x_gate`` (default ``x2``); ``(None, None)`` for a block without a shared expert."""
        shared = getattr(self, "shared_experts", None)
        if shared is None:
            return None, None
        T = x2.shape[0]
        s = shared(x2, torch.full((1,), T, dtype=torch.int32, device=x2.device),
                   torch.zeros(1, dtype=torch.int32, device=x2.device))
        gate = getattr(self, "shared_expert_gate", None)
        if gate is None:
            return s, None
        w = gate.weight
        z = nn.functional.linear(x2 if x_gate is None else x_gate, w if w.dtype == x2.dtype else w.to(x2.dtype))
        return s, torch.sigmoid(z.to(torch.float32)).reshape(-1)

    def expert_capacity(self, tokens: int):
        """Rows an expert may take in a call of ``tokens`` token rows: ``ceil(capacity_factor * tokens * top_k /
        num_experts)`` (at least 1), or None for a block without ``capacity_factor``.  The mask's count is not used: it
        lives on the device."""
        if self.capacity_factor is None:
            return None
        return min(max(1, math.ceil(self.capacity_factor * tokens * self.top_k / self.num_experts)), 0x7fffffff)

    def forward(self, x: torch.Tensor, token_mask=None):
        """``x`` [..., H] on the GPU (float32, or the experts' 16-bit ``activation_dtype``) ->
        ``(out [..., H], router_logits [T, E])``, T the number of tokens: at most 65535 per call, the limit of
        ``ops.combine_any`` (more raises there; split the batch).  Under grad mode the router also writes the full softmax (the sigmoids with ``scoring="sigmoid"``),
        and ``self.routing = (probs, tokens_per_expert, indices)`` of this call is kept for ``aux_loss`` until the next
        call (``probs`` is None under ``torch.no_grad()``); the weights and the output are the same bits either way.
        ``probs`` carries its autograd graph: a loop that holds many blocks and wants no ``aux_loss`` drops it with
        ``block.routing = None`` after the forward.

        ``token_mask`` [...] (``x``'s shape without its last dimension, bool, True for a real token): a masked token is
        not routed, its output is its shared expert's term (zero without one) and it sends the gate and the experts no
        gradient; ``router_logits`` still has a row for it.  With a mask or a ``capacity_factor`` the counts in
        ``self.routing`` are the DEMAND (what the router chose among the real tokens, before any drop: what ``aux_loss``
        and ``update_selection_bias`` balance on) and ``self.kept_per_expert`` the rows each expert took."""
        if not x.is_cuda:
            raise RuntimeError("QuantizedSparseMoEBlock runs on the GPU (the product path has no CPU fallback)")
        from . import ops
        x2 = x.reshape(-1, self.hidden_dim)
        capped = self.capacity_factor is not None or token_mask is not None
        mask = None
        if token_mask is not None:
            if not isinstance(token_mask, torch.Tensor) or not token_mask.is_cuda or token_mask.device != x.device:
                raise RuntimeError("token_mask must be a CUDA tensor on x's device")
            if token_mask.dtype not in (torch.bool, torch.uint8) or tuple(token_mask.shape) != tuple(x.shape[:-1]):
                raise RuntimeError("token_mask must be a bool tensor of x's shape without its last dimension")
            mask = token_mask.reshape(-1)
        # Two gates read the tokens through one alias: autograd sums their input gradients there and hands x2 one gate
        # part, so x.grad is two additions over three parts (dispatch, shared expert, gates) with or without the shared gate.
        x_gate = x2.view_as(x2) if getattr(self, "shared_expert_gate", None) is not None else x2
        logits = self.router_logits(x_gate)
        weights, indices, *probs = ops.router_score_topk(
            logits, self.top_k, self.scoring, self.selection_bias, self.n_group, self.topk_group, self.group_top,
            self.renormalize, self.routed_scaling_factor, return_scores=torch.is_grad_enabled())
        self._token_mask = mask
        if not capped:
            tpe, offs, token_of_sorted, pos_of_slot = ops.route_plan(indices, self.num_experts)
            self.routing = (probs[0] if probs else None, tpe, indices)
            self.kept_per_expert = tpe
            rows = ops.dispatch_rows(x2, token_of_sorted, pos_of_slot, self.top_k)
            y = self.experts(rows, tpe, offs)
            s, aw = self.shared_output(x2, x_gate)
            out = ops.combine_any(y, pos_of_slot, weights, addend=s, addend_weight=aw, out_dtype=x.dtype)
            return out.reshape(x.shape), logits
        tpe, offs, token_of_sorted, pos_of_slot, demand = ops.route_plan_capped(
            indices, self.num_experts, self.expert_capacity(x2.shape[0]), mask)
        self.routing = (probs[0] if probs else None, demand, indices)
        self.kept_per_expert = tpe
        rows = ops.dispatch_rows(x2, token_of_sorted, pos_of_slot, self.top_k, skip_dropped=True)
        y = self.experts(rows, tpe, offs)
        s, aw = self.shared_output(x2, x_gate)
        out = ops.combine_any(y, pos_of_slot, weights, addend=s, addend_weight=aw, out_dtype=x.dtype, skip_dropped=True)
        return out.reshape(x.shape), logits

    def aux_loss(self, probs=None, tokens_per_expert=None, token_mask=None):
        """The Switch / Mixtral load-balancing loss ``E * sum_e f_e * P_e``: ``f_e = tokens_per_expert[e] / T`` (the share
        of the tokens that chose expert e, a constant) and ``P_e`` the mean router probability of e, a few torch ops.
        Both default to what the last ``forward`` under grad mode kept (``self.routing``): no launch is repeated, and the
        gradient reaches the router logits through the ``grad_probs`` input of the router's backward.  Or pass the
        ``probs`` [T, E] of ``ops.router_topk(..., return_probs=True)`` and the counts of ``ops.route_plan``.  With
        ``scoring="sigmoid"`` ``P`` is taken from ``scores / scores.sum(-1, keepdim=True)``.

        ``token_mask`` [T] (or any shape of T elements; True for a real token) leaves the padding out: ``P_e`` is the mean
        over the real tokens only and ``f_e = tokens_per_expert[e] / n_real``, with the counts of the last forward the
        demand among the real tokens and ``n_real = token_mask.sum()`` taken on the device (at least 1).  It defaults to
        the mask of the last forward (none, when that forward had none), whether ``probs`` is given or not: pass the
        ``probs`` of another call together with that call's mask (an all-true one for none; a mask that does not have one
        element per row of ``probs`` raises ``RuntimeError``).  Without a mask the result is the one of before, bit for
        bit."""
        if token_mask is None:
            token_mask = getattr(self, "_token_mask", None)
        if probs is None or tokens_per_expert is None:
            kept = getattr(self, "routing", None)
            if kept is None or (probs is None and kept[0] is None):
                raise RuntimeError("aux_loss needs probs and tokens_per_expert, or a forward under grad mode before it")
            probs = kept[0] if probs is None else probs
            tokens_per_expert = kept[1] if tokens_per_expert is None else tokens_per_expert
        if self.scoring == "sigmoid":        # the sigmoids of a row do not sum to 1
            probs = probs / probs.sum(dim=-1, keepdim=True)
        if token_mask is not None:
            m = token_mask.reshape(-1).to(device=probs.device, dtype=torch.float32)
            if m.numel() != probs.shape[0]:
                raise RuntimeError("token_mask (given, or kept from the last forward) must have one element per row of probs")
            n_real = m.sum().clamp(min=1.0)
            f = tokens_per_expert.detach().to(torch.float32) / n_real
            return self.num_experts * torch.sum(f * ((probs * m.unsqueeze(1)).sum(dim=0) / n_real))
        f = tokens_per_expert.detach().to(torch.float32) / probs.shape[0]
        return self.num_experts * torch.sum(f * probs.mean(dim=0))

    def extra_repr(self) -> str:
        s = f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, top_k={self.top_k}, renormalize={self.renormalize}"
        if self.scoring != "softmax":
            s += f", scoring={self.scoring}"
        if self.n_group != 1:
            s += f", n_group={self.n_group}, topk_group={self.topk_group}, group_top={self.group_top}"
        if self.routed_scaling_factor != 1.0:
            s += f", routed_scaling_factor={self.routed_scaling_factor}"
        if self.selection_bias is not None:
            s += ", selection_bias=True"
        if getattr(self, "shared_experts", None) is not None:
            s += f", shared_ffn_dim={self.shared_experts.ffn_dim}"
        if getattr(self, "shared_expert_gate", None) is not None:
            s += ", shared_expert_gate=True"
        if self.gate.bias is not None:
            s += ", router_bias=True"
        if self.capacity_factor is not None:
            s += f", capacity_factor={self.capacity_factor}"
        return s + self.experts._activation_repr()
