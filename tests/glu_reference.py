"""float64 restatement (torch, on the tensors' device; no fql_* kernel is called) of the activation kinds of the gated FFN
experts, include/fql_int4.h FQL_ACT_*: h = g' * sigma(a) * u' and its backward.  Shared by tests/test_gpu_glu*.py."""
import math

import torch

KINDS = ["gelu_tanh", "swiglu_clamp"]
ALPHA, LIMIT = 1.702, 7.0
C0 = 2.0 * math.sqrt(2.0 / math.pi)
C1 = 0.044715 * C0


def act_kw(kind, alpha=ALPHA, limit=LIMIT):
    return dict(activation=kind, activation_alpha=alpha, activation_limit=limit)


def parts64(kind, g, u, alpha=ALPHA, limit=LIMIT):
    """(g', u', a, a', pass_g, pass_u) in float64; pass_*: where the clamped kind lets the gradient through."""
    g, u = g.double(), u.double()
    on = torch.ones_like(g, dtype=torch.bool)
    if kind == "silu":
        return g, u, g, torch.ones_like(g), on, on
    if kind == "gelu_tanh":
        return g, u, g * (C0 + C1 * g * g), C0 + 3.0 * C1 * g * g, on, on
    assert kind == "swiglu_clamp"
    gp = torch.clamp(g, max=limit)
    return gp, torch.clamp(u, -limit, limit) + 1.0, alpha * gp, torch.full_like(g, alpha), g <= limit, (u >= -limit) & (u <= limit)


def hidden64(kind, gate_up, alpha=ALPHA, limit=LIMIT):
    C = gate_up.shape[1] // 2
    gp, up, a, _, _, _ = parts64(kind, gate_up[:, :C], gate_up[:, C:], alpha, limit)
    return gp * torch.sigmoid(a) * up


def backward64(kind, gate_up, dh, alpha=ALPHA, limit=LIMIT):
    """(dg, du, S_dg, S_du, a): the float64 gradients, and the scales of the pointwise bound -- for dg the derivative with
    its two terms not allowed to cancel."""
    F = dh.shape[1]
    gp, up, a, ad, pg, pu = parts64(kind, gate_up[:, :F], gate_up[:, F:], alpha, limit)
    d = dh.double()
    sig = torch.sigmoid(a)
    om = torch.sigmoid(-a)                                       # 1 - sigma without cancellation
    dg = torch.where(pg, d * up * sig * (1.0 + gp * ad * om), torch.zeros_like(d))
    du = torch.where(pu, d * gp * sig, torch.zeros_like(d))
    s_dg = (d * up).abs() * sig * (1.0 + (gp * ad).abs() * om)
    return dg, du, s_dg, du.abs(), a


def hidden_autograd(kind, g, u, alpha=ALPHA, limit=LIMIT):
    """h from differentiable torch ops (float64 tensors in a graph): torch.clamp's backward passes equality."""
    if kind == "silu":
        return torch.nn.functional.silu(g) * u
    if kind == "gelu_tanh":
        return g * torch.sigmoid(g * (C0 + C1 * g * g)) * u
    gp = torch.clamp(g, max=limit)
    return gp * torch.sigmoid(alpha * gp) * (torch.clamp(u, -limit, limit) + 1.0)


def clamped_share(gate_up, limit=LIMIT):
    """(share of g above limit, share of u outside [-limit, limit])."""
    F = gate_up.shape[1] // 2
    g, u = gate_up[:, :F].double(), gate_up[:, F:].double()
    return float((g > limit).double().mean()), float((u.abs() > limit).double().mean())


def device_hidden(ops, gate_up, kind, tpe=None, offs=None, E=1, alpha=ALPHA, limit=LIMIT):
    """The device's own h [T, C] float32, 64 columns at a time: lora_gated_shrink at r = 64 with unit rows that select the
    columns -- a sum of h * 1 and exact zeros is h.  Rows no expert covers come back zero."""
    T, C = gate_up.shape[0], gate_up.shape[1] // 2
    out = torch.empty(T, C, dtype=torch.float32, device=gate_up.device)
    for c0 in range(0, C, 64):
        n = min(64, C - c0)
        W = torch.zeros(E, 64, C, device=gate_up.device)
        W[:, torch.arange(n), c0 + torch.arange(n)] = 1.0
        u = ops.lora_gated_shrink(gate_up, W if tpe is not None else W[0], "rc", tpe, offs, **act_kw(kind, alpha, limit))
        out[:, c0:c0 + n] = u[:, :n]
    return out
