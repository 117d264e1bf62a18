"""GeGLU (tanh form) and clamped-SwiGLU activations of the gated INT4 FFN experts on the GPU: the four ops
(ops.moe_gated_forward, lora_gated_shrink, lora_gated_grad with ``activation=``, and ops.glu_backward).

  1. the INT4 GEMM consumes, bit for bit, the h the down adapter sees;
  2. h, dg, du pointwise against float64 on a grid across both tails, the clamp boundaries included;
  3. Frobenius accuracy on random data with the clamp active;
  4. the 16-bit contract: a float16 / bfloat16 call is the float32 call on the widened operands, rounded once;
  5. a grouped call equals the per-expert calls;
  8. ``activation="silu"`` given explicitly, and FQL_ACT_SILU through the new entry points, is the call without it.

The layers are in tests/test_gpu_glu_layers.py.  Errors measured on an MI355X are listed in DESIGN.md section 21."""
import itertools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import ALPHA, KINDS, LIMIT, act_kw, backward64, clamped_share, device_hidden, hidden64
from helpers import EXACT_REL_FRO, clipped_ranges, expert_table, fq, misaligned, ops, rel_fro_dev, same_bits, tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn4(shape, g, dtype=torch.float32):
    """4 * randn: about 4 % of g above limit = 7 and 8 % of u outside +-7, so the clamp is active."""
    return (4.0 * torch.randn(shape, device=DEV, generator=g)).to(dtype)


def offset_view(t, nbytes):
    """A contiguous copy of the 16-bit ``t`` whose storage starts ``nbytes`` past a 16-byte boundary."""
    k = nbytes // 2
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def covered_mask(tpe, offs, T):
    m = torch.zeros(T, dtype=torch.bool)
    for lo, hi in clipped_ranges(tpe.cpu(), offs.cpu(), T):
        m[lo:hi] = True
    return m.to(DEV)


_WEIGHTS = {}


def down_weights(E, K, N, seed=3):
    key = (E, K, N, seed)
    if key not in _WEIGHTS:
        torch.manual_seed(seed)
        q = [fq().quantize_weights(torch.randn(N, K) * 0.1) for _ in range(E)]
        _WEIGHTS[key] = tuple(torch.stack([t[i] for t in q]).to(DEV) for i in range(3))
    return _WEIGHTS[key]


# ---- 1. the GEMM consumes the adapter's h ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("precision", ["default", "fast"])
def test_gemm_consumes_the_adapters_hidden_activation(precision, dtype, kind):
    F, N, E = 128, 96, 2
    P, S, Z = down_weights(E, F, N)
    tpe, offs, T = expert_table([19, 26], gaps=[1, 2], tail=3)
    gate_up = randn4((T, 2 * F), gen(11), dtype)
    h = device_hidden(ops(), gate_up.float(), kind, tpe, offs, E)
    unc = ~covered_mask(tpe, offs, T)
    assert int(unc.sum()) == 6 and torch.count_nonzero(h[unc]) == 0 and float(h.abs().max()) > 0
    if kind == "swiglu_clamp":
        assert min(clamped_share(gate_up[~unc])) > 0.01
    want = ops().moe_forward(P, S, Z, h, None, tpe, offs, precision=precision)
    got = ops().moe_gated_forward(P, S, Z, gate_up, tpe, offs, precision=precision, out_dtype=torch.float32, **act_kw(kind))
    assert same_bits(got, want)
    assert torch.count_nonzero(got[unc]) == 0 and torch.isfinite(got).all() and float(got.abs().max()) > 0
    if dtype != torch.float32:                                   # ... and the 16-bit call is the call on the widened rows
        wide = ops().moe_gated_forward(P, S, Z, gate_up.float(), tpe, offs, precision=precision, **act_kw(kind))
        assert same_bits(got, wide)
        assert same_bits(device_hidden(ops(), gate_up, kind, tpe, offs, E), h)
    # not the silu kernel by another name
    assert not torch.equal(got, ops().moe_gated_forward(P, S, Z, gate_up, tpe, offs, precision=precision,
                                                        out_dtype=torch.float32))


# ---- 2. pointwise accuracy on a grid --------------------------------------------------------------------------------------

GRID_G = [-200.0, -90.0, -20.0, -7.5, -3.0, -0.75, 0.0, 0.75, 3.0, 6.99, 7.0, 7.01, 20.0, 90.0, 200.0]
GRID_U = [-7.01, -7.0, -3.0, 0.0, 3.0, 7.0, 7.01]
GRID_D = [-3.0, 0.0, 3.0]


def check_pointwise(name, got, ref, scale, a):
    """|got - ref| <= (16 + 8 |a|) 2^-24 S: a carries up to four roundings, which expf amplifies by |a|, plus a handful of
    roundings in the products.  Where S < 1e-30 the result is finite and no larger than 1e-30."""
    got = got.double()
    assert torch.isfinite(got).all(), name
    tiny = scale < 1e-30
    assert float(got[tiny].abs().max()) <= 1e-30 if bool(tiny.any()) else True, name
    bound = (16.0 + 8.0 * a.abs()) * 2.0 ** -24 * scale
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300))[~tiny]
    worst = float(ratio.max())
    print(f"ERR glu grid {name} worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pad", [0, 1])
def test_pointwise_grid(pad, kind):
    """315 combinations in one row: an odd width, so element loads; padded to 320 columns for the 16-byte path."""
    combos = list(itertools.product(GRID_G, GRID_U, GRID_D))
    assert len(combos) == 315
    combos += [(0.0, 0.0, 0.0)] * ((-len(combos)) % 64 * pad)
    gv, uv, dv = (torch.tensor(c, dtype=torch.float32, device=DEV) for c in zip(*combos))
    gate_up, dh = torch.cat([gv, uv]).reshape(1, -1), dv.reshape(1, -1)
    F = dh.shape[1]
    assert F == (320 if pad else 315)
    h = device_hidden(ops(), gate_up, kind)
    dgu = ops().glu_backward(gate_up, dh, **act_kw(kind))
    assert tuple(dgu.shape) == (1, 2 * F)
    h_ref = hidden64(kind, gate_up)
    dg_ref, du_ref, s_dg, s_du, a = backward64(kind, gate_up, dh)
    tag = f"{kind} pad={pad}"
    check_pointwise(f"{tag} h", h, h_ref, h_ref.abs(), a)
    check_pointwise(f"{tag} dg", dgu[:, :F], dg_ref, s_dg, a)
    check_pointwise(f"{tag} du", dgu[:, F:], du_ref, s_du, a)
    if kind == "swiglu_clamp":
        g32, u32, live = gv.reshape(1, -1), uv.reshape(1, -1), dv.reshape(1, -1) != 0
        lim = torch.tensor(LIMIT, dtype=torch.float32, device=DEV)
        masked_g, masked_u = g32 > lim, (u32 < -lim) | (u32 > lim)
        assert int(masked_g.sum()) >= 4 * 21 and int(masked_u.sum()) >= 2 * 45
        assert torch.count_nonzero(dgu[:, :F][masked_g]) == 0            # exactly zero where the clamp is active
        assert torch.count_nonzero(dgu[:, F:][masked_u]) == 0
        # ... and the gradient passes at equality: g = 7 (u' != 0 on this grid), u = +-7 (g' sigma != 0 unless g = 0)
        at_g = (g32 == lim) & live
        at_u = (u32.abs() == lim) & live & (g32 != 0) & (g32 > -20)
        assert int(at_g.sum()) == 14 and int(at_u.sum()) > 40
        assert bool((dgu[:, :F][at_g] != 0).all()) and bool((dgu[:, F:][at_u] != 0).all())


# ---- 3. Frobenius accuracy on random data ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F,which", [(32, None), (130, None), (129, None), (32, "gate_up"), (32, "dh")])
def test_glu_backward_against_float64(F, which, kind):
    T = 37
    g = gen(F)
    gate_up, dh = randn4((T, 2 * F), g), torch.randn(T, F, device=DEV, generator=g)
    if which == "gate_up":
        gate_up = misaligned(gate_up, 1)
    elif which == "dh":
        dh = misaligned(dh, 1)
    for share in clamped_share(gate_up):
        assert 0.01 < share < 0.5, share
    got = ops().glu_backward(gate_up, dh, **act_kw(kind))
    dg, du, *_ = backward64(kind, gate_up, dh)
    err = rel_fro_dev(got, torch.cat([dg, du], dim=1))
    print(f"ERR glu_backward {kind} F={F} offset={which} fro={err:.3e}")
    assert tuple(got.shape) == (T, 2 * F) and got.dtype == torch.float32 and err < EXACT_REL_FRO


def gated_inputs(C, r, layout, seed, offset=0, dtype=torch.float32):
    """A ragged 3-expert table (one empty expert, gaps, uncovered tail), gate_up [T, 2C] and an adapter weight."""
    tpe, offs, T = expert_table([19, 0, 26], gaps=[1, 0, 2], tail=3)
    g = gen(seed)
    gate_up = randn4((T, 2 * C), g, dtype)
    if offset:
        gate_up = misaligned(gate_up, offset)
    w = torch.randn((3, r, C) if layout == "rc" else (3, C, r), device=DEV, generator=g)
    v = torch.randn(T, r, device=DEV, generator=g)
    return tpe, offs, T, gate_up, w, v


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", [4, 64])
@pytest.mark.parametrize("layout", ["rc", "cr"])
@pytest.mark.parametrize("C", [64, 130, 2816])
def test_gated_shrink_and_grad_against_float64(C, layout, r, kind):
    tpe, offs, T, gate_up, w, v = gated_inputs(C, r, layout, seed=C + r)
    h = hidden64(kind, gate_up)
    u = ops().lora_gated_shrink(gate_up, w, layout, tpe, offs, scale=0.5, **act_kw(kind))
    d = ops().lora_gated_grad(gate_up, v, layout, 3, tpe, offs, scale=0.5, **act_kw(kind))
    u_ref = torch.zeros(T, r, dtype=torch.float64, device=DEV)
    d_ref = torch.zeros_like(d, dtype=torch.float64)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        we = w[e].double() if layout == "rc" else w[e].double().t()              # [r, C]
        u_ref[lo:hi] = 0.5 * h[lo:hi] @ we.t()
        de = 0.5 * v[lo:hi].double().t() @ h[lo:hi]                              # [r, C]
        d_ref[e] = de if layout == "rc" else de.t()
    eu, ed = rel_fro_dev(u, u_ref), rel_fro_dev(d, d_ref)
    print(f"ERR glu gated {kind} C={C} {layout} r={r} shrink={eu:.3e} grad={ed:.3e}")
    assert eu < tol(EXACT_REL_FRO) and ed < tol(EXACT_REL_FRO)


# ---- 4. the 16-bit contract -----------------------------------------------------------------------------------------------

def ragged(T):
    if T < 10:
        return expert_table([T - 3, 0, 1], gaps=[1, 0, 0], tail=1)
    a = (T - 4) // 3
    return expert_table([a, 0, T - 4 - a], gaps=[1, 0, 1], tail=2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("precision", ["int8", "fast", "default"])       # L = 1, 2, 3
@pytest.mark.parametrize("T,offset", [(5, 0), (700, 0), (41, 2)])       # one row per workgroup / ACT_ROWS rows / element loads
def test_gated_forward_equals_float32_on_widened(T, offset, precision, dtype, kind):
    K, N = 96, 160
    P, S, Z = down_weights(3, K, N)
    tpe, offs, T_ = ragged(T)
    assert T_ == T
    gu = randn4((T, 2 * K), gen(T), dtype)
    if offset:
        gu = offset_view(gu, offset)
    kw = dict(precision=precision, **act_kw(kind))
    want32 = ops().moe_gated_forward(P, S, Z, gu.float(), tpe, offs, **kw)
    got = ops().moe_gated_forward(P, S, Z, gu, tpe, offs, **kw)
    assert got.dtype == dtype and same_bits(got, want32.to(dtype))
    got32 = ops().moe_gated_forward(P, S, Z, gu, tpe, offs, out_dtype=torch.float32, **kw)
    assert same_bits(got32, want32)
    assert same_bits(ops().moe_gated_forward(P, S, Z, gu.float(), tpe, offs, out_dtype=dtype, **kw), want32.to(dtype))
    assert torch.isfinite(want32).all() and float(want32.abs().max()) > 0
    unc = ~covered_mask(tpe, offs, T)
    assert int(unc.sum()) == (2 if T < 10 else 4) and torch.count_nonzero(got[unc]) == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,offset", [(2816, 0), (130, 0), (129, 0), (2816, 2)])     # 4, 2, 1 and 1 elements per load
def test_gated_shrink_and_grad_equal_float32_on_widened(C, offset, dtype, kind):
    g = gen(C)
    tpe, offs, T = ragged(48)
    gu = randn4((T, 2 * C), g, dtype)
    wide = gu.float()
    if offset:                                                   # one element off in either type: the same load width,
        gu, wide = offset_view(gu, offset), misaligned(wide, offset // 2)       # so the same summation order
    for r, layout in ((4, "rc"), (16, "cr"), (64, "rc")):
        v = torch.randn(T, r, device=DEV, generator=g)
        w = torch.randn((3, r, C) if layout == "rc" else (3, C, r), device=DEV, generator=g) * 0.1
        u16 = ops().lora_gated_shrink(gu, w, layout, tpe, offs, scale=1.5, **act_kw(kind))
        d16 = ops().lora_gated_grad(gu, v, layout, 3, tpe, offs, scale=0.5, **act_kw(kind))
        assert u16.dtype == torch.float32 and d16.dtype == torch.float32
        assert same_bits(u16, ops().lora_gated_shrink(wide, w, layout, tpe, offs, scale=1.5, **act_kw(kind)))
        assert same_bits(d16, ops().lora_gated_grad(wide, v, layout, 3, tpe, offs, scale=0.5, **act_kw(kind)))
        assert float(u16.abs().max()) > 0 and float(d16.abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,offset", [(2816, 0), (130, 0), (129, 0), (2816, 2)])
def test_glu_backward_equals_float32_on_widened(F, offset, dtype, kind):
    T = 19
    g = gen(F + offset)
    gu, dh = randn4((T, 2 * F), g, dtype), torch.randn(T, F, device=DEV, generator=g).to(dtype)
    if offset:
        gu = offset_view(gu, offset)
    kw = act_kw(kind)
    want32 = ops().glu_backward(gu.float(), dh.float(), **kw)
    got = ops().glu_backward(gu, dh, **kw)
    assert got.dtype == dtype and same_bits(got, want32.to(dtype))
    # every mix of the three element types (27 kernels per width)
    for a, b, o in itertools.product([torch.float32, dtype], repeat=3):
        assert same_bits(ops().glu_backward(gu.to(a), dh.to(b), out_dtype=o, **kw), want32.to(o)), (a, b, o)
    other = DTYPES[1 - DTYPES.index(dtype)]
    assert same_bits(ops().glu_backward(gu, dh.float().to(other), out_dtype=other, **kw),
                     ops().glu_backward(gu.float(), dh.float().to(other).float(), **kw).to(other))
    if kind == "swiglu_clamp":                                   # the masks survive the rounding: exact zeros
        big = gu[:, :F].float() > LIMIT
        assert int(big.sum()) > 0 and torch.count_nonzero(got[:, :F][big]) == 0


# ---- 5. grouped equals per expert -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", [4, 64])
@pytest.mark.parametrize("layout", ["rc", "cr"])
@pytest.mark.parametrize("C,offset", [(130, 0), (2816, 0), (2816, 1)])
def test_gated_kernels_grouped_equal_per_expert(C, offset, layout, r, kind):
    tpe, offs, T, gate_up, w, v = gated_inputs(C, r, layout, seed=7 * C + r, offset=offset)
    u = ops().lora_gated_shrink(gate_up, w, layout, tpe, offs, **act_kw(kind))
    d = ops().lora_gated_grad(gate_up, v, layout, 3, tpe, offs, **act_kw(kind))
    covered = torch.zeros(T, dtype=torch.bool)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        covered[lo:hi] = True
        if hi == lo:
            assert torch.count_nonzero(d[e]) == 0
            continue
        rows = gate_up[lo:hi].contiguous()
        if offset:
            rows = misaligned(rows, offset)                  # the same load width as the grouped call
        assert same_bits(u[lo:hi], ops().lora_gated_shrink(rows, w[e], layout, **act_kw(kind)))
        assert same_bits(d[e], ops().lora_gated_grad(rows, v[lo:hi].contiguous(), layout, **act_kw(kind))[0])
    assert torch.count_nonzero(u[~covered.to(DEV)]) == 0


# ---- 8. the default is untouched ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_explicit_silu_is_the_call_without_it(dtype):
    from fused_int4_amd import _native
    o = ops()
    K, N, r = 96, 160, 16
    P, S, Z = down_weights(3, K, N)
    tpe, offs, T = ragged(48)
    g = gen(5)
    gu = randn4((T, 2 * K), g, dtype)
    dh = torch.randn(T, K, device=DEV, generator=g).to(dtype)
    w = torch.randn(3, r, K, device=DEV, generator=g)
    v = torch.randn(T, r, device=DEV, generator=g)
    silu = act_kw("silu", alpha=3.0, limit=2.0)                  # the two floats are ignored
    y = o.moe_gated_forward(P, S, Z, gu, tpe, offs)
    u = o.lora_gated_shrink(gu, w, "rc", tpe, offs, scale=0.5)
    d = o.lora_gated_grad(gu, v, "rc", 3, tpe, offs, scale=0.5)
    b = o.swiglu_backward(gu, dh)
    assert same_bits(o.moe_gated_forward(P, S, Z, gu, tpe, offs, **silu), y)
    assert same_bits(o.lora_gated_shrink(gu, w, "rc", tpe, offs, scale=0.5, **silu), u)
    assert same_bits(o.lora_gated_grad(gu, v, "rc", 3, tpe, offs, scale=0.5, **silu), d)
    assert same_bits(o.glu_backward(gu, dh, **silu), b) and same_bits(o.glu_backward(gu, dh), b)
    # FQL_ACT_SILU through the four new entry points: the siblings' kernels, the siblings' bits
    dt, f32 = o._DTYPES[dtype], o._DTYPES[torch.float32]
    L = _native.lib()
    y2, u2, d2, b2 = torch.empty_like(y), torch.empty_like(u), torch.empty_like(d), torch.empty_like(b)
    o._launch("fql_moe_glu_fwd", gu.device, P, S, Z, gu, dt, tpe, offs, y2, dt, 3, T, K, N, 0, _native.ACT_SILU, float("nan"),
              -1.0, ws_bytes=L.fql_moe_workspace_bytes(3, T, K, N, 0))
    o._launch("fql_lora_glu_shrink", gu.device, gu, dt, w, _native.LORA_RC, tpe, offs, u2, 3, T, K, r, 0.5, _native.ACT_SILU,
              float("nan"), -1.0)
    o._launch("fql_lora_glu_grad", gu.device, gu, dt, v, tpe, offs, d2, _native.LORA_RC, 3, T, K, r, 0.5, _native.ACT_SILU,
              float("nan"), -1.0)
    o._launch("fql_glu_bwd", gu.device, gu, dt, dh, dt, b2, dt, T, K, _native.ACT_SILU, float("nan"), -1.0)
    assert f32 == 0
    for name, got, want in (("fwd", y2, y), ("shrink", u2, u), ("grad", d2, d), ("bwd", b2, b)):
        assert same_bits(got, want), name
