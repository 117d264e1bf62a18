"""Low-rank adapters on the gated INT4 FFN experts on the GPU (LoRAQuantizedMoEFFN, ops.moe_ffn_lora_forward and the
kernels behind ops.lora_gated_shrink / lora_gated_grad / swiglu_backward) against float64 torch on the dequantised
weights, plus the bitwise promises of include/fql_int4.h.

Errors measured on an MI355X are listed in DESIGN.md section 11."""
import itertools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import EXACT_REL_FRO, clipped_ranges, expert_table, fq, misaligned, ops, rel_fro_dev, row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANKS = [4, 8, 16, 32, 64]
FFN_REL_FRO = 2e-5             # the bound tests/test_gpu_backward.py holds the two-GEMM QuantizedMoEFFN backward to
# precision="fast" (two limbs): the bounds tests/test_gpu_backward_paths.py applies to QuantizedMoEFFN, restated
FAST_REL_FRO, FAST_ROW_TOL = 2e-4, 1e-3
ADAPTERS = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")


def tol(base):
    return max(base, 1e-5)


def w64(packed, scales, zps):
    return fq().dequantize_weights(packed.cpu(), scales.cpu(), zps.cpu()).double()


# ---- the module ---------------------------------------------------------------------------------------------------

_BASES = {}


def base_layer(E, H, F, seed, precision="default"):
    """One quantised QuantizedMoEFFN per shape on the device (shared by the ranks: quantising is the slow part)."""
    key = (E, H, F, seed, precision)
    if key not in _BASES:
        torch.manual_seed(seed)
        gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
        up = [torch.randn(F, H) * 0.1 for _ in range(E)]
        down = [torch.randn(H, F) * 0.1 for _ in range(E)]
        _BASES[key] = fq().QuantizedMoEFFN.from_weights(gate, up, down, precision=precision).to(DEV)
    return _BASES[key]


def ffn_layer(E, H, F, r, seed, precision="default"):
    base = base_layer(E, H, F, seed, precision)
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, r, alpha=2 * r)
    g = torch.Generator(device=DEV).manual_seed(seed + r)
    with torch.no_grad():
        m.gate_up_lora_B.normal_(0, 0.1, generator=g)
        m.down_lora_B.normal_(0, 0.1, generator=g)
    return base, m


def ffn_ref(m, x, tpe, offs, gy):
    """float64 forward and gradients (autograd on the CPU) of the block on the dequantised weights."""
    E, F, s = m.num_experts, m.ffn_dim, m.scaling
    Wgu = [w64(m.gate_up_packed[e], m.gate_up_scales[e], m.gate_up_zero_points[e]) for e in range(E)]
    Wd = [w64(m.down_packed[e], m.down_scales[e], m.down_zero_points[e]) for e in range(E)]
    x64, Agu, Bgu, Ad, Bd = (t.detach().cpu().double().requires_grad_()
                             for t in (x, m.gate_up_lora_A, m.gate_up_lora_B, m.down_lora_A, m.down_lora_B))
    T = x.shape[0]
    y = torch.zeros(T, m.hidden_dim, dtype=torch.float64)
    rows = []
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            continue
        xe = x64[lo:hi]
        gu = xe @ Wgu[e].t() + s * (xe @ Agu[e].t()) @ Bgu[e].t()
        h = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
        rows.append((lo, hi, h @ Wd[e].t() + s * (h @ Ad[e].t()) @ Bd[e].t()))
    for lo, hi, ye in rows:
        y = y.index_put((torch.arange(lo, hi),), ye)
    y.backward(gy.cpu().double())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return (y.detach(), zero(x64)) + tuple(zero(t) for t in (Agu, Bgu, Ad, Bd))


def run(m, x, tpe, offs, gy, requires=("x",) + ADAPTERS):
    """Forward + backward; returns (y, dx, dA_gu, dB_gu, dA_d, dB_d), None for what was not asked for."""
    for name in ADAPTERS:
        p = getattr(m, name)
        p.grad = None
        p.requires_grad_(name in requires)
    xg = x.detach().clone().requires_grad_("x" in requires)
    y = m(xg, tpe, offs)
    y.backward(gy)
    out = (y.detach(), xg.grad) + tuple(getattr(m, name).grad for name in ADAPTERS)
    for name in ADAPTERS:
        getattr(m, name).requires_grad_(True)
    return out


NAMES = ("y", "dx", "dA_gu", "dB_gu", "dA_d", "dB_d")
# (E, H, F, counts, gaps, tail)
CASES = {
    "small": (3, 128, 192, [20, 0, 30], None, 0),                       # as test_gated_ffn_backward
    "ragged": (4, 256, 320, [17, 0, 33, 5], [2, 0, 3, 1], 3),            # gaps and uncovered trailing rows
    "one_row": (3, 128, 192, [1, 40, 1], None, 0),
    "large": (4, 1024, 2816, [100, 50, 0, 150], None, 0),
}


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("case", list(CASES))
def test_ffn_lora_against_float64(case, r):
    E, H, F, counts, gaps, tail = CASES[case]
    _, m = ffn_layer(E, H, F, r, seed=100 + len(case))
    tpe, offs, T = expert_table(counts, gaps=gaps, tail=tail)
    g = torch.Generator(device=DEV).manual_seed(r)
    x = torch.randn(T, H, device=DEV, generator=g)
    gy = torch.randn(T, H, device=DEV, generator=g)
    got = run(m, x, tpe, offs, gy)
    ref = ffn_ref(m, x, tpe, offs, gy)
    errs = [rel_fro_dev(a, b) for a, b in zip(got, ref)]
    print(f"ERR ffn_lora {case} r={r} " + " ".join(f"{n}={e:.3e}" for n, e in zip(NAMES, errs)))
    for n, e in zip(NAMES, errs):
        assert e < FFN_REL_FRO, (n, e)


def test_ffn_lora_fast_precision():
    E, H, F = 3, 256, 384
    _, m = ffn_layer(E, H, F, 16, seed=42, precision="fast")
    tpe, offs, T = expert_table([30, 0, 50], gaps=[0, 0, 2], tail=1)
    g = torch.Generator(device=DEV).manual_seed(43)
    x = torch.randn(T, H, device=DEV, generator=g)
    gy = torch.randn(T, H, device=DEV, generator=g)
    got = run(m, x, tpe, offs, gy)
    ref = ffn_ref(m, x, tpe, offs, gy)
    for n, a, b in zip(NAMES[:2], got, ref):
        fro, row = rel_fro_dev(a, b), row_rel_err(a, b)
        print(f"ERR ffn_lora fast {n} fro={fro:.3e} row={row:.3e}")
        assert fro < FAST_REL_FRO and row < FAST_ROW_TOL, (n, fro, row)


# ---- the kernels alone --------------------------------------------------------------------------------------------

def hidden64(gate_up):
    C = gate_up.shape[1] // 2
    g = gate_up.double()
    return torch.nn.functional.silu(g[:, :C]) * g[:, C:]


def gated_inputs(C, r, layout, seed, offset=0):
    """A ragged 3-expert table (one empty expert, gaps, uncovered tail), gate_up [T, 2C] and an adapter weight."""
    tpe, offs, T = expert_table([19, 0, 26], gaps=[1, 0, 2], tail=3)
    g = torch.Generator(device=DEV).manual_seed(seed)
    gate_up = torch.randn(T, 2 * C, device=DEV, generator=g)
    if offset:
        gate_up = misaligned(gate_up, offset)
    w = torch.randn((3, r, C) if layout == "rc" else (3, C, r), device=DEV, generator=g)
    v = torch.randn(T, r, device=DEV, generator=g)
    return tpe, offs, T, gate_up, w, v


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("layout", ["rc", "cr"])
@pytest.mark.parametrize("C,offset", [(64, 0), (130, 0), (2816, 0), (2816, 1)])
def test_gated_shrink_and_grad_against_float64(C, offset, layout, r):
    tpe, offs, T, gate_up, w, v = gated_inputs(C, r, layout, seed=C + r, offset=offset)
    h = hidden64(gate_up)
    u = ops().lora_gated_shrink(gate_up, w, layout, tpe, offs, scale=0.5)
    d = ops().lora_gated_grad(gate_up, v, layout, 3, tpe, offs, scale=0.5)
    u_ref = torch.zeros(T, r, dtype=torch.float64, device=DEV)
    d_ref = torch.zeros_like(d, dtype=torch.float64)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        we = w[e].double() if layout == "rc" else w[e].double().t()              # [r, C]
        u_ref[lo:hi] = 0.5 * h[lo:hi] @ we.t()
        de = 0.5 * v[lo:hi].double().t() @ h[lo:hi]                              # [r, C]
        d_ref[e] = de if layout == "rc" else de.t()
    eu, ed = rel_fro_dev(u, u_ref), rel_fro_dev(d, d_ref)
    print(f"ERR gated C={C} off={offset} {layout} r={r} shrink={eu:.3e} grad={ed:.3e}")
    assert eu < tol(EXACT_REL_FRO) and ed < tol(EXACT_REL_FRO)


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("layout", ["rc", "cr"])
@pytest.mark.parametrize("C,offset", [(130, 0), (2816, 0), (2816, 1)])
def test_gated_kernels_grouped_equal_per_expert(C, offset, layout, r):
    tpe, offs, T, gate_up, w, v = gated_inputs(C, r, layout, seed=7 * C + r, offset=offset)
    u = ops().lora_gated_shrink(gate_up, w, layout, tpe, offs)
    d = ops().lora_gated_grad(gate_up, v, layout, 3, tpe, offs)
    covered = torch.zeros(T, dtype=torch.bool)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        covered[lo:hi] = True
        if hi == lo:
            assert torch.count_nonzero(d[e]) == 0
            continue
        rows = gate_up[lo:hi].contiguous()
        if offset:
            rows = misaligned(rows, offset)                  # the same load width as the grouped call
        assert torch.equal(u[lo:hi], ops().lora_gated_shrink(rows, w[e], layout))
        assert torch.equal(d[e], ops().lora_gated_grad(rows, v[lo:hi].contiguous(), layout)[0])
    assert torch.count_nonzero(u[~covered.to(DEV)]) == 0


def swiglu_ref(gate_up, dh):
    F = dh.shape[1]
    g, u, d = gate_up[:, :F].double(), gate_up[:, F:].double(), dh.double()
    sig = 1.0 / (1.0 + torch.exp(-g))
    return torch.cat([d * u * (sig * (1.0 + g * (1.0 - sig))), d * (g * sig)], dim=1)


@pytest.mark.parametrize("F,which", [(32, None), (130, None), (11008, None), (11008, "gate_up"), (11008, "dh")])
def test_swiglu_backward_against_float64(F, which):
    T = 37
    g = torch.Generator(device=DEV).manual_seed(F)
    gate_up = torch.randn(T, 2 * F, device=DEV, generator=g)
    dh = torch.randn(T, F, device=DEV, generator=g)
    if which == "gate_up":
        gate_up = misaligned(gate_up, 1)
    elif which == "dh":
        dh = misaligned(dh, 1)
    got = ops().swiglu_backward(gate_up, dh)
    err = rel_fro_dev(got, swiglu_ref(gate_up, dh))
    print(f"ERR swiglu_backward F={F} offset={which} fro={err:.3e}")
    assert tuple(got.shape) == (T, 2 * F) and err < EXACT_REL_FRO


@pytest.mark.parametrize("pad", [0, 1])
def test_swiglu_backward_grid(pad):
    """g far into both tails of the sigmoid: finite everywhere, within 16 * 2^-24 relative of float64, and exactly zero
    where the reference is below 1e-30 (expf overflows there: sigma must come out 0, not NaN).  63 combinations in one
    row (scalar path); padded to 64 columns for the 16-byte path."""
    combos = list(itertools.product([-200.0, -90.0, -20.0, 0.0, 20.0, 90.0, 200.0], [-3.0, 0.0, 3.0], [-3.0, 0.0, 3.0]))
    combos += [(0.0, 0.0, 0.0)] * pad
    gv, uv, dv = (torch.tensor(c, dtype=torch.float32, device=DEV) for c in zip(*combos))
    gate_up = torch.cat([gv, uv]).reshape(1, -1)
    dh = dv.reshape(1, -1)
    got = ops().swiglu_backward(gate_up, dh).double()
    ref = swiglu_ref(gate_up, dh)
    assert torch.isfinite(got).all()
    tiny = ref.abs() < 1e-30
    assert (got[tiny] == 0).all()
    rel = ((got - ref).abs() / ref.abs().clamp_min(1e-300))[~tiny]
    print(f"ERR swiglu_backward grid pad={pad} max rel={float(rel.max()):.3e}")
    assert float(rel.max()) <= 16 * 2.0 ** -24


# ---- bitwise promises ---------------------------------------------------------------------------------------------

def small_problem(r=16, seed=5):
    E, H, F = 4, 256, 320
    base, m = ffn_layer(E, H, F, r, seed=seed)
    tpe, offs, T = expert_table([17, 0, 33, 5], gaps=[2, 0, 3, 1], tail=3)
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, H, device=DEV, generator=g)
    gy = torch.randn(T, H, device=DEV, generator=g)
    return base, m, tpe, offs, T, x, gy


def test_two_runs_are_bitwise_equal():
    _, m, tpe, offs, T, x, gy = small_problem()
    a, b = run(m, x, tpe, offs, gy), run(m, x, tpe, offs, gy)
    for n, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), n


@pytest.mark.parametrize("r", [4, 16, 64])
def test_grouped_equals_per_expert(r):
    _, m, tpe, offs, T, x, gy = small_problem(r=r)
    y, dx, *grads = run(m, x, tpe, offs, gy)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    for e, (lo, hi) in enumerate(clipped_ranges(tpe.cpu(), offs.cpu(), T)):
        if hi == lo:
            for n, gr in zip(NAMES[2:], grads):
                assert torch.count_nonzero(gr[e]) == 0, n
            continue
        xe = x[lo:hi].clone().requires_grad_()
        ad = [getattr(m, n)[e:e + 1].detach().clone().requires_grad_() for n in ADAPTERS]
        ye = ops().moe_ffn_lora_forward(m.gate_up_packed[e:e + 1], m.gate_up_scales[e:e + 1],
                                        m.gate_up_zero_points[e:e + 1], m.down_packed[e:e + 1], m.down_scales[e:e + 1],
                                        m.down_zero_points[e:e + 1], xe, *ad, m.scaling, one * (hi - lo), one * 0,
                                        precision=m.precision)
        ye.backward(gy[lo:hi].clone())
        assert torch.equal(y[lo:hi], ye.detach()), e
        assert torch.equal(dx[lo:hi], xe.grad), e
        for n, gr, a in zip(NAMES[2:], grads, ad):
            assert torch.equal(gr[e], a.grad[0]), (n, e)


def test_fresh_adapter_equals_the_base_layer():
    E, H, F = 4, 256, 320
    base = base_layer(E, H, F, seed=5)
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, 16)               # B = 0
    tpe, offs, T = expert_table([17, 0, 33, 5], gaps=[2, 0, 3, 1], tail=3)
    x = torch.randn(T, H, device=DEV)
    with torch.no_grad():
        want = base(x, tpe, offs)
    assert torch.equal(m(x, tpe, offs), want)


def test_no_grad_forward_equals_grad_mode_forward_and_uncovered_rows_are_zero():
    _, m, tpe, offs, T, x, gy = small_problem()
    with torch.no_grad():
        y0 = m(x, tpe, offs)
    assert y0.grad_fn is None and not y0.requires_grad
    y, dx, *_ = run(m, x, tpe, offs, gy)
    assert torch.equal(y0, y)
    covered = torch.zeros(T, dtype=torch.bool, device=DEV)
    for lo, hi in clipped_ranges(tpe.cpu(), offs.cpu(), T):
        covered[lo:hi] = True
    assert (~covered).sum() == 9
    assert torch.count_nonzero(y[~covered]) == 0 and torch.count_nonzero(dx[~covered]) == 0


@pytest.mark.parametrize("requires", [("x",), ("down_lora_A", "down_lora_B"), ("gate_up_lora_B",)])
def test_selective_gradients(requires):
    _, m, tpe, offs, T, x, gy = small_problem()
    full = dict(zip(("x",) + ADAPTERS, run(m, x, tpe, offs, gy)[1:]))
    part = dict(zip(("x",) + ADAPTERS, run(m, x, tpe, offs, gy, requires=requires)[1:]))
    for name in ("x",) + ADAPTERS:
        if name in requires:
            assert torch.equal(part[name], full[name]), name
        else:
            assert part[name] is None, name


def test_nothing_of_shape_T_F_is_saved():
    """The node keeps inputs [T, H], gate_up [T, 2F], U_gu and U_d [T, r]: 4 T (H + 2F + 2r) bytes of float activations
    beyond the parameters, the buffers and the two tables."""
    E, H, F, r = 3, 128, 192, 8
    _, m = ffn_layer(E, H, F, r, seed=9)
    tpe, offs, T = expert_table([20, 0, 30])
    known = {t.data_ptr() for t in itertools.chain(m.parameters(), m.buffers())} | {tpe.data_ptr(), offs.data_ptr()}
    saved = []

    def pack(t):
        saved.append(t)
        return t

    x = torch.randn(T, H, device=DEV, requires_grad=True)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = m(x, tpe, offs)
    acts = {t.data_ptr(): t for t in saved if t.data_ptr() not in known}
    assert all(t.dtype == torch.float32 for t in acts.values())
    assert sum(t.numel() * t.element_size() for t in acts.values()) == 4 * T * (H + 2 * F + 2 * r)
    assert not any(tuple(t.shape) == (T, F) for t in saved)
    y.sum().backward()
    with torch.no_grad(), torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        del saved[:]
        m(x, tpe, offs)
    assert saved == []


def test_unsupported_inputs_raise():
    _, m, tpe, offs, T, x, gy = small_problem()
    with pytest.raises(RuntimeError):
        m(x.half(), tpe, offs)
    with pytest.raises(RuntimeError):
        m(x.cpu(), tpe, offs)
    with pytest.raises(RuntimeError):
        ops().swiglu_backward(torch.randn(4, 64, device=DEV), torch.randn(4, 33, device=DEV))
