"""Grouped NF4 (code-book) experts on the GPU (csrc/fql_gemm_lut4_group.h, csrc/fql_gemm_lut4_bwd.h):
the grouped forward, its gated entry and the grouped input gradient against float64 references built from W_e by the
definition, and ``NF4MoEFFN`` alone and inside ``QuantizedSparseMoEBlock``.  E = 3 with row counts [0, 129, 33]: an empty
expert, one row past the 128-row tile, a partial 32-row block; the second table lists the same segments in reverse order and
leaves a gap of uncovered rows."""
import functools

import pytest
import torch

from glu_reference import KINDS, act_kw, hidden64
from test_gpu_nf4 import _rows, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = [(64, 64), (192, 64), (256, 128)]
NS = [8, 136]
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -23
E, T = 3, 170
TABLES = [([0, 129, 33], [0, 0, 129]), ([0, 129, 33], [5, 38, 0])]           # (counts, offsets); rows 162 .. / 33 .. 37, 167 .. uncovered


def fq():
    import fused_int4_amd
    return fused_int4_amd


def d(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def _experts(K, block, N, exact):
    """(codes [E, N, K/2], absmax [E, N, K/block], code_book, W [E, N, K] float64) on the CPU, test_gpu_nf4's construction per expert."""
    per = [_weights(K, block, N, exact, 20 + e) for e in range(E)]
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), per[0][2], torch.stack([p[3] for p in per])


def _grouped64(rows, W, table, bias=None, transpose=True):
    """rows [T, C] float64 through each expert's W (``transpose``: rows @ W_e.T + bias_e, else rows @ W_e); zeros where uncovered."""
    out = torch.zeros(rows.shape[0], W.shape[1] if transpose else W.shape[2], dtype=torch.float64)
    for e, (cnt, lo) in enumerate(zip(*table)):
        seg = rows[lo:lo + cnt]
        out[lo:lo + cnt] = seg @ W[e].T + (0 if bias is None else bias[e].double()) if transpose else seg @ W[e]
    return out


@pytest.mark.parametrize("table", TABLES, ids=["in_order", "reversed_with_gap"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_exact_integers_bit_for_bit(K, block, N, dt, table):
    codes, absmax, book, W = _experts(K, block, N, True)
    x, gy = _rows(T, K, True, 2), _rows(T, N, True, 3)
    bias = torch.arange(E * N, dtype=torch.float32).reshape(E, N) - 3
    ref, dref = _grouped64(x.double(), W, table, bias), _grouped64(gy.double(), W, table, transpose=False)
    for r, m in ((ref, _grouped64(x.double().abs(), W.abs(), table, bias.abs())), (dref, _grouped64(gy.double().abs(), W.abs(), table, transpose=False))):
        assert bool((r * 4 == (r * 4).round()).all()) and float(m.max()) * 4 < 2 ** 24   # multiples of 2^-2, far below 2^24
    c, a, b, k = d(codes), d(absmax), d(bias), d(book)
    xs, gs = d(x.to(dt)), d(gy.to(dt))
    tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in table)
    out = torch.full((T, N), float("nan"), dtype=dt, device=DEV)               # the results start as NaN patterns
    dx = torch.full((T, K), float("nan"), dtype=dt, device=DEV)
    L, _native, I = fq()._native.lib(), fq()._native, {torch.float32: 0, torch.bfloat16: 2}[dt]
    st = torch.cuda.current_stream().cuda_stream
    _native.check(L.fql_moe_lut4_fwd(c.data_ptr(), a.data_ptr(), k.data_ptr(), block, xs.data_ptr(), I, b.data_ptr(), tpe.data_ptr(),
                                     offs.data_ptr(), out.data_ptr(), I, E, T, K, N, st), "fwd")
    _native.check(L.fql_moe_lut4_bwd_input(c.data_ptr(), a.data_ptr(), k.data_ptr(), block, gs.data_ptr(), I, tpe.data_ptr(),
                                           offs.data_ptr(), dx.data_ptr(), I, E, T, K, N, st), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.float().to(dt))                          # (the exact value, rounded once; zeros where uncovered)
    assert torch.equal(dx.cpu(), dref.float().to(dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_nf4_gaussian_equals_dense_and_within_the_float32_bound(K, block, N, dt):
    """The grouped result on an expert's rows is the dense op's on that expert's slices, bit for bit; and
    |got - ref| <= L 2^-23 sum |products| (+ 2^-8 |ref| for a bfloat16 result), as test_gpu_nf4."""
    ops = fq().ops
    codes, absmax, _, W = _experts(K, block, N, False)
    x, gy = _rows(T, K, False, 5).bfloat16(), _rows(T, N, False, 6).bfloat16()
    c, a, xs, gs = d(codes), d(absmax), d(x.to(dt)), d(gy.to(dt))
    worst = 0.0
    for table in TABLES:
        tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in table)
        out = ops.moe_forward_lut4(c, a, xs, tpe, offs, block=block)
        dx = ops.moe_backward_input_lut4(c, a, gs, tpe, offs, block=block, out_dtype=dt)
        assert out.dtype == dt and dx.dtype == dt
        for e, (cnt, lo) in enumerate(zip(*table)):
            if cnt:
                assert torch.equal(out[lo:lo + cnt], ops.linear_forward_lut4(c[e], a[e], xs[lo:lo + cnt], block=block)), e
                assert torch.equal(dx[lo:lo + cnt], ops.linear_backward_input_lut4(c[e], a[e], gs[lo:lo + cnt], block=block, out_dtype=dt)), e
        ref, dref = _grouped64(x.double(), W, table), _grouped64(gy.double(), W, table, transpose=False)
        bound = K * U * _grouped64(x.double().abs(), W.abs(), table)
        dbound = N * U * _grouped64(gy.double().abs(), W.abs(), table, transpose=False)
        if dt == torch.bfloat16:
            bound, dbound = bound + 2.0 ** -8 * ref.abs(), dbound + 2.0 ** -8 * dref.abs()
        for got, r, b in ((out.cpu(), ref, bound), (dx.cpu(), dref, dbound)):
            err = (got.double() - r).abs()
            worst = max(worst, float((err / b.clamp_min(1e-300))[b > 0].max()))
            assert bool((err <= b).all())                                      # (b == 0: an uncovered row, exactly zero)
    print(f"K={K} N={N} {dt}: largest |err| / bound = {worst:.4f}")
    one = ops.moe_forward_lut4(c[1:2], a[1:2], xs, None, None, block=block)    # E == 1 without a table: all rows
    assert torch.equal(one, ops.linear_forward_lut4(c[1], a[1], xs, block=block))
    assert torch.equal(ops.moe_backward_input_lut4(c[1:2], a[1:2], gs, None, None, block=block),
                       ops.linear_backward_input_lut4(c[1], a[1], gs, block=block))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["silu"] + KINDS)
def test_gated_entry(kind, dt):
    """Against the float64 product of bf16(hidden64(gate_up)).  The bound is the plain one plus 2^-7 sum |h W|: the device's
    float32 h rounds to the reference's bfloat16 value or to its neighbour, one unit in the 8-bit significand."""
    K, block, N = 192, 64, 136
    codes, absmax, _, W = _experts(K, block, N, False)
    gu = (_rows(T, 2 * K, False, 7) * 2).to(dt)
    h = hidden64(kind, gu).bfloat16().double()
    for table in TABLES:
        tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in table)
        out = fq().ops.moe_gated_forward_lut4(d(codes), d(absmax), d(gu), tpe, offs, block=block, **act_kw(kind)).cpu()
        ref, mag = _grouped64(h, W, table), _grouped64(h.abs(), W.abs(), table)
        bound = (K * U + 2.0 ** -7) * mag + (2.0 ** -8 * ref.abs() if dt == torch.bfloat16 else 0)
        err = (out.double() - ref).abs()
        print(f"{kind} {dt}: largest |err| / bound = {float((err / bound.clamp_min(1e-300))[bound > 0].max()):.4f}")
        assert out.dtype == dt and bool((err <= bound).all())


def test_one_non_finite_element_makes_exactly_its_row_nan():
    K, block, N = 192, 64, 136
    ops = fq().ops
    codes, absmax, _, _ = _experts(K, block, N, False)
    tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in TABLES[1])
    x, gy = _rows(T, K, False, 9), _rows(T, N, False, 10)
    run = lambda a, b: (ops.moe_forward_lut4(d(codes), d(absmax), d(a), tpe, offs, block=block).cpu(),
                        ops.moe_backward_input_lut4(d(codes), d(absmax), d(b), tpe, offs, block=block).cpu())
    clean = run(x, gy)
    xb, gb = x.clone(), gy.clone()
    xb[40, 191], gb[40, 0] = float("nan"), float("-inf")                      # row 40: expert 1's third row
    bad = torch.zeros(T, dtype=torch.bool)
    bad[40] = True
    for got, want in zip(run(xb, gb), clean):
        assert bool(got[bad].isnan().all()) and torch.equal(got[~bad], want[~bad])


def test_layer_forward_and_input_gradient_are_the_ops_composed():
    ops, H, F = fq().ops, 128, 64
    g = torch.Generator().manual_seed(11)
    gate, up, down = ([torch.randn(*s, generator=g) * 0.05 for _ in range(E)] for s in ((F, H), (F, H), (H, F)))
    bg, bu, bd = ([torch.randn(s, generator=g) for _ in range(E)] for s in (F, F, H))
    m = fq().NF4MoEFFN.from_weights(gate, up, down, bg, bu, bd, activation="gelu_tanh", input_grad=True).to(DEV)
    tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in TABLES[1])
    x, gy = d(_rows(T, H, False, 12)).requires_grad_(True), d(_rows(T, H, False, 13))
    y = m(x, tpe, offs)
    gu = ops.moe_forward_lut4(m.gate_up_codes, m.gate_up_absmax, x.detach(), tpe, offs, bias=m.gate_up_bias.detach())
    want = ops.moe_gated_forward_lut4(m.down_codes, m.down_absmax, gu, tpe, offs, activation="gelu_tanh", bias=m.down_bias.detach())
    assert torch.equal(y.detach(), want)
    y.backward(gy)
    dh = ops.moe_backward_input_lut4(m.down_codes, m.down_absmax, gy, tpe, offs)
    dgu = ops.glu_backward(gu, dh, *m.activation_args, out_dtype=torch.float32)
    assert torch.equal(x.grad, ops.moe_backward_input_lut4(m.gate_up_codes, m.gate_up_absmax, dgu, tpe, offs))
    with pytest.raises(RuntimeError, match="inference-only"):
        fq().NF4MoEFFN(E, H, F).to(DEV)(x, tpe, offs)


def test_block_with_nf4_experts_against_per_expert_nf4_linear_layers():
    """E = 4, top-2, H = F = 64, 33 tokens, forward and backward.  The reference runs NF4Linear per expert on each token's
    two experts (gate_up's bits are the grouped kernel's by the contract; h is formed in torch float32 and rounded to bfloat16
    by the down layer, the device's value or its neighbour) and sums with the block's routing weights: the bound is
    sum_j w_j (F 2^-23 + 2^-7) sum |h W_d| plus 2^-22 sum_j w_j |y_j| for the float32 combine."""
    NE, H, F, Tk = 4, 64, 64, 33
    g = torch.Generator().manual_seed(14)
    gate, up, down = ([torch.randn(*s, generator=g) * 0.1 for _ in range(NE)] for s in ((F, H), (F, H), (H, F)))
    experts = fq().NF4MoEFFN.from_weights(gate, up, down, input_grad=True)
    torch.manual_seed(15)
    blk = fq().QuantizedSparseMoEBlock(NE, H, F, top_k=2, experts=experts).to(DEV)
    x = torch.randn(Tk, H, generator=g).to(DEV).requires_grad_(True)
    out, _ = blk(x)
    out.backward(torch.randn(Tk, H, generator=g).to(DEV))
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(blk.gate.weight.grad).all())
    indices = blk.routing[2].long()
    with torch.no_grad():
        w = torch.softmax(blk.router_logits(x.detach()).float(), dim=-1).gather(1, indices)
        w = (w / w.sum(dim=-1, keepdim=True)).double().cpu()
    NL = fq().NF4Linear
    ref, bound = torch.zeros(Tk, H, dtype=torch.float64), torch.zeros(Tk, H, dtype=torch.float64)
    for e in range(NE):
        lgu = NL.from_bnb(experts.gate_up_codes[e], experts.gate_up_absmax[e]).to(DEV)
        ld = NL.from_bnb(experts.down_codes[e], experts.down_absmax[e]).to(DEV)
        with torch.no_grad():
            gu = lgu(x.detach())
            h = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
            y = ld(h).double().cpu()
        mag = h.bfloat16().double().abs().cpu() @ fq().dequantize_lut4(ld.codes.cpu(), ld.absmax.cpu()).double().abs().T
        for j in range(2):
            we = torch.where(indices[:, j].cpu() == e, w[:, j], torch.zeros(Tk, dtype=torch.float64)).unsqueeze(1)
            ref += we * y
            bound += we * ((F * U + 2.0 ** -7) * mag + 2 * U * y.abs())
    err = (out.detach().double().cpu() - ref).abs()
    print(f"block: largest |err| / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert bool((err <= bound).all())
