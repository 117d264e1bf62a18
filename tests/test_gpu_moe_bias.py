"""Per-expert biases of the grouped INT4 GEMM on the GPU, at the operator boundary (ops.moe_forward / moe_forward_any /
moe_gated_forward with ``bias=``, ops.moe_bias_grad) and, for the footprint of the new kernel, through the C ABI.

Forward: the bias is the epilogue's ``fl32(acc + bias[e][n])``, so a biased call is, bit for bit, the unbiased float32
result plus the bias of the row's expert (rounded once for a 16-bit output), and a row no expert covers is exactly zero.
The tables put 1..3, 5..70, 16..33, 3..129 and 129..131 rows into the experts, so that every tile family the dispatcher
picks for K = 64 adds a bias once (decode tiles, 32- and 64-row skinny tiles, the wide kernel); N = 200 leaves a partial
column tile, K = 34 takes the generic kernel.

moe_bias_grad: against the float64 sum of the widened rows with the bound that holds for ANY float32 summation order,
|got - ref| <= cnt_e * 2^-24 * sum_t |g[t][n]|; plus the promises of include/fql_int4.h that are bitwise."""
import functools

import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import ALPHA, LIMIT, act_kw
from helpers import (BIG, NAN, SENT, Guarded, assert_guards_intact, clipped_ranges, expert_table, fq, guarded_like, misaligned,
                     ops, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, K = 3, 64
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
# counts per expert; every table has a gap of 2 rows in front of expert 1 and one uncovered row at the end
TABLES = {"decode": (1, 2, 3), "empty_first": (0, 5, 70), "mid": (16, 32, 33), "empty_mid": (3, 0, 129), "wide": (129, 130, 131)}


@functools.lru_cache(maxsize=None)
def table(name):
    tpe, offs, T = expert_table(list(TABLES[name]), gaps=[0, 2, 0], tail=1)
    ranges = clipped_ranges(tpe.cpu(), offs.cpu(), T)
    expert_of_row = torch.full((T,), -1, dtype=torch.long)
    for e, (lo, hi) in enumerate(ranges):
        expert_of_row[lo:hi] = e
    assert int((expert_of_row < 0).sum()) == 3                          # the gap and the tail
    return tpe, offs, T, expert_of_row.to(DEV)


@functools.lru_cache(maxsize=None)
def weights(N, k=K):
    torch.manual_seed(N + k)
    q = [fq().quantize_weights(torch.randn(N, k) * 0.05) for _ in range(E)]
    P, S, Z = (torch.stack([t[i] for t in q]).to(DEV) for i in range(3))
    bias = torch.randn(E, N, generator=torch.Generator().manual_seed(7 * N)).to(DEV)
    return P, S, Z, bias


def rows(T, cols, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(T, cols, device=DEV, generator=g) * 2.0).to(dtype)


def expected(base32, bias, expert_of_row, dtype):
    """``dtype(fl32(base + bias[e]))`` on the rows an expert covers, zero elsewhere."""
    covered = expert_of_row >= 0
    want = torch.zeros_like(base32)
    want[covered] = base32[covered] + bias[expert_of_row[covered]]
    return want.to(dtype)


def check(got, want, expert_of_row, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.count_nonzero(got[expert_of_row < 0]) == 0, what + ": a row no expert covers is not zero"
    diff = int((got != want).sum())
    assert same_bits(got, want), f"{what}: {diff} elements differ from the unbiased result plus the bias"


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [96, 200])
@pytest.mark.parametrize("name", list(TABLES))
def test_forward_bias_is_the_unbiased_result_plus_the_bias(name, N, dtype):
    tpe, offs, T, eor = table(name)
    P, S, Z, bias = weights(N)
    x = rows(T, K, dtype, seed=N + T)
    o = ops()
    if dtype == torch.float32:
        base = o.moe_forward(P, S, Z, x, None, tpe, offs)
        got = o.moe_forward(P, S, Z, x, None, tpe, offs, bias=bias)
        assert same_bits(o.moe_forward(P, S, Z, x, None, tpe, offs, bias=None), base)
    else:
        base = o.moe_forward_any(P, S, Z, x, None, tpe, offs, out_dtype=torch.float32)
        got = o.moe_forward_any(P, S, Z, x, None, tpe, offs, bias=bias)
        assert same_bits(o.moe_forward_any(P, S, Z, x, None, tpe, offs, bias=None), o.moe_forward_any(P, S, Z, x, None, tpe, offs))
        # a float32 result from 16-bit rows takes the bias too
        check(o.moe_forward_any(P, S, Z, x, None, tpe, offs, out_dtype=torch.float32, bias=bias),
              expected(base, bias, eor, torch.float32), eor, f"moe_forward_any {name} N={N} {NAME[dtype]} -> f32")
    assert base.dtype == torch.float32
    check(got, expected(base, bias, eor, dtype), eor, f"moe_forward {name} N={N} {NAME[dtype]}")
    assert not same_bits(got.float(), base.to(dtype).float())           # the bias is not dropped


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [96, 200])
@pytest.mark.parametrize("name", ["empty_first", "mid", "empty_mid"])
def test_gated_forward_bias_is_the_unbiased_result_plus_the_bias(name, N, kind, dtype):
    tpe, offs, T, eor = table(name)
    P, S, Z, bias = weights(N)
    gate_up = rows(T, 2 * K, dtype, seed=3 * N + T)
    kw = act_kw(kind, ALPHA, LIMIT)
    o = ops()
    base = o.moe_gated_forward(P, S, Z, gate_up, tpe, offs, out_dtype=torch.float32, **kw)
    got = o.moe_gated_forward(P, S, Z, gate_up, tpe, offs, bias=bias, **kw)
    check(got, expected(base, bias, eor, dtype), eor, f"moe_gated_forward {kind} {name} N={N} {NAME[dtype]}")
    assert same_bits(o.moe_gated_forward(P, S, Z, gate_up, tpe, offs, bias=None, **kw),
                     o.moe_gated_forward(P, S, Z, gate_up, tpe, offs, **kw))
    if dtype != torch.float32:
        check(o.moe_gated_forward(P, S, Z, gate_up, tpe, offs, out_dtype=torch.float32, bias=bias, **kw),
              expected(base, bias, eor, torch.float32), eor, f"moe_gated_forward {kind} {name} N={N} {NAME[dtype]} -> f32")


@pytest.mark.parametrize("name", ["empty_first", "mid"])
def test_forward_bias_generic_kernel(name):
    """K = 34 is not MFMA-eligible: float32 rows take the generic kernel, which indexes the bias per expert too."""
    tpe, offs, T, eor = table(name)
    N, k = 96, 34
    P, S, Z, bias = weights(N, k)
    x = rows(T, k, torch.float32, seed=5)
    base = ops().moe_forward(P, S, Z, x, None, tpe, offs)
    check(ops().moe_forward(P, S, Z, x, None, tpe, offs, bias=bias), expected(base, bias, eor, torch.float32), eor,
          f"generic {name}")
    # 16-bit rows off the MFMA path: torch widens and rounds around the float32 call, the bias inside it
    x16 = x.to(torch.bfloat16)
    base16 = ops().moe_forward(P, S, Z, x16.float(), None, tpe, offs)
    check(ops().moe_forward_any(P, S, Z, x16, None, tpe, offs, bias=bias), expected(base16, bias, eor, torch.bfloat16), eor,
          f"generic bf16 {name}")


def test_forward_bias_argument_checks():
    tpe, offs, T, _ = table("mid")
    P, S, Z, bias = weights(96)
    x = rows(T, K, torch.float32, seed=1)
    for bad in (bias[:2], bias[:, :95], bias.double(), bias.cpu(), bias.reshape(-1)):
        with pytest.raises(RuntimeError):
            ops().moe_forward(P, S, Z, x, None, tpe, offs, bias=bad)
        with pytest.raises(RuntimeError):
            ops().moe_gated_forward(P, S, Z, rows(T, 2 * K, torch.float32, seed=2), tpe, offs, bias=bad)
    with pytest.raises(RuntimeError):                                   # forward-only: no gradient through this op
        ops().moe_gated_forward(P, S, Z, rows(T, 2 * K, torch.float32, seed=2), tpe, offs, bias=bias.clone().requires_grad_())


def test_moe_forward_bias_gradient():
    """_MoEFn: the bias gradient is moe_bias_grad of the incoming gradient, the input gradient is what it was."""
    tpe, offs, T, _ = table("mid")
    P, S, Z, bias = weights(96)
    for dtype in DTYPES:
        x = rows(T, K, dtype, seed=11).requires_grad_()
        b = bias.clone().requires_grad_()
        gy = rows(T, 96, dtype, seed=12)
        y = ops().moe_forward_any(P, S, Z, x, None, tpe, offs, bias=b)
        y.backward(gy)
        assert same_bits(b.grad, ops().moe_bias_grad(gy, E, tpe, offs))
        assert same_bits(x.grad, ops().moe_backward_input(P, S, Z, gy, tpe, offs, out_dtype=dtype))
        # a frozen bias gets no gradient; a bias alone can ask for one
        x2, b2 = x.detach().clone().requires_grad_(), bias.clone()
        ops().moe_forward_any(P, S, Z, x2, None, tpe, offs, bias=b2).backward(gy)
        assert b2.grad is None and same_bits(x2.grad, x.grad)
        b3 = bias.clone().requires_grad_()
        ops().moe_forward_any(P, S, Z, x.detach(), None, tpe, offs, bias=b3).backward(gy)
        assert same_bits(b3.grad, b.grad)


# ---- ops.moe_bias_grad ---------------------------------------------------------------------------------------------------

GRAD_COUNTS = [0, 1, 7, 8, 9, 65]
GRAD_NS = [1, 8, 200, 1001]                    # 8 and 200: 16-byte loads in every type; 1 and 1001: element loads


@functools.lru_cache(maxsize=None)
def grad_table():
    """Counts 0, 1, 7, 8, 9 and 65 in one table, two uncovered rows in front of expert 2, and a last range that says 75
    rows where 65 exist: clipped at T on the device."""
    tpe, offs, T = expert_table(GRAD_COUNTS, gaps=[0, 0, 2, 0, 0, 0])
    tpe = tpe.clone()
    tpe[-1] += 10
    ranges = clipped_ranges(tpe.cpu(), offs.cpu(), T)
    assert [hi - lo for lo, hi in ranges] == GRAD_COUNTS and ranges[-1][1] == T
    return tpe, offs, T, ranges


@functools.lru_cache(maxsize=None)
def grad_problem(N, dtype):
    tpe, offs, T, ranges = grad_table()
    g = rows(T, N, dtype, seed=100 + N)
    ref = torch.zeros(len(ranges), N, dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(ref)
    for e, (lo, hi) in enumerate(ranges):
        ref[e] = g[lo:hi].double().sum(0)
        mag[e] = g[lo:hi].double().abs().sum(0)
    return g, ref, mag


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", GRAD_NS)
def test_bias_grad_against_float64(N, dtype):
    tpe, offs, T, ranges = grad_table()
    g, ref, mag = grad_problem(N, dtype)
    got = ops().moe_bias_grad(g, len(ranges), tpe, offs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ranges), N)
    cnt = torch.tensor([hi - lo for lo, hi in ranges], dtype=torch.float64, device=DEV).reshape(-1, 1)
    err = (got.double() - ref).abs()
    bound = cnt * 2.0 ** -24 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"ERR bias_grad N={N} {NAME[dtype]} max err / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (N, dtype, worst)
    assert torch.count_nonzero(got[0]) == 0                             # the expert without rows: exact zeros
    assert same_bits(got[1], g[ranges[1][0]].float())                   # one row: the row itself
    assert same_bits(got, ops().moe_bias_grad(g, len(ranges), tpe, offs))       # run to run


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", GRAD_NS)
def test_bias_grad_order_depends_on_the_row_count_alone(N, dtype):
    tpe, offs, T, ranges = grad_table()
    g, _, _ = grad_problem(N, dtype)
    got = ops().moe_bias_grad(g, len(ranges), tpe, offs)
    # the experts reordered in the table (the same row sets)
    perm = torch.tensor([4, 0, 5, 2, 1, 3], device=DEV)
    assert same_bits(ops().moe_bias_grad(g, len(ranges), tpe[perm], offs[perm]), got[perm])
    # every expert alone: its rows as one segment without a table, and as the only expert of a one-entry table
    for e, (lo, hi) in enumerate(ranges):
        alone = ops().moe_bias_grad(g[lo:hi].contiguous(), 1)
        assert same_bits(alone[0], got[e]), e
        one = ops().moe_bias_grad(g, 1, tpe[e:e + 1], offs[e:e + 1])
        assert same_bits(one[0], got[e]), e
    # the load width does not enter: a base one element past a 16-byte boundary takes the element path
    assert same_bits(ops().moe_bias_grad(misaligned(g, 1), len(ranges), tpe, offs), got)


def test_bias_grad_null_table_and_empty_calls():
    g = rows(37, 200, torch.float32, seed=9)
    got = ops().moe_bias_grad(g, 1)
    ref = g.double().sum(0)
    assert bool(((got[0].double() - ref).abs() <= 37 * 2.0 ** -24 * g.double().abs().sum(0)).all())
    with pytest.raises(RuntimeError):                                   # no table: one expert only
        ops().moe_bias_grad(g, 2)
    tpe, offs, _ = expert_table([3, 4])
    z = ops().moe_bias_grad(g[:0], 2, tpe, offs)                        # T == 0: every output written, zeros
    assert tuple(z.shape) == (2, 200) and torch.count_nonzero(z) == 0
    assert tuple(ops().moe_bias_grad(g, 0, tpe[:0], offs[:0]).shape) == (0, 200)
    assert tuple(ops().moe_bias_grad(g[:, :0], 2, tpe, offs).shape) == (2, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N,offset", [(200, 16), (200, None), (1001, None), (1, None)])
def test_bias_grad_footprint(N, offset, dtype):
    """The C ABI with every pointer inside a guarded buffer: grad_bias between SENT (and SENT inside before the call: every
    one of the E * N outputs must be written), grad_rows between NaN, the table between BIG.  ``offset`` 16: the interior
    of grad_rows starts on a 16-byte boundary (16-byte loads at N = 200), None: one element past a 256-byte boundary."""
    from fused_int4_amd import _native
    tpe, offs, T, ranges = grad_table()
    n_e = len(ranges)
    g, _, _ = grad_problem(N, dtype)
    want = ops().moe_bias_grad(g, n_e, tpe, offs)
    G = guarded_like("grad_rows", g, NAN, offset=offset)
    Tp = guarded_like("tokens_per_expert", tpe, BIG)
    Of = guarded_like("input_offsets", offs, BIG)
    out = Guarded("grad_bias", n_e * N * 4, torch.float32, SENT, offset=4)
    out.view(torch.float32, n_e, N).fill_(SENT)
    rc = _native.lib().fql_moe_bias_grad(G.ptr, DT[dtype], Tp.ptr, Of.ptr, out.ptr, n_e, T, N,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert_guards_intact(G, Tp, Of, out, what=f"fql_moe_bias_grad N={N} {NAME[dtype]}")
    got = out.view(torch.float32, n_e, N)
    assert same_bits(got, want)
    assert int((got == SENT).sum()) == 0
