"""Low-rank adapters fused into the NVFP4 GEMMs on the GPU: ops.moe_forward_nvfp4_lora / moe_gated_forward_nvfp4_lora /
moe_backward_input_nvfp4_lora and the dense linear_forward_nvfp4_lora / linear_backward_input_nvfp4_lora (the LORA flag of
csrc/fql_gemm_nvfp4.h and csrc/fql_gemm_nvfp4_bwd.h), ops.moe_ffn_lora_forward_nvfp4 / linear_lora_forward_nvfp4, the layers
LoRANVFP4MoEFFN and LoRANVFP4Linear and QuantizedSparseMoEBlock with such experts.

Shapes: K in {32, 64, 96, 128, 288} (one piece, one whole stage, an odd number of stages, an even one, 4.5 stages), N in
{8, 40, 136, 201}, r over all of ops.LORA_RANKS (4: less than one 16-j step; 8: two of a lane's pack4 groups and still less
than a step; 16: exactly one; 32: the early exit after exactly two; 64: all four), (K, N, r) = (608, 40, 32) in the exact and
the zero-adapter test (nine whole stages and a half one, so the adapter stage overwrites an image that a weight stage used
last), three experts of [0, 1, 65] rows (65 crosses a 64-row tile) plus 2 uncovered rows, and E = 1 with one row and no table.

THE DEFINITION the references evaluate in float64, on the bfloat16-rounded operands:
    forward   S  = (sum_k x[t][k] W_e[n][k]) * g_e + sum_j v[t][j] B[e][n][j],   out = S + bias[e][n]
    backward  S' = (sum_n dY[t][n] W_e[n][k]) * g_e + sum_j dv[t][j] A[e][j][k]
The global scale g_e scales the weight term ONLY: a kernel that multiplies the finished accumulator fails the exact tests,
where g is 0.5 and 2 on the experts that have rows.

BOUNDS.  float32 result on Gaussian data, relative Frobenius error against that evaluation: 4 x FWD_MEASURED / BWD_MEASURED
(the project's rule, DESIGN.md sections 35 and 38), and never above depth x 2^-24, the worst case of a float32 sum of that
length (K + r terms in the forward, N + r in the input gradient, which contracts over N), at any shape.  A bfloat16 result adds its one rounding, 2^-9.  The layers' gradients against float64 autograd
(float64 adapters, straight-through across the bfloat16 roundings): section 26's rule, 4 x the measured value capped at 2^-6.

MEASURED (MI355X; printed by the tests with -s): FWD_MEASURED, BWD_MEASURED, LAYER_MEASURED, LINEAR_MEASURED below and
DESIGN.md sections 41 and 42.
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden_autograd
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits
from test_gpu_nvfp4 import BF16_OUT, NARROW, ffn_weights, pack
from test_gpu_nvfp4_bwd import GRAD_CAP, dequantized, grad_bound, ste

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
COUNTS, TAIL = (0, 1, 65), 2
KS, NS, RS = [32, 64, 96, 128, 288], [8, 40, 136, 201], [4, 8, 16, 32, 64]
DEEP = (608, 40, 32)               # nine whole stages and a half one: the adapter stage lands on the image a weight stage used last
SHAPES = [(K, N, r) for K in KS for N in NS for r in RS] + [DEEP]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
KEEP = object()                    # "the problem's own table" (None means no table)

# relative Frobenius error of the float32 result against the float64 definition, the largest value printed on an MI355X over
# the shapes of test_gaussian_data_against_the_definition
FWD_MEASURED = 7.434e-8            # (K = 288, N = 136, r = 64 with the bias; 3.5e-8 .. 7.4e-8 over the eight shapes, both row types;
                                   #  r = 32 at that K, N: 6.11e-8, (96, 40, 8): 4.35e-8)
BWD_MEASURED = 6.284e-8            # (K = 288, N = 136, r = 64; 3.2e-8 .. 6.3e-8 over the eight shapes; r = 32: 5.03e-8, (96, 40, 8): 3.29e-8)
# ... of the layers' results and gradients against float64 autograd, the largest per activation type
LAYER_MEASURED = {torch.float32: 2.757e-3, torch.bfloat16: 3.935e-3}    # (float32: x.grad; bfloat16: y, then x.grad 3.541e-3)
LINEAR_MEASURED = {torch.float32: 1.984e-3, torch.bfloat16: 2.628e-3}   # (y in both; x.grad 1.829e-3 / 2.238e-3, the adapters' 9e-8)


def bound(measured, depth, r):
    """4 x the measured value, which must stay below the worst case of a float32 sum of depth + r terms."""
    b = 4.0 * measured
    assert b <= (depth + r) * 2.0 ** -24, (b, depth, r)
    return b


def per_expert(p, f):
    """[T, .] float64: f(e, o, c) on the rows [o, o + c) of expert e, zero on the rows no expert covers."""
    out = None
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        part = f(e, o, c)
        if out is None:
            out = torch.zeros(p["T"], part.shape[1], dtype=torch.float64)
        out[o:o + c] = part
    return out


@functools.lru_cache(maxsize=None)
def problem(K, N, r, integer=False, counts=COUNTS, tail=TAIL):
    """NVFP4 weights [E, N, K] (random codes, scale bytes 0x30 .. 0x47 = 0.5 .. 3.75) with both directions' operands.
    ``integer``: x / dY and v / dv integers in [-4, 4], B / A in [-2, 2], the bias in [-8, 8], global scales from {0.5, 1, 2}
    (1 on the expert without rows, so the ones with rows have g != 1).  Otherwise Gaussian data, Gaussian-magnitude global
    scales that are no powers of two and adapter matrices sized so that the adapter term is of the base term's size.
    ``ref`` / ``ref_b`` / ``ref_g``: the float64 definition (forward without / with the bias, input gradient); ``base*``: the
    weight terms alone; ``mass*``: the sum of the absolute values of all terms of each output.  Computed once; nobody writes."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    g = torch.Generator().manual_seed(977 * K + 13 * N + r + (1 if integer else 0))
    E = len(counts)
    blocks = pack(torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8))
    scales = torch.randint(NARROW[0], NARROW[1] + 1, (E, N, K // 16), generator=g, dtype=torch.uint8)
    W = dequantize_nvfp4(blocks, scales).double()
    tpe, offs, T = expert_table(list(counts), tail=tail, device="cpu")
    p = dict(E=E, T=T, K=K, N=N, r=r, counts=list(counts), offs=offs)
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        gs = torch.tensor([[1.0, 0.5, 2.0][e % 3] for e in range(E)]) if E > 1 else torch.tensor([0.5])
        x, gy, v, dv = ri(-4, 4, T, K), ri(-4, 4, T, N), ri(-4, 4, T, r), ri(-4, 4, T, r)
        B, A, bias = ri(-2, 2, E, N, r), ri(-2, 2, E, r, K), ri(-8, 8, E, N)
    else:
        rn = lambda *s: torch.randn(*s, generator=g)
        gs = rn(E).abs() + 0.3
        x, gy, v, dv, bias = rn(T, K), rn(T, N), rn(T, r), rn(T, r), rn(E, N)
        wg = [float((W[e] * gs[e]).abs().mean()) for e in range(E)]
        B = torch.stack([rn(N, r) * (wg[e] * (K / r) ** 0.5) for e in range(E)])
        A = torch.stack([rn(r, K) * (wg[e] * (N / r) ** 0.5) for e in range(E)])
    d = lambda t: t.bfloat16().double()
    gd = gs.double()
    base = per_expert(p, lambda e, o, c: (d(x)[o:o + c] @ W[e].T) * gd[e])
    add = per_expert(p, lambda e, o, c: d(v)[o:o + c] @ d(B)[e].T)
    bterm = per_expert(p, lambda e, o, c: bias[e].double().expand(c, N))
    base_g = per_expert(p, lambda e, o, c: (d(gy)[o:o + c] @ W[e]) * gd[e])
    add_g = per_expert(p, lambda e, o, c: d(dv)[o:o + c] @ d(A)[e])
    mass = per_expert(p, lambda e, o, c: (d(x)[o:o + c].abs() @ W[e].abs().T) * gd[e] + d(v)[o:o + c].abs() @ d(B)[e].abs().T
                      + bias[e].abs().double())
    mass_g = per_expert(p, lambda e, o, c: (d(gy)[o:o + c].abs() @ W[e].abs()) * gd[e] + d(dv)[o:o + c].abs() @ d(A)[e].abs())
    dev = lambda t: t.to(DEV)
    p.update(blocks=dev(blocks), scales=dev(scales), gs=dev(gs), x=dev(x), gy=dev(gy), v=dev(v), dv=dev(dv), B=dev(B), A=dev(A),
             bias=dev(bias), tpe=dev(tpe), offs_d=dev(offs), W=W, base=base, ref=base + add, ref_b=base + add + bterm,
             base_g=base_g, ref_g=base_g + add_g, mass=mass, mass_g=mass_g)
    return p


def run_fwd(p, x=None, v=None, B=None, bias=False, out_dtype=None, tpe=KEEP, offs=KEEP, **over):
    return ops().moe_forward_nvfp4_lora(over.get("blocks", p["blocks"]), over.get("scales", p["scales"]), over.get("gs", p["gs"]),
                                        p["x"] if x is None else x, p["v"] if v is None else v, p["B"] if B is None else B,
                                        p["tpe"] if tpe is KEEP else tpe, p["offs_d"] if offs is KEEP else offs,
                                        bias=p["bias"] if bias else None, out_dtype=out_dtype)


def run_bwd(p, gy=None, dv=None, A=None, out_dtype=None, tpe=KEEP, offs=KEEP, **over):
    return ops().moe_backward_input_nvfp4_lora(over.get("blocks", p["blocks"]), over.get("scales", p["scales"]),
                                               over.get("gs", p["gs"]), p["gy"] if gy is None else gy,
                                               p["dv"] if dv is None else dv, p["A"] if A is None else A,
                                               p["tpe"] if tpe is KEEP else tpe, p["offs_d"] if offs is KEEP else offs,
                                               out_dtype=out_dtype)


def base_fwd(p, x, bias, out_dtype):
    return ops().moe_forward_nvfp4(p["blocks"], p["scales"], p["gs"], x, p["tpe"], p["offs_d"], bias=p["bias"] if bias else None,
                                   out_dtype=out_dtype)


def base_bwd(p, gy, out_dtype):
    return ops().moe_backward_input_nvfp4(p["blocks"], p["scales"], p["gs"], gy, p["tpe"], p["offs_d"], out_dtype=out_dtype)


def big(p):
    """(e, o, c) of the expert with the most rows."""
    e = max(range(p["E"]), key=lambda i: p["counts"][i])
    return e, p["offs"].tolist()[e], p["counts"][e]


# ---- the lane map and the place of the global scale, bit for bit

def assert_exactness_condition(p):
    """Every term is a multiple of 2^-6 (integer x code/2 x scale/16 x g >= 1/2) and the sum of the absolute values of all
    terms of one output stays below 2^18: granularity x mass < 2^24, so a float32 sum is exact in any order."""
    for ref, mass in ((p["ref_b"], p["mass"]), (p["ref_g"], p["mass_g"])):
        assert torch.equal(ref * 64, (ref * 64).round())
        assert 64.0 * float(mass.max()) < 2.0 ** 24
    assert not torch.equal(p["ref"], p["base"]) and not torch.equal(p["ref_g"], p["base_g"])


def test_every_accepted_rank_is_tested():
    assert tuple(RS) == tuple(ops().LORA_RANKS)                                      # a rank added later cannot go untested


@pytest.mark.parametrize("K,N,r", SHAPES)
def test_exact_on_integer_data_both_directions_plain_gated_and_dense(K, N, r):
    """Integer operands, scale bytes 0x30 .. 0x47, g in {0.5, 2} on the experts with rows, an integer bias: the float32
    result is the float64 definition bit for bit and the bfloat16 result its one rounding.  A swapped row, a wrong j slot, a
    stale weight in the image, a missing zero past r or a global scale applied to the adapter term fails."""
    p = problem(K, N, r, integer=True)
    assert_exactness_condition(p)
    T = p["T"]
    e, o, c = big(p)
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            ref = p["ref_b"] if bias else p["ref"]
            got = run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.float32)
            assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, r, din, bias)
            assert torch.count_nonzero(got[T - TAIL:]) == 0                          # uncovered rows: exactly zero
            got16 = run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16)  # one rounding of the exact value
            assert same_bits(got16.cpu(), ref.float().bfloat16())
        got = run_bwd(p, p["gy"].to(din))
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, K)
        assert torch.equal(got.cpu().double(), p["ref_g"]), (K, N, r, din)
        assert torch.count_nonzero(got[T - TAIL:]) == 0
        assert same_bits(run_bwd(p, p["gy"].to(din), out_dtype=torch.bfloat16).cpu(), p["ref_g"].float().bfloat16())
        # the gated entry: silu(32) = 32 exactly in float32 (the sigmoid is 1), so h = 32 * (x / 32) = x
        gu = torch.cat([torch.full_like(p["x"], 32.0), p["x"] / 32.0], dim=1).to(din)
        got = ops().moe_gated_forward_nvfp4_lora(p["blocks"], p["scales"], p["gs"], gu, p["v"], p["B"], p["tpe"], p["offs_d"],
                                                 bias=p["bias"], out_dtype=torch.float32, **act_kw("silu"))
        assert torch.equal(got.cpu().double(), p["ref_b"]), (K, N, r, din, "gated")
        # the dense entries on the largest expert's slice
        rows = slice(o, o + c)
        got = ops().linear_forward_nvfp4_lora(p["blocks"][e], p["scales"][e], p["gs"][e:e + 1], p["x"][rows].to(din).contiguous(),
                                              p["v"][rows].contiguous(), p["B"][e], bias=p["bias"][e], out_dtype=torch.float32)
        assert torch.equal(got.cpu().double(), p["ref_b"][rows]), (K, N, r, din, "dense")
        got = ops().linear_backward_input_nvfp4_lora(p["blocks"][e], p["scales"][e], p["gs"][e:e + 1],
                                                     p["gy"][rows].to(din).contiguous(), p["dv"][rows].contiguous(), p["A"][e])
        assert torch.equal(got.cpu().double(), p["ref_g"][rows]), (K, N, r, din, "dense bwd")


@pytest.mark.parametrize("r", RS)
def test_exact_one_expert_one_row_no_table(r):
    p = problem(96, 40, r, integer=True, counts=(1,), tail=0)
    assert_exactness_condition(p)
    assert torch.equal(run_fwd(p, bias=True, out_dtype=torch.float32).cpu().double(), p["ref_b"])
    assert torch.equal(run_fwd(p, bias=True, out_dtype=torch.float32, tpe=None, offs=None).cpu().double(), p["ref_b"])
    assert torch.equal(run_bwd(p).cpu().double(), p["ref_g"])
    assert torch.equal(run_bwd(p, tpe=None, offs=None).cpu().double(), p["ref_g"])
    none = run_fwd(p, out_dtype=torch.float32, gs=None)                              # no global scale: g = 1
    assert torch.equal(none.cpu().double(), (p["base"] / 0.5) + (p["ref"] - p["base"]))


# ---- a zero adapter is no adapter

@pytest.mark.parametrize("K,N,r", SHAPES)
def test_zero_adapter_gives_the_base_ops_bits(K, N, r):
    """Gaussian data, global scales that are no powers of two, a Gaussian bias: with B = 0 / A = 0 every entry returns the
    base op's result (torch.equal: the only possible difference is the sign of a zero under a negative global scale, and
    these are positive), plain, gated, input gradient and dense."""
    p = problem(K, N, r)
    g = torch.Generator().manual_seed(K + N)
    gate_up = (torch.randn(p["T"], 2 * K, generator=g) * 2.0).to(DEV)
    B0, A0 = torch.zeros_like(p["B"]), torch.zeros_like(p["A"])
    e, o, c = big(p)
    rows = slice(o, o + c)
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            assert torch.equal(run_fwd(p, p["x"].to(din), B=B0, bias=True, out_dtype=dout), base_fwd(p, p["x"].to(din), True, dout))
            got = ops().moe_gated_forward_nvfp4_lora(p["blocks"], p["scales"], p["gs"], gate_up.to(din), p["v"], B0, p["tpe"],
                                                     p["offs_d"], bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp"))
            assert torch.equal(got, ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], gate_up.to(din), p["tpe"],
                                                                  p["offs_d"], bias=p["bias"], out_dtype=dout,
                                                                  **act_kw("swiglu_clamp")))
            assert torch.equal(run_bwd(p, p["gy"].to(din), A=A0, out_dtype=dout), base_bwd(p, p["gy"].to(din), dout)), (din, dout)
        w = (p["blocks"][e], p["scales"][e], p["gs"][e:e + 1])
        x1, gy1 = p["x"][rows].to(din).contiguous(), p["gy"][rows].to(din).contiguous()
        got = ops().linear_forward_nvfp4_lora(*w, x1, p["v"][rows].contiguous(), B0[e], bias=p["bias"][e])
        assert torch.equal(got, ops().linear_forward_nvfp4(*w, x1, bias=p["bias"][e]))
        got = ops().linear_backward_input_nvfp4_lora(*w, gy1, p["dv"][rows].contiguous(), A0[e])
        assert torch.equal(got, ops().linear_backward_input_nvfp4(*w, gy1))


# ---- the gated entry

def own_hidden(gate_up, kind, tpe, offs, E):
    """The base gated op's own h [T, F] bfloat16: the op on unit weights (code 2 = 1.0 on the diagonal, scale byte 0x38 = 1,
    no global scale) returns h[t][n] * 1 plus exact zeros.  Rows no expert covers come back zero."""
    F = gate_up.shape[1] // 2
    codes = torch.zeros(E, F, F, dtype=torch.uint8)
    codes[:, torch.arange(F), torch.arange(F)] = 2
    blocks, scales = pack(codes).to(DEV), torch.full((E, F, F // 16), 0x38, dtype=torch.uint8, device=DEV)
    h = ops().moe_gated_forward_nvfp4(blocks, scales, None, gate_up, tpe, offs, out_dtype=torch.float32, **act_kw(kind))
    assert torch.equal(h, h.bfloat16().float())
    return h.bfloat16()


@pytest.mark.parametrize("kind", KINDS)
def test_gated_forward_is_the_plain_entry_on_the_gated_ops_own_h(kind):
    K, N, r = 96, 136, 16
    p = problem(K, N, r)
    g = torch.Generator().manual_seed(len(kind))
    gate_up = (torch.randn(p["T"], 2 * K, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        gu = gate_up.to(din)
        h = own_hidden(gu, kind, p["tpe"], p["offs_d"], p["E"])
        for dout in (torch.float32, torch.bfloat16):
            got = ops().moe_gated_forward_nvfp4_lora(p["blocks"], p["scales"], p["gs"], gu, p["v"], p["B"], p["tpe"], p["offs_d"],
                                                     bias=p["bias"], out_dtype=dout, **act_kw(kind))
            assert same_bits(got, run_fwd(p, h, bias=True, out_dtype=dout)), (kind, din, dout)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0


# ---- independence, bit for bit

@pytest.mark.parametrize("K,N,r", [(288, 136, 64), (96, 201, 4)])
def test_grouped_equals_one_expert_calls_and_other_experts_operands_do_not_matter(K, N, r):
    p = problem(K, N, r)
    got, gotb = run_fwd(p, bias=True), run_bwd(p)
    assert same_bits(got, run_fwd(p, bias=True)) and same_bits(gotb, run_bwd(p))     # two runs agree
    one_t = lambda c: (torch.tensor([c], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        w = (p["blocks"][e:e + 1], p["scales"][e:e + 1], p["gs"][e:e + 1])
        one = ops().moe_forward_nvfp4_lora(*w, p["x"][o:o + c].contiguous(), p["v"][o:o + c].contiguous(), p["B"][e:e + 1],
                                           *one_t(c), bias=p["bias"][e:e + 1])
        assert same_bits(one, got[o:o + c]), e
        one = ops().moe_backward_input_nvfp4_lora(*w, p["gy"][o:o + c].contiguous(), p["dv"][o:o + c].contiguous(),
                                                  p["A"][e:e + 1], *one_t(c))
        assert same_bits(one, gotb[o:o + c]), e
    perm = torch.tensor([2, 0, 1], device=DEV)                                       # the table in another order
    again = ops().moe_forward_nvfp4_lora(p["blocks"][perm], p["scales"][perm], p["gs"][perm], p["x"], p["v"], p["B"][perm],
                                         p["tpe"][perm], p["offs_d"][perm], bias=p["bias"][perm])
    assert same_bits(again, got)
    again = ops().moe_backward_input_nvfp4_lora(p["blocks"][perm], p["scales"][perm], p["gs"][perm], p["gy"], p["dv"],
                                                p["A"][perm], p["tpe"][perm], p["offs_d"][perm])
    assert same_bits(again, gotb)
    # everything of expert 1 (its row of x, v, its B, A, g) replaced: expert 2's rows keep their bits
    o1, o2, c2 = p["offs"].tolist()[1], p["offs"].tolist()[2], p["counts"][2]
    x, v, gy, dv, B, A, gs = (p[k].clone() for k in ("x", "v", "gy", "dv", "B", "A", "gs"))
    for t in (x, v, gy, dv):
        t[o1] = 3.0
    B[1], A[1], gs[1] = 1.0, -1.0, 7.0
    moved, movedb = run_fwd(p, x, v, B, bias=True, gs=gs), run_bwd(p, gy, dv, A, gs=gs)
    assert same_bits(moved[o2:o2 + c2], got[o2:o2 + c2]) and not same_bits(moved[o1], got[o1])
    assert same_bits(movedb[o2:o2 + c2], gotb[o2:o2 + c2]) and not same_bits(movedb[o1], gotb[o1])


# ---- accuracy on Gaussian data

@pytest.mark.parametrize("K,N,r", [(288, 136, 64), (288, 201, 16), (128, 136, 16), (96, 40, 4), (64, 8, 16), (32, 8, 64),
                                   (288, 136, 32), (96, 40, 8)])
def test_gaussian_data_against_the_definition(K, N, r):
    p = problem(K, N, r)
    assert rel_fro_dev(p["base"], p["ref"]) > 0.1 and rel_fro_dev(p["base_g"], p["ref_g"]) > 0.1   # the adapter term matters
    b, bb = bound(FWD_MEASURED, K, r), bound(BWD_MEASURED, N, r)                     # (the gradient contracts over N)
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            ref = p["ref_b"] if bias else p["ref"]
            e32 = rel_fro_dev(run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.float32), ref)
            e16 = rel_fro_dev(run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16), ref)
            print(f"nvfp4 lora fwd K={K} N={N} r={r} in={din} bias={bias}: rel_fro f32 out {e32:.3e} (bound {b:.3e}), "
                  f"bf16 out {e16:.3e} (bound {b + BF16_OUT:.3e})")
            assert e32 <= b and e16 <= b + BF16_OUT
        e32 = rel_fro_dev(run_bwd(p, p["gy"].to(din)), p["ref_g"])
        e16 = rel_fro_dev(run_bwd(p, p["gy"].to(din), out_dtype=torch.bfloat16), p["ref_g"])
        print(f"nvfp4 lora bwd K={K} N={N} r={r} in={din}: rel_fro f32 out {e32:.3e} (bound {bb:.3e}), "
              f"bf16 out {e16:.3e} (bound {bb + BF16_OUT:.3e})")
        assert e32 <= bb and e16 <= bb + BF16_OUT


# ---- non-finite values

@pytest.mark.parametrize("r", [4, 32, 64])
def test_inf_and_nan_shrunk_rows_are_nan_across_exactly_their_rows(r):
    p = problem(288, 136, r)
    t_inf = p["offs"].tolist()[2] + 40                                               # a row of the second 32-row wave
    t_nan = p["offs"].tolist()[2] + 64                                               # the row behind the 64-row tile
    for run, name in ((run_fwd, "v"), (run_bwd, "dv")):
        v = p[name].clone()
        v[t_inf, r - 1] = float("inf")
        v[t_nan, 0] = NAN
        got, want = run(p, **{name: v}), run(p)
        nan = torch.isnan(got)
        expect = torch.zeros_like(nan)
        expect[t_inf] = True
        expect[t_nan] = True
        assert torch.equal(nan, expect), name
        assert same_bits(got[~expect], want[~expect]), name


@pytest.mark.parametrize("K,N", [(288, 136), (128, 201)])
def test_nan_scale_byte_in_the_last_weight_stage_is_not_laundered(K, N):
    """Byte 0x7F in the last stage of the weights (the image the adapter stage overwrites next): the forward is NaN in
    exactly that weight row's column on the rows of its expert, the input gradient in exactly the 16 k of the block."""
    p = problem(K, N, 16)
    e, o, c = big(p)
    n, kb = N - 3, K // 16 - 1                                                       # the last 16 k: the last forward stage
    scales = p["scales"].clone()
    scales[e, n, kb] = 0x7F
    got, want = run_fwd(p, bias=True, scales=scales), run_fwd(p, bias=True)
    expect = torch.zeros_like(got, dtype=torch.bool)
    expect[o:o + c, n] = True
    assert torch.equal(torch.isnan(got), expect) and same_bits(got[~expect], want[~expect])
    n = N - 1                                                                        # the last n: the last stage of the gradient
    scales = p["scales"].clone()
    scales[e, n, 1] = 0x7F
    got, want = run_bwd(p, scales=scales), run_bwd(p)
    expect = torch.zeros_like(got, dtype=torch.bool)
    expect[o:o + c, 16:32] = True
    assert torch.equal(torch.isnan(got), expect) and same_bits(got[~expect], want[~expect])


# ---- guard bands

@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("off", [16, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("N,r", [(40, 4), (201, 4), (40, 32), (201, 32)], ids=["40", "201", "40-r32", "201-r32"])
def test_entries_stay_inside_their_buffers(N, r, off, dout):
    """K = 96, r = 4 or 32 (a lane's second 32-j half of B is then zeros, not a fetch of the next row or of the guard), a
    table whose last count leaves [0, T) and is clipped on the device.  Every pointer is the interior of a guarded buffer: SENT around the results, NaN around v, B and A, which end flush against their guard, so a read of
    v[t][j >= r], of a B row past N or of an A row past r would fetch NaN and show in the values; a write outside the result
    changes a guard.  ``off``: the adapter operands 16-byte aligned (the wide loads) or 4 bytes off (the element loads).  The
    gated entry runs on a stale workspace.  By construction the kernels' clamps keep every access inside: nothing is provoked,
    the results are the public ops' and the guards stay."""
    from fused_int4_amd import _native
    lib = _native.lib()
    K = 96
    p = problem(K, N, r)
    E, T = p["E"], p["T"]
    tpe = p["tpe"].clone()
    tpe[-1] += TAIL + 7                                                              # clipped to T on the device
    st = torch.cuda.current_stream().cuda_stream
    esz = 4 if dout == torch.float32 else 2
    cnt, offs = guarded_like("tokens_per_expert", tpe, 0x7F7F7F7F), guarded_like("input_offsets", p["offs_d"], 0x7F7F7F7F)
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    gs, bias = guarded_like("global_scale", p["gs"], NAN, offset=4), guarded_like("bias", p["bias"], NAN)
    rw, v, B = guarded_like("rows", p["x"], NAN, offset=16), guarded_like("v", p["v"], NAN, offset=off), guarded_like("B", p["B"], NAN, offset=off)
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert v.ptr % 16 == off % 16 and B.ptr % 16 == off % 16 and out.ptr % 16 == 4
    rc = lib.fql_moe_nvfp4_lora_fwd(bl.ptr, sc.ptr, gs.ptr, rw.ptr, 0, v.ptr, B.ptr, r, bias.ptr, cnt.ptr, offs.ptr, out.ptr,
                                    DT[dout], E, T, K, N, None, 0, st)
    assert rc == 0
    assert_guards_intact(bl, sc, gs, rw, v, B, bias, cnt, offs, out, what=f"nvfp4 lora fwd {dout} off={off}")
    want = run_fwd(p, bias=True, out_dtype=dout, tpe=tpe)
    assert same_bits(out.view(dout, T, N), want) and not bool(torch.isnan(want).any())
    # gated forward, a stale workspace
    g = torch.Generator().manual_seed(3)
    gate_up = torch.randn(T, 2 * K, generator=g).to(DEV)
    gu = guarded_like("gate_up", gate_up, NAN, offset=16)
    nbytes = lib.fql_moe_nvfp4_workspace_bytes(E, T, K, N, 1)
    ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
    ws.bytes().fill_(0xFF)                                                           # stale NaNs as bfloat16
    out.view(dout, T, N).fill_(SENT)
    rc = lib.fql_moe_nvfp4_glu_lora_fwd(bl.ptr, sc.ptr, gs.ptr, gu.ptr, 0, v.ptr, B.ptr, r, bias.ptr, cnt.ptr, offs.ptr, out.ptr,
                                        DT[dout], E, T, K, N, ACT["swiglu_clamp"], ALPHA, LIMIT, ws.ptr, nbytes, st)
    assert rc == 0
    assert_guards_intact(bl, sc, gs, gu, v, B, bias, cnt, offs, out, ws, what=f"nvfp4 lora glu fwd {dout} off={off}")
    want = ops().moe_gated_forward_nvfp4_lora(p["blocks"], p["scales"], p["gs"], gate_up, p["v"], p["B"], tpe, p["offs_d"],
                                              bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp"))
    assert same_bits(out.view(dout, T, N), want) and not bool(torch.isnan(want).any())
    # input gradient
    gy, dv, A = guarded_like("grad_out", p["gy"], NAN, offset=4), guarded_like("dv", p["dv"], NAN, offset=off), guarded_like("A", p["A"], NAN, offset=off)
    gx = Guarded("grad_in", T * K * esz, dout, SENT, offset=4)
    gx.view(dout, T, K).fill_(SENT)
    rc = lib.fql_moe_nvfp4_lora_bwd_input(bl.ptr, sc.ptr, gs.ptr, gy.ptr, 0, dv.ptr, A.ptr, r, cnt.ptr, offs.ptr, gx.ptr, DT[dout],
                                          E, T, K, N, st)
    assert rc == 0
    assert_guards_intact(bl, sc, gs, gy, dv, A, cnt, offs, gx, what=f"nvfp4 lora bwd {dout} off={off}")
    want = run_bwd(p, out_dtype=dout, tpe=tpe)
    assert same_bits(gx.view(dout, T, K), want) and not bool(torch.isnan(want).any())
    # the dense entries: expert 2's matrices, all T rows
    e = 2
    b1, s1 = guarded_like("blocks", p["blocks"][e], 0xFF, offset=16), guarded_like("scales", p["scales"][e], 0xFF, offset=1)
    g1, bi1 = guarded_like("global_scale", p["gs"][e:e + 1], NAN, offset=4), guarded_like("bias", p["bias"][e], NAN)
    B1, A1 = guarded_like("B", p["B"][e], NAN, offset=off), guarded_like("A", p["A"][e], NAN, offset=off)
    out.view(dout, T, N).fill_(SENT)
    rc = lib.fql_linear_nvfp4_lora_fwd(b1.ptr, s1.ptr, g1.ptr, rw.ptr, 0, v.ptr, B1.ptr, r, bi1.ptr, out.ptr, DT[dout], T, K, N,
                                       None, 0, st)
    assert rc == 0
    assert_guards_intact(b1, s1, g1, rw, v, B1, bi1, out, what=f"nvfp4 lora linear fwd {dout} off={off}")
    want = ops().linear_forward_nvfp4_lora(p["blocks"][e], p["scales"][e], p["gs"][e:e + 1], p["x"], p["v"], p["B"][e],
                                           bias=p["bias"][e], out_dtype=dout)
    assert same_bits(out.view(dout, T, N), want) and not bool(torch.isnan(want).any())
    gx.view(dout, T, K).fill_(SENT)
    rc = lib.fql_linear_nvfp4_lora_bwd_input(b1.ptr, s1.ptr, g1.ptr, gy.ptr, 0, dv.ptr, A1.ptr, r, gx.ptr, DT[dout], T, K, N, st)
    assert rc == 0
    assert_guards_intact(b1, s1, g1, gy, dv, A1, gx, what=f"nvfp4 lora linear bwd {dout} off={off}")
    want = ops().linear_backward_input_nvfp4_lora(p["blocks"][e], p["scales"][e], p["gs"][e:e + 1], p["gy"], p["dv"], p["A"][e],
                                                  out_dtype=dout)
    assert same_bits(gx.view(dout, T, K), want) and not bool(torch.isnan(want).any())


# ---- the layers

E_L, H_L, F_L, R_L = 4, 64, 96, 8
KIND = "swiglu_clamp"
NAMES = ["gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"]


def make_layers(dt, seed=5, randomise=True, E=E_L, F=F_L):
    """(the wrapped NVFP4MoEFFN with input_grad=True, the LoRANVFP4MoEFFN on its buffers); ``randomise``: B != 0."""
    w = ffn_weights(E, H_L, F, seed=seed)
    base = fq().NVFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                         down_bias=w["down_bias"], activation_dtype=dt, input_grad=True, **act_kw(KIND)).to(DEV)
    torch.manual_seed(seed + 1)                                                      # (the adapters' A)
    m = fq().LoRANVFP4MoEFFN.from_layer(base, R_L, alpha=2.0 * R_L)
    if randomise:
        g = torch.Generator().manual_seed(seed + 2)
        with torch.no_grad():
            m.gate_up_lora_B.copy_((torch.randn(m.gate_up_lora_B.shape, generator=g) * 0.2).to(DEV))
            m.down_lora_B.copy_((torch.randn(m.down_lora_B.shape, generator=g) * 0.2).to(DEV))
    return base, m


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fresh_layers_equal_the_layers_they_wrap(dt):
    base, m = make_layers(dt, randomise=False)
    assert all(p.is_cuda for p in m.parameters()) and torch.count_nonzero(m.gate_up_lora_A) > 0
    assert not torch.equal(m.gate_up_global, torch.ones_like(m.gate_up_global))      # (the global scales are in play)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H_L, device=DEV).to(dt)
    with torch.no_grad():
        want = base(x, tpe, offs)
        assert torch.equal(m(x, tpe, offs), want)
    y = m(x, tpe, offs)                                                              # under grad mode: the same bits
    assert y.requires_grad and y.dtype == dt and torch.equal(y.detach(), want)
    lin = fq().NVFP4Linear.from_linear(torch.nn.Linear(96, 40)).to(DEV)
    lora = fq().LoRANVFP4Linear.from_layer(lin, 8)
    assert lora.lora_A.is_cuda and lora.blocks.data_ptr() == lin.blocks.data_ptr()
    x = torch.randn(2, 3, 96, device=DEV).to(dt)
    y = lora(x)
    assert y.shape == (2, 3, 40) and y.requires_grad and y.dtype == dt and torch.equal(y.detach(), lin(x))


def adapter_rows64(Wgu, Wd, bgu, bd, ad, s, rows, counts, offsets):
    """The experts' output [T, H] in float64 (a graph) with float64 adapters ``ad`` = (A_gu, B_gu, A_d, B_d): x and h pass
    a straight-through rounding to bfloat16 into the base products, the adapter path is plain float64."""
    F, H = Wd.shape[2], Wd.shape[1]
    A_gu, B_gu, A_d, B_d = ad
    pieces, pos = [], 0
    for e, (c, o) in enumerate(zip(counts, offsets)):
        if c == 0:
            continue
        assert o >= pos
        pieces.append(torch.zeros(o - pos, H, dtype=torch.float64))
        x = rows[o:o + c]
        gu = ste(x) @ Wgu[e].T + bgu[e] + s * (x @ A_gu[e].T) @ B_gu[e].T
        h = hidden_autograd(KIND, gu[:, :F], gu[:, F:], ALPHA, LIMIT)
        pieces.append(ste(h) @ Wd[e].T + bd[e] + s * (h @ A_d[e].T) @ B_d[e].T)
        pos = o + c
    pieces.append(torch.zeros(rows.shape[0] - pos, H, dtype=torch.float64))
    return torch.cat(pieces)


def hand_composition(m, x, gy, tpe, offs, dt):
    """The layer's forward and backward from the ops, one launch a line: (y, grads by name)."""
    o, s, E = ops(), m.scaling, m.num_experts
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach() for n in NAMES)
    b_gu, b_d = m.gate_up_bias.detach(), m.down_bias.detach()
    wgu, wd = (m.gate_up_blocks, m.gate_up_scales, m.gate_up_global), (m.down_blocks, m.down_scales, m.down_global)
    kw = act_kw(KIND)
    v_gu = o.lora_shrink(x, A_gu, "rc", tpe, offs, scale=s)
    gate_up = o.moe_forward_nvfp4_lora(*wgu, x, v_gu, B_gu, tpe, offs, bias=b_gu, out_dtype=dt)
    v_d = o.lora_gated_shrink(gate_up, A_d, "rc", tpe, offs, scale=s, **kw)
    y = o.moe_gated_forward_nvfp4_lora(*wd, gate_up, v_d, B_d, tpe, offs, bias=b_d, out_dtype=dt, **kw)
    g = {}
    g["down_lora_B"] = o.lora_grad(gy, v_d, "cr", E, tpe, offs)
    g["down_bias"] = o.moe_bias_grad(gy, E, tpe, offs)
    dv_d = o.lora_shrink(gy, B_d, "cr", tpe, offs, scale=s)
    g["down_lora_A"] = o.lora_gated_grad(gate_up, dv_d, "rc", E, tpe, offs, **kw)
    dh = o.moe_backward_input_nvfp4_lora(*wd, gy, dv_d, A_d, tpe, offs, out_dtype=dt)
    dgu = o.glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
    g["gate_up_lora_B"] = o.lora_grad(dgu, v_gu, "cr", E, tpe, offs)
    g["gate_up_bias"] = o.moe_bias_grad(dgu, E, tpe, offs)
    dv_gu = o.lora_shrink(dgu, B_gu, "cr", tpe, offs, scale=s)
    g["x"] = o.moe_backward_input_nvfp4_lora(*wgu, dgu, dv_gu, A_gu, tpe, offs, out_dtype=dt)
    g["gate_up_lora_A"] = o.lora_grad(x, dv_gu, "rc", E, tpe, offs)
    return y, g


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_gradients_are_the_ops_composed_and_match_float64_autograd(dt):
    _, m = make_layers(dt)
    m.gate_up_bias.requires_grad_(True)
    m.down_bias.requires_grad_(True)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(T, H_L, generator=g).to(DEV).to(dt).requires_grad_(True)
    gy = torch.randn(T, H_L, generator=g).to(DEV).to(dt)
    y = m(x, tpe, offs)
    assert y.dtype == dt and y.requires_grad
    y.backward(gy)
    got = dict(x=x.grad, gate_up_bias=m.gate_up_bias.grad, down_bias=m.down_bias.grad, **{n: getattr(m, n).grad for n in NAMES})
    # (a) the hand composition, bit for bit
    want_y, want = hand_composition(m, x.detach(), gy, tpe, offs, dt)
    assert same_bits(y.detach(), want_y)
    for k, v in got.items():
        assert v is not None and v.dtype == (dt if k == "x" else torch.float32), k
        assert same_bits(v, want[k]), k
    assert torch.count_nonzero(x.grad[T - 2:]) == 0                                  # rows no expert covers
    with torch.no_grad():
        assert same_bits(m(x.detach(), tpe, offs), want_y)                           # without a graph: the same bits
    # (b) float64 autograd on dequantize_nvfp4(...) * global_scale, float64 adapters
    Wgu, Wd = dequantized(m)
    leaf = lambda t: t.detach().cpu().double().requires_grad_(True)
    x64, bgu, bd = leaf(x), leaf(m.gate_up_bias), leaf(m.down_bias)
    ad = [leaf(getattr(m, n)) for n in NAMES]
    ref_y = adapter_rows64(Wgu, Wd, bgu, bd, ad, m.scaling, x64, tpe.tolist(), offs.tolist())
    base_y = adapter_rows64(Wgu, Wd, bgu, bd, [torch.zeros_like(a) for a in ad], m.scaling, x64, tpe.tolist(), offs.tolist())
    assert rel_fro_dev(base_y.detach(), ref_y.detach()) > 5e-2                       # the adapter moves y by more than 5 %
    ref_y.backward(gy.detach().cpu().double())
    ref = dict(x=x64.grad, gate_up_bias=bgu.grad, down_bias=bd.grad, **{n: a.grad for n, a in zip(NAMES, ad)})
    errs = {k: rel_fro_dev(got[k], ref[k]) for k in got}
    b = grad_bound(LAYER_MEASURED[dt])
    print(f"nvfp4 lora layer {dt}: forward rel_fro {rel_fro_dev(y.detach(), ref_y.detach()):.3e}; gradients against float64 "
          "autograd " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {b:.3e})")
    assert b <= GRAD_CAP and rel_fro_dev(y.detach(), ref_y.detach()) <= b
    for k, v in errs.items():
        assert v <= b, k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_linear_layer_gradients_are_the_ops_composed_and_match_float64_autograd(dt):
    """K = 96, N = 40, r = 8, leading dimensions (2, 3), a bias."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    torch.manual_seed(3)
    m = fq().LoRANVFP4Linear.from_linear(torch.nn.Linear(96, 40), rank=8, alpha=16.0).to(DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        m.lora_B.copy_((torch.randn(40, 8, generator=g) * 0.2).to(DEV))
    x = torch.randn(2, 3, 96, generator=g).to(DEV).to(dt).requires_grad_(True)
    gy = torch.randn(2, 3, 40, generator=g).to(DEV).to(dt)
    y = m(x)
    assert y.shape == (2, 3, 40) and y.dtype == dt
    y.backward(gy)
    # (a) the ops composed by hand
    o, s = ops(), m.scaling
    x2, g2, A, B = x.detach().reshape(6, 96), gy.reshape(6, 40), m.lora_A.detach(), m.lora_B.detach()
    w = (m.blocks, m.scales, m.global_scale)
    v = o.lora_shrink(x2, A, "rc", scale=s)
    assert same_bits(y.detach().reshape(6, 40), o.linear_forward_nvfp4_lora(*w, x2, v, B, bias=m.bias, out_dtype=dt))
    dv = o.lora_shrink(g2, B, "cr", scale=s)
    assert same_bits(m.lora_B.grad, o.lora_grad(g2, v, "cr")[0]) and same_bits(m.lora_A.grad, o.lora_grad(x2, dv, "rc")[0])
    assert x.grad.shape == (2, 3, 96) and x.grad.dtype == dt
    assert same_bits(x.grad.reshape(6, 96), o.linear_backward_input_nvfp4_lora(*w, g2, dv, A, out_dtype=dt))
    # (b) float64 autograd
    W = dequantize_nvfp4(m.blocks.cpu(), m.scales.cpu()).double() * m.global_scale.cpu().double()
    leaf = lambda t: t.detach().cpu().double().requires_grad_(True)
    x64, A64, B64 = leaf(x2), leaf(A), leaf(B)
    ref_y = ste(x64) @ W.T + m.bias.cpu().double() + s * (x64 @ A64.T) @ B64.T
    assert rel_fro_dev((ste(x64) @ W.T + m.bias.cpu().double()).detach(), ref_y.detach()) > 5e-2
    ref_y.backward(g2.cpu().double())
    errs = dict(y=rel_fro_dev(y.detach().reshape(6, 40), ref_y.detach()), x=rel_fro_dev(x.grad.reshape(6, 96), x64.grad),
                lora_A=rel_fro_dev(m.lora_A.grad, A64.grad), lora_B=rel_fro_dev(m.lora_B.grad, B64.grad))
    b = grad_bound(LINEAR_MEASURED[dt])
    print(f"nvfp4 lora linear {dt}: against float64 autograd " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
          + f" (bound {b:.3e})")
    assert b <= GRAD_CAP
    for k, e in errs.items():
        assert e <= b, k


COUNTED = ("lora_shrink", "lora_grad", "_lora_grad", "moe_bias_grad", "_glu_backward", "moe_backward_input_nvfp4_lora",
           "linear_backward_input_nvfp4_lora")


@pytest.fixture
def calls(monkeypatch):
    """Counts the launches of the backward's ops (looked up in the ops module when the nodes run)."""
    n = {}
    for name in COUNTED:
        real = getattr(ops(), name)

        def spy(*a, _real=real, _name=name, **kw):
            n[_name] = n.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops(), name, spy)
    return n


def test_only_what_requires_grad_gets_a_gradient_and_the_other_launches_are_skipped(calls):
    _, m = make_layers(torch.float32)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    g = torch.Generator().manual_seed(22)
    x, gy = torch.randn(T, H_L, generator=g).to(DEV), torch.randn(T, H_L, generator=g).to(DEV)
    for n in NAMES[:3]:
        getattr(m, n).requires_grad_(False)
    y = m(x, tpe, offs)                                                              # down_lora_B alone
    calls.clear()
    y.backward(gy)
    assert m.down_lora_B.grad is not None and all(getattr(m, n).grad is None for n in NAMES[:3])
    assert m.gate_up_bias.grad is None and m.down_bias.grad is None and x.grad is None
    assert calls == {"lora_grad": 1, "_lora_grad": 1}, calls                         # dB_d (lora_grad is _lora_grad) and nothing else
    m.down_lora_B.requires_grad_(False)
    m.down_lora_A.requires_grad_(True)                                               # dA_d alone: dv_d and the gated grad
    y = m(x, tpe, offs)
    calls.clear()
    y.backward(gy)
    assert calls == {"lora_shrink": 1, "_lora_grad": 1}, calls
    m.down_lora_A.requires_grad_(False)
    m.gate_up_bias.requires_grad_(True)                                              # db_gu alone: through h, no dx, no dv_gu
    y = m(x, tpe, offs)
    calls.clear()
    y.backward(gy)
    assert calls == {"lora_shrink": 1, "moe_backward_input_nvfp4_lora": 1, "_glu_backward": 1, "moe_bias_grad": 1}, calls
    m.gate_up_bias.requires_grad_(False)
    assert not m(x, tpe, offs).requires_grad                                         # nothing wants a gradient: the plain ops
    with pytest.raises(RuntimeError, match="activation_dtype"):
        m(x.bfloat16(), tpe, offs)
    # the dense layer: lora_B alone, then x alone
    lin = fq().LoRANVFP4Linear.from_linear(torch.nn.Linear(96, 40), rank=8).to(DEV)
    lin.lora_A.requires_grad_(False)
    x1, g1 = torch.randn(6, 96, generator=g).to(DEV), torch.randn(6, 40, generator=g).to(DEV)
    y = lin(x1)
    calls.clear()
    y.backward(g1)
    assert lin.lora_B.grad is not None and lin.lora_A.grad is None and calls == {"lora_grad": 1, "_lora_grad": 1}, calls
    lin.lora_B.requires_grad_(False)
    x1.requires_grad_(True)
    y = lin(x1)
    calls.clear()
    y.backward(g1)
    assert x1.grad is not None and calls == {"lora_shrink": 1, "linear_backward_input_nvfp4_lora": 1}, calls


def test_bfloat16_layer_makes_no_float32_wide_tensor_and_saves_nothing_of_ffn_width(monkeypatch):
    """Every [T, .] tensor of the ops comes from torch.empty / torch.zeros in ops.py: with bfloat16 activations none of
    width H or more is float32, forward or backward, and the node saves x, gate_up and the two [T, r] shrunk rows."""
    _, m = make_layers(torch.bfloat16)
    m.gate_up_bias.requires_grad_(True)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H_L, device=DEV).bfloat16().requires_grad_(True)
    gy = torch.randn(T, H_L, device=DEV).bfloat16()
    made = []
    for name in ("empty", "zeros"):
        real = getattr(torch, name)

        def spy(*args, _real=real, **kw):
            out = _real(*args, **kw)
            made.append((tuple(out.shape), out.dtype))
            return out
        monkeypatch.setattr(torch, name, spy)
    y = m(x, tpe, offs)
    y.backward(gy)
    monkeypatch.undo()
    wide = [(s, d) for s, d in made if len(s) == 2 and s[0] == T and s[1] >= H_L]
    assert len(wide) >= 5 and all(d == torch.bfloat16 for _, d in wide), wide           # gate_up, y, dh, dgu, dx
    assert sorted(s for s, d in made if d == torch.float32 and len(s) == 2 and s[0] == T) == [(T, R_L)] * 4   # v_gu, v_d, dv_d, dv_gu
    y2 = m(x, tpe, offs)                                                             # (a graph that is still alive)
    saved = [tuple(t.shape) for t in y2.grad_fn.saved_tensors if t is not None and t.dim() == 2 and t.shape[0] == T]
    assert sorted(saved) == sorted([(T, H_L), (T, 2 * F_L), (T, R_L), (T, R_L)])
    assert not any(F_L in s for s in saved)


# ---- the block

@pytest.mark.parametrize("shared", [False, True], ids=["routed", "shared"])
def test_block_trains_the_adapters_through_the_router_in_one_optimiser_step(shared):
    """QuantizedSparseMoEBlock(experts=LoRANVFP4MoEFFN, top_k=2, T=50), with or without an NVFP4 LoRA shared expert: one SGD
    step on the adapters (the gate has its gradient too, but stays, so the routing does) lowers the loss, and the NVFP4
    buffers keep their bits."""
    T, top_k = 50, 2
    _, experts = make_layers(torch.float32, seed=9)
    sh = make_layers(torch.float32, seed=10, E=1, F=32)[1] if shared else None
    torch.manual_seed(13)                                                            # (the gate's initial weights)
    blk = fq().QuantizedSparseMoEBlock(E_L, H_L, F_L, top_k=top_k, experts=experts, shared_experts=sh, router_bias=True).to(DEV)
    assert blk.experts is experts and (not shared or blk.shared_experts is sh)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H_L, generator=g).to(DEV)
    target = torch.randn(T, H_L, generator=g).to(DEV)
    before = {n: b.clone() for n, b in blk.named_buffers()}
    params = [p for n, p in blk.named_parameters() if p.requires_grad and "lora" in n]
    assert len(params) == (8 if shared else 4) and sum(p is q for p in params for q in experts.parameters()) == 4
    opt = torch.optim.SGD(params, lr=0.2)
    loss = lambda: ((blk(x)[0] - target) ** 2).mean()
    first = loss()
    first.backward()
    for n in NAMES:
        v = getattr(experts, n).grad
        assert v is not None and bool(torch.isfinite(v).all()) and torch.count_nonzero(v) > 0, n
        if shared:
            v = getattr(sh, n).grad
            assert v is not None and bool(torch.isfinite(v).all()) and torch.count_nonzero(v) > 0, n
    assert blk.gate.weight.grad is not None and torch.count_nonzero(blk.gate.weight.grad) > 0
    opt.step()
    with torch.no_grad():
        second = loss()
    print(f"nvfp4 lora block shared={shared}: loss {first.item():.6f} -> {second.item():.6f}")
    assert second.item() < first.item()
    for n, b in blk.named_buffers():
        assert not b.requires_grad and b.grad is None and same_bits(b, before[n]), n
