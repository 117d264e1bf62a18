"""Low-rank adapters fused into the MXFP4 GEMMs on the GPU: ops.moe_forward_mxfp4_lora / moe_gated_forward_mxfp4_lora /
moe_backward_input_mxfp4_lora (the LORA flag of csrc/fql_gemm_mx4.h and csrc/fql_gemm_mx4_bwd.h), ops.moe_ffn_lora_forward_mxfp4,
the layer LoRAMXFP4MoEFFN and QuantizedSparseMoEBlock with such experts.

Shapes: K in {32, 96, 288} and N in {8, 40, 136, 201} as in tests/test_gpu_mxfp4.py and tests/test_gpu_mxfp4_bwd.py (N = 201:
an odd width, the element stores), r over all of ops.LORA_RANKS (4: less than one 16-j step; 8: two of a lane's pack4 groups
and still less than a step; 16: exactly one; 32: the early exit after exactly two; 64: all four), section 25's table of
[0, 1, 33, 70] rows plus 2 uncovered, and E = 1 with one row and no table.

BOUNDS.  The float32 result against the float64 product of the same bfloat16-rounded operands: section 25 asserts 2.64e-7 for
contractions of up to 288 terms (test_gpu_mxfp4.SAME_INPUT_BOUND).  The adapter stage adds r terms to the same float32
accumulation on the same instruction, and the worst-case error of a float32 sum grows linearly with its length, so the bound
here is 2.64e-7 * (K + r) / 288 where K + r exceeds 288 (3.23e-7 at K = 288, r = 64) and 2.64e-7 below.  A 16-bit result
adds its one rounding, 2^-9.  The layer's gradients against float64 autograd (float64 adapters, straight-through across the
bfloat16 roundings): section 26's rule, 4 x the measured value capped at 2^-6; the error is the operands' bfloat16 roundings,
about 2^-9 an element.

MEASURED (MI355X; printed by the tests with -s): see LAYER_MEASURED below and DESIGN.md section 35.
"""
import functools

import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden_autograd
from helpers import NAN, SENT, Guarded, assert_guards_intact, expert_table, fq, guarded_like, ops, rel_fro_dev, same_bits
import test_gpu_mxfp4 as fwd_t
import test_gpu_mxfp4_bwd as bwd_t
from test_gpu_mxfp4 import BF16_OUT, SAME_INPUT_BOUND, ffn_weights
from test_gpu_mxfp4_bwd import GRAD_CAP, grad_bound, ste

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
TAIL = 2
KS, NS, RS = [32, 96, 288], [8, 40, 136, 201], [4, 8, 16, 32, 64]
KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]
KEEP = object()                    # "the problem's own table" (None means no table)

# relative Frobenius error of the layer's gradients against float64 autograd, the largest of x.grad, the four adapter
# gradients and the two bias gradients printed on an MI355X, per activation type
LAYER_MEASURED = {torch.float32: 2.753e-3, torch.bfloat16: 3.687e-3}    # (x.grad in both; the others are below it)


def bound(K, r):
    """Section 25's bound for a float32 accumulation of K + r terms (the module docstring)."""
    return SAME_INPUT_BOUND * max(1.0, (K + r) / 288.0)


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
def fwd_problem(K, N, r, integer=False, counts=(0, 1, 33, 70), tail=TAIL):
    """test_gpu_mxfp4.problem plus the adapter operands: v [T, r] and B [E, N, r], integers in [-4, 4] / [-2, 2] (exact in
    bfloat16) or Gaussian.  ``ref`` / ``ref_b``: the float64 sum of both products on the bfloat16-rounded operands."""
    p = dict(fwd_t.problem(K, N, counts=counts, tail=tail, lo=125 if integer else 97, hi=129 if integer else 157, integer=integer))
    g = torch.Generator().manual_seed(7 * K + 3 * N + r)
    if integer:
        v, B = torch.randint(-4, 5, (p["T"], r), generator=g).float(), torch.randint(-2, 3, (p["E"], N, r), generator=g).float()
    else:
        v = torch.randn(p["T"], r, generator=g)                    # B sized so that the adapter term is of the base term's size
        B = torch.randn(p["E"], N, r, generator=g) * (float(p["ref"].abs().mean()) / r ** 0.5)
    vr, Br = v.bfloat16().double(), B.bfloat16().double()
    add = per_expert(p, lambda e, o, c: vr[o:o + c] @ Br[e].T)
    p.update(r=r, v=v.to(DEV), B=B.to(DEV), base=p["ref"], ref=p["ref"] + add, ref_b=p["ref_b"] + add)
    return p


@functools.lru_cache(maxsize=None)
def bwd_problem(K, N, r, integer=False, counts=(0, 1, 33, 70), tail=TAIL):
    """test_gpu_mxfp4_bwd.problem plus dv [T, r] and A [E, r, K]."""
    p = dict(bwd_t.problem(K, N, counts=counts, tail=tail, lo=125 if integer else 97, hi=129 if integer else 157, integer=integer))
    g = torch.Generator().manual_seed(11 * K + 5 * N + r)
    if integer:
        dv, A = torch.randint(-4, 5, (p["T"], r), generator=g).float(), torch.randint(-2, 3, (p["E"], r, K), generator=g).float()
    else:
        dv = torch.randn(p["T"], r, generator=g)                   # A sized so that the adapter term is of the base term's size
        A = torch.randn(p["E"], r, K, generator=g) * (float(p["ref"].abs().mean()) / r ** 0.5)
    vr, Ar = dv.bfloat16().double(), A.bfloat16().double()
    p.update(r=r, dv=dv.to(DEV), A=A.to(DEV), base=p["ref"], ref=p["ref"] + per_expert(p, lambda e, o, c: vr[o:o + c] @ Ar[e]))
    return p


def run_fwd(p, x=None, v=None, B=None, bias=False, out_dtype=None, tpe=KEEP, offs=KEEP):
    return ops().moe_forward_mxfp4_lora(p["blocks"], p["scales"], p["x"] if x is None else x, p["v"] if v is None else v,
                                        p["B"] if B is None else B, p["tpe"] if tpe is KEEP else tpe,
                                        p["offs"] if offs is KEEP else offs, bias=p["bias"] if bias else None, out_dtype=out_dtype)


def run_bwd(p, gy=None, dv=None, A=None, out_dtype=None, tpe=KEEP, offs=KEEP):
    return ops().moe_backward_input_mxfp4_lora(p["blocks"], p["scales"], p["gy"] if gy is None else gy,
                                               p["dv"] if dv is None else dv, p["A"] if A is None else A,
                                               p["tpe"] if tpe is KEEP else tpe, p["offs"] if offs is KEEP else offs,
                                               out_dtype=out_dtype)


# ---- the lane map, bit for bit

def test_every_accepted_rank_is_tested():
    assert tuple(RS) == tuple(ops().LORA_RANKS)                                      # a rank added later cannot go untested


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_forward_exact_on_integer_data(K, N, r):
    """Integer x in [-4, 4], v in [-4, 4] and B in [-2, 2], scale codes in [125, 129]: every product is a multiple of 2^-3
    and every partial sum is below 2^15 + 2^9, so the float32 result is the integer reference bit for bit.  B and v are
    asymmetric: a swapped row, a wrong j slot, a stale weight in the image or a missing zero past r fails."""
    p = fwd_problem(K, N, r, integer=True)
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            ref = p["ref_b"] if bias else p["ref"]
            assert float(ref.abs().max()) < 2 ** 16 and not torch.equal(ref, p["base"])
            got = run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.float32)
            assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), ref), (K, N, r, din, bias)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0                     # uncovered rows: exactly zero
            got16 = run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16)  # one rounding of the exact value
            assert same_bits(got16.cpu(), ref.float().bfloat16())


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_backward_exact_on_integer_data(K, N, r):
    """The same for the transposed kernel with integer dY, dv and A: the swizzled image, the store rotation and the
    transposed read of the adapter stage."""
    p = bwd_problem(K, N, r, integer=True)
    ref = p["ref"]
    assert float(ref.abs().max()) < 2 ** 16 and not torch.equal(ref, p["base"])
    for din in (torch.float32, torch.bfloat16):
        got = run_bwd(p, p["gy"].to(din))
        assert got.dtype == torch.float32 and tuple(got.shape) == (p["T"], K)
        assert torch.equal(got.cpu().double(), ref), (K, N, r, din)
        assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0
        got16 = run_bwd(p, p["gy"].to(din), out_dtype=torch.bfloat16)
        assert same_bits(got16.cpu(), ref.float().bfloat16())


@pytest.mark.parametrize("r", RS)
def test_exact_one_expert_one_row_no_table(r):
    p = fwd_problem(96, 40, r, integer=True, counts=(1,), tail=0)
    assert torch.equal(run_fwd(p, out_dtype=torch.float32).cpu().double(), p["ref"])
    assert torch.equal(run_fwd(p, out_dtype=torch.float32, tpe=None, offs=None).cpu().double(), p["ref"])
    q = bwd_problem(96, 40, r, integer=True, counts=(1,), tail=0)
    assert torch.equal(run_bwd(q).cpu().double(), q["ref"])
    assert torch.equal(run_bwd(q, tpe=None, offs=None).cpu().double(), q["ref"])


def own_hidden(gate_up, kind, tpe, offs, E):
    """The base gated op's own h [T, F] bfloat16: the op on unit weights (code 2 = 1.0 on the diagonal, scale code 127)
    returns h[t][n] * 1 plus exact zeros.  Rows no expert covers come back zero."""
    F = gate_up.shape[1] // 2
    codes = torch.zeros(E, F, F, dtype=torch.uint8)
    codes[:, torch.arange(F), torch.arange(F)] = 2
    blocks, scales = fwd_t.pack(codes).to(DEV), torch.full((E, F, F // 32), 127, dtype=torch.uint8, device=DEV)
    h = ops().moe_gated_forward_mxfp4(blocks, scales, gate_up, tpe, offs, out_dtype=torch.float32, **act_kw(kind))
    assert torch.equal(h, h.bfloat16().float())
    return h.bfloat16()


@pytest.mark.parametrize("kind", KINDS)
def test_gated_forward_is_the_plain_entry_on_the_gated_ops_own_h(kind):
    """One shape per activation kind: the gated adapter entry equals the plain adapter entry (exact above) on the bfloat16 h
    that the base gated op itself forms, bit for bit, for both row types, both result types and with the bias."""
    K, N, r = 96, 136, 16
    p = fwd_problem(K, N, r)
    g = torch.Generator().manual_seed(len(kind))
    gate_up = (torch.randn(p["T"], 2 * K, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        gu = gate_up.to(din)
        h = own_hidden(gu, kind, p["tpe"], p["offs"], p["E"])
        for dout in (torch.float32, torch.bfloat16):
            got = ops().moe_gated_forward_mxfp4_lora(p["blocks"], p["scales"], gu, p["v"], p["B"], p["tpe"], p["offs"],
                                                     bias=p["bias"], out_dtype=dout, **act_kw(kind))
            assert same_bits(got, run_fwd(p, h, bias=True, out_dtype=dout)), (kind, din, dout)
            assert torch.count_nonzero(got[p["T"] - TAIL:]) == 0


# ---- a zero adapter is no adapter

@pytest.mark.parametrize("K,N,r", [(288, 136, 64), (96, 201, 4), (32, 8, 16)])
def test_zero_adapter_gives_the_base_ops_bits(K, N, r):
    p, q = fwd_problem(K, N, r), bwd_problem(K, N, r)
    g = torch.Generator().manual_seed(K + N)
    gate_up = (torch.randn(p["T"], 2 * K, generator=g) * 2.0).to(DEV)
    for din in (torch.float32, torch.bfloat16):
        for dout in (torch.float32, torch.bfloat16):
            got = run_fwd(p, p["x"].to(din), B=torch.zeros_like(p["B"]), bias=True, out_dtype=dout)
            assert torch.equal(got, fwd_t.run(p, p["x"].to(din), bias=True, out_dtype=dout)), (din, dout)
            got = ops().moe_gated_forward_mxfp4_lora(p["blocks"], p["scales"], gate_up.to(din), p["v"], torch.zeros_like(p["B"]),
                                                     p["tpe"], p["offs"], bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp"))
            assert torch.equal(got, ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gate_up.to(din), p["tpe"], p["offs"],
                                                                  bias=p["bias"], out_dtype=dout, **act_kw("swiglu_clamp")))
            got = run_bwd(q, q["gy"].to(din), A=torch.zeros_like(q["A"]), out_dtype=dout)
            assert torch.equal(got, bwd_t.run(q, q["gy"].to(din), out_dtype=dout)), (din, dout)


E_L, H_L, F_L, R_L = 4, 64, 96, 8
KIND = "swiglu_clamp"


def make_layers(dt, seed=5, randomise=True):
    """(the wrapped MXFP4MoEFFN with input_grad=True, the LoRAMXFP4MoEFFN on its buffers); ``randomise``: B != 0."""
    w = ffn_weights(E_L, H_L, F_L, seed=seed)
    base = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gate_bias"], up_bias=w["up_bias"],
                                         down_bias=w["down_bias"], activation_dtype=dt, input_grad=True, **act_kw(KIND)).to(DEV)
    torch.manual_seed(seed + 1)                                                      # (the adapters' A)
    m = fq().LoRAMXFP4MoEFFN.from_layer(base, R_L, alpha=2.0 * R_L)
    if randomise:
        g = torch.Generator().manual_seed(seed + 2)
        with torch.no_grad():
            m.gate_up_lora_B.copy_((torch.randn(m.gate_up_lora_B.shape, generator=g) * 0.2).to(DEV))
            m.down_lora_B.copy_((torch.randn(m.down_lora_B.shape, generator=g) * 0.2).to(DEV))
    return base, m


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fresh_layer_equals_the_layer_it_wraps(dt):
    base, m = make_layers(dt, randomise=False)
    assert all(p.is_cuda for p in m.parameters()) and torch.count_nonzero(m.gate_up_lora_A) > 0
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    x = torch.randn(T, H_L, device=DEV).to(dt)
    with torch.no_grad():
        want = base(x, tpe, offs)
        assert torch.equal(m(x, tpe, offs), want)
    y = m(x, tpe, offs)                                                              # under grad mode: the same bits
    assert y.requires_grad and y.dtype == dt and torch.equal(y.detach(), want)


# ---- independence, bit for bit

@pytest.mark.parametrize("K,N,r", [(288, 136, 64), (96, 201, 4)])
def test_grouped_equals_one_expert_calls_and_other_experts_rows_do_not_matter(K, N, r):
    p, q = fwd_problem(K, N, r), bwd_problem(K, N, r)
    got, gotb = run_fwd(p, bias=True), run_bwd(q)
    assert same_bits(got, run_fwd(p, bias=True)) and same_bits(gotb, run_bwd(q))     # two runs agree
    one_t = lambda c: (torch.tensor([c], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    for e, (c, o) in enumerate(zip(p["counts"], p["offs"].tolist())):
        if c == 0:
            continue
        one = ops().moe_forward_mxfp4_lora(p["blocks"][e:e + 1], p["scales"][e:e + 1], p["x"][o:o + c].contiguous(),
                                           p["v"][o:o + c].contiguous(), p["B"][e:e + 1], *one_t(c), bias=p["bias"][e:e + 1])
        assert same_bits(one, got[o:o + c]), e
        one = ops().moe_backward_input_mxfp4_lora(q["blocks"][e:e + 1], q["scales"][e:e + 1], q["gy"][o:o + c].contiguous(),
                                                  q["dv"][o:o + c].contiguous(), q["A"][e:e + 1], *one_t(c))
        assert same_bits(one, gotb[o:o + c]), e
    perm = torch.tensor([2, 0, 3, 1], device=DEV)                                    # the table in another order
    again = ops().moe_forward_mxfp4_lora(p["blocks"][perm], p["scales"][perm], p["x"], p["v"], p["B"][perm], p["tpe"][perm],
                                         p["offs"][perm], bias=p["bias"][perm])
    assert same_bits(again, got)
    again = ops().moe_backward_input_mxfp4_lora(q["blocks"][perm], q["scales"][perm], q["gy"], q["dv"], q["A"][perm],
                                                q["tpe"][perm], q["offs"][perm])
    assert same_bits(again, gotb)
    # the rows of expert 3 permuted among themselves (and everything outside expert 2's range replaced): expert 2's rows stay
    o2, c2 = p["offs"].tolist()[2], p["counts"][2]
    o3, c3 = p["offs"].tolist()[3], p["counts"][3]
    idx = torch.arange(p["T"], device=DEV)
    idx[o3:o3 + c3] = o3 + torch.randperm(c3, generator=torch.Generator().manual_seed(1)).to(DEV)
    moved = run_fwd(p, p["x"][idx].contiguous(), p["v"][idx].contiguous(), bias=True)
    assert same_bits(moved[o2:o2 + c2], got[o2:o2 + c2]) and same_bits(moved, got[idx])
    movedb = run_bwd(q, q["gy"][idx].contiguous(), q["dv"][idx].contiguous())
    assert same_bits(movedb[o2:o2 + c2], gotb[o2:o2 + c2]) and same_bits(movedb, gotb[idx])


# ---- accuracy on Gaussian data

@pytest.mark.parametrize("K,N,r", [(288, 136, 64), (288, 201, 16), (96, 40, 4), (32, 8, 64), (288, 136, 32), (96, 40, 8)])
def test_gaussian_data_against_the_same_rounded_operands(K, N, r):
    p, q = fwd_problem(K, N, r), bwd_problem(K, N, r)
    b = bound(K, r)
    assert rel_fro_dev(p["base"], p["ref"]) > 0.1 and rel_fro_dev(q["base"], q["ref"]) > 0.1   # the adapter term matters
    for din in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            ref = p["ref_b"] if bias else p["ref"]
            e32 = rel_fro_dev(run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.float32), ref)
            e16 = rel_fro_dev(run_fwd(p, p["x"].to(din), bias=bias, out_dtype=torch.bfloat16), ref)
            print(f"mxfp4 lora fwd K={K} N={N} r={r} in={din} bias={bias}: rel_fro f32 out {e32:.3e} (bound {b:.3e}), "
                  f"bf16 out {e16:.3e} (bound {b + BF16_OUT:.3e})")
            assert e32 <= b and e16 <= b + BF16_OUT
        bb = bound(N, r)                                                             # the contraction of the gradient is N
        e32 = rel_fro_dev(run_bwd(q, q["gy"].to(din)), q["ref"])
        e16 = rel_fro_dev(run_bwd(q, q["gy"].to(din), out_dtype=torch.bfloat16), q["ref"])
        print(f"mxfp4 lora bwd K={K} N={N} r={r} in={din}: rel_fro f32 out {e32:.3e} (bound {bb:.3e}), "
              f"bf16 out {e16:.3e} (bound {bb + BF16_OUT:.3e})")
        assert e32 <= bb and e16 <= bb + BF16_OUT


# ---- non-finite values

@pytest.mark.parametrize("r", [4, 32, 64])
def test_inf_and_nan_shrunk_rows_are_nan_across_exactly_their_rows(r):
    p, q = fwd_problem(288, 136, r), bwd_problem(288, 136, r)
    t_inf = p["offs"].tolist()[3] + 40                                               # a row of the second 32-row wave
    t_nan = p["offs"].tolist()[2] + 5
    for run, prob, name in ((run_fwd, p, "v"), (run_bwd, q, "dv")):
        v = prob[name].clone()
        v[t_inf, r - 1] = float("inf")
        v[t_nan, 0] = NAN
        got, want = run(prob, **{name: v}), run(prob)
        nan = torch.isnan(got)
        expect = torch.zeros_like(nan)
        expect[t_inf] = True
        expect[t_nan] = True
        assert torch.equal(nan, expect), name
        assert same_bits(got[~expect], want[~expect]), name


# ---- guard bands

@pytest.mark.parametrize("dout", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("off,r", [(16, 4), (4, 4), (16, 32), (4, 32)], ids=["aligned", "off4", "aligned-r32", "off4-r32"])
def test_entries_stay_inside_their_buffers(off, r, dout):
    """N = 201, K = 96, r = 4 or 32 (a lane's second 32-j half of B is then zeros, not a fetch of the next row or of the
    guard), a table whose last count leaves [0, T) and is clipped on the device.  Every pointer is the
    interior of a guarded buffer: SENT around out, NaN around v, B and A, which end flush against their guard (Guarded puts
    the guard right behind the last element), so a read of v[t][16 xq + 15 >= r], of a B row past N or of an A row past r
    would fetch NaN and show in the values; a write outside [T, N] changes a guard.  ``off``: the adapter operands 16-byte
    aligned (the wide loads) or 4 bytes off (the element loads).  By construction the clamps of the kernels keep every
    access inside: this test does not provoke anything, it checks that the result is the public op's and the guards stay."""
    from fused_int4_amd import _native
    lib = _native.lib()
    K, N = 96, 201
    p, q = fwd_problem(K, N, r), bwd_problem(K, N, r)
    E, T = p["E"], p["T"]
    tpe = p["tpe"].clone()
    tpe[-1] += TAIL + 7                                                              # clipped to T on the device
    st = torch.cuda.current_stream().cuda_stream
    esz = 4 if dout == torch.float32 else 2
    cnt, offs = guarded_like("tokens_per_expert", tpe, 0x7F7F7F7F), guarded_like("input_offsets", p["offs"], 0x7F7F7F7F)
    bl, sc = guarded_like("blocks", p["blocks"], 0xFF, offset=16), guarded_like("scales", p["scales"], 0xFF, offset=1)
    bias = guarded_like("bias", p["bias"], NAN)
    # forward
    rw, v, B = guarded_like("rows", p["x"], NAN, offset=16), guarded_like("v", p["v"], NAN, offset=off), guarded_like("B", p["B"], NAN, offset=off)
    out = Guarded("out", T * N * esz, dout, SENT, offset=4)
    out.view(dout, T, N).fill_(SENT)
    assert v.ptr % 16 == off % 16 and B.ptr % 16 == off % 16 and out.ptr % 16 == 4
    rc = lib.fql_moe_mx4_lora_fwd(bl.ptr, sc.ptr, rw.ptr, 0, v.ptr, B.ptr, r, bias.ptr, cnt.ptr, offs.ptr, out.ptr, DT[dout],
                                  E, T, K, N, None, 0, st)
    assert rc == 0
    assert_guards_intact(bl, sc, rw, v, B, bias, cnt, offs, out, what=f"mx4 lora fwd {dout} off={off}")
    want = run_fwd(p, bias=True, out_dtype=dout, tpe=tpe)
    assert same_bits(out.view(dout, T, N), want) and not bool(torch.isnan(want).any())
    # gated forward
    g = torch.Generator().manual_seed(3)
    gate_up = torch.randn(T, 2 * K, generator=g).to(DEV)
    gu = guarded_like("gate_up", gate_up, NAN, offset=16)
    nbytes = lib.fql_moe_mx4_workspace_bytes(E, T, K, N, 1)
    ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
    ws.bytes().fill_(0xFF)                                                           # stale NaNs as bfloat16
    out.view(dout, T, N).fill_(SENT)
    rc = lib.fql_moe_mx4_glu_lora_fwd(bl.ptr, sc.ptr, gu.ptr, 0, v.ptr, B.ptr, r, bias.ptr, cnt.ptr, offs.ptr, out.ptr, DT[dout],
                                      E, T, K, N, ACT[KIND], ALPHA, LIMIT, ws.ptr, nbytes, st)
    assert rc == 0
    assert_guards_intact(bl, sc, gu, v, B, bias, cnt, offs, out, ws, what=f"mx4 lora glu fwd {dout} off={off}")
    want = ops().moe_gated_forward_mxfp4_lora(p["blocks"], p["scales"], gate_up, p["v"], p["B"], tpe, p["offs"], bias=p["bias"],
                                              out_dtype=dout, **act_kw(KIND))
    assert same_bits(out.view(dout, T, N), want) and not bool(torch.isnan(want).any())
    # input gradient
    bl, sc = guarded_like("blocks", q["blocks"], 0xFF, offset=16), guarded_like("scales", q["scales"], 0xFF, offset=1)
    gy, dv, A = guarded_like("grad_out", q["gy"], NAN, offset=4), guarded_like("dv", q["dv"], NAN, offset=off), guarded_like("A", q["A"], NAN, offset=off)
    gx = Guarded("grad_in", T * K * esz, dout, SENT, offset=4)
    gx.view(dout, T, K).fill_(SENT)
    rc = lib.fql_moe_mx4_lora_bwd_input(bl.ptr, sc.ptr, gy.ptr, 0, dv.ptr, A.ptr, r, cnt.ptr, offs.ptr, gx.ptr, DT[dout], E, T, K,
                                        N, st)
    assert rc == 0
    assert_guards_intact(bl, sc, gy, dv, A, cnt, offs, gx, what=f"mx4 lora bwd {dout} off={off}")
    want = run_bwd(q, out_dtype=dout, tpe=tpe)
    assert same_bits(gx.view(dout, T, K), want) and not bool(torch.isnan(want).any())
    # the clipped count covers the tail rows: they belong to the last expert now, and the unclipped rows keep their bits
    assert same_bits(want[:T - TAIL], run_bwd(q, out_dtype=dout)[:T - TAIL])


# ---- the layer's gradients

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


NAMES = ["gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"]


def hand_composition(m, x, gy, tpe, offs, dt):
    """The layer's forward and backward from the ops, one launch a line: (y, grads by name)."""
    o, s, E = ops(), m.scaling, m.num_experts
    A_gu, B_gu, A_d, B_d = (getattr(m, n).detach() for n in NAMES)
    b_gu, b_d = m.gate_up_bias.detach(), m.down_bias.detach()
    kw = act_kw(KIND)
    v_gu = o.lora_shrink(x, A_gu, "rc", tpe, offs, scale=s)
    gate_up = o.moe_forward_mxfp4_lora(m.gate_up_blocks, m.gate_up_scales, x, v_gu, B_gu, tpe, offs, bias=b_gu, out_dtype=dt)
    v_d = o.lora_gated_shrink(gate_up, A_d, "rc", tpe, offs, scale=s, **kw)
    y = o.moe_gated_forward_mxfp4_lora(m.down_blocks, m.down_scales, gate_up, v_d, B_d, tpe, offs, bias=b_d, out_dtype=dt, **kw)
    g = {}
    g["down_lora_B"] = o.lora_grad(gy, v_d, "cr", E, tpe, offs)
    g["down_bias"] = o.moe_bias_grad(gy, E, tpe, offs)
    dv_d = o.lora_shrink(gy, B_d, "cr", tpe, offs, scale=s)
    g["down_lora_A"] = o.lora_gated_grad(gate_up, dv_d, "rc", E, tpe, offs, **kw)
    dh = o.moe_backward_input_mxfp4_lora(m.down_blocks, m.down_scales, gy, dv_d, A_d, tpe, offs, out_dtype=dt)
    dgu = o.glu_backward(gate_up, dh, *m.activation_args, out_dtype=dt)
    g["gate_up_lora_B"] = o.lora_grad(dgu, v_gu, "cr", E, tpe, offs)
    g["gate_up_bias"] = o.moe_bias_grad(dgu, E, tpe, offs)
    dv_gu = o.lora_shrink(dgu, B_gu, "cr", tpe, offs, scale=s)
    g["x"] = o.moe_backward_input_mxfp4_lora(m.gate_up_blocks, m.gate_up_scales, dgu, dv_gu, A_gu, tpe, offs, out_dtype=dt)
    g["gate_up_lora_A"] = o.lora_grad(x, dv_gu, "rc", E, tpe, offs)
    return y, g


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_gradients_are_the_ops_composed_and_match_float64_autograd(dt):
    from fused_int4_amd.quantize import dequantize_mxfp4
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
    # (b) float64 autograd on the dequantised weights, float64 adapters
    Wgu = dequantize_mxfp4(m.gate_up_blocks.cpu(), m.gate_up_scales.cpu()).double()
    Wd = dequantize_mxfp4(m.down_blocks.cpu(), m.down_scales.cpu()).double()
    leaf = lambda t: t.detach().cpu().double().requires_grad_(True)
    x64, bgu, bd = leaf(x), leaf(m.gate_up_bias), leaf(m.down_bias)
    ad = [leaf(getattr(m, n)) for n in NAMES]
    ref_y = adapter_rows64(Wgu, Wd, bgu, bd, ad, m.scaling, x64, tpe.tolist(), offs.tolist())
    base_y = adapter_rows64(Wgu, Wd, bgu, bd, [torch.zeros_like(a) for a in ad], m.scaling, x64, tpe.tolist(), offs.tolist())
    assert rel_fro_dev(base_y.detach(), ref_y.detach()) > 5e-2                       # the adapter matters
    ref_y.backward(gy.detach().cpu().double())
    ref = dict(x=x64.grad, gate_up_bias=bgu.grad, down_bias=bd.grad, **{n: a.grad for n, a in zip(NAMES, ad)})
    errs = {k: rel_fro_dev(got[k], ref[k]) for k in got}
    b = grad_bound(LAYER_MEASURED[dt])
    print(f"mxfp4 lora layer {dt}: forward rel_fro {rel_fro_dev(y.detach(), ref_y.detach()):.3e}; gradients against float64 "
          "autograd " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {b:.3e})")
    assert b <= GRAD_CAP
    for k, v in errs.items():
        assert v <= b, k


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
    saved = [tuple(t.shape) for t in y2.grad_fn.saved_tensors if t.dim() == 2 and t.shape[0] == T]
    assert sorted(saved) == sorted([(T, H_L), (T, 2 * F_L), (T, R_L), (T, R_L)])


def test_only_what_requires_grad_gets_a_gradient():
    _, m = make_layers(torch.float32)
    tpe, offs, T = expert_table([5, 0, 40, 3], tail=2)
    g = torch.Generator().manual_seed(22)
    x, gy = torch.randn(T, H_L, generator=g).to(DEV), torch.randn(T, H_L, generator=g).to(DEV)
    for n in NAMES[:3]:
        getattr(m, n).requires_grad_(False)
    y = m(x, tpe, offs)                                                              # down_lora_B alone
    y.backward(gy)
    assert m.down_lora_B.grad is not None and all(getattr(m, n).grad is None for n in NAMES[:3])
    assert m.gate_up_bias.grad is None and m.down_bias.grad is None and x.grad is None
    m.down_lora_B.requires_grad_(False)
    assert not m(x, tpe, offs).requires_grad                                         # nothing wants a gradient: the plain ops
    with pytest.raises(RuntimeError, match="activation_dtype"):
        m(x.bfloat16(), tpe, offs)


# ---- the block

def test_block_trains_the_adapters_through_the_router():
    """QuantizedSparseMoEBlock(experts=LoRAMXFP4MoEFFN, top_k=2, T=50, router_bias=True): one backward gives finite gradients
    on the gate and all four adapters, the frozen buffers have none, and x.grad is the hand composition of the block's own
    steps around the layer's hand composition."""
    T, top_k = 50, 2
    _, experts = make_layers(torch.float32, seed=9)
    torch.manual_seed(13)                                                            # (the gate's initial weights)
    blk = fq().QuantizedSparseMoEBlock(E_L, H_L, F_L, top_k=top_k, experts=experts, router_bias=True).to(DEV)
    assert blk.experts is experts
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H_L, generator=g).to(DEV).requires_grad_(True)
    gout = torch.randn(T, H_L, generator=g).to(DEV)
    with torch.no_grad():
        blk.gate.bias.copy_((torch.randn(E_L, generator=g) * 0.1).to(DEV))
    out, logits = blk(x)
    out.backward(gout)
    grads = dict(x=x.grad, gate_weight=blk.gate.weight.grad, gate_bias=blk.gate.bias.grad,
                 **{n: getattr(experts, n).grad for n in NAMES})
    for k, v in grads.items():
        assert v is not None and bool(torch.isfinite(v).all()) and torch.count_nonzero(v) > 0, k
    for name, buf in blk.named_buffers():
        assert not buf.requires_grad and buf.grad is None, name
    assert experts.gate_up_bias.grad is None and experts.down_bias.grad is None      # frozen until asked
    # the hand composition: the block's own differentiable steps around the layer's ops composed by hand
    o = ops()
    hand = {}

    class HandFFN(torch.autograd.Function):
        @staticmethod
        def forward(ctx, rows, tpe, offs):
            ctx.save_for_backward(rows, tpe, offs)
            with torch.no_grad():
                return experts(rows, tpe, offs)

        @staticmethod
        def backward(ctx, gy):
            rows, tpe, offs = ctx.saved_tensors
            hand.update(hand_composition(experts, rows, gy.contiguous(), tpe, offs, torch.float32)[1])
            return hand["x"], None, None

    xd = x.detach().clone().requires_grad_(True)
    weights, indices, *_ = o.router_score_topk(blk.router_logits(xd), top_k, blk.scoring, blk.selection_bias, blk.n_group,
                                               blk.topk_group, blk.group_top, blk.renormalize, blk.routed_scaling_factor,
                                               return_scores=True)
    tpe, offs, token_of_sorted, pos_of_slot = o.route_plan(indices, E_L)
    rows = o.dispatch_rows(xd, token_of_sorted, pos_of_slot, top_k)
    res = o.combine_any(HandFFN.apply(rows, tpe, offs), pos_of_slot, weights, out_dtype=xd.dtype)
    assert same_bits(res.detach(), out.detach())
    gate_grads = [blk.gate.weight.grad.clone(), blk.gate.bias.grad.clone()]
    res.backward(gout)
    assert same_bits(xd.grad, x.grad)
    for n in NAMES:
        assert same_bits(getattr(experts, n).grad, hand[n]), n
    assert same_bits(blk.gate.weight.grad, gate_grads[0] + gate_grads[0]) and same_bits(blk.gate.bias.grad, gate_grads[1] + gate_grads[1])
