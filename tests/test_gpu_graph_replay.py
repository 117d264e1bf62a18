"""One captured graph serves every routing of its (E, T): the grouped ops under torch.cuda.graph with the expert table, the
rows and (for the block) the router's parameters changing between replays.

The entry points promise "asynchronous on the given stream, no host synchronisation, no allocation, no global state;
graph-capturable" (INTEGRATION.md): every grid is planned on the host from upper bounds (T and E) and the real row
blocks are found on the device, so a decode loop captures a layer once and replays it whatever the router chose.  Here
each family is captured ONCE at scene S0 (warmed up twice on a side stream first, as PyTorch asks) and replayed over

  S0 even split (captured) | S1 all T rows on expert 0 | S2 all on the last expert | S3 the family's ragged table (an
  empty expert, a one-row expert, a gap, an uncovered tail) | S4 = S3 with the experts permuted (offsets not monotone) |
  S5 every count 0 | S6 = S3 with a last count that leaves [0, T) (clipped on the device) | S7 = S0 again,

each scene with rows of its own, copied into the static inputs; the static output holds SENT before every replay.  After
each replay: (a) the output is bit for bit the eager result of the same op on the default stream on fresh clones; (b) it
agrees with a float64 reference within the family's own bound (exact equality where the data is integer), so a mistake
that eager and replay share cannot hide; (c) the rows no expert covers are exactly zero.  S7 must carry the bits of the
first S0 replay.  What fails here: a launch or memset that goes to the null stream (a capture error or a node missing
from the graph), anything the host derives from the table's contents or caches across calls, state one launch leaves for
the next in the workspace, the tile tables or the output.

The two-phase API (ops.act_quant + ops.gemm_i8) also takes its cached scratch for the first time inside a capture, and the
whole QuantizedSparseMoEBlock (INT4 and MXFP4 experts, with and without capacity_factor and a token mask, with a shared
expert) is captured once and replayed while its routing changes by itself: new tokens, the router bias overwritten in place,
a mask with one real token.  The block is held to its tests' dense float64 sum over the same expert module and, because a
stale table inside that module would be shared by both sides, to float64 torch on the dequantised weights as well.

The MXFP4 experts run in every precision under BOTH kernel forms pinned (bf16, fp8, fp4 and fp6 rows; the unpinned fp8
and fp4 families stay as they were), the fused adapter entries (ops.moe_forward_mxfp4_lora / moe_gated_forward_mxfp4_lora /
moe_backward_input_mxfp4_lora, with NaN shrunk rows where a scene leaves a row uncovered) go through the same scenes, the
block also wraps LoRAMXFP4MoEFFN experts, and the dense ops.linear_forward_mxfp4 / linear_gated_forward_mxfp4, which have
no expert table, replay their split form (two launches and a partial-sum workspace) over changing rows.

The NVFP4 experts (ops.moe_forward_nvfp4 / moe_gated_forward_nvfp4 under both kernel forms pinned, and
ops.moe_backward_input_nvfp4) go through the same scenes with a global scale per expert and a bias, at K = 288 and 96 and,
for the plain forward, at K = 608, where the decode kernel's load ring consumes a refilled slot; the dense
ops.linear_forward_nvfp4 / linear_gated_forward_nvfp4 replay over changing rows, and the block also wraps NVFP4MoEFFN.
The NVFP4 adapter entries (ops.moe_forward_nvfp4_lora / moe_gated_forward_nvfp4_lora / moe_backward_input_nvfp4_lora, with
NaN shrunk rows where a scene leaves a row uncovered and global scales that are not 1) go through the same scenes, the dense
ops.linear_forward_nvfp4_lora / linear_backward_input_nvfp4_lora replay beside the dense base ops, and the block also wraps
LoRANVFP4MoEFFN.

Every family asserts the kernel id the library reports for its shape (fql_tune_chosen_cfg / fql_tune_mx4_kernel /
fql_tune_mx4_scaled_kernel / fql_tune_mx4_f6_kernel / fql_tune_mx4_linear_kernel / fql_tune_nvfp4_kernel; the adapter entries
and the backwards have one form): if a
heuristic change moves the call, the test says so instead of silently testing another kernel.  test_gpu_side_stream.py
runs the same families on side streams."""
import functools

import numpy as np
import pytest
import torch

from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import (EXACT_REL_FRO, FAST_REL_FRO, FMA_REL_FRO, FP8_ACC_SCALED_REL_FRO, NAN, SENT, clipped_ranges, dequant_f64,
                     expert_table, first_diff, fq, heavy_rows, ops, rel_fro_dev, same_bits, uncovered_mask)
from test_gpu_expert_bias_layers import FFN_REL_FRO
from test_gpu_group_bwd import TABLES as BWD_TABLES, problem as group_bwd_problem
from test_gpu_group_moe_ops import FL, I8, problem as group_problem
from test_gpu_mxfp4 import GATED_BOUND as MX4_GATED_BOUND
from test_gpu_mxfp4_decode import SAME_INPUT_BOUND as MX4_BOUND, problem as mx4_problem
from test_gpu_mxfp4_f4 import SAME_INPUT_BOUND as MX4_Q_BOUND, q_host
from test_gpu_mxfp4_f6 import SAME_INPUT_BOUND as MX6_BOUND, q_host as q6_host
from test_gpu_mxfp4_f8 import quantise
from test_gpu_mxfp4_linear import gaussian_bound as linear_bound, own_hidden as linear_own_hidden, problem as linear_problem
from test_gpu_mxfp4_lora import SAME_INPUT_BOUND as LORA_BASE_BOUND, bound as lora_bound
from test_gpu_nvfp4 import GATED_BOUND as NV4_GATED_BOUND, NARROW as NV4_NARROW, epilogue as nv4_epilogue, problem as nv4_problem
from test_route_capped_cpu import plan_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_MAX = 2 ** 31 - 1
BLOCK_REL = 4e-6                    # the block against its dense float64 sum (tests/test_gpu_sparse_moe_block_capped.py REL)
assert MX4_BOUND == 2.64e-7 and MX4_Q_BOUND == 3e-5 and MX6_BOUND == 3e-5 and LORA_BASE_BOUND == MX4_BOUND
assert NV4_GATED_BOUND == 4 * 1.7e-5
MX4_MODE = {"fp8": 1, "fp4": 2}     # the mode of fql_tune_set_mx4_scaled_decode_max_rows / fql_tune_mx4_scaled_kernel
FORM = {"tile": 0, "decode": 1}     # what fql_tune_mx4_kernel / _scaled_kernel / _f6_kernel report


def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def tune():
    """tune(mx4="decode" | "tile", w4=0 | 1, scaled=("fp8" | "fp4", "decode" | "tile"), f6="decode" | "tile",
    linear=(rows of the split range, slices S), nvfp4="decode" | "tile"): the library's kernel choice for this test; its
    own comes back afterwards."""
    L = lib()
    rows_of = {"decode": INT_MAX, "tile": 0}
    decode = L.fql_tune_set_mx4_decode_max_rows(-1)                  # (a negative value changes nothing)
    scaled_was = {mode: L.fql_tune_set_mx4_scaled_decode_max_rows(mode, -1) for mode in MX4_MODE.values()}
    f6_was = L.fql_tune_set_mx4_f6_decode_max_rows(-1)
    lin_rows = L.fql_tune_set_mx4_linear_decode_max_rows(-1)
    nvfp4_was = L.fql_tune_set_nvfp4_decode_max_rows(-1)
    lin_slices = L.fql_tune_set_mx4_linear_slices(0)
    L.fql_tune_set_mx4_linear_slices(lin_slices)
    w4 = L.fql_tune_set_w4(1)
    L.fql_tune_set_w4(w4)

    def use(mx4=None, w4=None, scaled=None, f6=None, linear=None, nvfp4=None):
        if mx4 is not None:
            L.fql_tune_set_mx4_decode_max_rows(rows_of[mx4])
        if w4 is not None:
            L.fql_tune_set_w4(w4)
        if scaled is not None:
            L.fql_tune_set_mx4_scaled_decode_max_rows(MX4_MODE[scaled[0]], rows_of[scaled[1]])
        if f6 is not None:
            L.fql_tune_set_mx4_f6_decode_max_rows(rows_of[f6])
        if linear is not None:
            L.fql_tune_set_mx4_linear_decode_max_rows(linear[0])
            L.fql_tune_set_mx4_linear_slices(linear[1])
        if nvfp4 is not None:
            L.fql_tune_set_nvfp4_decode_max_rows(rows_of[nvfp4])
    try:
        yield use
    finally:
        L.fql_tune_set_mx4_decode_max_rows(decode)
        for mode, rows in scaled_was.items():
            L.fql_tune_set_mx4_scaled_decode_max_rows(mode, rows)
        L.fql_tune_set_mx4_f6_decode_max_rows(f6_was)
        L.fql_tune_set_mx4_linear_decode_max_rows(lin_rows)
        L.fql_tune_set_mx4_linear_slices(lin_slices)
        L.fql_tune_set_nvfp4_decode_max_rows(nvfp4_was)
        L.fql_tune_set_w4(w4)


# ---- capture

def capture(call, static, after_warmup=None):
    """Warm ``call(*static)`` up twice on a side stream, capture it once on that stream into the ``static`` tensors;
    returns (graph, static output(s), the stream)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            call(*static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    if after_warmup is not None:
        after_warmup()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call(*static)
    return graph, out, s


# ---- scenes

def tab(T, counts, gaps=None, tail=0):
    tpe, offs, total = expert_table(list(counts), gaps, tail, device="cpu")
    assert total == T, (total, T)
    return tpe, offs


def ragged_of(E, T):
    """The ragged table of a family without one of its own: an empty expert, a one-row expert, a gap of one row in front of
    the third expert, two uncovered tail rows; the other rows one third on the third expert and the rest on the last."""
    assert E >= 4 and T >= 10
    rest = T - 1 - 1 - 2
    counts = [0, 1, rest // 3] + [0] * (E - 4) + [rest - rest // 3]
    return counts, [0, 0, 1] + [0] * (E - 3), 2


def streaming_ragged(E, T):
    """One expert at 129 rows, sixteen at 1, the rest empty (helpers.footprint_table("G2") inside E experts); the other rows
    uncovered."""
    assert E >= 17 and T >= 145
    return [129] + [1] * 16 + [0] * (E - 17), None, T - 145


def scenes(E, T, ragged):
    """[(name, tokens_per_expert, input_offsets, seed of the rows)], int32 on the host."""
    even = tab(T, [T // E + (1 if e < T % E else 0) for e in range(E)])
    s3 = tab(T, *ragged)
    perm = torch.arange(E - 1, -1, -1)
    s4 = (s3[0][perm].contiguous(), s3[1][perm].contiguous())
    assert s4[1].tolist() != sorted(s4[1].tolist()) and int(s3[0].min()) == 0 and int(s3[0].sum()) < T
    zero = torch.zeros(E, dtype=torch.int32)
    clipped = s3[0].clone()
    clipped[-1] = T + 999
    assert int(s3[1][-1]) + int(clipped[-1]) > T
    return [("S0", *even, 0), ("S1", *tab(T, [T] + [0] * (E - 1)), 1), ("S2", *tab(T, [0] * (E - 1) + [T]), 2),
            ("S3", *s3, 3), ("S4", *s4, 4), ("S5", zero, zero.clone(), 5), ("S6", clipped, s3[1], 6), ("S7", *even, 0)]


def gen(seed, *salt):
    return torch.Generator().manual_seed(100003 * seed + sum(salt))


class Family:
    """One op at one shape: ``make_rows(seed)`` -> the per-scene device tensors in front of the table, ``call(*rows, tpe,
    offs)`` -> the result, ``reference(rows, ranges)`` -> float64 [T, C] with zero rows outside ``ranges``, ``bound`` (None:
    exact equality), ``kernel()`` -> (id the library reports, id expected), ``tune``: the arguments of the fixture."""

    def __init__(self, E, T, ragged, make_rows, call, reference, bound, kernel=None, tune=None):
        self.E, self.T, self.ragged, self.make_rows, self.call = E, T, ragged, make_rows, call
        self.reference, self.bound, self.kernel, self.tune = reference, bound, kernel, tune or {}

    def prepare(self, tune):
        tune(**self.tune)
        if self.kernel is not None:
            got, want = self.kernel()
            assert got == want, f"the library picks kernel {got} for this shape, the test is written for {want}"

    def check(self, what, got, rows, tpe, offs):
        """(b) and (c) on one result."""
        ranges = clipped_ranges(tpe.cpu(), offs.cpu(), self.T)
        covered = torch.zeros(self.T, dtype=torch.bool, device=DEV)
        for lo, hi in ranges:
            covered[lo:hi] = True
        assert torch.count_nonzero(got[~covered]) == 0, f"{what}: rows no expert covers must be zero"
        ref = self.reference(rows, ranges).to(DEV)
        assert torch.count_nonzero(ref[~covered]) == 0
        if self.bound is None:
            assert torch.equal(got.double(), ref), f"{what}: not the exact integer result"
        else:
            err = rel_fro_dev(got, ref)
            print(f"{what}: rel_fro {err:.3e} (bound {self.bound:.2e})")
            assert err < self.bound, (what, err)


def grouped64(rows64, W_of, ranges, C, bias=None):
    """float64 [T, C]: rows64[lo:hi] @ W_of(e) (+ bias[e]) over the rows of expert e, zero elsewhere."""
    out = torch.zeros(rows64.shape[0], C, dtype=torch.float64, device=rows64.device)
    for e, (lo, hi) in enumerate(ranges):
        if hi > lo:
            out[lo:hi] = rows64[lo:hi] @ W_of(e)
            if bias is not None:
                out[lo:hi] += bias[e].double().to(rows64.device)
    return out


def replay_scenes(fam, tune):
    fam.prepare(tune)
    sc = scenes(fam.E, fam.T, fam.ragged)
    static = [r.clone() for r in fam.make_rows(0)] + [sc[0][1].to(DEV), sc[0][2].to(DEV)]
    graph, out, _ = capture(fam.call, static)
    try:
        first = None
        for name, tpe, offs, seed in sc:
            rows, tpe, offs = fam.make_rows(seed), tpe.to(DEV), offs.to(DEV)
            for s, v in zip(static, (*rows, tpe, offs)):
                s.copy_(v)
            out.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            eager = fam.call(*[r.clone() for r in rows], tpe.clone(), offs.clone())
            assert same_bits(got, eager), f"{name}: the replay is not the eager result: (differing elements, first) = " \
                                          f"{first_diff(got, eager)}"
            fam.check(name, got, rows, tpe, offs)
            if name == "S0":
                first = got
        assert same_bits(got, first), "S7: S0 again does not carry the bits of the first S0 replay"
    finally:
        del graph


# ---- per-row INT4

@functools.lru_cache(maxsize=None)
def int4_weights(E, N, K):
    """Random codes, scales in [0.001, 0.003], zero points in 5 .. 10, a bias of the outputs' own size; made once."""
    g = torch.Generator().manual_seed(1000 * E + N + K)
    P = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8)
    S = 0.001 + 0.002 * torch.rand(E, N, generator=g)
    Z = torch.randint(5, 11, (E, N), generator=g).float()
    B = 0.2 * torch.randn(E, N, generator=g)
    return tuple(t.to(DEV) for t in (P, S, Z, B))


def chosen(precision, E, T, K, N, expect):
    return lambda: (lib().fql_tune_chosen_cfg(ops()._precision(precision), E, T, K, N, 1), expect)


def int4_forward(E, K, N, T, dtype, precision, expect, ragged, tune=None):
    P, S, Z, B = int4_weights(E, N, K)
    W_of = lambda e: dequant_f64(P[e], S[e], Z[e]).t()

    def make_rows(seed):
        return (torch.randn(T, K, generator=gen(seed, T, K)).to(dtype).to(DEV),)

    def call(x, tpe, offs):
        return ops().moe_forward_any(P, S, Z, x, None, tpe, offs, precision=precision, out_dtype=torch.float32, bias=B)

    def reference(rows, ranges):
        x64 = rows[0].double()
        if precision == "fp8":                                       # the e4m3 values the pre-pass makes of the rows
            from oracle import oracle as O
            b, s = O.quantize_activations_fp8(rows[0].float().cpu().numpy())
            x64 = torch.from_numpy(O.e4m3_decode(b).astype(np.float64) * s.astype(np.float64)[:, None]).to(DEV)
        return grouped64(x64, W_of, ranges, N, B)

    bound = {"exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "fp8": FP8_ACC_SCALED_REL_FRO}[precision]
    return Family(E, T, ragged, make_rows, call, reference, bound, chosen(precision, E, T, K, N, expect), tune)


def int4_gated(E, K, N, T, expect):
    P, S, Z, B = int4_weights(E, N, K)

    def make_rows(seed):
        return ((2.0 * torch.randn(T, 2 * K, generator=gen(seed, T, K, 1))).to(DEV),)

    def call(gate_up, tpe, offs):
        return ops().moe_gated_forward(P, S, Z, gate_up, tpe, offs, precision="exact", bias=B, **act_kw("swiglu_clamp"))

    def reference(rows, ranges):
        return grouped64(hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT), lambda e: dequant_f64(P[e], S[e], Z[e]).t(), ranges,
                         N, B)
    return Family(E, T, ragged_of(E, T), make_rows, call, reference, EXACT_REL_FRO, chosen("exact", E, T, K, N, expect))


def int4_gather(E, K, N, T, expect):
    P, S, Z, _ = int4_weights(E, N, K)
    n_tokens = T // 2

    def make_rows(seed):
        g = gen(seed, T, K, 2)
        return (torch.randn(n_tokens, K, generator=g).to(DEV),
                torch.randint(0, n_tokens, (T,), generator=g, dtype=torch.int32).to(DEV))

    def call(tokens, row_index, tpe, offs):
        return ops().moe_gather_forward(P, S, Z, tokens, row_index, tpe, offs, precision="exact")

    def reference(rows, ranges):
        return grouped64(rows[0][rows[1].long()].double(), lambda e: dequant_f64(P[e], S[e], Z[e]).t(), ranges, N)
    return Family(E, T, ragged_of(E, T), make_rows, call, reference, EXACT_REL_FRO, chosen("exact", E, T, K, N, expect))


def int4_two_phase(E, K, N, T, expect):
    """ops.act_quant then ops.gemm_i8; every fifth row heavy-tailed, so that the residual pass and its scratch are in use."""
    P, S, Z, _ = int4_weights(E, N, K)

    def make_rows(seed):
        x = torch.randn(T, K, generator=gen(seed, T, K, 3)).numpy()
        return (torch.from_numpy(heavy_rows(x, np.random.default_rng(seed))).to(DEV),)

    def call(x, tpe, offs):
        limbs, delta, rowsum = ops().act_quant(x, "exact", tpe, offs)
        return ops().gemm_i8(limbs, delta, rowsum, P, S, Z, tpe, offs, precision="exact")

    def reference(rows, ranges):
        return grouped64(rows[0].double(), lambda e: dequant_f64(P[e], S[e], Z[e]).t(), ranges, N)
    return Family(E, T, ragged_of(E, T), make_rows, call, reference, EXACT_REL_FRO, chosen("exact", E, T, K, N, expect))


def int4_backward(table, N, K):
    """ops.moe_backward_input on per-row weights at the shapes of tests/test_gpu_group_bwd.py."""
    E, counts = 3, BWD_TABLES[table]
    T = sum(counts) + 2
    P, S, Z, _ = int4_weights(E, N, K)

    def make_rows(seed):
        return (torch.randn(T, N, generator=gen(seed, T, N, 4)).to(DEV),)

    def call(gy, tpe, offs):
        return ops().moe_backward_input(P, S, Z, gy, tpe, offs, precision="exact")

    def reference(rows, ranges):
        return grouped64(rows[0].double(), lambda e: dequant_f64(P[e], S[e], Z[e]), ranges, K)
    return Family(E, T, (counts, None, 2), make_rows, call, reference, EXACT_REL_FRO)


# ---- per-group scales

def group_forward(path, N, group, gated):
    p = group_problem(path["counts"], path["K"], N, group)
    E, T, K = 3, p["T"], path["K"]
    bound = EXACT_REL_FRO if path is I8 else FMA_REL_FRO            # (the bounds of tests/test_gpu_group_moe_ops.py)

    def make_rows(seed):
        x = torch.randn(T, 2 * K if gated else K, generator=gen(seed, T, K, group))
        return ((2.0 * x if gated else x).to(DEV),)

    def call(x, tpe, offs):
        if gated:
            return ops().moe_gated_forward(p["P"], p["S"], p["Z"], x, tpe, offs, precision="exact", bias=p["bias"],
                                           **act_kw("swiglu_clamp"))
        return ops().moe_forward_any(p["P"], p["S"], p["Z"], x, None, tpe, offs, precision="exact", bias=p["bias"])

    def reference(rows, ranges):
        x64 = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT) if gated else rows[0].double()
        return grouped64(x64, lambda e: p["W64"][e].t(), ranges, N, p["bias"])
    return Family(E, T, (path["counts"], None, 2), make_rows, call, reference, bound)


def group_backward(table, N, K, group):
    p = group_bwd_problem(table, N, K, group)
    E, T = 3, p["T"]

    def make_rows(seed):
        return (torch.randn(T, N, generator=gen(seed, T, N, group)).to(DEV),)

    def call(gy, tpe, offs):
        return ops().moe_backward_input(p["P"], p["S"], p["Z"], gy, tpe, offs)

    def reference(rows, ranges):
        return grouped64(rows[0].double(), lambda e: dequant_f64(p["P"][e], p["S"][e], p["Z"][e]), ranges, K)
    return Family(E, T, (BWD_TABLES[table], None, 2), make_rows, call, reference, FMA_REL_FRO)


# ---- MXFP4

MX4_RAGGED = ([0, 1, 5, 32, 33], None, 2)


def mx4_W(p):
    from fused_int4_amd.quantize import dequantize_mxfp4
    return dequantize_mxfp4(p["blocks"].cpu(), p["scales"].cpu()).double().to(DEV)


def mx4_form(precision, kernel, E, T, K, N):
    """(kernel() of a Family, the arguments of the tune fixture) that pin ``precision`` to the "tile" or the "decode" form."""
    want = FORM[kernel]
    if precision == "bf16":
        return (lambda: (lib().fql_tune_mx4_kernel(E, T, K, N), want)), dict(mx4=kernel)
    if precision == "fp6":
        return (lambda: (lib().fql_tune_mx4_f6_kernel(E, T, K, N), want)), dict(f6=kernel)
    return (lambda: (lib().fql_tune_mx4_scaled_kernel(MX4_MODE[precision], E, T, K, N), want)), dict(scaled=(precision, kernel))


def mx4_forward(K, N, precision, kernel=None):
    """precision "bf16" (forced to the tile or the decode kernel): integer rows in [-4, 4] and scale codes in [125, 129],
    the float32 result is exact; "fp8" / "fp4" / "fp6" (``kernel`` None: whatever form the library picks, not asserted):
    randn rows against the float64 product of the values the host rule of the precision makes of them
    (tests/test_gpu_mxfp4_f8.py quantise, tests/test_gpu_mxfp4_f4.py and tests/test_gpu_mxfp4_f6.py q_host)."""
    exact = precision == "bf16"
    p = mx4_problem(K, N, lo=125, hi=129, integer=True) if exact else mx4_problem(K, N)
    E, T, W = p["E"], p["T"], mx4_W(p)
    assert (E, T) == (5, 73)

    def make_rows(seed):
        g = gen(seed, K, N)
        return ((torch.randint(-4, 5, (T, K), generator=g).float() if exact else torch.randn(T, K, generator=g)).to(DEV),)

    def call(x, tpe, offs):
        return ops().moe_forward_mxfp4(p["blocks"], p["scales"], x, tpe, offs, bias=p["bias"], out_dtype=torch.float32,
                                       precision=precision)

    def reference(rows, ranges):
        host = {"fp8": quantise, "fp4": q_host, "fp6": q6_host}
        x64 = rows[0].double() if exact else host[precision](rows[0])[2].to(DEV)
        ref = grouped64(x64, lambda e: W[e].t(), ranges, N, p["bias"])
        assert not exact or float(ref.abs().max()) < 2 ** 15        # (every partial sum then fits float32 exactly)
        return ref

    which, pin = (None, None) if kernel is None else mx4_form(precision, kernel, E, T, K, N)
    bound = None if exact else (MX6_BOUND if precision == "fp6" else MX4_Q_BOUND)
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, bound, which, pin)


def mx4_gated(K, N, kernel, precision="bf16"):
    """"bf16": against the bfloat16-rounded float64 h.  "fp6": h goes through the gated MXFP6 quantiser, whose float32 h
    lands on the other e2m3 neighbour of the float64 h for a code in a thousand (tests/test_gpu_mxfp4_f6.py holds it to
    quantize_mxfp6 of the float64 h within GATED_CODE_CAP), one step of 2^-4 of that element; so the reference is the
    float64 product of the values of ops.quantize_rows_mxfp6's own codes (dequantize_mxfp6 on the host), at the same-value
    bound of that file: the GEMM, its table and its workspace are what a replay can get wrong."""
    p = mx4_problem(K, N)
    E, T, W = p["E"], p["T"], mx4_W(p)
    kw = {} if precision == "bf16" else dict(precision=precision)

    def make_rows(seed):
        return ((2.0 * torch.randn(T, 2 * K, generator=gen(seed, K, N, 1))).to(DEV),)

    def call(gate_up, tpe, offs):
        return ops().moe_gated_forward_mxfp4(p["blocks"], p["scales"], gate_up, tpe, offs, bias=p["bias"],
                                             out_dtype=torch.float32, **kw, **act_kw("swiglu_clamp"))

    def reference(rows, ranges):
        if precision == "fp6":
            from fused_int4_amd.quantize import dequantize_mxfp6
            hc, hs = ops().quantize_rows_mxfp6(rows[0], **act_kw("swiglu_clamp"))
            h = dequantize_mxfp6(hc.cpu(), hs.cpu()).double().to(DEV)
        else:                                                        # the bfloat16-rounded float64 h (tests/test_gpu_mxfp4.py)
            h = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT).bfloat16().double()
        return grouped64(h, lambda e: W[e].t(), ranges, N, p["bias"])
    which, pin = mx4_form(precision, kernel, E, T, K, N)
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, MX6_BOUND if precision == "fp6" else MX4_GATED_BOUND, which, pin)


def mx4_backward(K, N):
    p = mx4_problem(K, N)
    E, T, W = p["E"], p["T"], mx4_W(p)

    def make_rows(seed):
        return (torch.randn(T, N, generator=gen(seed, K, N, 2)).to(DEV),)

    def call(gy, tpe, offs):
        return ops().moe_backward_input_mxfp4(p["blocks"], p["scales"], gy, tpe, offs)

    def reference(rows, ranges):
        return grouped64(rows[0].bfloat16().double(), lambda e: W[e], ranges, K)
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, MX4_BOUND)


def scene_uncovered(E, T, ragged):
    """seed of a scene's rows -> bool [T], the rows no expert of that scene covers (S0 and S7 share seed and table)."""
    return {seed: uncovered_mask(clipped_ranges(tpe, offs, T), T) for _, tpe, offs, seed in scenes(E, T, ragged)}


def mx4_lora(K, N, r, kind):
    """The adapter stage fused into the MXFP4 GEMMs (tests/test_gpu_mxfp4_lora.py): ``kind`` "fwd" (rows (x, v)), "glu"
    ((gate_up, v)) or "bwd" ((gy, dv)); the adapter matrix B [E, N, r] / A [E, r, K] is fixed.  "fwd" and "bwd": that file's
    integer recipe, rows and shrunk rows in [-4, 4], adapter integers in [-2, 2], scale codes 125 .. 129: every product is a
    multiple of 2^-3 and every sum stays below 2^17 (asserted), so the float32 result is the float64 reference.  "glu":
    Gaussian data against the float64 sum of both products on the bfloat16-rounded operands, at MX4_GATED_BOUND scaled by
    that file's rule for K + r terms.  The shrunk rows of the rows a scene leaves uncovered are NaN (S3 .. S6): an adapter
    row read under the wrong t shows.  The adapter entries have one kernel form (no decode kernel, nothing to report)."""
    exact = kind != "glu"
    p = mx4_problem(K, N, lo=125, hi=129, integer=True) if exact else mx4_problem(K, N)
    E, T, W = p["E"], p["T"], mx4_W(p)
    assert (E, T) == (5, 73)
    uncovered = scene_uncovered(E, T, MX4_RAGGED)
    assert all(bool(uncovered[s].any()) for s in (3, 4, 5)) and not bool(uncovered[0].any())   # (S6's clipped count takes the tail)
    g0 = gen(0, K, N, r, 7)
    C = N if kind == "bwd" else K                                   # the contraction of the base product
    if exact:
        M = torch.randint(-2, 3, (E, r, K) if kind == "bwd" else (E, N, r), generator=g0).float().to(DEV)
    else:                                                            # sized so that the adapter term is of the base term's size
        M = torch.randn(E, N, r, generator=g0).to(DEV) * (W.square().mean(dim=2, keepdim=True).sqrt() * (C / r) ** 0.5).float()
    M64 = M.bfloat16().double()

    def make_rows(seed):
        g = gen(seed, K, N, r, len(kind))
        if kind == "glu":
            rows, v = 2.0 * torch.randn(T, 2 * K, generator=g), torch.randn(T, r, generator=g)
        else:
            rows, v = torch.randint(-4, 5, (T, C), generator=g).float(), torch.randint(-4, 5, (T, r), generator=g).float()
        v[uncovered[seed]] = NAN
        return rows.to(DEV), v.to(DEV)

    def call(rows, v, tpe, offs):
        if kind == "fwd":
            return ops().moe_forward_mxfp4_lora(p["blocks"], p["scales"], rows, v, M, tpe, offs, bias=p["bias"],
                                                out_dtype=torch.float32)
        if kind == "glu":
            return ops().moe_gated_forward_mxfp4_lora(p["blocks"], p["scales"], rows, v, M, tpe, offs, bias=p["bias"],
                                                      out_dtype=torch.float32, **act_kw("swiglu_clamp"))
        return ops().moe_backward_input_mxfp4_lora(p["blocks"], p["scales"], rows, v, M, tpe, offs)

    def reference(rows, ranges):
        x64 = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT).bfloat16().double() if kind == "glu" else rows[0].double()
        v64 = rows[1].bfloat16().double()
        if kind == "bwd":
            ref = grouped64(x64, lambda e: W[e], ranges, K) + grouped64(v64, lambda e: M64[e], ranges, K)
        else:
            base = grouped64(x64, lambda e: W[e].t(), ranges, N, p["bias"])
            ref = base + grouped64(v64, lambda e: M64[e].t(), ranges, N)
            assert not ranges or torch.equal(ref, base) == all(hi <= lo for lo, hi in ranges)     # (the adapter matters)
        assert bool(torch.isfinite(ref).all()) and (not exact or float(ref.abs().max()) < 2 ** 17)
        return ref

    bound = None if exact else MX4_GATED_BOUND * lora_bound(K, r) / LORA_BASE_BOUND
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, bound)


# ---- NVFP4

NV4_COUNTS, NV4_TAIL = (0, 1, 5, 32, 33), 2          # MX4_RAGGED as test_gpu_nvfp4.problem takes it: E = 5, T = 73


def nv4_weights(K, N, integer):
    """test_gpu_nvfp4.problem on E = 5, T = 73: random codes, scale bytes 0x30 .. 0x47, a power-of-two global scale that
    differs between neighbouring experts, a bias (integers with ``integer``).  Returns (p, W float64 [E, N, K] on the
    device, WITHOUT the global scale)."""
    p = (nv4_problem(K, N, counts=NV4_COUNTS, tail=NV4_TAIL, scale_range=NV4_NARROW, integer=True) if integer else
         nv4_problem(K, N, counts=NV4_COUNTS, tail=NV4_TAIL, scale_range=NV4_NARROW, seed=7))
    assert (p["E"], p["T"]) == (5, 73) and len(set(p["gs"].tolist())) == 5
    return p, p["W"].to(DEV)


def nv4_grouped64(rows64, W_of, ranges, C, gs, bias=None):
    """float64 [T, C]: the contract of csrc/fql_gemm_nvfp4.h on a float64 sum, fl32(fl32(fl32(acc) * gs[e]) + bias[e]), over
    the rows of expert e, zero elsewhere."""
    out = torch.zeros(rows64.shape[0], C, dtype=torch.float64, device=rows64.device)
    for e, (lo, hi) in enumerate(ranges):
        if hi > lo:
            out[lo:hi] = nv4_epilogue(rows64[lo:hi] @ W_of(e), gs[e], None if bias is None else bias[e])
    return out


def nv4_form(kernel, E, T, K, N):
    return (lambda: (lib().fql_tune_nvfp4_kernel(E, T, K, N), FORM[kernel])), dict(nvfp4=kernel)


def nv4_forward(K, N, kernel):
    """ops.moe_forward_nvfp4 with the global scales and a bias, forced to the tile or the decode kernel, on the integer
    recipe of tests/test_gpu_nvfp4.py (rows in [-4, 4]; every sum below 2^16, asserted): the float32 result is exact."""
    p, W = nv4_weights(K, N, True)
    E, T = p["E"], p["T"]

    def make_rows(seed):
        return (torch.randint(-4, 5, (T, K), generator=gen(seed, K, N, 11)).float().to(DEV),)

    def call(x, tpe, offs):
        return ops().moe_forward_nvfp4(p["blocks"], p["scales"], p["gs"], x, tpe, offs, bias=p["bias"], out_dtype=torch.float32)

    def reference(rows, ranges):
        assert float(grouped64(rows[0].double(), lambda e: W[e].t(), ranges, N).abs().max()) < 2 ** 16
        return nv4_grouped64(rows[0].double(), lambda e: W[e].t(), ranges, N, p["gs"], p["bias"])
    which, pin = nv4_form(kernel, E, T, K, N)
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, None, which, pin)


def nv4_gated(K, N, kernel):
    """ops.moe_gated_forward_nvfp4 on Gaussian gate | up rows against the float64 product of the bfloat16-rounded float64 h,
    at tests/test_gpu_nvfp4.py's GATED_BOUND."""
    p, W = nv4_weights(K, N, False)
    E, T = p["E"], p["T"]

    def make_rows(seed):
        return ((2.0 * torch.randn(T, 2 * K, generator=gen(seed, K, N, 12))).to(DEV),)

    def call(gate_up, tpe, offs):
        return ops().moe_gated_forward_nvfp4(p["blocks"], p["scales"], p["gs"], gate_up, tpe, offs, bias=p["bias"],
                                             out_dtype=torch.float32, **act_kw("swiglu_clamp"))

    def reference(rows, ranges):
        h = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT).bfloat16().double()
        return nv4_grouped64(h, lambda e: W[e].t(), ranges, N, p["gs"], p["bias"])
    which, pin = nv4_form(kernel, E, T, K, N)
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, NV4_GATED_BOUND, which, pin)


def nv4_backward(K, N):
    """ops.moe_backward_input_nvfp4 with the global scales on integer gradients in [-4, 4] (every sum below 2^15, asserted):
    the float32 result is exact."""
    p, W = nv4_weights(K, N, True)
    E, T = p["E"], p["T"]

    def make_rows(seed):
        return (torch.randint(-4, 5, (T, N), generator=gen(seed, K, N, 13)).float().to(DEV),)

    def call(gy, tpe, offs):
        return ops().moe_backward_input_nvfp4(p["blocks"], p["scales"], p["gs"], gy, tpe, offs)

    def reference(rows, ranges):
        assert float(grouped64(rows[0].double(), lambda e: W[e], ranges, K).abs().max()) < 2 ** 15
        return nv4_grouped64(rows[0].double(), lambda e: W[e], ranges, K, p["gs"])
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, None)


NV4_LORA_GS = (0.5, 2.0, 0.25, 4.0, 0.125)            # the adapter families' global scales: none is 1, neighbours differ


def nv4_lora_exact64(base64, add64, g, bias64=None):
    """float64 (base64 * g + add64 + bias64) of the integer recipe of tests/test_gpu_nvfp4_lora.py, with that file's
    exactness condition asserted from the operands alone: every weight term is a multiple of g * 2^-5 (integer x code / 2 x
    scale byte / 16), every other term an integer, and the sum of the absolute values of all terms of one output (``base64``
    and ``add64`` are (value, that sum) pairs) stays below 2^24 of that unit, so a float32 sum is exact in any order."""
    unit = min(g * 2.0 ** -5, 1.0)
    mass = base64[1] * g + add64[1] + (0 if bias64 is None else bias64.abs())
    assert float(mass.max()) < 2.0 ** 24 * unit
    return base64[0] * g + add64[0] + (0 if bias64 is None else bias64)


def nv4_lora(K, N, r, kind):
    """The adapter stage fused into the NVFP4 GEMMs (tests/test_gpu_nvfp4_lora.py): ``kind`` "fwd" (rows (x, v)), "glu"
    ((gate_up, v)) or "bwd" ((gy, dv)); the adapter matrix B [E, N, r] / A [E, r, K] is fixed, the global scales are
    NV4_LORA_GS and scale the weight term ONLY, the forward kinds have a bias.  "fwd" and "bwd": that file's integer recipe,
    rows and shrunk rows in [-4, 4], adapter integers in [-2, 2], scale bytes 0x30 .. 0x47, an integer bias; its exactness
    condition is asserted per scene (nv4_lora_exact64), so the float32 result is the float64 definition.  "glu": Gaussian data
    against the float64 product of the bfloat16-rounded float64 h times g plus the float64 adapter term on the
    bfloat16-rounded v and B, at NV4_GATED_BOUND scaled as mx4_lora scales MX4_GATED_BOUND, by max(1, (K + r) / 288).  The
    shrunk rows of the rows a scene leaves uncovered are NaN (S3 .. S6).  The adapter entries have one kernel form."""
    exact = kind != "glu"
    p, W = nv4_weights(K, N, exact)
    E, T = p["E"], p["T"]
    gs = torch.tensor(NV4_LORA_GS, device=DEV)
    assert all(g != 1.0 for g in NV4_LORA_GS) and all(a != b for a, b in zip(NV4_LORA_GS, NV4_LORA_GS[1:])) and len(NV4_LORA_GS) == E
    uncovered = scene_uncovered(E, T, MX4_RAGGED)
    assert all(bool(uncovered[s].any()) for s in (3, 4, 5)) and not bool(uncovered[0].any())
    g0 = gen(0, K, N, r, 17)
    C = N if kind == "bwd" else K                                   # the contraction of the base product
    if exact:
        M = torch.randint(-2, 3, (E, r, K) if kind == "bwd" else (E, N, r), generator=g0).float().to(DEV)
    else:                                                            # sized so that the adapter term is of the base term's size
        rms = (W * gs.double().view(E, 1, 1)).square().mean(dim=2, keepdim=True).sqrt()
        M = torch.randn(E, N, r, generator=g0).to(DEV) * (rms * (C / r) ** 0.5).float()
    M64 = M.bfloat16().double()

    def make_rows(seed):
        g = gen(seed, K, N, r, 17 + len(kind))
        if kind == "glu":
            rows, v = 2.0 * torch.randn(T, 2 * K, generator=g), torch.randn(T, r, generator=g)
        else:
            rows, v = torch.randint(-4, 5, (T, C), generator=g).float(), torch.randint(-4, 5, (T, r), generator=g).float()
        v[uncovered[seed]] = NAN
        return rows.to(DEV), v.to(DEV)

    def call(rows, v, tpe, offs):
        w = (p["blocks"], p["scales"], gs)
        if kind == "fwd":
            return ops().moe_forward_nvfp4_lora(*w, rows, v, M, tpe, offs, bias=p["bias"], out_dtype=torch.float32)
        if kind == "glu":
            return ops().moe_gated_forward_nvfp4_lora(*w, rows, v, M, tpe, offs, bias=p["bias"], out_dtype=torch.float32,
                                                      **act_kw("swiglu_clamp"))
        return ops().moe_backward_input_nvfp4_lora(*w, rows, v, M, tpe, offs)

    def reference(rows, ranges):
        x64 = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT).bfloat16().double() if kind == "glu" else rows[0].double()
        v64 = rows[1].bfloat16().double()
        out = torch.zeros(T, K if kind == "bwd" else N, dtype=torch.float64, device=DEV)
        changed = False
        for e, (lo, hi) in enumerate(ranges):
            if hi <= lo:
                continue
            We, Me = (W[e], M64[e]) if kind == "bwd" else (W[e].t(), M64[e].t())
            base, add = x64[lo:hi] @ We, v64[lo:hi] @ Me
            bias64 = None if kind == "bwd" else p["bias"][e].double()
            if exact:
                out[lo:hi] = nv4_lora_exact64((base, x64[lo:hi].abs() @ We.abs()), (add, v64[lo:hi].abs() @ Me.abs()),
                                              NV4_LORA_GS[e], bias64)
            else:
                out[lo:hi] = base * NV4_LORA_GS[e] + add + bias64
            changed = changed or bool(add.count_nonzero())
        assert bool(torch.isfinite(out).all()) and changed == any(hi > lo for lo, hi in ranges)   # (the adapter matters)
        return out

    bound = None if exact else NV4_GATED_BOUND * lora_bound(K, r) / LORA_BASE_BOUND
    return Family(E, T, MX4_RAGGED, make_rows, call, reference, bound)


# ---- the families, by name (tests/test_gpu_side_stream.py takes its cases from here)

SMALL = dict(E=4, K=512, N=136)                   # wide_tiles < 128: the small regime of choose_cfg (csrc/fql_int4.hip)
SMALL_IDS = {40: 207, 100: 8, 232: 7, 400: 1}
STREAM = dict(E=64, K=512)                        # E x ceil(N / 256) >= 128 tiles: the streaming regime
# T -> (N, id): every N > 256 is in the regime, 264 keeps the cases small; at 100 rows per group only 512 < N <= 768
# makes the 128 x 192 tile cheaper than the 128 x 128 one (id 1 at N = 512), and the one-wave-per-SIMD kernel then takes
# it (id 301; 0 without)
STREAM_IDS = {640: (264, 202), 1600: (264, 103), 3200: (264, 301), 6400: (520, 301)}
F32, BF16 = torch.float32, torch.bfloat16

FAMILIES = {}
for _T, _id in SMALL_IDS.items():
    for _dt in (F32, BF16):
        FAMILIES[f"int4-small-T{_T}-{'f32' if _dt == F32 else 'bf16'}"] = functools.partial(
            int4_forward, 4, 512, 136, _T, _dt, "exact", _id, ragged_of(4, _T))
for _T, (_N, _id) in STREAM_IDS.items():
    for _dt in (F32, BF16):
        FAMILIES[f"int4-stream-T{_T}-{'f32' if _dt == F32 else 'bf16'}"] = functools.partial(
            int4_forward, 64, 512, _N, _T, _dt, "exact", _id, streaming_ragged(64, _T))
FAMILIES.update({
    "int4-stream-T6400-f32-wide": functools.partial(int4_forward, 64, 512, 520, 6400, F32, "exact", 0,
                                                    streaming_ragged(64, 6400), dict(w4=0)),
    "int4-small-T100-fast": functools.partial(int4_forward, 4, 512, 136, 100, F32, "fast", 8, ragged_of(4, 100)),
    "int4-small-T100-fp8": functools.partial(int4_forward, 4, 512, 136, 100, F32, "fp8", 8, ragged_of(4, 100)),
    "int4-gated-T100": functools.partial(int4_gated, 4, 512, 136, 100, 8),
    "int4-gather-T232": functools.partial(int4_gather, 4, 512, 136, 232, 7),
    "int4-two-phase-T100": functools.partial(int4_two_phase, 4, 512, 136, 100, 8),
    "int4-bwd-tiled-vec": functools.partial(int4_backward, "40-0-9", 136, 512),
    "int4-bwd-rows": functools.partial(int4_backward, "3-0-5", 33, 96),
    "group-i8": functools.partial(group_forward, I8, 136, 64, False),
    "group-i8-glu": functools.partial(group_forward, I8, 136, 64, True),
    "group-float": functools.partial(group_forward, FL, 136, 32, False),
    "group-float-glu": functools.partial(group_forward, FL, 136, 32, True),
    "group-bwd-tiled-vec": functools.partial(group_backward, "40-0-9", 136, 512, 64),
    "group-bwd-rows-g48": functools.partial(group_backward, "3-0-5", 33, 96, 48),
})
for _K, _N in ((288, 136), (96, 37)):
    FAMILIES.update({
        f"mx4-K{_K}-N{_N}-tile": functools.partial(mx4_forward, _K, _N, "bf16", "tile"),
        f"mx4-K{_K}-N{_N}-decode": functools.partial(mx4_forward, _K, _N, "bf16", "decode"),
        f"mx4-K{_K}-N{_N}-fp8": functools.partial(mx4_forward, _K, _N, "fp8"),
        f"mx4-K{_K}-N{_N}-fp4": functools.partial(mx4_forward, _K, _N, "fp4"),
        f"mx4-K{_K}-N{_N}-glu-tile": functools.partial(mx4_gated, _K, _N, "tile"),
        f"mx4-K{_K}-N{_N}-glu-decode": functools.partial(mx4_gated, _K, _N, "decode"),
        f"mx4-K{_K}-N{_N}-bwd": functools.partial(mx4_backward, _K, _N),
    })
    for _prec in ("fp8", "fp4", "fp6"):                             # the block-scaled precisions, both forms pinned
        for _form in ("tile", "decode"):
            FAMILIES[f"mx4-K{_K}-N{_N}-{_prec}-{_form}"] = functools.partial(mx4_forward, _K, _N, _prec, _form)
    FAMILIES[f"mx4-K{_K}-N{_N}-fp6-glu-decode"] = functools.partial(mx4_gated, _K, _N, "decode", "fp6")
for _K, _N, _r in ((288, 136, 16), (96, 37, 64)):                   # (r = 16: one 16-j step of the adapter stage, 64: all four)
    for _kind in ("fwd", "glu", "bwd"):
        FAMILIES[f"mx4-lora-{_kind}-K{_K}-N{_N}-r{_r}"] = functools.partial(mx4_lora, _K, _N, _r, _kind)
for _K, _N in ((288, 136), (96, 37), (608, 37)):                    # (K = 608: the decode ring's steady state, 9 pairs)
    for _form in ("tile", "decode"):
        FAMILIES[f"nv4-K{_K}-N{_N}-{_form}"] = functools.partial(nv4_forward, _K, _N, _form)
for _K, _N in ((288, 136), (96, 37)):
    for _form in ("tile", "decode"):
        FAMILIES[f"nv4-K{_K}-N{_N}-glu-{_form}"] = functools.partial(nv4_gated, _K, _N, _form)
    FAMILIES[f"nv4-K{_K}-N{_N}-bwd"] = functools.partial(nv4_backward, _K, _N)
for _K, _N, _r in ((288, 136, 16), (96, 37, 64)):                   # (the MXFP4 adapter families' shapes)
    for _kind in ("fwd", "glu", "bwd"):
        FAMILIES[f"nv4-lora-{_kind}-K{_K}-N{_N}-r{_r}"] = functools.partial(nv4_lora, _K, _N, _r, _kind)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_one_graph_serves_every_routing(tune, name):
    replay_scenes(FAMILIES[name](), tune)


# ---- the dense MXFP4 linear op: no expert table; two launches (three when gated) and a partial-sum workspace

LINEAR_T, LINEAR_N = 2, 136
LINEAR_CASES = {"plain-K288-S4": (288, 4, False), "gated-K288-S4": (288, 4, True), "plain-K96-S16": (96, 16, False)}


def linear_case(name, tune):
    """(call(rows) -> [T, N] float32, make_rows(seed), reference(rows) -> float64, bound or None) of one of LINEAR_CASES,
    with the split range opened and S forced (the kernel the library then reports is asserted).  Plain: the integer recipe
    of tests/test_gpu_mxfp4_linear.py, rows in [-4, 4], scale codes 125 .. 129, a bias in [-8, 8], every sum below 2^17
    (asserted): the float32 result is the float64 reference whatever the order of the S partial sums.  Gated: Gaussian
    gate | up rows; the reference is the float64 product of the bfloat16 h the grouped gated op itself forms (that file's
    own_hidden, asserted here to lie within one bfloat16 rounding of the float64 h), at that file's Gaussian bound.  At
    K = 96 there is one pair of blocks and an odd one: S = 16 leaves fourteen slices with nothing to do."""
    K, S, gated = LINEAR_CASES[name]
    T, N = LINEAR_T, LINEAR_N
    tune(linear=(128, S))
    got = lib().fql_tune_mx4_linear_kernel(T, K, N)
    assert (got >> 8, got & 0xFF) == (S, 2), f"the library reports (S, form) = {(got >> 8, got & 0xFF)}, the test is written for {(S, 2)}"
    p = linear_problem(K, N, integer=not gated)
    W, bias64 = p["W"].to(DEV), p["bias"].double()

    def make_rows(seed):
        g = gen(seed, K, N, S)
        return (2.0 * torch.randn(T, 2 * K, generator=g) if gated else torch.randint(-4, 5, (T, K), generator=g).float()).to(DEV)

    def call(rows):
        if gated:
            return ops().linear_gated_forward_mxfp4(p["blocks"], p["scales"], rows, bias=p["bias"], out_dtype=torch.float32,
                                                    split_k=True, **act_kw("swiglu_clamp"))
        return ops().linear_forward_mxfp4(p["blocks"], p["scales"], rows, bias=p["bias"], out_dtype=torch.float32, split_k=True)

    def reference(rows):
        if not gated:
            ref = rows.double() @ W.T + bias64
            assert float(ref.abs().max()) < 2 ** 17
            return ref
        h, h64 = linear_own_hidden(rows, "swiglu_clamp").double(), hidden64("swiglu_clamp", rows, ALPHA, LIMIT)
        assert bool(((h - h64).abs() <= 2.0 ** -8 * h64.abs() + 2.0 ** -126).all())
        return h @ W.T + bias64
    return call, make_rows, reference, linear_bound(K) if gated else None


@pytest.mark.parametrize("name", list(LINEAR_CASES))
def test_dense_linear_split_form_replays(tune, name):
    """ops.linear_forward_mxfp4 / linear_gated_forward_mxfp4(split_k=True) at T = 2, N = 136, captured once and replayed
    over four row sets, the last equal to the first, with SENT in the output before each replay.  The split form is
    mx4_linear_decode_kernel into partial[S][T][N] and then mx4_linear_reduce_kernel, behind the pre-pass that writes h in
    the gated entry; the launch boundaries are the only synchronisation and the workspace lives in the graph's pool.  A
    launch that left the capture stream is a capture error or a node missing from the graph, which shows as SENT or as the
    previous row set's sums."""
    call, make_rows, reference, bound = linear_case(name, tune)
    static = make_rows(0).clone()
    graph, out, _ = capture(call, [static])
    try:
        first = None
        for i, seed in enumerate((0, 1, 2, 0)):
            rows = make_rows(seed)
            static.copy_(rows)
            out.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            eager = call(rows.clone())
            assert same_bits(got, eager), (i, first_diff(got, eager))
            ref = reference(rows)
            if bound is None:
                assert torch.equal(got.double(), ref), f"replay {i}: not the exact integer result"
            else:
                err = rel_fro_dev(got, ref)
                print(f"dense linear {name} replay {i}: rel_fro {err:.3e} (bound {bound:.2e})")
                assert err <= bound, (i, err)
            if i == 0:
                first = got
            elif i < 3:
                assert not same_bits(got, first)                     # (the row sets are different problems)
        assert same_bits(got, first), "the first row set again does not carry the bits of its first replay"
    finally:
        del graph


# ---- the dense NVFP4 linear op: no expert table; the grouped launchers with E = 1 (the gated entry: a pre-pass in front)

NV4_LINEAR_T, NV4_LINEAR_K, NV4_LINEAR_N = 5, 96, 37


NV4_LINEAR_RANK = {"lora-fwd": 8, "lora-bwd": 32}      # (the two ranks the grouped adapter families do not run)


def nv4_linear_case(kind):
    """(call(*rows) -> [T, N] float32 ([T, K]: "lora-bwd"), make_rows(seed) -> the tuple of row tensors, reference(rows) ->
    float64, bound or None) of ``kind`` "plain", "gated", "lora-fwd" or "lora-bwd": expert 3's matrix, global scale and bias
    of the grouped NVFP4 families as a dense layer.  Plain: the integer recipe, exact.  Gated: Gaussian gate | up rows
    against the bfloat16-rounded float64 h at NV4_GATED_BOUND.  The adapter entries (ops.linear_forward_nvfp4_lora with the
    bias on rows (x, v), ops.linear_backward_input_nvfp4_lora on (gy, dv)): the integer recipe of nv4_lora with the global
    scale NV4_LORA_GS[3] on the weight term only, exact (nv4_lora_exact64)."""
    T, K, N = NV4_LINEAR_T, NV4_LINEAR_K, NV4_LINEAR_N
    gated = kind == "gated"
    p, W = nv4_weights(K, N, not gated)
    e = 3
    blocks, scales, gs, bias = p["blocks"][e], p["scales"][e], p["gs"][e:e + 1], p["bias"][e]
    if kind in NV4_LINEAR_RANK:
        r, bwd = NV4_LINEAR_RANK[kind], kind == "lora-bwd"
        C, g_e = (N if bwd else K), NV4_LORA_GS[e]
        gs = torch.tensor([g_e], device=DEV)
        M = torch.randint(-2, 3, (r, K) if bwd else (N, r), generator=gen(0, K, N, r, 19)).float().to(DEV)
        We, Me = (W[e], M.double()) if bwd else (W[e].t(), M.double().t())

        def make_rows(seed):
            g = gen(seed, K, N, r, 20 + bwd)
            return torch.randint(-4, 5, (T, C), generator=g).float().to(DEV), torch.randint(-4, 5, (T, r), generator=g).float().to(DEV)

        def call(rows, v):
            if bwd:
                return ops().linear_backward_input_nvfp4_lora(blocks, scales, gs, rows, v, M)
            return ops().linear_forward_nvfp4_lora(blocks, scales, gs, rows, v, M, bias=bias, out_dtype=torch.float32)

        def reference(rows):
            x64, v64 = rows[0].double(), rows[1].double()
            add = v64 @ Me
            assert bool(add.count_nonzero())                         # (the adapter matters)
            return nv4_lora_exact64((x64 @ We, x64.abs() @ We.abs()), (add, v64.abs() @ Me.abs()), g_e,
                                    None if bwd else bias.double())
        return call, make_rows, reference, None

    def make_rows(seed):
        g = gen(seed, K, N, 14 + gated)
        return ((2.0 * torch.randn(T, 2 * K, generator=g) if gated else torch.randint(-4, 5, (T, K), generator=g).float()).to(DEV),)

    def call(rows):
        if gated:
            return ops().linear_gated_forward_nvfp4(blocks, scales, gs, rows, bias=bias, out_dtype=torch.float32,
                                                    **act_kw("swiglu_clamp"))
        return ops().linear_forward_nvfp4(blocks, scales, gs, rows, bias=bias, out_dtype=torch.float32)

    def reference(rows):
        x64 = hidden64("swiglu_clamp", rows[0], ALPHA, LIMIT).bfloat16().double() if gated else rows[0].double()
        acc = x64 @ W[e].t()
        assert gated or float(acc.abs().max()) < 2 ** 16
        return nv4_epilogue(acc, gs[0], bias)
    return call, make_rows, reference, NV4_GATED_BOUND if gated else None


@pytest.mark.parametrize("kind", ["plain", "gated", "lora-fwd", "lora-bwd"])
def test_dense_nvfp4_linear_replays(kind):
    """ops.linear_forward_nvfp4 / linear_gated_forward_nvfp4 and the adapter entries ops.linear_forward_nvfp4_lora (r = 8) /
    linear_backward_input_nvfp4_lora (r = 32) at K = 96, N = 37, T = 5, captured once and replayed over four row sets, the
    last equal to the first, with SENT in the output before each replay: each replay is the eager result bit for bit, the
    reference (exactly, but for the gated entry: within its bound), and has overwritten every SENT.  The gated entry's
    pre-pass writes h into a workspace of the graph's pool in front of the GEMM; a launch that left the capture stream is a
    capture error or a node missing from the graph, which shows as SENT or as the previous row set's result."""
    call, make_rows, reference, bound = nv4_linear_case(kind)
    static = [t.clone() for t in make_rows(0)]
    graph, out, _ = capture(call, static)
    try:
        first = None
        for i, seed in enumerate((0, 1, 2, 0)):
            rows = make_rows(seed)
            for s, t in zip(static, rows):
                s.copy_(t)
            out.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            eager = call(*[t.clone() for t in rows])
            assert same_bits(got, eager), (i, first_diff(got, eager))
            ref = reference(rows)
            assert torch.equal(got == SENT, ref.float() == SENT), f"replay {i}: an element still holds the sentinel"
            if bound is None:
                assert torch.equal(got.double(), ref), f"replay {i}: not the exact integer result"
            else:
                err = rel_fro_dev(got, ref)
                print(f"dense nvfp4 linear gated replay {i}: rel_fro {err:.3e} (bound {bound:.2e})")
                assert err <= bound, (i, err)
            if i == 0:
                first = got
            elif i < 3:
                assert not same_bits(got, first)                     # (the row sets are different problems)
        assert same_bits(got, first), "the first row set again does not carry the bits of its first replay"
    finally:
        del graph


# ---- the scratch of the two-phase API, first taken inside a capture

def test_first_gemm_i8_inside_a_capture_then_eager_then_replay():
    """ops.gemm_scratch caches one buffer per (device, stream).  With an empty cache the first gemm_i8 of the precision
    happens inside the capture: its buffer is keyed to the capture stream and lives in the graph's private pool.  A replay,
    an eager call on the default stream, an eager call on the capture stream (which finds that buffer) and a second replay
    must agree bit for bit, and with the float64 reference."""
    o = ops()
    fam = FAMILIES["int4-two-phase-T100"]()
    assert lib().fql_gemm_scratch_bytes(o._precision("exact")) > 0
    tpe, offs = (t.to(DEV) for t in tab(fam.T, *fam.ragged))
    rows = fam.make_rows(3)
    static = [rows[0].clone(), tpe.clone(), offs.clone()]
    saved = dict(o._SCRATCH)
    graph = None
    try:
        graph, out, s = capture(fam.call, static, after_warmup=o._SCRATCH.clear)
        assert [k[1] for k in o._SCRATCH] == [s.cuda_stream]        # taken inside the capture, keyed to its stream
        results = {}
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        results["first replay"] = out.clone()
        results["eager, default stream"] = fam.call(rows[0].clone(), tpe.clone(), offs.clone())
        torch.cuda.synchronize()
        assert len(o._SCRATCH) == 2
        with torch.cuda.stream(s):
            results["eager, capture stream"] = fam.call(rows[0].clone(), tpe.clone(), offs.clone())
        torch.cuda.synchronize()
        assert len(o._SCRATCH) == 2
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        results["second replay"] = out.clone()
        for what, r in results.items():
            assert same_bits(r, results["first replay"]), what
        fam.check("two-phase, scratch first taken inside the capture", out, rows, tpe, offs)
    finally:
        del graph
        o._SCRATCH.clear()
        o._SCRATCH.update(saved)


# ---- the whole block: the routing changes by itself

BE, BH, BF, BTOPK = 4, 64, 96, 2
BRANK = 16                          # the rank of the "mxfp4-lora" and "nvfp4-lora" blocks' adapters


def block_weights():
    g = torch.Generator().manual_seed(41)
    r = lambda *shape, s=0.1: torch.randn(*shape, generator=g) * s
    many = lambda *shape, s=0.1: [r(*shape, s=s) for _ in range(BE)]
    return dict(gate_w=r(BE, BH, s=0.5), router_bias=r(BE, s=0.1), gate=many(BF, BH), up=many(BF, BH), down=many(BH, BF),
                gb=many(BF, s=0.3), ub=many(BF, s=0.3), db=many(BH, s=0.3), shared=(r(64, BH), r(64, BH), r(BH, 64)))


def build_block(kind, capped):
    """E = 4, H = 64, F = 96, top-2, a router bias; ``kind``: "int4", "int4-shared", "mxfp4", "mxfp4-lora", "nvfp4" or
    "nvfp4-lora" experts (swiglu_clamp with expert biases; "nvfp4": NVFP4MoEFFN, whose from_weights gives every expert global
    scales of its own; "mxfp4-lora" / "nvfp4-lora": LoRAMXFP4MoEFFN / LoRANVFP4MoEFFN of rank BRANK around the same MXFP4 /
    NVFP4 experts, with random values in BOTH B matrices -- a fresh adapter has B = 0 and would test nothing); ``capped``:
    capacity_factor = 1 (the forward then takes a token mask too)."""
    w = block_weights()
    factor = 1.0 if capped else None
    if kind in ("mxfp4", "mxfp4-lora", "nvfp4", "nvfp4-lora"):
        if kind in ("nvfp4", "nvfp4-lora"):
            experts = fq().NVFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gb"], up_bias=w["ub"],
                                                    down_bias=w["db"], input_grad=kind == "nvfp4-lora", **act_kw("swiglu_clamp"))
            assert len(set(experts.gate_up_global.tolist())) > 1 and len(set(experts.down_global.tolist())) > 1
        else:
            experts = fq().MXFP4MoEFFN.from_weights(w["gate"], w["up"], w["down"], gate_bias=w["gb"], up_bias=w["ub"],
                                                    down_bias=w["db"], input_grad=kind == "mxfp4-lora", **act_kw("swiglu_clamp"))
        if kind in ("mxfp4-lora", "nvfp4-lora"):
            torch.manual_seed(43)                                    # (the adapters' A)
            wrap = fq().LoRAMXFP4MoEFFN if kind == "mxfp4-lora" else fq().LoRANVFP4MoEFFN
            experts = wrap.from_layer(experts, BRANK, alpha=2.0 * BRANK)
            g = torch.Generator().manual_seed(44)
            with torch.no_grad():
                experts.gate_up_lora_B.copy_(torch.randn(experts.gate_up_lora_B.shape, generator=g) * 0.2)
                experts.down_lora_B.copy_(torch.randn(experts.down_lora_B.shape, generator=g) * 0.2)
        m = fq().QuantizedSparseMoEBlock(BE, BH, BF, top_k=BTOPK, experts=experts, router_bias=True, capacity_factor=factor)
        with torch.no_grad():
            m.gate.weight.copy_(w["gate_w"])
            m.gate.bias.copy_(w["router_bias"])
        return m.to(DEV)
    return fq().QuantizedSparseMoEBlock.from_weights(
        w["gate_w"], w["gate"], w["up"], w["down"], top_k=BTOPK, router_bias=w["router_bias"], activation="swiglu_clamp",
        gate_bias=w["gb"], up_bias=w["ub"], down_bias=w["db"], shared=w["shared"] if kind == "int4-shared" else None,
        capacity_factor=factor).to(DEV)


def block_reference(m, x, mask):
    """(out float64, indices, envelope): the dense restatement of tests/test_gpu_sparse_moe_block_capped.py -- a float64
    torch router, the drops of test_route_capped_cpu.plan_reference, the rows of the kept slots through the same expert
    module in expert order, a dense float64 sum of keep * w_k * y_k plus the shared term."""
    T = x.shape[0]
    logits = m.router_logits(x).double()
    idx = torch.sort(-logits, dim=-1, stable=True).indices[:, :BTOPK]
    sel = torch.softmax(logits, dim=-1).gather(1, idx)
    w = (sel / sel.sum(dim=-1, keepdim=True)).float()
    counts, offsets, token_of_sorted, pos, _ = plan_reference(idx, BE, m.expert_capacity(T), mask)
    keep = (pos >= 0).view(T, BTOPK)
    y = m.experts(x[token_of_sorted.long()], counts, offsets)
    yk = y.double()[pos.clamp(min=0).long()].view(T, BTOPK, BH)
    terms = w.double().unsqueeze(-1) * keep.unsqueeze(-1) * yk
    out = terms.sum(dim=1)
    s, _ = m.shared_output(x)
    if s is not None:
        out = out + s.double()
    return out, idx, terms.abs().sum(dim=1) + (0 if s is None else s.double().abs()), keep, w


def ffn64(mod, e, x64, mx4, raw64=None):
    """float64 [T, H]: expert ``e`` of a gated FFN module on every row of ``x64``, on its dequantised weights, with no
    kernel of the library and no expert table: gate_up (+ bias), swiglu_clamp, down (+ bias).  ``mx4``: the roundings of
    tests/test_gpu_mxfp4.py's block reference (gate_up kept in float32, h rounded to bfloat16); NVFP4 experts (a module with
    ``gate_up_global``) are dequantize_nvfp4 times the expert's global scale, in float64.  A module with adapters
    (``raw64``: the rows before their rounding to bfloat16) adds the two adapter terms with the kernels' roundings: the
    shrunk rows v = s A x (ops.lora_shrink on the unrounded rows) and v = s A h (ops.lora_gated_shrink on the float32 h)
    kept in float32, then v and B rounded to bfloat16 on their way into the GEMM."""
    lora = hasattr(mod, "gate_up_lora_A")
    term = lambda rows, A, B: (mod.scaling * (rows @ A[e].double().t())).float().bfloat16().double() @ B[e].bfloat16().double().t()
    if mx4 and hasattr(mod, "gate_up_global"):
        from fused_int4_amd.quantize import dequantize_nvfp4
        Wgu = dequantize_nvfp4(mod.gate_up_blocks[e:e + 1].cpu(), mod.gate_up_scales[e:e + 1].cpu())[0].double().to(DEV) \
            * mod.gate_up_global[e].double()
        Wd = dequantize_nvfp4(mod.down_blocks[e:e + 1].cpu(), mod.down_scales[e:e + 1].cpu())[0].double().to(DEV) \
            * mod.down_global[e].double()
    elif mx4:
        from fused_int4_amd.quantize import dequantize_mxfp4
        Wgu = dequantize_mxfp4(mod.gate_up_blocks[e:e + 1].cpu(), mod.gate_up_scales[e:e + 1].cpu())[0].double().to(DEV)
        Wd = dequantize_mxfp4(mod.down_blocks[e:e + 1].cpu(), mod.down_scales[e:e + 1].cpu())[0].double().to(DEV)
    else:
        Wgu = dequant_f64(mod.gate_up_packed[e], mod.gate_up_scales[e], mod.gate_up_zero_points[e])
        Wd = dequant_f64(mod.down_packed[e], mod.down_scales[e], mod.down_zero_points[e])
    b_gu, b_d = getattr(mod, "gate_up_bias", None), getattr(mod, "down_bias", None)
    gu = x64 @ Wgu.t() + (0 if b_gu is None else b_gu[e].double())
    if lora:
        gu = gu + term(raw64, mod.gate_up_lora_A.detach(), mod.gate_up_lora_B.detach())
    h = hidden64("swiglu_clamp", gu.float() if mx4 else gu, ALPHA, LIMIT)
    y = (h.bfloat16().double() if mx4 else h) @ Wd.t() + (0 if b_d is None else b_d[e].double())
    return y + term(h, mod.down_lora_A.detach(), mod.down_lora_B.detach()) if lora else y


def block_float64(m, x, idx, keep, w, mx4):
    """The block in float64 torch alone, given the float64 router's choice: sum_k keep * w_k * FFN_e(k)(x) + shared."""
    x64 = x.bfloat16().double() if mx4 else x.double()
    out = torch.zeros(x.shape[0], BH, dtype=torch.float64, device=DEV)
    for e in range(BE):
        y = ffn64(m.experts, e, x64, mx4, x.double())
        for k in range(BTOPK):
            sel = (idx[:, k] == e) & keep[:, k]
            out[sel] += w[sel, k].double().unsqueeze(-1) * y[sel]
    shared = getattr(m, "shared_experts", None)
    return out if shared is None else out + ffn64(shared, 0, x64, False)


@pytest.mark.parametrize("T", [3, 130])
@pytest.mark.parametrize("kind,capped", [("int4", False), ("int4", True), ("int4-shared", True), ("mxfp4", False),
                                         ("mxfp4", True), ("mxfp4-lora", False), ("mxfp4-lora", True), ("nvfp4", False),
                                         ("nvfp4", True), ("nvfp4-lora", False), ("nvfp4-lora", True)],
                         ids=["int4", "int4-capped", "int4-shared-capped", "mxfp4", "mxfp4-capped", "mxfp4-lora",
                              "mxfp4-lora-capped", "nvfp4", "nvfp4-capped", "nvfp4-lora", "nvfp4-lora-capped"])
def test_block_replays_under_changing_routing(tune, kind, capped, T):
    """QuantizedSparseMoEBlock under torch.no_grad(), captured once; then new tokens, the router bias overwritten in place
    so that every token picks experts 2 and 0, a mask with one real token (the capped blocks) and the first scene again.
    "mxfp4-lora": the same MXFP4 experts inside LoRAMXFP4MoEFFN with both B matrices random (its output is asserted once to
    differ from the "mxfp4" block's); the pure-float64 check adds the two adapter terms with the kernels' roundings
    (ffn64) and is held to the MXFP4 block's own bound, MX4_GATED_BOUND, unscaled.  "nvfp4": NVFP4MoEFFN experts; the
    pure-float64 check multiplies the dequantised weights by the experts' global scales and is held to the same unscaled
    MX4_GATED_BOUND (DESIGN.md section 40 has the measured values: no constant of its own).  "nvfp4-lora": those NVFP4
    experts inside LoRANVFP4MoEFFN, both B matrices random (the output is asserted once to differ from the "nvfp4"
    block's); ffn64 applies the global scales to the weight term and not to the adapter terms; the same unscaled bound."""
    m, mx4 = build_block(kind, capped), kind in ("mxfp4", "mxfp4-lora", "nvfp4", "nvfp4-lora")
    bias0 =m.gate.bias.detach().clone()
    same_two = torch.tensor([60.0, -60.0, 120.0, -60.0], device=DEV)      # (the logits without it stay within +-20)
    xs = [torch.randn(T, BH, generator=gen(i, T)).to(DEV) for i in range(3)]
    every = torch.ones(T, dtype=torch.bool, device=DEV)
    some = torch.rand(T, generator=gen(9, T)).to(DEV) < 0.75 if T > 3 else torch.tensor([True, False, True], device=DEV)
    one = torch.zeros(T, dtype=torch.bool, device=DEV)
    one[T // 2] = True
    scenes_ = [("first", xs[0], bias0, some), ("new tokens", xs[1], bias0, every), ("one pair of experts", xs[2], same_two, some),
               ("one real token", xs[1], bias0, one), ("first again", xs[0], bias0, some)]
    if not capped:
        scenes_ = [s for s in scenes_ if s[0] != "one real token"]
    static_x, static_mask = xs[0].clone(), some.clone()
    run = (lambda x, mask: m(x, token_mask=mask)) if capped else (lambda x, mask: m(x))
    graph = None
    with torch.no_grad():
        try:
            graph, (out, logits), _ = capture(run, [static_x, static_mask])
            first = None
            for name, x, bias, mask in scenes_:
                static_x.copy_(x)
                static_mask.copy_(mask)
                m.gate.bias.copy_(bias)
                out.fill_(SENT)
                logits.fill_(SENT)
                graph.replay()
                torch.cuda.synchronize()
                got, got_logits = out.clone(), logits.clone()
                eager, eager_logits = run(x.clone(), mask.clone())
                assert same_bits(got, eager) and same_bits(got_logits, eager_logits), (name, first_diff(got, eager))
                used = mask if capped else None
                ref, idx, envelope, keep, w = block_reference(m, x, used)
                _, got_idx = ops().router_topk(got_logits, BTOPK)
                assert torch.equal(got_idx.long(), idx), name
                if name == "one pair of experts":
                    assert got_idx.tolist() == [[2, 0]] * T
                err, bound = float(torch.linalg.vector_norm(got.double() - ref)), BLOCK_REL * float(torch.linalg.vector_norm(envelope))
                print(f"block {kind} capped={capped} T={T} {name}: ||out - ref||_F {err:.3e}, bound {bound:.3e}")
                assert err <= bound, name
                # ... and against float64 torch alone (no kernel, no table: a mistake the expert module shares with the
                # block cannot hide), at the bound the experts' own tests hold their layer to
                pure, pure_bound = rel_fro_dev(got, block_float64(m, x, idx, keep, w, mx4)), MX4_GATED_BOUND if mx4 else FFN_REL_FRO
                print(f"block {kind} capped={capped} T={T} {name}: rel_fro against float64 torch {pure:.3e}, "
                      f"bound {pure_bound:.1e}")
                assert pure < pure_bound, name
                if capped and kind != "int4-shared":
                    assert not got[~mask].any(), name                # a masked token's output is zero
                if name == "first":
                    first = (got, got_logits)
                    if kind in ("mxfp4-lora", "nvfp4-lora"):         # (the adapters matter: not the wrapped experts' output)
                        plain = build_block(kind[:-5], capped)
                        other = plain(x.clone(), token_mask=mask.clone())[0] if capped else plain(x.clone())[0]
                        print(f"block {kind} capped={capped} T={T}: rel_fro to the {kind[:-5]} block's output {rel_fro_dev(got, other):.3e}")
                        assert other.shape == got.shape and not same_bits(got, other)
            assert same_bits(got, first[0]) and same_bits(got_logits, first[1])
        finally:
            del graph
            m.gate.bias.copy_(bias0)
