"""Where the forward kernels write, and what else they read.

The value tests hand every kernel a ``torch.empty`` output and a workspace the caching allocator rounded up, whose
neighbours are other live tensors: a store one row past the output, a store past the workspace that
``fql_*_workspace_bytes()`` promises is enough, or a result that depends on stale workspace bytes would go unnoticed.
Here every pointer of a call is the test's own, through the C ABI (include/fql_int4.h, include/fql_int4_tune.h):

  * every buffer is the interior of a larger allocation with 64 KiB of guard on each side (helpers.Guarded): outputs
    between a sentinel no result can be, inputs between values that would show if they were used (NaN, 0xFF weights,
    huge indices), the workspace at exactly the promised size, 16 bytes past a 256-byte boundary; activations and
    outputs both 16-byte aligned (the hot path: vector loads and stores) and one element past such a boundary (the
    scalar pre-pass and the scalar store form of every epilogue), the packed weights 16-byte aligned (the matrix-core
    path refuses less), everything else element-aligned;
  * (a) after the call every guard still holds its pattern, and rows no expert covers are zero (product entry points)
    or still the sentinel (tuning hooks);
  * (b) the interior matches the float64 oracle at the tolerance the suite already states for that path (the constants
    of helpers.py: none is defined here), 16-bit outputs bit for bit the float32 run rounded once;
  * (c) the same call with the workspace prefilled with 0x00, 0xFF (NaN as float32, -1 as limbs) and 0x7F (huge deltas,
    limbs of 127) returns the same bits; the one-launch form a fourth time on what its previous run left behind.

A load that is fetched and then masked away cannot be seen this way, and is not looked for.

The problems are the smallest at which padding, tails and the row-tile classes all engage: G1 = 5 experts of
[129, 0, 1, 65, 33] rows plus 3 uncovered (classes of 128, 64 and 32 rows, a split remainder, an empty expert), G2 = one
expert of 129 rows and sixteen of 1 (every group leaves a nearly empty 32-row block: the worst case of row_blocks() and
m_slots), G1c = G1 with a last range that leaves [0, T); K = 544 (Kp = 768: not a multiple of 256, and the
one-wave-per-SIMD kernel's Kp >= 512), N = 200 (a 192-column tile and an 8-column rest) or 72.  In the 3- and 2-limb
runs every fifth row is heavy-tailed, so the residual limb set and the scratch behind the workspace are in use."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import (EXACT_REL_FRO, FAST_REL_FRO, FMA_REL_FRO, INT8_REL_FRO, INT8_REL_FRO_LARGE_K, FP8_ACC_REL_FRO, rel_fro,
                     rel_fro_dev, dequant_f64, clipped_ranges, Guarded, guarded_like, assert_guards_intact, GUARD_BYTES,
                     NAN, SENT, BIG, same_bits, first_diff, heavy_rows, footprint_table)
from oracle import oracle as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

PREC = {"default": 0, "int8": 1, "fast": 2, "exact": 3, "fp8": 8}
LIMBS = {"default": 3, "exact": 3, "fast": 2, "int8": 1, "fp8": 1}
TOL = {"default": EXACT_REL_FRO, "exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "int8": INT8_REL_FRO, "fp8": FP8_ACC_REL_FRO}
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
DT_NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
WS_PATTERN = 0x5A
PREFILLS = (0x00, 0xFF, 0x7F)
K = 544


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fused_int4_amd import _native
    h = _native.lib()
    void, i32 = ctypes.c_void_p, ctypes.c_int
    h.fql_tune_gemm_i8.restype = i32
    h.fql_tune_gemm_i8.argtypes = [i32] + [void] * 9 + [i32, void, void] + [i32] * 5 + [void, void, ctypes.c_size_t]
    for name in ("fql_tune_is_config", "fql_tune_chosen_cfg", "fql_tune_num_configs", "fql_tune_num_rows32_configs",
                 "fql_tune_num_rows16_configs", "fql_tune_num_w4_configs", "fql_tune_set_compute_units", "fql_tune_set_fused",
                 "fql_tune_set_fused_spin"):
        getattr(h, name).restype = i32
    return h


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------ problems (built once, never modified)
class Problem:
    pass


@functools.lru_cache(maxsize=None)
def moe_problem(name, N=None):
    p = Problem()
    rng = np.random.default_rng({"G1": 11, "G1c": 11, "G2": 12}[name] + (N or 0))
    p.counts, p.offs, p.T = footprint_table(name)           # (the table the device gets: G1c is clipped there)
    p.name, p.E, p.K, p.N = name, len(p.counts), K, N or (72 if name == "G2" else 200)
    ranges = clipped_ranges(torch.from_numpy(p.counts), torch.from_numpy(p.offs), p.T)
    p.ref_counts = np.array([hi - lo for lo, hi in ranges], np.int32)     # ... and the one the oracle gets
    p.ref_offs = np.array([lo for lo, hi in ranges], np.int32)
    p.covered = np.zeros(p.T, bool)
    for lo, hi in ranges:
        p.covered[lo:hi] = True
    assert p.covered.all() == (name != "G1")
    if p.N <= 256:
        q = [O.quantize_weights((rng.standard_normal((p.N, K)) * 0.02).astype(np.float32)) for _ in range(p.E)]
        p.P, p.S, p.Z = (np.stack([t[i] for t in q]) for i in range(3))
    else:                                                   # (a wide problem: the codes drawn directly, no quantiser pass)
        p.P = rng.integers(0, 256, size=(p.E, p.N, K // 2), dtype=np.uint8)
        p.S = (0.001 + 0.002 * rng.random((p.E, p.N))).astype(np.float32)
        p.Z = rng.integers(5, 11, size=(p.E, p.N)).astype(np.float32)
    p.x_plain = rng.standard_normal((p.T, K)).astype(np.float32)
    p.x_heavy = heavy_rows(p.x_plain.copy(), rng)
    return p


def moe_x(p, prec):
    return p.x_heavy if LIMBS[prec] >= 2 else p.x_plain


@functools.lru_cache(maxsize=None)
def moe_ref(name, heavy, N=None):
    p = moe_problem(name, N)
    x = p.x_heavy if heavy else p.x_plain
    if p.N <= 256:
        return C.moe_grouped(p.P, p.S, p.Z, x, p.ref_counts, p.ref_offs)
    ref = torch.zeros(p.T, p.N, dtype=torch.float64, device="cuda")       # wide: float64 dequantize-then-matmul on the device
    xd = torch.from_numpy(x).cuda().double()
    for e, (lo, c) in enumerate(zip(p.ref_offs, p.ref_counts)):
        if c:
            W = dequant_f64(torch.from_numpy(p.P[e]).cuda(), torch.from_numpy(p.S[e]), torch.from_numpy(p.Z[e]))
            ref[lo:lo + c] = xd[lo:lo + c] @ W.T
    return ref.cpu().numpy()


class Weights:
    """packed / scales / zps (+ the expert table) of a problem, each inside guards."""

    def __init__(self, P, S, Z, counts=None, offs=None):
        self.P = guarded_like("packed", P, 0xFF, offset=16)          # (the matrix-core path needs 16-byte aligned weights)
        self.S = guarded_like("scales", S, NAN)
        self.Z = guarded_like("zps", Z, NAN)
        self.all = [self.P, self.S, self.Z]
        self.cnt = self.off = None
        if counts is not None:
            self.cnt = guarded_like("tokens_per_expert", counts, BIG)
            self.off = guarded_like("input_offsets", offs, BIG)
            self.all += [self.cnt, self.off]


def workspace(nbytes):
    return Guarded("workspace", nbytes, torch.uint8, WS_PATTERN, offset=16) if nbytes else None


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


ALIGNS = ["aligned", "element"]


def off(align, dtype):
    """Where an activation or output buffer starts, past a 256-byte boundary: 16 bytes (the hot path: 16-byte loads in
    the pre-pass, vector stores in every epilogue) or one element (the least the entry points accept: the scalar pre-pass
    and the scalar store form of every epilogue)."""
    return 16 if align == "aligned" else esize(dtype)


def output(T, N, dtype, offset=16):
    return Guarded("out", T * N * esize(dtype), dtype, SENT, offset=offset)


def flag_words(lib, ws, T, E, prec="default"):
    """The row-group flag words of the one-launch form inside a 3-limb product workspace: carve() (csrc/fql_int4.hip)
    lays out limbs, delta [3][T], rowsum [2][3][T], then (T + 3) / 4 words of 8 bytes, each part rounded up to 16 bytes."""
    r16 = lambda n: (n + 15) // 16 * 16
    lb = lib.fql_act_limb_bytes(T, E, K, PREC[prec])
    start = lb + r16(3 * T * 4) + r16(2 * 3 * T * 4)
    return ws.bytes()[start:start + (T + 3) // 4 * 8]


def run_prefills(what, call, ws, out, dtype, shape, bufs, stale_rerun=False):
    """(a) + (c): the call once per workspace prefill (and once more on what the last run left, for the one-launch
    form), guards checked after every run, the outputs compared bit for bit.  Returns the first output."""
    bufs = [b for b in bufs if b is not None] + [b for b in (ws, out) if b is not None]
    outs, fills = [], list(PREFILLS) + (["left by the previous run"] if stale_rerun else [])
    for fill in fills:
        if ws is not None and isinstance(fill, int):
            ws.bytes().fill_(fill)
        o = out.view(dtype, *shape)
        o.fill_(SENT)
        rc = call(ws.ptr if ws is not None else None, ws.nbytes if ws is not None else 0, out.ptr)
        tag = f"{what}, workspace {fill:#04x}" if isinstance(fill, int) else f"{what}, workspace {fill}"
        assert rc == 0, (tag, rc)
        assert_guards_intact(*bufs, what=tag)
        outs.append(o.clone())
        if ws is None:
            break
    for fill, o in zip(fills[1:], outs[1:]):
        assert same_bits(o, outs[0]), f"{what}: the result depends on stale workspace bytes: prefill {fill} against " \
                                      f"{fills[0]:#04x}: (differing elements, first) = {first_diff(o, outs[0])}"
    return outs[0]


def check_values(what, got, ref, tol, covered=None, uncovered=0.0):
    g = got.float().cpu().numpy()
    covered = np.ones(g.shape[0], bool) if covered is None else covered
    assert np.isfinite(g).all(), what
    err = rel_fro(g[covered], np.asarray(ref)[covered])
    print(f"{what}: {err:.3e} (bound {tol:.1e})")
    assert err < tol, (what, err)
    assert (g[~covered] == uncovered).all(), f"{what}: rows no expert covers must hold {uncovered}"


def delta_of(lib, ws, T, E, prec):
    """delta [sets + 1][T] inside a product workspace: the plane carve() (csrc/fql_int4.hip) puts behind the limbs."""
    lb = lib.fql_act_limb_bytes(T, E, K, PREC[prec])
    sets = 2 if LIMBS[prec] >= 2 and prec != "fp8" else 1
    return ws.bytes()[lb:lb + (sets + 1) * T * 4].view(torch.float32).view(sets + 1, T)


def assert_residual_in_use(lib, ws, p, prec, covered=None):
    if LIMBS[prec] < 2:
        return
    cov = torch.from_numpy(p.covered if covered is None else covered).cuda()
    flagged = int(((delta_of(lib, ws, p.T, p.E, prec)[1] != 0) & cov).sum())
    assert 0 < flagged < int(cov.sum()), flagged


# ------------------------------------------------------------------------------ the helper itself
def test_guard_violation_names_buffer_and_offsets(lib):
    g = Guarded("probe", 40, torch.float32, SENT, offset=4)
    assert g.ptr % 256 == 4 and g.start >= GUARD_BYTES and g.raw.numel() - g.end >= GUARD_BYTES
    g.view(torch.float32, 10).fill_(1.0)
    assert_guards_intact(g, what="interior writes")
    g.raw[g.end + 8] = 1
    g.raw[g.end + 19] = 1
    with pytest.raises(AssertionError, match=r"'probe'.*offset 48 \(8 bytes past its end\), last at 59 \(19 bytes past"):
        assert_guards_intact(g, what="two bytes behind")
    h = Guarded("front", 64, torch.uint8, 0xFF, offset=1)
    assert h.ptr % 256 == 1
    h.raw[h.start - 3] = 0
    with pytest.raises(AssertionError, match=r"'front'.*offset -3 \(3 bytes in front of it\)"):
        assert_guards_intact(h, what="one byte in front")


# ------------------------------------------------------------------------------ grouped (MoE) entry points
@pytest.mark.parametrize("prec", ["default", "fast", "int8"])
@pytest.mark.parametrize("name,align", [("G1", 16), ("G2", 16), ("G1c", 16), ("G1", 4)])
def test_moe_fwd_f32(lib, name, align, prec):
    """align = 4: x and out one float past a 16-byte boundary (scalar pre-pass, scalar stores)."""
    p = moe_problem(name)
    x = moe_x(p, prec)
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    gx = guarded_like("inputs", x, NAN, offset=align)
    ws = workspace(lib.fql_moe_workspace_bytes(p.E, p.T, K, p.N, PREC[prec]))
    out = output(p.T, p.N, torch.float32, align)
    what = f"fql_moe_fwd_f32 {name} {prec} align {align}"
    call = lambda wp, wb, op: lib.fql_moe_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gx.ptr, w.cnt.ptr, w.off.ptr, op, p.E, p.T, K,
                                                  p.N, PREC[prec], wp, wb, stream())
    got = run_prefills(what, call, ws, out, torch.float32, (p.T, p.N), w.all + [gx])
    check_values(what, got, moe_ref(name, LIMBS[prec] >= 2), TOL[prec], p.covered)
    assert_residual_in_use(lib, ws, p, prec)


IO_PAIRS = [(i, o) for i in DT for o in DT if (i, o) != (torch.float32, torch.float32)]    # (that pair is fql_moe_fwd_f32, above)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("in_dtype,out_dtype", IO_PAIRS, ids=[f"{DT_NAME[i]}-{DT_NAME[o]}" for i, o in IO_PAIRS])
def test_moe_fwd_16bit(lib, in_dtype, out_dtype, align):
    """Every pair of element types with a 16-bit side (fql_native_dtype_supported answers by shape, for all of them)."""
    p = moe_problem("G1")
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    assert lib.fql_native_dtype_supported(p.T, p.E, K, p.N, 0, w.P.ptr, 1) == 1
    xin = torch.from_numpy(p.x_heavy).to(in_dtype)
    gx = guarded_like("inputs", xin, NAN, offset=off(align, in_dtype))
    gx32 = guarded_like("inputs (widened)", xin.float(), NAN, offset=off(align, torch.float32))
    ws = workspace(lib.fql_moe_workspace_bytes(p.E, p.T, K, p.N, 0))

    def run(g, idt, odt):
        out = output(p.T, p.N, odt, off(align, odt))
        what = f"fql_moe_fwd G1 {DT_NAME[idt]} -> {DT_NAME[odt]} {align}"
        call = lambda wp, wb, op: lib.fql_moe_fwd(w.P.ptr, w.S.ptr, w.Z.ptr, g.ptr, DT[idt], w.cnt.ptr, w.off.ptr, op, DT[odt],
                                                  p.E, p.T, K, p.N, 0, wp, wb, stream())
        return what, run_prefills(what, call, ws, out, odt, (p.T, p.N), w.all + [g])

    what, base = run(gx32, torch.float32, torch.float32)
    ref = C.moe_grouped(p.P, p.S, p.Z, xin.float().numpy(), p.ref_counts, p.ref_offs)
    check_values(what, base, ref, EXACT_REL_FRO, p.covered)
    what, got = run(gx, in_dtype, out_dtype)
    assert same_bits(got, base.to(out_dtype)), (what, first_diff(got, base.to(out_dtype)))
    assert_residual_in_use(lib, ws, p, "default")


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("scaled", [False, True], ids=["gather", "gather_scaled"])
def test_moe_gather_fwd_f32(lib, scaled, align):
    """100 source tokens behind a random index; the scaled form is the only user of the third delta plane."""
    p = moe_problem("G1")
    rng = np.random.default_rng(21)
    n_src = 100
    tokens = heavy_rows(rng.standard_normal((n_src, K)).astype(np.float32), rng)
    index = rng.integers(0, n_src, size=p.T).astype(np.int32)
    rw = (0.1 + 0.9 * rng.random(p.T)).astype(np.float32)
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    gt, gi, gw = guarded_like("tokens", tokens, NAN, offset=off(align, torch.float32)), guarded_like("row_index", index, BIG), guarded_like("row_weight", rw, NAN)
    ws = workspace(lib.fql_moe_workspace_bytes(p.E, p.T, K, p.N, 0))
    out = output(p.T, p.N, torch.float32, off(align, torch.float32))
    if scaled:
        what = f"fql_moe_gather_scaled_fwd_f32 G1 {align}"
        call = lambda wp, wb, op: lib.fql_moe_gather_scaled_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gt.ptr, gi.ptr, n_src, gw.ptr, w.cnt.ptr,
                                                                    w.off.ptr, op, p.E, p.T, K, p.N, 0, wp, wb, stream())
    else:
        what = f"fql_moe_gather_fwd_f32 G1 {align}"
        call = lambda wp, wb, op: lib.fql_moe_gather_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gt.ptr, gi.ptr, n_src, w.cnt.ptr, w.off.ptr, op,
                                                             p.E, p.T, K, p.N, 0, wp, wb, stream())
    got = run_prefills(what, call, ws, out, torch.float32, (p.T, p.N), w.all + [gt, gi, gw])
    ref = C.moe_grouped(p.P, p.S, p.Z, tokens[index], p.ref_counts, p.ref_offs)
    if scaled:
        ref = ref * rw[:, None].astype(np.float64)
    check_values(what, got, ref, EXACT_REL_FRO, p.covered)
    assert_residual_in_use(lib, ws, p, "default")


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=lambda d: DT_NAME[d])
def test_moe_fwd_f8(lib, out_dtype, align):
    p = moe_problem("G1")
    x8, xs = O.quantize_activations_fp8(p.x_plain)
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    gx, gs = guarded_like("inputs_e4m3", x8, 0xFF, offset=off(align, torch.uint8)), guarded_like("act_scales", xs, NAN)
    ws = workspace(lib.fql_moe_workspace_bytes(p.E, p.T, K, p.N, PREC["fp8"]))
    ref = O.reference_moe_grouped_fp8(x8, xs, p.P, p.S, p.Z, p.ref_counts, p.ref_offs)
    base = None
    for odt in dict.fromkeys((torch.float32, out_dtype)):
        out = output(p.T, p.N, odt, off(align, odt))
        what = f"fql_moe_fwd_f8 G1 -> {DT_NAME[odt]} {align}"
        call = lambda wp, wb, op: lib.fql_moe_fwd_f8(w.P.ptr, w.S.ptr, w.Z.ptr, gx.ptr, gs.ptr, w.cnt.ptr, w.off.ptr, op, DT[odt], p.E,
                                                     p.T, K, p.N, wp, wb, stream())
        got = run_prefills(what, call, ws, out, odt, (p.T, p.N), w.all + [gx, gs])
        if odt == torch.float32:
            base = got
            check_values(what, got, ref, FP8_ACC_REL_FRO, p.covered)
        else:
            assert same_bits(got, base.to(odt)), (what, first_diff(got, base.to(odt)))


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: DT_NAME[d])
def test_moe_gated_fwd(lib, dtype, align):
    """F = K and a [T, 2F] gate|up input; float32 through fql_moe_gated_fwd_f32, 16-bit gate_up and out through
    fql_moe_gated_fwd.  The oracle is O.gated_ffn_grouped's second half on the same gate_up: silu(g) * u and the down
    projection in float64."""
    p = moe_problem("G1")
    rng = np.random.default_rng(23)
    gu = rng.standard_normal((p.T, 2 * K)).astype(np.float32)
    gu[:, K:] = heavy_rows(gu[:, K:].copy(), rng)
    gu = torch.from_numpy(gu).to(dtype)
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    ws = workspace(lib.fql_moe_workspace_bytes(p.E, p.T, K, p.N, 0))
    g32 = guarded_like("gate_up (float32)", gu.float(), NAN, offset=off(align, torch.float32))
    out = output(p.T, p.N, torch.float32, off(align, torch.float32))
    what = f"fql_moe_gated_fwd_f32 G1 {align}"
    call = lambda wp, wb, op: lib.fql_moe_gated_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, g32.ptr, w.cnt.ptr, w.off.ptr, op, p.E, p.T, K, p.N,
                                                        0, wp, wb, stream())
    base = run_prefills(what, call, ws, out, torch.float32, (p.T, p.N), w.all + [g32])
    g64 = gu.double().numpy()
    h = (g64[:, :K] / (1.0 + np.exp(-g64[:, :K]))) * g64[:, K:]
    ref = np.zeros((p.T, p.N))
    for e, (lo, c) in enumerate(zip(p.ref_offs, p.ref_counts)):
        ref[lo:lo + c] = h[lo:lo + c] @ O.dequantize_weights(p.P[e], p.S[e], p.Z[e]).astype(np.float64).T
    check_values(what, base, ref, EXACT_REL_FRO, p.covered)
    assert_residual_in_use(lib, ws, p, "default")
    if dtype != torch.float32:
        g16 = guarded_like("gate_up", gu, NAN, offset=off(align, dtype))
        out = output(p.T, p.N, dtype, off(align, dtype))
        what = f"fql_moe_gated_fwd G1 {DT_NAME[dtype]} {align}"
        call = lambda wp, wb, op: lib.fql_moe_gated_fwd(w.P.ptr, w.S.ptr, w.Z.ptr, g16.ptr, DT[dtype], w.cnt.ptr, w.off.ptr, op, DT[dtype],
                                                        p.E, p.T, K, p.N, 0, wp, wb, stream())
        got = run_prefills(what, call, ws, out, dtype, (p.T, p.N), w.all + [g16])
        assert same_bits(got, base.to(dtype)), (what, first_diff(got, base.to(dtype)))


# ------------------------------------------------------------------------------ linear entry points
@functools.lru_cache(maxsize=None)
def linear_problem(B, Kx=K, N=200):
    p = Problem()
    rng = np.random.default_rng(1000 + B + Kx)
    p.B, p.K, p.N = B, Kx, N
    p.P, p.S, p.Z = O.quantize_weights((rng.standard_normal((N, Kx)) * 0.02).astype(np.float32))
    p.x_plain = rng.standard_normal((B, Kx)).astype(np.float32)
    p.x_heavy = heavy_rows(p.x_plain.copy(), rng)
    p.bias = rng.standard_normal(N).astype(np.float32)
    return p


LINEAR_CASES = [(131, K, "default"), (131, K, "fast"), (131, K, "int8"), (5, K, "default"), (17, K, "default"),
                (33, K, "default"), (2, K, "default"), (7, 66, "default"), (131, 66, "default")]


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("B,Kx,prec", LINEAR_CASES)
def test_linear_fwd_f32(lib, B, Kx, prec, bias, align):
    """L1 (B = 131) and L2 (B = 5, 17, 33: the 16- and 32-row tile families), B = 2 (the GEMV kernel: no workspace, a NULL
    pointer; with an element-aligned x the generic kernel) and K = 66 (the generic kernel, likewise)."""
    p = linear_problem(B, Kx)
    x = p.x_heavy if LIMBS[prec] >= 2 else p.x_plain
    w = Weights(p.P, p.S, p.Z)
    gx, gb = guarded_like("x", x, NAN, offset=off(align, torch.float32)), guarded_like("bias", p.bias, NAN)
    nbytes = lib.fql_linear_workspace_bytes(B, Kx, p.N, PREC[prec])
    mfma = B > 2 and Kx % 32 == 0
    assert (nbytes > 0) == mfma
    ws = workspace(nbytes)
    out = output(B, p.N, torch.float32, off(align, torch.float32))
    if bias:
        what = f"fql_linear_bias_fwd_f32 B={B} K={Kx} {prec} {align}"
        call = lambda wp, wb, op: lib.fql_linear_bias_fwd_f32(gx.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, gb.ptr, op, B, Kx, p.N, PREC[prec], wp, wb,
                                                              stream())
    else:
        what = f"fql_linear_fwd_f32 B={B} K={Kx} {prec} {align}"
        call = lambda wp, wb, op: lib.fql_linear_fwd_f32(gx.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, op, B, Kx, p.N, PREC[prec], wp, wb, stream())
    got = run_prefills(what, call, ws, out, torch.float32, (B, p.N), w.all + [gx, gb])
    ref = C.linear_f64acc(x, p.P, p.S, p.Z) + (p.bias.astype(np.float64)[None, :] if bias else 0.0)
    check_values(what, got, ref, TOL[prec] if mfma else FMA_REL_FRO)
    if mfma and LIMBS[prec] >= 2:
        flagged = int((delta_of(lib, ws, B, 1, prec)[1] != 0).sum())
        assert 0 < flagged < B, flagged


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
def test_linear_fwd_16bit(lib, bias, dtype, align):
    p = linear_problem(131)
    w = Weights(p.P, p.S, p.Z)
    xin = torch.from_numpy(p.x_heavy).to(dtype)
    gx, gb = guarded_like("x", xin, NAN, offset=off(align, dtype)), guarded_like("bias", p.bias, NAN)
    gx32 = guarded_like("x (widened)", xin.float(), NAN, offset=off(align, torch.float32))
    ws = workspace(lib.fql_linear_workspace_bytes(131, K, p.N, 0))

    def run(g, idt, odt):
        out = output(131, p.N, odt, off(align, odt))
        if bias:
            what = f"fql_linear_bias_fwd L1 {DT_NAME[idt]} -> {DT_NAME[odt]} {align}"
            call = lambda wp, wb, op: lib.fql_linear_bias_fwd(g.ptr, DT[idt], w.P.ptr, w.S.ptr, w.Z.ptr, gb.ptr, op, DT[odt], 131, K, p.N, 0,
                                                              wp, wb, stream())
        else:
            what = f"fql_linear_fwd L1 {DT_NAME[idt]} -> {DT_NAME[odt]} {align}"
            call = lambda wp, wb, op: lib.fql_linear_fwd(g.ptr, DT[idt], w.P.ptr, w.S.ptr, w.Z.ptr, op, DT[odt], 131, K, p.N, 0, wp, wb,
                                                         stream())
        return what, run_prefills(what, call, ws, out, odt, (131, p.N), w.all + [g, gb])

    what, base = run(gx32, torch.float32, torch.float32)
    ref = C.linear_f64acc(xin.float().numpy(), p.P, p.S, p.Z) + (p.bias.astype(np.float64)[None, :] if bias else 0.0)
    check_values(what, base, ref, EXACT_REL_FRO)
    for idt, odt in ((dtype, dtype), (torch.float32, dtype), (dtype, torch.float32)):
        what, got = run(gx if idt == dtype else gx32, idt, odt)
        assert same_bits(got, base.to(odt)), (what, first_diff(got, base.to(odt)))


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=lambda d: DT_NAME[d])
def test_linear_fwd_f8(lib, out_dtype, align):
    p = linear_problem(131)
    x8, xs = O.quantize_activations_fp8(p.x_plain)
    w = Weights(p.P, p.S, p.Z)
    gx, gs = guarded_like("x_e4m3", x8, 0xFF, offset=off(align, torch.uint8)), guarded_like("act_scales", xs, NAN)
    ws = workspace(lib.fql_linear_workspace_bytes(131, K, p.N, PREC["fp8"]))
    base = None
    for odt in dict.fromkeys((torch.float32, out_dtype)):
        out = output(131, p.N, odt, off(align, odt))
        what = f"fql_linear_fwd_f8 L1 -> {DT_NAME[odt]} {align}"
        call = lambda wp, wb, op: lib.fql_linear_fwd_f8(gx.ptr, gs.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, op, DT[odt], 131, K, p.N, wp, wb, stream())
        got = run_prefills(what, call, ws, out, odt, (131, p.N), w.all + [gx, gs])
        if odt == torch.float32:
            base = got
            check_values(what, got, O.reference_linear_fp8(x8, xs, p.P, p.S, p.Z), FP8_ACC_REL_FRO)
        else:
            assert same_bits(got, base.to(odt)), (what, first_diff(got, base.to(odt)))


# ------------------------------------------------------------------------------ per-group scales along K
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("B,N,Kx,group", [(3, 33, 96, 2), (7, 200, 512, 128), (40, 96, 1024, 32)])
def test_linear_group_fwd_f32(lib, B, N, Kx, group, align):
    """No workspace: the GEMV kernel with per-group constants (3 rows), and the float32 matrix-core kernel at 7 and at 40
    rows (shapes of tests/test_gpu_parity.py::test_per_group_scales_linear)."""
    rng = np.random.default_rng(B + Kx)
    P, S, Z = O.quantize_weights_grouped(rng.standard_normal((N, Kx)).astype(np.float32), group)
    x = rng.standard_normal((B, Kx)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    w = Weights(P, S, Z)
    gx, gb = guarded_like("x", x, NAN, offset=off(align, torch.float32)), guarded_like("bias", bias, NAN)
    out = output(B, N, torch.float32, off(align, torch.float32))
    what = f"fql_linear_group_fwd_f32 {B}x{N}x{Kx} group {group} {align}"
    call = lambda wp, wb, op: lib.fql_linear_group_fwd_f32(gx.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, gb.ptr, op, B, Kx, N, group, stream())
    got = run_prefills(what, call, None, out, torch.float32, (B, N), w.all + [gx, gb])
    check_values(what, got, O.reference_linear_grouped(x, P, S, Z) + bias.astype(np.float64)[None, :], FMA_REL_FRO)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("prec", ["exact", "fast", "int8"])
def test_linear_group_ws_fwd_f32(lib, prec, align):
    """(49, 72, 512, 256): the per-group path on the INT8 matrix cores, with exactly fql_group_workspace_bytes."""
    B, N, Kx, group = 49, 72, 512, 256
    rng = np.random.default_rng(B + Kx + group)
    P, S, Z = O.quantize_weights_grouped(rng.standard_normal((N, Kx)).astype(np.float32), group)
    x = rng.standard_normal((B, Kx)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    w = Weights(P, S, Z)
    gx, gb = guarded_like("x", x, NAN, offset=off(align, torch.float32)), guarded_like("bias", bias, NAN)
    ws = workspace(lib.fql_group_workspace_bytes(1, B, Kx, N, group, PREC[prec]))
    out = output(B, N, torch.float32, off(align, torch.float32))
    what = f"fql_linear_group_ws_fwd_f32 {prec} {align}"
    call = lambda wp, wb, op: lib.fql_linear_group_ws_fwd_f32(gx.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, gb.ptr, op, B, Kx, N, group, PREC[prec], wp,
                                                              wb, stream())
    got = run_prefills(what, call, ws, out, torch.float32, (B, N), w.all + [gx, gb])
    tol = {"exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "int8": INT8_REL_FRO_LARGE_K}[prec]   # (test_per_group_scales_integer_matrix_cores)
    check_values(what, got, O.reference_linear_grouped(x, P, S, Z) + bias.astype(np.float64)[None, :], tol)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("prec", ["exact", "fast", "int8"])
def test_moe_group_ws_fwd_f32(lib, prec, align):
    E, N, Kx, group, counts = 4, 136, 512, 128, np.array([150, 0, 40, 3], np.int32)
    rng = np.random.default_rng(5)
    offs = (np.cumsum(counts) - counts).astype(np.int32)
    T = int(counts.sum()) + 2
    q = [O.quantize_weights_grouped(rng.standard_normal((N, Kx)).astype(np.float32), group) for _ in range(E)]
    P, S, Z = (np.stack([t[i] for t in q]) for i in range(3))
    x = rng.standard_normal((T, Kx)).astype(np.float32)
    w = Weights(P, S, Z, counts, offs)
    gx = guarded_like("inputs", x, NAN, offset=off(align, torch.float32))
    ws = workspace(lib.fql_group_workspace_bytes(E, T, Kx, N, group, PREC[prec]))
    out = output(T, N, torch.float32, off(align, torch.float32))
    what = f"fql_moe_group_ws_fwd_f32 {prec} {align}"
    call = lambda wp, wb, op: lib.fql_moe_group_ws_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gx.ptr, w.cnt.ptr, w.off.ptr, op, E, T, Kx, N, group,
                                                           PREC[prec], wp, wb, stream())
    got = run_prefills(what, call, ws, out, torch.float32, (T, N), w.all + [gx])
    ref = np.zeros((T, N))
    covered = np.zeros(T, bool)
    for e in range(E):
        lo, c = int(offs[e]), int(counts[e])
        ref[lo:lo + c] = O.reference_linear_grouped(x[lo:lo + c], P[e], S[e], Z[e])
        covered[lo:lo + c] = True
    tol = {"exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "int8": INT8_REL_FRO_LARGE_K}[prec]
    check_values(what, got, ref, tol, covered)


# ------------------------------------------------------------------------------ every tile family by id
def tile_ids(lib, prec):
    ids = (list(range(lib.fql_tune_num_configs())) + list(range(100, 100 + lib.fql_tune_num_rows32_configs()))
           + list(range(200, 200 + lib.fql_tune_num_rows16_configs())) + list(range(220, 240))
           + list(range(300, 300 + lib.fql_tune_num_w4_configs())))
    return [c for c in ids if lib.fql_tune_is_config(c, PREC[prec]) == 1]


def tile_family_run(lib, name, prec, ids):
    """fql_act_quant_f32 into limbs of exactly fql_act_limb_bytes, delta and rowsum as ops.act_quant sizes them, then every
    id through fql_tune_gemm_i8 with a scratch of fql_gemm_scratch_bytes (these problems use its first slots only: the far
    end is test_scratch_is_used_up_to_its_last_slot's); all four buffers prefilled three ways.  Every id stores into a
    16-byte aligned output (vector stores) AND into one that starts one element past such a boundary (the scalar store
    form of its epilogue); the second prefill's pre-pass reads an element-aligned x (its scalar form)."""
    p = moe_problem(name)
    x = moe_x(p, prec)
    nl = LIMBS[prec]
    ns = 2 if nl >= 2 else 1
    w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
    gx, gx_el = guarded_like("x", x, NAN, offset=16), guarded_like("x (element-aligned)", x, NAN, offset=4)
    limbs = Guarded("limbs", lib.fql_act_limb_bytes(p.T, p.E, K, PREC[prec]), torch.uint8, WS_PATTERN, offset=16)
    delta = Guarded("delta", ns * p.T * 4, torch.float32, NAN, offset=4)
    rowsum = Guarded("rowsum", ns * nl * p.T * 4, torch.int32, BIG, offset=4)
    sbytes = lib.fql_gemm_scratch_bytes(PREC[prec])
    assert (sbytes > 0) == (nl >= 2)
    scratch = Guarded("scratch", sbytes, torch.uint8, WS_PATTERN, offset=16) if sbytes else None
    mids = [limbs, delta, rowsum] + ([scratch] if scratch else [])
    outs = {(dt, al): output(p.T, p.N, dt, off(al, dt)) for dt in DT for al in ALIGNS}
    first, first_id = None, None
    for fill in PREFILLS:
        for b in mids:
            b.bytes().fill_(fill)
        src = gx_el if fill == PREFILLS[1] else gx
        rc = lib.fql_act_quant_f32(src.ptr, limbs.ptr, delta.ptr, rowsum.ptr, w.cnt.ptr, w.off.ptr, p.E, p.T, K, PREC[prec], stream())
        assert rc == 0, rc
        assert_guards_intact(src, *mids, *w.all, what=f"fql_act_quant_f32 {name} {prec}, buffers {fill:#04x}")
        if nl >= 2:
            cov = torch.from_numpy(p.covered).cuda()
            flagged = int(((delta.view(torch.float32, ns, p.T)[1] != 0) & cov).sum())
            assert 0 < flagged < int(cov.sum()), flagged
        for i, cfg in enumerate(ids):
            dts = (torch.float32, (torch.float16, torch.bfloat16)[i % 2]) if fill == PREFILLS[0] else (torch.float32,)
            for dt, al in [(dt, al) for dt in dts for al in ALIGNS]:
                out = outs[(dt, al)]
                o = out.view(dt, p.T, p.N)
                o.fill_(SENT)
                rc = lib.fql_tune_gemm_i8(cfg, limbs.ptr, delta.ptr, rowsum.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, w.cnt.ptr, w.off.ptr,
                                          out.ptr, DT[dt], None, None, p.E, p.T, K, p.N, PREC[prec], stream(),
                                          scratch.ptr if scratch else None, sbytes)
                what = f"fql_tune_gemm_i8 id {cfg} {name} {prec} -> {DT_NAME[dt]} {al}, buffers {fill:#04x}"
                assert rc == 0, (what, rc)
                assert_guards_intact(out, *mids, *w.all, what=what)
                if first is None:
                    first, first_id = o.clone(), cfg
                    if prec == "fp8":
                        x8, xs = O.quantize_activations_fp8(x)
                        ref = O.reference_moe_grouped_fp8(x8, xs, p.P, p.S, p.Z, p.ref_counts, p.ref_offs)
                    else:
                        ref = moe_ref(name, nl >= 2)
                    check_values(what, first, ref, TOL[prec], p.covered, uncovered=SENT)
                want = first if dt == torch.float32 else first.to(dt)
                assert same_bits(o, want), f"{what}: differs from id {first_id}, buffers {PREFILLS[0]:#04x}: {first_diff(o, want)}"


@pytest.mark.parametrize("prec", ["exact", "fast", "int8", "fp8"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_every_tile_family_by_id(lib, name, prec):
    ids = tile_ids(lib, prec)
    assert len(ids) >= (7 if prec == "fp8" else 6 + 8 + 9 + 4), ids      # wide ids built for the precision + every id of 100.., 200.., 220..
    if prec != "fp8":
        assert {100, 107, 200, 208, 220, 223} <= set(ids) and ((300 in ids) == (prec == "exact"))
    tile_family_run(lib, name, prec, ids)


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_one_wave_per_simd_ids_walk_many_tiles(lib, name):
    """Grids sized for 8 compute units: every workgroup walks many tiles.  The scratch size is asked for afterwards."""
    old = lib.fql_tune_set_compute_units(8)
    try:
        tile_family_run(lib, name, "exact", [c for c in tile_ids(lib, "exact") if c >= 300])
    finally:
        lib.fql_tune_set_compute_units(old)


def test_scratch_is_used_up_to_its_last_slot(lib):
    """res_scratch_bytes() (csrc/fql_int4.hip) is max(256, CUs) x 8 waves x 4 fragments x 4 KiB, and a workgroup parks
    its residual partials at slot (blockIdx.x * waves + wave) x fragments.  Id 2 (128 x 256 tiles: 8 waves x 4 fragments,
    one workgroup per CU) uses exactly that per workgroup, so its last workgroup ends where the buffer ends: one 2-limb
    launch of 2048 x 4096 (16 x 16 = 256 tiles or more, every one with heavy-tailed rows) must write the last 4 KiB of
    the scratch and nothing behind it."""
    B, N, prec = 2048, 4096, "fast"
    assert lib.fql_tune_is_config(2, PREC[prec]) == 1
    rng = np.random.default_rng(77)
    P = rng.integers(0, 256, size=(N, K // 2), dtype=np.uint8)
    S = (0.001 + 0.002 * rng.random(N)).astype(np.float32)
    Z = rng.integers(5, 11, size=N).astype(np.float32)
    x = heavy_rows(rng.standard_normal((B, K)).astype(np.float32), rng)
    w = Weights(P, S, Z)
    gx = guarded_like("x", x, NAN, offset=16)
    limbs = Guarded("limbs", lib.fql_act_limb_bytes(B, 1, K, PREC[prec]), torch.uint8, WS_PATTERN, offset=16)
    delta = Guarded("delta", 2 * B * 4, torch.float32, NAN, offset=4)
    rowsum = Guarded("rowsum", 2 * 2 * B * 4, torch.int32, BIG, offset=4)
    sbytes = lib.fql_gemm_scratch_bytes(PREC[prec])
    scratch = Guarded("scratch", sbytes, torch.uint8, WS_PATTERN, offset=16)
    out = output(B, N, torch.float32)
    mids = [limbs, delta, rowsum, scratch]
    for b in mids:
        b.bytes().fill_(0xFF)
    out.view(torch.float32, B, N).fill_(SENT)
    assert lib.fql_act_quant_f32(gx.ptr, limbs.ptr, delta.ptr, rowsum.ptr, None, None, 1, B, K, PREC[prec], stream()) == 0
    rc = lib.fql_tune_gemm_i8(2, limbs.ptr, delta.ptr, rowsum.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, None, None, out.ptr, 0, None, None, 1, B, K, N,
                              PREC[prec], stream(), scratch.ptr, sbytes)
    assert rc == 0, rc
    assert_guards_intact(out, gx, *mids, *w.all, what="fql_tune_gemm_i8 id 2, 2048 x 4096, 2 limbs")
    flagged = int((delta.view(torch.float32, 2, B)[1] != 0).sum())
    assert 0 < flagged < B, flagged
    used = scratch.bytes().view(-1, 4096) != 0xFF
    assert bool(used[-1].any()), "the last 4 KiB slot of the scratch was not written: the launch did not reach the bound"
    print(f"scratch: {int(used.any(dim=1).sum())} of {used.shape[0]} 4 KiB slots written, the last one among them")
    W = dequant_f64(torch.from_numpy(P).cuda(), torch.from_numpy(S), torch.from_numpy(Z))
    err = rel_fro_dev(out.view(torch.float32, B, N), torch.from_numpy(x).cuda().double() @ W.T)
    print(f"id 2, 2048 x 4096, 2 limbs: {err:.3e} (bound {FAST_REL_FRO:.1e})")
    assert err < FAST_REL_FRO, err


# ------------------------------------------------------------------------------ the one-launch form
@functools.lru_cache(maxsize=None)
def wide_linear_problem(B, N):
    p = Problem()
    rng = np.random.default_rng(B + N)
    p.B, p.K, p.N = B, K, N
    p.P = rng.integers(0, 256, size=(N, K // 2), dtype=np.uint8)
    p.S = (0.001 + 0.002 * rng.random(N)).astype(np.float32)
    p.Z = rng.integers(5, 11, size=N).astype(np.float32)
    p.x_heavy = heavy_rows(rng.standard_normal((B, K)).astype(np.float32), rng)
    W = dequant_f64(torch.from_numpy(p.P).cuda(), torch.from_numpy(p.S), torch.from_numpy(p.Z))
    p.ref = (torch.from_numpy(p.x_heavy).cuda().double() @ W.T).cpu().numpy()
    return p


@pytest.mark.parametrize("spin", [None, 0], ids=["default_spin", "spin0"])
@pytest.mark.parametrize("name", ["G1", "L1", "G1-N6408", "L1-N16392"])
def test_one_launch_form(lib, name, spin):
    """fql_tune_set_fused(1): the pre-pass is the GEMM kernel's first phase and the flag words of the workspace must
    survive arbitrary contents, their own previous run included (a fourth run).  The switch acts where the dispatcher picks
    the one-wave-per-SIMD kernel (id 301).  At G1 and L1 it picks a skinny tile and the two-launch path runs, switched on
    or not: asserted, the flag words still hold the prefill afterwards.  So both are repeated at the smallest N at which
    301 is chosen: G1 at N = 6408 (5 experts x 26 column tiles of 256 reach the 128 wide tiles) and L1 at N = 16392 (129
    column tiles of 128 need a second round of the 256 CUs, 86 of 192 do not); there every flag word of a covered row
    group must have been rewritten."""
    old_fused = lib.fql_tune_set_fused(1)
    old_spin = lib.fql_tune_set_fused_spin(0) if spin == 0 else None
    try:
        wide = "-N" in name
        if name.startswith("L1"):
            p = wide_linear_problem(131, 16392) if wide else linear_problem(131)
            E, T, covered = 1, 131, np.ones(131, bool)
            assert (lib.fql_tune_chosen_cfg(3, 1, T, K, p.N, 0) == 301) == wide
            w = Weights(p.P, p.S, p.Z)
            gx = guarded_like("x", p.x_heavy, NAN, offset=16)
            ws = workspace(lib.fql_linear_workspace_bytes(T, K, p.N, 0))
            ref = p.ref if wide else C.linear_f64acc(p.x_heavy, p.P, p.S, p.Z)
            call = lambda wp, wb, op: lib.fql_linear_fwd_f32(gx.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, op, T, K, p.N, 0, wp, wb, stream())
        else:
            p = moe_problem("G1", 6408 if wide else None)
            E, T, covered = p.E, p.T, p.covered
            assert (lib.fql_tune_chosen_cfg(3, E, T, K, p.N, 1) == 301) == wide
            w = Weights(p.P, p.S, p.Z, p.counts, p.offs)
            gx = guarded_like("inputs", p.x_heavy, NAN, offset=16)
            ws = workspace(lib.fql_moe_workspace_bytes(E, T, K, p.N, 0))
            ref = moe_ref("G1", True, 6408 if wide else None)
            call = lambda wp, wb, op: lib.fql_moe_fwd_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gx.ptr, w.cnt.ptr, w.off.ptr, op, E, T, K, p.N, 0,
                                                          wp, wb, stream())
        out = output(T, p.N, torch.float32)
        what = f"one-launch {name} spin {spin}"
        got = run_prefills(what, call, ws, out, torch.float32, (T, p.N), w.all + [gx], stale_rerun=True)
        check_values(what, got, ref, EXACT_REL_FRO, covered)
        flagged = int(((delta_of(lib, ws, T, E, "default")[1] != 0) & torch.from_numpy(covered).cuda()).sum())
        assert 0 < flagged < int(covered.sum()), flagged
        # the last prefill was 0x7F: a flag word the kernel wrote is its launch token, never 0x7F7F7F7F7F7F7F7F
        rewritten = (flag_words(lib, ws, T, E).view(-1, 8) != 0x7F).any(dim=1).cpu().numpy()
        whole = covered[:T // 4 * 4].reshape(-1, 4).all(axis=1)         # row groups of 4 that an expert covers entirely
        print(f"{what}: {int(rewritten.sum())} of {rewritten.size} flag words rewritten")
        if wide:
            assert rewritten[:whole.size][whole].all(), "id 301 with the switch on, but flag words of covered rows were not written"
        else:
            assert not rewritten.any(), "the two-launch path wrote flag words"
    finally:
        if old_spin is not None:
            lib.fql_tune_set_fused_spin(old_spin)
        lib.fql_tune_set_fused(old_fused)


# ------------------------------------------------------------------------------ the side kernels
def i32_out(name, n):
    g = Guarded(name, 4 * n, torch.int32, BIG, offset=4)
    g.view(torch.int32, n).fill_(-99)
    return g


@pytest.mark.parametrize("T,E,top_k,clamp", [(1, 3, 1, False), (333, 64, 6, False), (300, 128, 2, False), (50, 8, 2, True)])
def test_route_plan_footprint(lib, T, E, top_k, clamp):
    """E = 128 is the LDS limit; ids -1 and E clamp to 0 and E - 1 (include/fql_int4.h): the stable sort of the clamped ids."""
    g = torch.Generator().manual_seed(T * 31 + E)
    idx = torch.stack([torch.randperm(E, generator=g)[:top_k] for _ in range(T)]).to(torch.int32)
    if clamp:
        idx[3, 0], idx[7, 1], idx[20, 0], idx[49, 1] = -1, E, E, -1
    n = T * top_k
    gi = guarded_like("expert_of_slot", idx, BIG)
    outs = [i32_out("counts", E), i32_out("offsets", E), i32_out("token_of_sorted", n), i32_out("pos_of_slot", n)]
    rc = lib.fql_route_plan_i32(gi.ptr, n, top_k, E, *(o.ptr for o in outs), stream())
    assert rc == 0, rc
    assert_guards_intact(gi, *outs, what=f"fql_route_plan_i32 T={T} E={E} top_k={top_k}")
    flat = idx.reshape(-1).long().clamp(0, E - 1)
    order = torch.argsort(flat, stable=True)
    ref_counts = torch.bincount(flat, minlength=E)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(n)
    for o, want in zip(outs, (ref_counts, torch.cumsum(ref_counts, 0) - ref_counts, order // top_k, inverse)):
        assert torch.equal(o.view(torch.int32, want.numel()).cpu().long(), want), o.name


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "null_weights"])
@pytest.mark.parametrize("align", [16, 4])
@pytest.mark.parametrize("N", [1004, 1001, 3])
@pytest.mark.parametrize("top_k", [1, 2, 4])
def test_combine_footprint(lib, top_k, N, align, weighted):
    """y and out 16-byte aligned with N % 4 == 0: 16-byte stores; one float past it, or N % 4 != 0: the scalar form."""
    T = 37
    g = torch.Generator().manual_seed(5 + N + top_k)
    R = T * top_k
    y = torch.randn(R, N, generator=g)
    pos = torch.randperm(R, generator=g).to(torch.int32)
    wt = torch.rand(T, top_k, generator=g) + 0.1
    gy, gp, gw = guarded_like("y", y, NAN, offset=align), guarded_like("pos_of_slot", pos, BIG), guarded_like("weights", wt, NAN)
    out = output(T, N, torch.float32, align)
    o = out.view(torch.float32, T, N)
    o.fill_(SENT)
    rc = lib.fql_combine_f32(gy.ptr, gp.ptr, gw.ptr if weighted else None, out.ptr, T, top_k, N, R, stream())
    assert rc == 0, rc
    assert_guards_intact(gy, gp, gw, out, what=f"fql_combine_f32 top_k={top_k} N={N} align {align}")
    rows = y[pos.long()].view(T, top_k, N)
    ref = (rows * wt.unsqueeze(-1) if weighted else rows).sum(dim=1)
    if top_k <= 2:
        assert torch.equal(o.cpu(), ref)                     # one addition: no ordering freedom
    else:
        assert torch.allclose(o.cpu(), ref, rtol=1e-6, atol=1e-6)        # (test_combine_kernel)


@pytest.mark.parametrize("with_gw", [True, False], ids=["grad_weights", "null_grad_weights"])
@pytest.mark.parametrize("N", [1004, 1001, 3])
@pytest.mark.parametrize("top_k", [1, 2, 4])
def test_combine_bwd_footprint(lib, top_k, N, with_gw):
    """grad_y = weights * grad_out is one multiply: bit exact.  grad_weights against the float64 dot product at the bound
    of tests/test_gpu_backward.py::test_combine_backward: 1e-6 of the largest gradient."""
    T = 37
    g = torch.Generator().manual_seed(9 + N + top_k)
    R = T * top_k
    y, go = torch.randn(R, N, generator=g), torch.randn(T, N, generator=g)
    pos = torch.randperm(R, generator=g).to(torch.int32)
    wt = torch.rand(T, top_k, generator=g) + 0.1
    ins = [guarded_like("grad_out", go, NAN), guarded_like("y", y, NAN), guarded_like("pos_of_slot", pos, BIG), guarded_like("weights", wt, NAN)]
    ggy = Guarded("grad_y", R * N * 4, torch.float32, SENT, offset=4)
    ggw = Guarded("grad_weights", R * 4, torch.float32, SENT, offset=4)
    ggy.view(torch.float32, R, N).fill_(SENT)
    ggw.view(torch.float32, T, top_k).fill_(SENT)
    rc = lib.fql_combine_bwd_f32(*(b.ptr for b in ins), ggy.ptr, ggw.ptr if with_gw else None, T, top_k, N, R, stream())
    assert rc == 0, rc
    assert_guards_intact(*ins, ggy, ggw, what=f"fql_combine_bwd_f32 top_k={top_k} N={N}")
    want = torch.empty(R, N)
    want[pos.long()] = (wt.unsqueeze(-1) * go.unsqueeze(1)).reshape(R, N)
    assert torch.equal(ggy.view(torch.float32, R, N).cpu(), want)
    gw = ggw.view(torch.float32, T, top_k).cpu()
    if with_gw:
        ref = (y[pos.long()].view(T, top_k, N).double() * go.double().unsqueeze(1)).sum(-1)
        assert (gw.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    else:
        assert bool((gw == SENT).all())


@pytest.mark.parametrize("G,EL", [(4, 3), (1, 1), (64, 128)])
def test_regroup_index_footprint(lib, G, EL):
    """(64, 128) is the 8192-entry limit of the LDS tables."""
    g = torch.Generator().manual_seed(9 + G)
    cnt = torch.randint(0, 7 if G * EL < 100 else 3, (G, EL), generator=g).to(torch.int32)
    cnt.view(-1)[::5] = 0
    if G * EL == 1:
        cnt[0, 0] = 4
    R = int(cnt.sum())
    gc = guarded_like("recv_counts", cnt, BIG)
    outs = [i32_out("tokens_per_expert", EL), i32_out("input_offsets", EL), i32_out("gather", R), i32_out("scatter", R)]
    rc = lib.fql_regroup_index_i32(gc.ptr, G, EL, *(o.ptr for o in outs), stream())
    assert rc == 0, rc
    assert_guards_intact(gc, *outs, what=f"fql_regroup_index_i32 G={G} EL={EL}")
    c = cnt.numpy().astype(np.int64)
    s_of, e_of = np.repeat(np.arange(G * EL) // EL, c.reshape(-1)), np.repeat(np.arange(G * EL) % EL, c.reshape(-1))
    want = np.lexsort((np.arange(R), s_of, e_of))           # received rows are (s, e, i)-ordered; expert-major sorts by (e, s, i)
    tot = c.sum(0)
    assert np.array_equal(outs[0].view(torch.int32, EL).cpu().numpy(), tot)
    assert np.array_equal(outs[1].view(torch.int32, EL).cpu().numpy(), np.cumsum(tot) - tot)
    gather = outs[2].view(torch.int32, R).cpu().numpy()
    assert np.array_equal(gather, want)
    assert np.array_equal(outs[3].view(torch.int32, R).cpu().numpy()[gather], np.arange(R))


@pytest.mark.parametrize("src_offset,dst_offset", [(8, 8), (1, 1), (8, 1), (1, 8)], ids=["aligned8", "odd", "odd_q", "odd_packed"])
@pytest.mark.parametrize("nbytes", [1, 3, 4, 5, 4099])
def test_unpack_footprint(lib, nbytes, src_offset, dst_offset):
    """The kernel takes its 4-byte form when source AND destination are 8-byte aligned: all four combinations."""
    p = np.random.default_rng(nbytes).integers(0, 256, size=nbytes, dtype=np.uint8)
    gp = guarded_like("packed", p, 0xFF, offset=src_offset)
    gq = Guarded("q", 2 * nbytes, torch.uint8, 0xEE, offset=dst_offset)
    gq.bytes().fill_(0xEE)
    rc = lib.fql_unpack_u8(gp.ptr, gq.ptr, nbytes, stream())
    assert rc == 0, rc
    assert_guards_intact(gp, gq, what=f"fql_unpack_u8 nbytes={nbytes} source offset {src_offset}, destination offset {dst_offset}")
    assert np.array_equal(gq.bytes().cpu().numpy(), O.unpack_nibbles(p[None])[0])


@pytest.mark.parametrize("N,Kx", [(1, 2), (5, 30), (300, 1030)])
def test_dequantize_and_quantisers_footprint(lib, N, Kx):
    """Bit exact against O.dequantize_weights, O.quantize_weights and the per-tensor rule (O.quantize_weights_moe, the
    restatement of quantize_weights_moe); the 2 * N floats of fql_quantize_tensor_f32's scratch are guarded too."""
    rng = np.random.default_rng(N + Kx)
    wf = (rng.standard_normal((N, Kx)) * 0.02).astype(np.float32)
    P, S, Z = O.quantize_weights(wf)
    w = Weights(P, S, Z)
    gout = Guarded("w", N * Kx * 4, torch.float32, SENT, offset=4)
    gout.view(torch.float32, N, Kx).fill_(SENT)
    assert lib.fql_dequantize_f32(w.P.ptr, w.S.ptr, w.Z.ptr, gout.ptr, N, Kx, stream()) == 0
    assert_guards_intact(*w.all, gout, what=f"fql_dequantize_f32 {N}x{Kx}")
    assert np.array_equal(gout.view(torch.float32, N, Kx).cpu().numpy(), O.dequantize_weights(P, S, Z))
    gw = guarded_like("w", wf, NAN)
    for per_tensor in (False, True):
        gp = Guarded("packed", N * Kx // 2, torch.uint8, 0xEE, offset=1)
        gs, gz = Guarded("scales", N * 4, torch.float32, SENT, offset=4), Guarded("zps", N * 4, torch.float32, SENT, offset=4)
        gscr = Guarded("scratch", 2 * N * 4, torch.float32, SENT, offset=4)
        for b in (gp, gs, gz, gscr):
            b.bytes().fill_(0xEE)
        if per_tensor:
            rc = lib.fql_quantize_tensor_f32(gw.ptr, gp.ptr, gs.ptr, gz.ptr, gscr.ptr, N, Kx, stream())
            rp, rs, rz = (a[0] for a in O.quantize_weights_moe([wf]))
        else:
            rc = lib.fql_quantize_rows_f32(gw.ptr, gp.ptr, gs.ptr, gz.ptr, N, Kx, stream())
            rp, rs, rz = P, S, Z
        assert rc == 0, rc
        assert_guards_intact(gw, gp, gs, gz, gscr, what=f"fql_quantize_{'tensor' if per_tensor else 'rows'}_f32 {N}x{Kx}")
        assert np.array_equal(gp.view(torch.uint8, N, Kx // 2).cpu().numpy(), rp)
        assert np.array_equal(gs.view(torch.float32, N).cpu().numpy(), rs) and np.array_equal(gz.view(torch.float32, N).cpu().numpy(), rz)
