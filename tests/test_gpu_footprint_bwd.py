"""Where the input-gradient kernels write, and what else they read (csrc/fql_bwd.h, fql_bwd.hip): the method of
tests/test_gpu_footprint.py on fql_linear_bwd_input[_f32] and fql_moe_bwd_input[_f32], through the C ABI.

Every pointer of a call is the interior of a helpers.Guarded buffer: grad_in between SENT (and SENT inside before the call),
grad_out, scales and zps between NaN, the expert table between BIG, the packed weights between 0xFF, the workspace at
exactly fql_*_bwd_workspace_bytes(), 16 bytes past a 256-byte boundary, between 0x5A.  Every case asserts
  (a) every guard is intact after the call, and rows no expert covers are zero;
  (b) grad_in against dY.double() @ dequant_f64(W_e) per clipped expert range, at helpers.fro_tol / ROW_TOL (the bounds of
      tests/test_gpu_backward_paths.py); a 16-bit grad_in bit for bit the float32 run on the widened gradient rounded once;
  (c) the same call with the workspace prefilled 0x00, 0xFF (delta2 = NaN: a tile that tests a stale delta2 takes the
      residual pass; limbs of -1) and 0x7F returns the same bits.
A load that is fetched and then masked away cannot be seen this way, and is not looked for.

The shapes are the smallest at which every form of the three kernels runs (launch_bwd, fql_bwd.hip):
  * tables: G1 / G1c / G2 of the forward file (helpers.footprint_table) and linear calls of B = 129 and 515 rows.  G1, G1c
    and B = 129 stay within 512 padded rows (the one-row pre-pass), G2 (21 blocks of 32) and B = 515 (515 % 4 = 3) do not;
  * N = 272 (N % 16 == 0: the vector pre-pass when grad_out, scales and zps are 16-byte aligned; Np = 512: two stages, the
    second with 16 live n) or N = 200 (the scalar pre-pass, one stage);
  * K = 160 (16-byte weight loads, a last column tile of 32), 140 (byte loads, 16-byte stores), 138 (byte loads, K / 2
    odd, scalar stores), and K = 160 with `packed` one byte past a 16-byte boundary (byte loads on a vector shape);
  * grad_out and grad_in both 16-byte aligned, both one element past such a boundary (scalar pre-pass, scalar stores),
    and grad_in alone one element past (the vector pre-pass and weight loads with scalar stores);
  * 3, 2 and 1 limbs; at 3 and 2 limbs and N = 272 every fifth gradient row is heavy-tailed and flagged (the residual
    set, delta2 and the second rowsum plane are in use: asserted on delta2, row by row).  At N = 200 the pre-pass cannot
    flag any row (flaggable(), below), so a heavy-tailed row there would only sit at the error the flag rule allows, above
    the Frobenius bounds of the mode: the gradient is plain there and delta2 must be zero everywhere; the scalar pre-pass
    meets the residual set at N = 272 with an element-aligned grad_out.  In the shapes marked `frac` a few zero points
    are z + 0.4, so the correction plane delta[sets * T + t] is in use (asserted)."""
import functools

import numpy as np
import pytest
import torch

from helpers import (BIG, NAN, ROW_TOL, SENT, Guarded, assert_guards_intact, clipped_ranges, dequant_f64, first_diff,
                     footprint_table, fro_tol, guarded_like, heavy_rows, rel_fro_dev, row_rel_err, same_bits)

pytestmark = pytest.mark.gpu

PREC = {"int8": 1, "fast": 2, "exact": 3}
LIMBS = {"exact": 3, "fast": 2, "int8": 1}
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
DT_NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
WS_PATTERN = 0x5A
PREFILLS = (0x00, 0xFF, 0x7F)
TABLES = ["G1", "G1c", "G2", "L129", "L515"]
# (N, alignment of grad_out / grad_in, K, offset of packed, fractional zero points): pre-pass | weight loads | stores
SHAPES = [
    (272, "aligned", 160, 16, False),      # vector  | 16-byte | 16-byte
    (272, "aligned", 140, 16, True),       # vector  | bytes   | 16-byte
    (272, "aligned", 138, 16, False),      # vector  | bytes, K / 2 odd | scalar
    (272, "out-element", 160, 16, False),  # vector  | 16-byte | scalar
    (200, "aligned", 160, 16, False),      # scalar  | 16-byte | 16-byte
    (200, "aligned", 160, 1, False),       # scalar  | bytes (packed + 1) | 16-byte
    (272, "element", 160, 16, False),      # scalar (grad_out + one element) | 16-byte | scalar
    (200, "element", 138, 16, True),       # scalar  | bytes, K / 2 odd | scalar
]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fused_int4_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


# ------------------------------------------------------------------------------ problems (built once, never modified)
class Problem:
    pass


@functools.lru_cache(maxsize=None)
def table(name):
    """E, T, the table the device gets (None: a linear call), the clipped ranges and the covered rows."""
    t = Problem()
    if name.startswith("L"):
        t.E, t.T, t.counts, t.offs = 1, int(name[1:]), None, None
        t.ranges = [(0, t.T)]
    else:
        t.counts, t.offs, t.T = footprint_table(name)
        t.E = len(t.counts)
        t.ranges = clipped_ranges(torch.from_numpy(t.counts), torch.from_numpy(t.offs), t.T)
    t.covered = np.zeros(t.T, bool)
    for lo, hi in t.ranges:
        t.covered[lo:hi] = True
    assert t.covered.all() == (name != "G1")
    return t


@functools.lru_cache(maxsize=None)
def weights(E, N, K, centred, frac):
    """Random codes, scales in [0.005, 0.015), integer zero points in [0, 15] (``centred``: [6, 9], as
    tests/test_gpu_backward_paths.py gives the one-limb runs); ``frac``: every seventh zero point + 0.4."""
    rng = np.random.default_rng(1000 * N + K + 7 * E + centred)
    P = rng.integers(0, 256, size=(E, N, K // 2), dtype=np.uint8)
    S = (0.005 + 0.01 * rng.random((E, N))).astype(np.float32)
    Z = rng.integers(6, 10, size=(E, N)).astype(np.float32) if centred else rng.integers(0, 16, size=(E, N)).astype(np.float32)
    if frac:
        Z.reshape(-1)[::7] += np.float32(0.4)
    return P, S, Z


def flaggable(N):
    """Whether the pre-pass can flag a row of length N at all (csrc/fql_act_quant.h: a row is flagged when
    sum_n (g / delta)^2 < N / (12 P^2), P = 1e-6 at 3 limbs and 2.5e-4 at 2).  max|g| / delta alone is above 2^(8L - 2), so
    nothing is ever flagged below N = 12 P^2 4^(8L - 2): 212 at 3 limbs, 202 at 2.  N = 200 is below both."""
    return N >= 212


@functools.lru_cache(maxsize=None)
def gradient(name, N, K, centred, frac, heavy):
    """randn; ``heavy``: every fifth row heavy-tailed (helpers.heavy_rows), its largest element then set so that the
    column-scaled row g = dY * s has max|g| = 1.01 * 2^8: max|g| / delta is 1.01 * 2^(8L - 2), the coarsest quantum a row can
    get, the sum above is (1.01 * 2^(8L - 2))^2 (1 + a few per cent) and N = 272 puts the limit 1.26 (3 limbs) and 1.32
    (2 limbs) times higher: the row is flagged in float32, float16 and bfloat16 alike (dY stays below 65504)."""
    t = table(name)
    rng = np.random.default_rng(len(name) + t.T + N)
    gy = rng.standard_normal((t.T, N)).astype(np.float32)
    if heavy:
        S = weights(t.E, N, K, centred, frac)[1]
        heavy_rows(gy, rng)
        for e, (lo, hi) in enumerate(t.ranges):
            for r in range(lo, hi):
                if r % 5 == 0:
                    c = int(np.abs(gy[r]).argmax())
                    gy[r, c] = np.float32(np.sign(gy[r, c]) * 1.01 * 256.0 / S[e, c])
    return gy


def reference(t, P, S, Z, gy):
    """float64 dX on the device: dY @ dequant(W_e) over the clipped range of every expert, zeros elsewhere."""
    ref = torch.zeros(t.T, 2 * P.shape[2], dtype=torch.float64, device="cuda")
    g = torch.as_tensor(gy).cuda().double()
    for e, (lo, hi) in enumerate(t.ranges):
        if hi > lo:
            ref[lo:hi] = g[lo:hi] @ dequant_f64(torch.from_numpy(P[e]).cuda(), torch.from_numpy(S[e]), torch.from_numpy(Z[e]))
    return ref


@functools.lru_cache(maxsize=None)
def reference_f32(name, N, K, centred, frac, heavy):
    t = table(name)
    return reference(t, *weights(t.E, N, K, centred, frac), gradient(name, N, K, centred, frac, heavy))


class Buffers:
    """The inputs of one call, each inside guards.  scales and zps are 16-byte aligned exactly when grad_out is: the
    vector pre-pass needs all three."""

    def __init__(self, t, P, S, Z, poff, in_aligned):
        self.P = guarded_like("packed", P, 0xFF, offset=poff)
        self.S = guarded_like("scales", S, NAN, offset=16 if in_aligned else 4)
        self.Z = guarded_like("zps", Z, NAN, offset=16 if in_aligned else 4)
        self.all = [self.P, self.S, self.Z]
        self.cnt = self.off = None
        if t.counts is not None:
            self.cnt = guarded_like("tokens_per_expert", t.counts, BIG)
            self.off = guarded_like("input_offsets", t.offs, BIG)
            self.all += [self.cnt, self.off]


def workspace_bytes(lib, t, K, N, prec):
    if t.counts is None:
        return lib.fql_linear_bwd_workspace_bytes(t.T, K, N, PREC[prec])
    return lib.fql_moe_bwd_workspace_bytes(t.E, t.T, K, N, PREC[prec])


def entry(lib, t, w, gy, idt, odt, K, N, prec):
    """(name, call(workspace pointer, workspace bytes, grad_in pointer)) of the entry point the case takes: the _f32 one
    for (float32, float32), the typed one otherwise."""
    p = (lambda g: g.ptr if g is not None else None)
    typed = (idt, odt) != (torch.float32, torch.float32)
    if t.counts is None:
        if typed:
            return "fql_linear_bwd_input", lambda wp, wb, op: lib.fql_linear_bwd_input(
                gy.ptr, DT[idt], w.P.ptr, w.S.ptr, w.Z.ptr, op, DT[odt], t.T, K, N, PREC[prec], wp, wb, stream())
        return "fql_linear_bwd_input_f32", lambda wp, wb, op: lib.fql_linear_bwd_input_f32(
            gy.ptr, w.P.ptr, w.S.ptr, w.Z.ptr, op, t.T, K, N, PREC[prec], wp, wb, stream())
    if typed:
        return "fql_moe_bwd_input", lambda wp, wb, op: lib.fql_moe_bwd_input(
            w.P.ptr, w.S.ptr, w.Z.ptr, gy.ptr, DT[idt], p(w.cnt), p(w.off), op, DT[odt], t.E, t.T, K, N, PREC[prec], wp, wb,
            stream())
    return "fql_moe_bwd_input_f32", lambda wp, wb, op: lib.fql_moe_bwd_input_f32(
        w.P.ptr, w.S.ptr, w.Z.ptr, gy.ptr, p(w.cnt), p(w.off), op, t.E, t.T, K, N, PREC[prec], wp, wb, stream())


def run_prefills(what, call, ws, out, dtype, shape, bufs):
    """(a) + (c): the call once per workspace prefill, the guards checked after every run, the results compared bit for
    bit.  Returns the first result."""
    outs = []
    for fill in PREFILLS:
        ws.bytes().fill_(fill)
        o = out.view(dtype, *shape)
        o.fill_(SENT)
        rc = call(ws.ptr, ws.nbytes, out.ptr)
        tag = f"{what}, workspace {fill:#04x}"
        assert rc == 0, (tag, rc)
        assert_guards_intact(out, ws, *bufs, what=tag)
        outs.append(o.clone())
    for fill, o in zip(PREFILLS[1:], outs[1:]):
        assert same_bits(o, outs[0]), f"{what}: the result depends on stale workspace bytes: prefill {fill:#04x} against " \
                                      f"{PREFILLS[0]:#04x}: (differing elements, first) = {first_diff(o, outs[0])}"
    return outs[0]


def delta_planes(lib, ws, t, N, prec):
    """delta [sets + 1][T] (delta, delta2 at 2 / 3 limbs, the float correction) behind the limbs (bwd_carve, fql_bwd.hip)."""
    sets = 2 if LIMBS[prec] >= 2 else 1
    lb = lib.fql_act_limb_bytes(t.T, t.E, N, PREC[prec])
    assert lb % 16 == 0 and lb + (sets + 1) * t.T * 4 <= ws.nbytes
    return ws.bytes()[lb:lb + (sets + 1) * t.T * 4].view(torch.float32).view(sets + 1, t.T)


def check_values(what, got, ref, t, gy, S, L, N):
    """(b): finite, the Frobenius bound of the mode, the per-row bound (at one limb on the rows without outliers, as
    tests/test_gpu_backward_paths.py applies it), and zeros in the rows no expert covers."""
    cov = torch.from_numpy(t.covered).cuda()
    assert bool(torch.isfinite(got).all()), what
    assert bool((got[~cov] == 0).all()), f"{what}: rows no expert covers must be zero"
    rows = cov
    if L == 1:
        g = torch.as_tensor(gy).cuda().double()
        for e, (lo, hi) in enumerate(t.ranges):
            g[lo:hi] *= torch.from_numpy(S[e]).cuda().double()
        rows = cov & (g.abs().amax(1) <= 5 * g.square().mean(1).sqrt())
    fro, row = rel_fro_dev(got, ref), row_rel_err(got[rows], ref[rows])
    print(f"{what}: fro {fro:.3e} (bound {fro_tol(L, N):.1e}) row {row:.3e} (bound {ROW_TOL[L]:.1e})")
    assert fro < fro_tol(L, N), (what, fro)
    assert row < ROW_TOL[L], (what, row)


def check_planes(lib, what, ws, t, N, prec, frac):
    """The residual set and the correction plane are in use where the case means them to be: at 2 / 3 limbs exactly the
    heavy-tailed rows that an expert covers carry a delta2 (none at an N that cannot flag)."""
    d = delta_planes(lib, ws, t, N, prec)
    cov = torch.from_numpy(t.covered).cuda()
    if LIMBS[prec] >= 2:
        heavy = torch.zeros(t.T, dtype=torch.bool, device="cuda")
        if flaggable(N):
            heavy[::5] = True
        flagged = (d[1] != 0) & cov
        assert torch.equal(flagged, heavy & cov), (what, (flagged != (heavy & cov)).nonzero().flatten().tolist())
    cor = d[-1][cov]
    assert bool((cor != 0).all()) if frac else bool((cor == 0).all()), what


def align_offsets(align, idt, odt):
    """Where grad_out and grad_in start, past a 256-byte boundary: 16 bytes, or one element."""
    return (16 if align in ("aligned", "out-element") else esize(idt)), (16 if align == "aligned" else esize(odt))


# ------------------------------------------------------------------------------ float32: every form of the kernels
@pytest.mark.parametrize("prec", ["exact", "fast", "int8"])
@pytest.mark.parametrize("N,align,K,poff,frac", SHAPES, ids=[f"N{n}-{a}-K{k}-p{p}{'-frac' if f else ''}" for n, a, k, p, f in SHAPES])
@pytest.mark.parametrize("name", TABLES)
def test_bwd_input_f32(lib, name, N, align, K, poff, frac, prec):
    t, L = table(name), LIMBS[prec]
    P, S, Z = weights(t.E, N, K, L == 1, frac)
    heavy = L >= 2 and flaggable(N)
    gy = gradient(name, N, K, L == 1, frac, heavy)
    goff, ooff = align_offsets(align, torch.float32, torch.float32)
    w = Buffers(t, P, S, Z, poff, goff == 16)
    g = guarded_like("grad_out", gy, NAN, offset=goff)
    ws = Guarded("workspace", workspace_bytes(lib, t, K, N, prec), torch.uint8, WS_PATTERN, offset=16)
    out = Guarded("grad_in", t.T * K * 4, torch.float32, SENT, offset=ooff)
    fn, call = entry(lib, t, w, g, torch.float32, torch.float32, K, N, prec)
    what = f"{fn} {name} N={N} K={K} {align} packed+{poff} {prec}{' frac' if frac else ''}"
    got = run_prefills(what, call, ws, out, torch.float32, (t.T, K), w.all + [g])
    check_values(what, got, reference_f32(name, N, K, L == 1, frac, heavy), t, gy, S, L, N)
    check_planes(lib, what, ws, t, N, prec, frac)


# ------------------------------------------------------------------------------ element types
PAIRS = [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]


@pytest.mark.parametrize("idt,odt", PAIRS, ids=[f"{DT_NAME[i]}-{DT_NAME[o]}" for i, o in PAIRS])
@pytest.mark.parametrize("N,align,K,frac", [(272, "aligned", 160, True), (200, "element", 138, False)])
@pytest.mark.parametrize("name", ["G1", "L129"])
def test_bwd_input_typed(lib, name, N, align, K, frac, idt, odt):
    """The typed entry points against the float32 entry point on the widened gradient, rounded once (include/fql_int4.h);
    G1's uncovered rows of a 16-bit grad_in come from the 2-byte zero fill."""
    t, prec = table(name), "exact"
    P, S, Z = weights(t.E, N, K, False, frac)
    gy = torch.from_numpy(gradient(name, N, K, False, frac, flaggable(N))).to(idt)
    wide = gy.float()

    def run(gyt, i, o):
        goff, ooff = align_offsets(align, i, o)
        w = Buffers(t, P, S, Z, 16, goff == 16)
        g = guarded_like("grad_out", gyt, NAN, offset=goff)
        ws = Guarded("workspace", workspace_bytes(lib, t, K, N, prec), torch.uint8, WS_PATTERN, offset=16)
        out = Guarded("grad_in", t.T * K * esize(o), o, SENT, offset=ooff)
        fn, call = entry(lib, t, w, g, i, o, K, N, prec)
        what = f"{fn} {name} N={N} K={K} {align} {DT_NAME[i]} -> {DT_NAME[o]}"
        got = run_prefills(what, call, ws, out, o, (t.T, K), w.all + [g])
        check_planes(lib, what, ws, t, N, prec, frac)
        return what, got

    what, base = run(wide, torch.float32, torch.float32)
    check_values(what, base, reference(t, P, S, Z, wide), t, wide, S, 3, N)
    what, got = run(gy, idt, odt)
    assert same_bits(got, base.to(odt)), (what, first_diff(got, base.to(odt)))
    assert bool((got[torch.from_numpy(~t.covered).cuda()] == 0).all()), what


# ------------------------------------------------------------------------------ empty calls
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16], ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize("name,empty", [("G1", "N"), ("G1", "T"), ("G1", "K"), ("G1", "E"), ("L129", "N"), ("L129", "T"), ("L129", "K")])
def test_bwd_input_empty(lib, name, empty, odt):
    """N == 0 (and E == 0, grouped): grad_in is zeroed, T * K elements of its type and not a byte more.  T == 0 and
    K == 0: nothing is written.  The other pointers are not needed then and are not given."""
    t, K = table(name), 138
    out = Guarded("grad_in", t.T * K * esize(odt), odt, SENT, offset=esize(odt))
    o = out.view(odt, t.T, K)
    o.fill_(SENT)
    E, T, Kc, N = (0 if empty == "E" else t.E), (0 if empty == "T" else t.T), (0 if empty == "K" else K), (0 if empty == "N" else 200)
    typed = odt != torch.float32
    if t.counts is None:
        fn = "fql_linear_bwd_input" if typed else "fql_linear_bwd_input_f32"
        rc = (lib.fql_linear_bwd_input(None, DT[odt], None, None, None, out.ptr, DT[odt], T, Kc, N, 0, None, 0, stream()) if typed
              else lib.fql_linear_bwd_input_f32(None, None, None, None, out.ptr, T, Kc, N, 0, None, 0, stream()))
    else:
        fn = "fql_moe_bwd_input" if typed else "fql_moe_bwd_input_f32"
        rc = (lib.fql_moe_bwd_input(None, None, None, None, DT[odt], None, None, out.ptr, DT[odt], E, T, Kc, N, 0, None, 0, stream())
              if typed else lib.fql_moe_bwd_input_f32(None, None, None, None, None, None, out.ptr, E, T, Kc, N, 0, None, 0, stream()))
    what = f"{fn} {name} {empty} == 0 -> {DT_NAME[odt]}"
    assert rc == 0, (what, rc)
    assert_guards_intact(out, what=what)
    want = 0.0 if empty in ("N", "E") else SENT
    assert bool((o == want).all()), f"{what}: grad_in must hold {want} everywhere"
