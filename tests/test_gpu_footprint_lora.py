"""Where the adapter kernels and the SwiGLU backward write, and what else they read (csrc/fql_lora.h, fql_lora.hip,
fql_lora16.hip, fql_ffn16.hip): the method of tests/test_gpu_footprint.py on fql_lora_shrink / _expand / _grad,
fql_lora_gated_shrink / _gated_grad and fql_swiglu_bwd, each as its _f32 and its typed entry point, through the C ABI.
These kernels have no workspace, so a case asserts
  (a) every guard is intact after the call: outputs lie between SENT and hold SENT before the call, float inputs
      between NaN, the expert table between BIG;
  (b) the interior against float64 at the bound the suite states for the path (helpers.ADAPTER_TOL for the float32
      kernels, helpers.F32_TOL for a gated gradient and for a 16-bit shrink that takes a narrower width than the float32
      call would); a 16-bit call bit for bit the float32 call on the widened operand (expand: rounded once) wherever
      the header promises it: shrink at equal widths, expand and grad always.
A load that is fetched and then masked away cannot be seen this way, and is not looked for.

The table is that of tests/test_gpu_lora16.py (counts [7, 0, 33, 1, 20, 64], gaps [0, 2, 0, 5, 0, 1], tail 3: T = 136, two
full 64-row coverage blocks and one of 8 rows, an empty expert), the same with a last count that leaves [0, T), and the
E == 1 form without a table.  C is the smallest at which every loop wraps once and every last block is nearly empty:
2052 at VEC 4 (513 groups over the 512 lanes of shrink; 3 column blocks in expand, the last of 4 columns), 1030 at VEC 2
(515 pairs; a last block of 6), 515 at VEC 1 (a last block of 3); and C = 2052 with the [T][C] bases one element past a
16-byte boundary (VEC 1 on a wide shape; shrink is then held to float64 only: the header promises its bits at equal
widths).  w, v (grad) and d are 16-byte aligned (the library refuses less), every other pointer element-aligned.  Rows
no expert covers hold NaN in the operand of shrink and grad: they must not reach a sum."""
import functools

import pytest
import torch

from helpers import (ADAPTER_TOL, BIG, EXACT_REL_FRO, F32_TOL, NAN, SENT, Guarded, assert_guards_intact, clipped_ranges,
                     expert_table, first_diff, guarded_like, rel_fro_dev, row_rel_err, same_bits)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DT = {F32: 0, F16: 1, BF16: 2}
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
DTYPES = [F32, F16, BF16]
RC, CR = 0, 1
LAYOUTS = {"rc": RC, "cr": CR}
RANKS = [4, 16, 64]                 # shrink tiles of 16, 4 and 1 rows
TABLES = ["T16", "T16c", "none"]
WIDTHS = [(4, 2052, True), (2, 1030, True), (1, 515, True), (1, 2052, False)]     # (VEC, C, [T][C] bases 16-byte aligned)
WIDTH_IDS = ["vec4-C2052", "vec2-C1030", "vec1-C515", "off1-C2052"]
SCALE = 1.5


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


def matrix(li, wi, di):
    """(rank, table) of a case, rotated so that every (layout, width, element type) runs once and every rank and every
    table once per (layout, width) and per (layout, element type)."""
    return RANKS[(li + wi + di) % 3], TABLES[(2 * li + wi + 2 * di) % 3]


CASES = [pytest.param(ln, w, dt, *matrix(li, wi, di), id=f"{ln}-{WIDTH_IDS[wi]}-{DT_NAME[dt]}")
         for li, ln in enumerate(LAYOUTS) for wi, w in enumerate(WIDTHS) for di, dt in enumerate(DTYPES)]


# ------------------------------------------------------------------------------ problems
class Problem:
    pass


@functools.lru_cache(maxsize=None)
def table(name):
    t = Problem()
    counts, gaps, tail = [7, 0, 33, 1, 20, 64], [0, 2, 0, 5, 0, 1], 3
    tpe, offs, t.T = expert_table(counts, gaps, tail, device="cpu")
    if name == "none":
        t.E, t.tpe, t.offs, t.ranges = 1, None, None, [(0, t.T)]
    else:
        if name == "T16c":
            tpe[-1] = 999                                   # the last range leaves [0, T): clipped on the device
        t.E, t.tpe, t.offs = len(counts), tpe, offs
        t.ranges = clipped_ranges(tpe, offs, t.T)
    t.covered = torch.zeros(t.T, dtype=torch.bool)
    for lo, hi in t.ranges:
        t.covered[lo:hi] = True
    assert bool(t.covered.all()) == (name == "none")
    assert any(hi == lo for lo, hi in t.ranges) == (name != "none")
    t.covered = t.covered.to(DEV)
    return t


def draw(seed, t, C, r, dtype, gated=False):
    """The operands of one case on the device: X [T][C] (gated: gate_up [T][2C]) of ``dtype``, the adapter matrix M
    [E][r][C] and V [T][r] in float32."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    X = torch.randn(t.T, 2 * C if gated else C, device=DEV, generator=g).to(dtype)
    M = torch.randn(t.E, r, C, device=DEV, generator=g) * 0.1
    V = torch.randn(t.T, r, device=DEV, generator=g)
    return X, M, V


def stored(M, layout):
    """M_e [r][C] as the layout stores it: [E][r][C] (rc) or [E][C][r] (cr)."""
    return M if layout == RC else M.transpose(1, 2).contiguous()


def hidden64(gate_up):
    C = gate_up.shape[1] // 2
    g = gate_up.double()
    return torch.nn.functional.silu(g[:, :C]) * g[:, C:]


def base_offset(aligned, dtype):
    """Where a [T][C] operand starts, past a 256-byte boundary: 16 bytes, or one element past such a boundary."""
    return 16 if aligned else 16 + esize(dtype)


class TableBuffers:
    def __init__(self, t):
        self.cnt = guarded_like("tokens_per_expert", t.tpe, BIG) if t.tpe is not None else None
        self.off = guarded_like("input_offsets", t.offs, BIG) if t.tpe is not None else None
        self.all = [b for b in (self.cnt, self.off) if b is not None]
        self.cp = self.cnt.ptr if self.cnt is not None else None
        self.op = self.off.ptr if self.off is not None else None


def check(what, got, ref, tol, rows=True):
    """Frobenius and (``rows``) per-row bound, rows of the output as stored (tests/test_gpu_lora_paths.py check)."""
    assert bool(torch.isfinite(got).all()), what
    got2, ref2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    fro = rel_fro_dev(got2, ref2)
    row = row_rel_err(got2, ref2) if rows else 0.0
    print(f"{what}: fro {fro:.3e} row {row:.3e} (bound {tol:.1e})")
    assert fro < tol, (what, fro)
    assert row < tol, (what, row)


def launch(what, call, out, view, bufs):
    """(a): SENT inside, the call, every guard intact.  Returns a copy of the interior."""
    o = out.view(*view)
    o.fill_(SENT)
    rc = call(out.ptr)
    assert rc == 0, (what, rc)
    assert_guards_intact(out, *bufs, what=what)
    return o.clone()


def with_nan_rows(X, t):
    """X with NaN in the rows no expert covers (never modified afterwards)."""
    X = X.clone()
    X[~t.covered] = NAN
    return X


# ------------------------------------------------------------------------------ shrink and gated shrink
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("layout,width,dtype,r,tname", CASES)
def test_shrink(lib, layout, width, dtype, r, tname, gated):
    vec, C, aligned = width
    t, lay = table(tname), LAYOUTS[layout]
    X, M, _ = draw(100 * C + r + gated, t, C, r, dtype, gated)
    X = with_nan_rows(X, t)
    tb = TableBuffers(t)
    gw = guarded_like("w", stored(M, lay), NAN, offset=16)
    name = "fql_lora_gated_shrink" if gated else "fql_lora_shrink"

    def run(x, dt):
        gx = guarded_like("gate_up" if gated else "in", x, NAN, offset=base_offset(aligned, dt))
        out = Guarded("out", t.T * r * 4, F32, SENT, offset=4)
        if dt == F32:
            fn = getattr(lib, name + "_f32")
            call = lambda op: fn(gx.ptr, gw.ptr, lay, tb.cp, tb.op, op, t.E, t.T, C, r, SCALE, stream())
        else:
            fn = getattr(lib, name)
            call = lambda op: fn(gx.ptr, DT[dt], gw.ptr, lay, tb.cp, tb.op, op, t.E, t.T, C, r, SCALE, stream())
        what = f"{name}{'_f32' if dt == F32 else ''} {layout} C={C} {'aligned' if aligned else 'one element off'} " \
               f"{DT_NAME[dt]} r={r} {tname}"
        return what, launch(what, call, out, (F32, t.T, r), tb.all + [gw, gx])

    ref = torch.zeros(t.T, r, dtype=torch.float64, device=DEV)
    h = hidden64(X) if gated else X.double()
    for e, (lo, hi) in enumerate(t.ranges):
        ref[lo:hi] = SCALE * h[lo:hi] @ M[e].double().T
    what, got = run(X, dtype)
    assert bool((got[~t.covered] == 0).all()), f"{what}: rows no expert covers must be zero"
    if dtype == F32 or not aligned:
        check(what, got, ref, ADAPTER_TOL if dtype == F32 else F32_TOL, rows=not gated)
    else:                                                    # equal widths: the bits of the float32 call on the widened operand
        what32, base = run(X.float(), F32)
        check(what32, base, ref, ADAPTER_TOL, rows=not gated)
        assert same_bits(got, base), (what, first_diff(got, base))


# ------------------------------------------------------------------------------ expand
def expand_case(lib, layout, width, idt, odt, r, tname, mode):
    vec, C, aligned = width
    t, lay = table(tname), LAYOUTS[layout]
    Y, M, V = draw(200 * C + r + len(mode), t, C, r, idt)
    tb = TableBuffers(t)
    gw = guarded_like("w", stored(M, lay), NAN, offset=16)
    gv = guarded_like("v", V, NAN, offset=4)

    def run(y, i, o):
        gin = guarded_like("in", y, NAN, offset=base_offset(aligned, i)) if mode == "in" else None
        out = Guarded("out", t.T * C * esize(o), o, SENT, offset=base_offset(aligned, o))
        what = f"fql_lora_expand{'_f32' if (i, o) == (F32, F32) else ''} {layout} C={C} " \
               f"{'aligned' if aligned else 'one element off'} {DT_NAME[i]} -> {DT_NAME[o]} r={r} {tname} {mode}"

        def call(op):
            ip = {"in": gin.ptr if gin is not None else None, "null": None, "inplace": op}[mode]
            if mode == "inplace":
                out.view(o, t.T, C).copy_(y)                 # (after launch() filled it with SENT)
            if (i, o) == (F32, F32):
                return lib.fql_lora_expand_f32(gv.ptr, gw.ptr, lay, tb.cp, tb.op, ip, op, t.E, t.T, C, r, SCALE, stream())
            return lib.fql_lora_expand(gv.ptr, gw.ptr, lay, tb.cp, tb.op, ip, DT[i], op, DT[o], t.E, t.T, C, r, SCALE, stream())

        return what, launch(what, call, out, (o, t.T, C), tb.all + [gw, gv] + ([gin] if gin is not None else []))

    start = torch.zeros(t.T, C, dtype=torch.float64, device=DEV) if mode == "null" else Y.double()
    ref = start.clone()
    for e, (lo, hi) in enumerate(t.ranges):
        ref[lo:hi] += SCALE * V[lo:hi].double() @ M[e].double()
    what, got = run(Y, idt, odt)
    unc = ~t.covered
    if mode == "null":
        assert bool((got[unc] == 0).all()), f"{what}: rows no expert covers must be zero"
    elif idt == odt:                                         # copied, or left alone in place: the exact bits
        assert same_bits(got[unc], Y[unc]), (what, first_diff(got[unc], Y[unc]))
    if (idt, odt) == (F32, F32):
        check(what, got, ref, ADAPTER_TOL)
    else:                      # (one lane per output column, j ascending: the bits do not depend on the width)
        what32, base = run(Y.float(), F32, F32)
        check(what32, base, ref, ADAPTER_TOL)
        assert same_bits(got, base.to(odt)), (what, first_diff(got, base.to(odt)))


@pytest.mark.parametrize("mode", ["in", "null", "inplace"])
@pytest.mark.parametrize("layout,width,dtype,r,tname", CASES)
def test_expand(lib, layout, width, dtype, r, tname, mode):
    """in != out: rows no expert covers are copied; in == NULL: they are zero; in == out: they keep their bits."""
    expand_case(lib, layout, width, dtype, dtype, r, tname, mode)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_expand_f32_in_bf16_out(lib, layout):
    expand_case(lib, layout, WIDTHS[0], F32, BF16, 16, "T16", "in")


# ------------------------------------------------------------------------------ grad and gated grad
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("layout,width,dtype,r,tname", CASES)
def test_grad(lib, layout, width, dtype, r, tname, gated):
    """d in both layouts; an expert without rows gives an all-zero d_e; the NaN rows no expert covers stay out of the sums."""
    vec, C, aligned = width
    t, lay = table(tname), LAYOUTS[layout]
    X, _, V = draw(300 * C + r + gated, t, C, r, dtype, gated)
    X = with_nan_rows(X, t)
    tb = TableBuffers(t)
    gv = guarded_like("v", V, NAN, offset=16)
    name = "fql_lora_gated_grad" if gated else "fql_lora_grad"
    shape = (t.E, r, C) if lay == RC else (t.E, C, r)

    def run(x, dt):
        gx = guarded_like("gate_up" if gated else "p", x, NAN, offset=base_offset(aligned, dt))
        d = Guarded("d", t.E * r * C * 4, F32, SENT, offset=16)
        if dt == F32:
            fn = getattr(lib, name + "_f32")
            call = lambda op: fn(gx.ptr, gv.ptr, tb.cp, tb.op, op, lay, t.E, t.T, C, r, SCALE, stream())
        else:
            fn = getattr(lib, name)
            call = lambda op: fn(gx.ptr, DT[dt], gv.ptr, tb.cp, tb.op, op, lay, t.E, t.T, C, r, SCALE, stream())
        what = f"{name}{'_f32' if dt == F32 else ''} {layout} C={C} {'aligned' if aligned else 'one element off'} " \
               f"{DT_NAME[dt]} r={r} {tname}"
        return what, launch(what, call, d, (F32,) + shape, tb.all + [gv, gx])

    ref = torch.zeros(t.E, r, C, dtype=torch.float64, device=DEV)
    h = hidden64(X) if gated else X.double()
    for e, (lo, hi) in enumerate(t.ranges):
        if hi > lo:
            ref[e] = SCALE * V[lo:hi].double().T @ h[lo:hi]
    ref = ref if lay == RC else ref.transpose(1, 2)
    what, got = run(X, dtype)
    for e, (lo, hi) in enumerate(t.ranges):
        if hi == lo:
            assert bool((got[e] == 0).all()), f"{what}: expert {e} has no rows: d_e must be zero"
    tol = F32_TOL if gated else ADAPTER_TOL
    if dtype == F32:
        check(what, got, ref, tol, rows=not gated)
    else:                      # (one lane per output column, a fixed order over t: the bits do not depend on the width)
        what32, base = run(X.float(), F32)
        check(what32, base, ref, tol, rows=not gated)
        assert same_bits(got, base), (what, first_diff(got, base))


# ------------------------------------------------------------------------------ SwiGLU backward
def swiglu_ref(gate_up, dh):
    F = dh.shape[1]
    g, u, d = gate_up[:, :F].double(), gate_up[:, F:].double(), dh.double()
    sig = 1.0 / (1.0 + torch.exp(-g))
    return torch.cat([d * u * (sig * (1.0 + g * (1.0 - sig))), d * (g * sig)], dim=1)


TRIPLES = [(F32, F32, F32), (F16, F16, F16), (BF16, BF16, BF16), (BF16, F32, F32)]      # gate_up, dh, dgate_up


@pytest.mark.parametrize("dg,dd,do", TRIPLES, ids=["-".join(DT_NAME[d] for d in tr) for tr in TRIPLES])
@pytest.mark.parametrize("F,dh_off", [(516, False), (515, False), (516, True)], ids=["F516", "F515", "F516-dh-off"])
def test_swiglu_bwd(lib, F, dh_off, dg, dd, do):
    """T = 5.  F = 516: the wide form, 645 lanes, a third block partly filled; F = 515, and F = 516 with dh one element
    past a 16-byte boundary: the scalar form.  One very negative g: sigma = 0, both gradients 0, everything finite."""
    T = 5
    g = torch.Generator(device=DEV).manual_seed(F + dh_off)
    gu = torch.randn(T, 2 * F, device=DEV, generator=g)
    gu[2, 7] = -200.0
    gu, dh = gu.to(dg), torch.randn(T, F, device=DEV, generator=g).to(dd)

    def run(a, b, ta, tb_, to):
        ga = guarded_like("gate_up", a, NAN, offset=16)
        gb = guarded_like("dh", b, NAN, offset=base_offset(not dh_off, tb_))
        out = Guarded("dgate_up", T * 2 * F * esize(to), to, SENT, offset=16)
        if (ta, tb_, to) == (F32, F32, F32):
            what = f"fql_swiglu_bwd_f32 F={F} dh off {dh_off}"
            call = lambda op: lib.fql_swiglu_bwd_f32(ga.ptr, gb.ptr, op, T, F, stream())
        else:
            what = f"fql_swiglu_bwd F={F} dh off {dh_off} {DT_NAME[ta]} {DT_NAME[tb_]} -> {DT_NAME[to]}"
            call = lambda op: lib.fql_swiglu_bwd(ga.ptr, DT[ta], gb.ptr, DT[tb_], op, DT[to], T, F, stream())
        return what, launch(what, call, out, (to, T, 2 * F), [ga, gb])

    what32, base = run(gu.float(), dh.float(), F32, F32, F32)
    assert bool(torch.isfinite(base).all()) and float(base[2, 7]) == 0.0 and float(base[2, F + 7]) == 0.0, what32
    err = rel_fro_dev(base, swiglu_ref(gu, dh))
    print(f"{what32}: fro {err:.3e} (bound {EXACT_REL_FRO:.1e})")
    assert err < EXACT_REL_FRO, (what32, err)
    if (dg, dd, do) != (F32, F32, F32):
        what, got = run(gu, dh, dg, dd, do)
        assert same_bits(got, base.to(do)), (what, first_diff(got, base.to(do)))
