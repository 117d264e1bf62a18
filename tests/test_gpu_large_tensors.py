"""Operands past 2 GiB and 4 GiB: every kernel family on a tensor whose byte offsets cross B31 = 2^31 and B32 = 2^32.

The rest of the suite never hands a kernel more than a few megabytes, while the library promises 64-bit addressing of
every operand (or refuses / changes path at a documented limit).  A 32-bit product that wraps at
2^31 or 2^32 reads the wrong expert or writes the wrong row, and no small shape shows it.  Here:

  * every operand of more than 2^31 bytes lives in a ``helpers.BigGuarded`` buffer: 2^31 bytes of poisoned guard in
    front of it, so a sign-wrapped offset lands in memory the test owns (an unsigned wrap lands inside the operand
    itself); NaN around float inputs, 0xFF around packed weights and scale bytes, SENT around outputs;
  * the shapes come from the library's own limits (``fql_native_dtype_supported``, ``fql_act_limb_bytes``) and the
    deriving functions assert what they derived; everything else is minimal (K = 32, N with a row stride that does not
    divide 2^31, so that one row really straddles each boundary);
  * the work is kept small by the expert table: 33 rows at the start, 70 rows around the row that crosses B31, 70 around
    the one that crosses B32, 33 rows ending 2 rows before T (``helpers.row_groups``); every other row must be exactly
    zero (``count_nonzero`` on the device);
  * the reference is float64 on the device from the covered slices only; the bound is the family's existing one
    (helpers.py, tests/test_gpu_mxfp4.py), equality where the family has an exact data recipe;
  * each case asserts that its data can tell a wrap from no wrap: what lies at ``offset mod 2^32`` and at the
    sign-wrapped offset differs from what lies at the offset (inputs), or is a row that must stay zero / a guard byte
    (outputs).

Memory: each test checks ``torch.cuda.mem_get_info()`` first, holds at most 24 GiB and frees its buffers at the end."""
import ctypes
import gc

import pytest
import torch

from helpers import (ADAPTER_TOL, B31, B32, EXACT_REL_FRO, F32_TOL, FMA_REL_FRO, FP8_FORMAT_REL_FRO, NAN, SENT, BigGuarded,
                     assert_guards_intact, dequant_f64, fro_tol, free_gib, ops, rel_fro_dev, row_groups, same_bits,
                     wrapped_offsets)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREC = {"int8": 1, "fast": 2, "exact": 3, "fp8": 8}
LIMBS = {"int8": 1, "fast": 2, "exact": 3, "fp8": 1}
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
OK, SHAPE, ALIGN, DTYPE = 0, -2, -7, -8
P16 = ctypes.c_void_p(16)          # a 16-byte aligned weight pointer for the shape queries (never dereferenced)
MAX_GIB = 24
MX4_KERNEL = {"tile": 0, "decode": 1}                        # what fql_tune_mx4_kernel reports


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fused_int4_amd import _native
    h = _native.lib()
    for name in ("fql_tune_is_config", "fql_tune_chosen_cfg"):
        getattr(h, name).restype = ctypes.c_int
        getattr(h, name).argtypes = [ctypes.c_int] * (2 if name == "fql_tune_is_config" else 6)
    return h


@pytest.fixture(autouse=True)
def release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def need(gib):
    """The test is about to hold ``gib`` GiB: skip only when the device does not have them free."""
    assert gib <= MAX_GIB
    gc.collect()
    torch.cuda.empty_cache()
    if free_gib() < gib + 1:
        pytest.skip(f"{gib} GiB needed, {free_gib():.1f} GiB free")


def tol_of(prec, K):
    return FP8_FORMAT_REL_FRO if prec == "fp8" else fro_tol(LIMBS[prec], K)


def table_of(groups, E=None, experts=None, T=None):
    """(tokens_per_expert, input_offsets) int32 on the device: group i goes to expert ``experts[i]`` (default i) of E."""
    experts = list(range(len(groups))) if experts is None else experts
    E = len(groups) if E is None else E
    tpe = torch.zeros(E, dtype=torch.int32)
    offs = torch.full((E,), 0 if T is None else T, dtype=torch.int32)
    for (lo, hi), e in zip(groups, experts):
        tpe[e], offs[e] = hi - lo, lo
    return tpe.to(DEV), offs.to(DEV)


def int4_weights(E, N, K, seed):
    """Codes drawn directly (tests/test_gpu_footprint.py): packed [E, N, K/2], scales in [1e-3, 3e-3], zero points 5..10."""
    g = torch.Generator().manual_seed(seed)
    P = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8)
    S = 0.001 + 0.002 * torch.rand(E, N, generator=g)
    Z = torch.randint(5, 11, (E, N), generator=g).float()
    return P.to(DEV), S.to(DEV), Z.to(DEV)


def output_wrap_is_visible(groups, row_bytes, buf):
    """Where a store to a covered row lands when its byte offset is truncated to 32 bits, for EVERY covered row: in the
    front guard (which must keep its pattern), on rows no group covers (which must stay zero), or on rows of ANOTHER
    group (never its own).  In each case the row's own place is then not written: it keeps the sentinel the output was
    filled with, which the comparison with the reference sees.  Returns how many rows would land on another group."""
    seen = hits = 0
    for gi, (lo, hi) in enumerate(groups):
        for t in range(lo, hi):
            for w in wrapped_offsets(t * row_bytes):
                if w is None:
                    continue
                seen += 1
                if w < 0:
                    assert -w <= buf.front, (t, w)
                    continue
                r = w // row_bytes                           # the store touches rows r and r + 1
                for gj, (a, b) in enumerate(groups):
                    if not (r + 1 < a or r >= b):
                        assert gj != gi, (t, w, r, groups)
                        hits += 1
    assert seen >= 60          # the rows past B31 (and past B32, where the operand gets there) are covered ones
    return hits


def input_wrap_is_visible(buf, byte_offset, n):
    """``n`` elements at ``byte_offset`` of the operand differ from what a truncated offset would read instead."""
    true = buf.at(byte_offset, n)
    seen = 0
    for w in wrapped_offsets(byte_offset):
        if w is not None:
            seen += 1
            assert not torch.equal(true.view(buf.idt), buf.at(w, n).view(buf.idt)), (byte_offset, w)
    return seen


def check_rows(out, groups, refs, bound, what, exact=False):
    """Covered rows against their float64 reference; every other row exactly zero (counted on the device)."""
    nz = 0
    for (lo, hi), ref in zip(groups, refs):
        got = out[lo:hi]
        if exact:
            assert torch.equal(got.double(), ref), (what, lo)
        else:
            err = rel_fro_dev(got, ref)
            print(f"{what}: rows [{lo}, {hi}) rel_fro {err:.3e} (bound {bound:.1e})")
            assert err <= bound, (what, lo, err)
        nz += int(torch.count_nonzero(got))
    assert int(torch.count_nonzero(out)) == nz, f"{what}: a row no expert covers is not zero"


# ======================================================================= INT4 per-row grouped forward: a large OUTPUT
def largest_rows(lib, prec, E, K, N):
    """The largest T the matrix-core path takes (``fql_native_dtype_supported``), found by bisection, with what it means
    asserted: the limb buffer of T rows stays below 2^31 bytes and that of T + 1 rows does not."""
    ok = lambda T: lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], P16, 1) == 1
    lo, hi = 1, (1 << 31) - 1
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert ok(lo) and not ok(lo + 1)
    assert lib.fql_act_limb_bytes(lo, E, K, PREC[prec]) < B31 <= lib.fql_act_limb_bytes(lo + 1, E, K, PREC[prec])
    return lo


def output_shape(lib, prec, K, esz):
    """(T, N): T the row limit of the matrix-core path, N the smallest of 136, 264, 392, ... (8 past a multiple of 128:
    the row stride divides no power of two above it) with which the output passes 2^32 bytes before the last group.
    A 16-bit output of fewer than 2^31 elements ends below 2^32 bytes: it is taken past 2^31 bytes instead (three row
    groups)."""
    E = 4
    top = B32 if esz == 4 else B31
    T = largest_rows(lib, prec, E, K, 136)
    N = 136
    while top // (N * esz) + 36 > T - 36:
        N += 128
    assert largest_rows(lib, prec, E, K, N) == T and T * N < (1 << 31) and T * N * esz > top
    return T, N


class Int4Output:
    """x [T + 1, K], weights of 4 experts, the four row groups and their float64 references (both for T and T + 1 rows)."""

    def __init__(self, lib, prec, K, out_dtype):
        esz = torch.empty((), dtype=out_dtype).element_size()
        self.T, self.N = output_shape(lib, prec, K, esz)
        self.K, self.E, self.prec, self.esz = K, 4, prec, esz
        g = torch.Generator(device=DEV).manual_seed(7)
        self.x = torch.randn(self.T + 1, K, generator=g, device=DEV)
        self.P, self.S, self.Z = int4_weights(self.E, self.N, K, 5)
        self.W = [dequant_f64(self.P[e], self.S[e], self.Z[e]) for e in range(self.E)]
        self.out = BigGuarded("out", (self.T + 1) * self.N * esz, out_dtype, SENT)

    def groups(self, T):
        g = row_groups(T, self.N * self.esz)
        assert len(g) == (4 if self.esz == 4 else 3)
        return g

    def refs(self, groups, x=None):
        x = self.x if x is None else x
        return [x[lo:hi].double() @ self.W[e].T for e, (lo, hi) in enumerate(groups)]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("prec,K", [("exact", 32), ("fast", 32), ("int8", 32), ("fp8", 32), ("exact", 288)])
def test_int4_forward_large_output_below_the_row_limit(lib, prec, K, out_dtype):
    """T at the row limit of ``mfma_addressable``, T * N * esz > 2^32 (bfloat16: > 2^31, see ``output_shape``).  The
    product entry (``fql_moe_fwd``: pre-pass +
    the GEMM it chooses, uncovered rows zeroed by the pre-pass), then every tile configuration built for the precision,
    pinned through ``ops.tune_gemm_i8`` on limbs from ``ops.act_quant`` (K = 288: the one-wave kernels 300 / 301, which
    need two 256-k stages)."""
    need(20)
    p = Int4Output(lib, prec, K, out_dtype)
    T, N, E = p.T, p.N, p.E
    groups = p.groups(T)
    tpe, offs = table_of(groups, E=E)
    xin = p.x[:T] if out_dtype == torch.float32 else p.x[:T].to(out_dtype)
    refs = p.refs(groups, xin)
    bound = tol_of(prec, K) + (2.0 ** -9 if out_dtype == torch.bfloat16 else 0.0)      # + one rounding of the result
    output_wrap_is_visible(groups, N * p.esz, p.out)
    out = p.out.view(T + 1, N)
    out.fill_(SENT)
    chosen = lib.fql_tune_chosen_cfg(PREC[prec], E, T, K, N, 1)
    assert lib.fql_tune_is_config(chosen, PREC[prec]) == 1 and (chosen < 100 or chosen >= 300), chosen   # a 64 / 128-row tile
    print(f"int4 large output {prec} K={K} {out_dtype}: T={T} N={N} out {T * N * p.esz / 2 ** 30:.2f} GiB, product cfg {chosen}")
    ops()._launch("fql_moe_fwd", out.device, p.P, p.S, p.Z, xin.contiguous(), DT[xin.dtype], tpe, offs, out, DT[out_dtype],
                  E, T, K, N, PREC[prec], ws_bytes=lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]))
    torch.cuda.synchronize()
    check_rows(out[:T], groups, refs, bound, f"product cfg {chosen}")
    assert bool((out[T] == SENT).all())
    assert_guards_intact(p.out, what="fql_moe_fwd")

    limbs, delta, rowsum = ops().act_quant(p.x[:T], prec, tpe, offs)
    ids = [c for c in range(0, 310) if lib.fql_tune_is_config(c, PREC[prec]) == 1]
    if K > 256:
        ids = [c for c in ids if c >= 300 or c == chosen]   # (K = 288 is about 300 / 301; the others run at K = 32)
    refs32 = p.refs(groups)                                 # (the limbs come from the float32 rows)
    ran = []
    for cfg in ids:
        for lo, hi in groups:
            out[lo:hi].zero_()
        rc = ops().tune_gemm_i8(cfg, limbs, delta, rowsum, p.P, p.S, p.Z, tpe, offs, out, E, T, K, N, prec, out_dtype=out_dtype)
        if cfg >= 300 and K < 257:
            assert rc == SHAPE, (cfg, rc)              # one 256-k stage: the one-wave kernels refuse
            continue
        assert rc == OK, (cfg, rc)
        torch.cuda.synchronize()
        check_rows(out[:T], groups, refs32, bound, f"cfg {cfg}")
        ran.append(cfg)
    print(f"int4 large output {prec} K={K}: pinned ids {ran}")
    families = {"wide": any(c < 100 for c in ran), "rows32": any(100 <= c < 200 for c in ran),
                "rows16": any(200 <= c < 300 for c in ran), "one-wave": any(c >= 300 for c in ran)}
    if prec == "fp8":
        assert families["wide"]
    elif K > 256:
        assert families["one-wave"] and 300 in ran and 301 in ran
    else:
        assert families["wide"] and families["rows32"] and families["rows16"]
    assert bool((out[T] == SENT).all())
    assert_guards_intact(p.out, what="tune_gemm_i8")
    del p, out, limbs, delta, rowsum


@pytest.mark.parametrize("prec", ["exact", "fast", "int8"])
def test_int4_forward_one_row_above_the_row_limit(lib, prec):
    """T + 1 rows: ``fql_native_dtype_supported`` says no.  The float32 entry silently runs the generic kernel and must
    return its result within the generic bound; the 16-bit, fp8, gather, row-weight and gated entries refuse with their
    documented code and write nothing; ``ops.moe_forward_any`` still answers through its float32 fallback."""
    need(22)
    K = 32
    p = Int4Output(lib, prec, K, torch.float32)
    T, N, E = p.T + 1, p.N, p.E
    assert lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], P16, 1) == 0
    groups = p.groups(T)
    tpe, offs = table_of(groups)
    refs = p.refs(groups)
    output_wrap_is_visible(groups, N * 4, p.out)
    out = p.out.view(T, N)
    out.fill_(SENT)
    L = ops()
    ws = torch.empty(lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]) + 16, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    x16 = p.x.bfloat16()
    ri = torch.arange(T, dtype=torch.int32, device=DEV)
    rw = torch.ones(T, device=DEV)
    ptr = lambda t: t.data_ptr()
    refused = {
        "fql_moe_fwd bf16": (lib.fql_moe_fwd(ptr(p.P), ptr(p.S), ptr(p.Z), ptr(x16), 2, ptr(tpe), ptr(offs), ptr(out), 2, E, T,
                                             K, N, PREC[prec], ptr(ws), ws.numel(), st), DTYPE),
        "fql_moe_gather_fwd_f32": (lib.fql_moe_gather_fwd_f32(ptr(p.P), ptr(p.S), ptr(p.Z), ptr(p.x), ptr(ri), T, ptr(tpe),
                                                              ptr(offs), ptr(out), E, T, K, N, PREC[prec], ptr(ws), ws.numel(),
                                                              st), ALIGN),
        "fql_moe_gather_scaled_fwd_f32": (lib.fql_moe_gather_scaled_fwd_f32(ptr(p.P), ptr(p.S), ptr(p.Z), ptr(p.x), ptr(ri), T,
                                                                            ptr(rw), ptr(tpe), ptr(offs), ptr(out), E, T, K, N,
                                                                            PREC[prec], ptr(ws), ws.numel(), st), ALIGN),
    }
    # gate | up rows [T, 2 K'] with K' = K: the down projection of a gated expert
    gu = torch.zeros(T, 2 * K, device=DEV)
    refused["fql_moe_gated_fwd_f32"] = (lib.fql_moe_gated_fwd_f32(ptr(p.P), ptr(p.S), ptr(p.Z), ptr(gu), ptr(tpe), ptr(offs),
                                                                  ptr(out), E, T, K, N, PREC[prec], ptr(ws), ws.numel(), st),
                                        ALIGN)
    if prec == "int8":            # fp8 rows have int8's one byte plane, hence its row limit: no float32 kernel stands in
        refused["fql_moe_fwd_f32 fp8"] = (lib.fql_moe_fwd_f32(ptr(p.P), ptr(p.S), ptr(p.Z), ptr(p.x), ptr(tpe), ptr(offs),
                                                              ptr(out), E, T, K, N, 8, ptr(ws), ws.numel(), st), ALIGN)
    for name, (rc, want) in refused.items():
        assert rc == want, (name, rc, want)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote to its output"
    del gu, ri, rw, ws, x16

    L._launch("fql_moe_fwd_f32", out.device, p.P, p.S, p.Z, p.x, tpe, offs, out, E, T, K, N, PREC[prec],
              ws_bytes=lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]))
    torch.cuda.synchronize()
    check_rows(out, groups, refs, FMA_REL_FRO, "generic fallback")
    assert_guards_intact(p.out, what="fql_moe_fwd_f32 above the limit")
    del out
    p.out = None
    torch.cuda.empty_cache()
    got = L.moe_forward_any(p.P, p.S, p.Z, p.x.bfloat16(), None, tpe, offs, precision=prec)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (T, N)
    x16refs = [p.x[lo:hi].bfloat16().double() @ p.W[e].T for e, (lo, hi) in enumerate(groups)]
    check_rows(got, groups, x16refs, FMA_REL_FRO + 2.0 ** -9, "moe_forward_any fallback")
    del got, p


# ======================================================================= INT4 per-row grouped forward: a large gather SOURCE
@pytest.mark.parametrize("prec", ["exact", "int8"])
def test_int4_gather_forward_large_input(lib, prec):
    """``ops.moe_gather_forward`` on tokens [n_src, 32] float32 past 2^32 bytes: ``row_index`` names source rows at the four
    places (128 bytes a row divide both boundaries: the groups lie on both sides of each), plain and with a row weight."""
    need(9)
    K, N, E = 32, 136, 4
    n_src = B32 // (K * 4) + 4096
    assert n_src * K * 4 > B32 and n_src * K < (1 << 31)
    tb = BigGuarded("tokens", n_src * K * 4, torch.float32, NAN)
    tokens = tb.view(n_src, K)
    g = torch.Generator(device=DEV).manual_seed(61)
    step = 1 << 22
    for a in range(0, n_src, step):
        b = min(a + step, n_src)
        tokens[a:b] = torch.randn(b - a, K, generator=g, device=DEV)
    r31, r32 = B31 // (K * 4), B32 // (K * 4)
    src = [(0, 33), (r31 - 35, r31 + 35), (r32 - 35, r32 + 35), (n_src - 35, n_src - 2)]
    for lo, hi in src[1:]:
        assert input_wrap_is_visible(tb, (hi - 1) * K * 4, K) >= 1
    groups, pos = [], 0
    for lo, hi in src:
        groups.append((pos, pos + hi - lo))
        pos += hi - lo
    T = pos + 3                                                              # three rows no expert covers
    row_index = torch.cat([torch.arange(lo, hi) for lo, hi in src] + [torch.zeros(3, dtype=torch.long)]).to(torch.int32).to(DEV)
    tpe, offs = table_of(groups)
    P, S, Z = int4_weights(E, N, K, 6)
    assert lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], ctypes.c_void_p(P.data_ptr()), 1) == 1
    refs = [tokens[lo:hi].double() @ dequant_f64(P[e], S[e], Z[e]).T for e, (lo, hi) in enumerate(src)]
    out = ops().moe_gather_forward(P, S, Z, tokens, row_index, tpe, offs, precision=prec)
    check_rows(out, groups, refs, tol_of(prec, K), f"gather {prec}")
    rw = 0.5 + torch.rand(T, generator=g, device=DEV)
    out = ops().moe_gather_forward(P, S, Z, tokens, row_index, tpe, offs, precision=prec, row_weight=rw)
    check_rows(out, groups, [r * rw[lo:hi, None].double() for r, (lo, hi) in zip(refs, groups)], tol_of(prec, K),
               f"gather {prec} with a row weight")
    assert_guards_intact(tb, what="gather source")
    del tokens, tb


# ======================================================================= INT4 per-row grouped forward: large WEIGHTS
def largest_experts(lib, prec, T, K, N):
    """The largest E the matrix-core path takes for T rows: every expert pads the limb buffer by one 32-row block, so the
    limb limit of ``mfma_addressable`` bounds E as well (3 limbs, K = 256: about 43600), below the 65535 of the grid."""
    ok = lambda E: lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], P16, 1) == 1
    lo, hi = 1, 65535
    if ok(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert lib.fql_act_limb_bytes(T, lo, K, PREC[prec]) < B31 <= lib.fql_act_limb_bytes(T, lo + 1, K, PREC[prec])
    return lo


@pytest.mark.parametrize("form", ["plain", "bias", "gated"])
@pytest.mark.parametrize("prec,K,N", [("int8", 512, 264), ("fast", 256, 776), ("exact", 256, 776)])
def test_int4_forward_large_weights(lib, prec, K, N, form):
    """E * N * K/2 > 2^32 with N * K/2 no power of two (67584 / 99328 bytes): rows go to expert 0, the expert whose
    weights straddle 2^31, the one that straddles 2^32 and E - 1; every other expert holds 0xFF codes and NaN scales.
    E is the library's own limit for the precision, or 64 experts past 2^32 bytes where that is fewer.  ``gated``: the
    same weights as the down projection of ``ops.moe_gated_forward`` (gate | up rows, the activation fused into the
    pre-pass) against the float64 h of tests/glu_reference.py."""
    from glu_reference import device_hidden, hidden64
    need(9)
    bias, gated = form == "bias", form == "gated"
    groups = [(0, 33), (40, 110), (113, 183), (190, 223)]
    T = 225
    wb = N * K // 2
    Emax = largest_experts(lib, prec, T, K, N)
    E = min(Emax, B32 // wb + 64)
    assert E * wb > B32 and B31 % wb and B32 % wb, (Emax, E)
    experts = [0, B31 // wb, B32 // wb, E - 1]
    assert experts[1] * wb < B31 < (experts[1] + 1) * wb and experts[2] * wb < B32 < (experts[2] + 1) * wb < (E - 1) * wb
    buf = BigGuarded("packed", E * wb, torch.uint8, 0xFF)
    P = buf.view(E, N, K // 2)
    P.fill_(0xFF)
    S = torch.full((E, N), NAN, device=DEV)
    Z = torch.full((E, N), NAN, device=DEV)
    B = torch.full((E, N), NAN, device=DEV) if bias else None
    g = torch.Generator(device=DEV).manual_seed(3)
    for e in experts:
        P[e] = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8)
        S[e] = 0.001 + 0.002 * torch.rand(N, generator=g, device=DEV)
        Z[e] = torch.randint(5, 11, (N,), generator=g, device=DEV).float()
        if bias:
            B[e] = torch.randn(N, generator=g, device=DEV)
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    x = torch.randn(T, 2 * K if gated else K, generator=g, device=DEV)
    xd = hidden64("silu", x) if gated else x.double()
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= 3   # each expert's last row
    refs = [xd[lo:hi] @ dequant_f64(P[e], S[e], Z[e]).T + (B[e].double() if bias else 0.0)
            for e, (lo, hi) in zip(experts, groups)]
    assert lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], ctypes.c_void_p(buf.ptr), 1) == 1
    chosen = lib.fql_tune_chosen_cfg(PREC[prec], E, T, K, N, 1)
    assert 200 <= chosen < 300, chosen                      # one row per expert on average: a 16-row decode tile
    out = torch.full((T, N), SENT, device=DEV)
    if gated:
        ops()._launch("fql_moe_gated_fwd", out.device, P, S, Z, x, 0, tpe, offs, out, 0, E, T, K, N, PREC[prec],
                      ws_bytes=lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]))
    else:
        name = "fql_moe_bias_fwd" if bias else "fql_moe_fwd"
        args = (P, S, Z, x, 0, tpe, offs) + ((B,) if bias else ()) + (out, 0, E, T, K, N, PREC[prec])
        ops()._launch(name, out.device, *args, ws_bytes=lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    if gated:
        # the gated family's own check (tests/test_gpu_glu.py): the bits of the plain entry on the device's float32 h
        h = device_hidden(ops(), x, "silu")
        want = torch.full((T, N), SENT, device=DEV)
        ops()._launch("fql_moe_fwd", out.device, P, S, Z, h, 0, tpe, offs, want, 0, E, T, K, N, PREC[prec],
                      ws_bytes=lib.fql_moe_workspace_bytes(E, T, K, N, PREC[prec]))
        assert same_bits(out, want), "gated: not the bits of the plain entry on the same h"
    if gated and prec == "int8":
        # (h = silu(g) u is heavy-tailed: the 8-bit bound of helpers.py is stated for rows without outliers and is held by
        #  the plain case on these weights; here the bit identity above carries it)
        assert int(torch.count_nonzero(out)) == sum(int(torch.count_nonzero(out[lo:hi])) for lo, hi in groups)
    else:
        check_rows(out, groups, refs, fro_tol(LIMBS[prec], K), f"large weights {prec} E={E} cfg {chosen}")
    # the input gradient on the same weights: it has no fallback, its limbs run along N (padded to 256) and every expert
    # pads them by a row block, so only the one-limb mode takes this many experts; the others refuse (workspace query 0)
    bwd_ws = lib.fql_moe_bwd_workspace_bytes(E, T, K, N, PREC[prec])
    assert (bwd_ws > 0) == (prec == "int8"), (prec, bwd_ws)
    if prec == "int8" and form == "plain":
        gy = torch.randn(T, N, generator=g, device=DEV)
        gx = ops().moe_backward_input(P, S, Z, gy, tpe, offs, precision=prec)
        grefs = [gy[lo:hi].double() @ dequant_f64(P[e], S[e], Z[e]) for e, (lo, hi) in zip(experts, groups)]
        assert bool(torch.isfinite(gx).all())
        check_rows(gx, groups, grefs, fro_tol(LIMBS[prec], N), f"large weights {prec} E={E} input gradient")
    elif form == "plain":
        with pytest.raises(RuntimeError, match="bad shape"):
            ops().moe_backward_input(P, S, Z, torch.zeros(T, N, device=DEV), tpe, offs, precision=prec)
    assert_guards_intact(buf, what="large INT4 weights")
    del P, buf


def test_int4_largest_single_expert(lib):
    """One expert at the column limit of ``mfma_addressable``: the largest N with (N + 256) * K/2 < 2^31 at K = 4096
    (2 GiB of packed weights less the margin), 64 rows, every tile configuration built for 3 limbs, through the linear
    and the grouped entry.  The last 320 columns, the first 320 and 64 random 32-column blocks against float64, every
    output finite.  Then N + 1: the float32 entries fall back to the generic kernel and stay right, the others refuse."""
    need(8)
    K, T, prec = 4096, 64, "exact"
    N = (B31 - 1) // (K // 2) - 256
    ok = lambda n, grouped: lib.fql_native_dtype_supported(T, 1, K, n, PREC[prec], P16, grouped)
    assert ok(N, 0) == ok(N, 1) == 1 and ok(N + 1, 0) == ok(N + 1, 1) == 0
    assert (N + 256) * (K // 2) < B31 <= (N + 257) * (K // 2)
    buf = BigGuarded("packed", (N + 1) * (K // 2), torch.uint8, 0xFF)
    P1 = buf.view(N + 1, K // 2)
    g = torch.Generator(device=DEV).manual_seed(9)
    step = 1 << 16
    for a in range(0, N + 1, step):
        b = min(a + step, N + 1)
        P1[a:b] = torch.randint(0, 256, (b - a, K // 2), generator=g, device=DEV, dtype=torch.uint8)
    S1 = 0.001 + 0.002 * torch.rand(N + 1, generator=g, device=DEV)
    Z1 = torch.randint(5, 11, (N + 1,), generator=g, device=DEV).float()
    x = torch.randn(T, K, generator=g, device=DEV)
    cols = torch.cat([torch.arange(0, 320), torch.arange(N - 320, N)] +
                     [torch.arange(32 * b, 32 * b + 32) for b in torch.randint(10, (N - 320) // 32, (64,), generator=torch.Generator().manual_seed(1)).tolist()]).to(DEV)
    ref = x.double() @ dequant_f64(P1[cols], S1[cols], Z1[cols]).T
    tpe, offs = table_of([(0, T)])
    L = ops()

    def check(out, what, bound=EXACT_REL_FRO):
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), what
        err = rel_fro_dev(out[:, cols], ref)
        print(f"largest expert N={out.shape[1]} {what}: rel_fro {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (what, err)

    P, S, Z = P1[:N], S1[:N], Z1[:N]
    out = torch.full((T, N), SENT, device=DEV)
    L._launch("fql_linear_fwd_f32", out.device, x, P, S, Z, out, T, K, N, PREC[prec],
              ws_bytes=lib.fql_linear_workspace_bytes(T, K, N, PREC[prec]))
    check(out, f"linear entry cfg {lib.fql_tune_chosen_cfg(PREC[prec], 1, T, K, N, 0)}")
    out.fill_(SENT)
    L._launch("fql_moe_fwd_f32", out.device, P.view(1, N, K // 2), S, Z, x, tpe, offs, out, 1, T, K, N, PREC[prec],
              ws_bytes=lib.fql_moe_workspace_bytes(1, T, K, N, PREC[prec]))
    check(out, f"grouped entry cfg {lib.fql_tune_chosen_cfg(PREC[prec], 1, T, K, N, 1)}")
    limbs, delta, rowsum = L.act_quant(x, prec, tpe, offs)
    ran = []
    for cfg in [c for c in range(0, 310) if lib.fql_tune_is_config(c, PREC[prec]) == 1]:
        out.fill_(SENT)
        assert L.tune_gemm_i8(cfg, limbs, delta, rowsum, P, S, Z, tpe, offs, out, 1, T, K, N, prec) == OK, cfg
        check(out, f"cfg {cfg}")
        ran.append(cfg)
    print("largest expert: pinned ids", ran)
    assert any(c < 100 for c in ran) and any(100 <= c < 200 for c in ran) and any(200 <= c < 300 for c in ran) and 300 in ran
    assert_guards_intact(buf, what="largest expert")
    del out

    # ---- one column more
    N2 = N + 1
    P, S, Z = P1, S1, Z1
    out = torch.full((T, N2), SENT, device=DEV)
    assert L.tune_gemm_i8(0, limbs, delta, rowsum, P, S, Z, tpe, offs, out, 1, T, K, N2, prec) == SHAPE
    ws = torch.empty(lib.fql_moe_workspace_bytes(1, T, K, N2, PREC[prec]) + 16, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    x16 = x.bfloat16()
    ptr = lambda t: t.data_ptr()
    assert lib.fql_linear_fwd(ptr(x16), 2, ptr(P), ptr(S), ptr(Z), ptr(out), 2, T, K, N2, PREC[prec], ptr(ws), ws.numel(), st) == DTYPE
    assert lib.fql_moe_fwd(ptr(P), ptr(S), ptr(Z), ptr(x16), 2, ptr(tpe), ptr(offs), ptr(out), 2, 1, T, K, N2, PREC[prec],
                           ptr(ws), ws.numel(), st) == DTYPE
    assert lib.fql_moe_fwd_f32(ptr(P), ptr(S), ptr(Z), ptr(x), ptr(tpe), ptr(offs), ptr(out), 1, T, K, N2, 8, ptr(ws), ws.numel(),
                               st) == ALIGN
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote to its output"
    cols2 = torch.cat([cols, torch.tensor([N], device=DEV)])
    ref2 = x.double() @ dequant_f64(P1[cols2], S1[cols2], Z1[cols2]).T
    for name, args in (("fql_linear_fwd_f32", (x, P, S, Z, out, T, K, N2, PREC[prec])),
                       ("fql_moe_fwd_f32", (P.view(1, N2, K // 2), S, Z, x, tpe, offs, out, 1, T, K, N2, PREC[prec]))):
        out.fill_(SENT)
        L._launch(name, out.device, *args, ws_bytes=ws.numel() - 16)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), name
        err = rel_fro_dev(out[:, cols2], ref2)
        print(f"largest expert N={N2} {name} (generic): rel_fro {err:.3e} (bound {FMA_REL_FRO:.1e})")
        assert err <= FMA_REL_FRO, (name, err)
    assert_guards_intact(buf, what="largest expert + 1")
    del out, P, P1, buf


# ======================================================================= MXFP4 experts: large WEIGHTS
@pytest.mark.parametrize("kernel", ["tile", "decode"])
def test_mxfp4_forward_large_weights(lib, kernel):
    """E * N * K/2 > 2^32 of MXFP4 blocks (N * K/2 = 67584 bytes), rows to expert 0, the two straddling experts and E - 1;
    every other expert holds 0xFF codes and scale bytes (NaN).  The exact recipe of tests/test_gpu_mxfp4.py: integer
    activations in [-4, 4], scale codes 125..129, so the float32 result IS the float64 reference.  Both bfloat16
    kernels: the 64-row tile (decode threshold set to 0) and the decode kernel (T <= 512)."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    need(9)
    K, N, E = 512, 264, 65534
    wb = N * K // 2
    assert E * wb > B32 and B31 % wb and B32 % wb
    experts = [0, B31 // wb, B32 // wb, E - 1]
    buf = BigGuarded("blocks", E * wb, torch.uint8, 0xFF)
    blocks = buf.view(E, N, K // 2)
    blocks.fill_(0xFF)
    scales = torch.full((E, N, K // 32), 0xFF, dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(4)
    for e in experts:
        blocks[e] = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8)
        scales[e] = torch.randint(125, 130, (N, K // 32), generator=g, device=DEV, dtype=torch.uint8)
    groups = [(0, 33), (40, 110), (113, 183), (190, 223)]
    T = 225
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    x = torch.randint(-4, 5, (T, K), generator=g, device=DEV).float()
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= 3   # each expert's last row
    Ws = [dequantize_mxfp4(blocks[e:e + 1].cpu(), scales[e:e + 1].cpu())[0].double().to(DEV) for e in experts]
    refs = [x[lo:hi].double() @ W.T for W, (lo, hi) in zip(Ws, groups)]
    assert all(float(r.abs().max()) < 2 ** 15 for r in refs)
    old = lib.fql_tune_set_mx4_decode_max_rows(-1)          # (a negative value changes nothing)
    lib.fql_tune_set_mx4_decode_max_rows(0 if kernel == "tile" else 512)
    try:
        reported = lib.fql_tune_mx4_kernel(E, T, K, N)
        got = ops().moe_forward_mxfp4(blocks, scales, x, tpe, offs, out_dtype=torch.float32)
        torch.cuda.synchronize()
    finally:
        lib.fql_tune_set_mx4_decode_max_rows(old)
    assert reported == MX4_KERNEL[kernel], (kernel, reported)
    check_rows(got, groups, refs, 0.0, f"mxfp4 {kernel}", exact=True)
    if kernel == "tile":                                    # the input gradient on the same blocks (one kernel), as exact
        gy = torch.randint(-4, 5, (T, N), generator=g, device=DEV).float()
        grefs = [gy[lo:hi].double() @ W for W, (lo, hi) in zip(Ws, groups)]
        assert all(float(r.abs().max()) < 2 ** 15 for r in grefs)
        gx = ops().moe_backward_input_mxfp4(blocks, scales, gy, tpe, offs)
        check_rows(gx, groups, grefs, 0.0, "mxfp4 input gradient", exact=True)
    assert_guards_intact(buf, what="large MXFP4 weights")
    del blocks, buf


# ======================================================================= swiglu / glu backward: every row live
@pytest.mark.parametrize("kind", ["silu", "gelu_tanh", "swiglu_clamp"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_glu_backward_large(kind, dtype):
    """2 * T * F just above 2^30 elements: gate_up and the result cross 2^32 bytes in float32, 2^31 in bfloat16.  Every
    row is live, so the rows of the four groups and a strided sample are compared (a) bit for bit with the same op on a
    compact copy of those rows and (b) with the float64 reference of tests/glu_reference.py at the bound of
    tests/test_gpu_glu.py (EXACT_REL_FRO; bfloat16: bit for bit the float32 op on the widened rows, rounded once)."""
    from glu_reference import backward64
    need(20)
    F = 1032
    T = (1 << 30) // (2 * F) + 128                       # (room for the group around the boundary and the last one)
    esz = 4 if dtype == torch.float32 else 2
    assert (1 << 30) < 2 * T * F < (1 << 31) and 2 * T * F * esz > (B32 if esz == 4 else B31)
    L = ops()
    dev = torch.device(DEV, 0)
    one = torch.empty(4, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match="bad shape"):                     # 2^31 elements and more: refused
        L._launch("fql_swiglu_bwd", dev, one, DT[dtype], one, DT[dtype], one, DT[dtype], (1 << 30) // F + 1, F)
    gu_b = BigGuarded("gate_up", 2 * T * F * esz, dtype, NAN)
    dh_b = BigGuarded("dh", T * F * esz, dtype, NAN, front=B31 if T * F * esz > B31 else 1 << 20)
    out_b = BigGuarded("dgate_up", 2 * T * F * esz, dtype, SENT)
    gu, dh, got = gu_b.view(T, 2 * F), dh_b.view(T, F), out_b.view(T, 2 * F)
    g = torch.Generator(device=DEV).manual_seed(11)
    step = 1 << 16
    for a in range(0, T, step):
        b = min(a + step, T)
        gu[a:b] = (3.0 * torch.randn(b - a, 2 * F, generator=g, device=DEV)).to(dtype)
        dh[a:b] = torch.randn(b - a, F, generator=g, device=DEV).to(dtype)
    got.fill_(SENT)
    groups = row_groups(T, 2 * F * esz)
    assert len(groups) == (4 if esz == 4 else 3)
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(gu_b, (hi - 1) * 2 * F * esz, 2 * F) >= 1
    # (a wrapped store leaves its own row at SENT and breaks the front guard or another row: the comparison below sees it)
    act = L.activation_of(kind)
    if kind == "silu":
        L._launch("fql_swiglu_bwd", dev, gu, DT[dtype], dh, DT[dtype], got, DT[dtype], T, F)
    else:
        L._launch("fql_glu_bwd", dev, gu, DT[dtype], dh, DT[dtype], got, DT[dtype], T, F, L._ACTIVATIONS[kind], act[1], act[2])
    torch.cuda.synchronize()
    rows = torch.cat([torch.arange(lo, hi) for lo, hi in groups] + [torch.arange(17, T, 4099)]).to(DEV)
    gur, dhr = gu[rows].contiguous(), dh[rows].contiguous()
    kw = dict(activation=kind)
    compact = L.glu_backward(gur, dhr, **kw)
    assert same_bits(got[rows].contiguous(), compact), "a row of the large call differs from the same row computed alone"
    wide = compact if esz == 4 else L.glu_backward(gur.float(), dhr.float(), **kw)
    if esz == 2:
        assert same_bits(compact, wide.to(dtype))
    dg, du, *_ = backward64(kind, gur.float(), dhr.float())
    err = rel_fro_dev(wide, torch.cat([dg, du], dim=1))
    print(f"glu_backward {kind} {dtype} T={T} F={F}: rel_fro {err:.3e} (bound {EXACT_REL_FRO:.1e})")
    assert err < EXACT_REL_FRO
    assert bool(torch.isfinite(got[rows]).all())
    assert_guards_intact(gu_b, dh_b, out_b, what="glu_backward")
    del got, gu, dh, gu_b, dh_b, out_b


# ======================================================================= combine, its backward, bias gradient
def far_rows(R, row_bytes, n):
    """``n`` row indices of a [R, N] operand: spread over the four row groups."""
    groups = row_groups(R, row_bytes)
    assert len(groups) in (3, 4)
    rows = torch.cat([torch.arange(lo, hi) for lo, hi in groups])
    pick = rows[torch.linspace(0, rows.numel() - 1, n).long()]
    assert pick.unique().numel() == n and int(pick[0]) == 0 and int(pick[-1]) == R - 3     # (every slot its own row)
    return groups, pick


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_combine_large_rows(dtype):
    """y [R, N] past 2^32 bytes; ``pos_of_slot`` points at the four places, dropped slots (-1) go nowhere
    (``skip_dropped``).  ``combine_any`` against float64 (the float32 sum of top_k products: FMA_REL_FRO, plus one
    rounding for a 16-bit result), ``ops.combine_any_backward``: the rows of grad_y that a slot names, exactly
    w * grad_out rounded once; every other row of grad_y zero."""
    need(20)
    esz = 4 if dtype == torch.float32 else 2
    N = 1032
    top = B32 if esz == 4 else B31                       # (fewer than 2^31 elements of 2 bytes end below 2^32 bytes)
    R = top // (N * esz) + 4096
    assert R * N < (1 << 31) and R * N * esz > top
    T, top_k = 32, 4                                     # 128 slots on the 136 / 206 rows of the groups
    yb = BigGuarded("y", R * N * esz, dtype, NAN)
    y = yb.view(R, N)
    groups, rows = far_rows(R, N * esz, T * top_k)
    g = torch.Generator(device=DEV).manual_seed(21)
    y.fill_(NAN)
    for lo, hi in groups:
        y[lo:hi] = torch.randn(hi - lo, N, generator=g, device=DEV).to(dtype)
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(yb, (hi - 1) * N * esz, N) >= 1
    pos = rows.to(torch.int32).to(DEV).reshape(T, top_k).clone()
    pos[::7, 1] = -1                                                         # dropped slots
    w = torch.rand(T, top_k, generator=g, device=DEV) + 0.5
    L = ops()
    out = L.combine_any(y, pos.flatten(), w, skip_dropped=True)
    keep = (pos >= 0)
    ref = torch.zeros(T, N, device=DEV)                                      # the kernel's own float32 order: exact
    for k in range(top_k):
        term = y[pos[:, k].clamp(min=0).long()].float() * w[:, k:k + 1]
        ref = torch.where(keep[:, k:k + 1], ref + term, ref)
    assert out.dtype == dtype and bool(torch.isfinite(out).all())
    assert same_bits(out, ref.to(dtype)), "combine_any: not the float32 sum of the rows pos_of_slot names"

    gout = torch.randn(T, N, generator=g, device=DEV).to(dtype)
    gy, gw, _, _ = L.combine_any_backward(gout, y, pos.flatten(), w, skip_dropped=True)
    torch.cuda.synchronize()
    assert gy.dtype == dtype and tuple(gy.shape) == (R, N) and tuple(gw.shape) == (T, top_k)
    nz = 0
    for t in range(T):
        for k in range(top_k):
            p = int(pos[t, k])
            if p < 0:
                assert float(gw[t, k]) == 0.0
                continue
            want = (gout[t].float() * w[t, k]).to(dtype)
            assert same_bits(gy[p], want), (t, k, p)
            nz += int(torch.count_nonzero(gy[p]))
    assert int(torch.count_nonzero(gy)) == nz, "combine backward wrote a row of grad_y no slot names"
    # grad_weights: a float32 dot product of N terms, |err| <= N 2^-24 sum |y g| whatever the order
    prod = [y[pos[:, k].clamp(min=0).long()].double() * gout.double() for k in range(top_k)]
    gwref = torch.stack([prod[k].sum(1) * keep[:, k] for k in range(top_k)], 1)
    gwmag = torch.stack([prod[k].abs().sum(1) for k in range(top_k)], 1)
    assert bool(((gw.double() - gwref).abs() <= N * 2.0 ** -24 * gwmag).all())
    assert_guards_intact(yb, what="combine")
    del y, gy, yb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_moe_bias_grad_large_rows(dtype):
    """grad_rows [T, N] past 2^32 bytes, the four row groups as four experts: the column sums of each group against
    float64 at the bound of tests/test_gpu_moe_bias.py's float32 sums (1e-5 of the column-sum norm)."""
    need(10)
    esz = 4 if dtype == torch.float32 else 2
    N = 1032
    top = B32 if esz == 4 else B31                       # (fewer than 2^31 elements of 2 bytes end below 2^32 bytes)
    T = top // (N * esz) + 4096
    assert T * N < (1 << 31) and T * N * esz > top
    gb = BigGuarded("grad_rows", T * N * esz, dtype, NAN)
    gr = gb.view(T, N)
    groups = row_groups(T, N * esz)
    g = torch.Generator(device=DEV).manual_seed(31)
    for lo, hi in groups:
        gr[lo:hi] = torch.randn(hi - lo, N, generator=g, device=DEV).to(dtype)
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(gb, (hi - 1) * N * esz, N) >= 1
    tpe, offs = table_of(groups)
    got = ops().moe_bias_grad(gr, len(groups), tpe, offs)
    ref = torch.stack([gr[lo:hi].double().sum(0) for lo, hi in groups])
    mag = torch.stack([gr[lo:hi].double().abs().sum(0) for lo, hi in groups])
    cnt = torch.tensor([hi - lo for lo, hi in groups], dtype=torch.float64, device=DEV).reshape(-1, 1)
    err = (got.double() - ref).abs()
    bound = cnt * 2.0 ** -24 * mag                                           # (tests/test_gpu_moe_bias.py)
    print(f"moe_bias_grad {dtype} T={T} N={N}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    assert_guards_intact(gb, what="moe_bias_grad")
    del gr, gb


# ======================================================================= router
@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_router_large_logits(scoring):
    """logits [T, 128] float32 past 2^32 bytes: the four row groups against torch (the reference of
    tests/test_gpu_router.py: softmax / sigmoid in float64, top-k on the logits, renormalised), every index in range, and
    the backward at the same rows against autograd."""
    need(16)
    E, top_k = 128, 4
    T = B32 // (E * 4) + 4096
    assert T * E * 4 > B32
    lb = BigGuarded("logits", T * E * 4, torch.float32, NAN)
    logits = lb.view(T, E)
    g = torch.Generator(device=DEV).manual_seed(41)
    step = 1 << 20
    for a in range(0, T, step):
        b = min(a + step, T)
        logits[a:b] = torch.randn(b - a, E, generator=g, device=DEV)
    # 512 bytes a row divide both boundaries: no row straddles, the groups sit on both sides of each boundary
    r31, r32 = B31 // (E * 4), B32 // (E * 4)
    groups = [(0, 33), (r31 - 35, r31 + 35), (r32 - 35, r32 + 35), (T - 35, T - 2)]
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(lb, (hi - 1) * E * 4, E) >= 1
    L = ops()
    code = {"softmax": 0, "sigmoid": 1}[scoring]
    sb = BigGuarded("scores", T * E * 4, torch.float32, SENT)
    scores = sb.view(T, E)
    scores.fill_(SENT)
    idx = torch.full((T, top_k), -1, dtype=torch.int32, device=DEV)
    wts = torch.full((T, top_k), SENT, device=DEV)
    L._launch("fql_router_score_topk_fwd", logits.device, logits, 0, T, E, top_k, code, None, 1, 1, 1, 1, 1.0, idx, wts, scores)
    torch.cuda.synchronize()
    assert int(idx.min()) >= 0 and int(idx.max()) < E
    rows = torch.cat([torch.arange(lo, hi) for lo, hi in groups]).to(DEV)
    ld = logits[rows].double().requires_grad_(True)
    sc = torch.softmax(ld, 1) if scoring == "softmax" else torch.sigmoid(ld)
    ti = torch.topk(ld, top_k, dim=1).indices
    assert torch.equal(idx[rows].long().sort(1).values, ti.sort(1).values)
    sel = sc.gather(1, idx[rows].long())
    wref = sel / sel.sum(1, keepdim=True)
    # the bounds of tests/test_gpu_router.py / test_gpu_router_score.py (scale = 1)
    inside = lambda got, ref: bool(((got.double() - ref).abs() <= 4e-6 * ref.abs() + 2.0 ** -148).all())
    assert inside(wts[rows], wref.detach()) and inside(scores[rows], sc.detach())
    gw = torch.randn(T, top_k, generator=g, device=DEV)
    assert_guards_intact(lb, sb, what="router forward")
    del scores, sb
    torch.cuda.empty_cache()
    glb = BigGuarded("grad_logits", T * E * 4, torch.float32, SENT)
    gl = glb.view(T, E)
    L._launch("fql_router_score_topk_bwd", logits.device, logits, 0, idx, gw, None, gl, T, E, top_k, code, 1, 1.0)
    torch.cuda.synchronize()
    (wref * gw[rows].double()).sum().backward()
    err = (gl[rows].double() - ld.grad).abs().amax(1)
    bound = 4e-5 * gw[rows].abs().amax(1).double()
    print(f"router {scoring} T={T}: backward max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and bool(torch.isfinite(gl[rows]).all())
    assert_guards_intact(lb, glb, what="router")
    del logits, lb, gl, glb


# ======================================================================= LoRA shrink and expand
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_lora_shrink_expand_large_rows(dtype):
    """T * C below 2^31 elements; float32 rows past 2^32 bytes, bfloat16 rows past 2^31.  The four row groups as four
    experts through the table: shrink against float64 at ADAPTER_TOL (16-bit rows: F32_TOL), expand with ``input=`` and
    ``out=``: covered rows input + scale * v W^T, every other row the input itself, bit for bit."""
    need(22)
    esz = 4 if dtype == torch.float32 else 2
    C, r, E = 1032, 8, 4
    T = (B32 if esz == 4 else B31) // (C * esz) + 4096
    assert T * C < (1 << 31) and T * C * esz > (B32 if esz == 4 else B31)
    xb = BigGuarded("input", T * C * esz, dtype, NAN)
    x = xb.view(T, C)
    groups = row_groups(T, C * esz)
    assert len(groups) == (4 if esz == 4 else 3)
    E = len(groups)
    g = torch.Generator(device=DEV).manual_seed(51)
    step = 1 << 18
    for a in range(0, T, step):
        b = min(a + step, T)
        x[a:b] = torch.randn(b - a, C, generator=g, device=DEV).to(dtype)
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(xb, (hi - 1) * C * esz, C) >= 1
    tpe, offs = table_of(groups)
    A = torch.randn(E, r, C, generator=g, device=DEV) / 32
    Bw = torch.randn(E, C, r, generator=g, device=DEV)
    L = ops()
    v = L.lora_shrink(x, A, "rc", tpe, offs, scale=0.5)
    refs = [0.5 * x[lo:hi].double() @ A[e].double().T for e, (lo, hi) in enumerate(groups)]
    check_rows(v, groups, refs, ADAPTER_TOL if esz == 4 else F32_TOL, f"lora_shrink {dtype}")

    ob = BigGuarded("out", T * C * esz, dtype, SENT)
    out = ob.view(T, C)
    out.fill_(SENT)
    L.lora_expand(v, Bw, "cr", tpe, offs, scale=2.0, input=x, out=out)
    torch.cuda.synchronize()
    covered = torch.zeros(T, dtype=torch.bool, device=DEV)
    for e, (lo, hi) in enumerate(groups):
        covered[lo:hi] = True
        ref = x[lo:hi].double() + 2.0 * v[lo:hi].double() @ Bw[e].double().T
        err = rel_fro_dev(out[lo:hi], ref)
        print(f"lora_expand {dtype} rows [{lo}, {hi}): rel_fro {err:.3e}")
        assert err <= (ADAPTER_TOL if esz == 4 else F32_TOL + 2.0 ** -8)    # (tests/test_gpu_lora_paths.py, test_gpu_lora16.py)
    idt = torch.int32 if esz == 4 else torch.int16
    step = 1 << 18
    for a in range(0, T, step):                                              # every other row: the input, bit for bit
        b = min(a + step, T)
        same = (out[a:b].view(idt) == x[a:b].view(idt)).all(1) | covered[a:b]
        assert bool(same.all()), f"lora_expand: an uncovered row in [{a}, {b}) is not the input"
    assert_guards_intact(xb, ob, what="lora")
    del out, ob
    torch.cuda.empty_cache()

    # ---- lora_grad on the same rows (p = x, v from the shrink), then the gated forms: x read as gate | up rows [T, 2 * C/2]
    tol = ADAPTER_TOL if esz == 4 else F32_TOL
    for layout in ("rc", "cr"):
        d = L.lora_grad(x, v, layout, E, tpe, offs, scale=0.25)
        ref = torch.stack([0.25 * (v[lo:hi].double().T @ x[lo:hi].double()) for lo, hi in groups])       # [E, r, C]
        err = rel_fro_dev(d, ref if layout == "rc" else ref.transpose(1, 2))
        print(f"lora_grad {layout} {dtype}: rel_fro {err:.3e} (bound {tol:.1e})")
        assert err <= tol and bool(torch.isfinite(d).all())
    from glu_reference import hidden64
    C2 = C // 2
    A2 = torch.randn(E, r, C2, generator=g, device=DEV) / 32
    for kind in ("silu", "swiglu_clamp"):
        hs = [hidden64(kind, x[lo:hi].float()) for lo, hi in groups]
        v2 = L.lora_gated_shrink(x, A2, "rc", tpe, offs, scale=0.5, activation=kind)
        check_rows(v2, groups, [0.5 * h @ A2[e].double().T for e, h in enumerate(hs)], tol, f"lora_gated_shrink {kind} {dtype}")
        d2 = L.lora_gated_grad(x, v2, "rc", E, tpe, offs, scale=0.25, activation=kind)
        ref2 = torch.stack([0.25 * (v2[lo:hi].double().T @ h) for (lo, hi), h in zip(groups, hs)])
        err = rel_fro_dev(d2, ref2)
        print(f"lora_gated_grad {kind} {dtype}: rel_fro {err:.3e} (bound {tol:.1e})")
        assert err <= tol and bool(torch.isfinite(d2).all())
    assert_guards_intact(xb, what="lora grad and gated forms")
    del x, xb


# ======================================================================= dispatch_rows: forward and backward
def test_dispatch_rows_large():
    """``ops.dispatch_rows`` on x [65535, 16648] float32 (the combine behind its backward takes at most 65535 tokens a
    call, so the width carries x past 2^32 bytes), top_k = 1, a random permutation as the plan: the rows are x's rows bit
    for bit, and x.grad is the gradient's rows back in token order bit for bit (a pure gather-add of one term)."""
    need(23)
    T, H = 65535, 16648
    assert T * H < (1 << 31) and T * H * 4 > B32
    xb = BigGuarded("x", T * H * 4, torch.float32, NAN)
    gb = BigGuarded("grad_rows", T * H * 4, torch.float32, NAN)
    x, grad = xb.view(T, H), gb.view(T, H)
    g = torch.Generator(device=DEV).manual_seed(71)
    step = 4096
    for a in range(0, T, step):
        b = min(a + step, T)
        x[a:b] = torch.randn(b - a, H, generator=g, device=DEV)
        grad[a:b] = torch.randn(b - a, H, generator=g, device=DEV)
    for t in (B31 // (H * 4) + 1, B32 // (H * 4) + 1, T - 1):
        assert input_wrap_is_visible(gb, t * H * 4, H) >= 1
    token_of_sorted = torch.randperm(T, generator=g, device=DEV).to(torch.int32)     # sorted position -> token
    pos_of_slot = torch.empty(T, dtype=torch.int32, device=DEV)                      # token -> sorted position
    pos_of_slot[token_of_sorted.long()] = torch.arange(T, dtype=torch.int32, device=DEV)
    xr = x.requires_grad_(True)
    rows = ops().dispatch_rows(xr, token_of_sorted, pos_of_slot, 1)
    rows.backward(grad)
    torch.cuda.synchronize()
    gx = xr.grad
    assert gx.dtype == torch.float32 and tuple(gx.shape) == (T, H)
    for a in range(0, T, step):
        b = min(a + step, T)
        assert torch.equal(rows[a:b].detach(), x.detach()[token_of_sorted[a:b].long()]), f"dispatch_rows: rows [{a}, {b})"
        assert same_bits(gx[a:b], grad[pos_of_slot[a:b].long()]), f"dispatch_rows backward: tokens [{a}, {b})"
    assert_guards_intact(xb, gb, what="dispatch_rows")
    del rows, gx, xr, x, grad, xb, gb


# ======================================================================= [T, K] rows past 2^32 bytes into the pre-passes
ROWS_K = 288                       # 1152 bytes a row: no power of two; Kp = 512; T stays inside the MXFP4 grid (64 x 65535 rows)


def big_rows(seed, width=ROWS_K):
    """x [T, width] float32 just past 2^32 bytes in a guarded buffer, randn in 2^18-row pieces, and the four row groups."""
    T = B32 // (width * 4) + 4096
    assert T * width * 4 > B32 and T * width < (1 << 31) and (T + 63) // 64 <= 65535
    xb = BigGuarded("rows", T * width * 4, torch.float32, NAN)
    x = xb.view(T, width)
    g = torch.Generator(device=DEV).manual_seed(seed)
    step = 1 << 18
    for a in range(0, T, step):
        b = min(a + step, T)
        x[a:b] = torch.randn(b - a, width, generator=g, device=DEV)
    groups = row_groups(T, width * 4)
    assert len(groups) == 4
    for lo, hi in groups[1:]:
        assert input_wrap_is_visible(xb, (hi - 1) * width * 4, width) >= 1
    return xb, x, groups, g


def compact_of(x, groups):
    """The covered rows alone, as one small problem: (rows, groups, table)."""
    small = torch.cat([x[lo:hi] for lo, hi in groups]).contiguous()
    g2, pos = [], 0
    for lo, hi in groups:
        g2.append((pos, pos + hi - lo))
        pos += hi - lo
    return small, g2, table_of(g2)


@pytest.mark.parametrize("prec", ["int8", "fp8"])
def test_int4_rows_past_4_gib(lib, prec):
    """x [T, 288] float32 past 2^32 bytes (the one-plane limb limit allows T = 3.7 M rows at Kp = 512) through the product
    entry with a bfloat16 result, and through ``ops.act_quant`` + the GEMM the library picks (``tune_gemm_i8`` with its
    chosen id)."""
    need(12)
    K, N, E = ROWS_K, 136, 4
    xb, x, groups, g = big_rows(81)
    T = x.shape[0]
    assert lib.fql_native_dtype_supported(T, E, K, N, PREC[prec], P16, 1) == 1
    tpe, offs = table_of(groups)
    P, S, Z = int4_weights(E, N, K, 8)
    refs = [x[lo:hi].double() @ dequant_f64(P[e], S[e], Z[e]).T for e, (lo, hi) in enumerate(groups)]
    bound = tol_of(prec, K) + 2.0 ** -9
    out = ops().moe_forward_any(P, S, Z, x, None, tpe, offs, precision=prec, out_dtype=torch.bfloat16)
    check_rows(out, groups, refs, bound, f"rows past 4 GiB {prec}: product")
    limbs, delta, rowsum = ops().act_quant(x, prec, tpe, offs)
    cfg = lib.fql_tune_chosen_cfg(PREC[prec], E, T, K, N, 1)
    out.zero_()
    assert ops().tune_gemm_i8(cfg, limbs, delta, rowsum, P, S, Z, tpe, offs, out, E, T, K, N, prec, out_dtype=torch.bfloat16) == OK
    torch.cuda.synchronize()
    check_rows(out, groups, refs, bound, f"rows past 4 GiB {prec}: act_quant + cfg {cfg}")
    assert_guards_intact(xb, what="rows into the INT4 pre-pass")
    del x, xb, limbs, out


def test_generic_rows_past_4_gib(lib):
    """The generic float32 kernel (K % 32 != 0: K = 286) on x [T, 286] float32 past 2^32 bytes."""
    need(8)
    K, N, E = 286, 8, 4
    xb, x, groups, g = big_rows(82, K)
    T = x.shape[0]
    assert lib.fql_native_dtype_supported(T, E, K, N, 3, P16, 1) == 0
    tpe, offs = table_of(groups)
    P, S, Z = int4_weights(E, N, K, 9)
    refs = [x[lo:hi].double() @ dequant_f64(P[e], S[e], Z[e]).T for e, (lo, hi) in enumerate(groups)]
    out = ops().moe_forward(P, S, Z, x, None, tpe, offs)
    check_rows(out, groups, refs, FMA_REL_FRO, "rows past 4 GiB: generic kernel")
    assert_guards_intact(xb, what="rows into the generic kernel")
    del x, xb


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_mxfp4_rows_past_4_gib(lib, gated):
    """Rows past 2^32 bytes into the MXFP4 quantiser (``ops.quantize_rows_mxfp4``, every row live) and into the fp8 / fp4
    pre-passes of the MXFP4 GEMM (four row groups).  Each result is bit for bit the same op on a compact copy of the rows
    (the small-shape tests tie that to the reference: tests/test_gpu_mxfp4_f8.py, test_gpu_mxfp4_f4.py), the quantiser also
    bit for bit ``quantize.quantize_mxfp4`` of the float64-free h / rows; rows no expert covers are zero."""
    from fused_int4_amd.quantize import quantize_mxfp4
    need(10)
    width = ROWS_K if not gated else 2 * 160                  # gated: gate | up rows [T, 320], K = 160 (1280 bytes a row)
    K = width // 2 if gated else width
    xb, x, groups, g = big_rows(83 + gated, width)
    T = x.shape[0]
    L = ops()
    kw = dict(activation="swiglu_clamp") if gated else {}
    qb, qs = L.quantize_rows_mxfp4(x, **kw)
    rows = torch.cat([torch.arange(lo, hi) for lo, hi in groups] + [torch.arange(5, T, 40009)]).to(DEV)
    cb, cs = L.quantize_rows_mxfp4(x[rows].contiguous(), **kw)
    assert torch.equal(qb[rows], cb) and torch.equal(qs[rows], cs), "quantize_rows_mxfp4: a row differs from the row alone"
    if not gated:
        rb, rs = quantize_mxfp4(x[rows].cpu())
        assert torch.equal(cb.cpu(), rb) and torch.equal(cs.cpu(), rs)
    del qb, qs
    E, N = 4, 40
    gw = torch.Generator().manual_seed(5)
    blocks = torch.randint(0, 256, (E, N, K // 2), generator=gw, dtype=torch.uint8).to(DEV)
    scales = torch.randint(120, 131, (E, N, K // 32), generator=gw, dtype=torch.uint8).to(DEV)
    tpe, offs = table_of(groups)
    small, g2, (tpe2, offs2) = compact_of(x, groups)
    for prec in ("fp8", "fp4", "bf16"):
        if gated:
            got = L.moe_gated_forward_mxfp4(blocks, scales, x, tpe, offs, precision=prec, out_dtype=torch.float32, **kw)
            want = L.moe_gated_forward_mxfp4(blocks, scales, small, tpe2, offs2, precision=prec, out_dtype=torch.float32, **kw)
        else:
            got = L.moe_forward_mxfp4(blocks, scales, x, tpe, offs, precision=prec, out_dtype=torch.float32)
            want = L.moe_forward_mxfp4(blocks, scales, small, tpe2, offs2, precision=prec, out_dtype=torch.float32)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        nz = 0
        for (lo, hi), (a, b) in zip(groups, g2):
            assert same_bits(got[lo:hi].contiguous(), want[a:b].contiguous()), (prec, lo)
            nz += int(torch.count_nonzero(got[lo:hi]))
        assert int(torch.count_nonzero(got)) == nz, f"mxfp4 {prec}: a row no expert covers is not zero"
        del got
    assert_guards_intact(xb, what="rows into the MXFP4 pre-passes")
    del x, xb


# ======================================================================= MXFP4 fp8 / fp4 / gated kernels: large WEIGHTS
@pytest.mark.parametrize("prec,gated", [("fp8", False), ("fp4", False), ("bf16", True), ("fp8", True), ("fp4", True),
                                        ("fp6", False), ("fp6", True)])
def test_mxfp4_modes_large_weights(lib, prec, gated):
    """The fp8-row, fp4-row, fp6-row and gated MXFP4 kernels on E * N * K/2 > 2^32 bytes of blocks: rows to expert 0, the two
    straddling experts and E - 1, 0xFF everywhere else.  Bit for bit the same op on the four experts alone."""
    need(9)                                                   # (plain bfloat16: test_mxfp4_forward_large_weights)
    K, N, E = 512, 264, 65534
    wb = N * K // 2
    experts = [0, B31 // wb, B32 // wb, E - 1]
    buf = BigGuarded("blocks", E * wb, torch.uint8, 0xFF)
    blocks = buf.view(E, N, K // 2)
    blocks.fill_(0xFF)
    scales = torch.full((E, N, K // 32), 0xFF, dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(14)
    for e in experts:
        blocks[e] = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8)
        scales[e] = torch.randint(120, 131, (N, K // 32), generator=g, device=DEV, dtype=torch.uint8)
    groups = [(0, 33), (40, 110), (113, 183), (190, 223)]
    T = 225
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    tpe2, offs2 = table_of(groups, E=4, T=T)
    x = torch.randn(T, 2 * K if gated else K, generator=g, device=DEV)
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= 3
    idx = torch.tensor(experts, device=DEV)
    b4, s4 = blocks[idx].contiguous(), scales[idx].contiguous()
    L = ops()
    if gated:
        run = lambda b, s, t, o: L.moe_gated_forward_mxfp4(b, s, x, t, o, activation="gelu_tanh", precision=prec, out_dtype=torch.float32)
    else:
        run = lambda b, s, t, o: L.moe_forward_mxfp4(b, s, x, t, o, precision=prec, out_dtype=torch.float32)
    got, want = run(blocks, scales, tpe, offs), run(b4, s4, tpe2, offs2)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert same_bits(got, want), f"mxfp4 {prec} gated={gated}: the far experts' rows differ from the four experts alone"
    assert int(torch.count_nonzero(got[223:])) == 0
    assert_guards_intact(buf, what="large MXFP4 weights, fp8 / fp4 / gated")
    del blocks, buf


# ======================================================================= MXFP4 experts with a fused adapter: large ADAPTERS
LORA_R = 64


def lora_large_shape(entry):
    """(K, N, E, blocks' bytes an expert, adapter's bytes an expert, the experts that get rows) of the adapter cases.
    "fwd": B [E, N, r] float32 with N = 264, r = 64 is 67584 bytes an expert, exactly the blocks' N * K/2 at K = 512, so
    both operands pass 2^31 and 2^32 inside the same experts.  "bwd": A [E, r, K] float32 with K = 544 is 139264 bytes an
    expert and the blocks are 71808: neither divides a boundary, and the two operands straddle in different experts, all
    of which get rows.  Needs no GPU."""
    N, E = 264, 65534
    K = 512 if entry == "fwd" else 544
    wb, ab = N * K // 2, (N if entry == "fwd" else K) * LORA_R * 4
    assert (wb, ab) == ((67584, 67584) if entry == "fwd" else (71808, 139264))
    experts = sorted({0, B31 // ab, B32 // ab, B31 // wb, B32 // wb, E - 1})
    for unit in (wb, ab):
        assert B31 % unit and B32 % unit and E * unit > B32 + 64 * unit
        for top in (B31, B32):
            e = top // unit
            assert e in experts and e * unit < top < (e + 1) * unit and 0 < e < E - 1       # expert e straddles the boundary
    assert len(experts) == (4 if entry == "fwd" else 6)
    return K, N, E, wb, ab, experts


def lora_large_groups(n):
    """n row groups (33 rows, 70 rows ..., 33 rows; 5 uncovered rows between neighbours, 2 behind) and T."""
    groups, pos = [], 0
    for size in [33] + [70] * (n - 2) + [33]:
        groups.append((pos, pos + size))
        pos += size + 5
    return groups, pos - 3


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_mxfp4_lora_large_adapters(lib, entry):
    """ops.moe_forward_mxfp4_lora with B [E, N, 64] and ops.moe_backward_input_mxfp4_lora with A [E, 64, K] past 2^32 bytes,
    on blocks past 2^32 bytes (``lora_large_shape``): rows go to expert 0, every expert in which either operand crosses 2^31
    or 2^32, and E - 1.  Every other expert's adapter is NaN and its blocks and scales are 0xFF; the shrunk rows of the rows
    no expert covers are NaN.  The integer recipe of tests/test_gpu_mxfp4_lora.py (rows and shrunk rows in [-4, 4], adapter
    integers in [-2, 2], scale codes 125 .. 129): the float32 result IS the float64 reference.  The adapter entries have one
    kernel form (the tile kernel; the library has no choice to report)."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    K, N, E, wb, ab, experts = lora_large_shape(entry)
    need(14 if entry == "fwd" else 19)
    torch.cuda.reset_peak_memory_stats()
    r = LORA_R
    buf = BigGuarded("blocks", E * wb, torch.uint8, 0xFF)
    blocks = buf.view(E, N, K // 2)
    blocks.fill_(0xFF)
    scales = torch.full((E, N, K // 32), 0xFF, dtype=torch.uint8, device=DEV)
    abuf = BigGuarded("adapter", E * ab, torch.float32, NAN)
    M = abuf.view(E, N, r) if entry == "fwd" else abuf.view(E, r, K)
    M.fill_(NAN)
    g = torch.Generator(device=DEV).manual_seed(24)
    for e in experts:
        blocks[e] = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8)
        scales[e] = torch.randint(125, 130, (N, K // 32), generator=g, device=DEV, dtype=torch.uint8)
        M[e] = torch.randint(-2, 3, tuple(M.shape[1:]), generator=g, device=DEV).float()
    groups, T = lora_large_groups(len(experts))
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    C = K if entry == "fwd" else N                            # the contraction of the base product
    x = torch.randint(-4, 5, (T, C), generator=g, device=DEV).float()
    v = torch.full((T, r), NAN, device=DEV)
    for lo, hi in groups:
        v[lo:hi] = torch.randint(-4, 5, (hi - lo, r), generator=g, device=DEV).float()
    last = M.shape[2] * 4                                     # the bytes of the last row of an expert's adapter matrix
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= len(experts) - 1
    assert sum(input_wrap_is_visible(abuf, (e + 1) * ab - last, last // 4) for e in experts) >= len(experts) - 1
    Ws = [dequantize_mxfp4(blocks[e:e + 1].cpu(), scales[e:e + 1].cpu())[0].double().to(DEV) for e in experts]
    if entry == "fwd":
        refs = [x[lo:hi].double() @ W.T + v[lo:hi].double() @ M[e].double().T for W, e, (lo, hi) in zip(Ws, experts, groups)]
        got = ops().moe_forward_mxfp4_lora(blocks, scales, x, v, M, tpe, offs, out_dtype=torch.float32)
    else:
        refs = [x[lo:hi].double() @ W + v[lo:hi].double() @ M[e].double() for W, e, (lo, hi) in zip(Ws, experts, groups)]
        got = ops().moe_backward_input_mxfp4_lora(blocks, scales, x, v, M, tpe, offs)
    torch.cuda.synchronize()
    print(f"mxfp4 lora {entry} large adapters: E={E} experts {experts} T={T}, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    assert all(float(ref.abs().max()) < 2 ** 17 for ref in refs)          # (multiples of 2^-3: every partial sum is exact)
    check_rows(got, groups, refs, 0.0, f"mxfp4 lora {entry}", exact=True)
    assert_guards_intact(buf, abuf, what=f"large MXFP4 adapters, {entry}")
    del blocks, M, buf, abuf


# ======================================================================= the dense MXFP4 linear op: a large MATRIX
def linear_large_shape():
    """(K, N, row stride in bytes, the live ranges of weight rows) of the dense case: K = 4128 gives rows of 2064 bytes,
    which divide neither 2^31 nor 2^32; N is the smallest multiple of 4 with N * 2064 > 2^32 + 64 * 2064; 40 weight rows
    are live at the start, around the row that crosses 2^31, around the row that crosses 2^32 and at the end.  Needs no
    GPU."""
    K = 4128
    stride = K // 2
    assert stride == 2064 and B31 % stride and B32 % stride
    N = (B32 // stride + 64) // 4 * 4 + 4
    assert N % 4 == 0 and N * stride > B32 + 64 * stride and (N - 4) * stride <= B32 + 64 * stride
    r31, r32 = B31 // stride, B32 // stride
    assert r31 * stride < B31 < (r31 + 1) * stride and r32 * stride < B32 < (r32 + 1) * stride
    live = [(0, 40), (r31 - 20, r31 + 20), (r32 - 20, r32 + 20), (N - 40, N)]
    assert all(a[1] < b[0] for a, b in zip(live, live[1:]))
    return K, N, stride, live


def test_mxfp4_linear_large_matrix(lib):
    """ops.linear_forward_mxfp4 on ONE matrix [N, K/2] past 2^32 bytes (``linear_large_shape``): T = 2 integer rows in
    [-4, 4], scale codes 125 .. 129 on the live weight rows, 0xFF blocks and scale bytes (NaN) on every other row, so that
    the live output columns are the float64 reference exactly (every sum below 4128 x 4 x 24 < 2^19, in multiples of 2^-3)
    and every other column is NaN.  ``split_k=False`` under both grouped kernels, then the split form forced to S = 4
    (mx4_linear_decode_kernel's wrow * K2 and (slice * T + t) * N, mx4_linear_reduce_kernel's s * plane), each with the
    kernel the library reports asserted.  The scales [N, 129] (270 MB) stay below 2^31 bytes and need no guard."""
    from fused_int4_amd.quantize import dequantize_mxfp4
    K, N, stride, live = linear_large_shape()
    need(8)
    torch.cuda.reset_peak_memory_stats()
    T = 2
    buf = BigGuarded("blocks", N * stride, torch.uint8, 0xFF)
    blocks = buf.view(N, stride)
    blocks.fill_(0xFF)
    scales = torch.full((N, K // 32), 0xFF, dtype=torch.uint8, device=DEV)
    assert scales.numel() < B31
    g = torch.Generator(device=DEV).manual_seed(34)
    for lo, hi in live:
        blocks[lo:hi] = torch.randint(0, 256, (hi - lo, stride), generator=g, device=DEV, dtype=torch.uint8)
        scales[lo:hi] = torch.randint(125, 130, (hi - lo, K // 32), generator=g, device=DEV, dtype=torch.uint8)
    x = torch.randint(-4, 5, (T, K), generator=g, device=DEV).float()
    bias = torch.randint(-8, 9, (N,), generator=g, device=DEV).float()
    assert sum(input_wrap_is_visible(buf, (hi - 1) * stride, stride) for lo, hi in live) >= 3    # each range's last row
    cols = torch.cat([torch.arange(lo, hi) for lo, hi in live]).to(DEV)
    W = dequantize_mxfp4(blocks[cols].cpu(), scales[cols].cpu()).double().to(DEV)
    ref = x.double() @ W.T + bias[cols].double()
    assert float(ref.abs().max()) < 2 ** 19
    dead = torch.ones(N, dtype=torch.bool, device=DEV)
    dead[cols] = False

    def check(got, what):
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, N), what
        assert torch.equal(got[:, cols].double(), ref), f"{what}: a live column is not the exact integer result"
        assert bool(torch.isnan(got[:, dead]).all()), f"{what}: a column of a 0xFF weight row is not NaN"

    hooks = (lib.fql_tune_set_mx4_decode_max_rows, lib.fql_tune_set_mx4_linear_decode_max_rows, lib.fql_tune_set_mx4_linear_slices)
    old = [hooks[0](-1), hooks[1](-1), hooks[2](0)]
    try:
        for kernel in ("tile", "decode"):
            hooks[0](0 if kernel == "tile" else 512)
            assert lib.fql_tune_mx4_kernel(1, T, K, N) == MX4_KERNEL[kernel], kernel
            check(ops().linear_forward_mxfp4(blocks, scales, x, bias=bias, out_dtype=torch.float32, split_k=False), kernel)
        hooks[1](128)
        hooks[2](4)
        assert lib.fql_tune_mx4_linear_kernel(T, K, N) == (4 << 8) | 2
        assert lib.fql_linear_mx4_workspace_bytes(T, K, N, 0, 1) == 16 * T * N * 4       # (sized for 16 slices; S = 4 uses 67 MB)
        check(ops().linear_forward_mxfp4(blocks, scales, x, bias=bias, out_dtype=torch.float32, split_k=True), "split form, S = 4")
    finally:
        for hook, value in zip(hooks, old):
            hook(value)
    print(f"mxfp4 linear large matrix: N={N} K={K}, {N * stride / 2 ** 30:.2f} GiB of blocks, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    assert_guards_intact(buf, what="large dense MXFP4 matrix")
    del blocks, buf


# ======================================================================= per-group INT4 weights: large WEIGHTS
def test_group_int4_large_weights(lib):
    """Per-group scales (group 128) on E * N * K/2 > 2^32 bytes of weights: the forward, and the input gradient through its
    tiled kernel and (a gradient one element past a 16-byte boundary) its element kernel; FMA_REL_FRO as in
    tests/test_gpu_group_moe_ops.py.  With one row per expert or fewer the forward is the one-wave-per-column kernel: the
    matrix-core forms launch (N / 32, T / 32, E) workgroups and want 4 rows an expert, 250 000 rows here."""
    from helpers import misaligned
    need(16)                                                  # (the typed entry's workspace is sized for E experts: 7 GiB)
    K, N, group = 512, 264, 128
    G = K // group
    wb = N * K // 2
    E = B32 // wb + 64
    assert E <= 65534 and E * wb > B32
    experts = [0, B31 // wb, B32 // wb, E - 1]
    buf = BigGuarded("packed", E * wb, torch.uint8, 0xFF)
    P = buf.view(E, N, K // 2)
    P.fill_(0xFF)
    S = torch.full((E, N, G), NAN, device=DEV)
    Z = torch.full((E, N, G), NAN, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(15)
    for e in experts:
        P[e] = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8)
        S[e] = 0.001 + 0.002 * torch.rand(N, G, generator=g, device=DEV)
        Z[e] = torch.randint(5, 11, (N, G), generator=g, device=DEV).float()
    groups = [(0, 33), (40, 110), (113, 183), (190, 223)]
    T = 225
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    x = torch.randn(T, K, generator=g, device=DEV)
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= 3
    W = [dequant_f64(P[e], S[e], Z[e]) for e in experts]
    out = ops().moe_forward(P, S, Z, x, None, tpe, offs)
    check_rows(out, groups, [x[lo:hi].double() @ w.T for w, (lo, hi) in zip(W, groups)], FMA_REL_FRO, "per-group forward")
    gy = torch.randn(T, N, generator=g, device=DEV)
    grefs = [gy[lo:hi].double() @ w for w, (lo, hi) in zip(W, groups)]
    gx = ops().moe_backward_input(P, S, Z, gy, tpe, offs)
    check_rows(gx, groups, grefs, FMA_REL_FRO, "per-group input gradient, tiled kernel")
    gx = ops().moe_backward_input(P, S, Z, misaligned(gy, 1), tpe, offs)
    check_rows(gx, groups, grefs, FMA_REL_FRO, "per-group input gradient, element kernel")
    assert_guards_intact(buf, what="large per-group weights")
    del P, buf


# ======================================================================= QuantizedSparseMoEBlock on large stacked weights
@pytest.mark.parametrize("kind", ["int4", "mxfp4"])
def test_sparse_moe_block_large_weights(kind):
    """``QuantizedSparseMoEBlock`` (E = 128, H = 4096, F = 8256, top-2, swiglu_clamp) whose stacked gate|up weights pass 2^32
    bytes (33 816 576 bytes an expert: expert 63 straddles 2^31, expert 127 straddles 2^32) and whose down weights pass 2^31;
    130 tokens, the gate set so that every token picks two of the experts 0, 63, 64 and 127; every other expert holds 0xFF
    codes and NaN / 0xFF scales.  Against float64 torch on the dequantised weights (``ffn64`` of
    tests/test_gpu_graph_replay.py, the float64 router of tests/test_gpu_sparse_moe_block.py) at the bound that file holds
    the block to: FFN_REL_FRO for INT4 experts, the gated MXFP4 bound for MXFP4 experts."""
    from fused_int4_amd.moe import MXFP4MoEFFN, QuantizedMoEFFN, QuantizedSparseMoEBlock
    from test_gpu_graph_replay import FFN_REL_FRO, MX4_GATED_BOUND, ffn64
    from test_gpu_sparse_moe_block import torch_router
    need(18)
    mx4 = kind == "mxfp4"
    E, H, F, top_k, T = 128, 4096, 8256, 2, 130
    used = [0, 63, 64, 127]
    per = 2 * F * H // 2
    assert E * per > B32 and 63 * per < B31 < 64 * per and 127 * per < B32 < 128 * per and E * H * F // 2 > B31
    with torch.device(DEV):
        experts = (MXFP4MoEFFN if mx4 else QuantizedMoEFFN)(E, H, F, activation="swiglu_clamp")
        m = QuantizedSparseMoEBlock(E, H, F, top_k=top_k, experts=experts)
    g = torch.Generator(device=DEV).manual_seed(91)
    bufs = []
    for name in (("gate_up_blocks", "down_blocks") if mx4 else ("gate_up_packed", "down_packed")):
        old = getattr(experts, name)
        b = BigGuarded(name, old.numel(), torch.uint8, 0xFF)
        v = b.view(*old.shape)
        v.fill_(0xFF)
        setattr(experts, name, v)
        del old
        torch.cuda.empty_cache()
        for e in used:
            v[e] = torch.randint(0, 256, tuple(v.shape[1:]), generator=g, device=DEV, dtype=torch.uint8)
        bufs.append(b)
    if mx4:
        for s in (experts.gate_up_scales, experts.down_scales):
            s.fill_(0xFF)
            for e in used:
                s[e] = torch.randint(116, 121, tuple(s.shape[1:]), generator=g, device=DEV, dtype=torch.uint8)
    else:
        for s, z in ((experts.gate_up_scales, experts.gate_up_zero_points), (experts.down_scales, experts.down_zero_points)):
            s.fill_(NAN)
            z.fill_(NAN)
            for e in used:
                s[e] = 0.001 + 0.002 * torch.rand(tuple(s.shape[1:]), generator=g, device=DEV)
                z[e] = torch.randint(5, 11, tuple(z.shape[1:]), generator=g, device=DEV).float()
    assert input_wrap_is_visible(bufs[0], 64 * per - H // 2, H // 2) >= 1 and input_wrap_is_visible(bufs[0], 128 * per - H // 2, H // 2) >= 1
    with torch.no_grad():
        m.gate.weight.zero_()
        m.gate.weight[used, 0] = 1.0
        m.gate.weight[used, 1:] = 0.01 * torch.randn(len(used), H - 1, generator=g, device=DEV)
        x = torch.randn(T, H, generator=g, device=DEV)
        x[:, 0] = 10.0
        out, logits = m(x)
        torch.cuda.synchronize()
        w, idx = torch_router(logits, top_k, m.renormalize, torch.float64)
        assert set(idx.flatten().tolist()) == set(used), "the far experts are not all in use"
        x64 = x.bfloat16().double() if mx4 else x.double()
        ref = torch.zeros(T, H, dtype=torch.float64, device=DEV)
        for e in used:
            y = ffn64(experts, e, x64, mx4)
            for k in range(top_k):
                sel = idx[:, k] == e
                ref[sel] += w[sel, k].double().unsqueeze(-1) * y[sel]
            del y
    err, bound = rel_fro_dev(out, ref), MX4_GATED_BOUND if mx4 else FFN_REL_FRO
    print(f"block {kind} on {E * per / 2 ** 30:.2f} GiB of gate|up weights: rel_fro {err:.3e} (bound {bound:.1e})")
    assert bool(torch.isfinite(out).all()) and err < bound
    assert_guards_intact(*bufs, what="block weights")
    del m, experts, bufs, v


# ======================================================================= NVFP4 experts: large WEIGHTS, SCALES and ROWS
NV4_KERNEL = {"tile": 0, "decode": 1}                        # what fql_tune_nvfp4_kernel reports
NV4_DECODE_ROWS = 512                                        # the decode threshold the "decode" cases set


def nv4_fill(blocks, scales, experts, g):
    """The integer recipe of tests/test_gpu_nvfp4.py on ``experts`` of an all-0xFF operand set (NaN scale bytes): random
    codes, scale bytes 0x30 .. 0x47, a power-of-two global scale per expert (2^-2, 2^-1, ...), NaN on every other expert.
    Returns (global_scale [E] on the device, [W float64 [N, K] without the global scale, on the device])."""
    from fused_int4_amd.quantize import dequantize_nvfp4
    E, N = blocks.shape[0], blocks.shape[1]
    gs = torch.full((E,), NAN, device=DEV)
    for i, e in enumerate(experts):
        blocks[e] = torch.randint(0, 256, blocks.shape[1:], generator=g, device=DEV, dtype=torch.uint8)
        scales[e] = torch.randint(0x30, 0x48, scales.shape[1:], generator=g, device=DEV, dtype=torch.uint8)
        gs[e] = 2.0 ** (i - 2)
    Ws = [dequantize_nvfp4(blocks[e:e + 1].cpu(), scales[e:e + 1].cpu())[0].double().to(DEV) for e in experts]
    return gs, Ws


def nv4_exact_refs(rows, Ws, gs, experts, groups, transposed, limit):
    """float64 references of the forward (rows @ W^T) or the backward (rows @ W) with the one float32 step * global_scale;
    every sum is asserted below ``limit`` (exact in float32: the products are multiples of 2^-5)."""
    refs = []
    for W, e, (lo, hi) in zip(Ws, experts, groups):
        acc = rows[lo:hi].double() @ (W if transposed else W.T)
        assert float(acc.abs().max()) < limit
        refs.append((acc.float() * gs[e]).double())
    return refs


def nv4_forced(lib, kernel, shape, call):
    """``call()`` with the NVFP4 decode threshold set for ``kernel``; asserts what the library reports for ``shape``."""
    old = lib.fql_tune_set_nvfp4_decode_max_rows(-1)        # (a negative value changes nothing)
    lib.fql_tune_set_nvfp4_decode_max_rows(0 if kernel == "tile" else NV4_DECODE_ROWS)
    try:
        reported = lib.fql_tune_nvfp4_kernel(*shape)
        got = call()
        torch.cuda.synchronize()
    finally:
        lib.fql_tune_set_nvfp4_decode_max_rows(old)
    assert reported == NV4_KERNEL[kernel], (kernel, reported)
    return got


@pytest.mark.parametrize("kernel", ["tile", "decode"])
def test_nvfp4_large_weights(lib, kernel):
    """test_mxfp4_forward_large_weights for NVFP4: E * N * K/2 > 2^32 bytes of blocks (and E * N * K/16 = 0.52 GiB of scale
    bytes), rows to expert 0, the two experts whose blocks straddle 2^31 and 2^32, and E - 1; every other expert holds 0xFF
    codes, 0xFF scale bytes (NaN) and a NaN global scale.  The integer recipe: the float32 result IS the float64
    reference.  Both forward kernels; the input gradient on the same operands rides with the tile case."""
    need(10)
    K, N, E = 512, 264, 65534
    wb = N * K // 2
    assert E * wb > B32 and B31 % wb and B32 % wb
    experts = [0, B31 // wb, B32 // wb, E - 1]
    buf = BigGuarded("blocks", E * wb, torch.uint8, 0xFF)
    blocks = buf.view(E, N, K // 2)
    blocks.fill_(0xFF)
    scales = torch.full((E, N, K // 16), 0xFF, dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(24)
    gs, Ws = nv4_fill(blocks, scales, experts, g)
    groups = [(0, 33), (40, 110), (113, 183), (190, 223)]
    T = 225
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    x = torch.randint(-4, 5, (T, K), generator=g, device=DEV).float()
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= 3   # each expert's last row
    refs = nv4_exact_refs(x, Ws, gs, experts, groups, False, 2 ** 16)
    got = nv4_forced(lib, kernel, (E, T, K, N),
                     lambda: ops().moe_forward_nvfp4(blocks, scales, gs, x, tpe, offs, out_dtype=torch.float32))
    check_rows(got, groups, refs, 0.0, f"nvfp4 {kernel}", exact=True)
    if kernel == "tile":                                    # the input gradient on the same operands (one kernel), as exact
        gy = torch.randint(-4, 5, (T, N), generator=g, device=DEV).float()
        grefs = nv4_exact_refs(gy, Ws, gs, experts, groups, True, 2 ** 15)
        gx = ops().moe_backward_input_nvfp4(blocks, scales, gs, gy, tpe, offs)
        check_rows(gx, groups, grefs, 0.0, "nvfp4 input gradient", exact=True)
    assert_guards_intact(buf, what="large NVFP4 weights")
    del blocks, buf


def test_nvfp4_scales_past_2_gib(lib):
    """The scale operand [E][N][K / 16] past 2^31 bytes: E = 65534, K = 512, N = 1032 is 33024 scale bytes an expert
    (2^8 x 129: 2^31 is no multiple of it, nor are 2^31 and 2^32 of the 264192 block bytes an expert), 2.016 GiB of scale
    bytes in a BigGuarded buffer and 16.1 GiB of blocks in a plain one (their own edges are test_nvfp4_large_weights'): the
    test holds 20.2 GiB.  Rows go to expert 0, the expert whose scale bytes straddle offset 2^31 and E - 1, 73 rows in all;
    everything else is 0xFF, NaN scale bytes and NaN global scales included, so a scale row fetched at a wrapped offset
    (the front guard, 0xFF) is a NaN in the result.  The integer recipe: both forward kernels and the input gradient are
    the float64 reference exactly.  Scale offsets past 2^32 would need 32 GiB of blocks with E <= 65534 and are not
    tested."""
    need(21)
    K, N, E = 512, 1032, 65534
    wb, sb = N * K // 2, N * K // 16
    assert E * sb > B31 and B31 % sb and B31 % wb and B32 % wb and E * sb < B32
    experts = [0, B31 // sb, E - 1]
    assert experts[1] * sb < B31 < (experts[1] + 1) * sb
    blocks = torch.empty(E, N, K // 2, dtype=torch.uint8, device=DEV)
    blocks.fill_(0xFF)
    sbuf = BigGuarded("scales", E * sb, torch.uint8, 0xFF)
    scales = sbuf.view(E, N, K // 16)
    scales.fill_(0xFF)
    g = torch.Generator(device=DEV).manual_seed(25)
    gs, Ws = nv4_fill(blocks, scales, experts, g)
    groups = [(0, 33), (34, 68), (69, 72)]
    T = 73
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    x = torch.randint(-4, 5, (T, K), generator=g, device=DEV).float()
    assert sum(input_wrap_is_visible(sbuf, (e + 1) * sb - K // 16, K // 16) for e in experts[1:]) == 2   # their last rows
    refs = nv4_exact_refs(x, Ws, gs, experts, groups, False, 2 ** 16)
    for kernel in ("tile", "decode"):
        got = nv4_forced(lib, kernel, (E, T, K, N),
                         lambda: ops().moe_forward_nvfp4(blocks, scales, gs, x, tpe, offs, out_dtype=torch.float32))
        check_rows(got, groups, refs, 0.0, f"nvfp4 scales past 2 GiB, {kernel}", exact=True)
        del got
    gy = torch.randint(-2, 3, (T, N), generator=g, device=DEV).float()       # (|sum| <= 1032 x 2 x 22.5 < 2^16)
    grefs = nv4_exact_refs(gy, Ws, gs, experts, groups, True, 2 ** 16)
    gx = ops().moe_backward_input_nvfp4(blocks, scales, gs, gy, tpe, offs)
    check_rows(gx, groups, grefs, 0.0, "nvfp4 scales past 2 GiB, input gradient", exact=True)
    assert_guards_intact(sbuf, what="NVFP4 scales past 2 GiB")
    del blocks, scales, sbuf


@pytest.mark.parametrize("case", ["plain", "gated", "bwd-dy", "bwd-dx"])
def test_nvfp4_rows_past_4_gib(lib, case):
    """[T, 288] (gated: gate | up rows [T, 320]) float32 past 2^32 bytes: into the forward, into the gated forward's
    pre-pass, as the gradient dY into the backward (N = 288, K = 32), and as the result dX out of it (K = 288, N = 8, into a
    guarded buffer full of SENT through the C entry).  T is far above any decode threshold: the tile kernel, asserted.  Each
    result is bit for bit the same op on a compact copy of the four row groups (the small-shape tests tie that to the
    reference: tests/test_gpu_nvfp4.py, test_gpu_nvfp4_bwd.py); rows no expert covers are zero and the guards intact."""
    need(10)
    E = 4
    L = ops()
    gw = torch.Generator().manual_seed(26)

    def weights(N, K):
        return (torch.randint(0, 256, (E, N, K // 2), generator=gw, dtype=torch.uint8).to(DEV),
                torch.randint(0x30, 0x48, (E, N, K // 16), generator=gw, dtype=torch.uint8).to(DEV),
                torch.tensor([0.5, 2.0, 0.25, 4.0], device=DEV))

    if case == "bwd-dx":
        K, N = ROWS_K, 8
        T = B32 // (K * 4) + 4096
        assert T * K * 4 > B32 and (T + 63) // 64 <= 65535
        groups = row_groups(T, K * 4)
        assert len(groups) == 4
        blocks, scales, gs = weights(N, K)
        gy = torch.randn(T, N, generator=torch.Generator(device=DEV).manual_seed(90), device=DEV)
        tpe, offs = table_of(groups)
        small, g2, (tpe2, offs2) = compact_of(gy, groups)
        want = L.moe_backward_input_nvfp4(blocks, scales, gs, small, tpe2, offs2)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        ob = BigGuarded("grad_in", T * K * 4, torch.float32, SENT)
        out = ob.view(T, K)
        step = 1 << 20
        for a in range(0, T, step):
            out[a:a + step] = SENT
        assert output_wrap_is_visible(groups, K * 4, ob) >= 0
        assert lib.fql_tune_nvfp4_kernel(E, T, K, N) == 0
        rc = lib.fql_moe_nvfp4_bwd_input(blocks.data_ptr(), scales.data_ptr(), gs.data_ptr(), gy.data_ptr(), DT[torch.float32],
                                         tpe.data_ptr(), offs.data_ptr(), ob.ptr, DT[torch.float32], E, T, K, N,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == OK
        torch.cuda.synchronize()
        nz = 0
        for (lo, hi), (a, b) in zip(groups, g2):
            assert same_bits(out[lo:hi].contiguous(), want[a:b].contiguous()), (case, lo)
            nz += int(torch.count_nonzero(out[lo:hi]))
        assert int(torch.count_nonzero(out)) == nz, "nvfp4 bwd-dx: a row no expert covers is not zero"
        assert_guards_intact(ob, what="dX out of the NVFP4 backward")
        del out, ob
        return

    width = 2 * 160 if case == "gated" else ROWS_K
    xb, x, groups, g = big_rows(86 + ["plain", "gated", "bwd-dy"].index(case), width)
    T = x.shape[0]
    tpe, offs = table_of(groups)
    small, g2, (tpe2, offs2) = compact_of(x, groups)
    if case == "bwd-dy":
        K, N = 32, width
        blocks, scales, gs = weights(N, K)
        run = lambda rows, t, o: L.moe_backward_input_nvfp4(blocks, scales, gs, rows, t, o)
    elif case == "gated":
        K, N = width // 2, 40
        blocks, scales, gs = weights(N, K)
        run = lambda rows, t, o: L.moe_gated_forward_nvfp4(blocks, scales, gs, rows, t, o, activation="swiglu_clamp",
                                                           out_dtype=torch.float32)
    else:
        K, N = width, 40
        blocks, scales, gs = weights(N, K)
        run = lambda rows, t, o: L.moe_forward_nvfp4(blocks, scales, gs, rows, t, o, out_dtype=torch.float32)
    assert lib.fql_tune_nvfp4_kernel(E, T, K, N) == 0
    got, want = run(x, tpe, offs), run(small, tpe2, offs2)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    nz = 0
    for (lo, hi), (a, b) in zip(groups, g2):
        assert same_bits(got[lo:hi].contiguous(), want[a:b].contiguous()), (case, lo)
        nz += int(torch.count_nonzero(got[lo:hi]))
    assert int(torch.count_nonzero(got)) == nz, f"nvfp4 {case}: a row no expert covers is not zero"
    assert_guards_intact(xb, what=f"rows into the NVFP4 {case} entry")
    del got, x, xb


# ======================================================================= NVFP4 experts with a fused adapter: large ADAPTERS
@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_nvfp4_lora_large_adapters(lib, entry):
    """test_mxfp4_lora_large_adapters for NVFP4: ops.moe_forward_nvfp4_lora with B [E, N, 64] and
    ops.moe_backward_input_nvfp4_lora with A [E, 64, K] past 2^32 bytes, on blocks past 2^32 bytes (``lora_large_shape``:
    the same shapes, the smallest that cross both boundaries): rows go to expert 0, every expert in which either operand
    crosses 2^31 or 2^32, and E - 1.  Every other expert's adapter is NaN, its blocks are 0xFF, its scale bytes 0xFF (NaN)
    and its global scale NaN; the shrunk rows of the rows no expert covers are NaN.  The scale bytes [E, N, K / 16] are twice
    the MXFP4 ones (0.52 and 0.55 GiB instead of 0.26 and 0.27): the test holds 12.9 and 17.6 GiB of its own, and in the
    whole suite's process, beside what earlier files keep cached, it printed peaks of 14.93 and 19.60 GiB on an MI355X (its
    twin 14.67 and 19.33), which is what ``need`` gets, rounded up.  The integer recipe of
    tests/test_gpu_nvfp4_lora.py (rows and shrunk rows in [-4, 4], adapter integers in [-2, 2], scale bytes 0x30 .. 0x47, a
    power-of-two global scale that differs between neighbouring live experts and scales the weight term only): a weight
    term is a multiple of g * 2^-5, an adapter term an integer, and the sum of the absolute values of all terms of one
    output is asserted below 2^24 of that unit, so the float32 result IS the float64 reference.  The adapter entries have
    one kernel form (the tile kernel; the library has no choice to report)."""
    K, N, E, wb, ab, experts = lora_large_shape(entry)
    need(15 if entry == "fwd" else 20)
    torch.cuda.reset_peak_memory_stats()
    r = LORA_R
    buf = BigGuarded("blocks", E * wb, torch.uint8, 0xFF)
    blocks = buf.view(E, N, K // 2)
    blocks.fill_(0xFF)
    scales = torch.full((E, N, K // 16), 0xFF, dtype=torch.uint8, device=DEV)
    abuf = BigGuarded("adapter", E * ab, torch.float32, NAN)
    M = abuf.view(E, N, r) if entry == "fwd" else abuf.view(E, r, K)
    M.fill_(NAN)
    g = torch.Generator(device=DEV).manual_seed(27)
    gs, Ws = nv4_fill(blocks, scales, experts, g)
    live = [float(gs[e]) for e in experts]
    assert all(a != b for a, b in zip(live, live[1:])) and int(torch.isnan(gs).sum()) == E - len(experts)
    for e in experts:
        M[e] = torch.randint(-2, 3, tuple(M.shape[1:]), generator=g, device=DEV).float()
    groups, T = lora_large_groups(len(experts))
    tpe, offs = table_of(groups, E=E, experts=experts, T=T)
    C = K if entry == "fwd" else N                            # the contraction of the base product
    x = torch.randint(-4, 5, (T, C), generator=g, device=DEV).float()
    v = torch.full((T, r), NAN, device=DEV)
    for lo, hi in groups:
        v[lo:hi] = torch.randint(-4, 5, (hi - lo, r), generator=g, device=DEV).float()
    last = M.shape[2] * 4                                     # the bytes of the last row of an expert's adapter matrix
    assert sum(input_wrap_is_visible(buf, (e + 1) * wb - K // 2, K // 2) for e in experts) >= len(experts) - 1
    assert sum(input_wrap_is_visible(abuf, (e + 1) * ab - last, last // 4) for e in experts) >= len(experts) - 1
    refs = []
    for W, e, ge, (lo, hi) in zip(Ws, experts, live, groups):
        We, Me = (W.T, M[e].double().T) if entry == "fwd" else (W, M[e].double())
        x64, v64 = x[lo:hi].double(), v[lo:hi].double()
        mass = (x64.abs() @ We.abs()) * ge + v64.abs() @ Me.abs()
        assert float(mass.max()) < 2.0 ** 24 * min(ge * 2.0 ** -5, 1.0)    # (every partial sum is exact in float32)
        refs.append((x64 @ We) * ge + v64 @ Me)
        assert bool((v64 @ Me).count_nonzero())               # (the adapter matters)
    if entry == "fwd":
        got = ops().moe_forward_nvfp4_lora(blocks, scales, gs, x, v, M, tpe, offs, out_dtype=torch.float32)
    else:
        got = ops().moe_backward_input_nvfp4_lora(blocks, scales, gs, x, v, M, tpe, offs)
    torch.cuda.synchronize()
    print(f"nvfp4 lora {entry} large adapters: E={E} experts {experts} T={T}, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    check_rows(got, groups, refs, 0.0, f"nvfp4 lora {entry}", exact=True)
    assert_guards_intact(buf, abuf, what=f"large NVFP4 adapters, {entry}")
    del blocks, M, buf, abuf
