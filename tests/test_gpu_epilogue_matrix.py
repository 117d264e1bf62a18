"""The GEMM epilogue options -- float16 / bfloat16 output, bias, per-row routing weight -- in EVERY tile kernel, and
16-bit activations through every form of the pre-pass.

The contract ("Numerics"): out = dtype(fl32(fl32(acc + bias) * row_weight)), one rounding per step, the
last one to nearest even; 16-bit inputs are widened exactly.  So every option is checked bit for bit against the plain
float32 result of the same kernel, which the other test files tie to the float64 oracle and to every other tile
configuration (and which is tied to the oracle here again, so that the reference is never only the code under test).

(a) every built tile configuration forced through the tuning hook, all twelve epilogue variants;
(b) one smallest shape per id the dispatcher can return, through the public entry points;
(c) round-to-nearest-even ties of both kinds and signs, in every kernel family;
(d) 16-bit rows through the one-row, the multi-row and the scalar pre-pass, with format extremes.

No tolerance here is a measured number: bit equality, a constant of tests/helpers.py, or u + (1 + u) * tol for one more
rounding of unit roundoff u."""
import numpy as np
import pytest
import torch

from helpers import (EXACT_REL_FRO, FAST_REL_FRO, INT8_REL_FRO, FP8_ACC_REL_FRO, FP8_FORMAT_REL_FRO, rel_fro, rel_fro_dev,
                     dequant_f64, misaligned)
from oracle import oracle as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # unit roundoff of ONE rounding to nearest
PREC_TOL = {"exact": EXACT_REL_FRO, "fast": FAST_REL_FRO, "int8": INT8_REL_FRO, "fp8": FP8_FORMAT_REL_FRO}
SIXTEEN = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def fq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fused_int4_amd as pkg
    from fused_int4_amd import _native
    _native.lib()
    return pkg


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """The raw bit patterns: -0.0 != +0.0, a NaN equals itself."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b.to(a.device)))


def first_diff(a, b):
    """(number of differing elements, index of the first one) for an assertion message."""
    d = (bits(a) != bits(b.to(a.device))).nonzero()
    return int(d.shape[0]), (d[0].tolist() if d.shape[0] else None)


def tile_config_ids(lib, prec_code, fp8):
    if fp8:
        return [1, 5, 6, 7, 8, 11, 12]
    return [c for c in (list(range(lib.fql_tune_num_configs())) + list(range(100, 100 + lib.fql_tune_num_rows32_configs()))
                        + list(range(200, 200 + lib.fql_tune_num_rows16_configs()))
                        + list(range(300, 300 + lib.fql_tune_num_w4_configs())))
            if lib.fql_tune_is_config(c, prec_code)]


# ------------------------------------------------------------------------------ (a) forced-configuration matrix
FILL = 768.0                       # exact in float32, float16 and bfloat16: what the test leaves in rows nobody may write
CASES_A = [("grouped", 200), ("grouped", 201), ("single_offset", 200)]


@pytest.mark.parametrize("case,N", CASES_A)
@pytest.mark.parametrize("prec", ["exact", "fast", "int8", "fp8"])
def test_every_tile_configuration_every_epilogue_variant(fq, prec, case, N):
    """{none, bias, row weight, both} x {float32, float16, bfloat16} in every built configuration, on the ragged grouped
    problem of test_heavy_tails_every_tile_configuration (every fifth row heavy-tailed: residual passes and the
    one-wave-per-SIMD kernel's modes 1 and 2 run) plus a 3-row uncovered tail: N = 200 (vector stores, ragged last
    fragment), N = 201 (scalar stores, odd 16-bit row pitch); and on one 130-row matrix whose output starts one element
    past an aligned address (16-bit outputs 2-byte aligned: no vector store is legal)."""
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    rng = np.random.default_rng(99)
    K = 768
    grouped = case == "grouped"
    if grouped:
        E = 5
        counts = np.array([0, 7, 33, 70, 129], np.int32)
        offs = (np.cumsum(counts) - counts).astype(np.int32)
        T = int(counts.sum()) + 3
    else:
        E, T = 1, 130
        counts, offs = np.array([T], np.int32), np.array([0], np.int32)
    covered = np.zeros(T, bool)
    covered[:int(counts.sum())] = True
    q = [O.quantize_weights((rng.standard_normal((N, K)) * 0.02).astype(np.float32)) for _ in range(E)]
    P, S, Z = (np.stack([t[i] for t in q]) for i in range(3))
    x = rng.standard_normal((T, K)).astype(np.float32)
    heavy = np.zeros(T, bool)
    heavy[::5] = True
    for t in range(0, T, 5):
        x[t, rng.choice(K, 2, replace=False)] *= 800.0
    bias = rng.standard_normal((E, N)).astype(np.float32)      # one vector per expert, as the scales
    expert_of = np.repeat(np.arange(E), counts)             # (the covered rows are the first sum(counts))
    rw = (0.1 + 0.9 * rng.random(T)).astype(np.float32)
    dP, dS, dZ, dx = dev(P if grouped else P[0]), dev(S if grouped else S[0]), dev(Z if grouped else Z[0]), dev(x)
    dc, do = (dev(counts), dev(offs)) if grouped else (None, None)
    dbias, drw = dev(bias), dev(rw)
    limbs, delta, rowsum = ops.act_quant(dx, precision=prec, tokens_per_expert=dc, input_offsets=do)   # ONE pre-pass
    if prec in ("exact", "fast"):
        assert 0 < int((delta[1] != 0).sum()) < T          # flagged and unflagged rows
    cfgs = tile_config_ids(lib, ops._precision(prec), prec == "fp8")
    assert len(cfgs) >= (7 if prec == "fp8" else 20)

    def run(cfg, dtype, b, w, old_hook=False):
        """One launch into a pre-filled buffer; returns (the whole buffer, the [T, N] output inside it, its offset)."""
        pad = 0 if grouped else 1
        buf = torch.full((T * N + 16,), FILL, dtype=dtype, device="cuda")
        if pad:                                             # one element past a 16-byte boundary
            pad += (-(buf.data_ptr() // buf.element_size())) % (16 // buf.element_size())
        out = buf[pad:pad + T * N].view(T, N)
        assert grouped or out.data_ptr() % 16 == out.element_size()
        if old_hook:
            rc = ops.tune_gemm_i8(cfg, limbs, delta, rowsum, dP, dS, dZ, dc, do, out, E, T, K, N, prec)
        else:
            rc = ops.tune_gemm_i8(cfg, limbs, delta, rowsum, dP, dS, dZ, dc, do, out, E, T, K, N, prec,
                                  out_dtype=dtype, bias=b, row_weight=w)
        assert rc == 0, (cfg, dtype, rc)
        return buf, out, pad

    # the plain float32 output of the first configuration against the float64 oracle ...
    o = run(cfgs[0], torch.float32, None, None, old_hook=True)[1].cpu().numpy()
    ok = covered.copy()
    if prec == "fp8":                                        # the kernel's own error on the same e4m3 inputs (helpers.py)
        xq, xs = O.quantize_activations_fp8(x)
        ref = O.reference_moe_grouped_fp8(xq, xs, P, S, Z, counts, offs)
        tol = FP8_ACC_REL_FRO
    else:
        ref = C.moe_grouped(P, S, Z, x, counts, offs)
        # 3e-4: the heavy-tail constant of 2 limbs (test_gpu_heavy_tails.py); 1 limb has no residual limb set, its
        # stated bound is for rows without outliers
        tol = {"exact": EXACT_REL_FRO, "fast": 3e-4, "int8": INT8_REL_FRO}[prec]
        if prec == "int8":
            ok &= ~heavy
    err = rel_fro(o[ok], ref[ok])
    print(f"{prec} {case} N={N}: configuration {cfgs[0]} vs oracle {err:.3e} (bound {tol:.1e})")
    assert err < tol, err
    assert (o[~covered] == FILL).all()
    # ... and what every variant must then be, in numpy float32: + bias, x row weight, one rounding each
    want = {}
    for b in (None, bias):
        for w in (None, rw):
            e = o.copy()
            if b is not None:
                e[covered] = (e[covered] + b[expert_of]).astype(np.float32)
            if w is not None:
                e[covered] = (e[covered] * w[covered, None]).astype(np.float32)
            e[~covered] = FILL
            for dtype in (torch.float32, torch.float16, torch.bfloat16):
                want[(b is not None, w is not None, dtype)] = torch.from_numpy(e).to(dtype).cuda()
    bad = []
    for cfg in cfgs:
        for (hb, hw, dtype), e in want.items():
            buf, out, pad = run(cfg, dtype, dbias if hb else None, drw if hw else None)
            if not same_bits(out, e):
                bad.append((cfg, "bias" if hb else "-", "row_weight" if hw else "-", str(dtype), first_diff(out, e)))
            # nothing outside the [T, N] block was written
            assert (buf[:pad] == FILL).all() and (buf[pad + T * N:] == FILL).all(), (cfg, hb, hw, dtype)
    torch.cuda.synchronize()
    assert not bad, f"{len(bad)} (configuration, variant) pairs differ, first: {bad[:6]}"


def test_hook_refuses_a_row_weight_that_is_not_the_plane_behind_delta(fq):
    """The kernels read the row weight from the plane behind delta's sets; the hook must not pretend otherwise."""
    import ctypes
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    x = torch.randn(40, 256, device="cuda")
    p, s, z = fq.quantize_weights(torch.randn(64, 256, device="cuda"))
    limbs, delta, rowsum = ops.act_quant(x, precision="exact")
    out = torch.zeros(40, 64, device="cuda")
    elsewhere = torch.ones(40, device="cuda")
    fn = lib.fql_tune_gemm_i8
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + \
        [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    args = [1, limbs.data_ptr(), delta.data_ptr(), rowsum.data_ptr(), p.data_ptr(), s.data_ptr(), z.data_ptr(), None, None,
            out.data_ptr()]
    assert fn(*args, 0, None, elsewhere.data_ptr(), 1, 40, 256, 64, 3, None, None, 0) == -7     # FQL_ERR_ALIGNMENT
    assert fn(*args, 3, None, None, 1, 40, 256, 64, 3, None, None, 0) == -8                     # FQL_ERR_DTYPE
    assert fn(*args, 0, None, None, 1, 40, 256, 64, 3, None, None, 0) == 0
    torch.cuda.synchronize()
    assert same_bits(out, ops.linear_forward(x, p, s, z, precision="exact"))


# ------------------------------------------------------------------------------ (b) dispatch matrix, public entry points
# (name, precision, expected id, K, N, rows: an int = one matrix of that many rows / a list = rows per expert, w4 on)
G202 = [16, 0, 13, 16, 9, 16, 16, 15]                       # <= 16 rows per expert
G103 = [30, 0, 17, 32, 25, 20, 32, 27]                      # 17 .. 32
G64 = [64, 0, 33, 50, 40, 64, 60, 45]                       # 33 .. 64
G128 = [70, 0, 128, 65, 100, 90, 80, 66]                    # 65 .. 128
S16, S32, S64, S128 = [16, 0, 9, 13], [30, 0, 17, 32], [64, 0, 33, 50], [128, 0, 65, 100]
NW = 3848                          # 16 column tiles of 256 x 8 experts: wide_tiles is exactly 128; N % 32 == 8
N192, N256 = 4104, 6152            # the 192-wide / 256-wide tile wins; N % 32 == 8: whole fragments and a ragged one
NS = 264                           # small N: "few tiles" branch; N % 32 == 8


def _rows(prec, wide192, wide64, few128):
    """The table of one limb precision: linear rows where one matrix reaches the id, grouped rows for every id."""
    return [
        (prec, 207, 512, 200, 10, True), (prec, 8, 512, 200, 24, True), (prec, 7, 512, 200, 50, True),
        (prec, few128, 512, 200, 100, True), (prec, 1, 512, 200, 130, True),
        (prec, 207, 512, NS, S16, True), (prec, 8, 512, NS, S32, True), (prec, 7, 512, NS, S64, True),
        (prec, few128, 512, NS, S128, True),
        (prec, 202, 512, NW, G202, True), (prec, 103, 512, NW, G103, True),
        (prec, wide64, 768, NW, G64, True), (prec, wide192, 768, N192, G128, True),
    ]


TABLE = (_rows("exact", 301, 301, 1)
         + [("exact", 9, 768, NW, G64, False), ("exact", 0, 768, N192, G128, False)]
         + _rows("fast", 3, 11, 13) + [("fast", 2, 512, N256, G128, True)]
         + _rows("int8", 12, 11, 13) + [("int8", 2, 512, N256, G128, True)]
         + [("fp8", 8, 512, 200, 24, True), ("fp8", 7, 512, 200, 50, True), ("fp8", 6, 512, 200, 100, True),
            ("fp8", 8, 512, NS, S32, True), ("fp8", 7, 512, NS, S64, True), ("fp8", 6, 512, NS, S128, True),
            ("fp8", 5, 512, NW, G103, True), ("fp8", 11, 512, NW, G64, True), ("fp8", 12, 512, N192, G128, True)])
EXPECTED_IDS = {
    "exact": {207, 8, 7, 1, 202, 103, 301, 9, 0},
    "fast": {207, 8, 7, 13, 202, 103, 11, 3, 1, 2},
    "int8": {207, 8, 7, 13, 202, 103, 11, 12, 1, 2},
    "fp8": {8, 7, 6, 5, 11, 12},
}


def _row_id(r):
    prec, cfg, K, N, rows, w4 = r
    shape = f"{rows}x{K}x{N}" if isinstance(rows, int) else f"E{len(rows)}m{max(rows)}x{K}x{N}"
    return f"{prec}-{cfg}-{shape}" + ("" if w4 else "-w4off")


def _row_shape(r):
    prec, cfg, K, N, rows, w4 = r
    if isinstance(rows, int):
        return 1, rows, 0
    return len(rows), sum(rows) + 3, 1                      # a 3-row tail no expert covers


def test_dispatch_table_covers_every_id_the_dispatcher_returns():
    """The table's ids are exactly the lists of choose_cfg / choose_cfg_f8 (csrc/fql_int4.hip), and both 301 classes
    (33..64 rows per group, and the 128 x 192 winner) are there.  Needs no GPU work: the library answers on the host."""
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    for prec, ids in EXPECTED_IDS.items():
        assert {r[1] for r in TABLE if r[0] == prec} == ids, prec
    assert {max(r[4]) > 64 for r in TABLE if r[0] == "exact" and r[1] == 301} == {True, False}
    old = lib.fql_tune_set_w4(1)
    try:
        for r in TABLE:
            prec, cfg, K, N, rows, w4 = r
            E, T, grouped = _row_shape(r)
            lib.fql_tune_set_w4(1 if w4 else 0)
            assert lib.fql_tune_chosen_cfg(ops._precision(prec), E, T, K, N, grouped) == cfg, _row_id(r)
    finally:
        lib.fql_tune_set_w4(old)


def _normal_range(ref, dtype):
    """Every reference output is inside the normal range of the format (with a factor 2 to spare at the top)."""
    fi = torch.finfo(dtype)
    a = ref.abs()
    return bool(a.max() < fi.max / 2) and bool((a[a > 0] >= fi.tiny).all())


@pytest.mark.parametrize("dtype", SIXTEEN, ids=["f16", "bf16"])
@pytest.mark.parametrize("row", TABLE, ids=[_row_id(r) for r in TABLE])
def test_dispatched_kernel_16bit_io_bias_and_row_weight(fq, row, dtype):
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    prec, cfg, K, N, rows, w4 = row
    E, T, grouped = _row_shape(row)
    tol, u = PREC_TOL[prec], UNIT[dtype]
    g = torch.Generator(device="cuda").manual_seed(1000 * cfg + T + N)
    q = [fq.quantize_weights(torch.randn(N, K, device="cuda", generator=g) * 0.02) for _ in range(E)]
    old = lib.fql_tune_set_w4(1 if w4 else 0)
    try:
        assert lib.fql_tune_chosen_cfg(ops._precision(prec), E, T, K, N, grouped) == cfg
        if grouped:
            P, S, Z = (torch.stack([t[i] for t in q]) for i in range(3))
            counts = torch.tensor(rows, dtype=torch.int32, device="cuda")
            offs = (torch.cumsum(counts, 0) - counts).to(torch.int32)
            spans = [(int(o), int(o + c)) for o, c in zip(offs.tolist(), rows)]
            assert lib.fql_native_dtype_supported(T, E, K, N, ops._precision(prec), P.data_ptr(), 1) == 1
        else:
            P, S, Z = q[0]
            spans = [(0, T)]
            assert lib.fql_native_dtype_supported(T, 1, K, N, ops._precision(prec), P.data_ptr(), 0) == 1
        Wd = [dequant_f64(*t) for t in q]
        # outputs of standard deviation ~ 4e3: inside the normal range of float16 at both ends.  The draw is repeated (a few
        # times at most) until the REFERENCE says so: one element in 1e8 lands below 2^-14 by chance.
        for attempt in range(4):
            x16 = (torch.randn(T, K, device="cuda", generator=g) * 8192.0).to(dtype)
            xf = x16.float()
            ref = torch.zeros(T, N, dtype=torch.float64, device="cuda")
            for (lo, hi), W in zip(spans, Wd):
                ref[lo:hi] = xf[lo:hi].double() @ W.T
            if _normal_range(ref, dtype):
                break
        assert _normal_range(ref, dtype)

        def fwd(xin, out_dtype):
            if grouped:
                return ops.moe_forward_any(P, S, Z, xin, None, counts, offs, precision=prec, out_dtype=out_dtype)
            return ops.linear_forward_any(xin, P, S, Z, precision=prec, out_dtype=out_dtype)

        base = fwd(xf, torch.float32)
        e32 = rel_fro_dev(base, ref)
        assert e32 < tol, e32                               # the float32 path against float64: not only itself
        want16 = base.to(dtype)
        got = fwd(x16, dtype)
        assert got.dtype == dtype and same_bits(got, want16), first_diff(got, want16)
        assert same_bits(fwd(xf, dtype), want16)
        assert same_bits(fwd(x16, torch.float32), base)
        e16 = rel_fro_dev(got, ref)
        print(f"{_row_id(row)} {dtype}: float32 path {e32:.3e} (bound {tol:.1e}), 16-bit output {e16:.3e} (bound {u + (1 + u) * tol:.3e})")
        assert e16 < u + (1 + u) * tol, e16
        if grouped:
            assert T - spans[-1][1] == 3 and not bits(got[-3:]).any() and not bits(base[-3:]).any()
            if prec != "fp8":                               # (the row-weight entry point has no fp8 form)
                ri = torch.arange(T, dtype=torch.int32, device="cuda")
                w = 0.1 + 0.9 * torch.rand(T, device="cuda", generator=g)
                y = ops.moe_gather_forward(P, S, Z, xf, ri, counts, offs, precision=prec)
                yw = ops.moe_gather_forward(P, S, Z, xf, ri, counts, offs, precision=prec, row_weight=w)
                assert same_bits(y, base)
                assert same_bits(yw, y * w[:, None]), first_diff(yw, y * w[:, None])
                assert not bits(yw[-3:]).any()
        else:
            bias = torch.randn(N, device="cuda", generator=g) * 4096.0
            with_bias = ops.linear_forward(xf, P, S, Z, precision=prec, bias=bias)
            assert same_bits(with_bias, base + bias[None, :]), first_diff(with_bias, base + bias[None, :])
            got = ops.linear_forward_any(x16, P, S, Z, precision=prec, bias=bias)
            assert same_bits(got, with_bias.to(dtype)), first_diff(got, with_bias.to(dtype))
            assert same_bits(ops.linear_forward_any(xf, P, S, Z, precision=prec, out_dtype=dtype, bias=bias), with_bias.to(dtype))
            assert same_bits(ops.linear_forward_any(x16, P, S, Z, precision=prec, out_dtype=torch.float32, bias=bias), with_bias)
    finally:
        lib.fql_tune_set_w4(old)


# ------------------------------------------------------------------------------ (c) ties
def tie_problem():
    """Integer activations and integer-valued weights (scale 1, integer zero points), K = 64: every output is an exact
    integer below 2^24.  Rows 0..31 are non-negative, rows 32..63 their negation; columns with zero point 0 give sums
    of a few thousand (float16 ties: odd integers in [2048, 4096)), the others sums of a few hundred (bfloat16 ties)."""
    rng = np.random.default_rng(5)
    T, N, K = 64, 96, 64
    qw = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    zp = np.where(np.arange(N) % 2 == 0, 0, rng.integers(6, 10, size=N)).astype(np.float32)
    xi = rng.integers(0, 9, size=(T, K))
    xi[T // 2:] = -xi[:T // 2]
    ei = xi.astype(np.int64) @ (qw.astype(np.int64) - zp.astype(np.int64)[:, None]).T
    assert np.abs(ei).max() < 2 ** 24
    return xi, qw, zp, ei


def tie_kinds(ei, dtype):
    """(sign, direction) of every exact tie among the integers ``ei`` when rounded to ``dtype``: direction -1 where the
    even neighbour is the smaller magnitude, +1 where it is the larger."""
    p = 11 if dtype == torch.float16 else 8                 # significand bits
    kinds = set()
    for v in np.unique(ei):
        a = abs(int(v))
        if a < 2 ** p:
            continue                                        # exactly representable
        spacing = 1 << (a.bit_length() - p)
        if a % spacing == spacing // 2:                     # an odd multiple of the half-spacing
            kinds.add((int(np.sign(v)), -1 if (a // spacing) % 2 == 0 else 1))
    return kinds


def test_ties_occur_in_the_reference():
    """On the reference alone (no GPU): both formats, both signs, both directions."""
    _, _, _, ei = tie_problem()
    every = {(s, d) for s in (-1, 1) for d in (-1, 1)}
    assert tie_kinds(ei, torch.float16) == every
    assert tie_kinds(ei, torch.bfloat16) == every
    odd = ei[(np.abs(ei) >= 2048) & (np.abs(ei) < 4096) & (ei % 2 != 0)]
    assert (odd > 0).any() and (odd < 0).any()              # float16: odd integers in [2048, 4096)
    # and torch's cast is the round-to-nearest-even the contract names
    t = torch.tensor([2049.0, 2051.0, -2049.0, -2051.0, 257.0, 259.0, -257.0, -259.0])
    assert t[:4].to(torch.float16).tolist() == [2048.0, 2052.0, -2048.0, -2052.0]
    assert t[4:].to(torch.bfloat16).float().tolist() == [256.0, 260.0, -256.0, -260.0]


@pytest.mark.parametrize("dtype", SIXTEEN, ids=["f16", "bf16"])
def test_ties_round_to_even_in_every_kernel_family(fq, dtype):
    """The ids the dispatcher returns, one or more per family: wide 8-, 4- and 2-wave (1, 7, 8), 32-row (103), 16-row
    (202, 207), one wave per SIMD (301; its pipeline wants K >= 257: the same problem with zero activations behind
    k = 64), at 3 limbs, the wide kernel at 2 limbs and 1 limb, and the fp8 form through its own entry point."""
    from fused_int4_amd import ops
    xi, qw, zp, ei = tie_problem()
    T, K = xi.shape
    N = qw.shape[0]
    want = torch.from_numpy(ei).to(torch.float32).to(dtype).cuda()       # exact below 2^24, then ONE rounding
    pack = lambda q: ((q[:, 1::2] << 4) | q[:, 0::2]).astype(np.uint8)
    ones = np.ones(N, np.float32)
    x = dev(xi.astype(np.float32))
    p, s, z = dev(pack(qw)), dev(ones), dev(zp)
    Kw = 512
    xw = np.zeros((T, Kw), np.float32)
    xw[:, :K] = xi
    qw_w = np.random.default_rng(6).integers(0, 16, size=(N, Kw), dtype=np.uint8)
    qw_w[:, :K] = qw
    for prec, cfgs in (("exact", (1, 7, 8, 103, 202, 207)), ("fast", (1,)), ("int8", (1,))):
        limbs, delta, rowsum = ops.act_quant(x, precision=prec)
        for cfg in cfgs:
            out = torch.zeros(T, N, dtype=dtype, device="cuda")
            assert ops.tune_gemm_i8(cfg, limbs, delta, rowsum, p, s, z, None, None, out, 1, T, K, N, prec, out_dtype=dtype) == 0
            assert same_bits(out, want), (prec, cfg, first_diff(out, want))
    limbs, delta, rowsum = ops.act_quant(dev(xw), precision="exact")
    out = torch.zeros(T, N, dtype=dtype, device="cuda")
    assert ops.tune_gemm_i8(301, limbs, delta, rowsum, dev(pack(qw_w)), s, z, None, None, out, 1, T, Kw, N, "exact", out_dtype=dtype) == 0
    assert same_bits(out, want), ("w4", first_diff(out, want))
    x8 = O.e4m3_encode(xi.astype(np.float32))
    assert np.array_equal(O.e4m3_decode(x8), xi.astype(np.float32))
    out = ops.linear_forward_fp8(dev(x8), None, p, s, z, out_dtype=dtype)
    assert same_bits(out, want), ("fp8", first_diff(out, want))
    # the product path as well (the dispatcher's own choice)
    assert same_bits(ops.linear_forward_any(x.to(dtype), p, s, z, precision="exact"), want)


# ------------------------------------------------------------------------------ (d) 16-bit inputs, every pre-pass form
def _native_equals_converted(ops, lib, prec, x16, p, s, z, what):
    """native(x16) == float32-path(x16.float()), bit for bit, and the native path was really taken."""
    T, K = x16.shape
    assert x16.is_contiguous()
    assert lib.fql_native_dtype_supported(T, 1, K, p.shape[0], ops._precision(prec), p.data_ptr(), 0) == 1, what
    want = ops.linear_forward(x16.float(), p, s, z, precision=prec)
    got = ops.linear_forward_any(x16, p, s, z, precision=prec, out_dtype=torch.float32)
    assert same_bits(got, want), (what, first_diff(got, want))
    return want


@pytest.mark.parametrize("dtype", SIXTEEN, ids=["f16", "bf16"])
@pytest.mark.parametrize("prec", ["exact", "fast", "int8", "fp8"])
def test_16bit_rows_through_every_pre_pass_form(fq, prec, dtype):
    """The limb (and e4m3) conversion starts from the exactly widened value, so no tolerance applies: one row per
    workgroup, the vectorised multi-row form (tuning switch), the scalar form (a base 2 bytes past a 16-byte boundary),
    rows of several 2048-k slabs, heavy-tailed rows (residual limb set), and the extremes of each format."""
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    g = torch.Generator(device="cuda").manual_seed(31)
    N = 72
    weights = {K: fq.quantize_weights(torch.randn(N, K, device="cuda", generator=g) * 0.02) for K in (512, 4128)}

    def rows(T, K):
        return torch.randn(T, K, device="cuda", generator=g)

    x = rows(40, 512)
    x[::4, 7] *= 800.0                                      # two 800 x outliers in every fourth row: flagged at 2 / 3 limbs,
    x[::4, 300] *= 800.0                                    # and |x| stays below float16's 65504
    x[5] = 0.0
    x[6, :] = 0.0
    x[6, 3] = -0.0
    special = x.to(dtype)
    special[9, 0] = 2.0 ** -24 if dtype == torch.float16 else 1e-38      # the smallest float16 subnormal / a tiny bfloat16
    if dtype == torch.float16:
        special[10, 11] = 65504.0                           # the largest float16
        special[11] = (rows(1, 512)[0] * 2.0 ** -20).to(dtype)            # a row of subnormals and near-subnormals
    else:
        special[10] = (rows(1, 512)[0] * 1e35).to(dtype)    # finite outputs near the top of the exponent range
        special[11] = (rows(1, 512)[0] * 1e-38).to(dtype)   # and at the bottom
        special[12, 5] = 3e38                               # (this row's outputs may overflow: the bits must still agree)
    p, s, z = weights[512]
    one = _native_equals_converted(ops, lib, prec, special, p, s, z, "one row per workgroup")
    assert torch.isfinite(one[:9]).all() and not bits(one[5]).any()
    print(f"{prec} {dtype}: non-finite rows among the extremes: {(~torch.isfinite(one).all(dim=1)).nonzero().flatten().tolist()}")
    if prec in ("exact", "fast"):
        _, d, _ = ops.act_quant(special.float(), precision=prec)
        assert 0 < int((d[1] != 0).sum()) < 40              # the residual limb set is in use
    old = lib.fql_tune_set_act_single_rows(0)
    try:
        multi = _native_equals_converted(ops, lib, prec, special, p, s, z, "multi-row")
        scalar_in = misaligned(special, 1)
        assert scalar_in.data_ptr() % 16 == 2
        scalar = _native_equals_converted(ops, lib, prec, scalar_in, p, s, z, "scalar, multi-row grid")
    finally:
        lib.fql_tune_set_act_single_rows(old)
    assert same_bits(multi, one) and same_bits(scalar, one)    # the three forms agree with each other as well
    _native_equals_converted(ops, lib, prec, misaligned(special, 1), p, s, z, "scalar")
    # rows of three 2048-k slabs (K % 256 != 0), all three forms
    p, s, z = weights[4128]
    long16 = rows(9, 4128).to(dtype)
    long16[::2, 4100] *= 500.0
    one = _native_equals_converted(ops, lib, prec, long16, p, s, z, "multi-slab")
    old = lib.fql_tune_set_act_single_rows(0)
    try:
        assert same_bits(_native_equals_converted(ops, lib, prec, long16, p, s, z, "multi-slab, multi-row"), one)
        assert same_bits(_native_equals_converted(ops, lib, prec, misaligned(long16, 1), p, s, z, "multi-slab, scalar"), one)
    finally:
        lib.fql_tune_set_act_single_rows(old)
    # grouped rows (an empty expert, a 3-row tail) through the multi-row form
    E, K = 4, 512
    q = [fq.quantize_weights(torch.randn(N, K, device="cuda", generator=g) * 0.02) for _ in range(E)]
    P, S, Z = (torch.stack([t[i] for t in q]) for i in range(3))
    counts = torch.tensor([9, 0, 33, 20], dtype=torch.int32, device="cuda")
    offs = (torch.cumsum(counts, 0) - counts).to(torch.int32)
    xg = rows(65, K).to(dtype)
    xg[::3, 100] *= 700.0
    assert lib.fql_native_dtype_supported(65, E, K, N, ops._precision(prec), P.data_ptr(), 1) == 1
    want = ops.moe_forward(P, S, Z, xg.float(), None, counts, offs, precision=prec)
    old = lib.fql_tune_set_act_single_rows(0)
    try:
        got = ops.moe_forward_any(P, S, Z, xg, None, counts, offs, precision=prec, out_dtype=torch.float32)
    finally:
        lib.fql_tune_set_act_single_rows(old)
    assert same_bits(got, want) and not bits(got[-3:]).any()
    assert same_bits(ops.moe_forward_any(P, S, Z, xg, None, counts, offs, precision=prec, out_dtype=torch.float32), want)
