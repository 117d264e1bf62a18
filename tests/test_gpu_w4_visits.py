"""GPU tests of the code AROUND the K loops of the one-wave-per-SIMD GEMM (csrc/fql_gemm_w4.h, tuning id 301): the
kernel's start and its tile table, the visit boundaries (per-row values and the next visit's scale / zero-point / bias
slice loaded at the start of a visit, one load per wave and round, used a K loop later) and the epilogue's store
paths.  One workgroup is made to walk every kind of visit sequence on small shapes: the
persistent grid is shrunk to 8 workgroups (tuning hook), and a model of the tile order (below) checks that the walks it
was built for are really there.  Every output must carry the bits of the 8-wave wide kernel (id 0) on the same limbs,
and sampled rows must be within the exact mode's constant of the float64 oracle.

Shapes: K in {512, 768} = 2 and 3 weight stages (both LDS buffer parities at a visit boundary); N = 352 = 11 fragments
(one 6- and one 5-fragment tile per row tile), N = 360 = 12 fragments with a ragged last one (8 columns)."""
import numpy as np
import pytest
import torch

from helpers import EXACT_REL_FRO, rel_fro
from oracle import oracle as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

CFG, WIDE, WGS, BM, NF, NTAB = 301, 0, 8, 128, 6, 16


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


# ---- the walks: a restatement of the tile order of csrc/fql_gemm_w4.h (row_groups, xcd_range_remap, tile_params) --------
def _upto(v, x):
    return 0 if v <= x else ((v - 1 - x) >> 3) + 1


def _remap(vb, lo, cnt):
    x = vb & 7
    return lo + sum(_upto(lo + cnt, xx) - _upto(lo, xx) for xx in range(x)) + _upto(vb, x) - _upto(lo, x)


def walks(counts, N, flagged, wgs=WGS):
    """Per workgroup the visits (fragments of the tile, rows, 'r' residual pass / 'm' main pass) in the order it makes
    them.  ``flagged`` [T] bool: rows with a residual set.  At N = 352 / 360 the plan has two column tiles, no
    alternative (a third tile would have fewer than 5 fragments)."""
    n_frag, n_tiles = (N + 31) // 32, 2
    assert (n_frag + NF - 1) // NF == n_tiles and n_frag // 3 < NF - 1
    f_base, f_rem = divmod(n_frag, n_tiles)
    offs = np.cumsum(counts) - np.asarray(counts)
    groups = ([], [], [])                                    # (first row, rows) of the row tiles: > 64 rows, 33..64, <= 32
    for c, o in zip(counts, offs):
        full, rem = divmod(int(c), BM)
        for s in range(full + (rem > 64)):
            groups[0].append((int(o) + s * BM, min(BM, int(c) - s * BM)))
        if 32 < rem <= 64:
            groups[1].append((int(o) + full * BM, rem))
        if 1 <= rem <= 32:
            groups[2].append((int(o) + full * BM, rem))
    sizes = [len(g) * n_tiles for g in groups]
    n_real = sum(sizes)
    assert n_real > wgs                                      # the launch has `wgs` workgroups
    out = []
    for b in range(wgs):
        visits = []
        for vb in range(b, n_real, wgs):
            grp = 0 if vb < sizes[0] else (1 if vb < sizes[0] + sizes[1] else 2)
            glo = sum(sizes[:grp])
            ms, nt = divmod(_remap(vb, glo, sizes[grp]) - glo, n_tiles)
            row0, rows = groups[grp][ms]
            nfr = f_base + (nt < f_rem)
            if flagged[row0:row0 + rows].any():
                visits.append((nfr, rows, "r"))
            visits.append((nfr, rows, "m"))
        out.append(visits)
    return out


def has_sequence(ws, *preds):
    """Some workgroup makes consecutive visits v0, v1, ... with preds[i](v_i)."""
    n = len(preds)
    return any(all(p(v) for p, v in zip(preds, w[i:i + n])) for w in ws for i in range(len(w) - n + 1))


def big(nfr):
    return lambda v: v[1] > 64 and v[0] == nfr


# counts per case (E experts; 0 = an empty expert), and what a workgroup's walk must contain
COUNTS_CLASSES = [168, 148, 192, 160, 40, 20, 33, 1, 0]      # 4 tiles of 128 rows, 4 tails of 33..64, 4 of <= 32: every workgroup walks one of each
COUNTS_BIG = [256, 128, 0, 384, 128, 256]                    # 9 row tiles of 128 rows = 18 tiles: 2 or 3 of alternating width per workgroup
COUNTS_MANY = [130, 40, 7, 0, 64, 33, 128, 1, 70] * 8        # 72 experts (two rounds of the 64-expert scan), 144 tiles: 18 per workgroup


def make_case(counts, N, K, seed, heavy_every=0):
    rng = np.random.default_rng(seed)
    E = len(counts)
    w = (rng.standard_normal((1, N, K)) * 0.02).astype(np.float32)
    q = [O.quantize_weights(np.roll(w[0], e, axis=0) * (1.0 + 0.01 * e)) for e in range(E)]
    P, S, Z = (np.stack([t[i] for t in q]) for i in range(3))
    cnt = np.asarray(counts, np.int32)
    offs = (np.cumsum(cnt) - cnt).astype(np.int32)
    T = int(cnt.sum())
    x = rng.standard_normal((T, K)).astype(np.float32)
    if heavy_every:
        for t in range(0, T, heavy_every):
            x[t, rng.choice(K, 2, replace=False)] *= 800.0
    return P, S, Z, x, cnt, offs


def run_pair(ops, lib, limbs, delta, rowsum, dP, dS, dZ, dc, do, E, T, K, N, **epi):
    """ids 0 and 301 at 8 workgroups; the previous grid size is restored."""
    dtype = epi.get("out_dtype") or torch.float32
    outs = {}
    old = lib.fql_tune_set_compute_units(WGS)
    try:
        for cfg in (WIDE, CFG):
            out = torch.full((T, N), float("nan"), dtype=dtype, device="cuda")
            rc = ops.tune_gemm_i8(cfg, limbs, delta, rowsum, dP, dS, dZ, dc, do, out, E, T, K, N, "exact", **epi)
            assert rc == 0, (cfg, rc)
            torch.cuda.synchronize()
            outs[cfg] = out
    finally:
        lib.fql_tune_set_compute_units(old)
    return outs[WIDE], outs[CFG]


def sample_rows(cnt, offs):
    """First, middle and last row of every expert that has rows."""
    rows = []
    for e, (c, o) in enumerate(zip(cnt.tolist(), offs.tolist())):
        rows += [(e, t) for t in sorted({o, o + c // 2, o + c - 1})] if c > 0 else []
    return rows


def oracle_rows(rows, P, S, Z, x, bias=None, rw=None):
    ref = np.stack([C.linear_f64acc(x[t][None], P[e], S[e], Z[e])[0] for e, t in rows]).astype(np.float64)
    if bias is not None:
        ref = ref + np.stack([bias[e] for e, _ in rows]).astype(np.float64)
    if rw is not None:
        ref = ref * np.asarray([rw[t] for _, t in rows], np.float64)[:, None]
    return ref


CASES = [
    # (counts, heavy_every, what some workgroup's walk must contain)
    ("classes", COUNTS_CLASSES, 0, [
        ("a 128-row tile, then a 33..64-row tail, then a tail of at most 32 rows",
         (lambda v: v[1] > 64, lambda v: 32 < v[1] <= 64, lambda v: v[1] <= 32))]),
    ("widths", COUNTS_BIG, 0, [
        ("6 -> 5 fragments", (big(6), big(NF - 1))), ("5 -> 6 fragments", (big(NF - 1), big(6)))]),
    ("residual", COUNTS_BIG, 37, [
        ("a residual pass followed by its main pass", (lambda v: v[2] == "r", lambda v: v[2] == "m")),
        ("5 -> 5 fragments", (big(NF - 1), big(NF - 1)))]),
    ("refill", COUNTS_MANY, 0, [
        ("more than 16 tiles in one workgroup", tuple([lambda v: v[2] == "m"] * (NTAB + 1)))]),
]


@pytest.mark.parametrize("K", [512, 768])
@pytest.mark.parametrize("N", [352, 360])
@pytest.mark.parametrize("name,counts,heavy,must", CASES, ids=[c[0] for c in CASES])
def test_visit_sequences_bit_identical_to_wide_kernel(fq, name, counts, heavy, must, N, K):
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    E = len(counts)
    P, S, Z, x, cnt, offs = make_case(counts, N, K, 31 * N + K + len(counts), heavy)
    T = x.shape[0]
    dP, dS, dZ, dx, dc, do = dev(P), dev(S), dev(Z), dev(x), dev(cnt), dev(offs)
    limbs, delta, rowsum = ops.act_quant(dx, precision="exact", tokens_per_expert=dc, input_offsets=do)
    flagged = (delta[1] != 0).cpu().numpy()
    assert bool(flagged.any()) == bool(heavy)
    ws = walks(counts, N, flagged)
    for what, preds in must:
        if "5 ->" in what or "6 ->" in what:
            if N != 352:                                     # N = 360: two tiles of 6 fragments, the second one ragged
                continue
        assert has_sequence(ws, *preds), f"the case was built for {what}: no workgroup walks it"
    wide, got = run_pair(ops, lib, limbs, delta, rowsum, dP, dS, dZ, dc, do, E, T, K, N)
    bad = (~(got == wide).all(dim=1)).nonzero().flatten().tolist()
    assert not bad, f"rows {bad[:8]} differ from the wide kernel"
    rows = sample_rows(cnt, offs)
    err = rel_fro(got[[t for _, t in rows]].cpu().numpy(), oracle_rows(rows, P, S, Z, x))
    print(f"{name} N={N} K={K}: {sum(len(w) for w in ws)} visits on {WGS} workgroups, sampled rows vs float64 oracle {err:.3e}")
    assert err < EXACT_REL_FRO


@pytest.mark.parametrize("N,K", [(352, 768), (360, 512)])
def test_visit_sequences_float16_bias_row_weight(fq, N, K):
    """The mixed-class walk once more through the rest of the epilogue: + bias, x row weight, float16 rows out.  Against
    the oracle the float16 rounding of an output comes on top of the exact mode's constant: 2^-11 relative per element
    in the normal range (outputs here are ~0.3 in magnitude; below 2^-14 the absolute error is at most 2^-25, nothing
    against the row norms), so at most 2^-11 in the Frobenius norm of a row sample."""
    from fused_int4_amd import ops, _native
    lib = _native.lib()
    counts = COUNTS_CLASSES
    E = len(counts)
    P, S, Z, x, cnt, offs = make_case(counts, N, K, 5 * N + K, 0)
    T = x.shape[0]
    rng = np.random.default_rng(N + K)
    bias = (rng.standard_normal((E, N)) * 0.1).astype(np.float32)
    rw = rng.uniform(0.25, 1.0, T).astype(np.float32)
    dP, dS, dZ, dx, dc, do = dev(P), dev(S), dev(Z), dev(x), dev(cnt), dev(offs)
    limbs, delta, rowsum = ops.act_quant(dx, precision="exact", tokens_per_expert=dc, input_offsets=do)
    wide, got = run_pair(ops, lib, limbs, delta, rowsum, dP, dS, dZ, dc, do, E, T, K, N,
                         out_dtype=torch.float16, bias=dev(bias), row_weight=dev(rw))
    assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16), wide.view(torch.int16))
    rows = sample_rows(cnt, offs)
    err = rel_fro(got[[t for _, t in rows]].float().cpu().numpy(), oracle_rows(rows, P, S, Z, x, bias, rw))
    print(f"float16 + bias + row weight N={N} K={K}: sampled rows vs float64 oracle {err:.3e}")
    assert err < EXACT_REL_FRO + 2.0 ** -11
