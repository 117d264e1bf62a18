"""Every compiled path of the INT4 input gradient (csrc/fql_bwd.h, fql_bwd.hip) against float64 torch references on the
GPU: dX = dY @ W64 with W64 the float64 dequantised weights (helpers.dequant_f64, no fql_* kernel).

Variants pinned here (fql_bwd.hip launch_bwd):
  * limbs L = 3 / 2 / 1 (exact or default / fast / int8 and fp8),
  * the weight stream: VW (K % 32 == 0, aligned: 16-byte loads) or the byte path (K = 130, 4098),
  * the pre-pass: vector rows (N % 16 == 0, aligned) with one row (few rows) or 4 rows per workgroup, or scalar rows,
  * the residual limb set of heavy-tailed rows (L >= 2),
  * linear (no table) and grouped (device expert table with gaps, empties, ranges past T, > 64 experts).
Every value test asserts the Frobenius bound of the mode and a per-row bound (helpers.row_rel_err)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import (EXACT_REL_FRO, ROW_TOL, act_limbs_reference, act_residual_reference, dequant_f64, expert_table, fq,
                     fro_tol, misaligned, ops, rel_fro_dev, row_rel_err)
from helpers import clipped_ranges as clamped

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREC = {3: "exact", 2: "fast", 1: "int8"}
LIM = {1: 127, 2: 127 * 256 + 127, 3: 127 * 65536 + 127 * 256 + 127}
FQL_BWD_MAX_N = 132104


def check(name, got, ref, L, N, rows=None, cond=None):
    """Frobenius and per-row bounds of mode L (``rows``: the rows the per-row bound applies to).  ``cond``: the rows'
    condition numbers (row_condition); the per-row bound is then scaled by max(1, cond_t)."""
    fro = rel_fro_dev(got, ref)
    if cond is not None:
        num = torch.linalg.vector_norm(got.double() - ref.double(), dim=1)
        den = torch.linalg.vector_norm(ref.double(), dim=1)
        assert (num[den == 0] == 0).all(), name
        e = (num / den.clamp_min(1e-300) / cond.clamp_min(1.0))[den > 0]
        if rows is not None:
            e = e[torch.isin(torch.nonzero(den > 0).flatten(), rows)]
        row = float(e.max())
        print(f"COND {name} median={float(cond.median()):.3g} max={float(cond.max()):.3g}")
    else:
        row = row_rel_err(got if rows is None else got[rows], ref if rows is None else ref[rows])
    print(f"ERR {name} L={L} fro={fro:.3e} row={row:.3e}")
    assert fro < fro_tol(L, N), (name, fro)
    assert row < ROW_TOL[L], (name, row)


def row_condition(gy, S, W):
    """cond_t = ||g_t|| ||Q||_F / (sqrt(N) ||g_t Q||), g_t = dY_t * s, Q = q - zp = W / s (float64): about 1 for a row
    whose result does not cancel, large for one that does.  The per-row bounds speak of the rounding of the gradient row
    relative to the row's own norm (csrc/fql_act_quant.h); an output row that cancels -- a zero point far
    from the centre of q whose common term sum_n g_n (c - zp_n) nearly vanishes for that row -- shows that error
    amplified by cond_t, whatever the arithmetic (float32 inputs alike)."""
    g = gy.double() * S.double()
    Q = W / S.double()[:, None]
    num = torch.linalg.vector_norm(g, dim=1) * torch.linalg.vector_norm(Q) / Q.shape[0] ** 0.5
    return num / torch.linalg.vector_norm(g @ Q, dim=1).clamp_min(1e-300)


def limb_image(g, L):
    """g_hat = delta * sum_l 256^l a_l: the pre-pass's rounding of the column-scaled rows g (helpers.act_limbs_reference,
    numpy), float64 on the device.  Without a residual set (L = 1) the kernel's dX is g_hat @ (q - zp) up to the float32
    rounding of its output."""
    d, delta, _ = act_limbs_reference(g.cpu().numpy(), L)
    X = sum(d[l].astype(np.float64) * 256.0 ** l for l in range(L))
    return torch.from_numpy(X * delta.astype(np.float64)[:, None]).to(DEV)


def no_outliers(g):
    """Rows of the column-scaled gradient without outliers (max |g_t| <= 5 rms(g_t)): the rows the L = 1 per-row bound
    speaks of (one 8-bit quantum per row, no residual set)."""
    rms = g.double().square().mean(1).sqrt()
    return (g.double().abs().amax(1) <= 5 * rms).nonzero().flatten()


def rand_weights(E, N, K, seed, zp="int"):
    """Random per-row INT4 weights [E, N, K/2] on the GPU: power-of-two-free scales in [0.005, 0.015); zero points
    integer in [0, 15] ("int": a mean of q - zp up to +-7.5 per channel, harder than quantize_weights), integer in
    [6, 9] ("centred": near the centre of q, as quantize_weights gives for symmetric rows) or "int" + U(-0.5, 0.5)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    P = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    S = 0.005 + 0.01 * torch.rand(E, N, device=DEV, generator=g)
    Z = torch.randint(0, 16, (E, N), device=DEV, generator=g).float()
    if zp == "centred":
        Z = torch.randint(6, 10, (E, N), device=DEV, generator=g).float()
    if zp == "frac":
        Z = Z + torch.rand(E, N, device=DEV, generator=g) - 0.5
    return P, S, Z


def grouped_ref(P, S, Z, gy, tpe, offs):
    """float64 dX of the grouped op, one expert dequantised at a time; rows no expert covers are 0."""
    T, K = gy.shape[0], 2 * P.shape[2]
    ref = torch.zeros(T, K, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clamped(tpe, offs, T)):
        if hi > lo:
            ref[lo:hi] = gy[lo:hi].double() @ dequant_f64(P[e], S[e], Z[e])
    return ref


def col_scaled(gy, S, tpe=None, offs=None):
    """g = dY * s[e] in float32 (the pre-pass's product) for the flag / outlier predicates."""
    if tpe is None:
        return gy * S.reshape(1, -1)
    g = torch.zeros_like(gy)
    for e, (lo, hi) in enumerate(clamped(tpe, offs, gy.shape[0])):
        g[lo:hi] = gy[lo:hi] * S[e]
    return g


# ---- 1. the headline shapes, both directions ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_size():
    """8 experts of quantised random weights for both directions of the FFN: 11008 -> 4096 and 4096 -> 11008."""
    out = {}
    g = torch.Generator(device=DEV).manual_seed(21)
    for N, K in ((11008, 4096), (4096, 11008)):
        P, S, Z = [], [], []
        for _ in range(8):
            p, s, z = fq().quantize_weights(torch.randn(N, K, device=DEV, generator=g) * 0.02)
            P.append(p); S.append(s); Z.append(z)
        out[(N, K)] = (torch.stack(P), torch.stack(S), torch.stack(Z))
    return out


@pytest.mark.parametrize("N,K", [(11008, 4096), (4096, 11008)])
def test_full_size_backward(full_size, N, K):
    P, S, Z = full_size[(N, K)]
    g = torch.Generator(device=DEV).manual_seed(22)
    for name, counts in (("balanced", [128] * 8), ("skewed", [485, 312, 126, 48, 30, 13, 6, 4])):
        tpe, offs, T = expert_table(counts)
        gy = torch.randn(T, N, device=DEV, generator=g)
        got = ops().moe_backward_input(P, S, Z, gy, tpe, offs)
        check(f"full {N}->{K} {name}", got, grouped_ref(P, S, Z, gy, tpe, offs), 3, N)
        for e in (0, 3):                                     # grouped == the linear op on the expert's rows, bitwise
            lo, c = int(offs[e]), counts[e]
            lin = ops().linear_backward_input(gy[lo:lo + c].contiguous(), P[e], S[e], Z[e])
            assert torch.equal(got[lo:lo + c], lin), (name, e)


# ---- 2. precision x weight path x form ----------------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 2, 1])
@pytest.mark.parametrize("K,N", [(4096, 1000), (256, 1024), (130, 5437), (4098, 1024)])
def test_limbs_paths_forms(L, K, N):
    """L in {1, 2, 3} x {VW: K = 4096, 256; byte loads: K = 130, 4098} x {linear, grouped with gaps}: every
    gemm_bwd_kernel<L, VW> instantiation; N = 1000 / 5437 take the scalar pre-pass, N = 1024 the vector one."""
    prec = PREC[L]
    # (L = 1: zero points near the centre of q; with a per-channel mean of q - zp up to +-7.5 the rank-one part of
    #  q - zp amplifies the 8-bit rounding of a row by up to ~2x in some rows -- the bitwise image check below holds
    #  for any zero points)
    P, S, Z = rand_weights(3, N, K, seed=L * 7 + K + N, zp="centred" if L == 1 else "int")
    g = torch.Generator(device=DEV).manual_seed(23 + L)
    gy = torch.randn(300, N, device=DEV, generator=g)
    got = ops().linear_backward_input(gy, P[0], S[0], Z[0], precision=prec)
    W0 = dequant_f64(P[0], S[0], Z[0])
    check(f"linear K={K} N={N}", got, gy.double() @ W0, L, N, no_outliers(col_scaled(gy, S[0])) if L == 1 else None)
    if L == 1:                  # every row is the exact integer product of its 8-bit image, float32-rounded once
        img = limb_image(col_scaled(gy, S[0]), 1) @ (W0 / S[0].double()[:, None])
        err = row_rel_err(got, img)
        print(f"ERR image linear K={K} N={N} row={err:.3e}")
        assert err < EXACT_REL_FRO

    tpe, offs, T = expert_table([37, 0, 150], gaps=[3, 0, 11], tail=5)
    gy = torch.randn(T, N, device=DEV, generator=g)
    got = ops().moe_backward_input(P, S, Z, gy, tpe, offs, precision=prec)
    ref = grouped_ref(P, S, Z, gy, tpe, offs)
    rows = no_outliers(col_scaled(gy, S, tpe, offs)) if L == 1 else None
    check(f"grouped K={K} N={N}", got, ref, L, N, rows)
    if L == 1:
        gh = limb_image(col_scaled(gy, S, tpe, offs), 1)
        img = torch.zeros_like(ref)
        for e, (lo, hi) in enumerate(clamped(tpe, offs, T)):
            img[lo:hi] = gh[lo:hi] @ (dequant_f64(P[e], S[e], Z[e]) / S[e].double()[:, None])
        err = row_rel_err(got, img)
        print(f"ERR image grouped K={K} N={N} row={err:.3e}")
        assert err < EXACT_REL_FRO
    covered = torch.zeros(T, dtype=torch.bool, device=DEV)
    for lo, hi in clamped(tpe, offs, T):
        covered[lo:hi] = True
    assert (got[~covered] == 0).all()
    if L == 1:                                               # fp8 layers take the same one-limb backward
        assert torch.equal(got, ops().moe_backward_input(P, S, Z, gy, tpe, offs, precision="fp8"))
        gl = gy[:64].contiguous()
        assert torch.equal(ops().linear_backward_input(gl, P[1], S[1], Z[1], precision="fp8"),
                           ops().linear_backward_input(gl, P[1], S[1], Z[1], precision="int8"))


# ---- 3. the residual limb set -------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("grouped", [False, True])
def test_residual_set_mixed_tiles(L, grouped):
    """Every 128-row tile mixes plain rows with rows made heavy (a) by dY outlier columns and (b) by column scales
    spanning 1e-4 .. 1e2 (dY of the plain rows is divided by s, so their g = dY s stays randn).  Every row meets the
    per-row bound; the plain rows are bitwise what they are when the heavy rows are replaced by plain ones."""
    N, K, T0 = 3000, 384, 300
    prec = PREC[L]
    g = torch.Generator(device=DEV).manual_seed(24 + L)
    E = 2 if grouped else 1
    P, S, Z = rand_weights(E, N, K, seed=25 + L, zp="frac")
    S = 10.0 ** (torch.rand(E, N, device=DEV, generator=g) * 4 - 4)       # 1e-4 .. 1 ...
    S[:, 1234] = 1e2                                                      # ... and one channel at 1e2
    tpe, offs, T = expert_table([130, T0 - 130], gaps=[0, 7]) if grouped else (None, None, T0)
    expert = torch.zeros(T, dtype=torch.long, device=DEV)
    if grouped:
        expert[int(offs[1]):] = 1
    plain = torch.randn(T, N, device=DEV, generator=g) / S[expert]
    gy = plain.clone()
    t = torch.arange(T, device=DEV)
    by_dy, by_s = t[t % 4 == 1], t[t % 4 == 3]
    gy[by_dy, 17] = 3e4 / S[expert[by_dy], 17]                           # (a) an outlier column of dY: g = 3e4
    gy[by_s] = torch.randn(len(by_s), N, device=DEV, generator=g)        # (b) g = randn * s: the scales' range,
    gy[by_s, 1234] = 3.0                                                  #     g = 300 on the 1e2 channel
    if grouped:
        got = ops().moe_backward_input(P, S, Z, gy, tpe, offs, precision=prec)
        base = ops().moe_backward_input(P, S, Z, plain, tpe, offs, precision=prec)
        ref = grouped_ref(P, S, Z, gy, tpe, offs)
    else:
        got = ops().linear_backward_input(gy, P[0], S[0], Z[0], precision=prec)
        base = ops().linear_backward_input(plain, P[0], S[0], Z[0], precision=prec)
        ref = gy.double() @ dequant_f64(P[0], S[0], Z[0])
    # the rows are on the intended side of the flag, clearly (helpers.act_residual_reference)
    flag = act_residual_reference(col_scaled(gy, S, tpe, offs).cpu().numpy() if grouped
                                  else col_scaled(gy, S[0]).cpu().numpy(), L)[0]
    heavy = np.zeros(T, bool)
    heavy[by_dy.cpu().numpy()] = heavy[by_s.cpu().numpy()] = True
    if grouped:
        heavy[130:137] = False                                            # (the gap rows: no expert, no flag)
    assert (flag == heavy).all(), np.nonzero(flag != heavy)
    check(f"residual {'grouped' if grouped else 'linear'}", got, ref, L, N)
    keep = torch.from_numpy(~heavy).to(DEV)
    assert torch.equal(got[keep], base[keep])


# ---- 4. row independence (fql_bwd.h: "a row's result does not depend on the tile shape or on the other rows") -------

@pytest.mark.parametrize("zp", ["int", "frac"])
@pytest.mark.parametrize("N", [1000, 1024])
def test_row_independence(N, zp):
    """The same 9 gradient rows at offsets 0, 1, 31 and 127 of a 256-row matrix (other rows random, different each
    time): bitwise equal dX, linear and grouped (the expert starts at the offset; expert 0 holds the rows before it).
    With fractional zero points the float correction sum_n g f is summed in a fixed per-row order too.  (Between pre-pass
    variants -- one row or 4 rows per workgroup, chosen by the number of rows, or the scalar rows of an unaligned dY --
    the threads split a row's n differently, so the correction's float sum, and with it the last bits, may differ; with
    integer zero points the correction is 0 and those variants agree bit for bit as well: test_misaligned_grad_out.)"""
    K, T = 512, 256
    P, S, Z = rand_weights(2, N, K, seed=26, zp=zp)
    g = torch.Generator(device=DEV).manual_seed(27)
    rows = torch.randn(9, N, device=DEV, generator=g)
    rows[4, 100] *= 1e4                                      # one heavy-tailed row among them
    lin, grp = [], []
    for o in (0, 1, 31, 127):
        gy = torch.randn(T, N, device=DEV, generator=g)
        gy[o:o + 9] = rows
        lin.append(ops().linear_backward_input(gy, P[1], S[1], Z[1])[o:o + 9])
        counts = [o, T - o] if o else [0, T]
        tpe = torch.tensor(counts, dtype=torch.int32, device=DEV)
        offs = torch.tensor([0, o], dtype=torch.int32, device=DEV)
        grp.append(ops().moe_backward_input(P, S, Z, gy, tpe, offs)[o:o + 9])
    for a in lin[1:] + grp:
        assert torch.equal(a, lin[0])
    check(f"row independence {zp}", lin[0], rows.double() @ dequant_f64(P[1], S[1], Z[1]), 3, N)


# ---- 5. zero points at and past the clamp of the integer image ----------------------------------------------------

ZPS = {"+112": 112.0, "-112": -112.0, "-113": -113.0, "150": 150.0, "-300": -300.0, "111.6": 111.6, "-111.6": -111.6,
       "112.4": 112.4, "-112.4": -112.4, "-112.5": -112.5, "112.6": 112.6}


@pytest.mark.parametrize("L", [3, 2])
def test_zero_points_at_and_past_the_clamp(L):
    """z = clamp(rint(zp), -112, 112) goes into the int8 image, f = zp - z through the float correction: each value on
    its own, then all of them mixed over the channels of one matrix (linear and grouped).  Zero points this far from
    the centre of q make rows whose result cancels (row_condition): the per-row bound is scaled by their condition."""
    N, K, B = 1000, 256, 96
    P, S, _ = rand_weights(2, N, K, seed=28)
    g = torch.Generator(device=DEV).manual_seed(29)
    gy = torch.randn(B, N, device=DEV, generator=g)
    for name, v in ZPS.items():
        Z = torch.full((N,), v, device=DEV)
        got = ops().linear_backward_input(gy, P[0], S[0], Z, precision=PREC[L])
        W = dequant_f64(P[0], S[0], Z)
        check(f"zp {name}", got, gy.double() @ W, L, N, cond=row_condition(gy, S[0], W))
    vals = torch.tensor(list(ZPS.values()) + [3.0, 7.25], device=DEV)
    Zm = vals[torch.randint(0, len(vals), (2, N), device=DEV, generator=g)]
    got = ops().linear_backward_input(gy, P[0], S[0], Zm[0], precision=PREC[L])
    W = dequant_f64(P[0], S[0], Zm[0])
    check("zp mixed", got, gy.double() @ W, L, N, cond=row_condition(gy, S[0], W))
    tpe, offs, T = expert_table([40, 50], gaps=[2, 1])
    gy2 = torch.randn(T, N, device=DEV, generator=g)
    got = ops().moe_backward_input(P, S, Zm, gy2, tpe, offs, precision=PREC[L])
    cond = torch.ones(T, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clamped(tpe, offs, T)):
        cond[lo:hi] = row_condition(gy2[lo:hi], S[e], dequant_f64(P[e], S[e], Zm[e]))
    check("zp mixed grouped", got, grouped_ref(P, S, Zm, gy2, tpe, offs), L, N, cond=cond)


def test_integer_bit_exact_at_the_clamp_ends():
    """Integer dY, power-of-two scales, zero points at the ends of the clamp: q - z reaches 127 (q = 15, z = -112) and
    -112 (q = 0, z = 112); the result is an exact integer combination and must equal int64 arithmetic bit for bit."""
    rng = np.random.default_rng(30)
    for (B, N, K) in [(64, 1000, 4096), (33, 257, 130)]:
        q = rng.integers(0, 16, size=(N, K))
        z = rng.choice([-112.0, 112.0, 0.0, 15.0], size=N).astype(np.float32)
        q[z == -112.0] = 15                                  # q - z = 127
        q[z == 112.0] = 0                                    # q - z = -112
        s = (2.0 ** rng.integers(-3, 2, size=N)).astype(np.float32)
        gy = rng.integers(-15, 16, size=(B, N)).astype(np.float32)
        packed = torch.from_numpy((q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8))
        got = ops().linear_backward_input(torch.from_numpy(gy).to(DEV), packed.to(DEV), torch.from_numpy(s).to(DEV),
                                          torch.from_numpy(z).to(DEV)).cpu().numpy()
        ref = (gy.astype(np.int64) * (s * 8).astype(np.int64)[None, :]) @ (q - z.astype(np.int64)[:, None])
        assert np.array_equal(got, (ref / 8.0).astype(np.float32)), (B, N, K)


# ---- 6. the i32 bound ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 2])
def test_i32_bound_at_max_n(L):
    """N = FQL_BWD_MAX_N with every limb at magnitude 127 (g = +-LIM 2^e) against q - z = 127 and -112: every inner dot
    product sits just under 2^31.  A wrap would be off by ~100 %."""
    N, K = FQL_BWD_MAX_N, 64
    g = torch.Generator(device=DEV).manual_seed(31)
    S = 2.0 ** torch.randint(-6, 3, (N,), device=DEV, generator=g).float()
    rows = torch.stack([torch.full((N,), float(LIM[L]) * 2.0 ** -10, device=DEV),
                        torch.full((N,), -float(LIM[L]) * 2.0 ** 4, device=DEV),
                        torch.randn(N, device=DEV, generator=g)])
    digits = act_limbs_reference(rows[:2].cpu().numpy(), L)[0]
    assert np.isin(np.abs(digits), (127, 128)).all()
    gy = rows / S                                            # exact: g = dY * s gives the rows back
    for q_val, zp in ((15, -112.0), (0, 112.0)):
        P = torch.full((N, K // 2), q_val | (q_val << 4), dtype=torch.uint8, device=DEV)
        Z = torch.full((N,), zp, device=DEV)
        got = ops().linear_backward_input(gy, P, S, Z, precision=PREC[L])
        ref = gy.double() @ dequant_f64(P, S, Z)
        check(f"i32 bound q={q_val} zp={zp}", got, ref, L, N)


# ---- 7. special rows ------------------------------------------------------------------------------------------------

def test_special_rows():
    """A zero dY row gives an exactly zero dX row; a NaN or Inf in a dY row makes that dX row NaN and leaves the other
    rows of its tile bitwise unchanged; channels with scale 0 contribute nothing (bitwise: as if dY were 0 there)."""
    N, K, T = 1000, 512, 200
    P, S, Z = rand_weights(2, N, K, seed=32, zp="frac")
    g = torch.Generator(device=DEV).manual_seed(33)
    gy = torch.randn(T, N, device=DEV, generator=g)
    gy[7] = 0.0
    gy[40, 3] = float("nan")
    gy[41, 999] = float("inf")
    gy[42, 0] = -float("inf")
    clean = gy.clone()
    clean[40:43] = torch.randn(3, N, device=DEV, generator=g)
    tpe, offs, _ = expert_table([100, 100])
    for name, run in (("linear", lambda x: ops().linear_backward_input(x, P[0], S[0], Z[0])),
                      ("grouped", lambda x: ops().moe_backward_input(P, S, Z, x, tpe, offs))):
        got, base = run(gy), run(clean)
        assert (got[7] == 0).all(), name
        assert torch.isnan(got[40:43]).all(), name
        others = torch.ones(T, dtype=torch.bool, device=DEV)
        others[40:43] = False
        assert torch.equal(got[others], base[others]), name
    S0 = S.clone()
    S0[:, 10::7] = 0.0
    big = clean.clone()
    big[:, 10::7] = 1e30
    zeroed = clean.clone()
    zeroed[:, 10::7] = 0.0
    got = ops().linear_backward_input(big, P[0], S0[0], Z[0])
    assert torch.equal(got, ops().linear_backward_input(zeroed, P[0], S0[0], Z[0]))
    check("zero scales", got, zeroed.double() @ dequant_f64(P[0], S0[0], Z[0]), 3, N)
    got = ops().moe_backward_input(P, S0, Z, big, tpe, offs)
    assert torch.equal(got, ops().moe_backward_input(P, S0, Z, zeroed, tpe, offs))


# ---- 8. expert tables ------------------------------------------------------------------------------------------------

def bwd_abi(P, S, Z, gy, tpe, offs, guard=8, precision=0):
    """fql_moe_bwd_input_f32 into a [T + guard, K] buffer whose guard rows hold a sentinel; returns the buffer."""
    lib = fq()._native.lib()
    E, N, K2 = P.shape
    T, K = gy.shape[0], 2 * K2
    out = torch.full((T + guard, K), -7.5, device=DEV)
    nbytes = lib.fql_moe_bwd_workspace_bytes(E, T, K, N, precision)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.fql_moe_bwd_input_f32(P.data_ptr(), S.data_ptr(), Z.data_ptr(), gy.data_ptr(), tpe.data_ptr(),
                                   offs.data_ptr(), out.data_ptr(), E, T, K, N, precision, ws.data_ptr(),
                                   ctypes.c_size_t(nbytes), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("case", ["gaps", "130_experts", "past_T"])
def test_expert_tables(case):
    N, K = 200, 256
    g = torch.Generator(device=DEV).manual_seed(34)
    if case == "gaps":
        tpe, offs, T = expert_table([50, 70, 0, 33], gaps=[4, 9, 3, 1], tail=6)
    elif case == "130_experts":
        counts = torch.randint(0, 6, (130,), generator=torch.Generator().manual_seed(35))
        counts[::9] = 0
        gaps = torch.randint(0, 3, (130,), generator=torch.Generator().manual_seed(36))
        tpe, offs, T = expert_table(counts.tolist(), gaps.tolist(), tail=2)
    else:                                                    # ranges leaving [0, T): clipped on the device
        T = 60
        tpe = torch.tensor([8, 6, 10, 999, 5, 3], dtype=torch.int32, device=DEV)
        offs = torch.tensor([-4, 4, 12, 30, T + 3, 25], dtype=torch.int32, device=DEV)
    E = tpe.numel()
    P, S, Z = rand_weights(E, N, K, seed=37, zp="frac")
    gy = torch.randn(T, N, device=DEV, generator=g)
    ref = grouped_ref(P, S, Z, gy, tpe, offs)
    got = ops().moe_backward_input(P, S, Z, gy, tpe, offs)
    check(f"table {case}", got, ref, 3, N)
    covered = torch.zeros(T, dtype=torch.bool, device=DEV)
    for lo, hi in clamped(tpe, offs, T):
        covered[lo:hi] = True
    assert (~covered).any() and (got[~covered] == 0).all()
    buf = bwd_abi(P, S, Z, gy, tpe, offs)
    assert torch.equal(buf[:T], got)
    assert (buf[T:] == -7.5).all()                           # guard rows after T untouched


# ---- 9. unaligned grad_out ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("floats", [1, 2, 3])
def test_misaligned_grad_out(floats):
    """N % 16 == 0 with dY 4 / 8 / 12 bytes off a 16-byte boundary: the scalar pre-pass.  With integer zero points it
    is bitwise the aligned (vector, one-row) pre-pass; with fractional ones within the bound."""
    N, K, T = 1024, 512, 64
    P, S, Z = rand_weights(2, N, K, seed=38)
    g = torch.Generator(device=DEV).manual_seed(39)
    gy = torch.randn(T, N, device=DEV, generator=g)
    gy[5, 77] *= 1e5                                         # a heavy row as well
    gm = misaligned(gy, floats)
    assert torch.equal(ops().linear_backward_input(gm, P[0], S[0], Z[0]),
                       ops().linear_backward_input(gy, P[0], S[0], Z[0]))
    tpe, offs, _ = expert_table([20, 44])
    assert torch.equal(ops().moe_backward_input(P, S, Z, gm, tpe, offs), ops().moe_backward_input(P, S, Z, gy, tpe, offs))
    Zf = Z + 0.25
    got = ops().linear_backward_input(gm, P[0], S[0], Zf[0])
    check(f"misaligned {floats} frac zp", got, gy.double() @ dequant_f64(P[0], S[0], Zf[0]), 3, N)


# ---- 10. 16-bit activations, and the modules at L = 2 -------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_input_gradients(dtype):
    """x.grad of linear_forward_any / moe_forward_any is the float32 backward of the float32 gradient, rounded once to
    the activations' dtype: bitwise, and within that rounding (plus the exact-mode bound) of float64."""
    N, K = 1000, 512
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    P, S, Z = rand_weights(3, N, K, seed=40)
    g = torch.Generator(device=DEV).manual_seed(41)
    x = torch.randn(70, K, device=DEV, generator=g).to(dtype).requires_grad_()
    gy = torch.randn(70, N, device=DEV, generator=g).to(dtype)
    ops().linear_forward_any(x, P[0], S[0], Z[0]).backward(gy)
    want = ops().linear_backward_input(gy.float(), P[0], S[0], Z[0])
    assert torch.equal(x.grad, want.to(dtype))
    ref = gy.double() @ dequant_f64(P[0], S[0], Z[0])
    fro, err = rel_fro_dev(x.grad, ref), row_rel_err(x.grad, ref)
    print(f"ERR 16-bit linear {dtype} fro={fro:.3e} row={err:.3e}")
    assert fro < u + EXACT_REL_FRO and err < u + EXACT_REL_FRO

    tpe, offs, T = expert_table([20, 0, 37], gaps=[1, 0, 2], tail=3)
    x = torch.randn(T, K, device=DEV, generator=g).to(dtype).requires_grad_()
    gy = torch.randn(T, N, device=DEV, generator=g).to(dtype)
    ops().moe_forward_any(P, S, Z, x, None, tpe, offs).backward(gy)
    want = ops().moe_backward_input(P, S, Z, gy.float(), tpe, offs)
    assert torch.equal(x.grad, want.to(dtype))
    ref = grouped_ref(P, S, Z, gy.float(), tpe, offs)
    fro, err = rel_fro_dev(x.grad, ref), row_rel_err(x.grad, ref)
    print(f"ERR 16-bit grouped {dtype} fro={fro:.3e} row={err:.3e}")
    assert fro < u + EXACT_REL_FRO and err < u + EXACT_REL_FRO


def test_modules_fast_precision():
    """MoEINT4 and QuantizedMoEFFN with precision='fast': x.grad within the FAST bounds of float64."""
    E, H, F = 3, 256, 384
    torch.manual_seed(42)
    tpe, offs, T = expert_table([30, 0, 50], gaps=[0, 0, 2], tail=1)
    m = fq().MoEINT4.from_weights([torch.randn(F, H) * 0.05 for _ in range(E)], precision="fast").to(DEV)
    x = torch.randn(T, H, device=DEV, requires_grad=True)
    gy = torch.randn(T, F, device=DEV)
    m(x, None, tpe, offs).backward(gy)
    check("MoEINT4 fast", x.grad, grouped_ref(m.packed_weights, m.scales, m.zero_points, gy, tpe, offs), 2, F)

    gate = [torch.randn(F, H) * 0.1 for _ in range(E)]
    up = [torch.randn(F, H) * 0.1 for _ in range(E)]
    down = [torch.randn(H, F) * 0.1 for _ in range(E)]
    ffn = fq().QuantizedMoEFFN.from_weights(gate, up, down, precision="fast").to(DEV)
    x = torch.randn(T, H, dtype=torch.float64, device=DEV)
    gy = torch.randn(T, H, dtype=torch.float64, device=DEV)
    xg = x.float().requires_grad_()
    ffn(xg, tpe, offs).backward(gy.float())
    ref = torch.zeros(T, H, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(clamped(tpe, offs, T)):
        if hi == lo:
            continue
        Wgu = dequant_f64(ffn.gate_up_packed[e], ffn.gate_up_scales[e], ffn.gate_up_zero_points[e])
        Wd = dequant_f64(ffn.down_packed[e], ffn.down_scales[e], ffn.down_zero_points[e])
        xe = x[lo:hi].clone().requires_grad_()
        gu = xe @ Wgu.T
        (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:] @ Wd.T).backward(gy[lo:hi])
        ref[lo:hi] = xe.grad
    check("QuantizedMoEFFN fast", xg.grad, ref, 2, F)
