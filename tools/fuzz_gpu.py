#!/usr/bin/env python3
"""Randomised parity sweep of the product calls against the C oracle (run on a GPU box; not part of the test
suite: tests/ holds the fixed cases).  Exercises every dispatch branch: GEMV, generic, wide / short-row / decode
tiles, grouped and dense, the three precisions and the 16-bit I/O, and the tile / decode kernel pair of the MXFP4
experts' fp8 and fp4 precisions (forced either way, compared bit for bit)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, torch
import fused_int4_amd as fq
from fused_int4_amd import ops
from oracle import oracle as O, c_oracle as C
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = np.random.default_rng(2024)
TOL = {"exact": 2e-6, "fast": 3e-4, "int8": 2.5e-2}
worst = {}
def rel(a, b):
    d = np.linalg.norm(b.astype(np.float64)); return np.linalg.norm(a.astype(np.float64) - b) / (d if d else 1.0)
for case in range(n_cases):
    prec = ["exact", "fast", "int8"][case % 3]
    K = int(rng.choice([32, 64, 96, 256, 544, 768, 1024, 34, 4096])) if case % 7 else int(rng.integers(1, 40)) * 2
    N = int(rng.choice([5, 17, 64, 96, 200, 264, 1000, 1024]))
    grouped = case % 2 == 0
    if grouped:
        E = int(rng.choice([1, 2, 3, 8, 17, 70]))
        hi = int(rng.choice([3, 17, 40, 150]))
        counts = rng.integers(0, hi, size=E).astype(np.int32)
        if rng.random() < 0.3: counts[rng.integers(0, E)] = 0
        gap = int(rng.integers(0, 4))
        offs = (np.cumsum(counts) - counts).astype(np.int32)
        T = int(counts.sum()) + gap
        if T == 0: continue
        P, S, Z = [], [], []
        for e in range(E):
            p, s, z = O.quantize_weights((rng.standard_normal((N, K)) * 0.05).astype(np.float32))
            P.append(p); S.append(s); Z.append(z)
        P, S, Z = np.stack(P), np.stack(S), np.stack(Z)
        x = rng.standard_normal((T, K)).astype(np.float32)
        if case % 6 == 4 and prec != "int8":
            x[::3, rng.integers(0, K, size=1)] *= 600.0
        ref = C.moe_grouped(P, S, Z, x, counts, offs)
        d = lambda a: torch.from_numpy(a).cuda()
        out = ops.moe_forward(d(P), d(S), d(Z), d(x), None, d(counts), d(offs), precision=prec).cpu().numpy()
        key = f"moe/{prec}"
        if K % 32 == 0 and case % 4 == 0:
            h = ops.moe_forward_any(d(P), d(S), d(Z), d(x).half(), None, d(counts), d(offs), precision=prec)
            w = ops.moe_forward(d(P), d(S), d(Z), d(x).half().float(), None, d(counts), d(offs), precision=prec).half()
            assert torch.equal(h, w), ("f16 io", case, E, N, K, counts)
    else:
        B = int(rng.choice([1, 2, 3, 4, 5, 9, 16, 17, 33, 64, 130]))
        if case % 10 == 9:              # many tiles: more than one round of the persistent launch, uneven column tiles
            B, N, K = int(rng.choice([600, 1500, 2300])), int(rng.choice([3000, 5437, 6200])), int(rng.choice([64, 256]))
        p, s, z = O.quantize_weights((rng.standard_normal((N, K)) * 0.05).astype(np.float32))
        x = rng.standard_normal((B, K)).astype(np.float32)
        if case % 5 == 3 and prec != "int8":   # heavy-tailed rows: outlier channels (residual limb set)
            x[:, rng.integers(0, K, size=2)] *= float(rng.choice([50.0, 800.0]))
        ref = C.linear_f64acc(x, p, s, z)
        d = lambda a: torch.from_numpy(a).cuda()
        out = ops.linear_forward(d(x), d(p), d(s), d(z), precision=prec).cpu().numpy()
        key = f"linear/{prec}"
    if case % 8 == 5:                      # per-group scales along K: every dispatch branch of that path
        group = int(rng.choice([16, 32, 64, 128, 256]))
        Kg = int(rng.choice([256, 512, 768, 192, 64, 1024]))
        if Kg % group != 0:
            group = 64 if Kg % 64 == 0 else 32
        if group >= Kg:                    # (one group per row IS the per-row layout: not this path)
            group = Kg // 2
        Ng = int(rng.choice([5, 64, 130, 264]))
        Bg = int(rng.choice([1, 2, 3, 4, 9, 39, 40, 41, 100, 300]))
        wq = O.quantize_weights_grouped(rng.standard_normal((Ng, Kg)).astype(np.float32), group)
        xg = rng.standard_normal((Bg, Kg)).astype(np.float32)
        refg = O.reference_linear_grouped(xg, *wq)
        d = lambda a: torch.from_numpy(a).cuda()
        outg = ops.linear_forward(d(xg), d(wq[0]), d(wq[1]), d(wq[2]), precision=prec).cpu().numpy()
        int_path = Bg >= 40 and Kg % 256 == 0 and group % 64 == 0 and Ng >= 4
        tolg = TOL[prec] if int_path else 2e-6
        if int_path and prec == "int8" and outg.size < 2000:
            tolg = 6e-2
        rg = rel(outg, refg)
        worst[f"group/{prec if int_path else 'f32'}"] = max(worst.get(f"group/{prec if int_path else 'f32'}", 0.0), rg)
        assert rg < tolg, ("per-group", case, rg, Bg, Ng, Kg, group, prec)
    if case % 8 == 3:                      # MXFP4 experts, the block-scaled precisions: the tile and the decode kernel, same bits
        L = fq._native.lib()
        mode = 1 + (case // 8) % 2         # 1: fp8 rows, 2: MXFP4 rows
        Em, Km, Nm = int(rng.choice([1, 3, 8, 33])), 32 * int(rng.integers(1, 24)), int(rng.choice([5, 32, 37, 96, 130, 264]))
        cm = rng.integers(0, int(rng.choice([3, 17, 40, 70])), size=Em).astype(np.int32)
        om = (np.cumsum(cm) - cm).astype(np.int32)
        Tm = int(cm.sum()) + int(rng.integers(0, 4))
        if Tm:
            d = lambda a: torch.from_numpy(a).cuda()
            bm = d(rng.integers(0, 256, size=(Em, Nm, Km // 2)).astype(np.uint8))
            sm = d(rng.integers(110, 135, size=(Em, Nm, Km // 32)).astype(np.uint8))
            xm = d(rng.standard_normal((Tm, Km)).astype(np.float32))
            bias = d(rng.standard_normal((Em, Nm)).astype(np.float32)) if case % 16 < 8 else None
            old = L.fql_tune_set_mx4_scaled_decode_max_rows(mode, -1)
            res = []
            for rows in (0, 2 ** 31 - 1):
                L.fql_tune_set_mx4_scaled_decode_max_rows(mode, rows)
                assert L.fql_tune_mx4_scaled_kernel(mode, Em, Tm, Km, Nm) == (rows > 0)
                res.append(ops.moe_forward_mxfp4(bm, sm, xm, d(cm), d(om), bias=bias, precision=("fp8", "fp4")[mode - 1]))
            L.fql_tune_set_mx4_scaled_decode_max_rows(mode, old)
            assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)), ("mxfp4 scaled", case, mode, Em, Tm, Km, Nm, cm)
            worst[f"mxfp4-{('fp8', 'fp4')[mode - 1]}/tile!=decode"] = 0.0
    mfma = (K % 32 == 0) and (grouped or x.shape[0] > 2)
    tol = TOL[prec] if mfma else 2e-6
    if mfma and prec == "int8" and out.size < 2000:
        tol = 6e-2                      # 8-bit activations: few outputs -> the relative Frobenius error is noisy
    r = rel(out, ref)
    worst[key] = max(worst.get(key, 0.0), r)
    assert r < tol, (case, key, r, K, N, x.shape)
print("cases", n_cases, "worst relative error per path:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})
