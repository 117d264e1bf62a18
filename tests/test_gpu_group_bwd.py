"""The per-group input gradient on the GPU: ``moe_backward_input`` with scales [E, N, K / group_size]
(fql_moe_group_bwd_input, csrc/fql_group_bwd.h): dX[t] = dY[t] @ W_e with W_e = (q - zp[g(k)]) * s[g(k)].

Tables: rows [40, 0, 9] and [3, 0, 5], each plus 2 uncovered tail rows (a ragged 64-row tile, an empty expert, one wave
of a tile without a valid row).  (N, K) = (136, 512): 16-byte gradient loads, three stages of 64 n, the last ragged;
(70, 192): N % 4 != 0, element loads, a half-used 128-column tile; (33, 96): K % 64 != 0, the one-wave-per-row fallback,
which group = 48 (not a multiple of 32) reaches too.

  1. against the float64 dY @ W_deq of the oracle's dequantiser at FMA_REL_FRO;
  2. 16-bit gradients in and out: bit for bit the float32 call on the widened gradient, rounded once;
  3. two runs identical; the grouped call equals the one-expert calls; a permuted table gives the same rows;
  4. rows no expert covers are zero (the guard-band test hands the kernel a buffer full of sentinels);
  5. the fallback kernel runs the tiled kernel's chain of fmaf: the same bits from a gradient that is not 16-byte aligned.
Every test fails on a library without the feature: 3-D scales raise RuntimeError there."""
import functools

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from helpers import FMA_REL_FRO, clipped_ranges, expert_table, misaligned, ops, rel_fro_dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 3
TABLES = {"40-0-9": (40, 0, 9), "3-0-5": (3, 0, 5)}
SHAPES = [(136, 512, 64), (136, 512, 256), (70, 192, 32), (70, 192, 64), (33, 96, 32), (33, 96, 48)]    # N, K, group
IDS = [f"N{n}-K{k}-g{g}" for n, k, g in SHAPES]
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def problem(table, N, K, group):
    from oracle import oracle as O
    rng = np.random.default_rng(7 * N + K + group)
    q = [O.quantize_weights_grouped(rng.standard_normal((N, K)).astype(np.float32) * 0.05, group) for _ in range(E)]
    W64 = [torch.from_numpy(O.dequantize_weights_grouped(*t).astype(np.float64)).to(DEV) for t in q]
    P, S, Z = (torch.from_numpy(np.stack([np.asarray(t[i]) for t in q])).to(DEV) for i in range(3))
    tpe, offs, T = expert_table(list(TABLES[table]), tail=2)
    gy = torch.randn(T, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K))
    ranges = clipped_ranges(tpe.cpu(), offs.cpu(), T)
    ref = torch.zeros(T, K, dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(ranges):
        ref[lo:hi] = gy[lo:hi].double() @ W64[e]
    return dict(P=P, S=S, Z=Z, tpe=tpe, offs=offs, T=T, gy=gy, ranges=ranges, ref=ref)


def bwd(p, gy, **kw):
    return ops().moe_backward_input(p["P"], p["S"], p["Z"], gy, p["tpe"], p["offs"], **kw)


@pytest.mark.parametrize("N,K,group", SHAPES, ids=IDS)
@pytest.mark.parametrize("table", list(TABLES))
def test_against_float64_and_run_to_run(table, N, K, group):
    p = problem(table, N, K, group)
    got = bwd(p, p["gy"])
    err = rel_fro_dev(got, p["ref"])
    print(f"ERR group bwd {table} N={N} K={K} group={group}: {err:.3e} (bound {FMA_REL_FRO:.1e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == (p["T"], K)
    assert err < FMA_REL_FRO
    assert torch.count_nonzero(got[p["T"] - 2:]) == 0 and float(got.abs().max()) > 0
    assert same_bits(bwd(p, p["gy"]), got)
    assert same_bits(bwd(p, p["gy"], precision="int8"), got)       # the precision does not enter


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N,K,group", SHAPES[::2], ids=IDS[::2])
@pytest.mark.parametrize("table", list(TABLES))
def test_16bit_is_the_float32_call_rounded_once(table, N, K, group, dtype):
    p = problem(table, N, K, group)
    g16 = p["gy"].to(dtype)
    want32 = bwd(p, g16.float())
    got = bwd(p, g16, out_dtype=dtype)
    assert got.dtype == dtype and same_bits(got, want32.to(dtype))
    assert same_bits(bwd(p, g16), want32)                           # 16-bit in, float32 out (the default)
    assert same_bits(bwd(p, g16.float(), out_dtype=dtype), want32.to(dtype))
    assert torch.count_nonzero(got[p["T"] - 2:]) == 0 and float(want32.abs().max()) > 0


@pytest.mark.parametrize("N,K,group", SHAPES[::2], ids=IDS[::2])
@pytest.mark.parametrize("table", list(TABLES))
def test_grouped_equals_one_expert_calls_and_a_permuted_table(table, N, K, group):
    p = problem(table, N, K, group)
    got = bwd(p, p["gy"])
    for e, (lo, hi) in enumerate(p["ranges"]):
        if hi == lo:
            continue
        one = expert_table([hi - lo])
        gy = p["gy"][lo:hi].contiguous()
        alone = ops().moe_backward_input(p["P"][e:e + 1], p["S"][e:e + 1], p["Z"][e:e + 1], gy, one[0], one[1])
        assert same_bits(alone, got[lo:hi]), e
    perm = torch.tensor([2, 0, 1], device=DEV)
    permuted = ops().moe_backward_input(p["P"][perm].contiguous(), p["S"][perm].contiguous(), p["Z"][perm].contiguous(),
                                        p["gy"], p["tpe"][perm].contiguous(), p["offs"][perm].contiguous())
    assert same_bits(permuted, got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fallback_runs_the_tiled_kernels_chain(dtype):
    p = problem("40-0-9", 136, 512, 64)
    gy = p["gy"].to(dtype)
    tiled = bwd(p, gy)
    off = misaligned(gy, 1 if dtype == torch.float32 else 2)        # 4 bytes past a 16-byte boundary: one wave per row
    assert off.data_ptr() % 16 == 4 and torch.equal(off, gy)
    assert same_bits(bwd(p, off), tiled)
