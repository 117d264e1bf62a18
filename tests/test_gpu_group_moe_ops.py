"""Per-group INT4 scales ([E, N, K / group_size]) through the grouped forward ops on the GPU: ``moe_forward``,
``moe_forward_any`` and ``moe_gated_forward`` (fql_moe_group_fwd / fql_moe_group_glu_fwd).

Integer path (csrc/fql_group_i8.h): E = 3, rows [40, 0, 9] plus 2 uncovered tail rows -- a ragged last row block and an
empty expert -- K = 512, group in {64, 128, 256}, N = 136 (ragged against the 128-column workgroup) and N = 70
(N % 4 != 0: scalar constant loads and stores).  Float path (csrc/fql_group.h, fql_generic.h between the two staging
kernels): rows [3, 0, 5], K = 192, group = 32.

  1. every precision against the float64 reference of the oracle (quantize_weights_grouped, reference_linear_grouped);
  2. 16-bit rows in and out: bit for bit the float32 call on the widened rows, rounded once;
  3. a per-expert bias: bit for bit out + bias[e] in float32, and added before the one rounding;
  4. rows no expert covers are exactly zero; the grouped call equals the one-expert calls bit for bit;
  5. the three activation kinds on gate|up rows [T, 2K] against tests/glu_reference.py.
Every test fails on a library without the feature: 3-D scales raise RuntimeError there."""
import functools

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from glu_reference import ALPHA, LIMIT, act_kw, hidden64
from helpers import (EXACT_REL_FRO, FAST_REL_FRO, FMA_REL_FRO, INT8_REL_FRO_LARGE_K, clipped_ranges, expert_table, ops,
                     rel_fro_dev, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 3
I8 = dict(counts=(40, 0, 9), K=512)          # 49 rows / 3 experts: the integer path
FL = dict(counts=(3, 0, 5), K=192)           # under 8 rows per expert, K % 256 != 0: the float32 kernels
GROUPS_I8 = [64, 128, 256]
NS = [136, 70]
PRECISIONS = [("exact", EXACT_REL_FRO), ("fast", FAST_REL_FRO), ("int8", INT8_REL_FRO_LARGE_K)]
DTYPES = [torch.bfloat16, torch.float16]
ALL_KINDS = ["silu", "gelu_tanh", "swiglu_clamp"]


@functools.lru_cache(maxsize=None)
def problem(counts, K, N, group):
    """Weights from the oracle's grouped quantiser, rows, gate|up rows, a bias and the float64 references; made once."""
    from oracle import oracle as O
    rng = np.random.default_rng(1000 * N + K + group)
    q = [O.quantize_weights_grouped(rng.standard_normal((N, K)).astype(np.float32) * 0.05, group) for _ in range(E)]
    W64 = [torch.from_numpy(O.dequantize_weights_grouped(*t).astype(np.float64)).to(DEV) for t in q]
    P, S, Z = (torch.from_numpy(np.stack([np.asarray(t[i]) for t in q])).to(DEV) for i in range(3))
    tpe, offs, T = expert_table(list(counts), tail=2)
    g = torch.Generator(device=DEV).manual_seed(N + group)
    x = torch.randn(T, K, device=DEV, generator=g)
    gate_up = 2.0 * torch.randn(T, 2 * K, device=DEV, generator=g)
    bias = torch.randn(E, N, device=DEV, generator=g)
    ranges = clipped_ranges(tpe.cpu(), offs.cpu(), T)
    return dict(P=P, S=S, Z=Z, W64=W64, tpe=tpe, offs=offs, T=T, x=x, gate_up=gate_up, bias=bias, ranges=ranges)


def ref64(p, rows64, bias=None):
    out = torch.zeros(p["T"], p["P"].shape[1], dtype=torch.float64, device=DEV)
    for e, (lo, hi) in enumerate(p["ranges"]):
        out[lo:hi] = rows64[lo:hi] @ p["W64"][e].t() + (0 if bias is None else bias[e].double())
    return out


def tail_is_zero(p, out):
    covered = torch.zeros(p["T"], dtype=torch.bool, device=DEV)
    for lo, hi in p["ranges"]:
        covered[lo:hi] = True
    assert int((~covered).sum()) == 2
    return torch.count_nonzero(out[~covered]) == 0


def weights(p):
    return p["P"], p["S"], p["Z"]


# ---- the integer path

@pytest.mark.parametrize("precision,bound", PRECISIONS, ids=[n for n, _ in PRECISIONS])
@pytest.mark.parametrize("group", GROUPS_I8)
@pytest.mark.parametrize("N", NS)
def test_forward_against_float64(N, group, precision, bound):
    p = problem(I8["counts"], I8["K"], N, group)
    got = ops().moe_forward(*weights(p), p["x"], None, p["tpe"], p["offs"], precision=precision)
    err = rel_fro_dev(got, ref64(p, p["x"].double()))
    print(f"ERR group fwd N={N} group={group} {precision}: {err:.3e} (bound {bound:.1e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == (p["T"], N)
    assert err < bound
    assert tail_is_zero(p, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("group", GROUPS_I8)
@pytest.mark.parametrize("N", NS)
def test_16bit_is_the_float32_call_rounded_once(N, group, dtype):
    p = problem(I8["counts"], I8["K"], N, group)
    x16 = p["x"].to(dtype)
    args = (None, p["tpe"], p["offs"])
    want32 = ops().moe_forward(*weights(p), x16.float(), *args)
    got = ops().moe_forward_any(*weights(p), x16, *args)
    assert got.dtype == dtype and same_bits(got, want32.to(dtype))
    assert same_bits(ops().moe_forward_any(*weights(p), x16, *args, out_dtype=torch.float32), want32)
    assert same_bits(ops().moe_forward_any(*weights(p), x16.float(), *args, out_dtype=dtype), want32.to(dtype))
    assert float(want32.abs().max()) > 0 and tail_is_zero(p, got)


@pytest.mark.parametrize("group", GROUPS_I8)
@pytest.mark.parametrize("N", NS)
def test_bias_is_added_in_float32_before_the_rounding(N, group):
    p = problem(I8["counts"], I8["K"], N, group)
    args = (None, p["tpe"], p["offs"])
    plain = ops().moe_forward(*weights(p), p["x"], *args)
    biased = ops().moe_forward(*weights(p), p["x"], *args, bias=p["bias"])
    assert tail_is_zero(p, biased)
    for dtype in DTYPES:
        x16 = p["x"].to(dtype)
        plain16 = ops().moe_forward(*weights(p), x16.float(), *args)
        got16 = ops().moe_forward_any(*weights(p), x16, *args, bias=p["bias"])
        assert got16.dtype == dtype and tail_is_zero(p, got16)
        for e, (lo, hi) in enumerate(p["ranges"]):
            assert same_bits(got16[lo:hi], (plain16[lo:hi] + p["bias"][e]).to(dtype)), (dtype, e)
    for e, (lo, hi) in enumerate(p["ranges"]):
        assert same_bits(biased[lo:hi], plain[lo:hi] + p["bias"][e]), e


@pytest.mark.parametrize("group", GROUPS_I8)
@pytest.mark.parametrize("N", NS)
def test_grouped_call_equals_the_one_expert_calls(N, group):
    p = problem(I8["counts"], I8["K"], N, group)
    P, S, Z = weights(p)
    got = ops().moe_forward(P, S, Z, p["x"], None, p["tpe"], p["offs"], bias=p["bias"])
    gated = ops().moe_gated_forward(P, S, Z, p["gate_up"], p["tpe"], p["offs"], activation="gelu_tanh")
    for e, (lo, hi) in enumerate(p["ranges"]):
        if hi == lo:
            continue
        one = expert_table([hi - lo])
        alone = ops().moe_forward(P[e:e + 1], S[e:e + 1], Z[e:e + 1], p["x"][lo:hi].contiguous(), None, one[0], one[1],
                                  bias=p["bias"][e:e + 1])
        assert same_bits(alone, got[lo:hi]), e
        alone = ops().moe_gated_forward(P[e:e + 1], S[e:e + 1], Z[e:e + 1], p["gate_up"][lo:hi].contiguous(), one[0], one[1],
                                        activation="gelu_tanh")
        assert same_bits(alone, gated[lo:hi]), e


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("group", GROUPS_I8)
@pytest.mark.parametrize("N", NS)
def test_glu_forward(N, group, kind):
    p = problem(I8["counts"], I8["K"], N, group)
    kw = act_kw(kind)
    got = ops().moe_gated_forward(*weights(p), p["gate_up"], p["tpe"], p["offs"], **kw)
    err = rel_fro_dev(got, ref64(p, hidden64(kind, p["gate_up"], ALPHA, LIMIT)))
    print(f"ERR group glu N={N} group={group} {kind}: {err:.3e}")
    assert got.dtype == torch.float32 and err < EXACT_REL_FRO and tail_is_zero(p, got)
    biased = ops().moe_gated_forward(*weights(p), p["gate_up"], p["tpe"], p["offs"], bias=p["bias"], **kw)
    for e, (lo, hi) in enumerate(p["ranges"]):
        assert same_bits(biased[lo:hi], got[lo:hi] + p["bias"][e]), e
    for dtype in DTYPES:
        gu16 = p["gate_up"].to(dtype)
        want32 = ops().moe_gated_forward(*weights(p), gu16.float(), p["tpe"], p["offs"], bias=p["bias"], **kw)
        got16 = ops().moe_gated_forward(*weights(p), gu16, p["tpe"], p["offs"], bias=p["bias"], **kw)
        assert got16.dtype == dtype and same_bits(got16, want32.to(dtype)) and tail_is_zero(p, got16)
        assert same_bits(ops().moe_gated_forward(*weights(p), gu16, p["tpe"], p["offs"], bias=p["bias"],
                                                 out_dtype=torch.float32, **kw), want32)


def test_fp8_and_malformed_triples_raise():
    p = problem(I8["counts"], I8["K"], 70, 64)
    P, S, Z = weights(p)
    args = (None, p["tpe"], p["offs"])
    with pytest.raises(RuntimeError, match="fp8"):
        ops().moe_forward(P, S, Z, p["x"], *args, precision="fp8")
    with pytest.raises(RuntimeError, match="fp8"):
        ops().moe_backward_input(P, S, Z, torch.zeros(p["T"], 70, device=DEV), p["tpe"], p["offs"], precision="fp8")
    with pytest.raises(RuntimeError, match="per-group scales and zero_points"):
        ops().moe_forward(P, S, Z[..., :4], p["x"], *args)
    with pytest.raises(RuntimeError, match="per-group scales and zero_points"):
        ops().moe_forward(P, S[..., :7], Z[..., :7], p["x"], *args)                    # 7 groups do not tile K = 512
    with pytest.raises(RuntimeError, match="scales must be float32 \\[num_experts, ffn_dim\\]"):
        ops().moe_forward(P, S[:, :, 0].reshape(-1), Z[:, :, 0], p["x"], *args)       # the per-row message of today
    # a last dimension of 1 is per-row: the kernels and the bits of the [E, N] call
    s1, z1 = S[:, :, :1].contiguous(), Z[:, :, :1].contiguous()
    assert same_bits(ops().moe_forward(P, s1, z1, p["x"], *args), ops().moe_forward(P, s1[..., 0], z1[..., 0], p["x"], *args))


# ---- the float32 kernels between the two staging kernels

@pytest.mark.parametrize("N", NS)
def test_float_path_forward_all_types(N):
    p = problem(FL["counts"], FL["K"], N, 32)
    args = (None, p["tpe"], p["offs"])
    for precision in ("exact", "int8"):                           # the precision does not enter the float32 arithmetic
        got = ops().moe_forward(*weights(p), p["x"], *args, precision=precision, bias=p["bias"])
        err = rel_fro_dev(got, ref64(p, p["x"].double(), p["bias"]))
        print(f"ERR group float fwd N={N} {precision}: {err:.3e}")
        assert err < FMA_REL_FRO and tail_is_zero(p, got)
    plain = ops().moe_forward(*weights(p), p["x"], *args)
    for e, (lo, hi) in enumerate(p["ranges"]):
        assert same_bits(got[lo:hi], plain[lo:hi] + p["bias"][e]), e
    for dtype in DTYPES:
        x16 = p["x"].to(dtype)
        want32 = ops().moe_forward(*weights(p), x16.float(), *args, bias=p["bias"])
        got16 = ops().moe_forward_any(*weights(p), x16, *args, bias=p["bias"])
        assert got16.dtype == dtype and same_bits(got16, want32.to(dtype)) and tail_is_zero(p, got16)
        assert same_bits(ops().moe_forward_any(*weights(p), x16, *args, bias=p["bias"], out_dtype=torch.float32), want32)
        assert same_bits(ops().moe_forward_any(*weights(p), x16.float(), *args, bias=p["bias"], out_dtype=dtype),
                         want32.to(dtype))


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("N", NS)
def test_float_path_glu_all_types(N, kind):
    p = problem(FL["counts"], FL["K"], N, 32)
    kw = act_kw(kind)
    got = ops().moe_gated_forward(*weights(p), p["gate_up"], p["tpe"], p["offs"], bias=p["bias"], **kw)
    err = rel_fro_dev(got, ref64(p, hidden64(kind, p["gate_up"], ALPHA, LIMIT), p["bias"]))
    print(f"ERR group float glu N={N} {kind}: {err:.3e}")
    assert got.dtype == torch.float32 and err < FMA_REL_FRO and tail_is_zero(p, got)
    for dtype in DTYPES:
        gu16 = p["gate_up"].to(dtype)
        want32 = ops().moe_gated_forward(*weights(p), gu16.float(), p["tpe"], p["offs"], bias=p["bias"], **kw)
        got16 = ops().moe_gated_forward(*weights(p), gu16, p["tpe"], p["offs"], bias=p["bias"], **kw)
        assert got16.dtype == dtype and same_bits(got16, want32.to(dtype)) and tail_is_zero(p, got16)
        assert same_bits(ops().moe_gated_forward(*weights(p), gu16, p["tpe"], p["offs"], bias=p["bias"],
                                                 out_dtype=torch.float32, **kw), want32)
