"""Per-group INT4 scales in the MoE experts, the part that needs no GPU: the C ABI of FQL_VERSION 330
(fql_moe_group_fwd, fql_moe_group_glu_fwd, fql_moe_group_bwd_input and their workspace queries: declared, exported and
validated in the documented order before any HIP call -- every call below is invalid, empty or stops at the workspace
check, so none launches) and ``group_size`` in QuantizedMoEFFN, LoRAQuantizedMoEFFN and QuantizedSparseMoEBlock."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_group_typed_workspace_bytes", "fql_moe_group_fwd", "fql_moe_group_glu_fwd",
       "fql_moe_group_bwd_workspace_bytes", "fql_moe_group_bwd_input")
OK, NULLP, SHAPE, ODD_K, WS, PREC, ALIGN, DTYPE = 0, -1, -2, -3, -4, -6, -7, -8
F32, F16, BF16 = 0, 1, 2
FP8 = 8
SILU, GELU, CLAMP = 0, 1, 2
NAN = float("nan")
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, group=32, prec=0, pk=P, sc=P, zp=P, x=P, tpe=P, offs=P, bias=P,
         out=P2, ws=None, nbytes=0):
    return lib.fql_moe_group_fwd(pk, sc, zp, x, di, tpe, offs, bias, out, do, E, T, K, N, group, prec, ws, nbytes, None)


def _glu(lib, act=CLAMP, alpha=1.702, limit=7.0, di=F32, do=F32, E=2, T=8, K=64, N=96, group=32, prec=0, pk=P, sc=P, zp=P,
         x=P, tpe=P, offs=P, bias=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_group_glu_fwd(pk, sc, zp, x, di, tpe, offs, bias, out, do, E, T, K, N, group, prec, act, alpha, limit,
                                     ws, nbytes, None)


def _bwd(lib, di=F32, do=F32, E=2, T=8, K=64, N=96, group=32, pk=P, sc=P, zp=P, gy=P, tpe=P, offs=P, gx=P2):
    return lib.fql_moe_group_bwd_input(pk, sc, zp, gy, di, tpe, offs, gx, do, E, T, K, N, group, None, 0, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 330


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "size_t (*q)(int, int, int, int, int, int) = fql_moe_group_typed_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, const float *, void *, int, int, int, int, int, int, int, void *, size_t,\n"
                    "         void *) = fql_moe_group_fwd;\n"
                    "int (*b)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, const float *, void *, int, int, int, int, int, int, int, int, float, float,\n"
                    "         void *, size_t, void *) = fql_moe_group_glu_fwd;\n"
                    "size_t (*r)(int, int, int, int, int) = fql_moe_group_bwd_workspace_bytes;\n"
                    "int (*c)(const uint8_t *, const float *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, void *, size_t, void *)\n"
                    "    = fql_moe_group_bwd_input;\n"
                    "int version_is_330[FQL_VERSION >= 330 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_workspace_queries(lib):
    q = lib.fql_moe_group_typed_workspace_bytes
    E, T, K, N = 3, 51, 512, 136
    stage = (T * K * 4 + 15) // 16 * 16 + (T * N * 4 + 15) // 16 * 16
    for prec in (0, 1, 2, 3):
        for group in (64, 128, 256):
            got = q(E, T, K, N, group, prec)
            assert got >= lib.fql_group_workspace_bytes(E, T, K, N, group, prec) > 0      # the integer path's need
            assert got >= stage and got % 16 == 0                                         # ... and the float path's staging
    assert q(3, 8, 80, 70, 40, 0) == (8 * 80 * 4 + 15) // 16 * 16 + (8 * 70 * 4 + 15) // 16 * 16     # K % 32 != 0: staging only
    for bad in ((0, T, K, N, 64, 0), (E, 0, K, N, 64, 0), (E, T, 0, N, 64, 0), (E, T, K, 0, 64, 0), (E, T, K, N, 0, 0),
                (E, T, K, N, 96, 0), (E, T, K, N, 64, FP8), (E, T, K, N, 64, 5)):
        assert q(*bad) == 0, bad
    assert lib.fql_moe_group_bwd_workspace_bytes(E, T, K, N, 64) == 0                     # documented: none needed


@pytest.mark.parametrize("call", [_fwd, _glu], ids=["fwd", "glu"])
def test_forward_argument_errors_in_order(lib, call):
    assert call(lib, prec=5) == PREC
    assert call(lib, prec=FP8) == PREC
    assert call(lib, prec=5, T=-1) == PREC                         # the precision comes first
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-2), dict(N=-1)):
        assert call(lib, **kw) == SHAPE, kw
    assert call(lib, K=65, group=5) == ODD_K                       # odd K before the group
    for group in (0, -32, 31, 48):                                 # not positive, odd, does not tile K = 64
        assert call(lib, group=group) == SHAPE, group
    assert call(lib, di=9) == DTYPE
    assert call(lib, do=3) == DTYPE
    assert call(lib, di=9, group=48) == SHAPE                      # the group before the types
    assert call(lib, T=0, pk=None) == OK                           # the empty call before the pointers
    assert call(lib, N=0, out=None) == OK
    for kw in (dict(pk=None), dict(sc=None), dict(zp=None), dict(x=None), dict(out=None), dict(tpe=None), dict(offs=None)):
        assert call(lib, **kw) == NULLP, kw
    assert call(lib, tpe=None, offs=None) == SHAPE                 # no table: one segment, E == 1 only
    assert call(lib, E=70000) == SHAPE
    assert call(lib, di=BF16, x=P_BYTE) == ALIGN
    assert call(lib, do=F16, out=P_BYTE) == ALIGN
    assert call(lib, di=F32, x=P_HALF) == ALIGN
    # off the integer path (K % 256 != 0) something is staged: a missing, misaligned or short workspace
    assert call(lib, di=BF16, do=BF16) == WS
    assert call(lib, di=BF16, do=BF16, ws=ctypes.c_void_p(24), nbytes=1 << 30) == WS
    assert call(lib, di=BF16, do=BF16, ws=P, nbytes=8 * 64 * 4 + 8 * 96 * 4 - 16) == WS


def test_glu_activation_errors(lib):
    assert _glu(lib, act=3) == SHAPE
    assert _glu(lib, act=-1) == SHAPE
    for kw in (dict(alpha=NAN), dict(limit=NAN), dict(limit=0.0), dict(limit=-1.0), dict(alpha=float("inf"))):
        assert _glu(lib, act=CLAMP, **kw) == SHAPE, kw
        assert _glu(lib, act=GELU, **kw) == SHAPE, kw
        assert _glu(lib, act=SILU, T=0, **kw) == OK, kw            # silu ignores its two floats
    assert _glu(lib, act=3, K=65) == SHAPE                         # the activation before odd K
    assert _glu(lib, act=3, prec=5) == PREC


def test_backward_argument_errors_in_order(lib):
    for kw in (dict(E=0), dict(T=-1), dict(K=-2), dict(N=-1)):
        assert _bwd(lib, **kw) == SHAPE, kw
    assert _bwd(lib, K=65, group=5) == ODD_K
    for group in (0, -32, 31, 48):
        assert _bwd(lib, group=group) == SHAPE, group
    assert _bwd(lib, di=9) == DTYPE
    assert _bwd(lib, do=3) == DTYPE
    assert _bwd(lib, T=0, gx=None) == OK
    assert _bwd(lib, K=0, group=0, gx=None) == OK                  # no column: nothing to write, no group to check
    assert _bwd(lib, gx=None) == NULLP
    for kw in (dict(pk=None), dict(sc=None), dict(zp=None), dict(gy=None), dict(tpe=None), dict(offs=None)):
        assert _bwd(lib, **kw) == NULLP, kw
    assert _bwd(lib, tpe=None, offs=None) == SHAPE                 # no table: E == 1 only
    assert _bwd(lib, E=65535) == SHAPE
    assert _bwd(lib, di=BF16, gy=P_BYTE) == ALIGN
    assert _bwd(lib, do=F16, gx=P_BYTE) == ALIGN
    assert _bwd(lib, gy=P_HALF) == ALIGN
    assert _bwd(lib, sc=P_HALF) == ALIGN


# ---- the layers

E, H, F = 3, 128, 256
KEYS = ["gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales", "down_zero_points"]


def _weights(seed=3):
    g = torch.Generator().manual_seed(seed)
    gate = [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)]
    up = [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)]
    down = [torch.randn(H, F, generator=g) * 0.1 for _ in range(E)]
    return gate, up, down


def test_buffer_shapes_and_keys():
    import fused_int4_amd as fq
    plain = fq.QuantizedMoEFFN(E, H, F)
    grouped = fq.QuantizedMoEFFN(E, H, F, group_size=64)
    assert list(plain.state_dict()) == list(grouped.state_dict()) == KEYS
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(plain) == {"gate_up_packed": (E, 2 * F, H // 2), "gate_up_scales": (E, 2 * F),
                             "gate_up_zero_points": (E, 2 * F), "down_packed": (E, H, F // 2), "down_scales": (E, H),
                             "down_zero_points": (E, H)}
    assert shapes(grouped) == {"gate_up_packed": (E, 2 * F, H // 2), "gate_up_scales": (E, 2 * F, H // 64),
                               "gate_up_zero_points": (E, 2 * F, H // 64), "down_packed": (E, H, F // 2),
                               "down_scales": (E, H, F // 64), "down_zero_points": (E, H, F // 64)}
    assert plain.group_size is None and grouped.group_size == 64
    assert "group_size=64" in repr(grouped) and "group_size" not in repr(plain)
    # one group in both projections is the layer of today; one group in one of them keeps a last dimension of 1
    one = fq.QuantizedMoEFFN(E, 128, 128, group_size=128)
    assert one.group_size is None and shapes(one) == shapes(fq.QuantizedMoEFFN(E, 128, 128))
    half = fq.QuantizedMoEFFN(E, H, F, group_size=128)
    assert tuple(half.gate_up_scales.shape) == (E, 2 * F, 1) and tuple(half.down_scales.shape) == (E, H, 2)
    grouped.load_state_dict(fq.QuantizedMoEFFN(E, H, F, group_size=64).state_dict())
    with pytest.raises(RuntimeError):
        grouped.load_state_dict(plain.state_dict())


def test_from_weights_is_the_oracles_grouped_quantiser():
    import fused_int4_amd as fq
    from oracle import oracle as O
    gate, up, down = _weights()
    m = fq.QuantizedMoEFFN.from_weights(gate, up, down, group_size=64)
    assert m.group_size == 64
    for e in range(E):
        p, s, z = O.quantize_weights_grouped(torch.cat([gate[e], up[e]]).numpy(), 64)
        assert np.array_equal(m.gate_up_packed[e].numpy(), p)
        assert np.array_equal(m.gate_up_scales[e].numpy().view(np.int32), np.asarray(s, np.float32).view(np.int32))
        assert np.array_equal(m.gate_up_zero_points[e].numpy().view(np.int32), np.asarray(z, np.float32).view(np.int32))
        p, s, z = O.quantize_weights_grouped(down[e].numpy(), 64)
        assert np.array_equal(m.down_packed[e].numpy(), p)
        assert np.array_equal(m.down_scales[e].numpy().view(np.int32), np.asarray(s, np.float32).view(np.int32))
        assert np.array_equal(m.down_zero_points[e].numpy().view(np.int32), np.asarray(z, np.float32).view(np.int32))
    # without group_size: the buffers of today
    a, b = fq.QuantizedMoEFFN.from_weights(gate, up, down), fq.QuantizedMoEFFN.from_weights(gate, up, down, group_size=None)
    for k in KEYS:
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]) and a.state_dict()[k].dim() == (3 if "packed" in k else 2)


@pytest.mark.parametrize("bad", [3, 48, 0, -64, 96, 64.0, True])
def test_group_size_must_be_even_and_divide_both_dimensions(bad):
    import fused_int4_amd as fq
    with pytest.raises(ValueError, match="group_size"):
        fq.QuantizedMoEFFN(E, H, F, group_size=bad)            # 48: even, divides neither; 96: divides neither 128 nor 256
    with pytest.raises(ValueError, match="group_size"):
        fq.LoRAQuantizedMoEFFN(E, H, F, 8, group_size=bad)


def test_group_size_and_fp8_do_not_combine():
    import fused_int4_amd as fq
    with pytest.raises(ValueError, match="fp8"):
        fq.QuantizedMoEFFN(E, H, F, precision="fp8", group_size=64)


def test_lora_from_quantized_round_trip():
    import fused_int4_amd as fq
    gate, up, down = _weights()
    base = fq.QuantizedMoEFFN.from_weights(gate, up, down, group_size=64)
    m = fq.LoRAQuantizedMoEFFN.from_quantized(base, 8)
    assert m.group_size == 64 and "group_size=64" in repr(m)
    for k in KEYS:
        assert getattr(m, k).data_ptr() == getattr(base, k).data_ptr()          # shared, not copied
    fresh = fq.LoRAQuantizedMoEFFN(E, H, F, 8, group_size=64)
    fresh.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    assert sorted(m.adapter_state_dict()) == ["down_lora_A", "down_lora_B", "gate_up_lora_A", "gate_up_lora_B"]
    assert fq.LoRAQuantizedMoEFFN.from_quantized(fq.QuantizedMoEFFN(E, H, F), 8).group_size is None


def test_block_hands_group_size_on_and_rejects_a_contradiction():
    import fused_int4_amd as fq
    b = fq.QuantizedSparseMoEBlock(4, H, F, top_k=2, shared_ffn_dim=128, group_size=64)
    assert b.experts.group_size == 64 and b.shared_experts.group_size == 64
    assert tuple(b.experts.down_scales.shape) == (4, H, F // 64)
    assert tuple(b.shared_experts.gate_up_scales.shape) == (1, 256, H // 64)
    assert "group_size=64" in repr(b)
    plain = fq.QuantizedSparseMoEBlock(4, H, F, top_k=2, shared_ffn_dim=128)
    assert plain.experts.group_size is None and sorted(plain.state_dict()) == sorted(b.state_dict())
    assert tuple(plain.experts.down_scales.shape) == (4, H)
    experts = fq.QuantizedMoEFFN(4, H, F, group_size=64)
    assert fq.QuantizedSparseMoEBlock(4, H, F, experts=experts).experts.group_size == 64          # keeps its own
    assert fq.QuantizedSparseMoEBlock(4, H, F, experts=experts, group_size=64).experts is experts
    with pytest.raises(ValueError, match="group_size=32 contradicts experts"):
        fq.QuantizedSparseMoEBlock(4, H, F, experts=experts, group_size=32)
    with pytest.raises(ValueError, match="group_size=64 contradicts experts"):
        fq.QuantizedSparseMoEBlock(4, H, F, experts=fq.QuantizedMoEFFN(4, H, F), group_size=64)
    with pytest.raises(ValueError, match="contradicts shared_experts"):
        fq.QuantizedSparseMoEBlock(4, H, F, shared_experts=fq.QuantizedMoEFFN(1, H, 128), group_size=64)
    with pytest.raises(ValueError, match="group_size"):
        fq.QuantizedSparseMoEBlock(4, H, F, group_size=48)
    gate, up, down = _weights()
    blk = fq.QuantizedSparseMoEBlock.from_weights(torch.randn(E, H), gate, up, down, top_k=2, group_size=64,
                                                  shared=(gate[0], up[0], down[0]))
    assert blk.experts.group_size == 64 and blk.shared_experts.group_size == 64
    ref = fq.QuantizedMoEFFN.from_weights(gate, up, down, group_size=64)
    for k in KEYS:
        assert torch.equal(getattr(blk.experts, k), getattr(ref, k)), k
