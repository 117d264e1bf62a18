"""OCP MXFP4 expert weights, the part that needs no GPU: the format helpers quantize_mxfp4 / dequantize_mxfp4, the C ABI of
FQL_VERSION 340 (fql_moe_mx4_fwd, fql_moe_mx4_glu_fwd and their workspace query: declared, exported and validated in the
documented order before any HIP call -- every call below is invalid, empty or stops at the workspace check, so none
launches) and the layer MXFP4MoEFFN up to its forward, which is GPU only."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_mx4_workspace_bytes", "fql_moe_mx4_fwd", "fql_moe_mx4_glu_fwd")
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
SILU, GELU, CLAMP = 0, 1, 2
NAN = float("nan")
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 16
VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def q():
    from fused_int4_amd import quantize
    return quantize


def pack(codes):
    return (codes[..., 1::2] << 4) | codes[..., 0::2]


# ---- the format helpers

def test_dequantise_every_code_and_the_edge_scales():
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)                    # one block of 32: every code twice
    for s in (0, 1, 126, 127, 128, 254):
        w = q().dequantize_mxfp4(pack(codes)[None], torch.tensor([[s]], dtype=torch.uint8))[0]
        assert w.dtype == torch.float32 and tuple(w.shape) == (32,)
        for i, c in enumerate(codes.tolist()):
            want = torch.tensor((-1.0 if c & 8 else 1.0) * VALUES[c & 7], dtype=torch.float64) * 2.0 ** (s - 127)
            assert w[i].item() == want.float().item(), (s, c)               # exact (float32's own range: 6 * 2^127 is inf)
            assert bool(torch.signbit(w[i])) == bool(c & 8), (s, c)         # code 8 is -0
    w = q().dequantize_mxfp4(pack(codes)[None], torch.tensor([[255]], dtype=torch.uint8))
    assert bool(torch.isnan(w).all())                                        # the zeros of the block as well


def test_even_k_sits_in_the_low_nibble_and_scales_belong_to_their_block():
    blocks = torch.zeros(2, 32, dtype=torch.uint8)                           # N = 2, K = 64
    blocks[0, 0] = 0x52                                                      # k = 0: code 2 (1.0); k = 1: code 5 (3.0)
    blocks[1, 16] = 0x0F                                                     # row 1, k = 32: code 15 (-6.0)
    scales = torch.tensor([[128, 127], [127, 125]], dtype=torch.uint8)
    w = q().dequantize_mxfp4(blocks, scales)
    assert w[0, 0] == 2.0 and w[0, 1] == 6.0 and w[1, 32] == -1.5 and torch.count_nonzero(w) == 3


def test_quantise_ties_go_to_the_even_mantissa_and_large_values_saturate():
    w = torch.zeros(1, 64)
    w[0, :6] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 5.0])
    w[0, 6] = -0.75
    w[0, 31] = 4.0                                                           # amax 5 and 4: shared exponent 0, scale code 127
    w[0, 32:34] = torch.tensor([7.0, 100.0])                                 # second block: amax 100 -> 2^4
    blocks, scales = q().quantize_mxfp4(w)
    assert blocks.dtype == scales.dtype == torch.uint8 and tuple(blocks.shape) == (1, 32) and tuple(scales.shape) == (1, 2)
    assert scales.tolist() == [[127, 131]]
    d = q().dequantize_mxfp4(blocks, scales)[0]
    assert d[:7].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, -1.0]
    assert d[32].item() == 8.0 and d[33].item() == 96.0                      # 7 / 16 -> 0.5, 100 / 16 = 6.25 -> 6 (the top)
    one = torch.zeros(1, 32)
    one[0, 0], one[0, 1] = 7.0, 4.0                                          # ... and 7 next to 4: saturates to 6 at scale 1
    assert q().dequantize_mxfp4(*q().quantize_mxfp4(one))[0, :2].tolist() == [6.0, 4.0]


def test_all_zero_block_and_non_finite_weights():
    blocks, scales = q().quantize_mxfp4(torch.zeros(3, 64))
    assert torch.count_nonzero(blocks) == 0 and bool((scales == 127).all())
    for bad in (float("inf"), float("-inf"), NAN):
        w = torch.ones(2, 32)
        w[1, 5] = bad
        with pytest.raises(ValueError):
            q().quantize_mxfp4(w)
    with pytest.raises(ValueError):
        q().quantize_mxfp4(torch.ones(2, 48))                                # K % 32


def test_round_trip_of_blocks_that_hold_a_4_or_a_6():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (3, 5, 96), generator=g, dtype=torch.uint8)
    top = torch.tensor([6, 7, 14, 15], dtype=torch.uint8)                    # +-4, +-6: the block's amax fixes its scale
    where = torch.randint(0, 32, (3, 5, 3), generator=g)
    codes.view(3, 5, 3, 32).scatter_(3, where[..., None], top[torch.randint(0, 4, (3, 5, 3, 1), generator=g)])
    blocks = pack(codes)
    scales = torch.randint(1, 251, (3, 5, 3), generator=g, dtype=torch.uint8)
    b2, s2 = q().quantize_mxfp4(q().dequantize_mxfp4(blocks, scales))
    assert torch.equal(b2, blocks) and torch.equal(s2, scales)


# ---- the C boundary

@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P, offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_fwd(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _glu(lib, act=CLAMP, alpha=1.702, limit=7.0, di=F32, do=F32, E=2, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, tpe=P,
         offs=P, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_mx4_glu_fwd(bl, sc, x, di, bias, tpe, offs, out, do, E, T, K, N, act, alpha, limit, ws, nbytes, None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 340


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "size_t (*w)(int, int, int, int, int) = fql_moe_mx4_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_mx4_fwd;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, float, float, void *, size_t, void *)\n"
                    "    = fql_moe_mx4_glu_fwd;\n"
                    "int version_is_340[FQL_VERSION >= 340 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_workspace_query(lib):
    w = lib.fql_moe_mx4_workspace_bytes
    assert w(3, 51, 96, 136, 0) == 0                                         # the plain call stages nothing
    assert w(3, 51, 96, 136, 1) == (51 * 96 * 2 + 15) // 16 * 16             # the gated call: h [T][K] bfloat16
    assert w(3, 0, 96, 136, 1) == 0 and w(3, 51, 0, 136, 1) == 0


@pytest.mark.parametrize("call", [_fwd, _glu], ids=["fwd", "glu"])
def test_argument_errors_in_order(lib, call):
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert call(lib, **kw) == SHAPE, kw
    assert call(lib, K=65) == ODD_K
    assert call(lib, K=65, E=0) == SHAPE                                     # the dimensions before odd K
    for K in (16, 48, 80, 2):
        assert call(lib, K=K) == SHAPE, K                                    # K % 32: one scale per 32 inputs
    assert call(lib, K=33, di=F16) == ODD_K                                  # odd K before the types
    assert call(lib, K=48, di=F16) == SHAPE                                  # ... and K % 32 too
    assert call(lib, di=F16) == DTYPE                                        # float16 rows are refused, not rounded
    assert call(lib, di=3) == DTYPE and call(lib, di=-1) == DTYPE and call(lib, do=3) == DTYPE
    for do in (F32, F16, BF16):
        assert call(lib, do=do, T=0) == OK
    assert call(lib, T=0, bl=None, x=None, out=None) == OK                   # the empty call before the pointers
    assert call(lib, N=0, out=None) == OK
    assert call(lib, T=0, di=F16) == DTYPE                                   # ... but behind the types
    for kw in (dict(bl=None), dict(sc=None), dict(x=None), dict(out=None), dict(tpe=None), dict(offs=None)):
        assert call(lib, **kw) == NULLP, kw
    assert call(lib, tpe=None, offs=None) == SHAPE                           # no table: one segment, E == 1 only
    assert call(lib, E=65535) == SHAPE and call(lib, E=65536) == SHAPE and call(lib, E=70000) == SHAPE
    assert call(lib, T=4194241) == SHAPE                                     # the grid's y
    assert call(lib, bl=P_WORD) == ALIGN                                     # blocks: 16 bytes
    assert call(lib, di=BF16, x=P_BYTE) == ALIGN
    assert call(lib, di=F32, x=P_HALF) == ALIGN
    assert call(lib, do=F16, out=P_BYTE) == ALIGN
    assert call(lib, do=F32, out=P_HALF) == ALIGN
    assert call(lib, bias=P_HALF) == ALIGN


def test_gated_activation_and_workspace_errors(lib):
    assert _glu(lib, act=3) == SHAPE and _glu(lib, act=-1) == SHAPE
    for kw in (dict(alpha=NAN), dict(limit=NAN), dict(limit=0.0), dict(limit=-1.0), dict(alpha=float("inf"))):
        assert _glu(lib, act=CLAMP, **kw) == SHAPE, kw
        assert _glu(lib, act=GELU, **kw) == SHAPE, kw
        assert _glu(lib, act=SILU, T=0, **kw) == OK, kw                      # silu ignores its two floats
    assert _glu(lib, act=3, K=65) == SHAPE                                   # the activation before odd K
    need = 8 * 64 * 2
    assert _glu(lib) == WS                                                   # everything else is fine: the workspace is last
    assert _glu(lib, ws=ctypes.c_void_p(24), nbytes=1 << 20) == WS           # misaligned
    assert _glu(lib, ws=P, nbytes=need - 16) == WS                           # short
    assert _glu(lib, bias=None) == WS and _glu(lib, tpe=None, offs=None, E=1) == WS      # both optional


# ---- the layer

E, H, F = 3, 64, 96
KEYS = ["gate_up_blocks", "gate_up_scales", "down_blocks", "down_scales"]


def fq():
    import fused_int4_amd
    return fused_int4_amd


def _format_tensors(seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    return r(E, 2 * F, H // 2), r(E, 2 * F, H // 32), r(E, H, F // 2), r(E, H, F // 32)


def test_state_dict_keys_shapes_and_what_the_block_reads():
    m = fq().MXFP4MoEFFN(E, H, F)
    assert list(m.state_dict()) == KEYS
    assert {k: (tuple(v.shape), v.dtype) for k, v in m.state_dict().items()} == {
        "gate_up_blocks": ((E, 2 * F, H // 2), torch.uint8), "gate_up_scales": ((E, 2 * F, H // 32), torch.uint8),
        "down_blocks": ((E, H, F // 2), torch.uint8), "down_scales": ((E, H, F // 32), torch.uint8)}
    b = fq().MXFP4MoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp")
    assert sorted(b.state_dict()) == sorted(KEYS + ["gate_up_bias", "down_bias"])
    assert tuple(b.gate_up_bias.shape) == (E, 2 * F) and tuple(b.down_bias.shape) == (E, H)
    assert not b.gate_up_bias.requires_grad and b.gate_up_bias.dtype == torch.float32
    assert (b.num_experts, b.hidden_dim, b.ffn_dim, b.group_size, b.expert_bias) == (E, H, F, None, True)
    assert b.activation_args == ("swiglu_clamp", 1.702, 7.0) and b.biases[0] is b.gate_up_bias
    assert m.biases == (None, None) and m.activation_args[0] == "silu"
    assert "mxfp4" in repr(b) and "swiglu_clamp" in repr(b)
    for bad in (dict(hidden_dim=48), dict(ffn_dim=80)):
        with pytest.raises(ValueError):
            fq().MXFP4MoEFFN(**{**dict(num_experts=E, hidden_dim=H, ffn_dim=F), **bad})
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN(E, H, F, activation_dtype=torch.float16)
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN(E, H, F, activation="relu")


def test_from_mxfp4_plain_interleaved_and_the_block_dimension():
    gub, gus, db, ds = _format_tensors()
    g = torch.Generator().manual_seed(2)
    bgu, bd = torch.randn(E, 2 * F, generator=g), torch.randn(E, H, generator=g)
    m = fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds)
    for k, t in zip(KEYS, (gub, gus, db, ds)):
        assert torch.equal(getattr(m, k), t), k
    assert not m.expert_bias and (m.num_experts, m.hidden_dim, m.ffn_dim) == (E, H, F)
    # the checkpoint's [E, N, K/32, 16] block dimension is flattened
    m4 = fq().MXFP4MoEFFN.from_mxfp4(gub.reshape(E, 2 * F, H // 32, 16), gus, db.reshape(E, H, F // 32, 16), ds)
    for k in KEYS:
        assert torch.equal(getattr(m4, k), getattr(m, k)), k
    # interleaved: rows 0, 2, 4, ... are the gate, 1, 3, 5, ... the up projection; against an explicit de-interleave
    mi = fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds, gate_up_bias=bgu, down_bias=bd, interleaved=True,
                                     activation="swiglu_clamp")
    gate_rows, up_rows = list(range(0, 2 * F, 2)), list(range(1, 2 * F, 2))
    for e in range(E):
        for i in range(F):
            assert torch.equal(mi.gate_up_blocks[e, i], gub[e, gate_rows[i]])
            assert torch.equal(mi.gate_up_blocks[e, F + i], gub[e, up_rows[i]])
            assert torch.equal(mi.gate_up_scales[e, i], gus[e, gate_rows[i]])
            assert torch.equal(mi.gate_up_scales[e, F + i], gus[e, up_rows[i]])
        assert torch.equal(mi.gate_up_bias[e, :F], bgu[e, gate_rows]) and torch.equal(mi.gate_up_bias[e, F:], bgu[e, up_rows])
    assert torch.equal(mi.down_blocks, db) and torch.equal(mi.down_bias, bd) and mi.activation == "swiglu_clamp"
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds, gate_up_bias=bgu)             # the biases come together
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_mxfp4(gub, gus[:, :, :1], db, ds)
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db[:, :-1], ds[:, :-1])
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_mxfp4(gub.float(), gus, db, ds)
    # a state dict round trip
    fresh = fq().MXFP4MoEFFN(E, H, F, expert_bias=True)
    fresh.load_state_dict(mi.state_dict())
    for k, v in mi.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k


def test_from_weights_quantises_with_quantize_mxfp4():
    g = torch.Generator().manual_seed(3)
    gate = [torch.randn(F, H, generator=g) for _ in range(E)]
    up = [torch.randn(F, H, generator=g) for _ in range(E)]
    down = [torch.randn(H, F, generator=g) for _ in range(E)]
    m = fq().MXFP4MoEFFN.from_weights(gate, up, down)
    for e in range(E):
        b, s = q().quantize_mxfp4(torch.cat([gate[e], up[e]]))
        assert torch.equal(m.gate_up_blocks[e], b) and torch.equal(m.gate_up_scales[e], s)
        b, s = q().quantize_mxfp4(down[e])
        assert torch.equal(m.down_blocks[e], b) and torch.equal(m.down_scales[e], s)
    with pytest.raises(ValueError):
        fq().MXFP4MoEFFN.from_weights(gate, up, down, gate_bias=[torch.zeros(F)] * E)


def test_cpu_forward_raises():
    m = fq().MXFP4MoEFFN(E, H, F)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(4, H), torch.tensor([4, 0, 0], dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


def test_block_accepts_the_layer_and_refuses_wrong_sizes():
    experts = fq().MXFP4MoEFFN(4, H, F, activation="swiglu_clamp", expert_bias=True)
    blk = fq().QuantizedSparseMoEBlock(4, H, F, top_k=2, experts=experts, router_bias=True)
    assert blk.experts is experts and "mxfp4" in repr(blk)
    assert sorted(blk.state_dict()) == sorted(["gate.weight", "gate.bias"] + ["experts." + k for k in
                                                                               KEYS + ["gate_up_bias", "down_bias"]])
    assert fq().QuantizedSparseMoEBlock(4, H, F, experts=experts, activation="swiglu_clamp", expert_bias=True).experts is experts
    for bad in ((3, H, F), (4, 128, F), (4, H, 64)):
        with pytest.raises(ValueError, match="experts must have"):
            fq().QuantizedSparseMoEBlock(*bad, experts=experts)
    with pytest.raises(ValueError, match="contradicts experts"):
        fq().QuantizedSparseMoEBlock(4, H, F, experts=experts, activation="silu")
    with pytest.raises(ValueError, match="contradicts experts"):
        fq().QuantizedSparseMoEBlock(4, H, F, experts=experts, group_size=32)
    for name in ("quantize_mxfp4", "dequantize_mxfp4", "MXFP4MoEFFN"):
        assert name in fq().__all__ and hasattr(fq(), name)
