"""Low-rank adapters on the NVFP4 weights, the part that needs no GPU: the C ABI of FQL_VERSION 450 (fql_moe_nvfp4_lora_fwd /
fql_moe_nvfp4_glu_lora_fwd / fql_moe_nvfp4_lora_bwd_input / fql_linear_nvfp4_lora_fwd / fql_linear_nvfp4_lora_bwd_input: declared,
exported and validated before any HIP call -- every call below is invalid or empty, so none launches), the argument errors of
the ops and the layers LoRANVFP4MoEFFN and LoRANVFP4Linear up to their forward, which is GPU only."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_nvfp4_lora_fwd", "fql_moe_nvfp4_glu_lora_fwd", "fql_moe_nvfp4_lora_bwd_input", "fql_linear_nvfp4_lora_fwd",
       "fql_linear_nvfp4_lora_bwd_input")
OK, NULLP, SHAPE, ODD_K, ALIGN, DTYPE, WORKSPACE = 0, -1, -2, -3, -7, -8, -4
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 16
RANKS = (4, 8, 16, 32, 64)
ADAPTERS = ["gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"]
KEYS = ["gate_up_blocks", "gate_up_scales", "gate_up_global", "down_blocks", "down_scales", "down_global"]


def fq():
    import fused_int4_amd
    return fused_int4_amd


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, gs=P, x=P, v=P, w=P, bias=None, tpe=P, offs=P, out=P2):
    return lib.fql_moe_nvfp4_lora_fwd(bl, sc, gs, x, di, v, w, r, bias, tpe, offs, out, do, E, T, K, N, None, 0, None)


def _glu(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, gs=P, x=P, v=P, w=P, bias=None, tpe=P, offs=P, out=P2,
         act=0, ws=None, nbytes=0):
    return lib.fql_moe_nvfp4_glu_lora_fwd(bl, sc, gs, x, di, v, w, r, bias, tpe, offs, out, do, E, T, K, N, act, 1.702, 7.0, ws,
                                          nbytes, None)


def _bwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, gs=P, x=P, v=P, w=P, tpe=P, offs=P, out=P2):
    return lib.fql_moe_nvfp4_lora_bwd_input(bl, sc, gs, x, di, v, w, r, tpe, offs, out, do, E, T, K, N, None)


def _lin(lib, di=BF16, do=BF16, T=8, K=64, N=96, r=8, bl=P, sc=P, gs=P, x=P, v=P, w=P, bias=None, out=P2):
    return lib.fql_linear_nvfp4_lora_fwd(bl, sc, gs, x, di, v, w, r, bias, out, do, T, K, N, None, 0, None)


def _lin_bwd(lib, di=BF16, do=BF16, T=8, K=64, N=96, r=8, bl=P, sc=P, gs=P, x=P, v=P, w=P, out=P2):
    return lib.fql_linear_nvfp4_lora_bwd_input(bl, sc, gs, x, di, v, w, r, out, do, T, K, N, None)


GROUPED = (_fwd, _glu, _bwd)
ENTRIES = GROUPED + (_lin, _lin_bwd)
IDS = ["fwd", "glu", "bwd", "linear", "linear_bwd"]


# ---- the C boundary

def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 450
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) >= 450 and int(m.group(1)) == lib.fql_version()


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const float *, int,\n"
                    "         const float *, const int32_t *, const int32_t *, void *, int, int, int, int, int, void *, size_t, void *)\n"
                    "    = fql_moe_nvfp4_lora_fwd;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const float *, int,\n"
                    "         const float *, const int32_t *, const int32_t *, void *, int, int, int, int, int, int, float, float,\n"
                    "         void *, size_t, void *) = fql_moe_nvfp4_glu_lora_fwd;\n"
                    "int (*c)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const float *, int,\n"
                    "         const int32_t *, const int32_t *, void *, int, int, int, int, int, void *)\n"
                    "    = fql_moe_nvfp4_lora_bwd_input;\n"
                    "int (*d)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const float *, int,\n"
                    "         const float *, void *, int, int, int, int, void *, size_t, void *) = fql_linear_nvfp4_lora_fwd;\n"
                    "int (*e)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const float *, int,\n"
                    "         void *, int, int, int, int, void *) = fql_linear_nvfp4_lora_bwd_input;\n"
                    "int version_is_450[FQL_VERSION >= 450 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_adapter_refusals_come_before_any_device_call(lib, entry):
    """A NULL lora_rows or adapter matrix, a rank outside the five and K % 32, each with every other argument valid: the code
    comes back from the host-side checks (no pointer below is memory, so a launch could not end well)."""
    assert entry(lib, v=None) == NULLP
    assert entry(lib, w=None) == NULLP
    assert entry(lib, v=None, w=None) == NULLP
    for r in (0, -8, 1, 2, 3, 5, 12, 24, 48, 65, 128):
        assert entry(lib, r=r) == SHAPE, r
    for K in (16, 48, 80, 2):
        assert entry(lib, K=K) == SHAPE, K
    assert entry(lib, K=65) == ODD_K
    assert entry(lib, v=P_HALF) == ALIGN and entry(lib, w=P_HALF) == ALIGN         # float32: 4 bytes
    assert entry(lib, gs=P_HALF) == ALIGN
    for r in RANKS:                                                                # the five pass the rank check ...
        assert entry(lib, r=r, T=0) == OK                                          # ... and T == 0 launches nothing
        assert entry(lib, r=r, bl=None) == NULLP


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_every_pointer_null_pins_the_order_of_the_return_codes(lib, entry):
    """The base entry's order, with the rank behind the types (a bad rank against a bad dtype: the dtype answers) and in
    front of the empty call."""
    null = dict(bl=None, sc=None, gs=None, x=None, v=None, w=None, out=None)
    if entry in GROUPED:
        null.update(tpe=None, offs=None)
    assert entry(lib, K=65, di=F16, r=3, **null) == ODD_K
    assert entry(lib, K=48, di=F16, r=3, **null) == SHAPE
    assert entry(lib, di=F16, r=3, **null) == DTYPE                                # float16 rows are refused, not rounded
    assert entry(lib, do=3, r=3, **null) == DTYPE
    assert entry(lib, T=0, r=3, **null) == SHAPE                                   # the rank before the empty call
    assert entry(lib, T=0, **null) == OK
    assert entry(lib, **null) == NULLP
    assert entry(lib, bl=P_WORD) == ALIGN
    if entry in GROUPED:
        assert entry(lib, E=0, K=65, di=F16, r=3, **null) == SHAPE
        assert entry(lib, E=65535, **null) == NULLP                                # the pointers before the grid's limits
        assert entry(lib, E=65535) == SHAPE
        assert entry(lib, tpe=None, offs=None) == SHAPE                            # no table: E == 1 only
        assert entry(lib, E=1, tpe=None, offs=None, bl=None) == NULLP


def test_the_empty_contraction_has_no_adapter_form(lib):
    assert _bwd(lib, N=0) == SHAPE and _bwd(lib, N=0, T=0) == OK
    assert _lin_bwd(lib, N=0) == SHAPE and _lin_bwd(lib, N=0, T=0) == OK
    assert _fwd(lib, N=0) == OK and _glu(lib, N=0) == OK and _lin(lib, N=0) == OK


def test_gated_entry_checks_its_workspace_last(lib):
    assert _glu(lib, act=7) == SHAPE
    assert _glu(lib) == WORKSPACE                                                  # NULL workspace: behind every other check
    assert _glu(lib, ws=P, nbytes=8) == WORKSPACE


# ---- the ops

E, H, F, T = 2, 64, 96, 6


def _operands():
    blocks, scales = torch.zeros(E, 2 * F, H // 2, dtype=torch.uint8), torch.full((E, 2 * F, H // 16), 0x38, dtype=torch.uint8)
    gs = torch.ones(E)
    tpe, offs = torch.tensor([3, 3], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    return blocks, scales, gs, tpe, offs


def test_forward_op_argument_errors_in_their_order():
    op = fq().ops.moe_forward_nvfp4_lora
    blocks, scales, gs, tpe, offs = _operands()
    x, v, B = torch.zeros(T, H), torch.zeros(T, 8), torch.zeros(E, 2 * F, 8)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        op(blocks.float(), scales, gs, x.half(), v.half(), B, tpe, offs)               # the rows first
    with pytest.raises(RuntimeError, match="uint8"):
        op(blocks.float(), scales, gs, x, v.half(), B, tpe, offs)                      # then the weights
    with pytest.raises(RuntimeError, match="columns"):
        op(blocks, scales, gs, torch.zeros(T, H + 32), v.half(), B, tpe, offs)
    with pytest.raises(RuntimeError, match="global_scale"):
        op(blocks, scales, torch.ones(E + 1), x, v.half(), B, tpe, offs)               # then the global scale
    with pytest.raises(RuntimeError, match="bias must be"):
        op(blocks, scales, gs, x, v.half(), B, tpe, offs, bias=torch.zeros(E, 3))      # then the bias, then the adapter
    for bad in (v.bfloat16(), v[:-1], v[0]):
        with pytest.raises(RuntimeError, match="shrunk rows"):
            op(blocks, scales, gs, x, bad, B.half(), tpe, offs)
    with pytest.raises(RuntimeError, match="rank must be one of"):
        op(blocks, scales, gs, x, torch.zeros(T, 12), torch.zeros(E, 2 * F, 12), tpe, offs)
    for bad in (B.bfloat16(), B[0], torch.zeros(E, 2 * F, 16), torch.zeros(E, 8, 2 * F)):
        with pytest.raises(RuntimeError, match="adapter matrix"):
            op(blocks, scales, gs, x, v, bad, tpe, offs, out_dtype=torch.int8)
    with pytest.raises(RuntimeError, match="out_dtype"):
        op(blocks, scales, gs, x, v, B, tpe, offs, out_dtype=torch.int8)
    with pytest.raises(RuntimeError, match="forward-only"):
        op(blocks, scales, gs, x, v, B.clone().requires_grad_(True), tpe, offs)
    for rows in (x, x.bfloat16()):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):            # no CPU fallback
            op(blocks, scales, gs, rows, v, B, tpe, offs)


def test_gated_backward_and_dense_op_argument_errors():
    blocks, scales, gs, tpe, offs = _operands()                                    # as the gate|up weights: N = 2F, K = H
    o = fq().ops
    gated, bwd = o.moe_gated_forward_nvfp4_lora, o.moe_backward_input_nvfp4_lora
    gu, v, B = torch.zeros(T, 2 * H), torch.zeros(T, 8), torch.zeros(E, 2 * F, 8)
    with pytest.raises(RuntimeError, match="columns"):
        gated(blocks, scales, gs, torch.zeros(T, H), v, B, tpe, offs)
    with pytest.raises(ValueError, match="activation must be"):
        gated(blocks, scales, gs, gu, v, B, tpe, offs, activation="relu")
    with pytest.raises(RuntimeError, match="adapter matrix"):
        gated(blocks, scales, gs, gu, v, torch.zeros(E, 8, H), tpe, offs)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        gated(blocks, scales, gs, gu, v, B, tpe, offs)
    gy, A = torch.zeros(T, 2 * F), torch.zeros(E, 8, H)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        bwd(blocks, scales, gs, gy.half(), v, A, tpe, offs)
    with pytest.raises(RuntimeError, match=r"\[T, N\]"):
        bwd(blocks, scales, gs, torch.zeros(T, H), v, A, tpe, offs)
    with pytest.raises(RuntimeError, match="global_scale"):
        bwd(blocks, scales, gs.double(), gy, v, B, tpe, offs)
    with pytest.raises(RuntimeError, match="adapter matrix"):
        bwd(blocks, scales, gs, gy, v, B, tpe, offs)                               # B's layout where A's belongs
    with pytest.raises(RuntimeError, match="rank must be one of"):
        bwd(blocks, scales, gs, gy, torch.zeros(T, 5), torch.zeros(E, 5, H), tpe, offs)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        bwd(blocks, scales, gs, gy, v, A, tpe, offs)
    # the dense forms: 2-D weights, one global scale, 2-D adapters
    b2, s2, g1 = blocks[0], scales[0], torch.ones(1)
    with pytest.raises(RuntimeError, match="uint8"):
        o.linear_forward_nvfp4_lora(blocks, scales, g1, torch.zeros(T, H), v, B[0])
    with pytest.raises(RuntimeError, match="adapter matrix"):
        o.linear_forward_nvfp4_lora(b2, s2, g1, torch.zeros(T, H), v, B)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        o.linear_forward_nvfp4_lora(b2, s2, g1, torch.zeros(T, H), v, B[0])
    with pytest.raises(RuntimeError, match="adapter matrix"):
        o.linear_backward_input_nvfp4_lora(b2, s2, g1, gy, v, A)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        o.linear_backward_input_nvfp4_lora(b2, s2, g1, gy, v, A[0])
    with pytest.raises(RuntimeError, match="float16 is refused"):
        o.linear_lora_forward_nvfp4(torch.zeros(T, H).half(), b2, s2, g1, A[0], B[0], 2.0)
    with pytest.raises(RuntimeError, match="rank must be one of"):
        o.linear_lora_forward_nvfp4(torch.zeros(T, H), b2, s2, g1, torch.zeros(12, H), torch.zeros(2 * F, 12), 2.0)
    with pytest.raises(RuntimeError, match="lora_A must be"):
        o.linear_lora_forward_nvfp4(torch.zeros(T, H), b2, s2, g1, A[0], torch.zeros(F, 8), 2.0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        o.linear_lora_forward_nvfp4(torch.zeros(T, H), b2, s2, g1, A[0], B[0], 2.0)


def test_ffn_op_argument_errors():
    op = fq().ops.moe_ffn_lora_forward_nvfp4
    gub, gus, gug, tpe, offs = _operands()
    db, ds, dg = torch.zeros(E, H, F // 2, dtype=torch.uint8), torch.full((E, H, F // 16), 0x38, dtype=torch.uint8), torch.ones(E)
    x = torch.zeros(T, H)
    ad = [torch.zeros(E, 8, H), torch.zeros(E, 2 * F, 8), torch.zeros(E, 8, F), torch.zeros(E, H, 8)]
    call = lambda x=x, ad=ad, **kw: op(gub, gus, gug, db, ds, dg, x, *ad, 2.0, tpe, offs, **kw)
    with pytest.raises(ValueError, match="float16"):
        call(activation_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="activation_dtype"):
        call(x=x.bfloat16())
    with pytest.raises(RuntimeError, match="activation_dtype"):
        call(activation_dtype=torch.bfloat16)
    for i in range(4):
        bad = list(ad)
        bad[i] = bad[i].bfloat16()
        with pytest.raises(RuntimeError, match="stay float32"):
            call(ad=bad)
        bad[i] = torch.zeros(E, 7, 9)
        with pytest.raises(RuntimeError, match="adapters must be"):
            call(ad=bad)
    with pytest.raises(RuntimeError, match="same rank"):
        call(ad=ad[:2] + [torch.zeros(E, 16, F), torch.zeros(E, H, 16)])
    with pytest.raises(RuntimeError, match="rank must be one of"):
        call(ad=[torch.zeros(E, 12, H), torch.zeros(E, 2 * F, 12), torch.zeros(E, 12, F), torch.zeros(E, H, 12)])
    with pytest.raises(RuntimeError, match="CUDA"):
        call()


# ---- the layers

def test_constructor_refusals():
    L = fq().LoRANVFP4MoEFFN
    for rank in (0, 3, 12, 128, None):
        with pytest.raises(ValueError, match="rank must be one of"):
            L(E, H, F, rank)
        with pytest.raises(ValueError, match="rank must be one of"):
            fq().LoRANVFP4Linear(H, F, rank)
    with pytest.raises(ValueError, match="float16"):
        L(E, H, F, 8, activation_dtype=torch.float16)
    with pytest.raises(ValueError, match="multiples of 32"):
        L(E, H + 16, F, 8)
    m = L(E, H, F, 16, alpha=32.0, activation="swiglu_clamp", activation_dtype=torch.bfloat16)
    assert m.rank == 16 and m.scaling == 2.0 and m.activation_dtype == torch.bfloat16 and m.input_grad is True
    assert L(E, H, F, 8, activation_dtype=torch.float32).activation_dtype is None
    assert L(E, H, F, 8, input_grad=False).input_grad is True                      # always on
    assert "rank=16" in repr(m) and "alpha=32" in repr(m) and "format=nvfp4" in repr(m)


def test_state_dict_is_the_base_layers_plus_the_four_adapters():
    base = fq().NVFP4MoEFFN(E, H, F, expert_bias=True)
    m = fq().LoRANVFP4MoEFFN(E, H, F, 8, expert_bias=True)
    assert sorted(m.state_dict()) == sorted(list(base.state_dict()) + ADAPTERS)
    assert sorted(fq().LoRANVFP4MoEFFN(E, H, F, 8).state_dict()) == sorted(KEYS + ADAPTERS)
    assert sorted(n for n, _ in m.named_parameters()) == sorted(ADAPTERS + ["gate_up_bias", "down_bias"])
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ADAPTERS     # the biases stay frozen until asked
    shapes = {"gate_up_lora_A": (E, 8, H), "gate_up_lora_B": (E, 2 * F, 8), "down_lora_A": (E, 8, F), "down_lora_B": (E, H, 8)}
    for name, shape in shapes.items():
        p = getattr(m, name)
        assert tuple(p.shape) == shape and p.dtype == torch.float32, name
    assert torch.count_nonzero(m.gate_up_lora_B) == 0 and torch.count_nonzero(m.down_lora_B) == 0   # PEFT: B = 0
    assert float(m.gate_up_lora_A.detach().abs().max()) <= 1.0 / H ** 0.5 and torch.count_nonzero(m.gate_up_lora_A) > 0
    assert float(m.down_lora_A.detach().abs().max()) <= 1.0 / F ** 0.5 and torch.count_nonzero(m.down_lora_A) > 0
    assert sorted(m.adapter_state_dict()) == sorted(ADAPTERS)
    for k, v in m.adapter_state_dict().items():
        assert v.data_ptr() == getattr(m, k).data_ptr(), k
    with torch.no_grad():
        m.gate_up_lora_B.fill_(1.0)
    m.reset_lora_parameters()
    assert torch.count_nonzero(m.gate_up_lora_B) == 0
    base.load_state_dict(m.state_dict(), strict=False)
    m.load_state_dict(base.state_dict(), strict=False)


def _nvfp4_tensors(seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randint(0, 0x7F, s, generator=g, dtype=torch.uint8)
    return r(E, 2 * F, H // 2), r(E, 2 * F, H // 16), torch.rand(E, generator=g) + 0.5, r(E, H, F // 2), r(E, H, F // 16), \
        torch.rand(E, generator=g) + 0.5, g


def test_from_layer_shares_storage_and_the_constructors_take_the_rank():
    gub, gus, gug, db, ds, dg, g = _nvfp4_tensors()
    base = fq().NVFP4MoEFFN.from_nvfp4(gub, gus, gug, db, ds, dg, gate_up_bias=torch.randn(E, 2 * F, generator=g),
                                       down_bias=torch.randn(E, H, generator=g), activation="gelu_tanh",
                                       activation_dtype=torch.bfloat16)
    base.down_bias.requires_grad_(True)
    m = fq().LoRANVFP4MoEFFN.from_layer(base, 16, alpha=8.0)
    for k in KEYS:
        assert getattr(m, k).data_ptr() == getattr(base, k).data_ptr(), k
    assert m.gate_up_bias is base.gate_up_bias and m.down_bias is base.down_bias
    assert m.down_bias.requires_grad and not m.gate_up_bias.requires_grad          # in the state they have
    assert (m.rank, m.scaling, m.activation, m.activation_dtype) == (16, 0.5, "gelu_tanh", torch.bfloat16)
    assert not base.input_grad and m.input_grad                                    # whatever the wrapped layer has
    n = fq().LoRANVFP4MoEFFN.from_nvfp4(gub, gus, gug, db, ds, dg, rank=4, alpha=4.0, activation="swiglu_clamp")
    assert n.rank == 4 and n.scaling == 1.0 and not n.expert_bias and torch.equal(n.gate_up_blocks, gub)
    assert torch.equal(n.down_global, dg)
    w = lambda *s: [torch.randn(*s, generator=g) for _ in range(E)]
    q = fq().LoRANVFP4MoEFFN.from_weights(w(F, H), w(F, H), w(H, F), rank=8)
    assert q.rank == 8 and tuple(q.gate_up_lora_B.shape) == (E, 2 * F, 8) and tuple(q.down_global.shape) == (E,)
    with pytest.raises(TypeError):
        fq().LoRANVFP4MoEFFN.from_nvfp4(gub, gus, gug, db, ds, dg)                 # no rank
    assert "LoRANVFP4MoEFFN" in fq().__all__ and "LoRANVFP4Linear" in fq().__all__


def test_the_block_accepts_the_layer_as_experts_and_as_shared_experts():
    experts = fq().LoRANVFP4MoEFFN(E, H, F, 8)
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=experts)
    assert blk.experts is experts
    shared = fq().LoRANVFP4MoEFFN(1, H, F, 8)
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=fq().LoRANVFP4MoEFFN(E, H, F, 8), shared_experts=shared)
    assert blk.shared_experts is shared
    names = [n for n, p in blk.named_parameters() if p.requires_grad]
    assert sum("lora" in n for n in names) == 8 and "gate.weight" in names


def test_linear_layer_surface():
    L = fq().LoRANVFP4Linear
    base = fq().NVFP4Linear(H, F, bias=True)
    m = L(H, F, 8, alpha=4.0, bias=True)
    assert sorted(m.state_dict()) == sorted(list(base.state_dict()) + ["lora_A", "lora_B"])
    assert sorted(L(H, F, 8).state_dict()) == sorted(["blocks", "scales", "global_scale", "lora_A", "lora_B"])
    assert [n for n, _ in m.named_parameters()] == ["lora_A", "lora_B"]
    assert tuple(m.lora_A.shape) == (8, H) and tuple(m.lora_B.shape) == (F, 8) and m.lora_A.dtype == torch.float32
    assert torch.count_nonzero(m.lora_B) == 0 and torch.count_nonzero(m.lora_A) > 0
    assert float(m.lora_A.detach().abs().max()) <= 1.0 / H ** 0.5
    assert m.scaling == 0.5 and m.input_grad is True and sorted(m.adapter_state_dict()) == ["lora_A", "lora_B"]
    assert "rank=8" in repr(m) and "format=nvfp4" in repr(m)
    lin = torch.nn.Linear(H, F)
    base = fq().NVFP4Linear.from_linear(lin)
    w = L.from_layer(base, 16, alpha=16.0)
    for k in ("blocks", "scales", "global_scale", "bias"):
        assert getattr(w, k).data_ptr() == getattr(base, k).data_ptr(), k
    assert w.rank == 16 and w.scaling == 1.0
    q = L.from_linear(lin, rank=4, alpha=2.0)
    assert q.rank == 4 and torch.equal(q.blocks, base.blocks) and torch.equal(q.bias, base.bias)
    n = L.from_nvfp4(base.blocks, base.scales, base.global_scale, rank=8)
    assert n.rank == 8 and n.bias is None and torch.equal(n.global_scale, base.global_scale)
    with pytest.raises(TypeError):
        L.from_nvfp4(base.blocks, base.scales)                                     # no rank


def test_cpu_forward_raises():
    tpe, offs = torch.tensor([4, 0], dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        fq().LoRANVFP4MoEFFN(E, H, F, 8)(torch.zeros(4, H), tpe, offs)
    with pytest.raises(RuntimeError, match="GPU"):
        fq().LoRANVFP4Linear(H, F, 8)(torch.zeros(2, 3, H))
