"""Low-rank adapters on the MXFP4 experts, the part that needs no GPU: the C ABI of FQL_VERSION 410 (fql_moe_mx4_lora_fwd /
fql_moe_mx4_glu_lora_fwd / fql_moe_mx4_lora_bwd_input: declared, exported and validated before any HIP call -- every call below
is invalid or empty, so none launches), the argument errors of the four ops and the layer LoRAMXFP4MoEFFN up to its forward,
which is GPU only."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_mx4_lora_fwd", "fql_moe_mx4_glu_lora_fwd", "fql_moe_mx4_lora_bwd_input")
OK, NULLP, SHAPE, ODD_K, ALIGN, DTYPE, WORKSPACE = 0, -1, -2, -3, -7, -8, -4
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 16
RANKS = (4, 8, 16, 32, 64)
ADAPTERS = ["gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"]
KEYS = ["gate_up_blocks", "gate_up_scales", "down_blocks", "down_scales"]


def fq():
    import fused_int4_amd
    return fused_int4_amd


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _fwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, x=P, v=P, w=P, bias=None, tpe=P, offs=P, out=P2):
    return lib.fql_moe_mx4_lora_fwd(bl, sc, x, di, v, w, r, bias, tpe, offs, out, do, E, T, K, N, None, 0, None)


def _glu(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, x=P, v=P, w=P, bias=None, tpe=P, offs=P, out=P2,
         act=0, ws=None, nbytes=0):
    return lib.fql_moe_mx4_glu_lora_fwd(bl, sc, x, di, v, w, r, bias, tpe, offs, out, do, E, T, K, N, act, 1.702, 7.0, ws,
                                        nbytes, None)


def _bwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, r=8, bl=P, sc=P, x=P, v=P, w=P, tpe=P, offs=P, out=P2):
    return lib.fql_moe_mx4_lora_bwd_input(bl, sc, x, di, v, w, r, tpe, offs, out, do, E, T, K, N, None)


ENTRIES = (_fwd, _glu, _bwd)


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
    assert lib.fql_version() >= 410
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) >= 410 and int(m.group(1)) == lib.fql_version()


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const uint8_t *, const void *, int, const float *, const float *, int, const float *,\n"
                    "         const int32_t *, const int32_t *, void *, int, int, int, int, int, void *, size_t, void *)\n"
                    "    = fql_moe_mx4_lora_fwd;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const void *, int, const float *, const float *, int, const float *,\n"
                    "         const int32_t *, const int32_t *, void *, int, int, int, int, int, int, float, float, void *, size_t,\n"
                    "         void *) = fql_moe_mx4_glu_lora_fwd;\n"
                    "int (*c)(const uint8_t *, const uint8_t *, const void *, int, const float *, const float *, int,\n"
                    "         const int32_t *, const int32_t *, void *, int, int, int, int, int, void *)\n"
                    "    = fql_moe_mx4_lora_bwd_input;\n"
                    "int version_is_410[FQL_VERSION >= 410 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


@pytest.mark.parametrize("entry", ENTRIES, ids=["fwd", "glu", "bwd"])
def test_adapter_refusals_come_before_any_device_call(lib, entry):
    """A NULL v or adapter matrix, a rank outside the five and K % 32, each with every other argument valid: the code comes
    back from the host-side checks (no pointer below is memory, so a launch could not end well)."""
    assert entry(lib, v=None) == NULLP
    assert entry(lib, w=None) == NULLP
    assert entry(lib, v=None, w=None) == NULLP
    for r in (0, -8, 1, 2, 3, 5, 12, 24, 48, 65, 128):
        assert entry(lib, r=r) == SHAPE, r
    for K in (16, 48, 80, 2):
        assert entry(lib, K=K) == SHAPE, K
    assert entry(lib, K=65) == ODD_K
    assert entry(lib, v=P_HALF) == ALIGN and entry(lib, w=P_HALF) == ALIGN         # float32: 4 bytes
    for r in RANKS:                                                                # the five pass the rank check ...
        assert entry(lib, r=r, T=0) == OK                                          # ... and T == 0 launches nothing
        assert entry(lib, r=r, bl=None) == NULLP


@pytest.mark.parametrize("entry", ENTRIES, ids=["fwd", "glu", "bwd"])
def test_every_pointer_null_pins_the_order_of_the_return_codes(lib, entry):
    """The base entry's order, with the rank behind the types and in front of the empty call."""
    null = dict(bl=None, sc=None, x=None, v=None, w=None, tpe=None, offs=None, out=None)
    assert entry(lib, E=0, K=65, di=F16, r=3, **null) == SHAPE
    assert entry(lib, K=65, di=F16, r=3, **null) == ODD_K
    assert entry(lib, K=48, di=F16, r=3, **null) == SHAPE
    assert entry(lib, di=F16, r=3, **null) == DTYPE                                # float16 rows are refused, not rounded
    assert entry(lib, do=3, r=3, **null) == DTYPE
    assert entry(lib, T=0, r=3, **null) == SHAPE                                   # the rank before the empty call
    assert entry(lib, T=0, **null) == OK
    assert entry(lib, **null) == NULLP
    assert entry(lib, E=65535, **null) == NULLP                                    # the pointers before the grid's limits
    assert entry(lib, E=65535) == SHAPE
    assert entry(lib, tpe=None, offs=None) == SHAPE                                # no table: E == 1 only
    assert entry(lib, bl=P_WORD) == ALIGN


def test_the_empty_contraction_has_no_adapter_form(lib):
    assert _bwd(lib, N=0) == SHAPE and _bwd(lib, N=0, T=0) == OK
    assert _fwd(lib, N=0) == OK and _glu(lib, N=0) == OK


def test_gated_entry_checks_its_workspace_last(lib):
    assert _glu(lib, act=7) == SHAPE
    assert _glu(lib) == WORKSPACE                                                  # NULL workspace: behind every other check
    assert _glu(lib, ws=P, nbytes=8) == WORKSPACE


# ---- the ops

E, H, F, T = 2, 64, 96, 6


def _operands():
    blocks, scales = torch.zeros(E, 2 * F, H // 2, dtype=torch.uint8), torch.full((E, 2 * F, H // 32), 127, dtype=torch.uint8)
    tpe, offs = torch.tensor([3, 3], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    return blocks, scales, tpe, offs


def test_forward_op_argument_errors():
    op = fq().ops.moe_forward_mxfp4_lora
    blocks, scales, tpe, offs = _operands()
    x, v, B = torch.zeros(T, H), torch.zeros(T, 8), torch.zeros(E, 2 * F, 8)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        op(blocks, scales, x.half(), v, B, tpe, offs)
    with pytest.raises(RuntimeError, match="uint8"):
        op(blocks.float(), scales, x, v, B, tpe, offs)
    with pytest.raises(RuntimeError, match="columns"):
        op(blocks, scales, torch.zeros(T, H + 32), v, B, tpe, offs)
    for bad in (v.bfloat16(), v[:-1], v[0]):
        with pytest.raises(RuntimeError, match="shrunk rows"):
            op(blocks, scales, x, bad, B, tpe, offs)
    with pytest.raises(RuntimeError, match="rank must be one of"):
        op(blocks, scales, x, torch.zeros(T, 12), torch.zeros(E, 2 * F, 12), tpe, offs)
    for bad in (B.bfloat16(), B[0], torch.zeros(E, 2 * F, 16), torch.zeros(E, 8, 2 * F)):
        with pytest.raises(RuntimeError, match="adapter matrix"):
            op(blocks, scales, x, v, bad, tpe, offs)
    with pytest.raises(RuntimeError, match="forward-only"):
        op(blocks, scales, x, v, B.clone().requires_grad_(True), tpe, offs)
    for rows in (x, x.bfloat16()):
        with pytest.raises(RuntimeError, match="CUDA"):                            # no CPU fallback
            op(blocks, scales, rows, v, B, tpe, offs)


def test_gated_and_backward_op_argument_errors():
    blocks, scales, tpe, offs = _operands()                                        # as the gate|up weights: N = 2F, K = H
    gated, bwd = fq().ops.moe_gated_forward_mxfp4_lora, fq().ops.moe_backward_input_mxfp4_lora
    gu, v, B = torch.zeros(T, 2 * H), torch.zeros(T, 8), torch.zeros(E, 2 * F, 8)
    with pytest.raises(RuntimeError, match="columns"):
        gated(blocks, scales, torch.zeros(T, H), v, B, tpe, offs)
    with pytest.raises(ValueError, match="activation must be"):
        gated(blocks, scales, gu, v, B, tpe, offs, activation="relu")
    with pytest.raises(RuntimeError, match="adapter matrix"):
        gated(blocks, scales, gu, v, torch.zeros(E, 8, H), tpe, offs)
    with pytest.raises(RuntimeError, match="CUDA"):
        gated(blocks, scales, gu, v, B, tpe, offs)
    gy, A = torch.zeros(T, 2 * F), torch.zeros(E, 8, H)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        bwd(blocks, scales, gy.half(), v, A, tpe, offs)
    with pytest.raises(RuntimeError, match="columns"):
        bwd(blocks, scales, torch.zeros(T, H), v, A, tpe, offs)
    with pytest.raises(RuntimeError, match="adapter matrix"):
        bwd(blocks, scales, gy, v, B, tpe, offs)                                   # B's layout where A's belongs
    with pytest.raises(RuntimeError, match="rank must be one of"):
        bwd(blocks, scales, gy, torch.zeros(T, 5), torch.zeros(E, 5, H), tpe, offs)
    with pytest.raises(RuntimeError, match="CUDA"):
        bwd(blocks, scales, gy, v, A, tpe, offs)


def test_ffn_op_argument_errors():
    op = fq().ops.moe_ffn_lora_forward_mxfp4
    gub, gus, tpe, offs = _operands()
    db, ds = torch.zeros(E, H, F // 2, dtype=torch.uint8), torch.full((E, H, F // 32), 127, dtype=torch.uint8)
    x = torch.zeros(T, H)
    ad = [torch.zeros(E, 8, H), torch.zeros(E, 2 * F, 8), torch.zeros(E, 8, F), torch.zeros(E, H, 8)]
    call = lambda x=x, ad=ad, **kw: op(gub, gus, db, ds, x, *ad, 2.0, tpe, offs, **kw)
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


# ---- the layer

def test_constructor_refusals():
    L = fq().LoRAMXFP4MoEFFN
    for rank in (0, 3, 12, 128, None):
        with pytest.raises(ValueError, match="rank must be one of"):
            L(E, H, F, rank)
    for precision in ("fp8", "fp6", "fp4"):
        with pytest.raises(ValueError, match="no backward"):
            L(E, H, F, 8, precision=precision)
    with pytest.raises(ValueError, match="precision"):
        L(E, H, F, 8, precision="int8")
    with pytest.raises(ValueError, match="float16"):
        L(E, H, F, 8, activation_dtype=torch.float16)
    with pytest.raises(ValueError, match="multiples of 32"):
        L(E, H + 16, F, 8)
    m = L(E, H, F, 16, alpha=32.0, activation="swiglu_clamp", activation_dtype=torch.bfloat16)
    assert m.rank == 16 and m.scaling == 2.0 and m.activation_dtype == torch.bfloat16 and m.input_grad is True
    assert L(E, H, F, 8, activation_dtype=torch.float32).activation_dtype is None
    assert "rank=16" in repr(m) and "alpha=32" in repr(m)


def test_state_dict_is_the_base_layers_plus_the_four_adapters():
    base = fq().MXFP4MoEFFN(E, H, F, expert_bias=True)
    m = fq().LoRAMXFP4MoEFFN(E, H, F, 8, expert_bias=True)
    assert sorted(m.state_dict()) == sorted(list(base.state_dict()) + ADAPTERS)
    assert sorted(fq().LoRAMXFP4MoEFFN(E, H, F, 8).state_dict()) == sorted(KEYS + ADAPTERS)
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
    base.load_state_dict(m.state_dict(), strict=False)
    m.load_state_dict(base.state_dict(), strict=False)


def test_from_layer_shares_storage_and_from_mxfp4_takes_the_rank():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randint(0, 255, s, generator=g, dtype=torch.uint8)
    gub, gus, db, ds = r(E, 2 * F, H // 2), r(E, 2 * F, H // 32), r(E, H, F // 2), r(E, H, F // 32)
    base = fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds, gate_up_bias=torch.randn(E, 2 * F, generator=g),
                                       down_bias=torch.randn(E, H, generator=g), activation="gelu_tanh",
                                       activation_dtype=torch.bfloat16)
    m = fq().LoRAMXFP4MoEFFN.from_layer(base, 16, alpha=8.0)
    for k in KEYS:
        assert getattr(m, k).data_ptr() == getattr(base, k).data_ptr(), k
    assert m.gate_up_bias is base.gate_up_bias and m.down_bias is base.down_bias
    assert (m.rank, m.scaling, m.activation, m.activation_dtype) == (16, 0.5, "gelu_tanh", torch.bfloat16)
    n = fq().LoRAMXFP4MoEFFN.from_mxfp4(gub, gus, db, ds, rank=4, alpha=4.0, activation="swiglu_clamp")
    assert n.rank == 4 and n.scaling == 1.0 and not n.expert_bias and torch.equal(n.gate_up_blocks, gub)
    with pytest.raises(ValueError, match="no backward"):
        fq().LoRAMXFP4MoEFFN.from_layer(fq().MXFP4MoEFFN(E, H, F, precision="fp8"), 8)
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=fq().LoRAMXFP4MoEFFN(E, H, F, 8))
    assert isinstance(blk.experts, fq().LoRAMXFP4MoEFFN)
    assert "LoRAMXFP4MoEFFN" in fq().__all__


def test_cpu_forward_raises():
    tpe, offs = torch.tensor([4, 0], dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    m = fq().LoRAMXFP4MoEFFN(E, H, F, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(4, H), tpe, offs)
