"""The input gradient of the MXFP4 expert weights, the part that needs no GPU: the C ABI of FQL_VERSION 350
(fql_moe_mx4_bwd_input: declared, exported and validated in the documented order before any HIP call -- every call below is
invalid or empty, so none launches), the argument errors of ops.moe_backward_input_mxfp4 and the input_grad keyword of
MXFP4MoEFFN up to its forward, which is GPU only."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NEW = ("fql_moe_mx4_bwd_input",)
OK, NULLP, SHAPE, ODD_K, ALIGN, DTYPE = 0, -1, -2, -3, -7, -8
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)   # 2-byte aligned only
P_BYTE = ctypes.c_void_p(17)   # not even 2-byte aligned
P_WORD = ctypes.c_void_p(20)   # 4-byte aligned, not 16


def fq():
    import fused_int4_amd
    return fused_int4_amd


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _bwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, gy=P, tpe=P, offs=P, gx=P2):
    return lib.fql_moe_mx4_bwd_input(bl, sc, gy, di, tpe, offs, gx, do, E, T, K, N, None)


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
    assert lib.fql_version() >= 350


def test_header_compiles_as_c():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const uint8_t *, const void *, int, const int32_t *, const int32_t *, void *,\n"
                    "         int, int, int, int, int, void *) = fql_moe_mx4_bwd_input;\n"
                    "int version_is_350[FQL_VERSION >= 350 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_every_pointer_null_pins_the_order_of_the_return_codes(lib):
    """With every pointer NULL a call walks the checks until the first that fails: each step below repairs the failure of
    the one before and nothing else."""
    null = dict(bl=None, sc=None, gy=None, tpe=None, offs=None, gx=None)
    assert _bwd(lib, E=0, K=65, di=F16, **null) == SHAPE                     # the dimensions first
    assert _bwd(lib, K=65, di=F16, **null) == ODD_K
    assert _bwd(lib, K=48, di=F16, **null) == SHAPE                          # K % 32: one scale per 32 outputs of dX
    assert _bwd(lib, di=F16, **null) == DTYPE                                # float16 gradients are refused, not rounded
    assert _bwd(lib, do=3, **null) == DTYPE
    assert _bwd(lib, T=0, **null) == OK                                      # the empty call before the pointers
    assert _bwd(lib, N=0, **null) == NULLP                                   # N == 0 still writes zeros: it needs grad_in
    assert _bwd(lib, **null) == NULLP
    assert _bwd(lib, E=65535, **null) == NULLP                               # the pointers before the grid's limits


def test_argument_errors_in_order(lib):
    for kw in (dict(E=0), dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert _bwd(lib, **kw) == SHAPE, kw
    assert _bwd(lib, K=65) == ODD_K
    assert _bwd(lib, K=65, E=0) == SHAPE
    for K in (16, 48, 80, 2):
        assert _bwd(lib, K=K) == SHAPE, K
    assert _bwd(lib, K=33, di=F16) == ODD_K and _bwd(lib, K=48, di=F16) == SHAPE
    assert _bwd(lib, di=F16) == DTYPE and _bwd(lib, di=3) == DTYPE and _bwd(lib, di=-1) == DTYPE
    assert _bwd(lib, do=3) == DTYPE and _bwd(lib, do=-1) == DTYPE
    for do in (F32, F16, BF16):
        assert _bwd(lib, do=do, T=0) == OK
    assert _bwd(lib, T=0, bl=None, gy=None, gx=None) == OK
    assert _bwd(lib, T=0, di=F16) == DTYPE                                   # ... but behind the types
    assert _bwd(lib, T=0, N=0, gx=None) == OK
    assert _bwd(lib, N=0, gx=None) == NULLP                                  # (N == 0 with a grad_in would launch a memset)
    for kw in (dict(bl=None), dict(sc=None), dict(gy=None), dict(gx=None), dict(tpe=None), dict(offs=None)):
        assert _bwd(lib, **kw) == NULLP, kw
    assert _bwd(lib, tpe=None, offs=None) == SHAPE                           # no table: one segment, E == 1 only
    assert _bwd(lib, E=65535) == SHAPE and _bwd(lib, E=70000) == SHAPE
    assert _bwd(lib, T=4194241) == SHAPE                                     # the grid's y
    assert _bwd(lib, bl=P_WORD) == ALIGN                                     # blocks: 16 bytes
    assert _bwd(lib, di=BF16, gy=P_BYTE) == ALIGN
    assert _bwd(lib, di=F32, gy=P_HALF) == ALIGN
    assert _bwd(lib, do=F16, gx=P_BYTE) == ALIGN
    assert _bwd(lib, do=F32, gx=P_HALF) == ALIGN


# ---- the op

def test_op_argument_errors():
    op = fq().ops.moe_backward_input_mxfp4
    E, N, K, T = 2, 40, 64, 6
    blocks, scales = torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.full((E, N, K // 32), 127, dtype=torch.uint8)
    tpe, offs = torch.tensor([3, 3], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    gy = torch.zeros(T, N)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        op(blocks, scales, gy.half(), tpe, offs)
    for bad in (gy.double(), gy.to(torch.int32), gy[0], gy[None]):
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            op(blocks, scales, bad, tpe, offs)
    for bl, sc in ((blocks.float(), scales), (blocks, scales.float()), (blocks[0], scales), (blocks, scales[0])):
        with pytest.raises(RuntimeError, match="uint8"):
            op(bl, sc, gy, tpe, offs)
    for width in (N - 1, N + 1, K):
        with pytest.raises(RuntimeError, match=r"\[T, N\]"):
            op(blocks, scales, torch.zeros(T, width), tpe, offs)
    for g in (gy, gy.bfloat16()):
        with pytest.raises(RuntimeError, match="CUDA"):                      # no CPU fallback
            op(blocks, scales, g, tpe, offs)
    assert "moe_backward_input_mxfp4" in dir(fq().ops)


# ---- the layer

E, H, F = 3, 64, 96
KEYS = ["gate_up_blocks", "gate_up_scales", "down_blocks", "down_scales"]


def test_input_grad_is_configuration_not_state():
    plain = fq().MXFP4MoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp")
    m = fq().MXFP4MoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp", input_grad=True)
    assert m.input_grad is True and plain.input_grad is False
    assert list(m.state_dict()) == list(plain.state_dict())
    assert sorted(m.state_dict()) == sorted(KEYS + ["gate_up_bias", "down_bias"])
    assert list(fq().MXFP4MoEFFN(E, H, F, input_grad=True).state_dict()) == KEYS
    assert "input_grad=True" in repr(m) and "input_grad" not in repr(plain)
    assert "input_grad" not in repr(fq().MXFP4MoEFFN(E, H, F, input_grad=False))
    plain.load_state_dict(m.state_dict())                                    # either way round
    m.load_state_dict(plain.state_dict())
    assert not m.gate_up_bias.requires_grad                                  # the biases stay frozen until asked


def test_input_grad_through_the_constructors():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    gub, gus, db, ds = r(E, 2 * F, H // 2), r(E, 2 * F, H // 32), r(E, H, F // 2), r(E, H, F // 32)
    assert fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds, input_grad=True).input_grad is True
    assert fq().MXFP4MoEFFN.from_mxfp4(gub, gus, db, ds).input_grad is False
    gate = [torch.randn(F, H, generator=g) for _ in range(E)]
    up = [torch.randn(F, H, generator=g) for _ in range(E)]
    down = [torch.randn(H, F, generator=g) for _ in range(E)]
    a = fq().MXFP4MoEFFN.from_weights(gate, up, down, input_grad=True, activation_dtype=torch.bfloat16)
    b = fq().MXFP4MoEFFN.from_weights(gate, up, down)
    assert a.input_grad is True and b.input_grad is False and a.activation_dtype == torch.bfloat16
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=a)
    assert blk.experts is a and "input_grad=True" in repr(blk)


def test_cpu_forward_still_raises():
    tpe, offs = torch.tensor([4, 0, 0], dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    for kw in (dict(), dict(input_grad=True)):
        m = fq().MXFP4MoEFFN(E, H, F, **kw)
        with pytest.raises(RuntimeError, match="GPU"):
            m(torch.zeros(4, H, requires_grad=True), tpe, offs)
        with pytest.raises(RuntimeError, match="GPU"):
            m(torch.zeros(4, H), tpe, offs)
