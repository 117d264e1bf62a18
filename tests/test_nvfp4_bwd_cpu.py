"""The input gradient of the NVFP4 weights, the part that needs no GPU: the C ABI of FQL_VERSION 440
(fql_moe_nvfp4_bwd_input: declared, exported, bound and validated in mx4_check's order before any HIP call -- every call
below is invalid or empty, with host pointers that are never dereferenced, so none launches), the argument errors of
ops.moe_backward_input_nvfp4 / ops.linear_backward_input_nvfp4 (types and shapes before devices) and the input_grad keyword
of NVFP4MoEFFN and NVFP4Linear up to their GPU-only gradient."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT

NEW = ("fql_moe_nvfp4_bwd_input",)
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


def _bwd(lib, di=BF16, do=BF16, E=2, T=8, K=64, N=96, bl=P, sc=P, gs=P, gy=P, tpe=P, offs=P, gx=P2):
    return lib.fql_moe_nvfp4_bwd_input(bl, sc, gs, gy, di, tpe, offs, gx, do, E, T, K, N, None)


# ---- the C boundary

def test_declared_exported_bound_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
        assert getattr(lib, name).restype is ctypes.c_int and len(getattr(lib, name).argtypes) == 14, name
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) >= 440 and int(m.group(1)) == lib.fql_version()


def test_header_compiles_as_c_with_the_documented_signature():
    header = os.path.join(ROOT, "include", "fql_int4.h")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n'
                    "int (*a)(const uint8_t *, const uint8_t *, const float *, const void *, int, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *) = fql_moe_nvfp4_bwd_input;\n"
                    "int version_is_440[FQL_VERSION >= 440 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(header), "-c", src,
                               "-o", os.path.join(tmp, "use.o")])


def test_every_pointer_null_pins_the_order_of_the_return_codes(lib):
    """With every pointer NULL a call walks the checks until the first that fails: each step below repairs the failure of
    the one before and nothing else."""
    null = dict(bl=None, sc=None, gs=None, gy=None, tpe=None, offs=None, gx=None)
    assert _bwd(lib, E=0, K=65, di=F16, **null) == SHAPE                     # the dimensions first
    assert _bwd(lib, K=65, di=F16, **null) == ODD_K
    assert _bwd(lib, K=48, di=F16, **null) == SHAPE                          # K % 32: a staging piece is 32 k
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
    assert _bwd(lib, T=0, bl=None, gy=None, gx=None, gs=None) == OK
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
    assert _bwd(lib, gs=P_HALF) == ALIGN                                     # global_scale: 4 bytes ...
    assert _bwd(lib, gs=P_HALF, E=65535) == SHAPE                            # ... behind the grid's limits
    assert _bwd(lib, sc=None, gs=P_HALF) == NULLP                            # ... and behind the pointers


# ---- the ops

def test_ops_check_types_and_shapes_before_devices():
    ops = fq().ops
    grouped, dense = ops.moe_backward_input_nvfp4, ops.linear_backward_input_nvfp4
    E, N, K, T = 2, 40, 64, 6
    b, s, gs = torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.full((E, N, K // 16), 0x38, dtype=torch.uint8), torch.ones(E)
    tpe, offs = torch.tensor([3, 3], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    gy = torch.zeros(T, N)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        grouped(b, s, gs, gy.half(), tpe, offs)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        dense(b[0], s[0], None, gy.half())
    for bad in (gy.double(), gy.to(torch.int32), gy[0], gy[None]):
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            grouped(b, s, gs, bad, tpe, offs)
    for bl, sc in ((b.float(), s), (b, s.float()), (b[0], s), (b, s[0])):
        with pytest.raises(RuntimeError, match="uint8"):                     # the weights behind the rows' type
            grouped(bl, sc, gs, gy, tpe, offs)
    with pytest.raises(RuntimeError, match=r"\[N, K/2\]"):
        dense(b, s, None, gy)
    with pytest.raises(RuntimeError, match="K/16"):
        grouped(b, s[:, :, :2], gs, gy, tpe, offs)
    with pytest.raises(RuntimeError, match="K % 32"):
        grouped(b[:, :, :24], s[:, :, :3], gs, gy, tpe, offs)
    for width in (N - 1, N + 1, K):
        with pytest.raises(RuntimeError, match=r"\[T, N\]"):
            grouped(b, s, gs, torch.zeros(T, width), tpe, offs)
        with pytest.raises(RuntimeError, match=r"\[T, N\]"):
            dense(b[0], s[0], None, torch.zeros(T, width))
    with pytest.raises(RuntimeError, match="global_scale"):                  # the shapes before the global scale
        grouped(b, s, gs[:1], gy, tpe, offs)
    with pytest.raises(RuntimeError, match="global_scale"):
        grouped(b, s, gs.double(), gy, tpe, offs)
    with pytest.raises(RuntimeError, match="global_scale"):
        dense(b[0], s[0], gs, gy)
    with pytest.raises(RuntimeError, match=r"\[T, N\]"):
        grouped(b, s, gs[:1], torch.zeros(T, K), tpe, offs)
    with pytest.raises(RuntimeError, match="out_dtype"):                     # the global scale before out_dtype
        grouped(b, s, gs, gy, tpe, offs, out_dtype=torch.float64)
    with pytest.raises(RuntimeError, match="global_scale"):
        grouped(b, s, gs[:1], gy, tpe, offs, out_dtype=torch.float64)
    for call in (lambda: grouped(b, s, gs, gy, tpe, offs), lambda: grouped(b, s, None, gy.bfloat16(), tpe, offs),
                 lambda: grouped(b, s, gs, gy, tpe, offs, out_dtype=torch.float16),
                 lambda: dense(b[0], s[0], gs[:1], gy), lambda: dense(b[0], s[0], None, gy.bfloat16(), out_dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):     # everything else is fine: the device is last
            call()


# ---- the layers

E, H, F = 3, 64, 96
KEYS = ["gate_up_blocks", "gate_up_scales", "gate_up_global", "down_blocks", "down_scales", "down_global"]


def test_ffn_input_grad_is_configuration_not_state():
    plain = fq().NVFP4MoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp")
    m = fq().NVFP4MoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp", input_grad=True)
    assert m.input_grad is True and plain.input_grad is False
    assert list(m.state_dict()) == list(plain.state_dict())
    assert sorted(m.state_dict()) == sorted(KEYS + ["gate_up_bias", "down_bias"])
    assert list(fq().NVFP4MoEFFN(E, H, F, input_grad=True).state_dict()) == KEYS
    assert "input_grad=True" in repr(m) and "input_grad" not in repr(plain)
    assert "input_grad" not in repr(fq().NVFP4MoEFFN(E, H, F, input_grad=False))
    plain.load_state_dict(m.state_dict())                                    # either way round
    m.load_state_dict(plain.state_dict())
    assert not m.gate_up_bias.requires_grad                                  # the biases stay frozen until asked


def test_ffn_input_grad_through_the_constructors():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    gub, gus, db, ds = r(E, 2 * F, H // 2), r(E, 2 * F, H // 16), r(E, H, F // 2), r(E, H, F // 16)
    N4 = fq().NVFP4MoEFFN
    assert N4.from_nvfp4(gub, gus, None, db, ds, torch.ones(E), input_grad=True).input_grad is True
    assert N4.from_nvfp4(gub, gus, None, db, ds, None).input_grad is False
    gate = [torch.randn(F, H, generator=g) for _ in range(E)]
    up = [torch.randn(F, H, generator=g) for _ in range(E)]
    down = [torch.randn(H, F, generator=g) for _ in range(E)]
    a = N4.from_weights(gate, up, down, input_grad=True, activation_dtype=torch.bfloat16)
    b = N4.from_weights(gate, up, down)
    assert a.input_grad is True and b.input_grad is False and a.activation_dtype == torch.bfloat16
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    blk = fq().QuantizedSparseMoEBlock(E, H, F, top_k=2, experts=a)
    assert blk.experts is a and "input_grad=True" in repr(blk)


def test_ffn_cpu_forward_still_raises():
    tpe, offs = torch.tensor([4, 0, 0], dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    for kw in (dict(), dict(input_grad=True)):
        m = fq().NVFP4MoEFFN(E, H, F, **kw)
        with pytest.raises(RuntimeError, match="GPU"):
            m(torch.zeros(4, H, requires_grad=True), tpe, offs)
        with pytest.raises(RuntimeError, match="GPU"):
            m(torch.zeros(4, H), tpe, offs)


def test_linear_input_grad_round_trips_and_runs_on_the_gpu_only():
    L = fq().NVFP4Linear
    g = torch.Generator().manual_seed(2)
    lin = torch.nn.Linear(64, 8, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(8, 64, generator=g))
    plain, m = L.from_linear(lin), L.from_linear(lin, input_grad=True)
    assert m.input_grad is True and plain.input_grad is False
    assert L(64, 8, input_grad=True).input_grad is True and L(64, 8).input_grad is False
    assert L.from_nvfp4(m.blocks, m.scales, m.global_scale, input_grad=True).input_grad is True
    assert L.from_nvfp4(m.blocks, m.scales, m.global_scale).input_grad is False
    assert list(m.state_dict()) == list(plain.state_dict()) == ["blocks", "scales", "global_scale", "bias"]
    assert "input_grad=True" in repr(m) and "input_grad" not in repr(plain)
    plain.load_state_dict(m.state_dict())
    m.load_state_dict(plain.state_dict())
    x = torch.randn(2, 3, 64, generator=g)
    with pytest.raises(RuntimeError, match="the input gradient runs on the GPU only"):
        m(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="inference-only"):                # the default layer as it was
        plain(x.clone().requires_grad_(True))
    with torch.no_grad():                                                    # the CPU forward under no_grad is unchanged
        y = m(x.clone().requires_grad_(True))
    assert y.shape == (2, 3, 8) and torch.equal(y, plain(x)) and torch.equal(y, m(x))


def test_default_layers_still_raise_inference_only():
    """NVFP4Linear on the CPU; NVFP4MoEFFN looks at the device first (test_ffn_cpu_forward_still_raises), so its message
    is pinned in tests/test_gpu_nvfp4_bwd.py."""
    for m in (fq().NVFP4Linear(64, 8), fq().NVFP4Linear(64, 8, input_grad=False)):
        with pytest.raises(RuntimeError, match=r"inference-only.*input_grad=True"):
            m(torch.zeros(2, 64, requires_grad=True))
    assert fq().NVFP4MoEFFN(E, H, F).input_grad is False
