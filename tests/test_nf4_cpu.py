"""4-bit code-book (NF4) weights without a GPU: the quantiser and the definition, bitsandbytes' nibble order, the nested
statistics, the C ABI of FQL_VERSION 470 (declared, exported, bound, validated in mx4_check's order before any HIP call: every
call below is invalid or empty, with host pointers that are never dereferenced) and the layers on the CPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

OK, NULLP, SHAPE, ODD_K, ALIGN, DTYPE = 0, -1, -2, -3, -7, -8
F32, F16, BF16 = 0, 1, 2
P, P2 = ctypes.c_void_p(16), ctypes.c_void_p(32)       # never dereferenced
P_HALF, P_BYTE, P_WORD = ctypes.c_void_p(18), ctypes.c_void_p(17), ctypes.c_void_p(20)


def fq():
    import fused_int4_amd
    return fused_int4_amd


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def _case(N=5, K=128, block=64, seed=0):
    """Table values times a power-of-two absmax: every block holds +-1 (so absmax is recovered) and random codes."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g)
    codes[:, ::block] = 15                                                    # the block's largest magnitude: 1.0 * absmax
    absmax = torch.ldexp(torch.ones(N, K // block), torch.randint(-3, 4, (N, K // block), generator=g))
    book = torch.tensor(fq().NF4_CODE_BOOK, dtype=torch.float32)
    w = book[codes] * absmax.repeat_interleave(block, dim=1)
    return codes, absmax, w


@pytest.mark.parametrize("block", [64, 128])
def test_round_trip_and_nibble_order(block):
    codes, absmax, w = _case(K=256, block=block)
    q, am = fq().quantize_lut4(w, block=block)
    assert fq().quantize_nf4 is fq().quantize_lut4
    assert q.dtype == torch.uint8 and tuple(q.shape) == (5, 128) and torch.equal(am, absmax)
    assert torch.equal(q >> 4, codes[:, 0::2].to(torch.uint8)) and torch.equal(q & 15, codes[:, 1::2].to(torch.uint8))
    assert int(q[0, 0]) >> 4 == 15                                            # input 0 in bits 7..4
    d = fq().dequantize_lut4(q, am, block=block)
    assert d.dtype == torch.bfloat16 and torch.equal(d, w.bfloat16())         # (a power-of-two scale: only the one rounding)
    with pytest.raises(ValueError, match="block"):
        fq().quantize_lut4(w, block=96)
    with pytest.raises(ValueError, match="block"):
        fq().quantize_lut4(w[:, :96])


def test_nested_absmax_by_hand():
    code256 = torch.arange(256, dtype=torch.float32) / 128 - 1
    u8 = torch.tensor([0, 128, 255, 64, 192], dtype=torch.uint8)
    got = fq().bnb_nested_absmax(u8, code256, torch.tensor([2.0, 4.0, 8.0]), 0.5, nested_block=2)
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.tensor([-1.5, 0.5, 127 / 128 * 4 + 0.5, -0.5 * 4 + 0.5, 0.5 * 8 + 0.5]))


def _fwd(lib, di=BF16, do=BF16, T=8, K=128, N=40, block=64, c=P, a=P, book=None, x=P, b=None, o=P2):
    return lib.fql_linear_lut4_fwd(c, a, book, block, x, di, b, o, do, T, K, N, None)


def _bwd(lib, di=BF16, do=BF16, T=8, K=128, N=40, block=64, c=P, a=P, book=None, x=P, o=P2):
    return lib.fql_linear_lut4_bwd_input(c, a, book, block, x, di, o, do, T, K, N, None)


def test_abi_symbols_version_and_check_order(lib):
    import test_c_abi
    from fused_int4_amd import _native
    raw = ctypes.CDLL(lib._name)
    for name, nargs in (("fql_linear_lut4_fwd", 13), ("fql_linear_lut4_bwd_input", 12)):
        assert name in test_c_abi.declared_symbols() and hasattr(raw, name) and name in _native.exported_symbols()
        assert len(getattr(lib, name).argtypes) == nargs
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) >= 470 and int(m.group(1)) == lib.fql_version()
    null = dict(c=None, a=None, x=None, o=None)
    for call in (_fwd, _bwd):                                                 # each step repairs the failure before it
        assert call(lib, T=-1, K=65, block=48, di=F16, **null) == SHAPE
        assert call(lib, K=65, block=48, di=F16, **null) == ODD_K
        assert call(lib, K=96, block=48, di=F16, **null) == SHAPE             # K % 64
        for block in (48, 32, 96, 256, 0, -64):                               # no power of two, < 64, K % block
            assert call(lib, block=block, di=F16, **null) == SHAPE, block
        assert call(lib, di=F16, **null) == DTYPE and call(lib, do=3, **null) == DTYPE
        assert call(lib, T=0, **null) == OK                                   # the empty call before the pointers
        assert call(lib, **null) == NULLP
        for kw in (dict(c=None), dict(a=None), dict(x=None), dict(o=None)):
            assert call(lib, **kw) == NULLP, kw
        assert call(lib, T=65535 * 256 + 1, c=P_WORD) == SHAPE                # the grid before the alignment
        for kw in (dict(c=P_WORD), dict(a=P_HALF), dict(book=P_HALF), dict(x=P_BYTE), dict(di=F32, x=P_HALF),
                   dict(do=F32, o=P_HALF)):
            assert call(lib, **kw) == ALIGN, kw
    assert _fwd(lib, b=P_HALF) == ALIGN
    assert _fwd(lib, N=0, **null) == OK and _bwd(lib, N=0, **null) == NULLP   # (the gradient of N == 0 writes zeros)


def test_ops_check_types_and_shapes_before_devices():
    ops = fq().ops
    c, a, x = torch.zeros(40, 64, dtype=torch.uint8), torch.ones(40, 2), torch.zeros(6, 128)
    for call, rows in ((ops.linear_forward_lut4, x), (ops.linear_backward_input_lut4, torch.zeros(6, 40))):
        with pytest.raises(RuntimeError, match="float16 is refused"):
            call(c, a, rows.half())
        with pytest.raises(RuntimeError, match="uint8"):
            call(c.float(), a, rows)
        with pytest.raises(RuntimeError, match="block"):
            call(c, a, rows, block=96)
        with pytest.raises(RuntimeError, match="absmax"):
            call(c, a, rows, block=128)
        with pytest.raises(RuntimeError, match="columns"):
            call(c, a, rows[:, :-1])
        with pytest.raises(RuntimeError, match="code_book"):
            call(c, a, rows, code_book=torch.zeros(15))
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):      # everything else is fine: the device is last
            call(c, a, rows)


def test_layers_on_the_cpu_are_the_definition():
    L, LL = fq().NF4Linear, fq().LoRANF4Linear
    codes, absmax, w = _case(N=8, K=128)
    q, am = fq().quantize_lut4(w)
    bias = torch.arange(8, dtype=torch.float32)
    m = L.from_bnb(q.reshape(-1, 1), am.reshape(-1), bias=bias, out_features=8)        # bitsandbytes' own shapes
    assert torch.equal(m.codes, q) and torch.equal(m.absmax, am) and m.block == 64
    assert list(m.state_dict()) == ["codes", "absmax", "code_book", "bias"]
    assert list(L(128, 8).state_dict()) == ["codes", "absmax", "code_book"]
    x = torch.randn(2, 3, 128, generator=torch.Generator().manual_seed(1))
    ref = x.bfloat16().float() @ w.bfloat16().float().T + bias
    assert torch.equal(m(x), ref) and torch.equal(m(x.bfloat16()), ref.bfloat16())
    assert torch.equal(L(128, 8)(x), torch.zeros(2, 3, 8))                    # a fresh layer is the zero matrix
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.from_bnb(q, am, input_grad=True)(x.clone().requires_grad_(True))
    lin = torch.nn.Linear(128, 8)
    assert torch.equal(L.from_linear(lin).codes, fq().quantize_lut4(lin.weight.detach())[0])
    lo = LL.from_layer(m, rank=8, alpha=16.0)
    assert lo.codes is m.codes and lo.scaling == 2.0 and bool((lo.lora_B == 0).all())
    assert sorted(lo.state_dict()) == sorted(["codes", "absmax", "code_book", "bias", "lora_A", "lora_B"])
    assert sorted(LL.from_bnb(q, am, rank=4).adapter_state_dict()) == ["lora_A", "lora_B"]
    with pytest.raises(RuntimeError, match="GPU"):
        lo(x)
