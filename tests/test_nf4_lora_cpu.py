"""The fused adapter forms of the NF4 tile kernels without a GPU (FQL_VERSION 490): the two C entries
declared, exported, bound and refusing before any HIP call (every call below is invalid or empty, so none launches), the ops'
operand checks, and the layer's ``fused`` keyword."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

OK, NULLP, SHAPE, ODD_K, ALIGN, DTYPE = 0, -1, -2, -3, -7, -8
F16, BF16 = 1, 2
P, P_HALF, P_WORD = ctypes.c_void_p(16), ctypes.c_void_p(18), ctypes.c_void_p(20)   # never dereferenced; 2- and 4-byte aligned only
K, N, T = 64, 96, 6


def _fwd(lib, di=BF16, do=BF16, T=8, K=K, N=N, r=8, block=64, c=P, a=P, x=P, v=P, w=P, out=P):
    return lib.fql_linear_lut4_lora_fwd(c, a, None, block, x, di, v, w, r, None, out, do, T, K, N, None)


def _bwd(lib, di=BF16, do=BF16, T=8, K=K, N=N, r=8, block=64, c=P, a=P, x=P, v=P, w=P, out=P):
    return lib.fql_linear_lut4_lora_bwd_input(c, a, None, block, x, di, v, w, r, out, do, T, K, N, None)


@pytest.mark.parametrize("entry,name", ((_fwd, "fql_linear_lut4_lora_fwd"), (_bwd, "fql_linear_lut4_lora_bwd_input")))
def test_c_entries_declared_bound_and_refusing_in_order(entry, name):
    """lut4_check's order, the adapter checks in their places: the rank behind the types, the pointers and alignment with the others."""
    import test_c_abi
    from fused_int4_amd import _native
    lib = _native.lib()
    assert name in test_c_abi.declared_symbols() and name in _native.exported_symbols() and hasattr(ctypes.CDLL(lib._name), name)
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        assert lib.fql_version() == int(re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read()).group(1)) >= 490
    null = dict(c=None, a=None, x=None, v=None, w=None, out=None)
    assert entry(lib, K=65, di=F16, r=3, **null) == ODD_K
    assert entry(lib, K=96, di=F16, r=3, **null) == SHAPE and entry(lib, block=32, di=F16, r=3, **null) == SHAPE
    assert entry(lib, di=F16, r=3, **null) == DTYPE and entry(lib, do=3, r=3, **null) == DTYPE   # float16 rows are refused
    assert entry(lib, T=0, r=3, **null) == SHAPE and entry(lib, T=0, **null) == OK               # the rank before the empty call
    assert entry(lib, **null) == NULLP
    for r in (0, -8, 1, 2, 3, 5, 12, 24, 48, 65, 128):
        assert entry(lib, r=r) == SHAPE, r
    for r in (4, 8, 16, 32, 64):
        assert entry(lib, r=r, T=0) == OK and entry(lib, r=r, c=None) == NULLP
    assert entry(lib, v=None) == NULLP and entry(lib, w=None) == NULLP
    assert entry(lib, T=65535 * 256 + 1, v=None) == NULLP and entry(lib, T=65535 * 256 + 1) == SHAPE   # pointers, then the grid
    assert entry(lib, v=P_HALF) == ALIGN and entry(lib, w=P_HALF) == ALIGN and entry(lib, c=P_WORD) == ALIGN
    assert entry(lib, N=0, T=0) == OK and entry(lib, N=0) == (SHAPE if entry is _bwd else OK)   # no adapter form of the empty contraction


def test_op_operand_checks_raise_before_any_device_is_touched():
    import fused_int4_amd as fq
    o = fq.ops
    codes, absmax = torch.zeros(N, K // 2, dtype=torch.uint8), torch.ones(N, K // 64)
    x, gy, v, A, B = torch.zeros(T, K), torch.zeros(T, N), torch.zeros(T, 8), torch.zeros(8, K), torch.zeros(N, 8)
    for op, rows, w, other in ((o.linear_forward_lut4_lora, x, B, A), (o.linear_backward_input_lut4_lora, gy, A, B)):
        with pytest.raises(RuntimeError, match="float16 is refused"):
            op(codes, absmax, rows.half(), v.half(), w)                            # the rows first
        for bad in (v.bfloat16(), v[:-1], v[0]):                                   # then the adapter operands
            with pytest.raises(RuntimeError, match="shrunk rows"):
                op(codes, absmax, rows, bad, w.half())
        with pytest.raises(RuntimeError, match="rank must be one of"):
            op(codes, absmax, rows, torch.zeros(T, 12), torch.zeros(12, 12))
        for bad in (w.bfloat16(), other, w[None]):
            with pytest.raises(RuntimeError, match="adapter matrix"):
                op(codes, absmax, rows, v, bad, out_dtype=torch.int8)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):            # no CPU fallback
            op(codes, absmax, rows, v, w)
    with pytest.raises(RuntimeError, match="forward-only"):
        o.linear_forward_lut4_lora(codes, absmax, x, v, B.clone().requires_grad_(True))
    pytest.raises(ValueError, o.linear_lora_forward_lut4, x, codes, absmax, A, B, 2.0, split_k=True, fused=True)


def test_fused_is_configuration_not_state():
    import fused_int4_amd as fq
    L, base = fq.LoRANF4Linear, fq.NF4Linear(K, N, bias=True)
    plain, fused = L(K, N, 8, bias=True), L(K, N, 8, bias=True, fused=True)
    assert sorted(fused.state_dict()) == sorted(plain.state_dict()) == sorted(list(base.state_dict()) + ["lora_A", "lora_B"])
    assert fused.fused is True and plain.fused is False and "fused=True" in repr(fused) and "fused" not in repr(plain)
    pytest.raises(ValueError, L, K, N, 8, fused=True, split_k=True)
    assert L.from_bnb(base.codes, base.absmax, rank=4, fused=True).fused and not L.from_bnb(base.codes, base.absmax, rank=4).fused
    assert L.from_linear(torch.nn.Linear(K, N), rank=4, fused=True).fused
    assert L.from_layer(base, 16, fused=True).fused and not L.from_layer(base, 16).fused
    pytest.raises(RuntimeError, fused, torch.zeros(2, K))                           # the adapter path runs on the GPU only
