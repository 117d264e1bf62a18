"""The dense MXFP4 linear layer (FQL_VERSION 420), the part that needs no GPU: the C ABI of fql_linear_mx4_fwd /
fql_linear_mx4_glu_fwd / fql_linear_mx4_workspace_bytes and the three tuning hooks (declared, exported, validated in
fql_moe_mx4_fwd's order before any HIP call -- every call below is invalid, empty or stops at the workspace check, with
host pointers that are never dereferenced), the workspace arithmetic, the slice policy as the reporting hook shows it, and
``MXFP4Linear`` / the ops' argument errors on the CPU."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT

NEW = ("fql_linear_mx4_workspace_bytes", "fql_linear_mx4_fwd", "fql_linear_mx4_glu_fwd")
HOOKS = ("fql_tune_set_mx4_linear_decode_max_rows", "fql_tune_set_mx4_linear_slices", "fql_tune_mx4_linear_kernel")
INT_MAX = 2 ** 31 - 1
T_MAX = 4194240                # the largest T mx4_check admits
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)
P_WORD = ctypes.c_void_p(20)
KS, NS, TS = (32, 96, 288, 544, 1024), (8, 40, 136), (1, 2, 33, 70)


def fq():
    import fused_int4_amd
    return fused_int4_amd


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


@pytest.fixture
def hooks(lib):
    """The two setters; the values the library was built with come back afterwards."""
    rows, slices = lib.fql_tune_set_mx4_linear_decode_max_rows(-1), lib.fql_tune_set_mx4_linear_slices(-1)
    try:
        yield lib.fql_tune_set_mx4_linear_decode_max_rows, lib.fql_tune_set_mx4_linear_slices
    finally:
        lib.fql_tune_set_mx4_linear_decode_max_rows(rows)
        lib.fql_tune_set_mx4_linear_slices(slices)
    assert lib.fql_tune_set_mx4_linear_decode_max_rows(-1) == rows and lib.fql_tune_set_mx4_linear_slices(-1) == slices


def _fwd(lib, di=BF16, do=BF16, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, out=P2, split=1, ws=None, nbytes=0):
    return lib.fql_linear_mx4_fwd(bl, sc, x, di, bias, out, do, T, K, N, split, ws, nbytes, None)


def _glu(lib, di=F32, do=F32, T=8, K=64, N=96, bl=P, sc=P, x=P, bias=P, out=P2, split=1, ws=None, nbytes=0, act=2, alpha=1.702,
         limit=7.0):
    return lib.fql_linear_mx4_glu_fwd(bl, sc, x, di, bias, out, do, T, K, N, act, alpha, limit, split, ws, nbytes, None)


ENTRIES = (_fwd, _glu)
NONE = dict(bl=None, sc=None, x=None, bias=None, out=None)


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
    assert lib.fql_version() >= 420
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        boundary = f.read()
    m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", boundary)
    assert m and int(m.group(1)) >= 420 and int(m.group(1)) == lib.fql_version()
    tune = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fql_int4_tune.h")).read(), flags=re.S)
    boundary = re.sub(r"/\*.*?\*/", "", boundary, flags=re.S)
    for name in HOOKS:
        assert re.search(r"FQL_API\s+int\s+" + name + r"\s*\(", tune), name
        assert name not in boundary, name                      # tools and tests only: not part of the drop-in boundary
        assert hasattr(raw, name) and name in _native.exported_symbols(), name


def test_header_compiles_as_c_with_the_documented_signatures():
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "use.c")
        with open(src, "w") as f:
            f.write('#include "fql_int4.h"\n#include "fql_int4_tune.h"\n'
                    "size_t (*w)(int, int, int, int, int) = fql_linear_mx4_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const uint8_t *, const void *, int, const float *, void *, int, int, int, int, int,\n"
                    "         void *, size_t, void *) = fql_linear_mx4_fwd;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const void *, int, const float *, void *, int, int, int, int, int,\n"
                    "         float, float, int, void *, size_t, void *) = fql_linear_mx4_glu_fwd;\n"
                    "int (*h0)(int) = fql_tune_set_mx4_linear_decode_max_rows;\n"
                    "int (*h1)(int) = fql_tune_set_mx4_linear_slices;\n"
                    "int (*h2)(int, int, int) = fql_tune_mx4_linear_kernel;\n"
                    "int version_is_420[FQL_VERSION >= 420 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", src, "-o",
                               os.path.join(tmp, "use.o")])


@pytest.mark.parametrize("split", [0, 1], ids=["plain", "split"])
@pytest.mark.parametrize("entry", ENTRIES, ids=["fwd", "glu"])
def test_return_codes_in_the_documented_order(lib, entry, split):
    """fql_moe_mx4_fwd's order with E = 1 and no table, every check in front of any HIP call, the workspace last."""
    call = lambda **kw: entry(lib, split=split, **kw)
    for kw in (dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert call(**NONE, **kw) == SHAPE, kw
    assert call(**NONE, K=65) == ODD_K
    assert call(**NONE, K=65, T=-1) == SHAPE
    for K in (16, 48, 80, 2):
        assert call(**NONE, K=K) == SHAPE, K
    assert call(**NONE, K=33, di=F16) == ODD_K
    assert call(**NONE, di=F16) == DTYPE and call(**NONE, di=3) == DTYPE and call(**NONE, do=3) == DTYPE
    assert call(**NONE, T=0) == OK and call(**NONE, N=0) == OK          # empty: nothing launched, nothing else looked at
    assert call(**NONE, T=0, di=F16) == DTYPE
    assert call(**NONE) == NULLP
    for name in ("bl", "sc", "x", "out"):
        assert call(**{name: None}) == NULLP, name
    assert call(T=T_MAX + 1) == SHAPE and call(T=T_MAX + 1, bl=None) == NULLP   # the pointers before the grid's limits
    assert call(bl=P_WORD) == ALIGN and call(bias=P_HALF) == ALIGN
    assert call(x=ctypes.c_void_p(17)) == ALIGN and call(out=ctypes.c_void_p(33)) == ALIGN
    if entry is _glu:
        assert call(act=3) == SHAPE and call(limit=0.0) == SHAPE and call(alpha=float("nan")) == SHAPE
        assert call(act=3, K=65) == SHAPE                                 # the activation with the first shape check
    if entry is _glu or split:
        need = lib.fql_linear_mx4_workspace_bytes(8, 64, 96, int(entry is _glu), split)
        assert need > 0
        assert call() == WS and call(bias=None) == WS                     # everything else is fine: the workspace is last
        assert call(ws=P, nbytes=need - 1) == WS                          # short
        assert call(ws=P_WORD, nbytes=need) == WS                         # misaligned
        assert call(ws=None, nbytes=need) == WS
        assert call(ws=P, nbytes=need, bl=P_WORD) == ALIGN                # ... and behind every other check


def test_workspace_bytes(lib, hooks):
    rows, _ = hooks
    w = lib.fql_linear_mx4_workspace_bytes
    rows(64)
    r16 = lambda v: (v + 15) // 16 * 16
    for T in (1, 2, 33, 64):
        for K in (32, 96, 1024):
            for N in (8, 40, 136):
                h = r16(2 * T * K)
                assert w(T, K, N, 0, 0) == 0
                assert w(T, K, N, 1, 0) == h == lib.fql_moe_mx4_workspace_bytes(1, T, K, N, 1)
                assert w(T, K, N, 0, 1) == 64 * T * N                     # 16 slices of [T][N] float32, whatever S(K, N)
                assert w(T, K, N, 1, 1) == h + 64 * T * N
                assert w(T, K, N, 1, 7) == h + 64 * T * N                 # split_k is a flag
    assert w(65, 64, 96, 0, 1) == 0 and w(65, 64, 96, 1, 1) == r16(2 * 65 * 64)    # above the threshold: no partials
    assert w(0, 64, 96, 1, 1) == 0 and w(-1, 64, 96, 1, 1) == 0 and w(8, 64, 0, 0, 1) == 0 and w(8, 0, 96, 1, 0) == 0
    rows(0)
    assert w(1, 64, 96, 0, 1) == 0
    # no int overflow at the bounds the checks admit: T = 4194240, K and N up to the largest int
    rows(INT_MAX)
    k_max, n_max = INT_MAX - 31, INT_MAX
    assert w(T_MAX, 32, n_max, 0, 1) == 64 * T_MAX * n_max
    assert w(T_MAX, k_max, 8, 1, 0) == r16(2 * T_MAX * k_max)
    assert w(T_MAX, k_max, n_max, 1, 1) == r16(2 * T_MAX * k_max) + 64 * T_MAX * n_max < 2 ** 64


def test_hooks_return_the_previous_value_and_refuse_what_they_do_not_know(lib, hooks):
    rows, slices = hooks
    default = rows(17)
    with open(os.path.join(ROOT, "fused-4-bit-dequantize-linear-cuda-kernel_amd", "csrc", "fql_mx4.hip")) as f:
        built = re.search(r"#define\s+FQL_MX4_LINEAR_DECODE_MAX_ROWS\s+(\d+)", f.read())
    assert built and default == int(built.group(1)) >= 0               # the library's own value, set from the sweep
    assert rows(64) == 17 and rows(0) == 64 and rows(INT_MAX) == 0
    assert rows(-5) == INT_MAX and rows(-1) == INT_MAX                   # refused, nothing changed
    assert slices(0) in (0, 1, 2, 4, 8, 16)
    prev = 0
    for s in (1, 2, 4, 8, 16, 0, 16):
        assert slices(s) == prev
        prev = s
    for bad in (3, 32, -1, 5, 6, 7, 12, 17, 64, INT_MAX, -16):
        assert slices(bad) == 16                                          # returns the value in force ...
    assert slices(0) == 16                                                # ... which nothing above has changed
    assert slices(0) == 0


def test_reported_kernel(lib, hooks):
    rows, slices = hooks
    k = lib.fql_tune_mx4_linear_kernel
    dec = lib.fql_tune_mx4_kernel
    rows(64)
    slices(0)
    for K in KS + (64, 128, 2880, 4096, 8192, 28672):
        for N in NS + (1, 32, 2880, 5120, 8192, 28672, 32768, 65536):
            got = [k(T, K, N) for T in (1, 2, 33, 64)]
            assert len(set(got)) == 1, (K, N)                             # S is a function of (K, N), never of T
            S, form = got[0] >> 8, got[0] & 0xFF
            assert S in (1, 2, 4, 8, 16) and S <= max(1, K // 64), (K, N, S)
            assert form == (2 if S > 1 else dec(1, 1, K, N)), (K, N)
            if S < 16 and 2 * S <= max(1, K // 64):
                assert -(-N // 32) * S >= 640, (K, N, S)                   # the smallest S with that many waves ...
            if S > 1:
                assert -(-N // 32) * (S // 2) < 640, (K, N, S)             # ... (FQL_MX4_LINEAR_FILL_WAVES in csrc/fql_mx4.hip)
            for T in (65, 70, 4096):                                      # above the threshold: S = 1, the grouped choice
                assert k(T, K, N) == (1 << 8) | dec(1, T, K, N), (T, K, N)
            assert k(0, K, N) == (1 << 8) | dec(1, 0, K, N)
    # the test shapes: P = 0, 1, 4, 8, 16 whole pairs cap the policy at 1, 1, 4, 8, 16
    assert [k(1, K, 40) >> 8 for K in KS] == [1, 1, 4, 8, 16]
    # the measured shapes
    assert [k(1, K, N) >> 8 for K, N in ((2880, 5120), (4096, 2880), (8192, 8192), (8192, 28672), (28672, 8192))] == [4, 8, 4, 1, 4]
    for S in (1, 2, 4, 8, 16):                                            # forced: every shape, S above P too
        slices(S)
        for K in KS:
            assert k(1, K, 8) == ((S << 8) | (2 if S > 1 else dec(1, 1, K, 8)))
            assert k(65, K, 8) >> 8 == 1
    slices(0)
    rows(0)
    assert k(1, 1024, 40) >> 8 == 1
    rows(INT_MAX)
    assert k(32 * 65535, 1024, 40) >> 8 == 16 and k(32 * 65535 + 1, 1024, 40) >> 8 == 1     # the grid's y


# ---- the layer and the ops on the CPU

def _weights(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g) * 0.1, g


def test_exported():
    assert "MXFP4Linear" in fq().__all__ and hasattr(fq(), "MXFP4Linear")
    for name in ("linear_forward_mxfp4", "linear_gated_forward_mxfp4", "linear_backward_input_mxfp4"):
        assert hasattr(fq().ops, name), name


@pytest.mark.parametrize("bias", [False, True])
def test_state_dict_and_from_linear(bias):
    from fused_int4_amd.quantize import quantize_mxfp4
    K, N = 96, 40
    m = fq().MXFP4Linear(K, N, bias=bias)
    sd = m.state_dict()
    assert sorted(sd) == (["bias"] if bias else []) + ["blocks", "scales"]
    assert tuple(sd["blocks"].shape) == (N, K // 2) and sd["blocks"].dtype == torch.uint8
    assert tuple(sd["scales"].shape) == (N, K // 32) and sd["scales"].dtype == torch.uint8
    if bias:
        assert tuple(sd["bias"].shape) == (N,) and sd["bias"].dtype == torch.float32
    assert not list(m.parameters())                                       # frozen: buffers only
    lin = torch.nn.Linear(K, N, bias=bias)
    q = fq().MXFP4Linear.from_linear(lin, split_k=False)
    blocks, scales = quantize_mxfp4(lin.weight.detach())
    assert torch.equal(q.blocks, blocks) and torch.equal(q.scales, scales)             # bit for bit
    assert (q.bias is None) == (not bias) and (not bias or torch.equal(q.bias, lin.bias.detach()))
    assert sorted(q.state_dict()) == sorted(sd)
    m.load_state_dict(q.state_dict())
    assert torch.equal(m.blocks, blocks) and torch.equal(m.scales, scales)
    r = repr(q)
    assert "in_features=96" in r and "out_features=40" in r and "mxfp4" in r and "split_k=False" in r
    assert "input_grad" not in r and "input_grad=True" in repr(fq().MXFP4Linear(32, 8, input_grad=True))
    assert "precision=fp8" in repr(fq().MXFP4Linear(32, 8, precision="fp8"))


def test_from_mxfp4_round_trip():
    from fused_int4_amd.quantize import quantize_mxfp4
    w, g = _weights(40, 96)
    blocks, scales = quantize_mxfp4(w)
    b = torch.randn(40, generator=g)
    m = fq().MXFP4Linear.from_mxfp4(blocks, scales, bias=b)
    assert torch.equal(m.blocks, blocks) and torch.equal(m.scales, scales) and torch.equal(m.bias, b)
    assert m.blocks.data_ptr() != blocks.data_ptr()                       # its own copy
    assert (m.in_features, m.out_features) == (96, 40)
    m4 = fq().MXFP4Linear.from_mxfp4(blocks.reshape(40, 3, 16), scales)   # the checkpoint's block dimension
    assert torch.equal(m4.blocks, blocks) and m4.bias is None
    again = fq().MXFP4Linear.from_mxfp4(m.state_dict()["blocks"], m.state_dict()["scales"], bias=m.state_dict()["bias"])
    assert all(torch.equal(again.state_dict()[k], v) for k, v in m.state_dict().items())
    for bad in (dict(blocks=blocks.int()), dict(scales=scales[:, :2]), dict(blocks=blocks[:, :40]), dict(bias=b[:3])):
        a = dict(blocks=blocks, scales=scales, bias=None)
        a.update(bad)
        with pytest.raises(ValueError):
            fq().MXFP4Linear.from_mxfp4(a["blocks"], a["scales"], bias=a["bias"])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("bias", [False, True])
def test_cpu_forward_is_the_definition(bias, dt):
    from fused_int4_amd.quantize import dequantize_mxfp4, quantize_mxfp4
    w, g = _weights(40, 96, seed=1)
    blocks, scales = quantize_mxfp4(w)
    b = torch.randn(40, generator=g) if bias else None
    m = fq().MXFP4Linear.from_mxfp4(blocks, scales, bias=b)
    W = dequantize_mxfp4(blocks, scales)
    for shape in ((96,), (5, 96), (2, 3, 96), (0, 96)):
        x = torch.randn(*shape, generator=g).to(dt)
        ref = x.bfloat16().float() @ W.T
        if bias:
            ref = ref + b
        got = m(x)
        assert got.dtype == dt and tuple(got.shape) == shape[:-1] + (40,)
        assert torch.equal(got, ref.to(dt)), shape


def test_refusals_without_a_gpu():
    from fused_int4_amd.quantize import quantize_mxfp4
    ops = fq().ops
    w, g = _weights(40, 96, seed=2)
    blocks, scales = quantize_mxfp4(w)
    x = torch.randn(3, 96, generator=g)
    m = fq().MXFP4Linear.from_mxfp4(blocks, scales)
    with pytest.raises(RuntimeError, match="float16 is refused"):
        m(x.half())
    with pytest.raises(RuntimeError, match="in_features"):
        m(x[:, :64])
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x.clone().requires_grad_(True))
    with torch.no_grad():
        assert m(x.clone().requires_grad_(True)).shape == (3, 40)
    for precision in ("fp8", "fp6", "fp4"):
        with pytest.raises(ValueError, match="has no backward"):
            fq().MXFP4Linear(96, 40, precision=precision, input_grad=True)
        with pytest.raises(RuntimeError, match="GPU only"):
            fq().MXFP4Linear.from_mxfp4(blocks, scales, precision=precision)(x)
    with pytest.raises(ValueError, match="precision"):
        fq().MXFP4Linear(96, 40, precision="int8")
    for K, N in ((48, 8), (0, 8), (32, 0)):
        with pytest.raises(ValueError, match="multiple of 32"):
            fq().MXFP4Linear(K, N)
    # the two ops: types and shapes in front of the devices, so the messages read the same here
    gu = torch.randn(3, 192, generator=g)
    for op, rows in ((ops.linear_forward_mxfp4, x), (ops.linear_gated_forward_mxfp4, gu)):
        with pytest.raises(RuntimeError, match="float16 is refused"):
            op(blocks, scales, rows.half())
        with pytest.raises(RuntimeError, match="2-D"):
            op(blocks, scales, rows[0])
        with pytest.raises(RuntimeError, match=r"uint8 \[N, K/2\]"):
            op(blocks[None], scales[None], rows)
        with pytest.raises(RuntimeError, match=r"uint8 \[N, K/2\]"):
            op(blocks.int(), scales, rows)
        with pytest.raises(RuntimeError, match=r"K % 32 == 0"):
            op(blocks, scales[:, :2], rows)
        with pytest.raises(RuntimeError, match="columns"):
            op(blocks, scales, rows[:, :64])
        with pytest.raises(RuntimeError, match=r"bias must be a float32 \[N\]"):
            op(blocks, scales, rows, bias=torch.zeros(39))
        with pytest.raises(RuntimeError, match=r"bias must be a float32 \[N\]"):
            op(blocks, scales, rows, bias=torch.zeros(40, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="out_dtype"):
            op(blocks, scales, rows, out_dtype=torch.float64)
        with pytest.raises(ValueError, match="precision"):
            op(blocks, scales, rows, precision="int8")
        with pytest.raises(RuntimeError, match="forward-only"):
            op(blocks, scales, rows.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):      # everything else is fine: the device is last
            op(blocks, scales, rows)
    with pytest.raises(ValueError, match="activation"):
        ops.linear_gated_forward_mxfp4(blocks, scales, gu, activation="relu")
    with pytest.raises(RuntimeError, match=r"uint8 \[N, K/2\]"):
        ops.linear_backward_input_mxfp4(blocks[None], scales[None], torch.zeros(3, 40))
    with pytest.raises(RuntimeError, match="float16 is"):
        ops.linear_backward_input_mxfp4(blocks, scales, torch.zeros(3, 40).half())
