"""NVFP4 weights (FQL_VERSION 430), the part that needs no GPU: the host quantiser (``quantize_nvfp4`` /
``dequantize_nvfp4`` / ``nvfp4_scale_values``), the C ABI of fql_moe_nvfp4_fwd / fql_moe_nvfp4_glu_fwd /
fql_linear_nvfp4_fwd / fql_linear_nvfp4_glu_fwd with their workspace queries and tuning hooks (declared, exported,
validated in mx4_check's order before any HIP call -- every call below is invalid, empty or stops at the workspace check,
with host pointers that are never dereferenced), ``NVFP4Linear`` on the CPU, the refusals, the state-dict keys, and the
block's acceptance of an ``NVFP4MoEFFN``."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT

NEW = ("fql_moe_nvfp4_workspace_bytes", "fql_moe_nvfp4_fwd", "fql_moe_nvfp4_glu_fwd", "fql_linear_nvfp4_workspace_bytes",
       "fql_linear_nvfp4_fwd", "fql_linear_nvfp4_glu_fwd")
HOOKS = ("fql_tune_set_nvfp4_decode_max_rows", "fql_tune_nvfp4_kernel")
INT_MAX = 2 ** 31 - 1
T_MAX = 4194240                # the largest T mx4_check admits
OK, NULLP, SHAPE, ODD_K, WS, ALIGN, DTYPE = 0, -1, -2, -3, -4, -7, -8
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(16)        # never dereferenced
P2 = ctypes.c_void_p(32)
P_HALF = ctypes.c_void_p(18)
P_WORD = ctypes.c_void_p(20)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def fq():
    import fused_int4_amd
    return fused_int4_amd


def Q():
    from fused_int4_amd import quantize
    return quantize


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


# ---- the quantiser

def e4m3_value(b):
    """The definition, in Python floats: sign, exponent field of bias 7, three mantissa bits, subnormals, 0x7F / 0xFF NaN."""
    if b & 0x7F == 0x7F:
        return float("nan")
    ex, m = (b >> 3) & 15, b & 7
    mag = m * 2.0 ** -9 if ex == 0 else (1 + m / 8) * 2.0 ** (ex - 7)
    return -mag if b & 0x80 else mag


def test_all_256_scale_bytes_decode_as_the_definition():
    b = torch.arange(256, dtype=torch.uint8)
    got = Q().nvfp4_scale_values(b)
    assert got.dtype == torch.float32
    for i in range(256):
        want = e4m3_value(i)
        assert (got[i] != got[i]) if want != want else float(got[i]) == want, i
    assert float(got[0x7E]) == 448.0 and float(got[0x38]) == 1.0 and float(got[0x01]) == 2.0 ** -9 and float(got[0xB8]) == -1.0
    assert bool(torch.signbit(got[0x80])) and float(got[0x80]) == 0.0
    torch_view = b.view(torch.float8_e4m3fn).float()                     # torch's own decoding agrees
    assert torch.equal(torch.nan_to_num(got, nan=-1e9), torch.nan_to_num(torch_view, nan=-1e9))


def test_every_product_is_exact_in_bfloat16():
    s = Q().nvfp4_scale_values(torch.arange(256, dtype=torch.uint8))
    s = s[torch.isfinite(s)]
    assert s.numel() == 254
    prod = s[:, None].double() * torch.tensor(E2M1, dtype=torch.float64)[None, 1:]
    assert torch.equal(prod.float().bfloat16().double(), prod)
    mags = prod.abs()[prod != 0]
    assert float(mags.min()) == 2.0 ** -10 and float(mags.max()) == 2688.0


@pytest.mark.parametrize("lead", [(), (3,)], ids=["N,K", "E,N,K"])
def test_round_trip_on_grid_values_is_exact(lead):
    """Weights that lie on the format's grid already: codes, finite positive scale bytes with the block's largest code 6
    (so that block_amax / 6 is the scale itself) and a power-of-two global scale come back bit for bit."""
    g = torch.Generator().manual_seed(1)
    N, K = 5, 64
    codes = torch.randint(0, 16, (*lead, N, K), generator=g, dtype=torch.uint8)
    codes[..., ::16] = 7                                                  # every block holds a 6
    scales = torch.randint(0x08, 0x7F, (*lead, N, K // 16), generator=g, dtype=torch.uint8)
    scales[..., 0, 0] = 0x7E                                              # amax = 6 * 448 * gs: the rule's own global scale
    blocks = Q().pack_nibbles(codes)
    gs = torch.full(lead or (1,), 2.0 ** -4)
    w = Q().dequantize_nvfp4(blocks, scales, gs)
    assert w.shape == (*lead, N, K) and w.dtype == torch.float32
    for given in (gs, None):
        b2, s2, g2 = Q().quantize_nvfp4(w, given)
        assert b2.shape == blocks.shape and s2.shape == scales.shape and g2.shape == (lead or (1,)) and g2.dtype == torch.float32
        assert torch.equal(g2, gs) and torch.equal(s2, scales)
        assert torch.equal(b2 & 0x77, blocks & 0x77)                      # the magnitudes
        assert torch.equal(Q().dequantize_nvfp4(b2, s2, g2), w)          # (a -0 and a +0 are the same weight)
    table = torch.tensor(E2M1 + tuple(-v for v in E2M1))
    manual = table[codes.long()] * Q().nvfp4_scale_values(scales).repeat_interleave(16, dim=-1) * 2.0 ** -4
    assert torch.equal(w, manual)


def test_the_clamp_at_448_comes_before_the_cast():
    """A caller's global scale that is too small asks for a block scale above 448: it is clamped (a cast of a value above
    464 would be NaN), and the codes saturate at 6."""
    w = torch.zeros(2, 32)
    w[0, 0], w[1, 5] = 6.0 * 448.0 * 4.0, -6.0
    blocks, scales, gs = Q().quantize_nvfp4(w, torch.tensor([1.0]))
    assert int(scales[0, 0]) == 0x7E and bool(torch.isfinite(Q().nvfp4_scale_values(scales)).all())
    assert int(blocks[0, 0]) & 0xF == 7
    assert float(Q().dequantize_nvfp4(blocks, scales, gs)[0, 0]) == 2688.0
    assert float(Q().dequantize_nvfp4(blocks, scales, gs)[1, 5]) == -6.0 and int(scales[1, 0]) == 0x38
    auto = Q().quantize_nvfp4(w)[2]
    assert float(auto[0]) == pytest.approx(4.0) and auto.shape == (1,)


def test_zero_block_and_zero_matrix():
    w = torch.randn(3, 4, 32, generator=torch.Generator().manual_seed(2))
    w[0, 1, 16:] = 0                                                      # an all-zero block
    w[1] = 0                                                              # an all-zero matrix
    blocks, scales, gs = Q().quantize_nvfp4(w)
    assert int(scales[0, 1, 1]) == 0 and int(blocks[0, 1, 8:].sum()) == 0
    assert float(gs[1]) == 1.0 and int(scales[1].sum()) == 0 and int(blocks[1].sum()) == 0
    assert float(gs[0]) == float(w[0].abs().max() / (6 * 448))
    d = Q().dequantize_nvfp4(blocks, scales, gs)
    assert torch.count_nonzero(d[1]) == 0 and torch.count_nonzero(d[0, 1, 16:]) == 0
    err = float((d - w).norm() / w.norm())
    assert err < 0.15, err                                                # e2m1's own error on Gaussian weights, about 0.1
    tiny = torch.full((1, 16), 1e-30)                                     # a block scale that rounds to zero: zero codes
    b, s, _ = Q().quantize_nvfp4(tiny, torch.tensor([1.0]))
    assert int(s.sum()) == 0 and int(b.sum()) == 0


def test_quantiser_refusals():
    with pytest.raises(ValueError, match="K % 16"):
        Q().quantize_nvfp4(torch.zeros(4, 24))
    with pytest.raises(ValueError, match="finite"):
        Q().quantize_nvfp4(torch.full((4, 32), float("inf")))
    with pytest.raises(ValueError, match="positive"):
        Q().quantize_nvfp4(torch.ones(4, 32), torch.tensor([0.0]))
    with pytest.raises(ValueError, match="uint8"):
        Q().dequantize_nvfp4(torch.zeros(4, 16), torch.zeros(4, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="K/16"):
        Q().dequantize_nvfp4(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(4, 1, dtype=torch.uint8))


# ---- the C boundary

def _moe(lib, di=BF16, do=BF16, E=1, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, tpe=None, offs=None, out=P2, ws=None, nbytes=0):
    return lib.fql_moe_nvfp4_fwd(bl, sc, gs, x, di, bias, tpe, offs, out, do, E, T, K, N, ws, nbytes, None)


def _moe_glu(lib, di=F32, do=F32, E=1, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, tpe=None, offs=None, out=P2, ws=None,
             nbytes=0, act=2, alpha=1.702, limit=7.0):
    return lib.fql_moe_nvfp4_glu_fwd(bl, sc, gs, x, di, bias, tpe, offs, out, do, E, T, K, N, act, alpha, limit, ws, nbytes, None)


def _lin(lib, di=BF16, do=BF16, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, out=P2, ws=None, nbytes=0, **grouped):
    assert not grouped or set(grouped) <= {"E", "tpe", "offs"}
    return lib.fql_linear_nvfp4_fwd(bl, sc, gs, x, di, bias, out, do, T, K, N, ws, nbytes, None)


def _lin_glu(lib, di=F32, do=F32, T=8, K=64, N=96, bl=P, sc=P, gs=P, x=P, bias=P, out=P2, ws=None, nbytes=0, act=2, alpha=1.702,
             limit=7.0):
    return lib.fql_linear_nvfp4_glu_fwd(bl, sc, gs, x, di, bias, out, do, T, K, N, act, alpha, limit, ws, nbytes, None)


ENTRIES = (_moe, _moe_glu, _lin, _lin_glu)
GATED = (_moe_glu, _lin_glu)
NONE = dict(bl=None, sc=None, gs=None, x=None, bias=None, out=None)


def test_declared_exported_and_versioned(lib):
    import test_c_abi
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NEW:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 430
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        boundary = f.read()
    m = re.search(r"#define\s+FQL_VERSION\s+(\d+)", boundary)
    assert m and int(m.group(1)) >= 430 and int(m.group(1)) == lib.fql_version()
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
                    "size_t (*w0)(int, int, int, int, int) = fql_moe_nvfp4_workspace_bytes;\n"
                    "size_t (*w1)(int, int, int, int) = fql_linear_nvfp4_workspace_bytes;\n"
                    "int (*a)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, void *, size_t, void *) = fql_moe_nvfp4_fwd;\n"
                    "int (*b)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, const int32_t *,\n"
                    "         const int32_t *, void *, int, int, int, int, int, int, float, float, void *, size_t, void *)\n"
                    "    = fql_moe_nvfp4_glu_fwd;\n"
                    "int (*c)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, void *, int, int,\n"
                    "         int, int, void *, size_t, void *) = fql_linear_nvfp4_fwd;\n"
                    "int (*d)(const uint8_t *, const uint8_t *, const float *, const void *, int, const float *, void *, int, int,\n"
                    "         int, int, int, float, float, void *, size_t, void *) = fql_linear_nvfp4_glu_fwd;\n"
                    "int (*h0)(int) = fql_tune_set_nvfp4_decode_max_rows;\n"
                    "int (*h1)(int, int, int, int) = fql_tune_nvfp4_kernel;\n"
                    "int version_is_430[FQL_VERSION >= 430 ? 1 : -1];\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", src, "-o",
                               os.path.join(tmp, "use.o")])


@pytest.mark.parametrize("entry", ENTRIES, ids=["moe", "moe_glu", "linear", "linear_glu"])
def test_return_codes_in_mx4_checks_order(lib, entry):
    """fql_moe_mx4_fwd's order, every check in front of any HIP call, the workspace last."""
    call = lambda **kw: entry(lib, **kw)
    for kw in (dict(T=-1), dict(K=0), dict(K=-32), dict(N=-1)):
        assert call(**NONE, **kw) == SHAPE, kw
    assert call(**NONE, K=65) == ODD_K
    assert call(**NONE, K=65, T=-1) == SHAPE
    for K in (16, 48, 80, 2):
        assert call(**NONE, K=K) == SHAPE, K                                # K % 32 == 0, although a scale block is 16
    assert call(**NONE, K=33, di=F16) == ODD_K
    assert call(**NONE, di=F16) == DTYPE and call(**NONE, di=3) == DTYPE and call(**NONE, do=3) == DTYPE
    assert call(**NONE, T=0) == OK and call(**NONE, N=0) == OK          # empty: nothing launched, nothing else looked at
    assert call(**NONE, T=0, di=F16) == DTYPE
    assert call(**NONE) == NULLP
    for name in ("bl", "sc", "x", "out"):
        assert call(**{name: None}) == NULLP, name
    assert call(T=T_MAX + 1) == SHAPE and call(T=T_MAX + 1, bl=None) == NULLP   # the pointers before the grid's limits
    assert call(bl=P_WORD) == ALIGN and call(bias=P_HALF) == ALIGN and call(gs=P_HALF) == ALIGN
    assert call(x=ctypes.c_void_p(17)) == ALIGN and call(out=ctypes.c_void_p(33)) == ALIGN
    if entry in (_moe, _moe_glu):
        assert call(E=0) == SHAPE and call(E=2) == SHAPE                    # no table: one expert
        assert call(E=2, tpe=P) == NULLP and call(E=2, offs=P) == NULLP     # the table's pointers come together
        assert call(E=65535, tpe=P, offs=P) == SHAPE
    if entry in GATED:
        assert call(act=3) == SHAPE and call(limit=0.0) == SHAPE and call(alpha=float("nan")) == SHAPE
        assert call(act=3, K=65) == SHAPE                                 # the activation with the first shape check
        need = lib.fql_moe_nvfp4_workspace_bytes(1, 8, 64, 96, 1)
        assert need == lib.fql_linear_nvfp4_workspace_bytes(8, 64, 96, 1) > 0
        assert call() == WS and call(bias=None, gs=None) == WS              # everything else is fine: the workspace is last
        assert call(ws=P, nbytes=need - 1) == WS                          # short
        assert call(ws=P_WORD, nbytes=need) == WS                         # misaligned
        assert call(ws=None, nbytes=need) == WS
        assert call(ws=P, nbytes=need, bl=P_WORD) == ALIGN                # ... and behind every other check


def test_workspace_bytes(lib):
    r16 = lambda v: (v + 15) // 16 * 16
    for T in (1, 2, 33, 64):
        for K in (32, 96, 1024):
            for N in (8, 40, 136):
                for E in (1, 4):
                    assert lib.fql_moe_nvfp4_workspace_bytes(E, T, K, N, 0) == 0
                    assert lib.fql_moe_nvfp4_workspace_bytes(E, T, K, N, 1) == r16(2 * T * K) == lib.fql_moe_mx4_workspace_bytes(E, T, K, N, 1)
                assert lib.fql_linear_nvfp4_workspace_bytes(T, K, N, 0) == 0
                assert lib.fql_linear_nvfp4_workspace_bytes(T, K, N, 1) == r16(2 * T * K)
    assert lib.fql_moe_nvfp4_workspace_bytes(1, 0, 64, 8, 1) == 0 and lib.fql_linear_nvfp4_workspace_bytes(-1, 64, 8, 1) == 0
    assert lib.fql_linear_nvfp4_workspace_bytes(T_MAX, INT_MAX - 31, 8, 1) == r16(2 * T_MAX * (INT_MAX - 31))


def test_hooks(lib):
    rows, k = lib.fql_tune_set_nvfp4_decode_max_rows, lib.fql_tune_nvfp4_kernel
    default = rows(17)
    try:
        with open(os.path.join(ROOT, "fused-4-bit-dequantize-linear-cuda-kernel_amd", "csrc", "fql_mx4.hip")) as f:
            built = re.search(r"#define\s+FQL_NVFP4_DECODE_MAX_ROWS\s+(\d+)", f.read())
        assert built and default == int(built.group(1)) >= 0               # the library's own value, set from the sweep
        mx = lib.fql_tune_set_mx4_decode_max_rows(-1)
        assert k(4, 17, 64, 8) == 1 and k(4, 18, 64, 8) == 0 and k(4, 0, 64, 8) == 0
        assert rows(64) == 17 and rows(0) == 64 and k(1, 1, 64, 8) == 0
        assert rows(INT_MAX) == 0 and k(1, 1, 64, 8) == 1 and k(1, 65535 * 32, 64, 8) == 1
        assert k(1, 65535 * 32 + 1, 64, 8) == 0 and k(1, INT_MAX, 64, 8) == 0   # the decode grid's y is bounded
        assert rows(-5) == INT_MAX and rows(-1) == INT_MAX                   # refused, nothing changed
        assert lib.fql_tune_set_mx4_decode_max_rows(-1) == mx               # a threshold of its own
    finally:
        rows(default)
    assert rows(-1) == default


# ---- the layers on the CPU

def test_linear_on_the_cpu_is_the_definition():
    g = torch.Generator().manual_seed(3)
    lin = torch.nn.Linear(64, 24)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(24, 64, generator=g))
        lin.bias.copy_(torch.randn(24, generator=g))
    m = fq().NVFP4Linear.from_linear(lin)
    assert list(m.state_dict()) == ["blocks", "scales", "global_scale", "bias"]
    assert m.blocks.shape == (24, 32) and m.scales.shape == (24, 4) and m.global_scale.shape == (1,)
    x = torch.randn(2, 3, 64, generator=g)
    W = Q().dequantize_nvfp4(m.blocks, m.scales)
    want = (x.bfloat16().float() @ W.T) * m.global_scale + lin.bias.detach()
    got = m(x)
    assert got.shape == (2, 3, 24) and got.dtype == torch.float32 and torch.equal(got, want)
    assert m(x.bfloat16()).dtype == torch.bfloat16 and torch.equal(m(x.bfloat16()), want.bfloat16())
    ref = lin(x).detach()
    assert float((got - ref).norm() / ref.norm()) < 0.15           # the format's own error
    again = fq().NVFP4Linear.from_nvfp4(m.blocks, m.scales.view(torch.float8_e4m3fn), m.global_scale, bias=m.bias)
    assert torch.equal(again(x), got)                                     # a float8 scale tensor is taken as its bytes
    no_gs = fq().NVFP4Linear.from_nvfp4(m.blocks, m.scales)
    assert list(no_gs.state_dict()) == ["blocks", "scales", "global_scale"] and float(no_gs.global_scale) == 1.0
    assert torch.equal(no_gs(x), x.bfloat16().float() @ W.T)
    m2 = fq().NVFP4Linear(64, 24, bias=True)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(x), got)
    assert "format=nvfp4" in repr(m)


def test_linear_refusals():
    L = fq().NVFP4Linear
    with pytest.raises(ValueError, match="multiple of 32"):
        L(48, 8)
    b, s = torch.zeros(8, 32, dtype=torch.uint8), torch.full((8, 4), 0x38, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        L.from_nvfp4(b.float(), s)
    with pytest.raises(ValueError, match="K/16"):
        L.from_nvfp4(b, s[:, :2])
    with pytest.raises(ValueError, match="bias"):
        L.from_nvfp4(b, s, bias=torch.zeros(7))
    with pytest.raises(ValueError, match="one value"):
        L.from_nvfp4(b, s, torch.ones(2))
    m = L.from_nvfp4(b, s)
    with pytest.raises(RuntimeError, match="float16"):
        m(torch.zeros(2, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="in_features"):
        m(torch.zeros(2, 32))
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(2, 64, requires_grad=True))
    with torch.no_grad():
        assert m(torch.zeros(2, 64, requires_grad=True)).shape == (2, 8)


def test_ops_check_types_and_shapes_before_devices():
    from fused_int4_amd import ops
    b, s, gs = torch.zeros(2, 8, 32, dtype=torch.uint8), torch.zeros(2, 8, 4, dtype=torch.uint8), torch.ones(2)
    x = torch.zeros(3, 64)
    t = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="float16"):
        ops.moe_forward_nvfp4(b, s, gs, x.half(), t, t)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.moe_forward_nvfp4(b.float(), s, gs, x, t, t)
    with pytest.raises(RuntimeError, match="K/16"):
        ops.moe_forward_nvfp4(b, s[:, :, :2], gs, x, t, t)
    with pytest.raises(RuntimeError, match="64 columns"):
        ops.moe_forward_nvfp4(b, s, gs, x[:, :32], t, t)
    with pytest.raises(RuntimeError, match="128 columns"):
        ops.moe_gated_forward_nvfp4(b, s, gs, x, t, t)
    with pytest.raises(RuntimeError, match="global_scale"):
        ops.moe_forward_nvfp4(b, s, gs[:1], x, t, t)
    with pytest.raises(RuntimeError, match="global_scale"):
        ops.linear_forward_nvfp4(b[0], s[0], gs, x)
    with pytest.raises(RuntimeError, match="bias"):
        ops.moe_forward_nvfp4(b, s, gs, x, t, t, bias=torch.zeros(8))
    with pytest.raises(RuntimeError, match=r"\[N, K/2\]"):
        ops.linear_forward_nvfp4(b, s, None, x)
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.moe_forward_nvfp4(b, s, gs, x, t, t, out_dtype=torch.float64)
    for call in (lambda: ops.moe_forward_nvfp4(b, s, gs, x, t, t), lambda: ops.linear_forward_nvfp4(b[0], s[0], gs[:1], x),
                 lambda: ops.moe_gated_forward_nvfp4(b, s, None, torch.zeros(3, 128), t, t),
                 lambda: ops.linear_gated_forward_nvfp4(b[0], s[0], None, torch.zeros(3, 128))):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):      # everything else is fine: the device is last
            call()
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.moe_forward_nvfp4(b, s, gs, x.clone().requires_grad_(True), t, t)


def ffn(E=4, H=64, F=32, **kw):
    g = torch.Generator().manual_seed(4)
    mk = lambda *s: [torch.randn(*s, generator=g) for _ in range(E)]
    return fq().NVFP4MoEFFN.from_weights(mk(F, H), mk(F, H), mk(H, F), **kw)


def test_ffn_layer_buffers_and_refusals():
    m = ffn()
    assert list(m.state_dict()) == ["gate_up_blocks", "gate_up_scales", "gate_up_global", "down_blocks", "down_scales", "down_global"]
    assert m.gate_up_blocks.shape == (4, 64, 32) and m.gate_up_scales.shape == (4, 64, 4) and m.gate_up_global.shape == (4,)
    assert m.down_blocks.shape == (4, 64, 16) and m.down_scales.shape == (4, 64, 2) and m.down_global.shape == (4,)
    assert (m.num_experts, m.hidden_dim, m.ffn_dim, m.expert_bias) == (4, 64, 32, False)
    assert m.activation_args == ("silu", 1.702, 7.0) and "format=nvfp4" in repr(m)
    g = torch.Generator().manual_seed(5)
    biased = ffn(gate_bias=[torch.randn(32, generator=g)] * 4, up_bias=[torch.randn(32, generator=g)] * 4,
                 down_bias=[torch.randn(64, generator=g)] * 4, activation="swiglu_clamp")
    assert biased.expert_bias and list(biased.state_dict())[:2] == ["gate_up_bias", "down_bias"]      # (parameters, as MXFP4MoEFFN's)
    assert biased.activation_args[0] == "swiglu_clamp"
    # the interleaved order is undone once: rows 0, 2, 4, ... are the gate
    inter = torch.stack([m.gate_up_blocks[:, :32], m.gate_up_blocks[:, 32:]], dim=2).reshape(4, 64, 32)
    inter_s = torch.stack([m.gate_up_scales[:, :32], m.gate_up_scales[:, 32:]], dim=2).reshape(4, 64, 4)
    again = fq().NVFP4MoEFFN.from_nvfp4(inter, inter_s, m.gate_up_global, m.down_blocks, m.down_scales, None, interleaved=True)
    assert torch.equal(again.gate_up_blocks, m.gate_up_blocks) and torch.equal(again.gate_up_scales, m.gate_up_scales)
    assert torch.equal(again.down_global, torch.ones(4))
    fresh = fq().NVFP4MoEFFN(4, 64, 32)
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(fresh.down_scales, m.down_scales)
    with pytest.raises(ValueError, match="multiples of 32"):
        fq().NVFP4MoEFFN(4, 48, 32)
    with pytest.raises(ValueError, match="K/16"):
        fq().NVFP4MoEFFN.from_nvfp4(m.gate_up_blocks, m.gate_up_scales[:, :, :2], None, m.down_blocks, m.down_scales, None)
    with pytest.raises(ValueError, match="one float32 value per expert"):
        fq().NVFP4MoEFFN.from_nvfp4(m.gate_up_blocks, m.gate_up_scales, torch.ones(3), m.down_blocks, m.down_scales, None)
    with pytest.raises(ValueError, match="same E, H and F"):
        fq().NVFP4MoEFFN.from_nvfp4(m.gate_up_blocks, m.gate_up_scales, None, m.down_blocks[:, :32], m.down_scales[:, :32], None)
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        m(torch.zeros(3, 64), t, t)


def test_block_accepts_nvfp4_experts_and_rejects_mismatched_ones():
    B = fq().QuantizedSparseMoEBlock
    experts, shared = ffn(), ffn(E=1, F=96)
    blk = B(4, 64, 32, top_k=2, experts=experts, shared_experts=shared)
    assert blk.experts is experts and blk.shared_experts is shared
    keys = list(blk.state_dict())
    assert "experts.gate_up_global" in keys and "shared_experts.down_scales" in keys and "gate.weight" in keys
    with pytest.raises(ValueError, match="num_experts, hidden_dim and ffn_dim"):
        B(4, 64, 64, experts=experts)
    with pytest.raises(ValueError, match="num_experts, hidden_dim and ffn_dim"):
        B(8, 64, 32, experts=experts)
    with pytest.raises(ValueError, match="one expert"):
        B(4, 64, 32, experts=experts, shared_experts=ffn(E=2))
    with pytest.raises(ValueError, match="activation"):
        B(4, 64, 32, experts=experts, activation="gelu_tanh")
    with pytest.raises(ValueError, match="expert_bias"):
        B(4, 64, 32, experts=experts, expert_bias=True)
    with pytest.raises(ValueError, match="group_size"):
        B(4, 64, 32, experts=experts, group_size=32)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        blk(torch.zeros(3, 64))
