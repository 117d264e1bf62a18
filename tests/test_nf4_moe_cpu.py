"""Grouped NF4 (code-book) experts without a GPU (FQL_VERSION 500): the four entries are declared, exported and bound, and
validate in lut4_check's order with the expert-table tests where mx4_check has them, before any HIP call (every call below is
invalid or empty, with host pointers that are never dereferenced); the ops' operand errors come before their device check;
``NF4MoEFFN``'s constructors."""
import os
import re

import pytest
import torch

from conftest import ROOT
from test_nf4_cpu import ALIGN, BF16, DTYPE, F16, NULLP, ODD_K, OK, P, P2, P_WORD, SHAPE, fq, lib  # noqa: F401

WS = -4


def _fwd(lib, di=BF16, do=BF16, E=3, T=8, K=128, N=40, block=64, c=P, a=P, x=P, o=P2, tpe=P, offs=P, gated=None, ws=P,
         ws_bytes=1 << 30):
    if gated is None:
        return lib.fql_moe_lut4_fwd(c, a, None, block, x, di, None, tpe, offs, o, do, E, T, K, N, None)
    return lib.fql_moe_lut4_glu_fwd(c, a, None, block, x, di, None, tpe, offs, o, do, E, T, K, N, *gated, ws, ws_bytes, None)


def _bwd(lib, di=BF16, do=BF16, E=3, T=8, K=128, N=40, block=64, c=P, a=P, g=P, o=P2, tpe=P, offs=P):
    return lib.fql_moe_lut4_bwd_input(c, a, None, block, g, di, tpe, offs, o, do, E, T, K, N, None)


def test_entries_abi_and_check_order(lib):
    import test_c_abi
    from fused_int4_amd import _native
    for name, nargs in (("fql_moe_lut4_fwd", 16), ("fql_moe_lut4_glu_fwd", 21), ("fql_moe_lut4_bwd_input", 15),
                        ("fql_moe_lut4_workspace_bytes", 5)):
        assert name in test_c_abi.declared_symbols() and name in _native.exported_symbols()
        assert len(getattr(lib, name).argtypes) == nargs
    with open(os.path.join(ROOT, "include", "fql_int4.h")) as f:
        header = int(re.search(r"#define\s+FQL_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.fql_version() >= 500 and lib.fql_version() == header
    null = dict(c=None, a=None, o=None, tpe=None, offs=None)
    silu, bad_act = (0, 0.0, 0.0), (99, 0.0, 0.0)
    for call, rows in ((_fwd, "x"), (_bwd, "g")):
        nul = dict(null, **{rows: None})
        assert call(lib, E=0, K=65, block=48, di=F16, **nul) == SHAPE         # each step repairs the failure before it
        assert call(lib, K=65, block=48, di=F16, **nul) == ODD_K
        assert call(lib, K=96, block=48, di=F16, **nul) == SHAPE
        assert call(lib, block=32, di=F16, **nul) == SHAPE
        assert call(lib, di=F16, **nul) == DTYPE
        assert call(lib, T=0, **nul) == OK
        assert call(lib, **nul) == NULLP
        assert call(lib, offs=None) == NULLP                                   # one table pointer without the other
        assert call(lib, tpe=None, offs=None) == SHAPE                         # no table: one expert only
        assert call(lib, E=65535) == SHAPE
        assert call(lib, T=65535 * 128 + 1) == SHAPE                           # the grid's y, whichever tile
        assert call(lib, c=P_WORD) == ALIGN
    assert _fwd(lib, N=0, **dict(null, x=None)) == OK                          # forward: N == 0 is empty
    assert _bwd(lib, N=0, o=None) == NULLP                                     # input gradient: N == 0 writes zeros
    assert _fwd(lib, gated=bad_act, E=0) == SHAPE and _fwd(lib, gated=bad_act) == SHAPE
    assert _fwd(lib, gated=silu, c=P_WORD, ws=None) == ALIGN                   # the alignment before the workspace
    need = lib.fql_moe_lut4_workspace_bytes(3, 8, 128, 40, 1)
    assert need == 8 * 128 * 2 and lib.fql_moe_lut4_workspace_bytes(3, 8, 128, 40, 0) == 0
    for kw in (dict(ws=None), dict(ws=P_WORD), dict(ws_bytes=need - 1)):
        assert _fwd(lib, gated=silu, **kw) == WS, kw


def test_ops_check_operands_before_devices():
    ops = fq().ops
    c, a = torch.zeros(3, 40, 64, dtype=torch.uint8), torch.ones(3, 40, 2)
    x, gu, gy, tab = torch.zeros(6, 128), torch.zeros(6, 256), torch.zeros(6, 40), torch.zeros(3, dtype=torch.int32)
    for op, rows in ((ops.moe_forward_lut4, x), (ops.moe_gated_forward_lut4, gu), (ops.moe_backward_input_lut4, gy)):
        with pytest.raises(RuntimeError, match="float16 is refused"):
            op(c, a, rows.half(), tab, tab)
        with pytest.raises(RuntimeError, match=r"\[num_experts, N, K/2\]"):
            op(c[0], a[0], rows, tab, tab)
        with pytest.raises(RuntimeError, match="block"):
            op(c, a, rows, tab, tab, block=96)
        with pytest.raises(RuntimeError, match="absmax must be"):
            op(c, a[:, :, :1], rows, tab, tab)
        with pytest.raises(RuntimeError, match="columns"):
            op(c, a, rows[:, :-1], tab, tab)
        with pytest.raises(RuntimeError, match="code_book"):
            op(c, a, rows, tab, tab, code_book=torch.zeros(8))
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            op(c, a, rows, tab, tab)
    with pytest.raises(RuntimeError, match=r"bias must be a float32 \[num_experts, N\]"):
        ops.moe_forward_lut4(c, a, x, tab, tab, bias=torch.zeros(40))
    with pytest.raises(ValueError, match="activation"):
        ops.moe_gated_forward_lut4(c, a, gu, tab, tab, activation="relu")


def test_layer_constructors_state_dict_and_bnb_experts():
    F4 = fq().NF4MoEFFN
    for kw in (dict(hidden_dim=96), dict(ffn_dim=32), dict(block=48), dict(block=128), dict(num_experts=0),
               dict(activation_dtype=torch.float16)):
        with pytest.raises(ValueError):
            F4(**dict(dict(num_experts=2, hidden_dim=64, ffn_dim=64), **kw))
    m = F4(2, 128, 64, expert_bias=True)
    assert list(m.state_dict()) == ["gate_up_bias", "down_bias", "gate_up_codes", "gate_up_absmax", "down_codes", "down_absmax",
                                    "code_book"]
    assert [tuple(t.shape) for t in (m.gate_up_codes, m.gate_up_absmax, m.down_codes, m.down_absmax, m.code_book)] == \
        [(2, 128, 64), (2, 128, 2), (2, 128, 32), (2, 128, 1), (16,)]
    assert (m.group_size, m.precision, m.activation_args[0]) == (None, "bf16", "silu") and m.biases[0] is m.gate_up_bias
    assert m.total_memory_bytes == sum(t.numel() * t.element_size() for t in m.state_dict().values())
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        m(torch.zeros(4, 128), None, None)

    E, H, F = 2, 128, 64
    g = torch.Generator().manual_seed(0)
    gate, up, down = ([torch.randn(*s, generator=g) for _ in range(E)] for s in ((F, H), (F, H), (H, F)))
    q = fq().quantize_nf4
    flat = lambda w: tuple(t.reshape(-1, 1) if t.dtype == torch.uint8 else t.reshape(-1) for t in q(w))   # as bitsandbytes stores it
    a = F4.from_bnb_experts([flat(w) for w in gate], [flat(w) for w in up], [flat(w) for w in down], hidden_dim=H, ffn_dim=F)
    b = F4.from_weights(gate, up, down)
    c = F4.from_bnb(b.gate_up_codes, b.gate_up_absmax, b.down_codes, b.down_absmax)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, c.state_dict()[k]), k
    W = fq().dequantize_lut4(a.gate_up_codes, a.gate_up_absmax)
    for e in range(E):
        assert torch.equal(W[e], torch.cat([fq().dequantize_lut4(*q(gate[e])), fq().dequantize_lut4(*q(up[e]))]))
    with pytest.raises(ValueError, match="same E, H and F"):
        F4.from_bnb(b.gate_up_codes, b.gate_up_absmax, b.down_codes[:, :64], b.down_absmax[:, :64])
