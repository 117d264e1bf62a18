"""Where the per-group grouped entry points write, and what else they read: the method of tests/test_gpu_footprint_bwd.py
on fql_moe_group_fwd, fql_moe_group_glu_fwd and fql_moe_group_bwd_input, through the C ABI.

Every pointer of a call is the interior of a helpers.Guarded buffer: the output between SENT (and SENT inside before the
call), rows / gradient, scales, zps and bias between NaN, the expert table between BIG (a slot past the table that is used
sends a kernel far away), the packed weights between 0xFF, the workspace at exactly fql_moe_group_typed_workspace_bytes(),
16 bytes past a 256-byte boundary, between 0x5A (the backward's query is 0: it gets NULL).  The forward entries run once per
stale workspace content (PREFILLS: 0x00, 0xFF -- a NaN in every format the workspace holds -- and 0x7F) and must return the
same bits each time: a replayed graph finds there what the previous launch left.  Every case asserts that all
guards are intact, that the rows no expert covers are zero (they held SENT), and that the result is bit for bit what the
public op returns on plain tensors.  The problems are those of tests/test_gpu_group_moe_ops.py and test_gpu_group_bwd.py:
the integer path (rows [40, 0, 9] + 2, K = 512, N = 136 and 70), the float32 kernels with both staging kernels (rows
[3, 0, 5] + 2, K = 192), the tiled backward with 16-byte and element loads and the one-wave-per-row fallback."""
import pytest
import torch

from helpers import BIG, NAN, SENT, Guarded, assert_guards_intact, guarded_like, ops, same_bits
from test_gpu_group_bwd import problem as bwd_problem
from test_gpu_group_moe_ops import FL, I8, problem as fwd_problem

pytestmark = pytest.mark.gpu
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"silu": 0, "gelu_tanh": 1, "swiglu_clamp": 2}
ALPHA, LIMIT = 1.702, 7.0
PREFILLS = (0x00, 0xFF, 0x7F)                            # (tests/test_gpu_footprint.py; 0xFF: NaN in every format)
TYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32)]
TYPE_IDS = ["f32-f32", "bf16-bf16", "f16-f32"]


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guarded_inputs(p, rows, bias=None):
    """(packed, scales, zps, rows, tokens_per_expert, input_offsets[, bias]) inside guards."""
    bufs = [guarded_like("packed", p["P"], 0xFF, offset=16), guarded_like("scales", p["S"], NAN),
            guarded_like("zps", p["Z"], NAN), guarded_like("rows", rows, NAN, offset=16),
            guarded_like("tokens_per_expert", p["tpe"], BIG), guarded_like("input_offsets", p["offs"], BIG)]
    if bias is not None:
        bufs.append(guarded_like("bias", bias, NAN))
    return bufs


def guarded_out(T, C, dtype):
    out = Guarded("out", T * C * esize(dtype), dtype, SENT, offset=16)
    out.view(dtype, T, C).fill_(SENT)
    return out


def uncovered_rows_are_zero(p, got):
    return torch.count_nonzero(got[p["T"] - 2:]) == 0


@pytest.mark.parametrize("din,dout", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", [None, "swiglu_clamp"], ids=["plain", "glu"])
@pytest.mark.parametrize("path,N,group", [(I8, 136, 64), (I8, 70, 256), (FL, 136, 32), (FL, 70, 32)],
                         ids=["i8-N136", "i8-N70", "float-N136", "float-N70"])
def test_forward_entries_stay_inside_their_buffers(lib, path, N, group, kind, din, dout):
    K = path["K"]
    p = fwd_problem(path["counts"], K, N, group)
    E, T = 3, p["T"]
    rows = (p["x"] if kind is None else p["gate_up"]).to(din)
    pk, sc, zp, rw, cnt, off, bias = guarded_inputs(p, rows, p["bias"])
    out = guarded_out(T, N, dout)
    nbytes = lib.fql_moe_group_typed_workspace_bytes(E, T, K, N, group, 0)
    assert nbytes > 0
    ws = Guarded("workspace", nbytes, torch.uint8, 0x5A, offset=16)
    if kind is None:
        want = ops().moe_forward_any(p["P"], p["S"], p["Z"], rows, None, p["tpe"], p["offs"], out_dtype=dout, bias=p["bias"])
    else:
        want = ops().moe_gated_forward(p["P"], p["S"], p["Z"], rows, p["tpe"], p["offs"], out_dtype=dout, bias=p["bias"],
                                       activation=kind, activation_alpha=ALPHA, activation_limit=LIMIT)
    got = out.view(dout, T, N)
    results = []
    for fill in PREFILLS:                                   # what an earlier launch may have left in the workspace
        ws.bytes().fill_(fill)
        got.fill_(SENT)
        if kind is None:
            rc = lib.fql_moe_group_fwd(pk.ptr, sc.ptr, zp.ptr, rw.ptr, DT[din], cnt.ptr, off.ptr, bias.ptr, out.ptr, DT[dout], E,
                                       T, K, N, group, 0, ws.ptr, nbytes, stream())
        else:
            rc = lib.fql_moe_group_glu_fwd(pk.ptr, sc.ptr, zp.ptr, rw.ptr, DT[din], cnt.ptr, off.ptr, bias.ptr, out.ptr,
                                           DT[dout], E, T, K, N, group, 0, ACT[kind], ALPHA, LIMIT, ws.ptr, nbytes, stream())
        assert rc == 0
        assert_guards_intact(pk, sc, zp, rw, cnt, off, bias, out, ws,
                             what=f"group fwd {kind} N={N} group={group} workspace {fill:#04x}")
        assert uncovered_rows_are_zero(p, got), hex(fill)
        assert same_bits(got, want), hex(fill)
        results.append(got.clone())
    assert all(same_bits(r, results[0]) for r in results[1:])


@pytest.mark.parametrize("din,dout", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("table,N,K,group", [("40-0-9", 136, 512, 64), ("40-0-9", 70, 192, 32), ("3-0-5", 136, 512, 256),
                                             ("40-0-9", 33, 96, 32), ("3-0-5", 33, 96, 48)],
                         ids=["tiled-vec", "tiled-elem", "tiled-few-rows", "rows", "rows-g48"])
def test_backward_entry_stays_inside_its_buffers(lib, table, N, K, group, din, dout):
    p = bwd_problem(table, N, K, group)
    E, T = 3, p["T"]
    gy = p["gy"].to(din)
    pk, sc, zp, g, cnt, off = guarded_inputs(p, gy)
    out = guarded_out(T, K, dout)
    assert lib.fql_moe_group_bwd_workspace_bytes(E, T, K, N, group) == 0
    rc = lib.fql_moe_group_bwd_input(pk.ptr, sc.ptr, zp.ptr, g.ptr, DT[din], cnt.ptr, off.ptr, out.ptr, DT[dout], E, T, K, N,
                                     group, None, 0, stream())
    assert rc == 0
    assert_guards_intact(pk, sc, zp, g, cnt, off, out, what=f"group bwd {table} N={N} K={K} group={group}")
    got = out.view(dout, T, K)
    assert uncovered_rows_are_zero(p, got)
    assert same_bits(got, ops().moe_backward_input(p["P"], p["S"], p["Z"], gy, p["tpe"], p["offs"], out_dtype=dout))
