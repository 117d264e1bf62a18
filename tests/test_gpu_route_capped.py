"""fql_route_plan_capped_i32 and the sparse combine pair on the GPU (csrc/fql_routing.h, FQL_VERSION 320).

The plan is compared, integer for integer, with ``plan_reference`` of tests/test_route_capped_cpu.py (stable argsort,
per-expert rank, cap, mask), the zero tail of ``token_of_sorted`` included.  Its outputs sit in guarded buffers, and the
input table is followed by huge indices that would send a kernel far away if it read them.

The sparse combine has no arithmetic of its own, so every comparison is bit for bit against the dense pair:
  * forward:  ``combine_any`` on the same inputs with the negative positions set to 0 and the dropped slots' weights to 0
              (without weights: with the weights 1 / 0);
  * backward: ``combine_any_backward`` with the dropped slots pointed at the rows no kept slot names (a permutation
              again, as the dense kernel requires) and their weights 0: the kept rows of ``grad_y``, the kept slots of
              ``grad_weights`` and both addend gradients have the same bits; the unnamed rows and the dropped slots'
              weight gradients are exactly zero."""
import functools
import itertools

import pytest
import torch

from helpers import BIG, Guarded, assert_guards_intact, guarded_like, misaligned, ops
from test_route_capped_cpu import plan_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.5
DT_NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def lib():
    from fused_int4_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- plan
PLAN_SHAPES = [(1, 1, 1), (5, 2, 8), (37, 8, 64), (300, 2, 128), (129, 3, 7)]
# A thread walks its ceil(n_slots / 256) slots in batches of ROUTE_BATCH = 4 and carries the token index from one batch to
# the next; the shapes above give a thread at most 3 slots, one batch.  These give 9 (two full batches and one slot,
# top_k = 3 never ends a batch on a token), 8 (two full batches, top_k divides the batch: the headline's plan), 42 (ten
# full batches and two slots, top_k = 5 longer than a batch, the largest LDS footprint) and 5 (a batch, then one slot).
MULTI_BATCH_SHAPES = [(700, 3, 7), (1024, 2, 8), (2100, 5, 128), (256, 5, 16)]
ALL_PLAN_SHAPES = PLAN_SHAPES + MULTI_BATCH_SHAPES
MASKS = ("none", "all_true", "all_false", "random")
NAMES = ("counts", "offsets", "token_of_sorted", "pos_of_slot", "demand")


def make_mask(kind, T, g):
    if kind == "none":
        return None
    if kind == "all_true":
        return torch.ones(T, dtype=torch.bool, device=DEV)
    if kind == "all_false":
        return torch.zeros(T, dtype=torch.bool, device=DEV)
    return (torch.rand(T, generator=g) < 0.6).to(DEV)


def run_plan_guarded(idx, E, capacity, mask):
    """The C entry point on guarded buffers: the five outputs as int32 tensors, in the order of ``plan_reference``."""
    T, top_k = idx.shape
    n = T * top_k
    table = guarded_like("expert_of_slot", idx.reshape(-1).to(torch.int32), BIG)
    mbuf = None if mask is None else guarded_like("token_mask", mask.to(torch.uint8), 0xFF)
    outs = {name: Guarded(name, 4 * (E if name in ("counts", "offsets", "demand") else n), torch.int32, BIG, 4)
            for name in NAMES}
    for b in outs.values():
        b.bytes().fill_(0xA5)                                   # nothing the plan writes: every element must be written
    rc = lib().fql_route_plan_capped_i32(table.ptr, n, top_k, E, None if mbuf is None else mbuf.ptr,
                                         0 if capacity is None else capacity, outs["demand"].ptr, outs["counts"].ptr,
                                         outs["offsets"].ptr, outs["token_of_sorted"].ptr, outs["pos_of_slot"].ptr,
                                         stream())
    assert rc == 0
    assert_guards_intact(table, *([mbuf] if mbuf is not None else []), *outs.values(), what="fql_route_plan_capped_i32")
    return tuple(outs[name].view(torch.int32, -1).clone() for name in NAMES)


def check_plan(idx, E, capacity, mask, what):
    got = run_plan_guarded(idx, E, capacity, mask)
    ref = plan_reference(idx, E, capacity, mask)
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), (what, name)
    return ref


@pytest.mark.parametrize("T,top_k,E", ALL_PLAN_SHAPES, ids=lambda v: str(v))
def test_plan_against_the_restatement(T, top_k, E):
    g = torch.Generator().manual_seed(100 * T + E)
    idx = torch.randint(0, E, (T, top_k), generator=g, dtype=torch.int32).to(DEV)
    n, checked, dropped = T * top_k, 0, 0
    for kind in MASKS:
        mask = make_mask(kind, T, g)
        top = int(plan_reference(idx, E, None, mask)[4].max())
        capacities = [None] + sorted({c for c in (1, top, top - 1, n + 5) if c >= 1})
        for capacity in capacities:
            counts, offsets, tos, pos, demand = check_plan(idx, E, capacity, mask, (T, top_k, E, kind, capacity))
            kept = int(counts.sum())
            assert int((pos >= 0).sum()) == kept and not tos[kept:].any()
            if kind == "all_false":
                assert not counts.any() and not demand.any() and bool((pos == -1).all())
            if capacity is not None:
                assert int(counts.max()) <= capacity
            dropped += int(demand.sum()) - kept
            checked += 1
    print(f"capped plan T={T} top_k={top_k} E={E}: {checked} cases integer-equal, {dropped} slots dropped by a capacity")
    assert dropped > 0 or n == 1


@pytest.mark.parametrize("T,top_k,E", [(129, 3, 7), (700, 3, 7)], ids=lambda v: str(v))
def test_plan_every_slot_on_one_expert(T, top_k, E):
    idx = torch.full((T, top_k), 4, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(5)
    for capacity, kind in itertools.product((None, 1, 100, T * top_k - 1, T * top_k), ("none", "random")):
        counts, _, _, pos, demand = check_plan(idx, E, capacity, make_mask(kind, T, g), (capacity, kind))
        assert int(demand[4]) == int(demand.sum()) and int(counts[4]) == int(counts.sum())
        if capacity == 100:
            assert int(counts[4]) == 100 and int((pos >= 0).sum()) == 100


@pytest.mark.parametrize("T,top_k,E", [(37, 8, 64), (2100, 5, 128)], ids=lambda v: str(v))
def test_plan_ids_outside_the_range_are_clamped(T, top_k, E):
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(-E - 6, 2 * E + 12, (T, top_k), generator=g, dtype=torch.int32)
    idx[0, 0], idx[0, 1] = -2 ** 31, 2 ** 31 - 1
    idx = idx.to(DEV)
    assert bool((idx < 0).any()) and bool((idx >= E).any())
    for capacity, kind in itertools.product((None, 2), ("none", "random")):
        check_plan(idx, E, capacity, make_mask(kind, T, g), (capacity, kind))


@pytest.mark.parametrize("T,top_k,E", ALL_PLAN_SHAPES, ids=lambda v: str(v))
def test_plan_unlimited_and_unmasked_is_route_plan(T, top_k, E):
    g = torch.Generator().manual_seed(7 * T + E)
    idx = torch.randint(0, E, (T, top_k), generator=g, dtype=torch.int32).to(DEV)
    old = ops().route_plan(idx, E)
    new = ops().route_plan_capped(idx, E)
    assert len(new) == 5
    for a, b in zip(old, new[:4]):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    assert torch.equal(new[4], new[0])
    raw = run_plan_guarded(idx, E, None, None)
    for a, b in zip(old, raw[:4]):
        assert torch.equal(a, b)
    # the Python op with both arguments is the C call; a bool and a uint8 mask are the same mask
    mask = make_mask("random", T, g)
    for capacity in (None, 2):
        ref = plan_reference(idx, E, capacity, mask)
        for m in (mask, mask.to(torch.uint8)):
            for a, b in zip(ops().route_plan_capped(idx, E, capacity, m), ref):
                assert torch.equal(a, b)
    again = ops().route_plan_capped(idx.long(), E, 2, mask)                      # any integer type of indices
    for a, b in zip(again, plan_reference(idx, E, 2, mask)):
        assert torch.equal(a, b)


def test_plan_refusals():
    o = ops()
    idx = torch.zeros(5, 2, dtype=torch.int32, device=DEV)
    mask = torch.ones(5, dtype=torch.bool, device=DEV)
    for bad in (0, -1, 1.5, float("nan"), float("inf"), float("-inf"), "8", 2 ** 31):
        with pytest.raises(RuntimeError, match="capacity"):
            o.route_plan_capped(idx, 8, capacity=bad)
    with pytest.raises(RuntimeError, match="token_mask"):
        o.route_plan_capped(idx, 8, token_mask=mask.cpu())                       # the wrong device
    with pytest.raises(RuntimeError, match="token_mask"):
        o.route_plan_capped(idx, 8, token_mask=mask[:4])                         # the wrong length
    with pytest.raises(RuntimeError, match="token_mask"):
        o.route_plan_capped(idx, 8, token_mask=mask.reshape(5, 1))               # the wrong rank
    with pytest.raises(RuntimeError, match="token_mask"):
        o.route_plan_capped(idx, 8, token_mask=mask.float())
    with pytest.raises(RuntimeError, match="expert_indices"):
        o.route_plan_capped(idx.reshape(-1), 8)
    with pytest.raises(RuntimeError, match="experts"):
        o.route_plan_capped(idx, 129)


# ------------------------------------------------------------------------------------------------------ sparse combine
T_C = 7
COMBINE_TYPES = [(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
                 (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)]
NS, KS = (1, 8, 1001, 4096), (1, 2, 8)
ADDENDS = ("none", "addend", "weighted")


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(top_k, N, dtype):
    """Inputs of one shape, built once and never modified.  Token 0 loses every slot, token 1 keeps every slot, the
    others lose a slot with probability 1 / 3; ``pos`` is an injection of the kept slots into the R = T * top_k rows."""
    p = Problem()
    T = T_C
    g = torch.Generator().manual_seed(100 * top_k + N)
    p.T, p.top_k, p.N, p.R = T, top_k, N, T * top_k
    keep = torch.rand(T, top_k, generator=g) >= 1.0 / 3.0
    keep[0], keep[1] = False, True
    if top_k > 1:
        keep[2, 0], keep[2, 1] = True, False                   # a token that is neither
    assert bool((~keep).all(dim=1).any()) and bool(keep.all(dim=1).any())         # the test's own input
    if top_k == 8:
        assert 0.15 < float((~keep).float().mean()) < 0.55
    p.keep = keep.to(DEV)
    perm = torch.randperm(p.R, generator=g).to(torch.int32).view(T, top_k)
    p.pos_perm = perm.to(DEV)                                                     # dropped slots name the unused rows
    p.pos = torch.where(keep, perm, torch.full_like(perm, -1)).to(DEV)
    p.pos[0, 0] = -2 ** 31                                                        # any negative position is a drop
    p.pos_clamped = p.pos.clamp(min=0)
    p.y = torch.randn(p.R, N, generator=g).to(dtype).to(DEV)
    w = torch.randn(T, top_k, generator=g)
    p.w = w.to(DEV)
    p.w_zeroed = torch.where(keep, w, torch.zeros_like(w)).to(DEV)
    p.addend = torch.randn(T, N, generator=g).to(dtype).to(DEV)
    p.aw = torch.randn(T, generator=g).to(DEV)
    p.g32 = torch.randn(T, N, generator=g).to(DEV)
    return p


# Every buffer of a call starts `off` elements past a 16-byte boundary.  0: the wide accesses (N a multiple of the vector);
# 2 with an even N: the two-element accesses; 1, or an odd N: one element at a time (csrc/fql_routing.h, CombRow::mode).
OFFSETS = (0, 1, 2)


def guarded(name, shape, dtype, off, fill=SENT):
    esz = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    b = Guarded(name, n * esz, dtype, SENT, off * esz if off else 16)
    b.view(dtype, *shape).fill_(fill)
    return b


def placed(t, off):
    return misaligned(t, off) if off else t.contiguous()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("in_dtype,out_dtype", COMBINE_TYPES, ids=[f"{DT_NAME[a]}-{DT_NAME[b]}" for a, b in COMBINE_TYPES])
def test_sparse_combine_bits(in_dtype, out_dtype, N):
    o, L, checked = ops(), lib(), 0
    T = T_C
    with torch.no_grad():
        for top_k, off, addend, weights in itertools.product(KS, OFFSETS, ADDENDS, (True, False)):
            p = problem(top_k, N, in_dtype)
            R, what = p.R, (top_k, off, addend, weights)
            y = placed(p.y, off)
            a = placed(p.addend, off) if addend != "none" else None
            aw = p.aw if addend == "weighted" else None
            w = p.w.contiguous() if weights else None
            pos = p.pos.contiguous()
            ptr = lambda t: None if t is None else t.data_ptr()
            # ---- forward
            out = guarded("out", (T, N), out_dtype, off)
            rc = L.fql_combine_sparse(y.data_ptr(), DT_CODE[in_dtype], pos.data_ptr(), ptr(w), ptr(a), ptr(aw), out.ptr,
                                      DT_CODE[out_dtype], T, top_k, N, R, stream())
            assert rc == 0, what
            assert_guards_intact(out, what="fql_combine_sparse")
            w_ref = p.w_zeroed if weights else p.keep.float()
            ref = o.combine_any(p.y, p.pos_clamped, w_ref, addend=None if a is None else p.addend, addend_weight=aw,
                                out_dtype=out_dtype)
            got = out.view(out_dtype, T, N)
            assert same_bits(got, ref), what
            if addend == "none":
                assert not got[0].any(), what                   # every slot dropped, no addend: zeros
            # the Python op takes the same kernel
            assert same_bits(o.combine_any(y, pos, w, top_k, addend=a, addend_weight=aw, out_dtype=out_dtype,
                                           skip_dropped=True), ref), what
            # ---- backward
            g = placed(p.g32.to(out_dtype), off)
            gy = guarded("grad_y", (R, N), in_dtype, off, fill=0.0)
            gw = guarded("grad_weights", (T, top_k), torch.float32, off) if weights else None
            ga = guarded("grad_addend", (T, N), in_dtype, off) if a is not None else None
            gaw = guarded("grad_addend_weight", (T,), torch.float32, off) if aw is not None else None
            gptr = lambda b: None if b is None else b.ptr
            rc = L.fql_combine_sparse_bwd(g.data_ptr(), DT_CODE[out_dtype], y.data_ptr(), pos.data_ptr(), ptr(w), ptr(a),
                                          ptr(aw), DT_CODE[in_dtype], gy.ptr, gptr(gw), gptr(ga), gptr(gaw), T, top_k, N, R,
                                          stream())
            assert rc == 0, what
            assert_guards_intact(*(b for b in (gy, gw, ga, gaw) if b is not None), what="fql_combine_sparse_bwd")
            r_gy, r_gw, r_ga, r_gaw = o.combine_any_backward(p.g32.to(out_dtype), p.y, p.pos_perm, w_ref,
                                                             addend=None if a is None else p.addend, addend_weight=aw)
            named = torch.zeros(R, dtype=torch.bool, device=DEV)
            named[p.pos_perm[p.keep].long()] = True
            got_gy = gy.view(in_dtype, R, N)
            assert int(named.sum()) == int(p.keep.sum())
            assert same_bits(got_gy[named], r_gy[named]), what
            assert not got_gy[~named].any(), what
            if weights:
                got_gw = gw.view(torch.float32, T, top_k)
                assert same_bits(got_gw[p.keep], r_gw[p.keep]), what
                assert torch.equal(bits(got_gw[~p.keep]), torch.zeros_like(bits(got_gw[~p.keep]))), what
            if a is not None:
                assert same_bits(ga.view(in_dtype, T, N), r_ga), what
            if aw is not None:
                assert same_bits(gaw.view(torch.float32, T), r_gaw), what
            s_gy, s_gw, s_ga, s_gaw = o.combine_any_backward(g, y, pos, w, top_k, addend=a, addend_weight=aw,
                                                             skip_dropped=True)
            assert same_bits(s_gy, got_gy) and (not weights or same_bits(s_gw, got_gw)), what
            assert (s_ga is None) == (a is None) and (s_gaw is None) == (aw is None), what
            checked += 1
    print(f"sparse combine {DT_NAME[in_dtype]}->{DT_NAME[out_dtype]} N={N}: {checked} forward + backward cases bit-identical")


def test_sparse_combine_clamps_a_position_past_the_rows():
    p = problem(2, 8, torch.float32)
    pos = p.pos.clone()
    pos[1, 0] = p.R + 7
    with torch.no_grad():
        got = ops().combine_any(p.y, pos, p.w, skip_dropped=True)
        pos[1, 0] = p.R - 1
        assert same_bits(got, ops().combine_any(p.y, pos.clamp(min=0), p.w_zeroed))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sparse_autograd(dtype):
    """``combine_any`` and ``dispatch_rows`` carry ``skip_dropped`` through autograd; without it the dense kernels run."""
    o = ops()
    p = problem(2, 1001, dtype)
    g = p.g32.to(dtype)
    with torch.no_grad():
        want = o.combine_any_backward(g, p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw, skip_dropped=True)
        want_out = o.combine_any(p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw, skip_dropped=True)
    leaves = [t.clone().requires_grad_(True) for t in (p.y, p.w, p.addend, p.aw)]
    out = o.combine_any(leaves[0], p.pos, leaves[1], addend=leaves[2], addend_weight=leaves[3], skip_dropped=True)
    assert same_bits(out.detach(), want_out)
    out.backward(g)
    for leaf, ref in zip(leaves, want):
        assert same_bits(leaf.grad, ref)
    assert not leaves[1].grad[~p.keep].any()
    # the dispatch: x[token_of_sorted] forward; backward the sparse gather-add over pos
    T, top_k = p.T, p.top_k
    x = torch.randn(T, 64, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    tos = torch.zeros(T * top_k, dtype=torch.int32, device=DEV)
    tos[p.pos_perm[p.keep].long()] = torch.arange(T * top_k, device=DEV).view(T, top_k)[p.keep].int() // top_k
    grad_rows = torch.randn(T * top_k, 64, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    xg = x.clone().requires_grad_(True)
    rows = o.dispatch_rows(xg, tos, p.pos, top_k, skip_dropped=True)
    assert same_bits(rows.detach(), x[tos.long()])
    rows.backward(grad_rows)
    with torch.no_grad():
        ref = o.combine_any(grad_rows, p.pos_clamped, p.keep.float(), out_dtype=dtype)
    assert same_bits(xg.grad, ref) and not xg.grad[0].any()
