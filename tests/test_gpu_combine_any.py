"""ops.combine_any / ops.combine_any_backward (csrc/fql_routing.h: combine_kernel, combine_bwd_kernel) on the GPU.

Every reference is built from the float32 instantiation alone (``ops.combine`` / ``ops.combine_backward``) and torch's
own casts and arithmetic, and every comparison is bit for bit:

  * no addend:    ``combine_any(y, ..., out_dtype=d) == ops.combine(y.float(), ...).to(d)`` (all float32: ``ops.combine``);
  * addend:       ``(ops.combine(y.float(), ...) + addend.float() * aw[:, None]).to(d)``: torch eager multiplies and adds in
                  two float32 kernels, no FMA; without ``aw`` the reference is ``+ addend.float()``;
  * grad_y, grad_weights: ``ops.combine_backward(g.float(), y.float(), ...)``, the first rounded once to y's type; the rows
                  no slot names come back zero;
  * grad_addend:  ``(aw[:, None] * g.float()).to(in_dtype)``;
  * grad_addend_weight: ``ops.combine_backward(g.float(), addend.float(), arange(T), ones(T, 1))[1][:, 0]``: the same
                  reduction, hence the same bits.

Shapes: T in {1, 5}, top_k in {1, 2, 8}, N in {8, 129, 130, 1029, 1032} (every access width of both element sizes, and a
second column block past 1024), R = T * top_k + 3 with ``pos`` a random injection into [0, R), weights of both signs
with a zero among them.  The guard-band tests follow tests/test_gpu_footprint.py."""
import functools
import itertools

import pytest
import torch

from helpers import ops, Guarded, assert_guards_intact

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DT_NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
TS, KS, NS = (1, 5), (1, 2, 8), (8, 129, 130, 1029, 1032)
ADDENDS = ("none", "addend", "weighted")
SENT = -7.5                        # exact in float32, float16 and bfloat16; no result of these problems


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(T, top_k, N, dtype):
    """Inputs and float32 references of one shape, built once and never modified."""
    p = Problem()
    g = torch.Generator().manual_seed(1000 * T + 100 * top_k + N)
    p.T, p.top_k, p.N, p.R = T, top_k, N, T * top_k + 3
    p.y = torch.randn(p.R, N, generator=g).to(dtype).to(DEV)
    p.pos = torch.randperm(p.R, generator=g)[:T * top_k].to(torch.int32).to(DEV)
    w = torch.randn(T, top_k, generator=g)
    w.view(-1)[-1] = 0.0                                       # (randn gives both signs wherever there are two weights)
    p.w = w.to(DEV)
    p.addend = torch.randn(T, N, generator=g).to(dtype).to(DEV)
    p.aw = torch.randn(T, generator=g).to(DEV)
    p.g32 = torch.randn(T, N, generator=g).to(DEV)
    with torch.no_grad():
        o = ops()
        p.ref = {True: o.combine(p.y.float(), p.pos, p.w), False: o.combine(p.y.float(), p.pos, None, top_k)}
        p.term = {"none": None, "addend": p.addend.float(), "weighted": p.addend.float() * p.aw[:, None]}
    return p


def operands(p, weights, addend):
    return (p.w if weights else None, p.addend if addend != "none" else None, p.aw if addend == "weighted" else None)


def forward_reference(p, weights, addend, out_dtype):
    ref = p.ref[weights]
    if addend != "none":
        ref = ref + p.term[addend]
    return ref.to(out_dtype)


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
def test_forward_bits(dtype, N):
    checked = 0
    with torch.no_grad():
        for T, top_k, weights, addend, out_dtype in itertools.product(TS, KS, (True, False), ADDENDS, DTYPES):
            p = problem(T, top_k, N, dtype)
            w, a, aw = operands(p, weights, addend)
            got = ops().combine_any(p.y, p.pos, w, top_k, addend=a, addend_weight=aw, out_dtype=out_dtype)
            ref = forward_reference(p, weights, addend, out_dtype)
            assert same_bits(got, ref), (T, top_k, weights, addend, out_dtype)
            again = ops().combine_any(p.y, p.pos, w, top_k, addend=a, addend_weight=aw, out_dtype=out_dtype)
            assert same_bits(again, got), "a second call gives other bits"
            checked += 1
        p = problem(5, 2, N, dtype)
        assert ops().combine_any(p.y, p.pos, p.w).dtype == dtype                  # out_dtype defaults to y's
        if dtype == torch.float32:
            assert same_bits(ops().combine_any(p.y, p.pos, p.w), ops().combine(p.y, p.pos, p.w))
    print(f"combine_any {DT_NAME[dtype]} N={N}: {checked} forward cases bit-identical")


def test_float16_overflow_gives_inf():
    y = torch.full((4, 130), 60000.0, dtype=torch.float16, device=DEV)
    y[1] = -60000.0
    pos = torch.arange(4, dtype=torch.int32, device=DEV)
    w = torch.ones(2, 2, device=DEV)
    addend = torch.full((2, 130), 30000.0, dtype=torch.float16, device=DEV)
    with torch.no_grad():
        got = ops().combine_any(y, pos, w)
        ref = ops().combine(y.float(), pos, w).to(torch.float16)
        assert same_bits(got, ref) and bool(torch.isinf(got[1]).all()) and bool((got[0] == 0).all())
        got = ops().combine_any(y[2:], pos[:2], w[:, :1], addend=addend)
        ref = (ops().combine(y[2:].float(), pos[:2], w[:, :1]) + addend.float()).to(torch.float16)
        assert same_bits(got, ref) and bool(torch.isinf(got).all())
        wide = ops().combine_any(y[2:], pos[:2], w[:, :1], addend=addend, out_dtype=torch.float32)
        assert bool((wide == 90000.0).all())                                       # the sum itself is float32


# ----------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
def test_backward_bits(dtype, N):
    o, checked = ops(), 0
    with torch.no_grad():
        for T, top_k, weights, addend, out_dtype in itertools.product(TS, KS, (True, False), ADDENDS, DTYPES):
            p = problem(T, top_k, N, dtype)
            w, a, aw = operands(p, weights, addend)
            g = p.g32.to(out_dtype)
            gy, gw, ga, gaw = o.combine_any_backward(g, p.y, p.pos, w, top_k, addend=a, addend_weight=aw)
            what = (T, top_k, weights, addend, out_dtype)
            ref_gy, ref_gw = o.combine_backward(g.float(), p.y.float(), p.pos, w, top_k)
            assert same_bits(gy, ref_gy.to(dtype)), what
            named = torch.zeros(p.R, dtype=torch.bool, device=DEV)
            named[p.pos.long()] = True
            assert int(named.sum()) == T * top_k and bool((gy[~named] == 0).all()), what
            assert (gw is None and ref_gw is None) or same_bits(gw, ref_gw), what
            if addend == "none":
                assert ga is None and gaw is None
            else:
                ref_ga = (aw[:, None] * g.float() if aw is not None else g.float()).to(dtype)
                assert same_bits(ga, ref_ga), what
            if addend == "weighted":
                ref_gaw = o.combine_backward(g.float(), p.addend.float(), torch.arange(T, dtype=torch.int32, device=DEV),
                                             torch.ones(T, 1, device=DEV))[1][:, 0]
                assert same_bits(gaw, ref_gaw), what
            else:
                assert gaw is None
            again = o.combine_any_backward(g, p.y, p.pos, w, top_k, addend=a, addend_weight=aw)
            for first, second in zip((gy, gw, ga, gaw), again):
                assert (first is None and second is None) or same_bits(first, second), "a second call gives other bits"
            checked += 1
    print(f"combine_any_backward {DT_NAME[dtype]} N={N}: {checked} cases bit-identical")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
def test_autograd_returns_the_four_gradients(dtype):
    o = ops()
    p = problem(5, 2, 130, dtype)
    out_dtype = torch.float32 if dtype == torch.float16 else dtype
    g = p.g32.to(out_dtype)
    with torch.no_grad():
        want = o.combine_any_backward(g, p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw)
        want_out = o.combine_any(p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw, out_dtype=out_dtype)
    leaves = [t.clone().requires_grad_(True) for t in (p.y, p.w, p.addend, p.aw)]
    out = o.combine_any(leaves[0], p.pos, leaves[1], addend=leaves[2], addend_weight=leaves[3], out_dtype=out_dtype)
    assert same_bits(out.detach(), want_out)
    out.backward(g)
    for leaf, ref in zip(leaves, want):
        assert same_bits(leaf.grad, ref)
    # None where an input does not require grad: each input alone
    for i in range(4):
        leaves = [t.clone().requires_grad_(j == i) for j, t in enumerate((p.y, p.w, p.addend, p.aw))]
        out = o.combine_any(leaves[0], p.pos, leaves[1], addend=leaves[2], addend_weight=leaves[3], out_dtype=out_dtype)
        out.backward(g)
        for j, (leaf, ref) in enumerate(zip(leaves, want)):
            if j == i:
                assert same_bits(leaf.grad, ref), (i, j)
            else:
                assert leaf.grad is None, (i, j)
    # the pure gather-add form (no weights: top_k given) through autograd
    y = p.y.clone().requires_grad_(True)
    o.combine_any(y, p.pos, None, 2, out_dtype=out_dtype).backward(g)
    assert same_bits(y.grad, o.combine_backward(g.float(), p.y.float(), p.pos, None, 2)[0].to(dtype))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    o = ops()
    p = problem(5, 2, 8, torch.bfloat16)
    with pytest.raises(RuntimeError, match="y must be"):
        o.combine_any(p.y.cpu(), p.pos, p.w)
    with pytest.raises(RuntimeError, match="y must be"):
        o.combine_any(p.y.double(), p.pos, p.w)
    with pytest.raises(RuntimeError, match="y must be"):
        o.combine_any(p.y[0], p.pos, p.w)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend.cpu())
    with pytest.raises(RuntimeError, match="addend must be"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend.float())                    # not y's type
    with pytest.raises(RuntimeError, match="addend must be"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend[:4])
    with pytest.raises(RuntimeError, match="addend must be"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend[:, :4])
    with pytest.raises(RuntimeError, match="addend_weight needs an addend"):
        o.combine_any(p.y, p.pos, p.w, addend_weight=p.aw)
    with pytest.raises(RuntimeError, match="addend_weight must be"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="addend_weight must be"):
        o.combine_any(p.y, p.pos, p.w, addend=p.addend, addend_weight=p.aw[:, None])
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        o.combine_any(p.y, p.pos, p.w, out_dtype=torch.float64)
    with pytest.raises(RuntimeError, match="top_k is needed"):
        o.combine_any(p.y, p.pos, None)
    with pytest.raises(RuntimeError, match="pos_of_slot must have"):
        o.combine_any(p.y, p.pos[:3], p.w)
    T = 65536
    y = torch.zeros(8, 8, dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="65535"):
        o.combine_any(y, pos, None, 1)
    g = p.g32.to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="grad_out must be"):
        o.combine_any_backward(g[:4], p.y, p.pos, p.w)
    with pytest.raises(RuntimeError, match="grad_out must be"):
        o.combine_any_backward(g.double(), p.y, p.pos, p.w)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        o.combine_any_backward(g.cpu(), p.y, p.pos, p.w)
    with pytest.raises(RuntimeError, match="addend_weight needs an addend"):
        o.combine_any_backward(g, p.y, p.pos, p.w, addend_weight=p.aw)
    # ops.combine keeps its own refusals
    with pytest.raises(RuntimeError, match="y must be"):
        o.combine(p.y, p.pos, p.w)


# --------------------------------------------------------------------------------------------------------- guard bands
GUARD_CASES = [(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
               (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)]
# (N, offset of every guarded buffer past a 256-byte boundary in elements; 0: 16 bytes, the wide accesses engage)
GUARD_SHAPES = [(129, 1), (1029, 1), (130, 0), (1032, 0)]


def guarded(name, shape, dtype, aligned):
    t = torch.empty((), dtype=dtype)
    n = 1
    for s in shape:
        n *= s
    b = Guarded(name, n * t.element_size(), dtype, SENT, 16 if aligned else t.element_size())
    b.view(dtype, *shape).fill_(SENT)
    return b


@pytest.mark.parametrize("N,offset", GUARD_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("in_dtype,out_dtype", GUARD_CASES, ids=[f"{DT_NAME[a]}-{DT_NAME[b]}" for a, b in GUARD_CASES])
def test_guard_bands(in_dtype, out_dtype, N, offset):
    from fused_int4_amd import _native
    lib = _native.lib()
    T, top_k = 5, 2
    p = problem(T, top_k, N, in_dtype)
    R, aligned = p.R, offset == 0
    stream = torch.cuda.current_stream().cuda_stream
    w, pos = p.w.contiguous(), p.pos.contiguous()
    out = guarded("out", (T, N), out_dtype, aligned)
    rc = lib.fql_combine(p.y.data_ptr(), DT_CODE[in_dtype], pos.data_ptr(), w.data_ptr(), p.addend.data_ptr(), p.aw.data_ptr(),
                         out.ptr, DT_CODE[out_dtype], T, top_k, N, R, stream)
    assert rc == 0
    assert_guards_intact(out, what="fql_combine")
    assert same_bits(out.view(out_dtype, T, N), forward_reference(p, True, "weighted", out_dtype))

    g = p.g32.to(out_dtype)
    gy = guarded("grad_y", (R, N), in_dtype, aligned)
    ga = guarded("grad_addend", (T, N), in_dtype, aligned)
    gw = guarded("grad_weights", (T, top_k), torch.float32, aligned)
    gaw = guarded("grad_addend_weight", (T,), torch.float32, aligned)
    rc = lib.fql_combine_bwd(g.data_ptr(), DT_CODE[out_dtype], p.y.data_ptr(), pos.data_ptr(), w.data_ptr(),
                             p.addend.data_ptr(), p.aw.data_ptr(), DT_CODE[in_dtype], gy.ptr, gw.ptr, ga.ptr, gaw.ptr, T, top_k, N,
                             R, stream)
    assert rc == 0
    assert_guards_intact(gy, ga, gw, gaw, what="fql_combine_bwd")
    ref_gy, ref_gw = ops().combine_backward(g.float(), p.y.float(), p.pos, p.w)
    named = torch.zeros(R, dtype=torch.bool, device=DEV)
    named[p.pos.long()] = True
    got_gy = gy.view(in_dtype, R, N)
    assert int((~named).sum()) == 3 and bool((got_gy[~named] == SENT).all()), "a row no slot names was written"
    assert same_bits(got_gy[named], ref_gy.to(in_dtype)[named])
    assert same_bits(gw.view(torch.float32, T, top_k), ref_gw)
    assert same_bits(ga.view(in_dtype, T, N), (p.aw[:, None] * g.float()).to(in_dtype))
    assert not bool((gaw.view(torch.float32, T) == SENT).any())
