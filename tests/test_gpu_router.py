"""The fused top-k router (csrc/fql_router.h, ops.router_topk) on the GPU.

The reference is float64 torch on the widened logits: ``softmax``, the selection ``torch.sort(-logits, stable=True)``
(slot j = the j-th largest logit, ties to the lower expert id), the selected probabilities and their renormalisation.

Bounds, for |logit| <= 16:
  * weights and probs: relative error <= 4e-6 -- the rounding of l - m (up to 2^-19 relative to the exponent's argument),
    one accurate expf, a pairwise sum of at most 128 terms, at most 8 adds and a divide for the renormalisation;
  * |sum_j w_j - 1| <= top_k * 2^-23 when renormalised;
  * grad_logits: per row |err| <= 4e-5 * (max|grad_weights| + max|grad_probs|), the forward bound through at most
    top_k + 2 products.
Indices are exact.  The measured maxima are printed by each test before it asserts."""
import functools

import pytest
import torch

from helpers import Guarded, guarded_like, assert_guards_intact

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
IDS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
EXPERTS = (1, 2, 5, 8, 60, 64, 128)
TOP_KS = (1, 2, 4, 8)
TOKENS = (1, 3, 257)
REL = 4e-6
GRAD_REL = 4e-5
SENT = -7.5                        # exact in float32, float16 and bfloat16; no result of these problems
NAN = float("nan")
BIG = 0x7F7F7F7F


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fused_int4_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib(ops):
    from fused_int4_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def make_logits(T, E, dtype, seed=0):
    """Uniform in [-16, 16], rounded to ``dtype`` (built once per shape, never modified)."""
    g = torch.Generator().manual_seed(1000 * T + 7 * E + seed)
    return ((torch.rand(T, E, generator=g) * 32.0 - 16.0).to(dtype)).cuda()


def reference(logits, top_k, renormalize):
    """(indices int64, weights float64, probs float64) of the widened logits."""
    l = logits.double()
    idx = torch.sort(-l, dim=-1, stable=True).indices[:, :top_k]
    p = torch.softmax(l, dim=-1)
    sel = p.gather(1, idx)
    return idx, (sel / sel.sum(dim=-1, keepdim=True) if renormalize else sel), p


def cases():
    return [(T, E, k) for E in EXPERTS for k in TOP_KS if k <= E for T in TOKENS]


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("renormalize", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_forward_matches_float64(ops, dtype, renormalize):
    worst_w = worst_p = worst_sum = 0.0
    for T, E, k in cases():
        logits = make_logits(T, E, dtype)
        w, idx, p = ops.router_topk(logits, k, renormalize=renormalize, return_probs=True)
        assert idx.dtype == torch.int32 and w.dtype == torch.float32 and p.dtype == torch.float32
        assert idx.shape == (T, k) and w.shape == (T, k) and p.shape == (T, E)
        ridx, rw, rp = reference(logits, k, renormalize)
        assert torch.equal(idx.long(), ridx), (T, E, k)
        ew = float(((w.double() - rw).abs() / rw).max())
        ep = float(((p.double() - rp).abs() / rp).max())
        worst_w, worst_p = max(worst_w, ew), max(worst_p, ep)
        assert ew <= REL and ep <= REL, (T, E, k, ew, ep)
        if renormalize:
            es = float((w.double().sum(dim=-1) - 1.0).abs().max())
            worst_sum = max(worst_sum, es / k)
            assert es <= k * 2.0 ** -23, (T, E, k, es)
        else:                                                # the same division: the bits of probs at the chosen ids
            assert torch.equal(w, p.gather(1, idx.long())), (T, E, k)
        w2, idx2 = ops.router_topk(logits, k, renormalize=renormalize)
        assert torch.equal(idx2, idx) and same_bits(w2, w)   # probs or not: the same weights
    print(f"router forward {IDS[dtype]} renormalize={renormalize}: max rel err weights {worst_w:.3e} probs {worst_p:.3e} "
          f"(bound {REL:.0e}); max |sum w - 1| / top_k {worst_sum:.3e} (bound {2.0 ** -23:.3e})")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ties(ops, dtype):
    for T, E, k in cases():
        zeros = torch.zeros(T, E, dtype=dtype, device="cuda")
        w, idx = ops.router_topk(zeros, k)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device="cuda").expand(T, k)), (T, E, k)
        assert torch.equal(w, torch.full((T, k), 1.0 / k, dtype=torch.float32, device="cuda")), (T, E, k)
        g = torch.Generator().manual_seed(T + 31 * E + k)
        ints = torch.randint(-1, 2, (T, E), generator=g).to(dtype).cuda()
        ints[0, 0] = -0.0                                    # -0.0 == 0.0: a tie like any other
        w, idx = ops.router_topk(ints, k)
        ridx, rw, _ = reference(ints, k, True)
        assert torch.equal(idx.long(), ridx), (T, E, k)
        assert float(((w.double() - rw).abs() / rw).max()) <= REL


def test_route_plan_takes_the_indices_as_they_are(ops):
    logits = make_logits(257, 8, torch.float32)
    _, idx = ops.router_topk(logits, 2)
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert idx.reshape(-1).to(torch.int32).contiguous().data_ptr() == idx.data_ptr()      # what ops.route_plan does: no copy
    tpe, offs, token_of_sorted, pos_of_slot = ops.route_plan(idx, 8)
    assert torch.equal(tpe.long(), torch.bincount(idx.reshape(-1).long(), minlength=8))
    assert torch.equal(token_of_sorted.long(), torch.argsort(idx.reshape(-1).long(), stable=True) // 2)


# ----------------------------------------------------------------------------------------------------------- backward
def grad_reference(logits, idx, gw, gp, renormalize):
    l = logits.double().detach().requires_grad_(True)
    p = torch.softmax(l, dim=-1)
    sel = p.gather(1, idx.long())
    w = sel / sel.sum(dim=-1, keepdim=True) if renormalize else sel
    loss = l.sum() * 0.0
    if gw is not None:
        loss = loss + (w * gw.double()).sum()
    if gp is not None:
        loss = loss + (p * gp.double()).sum()
    return torch.autograd.grad(loss, l)[0]


BWD_CASES = [(T, E, k) for (T, E, k) in cases() if T != 3]


@pytest.mark.parametrize("which", ["weights", "weights+probs", "probs"])
@pytest.mark.parametrize("renormalize", [True, False], ids=["renorm", "plain"])
def test_backward_matches_float64(ops, renormalize, which):
    worst = 0.0
    for T, E, k in BWD_CASES:
        logits = make_logits(T, E, torch.float32)
        g = torch.Generator().manual_seed(5 + T + E + k)
        gw = torch.randn(T, k, generator=g).cuda() if "weights" in which else None
        gp = torch.randn(T, E, generator=g).cuda() if "probs" in which else None
        x = logits.clone().requires_grad_(True)
        out = ops.router_topk(x, k, renormalize=renormalize, return_probs=gp is not None)
        assert not out[1].requires_grad and out[0].requires_grad
        loss = (out[0] * gw).sum() if gw is not None else 0.0
        if gp is not None:
            loss = loss + (out[2] * gp).sum()
        got, = torch.autograd.grad(loss, x)
        assert got.dtype == torch.float32 and got.shape == (T, E)
        direct = ops.router_topk_backward(logits, out[1], gw, gp, renormalize=renormalize)
        assert same_bits(got, direct)                        # autograd hands over exactly the gradients that exist
        ref = grad_reference(logits, out[1], gw, gp, renormalize)
        scale = (gw.abs().amax(dim=1) if gw is not None else 0.0) + (gp.abs().amax(dim=1) if gp is not None else 0.0)
        err = float(((got.double() - ref).abs().amax(dim=1) / scale.double()).max())
        worst = max(worst, err)
        assert err <= GRAD_REL, (T, E, k, err)
        if renormalize and gp is None:                       # an expert no slot names: exactly 0.0
            chosen = torch.zeros(T, E, dtype=torch.bool, device="cuda").scatter_(1, out[1].long(), True)
            assert torch.equal(bits(got)[~chosen], torch.zeros_like(bits(got)[~chosen])), (T, E, k)
    print(f"router backward renormalize={renormalize} {which}: max row err / (max|g_w| + max|g_p|) {worst:.3e} "
          f"(bound {GRAD_REL:.0e})")


def test_backward_without_gradients_is_zero(ops):
    logits = make_logits(257, 5, torch.float32)
    _, idx = ops.router_topk(logits, 2)
    got = ops.router_topk_backward(logits, idx, None, None)
    assert torch.equal(bits(got), torch.zeros_like(bits(got)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=IDS.get)
def test_backward_16bit_is_the_float32_result_rounded_once(ops, dtype):
    for T, E, k in [(257, 5, 2), (257, 64, 8), (3, 128, 4), (1, 1, 1), (257, 8, 2)]:
        for renormalize in (True, False):
            logits = make_logits(T, E, dtype)
            g = torch.Generator().manual_seed(T + E)
            gw, gp = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
            _, idx = ops.router_topk(logits, k, renormalize=renormalize)
            got = ops.router_topk_backward(logits, idx, gw, gp, renormalize=renormalize)
            wide = ops.router_topk_backward(logits.float(), idx, gw, gp, renormalize=renormalize)
            assert got.dtype == dtype and same_bits(got, wide.to(dtype)), (T, E, k, renormalize)
            x = logits.clone().requires_grad_(True)          # through autograd: the gradient has the logits' type
            w, _ = ops.router_topk(x, k, renormalize=renormalize)
            (w * gw).sum().backward()
            assert x.grad.dtype == dtype
            assert same_bits(x.grad, ops.router_topk_backward(logits.float(), idx, gw, None, renormalize=renormalize).to(dtype))


# ------------------------------------------------------------------------------- row independence and repeatability
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("E,k", [(5, 2), (8, 2), (60, 8), (128, 4)])
def test_rows_are_independent_and_calls_repeat(ops, E, k, dtype):
    T = 257
    logits = make_logits(T, E, dtype)
    g = torch.Generator().manual_seed(E)
    gw, gp = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
    for renormalize in (True, False):
        w, idx, p = ops.router_topk(logits, k, renormalize=renormalize, return_probs=True)
        d = ops.router_topk_backward(logits, idx, gw, gp, renormalize=renormalize)
        w2, idx2, p2 = ops.router_topk(logits, k, renormalize=renormalize, return_probs=True)
        d2 = ops.router_topk_backward(logits, idx, gw, gp, renormalize=renormalize)
        assert torch.equal(idx, idx2) and same_bits(w, w2) and same_bits(p, p2) and same_bits(d, d2)
        for t in (0, 1, 7, 63, 64, 100, 255, 256):
            w1, idx1, p1 = ops.router_topk(logits[t:t + 1], k, renormalize=renormalize, return_probs=True)
            d1 = ops.router_topk_backward(logits[t:t + 1], idx1, gw[t:t + 1], gp[t:t + 1], renormalize=renormalize)
            assert torch.equal(idx1, idx[t:t + 1]) and same_bits(w1, w[t:t + 1]) and same_bits(p1, p[t:t + 1]), (t, renormalize)
            assert same_bits(d1, d[t:t + 1]), (t, renormalize)


# ---------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("E,k", [(8, 2), (5, 4), (128, 8)])
def test_non_finite_rows(ops, E, k, dtype):
    T = 19
    clean = make_logits(T, E, dtype, seed=9)
    dirty = clean.clone()
    bad = {1: NAN, 4: float("inf"), 10: float("-inf"), 18: NAN}
    for t, v in bad.items():
        dirty[t, (3 * t) % E] = v
    rows = torch.tensor(sorted(bad), device="cuda")
    good = torch.tensor([t for t in range(T) if t not in bad], device="cuda")
    g = torch.Generator().manual_seed(2)
    gw, gp = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
    for renormalize in (True, False):
        w, idx, p = ops.router_topk(dirty, k, renormalize=renormalize, return_probs=True)
        wc, idxc, pc = ops.router_topk(clean, k, renormalize=renormalize, return_probs=True)
        assert torch.isnan(w[rows]).all() and torch.isnan(p[rows]).all()
        assert torch.equal(idx[rows], torch.arange(k, dtype=torch.int32, device="cuda").expand(len(bad), k))
        assert bool(((idx >= 0) & (idx < E)).all())
        assert torch.equal(idx[good], idxc[good]) and same_bits(w[good], wc[good]) and same_bits(p[good], pc[good])
        d = ops.router_topk_backward(dirty, idx, gw, gp, renormalize=renormalize)
        dc = ops.router_topk_backward(clean, idxc, gw, gp, renormalize=renormalize)
        assert torch.isnan(d[rows]).all()
        assert same_bits(d[good], dc[good])


# ----------------------------------------------------------------------------------------------------------- footprint
def out_buffer(name, n, dtype):
    esz = torch.empty((), dtype=dtype).element_size()
    g = Guarded(name, n * esz, dtype, BIG if dtype == torch.int32 else SENT, offset=esz)
    g.view(dtype, n).fill_(-99 if dtype == torch.int32 else SENT)
    return g


@pytest.mark.parametrize("with_probs", [True, False], ids=["probs", "null_probs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_forward_footprint(ops, lib, dtype, with_probs):
    T, E, k = 257, 5, 2
    logits = make_logits(T, E, dtype)
    gl = guarded_like("logits", logits, NAN)
    gi, gw, gp = out_buffer("indices", T * k, torch.int32), out_buffer("weights", T * k, torch.float32), out_buffer("probs", T * E, torch.float32)
    rc = lib.fql_router_topk_fwd(gl.ptr, DT[dtype], T, E, k, 1, gi.ptr, gw.ptr, gp.ptr if with_probs else None, stream())
    assert rc == 0, rc
    assert_guards_intact(gl, gi, gw, gp, what=f"fql_router_topk_fwd {IDS[dtype]} probs={with_probs}")
    w, idx, p = ops.router_topk(logits, k, return_probs=True)
    assert torch.equal(gi.view(torch.int32, T, k), idx) and same_bits(gw.view(torch.float32, T, k), w)
    if with_probs:
        assert same_bits(gp.view(torch.float32, T, E), p)
    else:                                                    # nothing beyond weights / indices is written
        assert bool((gp.view(torch.float32, T * E) == SENT).all())
    assert same_bits(gl.view(dtype, T, E), logits)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_backward_footprint(ops, lib, dtype):
    T, E, k = 257, 5, 2
    logits = make_logits(T, E, dtype)
    g = torch.Generator().manual_seed(4)
    gw, gp = torch.randn(T, k, generator=g), torch.randn(T, E, generator=g)
    _, idx = ops.router_topk(logits, k)
    ins = [guarded_like("logits", logits, NAN), guarded_like("indices", idx, BIG), guarded_like("grad_weights", gw, NAN),
           guarded_like("grad_probs", gp, NAN)]
    out = out_buffer("grad_logits", T * E, dtype)
    rc = lib.fql_router_topk_bwd(ins[0].ptr, DT[dtype], ins[1].ptr, ins[2].ptr, ins[3].ptr, out.ptr, T, E, k, 1, stream())
    assert rc == 0, rc
    assert_guards_intact(*ins, out, what=f"fql_router_topk_bwd {IDS[dtype]}")
    assert same_bits(out.view(dtype, T, E), ops.router_topk_backward(logits, idx, gw.cuda(), gp.cuda()))


# ----------------------------------------------------------------------------------------------------------- refusals
def _good():
    return make_logits(3, 8, torch.float32)


REFUSALS = [
    ("cpu-logits", lambda: (_good().cpu(), 2)),
    ("int-logits", lambda: (_good().to(torch.int32), 2)),
    ("float64-logits", lambda: (_good().double(), 2)),
    ("1-d-logits", lambda: (_good()[0], 2)),
    ("3-d-logits", lambda: (_good().unsqueeze(0), 2)),
    ("129-experts", lambda: (torch.zeros(3, 129, device="cuda"), 2)),
    ("no-experts", lambda: (torch.zeros(3, 0, device="cuda"), 1)),
    ("top_k-0", lambda: (_good(), 0)),
    ("top_k-past-E", lambda: (make_logits(3, 5, torch.float32), 6)),
    ("top_k-9", lambda: (make_logits(3, 64, torch.float32), 9)),
    ("top_k-float", lambda: (_good(), 2.0)),
]


@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=lambda i: REFUSALS[i][0])
def test_refusals(ops, row):
    logits, k = REFUSALS[row][1]()
    with pytest.raises(RuntimeError):
        ops.router_topk(logits, k)
    if logits.dtype.is_floating_point and logits.dtype != torch.float64:
        with pytest.raises(RuntimeError):
            ops.router_topk(logits.clone().requires_grad_(True), k)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_non_contiguous_logits_are_accepted(ops, dtype):
    wide = make_logits(257, 128, dtype)
    view = wide[:, 3:63:1][:, ::2]                           # [257, 30], strides (128, 2)
    assert not view.is_contiguous()
    w, idx, p = ops.router_topk(view, 4, return_probs=True)
    wc, idxc, pc = ops.router_topk(view.contiguous(), 4, return_probs=True)
    assert torch.equal(idx, idxc) and same_bits(w, wc) and same_bits(p, pc)
    gw = torch.ones(257, 4, device="cuda")
    assert same_bits(ops.router_topk_backward(view, idx, gw, None), ops.router_topk_backward(view.contiguous(), idxc, gw, None))


def test_empty_batch(ops):
    w, idx, p = ops.router_topk(torch.zeros(0, 8, device="cuda"), 2, return_probs=True)
    assert w.shape == (0, 2) and idx.shape == (0, 2) and p.shape == (0, 8)
