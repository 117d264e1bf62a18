"""The scored router (csrc/fql_router.h, ops.router_score_topk) on the GPU: sigmoid / softmax scores, selection
bias, group-limited selection, scaling factor.

Two references, neither of them the kernel:
  * VALUES: float64 torch on the widened logits (``torch.softmax`` / ``torch.sigmoid``, the documented weight formulas on
    the kernel's indices, autograd for the gradients).
  * SELECTION: a float32 torch restatement on the kernel's own float32 ``scores`` (checked against float64 by the value
    test): key = logit without a bias, else ``scores + bias`` (one add); a group's score ``amax`` or the sum of its two
    largest (one add); ``torch.sort(-x, stable=True)`` for the groups and for the experts.  Every step is a single IEEE
    operation or a comparison, so the indices are compared for equality, in every case.

Inputs: logits uniform in [-16, 16] rounded to the element type; with at least 3 tokens, row 1 holds +30 and -30 and
row 2 holds +120 and -120 (a sigmoid is exactly 1.0f at +30 and +120 and exactly 0.0f at -120; asserted).  A single
expert (E = 1) gets no -120: its one weight 0 / (0 + 1e-20) would be compared with float64's 7.7e-53 / 1e-20.  The bias is
uniform in [-0.2, 0.2]: it reorders experts and groups, and cannot push the expert at +120 out of a softmax selection
(all the others' probabilities underflow there, and a renormalised 0 / 0 is no case of this test).

Bounds, as DESIGN.md section 16 derives them (the op counts here are no larger: one accurate expf, one add and one
divide for a sigmoid; the softmax as there; at most 8 adds, one divide and one multiply for a weight):
  * weights and scores: |err| <= 4e-6 * |ref| + 2^-148 * max(1, |scale|).  The second term is two spacings of float32
    below its normal range: where the float64 value is under 2^-126 (softmax next to a logit of 120; the sigmoid of
    -120) float32 holds 0 or one subnormal step;
  * grad_logits: per row |err| <= 4e-5 * (|scale| * max|grad_weights| + max|grad_scores|).
The measured maxima are printed by each test before it asserts."""
import functools
import itertools

import pytest
import torch

from helpers import Guarded, guarded_like, assert_guards_intact

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
IDS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
SCORINGS = ["softmax", "sigmoid"]
# (E, n_group, topk_group, top_k): groups that are no power of two wide, split across a lane's two experts, straddling
# the wave's halves, one expert per group, two per group, no groups at 64 / 5 / 1 experts
CONFIGS = [(60, 4, 2, 8), (128, 8, 4, 8), (96, 3, 1, 4), (8, 8, 2, 2), (8, 4, 1, 2), (64, 1, 1, 6), (5, 1, 1, 2), (1, 1, 1, 1)]
TOKENS = (1, 3, 257)
SCALES = (1.0, 2.5)
REL = 4e-6
GRAD_REL = 4e-5
TINY = 2.0 ** -148
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
def make_logits(T, E, dtype, seed=0, special=True):
    """Uniform in [-16, 16] rounded to ``dtype``, plus the rows at +-30 and +-120 (built once, never modified)."""
    g = torch.Generator().manual_seed(1000 * T + 7 * E + seed)
    l = torch.rand(T, E, generator=g) * 32.0 - 16.0
    if special and T >= 3:
        l[1, (E - 1) // 2] = 30.0
        l[2, 1 % E] = 120.0
        if E > 1:
            l[1, E - 1] = -30.0
            l[2, E - 1] = -120.0
    return l.to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def make_bias(E, seed=0):
    g = torch.Generator().manual_seed(77 + E + seed)
    return (torch.rand(E, generator=g) * 0.4 - 0.2).cuda()


def scores64(logits, scoring):
    l = logits.double()
    return torch.softmax(l, dim=-1) if scoring == "softmax" else torch.sigmoid(l)


def weights64(s, idx, scoring, renormalize, scale):
    """The documented weight formulas in float64 on the scores ``s`` (differentiable)."""
    sel = s.gather(1, idx.long())
    if renormalize:
        sel = sel / (sel.sum(dim=-1, keepdim=True) + (1e-20 if scoring == "sigmoid" else 0.0))
    return sel * scale


def select32(logits, scores, bias, n_group, topk_group, group_top, top_k):
    """The selection restated in float32 torch on the kernel's ``scores``: (indices int64, chosen groups bool)."""
    T, E = scores.shape
    key = logits.float() if bias is None else scores + bias                        # the one add
    gv = scores if bias is None else key
    allowed = torch.ones(T, E, dtype=torch.bool, device=scores.device)
    chosen = torch.ones(T, 1, dtype=torch.bool, device=scores.device)
    if n_group > 1:
        per = E // n_group
        v = gv.view(T, n_group, per)
        if group_top == 1 or per == 1:
            gs = v.amax(dim=-1)
        else:
            top2 = torch.sort(v, dim=-1, descending=True).values
            gs = top2[..., 0] + top2[..., 1]                                       # the one add
        gidx = torch.sort(-gs, dim=-1, stable=True).indices[:, :topk_group]
        chosen = torch.zeros(T, n_group, dtype=torch.bool, device=scores.device).scatter_(1, gidx, True)
        allowed = chosen.repeat_interleave(per, dim=1)
    order = torch.sort(-key, dim=-1, stable=True).indices
    ok = allowed.gather(1, order)
    pick = ok & (ok.cumsum(dim=1) <= top_k)                                        # the first top_k allowed, in key order
    assert bool((pick.sum(dim=1) == top_k).all())
    return order[pick].view(T, top_k), chosen


def value_error(got, ref, scale=1.0):
    """max over the elements of |got - ref| / (REL * |ref| + TINY * max(1, |scale|)): <= 1 is inside the bound; and the
    largest relative error among the elements of normal size, for the report."""
    err = (got.double() - ref).abs()
    tol = REL * ref.abs() + TINY * max(1.0, abs(scale))
    normal = ref.abs() >= 2.0 ** -100
    rel = float((err[normal] / ref.abs()[normal]).max()) if bool(normal.any()) else 0.0
    return float((err / tol).max()), rel


def settings():
    """(group_top, bias?, renormalize, scale) for every configuration."""
    return list(itertools.product((1, 2), (False, True), (True, False), SCALES))


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_forward_values_and_selection(ops, dtype, scoring):
    worst_w = worst_s = 0.0
    for (E, n_group, topk_group, k), T in itertools.product(CONFIGS, TOKENS):
        logits = make_logits(T, E, dtype)
        s64 = scores64(logits, scoring)
        for group_top, with_bias, renormalize, scale in settings():
            bias = make_bias(E) if with_bias else None
            what = (T, E, n_group, topk_group, k, group_top, with_bias, renormalize, scale)
            w, idx, s = ops.router_score_topk(logits, k, scoring, bias, n_group, topk_group, group_top, renormalize, scale,
                                              return_scores=True)
            assert idx.dtype == torch.int32 and w.dtype == torch.float32 and s.dtype == torch.float32
            assert idx.shape == (T, k) and w.shape == (T, k) and s.shape == (T, E)
            es, rel_s = value_error(s, s64)
            assert es <= 1.0, (what, es, rel_s)
            ridx, _ = select32(logits, s, bias, n_group, topk_group, group_top, k)
            assert torch.equal(idx.long(), ridx), what
            ew, rel_w = value_error(w, weights64(s64, idx, scoring, renormalize, scale), scale)
            assert ew <= 1.0, (what, ew, rel_w)
            worst_w, worst_s = max(worst_w, rel_w), max(worst_s, rel_s)
            if not renormalize and scale == 1.0:             # the bits of scores at the chosen ids
                assert torch.equal(w, s.gather(1, idx.long())), what
            w2, idx2 = ops.router_score_topk(logits, k, scoring, bias, n_group, topk_group, group_top, renormalize, scale)
            assert torch.equal(idx2, idx) and same_bits(w2, w), what      # scores or not: the same weights
        if scoring == "sigmoid" and T >= 3:                  # saturation is exact
            assert float(s[1, (E - 1) // 2]) == 1.0 and float(s[2, 1 % E]) == 1.0
            if E > 1:
                assert float(s[2, E - 1]) == 0.0 and float(s[1, E - 1]) > 0.0
    print(f"router_score forward {IDS[dtype]} {scoring}: max rel err weights {worst_w:.3e} scores {worst_s:.3e} "
          f"(bound {REL:.0e})")


@pytest.mark.parametrize("scoring", SCORINGS)
def test_ties_go_to_the_lower_group_then_the_lower_id(ops, scoring):
    for (E, n_group, topk_group, k), T, group_top, bias_value in itertools.product(CONFIGS, (1, 257), (1, 2), (None, 0.25)):
        zeros = torch.zeros(T, E, device="cuda")
        bias = None if bias_value is None else torch.full((E,), bias_value, device="cuda")
        w, idx = ops.router_score_topk(zeros, k, scoring, bias, n_group, topk_group, group_top)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device="cuda").expand(T, k)), (E, n_group, k, group_top)
        assert float((w.double() - 1.0 / k).abs().max()) <= REL / k
    g = torch.Generator().manual_seed(3)
    for (E, n_group, topk_group, k), group_top in itertools.product(CONFIGS, (1, 2)):
        ints = torch.randint(-1, 2, (257, E), generator=g).float().cuda()         # many ties, -0.0 among them
        ints[0, 0] = -0.0
        bias = (torch.randint(-1, 2, (E,), generator=g).float() * 0.5).cuda()
        for b in (None, bias):
            w, idx, s = ops.router_score_topk(ints, k, scoring, b, n_group, topk_group, group_top, return_scores=True)
            assert torch.equal(idx.long(), select32(ints, s, b, n_group, topk_group, group_top, k)[0]), (E, n_group, k)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_masked_experts_are_never_selected(ops, scoring):
    """Every bias -10: all keys are negative, where a 0.0 fill of the masked experts would let them win."""
    for (E, n_group, topk_group, k), group_top in itertools.product(CONFIGS, (1, 2)):
        logits = make_logits(257, E, torch.float32, special=False)
        bias = torch.full((E,), -10.0, device="cuda")
        w, idx, s = ops.router_score_topk(logits, k, scoring, bias, n_group, topk_group, group_top, return_scores=True)
        assert bool(((s + bias) < 0).all())
        ridx, chosen = select32(logits, s, bias, n_group, topk_group, group_top, k)
        assert torch.equal(idx.long(), ridx), (E, n_group, k, group_top)
        if n_group > 1:
            assert bool((chosen.sum(dim=1) == topk_group).all())
            assert bool(chosen.gather(1, idx.long() // (E // n_group)).all()), (E, n_group, k, group_top)
        assert bool((idx.long().sort(dim=1).values.diff(dim=1) > 0).all()) or k == 1      # no expert twice


# ----------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_defaults_are_the_bits_of_router_topk(ops, dtype):
    for (E, _, _, k), T, renormalize in itertools.product(CONFIGS, TOKENS, (True, False)):
        logits = make_logits(T, E, dtype)
        w0, i0, p0 = ops.router_topk(logits, k, renormalize=renormalize, return_probs=True)
        w1, i1, p1 = ops.router_score_topk(logits, k, renormalize=renormalize, return_scores=True)
        assert torch.equal(i0, i1) and same_bits(w0, w1) and same_bits(p0, p1), (T, E, k, renormalize)
        # every group allowed and the key still the logit: the same rule through the scored kernel variant
        d = next((n for n in range(2, 9) if E % n == 0), 1)           # (E = 1 has no such divisor: one group)
        w2, i2, p2 = ops.router_score_topk(logits, k, n_group=d, topk_group=d, renormalize=renormalize, return_scores=True)
        assert torch.equal(i0, i2) and same_bits(w0, w2) and same_bits(p0, p2), (T, E, k, renormalize, d)
        g = torch.Generator().manual_seed(T + E)
        gw, gp = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
        for a, b in ((gw, gp), (gw, None), (None, gp)):
            d0 = ops.router_topk_backward(logits, i0, a, b, renormalize=renormalize)
            d1 = ops.router_score_topk_backward(logits, i1, a, b, "softmax", renormalize, 1.0)
            d2 = ops.router_score_topk_backward(logits, i2, a, b, "softmax", renormalize, 1.0)
            assert same_bits(d0, d1) and same_bits(d0, d2), (T, E, k, renormalize)


# ----------------------------------------------------------------------------------------------------------- backward
def grad_reference(logits, idx, gw, gs, scoring, renormalize, scale):
    l = logits.double().detach().requires_grad_(True)
    s = scores64(l, scoring)
    loss = l.sum() * 0.0
    if gw is not None:
        loss = loss + (weights64(s, idx, scoring, renormalize, scale) * gw.double()).sum()
    if gs is not None:
        loss = loss + (s * gs.double()).sum()
    return torch.autograd.grad(loss, l)[0]


@pytest.mark.parametrize("which", ["weights", "weights+scores", "scores"])
@pytest.mark.parametrize("scoring", SCORINGS)
def test_backward_matches_float64(ops, scoring, which):
    worst = 0.0
    for (E, n_group, topk_group, k), T in itertools.product(CONFIGS, (1, 257)):
        logits = make_logits(T, E, torch.float32)
        g = torch.Generator().manual_seed(5 + T + E + k)
        gw = torch.randn(T, k, generator=g).cuda() if "weights" in which else None
        gs = torch.randn(T, E, generator=g).cuda() if "scores" in which else None
        for group_top, with_bias, renormalize, scale in settings():
            if group_top == 1 and n_group == 1:
                continue                                     # (the same call as group_top == 2)
            bias = make_bias(E) if with_bias else None
            what = (T, E, n_group, k, group_top, with_bias, renormalize, scale)
            x = logits.clone().requires_grad_(True)
            out = ops.router_score_topk(x, k, scoring, bias, n_group, topk_group, group_top, renormalize, scale,
                                        return_scores=gs is not None)
            assert not out[1].requires_grad and out[0].requires_grad
            loss = (out[0] * gw).sum() if gw is not None else 0.0
            if gs is not None:
                loss = loss + (out[2] * gs).sum()
            got, = torch.autograd.grad(loss, x)
            assert got.dtype == torch.float32 and got.shape == (T, E)
            direct = ops.router_score_topk_backward(logits, out[1], gw, gs, scoring, renormalize, scale)
            assert same_bits(got, direct), what              # autograd hands over exactly the gradients that exist
            ref = grad_reference(logits, out[1], gw, gs, scoring, renormalize, scale)
            size = (abs(scale) * gw.abs().amax(dim=1) if gw is not None else 0.0) + \
                (gs.abs().amax(dim=1) if gs is not None else 0.0)
            err = float(((got.double() - ref).abs().amax(dim=1) / size.double()).max())
            worst = max(worst, err)
            assert err <= GRAD_REL, (what, err)
            if gs is None and (scoring == "sigmoid" or renormalize):          # an expert no slot names: exactly 0.0
                named = torch.zeros(T, E, dtype=torch.bool, device="cuda").scatter_(1, out[1].long(), True)
                assert torch.equal(bits(got)[~named], torch.zeros_like(bits(got)[~named])), what
    print(f"router_score backward {scoring} {which}: max row err / (|scale| max|g_w| + max|g_s|) {worst:.3e} "
          f"(bound {GRAD_REL:.0e})")


@pytest.mark.parametrize("scoring", SCORINGS)
def test_backward_without_gradients_is_zero(ops, scoring):
    logits = make_logits(257, 60, torch.float32)
    _, idx = ops.router_score_topk(logits, 8, scoring, make_bias(60), 4, 2)
    got = ops.router_score_topk_backward(logits, idx, None, None, scoring, True, 2.5)
    assert torch.equal(bits(got), torch.zeros_like(bits(got)))


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=IDS.get)
def test_backward_16bit_is_the_float32_result_rounded_once(ops, dtype, scoring):
    for (E, n_group, topk_group, k), T, renormalize in itertools.product(CONFIGS, (3, 257), (True, False)):
        logits = make_logits(T, E, dtype)
        g = torch.Generator().manual_seed(T + E)
        gw, gs = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
        bias = make_bias(E)
        _, idx = ops.router_score_topk(logits, k, scoring, bias, n_group, topk_group, 2, renormalize, 2.5)
        got = ops.router_score_topk_backward(logits, idx, gw, gs, scoring, renormalize, 2.5)
        wide = ops.router_score_topk_backward(logits.float(), idx, gw, gs, scoring, renormalize, 2.5)
        assert got.dtype == dtype and same_bits(got, wide.to(dtype)), (T, E, k, renormalize)
        x = logits.clone().requires_grad_(True)              # through autograd: the gradient has the logits' type
        w, _ = ops.router_score_topk(x, k, scoring, bias, n_group, topk_group, 2, renormalize, 2.5)
        (w * gw).sum().backward()
        assert x.grad.dtype == dtype
        assert same_bits(x.grad, ops.router_score_topk_backward(logits.float(), idx, gw, None, scoring, renormalize,
                                                                2.5).to(dtype))


# ------------------------------------------------------------------------------- row independence and repeatability
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("config", [(60, 4, 2, 8), (128, 8, 4, 8), (96, 3, 1, 4), (8, 4, 1, 2), (5, 1, 1, 2)],
                         ids=lambda c: "E%d-g%d-%d-k%d" % c)
def test_rows_are_independent_and_calls_repeat(ops, config, dtype, scoring):
    E, n_group, topk_group, k = config
    T = 257
    logits, bias = make_logits(T, E, dtype), make_bias(E)
    g = torch.Generator().manual_seed(E)
    gw, gs = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
    for renormalize in (True, False):
        def fwd(l):
            return ops.router_score_topk(l, k, scoring, bias, n_group, topk_group, 2, renormalize, 2.5, return_scores=True)

        def bwd(l, i, a, b):
            return ops.router_score_topk_backward(l, i, a, b, scoring, renormalize, 2.5)

        w, idx, s = fwd(logits)
        d = bwd(logits, idx, gw, gs)
        w2, idx2, s2 = fwd(logits)
        assert torch.equal(idx, idx2) and same_bits(w, w2) and same_bits(s, s2) and same_bits(d, bwd(logits, idx, gw, gs))
        for t in (0, 1, 2, 7, 63, 64, 100, 255, 256):
            w1, idx1, s1 = fwd(logits[t:t + 1])
            d1 = bwd(logits[t:t + 1], idx1, gw[t:t + 1], gs[t:t + 1])
            assert torch.equal(idx1, idx[t:t + 1]) and same_bits(w1, w[t:t + 1]) and same_bits(s1, s[t:t + 1]), (t, renormalize)
            assert same_bits(d1, d[t:t + 1]), (t, renormalize)


# ---------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("config", [(8, 4, 1, 2), (60, 4, 2, 8), (128, 8, 4, 8), (5, 1, 1, 2)], ids=lambda c: "E%d-g%d-%d-k%d" % c)
def test_non_finite_rows(ops, config, dtype, scoring):
    E, n_group, topk_group, k = config
    T = 19
    clean = make_logits(T, E, dtype, seed=9)
    dirty = clean.clone()
    bad = {1: NAN, 4: float("inf"), 10: float("-inf"), 18: NAN}
    for t, v in bad.items():
        dirty[t, (3 * t) % E] = v
    rows = torch.tensor(sorted(bad), device="cuda")
    good = torch.tensor([t for t in range(T) if t not in bad], device="cuda")
    g = torch.Generator().manual_seed(2)
    gw, gs = torch.randn(T, k, generator=g).cuda(), torch.randn(T, E, generator=g).cuda()
    for renormalize, bias in itertools.product((True, False), (None, make_bias(E))):
        def fwd(l):
            return ops.router_score_topk(l, k, scoring, bias, n_group, topk_group, 2, renormalize, 2.5, return_scores=True)

        w, idx, s = fwd(dirty)
        wc, idxc, sc = fwd(clean)
        assert torch.isnan(w[rows]).all() and torch.isnan(s[rows]).all()
        assert torch.equal(idx[rows], torch.arange(k, dtype=torch.int32, device="cuda").expand(len(bad), k))
        assert bool(((idx >= 0) & (idx < E)).all())
        assert torch.equal(idx[good], idxc[good]) and same_bits(w[good], wc[good]) and same_bits(s[good], sc[good])
        d = ops.router_score_topk_backward(dirty, idx, gw, gs, scoring, renormalize, 2.5)
        dc = ops.router_score_topk_backward(clean, idxc, gw, gs, scoring, renormalize, 2.5)
        assert torch.isnan(d[rows]).all() and same_bits(d[good], dc[good])
        assert torch.isnan(ops.router_score_topk_backward(dirty, idx, None, None, scoring, renormalize, 2.5)[rows]).all()
    wild = torch.tensor([NAN, float("inf"), float("-inf")], device="cuda").repeat(E)[:E]      # the caller's error: ids stay valid
    _, idx = ops.router_score_topk(clean, k, scoring, wild, n_group, topk_group, 2)
    assert bool(((idx >= 0) & (idx < E)).all())


# ----------------------------------------------------------------------------------------------------------- footprint
def out_buffer(name, n, dtype):
    esz = torch.empty((), dtype=dtype).element_size()
    g = Guarded(name, n * esz, dtype, BIG if dtype == torch.int32 else SENT, offset=esz)
    g.view(dtype, n).fill_(-99 if dtype == torch.int32 else SENT)
    return g


FOOT = [(60, 4, 2, 8), (128, 8, 4, 8)]


@pytest.mark.parametrize("with_scores", [True, False], ids=["scores", "null_scores"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("config", FOOT, ids=lambda c: "E%d" % c[0])
def test_forward_footprint(ops, lib, config, dtype, with_scores):
    E, n_group, topk_group, k = config
    T = 257
    logits, bias = make_logits(T, E, dtype), make_bias(E)
    gl, gb = guarded_like("logits", logits, NAN), guarded_like("select_bias", bias, NAN)
    gi, gw, gs = out_buffer("indices", T * k, torch.int32), out_buffer("weights", T * k, torch.float32), out_buffer("scores", T * E, torch.float32)
    rc = lib.fql_router_score_topk_fwd(gl.ptr, DT[dtype], T, E, k, 1, gb.ptr, n_group, topk_group, 2, 1, 2.5, gi.ptr, gw.ptr,
                                       gs.ptr if with_scores else None, stream())
    assert rc == 0, rc
    assert_guards_intact(gl, gb, gi, gw, gs, what=f"fql_router_score_topk_fwd {IDS[dtype]} E={E} scores={with_scores}")
    w, idx, s = ops.router_score_topk(logits, k, "sigmoid", bias, n_group, topk_group, 2, True, 2.5, return_scores=True)
    assert torch.equal(gi.view(torch.int32, T, k), idx) and same_bits(gw.view(torch.float32, T, k), w)
    if with_scores:
        assert same_bits(gs.view(torch.float32, T, E), s)
    else:                                                    # nothing beyond weights / indices is written
        assert bool((gs.view(torch.float32, T * E) == SENT).all())
    assert same_bits(gl.view(dtype, T, E), logits) and same_bits(gb.view(torch.float32, E), bias)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("config", FOOT, ids=lambda c: "E%d" % c[0])
def test_backward_footprint(ops, lib, config, dtype):
    E, n_group, topk_group, k = config
    T = 257
    logits = make_logits(T, E, dtype)
    g = torch.Generator().manual_seed(4)
    gw, gp = torch.randn(T, k, generator=g), torch.randn(T, E, generator=g)
    _, idx = ops.router_score_topk(logits, k, "sigmoid", make_bias(E), n_group, topk_group)
    ins = [guarded_like("logits", logits, NAN), guarded_like("indices", idx, BIG), guarded_like("grad_weights", gw, NAN),
           guarded_like("grad_scores", gp, NAN)]
    out = out_buffer("grad_logits", T * E, dtype)
    rc = lib.fql_router_score_topk_bwd(ins[0].ptr, DT[dtype], ins[1].ptr, ins[2].ptr, ins[3].ptr, out.ptr, T, E, k, 1, 1, 2.5,
                                       stream())
    assert rc == 0, rc
    assert_guards_intact(*ins, out, what=f"fql_router_score_topk_bwd {IDS[dtype]} E={E}")
    assert same_bits(out.view(dtype, T, E), ops.router_score_topk_backward(logits, idx, gw.cuda(), gp.cuda(), "sigmoid", True, 2.5))


# ----------------------------------------------------------------------------------------------------------- refusals
def _good():
    return make_logits(3, 8, torch.float32)


def _bias(n=8, **kw):
    return torch.zeros(n, device="cuda", **kw)


REFUSALS = [
    ("cpu-logits", lambda: (_good().cpu(), 2, {})),
    ("int-logits", lambda: (_good().to(torch.int32), 2, {})),
    ("float64-logits", lambda: (_good().double(), 2, {})),
    ("1-d-logits", lambda: (_good()[0], 2, {})),
    ("129-experts", lambda: (torch.zeros(3, 129, device="cuda"), 2, {})),
    ("no-experts", lambda: (torch.zeros(3, 0, device="cuda"), 1, {})),
    ("top_k-0", lambda: (_good(), 0, {})),
    ("top_k-past-E", lambda: (make_logits(3, 5, torch.float32), 6, {})),
    ("top_k-9", lambda: (make_logits(3, 64, torch.float32), 9, {})),
    ("top_k-float", lambda: (_good(), 2.0, {})),
    ("cpu-bias", lambda: (_good(), 2, dict(select_bias=torch.zeros(8)))),
    ("bias-shape", lambda: (_good(), 2, dict(select_bias=_bias(7)))),
    ("bias-2-d", lambda: (_good(), 2, dict(select_bias=_bias(8).view(1, 8)))),
    ("bias-float16", lambda: (_good(), 2, dict(select_bias=_bias(8, dtype=torch.float16)))),
    ("bias-float64", lambda: (_good(), 2, dict(select_bias=_bias(8, dtype=torch.float64)))),
    ("n_group-0", lambda: (_good(), 2, dict(n_group=0))),
    ("n_group-3", lambda: (_good(), 2, dict(n_group=3, topk_group=1))),
    ("n_group-16", lambda: (make_logits(3, 64, torch.float32), 2, dict(n_group=16, topk_group=16))),
    ("n_group-float", lambda: (_good(), 2, dict(n_group=2.0, topk_group=1))),
    ("topk_group-0", lambda: (_good(), 2, dict(n_group=4, topk_group=0))),
    ("topk_group-past-n_group", lambda: (_good(), 2, dict(n_group=4, topk_group=5))),
    ("groups-hold-fewer-than-top_k", lambda: (_good(), 4, dict(n_group=4, topk_group=1))),
    ("group_top-0", lambda: (_good(), 2, dict(group_top=0))),
    ("group_top-3", lambda: (_good(), 2, dict(group_top=3))),
    ("scale-inf", lambda: (_good(), 2, dict(scale=float("inf")))),
    ("scale-nan", lambda: (_good(), 2, dict(scale=NAN))),
]


@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=lambda i: REFUSALS[i][0])
def test_refusals(ops, row):
    logits, k, kwargs = REFUSALS[row][1]()
    with pytest.raises(RuntimeError):
        ops.router_score_topk(logits, k, "sigmoid", **kwargs)
    if logits.dtype.is_floating_point and logits.dtype != torch.float64:
        with pytest.raises(RuntimeError):
            ops.router_score_topk(logits.clone().requires_grad_(True), k, "sigmoid", **kwargs)


def test_unknown_scoring_and_backward_refusals(ops):
    with pytest.raises(ValueError):
        ops.router_score_topk(_good(), 2, "tanh")
    _, idx = ops.router_score_topk(_good(), 2, "sigmoid")
    gw = torch.ones(3, 2, device="cuda")
    for args in [(_good().cpu(), idx, gw, None), (_good(), idx.cpu(), gw, None), (_good(), idx, gw.cpu(), None),
                 (_good(), idx, gw[:, :1], None), (_good(), idx, gw, torch.ones(3, 7, device="cuda")),
                 (_good(), idx[:2], gw, None)]:
        with pytest.raises(RuntimeError):
            ops.router_score_topk_backward(*args, scoring="sigmoid")
    with pytest.raises(RuntimeError):
        ops.router_score_topk_backward(_good(), idx, gw, None, scoring="sigmoid", scale=NAN)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_non_contiguous_logits_and_bias_are_accepted(ops, dtype):
    wide = make_logits(257, 128, dtype)
    view = wide[:, 3:63:1][:, ::2]                           # [257, 30], strides (128, 2)
    bias = make_bias(60)[::2]
    assert not view.is_contiguous() and not bias.is_contiguous()
    a = ops.router_score_topk(view, 4, "sigmoid", bias, 3, 2, return_scores=True)
    b = ops.router_score_topk(view.contiguous(), 4, "sigmoid", bias.contiguous(), 3, 2, return_scores=True)
    assert torch.equal(a[1], b[1]) and same_bits(a[0], b[0]) and same_bits(a[2], b[2])


def test_empty_batch(ops):
    w, idx, s = ops.router_score_topk(torch.zeros(0, 8, device="cuda"), 2, "sigmoid", _bias(8), 4, 2, return_scores=True)
    assert w.shape == (0, 2) and idx.shape == (0, 2) and s.shape == (0, 8)
