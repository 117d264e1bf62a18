"""QuantizedSparseMoEBlock with ``capacity_factor`` and ``forward(x, token_mask)`` on the GPU.

E = 8, H = 64, F = 96, T in (1, 64, 130), top_k in (1, 2), capacity_factor in (0.5, 1.0); masks: random (three tokens in
four real) and a masked prefix of ten tokens.  At 0.5 the capacity is ceil(T * top_k / 16): with at least 33 (T = 64) or
73 (T = 130) real tokens some expert must overflow, which ``problem`` asserts of its own masks; T = 1 cannot overflow and
is the case where the capacity is 1 and nothing drops.

  * plumbing:  the block's output and ``router_logits`` equal, bit for bit, the same public ops composed by hand
               (``ops.router_score_topk``, ``ops.route_plan_capped``, ``ops.dispatch_rows`` / ``ops.combine_any`` with
               ``skip_dropped``), for float32 and bfloat16, LoRA experts, a gated shared expert, and the clamped SwiGLU
               with expert biases; so are x.grad and every parameter gradient.
  * no-op:     a capacity_factor of E (capacity T * top_k) plus an all-true mask gives the bits of the block built
               without the feature, output and every gradient.
  * meaning:   against a dense torch reference with a float64 router that applies the same drops (the restatement of
               tests/test_route_capped_cpu.py), the bounds of tests/test_gpu_sparse_moe_block.py: forward
               ``||out - ref||_F <= 4e-6 * || sum_k |w_k| |y_k| ||_F`` over the kept slots (one ulp per element added on
               16-bit activations), gradients within 4x the error the same reference shows with a float32 router.
Each test prints its measured figures before it asserts."""
import functools
import math

import pytest
import torch

from helpers import fq, ops, rel_fro_dev
from test_route_capped_cpu import plan_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
E, H, F, FS, RANK = 8, 64, 96, 64, 8
REL = 4e-6
MANT = {torch.float16: 10, torch.bfloat16: 7}
TS, KS, FACTORS, MASKS = (1, 64, 130), (1, 2), (0.5, 1.0), ("random", "prefix")
KINDS = ("plain", "lora", "shared", "bias")
PLUMBING = [("plain", torch.float32), ("plain", torch.bfloat16), ("lora", torch.float32), ("lora", torch.bfloat16),
            ("shared", torch.float32), ("shared", torch.bfloat16), ("bias", torch.float32), ("bias", torch.bfloat16)]
IDS = [f"{k}-{'f32' if d == torch.float32 else 'bf16'}" for k, d in PLUMBING]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def raw():
    g = torch.Generator().manual_seed(41)
    r = lambda *shape, s=0.1: torch.randn(*shape, generator=g) * s
    return dict(gate_w=r(E, H, s=0.5), gate=[r(F, H) for _ in range(E)], up=[r(F, H) for _ in range(E)],
                down=[r(H, F) for _ in range(E)], shared=(r(FS, H), r(FS, H), r(H, FS)), shared_gate=r(1, H, s=0.5),
                gb=[r(F, s=0.3) for _ in range(E)], ub=[r(F, s=0.3) for _ in range(E)], db=[r(H, s=0.3) for _ in range(E)])


def build(kind, dtype, top_k, capacity_factor=None, **routing):
    """A block of one of the four kinds; two calls with the same arguments give the same parameters."""
    w = raw()
    adt = None if dtype == torch.float32 else dtype
    kw = dict(top_k=top_k, activation_dtype=adt, renormalize=top_k > 1, capacity_factor=capacity_factor, **routing)
    if kind == "shared":
        kw.update(shared=w["shared"], shared_expert_gate_weight=w["shared_gate"])
    if kind == "bias":
        kw.update(activation="swiglu_clamp", gate_bias=w["gb"], up_bias=w["ub"], down_bias=w["db"])
    m = fq().QuantizedSparseMoEBlock.from_weights(w["gate_w"], w["gate"], w["up"], w["down"], **kw).to(DEV)
    if kind == "bias":
        m.experts.gate_up_bias.requires_grad_(True)
        m.experts.down_bias.requires_grad_(True)
    if kind == "lora":
        experts = fq().LoRAQuantizedMoEFFN.from_quantized(m.experts, RANK, alpha=2 * RANK)
        g = torch.Generator(device=DEV).manual_seed(3)
        with torch.no_grad():
            experts.gate_up_lora_A.normal_(0, 0.1, generator=g)
            experts.gate_up_lora_B.normal_(0, 0.1, generator=g)
            experts.down_lora_A.normal_(0, 0.1, generator=g)
            experts.down_lora_B.normal_(0, 0.1, generator=g)
        gate_w = m.gate.weight.detach().clone()
        m = fq().QuantizedSparseMoEBlock(E, H, F, top_k=top_k, activation_dtype=experts.activation_dtype,
                                         renormalize=top_k > 1, experts=experts, capacity_factor=capacity_factor).to(DEV)
        with torch.no_grad():
            m.gate.weight.copy_(gate_w)
    return m


def trainable(m):
    return {n: p for n, p in m.named_parameters() if p.requires_grad}


@functools.lru_cache(maxsize=None)
def problem(T, dtype, mask_kind):
    g = torch.Generator().manual_seed(7 * T + (1 if mask_kind == "random" else 2))
    x = torch.randn(T, H, generator=g).to(dtype).to(DEV)
    gy = torch.randn(T, H, generator=g).to(dtype).to(DEV)
    if mask_kind == "random":
        mask = torch.rand(T, generator=g) < 0.75
    else:
        mask = torch.arange(T) >= 10
    if T == 1:
        mask[:] = True                                           # (a single masked token is the all-false case of the plan test)
    real = int(mask.sum())
    assert real >= {1: 1, 64: 33, 130: 73}[T] and (T == 1 or real < T)           # the test's own input: see the docstring
    return x, gy, mask.to(DEV)


def compose(m, x, mask, keep_weights=None):
    """The capped forward from the public ops, by hand."""
    o = ops()
    x2 = x.reshape(-1, H)
    # (the two gates read the tokens through one alias, as in the block: autograd then adds x.grad up in the same order)
    x_gate = x2.view_as(x2) if getattr(m, "shared_expert_gate", None) is not None else x2
    logits = m.router_logits(x_gate)
    weights, indices = o.router_score_topk(logits, m.top_k, m.scoring, m.selection_bias, m.n_group, m.topk_group,
                                           m.group_top, m.renormalize, m.routed_scaling_factor)[:2]
    if keep_weights is not None:
        weights.retain_grad()
        keep_weights.append(weights)
    capacity = None if m.capacity_factor is None else max(1, math.ceil(m.capacity_factor * x2.shape[0] * m.top_k / E))
    tpe, offs, token_of_sorted, pos_of_slot, demand = o.route_plan_capped(indices, E, capacity, mask)
    rows = o.dispatch_rows(x2, token_of_sorted, pos_of_slot, m.top_k, skip_dropped=True)
    y = m.experts(rows, tpe, offs)
    s, aw = m.shared_output(x2, x_gate)
    out = o.combine_any(y, pos_of_slot, weights, addend=s, addend_weight=aw, out_dtype=x.dtype, skip_dropped=True)
    return out.reshape(x.shape), logits, (tpe, demand, pos_of_slot)


def grads_of(run, m, x, gy):
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    out, logits = run(xg)[:2]
    out.backward(gy)
    got = {n: (None if p.grad is None else p.grad.clone()) for n, p in trainable(m).items()}
    return out.detach(), logits.detach(), xg.grad.clone(), got


# ----------------------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("kind,dtype", PLUMBING, ids=IDS)
def test_block_is_the_public_ops_composed_by_hand(kind, dtype):
    checked = dropped_cases = 0
    for top_k, factor in [(k, f) for k in KS for f in FACTORS]:
        m = build(kind, dtype, top_k, factor)
        for T, mask_kind in [(t, mk) for t in TS for mk in MASKS]:
            x, gy, mask = problem(T, dtype, mask_kind)
            what = (top_k, factor, T, mask_kind)
            with torch.no_grad():
                out, logits = m(x, token_mask=mask)
                demand, kept = m.routing[1].clone(), m.kept_per_expert.clone()
                ref, ref_logits, (tpe, ref_demand, _) = compose(m, x, mask)
            assert out.shape == x.shape and out.dtype == dtype and logits.shape == (T, E)
            assert same_bits(out, ref) and same_bits(logits, ref_logits), what
            assert torch.equal(kept, tpe) and torch.equal(demand, ref_demand) and bool((kept <= demand).all()), what
            assert int(demand.sum()) == int(mask.sum()) * top_k, what
            assert int(kept.max()) <= m.expert_capacity(T), what
            if factor == 0.5 and T > 1:
                assert bool((kept < demand).any()), what          # 0.5 must drop something
                dropped_cases += 1
            # [..., H] in, [..., H] out, the mask in the same leading shape
            out3, _ = m(x.reshape(1, T, H), token_mask=mask.reshape(1, T))
            assert same_bits(out3.detach().reshape(T, H), out), what
            # under autograd: the same bits forward, and every gradient that of the composition
            o1, l1, gx1, gp1 = grads_of(lambda t: m(t, token_mask=mask), m, x, gy)
            o2, l2, gx2, gp2 = grads_of(lambda t: compose(m, t, mask), m, x, gy)
            assert same_bits(o1, out) and same_bits(o1, o2) and same_bits(l1, l2) and same_bits(gx1, gx2), what
            assert set(gp1) == set(gp2) and len(gp1) >= 1
            for n in gp1:
                assert gp1[n] is not None and same_bits(gp1[n], gp2[n]), (what, n)
                assert bool(torch.isfinite(gp1[n]).all()), (what, n)
            checked += 1
    print(f"capped block {kind} {dtype}: {checked} cases bit-identical to the composition, {dropped_cases} with drops")
    assert dropped_cases == 2 * 2 * 2


# -------------------------------------------------------------------------------------------------------------- no-op
@pytest.mark.parametrize("kind,dtype", PLUMBING, ids=IDS)
def test_nothing_dropped_and_nothing_masked_is_the_block_without_the_feature(kind, dtype):
    for top_k in KS:
        plain, capped = build(kind, dtype, top_k), build(kind, dtype, top_k, float(E))
        assert plain.capacity_factor is None and list(plain.state_dict()) == list(capped.state_dict())
        for T in TS:
            x, gy, _ = problem(T, dtype, "random")
            mask = torch.ones(T, dtype=torch.bool, device=DEV)
            o0, l0, gx0, gp0 = grads_of(lambda t: plain(t), plain, x, gy)
            o1, l1, gx1, gp1 = grads_of(lambda t: capped(t, token_mask=mask), capped, x, gy)
            assert capped.expert_capacity(T) == T * top_k
            assert torch.equal(capped.kept_per_expert, capped.routing[1]) and torch.equal(plain.routing[1], capped.routing[1])
            assert torch.equal(plain.kept_per_expert, plain.routing[1])
            assert same_bits(o0, o1) and same_bits(l0, l1) and same_bits(gx0, gx1), (top_k, T)
            assert set(gp0) == set(gp1)
            for n in gp0:
                assert same_bits(gp0[n], gp1[n]), (top_k, T, n)
            if kind == "lora":
                assert {"experts.gate_up_lora_A", "experts.gate_up_lora_B", "experts.down_lora_A",
                        "experts.down_lora_B", "gate.weight"} <= set(gp0)
            if kind == "bias":
                assert {"experts.gate_up_bias", "experts.down_bias"} <= set(gp0)


# ------------------------------------------------------------------------------------------------------------ meaning
def torch_router(logits, top_k, renormalize, router_dtype):
    l = logits.to(router_dtype)
    idx = torch.sort(-l.detach(), dim=-1, stable=True).indices[:, :top_k]
    p = torch.softmax(l, dim=-1)
    sel = p.gather(1, idx)
    w = sel / sel.sum(dim=-1, keepdim=True) if renormalize else sel
    return w.to(torch.float32), idx


def dense_reference(m, x, mask, router_dtype=torch.float64):
    """(out float64, indices, kept [T, top_k], envelope): a torch router of ``router_dtype``, the drops of the
    restatement, the rows of the kept slots through the SAME expert module in expert order, and a dense float64 sum
    ``sum_k keep * w_k * y_k`` plus the shared term."""
    T = x.shape[0]
    x2 = x.reshape(-1, H)
    w, idx = torch_router(m.router_logits(x2), m.top_k, m.renormalize, router_dtype)
    counts, offsets, token_of_sorted, pos, _ = plan_reference(idx, E, m.expert_capacity(T), mask)
    keep = (pos >= 0).view(T, m.top_k)
    rows = x2[token_of_sorted.long()]                            # torch's own gather (and index_add in its backward)
    y = m.experts(rows, counts, offsets)
    yk = y.double()[pos.clamp(min=0).long()].view(T, m.top_k, H)
    terms = w.double().unsqueeze(-1) * keep.unsqueeze(-1) * yk
    out = terms.sum(dim=1)
    s, aw = m.shared_output(x2)
    if s is not None:
        out = out + s.double() * (1.0 if aw is None else aw.double().unsqueeze(-1))
    return out, idx, keep, terms.detach().abs().sum(dim=1)


def ulp_of(ref, dtype):
    a = ref.double().abs().clamp_min(2.0 ** -24)
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


@pytest.mark.parametrize("kind,dtype", [("plain", torch.float32), ("plain", torch.bfloat16), ("shared", torch.float32)],
                         ids=["plain-f32", "plain-bf16", "shared-f32"])
def test_forward_against_the_dense_reference(kind, dtype):
    for top_k, factor in [(k, f) for k in KS for f in FACTORS]:
        m = build(kind, dtype, top_k, factor)
        for T, mask_kind in [(t, mk) for t in TS for mk in MASKS]:
            x, _, mask = problem(T, dtype, mask_kind)
            with torch.no_grad():
                out, logits = m(x, token_mask=mask)
                ref, idx, keep, envelope = dense_reference(m, x, mask)
                _, got_idx = ops().router_topk(logits, top_k, m.renormalize)
                assert torch.equal(got_idx.long(), idx)
                bound = REL * float(torch.linalg.vector_norm(envelope))
                if dtype != torch.float32:
                    bound += float(torch.linalg.vector_norm(ulp_of(ref, dtype)))
                err = float(torch.linalg.vector_norm(out.double() - ref))
                print(f"capped forward {kind} {dtype} top_k={top_k} cf={factor} T={T} {mask_kind}: ||out - ref||_F "
                      f"{err:.3e}, bound {bound:.3e}, {int((~keep).sum())} of {keep.numel()} slots without a row")
                assert err <= bound
                # a masked token's output is its shared term exactly: zero without a shared expert
                s, aw = m.shared_output(x)
                if s is None:
                    assert not out[~mask].any()
                else:
                    term = (s.float() * aw.unsqueeze(-1)).to(dtype)
                    assert torch.equal(out[~mask], term[~mask])
                # ... and so is that of a token that lost every slot to the capacity
                lost = mask & ~keep.any(dim=1)
                if s is None:
                    assert not out[lost].any()


@pytest.mark.parametrize("kind", ["plain", "shared"])
def test_gradients_against_the_dense_reference(kind):
    dtype = torch.float32
    for top_k, factor in [(2, 0.5), (2, 1.0), (1, 0.5)]:
        m = build(kind, dtype, top_k, factor)                    # (top-1 is built un-renormalised: its gate has a gradient)
        for T, mask_kind in [(64, "random"), (130, "prefix")]:
            x, gy, mask = problem(T, dtype, mask_kind)

            def ref_grads(router_dtype):
                m.zero_grad(set_to_none=True)
                xg = x.clone().requires_grad_(True)
                dense_reference(m, xg, mask, router_dtype)[0].backward(gy.double())
                return xg.grad.clone(), m.gate.weight.grad.clone()

            gx64, gg64 = ref_grads(torch.float64)
            gx32, gg32 = ref_grads(torch.float32)
            _, _, gx, gp = grads_of(lambda t: m(t, token_mask=mask), m, x, gy)
            gg = gp["gate.weight"]
            ex32, eg32 = rel_fro_dev(gx32, gx64), rel_fro_dev(gg32, gg64)
            ex, eg = rel_fro_dev(gx, gx64), rel_fro_dev(gg, gg64)
            print(f"capped gradients {kind} top_k={top_k} cf={factor} T={T} {mask_kind}: x.grad rel err {ex:.3e} (float32 "
                  f"torch router {ex32:.3e}, bound {4 * ex32:.3e}); gate.weight.grad {eg:.3e} (float32 torch router "
                  f"{eg32:.3e}, bound {4 * eg32:.3e})")
            assert float(torch.linalg.vector_norm(gg64.double())) > 0
            assert ex <= 4 * ex32
            assert eg <= 4 * eg32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_masked_tokens_and_dropped_slots_send_nothing_back(dtype):
    top_k, T = 2, 64
    x, gy, mask = problem(T, dtype, "random")
    # without a shared expert a masked token's x.grad is exactly zero: no routed part, and nothing through the gate
    m = build("plain", dtype, top_k, 0.5)
    seen = {}
    xg = x.clone().requires_grad_(True)
    out, logits = m(xg, token_mask=mask)
    logits.register_hook(lambda g: seen.__setitem__("dlogits", g.detach().clone()))
    out.backward(gy)
    assert not xg.grad[~mask].any() and bool(xg.grad[mask].any())
    assert not seen["dlogits"][~mask].any() and bool(seen["dlogits"][mask].any())      # the gate sees no masked token
    # the routing weight of a dropped or masked slot gets a zero gradient (the composition has the block's bits)
    kept_w = []
    m.zero_grad(set_to_none=True)
    out2, _, (tpe, demand, pos) = compose(m, x.clone().requires_grad_(True), mask, keep_weights=kept_w)
    assert same_bits(out2.detach(), out.detach())
    out2.backward(gy)
    gw, keep = kept_w[0].grad, (pos >= 0).view(T, top_k)
    assert int((~keep).sum()) > int((~mask).sum()) * top_k                              # masked slots and dropped ones
    assert not gw[~keep].any() and bool(gw[keep].any())
    # with a shared expert, a masked token's x.grad is the shared path's alone
    ms = build("shared", dtype, top_k, 0.5)
    xs = x.clone().requires_grad_(True)
    ms(xs, token_mask=mask)[0].backward(gy)
    xr = x.clone().requires_grad_(True)
    s, aw = ms.shared_output(xr)
    with torch.no_grad():
        none = torch.full((T, top_k), -1, dtype=torch.int32, device=DEV)
        y0 = torch.zeros(1, H, dtype=dtype, device=DEV)
    ops().combine_any(y0, none, None, top_k, addend=s, addend_weight=aw, skip_dropped=True).backward(gy)
    assert same_bits(xs.grad[~mask], xr.grad[~mask])


def test_update_selection_bias_moves_on_the_demand():
    top_k, T = 2, 130
    m = build("plain", torch.float32, top_k, 0.5, scoring="sigmoid", selection_bias=True)
    x, _, mask = problem(T, torch.float32, "random")
    with torch.no_grad():
        m(x, token_mask=mask)
    probs, demand, indices = m.routing
    kept = m.kept_per_expert
    assert probs is None and indices.shape == (T, top_k)
    d, k = demand.float(), kept.float()
    by_demand, by_kept = torch.sign(d.mean() - d), torch.sign(k.mean() - k)
    assert not torch.equal(by_demand, by_kept)                   # the two rules disagree on this input
    m.update_selection_bias(0.25)
    assert torch.equal(m.selection_bias, 0.25 * by_demand)


def test_refusals():
    m = build("plain", torch.float32, 2, 1.0)
    x, _, mask = problem(64, torch.float32, "random")
    with pytest.raises(RuntimeError, match="token_mask"):
        m(x, token_mask=mask[:-1])                               # the wrong shape
    with pytest.raises(RuntimeError, match="token_mask"):
        m(x, token_mask=mask.reshape(1, 64))
    with pytest.raises(RuntimeError, match="token_mask"):
        m(x.reshape(2, 32, H), token_mask=mask)
    with pytest.raises(RuntimeError, match="token_mask"):
        m(x, token_mask=mask.cpu())                              # the wrong device
    with pytest.raises(RuntimeError, match="token_mask"):
        m(x, token_mask=mask.float())
    with torch.no_grad():
        out, _ = m(x)                                            # a capacity alone, no mask
        assert m.kept_per_expert is not None and bool((m.kept_per_expert <= m.expert_capacity(64)).all())
        assert int(m.routing[1].sum()) == 64 * 2
