"""QuantizedSparseMoEBlock with a shared expert (and its sigmoid gate) on the GPU.

Two blocks, E=4 / top_k=2 / T=37 and E=8 / top_k=1 / T=5 (experts that receive no rows), H = F = 64 and a shared expert of
96, each in float32 and bfloat16, with the shared gate off and on, under Mixtral routing and one scored configuration
(``scoring="sigmoid", routed_scaling_factor=2.5``).  (Top-1 runs un-renormalised, as in tests/test_gpu_sparse_moe_block.py:
renormalised top-1 weights are constant and give the gate no gradient.)

  * forward: bit for bit the chain of the pieces built by hand from the block's own modules,
    ``(ops.combine(y.float(), pos, w) + s.float() [* sigmoid(z)[:, None]]).to(dtype)``, ``z`` the shared gate's output
    widened to float32; ``router_logits`` are those of a block without the shared expert on the same gate and experts.
  * ``routed_scaling_factor`` does not reach the shared part: two float32 blocks that differ in it alone add the same
    shared term to their routed sums.
  * ``x.grad`` against the sum of three separately obtained parts, a (dispatch, experts, combine), b (shared expert) and c
    (the gate or gates): ``|x.grad - (a + b + c)| <= 2 * u * (|a| + |b| + |c|)`` elementwise, u = 2^-24 (float32) or 2^-8
    (bfloat16, where the parts arrive already rounded): two additions in an order autograd chooses.  (With the shared gate
    on, c is one autograd sum of the two gates' parts, here and in the block, which reads the tokens for both gates
    through one alias: the same two addends, hence the same bits whichever comes first.)
  * ``gate.weight.grad``: bit for bit that of the block without the shared expert (shared gate off).
  * ``shared_expert_gate.weight.grad``: 4e-6 relative Frobenius (one dot product plus one sigmoid)
    against a float64 evaluation of ``dz = <s, g> * sigmoid'(z)`` on the same s, g and z, handed to the torch layer's own
    backward in the activations' type (in bfloat16 that backward rounds to bfloat16, in the block and here alike).
  * LoRA on the shared expert, determinism, state dict, refusals.
Each comparison with a bound prints its figures before it asserts."""
import functools

import pytest
import torch
from torch import nn

from helpers import fq, ops, rel_fro_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, F, FS = 64, 64, 96
SHAPES = {"E4k2": dict(E=4, top_k=2, T=37, renormalize=True), "E8k1": dict(E=8, top_k=1, T=5, renormalize=False)}
ROUTINGS = {"mixtral": {}, "scored": dict(scoring="sigmoid", routed_scaling_factor=2.5)}
CASES = [(s, d, g, r) for s in SHAPES for d in (torch.float32, torch.bfloat16) for g in (False, True) for r in ROUTINGS]
IDS = [f"{s}-{'f32' if d == torch.float32 else 'bf16'}-{'gated' if g else 'plain'}-{r}" for s, d, g, r in CASES]
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}
OLD_KEYS = {"gate.weight"} | {f"experts.{n}" for n in ("gate_up_packed", "gate_up_scales", "gate_up_zero_points",
                                                       "down_packed", "down_scales", "down_zero_points")}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def weights_of(shape):
    E = SHAPES[shape]["E"]
    g = torch.Generator().manual_seed(23 + E)
    r = lambda *s, scale=0.1: torch.randn(*s, generator=g) * scale
    return dict(gate_w=r(E, H, scale=0.5), gate=[r(F, H) for _ in range(E)], up=[r(F, H) for _ in range(E)],
                down=[r(H, F) for _ in range(E)], shared=(r(FS, H), r(FS, H), r(H, FS)), shared_gate_w=r(1, H, scale=0.5))


def make_block(shape, dtype, gated, routing, shared=True, **over):
    s, w = SHAPES[shape], weights_of(shape)
    kw = dict(top_k=s["top_k"], activation_dtype=None if dtype == torch.float32 else dtype, renormalize=s["renormalize"],
              **{**ROUTINGS[routing], **over})
    if shared:
        kw.update(shared=w["shared"], shared_expert_gate_weight=w["shared_gate_w"] if gated else None)
    return fq().QuantizedSparseMoEBlock.from_weights(w["gate_w"], w["gate"], w["up"], w["down"], **kw).to(DEV)


def make_x(shape, dtype, seed=0):
    T = SHAPES[shape]["T"]
    g = torch.Generator().manual_seed(seed + T)
    return torch.randn(T, H, generator=g).to(dtype).to(DEV), torch.randn(T, H, generator=g).to(dtype).to(DEV)


def route(m, logits):
    """(weights, indices, tokens_per_expert, input_offsets, token_of_sorted, pos_of_slot) as the block routes."""
    if m.scored_routing:
        w, idx = ops().router_score_topk(logits, m.top_k, m.scoring, m.selection_bias, m.n_group, m.topk_group, m.group_top,
                                         m.renormalize, m.routed_scaling_factor)
    else:
        w, idx = ops().router_topk(logits, m.top_k, m.renormalize)
    return (w, idx) + tuple(ops().route_plan(idx, m.num_experts))


def shared_rows(m, x2):
    T = x2.shape[0]
    return m.shared_experts(x2, torch.full((1,), T, dtype=torch.int32, device=x2.device),
                            torch.zeros(1, dtype=torch.int32, device=x2.device))


def shared_logit(m, x2):
    """z [T] float32: the shared gate's output, computed in the activations' type as the block does, then widened."""
    return nn.functional.linear(x2, m.shared_expert_gate.weight.to(x2.dtype)).float().reshape(-1)


def shared_term(m, x2):
    """The float32 term the shared part adds: s, or s * sigmoid(z)."""
    term = shared_rows(m, x2).float()
    if hasattr(m, "shared_expert_gate"):
        term = term * torch.sigmoid(shared_logit(m, x2))[:, None]
    return term


def hand_chain(m, x2):
    """(out, logits, routed float32 sum, shared float32 term) from the pieces, through ops.combine."""
    logits = m.router_logits(x2)
    w, idx, tpe, offs, tos, pos = route(m, logits)
    y = m.experts(ops().dispatch_rows(x2, tos, pos, m.top_k), tpe, offs)
    routed = ops().combine(y.float(), pos, w)
    term = shared_term(m, x2)
    return (routed + term).to(x2.dtype), logits, routed, term


def plain_twin(m, shape, dtype, routing):
    """A block without the shared expert on m's own gate and experts."""
    twin = make_block(shape, dtype, False, routing, shared=False)
    twin.gate, twin.experts = m.gate, m.experts
    return twin


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,dtype,gated,routing", CASES, ids=IDS)
def test_forward_is_the_chain_of_the_pieces(shape, dtype, gated, routing):
    m = make_block(shape, dtype, gated, routing)
    x, _ = make_x(shape, dtype)
    with torch.no_grad():
        out, logits = m(x)
        ref, ref_logits, routed, term = hand_chain(m, x)
        plain_out, plain_logits = plain_twin(m, shape, dtype, routing)(x)
        tpe = route(m, logits)[2]
    assert out.dtype == dtype and out.shape == x.shape
    assert same_bits(out, ref) and same_bits(logits, ref_logits) and same_bits(logits, plain_logits)
    assert same_bits(plain_out, routed.to(dtype))
    assert float(term.abs().max()) > 0 and not same_bits(out, plain_out)
    if SHAPES[shape]["top_k"] == 1:
        assert int((tpe == 0).sum()) >= 1                    # experts without rows are part of this case
    with torch.enable_grad():                                # the training path gives the same bits
        assert same_bits(m(x.clone().requires_grad_(True))[0].detach(), out)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_routed_scaling_factor_does_not_reach_the_shared_part(shape, gated):
    a = make_block(shape, torch.float32, gated, "scored")
    b = make_block(shape, torch.float32, gated, "scored", routed_scaling_factor=1.5)
    x, _ = make_x(shape, torch.float32)
    with torch.no_grad():
        out_a, out_b = a(x)[0], b(x)[0]
        _, logits, routed_a, term_a = hand_chain(a, x)
        _, _, routed_b, term_b = hand_chain(b, x)
        wa, ia = route(a, logits)[:2]
        wb, ib = route(b, logits)[:2]
    assert torch.equal(ia, ib) and not torch.equal(wa, wb)
    assert same_bits(term_a, term_b)
    assert same_bits(out_a, routed_a + term_a) and same_bits(out_b, routed_b + term_a)
    assert not same_bits(routed_a, routed_b)


# ---------------------------------------------------------------------------------------------------------- gradients
def block_grads(m, x, g):
    for p in m.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    m(xg)[0].backward(g)
    return xg.grad, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("shape,dtype,gated,routing", CASES, ids=IDS)
def test_input_gradient_is_the_sum_of_its_parts(shape, dtype, gated, routing):
    m = make_block(shape, dtype, gated, routing)
    x, g = make_x(shape, dtype)
    got, _ = block_grads(m, x, g)
    with torch.no_grad():
        logits = m.router_logits(x)
        w, idx, tpe, offs, tos, pos = route(m, logits)
        y = m.experts(ops().dispatch_rows(x, tos, pos, m.top_k), tpe, offs)
        s = shared_rows(m, x)
        aw = torch.sigmoid(shared_logit(m, x)) if gated else None
    # a: dispatch -> experts -> combine, the routing weights held fixed
    xa = x.clone().requires_grad_(True)
    ya = m.experts(ops().dispatch_rows(xa, tos, pos, m.top_k), tpe, offs)
    ops().combine(ya.float(), pos, w).to(dtype).backward(g)
    # b: the shared expert, its weight held fixed
    xb = x.clone().requires_grad_(True)
    sb = shared_rows(m, xb).float()
    (sb * aw[:, None] if gated else sb).to(dtype).backward(g)
    # c: the router's gate (and the shared gate), the expert and shared rows held fixed.  Through the block's own combine:
    # the parts must be the block's to the bit for the bound to be about the additions alone, and a torch product-and-sum
    # would order the shared gate's dot product <s, g> differently (tests/test_gpu_combine_any.py checks those bits).
    xc = x.clone().requires_grad_(True)
    wc = route(m, m.router_logits(xc))[0]
    awc = torch.sigmoid(shared_logit(m, xc)) if gated else None
    ops().combine_any(y, pos, wc, addend=s, addend_weight=awc, out_dtype=dtype).backward(g)
    a, b, c = xa.grad.double(), xb.grad.double(), xc.grad.double()
    assert got.dtype == dtype
    err = (got.double() - (a + b + c)).abs()
    bound = 2 * UNIT[dtype] * (a.abs() + b.abs() + c.abs())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"x.grad {shape} {dtype} gated={gated} {routing}: max |err| / bound = {ratio:.3f}, "
          f"|a| {float(a.abs().max()):.3e} |b| {float(b.abs().max()):.3e} |c| {float(c.abs().max()):.3e}")
    assert float(b.abs().max()) > 0 and float(c.abs().max()) > 0
    assert bool((err <= bound).all())


@pytest.mark.parametrize("shape,dtype,routing", [(s, d, r) for s, d, g, r in CASES if not g],
                         ids=[i for i, c in zip(IDS, CASES) if not c[2]])
def test_gate_gradient_is_that_of_the_block_without_the_shared_expert(shape, dtype, routing):
    m = make_block(shape, dtype, False, routing)
    x, g = make_x(shape, dtype)
    _, grads = block_grads(m, x, g)
    twin = plain_twin(m, shape, dtype, routing)
    _, twin_grads = block_grads(twin, x, g)
    assert float(grads["gate.weight"].abs().max()) > 0
    assert same_bits(grads["gate.weight"], twin_grads["gate.weight"])


@pytest.mark.parametrize("shape,dtype,routing", [(s, d, r) for s, d, g, r in CASES if g],
                         ids=[i for i, c in zip(IDS, CASES) if c[2]])
def test_shared_gate_gradient(shape, dtype, routing):
    m = make_block(shape, dtype, True, routing)
    x, g = make_x(shape, dtype)
    _, grads = block_grads(m, x, g)
    got = grads["shared_expert_gate.weight"]
    with torch.no_grad():
        s = shared_rows(m, x)
        z = shared_logit(m, x).double()
        sig = torch.sigmoid(z)
        dz = (s.double() * g.double()).sum(dim=-1) * sig * (1.0 - sig)
    wg = m.shared_expert_gate.weight
    z_again = nn.functional.linear(x, wg.to(dtype))
    ref, = torch.autograd.grad(z_again, wg, grad_outputs=dz.to(dtype).reshape(-1, 1))
    err = rel_fro_dev(got, ref)
    print(f"shared_expert_gate.weight.grad {shape} {dtype} {routing}: rel fro {err:.3e} (bound 4e-6)")
    assert got.dtype == torch.float32 and float(ref.abs().max()) > 0
    assert err <= 4e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_lora_on_the_shared_expert(dtype, gated):
    shape, w = "E4k2", weights_of("E4k2")
    adt = None if dtype == torch.float32 else dtype
    base = fq().QuantizedMoEFFN.from_weights(*[[t] for t in w["shared"]], activation_dtype=adt)
    lora = fq().LoRAQuantizedMoEFFN.from_quantized(base, rank=8).to(DEV)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in lora.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    m = make_block(shape, dtype, False, "mixtral", shared=False)
    s = SHAPES[shape]
    block = fq().QuantizedSparseMoEBlock(s["E"], H, F, top_k=s["top_k"], activation_dtype=adt, experts=m.experts,
                                         shared_experts=lora, shared_expert_gate=gated).to(DEV)
    block.gate = m.gate
    x, g = make_x(shape, dtype)
    _, grads = block_grads(block, x, g)
    names = [n for n, _ in lora.named_parameters()]
    assert names and all("lora" in n for n in names)
    for p in lora.parameters():
        p.grad = None
    upstream = g
    if gated:
        with torch.no_grad():
            upstream = (torch.sigmoid(shared_logit(block, x))[:, None] * g.float()).to(dtype)
    shared_rows(block, x).backward(upstream)
    for n, p in lora.named_parameters():
        assert float(p.grad.abs().max()) > 0, n
        assert same_bits(grads[f"shared_experts.{n}"], p.grad), n


@pytest.mark.parametrize("shape,dtype,gated,routing", [c for c in CASES if c[3] == "scored"],
                         ids=[i for i, c in zip(IDS, CASES) if c[3] == "scored"])
def test_two_passes_give_the_same_bits(shape, dtype, gated, routing):
    m = make_block(shape, dtype, gated, routing)
    x, g = make_x(shape, dtype)
    gx1, grads1 = block_grads(m, x, g)
    gx2, grads2 = block_grads(m, x, g)
    assert same_bits(gx1, gx2) and set(grads1) == set(grads2)
    assert "gate.weight" in grads1 and (("shared_expert_gate.weight" in grads1) == gated)
    for n in grads1:
        assert same_bits(grads1[n], grads2[n]), n


# --------------------------------------------------------------------------------------------- state dict and refusals
def test_state_dict():
    plain = make_block("E4k2", torch.float32, False, "mixtral", shared=False)
    assert set(plain.state_dict()) == OLD_KEYS
    assert not hasattr(plain, "shared_experts") and not hasattr(plain, "shared_expert_gate")
    m = make_block("E4k2", torch.float32, True, "mixtral")
    sd = m.state_dict()
    new = {"shared_expert_gate.weight"} | {k.replace("experts.", "shared_experts.", 1) for k in OLD_KEYS if k.startswith("experts.")}
    assert set(sd) == OLD_KEYS | new
    s = SHAPES["E4k2"]
    fresh = fq().QuantizedSparseMoEBlock(s["E"], H, F, top_k=s["top_k"], shared_ffn_dim=FS, shared_expert_gate=True).to(DEV)
    assert set(fresh.state_dict()) == set(sd)
    fresh.load_state_dict(sd)
    x, _ = make_x("E4k2", torch.float32)
    with torch.no_grad():
        assert same_bits(fresh(x)[0], m(x)[0])
    with pytest.raises(RuntimeError, match="Missing key"):
        fresh.load_state_dict(plain.state_dict())
    plain.load_state_dict({k: v for k, v in sd.items() if k in OLD_KEYS})     # an old state dict loads into an old block
    assert "shared_ffn_dim=96" in repr(m) and "shared_expert_gate=True" in repr(m)
    assert "shared" not in repr(plain).replace("QuantizedSparseMoEBlock", "")


def test_refusals():
    B, FFN = fq().QuantizedSparseMoEBlock, fq().QuantizedMoEFFN
    with pytest.raises(ValueError, match="shared_ffn_dim"):
        B(4, H, F, shared_ffn_dim=40)
    with pytest.raises(ValueError, match="shared_experts must be"):
        B(4, H, F, shared_experts=FFN(1, 2 * H, FS))
    with pytest.raises(ValueError, match="shared_experts must be"):
        B(4, H, F, shared_experts=FFN(2, H, FS))
    with pytest.raises(ValueError, match="differ"):
        B(4, H, F, shared_ffn_dim=FS, shared_experts=FFN(1, H, 2 * FS))
    with pytest.raises(ValueError, match="needs a shared expert"):
        B(4, H, F, shared_expert_gate=True)
    w = weights_of("E4k2")
    with pytest.raises(ValueError, match="shared_expert_gate_weight"):
        B.from_weights(w["gate_w"], w["gate"], w["up"], w["down"], shared=w["shared"],
                       shared_expert_gate_weight=torch.zeros(2, H))
    B(4, H, F, shared_ffn_dim=FS, shared_experts=FFN(1, H, FS))             # the same size twice is no conflict
