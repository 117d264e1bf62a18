"""QuantizedSparseMoEBlock with the scored router on the GPU: sigmoid scores, a selection bias, 4 groups of which 2 are
searched, routed_scaling_factor 2.5 (E=8, H=F=64, top_k=2, T=37).

  * forward: the bits of the chain ``ops.router_score_topk -> route_plan -> dispatch_rows -> experts -> combine``;
  * gradients: the rule of DESIGN.md section 16.  The comparison chain is ``dispatch_grouped``, the same experts and
    ``combine_grouped`` behind a torch router (sigmoid, the chosen scores divided by their sum + 1e-20, times the
    factor) on the block's indices; its error with a FLOAT32 router against the float64 router is measured on the same
    inputs, and the block is allowed 4x that;
  * two passes give the same gradient bits;
  * ``update_selection_bias`` moves every bias by exactly +-rate or 0, against the load;
  * a block built with the default arguments still computes what ``ops.router_topk`` gives."""
import functools

import pytest
import torch

from helpers import fq, ops, rel_fro_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
E, H, F, TOP_K, T = 8, 64, 64, 2, 37
ROUTING = dict(scoring="sigmoid", n_group=4, topk_group=2, group_top=2, routed_scaling_factor=2.5, selection_bias=True)
DTYPES = [torch.float32, torch.bfloat16]
DIDS = ["f32", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def weights_of():
    g = torch.Generator().manual_seed(29)
    return (torch.randn(E, H, generator=g) * 0.5, [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)],
            [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)], [torch.randn(H, F, generator=g) * 0.1 for _ in range(E)],
            torch.rand(E, generator=g) * 0.4 - 0.2)


def make_block(dtype, renormalize=True, **routing):
    gate_w, gate, up, down, bias = weights_of()
    adt = None if dtype == torch.float32 else dtype
    m = fq().QuantizedSparseMoEBlock.from_weights(gate_w, gate, up, down, top_k=TOP_K, activation_dtype=adt,
                                                  renormalize=renormalize, **routing).to(DEV)
    if m.selection_bias is not None:
        with torch.no_grad():
            m.selection_bias.copy_(bias)
    return m


def make_x(dtype, seed=0):
    g = torch.Generator().manual_seed(seed + T)
    return torch.randn(T, H, generator=g).to(dtype).to(DEV)


def score_args(m):
    return (m.top_k, m.scoring, m.selection_bias, m.n_group, m.topk_group, m.group_top, m.renormalize, m.routed_scaling_factor)


def torch_chain(m, x, router_dtype):
    """The comparison chain: a torch router in ``router_dtype`` on the block's own indices, then the grouped pieces."""
    x2 = x.reshape(-1, m.hidden_dim)
    logits = m.router_logits(x2)
    idx = ops().router_score_topk(logits.detach(), *score_args(m))[1].long()
    sel = torch.sigmoid(logits.to(router_dtype)).gather(1, idx)
    if m.renormalize:
        sel = sel / (sel.sum(dim=-1, keepdim=True) + 1e-20)
    w = (sel * m.routed_scaling_factor).to(torch.float32)
    rows, tpe, offs, inverse = fq().dispatch_grouped(x2, idx, m.num_experts)
    y = m.experts(rows, tpe, offs)
    return fq().combine_grouped(y.float(), w, inverse, m.top_k).to(x.dtype).reshape(x.shape)


def grads_of(run, m, x, gy):
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    run(xg).backward(gy)
    return xg.grad.clone(), m.gate.weight.grad.clone()


@pytest.mark.parametrize("renormalize", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_forward_is_the_chain_of_the_pieces(dtype, renormalize):
    m, x = make_block(dtype, renormalize, **ROUTING), make_x(dtype)
    assert m.scored_routing and float(m.selection_bias.abs().max()) > 0
    with torch.no_grad():
        out, logits = m(x)
        w, idx = ops().router_score_topk(logits, *score_args(m))
        tpe, offs, token_of_sorted, pos_of_slot = ops().route_plan(idx, E)
        y = m.experts(ops().dispatch_rows(x, token_of_sorted, pos_of_slot, TOP_K), tpe, offs)
        ref = ops().combine(y.float(), pos_of_slot, w).to(dtype)
    assert out.shape == x.shape and out.dtype == dtype and logits.shape == (T, E)
    assert same_bits(out, ref)
    assert torch.equal(m.routing[2], idx) and torch.equal(m.routing[1], tpe) and m.routing[0] is None
    assert bool(((idx >= 0) & (idx < E)).all()) and bool((idx[:, 0] != idx[:, 1]).all())
    out1, _ = m(x.clone().requires_grad_(True))                                   # grad mode: the same bits, scores kept
    assert same_bits(out1.detach(), out) and m.routing[0].shape == (T, E) and m.routing[0].requires_grad
    plain = make_block(dtype, renormalize)                                        # and the routing really differs
    with torch.no_grad():
        assert not torch.equal(plain(x)[0], out)


@pytest.mark.parametrize("renormalize", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_gradients(dtype, renormalize):
    m, x, gy = make_block(dtype, renormalize, **ROUTING), make_x(dtype), make_x(dtype, seed=5)
    gx64, gg64 = grads_of(lambda t: torch_chain(m, t, torch.float64), m, x, gy)
    gx32, gg32 = grads_of(lambda t: torch_chain(m, t, torch.float32), m, x, gy)
    gx, gg = grads_of(lambda t: m(t)[0], m, x, gy)
    assert gx.dtype == dtype and gg.dtype == torch.float32
    ex32, eg32 = rel_fro_dev(gx32, gx64), rel_fro_dev(gg32, gg64)
    ex, eg = rel_fro_dev(gx, gx64), rel_fro_dev(gg, gg64)
    print(f"scored block gradients {dtype} renormalize={renormalize}: x.grad rel err {ex:.3e} (float32 torch router "
          f"{ex32:.3e}, bound {4 * ex32:.3e}); gate.weight.grad {eg:.3e} (float32 torch router {eg32:.3e}, bound {4 * eg32:.3e})")
    assert float(torch.linalg.vector_norm(gg64.double())) > 0
    assert m.selection_bias.grad is None                                          # the bias gets no gradient
    assert ex <= 4 * ex32
    assert eg <= 4 * eg32


@pytest.mark.parametrize("renormalize", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_two_passes_give_the_same_gradient_bits(dtype, renormalize):
    m, x, gy = make_block(dtype, renormalize, **ROUTING), make_x(dtype), make_x(dtype, seed=5)

    def run(t):
        out, _ = m(t)
        return out + 0.01 * m.aux_loss().to(out.dtype)                            # grad_scores joins the router backward

    gx0, gg0 = grads_of(run, m, x, gy)
    gx1, gg1 = grads_of(run, m, x, gy)
    assert torch.isfinite(gx0).all() and float(gx0.abs().max()) > 0 and float(gg0.abs().max()) > 0
    assert same_bits(gx0, gx1) and same_bits(gg0, gg1)


def test_aux_loss_uses_the_normalised_sigmoids():
    m, x = make_block(torch.float32, True, **ROUTING), make_x(torch.float32)
    _, logits = m(x)
    s64 = torch.sigmoid(logits.detach().double())
    f = m.routing[1].double() / T
    ref = E * torch.sum(f * (s64 / s64.sum(dim=-1, keepdim=True)).mean(dim=0))
    err = abs(float(m.aux_loss().detach()) - float(ref)) / float(ref)
    print(f"scored block aux loss: rel err {err:.3e} (bound 4e-6)")
    assert err <= 4e-6


def test_update_selection_bias_moves_against_the_load():
    m = make_block(torch.float32, True, **ROUTING)
    with torch.no_grad():
        m.selection_bias.zero_()
        x = (m.gate.weight[3] * 4.0).repeat(T, 1)                                 # a skewed batch: every token wants expert 3
        x[:5] = m.gate.weight[6] * 4.0                                            # ... but five want expert 6
        m(x)
    counts = torch.bincount(m.routing[2].reshape(-1).long(), minlength=E).float()
    assert float(counts.max()) >= T - 5 and float(counts.min()) == 0              # skewed indeed
    step = torch.tensor(0.01, dtype=torch.float32, device=DEV)
    expected = torch.sign(counts.mean() - counts) * step
    m.update_selection_bias(0.01)
    assert torch.equal(m.selection_bias, expected)
    assert bool(((m.selection_bias == step) | (m.selection_bias == -step) | (m.selection_bias == 0)).all())
    assert float(m.selection_bias[3]) == -float(step) and bool((m.selection_bias[counts == 0] == step).all())
    before = m.selection_bias.clone()
    m.update_selection_bias(0.01)                                                 # the same counts again: twice the step
    assert torch.equal(m.selection_bias, before + expected)
    assert "gate.e_score_correction_bias" in m.state_dict()


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_default_block_still_runs_router_topk(dtype):
    m, x = make_block(dtype), make_x(dtype)
    assert not m.scored_routing and set(m.state_dict()) == {"gate.weight"} | {k for k in m.state_dict() if k.startswith("experts.")}
    with torch.no_grad():
        out, logits = m(x)
        w, idx = ops().router_topk(logits, TOP_K, True)
        tpe, offs, token_of_sorted, pos_of_slot = ops().route_plan(idx, E)
        y = m.experts(ops().dispatch_rows(x, token_of_sorted, pos_of_slot, TOP_K), tpe, offs)
        ref = ops().combine(y.float(), pos_of_slot, w).to(dtype)
    assert same_bits(out, ref) and torch.equal(m.routing[2], idx)
    xg = x.clone().requires_grad_(True)
    out1, logits1 = m(xg)
    _, _, probs = ops().router_topk(logits1.detach(), TOP_K, True, return_probs=True)
    assert same_bits(out1.detach(), out) and same_bits(m.routing[0].detach(), probs)
