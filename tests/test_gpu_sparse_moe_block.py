"""QuantizedSparseMoEBlock on the GPU against a chain of the existing public pieces with a torch router.

The comparison chain: ``logits = gate(x)`` as the block computes them, a float64 torch router on the widened logits
(softmax, ``torch.sort(-logits, stable=True)`` selection, renormalisation), its weights cast to float32, then
``dispatch_grouped``, the SAME expert module and ``combine_grouped``.  Only the router of that chain runs in torch
autograd; the experts and the combine are the existing autograd functions.

Bounds:
  * forward: identical indices, hence bit-identical expert rows (the same kernels on the same rows), and
    ``||out - ref||_F <= 4e-6 * || sum_k |w_k| |y_k| ||_F``: the router's weight bound and nothing else.  16-bit: compared
    after the one final rounding, one ulp of the 16-bit type added per element.
  * gradients: the error of the same chain with a FLOAT32 torch router against the float64-router chain is measured on
    the same inputs (neither is the code under test); the block is allowed 4x that, since its operation order differs and
    the dispatch backward sums in another order.  The same rule holds on 16-bit activations, with nothing added.
  * aux_loss: the probs bound, 4e-6 relative.
Each test prints its measured figures before it asserts."""
import functools

import pytest
import torch

from helpers import fq, ops, rel_fro_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL = 4e-6
MANT = {torch.float16: 10, torch.bfloat16: 7}
# (top-1 with renormalisation has the constant weight 1 and no gradient to the gate: the gradient comparisons run that
# shape un-renormalised, "E8k1"; the renormalised form "E8k1r" joins every test that does not compare a gate gradient)
SHAPES = {"E4k2": dict(E=4, H=64, F=64, top_k=2, T=37, renormalize=True),
          "E8k1": dict(E=8, H=64, F=64, top_k=1, T=5, renormalize=False),
          "E8k1r": dict(E=8, H=64, F=64, top_k=1, T=5, renormalize=True)}
CASES = [("E4k2", torch.float32), ("E8k1", torch.float32), ("E4k2", torch.bfloat16), ("E8k1", torch.bfloat16)]
ALL_CASES = CASES + [("E8k1r", torch.float32), ("E8k1r", torch.bfloat16)]


def _ids(cases):
    return [f"{s}-{'f32' if d == torch.float32 else 'bf16'}" for s, d in cases]


CASE_IDS, ALL_IDS = _ids(CASES), _ids(ALL_CASES)


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
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(17 + s["E"])
    E, H, F = s["E"], s["H"], s["F"]
    return (torch.randn(E, H, generator=g) * 0.5, [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)],
            [torch.randn(F, H, generator=g) * 0.1 for _ in range(E)], [torch.randn(H, F, generator=g) * 0.1 for _ in range(E)])


def make_block(shape, dtype, renormalize=None):
    s = SHAPES[shape]
    renormalize = s["renormalize"] if renormalize is None else renormalize
    gate_w, gate, up, down = weights_of(shape)
    adt = None if dtype == torch.float32 else dtype
    return fq().QuantizedSparseMoEBlock.from_weights(gate_w, gate, up, down, top_k=s["top_k"], activation_dtype=adt,
                                                     renormalize=renormalize).to(DEV)


def make_x(shape, dtype, seed=0):
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(seed + s["T"])
    return torch.randn(s["T"], s["H"], generator=g).to(dtype).to(DEV)


def torch_router(logits, top_k, renormalize, router_dtype):
    l = logits.to(router_dtype)
    idx = torch.sort(-l.detach(), dim=-1, stable=True).indices[:, :top_k]
    p = torch.softmax(l, dim=-1)
    sel = p.gather(1, idx)
    w = sel / sel.sum(dim=-1, keepdim=True) if renormalize else sel
    return w.to(torch.float32), idx


def chain(m, x, router_dtype=torch.float64):
    """(out, indices, expert rows y, weights) of the comparison chain."""
    x2 = x.reshape(-1, m.hidden_dim)
    logits = m.router_logits(x2)
    w, idx = torch_router(logits, m.top_k, m.renormalize, router_dtype)
    rows, tpe, offs, inverse = fq().dispatch_grouped(x2, idx, m.num_experts)
    y = m.experts(rows, tpe, offs)
    out = fq().combine_grouped(y.float(), w, inverse, m.top_k)
    return out.to(x.dtype).reshape(x.shape), idx, y, w


def ulp_of(ref, dtype):
    """Spacing of ``dtype`` at |ref| (float64)."""
    a = ref.double().abs().clamp_min(2.0 ** -24)
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,dtype", ALL_CASES, ids=ALL_IDS)
def test_forward_parity(shape, dtype):
    m, x = make_block(shape, dtype), make_x(shape, dtype)
    seen = {}
    hook = m.experts.register_forward_hook(lambda mod, inp, out: seen.setdefault("y", []).append(out))
    with torch.no_grad():
        out, logits = m(x)
        ref, idx, y_ref, w_ref = chain(m, x)
    hook.remove()
    s = SHAPES[shape]
    assert out.shape == x.shape and out.dtype == dtype and logits.shape == (s["T"], s["E"])
    w, got_idx = ops().router_topk(logits, m.top_k, m.renormalize)
    assert torch.equal(got_idx.long(), idx)
    tpe = ops().route_plan(got_idx, m.num_experts)[0]
    if s["top_k"] == 1:
        assert int((tpe == 0).sum()) >= 1                    # an empty expert is part of this case
    y_block, y_chain = seen["y"]
    assert same_bits(y_block, y_chain) and same_bits(y_chain, y_ref)
    pos = ops().route_plan(got_idx, m.num_experts)[3].long().view(-1, m.top_k)
    envelope = (w_ref.double().abs().unsqueeze(-1) * y_ref.double().abs()[pos]).sum(dim=1)
    bound = REL * float(torch.linalg.vector_norm(envelope))
    if dtype != torch.float32:
        bound += float(torch.linalg.vector_norm(ulp_of(ref, dtype)))
    err = float(torch.linalg.vector_norm(out.double() - ref.double()))
    print(f"block forward {shape} {dtype}: ||out - ref||_F {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("shape,dtype", ALL_CASES, ids=ALL_IDS)
def test_inference_path_gives_the_same_bits(shape, dtype):
    m, x = make_block(shape, dtype), make_x(shape, dtype)
    with torch.no_grad():
        out0, logits0 = m(x)
    out1, logits1 = m(x.clone().requires_grad_(True))
    assert out1.requires_grad and logits1.requires_grad and not out0.requires_grad
    assert same_bits(out0, out1.detach()) and same_bits(logits0, logits1.detach())
    out2, _ = m(x.reshape(1, -1, x.shape[-1]))               # [..., H] in, [..., H] out
    assert out2.shape == (1,) + x.shape and same_bits(out2.detach().reshape(x.shape), out0)


# ---------------------------------------------------------------------------------------------------------- gradients
def grads_of(run, m, x, gy):
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    out = run(xg)
    out.backward(gy)
    return xg.grad.clone(), m.gate.weight.grad.clone()


@pytest.mark.parametrize("shape,dtype", CASES, ids=CASE_IDS)
def test_gradients(shape, dtype):
    m, x = make_block(shape, dtype), make_x(shape, dtype)
    gy = make_x(shape, dtype, seed=5)
    gx64, gg64 = grads_of(lambda t: chain(m, t, torch.float64)[0], m, x, gy)
    gx32, gg32 = grads_of(lambda t: chain(m, t, torch.float32)[0], m, x, gy)
    gx, gg = grads_of(lambda t: m(t)[0], m, x, gy)
    assert gx.dtype == dtype and gg.dtype == torch.float32
    ex32, eg32 = rel_fro_dev(gx32, gx64), rel_fro_dev(gg32, gg64)
    ex, eg = rel_fro_dev(gx, gx64), rel_fro_dev(gg, gg64)
    print(f"block gradients {shape} {dtype}: x.grad rel err {ex:.3e} (float32 torch router {ex32:.3e}, bound {4 * ex32:.3e}); "
          f"gate.weight.grad {eg:.3e} (float32 torch router {eg32:.3e}, bound {4 * eg32:.3e})")
    assert float(torch.linalg.vector_norm(gg64.double())) > 0
    assert ex <= 4 * ex32
    assert eg <= 4 * eg32


# -------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("shape,dtype", ALL_CASES, ids=ALL_IDS)
def test_two_passes_give_the_same_gradient_bits(shape, dtype):
    """Forward + backward of the block twice from the same state: ``x.grad`` and ``gate.weight.grad`` bit for bit, the
    point of running the dispatch backward through the gather-add kernel and not through ``index_add_``."""
    m, x = make_block(shape, dtype), make_x(shape, dtype)
    gy = make_x(shape, dtype, seed=5)
    gx0, gg0 = grads_of(lambda t: m(t)[0], m, x, gy)
    gx1, gg1 = grads_of(lambda t: m(t)[0], m, x, gy)          # grads_of zeroes the module's gradients first
    assert torch.isfinite(gx0).all() and float(gx0.abs().max()) > 0
    assert same_bits(gx0, gx1)
    assert same_bits(gg0, gg1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dispatch_rows_alone(dtype):
    """``ops.dispatch_rows`` by itself: the forward is ``x[token_of_sorted]``; the backward is the sum of a token's
    ``top_k`` gradient rows in float32 (each partial sum rounded once: ``(top_k - 1) * 2^-24 * sum_j |g_j|`` against
    float64), a 16-bit gradient being that float32 sum rounded once; two calls give the same bits."""
    T, H, E, top_k = 37, 64, 4, 2
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H, generator=g).to(dtype).to(DEV)
    idx = torch.stack([torch.randperm(E, generator=g)[:top_k] for _ in range(T)]).to(torch.int32).to(DEV)
    _, _, token_of_sorted, pos_of_slot = ops().route_plan(idx, E)
    gy = torch.randn(T * top_k, H, generator=g).to(dtype).to(DEV)

    def run(xin, grad):
        xg = xin.clone().requires_grad_(True)
        rows = ops().dispatch_rows(xg, token_of_sorted, pos_of_slot, top_k)
        rows.backward(grad)
        return rows.detach(), xg.grad

    rows, gx = run(x, gy)
    assert same_bits(rows, x[token_of_sorted.long()])
    with torch.no_grad():
        assert same_bits(ops().dispatch_rows(x, token_of_sorted, pos_of_slot, top_k), rows)
    assert gx.dtype == dtype and same_bits(gx, run(x, gy)[1])
    gx32 = run(x.float(), gy.float())[1]
    terms = gy.double()[pos_of_slot.long().view(T, top_k)]
    err = (gx32.double() - terms.sum(dim=1)).abs()
    assert bool((err <= (top_k - 1) * 2.0 ** -24 * terms.abs().sum(dim=1)).all())
    if dtype != torch.float32:
        assert same_bits(gx, gx32.to(dtype))


# --------------------------------------------------------------------------------------------------------------- LoRA
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_lora_experts_train_through_the_block(dtype):
    shape = "E4k2"
    s = SHAPES[shape]
    base = make_block(shape, dtype)
    experts = fq().LoRAQuantizedMoEFFN.from_quantized(base.experts, 8, alpha=16)
    g = torch.Generator(device=DEV).manual_seed(3)
    with torch.no_grad():
        experts.gate_up_lora_B.normal_(0, 0.1, generator=g)
        experts.down_lora_B.normal_(0, 0.1, generator=g)
    m = fq().QuantizedSparseMoEBlock(s["E"], s["H"], s["F"], top_k=s["top_k"], activation_dtype=experts.activation_dtype,
                                     experts=experts).to(DEV)
    with torch.no_grad():
        m.gate.weight.copy_(base.gate.weight)
    names = ("gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B")
    x, gy = make_x(shape, dtype), make_x(shape, dtype, seed=7)
    seen = {}

    def hook(mod, inp, out):
        seen["in"] = (inp[0].detach(), inp[1], inp[2])
        out.register_hook(lambda grad: seen.__setitem__("gy", grad.detach().clone()))

    h = m.experts.register_forward_hook(hook)
    out, _ = m(x.clone().requires_grad_(True))
    out.backward(gy)
    h.remove()
    got = {n: getattr(experts, n).grad.clone() for n in names}
    assert m.gate.weight.grad is not None and float(m.gate.weight.grad.abs().max()) > 0
    for n in names:
        assert float(got[n].abs().max()) > 0, n
    m.zero_grad(set_to_none=True)
    rows, tpe, offs = seen["in"]
    y = experts(rows.clone().requires_grad_(True), tpe, offs)
    y.backward(seen["gy"])
    for n in names:
        assert same_bits(got[n], getattr(experts, n).grad), n


# ----------------------------------------------------------------------------------------------------------- aux loss
@pytest.mark.parametrize("shape,dtype", ALL_CASES, ids=ALL_IDS)
def test_aux_loss(shape, dtype):
    m, x = make_block(shape, dtype), make_x(shape, dtype)
    s = SHAPES[shape]
    T, E = s["T"], s["E"]
    with torch.no_grad():
        m(x)
    idx_plain = m.routing[2].clone()                         # a forward that no auxiliary loss ever followed
    assert m.routing[0] is None
    with pytest.raises(RuntimeError):
        m.aux_loss()                                         # no probabilities were kept under no_grad
    out, logits = m(x)
    probs, tpe, idx = m.routing
    assert torch.equal(idx, idx_plain) and probs.shape == (T, E) and probs.requires_grad
    assert torch.equal(tpe.long(), torch.bincount(idx.reshape(-1).long(), minlength=E))
    aux = m.aux_loss()
    p64 = torch.softmax(logits.detach().double(), dim=-1)
    f = tpe.double() / T
    ref = E * torch.sum(f * p64.mean(dim=0))
    err = abs(float(aux.detach()) - float(ref)) / float(ref)
    print(f"aux loss {shape} {dtype}: {float(aux.detach()):.7f} vs float64 {float(ref):.7f}, rel err {err:.3e} (bound {REL:.0e})")
    assert err <= REL
    _, idx2, probs2 = ops().router_topk(logits.detach(), m.top_k, m.renormalize, return_probs=True)
    assert float(m.aux_loss(probs2, ops().route_plan(idx2, E)[0])) == float(aux.detach())       # the explicit form
    g_aux, = torch.autograd.grad(aux, m.gate.weight, retain_graph=True)
    assert torch.isfinite(g_aux).all() and float(g_aux.abs().max()) > 0
    l64 = logits.detach().double().requires_grad_(True)
    (E * torch.sum(f * torch.softmax(l64, dim=-1).mean(dim=0))).backward()
    g_logits, = torch.autograd.grad(aux, logits, retain_graph=True)
    if dtype == torch.float32:                               # the router backward's bound, grad_probs = E * f_e / T
        scale = float((E * f / T).abs().max())
        assert float((g_logits.double() - l64.grad).abs().max()) <= 4e-5 * scale
    m.zero_grad(set_to_none=True)
    (out.float().sum() + 0.01 * aux).backward()
    assert m.gate.weight.grad is not None and torch.isfinite(m.gate.weight.grad).all()
    out_again, _ = m(x)                                      # a second forward, after the backward with the aux term
    assert torch.equal(m.routing[2], idx_plain) and same_bits(out_again.detach(), out.detach())


def test_plain_weights_and_state_dict_round_trip():
    m = make_block("E4k2", torch.float32, renormalize=False)
    x = make_x("E4k2", torch.float32)
    with torch.no_grad():
        out, _ = m(x)
        ref, _, _, _ = chain(m, x)
    assert rel_fro_dev(out, ref) <= 1e-5
    m2 = fq().QuantizedSparseMoEBlock(4, 64, 64, top_k=2, renormalize=False).to(DEV)
    m2.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert same_bits(m2(x)[0], out)
