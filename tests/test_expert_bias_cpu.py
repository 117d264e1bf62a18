"""Per-expert biases of the gated FFN layers on the CPU: the parameters and their state-dict keys, ``from_weights``,
``from_quantized``, the sparse block's conflict rule and router bias, extra_repr and the ops' argument checks (the forward
is GPU only)."""
import pytest
import torch

from conftest import ROOT  # noqa: F401

BASE_KEYS = {"gate_up_packed", "gate_up_scales", "gate_up_zero_points", "down_packed", "down_scales", "down_zero_points"}
BIAS_KEYS = {"gate_up_bias", "down_bias"}
ADAPTER_KEYS = {"gate_up_lora_A", "gate_up_lora_B", "down_lora_A", "down_lora_B"}
E, H, F = 2, 64, 96


def fq():
    import fused_int4_amd
    return fused_int4_amd


def ops():
    from fused_int4_amd import ops as o
    return o


def weights(seed=0):
    torch.manual_seed(seed)
    return ([torch.randn(F, H) * 0.1 for _ in range(E)], [torch.randn(F, H) * 0.1 for _ in range(E)],
            [torch.randn(H, F) * 0.1 for _ in range(E)])


def biases(seed=1):
    torch.manual_seed(seed)
    return [torch.randn(F) for _ in range(E)], [torch.randn(F) for _ in range(E)], [torch.randn(H) for _ in range(E)]


def test_state_dict_keys_and_parameters():
    m = fq().QuantizedMoEFFN(E, H, F)
    assert set(m.state_dict()) == BASE_KEYS and list(m.parameters()) == []
    assert m.expert_bias is False and m.biases == (None, None)
    m = fq().QuantizedMoEFFN(E, H, F, expert_bias=True)
    assert set(m.state_dict()) == BASE_KEYS | BIAS_KEYS
    assert {n for n, _ in m.named_parameters()} == BIAS_KEYS
    for name, shape in (("gate_up_bias", (E, 2 * F)), ("down_bias", (E, H))):
        p = getattr(m, name)
        assert isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 and tuple(p.shape) == shape
        assert not p.requires_grad and torch.count_nonzero(p) == 0       # frozen like the weights, zeros until loaded
    m.gate_up_bias.requires_grad_(True)
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["gate_up_bias"]
    lo = fq().LoRAQuantizedMoEFFN(E, H, F, rank=4)
    assert set(lo.state_dict()) == BASE_KEYS | ADAPTER_KEYS
    lo = fq().LoRAQuantizedMoEFFN(E, H, F, rank=4, expert_bias=True)
    assert set(lo.state_dict()) == BASE_KEYS | ADAPTER_KEYS | BIAS_KEYS
    assert set(lo.adapter_state_dict()) == ADAPTER_KEYS
    assert {n for n, p in lo.named_parameters() if p.requires_grad} == ADAPTER_KEYS


def test_a_biased_checkpoint_loads_and_a_plain_one_does_not_grow():
    g, u, d = weights()
    gb, ub, db = biases()
    src = fq().QuantizedMoEFFN.from_weights(g, u, d, gate_bias=gb, up_bias=ub, down_bias=db)
    dst = fq().QuantizedMoEFFN(E, H, F, expert_bias=True)
    dst.load_state_dict(src.state_dict())
    assert torch.equal(dst.gate_up_bias, src.gate_up_bias) and torch.equal(dst.down_bias, src.down_bias)
    assert not dst.gate_up_bias.requires_grad
    plain = fq().QuantizedMoEFFN(E, H, F)
    with pytest.raises(RuntimeError):                                   # unexpected keys: a plain layer has no bias
        plain.load_state_dict(src.state_dict())


def test_from_weights():
    g, u, d = weights()
    gb, ub, db = biases()
    m = fq().QuantizedMoEFFN.from_weights(g, u, d, gate_bias=gb, up_bias=ub, down_bias=db)
    assert m.expert_bias and set(m.state_dict()) == BASE_KEYS | BIAS_KEYS
    for e in range(E):                                                  # gate | up, stacked like the weight rows
        assert torch.equal(m.gate_up_bias[e, :F], gb[e]) and torch.equal(m.gate_up_bias[e, F:], ub[e])
        assert torch.equal(m.down_bias[e], db[e])
    assert not m.gate_up_bias.requires_grad and not m.down_bias.requires_grad
    plain = fq().QuantizedMoEFFN.from_weights(g, u, d)
    assert not plain.expert_bias and set(plain.state_dict()) == BASE_KEYS
    assert torch.equal(plain.gate_up_packed, m.gate_up_packed)          # the weights do not depend on the biases
    for kw in (dict(gate_bias=gb), dict(up_bias=ub, down_bias=db), dict(gate_bias=gb, up_bias=ub),
               dict(gate_bias=gb, down_bias=db)):
        with pytest.raises(ValueError):
            fq().QuantizedMoEFFN.from_weights(g, u, d, **kw)
    with pytest.raises(ValueError):                                     # wrong length of one of them
        fq().QuantizedMoEFFN.from_weights(g, u, d, gate_bias=gb, up_bias=ub, down_bias=[torch.randn(H + 1)] * E)
    with pytest.raises(ValueError):
        fq().QuantizedMoEFFN.from_weights(g, u, d, gate_bias=gb[:1], up_bias=ub, down_bias=db)


def test_from_quantized_carries_the_biases():
    g, u, d = weights()
    gb, ub, db = biases()
    base = fq().QuantizedMoEFFN.from_weights(g, u, d, gate_bias=gb, up_bias=ub, down_bias=db)
    base.down_bias.requires_grad_(True)
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, 8)
    assert m.expert_bias
    assert m.gate_up_bias is base.gate_up_bias and m.down_bias is base.down_bias       # shared, like the buffers
    assert not m.gate_up_bias.requires_grad and m.down_bias.requires_grad              # in the state they had
    assert set(m.state_dict()) == BASE_KEYS | ADAPTER_KEYS | BIAS_KEYS
    plain = fq().LoRAQuantizedMoEFFN.from_quantized(fq().QuantizedMoEFFN.from_weights(g, u, d), 8)
    assert not plain.expert_bias and set(plain.state_dict()) == BASE_KEYS | ADAPTER_KEYS


def test_sparse_block_arguments():
    Block = fq().QuantizedSparseMoEBlock
    plain = Block(E, H, F, top_k=1)
    assert set(plain.state_dict()) == {"gate.weight"} | {"experts." + k for k in BASE_KEYS}
    assert plain.gate.bias is None and not plain.experts.expert_bias
    b = Block(E, H, F, top_k=1, expert_bias=True, router_bias=True)
    assert set(b.state_dict()) == {"gate.weight", "gate.bias"} | {"experts." + k for k in BASE_KEYS | BIAS_KEYS}
    assert b.gate.bias.requires_grad and tuple(b.gate.bias.shape) == (E,)
    # a module passed in keeps its own; an explicit contradiction raises
    with_bias = fq().QuantizedMoEFFN(E, H, F, expert_bias=True)
    without = fq().QuantizedMoEFFN(E, H, F)
    assert Block(E, H, F, top_k=1, experts=with_bias).experts.expert_bias
    assert Block(E, H, F, top_k=1, experts=with_bias, expert_bias=True).experts is with_bias
    assert not Block(E, H, F, top_k=1, experts=without, expert_bias=False).experts.expert_bias
    with pytest.raises(ValueError) as e:
        Block(E, H, F, top_k=1, experts=with_bias, expert_bias=False)
    assert "expert_bias" in str(e.value)
    with pytest.raises(ValueError):
        Block(E, H, F, top_k=1, experts=without, expert_bias=True)
    # the shared expert the block builds carries none
    s = Block(E, H, F, top_k=1, expert_bias=True, shared_ffn_dim=64)
    assert not s.shared_experts.expert_bias


def test_sparse_block_from_weights_and_router_logits():
    g, u, d = weights()
    gb, ub, db = biases()
    torch.manual_seed(3)
    gw, rb = torch.randn(E, H), torch.randn(E)
    b = fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1, router_bias=rb, gate_bias=gb, up_bias=ub, down_bias=db)
    assert torch.equal(b.gate.bias, rb) and b.experts.expert_bias
    assert torch.equal(b.experts.down_bias[1], db[1])
    x = torch.randn(5, H)
    assert torch.equal(b.router_logits(x), torch.nn.functional.linear(x, gw, rb))
    plain = fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1)
    assert plain.gate.bias is None and torch.equal(plain.router_logits(x), torch.nn.functional.linear(x, gw))
    with pytest.raises(ValueError):
        fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1, router_bias=torch.randn(E + 1))
    with pytest.raises(ValueError):
        fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1, gate_bias=gb)


def test_extra_repr():
    assert "expert_bias" not in repr(fq().QuantizedMoEFFN(E, H, F))
    assert "expert_bias=True" in fq().QuantizedMoEFFN(E, H, F, expert_bias=True).extra_repr()
    m = fq().QuantizedMoEFFN(E, H, F, expert_bias=True, activation="swiglu_clamp")
    assert "activation=swiglu_clamp" in m.extra_repr() and "expert_bias=True" in m.extra_repr()
    assert "expert_bias=True" in fq().LoRAQuantizedMoEFFN(E, H, F, rank=4, expert_bias=True).extra_repr()
    r = fq().QuantizedSparseMoEBlock(E, H, F, top_k=1, expert_bias=True, router_bias=True).extra_repr()
    assert "expert_bias=True" in r and "router_bias=True" in r
    r = fq().QuantizedSparseMoEBlock(E, H, F, top_k=1).extra_repr()
    assert "expert_bias" not in r and "router_bias" not in r


def test_ops_refuse_host_tensors():
    o = ops()
    with pytest.raises(RuntimeError):
        o.moe_bias_grad(torch.randn(4, 8), 2, torch.tensor([2, 2]), torch.tensor([0, 2]))
    with pytest.raises(RuntimeError):
        o.moe_forward(torch.zeros(2, 8, 16, dtype=torch.uint8), torch.ones(2, 8), torch.zeros(2, 8), torch.randn(4, 32), None,
                      torch.tensor([2, 2]), torch.tensor([0, 2]), bias=torch.zeros(2, 8))
