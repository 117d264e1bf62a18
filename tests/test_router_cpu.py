"""QuantizedSparseMoEBlock without a GPU: export, construction, state-dict keys, from_weights, refusals."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

EXPERT_KEYS = {"experts.gate_up_packed", "experts.gate_up_scales", "experts.gate_up_zero_points",
               "experts.down_packed", "experts.down_scales", "experts.down_zero_points"}
LORA_KEYS = {"experts.gate_up_lora_A", "experts.gate_up_lora_B", "experts.down_lora_A", "experts.down_lora_B"}


@pytest.fixture(scope="module")
def fq():
    import fused_int4_amd
    return fused_int4_amd


def test_exported(fq):
    assert "QuantizedSparseMoEBlock" in fq.__all__
    assert fq.QuantizedSparseMoEBlock is fq.moe.QuantizedSparseMoEBlock


def test_construction_and_keys(fq):
    m = fq.QuantizedSparseMoEBlock(4, 64, 96, top_k=2)
    assert set(m.state_dict()) == {"gate.weight"} | EXPERT_KEYS
    assert m.gate.weight.shape == (4, 64) and m.gate.weight.dtype == torch.float32 and m.gate.weight.requires_grad
    assert m.gate.bias is None
    assert isinstance(m.experts, fq.QuantizedMoEFFN) and m.experts.activation_dtype is None
    assert [n for n, _ in m.named_parameters()] == ["gate.weight"]
    assert (m.top_k, m.renormalize, m.num_experts, m.hidden_dim, m.ffn_dim) == (2, True, 4, 64, 96)
    m16 = fq.QuantizedSparseMoEBlock(4, 64, 96, top_k=1, activation_dtype=torch.bfloat16, renormalize=False)
    assert m16.experts.activation_dtype == torch.bfloat16 and m16.renormalize is False


def test_lora_experts_are_taken(fq):
    experts = fq.LoRAQuantizedMoEFFN(4, 64, 96, rank=8)
    m = fq.QuantizedSparseMoEBlock(4, 64, 96, top_k=2, experts=experts)
    assert m.experts is experts
    assert set(m.state_dict()) == {"gate.weight"} | EXPERT_KEYS | LORA_KEYS
    with pytest.raises(ValueError):
        fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, experts=experts)


def test_from_weights(fq):
    g = torch.Generator().manual_seed(3)
    E, H, F = 3, 64, 32
    gate_w = torch.randn(E, H, generator=g)
    gate = [torch.randn(F, H, generator=g) for _ in range(E)]
    up = [torch.randn(F, H, generator=g) for _ in range(E)]
    down = [torch.randn(H, F, generator=g) for _ in range(E)]
    m = fq.QuantizedSparseMoEBlock.from_weights(gate_w, gate, up, down, top_k=2, renormalize=False)
    sd = m.state_dict()
    assert set(sd) == {"gate.weight"} | EXPERT_KEYS
    assert torch.equal(sd["gate.weight"], gate_w)
    assert sd["experts.gate_up_packed"].shape == (E, 2 * F, H // 2) and sd["experts.gate_up_packed"].dtype == torch.uint8
    assert sd["experts.gate_up_scales"].shape == (E, 2 * F) and sd["experts.gate_up_zero_points"].shape == (E, 2 * F)
    assert sd["experts.down_packed"].shape == (E, H, F // 2)
    assert sd["experts.down_scales"].shape == (E, H) and sd["experts.down_zero_points"].shape == (E, H)
    assert (m.num_experts, m.hidden_dim, m.ffn_dim, m.top_k, m.renormalize) == (E, H, F, 2, False)
    ref = fq.QuantizedMoEFFN.from_weights(gate, up, down)
    for k, v in ref.state_dict().items():
        assert torch.equal(sd["experts." + k], v), k
    with pytest.raises(ValueError):
        fq.QuantizedSparseMoEBlock.from_weights(torch.randn(E + 1, H), gate, up, down)


def test_cpu_forward_raises(fq):
    m = fq.QuantizedSparseMoEBlock(4, 64, 96, top_k=2)
    with pytest.raises(RuntimeError):
        m(torch.randn(5, 64))
    from fused_int4_amd import ops
    with pytest.raises(RuntimeError):
        ops.router_topk(torch.randn(5, 4), 2)


@pytest.mark.parametrize("E,top_k", [(4, 5), (16, 9), (129, 2), (4, 0), (0, 1)])
def test_limits_raise_at_construction(fq, E, top_k):
    with pytest.raises(ValueError):
        fq.QuantizedSparseMoEBlock(E, 64, 96, top_k=top_k)
