"""The routing settings of QuantizedSparseMoEBlock (scoring, groups, scaling factor, selection bias) without a GPU:
construction, state-dict keys, from_weights, repr, refusals."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

EXPERT_KEYS = {"experts.gate_up_packed", "experts.gate_up_scales", "experts.gate_up_zero_points",
               "experts.down_packed", "experts.down_scales", "experts.down_zero_points"}
BIAS_KEY = "gate.e_score_correction_bias"


@pytest.fixture(scope="module")
def fq():
    import fused_int4_amd
    return fused_int4_amd


def test_construction_with_the_new_arguments(fq):
    m = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid", n_group=4, topk_group=2, group_top=1,
                                   routed_scaling_factor=2.5, selection_bias=True)
    assert (m.scoring, m.n_group, m.topk_group, m.group_top, m.routed_scaling_factor) == ("sigmoid", 4, 2, 1, 2.5)
    assert m.scored_routing
    b = m.selection_bias
    assert b is m.gate.e_score_correction_bias and b.shape == (8,) and b.dtype == torch.float32
    assert torch.equal(b, torch.zeros(8)) and not b.requires_grad
    assert [n for n, _ in m.named_parameters()] == ["gate.weight"]           # a buffer, not a parameter
    assert set(m.state_dict()) == {"gate.weight", BIAS_KEY} | EXPERT_KEYS
    d = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2)
    assert (d.scoring, d.n_group, d.topk_group, d.group_top, d.routed_scaling_factor) == ("softmax", 1, 1, 2, 1.0)
    assert d.selection_bias is None and not d.scored_routing


@pytest.mark.parametrize("kwargs", [dict(scoring="sigmoid"), dict(n_group=4, topk_group=2), dict(routed_scaling_factor=2.5),
                                    dict(scoring="sigmoid", n_group=2, topk_group=1, group_top=1)],
                         ids=["sigmoid", "groups", "scale", "all"])
def test_keys_are_the_old_keys_without_a_bias(fq, kwargs):
    m = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, **kwargs)
    assert set(m.state_dict()) == {"gate.weight"} | EXPERT_KEYS
    assert m.selection_bias is None and m.scored_routing


def test_bias_round_trips_through_the_state_dict(fq):
    a = fq.QuantizedSparseMoEBlock(4, 64, 32, top_k=2, scoring="sigmoid", selection_bias=True)
    with torch.no_grad():
        a.selection_bias.copy_(torch.tensor([0.5, -1.0, 0.25, 2.0]))
    b = fq.QuantizedSparseMoEBlock(4, 64, 32, top_k=2, scoring="sigmoid", selection_bias=True)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.selection_bias, a.selection_bias)
    with pytest.raises(RuntimeError):                                         # the plain block has no such key
        fq.QuantizedSparseMoEBlock(4, 64, 32, top_k=2).load_state_dict(a.state_dict())


def test_from_weights_passes_the_arguments_through(fq):
    g = torch.Generator().manual_seed(3)
    E, H, F = 4, 64, 32
    gate_w = torch.randn(E, H, generator=g)
    gate = [torch.randn(F, H, generator=g) for _ in range(E)]
    up = [torch.randn(F, H, generator=g) for _ in range(E)]
    down = [torch.randn(H, F, generator=g) for _ in range(E)]
    m = fq.QuantizedSparseMoEBlock.from_weights(gate_w, gate, up, down, top_k=2, renormalize=False, scoring="sigmoid",
                                                n_group=2, topk_group=1, group_top=1, routed_scaling_factor=1.5,
                                                selection_bias=True)
    assert (m.scoring, m.n_group, m.topk_group, m.group_top, m.routed_scaling_factor, m.renormalize) == \
        ("sigmoid", 2, 1, 1, 1.5, False)
    assert set(m.state_dict()) == {"gate.weight", BIAS_KEY} | EXPERT_KEYS
    assert torch.equal(m.state_dict()["gate.weight"], gate_w)
    plain = fq.QuantizedSparseMoEBlock.from_weights(gate_w, gate, up, down, top_k=2)
    assert set(plain.state_dict()) == {"gate.weight"} | EXPERT_KEYS and not plain.scored_routing


def test_repr_shows_only_what_differs(fq):
    base = "num_experts=8, hidden_dim=64, top_k=2, renormalize=True"
    assert fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2).extra_repr() == base
    m = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid", n_group=4, topk_group=2, routed_scaling_factor=2.5,
                                   selection_bias=True)
    r = m.extra_repr()
    assert r.startswith(base)
    for piece in ("scoring=sigmoid", "n_group=4", "topk_group=2", "group_top=2", "routed_scaling_factor=2.5",
                  "selection_bias=True"):
        assert piece in r, piece
    assert "n_group" not in fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid").extra_repr()


@pytest.mark.parametrize("kwargs", [
    dict(scoring="tanh"), dict(scoring=None), dict(n_group=0), dict(n_group=3), dict(n_group=16, topk_group=1),
    dict(n_group=4, topk_group=0), dict(n_group=4, topk_group=5), dict(n_group=8, topk_group=1),
    dict(group_top=0), dict(group_top=3), dict(routed_scaling_factor=float("inf")), dict(routed_scaling_factor=float("nan")),
], ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_bad_settings_raise_at_construction(fq, kwargs):
    with pytest.raises(ValueError):
        fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, **kwargs)           # (n_group=8, topk_group=1: one expert < top_k)
    fq.QuantizedSparseMoEBlock(16, 64, 96, top_k=2, n_group=8, topk_group=1)


def test_cpu_tensors_raise(fq):
    from fused_int4_amd import ops
    m = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid", n_group=4, topk_group=2, selection_bias=True)
    with pytest.raises(RuntimeError):
        m(torch.randn(5, 64))
    with pytest.raises(RuntimeError):
        ops.router_score_topk(torch.randn(5, 8), 2, scoring="sigmoid")
    with pytest.raises(RuntimeError):
        ops.router_score_topk(torch.randn(5, 8, requires_grad=True), 2, scoring="sigmoid", select_bias=torch.zeros(8))
    with pytest.raises(RuntimeError):
        ops.router_score_topk_backward(torch.randn(5, 8), torch.zeros(5, 2, dtype=torch.int32), torch.randn(5, 2), None,
                                       scoring="sigmoid")


def test_update_selection_bias_needs_a_buffer_and_a_forward(fq):
    with pytest.raises(RuntimeError):
        fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid").update_selection_bias(0.01)
    m = fq.QuantizedSparseMoEBlock(8, 64, 96, top_k=2, scoring="sigmoid", selection_bias=True)
    with pytest.raises(RuntimeError):
        m.update_selection_bias(0.01)
    m.routing = (None, torch.tensor([5, 0, 1, 1, 1, 0, 0, 0], dtype=torch.int32), None)   # the counts a forward would keep
    m.update_selection_bias(0.01)
    assert torch.equal(m.selection_bias, torch.tensor([-0.01, 0.01, 0.0, 0.0, 0.0, 0.01, 0.01, 0.01]))
