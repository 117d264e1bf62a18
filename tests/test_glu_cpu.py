"""The activation kinds of the gated FFN layers on the CPU: argument checks, the alias, state-dict neutrality, the
sparse block's conflict rule and extra_repr (the forward is GPU only)."""
import pytest
import torch

from conftest import ROOT  # noqa: F401

INF, NAN = float("inf"), float("nan")


def fq():
    import fused_int4_amd
    return fused_int4_amd


def ops():
    from fused_int4_amd import ops as o
    return o


def weights(E=2, H=64, F=96, seed=0):
    torch.manual_seed(seed)
    return ([torch.randn(F, H) * 0.1 for _ in range(E)], [torch.randn(F, H) * 0.1 for _ in range(E)],
            [torch.randn(H, F) * 0.1 for _ in range(E)])


def test_activation_of():
    o = ops()
    assert tuple(o.ACTIVATIONS) == ("silu", "gelu_tanh", "swiglu_clamp")
    assert o.activation_of() == ("silu", 1.702, 7.0)
    assert o.activation_of("gelu_pytorch_tanh")[0] == "gelu_tanh"
    assert o.activation_of("swiglu_clamp", 2, 5) == ("swiglu_clamp", 2.0, 5.0)
    for bad in ("gelu", "relu2", "SILU", "", None, 1):
        with pytest.raises(ValueError) as e:
            o.activation_of(bad)
        for kind in o.ACTIVATIONS:
            assert kind in str(e.value)
    for alpha in (INF, -INF, NAN, "x"):
        with pytest.raises(ValueError):
            o.activation_of("swiglu_clamp", alpha, 7.0)
    for limit in (0.0, -1.0, INF, NAN, None):
        with pytest.raises(ValueError):
            o.activation_of("swiglu_clamp", 1.702, limit)


def test_ops_check_the_activation_before_anything_else():
    o = ops()
    gu, w, v, dh = torch.randn(4, 64), torch.randn(4, 32), torch.randn(4, 4), torch.randn(4, 32)
    with pytest.raises(ValueError):
        o.lora_gated_shrink(gu, w, activation="gelu")
    with pytest.raises(ValueError):
        o.lora_gated_grad(gu, v, "rc", activation="swiglu_clamp", activation_limit=0.0)
    with pytest.raises(ValueError):
        o.glu_backward(gu, dh, activation="swiglu_clamp", activation_alpha=NAN)
    with pytest.raises(ValueError):
        o.moe_gated_forward(None, None, None, gu, None, None, activation="tanh")
    with pytest.raises(RuntimeError):                          # a valid kind: the usual refusal of a host tensor
        o.glu_backward(gu, dh, activation="gelu_tanh")
    with pytest.raises(RuntimeError):
        o.lora_gated_shrink(gu, w, activation="swiglu_clamp")


@pytest.mark.parametrize("cls", ["QuantizedMoEFFN", "LoRAQuantizedMoEFFN"])
def test_constructor_validation(cls):
    make = (lambda **kw: fq().QuantizedMoEFFN(2, 64, 96, **kw)) if cls == "QuantizedMoEFFN" else \
        (lambda **kw: fq().LoRAQuantizedMoEFFN(2, 64, 96, rank=4, **kw))
    m = make()
    assert m.activation_args == ("silu", 1.702, 7.0)
    m = make(activation="gelu_pytorch_tanh")
    assert m.activation == "gelu_tanh"
    m = make(activation="swiglu_clamp", activation_alpha=1.5, activation_limit=6)
    assert m.activation_args == ("swiglu_clamp", 1.5, 6.0)
    for kw in (dict(activation="gelu"), dict(activation="swiglu_clamp", activation_limit=0.0),
               dict(activation="swiglu_clamp", activation_limit=INF), dict(activation="swiglu_clamp", activation_alpha=NAN),
               dict(activation="gelu_tanh", activation_alpha=INF)):
        with pytest.raises(ValueError):
            make(**kw)


def test_from_weights_and_from_quantized():
    g, u, d = weights()
    with pytest.raises(ValueError):
        fq().QuantizedMoEFFN.from_weights(g, u, d, activation="erf")
    base = fq().QuantizedMoEFFN.from_weights(g, u, d, activation="swiglu_clamp", activation_alpha=1.25, activation_limit=5.0)
    assert base.activation_args == ("swiglu_clamp", 1.25, 5.0)
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, 8)
    assert m.activation_args == base.activation_args
    assert fq().LoRAQuantizedMoEFFN.from_quantized(fq().QuantizedMoEFFN.from_weights(g, u, d), 8).activation == "silu"


def test_state_dict_is_that_of_a_default_layer():
    g, u, d = weights()
    default = fq().QuantizedMoEFFN.from_weights(g, u, d)
    for kw in (dict(activation="gelu_tanh"), dict(activation="swiglu_clamp", activation_alpha=1.0, activation_limit=3.0)):
        m = fq().QuantizedMoEFFN.from_weights(g, u, d, **kw)
        a, b = default.state_dict(), m.state_dict()
        assert list(a) == list(b)
        assert all(torch.equal(a[k], b[k]) for k in a)
        default.load_state_dict(b)                               # either way round, strictly
        m.load_state_dict(a)
        assert m.activation == kw["activation"]
        lora_default = fq().LoRAQuantizedMoEFFN.from_quantized(default, 4)
        assert list(fq().LoRAQuantizedMoEFFN.from_quantized(m, 4).state_dict()) == list(lora_default.state_dict())
    gw = torch.randn(2, 64)
    blk = fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1, shared=(g[0], u[0], d[0]))
    blk_g = fq().QuantizedSparseMoEBlock.from_weights(gw, g, u, d, top_k=1, shared=(g[0], u[0], d[0]),
                                                       activation="gelu_tanh")
    assert list(blk.state_dict()) == list(blk_g.state_dict())
    assert all(torch.equal(v, blk_g.state_dict()[k]) for k, v in blk.state_dict().items())


def test_block_forwards_the_activation_to_what_it_builds():
    blk = fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2, shared_ffn_dim=32, activation="swiglu_clamp",
                                       activation_alpha=1.5, activation_limit=6.0)
    assert blk.experts.activation_args == ("swiglu_clamp", 1.5, 6.0)
    assert blk.shared_experts.activation_args == ("swiglu_clamp", 1.5, 6.0)
    blk = fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2, shared_ffn_dim=32)
    assert blk.experts.activation == "silu" and blk.shared_experts.activation == "silu"
    g, u, d = weights(E=4)
    blk = fq().QuantizedSparseMoEBlock.from_weights(torch.randn(4, 64), g, u, d, shared=(g[0], u[0], d[0]),
                                                     activation="gelu_pytorch_tanh")
    assert blk.experts.activation == "gelu_tanh" and blk.shared_experts.activation == "gelu_tanh"
    with pytest.raises(ValueError):
        fq().QuantizedSparseMoEBlock(4, 64, 96, activation="gelu")


def test_block_conflict_rule():
    B = fq().QuantizedSparseMoEBlock
    gelu = fq().QuantizedMoEFFN(4, 64, 96, activation="gelu_tanh")
    shared_silu = fq().QuantizedMoEFFN(1, 64, 32)
    clamp = fq().QuantizedMoEFFN(4, 64, 96, activation="swiglu_clamp", activation_alpha=1.5)
    # a passed-in module keeps its own activation
    blk = B(4, 64, 96, experts=gelu, shared_experts=shared_silu)
    assert blk.experts.activation == "gelu_tanh" and blk.shared_experts.activation == "silu"
    assert B(4, 64, 96, experts=gelu, activation="gelu_pytorch_tanh").experts is gelu       # agreeing is fine
    assert B(4, 64, 96, experts=clamp, activation="swiglu_clamp", activation_alpha=1.5).experts is clamp
    # an explicit argument that contradicts it raises
    with pytest.raises(ValueError):
        B(4, 64, 96, experts=gelu, activation="silu")
    with pytest.raises(ValueError):
        B(4, 64, 96, experts=gelu, activation="swiglu_clamp")
    with pytest.raises(ValueError):
        B(4, 64, 96, shared_experts=shared_silu, activation="gelu_tanh")
    with pytest.raises(ValueError):
        B(4, 64, 96, experts=clamp, activation_alpha=1.702)
    with pytest.raises(ValueError):
        B(4, 64, 96, experts=clamp, activation="swiglu_clamp", activation_alpha=1.5, activation_limit=5.0)
    # a built shared expert takes the block's argument even next to passed-in experts
    blk = B(4, 64, 96, experts=gelu, activation="gelu_tanh", shared_ffn_dim=32)
    assert blk.shared_experts.activation == "gelu_tanh"


def test_extra_repr_shows_a_non_default_kind():
    assert "activation" not in repr(fq().QuantizedMoEFFN(2, 64, 96))
    assert "activation" not in repr(fq().LoRAQuantizedMoEFFN(2, 64, 96, rank=4))
    assert "activation" not in repr(fq().QuantizedSparseMoEBlock(2, 64, 96, top_k=1))
    assert "activation=gelu_tanh" in repr(fq().QuantizedMoEFFN(2, 64, 96, activation="gelu_tanh"))
    r = repr(fq().LoRAQuantizedMoEFFN(2, 64, 96, rank=4, activation="swiglu_clamp", activation_limit=5.0))
    assert "rank=4" in r and "activation=swiglu_clamp" in r and "activation_alpha=1.702" in r and "activation_limit=5" in r
    r = fq().QuantizedSparseMoEBlock(2, 64, 96, top_k=1, activation="gelu_tanh").extra_repr()
    assert "top_k=1" in r and "activation=gelu_tanh" in r
