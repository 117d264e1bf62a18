"""LoRAQuantizedMoEFFN on the CPU: surface, parameters, state_dict, PEFT initialisation (the forward is GPU only)."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401

ADAPTERS = ["down_lora_A", "down_lora_B", "gate_up_lora_A", "gate_up_lora_B"]


def fq():
    import fused_int4_amd
    return fused_int4_amd


def _base(E=3, H=64, F=96, seed=0):
    torch.manual_seed(seed)
    return fq().QuantizedMoEFFN.from_weights([torch.randn(F, H) * 0.1 for _ in range(E)],
                                             [torch.randn(F, H) * 0.1 for _ in range(E)],
                                             [torch.randn(H, F) * 0.1 for _ in range(E)])


def test_exported():
    assert "LoRAQuantizedMoEFFN" in fq().__all__
    assert issubclass(fq().LoRAQuantizedMoEFFN, fq().QuantizedMoEFFN)
    from fused_int4_amd import ops
    for name in ("lora_gated_shrink", "lora_gated_grad", "swiglu_backward", "moe_ffn_lora_forward"):
        assert callable(getattr(ops, name)), name


def test_parameters_are_exactly_the_adapters():
    m = fq().LoRAQuantizedMoEFFN(4, 64, 96, rank=16)
    assert sorted(n for n, _ in m.named_parameters()) == ADAPTERS
    assert all(p.dtype == torch.float32 and p.requires_grad for p in m.parameters())
    assert tuple(m.gate_up_lora_A.shape) == (4, 16, 64) and tuple(m.gate_up_lora_B.shape) == (4, 192, 16)
    assert tuple(m.down_lora_A.shape) == (4, 16, 96) and tuple(m.down_lora_B.shape) == (4, 64, 16)
    assert "rank=16" in repr(m) and "alpha=16" in repr(m)


def test_state_dict_keys_and_adapter_state_dict():
    base = _base()
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, 8)
    assert set(m.state_dict()) == set(base.state_dict()) | set(ADAPTERS)
    assert sorted(m.adapter_state_dict()) == ADAPTERS
    # a base checkpoint loads with strict=False and leaves the adapters alone
    fresh = fq().LoRAQuantizedMoEFFN(3, 64, 96, rank=8)
    A = fresh.down_lora_A.detach().clone()
    res = fresh.load_state_dict(base.state_dict(), strict=False)
    assert sorted(res.missing_keys) == ADAPTERS and not res.unexpected_keys
    assert torch.equal(fresh.gate_up_packed, base.gate_up_packed) and torch.equal(fresh.down_scales, base.down_scales)
    assert torch.equal(fresh.down_lora_A, A)


def test_from_quantized_shares_buffers():
    base = _base()
    m = fq().LoRAQuantizedMoEFFN.from_quantized(base, 4, alpha=8)
    for name, buf in base.named_buffers():
        assert getattr(m, name).data_ptr() == buf.data_ptr(), name
    assert m.scaling == 2.0 and m.rank == 4 and m.precision == base.precision


def test_peft_initialisation_and_scaling():
    torch.manual_seed(0)
    m = fq().LoRAQuantizedMoEFFN(3, 256, 64, rank=16, alpha=32)
    assert m.scaling == 2.0 and fq().LoRAQuantizedMoEFFN(3, 256, 64, rank=16).scaling == 1.0
    assert torch.count_nonzero(m.gate_up_lora_B) == 0 and torch.count_nonzero(m.down_lora_B) == 0
    for A, fan_in in ((m.gate_up_lora_A, 256), (m.down_lora_A, 64)):
        bound = 1.0 / math.sqrt(fan_in)                        # kaiming_uniform(a=sqrt(5)) on the expert's fan-in
        assert A.abs().max() <= bound and A.abs().max() > 0.5 * bound
    with torch.no_grad():
        m.down_lora_B.fill_(1.0)
    m.reset_lora_parameters()
    assert torch.count_nonzero(m.down_lora_B) == 0


@pytest.mark.parametrize("bad", [0, 3, 12, 128])
def test_bad_rank_raises(bad):
    with pytest.raises(ValueError):
        fq().LoRAQuantizedMoEFFN(2, 64, 32, rank=bad)


def test_host_tensors_raise():
    m = fq().LoRAQuantizedMoEFFN.from_quantized(_base(), 4)
    tpe = torch.tensor([2, 0, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        m(torch.randn(5, 64), tpe, torch.cumsum(tpe, 0).to(torch.int32) - tpe)
    from fused_int4_amd import ops
    with pytest.raises(RuntimeError):
        ops.swiglu_backward(torch.randn(4, 64), torch.randn(4, 32))
    with pytest.raises(RuntimeError):
        ops.lora_gated_shrink(torch.randn(4, 64), torch.randn(4, 32))
