"""LoRA modules on the CPU: surface, parameters, state_dict, PEFT initialisation and gradients against float64 autograd."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401


def fq():
    import fused_int4_amd
    return fused_int4_amd


def _layer(K=64, N=48, r=8, alpha=None, bias=False, group_size=None, seed=0):
    torch.manual_seed(seed)
    base = fq().QuantizedLinear.from_linear(torch.nn.Linear(K, N, bias=bias), group_size=group_size)
    return base, fq().LoRAQuantizedLinear.from_quantized(base, r, alpha)


def test_exported():
    assert "LoRAQuantizedLinear" in fq().__all__ and "LoRAMoEINT4" in fq().__all__
    from fused_int4_amd import ops
    for name in ("lora_shrink", "lora_expand", "lora_grad", "linear_lora_forward", "moe_lora_forward"):
        assert callable(getattr(ops, name)), name


def test_parameters_are_exactly_the_adapters():
    _, m = _layer(bias=True)
    names = [n for n, _ in m.named_parameters()]
    assert sorted(names) == ["lora_A", "lora_B"]
    assert all(p.dtype == torch.float32 and p.requires_grad for p in m.parameters())
    moe = fq().LoRAMoEINT4(4, 64, 96, rank=16)
    assert sorted(n for n, _ in moe.named_parameters()) == ["lora_A", "lora_B"]
    assert tuple(moe.lora_A.shape) == (4, 16, 64) and tuple(moe.lora_B.shape) == (4, 96, 16)


def test_state_dict_keys_and_adapter_state_dict():
    base, m = _layer(K=64, N=48, r=4, bias=True)
    assert set(m.state_dict()) == set(base.state_dict()) | {"lora_A", "lora_B"}
    assert set(m.adapter_state_dict()) == {"lora_A", "lora_B"}
    assert tuple(m.state_dict()["lora_A"].shape) == (4, 64) and tuple(m.state_dict()["lora_B"].shape) == (48, 4)
    # a base checkpoint loads with strict=False and leaves the adapters alone
    fresh = fq().LoRAQuantizedLinear(64, 48, rank=4, bias=True)
    A = fresh.lora_A.detach().clone()
    res = fresh.load_state_dict(base.state_dict(), strict=False)
    assert sorted(res.missing_keys) == ["lora_A", "lora_B"] and not res.unexpected_keys
    assert torch.equal(fresh.packed_weights, base.packed_weights) and torch.equal(fresh.lora_A, A)
    moe = fq().LoRAMoEINT4(2, 64, 32, rank=8)
    assert set(moe.state_dict()) == set(fq().MoEINT4(2, 64, 32).state_dict()) | {"lora_A", "lora_B"}


def test_from_quantized_shares_buffers():
    base, m = _layer()
    assert m.packed_weights is base.packed_weights and m.scales is base.scales
    assert m.zero_points is base.zero_points
    moe_base = fq().MoEINT4(2, 64, 32)
    moe = fq().LoRAMoEINT4.from_quantized(moe_base, 4, alpha=8)
    assert moe.packed_weights is moe_base.packed_weights and moe.scaling == 2.0


def test_peft_initialisation_and_scaling():
    torch.manual_seed(0)
    m = fq().LoRAQuantizedLinear(256, 64, rank=16, alpha=32)
    assert m.scaling == 2.0 and fq().LoRAQuantizedLinear(256, 64, rank=16).scaling == 1.0
    assert torch.count_nonzero(m.lora_B) == 0
    bound = 1.0 / math.sqrt(256)                               # kaiming_uniform(a=sqrt(5)) on fan_in = K
    assert m.lora_A.abs().max() <= bound and m.lora_A.abs().max() > 0.5 * bound
    moe = fq().LoRAMoEINT4(3, 256, 64, rank=8)
    assert moe.lora_A.abs().max() <= bound and torch.count_nonzero(moe.lora_B) == 0


@pytest.mark.parametrize("bad", [0, 3, 12, 128])
def test_bad_rank_raises(bad):
    with pytest.raises(ValueError):
        fq().LoRAQuantizedLinear(64, 32, rank=bad)
    with pytest.raises(ValueError):
        fq().LoRAMoEINT4(2, 64, 32, rank=bad)


@pytest.mark.parametrize("bias,group_size", [(False, None), (True, None), (False, 32)])
def test_zero_B_returns_the_base_output(bias, group_size):
    base, m = _layer(K=128, N=40, r=8, bias=bias, group_size=group_size)
    x = torch.randn(5, 128)
    assert torch.equal(m(x), base(x))
    assert torch.equal(m(x[0]), base(x[0]))


@pytest.mark.parametrize("bias", [False, True])
def test_cpu_gradients_against_float64(bias):
    base, m = _layer(K=96, N=40, r=8, alpha=16, bias=bias, seed=3)
    torch.manual_seed(4)
    with torch.no_grad():
        m.lora_B.normal_()
    x = torch.randn(7, 96, requires_grad=True)
    gy = torch.randn(7, 40)
    m(x).backward(gy)

    W = fq().dequantize_weights(base.packed_weights, base.scales, base.zero_points).double()
    x64 = x.detach().double().requires_grad_()
    A64 = m.lora_A.detach().double().requires_grad_()
    B64 = m.lora_B.detach().double().requires_grad_()
    y64 = x64 @ W.t() + 2.0 * (x64 @ A64.t()) @ B64.t()
    y64.backward(gy.double())
    for got, ref in ((x.grad, x64.grad), (m.lora_A.grad, A64.grad), (m.lora_B.grad, B64.grad)):
        assert (got.double() - ref).norm() / ref.norm() < 1e-5


def test_adamw_trains_only_the_adapters():
    base, m = _layer(K=64, N=32, r=4)
    before = {k: v.clone() for k, v in base.state_dict().items()}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    x = torch.randn(16, 64)
    for _ in range(3):
        opt.zero_grad()
        m(x).square().mean().backward()
        opt.step()
    assert torch.count_nonzero(m.lora_B) > 0
    for k, v in base.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_moe_lora_is_gpu_only():
    moe = fq().LoRAMoEINT4(2, 64, 32, rank=4)
    counts = torch.tensor([3, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        moe(torch.randn(5, 64), None, counts, torch.tensor([0, 3], dtype=torch.int32))
