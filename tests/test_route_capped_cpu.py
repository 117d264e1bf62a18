"""Expert capacity and the token mask without a GPU: the constructor's checks, ``aux_loss`` with and without a mask
against the formula written out in float64, and ``plan_reference``: a torch restatement of
``fql_route_plan_capped_i32`` (stable argsort, per-expert rank, cap, mask) that tests/test_gpu_route_capped.py imports."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


def fq():
    import fused_int4_amd
    return fused_int4_amd


def plan_reference(expert_indices, num_experts, capacity=None, token_mask=None):
    """``(counts, offsets, token_of_sorted, pos_of_slot, demand)`` int32, on ``expert_indices``' device, as
    include/fql_int4.h states them for fql_route_plan_capped_i32.  A stable argsort puts the eligible slots of an expert
    in ascending slot order; a slot's rank in its expert is its sorted position minus the expert's first; it is kept when
    that rank is below the capacity."""
    T, top_k = expert_indices.shape
    dev = expert_indices.device
    n = T * top_k
    e = expert_indices.reshape(-1).long().clamp(0, num_experts - 1)
    eligible = torch.ones(n, dtype=torch.bool, device=dev)
    if token_mask is not None:
        eligible = token_mask.reshape(-1).to(dev).ne(0).repeat_interleave(top_k)
    key = torch.where(eligible, e, torch.full_like(e, num_experts))          # the ineligible slots go behind every expert
    order = torch.sort(key, stable=True).indices
    demand = torch.bincount(key, minlength=num_experts + 1)[:num_experts]
    first = torch.cumsum(demand, 0) - demand                                  # an expert's first position in `order`
    rank = torch.empty(n, dtype=torch.long, device=dev)
    rank[order] = torch.arange(n, device=dev) - torch.cat((first, first.new_zeros(1)))[key[order]]
    kept = eligible & (rank < (capacity if capacity is not None else n + 1))
    counts = demand.clamp(max=capacity) if capacity is not None else demand.clone()
    offsets = torch.cumsum(counts, 0) - counts
    pos = torch.where(kept, offsets[e] + rank, torch.full_like(rank, -1))
    token_of_sorted = torch.zeros(n, dtype=torch.long, device=dev)
    slots = torch.arange(n, device=dev)
    token_of_sorted[pos[kept]] = slots[kept] // top_k
    to32 = lambda t: t.to(torch.int32)
    return to32(counts), to32(offsets), to32(token_of_sorted), to32(pos), to32(demand)


def test_plan_reference_on_a_case_worked_by_hand():
    idx = torch.tensor([[0, 1], [0, 2], [0, 1], [9, -4]])                     # the last token's ids are clamped to 2 and 0
    counts, offsets, tos, pos, demand = plan_reference(idx, 3)
    assert demand.tolist() == [4, 2, 2] and counts.tolist() == [4, 2, 2] and offsets.tolist() == [0, 4, 6]
    assert pos.tolist() == [0, 4, 1, 6, 2, 5, 7, 3] and tos.tolist() == [0, 1, 2, 3, 0, 2, 1, 3]
    counts, offsets, tos, pos, demand = plan_reference(idx, 3, capacity=2)
    assert demand.tolist() == [4, 2, 2] and counts.tolist() == [2, 2, 2] and offsets.tolist() == [0, 2, 4]
    assert pos.tolist() == [0, 2, 1, 4, -1, 3, 5, -1] and tos.tolist() == [0, 1, 0, 2, 1, 3, 0, 0]
    mask = torch.tensor([True, False, True, True])
    counts, offsets, tos, pos, demand = plan_reference(idx, 3, capacity=2, token_mask=mask)
    assert demand.tolist() == [3, 2, 1] and counts.tolist() == [2, 2, 1] and offsets.tolist() == [0, 2, 4]
    assert pos.tolist() == [0, 2, -1, -1, 1, 3, 4, -1] and tos.tolist() == [0, 2, 0, 2, 3, 0, 0, 0]
    counts, _, tos, pos, demand = plan_reference(idx, 3, token_mask=torch.zeros(4, dtype=torch.uint8))
    assert demand.tolist() == [0, 0, 0] and counts.tolist() == [0, 0, 0] and set(pos.tolist()) == {-1} and not tos.any()


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("-inf"), float("nan"), "much"])
def test_constructor_refuses_a_bad_capacity_factor(bad):
    with pytest.raises(ValueError, match="capacity_factor"):
        fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2, capacity_factor=bad)


def test_constructor_keeps_the_factor_and_the_state_dict():
    plain = fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2)
    m = fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2, capacity_factor=1.25)
    assert plain.capacity_factor is None and m.capacity_factor == 1.25
    assert set(m.state_dict()) == set(plain.state_dict())
    assert "capacity_factor=1.25" in m.extra_repr() and "capacity_factor" not in plain.extra_repr()
    assert plain.kept_per_expert is None and plain.routing is None
    assert plain.expert_capacity(64) is None
    for T in (1, 64, 130):
        assert m.expert_capacity(T) == math.ceil(1.25 * T * 2 / 4)
    assert fq().QuantizedSparseMoEBlock(8, 64, 96, top_k=1, capacity_factor=0.5).expert_capacity(1) == 1


def test_forward_and_the_ops_refuse_cpu_tensors():
    m = fq().QuantizedSparseMoEBlock(4, 64, 96, top_k=2, capacity_factor=1.0)
    with pytest.raises(RuntimeError):
        m(torch.zeros(3, 64), token_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        fq().ops.route_plan_capped(torch.zeros(3, 2, dtype=torch.int32), 4, capacity=2)


def _probs_and_demand(scoring, seed=3, T=37, E=8):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, E, generator=g)
    probs = torch.softmax(z, dim=-1) if scoring == "softmax" else torch.sigmoid(z)
    demand = torch.randint(0, 9, (E,), generator=g, dtype=torch.int32)
    mask = torch.rand(T, generator=g) < 0.6
    mask[0], mask[1] = True, False
    return probs, demand, mask


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_aux_loss_with_a_mask_is_the_formula(scoring):
    E = 8
    m = fq().QuantizedSparseMoEBlock(E, 64, 96, top_k=2, scoring=scoring)
    probs, demand, mask = _probs_and_demand(scoring)
    got = m.aux_loss(probs, demand, token_mask=mask)
    p = probs.double()
    if scoring == "sigmoid":
        p = p / p.sum(dim=-1, keepdim=True)
    n_real = int(mask.sum())
    P = p[mask].sum(dim=0) / n_real
    f = demand.double() / n_real
    ref = E * torch.sum(f * P)
    # float32 sums of at most 37 + 8 positive terms and a handful of roundings: 64 * 2^-24 relative is generous and fixed
    assert abs(float(got) - float(ref)) <= 64 * 2.0 ** -24 * float(ref)
    assert float(m.aux_loss(probs, demand, token_mask=mask.to(torch.uint8).reshape(1, -1))) == float(got)
    # an all-true mask: n_real == T, the same value up to the order of the float32 operations
    full = m.aux_loss(probs, demand, token_mask=torch.ones_like(mask))
    assert abs(float(full) - float(m.aux_loss(probs, demand))) <= 64 * 2.0 ** -24 * float(full)
    # a masked row sends its probabilities no gradient
    pg = probs.clone().requires_grad_(True)
    m.aux_loss(pg, demand, token_mask=mask).backward()
    assert not pg.grad[~mask].any() and pg.grad[mask].abs().sum() > 0
    with pytest.raises(RuntimeError):
        m.aux_loss(probs, demand, token_mask=mask[:-1])


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_aux_loss_without_a_mask_keeps_its_bits(scoring):
    E = 8
    m = fq().QuantizedSparseMoEBlock(E, 64, 96, top_k=2, scoring=scoring, capacity_factor=2.0)
    probs, demand, _ = _probs_and_demand(scoring)
    p = probs / probs.sum(dim=-1, keepdim=True) if scoring == "sigmoid" else probs
    today = E * torch.sum((demand.to(torch.float32) / probs.shape[0]) * p.mean(dim=0))
    got = m.aux_loss(probs, demand)
    assert got.dtype == torch.float32 and got.view(torch.int32).item() == today.view(torch.int32).item()


def test_aux_loss_defaults_to_the_mask_of_the_last_forward():
    E = 8
    m = fq().QuantizedSparseMoEBlock(E, 64, 96, top_k=2)
    probs, demand, mask = _probs_and_demand("softmax")
    m.routing, m._token_mask = (probs, demand, None), mask                    # what a masked forward leaves behind
    masked = float(m.aux_loss(probs, demand, token_mask=mask))
    assert float(m.aux_loss()) == masked
    assert float(m.aux_loss(probs, demand)) == masked                        # explicit probs: the kept mask still holds
    assert float(m.aux_loss(m.routing[0])) == masked
    plain = float(m.aux_loss(probs, demand, token_mask=torch.ones_like(mask)))
    assert plain != masked                                                   # an all-true mask says "no padding"
    with pytest.raises(RuntimeError, match="token_mask"):
        m.aux_loss(probs[:-1], demand)                                       # another call's probs need that call's mask
    m._token_mask = None                                                     # what an unmasked forward leaves behind
    today = 8 * torch.sum((demand.to(torch.float32) / probs.shape[0]) * probs.mean(dim=0))
    assert m.aux_loss().view(torch.int32).item() == today.view(torch.int32).item()
