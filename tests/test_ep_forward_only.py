"""ExpertParallelMoE has no backward across ranks (nor on the GPU): an input that requires grad is refused instead of
getting a partial gradient (before, the routing weights got one and x silently none).  CPU, gloo, world size 2."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_ep_gloo import _expert_fn_factory, _make_problem


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from fused_int4_amd.ep import ExpertParallelMoE
        E, N = 4, 24
        P, S, Z, x, idx, w = _make_problem(E, 32, N, 8, 2, 3)
        fn = _expert_fn_factory(ExpertParallelMoE.shard(P, rank, world), ExpertParallelMoE.shard(S, rank, world),
                                ExpertParallelMoE.shard(Z, rank, world))
        ep = ExpertParallelMoE(E, expert_fn=fn, out_features=N)
        x, idx, w = x[4 * rank:4 * rank + 4], idx[4 * rank:4 * rank + 4], w[4 * rank:4 * rank + 4]
        refused = 0
        for xi, wi in ((x.clone().requires_grad_(), w), (x, w.clone().requires_grad_())):
            try:
                ep(xi, idx, wi)
            except RuntimeError as exc:
                refused += "no backward" in str(exc)
        with torch.no_grad():                                # inference is untouched
            y = ep(x.clone().requires_grad_(), idx, w.clone().requires_grad_())
        ret[rank] = (refused, tuple(y.shape), y.requires_grad)
    finally:
        dist.destroy_process_group()


def test_requires_grad_is_refused_across_ranks():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for rank in range(world):
        assert ret[rank] == (2, (4, 24), False), ret[rank]


def test_single_cpu_rank_still_differentiates():
    from fused_int4_amd.ep import ExpertParallelMoE
    P, S, Z, x, idx, w = _make_problem(4, 32, 24, 10, 2, 5)
    ep = ExpertParallelMoE(4, expert_fn=_expert_fn_factory(P, S, Z), out_features=24)
    x = x.clone().requires_grad_()
    ep(x, idx, w).sum().backward()
    assert x.grad is not None and x.grad.abs().sum() > 0
