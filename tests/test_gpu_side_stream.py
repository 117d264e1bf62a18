"""The grouped ops on a stream that is not the default one.  Every other test runs on torch's current stream, which is the
default stream: there a launch, a hipMemsetAsync or a one-time set-up that goes to the null stream instead of the stream
it was given is invisible.

One case per family of tests/test_gpu_graph_replay.py, at its ragged table (S3).  On a non-default torch.cuda.Stream, with
no synchronisation in between: a few large matmuls (so that the stream is still busy when the host has enqueued the
rest), then copy_ of the real inputs over input buffers that hold NaN (the float ones) or zeros (the tables and indices: an
all-zero table is a legal one, scene S5, so a launch that reads it early computes nothing and harms nothing), then the op.
The default stream then waits for the side stream and the result must be bit for bit the default-stream result.  A launch
that went to another stream reads NaN, an empty table or unwritten memory; the test can miss such a mistake, but it cannot
fail without one.  The last test issues the same op on two side streams with different tables before synchronising
either, and checks both: what two overlapping launches must not share (a workspace, the scratch of ops.gemm_i8).

The dense ops.linear_forward_mxfp4 / linear_gated_forward_mxfp4 have no table and therefore no family: their split form
(a decode launch into a partial-sum workspace, a reduce launch, and the gated pre-pass in front of both) has a test of its
own at the end, on one side stream and on two at once; so do the dense ops.linear_forward_nvfp4 /
linear_gated_forward_nvfp4 (the grouped launchers with one expert; the gated entry's pre-pass in front of the GEMM) and
the dense adapter entries ops.linear_forward_nvfp4_lora / linear_backward_input_nvfp4_lora."""
import pytest
import torch

from helpers import first_diff, same_bits
from test_gpu_graph_replay import (DEV, FAMILIES, LINEAR_CASES, build_block, gen, linear_case, nv4_linear_case,  # noqa: F401
                                   scenes, tune)                   # (tune: the fixture)

pytestmark = pytest.mark.gpu
CASES = ["int4-small-T232-bf16", "int4-stream-T1600-f32", "int4-small-T100-fast", "int4-small-T100-fp8", "int4-gated-T100",
         "int4-gather-T232", "int4-two-phase-T100", "int4-bwd-tiled-vec", "group-i8", "group-float-glu", "group-bwd-rows-g48",
         "mx4-K288-N136-tile", "mx4-K288-N136-decode", "mx4-K96-N37-fp8", "mx4-K96-N37-fp4", "mx4-K288-N136-glu-decode",
         "mx4-K288-N136-bwd", "mx4-K288-N136-fp6-tile", "mx4-K96-N37-fp6-glu-decode", "mx4-K288-N136-fp8-decode",
         "mx4-K96-N37-fp4-decode", "mx4-lora-fwd-K288-N136-r16", "mx4-lora-glu-K96-N37-r64", "mx4-lora-bwd-K288-N136-r16",
         "nv4-K288-N136-tile", "nv4-K96-N37-decode", "nv4-K608-N37-decode", "nv4-K288-N136-glu-decode", "nv4-K96-N37-bwd",
         "nv4-lora-fwd-K288-N136-r16", "nv4-lora-glu-K96-N37-r64", "nv4-lora-bwd-K288-N136-r16"]
TWO_STREAMS = ["int4-small-T100-fast", "int4-two-phase-T100", "group-i8-glu", "mx4-K288-N136-glu-tile", "mx4-K96-N37-fp4",
               "mx4-lora-glu-K288-N136-r16", "mx4-K288-N136-fp6-decode", "nv4-K288-N136-glu-tile", "nv4-K96-N37-bwd",
               "nv4-lora-glu-K288-N136-r16", "nv4-lora-bwd-K96-N37-r64"]


def poisoned_like(t):
    """A buffer of ``t``'s shape and type full of NaN (zeros for an integer or bool tensor)."""
    return torch.full_like(t, float("nan")) if t.is_floating_point() else torch.zeros_like(t)


def enqueue(call, inputs, stream, busy):
    """On ``stream``: the busy work, the inputs copied over poisoned buffers, the call.  Nothing waits for anything."""
    buffers = [poisoned_like(t) for t in inputs]
    stream.wait_stream(torch.cuda.current_stream())                  # (the poison and the inputs are there)
    with torch.cuda.stream(stream):
        for _ in range(4):
            busy = busy @ busy
        for b, t in zip(buffers, inputs):
            b.copy_(t, non_blocking=True)
        return call(*buffers), buffers, busy


def busy_matrix():
    return torch.eye(4096, device=DEV) * 0.5 + 1e-6


def scene(fam, name):
    for n, tpe, offs, seed in scenes(fam.E, fam.T, fam.ragged):
        if n == name:
            return [*fam.make_rows(seed), tpe.to(DEV), offs.to(DEV)]


@pytest.mark.parametrize("name", CASES)
def test_op_on_a_side_stream_gives_the_default_stream_bits(tune, name):
    fam = FAMILIES[name]()
    fam.prepare(tune)
    inputs = scene(fam, "S3")
    want = fam.call(*[t.clone() for t in inputs])
    assert float(want.abs().max()) > 0
    for _ in range(2):                              # (two streams of torch's pool: they need not share a hardware queue)
        busy = busy_matrix()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        got, keep, busy = enqueue(fam.call, inputs, side, busy)
        torch.cuda.current_stream().wait_stream(side)
        assert same_bits(got, want), first_diff(got, want)
        torch.cuda.synchronize()
        del keep


@pytest.mark.parametrize("T", [3, 130])
def test_block_on_a_side_stream(T):
    m = build_block("int4-shared", True)
    x = torch.randn(T, 64, generator=gen(1, T)).to(DEV)
    mask = torch.rand(T, generator=gen(2, T)).to(DEV) < 0.75
    run = lambda x, mask: m(x, token_mask=mask)
    with torch.no_grad():
        want, want_logits = run(x.clone(), mask.clone())
        for _ in range(2):
            busy = busy_matrix()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            (got, got_logits), keep, busy = enqueue(run, [x, mask], side, busy)
            torch.cuda.current_stream().wait_stream(side)
            assert same_bits(got, want) and same_bits(got_logits, want_logits)
            torch.cuda.synchronize()


@pytest.mark.parametrize("name", TWO_STREAMS)
def test_two_side_streams_with_different_tables(tune, name):
    fam = FAMILIES[name]()
    fam.prepare(tune)
    a, b = scene(fam, "S3"), scene(fam, "S1")
    want_a, want_b = fam.call(*[t.clone() for t in a]), fam.call(*[t.clone() for t in b])
    busy_a, busy_b = busy_matrix(), busy_matrix()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got_a, keep_a, busy_a = enqueue(fam.call, a, sa, busy_a)
    got_b, keep_b, busy_b = enqueue(fam.call, b, sb, busy_b)
    torch.cuda.current_stream().wait_stream(sa)
    torch.cuda.current_stream().wait_stream(sb)
    assert same_bits(got_a, want_a), ("S3", first_diff(got_a, want_a))
    assert same_bits(got_b, want_b), ("S1", first_diff(got_b, want_b))
    assert not same_bits(want_a, want_b)
    torch.cuda.synchronize()
    del keep_a, keep_b


# ---- the dense MXFP4 linear op: the split form's two launches, and the gated entry's pre-pass in front of them

@pytest.mark.parametrize("name", list(LINEAR_CASES))
def test_dense_linear_split_form_on_side_streams(tune, name):
    """ops.linear_forward_mxfp4 / linear_gated_forward_mxfp4(split_k=True) with S forced (test_gpu_graph_replay.linear_case):
    mx4_linear_decode_kernel writes partial[S][T][N] and mx4_linear_reduce_kernel sums it, the gated entry writes h in
    front of both; the launch boundaries on ONE stream are their only synchronisation.  First on one side stream with
    poisoned input buffers, then on two side streams at once with different rows: every result carries the default-stream
    bits.  A reduce launch (or the gated pre-pass) that went to another stream than the decode kernel runs while the side
    stream is still busy with the matmuls: it sums a workspace nobody has written, or the decode kernel reads an h that
    is not there yet."""
    call, make_rows, _, _ = linear_case(name, tune)
    dense_on_side_streams(call, make_rows)


@pytest.mark.parametrize("kind", ["plain", "gated", "lora-fwd", "lora-bwd"])
def test_dense_nvfp4_linear_on_side_streams(kind):
    """ops.linear_forward_nvfp4 / linear_gated_forward_nvfp4 and the adapter entries ops.linear_forward_nvfp4_lora /
    linear_backward_input_nvfp4_lora (test_gpu_graph_replay.nv4_linear_case: K = 96, N = 37, T = 5) as the MXFP4 dense ops
    above: one side stream with poisoned input buffers, then two at once with different rows (the gated entry: a workspace
    per stream)."""
    call, make_rows, _, _ = nv4_linear_case(kind)
    dense_on_side_streams(call, make_rows)


def dense_on_side_streams(call, make_rows):
    """``make_rows(seed)``: one tensor or the tuple of the call's row tensors."""
    as_list = lambda rows: list(rows) if isinstance(rows, tuple) else [rows]
    a, b = as_list(make_rows(1)), as_list(make_rows(2))
    want_a, want_b = call(*[t.clone() for t in a]), call(*[t.clone() for t in b])
    assert float(want_a.abs().max()) > 0 and not same_bits(want_a, want_b)
    for _ in range(2):
        busy = busy_matrix()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        got, keep, busy = enqueue(call, a, side, busy)
        torch.cuda.current_stream().wait_stream(side)
        assert same_bits(got, want_a), first_diff(got, want_a)
        torch.cuda.synchronize()
        del keep
    busy_a, busy_b = busy_matrix(), busy_matrix()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got_a, keep_a, busy_a = enqueue(call, a, sa, busy_a)
    got_b, keep_b, busy_b = enqueue(call, b, sb, busy_b)
    torch.cuda.current_stream().wait_stream(sa)
    torch.cuda.current_stream().wait_stream(sb)
    assert same_bits(got_a, want_a), ("a", first_diff(got_a, want_a))
    assert same_bits(got_b, want_b), ("b", first_diff(got_b, want_b))
    torch.cuda.synchronize()
    del keep_a, keep_b
