"""The decode forms of the grouped NF4 experts on the GPU (csrc/fql_gemm_lut4_group_decode.h): the
one-wave kernel (the tile's bits) and the split-K form against float64 references.  E = 3 with counts [0, 33, 1]: an empty
expert, one row past the 32-row block, a single row; in order, and as a reversed table with a gap of uncovered rows.
K: one pair (less than the ring), five pairs (one ring round and a tail; at S = 4 the last slice is empty), nine pairs, and
ten pairs under block = 128 (two pairs per absmax; the issue's (576, 128) is no valid shape: K % block != 0).  N = 40 / 37:
a partial 32-row block, with 37 the scalar stores.  The tests set the hooks and put them back."""
import functools

import pytest
import torch

from glu_reference import act_kw, hidden64
from helpers import Guarded, assert_guards_intact
from test_gpu_nf4 import _rows, _weights
from test_gpu_nf4_moe import _grouped64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = [(64, 64), (320, 64), (576, 64), (640, 128)]
NS = [40, 37]
DTYPES = [torch.float32, torch.bfloat16]
SLICES = [1, 2, 4, 8, 16]
U = 2.0 ** -23
E, T = 3, 40
TABLES = [([0, 33, 1], [0, 0, 33]), ([0, 33, 1], [5, 6, 0])]                   # rows 34 .. 39 / 1 .. 5 and 39 uncovered
IDS = ["in_order", "reversed_with_gap"]
SETTERS = ("fql_tune_set_lut4_group_decode_max_rows", "fql_tune_set_lut4_group_split_max_rows", "fql_tune_set_lut4_group_slices")


def fq():
    import fused_int4_amd
    return fused_int4_amd


def d(t):
    return None if t is None else t.to(DEV)


@pytest.fixture
def form():
    """form(f, T, K, N) sets the hooks: f "tile" or "decode" (the plain entries' two kernels), or a slice count (0: S(K, N))
    for the split entries; returns the ops' ``split_k``.  The hooks are put back afterwards."""
    L = fq()._native.lib()
    old = [getattr(L, n)(-1) for n in SETTERS]

    def use(f, T, K, N):
        if isinstance(f, int):
            L.fql_tune_set_lut4_group_split_max_rows(1 << 20)
            L.fql_tune_set_lut4_group_slices(f)
            code = L.fql_tune_lut4_group_split_kernel(T, K, N)
            assert code & 255 == 2 and (f == 0 or code >> 8 == f)
            return True
        L.fql_tune_set_lut4_group_decode_max_rows((1 << 20) if f == "decode" else 0)
        assert L.fql_tune_lut4_group_kernel(T) == int(f == "decode")
        return False
    yield use
    for n, v in zip(SETTERS, old):
        getattr(L, n)(v)


@functools.lru_cache(maxsize=None)
def _experts(K, block, N, exact):
    per = [_weights(K, block, N, exact, 20 + e) for e in range(E)]
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), per[0][2], torch.stack([p[3] for p in per])


def _tables(table):
    return tuple(torch.tensor(v, dtype=torch.int32, device=DEV) for v in table)


def _raw(split, c, a, k, block, xs, b, tpe, offs, out, K, N, ws=None):
    """One plain or split C call into ``out`` (a tensor or a Guarded); ``ws``: a Guarded workspace, or allocated here."""
    L, _native = fq()._native.lib(), fq()._native
    I, O = ({torch.float32: 0, torch.bfloat16: 2}[t] for t in (xs.dtype, out.dtype if isinstance(out, torch.Tensor) else xs.dtype))
    Tn = xs.shape[0]
    ptr = lambda t: None if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())
    head = (ptr(c), ptr(a), ptr(k), block, ptr(xs), I, ptr(b), ptr(tpe), ptr(offs), ptr(out), O, c.shape[0], Tn, K, N)
    st = torch.cuda.current_stream().cuda_stream
    if not split:
        return _native.check(L.fql_moe_lut4_fwd(*head, st), "fwd")
    need = L.fql_moe_lut4_split_workspace_bytes(c.shape[0], Tn, K, N, 0)
    ws = ws if ws is not None else torch.empty(need, dtype=torch.uint8, device=DEV)
    _native.check(L.fql_moe_lut4_split_fwd(*head, ptr(ws), need, st), "split")
    torch.cuda.synchronize()                                                   # (the workspace lives until here)


@pytest.mark.parametrize("table", TABLES, ids=IDS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_exact_integers_bit_for_bit_in_every_form(form, K, block, N, dt, table):
    codes, absmax, book, W = _experts(K, block, N, True)
    x = _rows(T, K, True, 2)
    bias = torch.arange(E * N, dtype=torch.float32).reshape(E, N) - 3
    ref = _grouped64(x.double(), W, table, bias)
    assert bool((ref * 4 == (ref * 4).round()).all()) and float(_grouped64(x.double().abs(), W.abs(), table, bias.abs()).max()) * 4 < 2 ** 24
    c, a, b, k, xs = d(codes), d(absmax), d(bias), d(book), d(x.to(dt))
    tpe, offs = _tables(table)
    for f in ["decode", "tile"] + SLICES:
        out = torch.full((T, N), float("nan"), dtype=dt, device=DEV)          # the result starts as NaN patterns
        _raw(form(f, T, K, N), c, a, k, block, xs, b, tpe, offs, out, K, N)
        assert torch.equal(out.cpu(), ref.float().to(dt)), f                   # the exact value rounded once; zeros where uncovered


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,block", KB)
def test_nf4_gaussian_decode_is_the_tile_and_split_is_within_the_bound(form, K, block, N, dt):
    """Decode == tile == the dense op per expert, bit for bit; split at S = 1 those bits; the other S within section 48's
    K 2^-23 sum |x W| (+ 2^-8 |ref| for a bfloat16 result): S - 1 <= K more float32 additions stay inside it."""
    ops = fq().ops
    codes, absmax, _, W = _experts(K, block, N, False)
    x = _rows(T, K, False, 5).bfloat16()
    c, a, xs = d(codes), d(absmax), d(x.to(dt))
    worst = 0.0
    for table in TABLES:
        tpe, offs = _tables(table)
        run = lambda f: ops.moe_forward_lut4(c, a, xs, tpe, offs, block=block, split_k=form(f, T, K, N))
        dec = run("decode")
        assert dec.dtype == dt and torch.equal(dec, run("tile")) and torch.equal(dec, run(1))
        for e, (cnt, lo) in enumerate(zip(*table)):
            if cnt:
                assert torch.equal(dec[lo:lo + cnt], ops.linear_forward_lut4(c[e], a[e], xs[lo:lo + cnt], block=block)), e
        ref = _grouped64(x.double(), W, table)
        bound = K * U * _grouped64(x.double().abs(), W.abs(), table) + (2.0 ** -8 * ref.abs() if dt == torch.bfloat16 else 0)
        for S in SLICES[1:]:
            err = (run(S).cpu().double() - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()))
            assert bool((err <= bound).all()), S                               # (bound == 0: an uncovered row, exactly zero)
    print(f"K={K} N={N} {dt}: largest |err| / bound over S = {worst:.4f}")


@pytest.mark.parametrize("K,block", KB)
def test_split_bits_do_not_depend_on_batch_or_routing(form, K, block):
    """A row alone (T = 1, E = 1, no table) has the bits it has inside the 40-row call, under both tables, at S(K, N)."""
    ops, N = fq().ops, 40
    codes, absmax, _, _ = _experts(K, block, N, False)
    c, a, xs = d(codes), d(absmax), d(_rows(T, K, False, 6))
    split = form(0, T, K, N)
    for table in TABLES:
        out = ops.moe_forward_lut4(c, a, xs, *_tables(table), block=block, split_k=split)
        for e, (cnt, lo) in enumerate(zip(*table)):
            for t in {lo, lo + cnt - 1} if cnt else ():
                alone = ops.moe_forward_lut4(c[e:e + 1], a[e:e + 1], xs[t:t + 1], None, None, block=block, split_k=split)
                assert torch.equal(alone[0], out[t]), (e, t)


@pytest.mark.parametrize("dt", DTYPES)
def test_gated_entry_in_both_forms(form, dt):
    """Section 48's gated bound, (K 2^-23 + 2^-7) sum |h W| (+ 2^-8 |ref|); decode == tile bit for bit."""
    K, block, N, kind = 320, 64, 37, "gelu_tanh"
    codes, absmax, _, W = _experts(K, block, N, False)
    gu = (_rows(T, 2 * K, False, 7) * 2).to(dt)
    h = hidden64(kind, gu).bfloat16().double()
    for table in TABLES:
        run = lambda f: fq().ops.moe_gated_forward_lut4(d(codes), d(absmax), d(gu), *_tables(table), block=block,
                                                        split_k=form(f, T, K, N), **act_kw(kind))
        dec, ref, mag = run("decode"), _grouped64(h, W, table), _grouped64(h.abs(), W.abs(), table)
        assert torch.equal(dec, run("tile")) and torch.equal(dec, run(1))
        bound = (K * U + 2.0 ** -7) * mag + (2.0 ** -8 * ref.abs() if dt == torch.bfloat16 else 0)
        for out in (dec, run(0), run(16)):
            err = (out.cpu().double() - ref).abs()
            print(f"{kind} {dt}: largest |err| / bound = {float((err / bound.clamp_min(1e-300))[bound > 0].max()):.4f}")
            assert out.dtype == dt and bool((err <= bound).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_non_finite_rows_unaligned_rows_and_guards(form, dt):
    K, block, N = 320, 64, 37
    ops = fq().ops
    codes, absmax, book, _ = _experts(K, block, N, False)
    c, a, k = d(codes), d(absmax), d(book)
    tpe, offs = _tables(TABLES[1])
    x = _rows(T, K, False, 9).to(dt)
    bad = torch.zeros(T, dtype=torch.bool)
    bad[8] = True                                                              # expert 1's third row
    for f in ("decode", 4):                                                    # S = 4: slices of k 0 .. 127, 128 .. 255, 256 .. 319, none
        split = form(f, T, K, N)
        clean = ops.moe_forward_lut4(c, a, d(x), tpe, offs, block=block, split_k=split).cpu()
        for col, v in ((0, float("nan")), (200, float("inf")), (319, float("-inf"))):
            xb = x.clone()
            xb[8, col] = v
            got = ops.moe_forward_lut4(c, a, d(xb), tpe, offs, block=block, split_k=split).cpu()
            assert bool(got[bad].isnan().all()) and torch.equal(got[~bad], clean[~bad]), (f, col)
        flat = torch.zeros(T * K + 9, dtype=dt, device=DEV)                    # a row base one element off 16 bytes
        off = flat[1:1 + T * K].view(T, K).copy_(x)
        assert off.data_ptr() % 16 == x.element_size()
        assert torch.equal(ops.moe_forward_lut4(c, a, off, tpe, offs, block=block, split_k=split).cpu(), clean), f
        es = x.element_size()
        out = Guarded("out", T * N * es, dt, 12345.0, offset=es, device=DEV)
        ws = Guarded("workspace", max(16, fq()._native.lib().fql_moe_lut4_split_workspace_bytes(E, T, K, N, 0)), torch.float32, 54321.0,
                     device=DEV)
        xg = Guarded("rows", T * K * es, dt, float("nan"), offset=16, device=DEV)
        xg.put(x)
        out.view(dt, T, N).fill_(float("nan"))
        _raw(split, c, a, k, block, xg.view(dt, T, K), None, tpe, offs, out, K, N, ws=ws)
        assert_guards_intact(out, ws, xg, what=f"form {f}")
        assert torch.equal(out.view(dt, T, N).cpu(), clean), f


def test_layer_with_split_k_alone_and_inside_the_block(form):
    ops, NE, H, F, Tk = fq().ops, 4, 128, 64, 4
    g = torch.Generator().manual_seed(11)
    gate, up, down = ([torch.randn(*s, generator=g) * 0.05 for _ in range(NE)] for s in ((F, H), (F, H), (H, F)))
    bg, bu, bd = ([torch.randn(s, generator=g) for _ in range(NE)] for s in (F, F, H))
    m = fq().NF4MoEFFN.from_weights(gate, up, down, bg, bu, bd, activation="gelu_tanh", split_k=True).to(DEV)
    tpe, offs = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([2, 0, 1, 1], [0, 2, 2, 3]))
    x = d(_rows(Tk, H, False, 12))
    assert form(0, Tk, H, 2 * F)
    gu = ops.moe_forward_lut4(m.gate_up_codes, m.gate_up_absmax, x, tpe, offs, bias=m.gate_up_bias.detach(), split_k=True)
    want = ops.moe_gated_forward_lut4(m.down_codes, m.down_absmax, gu, tpe, offs, activation="gelu_tanh", bias=m.down_bias.detach(),
                                      split_k=True)
    assert torch.equal(m(x, tpe, offs), want)
    # inside the block the layer is passed through untouched: at S = 1 its bits are the default layer's, so the block's are too
    plain = fq().NF4MoEFFN.from_weights(gate, up, down, bg, bu, bd, activation="gelu_tanh")
    blocks = []
    for experts in (m, plain):
        torch.manual_seed(15)
        blocks.append(fq().QuantizedSparseMoEBlock(NE, H, F, top_k=2, experts=experts).to(DEV))
    assert blocks[0].experts is m and m.split_k
    form(1, 2 * Tk, H, 2 * F)
    with torch.no_grad():
        assert torch.equal(blocks[0](x)[0], blocks[1](x)[0])
