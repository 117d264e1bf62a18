"""Shared helpers for the tests (CPU restatements of the library's OWN conventions, and tolerances)."""
import numpy as np

# ---- stated floating-point tolerances (see DESIGN.md "Numerics") -------------------------------
# exact mode (3 limbs, 23-bit fixed point per activation row): float32-class.
EXACT_REL_FRO = 2e-6          # ||got - ref64||_F / ||ref64||_F
# fast mode (2 limbs, 15-bit fixed point): north_star bound is 1e-3 relative; measured ~3e-5.
FAST_REL_FRO = 2e-4
# int8 mode (1 limb, 8-bit activations per row): the "8-bit activations + INT4 weights" serving mode of BASELINE
# config 5; outside the north_star 1e-3 claim, own stated bound: ||d||_F / ||ref||_F < 1.5e-2 at the shapes of
# test_gpu_parity.py (round-1 bound, kept).  The K = 7168 configs[4] shapes (rows whose maximum sits further out in the
# tail of 7168 samples: coarser 8-bit quantum against the same rms) and the per-group INT8 kernel get the wider bound.
INT8_REL_FRO = 1.5e-2
INT8_REL_FRO_LARGE_K = 2.5e-2
# GEMV / generic float32 FMA paths: summation-order noise only.
FMA_REL_FRO = 2e-6
# the adapter (LoRA) kernels alone: float32 FMA chains, summation order only (tests/test_gpu_lora_paths.py)
ADAPTER_TOL = FMA_REL_FRO


def tol(base):
    """A bound of the INT4 path with the float32 floor of the adapter sums (tests/test_gpu_lora.py)."""
    return max(base, 1e-5)


# the float32 adapter kernels on a 16-bit operand that takes a narrower vector width (tests/test_gpu_lora16.py)
F32_TOL = tol(EXACT_REL_FRO)
# input gradient (tests/test_gpu_backward_paths.py): per-row bounds, from the heavy-row flag of the pre-pass
# (csrc/fql_act_quant.h: a row is flagged when its predicted relative error exceeds 1e-6 at L = 3 and 2.5e-4 at L = 2);
# L = 1 has no residual set: rows without outliers only
ROW_TOL = {3: EXACT_REL_FRO, 2: 1e-3, 1: INT8_REL_FRO_LARGE_K}


def fro_tol(L, N):
    """Frobenius bound of the mode; at L = 1 a contraction longer than 4096 gets the wider int8 bound."""
    if L == 1:
        return INT8_REL_FRO_LARGE_K if N > 4096 else INT8_REL_FRO
    return {3: EXACT_REL_FRO, 2: FAST_REL_FRO}[L]


def rel_fro(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref)
    return np.linalg.norm(got - ref) / (den if den > 0 else 1.0)


def act_limbs_reference(x, L):
    """numpy restatement of the library's activation pre-pass (csrc/fql_act_quant.h): per row,
    delta = 2^e with the smallest e such that rint(max|x| / 2^e) <= LIM(L); X = rint(x / delta);
    balanced base-256 digits a_l in [-128, 127].  Returns (digits [L,T,K] int32, delta [T], rowsum [L,T])."""
    x = np.asarray(x, dtype=np.float32)
    T, K = x.shape
    lim = {1: 127, 2: 127 * 256 + 127, 3: 127 * 65536 + 127 * 256 + 127}[L]
    digits = np.zeros((L, T, K), dtype=np.int64)
    delta = np.zeros(T, dtype=np.float32)
    for t in range(T):
        m = np.float32(np.abs(x[t]).max()) if K else np.float32(0)
        if m == 0:
            e = 0
        else:
            _, ex = np.frexp(m)
            e = max(int(ex) - 1 - (8 * L - 2), -126)
            if np.rint(np.float32(m) * np.float32(2.0 ** -e)) > lim:
                e += 1
        delta[t] = np.float32(2.0 ** e)
        X = np.rint(x[t].astype(np.float32) * np.float32(2.0 ** -e)).astype(np.int64)
        for l in range(L):
            if l == L - 1:
                d = X
            else:
                d = ((X + 128) & 255) - 128
                X = (X - d) >> 8
            digits[l, t] = d
    return digits, delta, digits.sum(axis=2)


def decode_limbs(limbs_bytes, L, T, E, K, Kp, counts=None, offsets=None, which=0):
    """Invert the fragment-native layout written by the pre-pass:
    limbs[l][kb][mb][ks][lane][16 B] -> digits [L, T, Kp] in natural k order.  ``which`` = 1 selects the residual
    set of heavy-tailed rows (2 / 3 limbs only)."""
    raw = np.asarray(limbs_bytes).view(np.int8)
    KB = Kp // 256
    MBT = (T + 32 * E + 128 + 31) // 32                     # the library's row_blocks(T, E) (csrc/fql_int4.hip)
    one = L * KB * MBT * 8192
    assert raw.size in (one, 2 * one), (raw.size, one)      # 2 / 3 limbs carry a second (residual) set
    arr = raw[which * one:(which + 1) * one].reshape(L, KB, MBT, 8, 64, 16)
    # padded row of every t
    if counts is None:
        prow = np.arange(T)
        covered = np.ones(T, bool)
    else:
        prow = np.zeros(T, dtype=np.int64)
        covered = np.zeros(T, bool)
        pbase = 0
        for c, o in zip(counts, offsets):
            lo, hi = max(int(o), 0), min(int(o) + int(c), T)
            cnt = max(hi - lo, 0)
            for t in range(lo, hi):
                if not covered[t]:
                    prow[t] = pbase + (t - lo)
                    covered[t] = True
            pbase += (cnt + 31) // 32 * 32
    out = np.zeros((L, T, Kp), dtype=np.int64)
    perm8 = [0, 2, 4, 6, 1, 3, 5, 7]                         # stored position i holds natural k perm8[i]
    for t in range(T):
        if not covered[t]:
            continue
        p = int(prow[t])
        for kb in range(KB):
            for c in range(8):                               # 32-k chunk of the 256 block
                v, g = c >> 1, c & 1
                for b in range(2):
                    ks = 2 * v + b
                    sixteen = arr[:, kb, p >> 5, ks, g * 32 + (p & 31), :]      # [L,16]
                    k0 = kb * 256 + 32 * c + 16 * b
                    for h in range(2):                       # two groups of 8
                        for i in range(8):
                            out[:, t, k0 + 8 * h + perm8[i]] = sixteen[:, 8 * h + i]
    return out, covered


def row_quantum_bound(x, L):
    """Predicted relative output error of each row from the one rounding of its activations to the row's
    fixed-point quantum: delta[t] / sqrt(12) * sqrt(K) / ||x_t||_2 (rounding errors uniform in +-delta/2 and
    uncorrelated with the weights).  Never above 2^-(8L-2) * sqrt(K/12): max|x_t| <= ||x_t||_2."""
    x = np.asarray(x, dtype=np.float32)
    _, delta, _ = act_limbs_reference(x, L)
    nrm = np.linalg.norm(x.astype(np.float64), axis=1)
    nrm[nrm == 0] = 1.0
    return delta.astype(np.float64) / np.sqrt(12.0) * np.sqrt(x.shape[1]) / nrm


# ---- fp8 (OCP e4m3) activations, BASELINE.json configs[4]; not in the reference (README.md:228: future work) ----------
# (1) kernel error: the fp8 matrix-core pass against a float64 matmul of the SAME e4m3 inputs.  The accumulator is
#     float32, but the instruction adds its 64 products in a fixed-point adder aligned to the largest of them, so the
#     result is NOT a float32 fma chain: measured on MI355X 1.2e-4 .. 2.6e-4 (Frobenius) on uniformly random e4m3 codes
#     (exponents spread over 2^-9 .. 2^8 in one dot product: the worst case) and 2.0e-5 .. 2.5e-5 on per-row scaled
#     randn activations (FQL_PRECISION_FP8's own quantiser).  Small integers are exact (tests/test_gpu_fp8.py).
FP8_ACC_REL_FRO = 6e-4
FP8_ACC_SCALED_REL_FRO = 1e-4
# (2) format error: e4m3 has a 4-bit significand; per-row scaled randn activations land at ~2.7e-2 relative (Frobenius)
#     against float32 activations.  Outside the north-star 1e-3 claim, stated on its own.
FP8_FORMAT_REL_FRO = 6e-2


def act_residual_reference(x, L):
    """numpy restatement of the heavy-tail rule of the pre-pass (csrc/fql_act_quant.h, pass 3): a row is flagged when
    sum_k (x/delta)^2 < K / (12 P^2), P = 1e-6 (3 limbs) / 2.5e-4 (2 limbs); its residual digits are those of
    R = rint((x/delta - rint(x/delta)) * 2^(8L-1)), delta2 = delta * 2^-(8L-1).
    Returns (flag [T] bool, digits [L,T,K], delta2 [T], rowsum2 [L,T]).  (The flag's float32 sum is order dependent in
    its last bits: callers test rows that are clearly on one side.)"""
    x = np.asarray(x, dtype=np.float32)
    T, K = x.shape
    _, delta, _ = act_limbs_reference(x, L)
    xs = (x.astype(np.float64) / delta[:, None].astype(np.float64))            # exact: delta is a power of two
    lim = K * (8.3333e10 if L == 3 else 1.3333e6)
    flag = ((xs ** 2).sum(axis=1) < lim) & (np.abs(x).max(axis=1) > 0)
    rb = 8 * L - 1
    R = np.rint((xs - np.rint(xs)) * float(1 << rb)).astype(np.int64)
    digits = np.zeros((L, T, K), dtype=np.int64)
    Xr = R.copy()
    for l in range(L):
        if l == L - 1:
            d = Xr
        else:
            d = ((Xr + 128) & 255) - 128
            Xr = (Xr - d) >> 8
        digits[l] = d
    delta2 = np.where(flag, delta.astype(np.float64) * 2.0 ** -rb, 0.0).astype(np.float32)
    return flag, digits, delta2, digits.sum(axis=2)


# ---- device-side float64 references (torch only: no fql_* kernel is called) -------------------------------------------
def dequant_f64(packed, scales, zps):
    """float64 weights ``(q - zp) * s`` [N, K] of one INT4 matrix, on the tensors' device: ``packed`` [N, K/2] uint8
    (byte j of a row = q[2j] | q[2j+1] << 4), ``scales`` / ``zps`` [N] (per row) or [N, G] (per group of K / G)."""
    import torch
    p = packed.to(torch.int16)
    q = torch.stack((p & 15, p >> 4), dim=-1).reshape(packed.shape[0], -1).to(torch.float64)
    s, z = scales.to(q.device, torch.float64), zps.to(q.device, torch.float64)
    if s.dim() == 2 and s.shape[1] > 1:                      # per group along K
        G = s.shape[1]
        return ((q.reshape(q.shape[0], G, -1) - z[..., None]) * s[..., None]).reshape(q.shape)
    s, z = s.reshape(-1, 1), z.reshape(-1, 1)
    return (q - z) * s


def row_rel_err(got, ref):
    """max over rows t of ||got_t - ref_t|| / ||ref_t|| (float64).  A row whose reference is exactly zero must be
    exactly zero in ``got`` (its error is then 0, otherwise inf).  Accepts numpy arrays or torch tensors."""
    import torch
    g = torch.as_tensor(got).to(torch.float64)
    r = torch.as_tensor(ref).to(device=g.device, dtype=torch.float64)
    g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    if g.shape[0] == 0:
        return 0.0
    num = torch.linalg.vector_norm(g - r, dim=1)
    den = torch.linalg.vector_norm(r, dim=1)
    zero = den == 0
    err = torch.where(zero, torch.where(num == 0, 0.0, float("inf")).to(num), num / torch.where(zero, 1.0, den))
    return float(err.max())


def misaligned(t, floats):
    """A contiguous copy of ``t`` whose data pointer sits ``floats`` elements (for float32: 1, 2 or 3 = 4, 8 or 12 bytes)
    past a 16-byte boundary: the public ops keep it as it is (it is contiguous), so the kernels see an unaligned base."""
    import torch
    per16 = 16 // t.element_size()                           # elements per 16 bytes
    buf = torch.empty(t.numel() + per16 + floats, dtype=t.dtype, device=t.device)
    start = (-(buf.data_ptr() // t.element_size()) + floats) % per16
    out = buf[start:start + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == floats * t.element_size()
    return out


# ---- shared by the GPU test files of the backward and adapter paths ---------------------------------------------------
def fq():
    import fused_int4_amd
    return fused_int4_amd


def ops():
    from fused_int4_amd import ops as o
    return o


def rel_fro_dev(got, ref):
    """``rel_fro`` for torch tensors on the device, in float64."""
    import torch
    got, ref = got.double(), ref.to(got.device).double()
    den = torch.linalg.vector_norm(ref)
    return float(torch.linalg.vector_norm(got - ref) / (den if den > 0 else 1.0))


def expert_table(counts, gaps=None, tail=0, device="cuda"):
    """(tokens_per_expert, input_offsets, T) int32 on ``device``: ``gaps[e]`` uncovered rows in front of expert e,
    ``tail`` uncovered rows after the last."""
    import torch
    gaps = gaps or [0] * len(counts)
    offs, pos = [], 0
    for c, gp in zip(counts, gaps):
        pos += gp
        offs.append(pos)
        pos += c
    return (torch.tensor(counts, dtype=torch.int32, device=device),
            torch.tensor(offs, dtype=torch.int32, device=device), pos + tail)


def clipped_ranges(tokens_per_expert, input_offsets, T):
    """The device's clipping of an expert table (csrc/fql_common.h expert_range, csrc/fql_lora.h expert_rows): rows
    [lo, hi) of expert e with lo = clamp(offset, 0, T), hi = clamp(offset + count, lo, T) (empty for count <= 0)."""
    out = []
    for c, o in zip(tokens_per_expert.tolist(), input_offsets.tolist()):
        lo = min(max(o, 0), T)
        hi = min(max(o + c, lo), T) if c > 0 else lo
        out.append((lo, hi))
    return out


# ---- hostile and large expert tables (tests/test_gpu_mxfp4_tables.py) --------------------------------------------------
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
HOSTILE_TABLES = ("e65", "e130-descending", "e128-decode", "clipped", "gaps-descending", "all-empty", "one-expert-inside")
E128_OWNERS = ((3, 5), (17, 0), (42, 7), (63, 2), (64, 1), (77, 6), (100, 3), (127, 4))   # (expert, its one row) of e128-decode


def hostile_table(name):
    """(tokens_per_expert, input_offsets, T, ranges) of one of HOSTILE_TABLES: the raw int32 values as CPU tensors, as the
    device gets them, and ``clipped_ranges`` of them.  The ranges are asserted to lie in [0, T] and not to overlap.

    e65: 65 experts, rows [0 1] . [e0: 1] [e63: 33] . . [e64: 3] . (a dot: a row no expert covers); the others are empty.
    e130-descending: expert e owns the one row T - 2 - e of T = 132.  e128-decode: T = 8, the experts of E128_OWNERS own
    one row each in a scrambled order, the 120 others are empty at offsets all over [0, T].  clipped: T = 40 with negative
    offsets and counts, a count past T, an offset past T and both int32 extremes.  gaps-descending: counts [33, 0, 70, 1]
    laid out from the last expert to the first with 3 rows in front, 5 between neighbours and 2 behind.  all-empty: three
    empty experts over 5 rows.  one-expert-inside: one expert on [1, 34) of 35 rows."""
    import torch
    if name == "e65":
        counts = [1] + [0] * 62 + [33, 3]
        gaps = [2] + [0] * 63 + [2]
        tpe, offs, T = expert_table(counts, gaps=gaps, tail=1, device="cpu")
    elif name == "e130-descending":
        T = 132
        tpe, offs = torch.ones(130, dtype=torch.int32), torch.tensor([T - 2 - e for e in range(130)], dtype=torch.int32)
    elif name == "e128-decode":
        T = 8
        tpe, offs = torch.zeros(128, dtype=torch.int32), torch.tensor([(5 * e) % 9 for e in range(128)], dtype=torch.int32)
        for e, row in E128_OWNERS:
            tpe[e], offs[e] = 1, row
    elif name == "clipped":
        T = 40
        pairs = [(-3, 5), (2, 0), (10, -4), (30, 999), (50, 3), (INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MAX)]
        offs = torch.tensor([o for o, _ in pairs], dtype=torch.int32)
        tpe = torch.tensor([c for _, c in pairs], dtype=torch.int32)
    elif name == "gaps-descending":
        rev_t, rev_o, T = expert_table([1, 70, 0, 33], gaps=[3, 5, 5, 5], tail=2, device="cpu")
        tpe, offs = rev_t.flip(0).contiguous(), rev_o.flip(0).contiguous()
    elif name == "all-empty":
        T = 5
        tpe, offs = torch.zeros(3, dtype=torch.int32), torch.tensor([0, 2, 5], dtype=torch.int32)
    elif name == "one-expert-inside":
        T = 35
        tpe, offs = torch.tensor([T - 2], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    else:
        raise KeyError(name)
    ranges = clipped_ranges(tpe, offs, T)
    taken = sorted((lo, hi) for lo, hi in ranges if hi > lo)
    assert all(0 <= lo <= hi <= T for lo, hi in ranges), name
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:])), f"{name}: overlapping ranges are outside the contract"
    return tpe, offs, T, ranges


def uncovered_mask(ranges, T):
    """bool [T]: the rows no range of ``ranges`` holds."""
    import torch
    mask = torch.ones(T, dtype=torch.bool)
    for lo, hi in ranges:
        mask[lo:hi] = False
    return mask


# ---- guard bands (tests/test_gpu_footprint*.py): a kernel that leaves its buffer lands in memory the test owns ----------
GUARD_BYTES = 64 * 1024
NAN = float("nan")
SENT = -7.5                        # exact in float32, float16 and bfloat16; no result of the footprint problems
BIG = 0x7F7F7F7F                   # a table entry or index that is used sends a kernel far away


def footprint_table(name):
    """(tokens_per_expert, input_offsets, T) of the footprint problems, int32 numpy, as the device gets them.  G1: experts
    of [129, 0, 1, 65, 33] rows plus 3 uncovered (a 128-row tile plus one row, an empty expert); G1c: G1 with a last
    count that leaves [0, T) and is clipped on the device; G2: one expert of 129 rows and sixteen of 1 (every group
    leaves a nearly empty 32-row block: the worst case of row_blocks() and m_slots)."""
    counts, tail = ([129] + [1] * 16, 0) if name == "G2" else ([129, 0, 1, 65, 33], 3)
    counts = np.array(counts, np.int32)
    offs = (np.cumsum(counts) - counts).astype(np.int32)
    T = int(counts.sum()) + tail
    if name == "G1c":
        counts[-1] = 999
        assert offs[-1] + counts[-1] > T
    return counts, offs, T


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def first_diff(a, b):
    d = (bits(a) != bits(b)).nonzero()
    return int(d.shape[0]), (d[0].tolist() if d.shape[0] else None)


def heavy_rows(x, rng, step=5, factor=800.0):
    """Two channels x 800 in every fifth row (make_moe of tests/test_gpu_w4.py): flagged by the pre-pass at 2 / 3 limbs."""
    for t in range(0, x.shape[0], step):
        x[t, rng.choice(x.shape[1], 2, replace=False)] *= factor
    return x


class Guarded:
    """``nbytes`` of device memory (the interior) inside one larger uint8 allocation, with at least GUARD_BYTES of guard
    on each side.  The interior starts ``offset`` bytes past a 256-byte boundary: 16 for a workspace, limb or scratch
    buffer (the least the library accepts), the element size for everything else.  The guards hold ``guard_value``
    repeated as elements of ``guard_dtype`` (a sentinel no result can be around an output; NaN, 0xFF or a huge index
    around an input, so that a guard element that is USED shows in the values as well)."""

    def __init__(self, name, nbytes, guard_dtype, guard_value, offset=16, device="cuda"):
        import torch
        esz = torch.empty((), dtype=guard_dtype).element_size()
        assert offset % esz == 0 and nbytes % esz == 0 and 0 <= offset < 256, (name, offset, nbytes, esz)
        self.name, self.nbytes = name, int(nbytes)
        self.raw = torch.empty(2 * GUARD_BYTES + 512 + self.nbytes, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        assert base % 16 == 0
        self.start = GUARD_BYTES + (offset - (base + GUARD_BYTES)) % 256
        assert (base + self.start) % 256 == offset and self.start % esz == 0
        self.end = self.start + self.nbytes
        self.ptr = base + self.start
        self.raw.zero_()
        if guard_dtype == torch.int32 or guard_dtype == torch.uint8:
            self.raw[:self.start].view(guard_dtype).fill_(guard_value)
            self.raw[self.end:self.end + GUARD_BYTES].view(guard_dtype).fill_(guard_value)
        else:
            self.raw[:self.start].view(guard_dtype).fill_(float(guard_value))
            self.raw[self.end:self.end + GUARD_BYTES].view(guard_dtype).fill_(float(guard_value))
        self._lo = self.raw[:self.start].clone()
        self._hi = self.raw[self.end:self.end + GUARD_BYTES].clone()

    def bytes(self):
        """The interior as uint8 [nbytes] (a view)."""
        return self.raw[self.start:self.end]

    def view(self, dtype, *shape):
        """The interior as a tensor of ``dtype`` and ``shape`` (a view: the kernels' buffer itself)."""
        return self.bytes().view(dtype).view(*shape)

    def put(self, tensor):
        """Copy ``tensor`` (any device) into the interior; returns the interior view of its dtype and shape."""
        v = self.view(tensor.dtype, *tensor.shape)
        v.copy_(tensor)
        return v

    def violations(self):
        """None, or (first, last) changed guard byte as offsets from the start of the interior (negative: in front of
        it; >= nbytes: behind it)."""
        import torch
        if torch.equal(self.raw[:self.start], self._lo) and torch.equal(self.raw[self.end:self.end + GUARD_BYTES], self._hi):
            return None
        lo = (self.raw[:self.start] != self._lo).nonzero().flatten() - self.start
        hi = (self.raw[self.end:self.end + GUARD_BYTES] != self._hi).nonzero().flatten() + self.nbytes
        bad = torch.cat((lo, hi))
        return int(bad.min()), int(bad.max())


def guarded_like(name, tensor, guard_value, offset=None, guard_dtype=None, device="cuda"):
    """A Guarded buffer holding a copy of ``tensor`` (numpy or torch); ``offset`` defaults to the element size."""
    import torch
    t = torch.as_tensor(tensor)
    g = Guarded(name, t.numel() * t.element_size(), guard_dtype or t.dtype, guard_value,
                t.element_size() if offset is None else offset, device)
    g.put(t.contiguous())
    return g


def assert_guards_intact(*buffers, what=""):
    """After a synchronize: no guard byte of any buffer has changed.  The message names the buffer and the first and
    last changed byte relative to its interior."""
    import torch
    if buffers and buffers[0].raw.is_cuda:
        torch.cuda.synchronize()
    for b in buffers:
        v = b.violations()
        if v is not None:
            first, last = v
            where = lambda o: f"{-o} bytes in front of it" if o < 0 else f"{o - b.nbytes} bytes past its end"
            raise AssertionError(f"{what}: buffer '{b.name}' ({b.nbytes} bytes): guard changed, first byte at interior "
                                 f"offset {first} ({where(first)}), last at {last} ({where(last)})")


# ---- operands past 2 GiB and 4 GiB (tests/test_gpu_large_tensors.py): a 32-bit offset that wraps stays in memory the test owns
B31 = 1 << 31
B32 = 1 << 32


def bit_pattern(dtype, value):
    """(integer dtype of the same width, integer) whose bits are ``value`` as one element of ``dtype``."""
    import torch
    one = torch.empty(1, dtype=dtype)
    one.fill_(value)
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[one.element_size()]
    return idt, int(one.view(idt)[0])


class BigGuarded:
    """``Guarded`` for an operand of more than 2^31 bytes: the guard IN FRONT of the interior is 2^31 bytes (plus the
    alignment), the one behind it GUARD_BYTES.  A byte offset in [2^31, 2^32) that is truncated to a signed 32-bit value
    lands at most 2^31 bytes in front of the base, inside the front guard; one in [2^32, 2^33) truncated to an unsigned
    32-bit value lands inside the interior itself (which is larger than 2^32 bytes then).  Both guards hold ``poison`` as
    elements of ``dtype`` (NaN around float inputs, 0xFF around packed weights and E8M0 scales, SENT around outputs), so a
    wrapped load returns poison, a wrapped store breaks the pattern, and neither leaves memory the test owns.  The
    interior starts 16 bytes past a 256-byte boundary (every vector width the kernels pick stays legal) and is NOT
    initialised: the caller fills it.  The guards are checked against the pattern in 256 MiB pieces (no second copy)."""
    PIECE = 1 << 28

    def __init__(self, name, nbytes, dtype, poison, front=B31, device="cuda"):
        import torch
        self.idt, self.pattern = bit_pattern(dtype, poison)
        esz = torch.empty((), dtype=dtype).element_size()
        assert nbytes % esz == 0 and front % 256 == 0
        self.name, self.nbytes, self.dtype, self.front, self.esz = name, int(nbytes), dtype, int(front), esz
        self.raw = torch.empty(self.front + 512 + self.nbytes + GUARD_BYTES, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        assert base % 16 == 0
        self.start = self.front + (16 - (base + self.front)) % 256
        self.end = self.start + self.nbytes
        self.ptr = base + self.start
        assert self.ptr % 256 == 16 and self.start >= self.front and self.end + GUARD_BYTES <= self.raw.numel()
        self.raw[:self.start].view(self.idt).fill_(self.pattern)
        self.raw[self.end:self.end + GUARD_BYTES].view(self.idt).fill_(self.pattern)

    def bytes(self):
        return self.raw[self.start:self.end]

    def view(self, *shape):
        """The interior as a tensor of the operand's dtype and ``shape`` (a view: the kernels' buffer itself)."""
        return self.bytes().view(self.dtype).view(*shape)

    def at(self, byte_offset, n):
        """``n`` elements at ``byte_offset`` from the START OF THE INTERIOR, which may be negative (the front guard)."""
        a = self.start + byte_offset
        assert 0 <= a and a + n * self.esz <= self.raw.numel() and byte_offset % self.esz == 0
        return self.raw[a:a + n * self.esz].view(self.dtype)

    def violations(self):
        """None, or (first, last) changed guard byte as offsets from the start of the interior."""
        bad = []
        for lo, hi, rel in ((0, self.start, -self.start), (self.end, self.end + GUARD_BYTES, self.nbytes - self.end)):
            for a in range(lo, hi, self.PIECE):
                b = min(a + self.PIECE, hi)
                diff = self.raw[a:b].view(self.idt) != self.pattern
                if bool(diff.any()):
                    w = diff.nonzero().flatten() * self.raw[a:b].view(self.idt).element_size()
                    bad += [int(w.min()) + a + rel, int(w.max()) + a + rel]
                del diff
        return (min(bad), max(bad)) if bad else None


def wrapped_offsets(byte_offset):
    """Where a byte offset lands when a kernel truncates it to 32 bits: ``(unsigned, signed)`` -- ``offset mod 2^32``, and
    that value read as a signed int (negative for a remainder of 2^31 or more: in front of the base).  Either is None
    where it equals the offset itself (nothing to tell apart)."""
    u = byte_offset % B32
    s = u - B32 if u >= B31 else u
    return (u if u != byte_offset else None), (s if s != byte_offset else None)


def row_groups(T, row_bytes):
    """The four row groups of the large-operand tests, as (lo, hi) pairs: 33 rows at the start, 70 rows around the row in
    which the byte offset crosses 2^31, 70 around the one that crosses 2^32 (left out when the operand ends before it),
    33 rows ending 2 rows before T.  Asserts that they are disjoint, in order, and that the straddling rows straddle."""
    g = [(0, 33)]
    for b in (B31, B32):
        r = b // row_bytes
        if (r + 36) * row_bytes <= (T - 35) * row_bytes:
            assert r * row_bytes < b < (r + 1) * row_bytes, "the row stride divides the boundary: no row straddles it"
            g.append((r - 35, r + 35))
    g.append((T - 35, T - 2))
    assert all(a[1] < b[0] for a, b in zip(g, g[1:])) and g[-1][1] * row_bytes <= T * row_bytes, g
    return g


def free_gib():
    import torch
    return torch.cuda.mem_get_info()[0] / 2 ** 30
