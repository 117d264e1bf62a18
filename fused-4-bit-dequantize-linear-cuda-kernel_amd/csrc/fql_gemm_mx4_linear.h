// The dense MXFP4 linear layer at decode (include/fql_int4.h, fql_linear_mx4_fwd / fql_linear_mx4_glu_fwd with split_k set):
// mx4_decode_kernel (fql_gemm_mx4_decode.h) cut along K, and the kernel that adds the pieces up.
//
// A grouped call gets its waves from E x top-k; one dense matrix at a few rows has ceil(N / 32) of them for all of K, and
// a wave's time is K / 64 ring slots however few bytes it moves.  The only other axis is K.
//
// mx4_linear_decode_kernel: workgroup = ONE wave = 32 weight rows n x one block of up to 32 rows t x slice s of K.
//   grid = (ceil(N / 32), ceil(T / 32), S).  No expert table.  The body is mx4_decode_body's, written out a second time so
//   that the grouped kernel's instruction stream stays what it was (fql_gemm_mx4_sdecode.h took the same trade): the same
//   loads, ring, lane swaps, mx4_pair conversion and non-finite test, bfloat16 or float32 rows, and the element-load form
//   for an unaligned base.  It differs in three places:
//   * Slices.  P = K / 64 whole pairs; slice s runs pairs [s * ceil(P / S), min(P, (s + 1) * ceil(P / S))) in ascending order
//     on an accumulator that starts at zero.  The odd last block of K % 64 == 32 belongs to the LAST slice, followed by the
//     two instructions on zeros as in mx4_decode_body: S = 1 is that kernel's sequence exactly.  A slice with nothing to do
//     stores zeros.
//   * Epilogue.  A plain float32 store of the partial sum to partial[s][t][n] (16-byte stores where N % 4 == 0), rows t < T
//     and columns n < N only.  No bias, no rounding: both belong to the reduce kernel.
//   * NON-FINITE.  A slice whose part of a row is non-finite stores NaN for that whole partial row, and a block with scale
//     code 255 gives NaN for its weight row (0x7FC0 across the block, as everywhere): NaN + anything is NaN, so the sum carries
//     both rules of fql_moe_mx4_fwd without a flag word.
//
// mx4_linear_reduce_kernel: out[t][n] = round_OUT( (((p_0 + p_1) + p_2) + ... + p_{S-1}) + bias[n] ), float32, the order
//   fixed, one rounding, 16-byte accesses where N % 4 == 0 and the bases allow; every element of out [T][N] is written once.
//
// Two launches on one stream; the launch boundary is the only synchronisation (no atomics, no flags, no polling).
#pragma once
#include "fql_gemm_mx4_decode.h"

template <int IN, bool VEC, int DEPTH, int GROUP>
__device__ __forceinline__ void mx4_linear_decode_body(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    float *__restrict__ partial, int T, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Mx4DecodeSlot<IN>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN, t_blk = (int)blockIdx.y * Mx4DecodeCfg::BT;
    const int slice = blockIdx.z, S = gridDim.z;
    const int K2 = K >> 1, KB = K >> 5;
    constexpr int es = IN == 0 ? 4 : 2;
    // Loads are unconditional: a lane past N reads row N - 1, a lane past T reads row T - 1 (neither is stored).
    const size_t wrow = (size_t)(n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KB;
    const bool row_ok = t_blk + r < T;
    const int t = row_ok ? t_blk + r : T - 1;
    const char *xrow = reinterpret_cast<const char *>(x) + ((size_t)t * K + 8 * h) * es;

    auto load_x = [&](Slot &sl, int j, int s) {                    // x[t][64 j + 16 s + 8 h .. + 7]
        const char *p = xrow + (size_t)(64 * j + 16 * s) * es;
        if constexpr (IN == 0) {
            if constexpr (VEC) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const v4f v = *reinterpret_cast<const v4f *>(p + 16 * i);
#pragma unroll
                    for (int c = 0; c < 4; ++c) sl.x[s][4 * i + c] = v[c];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) sl.x[s][i] = reinterpret_cast<const float *>(p)[i];
            }
        } else {
            if constexpr (VEC) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                sl.x[s][0] = v.x; sl.x[s][1] = v.y; sl.x[s][2] = v.z; sl.x[s][3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned short *q = reinterpret_cast<const unsigned short *>(p) + 2 * i;
                    sl.x[s][i] = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
                }
            }
        }
    };
    auto load_slot = [&](Slot &sl, int j) {                        // the 64 k of pair j (both scale blocks exist)
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * j + 16 * h);
        sl.sc = sbase[2 * j + h];
#pragma unroll
        for (int s = 0; s < 4; ++s) load_x(sl, j, s);
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    uint32_t bad = 0u;

    auto consume = [&](const Slot &sl) {                           // four instructions: k0 = 64 j + 16 s, s = 0 .. 3
        uint32_t w[4], own;
        mx4_decode_copy(sl.wq, sl.sc, w, own);
        const auto lo = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);         // {d0 | d1}, {e0 | e1}
        const auto hi = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);         // {d2 | d3}, {e2 | e3}
        const auto sc = __builtin_amdgcn_permlane32_swap(own, own, false, false);           // block 2 j, block 2 j + 1
        const uint32_t words[4] = {lo[0], hi[0], lo[1], hi[1]};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int code = (int)sc[s >> 1];
            const bool nan = code == 255;
            const int sv = nan ? 127 : code;
            uint4 a;
            a.x = mx4_pair<0>(words[s], sv);
            a.y = mx4_pair<1>(words[s], sv);
            a.z = mx4_pair<2>(words[s], sv);
            a.w = mx4_pair<3>(words[s], sv);
            if (nan) a = make_uint4(0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u);
            uint32_t xw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (IN == 0) xw[i] = mx4_pack_bf16(sl.x[s][2 * i], sl.x[s][2 * i + 1]);
                else xw[i] = sl.x[s][i];
                bad |= mx4_nonfinite2(xw[i]);
            }
            const uint4 xb = make_uint4(xw[0], xw[1], xw[2], xw[3]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, xb), acc, 0, 0, 0);
        }
    };

    // The slice's pairs [lo, hi) (wave-uniform); the odd last block of K % 64 == 32 is the last slice's.
    const int pairs = K >> 6;
    const int per = (pairs + S - 1) / S;
    const int lo = slice * per < pairs ? slice * per : pairs;
    const int hi = lo + per < pairs ? lo + per : pairs;
    const bool odd = (K & 32) != 0 && slice == S - 1;
    Slot tail;
    if (odd) {
        tail.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * pairs);
        tail.sc = sbase[2 * pairs];
#pragma unroll
        for (int s = 0; s < 2; ++s) load_x(tail, pairs, s);
    }
    __builtin_amdgcn_sched_barrier(0);

    // As in mx4_decode_body: no branch in the loop that loads; a slot index past the slice's last pair loads that pair
    // again (inside the slice, so inside the operands) and is not used.
    if (hi > lo) {
        const int last = hi - 1;
        Slot ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            load_slot(ring[i], lo + i < last ? lo + i : last);
            __builtin_amdgcn_sched_barrier(0);
        }
        int j = lo;
        for (; j + DEPTH <= hi; j += DEPTH) {
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) {
                consume(ring[i]);
                if (i % GROUP == GROUP - 1) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = i - (GROUP - 1); q <= i; ++q) {
                        const int nx = j + q + DEPTH;
                        load_slot(ring[q], nx < last ? nx : last);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < DEPTH - 1; ++i)
            if (j + i < hi) consume(ring[i]);                      // (uniform; slot i holds pair j + i)
    }
    if (odd) {
        if (h) { tail.wq = make_uint4(0u, 0u, 0u, 0u); tail.sc = 127; }
#pragma unroll
        for (int s = 2; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < (IN == 0 ? 8 : 4); ++i) tail.x[s][i] = 0;
        consume(tail);
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    const auto both = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);   // the row's other half of the slice's k
    if (!row_ok) return;
    const bool row_nan = ((both[0] | both[1]) & 0x80008000u) != 0u;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 15) == 0;
    const size_t prow = ((size_t)slice * T + t) * N;               // partial[s][t][.]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nc = n0 + 8 * q + 4 * h;
        if (nc >= N) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = row_nan ? __uint_as_float(0x7FC00000u) : acc[4 * q + c];
        store_out4(partial, 0, prow, nc, N, vec, v);
    }
}

// IN as mx4_kernel's (0 float32 rows, 2 bfloat16 rows); the partial sums are float32.
template <int IN>
__global__ __launch_bounds__(64) void mx4_linear_decode_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    float *__restrict__ partial, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4DecodeCfg;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        mx4_linear_decode_body<IN, true, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(blocks, scales, x, partial, T, K, N);
    else
        mx4_linear_decode_body<IN, false, 1, 1>(blocks, scales, x, partial, T, K, N);
#endif
}

struct Mx4LinearReduceCfg {
    static constexpr int THREADS = 256, QUADS = 64, ROWS = THREADS / QUADS;   // a workgroup: 4 rows x 64 quads of columns
    static constexpr int COLS = 4 * QUADS;
};

// partial [S][T][N] float32 -> out [T][N] of OUT; grid = (ceil(N / 256), min(ceil(T / 4), 65535)), the rows strided over y.
template <int OUT, int S>
__global__ __launch_bounds__(256) void mx4_linear_reduce_kernel(
    const float *__restrict__ partial, const float *__restrict__ bias, void *__restrict__ out, int T, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4LinearReduceCfg;
    const int n = (int)blockIdx.x * C::COLS + 4 * ((int)threadIdx.x & (C::QUADS - 1));
    if (n >= N) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 15) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const size_t plane = (size_t)T * N;
    float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bias != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c) if (n + c < N) b[c] = bias[n + c];
    }
    for (int t = (int)blockIdx.y * C::ROWS + ((int)threadIdx.x >> 6); t < T; t += (int)gridDim.y * C::ROWS) {
        const float *p = partial + (size_t)t * N + n;
        float part[S][4];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (vec) {
                const v4f v = *reinterpret_cast<const v4f *>(p + s * plane);
#pragma unroll
                for (int c = 0; c < 4; ++c) part[s][c] = v[c];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) part[s][c] = n + c < N ? p[s * plane + c] : 0.0f;
            }
        }
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = part[0][c];
#pragma unroll
            for (int s = 1; s < S; ++s) v[c] += part[s][c];
            if (bias != nullptr) v[c] += b[c];
        }
        store_out4(out, OUT, (size_t)t * N, n, N, vec, v);
    }
#endif
}
