// The dense NVFP4 linear layer at decode (include/fql_int4.h, fql_linear_nvfp4_split_fwd / fql_linear_nvfp4_glu_split_fwd;
// DESIGN.md section 43): nv4_decode_kernel (fql_gemm_nvfp4.h) cut along K, and the kernel that adds the pieces up, scales
// the sum and adds the bias.
//
// One dense matrix at a few rows has ceil(N / 32) waves for all of K, and every one of them pays the three-instruction
// e4m3 x e2m1 conversion in the loop that feeds its matrix core.  The only other axis is K: S slices are S times the waves,
// each with 1 / S of the conversion work, on SIMDs that had nothing to do.
//
// nv4_linear_decode_kernel<IN>: workgroup = ONE wave = 32 weight rows n x one block of up to 32 rows t x slice s of K.
//   grid = (ceil(N / 32), ceil(T / 32), S).  No expert table, no mx4_group_begin, no bias, no global scale.
//   * Slices.  P = K / 64 whole pairs; slice s runs pairs [s * ceil(P / S), min(P, (s + 1) * ceil(P / S))) in ascending order
//     on an accumulator that starts at zero, nv4_dequant8 and v_mfma_f32_32x32x16_bf16 as nv4_decode_body feeds them.  The
//     odd piece of K % 64 == 32 belongs to the LAST slice: it runs under the bytes 0x3838 for the piece that is not there,
//     followed by the two instructions on zeros, so S = 1 is nv4_decode_body's sequence.  A slice with nothing to do stores
//     zeros.
//   * The ring is sized for a SLICE, not for K: FQL_NVFP4_LINEAR_DEPTH slots (float32 rows: half as many), refilled GROUP
//     at a time.  nv4_decode_kernel's 8 slots are 240 / 333 registers, one wave a SIMD; a slice of the policy's walks 6 to 112
//     pairs, and 4 slots are 116 + 16 (float32 rows) / 172 + 16 (bfloat16 rows) registers without scratch: three / two
//     waves a SIMD, so where the grid has more than 1024 waves one wave's conversion runs under another's loads.  Measured
//     3 to 10 % faster than 8 slots.
//   * The scale bytes.  DIRECT = false: a lane loads the two bytes of ITS piece and a third v_permlane32_swap gives both
//     halves all four (nv4_decode_body's way).  DIRECT = true: every lane loads the four bytes of the pair itself (they are
//     adjacent: one more 2-byte reach into a line the lane touches anyway) and the swap, the copy it needs and its wait
//     states leave the conversion's VALU stream.  Same values either way; FQL_NVFP4_LINEAR_DIRECT_SCALES chooses.
//   * Epilogue.  A plain float32 store of the partial sum to partial[s][t][n] (16-byte stores where N % 4 == 0 and the base
//     allows), rows t < T and columns n < N only.
//   * NON-FINITE, without a flag word.  A slice whose part of a row is non-finite stores NaN for that whole partial row; a
//     NaN scale byte (0x7F, 0xFF) is a NaN weight block, so the matrix core makes its weight row's partial NaN on every
//     row.  NaN + anything is NaN: the reduce kernel's sum carries both rules of fql_moe_nvfp4_fwd.
//   * Rows whose base is not 16-byte aligned take the element-load form with a ring of one slot, as everywhere.
//
// nv4_linear_reduce_kernel<OUT, S>:
//   out[t][n] = round_OUT( fl32( fl32( (((p_0 + p_1) + p_2) + ... + p_{S-1}) * global_scale ) + bias[n] ) )
//   float32, the order fixed, the multiply then the add, never an FMA (contraction off, as nv4_epilogue).  Without a global
//   scale and a bias the result is the sum's bits.  Every element of out [T][N] is written once.
//
// Two launches on one stream; the launch boundary is the only synchronisation (no atomics, no flags, no polling).
//
// Both kernels are compiled without the packed float32 instructions (the target attribute below): nv4_pair's two products
// are two v_mul_f32 here and the reduce kernel's sums are v_add_f32.  The products are exact, so the bits are nv4_kernel's.
#pragma once
#include "fql_gemm_nvfp4.h"

#ifndef FQL_NVFP4_LINEAR_DEPTH
#define FQL_NVFP4_LINEAR_DEPTH 4           // ring slots of the bfloat16-row kernel (A/B knob; float32 rows take half as many)
#endif
#ifndef FQL_NVFP4_LINEAR_DIRECT_SCALES
#define FQL_NVFP4_LINEAR_DIRECT_SCALES 1   // 1: a lane loads the pair's four scale bytes itself; 0: two bytes and a lane swap
#endif
#define FQL_NV4_LINEAR_TARGET __attribute__((target("no-packed-fp32-ops")))

struct Nv4LinearCfg {
    static constexpr int DEPTH_BF16 = FQL_NVFP4_LINEAR_DEPTH, DEPTH_F32 = DEPTH_BF16 > 1 ? DEPTH_BF16 / 2 : 1;
    static constexpr int GROUP_BF16 = DEPTH_BF16 >= 4 ? 4 : DEPTH_BF16, GROUP_F32 = DEPTH_F32 >= 2 ? 2 : 1;
    static constexpr bool DIRECT = FQL_NVFP4_LINEAR_DIRECT_SCALES != 0;
};

// One ring slot: the piece, the scale bytes (DIRECT: the pair's four, byte s for step s; else the piece's two in the low
// half) and the four row fragments of 64 k.
template <int IN>
struct Nv4LinearSlot {
    uint4 wq;
    uint32_t sc;
    typename std::conditional<IN == 0, float, uint32_t>::type x[4][IN == 0 ? 8 : 4];
};

template <int IN, bool VEC, bool DIRECT, int DEPTH, int GROUP>
__device__ __forceinline__ void nv4_linear_decode_body(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    float *__restrict__ partial, int T, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Nv4LinearSlot<IN>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN, t_blk = (int)blockIdx.y * Mx4DecodeCfg::BT;
    const int slice = blockIdx.z, S = gridDim.z;
    const int K2 = K >> 1, KS = K >> 4;
    constexpr int es = IN == 0 ? 4 : 2;
    // Loads are unconditional: a lane past N reads row N - 1, a lane past T reads row T - 1 (neither is stored).
    const size_t wrow = (size_t)(n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KS;
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
    auto load_scales = [&](int piece) {                            // the two scale bytes of the piece of 32 k number `piece`
        return (uint32_t)sbase[2 * piece] | ((uint32_t)sbase[2 * piece + 1] << 8);
    };
    auto load_slot = [&](Slot &sl, int j) {                        // the 64 k of pair j (both pieces exist)
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * j + 16 * h);
        if constexpr (DIRECT) sl.sc = load_scales(2 * j) | (load_scales(2 * j + 1) << 16);
        else sl.sc = load_scales(2 * j + h);
#pragma unroll
        for (int s = 0; s < 4; ++s) load_x(sl, j, s);
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    uint32_t bad = 0u;

    auto consume = [&](const Slot &sl) {                           // four instructions: k0 = 64 j + 16 s, s = 0 .. 3
        uint32_t w[4], own;
        mx4_decode_copy(sl.wq, sl.sc, w, own);                     // (the swaps overwrite copies)
        const auto lo = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);         // {d0 | d1}, {e0 | e1}
        const auto hi = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);         // {d2 | d3}, {e2 | e3}
        const uint32_t words[4] = {lo[0], hi[0], lo[1], hi[1]};
        float sv[4];
        if constexpr (DIRECT) {
            sv[0] = nv4_scale<0>(sl.sc); sv[1] = nv4_scale<1>(sl.sc); sv[2] = nv4_scale<2>(sl.sc); sv[3] = nv4_scale<3>(sl.sc);
        } else {
            const auto sc = __builtin_amdgcn_permlane32_swap(own, own, false, false);       // piece 2 j's bytes, piece 2 j + 1's
            sv[0] = nv4_scale<0>(sc[0]); sv[1] = nv4_scale<1>(sc[0]); sv[2] = nv4_scale<0>(sc[1]); sv[3] = nv4_scale<1>(sc[1]);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {                              // step s is scale block 4 j + s, for both halves
            const uint4 a = nv4_dequant8(words[s], sv[s]);
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

    // The slice's pairs [lo, hi) (wave-uniform); the odd last piece of K % 64 == 32 is the last slice's.  Both halves load
    // it (the h = 1 lanes drop theirs below) and the 32 k of x that exist.
    const int pairs = K >> 6;
    const int per = (pairs + S - 1) / S;
    const int lo = slice * per < pairs ? slice * per : pairs;
    const int hi = lo + per < pairs ? lo + per : pairs;
    const bool odd = (K & 32) != 0 && slice == S - 1;
    Slot tail;
    if (odd) {
        tail.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * pairs);
        tail.sc = load_scales(2 * pairs);
#pragma unroll
        for (int s = 0; s < 2; ++s) load_x(tail, pairs, s);
    }
    __builtin_amdgcn_sched_barrier(0);

    // No branch in the loop that loads: a slot index past the slice's last pair loads that pair again (inside the slice, so
    // inside the operands) and is not used.
    if (hi > lo) {
        const int last = hi - 1;
        Slot ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {                          // (in the order of their use: the waits count on it)
            load_slot(ring[i], lo + i < last ? lo + i : last);
            __builtin_amdgcn_sched_barrier(0);
        }
        int j = lo;
        for (; j + DEPTH <= hi; j += DEPTH) {
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) {
                consume(ring[i]);
                if (i % GROUP == GROUP - 1) {                      // refill the GROUP slots just used, back to back
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
        // the piece that is not there: zero codes under 0x38 (1.0), as nv4_kernel pads its last stage
        if constexpr (DIRECT) tail.sc |= 0x38380000u;
        if (h) { tail.wq = make_uint4(0u, 0u, 0u, 0u); if constexpr (!DIRECT) tail.sc = 0x3838u; }
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

// IN as nv4_kernel's (0 float32 rows, 2 bfloat16 rows); the partial sums are float32.
template <int IN>
__global__ __launch_bounds__(64) FQL_NV4_LINEAR_TARGET void nv4_linear_decode_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    float *__restrict__ partial, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Nv4LinearCfg;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        nv4_linear_decode_body<IN, true, C::DIRECT, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(blocks, scales, x, partial, T, K, N);
    else
        nv4_linear_decode_body<IN, false, C::DIRECT, 1, 1>(blocks, scales, x, partial, T, K, N);
#endif
}

struct Nv4LinearReduceCfg {
    static constexpr int THREADS = 256, QUADS = 64, ROWS = THREADS / QUADS;   // a workgroup: 4 rows x 64 quads of columns
    static constexpr int COLS = 4 * QUADS;
};

// partial [S][T][N] float32 -> out [T][N] of OUT; grid = (ceil(N / 256), min(ceil(T / 4), 65535)), the rows strided over y.
// gscale: one float32 or NULL (1, no multiply); bias [N] or NULL.
template <int OUT, int S>
__global__ __launch_bounds__(256) FQL_NV4_LINEAR_TARGET void nv4_linear_reduce_kernel(
    const float *__restrict__ partial, const float *__restrict__ gscale, const float *__restrict__ bias, void *__restrict__ out,
    int T, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)                     // sum * global_scale, THEN + bias: two roundings, never an FMA
    using C = Nv4LinearReduceCfg;
    const int n = (int)blockIdx.x * C::COLS + 4 * ((int)threadIdx.x & (C::QUADS - 1));
    if (n >= N) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 15) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const size_t plane = (size_t)T * N;
    const bool has_gs = gscale != nullptr;
    const float gs = has_gs ? gscale[0] : 1.0f;
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
            for (int s = 1; s < S; ++s) v[c] = __fadd_rn(v[c], part[s][c]);
            if (has_gs) v[c] = __fmul_rn(v[c], gs);
            if (bias != nullptr) v[c] = __fadd_rn(v[c], b[c]);
        }
        store_out4(out, OUT, (size_t)t * N, n, N, vec, v);
    }
#endif
}
