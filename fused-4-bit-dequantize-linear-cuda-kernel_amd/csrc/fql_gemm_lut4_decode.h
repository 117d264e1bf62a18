// The dense 4-bit code-book (NF4) linear layer at decode (include/fql_int4.h, fql_linear_lut4_split_fwd):
// lut4_kernel's product at one to a few dozen rows, cut along K, and the kernel that adds the pieces up and adds the bias.
//
// lut4_kernel is a tile 256 token rows tall on a grid of ceil(N / 128) workgroups: at one row 4096 -> 4096 runs on 32 of
// 256 compute units.  Here the grid is section 43's, (ceil(N / 32), ceil(T / 32), S):
//
// lut4_decode_kernel<IN>: workgroup = ONE wave = 32 weight rows n x one block of up to 32 rows t x slice s of K.
//   * The weight is lut4_kernel's, bit for bit: W[n][k] = bf16_rn( fl32( code_book[c] * absmax[n][k / B] ) ), the weights as
//     the A operand of v_mfma_f32_32x32x16_bf16.  Lane (r, h) streams the 16 bytes of codes k = 64 j + 32 h .. + 31 of weight
//     row n0 + r as they are stored (bitsandbytes' nibble order) and two v_permlane32_swap hand each half the dword of its
//     8 k of every step, as mx4_decode_body does.  K % 64 == 0 and B >= 64: a pair of 64 k has exactly one absmax per weight
//     row and there is no odd piece.
//   * Slices.  P = K / 64 pairs; slice s runs pairs [s * ceil(P / S), min(P, (s + 1) * ceil(P / S))) in ascending order on an
//     accumulator that starts at zero.  A slice with nothing to do stores zeros.
//   * THE CONVERSION.  Every code is converted exactly once, by the wave that streams it, so the instructions of a code sit
//     directly against the wave's share of the HBM rate.  Two forms, the same W bits (FQL_LUT4_DECODE_PREMUL chooses):
//       0: lut4_dequant8 (mechanism (a) of section 44): the 16 float32 entries in the workgroup's LDS; a code is one
//          ds_read_b32, its address, one v_mul_f32 and half a v_cvt_pk_bf16_f32.
//       1: a table PREMULTIPLIED once per pair.  Lane (r, h) multiplies entries 8 h .. 8 h + 7 of the table (kept in eight
//          registers) by the pair's absmax of row r, rounds them to bfloat16 (8 v_mul_f32, 4 v_cvt_pk_bf16_f32: the very
//          operations lut4_dequant8 does per code, so the same bits) and writes them to column r of a 16 x 32 image of
//          dwords in LDS (2 KiB; entry c of row r at byte 128 c + 4 r: the 32 lanes of a half wave read 32 different
//          banks whatever their codes).  A code is then ONE 16-bit LDS read and its address; no multiply, no convert.
//          48 products and 24 packs less per lane and pair, for 8 LDS writes.
//     Measured at one row: form 0 is as fast or up to 5 % faster, so it is the default; the kernel
//     is not bound by the conversion, and form 1 pays two dependent LDS round trips a pair.
//   * The ring: FQL_LUT4_DECODE_DEPTH slots of one pair each (float32 rows: half as many), refilled GROUP at a time as
//     nv4_linear_decode_body does; a slot is the 16 bytes of codes, the absmax and the four row fragments.
//   * Epilogue: a plain float32 store of the partial sum to partial[s][t][n], rows t < T and columns n < N only.  Weight
//     rows past N and token rows past T read a clamped row and are never stored.
//   * NON-FINITE, without a flag word: a slice whose part of a row is non-finite stores NaN for that whole partial row, and
//     NaN + anything is NaN in the reduce kernel.  absmax and the table are not screened.
//   * Rows whose base is not 16-byte aligned take the element-load form with a ring of one slot, as everywhere.
//
// lut4_linear_reduce_kernel<OUT, S>: out[t][n] = round_OUT( fl32( (((p_0 + p_1) + ...) + p_{S-1}) + bias[n] ) ), float32, the
// order fixed, every element written once: nv4_linear_reduce_kernel's twin without a global scale.  S = 1 runs it too (there
// is no one-wave kernel to fall back on): the bits of every S come from one epilogue.
//
// Two launches on one stream; the launch boundary is the only synchronisation (no atomics, no flags, graph-capturable).
// Compiled without the packed float32 instructions, contraction off in the conversion; no scratch.
#pragma once
#include "fql_gemm_lut4.h"
#include "fql_gemm_nvfp4_linear.h"

#ifndef FQL_LUT4_DECODE_DEPTH
#define FQL_LUT4_DECODE_DEPTH 4            // ring slots of the bfloat16-row kernel (A/B knob; float32 rows take half as many)
#endif
#ifndef FQL_LUT4_DECODE_PREMUL
#define FQL_LUT4_DECODE_PREMUL 0           // 0: lut4_dequant8 on the float32 table (measured faster); 1: the per-pair premultiplied table
#endif

struct Lut4DecodeCfg {
    static constexpr int DEPTH_BF16 = FQL_LUT4_DECODE_DEPTH, DEPTH_F32 = DEPTH_BF16 > 1 ? DEPTH_BF16 / 2 : 1;
    static constexpr int GROUP_BF16 = DEPTH_BF16 >= 4 ? 4 : DEPTH_BF16, GROUP_F32 = DEPTH_F32 >= 2 ? 2 : 1;
    static constexpr bool PREMUL = FQL_LUT4_DECODE_PREMUL != 0;
    static constexpr int TAB_PITCH = 64;   // 16-bit elements between two entries of the premultiplied image (128 bytes)
};

// One ring slot: the piece of 32 codes, the pair's absmax of the lane's weight row and the four row fragments of 64 k.
template <int IN>
struct Lut4DecodeSlot {
    uint4 wq;
    float am;
    typename std::conditional<IN == 0, float, uint32_t>::type x[4][IN == 0 ? 8 : 4];
};

// One dword of a packed piece through the premultiplied image: col points at the lane's column (entry c at col[64 c]).
__device__ __forceinline__ uint4 lut4_lookup8(uint32_t w, const unsigned short *col)
{
    constexpr int P = Lut4DecodeCfg::TAB_PITCH;
    uint32_t o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        typedef unsigned short v2us __attribute__((ext_vector_type(2)));
        v2us p;
        p[0] = col[((w >> (8 * b + 4)) & 15u) * P];                // even k: the HIGH nibble
        p[1] = col[((w >> (8 * b)) & 15u) * P];
        o[b] = __builtin_bit_cast(uint32_t, p);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// tab: PREMUL the image of 16 x 64 bfloat16 (every other one used), else the 16 float32 entries, viewed as bytes.
template <int IN, bool VEC, bool PREMUL, int DEPTH, int GROUP>
__device__ __forceinline__ void lut4_decode_body(
    void *tab, const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, float *__restrict__ partial, int bshift, int T, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Lut4DecodeSlot<IN>;
    using C = Lut4DecodeCfg;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN, t_blk = (int)blockIdx.y * Mx4DecodeCfg::BT;
    const int slice = blockIdx.z, S = gridDim.z;
    const int K2 = K >> 1, KB = K >> bshift;
    constexpr int es = IN == 0 ? 4 : 2;
    // Loads are unconditional: a lane past N reads row N - 1, a lane past T reads row T - 1 (neither is stored).
    const size_t wrow = (size_t)(n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = codes + wrow * K2 + 16 * h;
    const float *abase = absmax + wrow * KB;
    const bool row_ok = t_blk + r < T;
    const int t = row_ok ? t_blk + r : T - 1;
    const char *xrow = reinterpret_cast<const char *>(x) + ((size_t)t * K + 8 * h) * es;

    // The table.  PREMUL: entries 8 h .. 8 h + 7 in registers; else all 16 in LDS.
    float bk[8];
    float *lut = reinterpret_cast<float *>(tab);
    unsigned short *img = reinterpret_cast<unsigned short *>(tab);
    if constexpr (PREMUL) {
#pragma unroll
        for (int i = 0; i < 8; ++i) bk[i] = book != nullptr ? book[8 * h + i] : lut4_nf4_book[8 * h + i];
    } else {
        lut4_load_table(lut, book);
        __syncthreads();
    }
    unsigned short *wcol = img + 8 * h * C::TAB_PITCH + 2 * r;    // where the lane writes its eight entries of column r
    const unsigned short *col = img + 2 * r;                       // the column it reads

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
    auto load_slot = [&](Slot &sl, int j) {                        // the 64 k of pair j (codes is 16-byte aligned, K2 % 32 == 0)
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * j);
        sl.am = abase[(64 * j) >> bshift];
#pragma unroll
        for (int s = 0; s < 4; ++s) load_x(sl, j, s);
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    uint32_t bad = 0u;

    auto consume = [&](const Slot &sl) {                           // four instructions: k0 = 64 j + 16 s, s = 0 .. 3
        uint32_t w[4], own;
        mx4_decode_copy(sl.wq, 0u, w, own);                        // (the swaps overwrite copies)
        const auto lo = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);         // {d0 | d1}, {e0 | e1}
        const auto hi = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);         // {d2 | d3}, {e2 | e3}
        const uint32_t words[4] = {lo[0], hi[0], lo[1], hi[1]};
        if constexpr (PREMUL) {
#pragma clang fp contract(off)
            __syncthreads();                                       // (one wave: no s_barrier; the last pair's reads are done)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t p = mx4_pack_bf16(__fmul_rn(bk[2 * i], sl.am), __fmul_rn(bk[2 * i + 1], sl.am));
                wcol[(2 * i) * C::TAB_PITCH] = (unsigned short)p;
                wcol[(2 * i + 1) * C::TAB_PITCH] = (unsigned short)(p >> 16);
            }
            __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 a;
            if constexpr (PREMUL) a = lut4_lookup8(words[s], col);
            else a = lut4_dequant8(words[s], sl.am, lut);
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

    // The slice's pairs [lo, hi) (wave-uniform).
    const int pairs = K >> 6;
    const int per = (pairs + S - 1) / S;
    const int lo = slice * per < pairs ? slice * per : pairs;
    const int hi = lo + per < pairs ? lo + per : pairs;

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

// IN as lut4_kernel's (0 float32 rows, 2 bfloat16 rows); the partial sums are float32.  bshift = log2(B).
template <int IN>
__global__ __launch_bounds__(64) FQL_LUT4_TARGET void lut4_decode_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, float *__restrict__ partial, int bshift, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Lut4DecodeCfg;
    __shared__ __attribute__((aligned(16))) unsigned short tab[C::PREMUL ? 16 * C::TAB_PITCH : 32];
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        lut4_decode_body<IN, true, C::PREMUL, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(
            tab, codes, absmax, book, x, partial, bshift, T, K, N);
    else
        lut4_decode_body<IN, false, C::PREMUL, 1, 1>(tab, codes, absmax, book, x, partial, bshift, T, K, N);
#endif
}

// partial [S][T][N] float32 -> out [T][N] of OUT (+ bias [N] or NULL): nv4_linear_reduce_kernel's twin without a global scale,
// on its grid (Nv4LinearReduceCfg).  A twin and not a shared body: moving nv4_linear_reduce_kernel's body into an inline
// function changed that kernel's register allocation and schedule.
template <int OUT, int S>
__global__ __launch_bounds__(256) FQL_LUT4_TARGET void lut4_linear_reduce_kernel(
    const float *__restrict__ partial, const float *__restrict__ bias, void *__restrict__ out, int T, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    using C = Nv4LinearReduceCfg;
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
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < S; ++s) {                              // ((p_0 + p_1) + ...) + p_{S-1}, v starts as p_0
            float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (vec) {
                const v4f q = *reinterpret_cast<const v4f *>(p + s * plane);
#pragma unroll
                for (int c = 0; c < 4; ++c) part[c] = q[c];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) if (n + c < N) part[c] = p[s * plane + c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = s == 0 ? part[c] : __fadd_rn(v[c], part[c]);
        }
        if (bias != nullptr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = __fadd_rn(v[c], b[c]);
        }
        store_out4(out, OUT, (size_t)t * N, n, N, vec, v);
    }
#endif
}
