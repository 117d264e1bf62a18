// The decode forms of lut4_group_kernel (fql_gemm_lut4_group.h): the grouped GEMM on 4-bit code-book (NF4) expert weights for a
// FEW rows an expert, where the call is a weight stream and a 128 x 128 tile with a barrier every 32 k converts every code
// for 128 token rows that are not there (include/fql_int4.h, fql_moe_lut4_fwd / fql_moe_lut4_split_fwd).
//
// lut4_group_decode_kernel<IN, OUT>: workgroup = ONE wave = 32 weight rows n of one expert x one block of up to 32 of that
// expert's rows t, for all of K.  grid = (ceil(N / 32), ceil(T / 32), E (+ 1 with a table)) behind mx4_group_begin, as
// mx4_decode_kernel: the coverage slice zeroes the rows no expert covers, the workgroups of an expert without rows in that
// block leave at once, a count above 32 is the next row block's, so the kernel is right for every T.
//   * THE SAME BITS AS lut4_group_kernel, by the argument at the top of fql_gemm_mx4_decode.h: an element of an MFMA's
//     result depends on its own A row, its own B column and its own accumulator only, and the sequence agrees:
//     v_mfma_f32_32x32x16_bf16 with the weights as A and the rows as B, k0 = 0, 16, 32, ... one instruction per 16 k on ONE
//     accumulator that starts at zero, lane (r, h) supplying W[n_r][k0 + 8 h .. + 7] and x[t_r][k0 + 8 h .. + 7];
//     lut4_dequant8 as it is (the 16 float32 entries in LDS, one v_mul_f32 and half a v_cvt_pk_bf16_f32 a code, contraction
//     off, no packed float32 instructions), mx4_pack_bf16 on float32 rows; nv4_epilogue with the expert's bias row and no
//     global scale; the row's NaN flag.  Hence also fql_linear_lut4_fwd's bits on the expert's matrix.
//   * Weights.  Lane (r, h) streams the 16 bytes of codes k = 64 j + 32 h .. + 31 of weight row e N + n0 + r as they are
//     stored; two v_permlane32_swap (behind mx4_decode_copy) hand each half the dword of its 8 k of every 16-k step, as
//     lut4_decode_body does.  K % 64 == 0 and block >= 64 (lut4_check): a pair of 64 k has one absmax per weight row.
//   * Rows.  The lane loads its own fragments from global memory.  A row past the expert's count is the expert's last row
//     again (inside the expert's range; never stored); a weight row past N is row N - 1 of the expert (never stored).
//   * Ring.  Lut4DecodeCfg's: FQL_LUT4_DECODE_DEPTH slots of one pair each (float32 rows: half), refilled GROUP at a time:
//     the stream a lane sees is the dense decode kernel's, so its measured depth is taken over and the knob is shared.  Rows
//     whose base is not 16-byte aligned take the element-load form with a ring of one slot.
//   * Weight and absmax offsets are size_t: E N K / 2 passes 4 GiB at real sizes.
//   * 64 bytes of LDS (the table), one barrier (one wave: no s_barrier instruction), no scratch.
//
// lut4_group_sdecode_kernel<IN>: the same body on slice s of K, lut4_decode_body's arithmetic: P = K / 64 pairs, slice s runs
// pairs [s * ceil(P / S), min(P, (s + 1) * ceil(P / S))) in ascending order from zero and stores its float32 partial sums to
// partial[s][t][n], live rows and columns only.  An empty slice stores zeros; a slice that saw a non-finite element of a
// row stores NaN for that partial row.  grid = (ceil(N / 32), ceil(T / 32), E * S), z = e * S + s: no coverage slice (the
// reduce kernel has it), and the host bounds E * 16 by the grid's z before any HIP call.
//
// lut4_group_reduce_kernel<OUT, S>: out[t][n] = round_OUT( fl32( (((p_0 + p_1) + ...) + p_{S-1}) + bias[e][n] ) ), the order
// fixed, every element written once, no atomics.  grid = (ceil(N / 256), ceil(T / 32), E (+ 1 with a table)) behind
// mx4_group_begin: it knows its expert (the bias row, the live rows) and its coverage slice zeroes the uncovered rows of out.
// lut4_linear_reduce_kernel's twin, not a shared body (moving a reduce kernel's body into an inline
// function changed that kernel's schedule).  S = 1 runs it too, so the bits of every S come from one epilogue.
// Two launches on one stream; the launch boundary is the only synchronisation (graph-capturable).
#pragma once
#include "fql_gemm_lut4_decode.h"

struct Lut4GroupReduceCfg {
    static constexpr int THREADS = 256, QUADS = 64, ROWS = THREADS / QUADS;   // a workgroup: 4 rows x 64 quads of columns at a time
    static constexpr int COLS = 4 * QUADS, BT = Mx4DecodeCfg::BT;             // ... over a block of 32 of the expert's rows
};

// SPLIT: slice `slice` of S into partial (dst; OUT and bias unused); else all of K into out (dst) through nv4_epilogue.
// Expert e holds rows row_lo .. row_lo + cnt - 1; the workgroup's block starts at row t_blk of them (t_blk < cnt).
// lut: the table's 16 entries in LDS, loaded and behind the caller's barrier.
template <int IN, int OUT, bool SPLIT, bool VEC, int DEPTH, int GROUP>
__device__ __forceinline__ void lut4_group_decode_body(
    const float *lut, const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const void *__restrict__ x,
    const float *__restrict__ bias, void *__restrict__ dst, int bshift, int e, int row_lo, int cnt, int t_blk, int slice, int S,
    int T, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Lut4DecodeSlot<IN>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN;
    const int K2 = K >> 1, KB = K >> bshift;
    constexpr int es = IN == 0 ? 4 : 2;
    // Loads are unconditional: a lane past N reads the expert's row N - 1, a lane past the count the expert's last row
    // (neither is stored, and neither reaches another lane's results).
    const size_t wrow = (size_t)e * N + (n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = codes + wrow * K2 + 16 * h;
    const float *abase = absmax + wrow * KB;
    const bool row_ok = t_blk + r < cnt;
    const int t = row_lo + (row_ok ? t_blk + r : cnt - 1);
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
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 a = lut4_dequant8(words[s], sl.am, lut);
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

    // The pairs [lo, hi) of this workgroup (wave-uniform): all of them, or the slice's.
    const int pairs = K >> 6;
    int lo = 0, hi = pairs;
    if constexpr (SPLIT) {
        const int per = (pairs + S - 1) / S;
        lo = slice * per < pairs ? slice * per : pairs;
        hi = lo + per < pairs ? lo + per : pairs;
    }

    // No branch in the loop that loads: a slot index past the last pair loads that pair again (inside the slice, so inside
    // the operands) and is not used.
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
    const auto both = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);   // the row's other half of k
    if (!row_ok) return;
    const bool row_nan = ((both[0] | both[1]) & 0x80008000u) != 0u;
    if constexpr (SPLIT) {
        float *partial = reinterpret_cast<float *>(dst);
        const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 15) == 0;
        const size_t prow = ((size_t)slice * T + t) * N;           // partial[s][t][.]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nc = n0 + 8 * q + 4 * h;
            if (nc >= N) continue;
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = row_nan ? __uint_as_float(0x7FC00000u) : acc[4 * q + c];
            store_out4(partial, 0, prow, nc, N, vec, v);
        }
    } else {
        const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & (OUT == 0 ? 15 : 7)) == 0;
        const float *brow = bias != nullptr ? bias + (size_t)e * N : nullptr;
        nv4_epilogue<OUT>(acc, dst, t, N, n0, h, vec, brow, false, 1.0f, row_nan);
    }
}

// The two forms of the rows' loads around one body.
template <int IN, int OUT, bool SPLIT>
__device__ __forceinline__ void lut4_group_decode_run(
    const float *lut, const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const void *__restrict__ x,
    const float *__restrict__ bias, void *__restrict__ dst, int bshift, int e, int row_lo, int cnt, int t_blk, int slice, int S,
    int T, int K, int N)
{
    using C = Lut4DecodeCfg;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)                // (K % 64 == 0: every row and fragment is aligned then)
        lut4_group_decode_body<IN, OUT, SPLIT, true, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(
            lut, codes, absmax, x, bias, dst, bshift, e, row_lo, cnt, t_blk, slice, S, T, K, N);
    else
        lut4_group_decode_body<IN, OUT, SPLIT, false, 1, 1>(lut, codes, absmax, x, bias, dst, bshift, e, row_lo, cnt, t_blk, slice, S,
                                                            T, K, N);
}

// IN, OUT as lut4_group_kernel's, and its arguments.
template <int IN, int OUT>
__global__ __launch_bounds__(64) FQL_LUT4_TARGET void lut4_group_decode_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int bshift, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4DecodeCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    __shared__ float lut[16];
    lut4_load_table(lut, book);
    __syncthreads();
    lut4_group_decode_run<IN, OUT, false>(lut, codes, absmax, x, bias, out, bshift, (int)blockIdx.z, row_lo, cnt, t_blk, 0, 1, T, K, N);
#endif
}

// The sliced form: z = e * S + s, no coverage slice; partial [S][T][N] float32.
template <int IN>
__global__ __launch_bounds__(64) FQL_LUT4_TARGET void lut4_group_sdecode_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, float *__restrict__ partial, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
    int bshift, int S, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int e = (int)blockIdx.z / S, slice = (int)blockIdx.z - e * S;
    int row_lo = 0, cnt = T;
    if (tpe != nullptr) expert_range(tpe, offs, e, T, row_lo, cnt);
    const int t_blk = (int)blockIdx.y * Mx4DecodeCfg::BT;
    if (t_blk >= cnt) return;                                      // (uniform per workgroup, before the barrier)
    __shared__ float lut[16];
    lut4_load_table(lut, book);
    __syncthreads();
    lut4_group_decode_run<IN, 0, true>(lut, codes, absmax, x, nullptr, partial, bshift, e, row_lo, cnt, t_blk, slice, S, T, K, N);
#endif
}

// partial [S][T][N] float32 -> the live rows of out [T][N] of OUT (+ bias [E][N] or NULL), the rows no expert covers zeroed.
template <int OUT, int S>
__global__ __launch_bounds__(256) FQL_LUT4_TARGET void lut4_group_reduce_kernel(
    const float *__restrict__ partial, const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    using C = Lut4GroupReduceCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    const int n = (int)blockIdx.x * C::COLS + 4 * ((int)threadIdx.x & (C::QUADS - 1));
    if (n >= N) return;
    const float *brow = bias != nullptr ? bias + (size_t)blockIdx.z * N : nullptr;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(partial) & 15) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const size_t plane = (size_t)T * N;
    float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (brow != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c) if (n + c < N) b[c] = brow[n + c];
    }
    const int t_end = t_blk + C::BT < cnt ? t_blk + C::BT : cnt;
    for (int tl = t_blk + ((int)threadIdx.x >> 6); tl < t_end; tl += C::ROWS) {
        const int t = row_lo + tl;
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
        if (brow != nullptr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = __fadd_rn(v[c], b[c]);
        }
        store_out4(out, OUT, (size_t)t * N, n, N, vec, v);
    }
#endif
}
