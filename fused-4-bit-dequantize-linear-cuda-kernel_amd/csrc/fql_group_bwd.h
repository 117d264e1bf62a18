// Input gradient of the grouped INT4 GEMM with per-GROUP scales along K (scales / zps [E][N][K / group]):
//
//   dX[t][k] = sum_n dY[t][n] * s[e][n][g(k)] * (q[e][n][k] - zp[e][n][g(k)]),        g(k) = k / group
//
// The integer scheme of fql_bwd.h folds the one scale of a weight row into the gradient row before it is cut into limbs.
// Here the scale varies with the contraction index n AND with the group of the output k, so that fold would need one
// limb set per group: it does not apply.  The weights are dequantised in registers instead, exactly as the forward's
// float32 kernel does (fql_group.h: dq = (q - zp) * scale), and the contraction runs on v_mfma_f32_32x32x2f32: float32
// products, float32 accumulation, bit for bit a chain of fmaf in the order the instructions are issued.  157 TFLOP/s is
// that instruction's ceiling, 1/32 of the INT8 rate of fql_bwd.h: the batch path of an additive option.
//
// group_bwd_kernel: workgroup = 4 waves = a tile of 64 rows t x 128 columns k of one expert; the expert table is read on
// the device (blockIdx.z = expert, row blocks past its count leave at once).  The weights are the MFMA's A operand
// (rows = k), the gradient rows its B operand (columns = t), so a lane owns one output row t and registers 4q .. 4q+3 of
// an accumulator are 4 consecutive k: 16-byte stores.  Wave w takes the 32 rows (w >> 1) and the two 32-k blocks
// 2 (w & 1), 2 (w & 1) + 1, which share its gradient registers.
//   * Weight stage = 64 n x 128 k.  Thread p reads ONE 16-byte piece of a packed row (row n0 + (p >> 2), the 32 k of
//     piece p & 3: group % 32 == 0 keeps a piece inside one group, so one scale and one zero point per piece),
//     dequantises its 32 nibbles and writes them to the LDS image [64 n][128 k] of float32 (8 x 16 bytes), double
//     buffered (2 x 32 KiB): one workgroup barrier per stage.  Pieces past N or K are written as zeros.
//   * A operand: lane (i = lane & 31, h = lane >> 5) reads image[s + 32 h][32 b + i] for step s: 32 consecutive floats
//     per half with ds_read_b32, whose banking is per 32-lane half: conflict-free without padding.
//   * B operand: lane (j = lane & 31, h) holds dY[t_j][n0 + 32 h .. n0 + 32 h + 31] of the stage in registers (16-byte
//     loads of the row as it is, float16 / bfloat16 widened in registers), one stage ahead of the arithmetic.
//   * FIXED ORDER.  Stage n0 = 0, 64, ... ; inside a stage step s = 0 .. 31 contracts n0 + s, then n0 + 32 + s.  A
//     row's result is that chain of fmaf over its own gradient row and the weights: it does not depend on the other
//     rows of its tile, on E or on the table, so the grouped call equals E one-expert calls bit for bit.  Indices past N
//     contribute fmaf(0, 0, acc).
//   * No atomics, every element is written once.  With a table the launch carries one more z-slice whose workgroups zero
//     the rows of dX that no expert covers (act_zero_uncovered, fql_act_quant.h).
//
// group_bwd_rows_kernel: the fallback for every other shape (K % 64 != 0, group % 32 != 0, a base that is not 16-byte
// aligned): one wave per row t, lane = k, the same chain of fmaf in the same order.  Correct, not tuned.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

struct GroupBwdCfg {
    static constexpr int BT = 64, BK = 128, BN = 64;   // rows, columns and contraction depth of a stage
    static constexpr int THREADS = 256;
};

// element n of a gradient row of type IN, widened
template <int IN>
__device__ __forceinline__ float group_bwd_elem(const void *row, int n)
{
    if (IN == 0) return reinterpret_cast<const float *>(row)[n];
    return act_widen<IN>(reinterpret_cast<const unsigned short *>(row)[n]);
}

// OUT: element type of gx (FQL_DTYPE_*), rounded once in the epilogue (store_out4, fql_common.h)
template <int IN, int OUT>
__global__ __launch_bounds__(256) void group_bwd_kernel(
    const void *__restrict__ gy, const uint8_t *__restrict__ packed, const float *__restrict__ scales,
    const float *__restrict__ zps, void *__restrict__ gx, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N, int group)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = GroupBwdCfg;
    if ((int)blockIdx.z == E) {                                    // (with a table only) the rows no expert covers
        const int blk = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        if ((long long)blk * 256 < T) act_zero_uncovered(blk, gx, OUT == 0 ? 4 : 2, K, tpe, offs, E, T);
        return;
    }
    __shared__ __attribute__((aligned(16))) float image[2][C::BN][C::BK];

    const int e = blockIdx.z;
    int row_lo = 0, cnt = T;
    if (tpe != nullptr) expert_range(tpe, offs, e, T, row_lo, cnt);
    const int t_blk = (int)blockIdx.y * C::BT;
    if (t_blk >= cnt) return;                                      // (uniform per workgroup)
    const int k0 = (int)blockIdx.x * C::BK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int kb = (wave & 1) * 2;                                 // first of this wave's two 32-k blocks
    const int rl = t_blk + (wave >> 1) * 32 + l31;                 // this lane's row inside the expert's range
    const bool row_ok = rl < cnt;
    const int t = row_lo + (row_ok ? rl : cnt - 1);                // (clamped: loads are unconditional)
    const int K2 = K >> 1, G = K / group;
    const int es = IN == 0 ? 4 : 2;
    const char *grow = reinterpret_cast<const char *>(gy) + (size_t)t * N * es;
    const bool vec_n = (N % (16 / es) == 0);                       // every 16-byte piece of a gradient row is aligned and whole

    // staging role of this thread: row sn of the stage, 16-byte piece sp (32 k)
    const int sn = tid >> 2, sp = tid & 3;
    const int kp = k0 + 32 * sp;
    const uint8_t *wbase = packed + (size_t)e * N * K2 + (kp >> 1);
    const float *sbase = scales + (size_t)e * N * G + kp / group;
    const float *zbase = zps + (size_t)e * N * G + kp / group;

    uint4 wq;
    float sc, zp;
    auto load_w = [&](int n0) {                                    // stage n0: packed piece + its two constants -> registers
        const int n = n0 + sn;
        const bool ok = n < N && kp < K;
        wq = make_uint4(0u, 0u, 0u, 0u);
        sc = 0.0f;
        zp = 0.0f;
        if (ok) {
            wq = *reinterpret_cast<const uint4 *>(wbase + (size_t)n * K2);
            sc = sbase[(size_t)n * G];
            zp = zbase[(size_t)n * G];
        }
    };
    auto store_w = [&](float (*buf)[C::BK]) {                      // registers -> LDS image (dequantised, natural k order)
        const uint32_t words[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v4f o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int nib = 4 * i + c;                         // nibble nib of the 16 bytes is k = kp + nib
                const float q = (float)((words[nib >> 3] >> (4 * (nib & 7))) & 0xFu);
                o[c] = (q - zp) * sc;                              // the forward's dq (fql_group.h)
            }
            *reinterpret_cast<v4f *>(&buf[sn][32 * sp + 4 * i]) = o;
        }
    };
    float gn[32];
    auto load_g = [&](int n0) {                                    // dY[t][n0 + 32 h + (0 .. 31)], widened; zeros past N
        const int nb = n0 + 32 * h;
        if (vec_n) {
            if (IN == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v4f v = v4f{0.0f, 0.0f, 0.0f, 0.0f};
                    if (nb + 4 * i < N) v = *reinterpret_cast<const v4f *>(grow + (size_t)(nb + 4 * i) * 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) gn[4 * i + c] = v[c];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (nb + 8 * i < N) v = *reinterpret_cast<const uint4 *>(grow + (size_t)(nb + 8 * i) * 2);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        gn[8 * i + 2 * c] = act_widen<IN>((unsigned short)(w[c] & 0xFFFFu));
                        gn[8 * i + 2 * c + 1] = act_widen<IN>((unsigned short)(w[c] >> 16));
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 32; ++i) gn[i] = nb + i < N ? group_bwd_elem<IN>(grow, nb + i) : 0.0f;
        }
    };

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;

    load_w(0);
    load_g(0);
    store_w(image[0]);
    __syncthreads();
    int it = 0;
    for (int n0 = 0; n0 < N; n0 += C::BN, ++it) {
        float gc[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) gc[i] = gn[i];
        const bool more = n0 + C::BN < N;
        if (more) {                                                // the next stage's loads, ahead of this stage's arithmetic
            load_w(n0 + C::BN);
            load_g(n0 + C::BN);
        }
        const float(*cur)[C::BK] = image[it & 1];
#pragma unroll
        for (int s = 0; s < 32; ++s) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float a = cur[s + 32 * h][32 * (kb + b) + l31];
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gc[s], acc[b], 0, 0, 0);
            }
        }
        if (more) store_w(image[(it + 1) & 1]);                    // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    }

    // D[i][j]: i = k (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are k = 8 q + 4 h + (0 .. 3) of the block
    if (!row_ok) return;
    const bool vec = (reinterpret_cast<uintptr_t>(gx) & (OUT == 0 ? 15 : 7)) == 0;     // (K % 64 == 0)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kc = k0 + 32 * (kb + b) + 8 * q + 4 * h;
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = acc[b][4 * q + c];
            if (kc < K) store_out4(gx, OUT, (size_t)t * K, kc, K, vec, v);
        }
#endif
}

// One wave per row t: the expert that covers it is found in the table (the first one, if ranges overlap), every lane takes
// the columns k = lane, lane + 64, ... and runs the chain of group_bwd_kernel: stage by stage, n0 + s then n0 + 32 + s.
template <int IN, int OUT>
__global__ __launch_bounds__(64) void group_bwd_rows_kernel(
    const void *__restrict__ gy, const uint8_t *__restrict__ packed, const float *__restrict__ scales,
    const float *__restrict__ zps, void *__restrict__ gx, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N, int group)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int t = blockIdx.x, lane = threadIdx.x;
    int e = tpe == nullptr ? 0 : -1;
    if (tpe != nullptr) {
        for (int i = 0; i < E && e < 0; ++i) {
            int lo, cnt;
            expert_range(tpe, offs, i, T, lo, cnt);
            if (t >= lo && t < lo + cnt) e = i;
        }
    }
    const int K2 = K >> 1, G = K / group;
    const char *grow = reinterpret_cast<const char *>(gy) + (size_t)t * N * (IN == 0 ? 4 : 2);
    for (int k = lane; k < K; k += 64) {
        float acc = 0.0f;
        if (e >= 0) {
            const uint8_t *wcol = packed + (size_t)e * N * K2 + (k >> 1);
            const float *scol = scales + (size_t)e * N * G + k / group;
            const float *zcol = zps + (size_t)e * N * G + k / group;
            const int shift = 4 * (k & 1);
            for (int n0 = 0; n0 < N; n0 += GroupBwdCfg::BN)
                for (int s = 0; s < 32; ++s)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int n = n0 + 32 * hh + s;
                        float w = 0.0f, g = 0.0f;
                        if (n < N) {
                            const float q = (float)((wcol[(size_t)n * K2] >> shift) & 0xFu);
                            w = (q - zcol[(size_t)n * G]) * scol[(size_t)n * G];
                            g = group_bwd_elem<IN>(grow, n);
                        }
                        acc = fmaf(w, g, acc);
                    }
        }
        // float16: round the float32 result, never the last fmaf rounded straight to float16 (fql_bwd.h, epilogue)
        if constexpr (OUT == 1) asm volatile("" : "+v"(acc));
        if (OUT == 0) reinterpret_cast<float *>(gx)[(size_t)t * K + k] = acc;
        else reinterpret_cast<unsigned short *>(gx)[(size_t)t * K + k] = OUT == 1 ? f32_to_f16_bits(acc) : f32_to_bf16_bits(acc);
    }
#endif
}
