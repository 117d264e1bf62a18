// Grouped GEMM on OCP MXFP4 expert weights (include/fql_int4.h, fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd):
//
//   out[t][n] = sum_k bf16(x[t][k]) * W_e[n][k] (+ bias[e][n]),     W_e[n][k] = e2m1(code[e][n][k]) * 2^(s[e][n][k / 32] - 127)
//
// blocks [E][N][K / 2] uint8 (even k in the low nibble, the INT4 byte layout), scales [E][N][K / 32] uint8 (E8M0, 255 = NaN).
// The element codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6 and 8 .. 15 their negatives; every such value times a power of two
// is exact in bfloat16 (two mantissa bits), so the weights are dequantised to bfloat16 without an error and the contraction
// runs on v_mfma_f32_32x32x16_bf16 with float32 accumulation.  The activations are rounded once to bfloat16 (to nearest
// even) unless they already are.  The dequantised matrix exists in LDS only.
//
// mx4_kernel: workgroup = 4 waves = a tile of 64 rows t x 128 columns n of one expert; the expert table is read on the
// device (blockIdx.z = expert, row blocks past its count leave at once).  The weights are the MFMA's A operand (rows = n),
// the activation rows its B operand (columns = t), so a lane owns one output row t and registers 4q .. 4q+3 of an
// accumulator are 4 consecutive n: 16-byte stores (store_out4).  Wave w takes the 32 rows (w >> 1) and the two 32-n blocks
// 2 (w & 1), 2 (w & 1) + 1, which share its activation registers.  (The skeleton is group_bwd_kernel's, fql_group_bwd.h.)
//   * Weight stage = 128 n x 64 k.  Thread p reads ONE 16-byte piece of a packed row (row n0 + (p >> 1), the 32 k of piece
//     p & 1: exactly one scale block, so one scale byte per piece), converts its 32 codes to bfloat16 and writes them to the
//     LDS image [128 n][64 k (+ 8 pad)] of bfloat16 (4 x 16 bytes), double buffered (2 x 18 KiB): one workgroup barrier per
//     stage.  Pieces past N or K are written as zeros: K % 32 == 0 is all the kernel asks, a last stage of 32 k is the
//     normal case (gpt-oss: K = 2880 = 45 stages).
//   * A operand: lane (r = lane & 31, h = lane >> 5) reads image[32 b + r][16 s + 8 h .. + 7] for step s: one ds_read_b128;
//     the 144-byte row pitch spreads the 32 rows of a half over the banks.
//   * Activation stage = 64 t x 64 k.  Thread p reads the 16 k of quarter p & 3 of row p >> 2 as they are (16-byte loads,
//     four threads a 128-byte line of a bfloat16 row), rounds float32 to bfloat16 in registers and writes the second LDS
//     image [64 t][64 k (+ 8 pad)], double buffered as well (2 x 9 KiB).  (A lane that loads its own fragment from its own
//     row touches 32 cache lines per load instruction, and both waves of a row block do it again: that form spent its time
//     in the vector memory pipeline.)
//   * B operand: the lane reads ximage[t_r][16 s + 8 h .. + 7] for step s: one ds_read_b128, shared by its two n blocks.
//   * The loads of a stage (packed piece, scale byte, activations) are issued TWO stages ahead of their use, into two
//     register sets that alternate.
//   * FIXED ORDER.  Stage k0 = 0, 64, ... ; inside a stage step s = 0 .. 3 contracts k0 + 16 s .. + 15 with one instruction.
//     A row's result is that sequence over its own activation row and its expert's weights: it does not depend on the
//     other rows of its tile, on T, E or the table, so the grouped call equals E one-expert calls bit for bit.
//     With LORA (below) one adapter stage follows the last weight stage: steps s with 16 s < r contract j = 16 s .. + 15 of
//     the shrunk row and the adapter matrix.  A row's result is then that sequence over its own rows of x and v and its
//     expert's W and B, and nothing else.
//   * NON-FINITE.  A scale code 255 makes the 32 weights of its block NaN (zeros included), hence NaN in every output of
//     that weight row for the rows of that expert.  A non-finite activation must make its whole output row NaN (the
//     project's convention); Inf * w is only NaN where w == 0, so the staging thread flags the row in LDS when a bfloat16
//     word it writes has an exponent field of 255, and the epilogue writes NaN across a flagged row.
//   * RANGE.  2^(s - 127) * |e2m1| below 2^-126 (scale codes 0 and 1 with the smallest codes) may be flushed to zero.
//   * No atomics, every element is written once.  With a table the launch carries one more z-slice whose workgroups zero
//     the rows of out that no expert covers (mx4_group_begin, fql_mx4_common.h).
//
//   * LORA (mx4_kernel<IN, OUT, Mx4Lora>; fql_moe_mx4_lora_fwd / fql_moe_mx4_glu_lora_fwd): a low-rank adapter
//     fused in as one more stage of the same loop,
//       out[t][n] = round_OUT( sum_k bf16(x[t][k]) W_e[n][k] + sum_{j < r} bf16(v[t][j]) bf16(B[e][n][j]) + bias[e][n] ),
//     v [T][r] float32 the caller's shrunk rows (scale included), B [E][N][r] float32, r in {4, 8, 16, 32, 64}.  B has the
//     weight image's layout [n][k] and v the activation image's, so behind the loop's last barrier the staging thread of
//     weight row sn, piece sp packs B[e][n0 + sn][32 sp .. + 31] into image[0] (zeros past N or r) and the staging thread
//     of row xs, quarter xq packs v[tx][16 xq .. + 15] into ximage[0] (zeros from r on), both rounded to bfloat16 as x is;
//     one barrier, then the steps.  Both images are written in full: nothing stale of a weight stage is contracted.  v
//     feeds the same exponent-field test as x: a non-finite v[t][j] makes the whole output row NaN.  B is not screened:
//     what a non-finite B gives is what the arithmetic gives, as with scale code 255.  r * 4 is a multiple of 16, so the
//     16-byte loads hold whenever the base pointers are 16-byte aligned; element loads otherwise.  No LDS beyond the two
//     images, and the kernel without the flag is the code it was.
//
// The gated form runs mx4_glu_kernel (fql_mx4_quant.h) first and reads its bfloat16 h [T][K] as x.
#pragma once
#include "fql_mx4_common.h"

struct Mx4Cfg {
    static constexpr int BT = 64, BN = 128, BK = 64;   // rows, columns and contraction depth of a stage
    static constexpr int PITCH = BK + 8;               // bfloat16 elements of an image row (144 bytes)
    static constexpr int THREADS = 256;
};

// Four float32 of an adapter operand (p is a multiple of four elements into its tensor) as two words of two bfloat16.
__device__ __forceinline__ void mx4_lora_pack4(const float *__restrict__ p, bool vec, bool ok, uint32_t &w0, uint32_t &w1)
{
    v4f f = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
        if (vec) f = *reinterpret_cast<const v4f *>(p);
        else { f[0] = p[0]; f[1] = p[1]; f[2] = p[2]; f[3] = p[3]; }
    }
    w0 = mx4_pack_bf16(f[0], f[1]);
    w1 = mx4_pack_bf16(f[2], f[3]);
}

// The operands of the adapter stage, the one kernel argument more of the LORA form: rows [T][rank] float32 (v, or dv in the
// input gradient), w the adapter matrix (B [E][N][rank], or A [E][rank][K] there).
struct Mx4Lora {
    const float *rows, *w;
    int rank;
};

// IN: element type of x (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of out, rounded once in the epilogue.
// LA: nothing (mx4_kernel<IN, OUT>: the signature, the code and the bits it always had), or Mx4Lora: the compile-time LORA
// flag, set by the argument that carries what it needs.  (54 KiB of LDS: two workgroups a compute unit.)
template <int IN, int OUT, class... LA>
__global__ __launch_bounds__(256) void mx4_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N, LA... lora)
{
    static_assert(sizeof...(LA) == 0 || (sizeof...(LA) == 1 && (std::is_same<LA, Mx4Lora>::value && ...)), "LA: nothing or Mx4Lora");
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool LORA = sizeof...(LA) == 1;
    using C = Mx4Cfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    __shared__ __attribute__((aligned(16))) unsigned short image[2][C::BN][C::PITCH];      // weights, bfloat16
    __shared__ __attribute__((aligned(16))) unsigned short ximage[2][C::BT][C::PITCH];     // activation rows, bfloat16
    __shared__ int row_bad[C::BT];                                 // != 0: the row holds a non-finite activation

    const int e = blockIdx.z;
    const int n0 = (int)blockIdx.x * C::BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nb = (wave & 1) * 2;                                 // first of this wave's two 32-n blocks
    const int tr = (wave >> 1) * 32 + r;                           // this lane's row inside the tile
    const bool row_ok = t_blk + tr < cnt;
    const int t = row_lo + t_blk + tr;
    const int K2 = K >> 1, KB = K >> 5;
    const int es = IN == 0 ? 4 : 2;

    // staging roles of this thread.  Weights: row sn of the stage, 16-byte piece sp (32 k = one scale block).
    // Activations: row xs of the tile (clamped into the expert's range: loads are unconditional), the 16 k of quarter xq.
    const int sn = tid >> 1, sp = tid & 1;
    const bool n_ok = n0 + sn < N;
    const size_t wrow = ((size_t)e * N + (n_ok ? n0 + sn : 0));
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KB;
    const int xs = tid >> 2, xq = tid & 3;
    const int tx = row_lo + (t_blk + xs < cnt ? t_blk + xs : cnt - 1);
    const char *xrow = reinterpret_cast<const char *>(x) + (size_t)tx * K * es;
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (K % 32 == 0: every row starts on a 16-byte boundary then)

    // What a thread holds of one stage between its loads and their use: its packed piece with the scale byte and its 16
    // activations as loaded (float32 rows are rounded when they are written to LDS, so the loads stay in flight).
    struct Stage {
        uint4 wq;
        int sc;
        typename std::conditional<IN == 0, float, uint32_t>::type x[IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int k0) {
        const int kp = k0 + 32 * sp;                               // packed piece + its scale byte
        st.wq = make_uint4(0u, 0u, 0u, 0u);
        st.sc = 127;
        if (n_ok && kp < K) {
            st.wq = *reinterpret_cast<const uint4 *>(wbase + (kp >> 1));
            st.sc = sbase[kp >> 5];
        }
        const int k = k0 + 16 * xq;                                // x[tx][k .. k + 15]; zeros past K
        constexpr int NX = IN == 0 ? 16 : 8;
#pragma unroll
        for (int i = 0; i < NX; ++i) st.x[i] = 0;
        if (k < K) {
            if (vec_x) {
#pragma unroll
                for (int i = 0; i < NX / 4; ++i) {
                    if constexpr (IN == 0) {
                        const v4f v = *reinterpret_cast<const v4f *>(xrow + (size_t)k * 4 + 16 * i);
#pragma unroll
                        for (int c = 0; c < 4; ++c) st.x[4 * i + c] = v[c];
                    } else {
                        const uint4 v = *reinterpret_cast<const uint4 *>(xrow + (size_t)k * 2 + 16 * i);
                        st.x[4 * i] = v.x; st.x[4 * i + 1] = v.y; st.x[4 * i + 2] = v.z; st.x[4 * i + 3] = v.w;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    if constexpr (IN == 0) {
                        st.x[i] = reinterpret_cast<const float *>(xrow)[k + i];
                    } else {
                        const unsigned short *p = reinterpret_cast<const unsigned short *>(xrow) + k + 2 * i;
                        st.x[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 16);
                    }
                }
            }
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> the two LDS images (bfloat16, natural k order)
        const uint32_t words[4] = {st.wq.x, st.wq.y, st.wq.z, st.wq.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)                                // dword i of the piece is k = kp + 8 i .. + 7
            *reinterpret_cast<uint4 *>(&image[buf][sn][32 * sp + 8 * i]) = mx4_dequant8(words[i], st.sc);
        uint32_t xw[8], bad = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (IN == 0) xw[i] = mx4_pack_bf16(st.x[2 * i], st.x[2 * i + 1]);
            else xw[i] = st.x[i];
            bad |= mx4_nonfinite2(xw[i]);
        }
        *reinterpret_cast<uint4 *>(&ximage[buf][xs][16 * xq]) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
        *reinterpret_cast<uint4 *>(&ximage[buf][xs][16 * xq + 8]) = make_uint4(xw[4], xw[5], xw[6], xw[7]);
        if (bad & 0x80008000u) row_bad[xs] = 1;                    // an exponent field of 255 (every writer writes 1)
    };

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    // Stage i: refill `mine` (consumed one stage ago) with the loads of stage i + 2, contract the images of stage i, then
    // turn `other` (stage i + 1, loaded one stage ago) into the other pair of images.  Two stages of loads are in flight.
    auto run_stage = [&](Stage &mine, const Stage &other, int k0, int it) {
        if (k0 + 2 * C::BK < K) load_stage(mine, k0 + 2 * C::BK);
        const unsigned short(*cur)[C::PITCH] = image[it & 1];
        const unsigned short(*xcur)[C::PITCH] = ximage[it & 1];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 xb = *reinterpret_cast<const uint4 *>(&xcur[tr][16 * s + 8 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const uint4 a = *reinterpret_cast<const uint4 *>(&cur[32 * (nb + b) + r][16 * s + 8 * h]);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, xb),
                                                                 acc[b], 0, 0, 0);
            }
        }
        if (k0 + C::BK < K) store_stage(other, (it + 1) & 1);      // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    };

    if (tid < C::BT) row_bad[tid] = 0;
    __syncthreads();
    Stage s0, s1;
    load_stage(s0, 0);
    s1 = s0;                                                       // (K == 32 or 64: never read)
    if (C::BK < K) load_stage(s1, C::BK);
    store_stage(s0, 0);
    __syncthreads();
    for (int k0 = 0, it = 0; k0 < K; k0 += 2 * C::BK, it += 2) {
        run_stage(s0, s1, k0, it);
        if (k0 + C::BK < K) run_stage(s1, s0, k0 + C::BK, it + 1);
    }

    if constexpr (LORA) {
        // The adapter stage.  Every thread is behind the last stage's barrier, which no store followed: both pairs of images
        // are free.  Pair 0 is written in full (zeros past N and from `rank` on), then one barrier, then the steps.
        const Mx4Lora la{lora...};
        const int rank = la.rank;
        const float *vrow = la.rows + (size_t)tx * rank;
        const float *brow = la.w + wrow * rank;
        const bool vec_v = (reinterpret_cast<uintptr_t>(la.rows) & 15) == 0, vec_b = (reinterpret_cast<uintptr_t>(la.w) & 15) == 0;
        uint32_t xw[8], bad = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                              // v[tx][16 xq + 4 i .. + 3]
            const int j = 16 * xq + 4 * i;
            mx4_lora_pack4(vrow + j, vec_v, j < rank, xw[2 * i], xw[2 * i + 1]);
            bad |= mx4_nonfinite2(xw[2 * i]) | mx4_nonfinite2(xw[2 * i + 1]);
        }
        *reinterpret_cast<uint4 *>(&ximage[0][xs][16 * xq]) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
        *reinterpret_cast<uint4 *>(&ximage[0][xs][16 * xq + 8]) = make_uint4(xw[4], xw[5], xw[6], xw[7]);
        if (bad & 0x80008000u) row_bad[xs] = 1;                    // (read behind the barrier below)
#pragma unroll
        for (int i = 0; i < 4; ++i) {                              // B[e][n0 + sn][32 sp + 8 i .. + 7]
            const int j = 32 * sp + 8 * i;
            uint4 w;
            mx4_lora_pack4(brow + j, vec_b, n_ok && j < rank, w.x, w.y);
            mx4_lora_pack4(brow + j + 4, vec_b, n_ok && j + 4 < rank, w.z, w.w);
            *reinterpret_cast<uint4 *>(&image[0][sn][j]) = w;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (16 * s >= rank) break;                             // (uniform)
            const uint4 xb = *reinterpret_cast<const uint4 *>(&ximage[0][tr][16 * s + 8 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const uint4 a = *reinterpret_cast<const uint4 *>(&image[0][32 * (nb + b) + r][16 * s + 8 * h]);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, xb),
                                                                 acc[b], 0, 0, 0);
            }
        }
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    // (Every write of row_bad lies behind a barrier of the loop or of the adapter stage.)
    const uint32_t bad = row_bad[tr] != 0 ? 0x8000u : 0u;
    if (!row_ok) return;
    const bool row_nan = (bad & 0x80008000u) != 0u;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nc = n0 + 32 * (nb + b) + 8 * q + 4 * h;
            if (nc >= N) continue;
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = acc[b][4 * q + c];
                if (brow != nullptr && nc + c < N) v[c] += brow[nc + c];
                if (row_nan) v[c] = __uint_as_float(0x7FC00000u);
            }
            store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
        }
#endif
}
