// The grouped GEMM on 4-bit CODE-BOOK expert weights (NF4 experts of the `*-bnb-4bit` MoE checkpoints) (include/fql_int4.h,
// fql_moe_lut4_fwd / fql_moe_lut4_glu_fwd):
//
//   W_e[n][k] = bf16_rn( fl32( code_book[c(e, n, k)] * absmax[e][n][k / B] ) )                       (fql_gemm_lut4.h, per expert)
//   out[t][n] = round_OUT( fl32( acc + bias[e][n] ) ),   acc = sum_k bf16(x[t][k]) * W_e[n][k]       over the rows t of expert e
//
// codes [E][N][K / 2] uint8 in bitsandbytes' nibble order, read as stored; absmax [E][N][K / B] float32; code_book [16] or NULL
// (the NF4 table), ONE table for all experts; bias [E][N] float32 or NULL.  The conversion is lut4_dequant8 as it is
// (contraction off, no packed float32 instructions), the contraction v_mfma_f32_32x32x16_bf16 over ascending k, 16 a step,
// from zero, the epilogue nv4_epilogue without a global scale, the row flag for non-finite activations.
// THE CONTRACT that follows by construction: the bits of a row are those fql_linear_lut4_fwd gives that row on that
// expert's matrix (the same weights, the same products in the same order on the same instruction, the same one addition
// and one rounding), so the grouped call equals E one-expert calls bit for bit, and rows no expert covers are zeros.
//
// lut4_group_kernel: lut4_kernel's tile is 256 token rows tall so that one table lookup serves many rows; experts do not
// have that many rows (the headline routing gives an expert 128), so this kernel has a tile of its own.
//   workgroup = 4 waves = 128 rows t x 128 weight rows n, one stage = 32 k (one absmax per weight row and stage).
//   grid = (ceil(N / 128), ceil(T / 128), E (+ 1 with a table)); the head is mx4_group_begin: the expert's row range is read
//   on the device, the slice past the experts zeroes the uncovered rows, row blocks past the expert's count return at once.
//   * Wave w owns rows 32 w .. 32 w + 31 of the tile and all 128 columns: 1 x 4 accumulators (64 registers; lut4_kernel has
//     2 x 4 and 128), the weights as the A operand.  A step of 16 k reads one row fragment and four weight fragments for
//     four matrix instructions.  A wave whose 32 rows all lie past the expert's count contracts nothing (uniform per
//     wave); it still stages and meets every barrier.
//   * Staging.  Thread (sn = tid >> 1, sp = tid & 1) converts the 8-byte piece of 16 codes of weight row sn under one absmax;
//     thread (xs = tid >> 1, xq = tid & 1) packs 16 k of row xs (one row a thread; lut4_kernel packs two).  Rows past the
//     expert's count are the expert's last row again (clamped INSIDE the expert's range; loads are unconditional; never
//     stored); weight rows past N are zeros in the image.  K % 64 == 0: there is no partial stage.
//   * Two pairs of images at lut4_kernel's pitch of 80 bytes: 40 KiB of LDS, plus the table and 128 row flags.  The loads
//     of stage i + 1 are in flight under the contraction of stage i, one barrier a stage.
//   * The shorter tile halves the accumulators and the staged rows, so the kernel fits 256 registers without scratch and
//     two workgroups share a compute unit: one converts while the other contracts (__launch_bounds__(256, 2)).
//   * Weight and absmax offsets are size_t: E N K / 2 passes 4 GiB at real sizes.
// The gated form runs mx4_glu_kernel (fql_mx4_quant.h) first and reads its bfloat16 h [T][K] as x.
// For few rows an expert the host runs the one-wave decode kernel of fql_gemm_lut4_group_decode.h instead: the same bits.
// Out of scope: adapter forms, a per-expert table.
#pragma once
#include "fql_gemm_lut4.h"

struct Lut4GroupCfg {
    static constexpr int WAVES = 4, WT = 32;                    // waves of a workgroup, token rows a wave owns
    static constexpr int BT = WAVES * WT, BN = 128, BK = 32;    // rows, columns and contraction depth of a stage
    static constexpr int PITCH = Lut4Cfg::PITCH;                // bfloat16 elements of an image row (80 bytes)
    static constexpr int THREADS = 64 * WAVES;
};

// The kernel's body behind mx4_group_begin (inlined into lut4_group_kernel, which carries the target attribute and the LDS: as
// lut4_body; the lambdas of a function that carries the attribute itself would not be inlined into it).  Expert e holds rows
// row_lo .. row_lo + cnt - 1, the workgroup's tile starts at row t_blk of them (t_blk < cnt).
template <int IN, int OUT>
__device__ __forceinline__ void lut4_group_body(
    unsigned short (&image)[2][Lut4GroupCfg::BN][Lut4GroupCfg::PITCH], unsigned short (&ximage)[2][Lut4GroupCfg::BT][Lut4GroupCfg::PITCH],
    float (&lut)[16], int (&row_bad)[Lut4GroupCfg::BT],
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, int bshift, int e, int row_lo, int cnt,
    int t_blk, int K, int N)
{
    using C = Lut4GroupCfg;
    static_assert(C::BN * 2 == C::THREADS && C::BT * 2 == C::THREADS, "two staging threads a weight row and a token row");
    const int n0 = (int)blockIdx.x * C::BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const bool wave_live = t_blk + C::WT * wave < cnt;             // (uniform per wave)
    const int K2 = K >> 1, KB = K >> bshift;
    constexpr int es = IN == 0 ? 4 : 2;

    // staging roles.  Weights: row sn of the tile, 8-byte piece sp (16 codes, inside one absmax block).  Activations: the
    // 16 k of half xq of row xs (clamped into the expert's range: t_blk < cnt, so cnt >= 1).
    const int sn = tid >> 1, sp = tid & 1;
    const bool n_ok = n0 + sn < N;
    const size_t wrow = (size_t)e * N + (n_ok ? n0 + sn : 0);
    const uint8_t *wbase = codes + wrow * K2 + 8 * sp;
    const float *abase = absmax + wrow * KB;
    const int xs = tid >> 1, xq = tid & 1;
    const int tx = row_lo + (t_blk + xs < cnt ? t_blk + xs : cnt - 1);
    const char *xrow = reinterpret_cast<const char *>(x) + ((size_t)tx * K + 16 * xq) * es;
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (K % 64 == 0: every row starts on a 16-byte boundary then)

    struct Stage {
        uint2 wq;
        float am;
        typename std::conditional<IN == 0, float, uint32_t>::type x[IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int k0) {                     // (k0 + 31 < K)
        st.wq = *reinterpret_cast<const uint2 *>(wbase + (k0 >> 1));
        st.am = abase[k0 >> bshift];
        const char *p = xrow + (size_t)k0 * es;
        if (vec_x) {
#pragma unroll
            for (int j = 0; j < (IN == 0 ? 4 : 2); ++j) {
                if constexpr (IN == 0) {
                    const v4f v = *reinterpret_cast<const v4f *>(p + 16 * j);
#pragma unroll
                    for (int c = 0; c < 4; ++c) st.x[4 * j + c] = v[c];
                } else {
                    const uint4 v = *reinterpret_cast<const uint4 *>(p + 16 * j);
                    st.x[4 * j] = v.x; st.x[4 * j + 1] = v.y; st.x[4 * j + 2] = v.z; st.x[4 * j + 3] = v.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < (IN == 0 ? 16 : 8); ++j) {
                if constexpr (IN == 0) {
                    st.x[j] = reinterpret_cast<const float *>(p)[j];
                } else {
                    const unsigned short *q = reinterpret_cast<const unsigned short *>(p) + 2 * j;
                    st.x[j] = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
                }
            }
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> the two LDS images (bfloat16, natural k order)
        const uint32_t words[2] = {st.wq.x, st.wq.y};
#pragma unroll
        for (int i = 0; i < 2; ++i) {                              // dword i of the piece is k = 16 sp + 8 i .. + 7
            uint4 w = lut4_dequant8(words[i], st.am, lut);
            if (!n_ok) w = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4 *>(&image[buf][sn][16 * sp + 8 * i]) = w;
        }
        uint32_t xw[8], bad = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (IN == 0) xw[j] = mx4_pack_bf16(st.x[2 * j], st.x[2 * j + 1]);
            else xw[j] = st.x[j];
            bad |= mx4_nonfinite2(xw[j]);
        }
        *reinterpret_cast<uint4 *>(&ximage[buf][xs][16 * xq]) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
        *reinterpret_cast<uint4 *>(&ximage[buf][xs][16 * xq + 8]) = make_uint4(xw[4], xw[5], xw[6], xw[7]);
        if (bad & 0x80008000u) row_bad[xs] = 1;                    // an exponent field of 255 (every writer writes 1)
    };

    v16f acc[4];                                                   // [block of 32 columns]
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    lut4_load_table(lut, book);
    if (tid < C::BT) row_bad[tid] = 0;
    __syncthreads();
    Stage st;
    load_stage(st, 0);
    store_stage(st, 0);
    __syncthreads();
    for (int k0 = 0, it = 0; k0 < K; k0 += C::BK, ++it) {
        const bool more = k0 + C::BK < K;                          // (uniform)
        if (more) load_stage(st, k0 + C::BK);
        if (wave_live) {
            const unsigned short(*cur)[C::PITCH] = image[it & 1];
            const unsigned short(*xcur)[C::PITCH] = ximage[it & 1];
#pragma unroll
            for (int s = 0; s < C::BK / 16; ++s) {
                const uint4 xb = *reinterpret_cast<const uint4 *>(&xcur[C::WT * wave + r][16 * s + 8 * h]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint4 wa = *reinterpret_cast<const uint4 *>(&cur[32 * b + r][16 * s + 8 * h]);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, wa), __builtin_bit_cast(v8bf, xb), acc[b],
                                                                     0, 0, 0);
                }
            }
        }
        if (more) store_stage(st, (it + 1) & 1);                   // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    // (Every write of row_bad lies behind a barrier of the loop.)
    const int tr = C::WT * wave + r;
    if (t_blk + tr >= cnt) return;
    const int t = row_lo + t_blk + tr;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias != nullptr ? bias + (size_t)e * N : nullptr;
    const bool row_nan = row_bad[tr] != 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) nv4_epilogue<OUT>(acc[b], out, t, N, n0 + 32 * b, h, vec, brow, false, 1.0f, row_nan);
}

// IN: element type of x (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of out, rounded once in the epilogue.
// bshift = log2(B).
template <int IN, int OUT>
__global__ __launch_bounds__(256, 2) FQL_LUT4_TARGET void lut4_group_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int bshift, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Lut4GroupCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    __shared__ __attribute__((aligned(16))) unsigned short image[2][C::BN][C::PITCH];      // weights, bfloat16
    __shared__ __attribute__((aligned(16))) unsigned short ximage[2][C::BT][C::PITCH];     // activation rows, bfloat16
    __shared__ float lut[16];
    __shared__ int row_bad[C::BT];                                 // != 0: the row holds a non-finite activation
    lut4_group_body<IN, OUT>(image, ximage, lut, row_bad, codes, absmax, book, x, bias, out, bshift, (int)blockIdx.z, row_lo, cnt, t_blk,
                             K, N);
#endif
}
