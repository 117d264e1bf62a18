// A dense linear layer on 4-bit CODE-BOOK weights ("LUT4"; NF4 of bitsandbytes / QLoRA is the named instance) (include/fql_int4.h,
// fql_linear_lut4_fwd):
//
//   W[n][k]   = bf16_rn( fl32( code_book[c(n, k)] * absmax[n][k / B] ) )
//   out[t][n] = round_OUT( fl32( acc + bias[n] ) ),   acc = sum_k bf16(x[t][k]) * W[n][k]
//
// codes [N][K / 2] uint8 in bitsandbytes' own order: input 2 i in the HIGH nibble of byte i, input 2 i + 1 in the low one (the
// opposite of the INT4 / MXFP4 / NVFP4 buffers of this tree; a table lookup does not care, so the bytes are read as stored).
// absmax [N][K / B] float32, B a power of two >= 64, K % B == 0, K % 64 == 0.  code_book [16] float32.  The weight is NOT exact
// in bfloat16: the one rounding of the product is part of the definition (it is what dequantize_4bit to bfloat16 gives).
//
// THE CONVERSION (lut4_dequant8).  There is no convert instruction for a table.  The 16 float32 entries sit in LDS as 16
// consecutive dwords, 16 different banks: any pattern of lane addresses is conflict-free and equal addresses broadcast.  A
// code costs one ds_read_b32 lane-read, the two integer instructions of its address, one v_mul_f32 (__fmul_rn: never
// contracted, never packed) and half a v_cvt_pk_bf16_f32.
//
// lut4_kernel: a tile TALL IN TOKEN ROWS, so that one converted weight serves four times the rows it serves in nv4_kernel.
//   workgroup = 4 waves = 256 rows t x 128 weight rows n, one stage = 32 k (one absmax per weight row and stage, since
//   B >= 64 and a stage starts on a multiple of 32).  grid = (ceil(N / 128), ceil(T / 256)).
//   * Wave w owns rows 64 w .. 64 w + 63 of the tile and all 128 columns: 2 x 4 accumulators of v_mfma_f32_32x32x16_bf16
//     (128 registers), the weights as the A operand.  A step of 16 k reads two row fragments and four weight fragments for
//     eight matrix instructions (nv4_kernel: one and two for two).  A wave whose 64 rows all lie past T contracts nothing
//     (uniform per wave); it still stages and meets every barrier.
//   * Staging.  Thread (sn = tid >> 1, sp = tid & 1) converts the 8-byte piece of 16 codes of weight row sn into the
//     image (a stage converts 128 x 32 = 4096 codes ONCE for 256 rows); thread (xs = tid >> 1, xq = tid & 1) packs 16 k of
//     rows xs and xs + 128.  Rows past T are row T - 1 again (loads are unconditional; never stored); weight rows past N
//     are zeros in the image.  K % 64 == 0: there is no partial stage.
//   * Two pairs of images at a pitch of 80 bytes (20 dwords: the 16 rows of a ds_read_b128 group start in 16 different
//     groups of four banks), 61 KiB of LDS with the table and the row flags: under the 64 KiB a workgroup may take
//     everywhere, and two workgroups fit a compute unit where the registers allow.  The loads of stage i + 1 are in flight
//     under the contraction of stage i, one barrier a stage.
//   * Epilogue: nv4_epilogue without a global scale (acc + bias, one float32 addition, then the one rounding to OUT).
//   * NON-FINITE: mx4_kernel's row flag (a non-finite activation makes exactly its output row NaN); absmax and the table
//     are not screened, plain arithmetic decides.
// A few rows take the split-K decode form of fql_gemm_lut4_decode.h.  The grouped form over an expert table (stacked NF4
// experts) has a shorter tile of its own, lut4_group_kernel in fql_gemm_lut4_group.h: experts do not have 256 rows.
//
// LORA (lut4_kernel<IN, OUT, Mx4Lora>; fql_linear_lut4_lora_fwd): the adapter as one more contraction
// stage behind the K loop's last barrier,
//   out[t][n] = round_OUT( fl32( S + bias[n] ) ),   S = acc (+) sum_{j < r} bf16(v[t][j]) bf16(B[n][j])
// with (+) the matrix instruction accumulating onto its C operand in ascending j, 16 a step.  No store follows the loop's
// last barrier, so both pairs of images are free, and a pair holds 32 columns of j:
//   * Staging thread (sn, sp) packs B[n0 + sn][32 p + 16 sp .. + 15] into image[p][sn][16 sp ..], zeros past N and from r
//     on; thread (xs, xq) packs v[tx][32 p + 16 xq .. + 15] of its XR rows xs + 128 i (clamped to T - 1, as x) into
//     ximage[p], zeros from r on; the packed words of v feed the row flag, B is not screened.  p = 0 for r <= 32; r = 64
//     writes p = 1 in the same pass.  A pair that is written is written in full (all 32 columns of all rows), so nothing
//     of a weight stage is contracted a second time, and a pair that is not written is not read.
//   * ONE barrier for every rank, then the steps s = 0 .. 3 with 16 s < r on pair s >> 1, columns 16 (s & 1) .. + 15: the
//     K loop's own 2 x 4 fragment loop, eight matrix instructions a step.  A dead wave stages and meets the barrier.
//   * 16-byte loads of v / B when their base is 16-byte aligned (4 r is a multiple of 16), element loads otherwise.
//   * No LDS beyond the kernel's, no global scale (nothing moves in front of the stage), nv4_epilogue as it is.  With
//     B = 0 the steps add +0 to every register: the base kernel's bits.  lut4_kernel<IN, OUT> is the code it was.
//
// Compiled without the packed float32 instructions (the target attribute below), contraction off in the conversion.
#pragma once
#include "fql_gemm_nvfp4.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define FQL_LUT4_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define FQL_LUT4_TARGET                    // (the host pass does not know the feature)
#endif

struct Lut4Cfg {
    static constexpr int WAVES = 4, WT = 64;                    // waves of a workgroup, token rows a wave owns
    static constexpr int BT = WAVES * WT, BN = 128, BK = 32;    // rows, columns and contraction depth of a stage
    static constexpr int PITCH = BK + 8;                        // bfloat16 elements of an image row (80 bytes)
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int XR = BT / 128;                         // rows a staging thread packs 16 k of
};

// bitsandbytes' NF4 table (the decimal strings it documents, as float32): the code book of a call that passes none.
__constant__ const float lut4_nf4_book[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f,
    -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

// The 16 table entries into LDS (threads 0 .. 15; the caller's barrier follows).  book == NULL: the NF4 table.
__device__ __forceinline__ void lut4_load_table(float *lut, const float *__restrict__ book)
{
    if (threadIdx.x < 16) lut[threadIdx.x] = book != nullptr ? book[threadIdx.x] : lut4_nf4_book[threadIdx.x];
}

// One dword of a packed piece (8 codes, 8 consecutive k: byte b holds k = 2 b in its HIGH nibble and k = 2 b + 1 in its low
// one) under its block's absmax -> 8 bfloat16 in k order.  lut: the table in LDS.
__device__ __forceinline__ uint4 lut4_dequant8(uint32_t w, float am, const float *lut)
{
#pragma clang fp contract(off)
    uint32_t o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float even = __fmul_rn(lut[(w >> (8 * b + 4)) & 15u], am);
        const float odd = __fmul_rn(lut[(w >> (8 * b)) & 15u], am);
        o[b] = mx4_pack_bf16(even, odd);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// The kernel's body (inlined into lut4_kernel, which carries the target attribute and the LDS: as nv4_linear_decode_body).
// LA: nothing, or Mx4Lora: the compile-time LORA flag, set by the argument that carries what it needs.
template <int IN, int OUT, class... LA>
__device__ __forceinline__ void lut4_body(
    unsigned short (&image)[2][Lut4Cfg::BN][Lut4Cfg::PITCH], unsigned short (&ximage)[2][Lut4Cfg::BT][Lut4Cfg::PITCH],
    float (&lut)[16], int (&row_bad)[Lut4Cfg::BT],
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, int bshift, int T, int K, int N,
    LA... lora)
{
    static_assert(sizeof...(LA) == 0 || (sizeof...(LA) == 1 && (std::is_same<LA, Mx4Lora>::value && ...)), "LA: nothing or Mx4Lora");
    constexpr bool LORA = sizeof...(LA) == 1;
    using C = Lut4Cfg;
    const int n0 = (int)blockIdx.x * C::BN, t_blk = (int)blockIdx.y * C::BT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const bool wave_live = t_blk + C::WT * wave < T;               // (uniform per wave)
    const int K2 = K >> 1, KB = K >> bshift;
    constexpr int es = IN == 0 ? 4 : 2;

    // staging roles.  Weights: row sn of the tile, 8-byte piece sp (16 codes, inside one absmax block).  Activations: the
    // 16 k of half xq of rows xs + 128 i (clamped to T - 1).
    const int sn = tid >> 1, sp = tid & 1;
    const bool n_ok = n0 + sn < N;
    const size_t wrow = (size_t)(n_ok ? n0 + sn : 0);
    const uint8_t *wbase = codes + wrow * K2 + 8 * sp;
    const float *abase = absmax + wrow * KB;
    const int xs = tid >> 1, xq = tid & 1;
    const char *xrow[C::XR];
#pragma unroll
    for (int i = 0; i < C::XR; ++i) {
        const int tx = t_blk + xs + 128 * i < T ? t_blk + xs + 128 * i : T - 1;
        xrow[i] = reinterpret_cast<const char *>(x) + ((size_t)tx * K + 16 * xq) * es;
    }
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (K % 64 == 0: every row starts on a 16-byte boundary then)

    struct Stage {
        uint2 wq;
        float am;
        typename std::conditional<IN == 0, float, uint32_t>::type x[C::XR][IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int k0) {                     // (k0 + 31 < K)
        st.wq = *reinterpret_cast<const uint2 *>(wbase + (k0 >> 1));
        st.am = abase[k0 >> bshift];
#pragma unroll
        for (int i = 0; i < C::XR; ++i) {
            const char *p = xrow[i] + (size_t)k0 * es;
            if (vec_x) {
#pragma unroll
                for (int j = 0; j < (IN == 0 ? 4 : 2); ++j) {
                    if constexpr (IN == 0) {
                        const v4f v = *reinterpret_cast<const v4f *>(p + 16 * j);
#pragma unroll
                        for (int c = 0; c < 4; ++c) st.x[i][4 * j + c] = v[c];
                    } else {
                        const uint4 v = *reinterpret_cast<const uint4 *>(p + 16 * j);
                        st.x[i][4 * j] = v.x; st.x[i][4 * j + 1] = v.y; st.x[i][4 * j + 2] = v.z; st.x[i][4 * j + 3] = v.w;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < (IN == 0 ? 16 : 8); ++j) {
                    if constexpr (IN == 0) {
                        st.x[i][j] = reinterpret_cast<const float *>(p)[j];
                    } else {
                        const unsigned short *q = reinterpret_cast<const unsigned short *>(p) + 2 * j;
                        st.x[i][j] = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
                    }
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
#pragma unroll
        for (int i = 0; i < C::XR; ++i) {
            uint32_t xw[8], bad = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (IN == 0) xw[j] = mx4_pack_bf16(st.x[i][2 * j], st.x[i][2 * j + 1]);
                else xw[j] = st.x[i][j];
                bad |= mx4_nonfinite2(xw[j]);
            }
            *reinterpret_cast<uint4 *>(&ximage[buf][xs + 128 * i][16 * xq]) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
            *reinterpret_cast<uint4 *>(&ximage[buf][xs + 128 * i][16 * xq + 8]) = make_uint4(xw[4], xw[5], xw[6], xw[7]);
            if (bad & 0x80008000u) row_bad[xs + 128 * i] = 1;       // an exponent field of 255 (every writer writes 1)
        }
    };

    v16f acc[2][4];                                                // [block of 32 rows][block of 32 columns]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.0f;

    lut4_load_table(lut, book);
    row_bad[tid] = 0;
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
                uint4 xb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) xb[a] = *reinterpret_cast<const uint4 *>(&xcur[C::WT * wave + 32 * a + r][16 * s + 8 * h]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint4 wa = *reinterpret_cast<const uint4 *>(&cur[32 * b + r][16 * s + 8 * h]);
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, wa), __builtin_bit_cast(v8bf, xb[a]),
                                                                            acc[a][b], 0, 0, 0);
                }
            }
        }
        if (more) store_stage(st, (it + 1) & 1);                   // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    }

    if constexpr (LORA) {
        // The adapter stage.  Every thread is behind the loop's last barrier, which no store followed: both pairs of images
        // are free.  Pair p takes columns j = 32 p .. 32 p + 31 of B and of v, written in full (zeros past N and from
        // `rank` on); pair 1 only for rank 64 (uniform).  One barrier, then the steps.
        const Mx4Lora la{lora...};
        const int rank = la.rank;
        const float *brow = la.w + wrow * rank;
        const bool vec_v = (reinterpret_cast<uintptr_t>(la.rows) & 15) == 0, vec_b = (reinterpret_cast<uintptr_t>(la.w) & 15) == 0;
        const float *vrow[C::XR];
#pragma unroll
        for (int i = 0; i < C::XR; ++i) {
            const int tx = t_blk + xs + 128 * i < T ? t_blk + xs + 128 * i : T - 1;
            vrow[i] = la.rows + (size_t)tx * rank;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (32 * p >= rank) break;                             // (uniform)
            uint32_t bw[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                          // B[n0 + sn][32 p + 16 sp + 4 i .. + 3]
                const int j = 32 * p + 16 * sp + 4 * i;
                mx4_lora_pack4(brow + j, vec_b, n_ok && j < rank, bw[2 * i], bw[2 * i + 1]);
            }
            *reinterpret_cast<uint4 *>(&image[p][sn][16 * sp]) = make_uint4(bw[0], bw[1], bw[2], bw[3]);
            *reinterpret_cast<uint4 *>(&image[p][sn][16 * sp + 8]) = make_uint4(bw[4], bw[5], bw[6], bw[7]);
#pragma unroll
            for (int i = 0; i < C::XR; ++i) {
                uint32_t xw[8], bad = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {                      // v[tx][32 p + 16 xq + 4 q .. + 3]
                    const int j = 32 * p + 16 * xq + 4 * q;
                    mx4_lora_pack4(vrow[i] + j, vec_v, j < rank, xw[2 * q], xw[2 * q + 1]);
                    bad |= mx4_nonfinite2(xw[2 * q]) | mx4_nonfinite2(xw[2 * q + 1]);
                }
                *reinterpret_cast<uint4 *>(&ximage[p][xs + 128 * i][16 * xq]) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
                *reinterpret_cast<uint4 *>(&ximage[p][xs + 128 * i][16 * xq + 8]) = make_uint4(xw[4], xw[5], xw[6], xw[7]);
                if (bad & 0x80008000u) row_bad[xs + 128 * i] = 1;   // (read behind the barrier below)
            }
        }
        __syncthreads();
        if (wave_live) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (16 * s >= rank) break;                         // (uniform)
                const unsigned short(*cur)[C::PITCH] = image[s >> 1];
                const unsigned short(*xcur)[C::PITCH] = ximage[s >> 1];
                const int c0 = 16 * (s & 1) + 8 * h;
                uint4 xb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) xb[a] = *reinterpret_cast<const uint4 *>(&xcur[C::WT * wave + 32 * a + r][c0]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint4 wa = *reinterpret_cast<const uint4 *>(&cur[32 * b + r][c0]);
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, wa), __builtin_bit_cast(v8bf, xb[a]),
                                                                            acc[a][b], 0, 0, 0);
                }
            }
        }
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    // (Every write of row_bad lies behind a barrier of the loop or of the adapter stage.)
    if (!wave_live) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int tr = C::WT * wave + 32 * a + r, t = t_blk + tr;
        if (t >= T) continue;
        const bool row_nan = row_bad[tr] != 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            nv4_epilogue<OUT>(acc[a][b], out, t, N, n0 + 32 * b, h, vec, bias, false, 1.0f, row_nan);
    }
}

// IN: element type of x (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of out, rounded once in the epilogue.
// bshift = log2(B).  LA: nothing (lut4_kernel<IN, OUT>: the signature, the code and the bits it always had), or Mx4Lora.
template <int IN, int OUT, class... LA>
__global__ __launch_bounds__(256) FQL_LUT4_TARGET void lut4_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ absmax, const float *__restrict__ book,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, int bshift, int T, int K, int N,
    LA... lora)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Lut4Cfg;
    __shared__ __attribute__((aligned(16))) unsigned short image[2][C::BN][C::PITCH];      // weights, bfloat16
    __shared__ __attribute__((aligned(16))) unsigned short ximage[2][C::BT][C::PITCH];     // activation rows, bfloat16
    __shared__ float lut[16];
    __shared__ int row_bad[C::BT];                                 // != 0: the row holds a non-finite activation
    lut4_body<IN, OUT, LA...>(image, ximage, lut, row_bad, codes, absmax, book, x, bias, out, bshift, T, K, N, lora...);
#endif
}
