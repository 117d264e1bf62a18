// Grouped GEMM on NVFP4 expert weights (include/fql_int4.h, fql_moe_nvfp4_fwd / fql_moe_nvfp4_glu_fwd):
//
//   out[t][n] = round_OUT( fl32( fl32(acc * global_scale[e]) + bias[e][n] ) ),   acc = sum_k bf16(x[t][k]) * W_e[n][k],
//   W_e[n][k] = e2m1(code[e][n][k]) * e4m3(s[e][n][k / 16])
//
// blocks [E][N][K / 2] uint8 (the MXFP4 layout: even k in the low nibble), scales [E][N][K / 16] uint8, the OCP e4m3fn value
// of the byte (bias 7, subnormals, 0x7F and 0xFF NaN, the sign honoured), global_scale [E] float32 or NULL (1).  Every
// product of an e2m1 value and a finite e4m3 value has at most six significant bits and lies in 2^-10 .. 2688, so it is
// exact in bfloat16: as with MXFP4 the weights are dequantised without an error on their way to the matrix cores, and the
// kernels are the MXFP4 ones (fql_gemm_mx4.h, fql_gemm_mx4_decode.h) with another conversion and one more epilogue step.
// They live in a file of their own so that the MXFP4 kernels stay the instructions they were.
//
// THE CONVERSION (nv4_dequant8).  v_cvt_f32_fp8 turns the scale byte into float32 (once per 16 codes),
// v_cvt_scalef32_pk_f32_fp4 with a scale of 1 turns a byte of two codes into two float32, one multiply each and
// v_cvt_pk_bf16_f32 packs the pair: all four steps exact.  A NaN byte is replaced by a float32 NaN before the multiply,
// so its 16 weights are NaN, zeros included, whatever the convert gives for it.
//
// nv4_kernel: mx4_kernel's skeleton (64 x 128 tiles, the weights as the A operand of v_mfma_f32_32x32x16_bf16, two pairs
// of LDS images, loads two stages ahead, mx4_group_begin and its coverage slice).  A staging thread's 16-byte piece is 32 k =
// TWO scale blocks: it loads the two adjacent scale bytes (two byte loads: no alignment is asked of `scales`), dwords 0-1
// take the first and dwords 2-3 the second.  Absent pieces are zero codes under the byte 0x38 (1.0).
// nv4_decode_kernel: mx4_decode_kernel's shape (one wave, 32 weight rows over all of K, up to 32 rows), THE SAME BITS as
// nv4_kernel: the same instruction on ascending k, one accumulator from zero, nv4_dequant8 and nv4_epilogue as they are.
// Lane (r, h) loads the piece of 32 k number 2 j + h and its two scale bytes; the swap that gives both halves both pieces
// gives them all four bytes, and step s of the 64 k (16 k = one scale block) converts under byte s.
// EPILOGUE (nv4_epilogue, both kernels).  global_scale[e] is read once per workgroup; a result is multiplied by it, then
// the bias is added, two float32 roundings, never an FMA.  Without a global scale and a bias the result is acc's bits.
// NON-FINITE: as mx4_kernel (the row flag); global_scale is not screened.
//
// LORA (nv4_kernel<IN, OUT, Mx4Lora>; fql_moe_nvfp4_lora_fwd / fql_moe_nvfp4_glu_lora_fwd / fql_linear_nvfp4_lora_fwd, DESIGN.md
// section 41): mx4_kernel's adapter stage, one more contraction stage behind the last weight stage's barrier,
//   out[t][n] = round_OUT( fl32( S + bias[e][n] ) ),   S = fl32(acc * global_scale[e]) (+) sum_{j < r} bf16(v[t][j]) bf16(B[e][n][j])
// with (+) the matrix instruction accumulating onto its C operand in ascending j, 16 a step.  THE GLOBAL SCALE belongs to
// the weights alone, so it cannot stay in the epilogue, where the accumulator also holds the adapter term: the LORA form
// multiplies the 32 accumulator registers by it behind the last weight stage (one __fmul_rn each, contraction off, only
// with a global scale), the steps accumulate onto the scaled value and nv4_epilogue is called without the multiply.  With
// B = 0 the steps add +0, so the result is the base kernel's (but for the sign of a zero under a negative scale).
// The stage writes pair 0 of the images in full (zeros past N and from r on), so nothing stale of a weight stage, a NaN
// block under byte 0x7F included, meets a zero; v feeds the row flag, B is not screened.  nv4_kernel<IN, OUT> is the code
// it was; the decode kernel has no adapter form.
#pragma once
#include "fql_gemm_mx4_decode.h"

typedef float v2f __attribute__((ext_vector_type(2)));

// The float32 value of byte SEL of sc (e4m3fn); NaN for 0x7F / 0xFF.
template <int SEL>
__device__ __forceinline__ float nv4_scale(uint32_t sc)
{
    const float s = __builtin_amdgcn_cvt_f32_fp8((int)sc, SEL);
    return ((sc >> (8 * SEL)) & 0x7Fu) == 0x7Fu ? __uint_as_float(0x7FC00000u) : s;
}

// The two codes of byte B of w times s as one word of two bfloat16 (low nibble = even k in the low half).
template <int B>
__device__ __forceinline__ uint32_t nv4_pair(uint32_t w, float s)
{
    const v2f p = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, B) * v2f{s, s};   // (v_pk_mul_f32; the products are exact)
    return mx4_pack_bf16(p[0], p[1]);
}

// One dword of a packed piece (8 codes, 8 consecutive k, inside one scale block) times its block's scale -> 8 bfloat16.
__device__ __forceinline__ uint4 nv4_dequant8(uint32_t w, float s)
{
    uint4 o;
    o.x = nv4_pair<0>(w, s);
    o.y = nv4_pair<1>(w, s);
    o.z = nv4_pair<2>(w, s);
    o.w = nv4_pair<3>(w, s);
    return o;
}

// The epilogue of one 32-n block (columns nb0 .. nb0 + 31) of the lane's row t: registers 4q .. 4q+3 of acc are
// n = nb0 + 8 q + 4 h + (0 .. 3).  brow: the expert's bias row or NULL; gs: its global scale (has_gs: there is one).
template <int OUT>
__device__ __forceinline__ void nv4_epilogue(const v16f &acc, void *__restrict__ out, int t, int N, int nb0, int h, bool vec,
                                             const float *__restrict__ brow, bool has_gs, float gs, bool row_nan)
{
#pragma clang fp contract(off)                     // acc * global_scale, THEN + bias: two roundings, never an FMA
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nc = nb0 + 8 * q + 4 * h;
        if (nc >= N) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = acc[4 * q + c];
            if (has_gs) v[c] = __fmul_rn(v[c], gs);
            if (brow != nullptr && nc + c < N) v[c] = __fadd_rn(v[c], brow[nc + c]);
            if (row_nan) v[c] = __uint_as_float(0x7FC00000u);
        }
        store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
    }
}

// IN: element type of x (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of out, rounded once in the epilogue.
// LA: nothing (nv4_kernel<IN, OUT>: the signature, the code and the bits it always had), or Mx4Lora: the compile-time LORA
// flag, set by the argument that carries what it needs.  (54 KiB of LDS, as mx4_kernel: two workgroups a compute unit.)
template <int IN, int OUT, class... LA>
__global__ __launch_bounds__(256) void nv4_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const float *__restrict__ gscale,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
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
    const int K2 = K >> 1, KS = K >> 4;
    const int es = IN == 0 ? 4 : 2;
    const bool has_gs = gscale != nullptr;
    const float gs = has_gs ? gscale[e] : 1.0f;                    // (uniform: once per workgroup)

    // staging roles of this thread.  Weights: row sn of the stage, 16-byte piece sp (32 k = two scale blocks).
    // Activations: row xs of the tile (clamped into the expert's range: loads are unconditional), the 16 k of quarter xq.
    const int sn = tid >> 1, sp = tid & 1;
    const bool n_ok = n0 + sn < N;
    const size_t wrow = ((size_t)e * N + (n_ok ? n0 + sn : 0));
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KS;
    const int xs = tid >> 2, xq = tid & 3;
    const int tx = row_lo + (t_blk + xs < cnt ? t_blk + xs : cnt - 1);
    const char *xrow = reinterpret_cast<const char *>(x) + (size_t)tx * K * es;
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (K % 32 == 0: every row starts on a 16-byte boundary then)

    // What a thread holds of one stage between its loads and their use: its packed piece with the two scale bytes (byte 0:
    // dwords 0-1, byte 1: dwords 2-3) and its 16 activations as loaded.
    struct Stage {
        uint4 wq;
        uint32_t sc;
        typename std::conditional<IN == 0, float, uint32_t>::type x[IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int k0) {
        const int kp = k0 + 32 * sp;                               // packed piece + its two scale bytes
        st.wq = make_uint4(0u, 0u, 0u, 0u);
        st.sc = 0x3838u;
        if (n_ok && kp < K) {                                      // (kp + 31 < K: both bytes lie inside the row's K / 16)
            st.wq = *reinterpret_cast<const uint4 *>(wbase + (kp >> 1));
            st.sc = (uint32_t)sbase[kp >> 4] | ((uint32_t)sbase[(kp >> 4) + 1] << 8);
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
        const float s01 = nv4_scale<0>(st.sc), s23 = nv4_scale<1>(st.sc);
#pragma unroll
        for (int i = 0; i < 4; ++i)                                // dword i of the piece is k = kp + 8 i .. + 7
            *reinterpret_cast<uint4 *>(&image[buf][sn][32 * sp + 8 * i]) = nv4_dequant8(words[i], i < 2 ? s01 : s23);
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
        // global_scale belongs to the weights alone: the finished weight sum is multiplied here, one rounding a register
        // and never an FMA, the adapter steps accumulate onto the scaled value and the epilogue multiplies no more.
        if (has_gs) {
#pragma clang fp contract(off)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[b][q] = __fmul_rn(acc[b][q], gs);
        }
        // The adapter stage (mx4_kernel's).  Every thread is behind the last stage's barrier, which no store followed:
        // both pairs of images are free.  Pair 0 is written in full (zeros past N and from `rank` on), so nothing of a
        // weight stage, a NaN block included, meets a zero; then one barrier, then the steps.
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
    const bool row_nan = row_bad[tr] != 0;
    if (!row_ok) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
#pragma unroll
    for (int b = 0; b < 2; ++b)
        nv4_epilogue<OUT>(acc[b], out, t, N, n0 + 32 * (nb + b), h, vec, brow, !LORA && has_gs, gs, row_nan);
#endif
}

// One ring slot of the decode kernel: what lane (r, h) holds of 64 k between its loads and their use.
template <int IN>
struct Nv4DecodeSlot {
    uint4 wq;                                                      // the 16-byte piece of 32 k number 2 j + h
    uint16_t sc;                                                   // its two scale bytes (kept narrow: see mx4_decode_body's consume)
    typename std::conditional<IN == 0, float, uint32_t>::type x[4][IN == 0 ? 8 : 4];   // x[t_r][64 j + 16 s + 8 h .. + 7], step s
};

// VEC: the rows' base is 16-byte aligned (every row and every fragment is, then: K % 32 == 0).
template <int IN, int OUT, bool VEC, int DEPTH, int GROUP>
__device__ __forceinline__ void nv4_decode_body(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const float *__restrict__ gscale,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, int e, int row_lo, int cnt, int t_blk,
    int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Nv4DecodeSlot<IN>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN;
    const int K2 = K >> 1, KS = K >> 4;
    constexpr int es = IN == 0 ? 4 : 2;
    const bool has_gs = gscale != nullptr;
    const float gs = has_gs ? gscale[e] : 1.0f;
    // Loads are unconditional: a lane past N reads row N - 1 (its results are never stored and reach no other lane's), a
    // lane past the count reads the expert's last row.
    const size_t wrow = (size_t)e * N + (n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KS;
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
    auto load_scales = [&](int piece) {                            // the two scale bytes of the piece of 32 k number `piece`
        return (uint16_t)((uint32_t)sbase[2 * piece] | ((uint32_t)sbase[2 * piece + 1] << 8));
    };
    auto load_slot = [&](Slot &sl, int j) {                        // the 64 k of pair j (both pieces exist)
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * j + 16 * h);
        sl.sc = load_scales(2 * j + h);
#pragma unroll
        for (int s = 0; s < 4; ++s) load_x(sl, j, s);
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    uint32_t bad = 0u;

    auto consume = [&](const Slot &sl) {                           // four instructions: k0 = 64 j + 16 s, s = 0 .. 3
        uint32_t w[4], own;
        mx4_decode_copy(sl.wq, sl.sc, w, own);                     // (as mx4_decode_body: the swaps overwrite copies)
        const auto lo = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);         // {d0 | d1}, {e0 | e1}
        const auto hi = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);         // {d2 | d3}, {e2 | e3}
        const auto sc = __builtin_amdgcn_permlane32_swap(own, own, false, false);           // piece 2 j's bytes, piece 2 j + 1's
        const uint32_t words[4] = {lo[0], hi[0], lo[1], hi[1]};
        const float sv[4] = {nv4_scale<0>(sc[0]), nv4_scale<1>(sc[0]), nv4_scale<0>(sc[1]), nv4_scale<1>(sc[1])};
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

    // K % 64 == 32: the last piece has no partner.  Both halves load it (the h = 1 lanes drop theirs below) and the 32 k
    // of x that exist; the rest of the slot is the zeros nv4_kernel pads its last stage with.
    const int pairs = K >> 6;
    const bool odd = (K & 32) != 0;
    Slot tail;
    if (odd) {
        tail.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * pairs);
        tail.sc = load_scales(2 * pairs);
#pragma unroll
        for (int s = 0; s < 2; ++s) load_x(tail, pairs, s);
    }
    __builtin_amdgcn_sched_barrier(0);

    // The ring, as mx4_decode_body's: no branch in the loop that loads; a slot index past the last pair loads the last
    // pair again and is not used.
    if (pairs > 0) {
        const int last = pairs - 1;
        Slot ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {                          // (in the order of their use: the waits count on it)
            load_slot(ring[i], i < last ? i : last);
            __builtin_amdgcn_sched_barrier(0);
        }
        int j = 0;
        for (; j + DEPTH <= pairs; j += DEPTH) {
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
            if (j + i < pairs) consume(ring[i]);                   // (uniform; slot i holds pair j + i)
    }
    if (odd) {
        if (h) { tail.wq = make_uint4(0u, 0u, 0u, 0u); tail.sc = 0x3838; }
#pragma unroll
        for (int s = 2; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < (IN == 0 ? 8 : 4); ++i) tail.x[s][i] = 0;
        consume(tail);
    }

    const auto both = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);   // the row's other half of k
    if (!row_ok) return;
    const bool row_nan = ((both[0] | both[1]) & 0x80008000u) != 0u;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
    nv4_epilogue<OUT>(acc, out, t, N, n0, h, vec, brow, has_gs, gs, row_nan);
}

// IN, OUT as nv4_kernel's.
template <int IN, int OUT>
__global__ __launch_bounds__(64) void nv4_decode_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const float *__restrict__ gscale,
    const void *__restrict__ x, const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4DecodeCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    const int e = blockIdx.z;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        nv4_decode_body<IN, OUT, true, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(blocks, scales, gscale, x, bias, out, e, row_lo, cnt, t_blk, K, N);
    else
        nv4_decode_body<IN, OUT, false, 1, 1>(blocks, scales, gscale, x, bias, out, e, row_lo, cnt, t_blk, K, N);
#endif
}
