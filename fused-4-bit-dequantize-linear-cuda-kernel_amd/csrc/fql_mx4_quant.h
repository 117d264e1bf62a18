// The row pre-passes of the MXFP4 expert kernels (include/fql_int4.h; DESIGN.md sections 25, 27, 28): each turns float32 or
// bfloat16 rows [T][K], or (GATED) act_glu_mul(gate_up[t][k], gate_up[t][K + k]) of gate_up [T][2 K] in float32, into the
// operand its GEMM reads, in the caller's workspace.  The three quantisers share one loader, mx4_load8.
//
// mx4_glu_kernel: the streaming pre-pass of the gated bfloat16 form.  h[t][k] = act_glu_mul(gate_up[t][k], gate_up[t][F + k])
// rounded once to bfloat16 into [T][F]; mx4_kernel then reads h as a bfloat16 operand.  (Forming h on load would evaluate
// expf once per 128-column block of the output: 23 times at gpt-oss's N = 2880.)
//
// mx4_q8_kernel: e4m3 rows with one float32 scale a row.  One wave a row: pass 1 takes max|v| over the row, pass 2 writes
// byte = e4m3(v / scale) (float32 division, to nearest even) with scale = max|v| / 448 in float32 (1 for an all-zero row):
// bit for bit oracle.quantize_activations_fp8.  GATED: v is evaluated in both passes (the row comes from cache the second
// time; no [T][K] float tensor exists).  A row with a non-finite v gets zero bytes and a NaN scale.
//
// mx4_q4_kernel: MXFP4 rows, quantize.quantize_mxfp4's rule bit for bit for every finite float32 / bfloat16 input.  Four
// lanes share a block of 32, eight elements each; the block's max |v| is taken on the float32 bits over two __shfl_xor
// steps; the scale code is max(exponent field - 2, 0) (= floor(log2 max) - 2 clamped at -127, + 127; the upper clamp
// cannot be reached), 127 for an all-zero block; mx4_e2m1_code rounds an element in integer arithmetic (subnormals
// included: no float32 operation whose result could be flushed or rounded twice).  Each lane stores one dword of codes
// (a quad: 16 contiguous bytes = one block), lane 0 of the quad the scale byte.  A block with a non-finite value gets zero
// codes and scale code 255.  GATED: v is evaluated once.
//
// mx4_q6_kernel: MXFP6 (e2m3) rows, quantize.quantize_mxfp6's rule bit for bit in the same way (mx4_e2m3_code; the scale code
// is mx4_q4_kernel's: both formats' largest exponent is 2); the comment at the kernel has the packing.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

// E8M0 code of a block whose largest |v| has the float32 bits mu (finite): shared = floor(log2 max) - 2 clamped to
// [-127, 127], + 127.  A subnormal or the two smallest normal binades clamp to code 0; an all-zero block is code 127.
__host__ __device__ inline int mx4_block_scale_code(uint32_t mu)
{
    if (mu == 0u) return 127;
    const int c = (int)(mu >> 23) - 2;
    return c < 0 ? 0 : c;
}

// e2m1 code of the float32 with bits `bits` (finite) under scale code c (of its own block: |v| / 2^(c - 127) < 8): to
// nearest even on {0, .5, 1, 1.5, 2, 3, 4, 6}, saturated at 6, the sign kept.  F = |v| / 2^(c - 127) in units of 2^-22
// with a sticky bit; the step of the grid is 2^21 units below 2, 2^22 below 4, 2^23 above.
__host__ __device__ inline uint32_t mx4_e2m1_code(uint32_t bits, int c)
{
    const uint32_t sign = (bits >> 28) & 8u, ex = (bits >> 23) & 255u, man = bits & 0x7FFFFFu;
    const uint32_t M = ex ? (man | 0x800000u) : man;
    const int sh = (int)(ex ? ex : 1u) - 1 - c;                    // (<= 1: the block's own maximum has ex - c <= 2)
    uint32_t F, sticky = 0u;
    if (sh >= 0) F = M << sh;
    else if (sh > -32) { F = M >> -sh; sticky = (M & ((1u << -sh) - 1u)) != 0u; }
    else { F = 0u; sticky = M != 0u; }
    const int s = F >= (1u << 24) ? 23 : F >= (1u << 23) ? 22 : 21;
    uint32_t q = F >> s;
    const uint32_t rem = F & ((1u << s) - 1u), half = 1u << (s - 1);
    if (rem > half || (rem == half && (sticky || (q & 1u)))) ++q;
    uint32_t hv = q << (s - 21);                                   // twice the rounded value: 0 1 2 3 4 6 8 12 (16)
    if (hv > 12u) hv = 12u;
    return sign | (hv < 4u ? hv : hv < 8u ? (hv >> 1) + 2u : (hv >> 2) + 4u);
}

// 8 consecutive elements at p of float32 (IN == 0) or bfloat16, widened.  vec: p is 16-byte aligned.
template <int IN>
__device__ __forceinline__ void mx4_load8(const char *p, bool vec, float (&v)[8])
{
    if constexpr (IN == 0) {
        const float *f = reinterpret_cast<const float *>(p);
        if (vec) {
            const v4f a = *reinterpret_cast<const v4f *>(f), b = *reinterpret_cast<const v4f *>(f + 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) { v[c] = a[c]; v[4 + c] = b[c]; }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = f[c];
        }
    } else {
        const unsigned short *s = reinterpret_cast<const unsigned short *>(p);
        if (vec) {
            const uint4 a = *reinterpret_cast<const uint4 *>(s);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) { v[2 * c] = __uint_as_float(w[c] << 16); v[2 * c + 1] = __uint_as_float(w[c] & 0xFFFF0000u); }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = act_widen<2>(s[c]);
        }
    }
}

// v[i] of k .. k + 7 of the row at `row` (K elements, GATED: gate (K) | up (K)); k % 8 == 0 and K % 32 == 0, so a
// 16-byte aligned base (vec) makes every piece 16-byte aligned.
template <int IN, bool GATED>
__device__ __forceinline__ void mx4_value8(const char *row, int k, int K, bool vec, int kind, float alpha, float limit,
                                           float (&v)[8])
{
    constexpr int es = IN == 0 ? 4 : 2;
    mx4_load8<IN>(row + (size_t)k * es, vec, v);
    if constexpr (GATED) {
        float u[8];
        mx4_load8<IN>(row + (size_t)(K + k) * es, vec, u);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = act_glu_mul(kind, alpha, limit, v[c], u[c]);
    }
}

// h[t][k] = bf16(act_glu_mul(gate_up[t][k], gate_up[t][F + k])): one thread = 8 consecutive k of one row (F % 32 == 0).
// (It loads gate and up side by side under ONE test of the alignment, four loads in flight: two mx4_load8 calls compile to
// two tests with a wait between them, so this kernel keeps its own loads.)
template <int IN>
__global__ __launch_bounds__(256) void mx4_glu_kernel(const void *__restrict__ gate_up, unsigned short *__restrict__ hbuf,
                                                      int T, int F, int kind, float alpha, float limit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int per_row = F >> 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)T * per_row) return;
    const int t = (int)(idx / per_row), k = (int)(idx % per_row) * 8;
    const int es = IN == 0 ? 4 : 2;
    const char *row = reinterpret_cast<const char *>(gate_up) + (size_t)t * 2 * F * es;
    const bool vec = (reinterpret_cast<uintptr_t>(gate_up) & 15) == 0;
    float g[8], u[8];
    if (IN == 0) {
        const float *gp = reinterpret_cast<const float *>(row) + k, *up = gp + F;
        if (vec) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const v4f a = *reinterpret_cast<const v4f *>(gp + 4 * i), b = *reinterpret_cast<const v4f *>(up + 4 * i);
#pragma unroll
                for (int c = 0; c < 4; ++c) { g[4 * i + c] = a[c]; u[4 * i + c] = b[c]; }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { g[c] = gp[c]; u[c] = up[c]; }
        }
    } else {
        const unsigned short *gp = reinterpret_cast<const unsigned short *>(row) + k, *up = gp + F;
        if (vec) {
            const uint4 a = *reinterpret_cast<const uint4 *>(gp), b = *reinterpret_cast<const uint4 *>(up);
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                g[2 * c] = __uint_as_float(aw[c] << 16); g[2 * c + 1] = __uint_as_float(aw[c] & 0xFFFF0000u);
                u[2 * c] = __uint_as_float(bw[c] << 16); u[2 * c + 1] = __uint_as_float(bw[c] & 0xFFFF0000u);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { g[c] = act_widen<2>(gp[c]); u[c] = act_widen<2>(up[c]); }
        }
    }
    uint4 o;
    uint32_t w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        w[c] = (uint32_t)f32_to_bf16_bits(act_glu_mul(kind, alpha, limit, g[2 * c], u[2 * c])) |
               ((uint32_t)f32_to_bf16_bits(act_glu_mul(kind, alpha, limit, g[2 * c + 1], u[2 * c + 1])) << 16);
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    *reinterpret_cast<uint4 *>(hbuf + (size_t)t * F + k) = o;      // (workspace: 16-byte aligned, F % 8 == 0)
#endif
}

// rows [T][K] (GATED: gate_up [T][2 K]) of float32 (IN == 0) or bfloat16 -> q [T][K] e4m3 bytes, act_scale [T].  One wave a
// row, a lane 8 consecutive k at a time (K % 32 == 0; q is 16-byte aligned, so its 8-byte stores are aligned).
template <int IN, bool GATED>
__global__ __launch_bounds__(256) void mx4_q8_kernel(const void *__restrict__ rows, uint8_t *__restrict__ q,
                                                     float *__restrict__ act_scale, int T, int K, int kind, float alpha,
                                                     float limit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;                                            // (uniform per wave)
    constexpr int es = IN == 0 ? 4 : 2;
    const char *row = reinterpret_cast<const char *>(rows) + (size_t)t * (GATED ? 2 : 1) * K * es;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    uint32_t mu = 0u;                                              // max |v| as bits (an exponent field of 255 wins)
    for (int k = 8 * lane; k < K; k += 512) {
        float v[8];
        mx4_value8<IN, GATED>(row, k, K, vec, kind, alpha, limit, v);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t u = __float_as_uint(v[c]) & 0x7FFFFFFFu;
            mu = u > mu ? u : mu;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mu, o, 64);
        mu = other > mu ? other : mu;
    }
    const bool bad = mu >= 0x7F800000u;
    const float m = __uint_as_float(mu);
    const float scale = (bad || m == 0.0f) ? 1.0f : m / 448.0f;
    if (lane == 0) act_scale[t] = bad ? __builtin_nanf("") : scale;
    uint8_t *qrow = q + (size_t)t * K;
    for (int k = 8 * lane; k < K; k += 512) {
        float v[8];
        mx4_value8<IN, GATED>(row, k, K, vec, kind, alpha, limit, v);
        float y[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) y[c] = (bad ? 0.0f : v[c]) / scale;
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
        *reinterpret_cast<uint2 *>(qrow + k) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
#endif
}

// rows [T][K] (GATED: gate_up [T][2 K]) of float32 (IN == 0) or bfloat16 -> qb [T][K / 2] packed e2m1, qs [T][K / 32] E8M0.
// One thread 8 consecutive k (K % 32 == 0: a quad of lanes is one block of one row, and a wave holds whole quads); qb is
// 4-byte aligned at least (every entry asks for 16), so a lane's dword store is aligned.
template <int IN, bool GATED>
__global__ __launch_bounds__(256) void mx4_q4_kernel(const void *__restrict__ rows, uint8_t *__restrict__ qb,
                                                     uint8_t *__restrict__ qs, int T, int K, int kind, float alpha, float limit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int per_row = K >> 3;
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long long)T * per_row) return;                    // (whole quads: T * K / 8 is a multiple of 4)
    const long long t = item / per_row;
    const int k = (int)(item - t * per_row) * 8;
    constexpr int es = IN == 0 ? 4 : 2;
    const char *row = reinterpret_cast<const char *>(rows) + (size_t)t * (GATED ? 2 : 1) * K * es;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    float v[8];
    mx4_load8<IN>(row + (size_t)k * es, vec, v);
    if constexpr (GATED) {
        float u[8];
        mx4_load8<IN>(row + (size_t)(K + k) * es, vec, u);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = act_glu_mul(kind, alpha, limit, v[c], u[c]);
    }
    uint32_t mu = 0u;                                              // max |v| as bits (an exponent field of 255 wins)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t u = __float_as_uint(v[c]) & 0x7FFFFFFFu;
        mu = u > mu ? u : mu;
    }
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mu, o, 64);
        mu = other > mu ? other : mu;
    }
    const bool bad = mu >= 0x7F800000u;
    const int code = bad ? 255 : mx4_block_scale_code(mu);
    uint32_t word = 0u;
    if (!bad) {
#pragma unroll
        for (int c = 0; c < 8; ++c) word |= mx4_e2m1_code(__float_as_uint(v[c]), code) << (4 * c);
    }
    *reinterpret_cast<uint32_t *>(qb + (size_t)t * (K >> 1) + (k >> 1)) = word;
    if ((threadIdx.x & 3) == 0) qs[(size_t)t * (K >> 5) + (k >> 5)] = (uint8_t)code;
#endif
}

// e2m3 code (sign << 5 | exponent << 3 | mantissa, bias 1) of the float32 with bits `bits` (finite) under scale code c of
// its own block, as mx4_e2m1_code: to nearest even on the grid whose step is 1/8 below 2, 1/4 below 4 and 1/2 above,
// saturated at 7.5 (7.75 is a tie that goes up to 8 and saturates), the sign kept.  F is in units of 2^-22, so the three
// steps are 2^19, 2^20 and 2^21 units.
__host__ __device__ inline uint32_t mx4_e2m3_code(uint32_t bits, int c)
{
    const uint32_t sign = (bits >> 26) & 32u, ex = (bits >> 23) & 255u, man = bits & 0x7FFFFFu;
    const uint32_t M = ex ? (man | 0x800000u) : man;
    const int sh = (int)(ex ? ex : 1u) - 1 - c;                    // (<= 1: the block's own maximum has ex - c <= 2)
    uint32_t F, sticky = 0u;
    if (sh >= 0) F = M << sh;
    else if (sh > -32) { F = M >> -sh; sticky = (M & ((1u << -sh) - 1u)) != 0u; }
    else { F = 0u; sticky = M != 0u; }
    const int s = F >= (1u << 24) ? 21 : F >= (1u << 23) ? 20 : 19;
    uint32_t q = F >> s;
    const uint32_t rem = F & ((1u << s) - 1u), half = 1u << (s - 1);
    if (rem > half || (rem == half && (sticky || (q & 1u)))) ++q;
    uint32_t ev = q << (s - 19);                                   // eight times the rounded value: 0 .. 64
    if (ev > 60u) ev = 60u;
    return sign | (ev < 16u ? ev : ev < 32u ? (ev >> 1) + 8u : (ev >> 2) + 16u);
}

// rows [T][K] (GATED: gate_up [T][2 K]) of float32 (IN == 0) or bfloat16 -> qc [T][3 K / 4] packed e2m3 (MXFP6: element i of
// block b is bits 6 i .. 6 i + 5 of the 24 bytes at 24 b, little endian), qs [T][K / 32] E8M0: quantize.quantize_mxfp6's rule
// bit for bit for every finite input, mx4_q4_kernel's skeleton.  One thread 8 consecutive k = 48 bits of its block; lane j of
// a quad then holds bits 48 j .. 48 j + 47, and lanes 0 .. 2 each store one 8-byte word of the block, (P_j >> 16 j) |
// (P_(j + 1) << (48 - 16 j)), with the next lane's bits from two __shfl_down.  qc is 8-byte aligned at least (every entry
// asks for 16) and a block starts at a multiple of 24 bytes of it, so the stores are aligned.  A block with a non-finite
// value gets zero codes and scale code 255.
template <int IN, bool GATED>
__global__ __launch_bounds__(256) void mx4_q6_kernel(const void *__restrict__ rows, uint8_t *__restrict__ qc,
                                                     uint8_t *__restrict__ qs, int T, int K, int kind, float alpha, float limit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int per_row = K >> 3;
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long long)T * per_row) return;                    // (whole quads: T * K / 8 is a multiple of 4)
    const long long t = item / per_row;
    const int k = (int)(item - t * per_row) * 8;
    constexpr int es = IN == 0 ? 4 : 2;
    const char *row = reinterpret_cast<const char *>(rows) + (size_t)t * (GATED ? 2 : 1) * K * es;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    float v[8];
    mx4_load8<IN>(row + (size_t)k * es, vec, v);
    if constexpr (GATED) {
        float u[8];
        mx4_load8<IN>(row + (size_t)(K + k) * es, vec, u);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = act_glu_mul(kind, alpha, limit, v[c], u[c]);
    }
    uint32_t mu = 0u;                                              // max |v| as bits (an exponent field of 255 wins)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t u = __float_as_uint(v[c]) & 0x7FFFFFFFu;
        mu = u > mu ? u : mu;
    }
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mu, o, 64);
        mu = other > mu ? other : mu;
    }
    const bool bad = mu >= 0x7F800000u;
    const int code = bad ? 255 : mx4_block_scale_code(mu);
    unsigned long long P = 0ull;
    if (!bad) {
#pragma unroll
        for (int c = 0; c < 8; ++c) P |= (unsigned long long)mx4_e2m3_code(__float_as_uint(v[c]), code) << (6 * c);
    }
    const int j = threadIdx.x & 3;
    const uint32_t nlo = (uint32_t)__shfl_down((int)(uint32_t)P, 1, 64), nhi = (uint32_t)__shfl_down((int)(uint32_t)(P >> 32), 1, 64);
    const unsigned long long Pn = ((unsigned long long)nhi << 32) | nlo;
    if (j < 3) {
        const unsigned long long w = (P >> (16 * j)) | (Pn << (48 - 16 * j));
        *reinterpret_cast<uint2 *>(qc + (size_t)t * (3 * (K >> 2)) + 24 * (k >> 5) + 8 * j) = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
    } else {
        qs[(size_t)t * (K >> 5) + (k >> 5)] = (uint8_t)code;
    }
#endif
}
