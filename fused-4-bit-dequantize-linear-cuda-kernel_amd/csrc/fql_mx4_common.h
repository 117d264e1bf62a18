// What the grouped MXFP4 kernels share: the workgroup preamble of all of them, and the code-to-bfloat16
// conversion and the non-finite flag of the three bfloat16 kernels (fql_gemm_mx4.h, fql_gemm_mx4_decode.h,
// fql_gemm_mx4_bwd.h).  Every function here replaces literal copies; none adds a step.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

#ifndef FQL_MX4_CVT
#define FQL_MX4_CVT 1          // 1: v_cvt_scalef32_pk_bf16_fp4 (two codes an instruction); 0: integer arithmetic
#endif

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

// The head of a grouped kernel whose grid is (column blocks, blocks of BT rows, E (+ 1 with a table)).  The z-slice past
// the experts zeroes the rows of out [T][width] no expert covers, THREADS rows a workgroup (act_zero_uncovered); the others
// read their expert's row range from the table on the device.  False: the workgroup has nothing to do, uniformly (the
// coverage slice, or a row block past the expert's count), and returns before its first barrier.
template <int THREADS, int OUT>
__device__ __forceinline__ bool mx4_group_begin(void *__restrict__ out, int width, const int32_t *__restrict__ tpe,
                                                const int32_t *__restrict__ offs, int E, int T, int BT, int &row_lo, int &cnt,
                                                int &t_blk)
{
    if ((int)blockIdx.z == E) {                                    // (with a table only) the rows no expert covers
        long long blk;                                             // (a tile grid's flat index fits 32 bits, a one-wave grid's may not)
        if constexpr (THREADS == 256) blk = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        else blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
        if (blk * THREADS < T) act_zero_uncovered<THREADS>((int)blk, out, OUT == 0 ? 4 : 2, width, tpe, offs, E, T);
        return false;
    }
    row_lo = 0;
    cnt = T;
    if (tpe != nullptr) expert_range(tpe, offs, blockIdx.z, T, row_lo, cnt);
    t_blk = (int)blockIdx.y * BT;
    return t_blk < cnt;                                            // (uniform per workgroup)
}

// bfloat16 bits of e2m1 code c (4 bits, sign included) times 2^(s - 127); base = (s - 1) << 7.  Code 1 (0.5) is e2m1's
// one subnormal: exponent field s - 1, mantissa 0; codes 2 .. 7 are (mag << 6) above that.  A field below 1 is flushed
// to zero, one above 254 is infinity.
__device__ __forceinline__ uint32_t mx4_elem_bits(uint32_t c, int base)
{
    const uint32_t mag = c & 7u;
    int v = base + (mag == 1u ? 0 : (int)(mag << 6));
    v = v < 128 ? 0 : (v > 0x7F80 ? 0x7F80 : v);
    if (mag == 0u) v = 0;
    return (uint32_t)v | ((c & 8u) << 12);
}

// The two codes of byte `B` of w as one word of two bfloat16 (low nibble = even k in the low half), times the scale of
// code sc (< 255: the caller handles NaN).
template <int B>
__device__ __forceinline__ uint32_t mx4_pair(uint32_t w, int sc)
{
#if FQL_MX4_CVT
    const float scale = __uint_as_float(sc == 0 ? 0x00400000u : (uint32_t)sc << 23);
    const v2bf p = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, B);
    return __builtin_bit_cast(uint32_t, p);
#else
    const uint32_t byte = (w >> (8 * B)) & 0xFFu;
    const int base = (sc - 1) * 128;
    return mx4_elem_bits(byte & 0xFu, base) | (mx4_elem_bits(byte >> 4, base) << 16);
#endif
}

// One dword of a packed piece (8 codes, 8 consecutive k) under its block's scale code -> 8 bfloat16; code 255: NaN across.
__device__ __forceinline__ uint4 mx4_dequant8(uint32_t w, int code)
{
    const bool nan = code == 255;
    const int s = nan ? 127 : code;
    uint4 o;
    o.x = mx4_pair<0>(w, s);
    o.y = mx4_pair<1>(w, s);
    o.z = mx4_pair<2>(w, s);
    o.w = mx4_pair<3>(w, s);
    if (nan) o = make_uint4(0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u);
    return o;
}

// two float32 -> one word of two bfloat16, to nearest even (lo in the low half)
__device__ __forceinline__ uint32_t mx4_pack_bf16(float lo, float hi)
{
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// Non-finite flag of a word of two bfloat16: bit 15 of a half is set where its exponent field is 255 (0x7F80 + 0x80 =
// 0x8000 in a half; no carry between them).  OR the words of a row, then test with 0x80008000.
__device__ __forceinline__ uint32_t mx4_nonfinite2(uint32_t w) { return (w & 0x7F807F80u) + 0x00800080u; }
