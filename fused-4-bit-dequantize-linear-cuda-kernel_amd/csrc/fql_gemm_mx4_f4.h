// Grouped GEMM on OCP MXFP4 expert weights over MXFP4 activation rows, both operands e2m1 with their own E8M0 block scales,
// on the block-scaled matrix cores (include/fql_int4.h, fql_moe_mx4_fwd_f4 / fql_moe_mx4_fwd_q4 / fql_moe_mx4_glu_fwd_q4 /
// fql_mx4_quantize_rows):
//
//   out[t][n] = sum_k e2m1(xc[t][k]) 2^(xs[t][k / 32] - 127) * e2m1(code[e][n][k]) 2^(s[e][n][k / 32] - 127)  (+ bias[e][n])
//
// blocks [E][N][K / 2] and scales [E][N][K / 32] as fql_gemm_mx4.h reads them; the rows are in the SAME layout, in_blocks
// [T][K / 2] (even k in the low nibble) and in_scales [T][K / 32].  Nothing is dequantised: both are operands of
// v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = 4 and blgp = 4, each with its scale byte.  The operand map, as
// tools/micro/mfma_f4_probe.hip f4f4 measured it (profiles/mfma_f4f4_probe.txt), lane = (r = lane & 31, h = lane >> 5):
//   * fp4 B mirrors fp4 A: the lane's 16 bytes (registers 0 .. 3; 4 .. 7 are ignored on both sides) are column r,
//     k = 32 h .. 32 h + 31 in memory order, the low nibble of a byte first: the bytes of one scale block of a packed row.
//     The two operands share slots (unlike fp4 x e4m3, fql_gemm_mx4_f8.h).
//   * scale B: byte op_sel (B's own selector, independent of A's) of the lane's B scale register scales the lane's own
//     32 nibbles (column r, block h).
//   * B scale code 255 makes the 32 outputs of its column NaN, against zero codes on either side too, and leaves the other
//     columns alone; codes 0 and 254 are 2^-127 and 2^127 (1.0 * 1.0 * 2^-127 came back as 0x00400000, nothing is flushed).
//     A column of the instruction is an output row t here: a row whose block holds a non-finite value gets scale code 255
//     from the quantiser and is NaN across exactly that row, with nothing flagged in the kernel.
//
// mx4_f4_kernel: mx4_f8_kernel's skeleton (workgroup = 4 waves = 64 rows t x 128 columns n of one expert, the table read on
// the device, blockIdx.z = expert, one more z-slice zeroes the rows no expert covers; wave w owns rows 32 (w >> 1) .. + 31
// and the 32-n blocks 2 (w & 1) and 2 (w & 1) + 1; a lane owns one output row t, registers 4q .. 4q+3 are 4 consecutive n).
//   * Stage = 128 k.  Weights: 128 n x 64 bytes, thread p copies the 16-byte pieces (row (p >> 2) + 64 i, block p & 3),
//     i = 0, 1, and their scale bytes.  Activations: 64 t x 64 bytes (half the fp8 kernel's), thread p copies the ONE piece
//     (row p >> 2 of the tile, clamped into the expert's range; block p & 3) and its scale byte.  in_blocks is 16-byte
//     aligned and K % 32 == 0, so every piece is one aligned 16-byte load.  Double buffered: 2 x (8 + 4) KiB of images and
//     1.5 KiB of scale bytes, 25.5 KiB.  Pieces past N or K are zero codes with scale code 127 on both sides (their scale
//     bytes are not read; an absent block is never NaN).  An instruction whose 64 k lie past K entirely is not issued.
//   * No padding: the 16-byte slot c of weight row n lives at slot c ^ ((n >> 2) & 3) of its 64-byte row, and slot c of
//     activation row t at c ^ ((t >> 2) & 3) of its 64-byte row: the same rule.  A ds_read_b128 is served in groups of 16
//     lanes; a group reads 16 consecutive rows (r .. r + 15 of a fragment) at the same c.  Four 64-byte rows fill a
//     256-byte bank row: row i of the group lies at byte 64 (i & 3) + 16 (c ^ ((i >> 2) & 3)) of its bank row, and (i & 3,
//     (i >> 2) & 3) takes 16 distinct values, so the group covers the 16 slots once: conflict free, for both operands.
//   * A operand of instruction s (k = k0 + 64 s .. + 63): slot 2 s + h of row 32 b + r; B operand: slot 2 s + h of row t,
//     shared by the wave's two n blocks: one ds_read_b128 each.  The scale bytes lie in LDS as [h][row][s], so one 16-bit
//     read per fragment and stage gives a lane both of its bytes, byte s selected by op_sel (A's and B's alike).
//   * The loads of a stage are issued TWO stages ahead of their use, into two register sets that alternate.
//   * FIXED ORDER.  Stages in ascending k, instruction 0 then 1 inside a stage, one accumulator per output.  A row's result
//     depends on its own bytes, its scales and its expert's weights only.  No atomics, every element is written once.
//   * EPILOGUE, float32: v = acc, with a bias v = acc + bias[e][n] (one addition), then the one rounding to out's type.
//
// mx4_q4_kernel: the quantiser, quantize.quantize_mxfp4's rule bit for bit for every finite float32 / bfloat16 input.  Four
// lanes share a block of 32, eight elements each; the block's max |v| is taken on the float32 bits over two __shfl_xor
// steps; the scale code is max(exponent field - 2, 0) (= floor(log2 max) - 2 clamped at -127, + 127; the upper clamp
// cannot be reached), 127 for an all-zero block; mx4_e2m1_code rounds an element in integer arithmetic (subnormals
// included: no float32 operation whose result could be flushed or rounded twice).  Each lane stores one dword of codes
// (a quad: 16 contiguous bytes = one block), lane 0 of the quad the scale byte.  A block with a non-finite value gets zero
// codes and scale code 255.  GATED: v = act_glu_mul(gate_up[t][k], gate_up[t][K + k]) in float32, evaluated once.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

struct Mx4F4Cfg {
    static constexpr int BT = 64, BN = 128, BK = 128;  // rows, columns and contraction depth of a stage
    static constexpr int THREADS = 256;
};

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

// The epilogue of one 32-n block (columns nb0 .. nb0 + 31) of the lane's row t, shared by mx4_f4_kernel and the decode
// kernel (fql_gemm_mx4_sdecode.h): registers 4q .. 4q+3 of acc are n = nb0 + 8 q + 4 h + (0 .. 3).
template <int OUT>
__device__ __forceinline__ void mx4_f4_epilogue(const v16f &acc, void *__restrict__ out, int t, int N, int nb0, int h, bool vec,
                                                const float *__restrict__ brow)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nc = nb0 + 8 * q + 4 * h;
        if (nc >= N) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = acc[4 * q + c];
            if (brow != nullptr && nc + c < N) v[c] = __fadd_rn(v[c], brow[nc + c]);
        }
        store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
    }
}

// OUT: element type of out, rounded once in the epilogue.
template <int OUT>
__global__ __launch_bounds__(256) void mx4_f4_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const uint8_t *__restrict__ xb,
    const uint8_t *__restrict__ xs, const float *__restrict__ bias, void *__restrict__ out,
    const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4F4Cfg;
    if ((int)blockIdx.z == E) {                                    // (with a table only) the rows no expert covers
        const int blk = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        if ((long long)blk * 256 < T) act_zero_uncovered(blk, out, OUT == 0 ? 4 : 2, N, tpe, offs, E, T);
        return;
    }
    __shared__ __attribute__((aligned(16))) uint4 wimg[2][C::BN][4];   // packed weight rows, 128 k = 64 bytes, slots swizzled
    __shared__ __attribute__((aligned(16))) uint4 ximg[2][C::BT][4];   // packed activation rows, the same
    __shared__ __attribute__((aligned(4))) uint8_t simg[2][2][C::BN][2];   // E8M0 bytes: [h][n][s] = block 2 s + h of the stage (read in pairs)
    __shared__ __attribute__((aligned(4))) uint8_t ximgs[2][2][C::BT][2];  // the activations': [h][t][s]

    const int e = blockIdx.z;
    int row_lo = 0, cnt = T;
    if (tpe != nullptr) expert_range(tpe, offs, e, T, row_lo, cnt);
    const int t_blk = (int)blockIdx.y * C::BT;
    if (t_blk >= cnt) return;                                      // (uniform per workgroup)
    const int n0 = (int)blockIdx.x * C::BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nb = (wave & 1) * 2;                                 // first of this wave's two 32-n blocks
    const int tr = (wave >> 1) * 32 + r;                           // this lane's row inside the tile
    const bool row_ok = t_blk + tr < cnt;
    const int t = row_lo + t_blk + tr;
    const int K2 = K >> 1, KB = K >> 5;

    // staging roles of this thread: weight pieces (row sn + 64 i, block sc of the stage), the activation piece (row sn of
    // the tile, clamped into the expert's range: loads are unconditional; block sc)
    const int sn = tid >> 2, sc = tid & 3;
    const uint8_t *wbase[2], *sbase[2];
    bool n_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        n_ok[i] = n0 + sn + 64 * i < N;
        const size_t wrow = (size_t)e * N + (n_ok[i] ? n0 + sn + 64 * i : 0);
        wbase[i] = blocks + wrow * K2 + 16 * sc;
        sbase[i] = scales + wrow * KB + sc;
    }
    const size_t tx = (size_t)(row_lo + (t_blk + sn < cnt ? t_blk + sn : cnt - 1));
    const uint8_t *xbase = xb + tx * K2 + 16 * sc, *xsbase = xs + tx * KB + sc;

    struct Stage {                                                 // what a thread holds of one stage between load and use
        uint4 w[2], x;
        int s[2], xs;
    };
    auto load_stage = [&](Stage &st, int k0) {
        const bool k_ok = k0 + 32 * sc < K;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            st.w[i] = make_uint4(0u, 0u, 0u, 0u);
            st.s[i] = 127;
            if (n_ok[i] && k_ok) {
                st.w[i] = *reinterpret_cast<const uint4 *>(wbase[i] + (k0 >> 1));
                st.s[i] = sbase[i][k0 >> 5];
            }
        }
        st.x = make_uint4(0u, 0u, 0u, 0u);
        st.xs = 127;
        if (k_ok) {
            st.x = *reinterpret_cast<const uint4 *>(xbase + (k0 >> 1));
            st.xs = xsbase[k0 >> 5];
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> LDS, bytes as loaded
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = sn + 64 * i;
            wimg[buf][n][sc ^ ((n >> 2) & 3)] = st.w[i];
            simg[buf][sc & 1][n][sc >> 1] = (uint8_t)st.s[i];
        }
        ximg[buf][sn][sc ^ ((sn >> 2) & 3)] = st.x;
        ximgs[buf][sc & 1][sn][sc >> 1] = (uint8_t)st.xs;
    };

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    // instruction S of the stage in buffer `buf`: k = k0 + 64 S .. + 63
    auto step = [&](auto S, int buf, const int (&sw)[2], int sx) {
        constexpr int s = decltype(S)::value;
        const uint4 x = ximg[buf][tr][(2 * s + h) ^ ((tr >> 2) & 3)];
        const v8i bv = {(int)x.x, (int)x.y, (int)x.z, (int)x.w, 0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = 32 * (nb + b) + r;
            const uint4 a = wimg[buf][n][(2 * s + h) ^ ((n >> 2) & 3)];
            const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
            acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[b], 4, 4, s, sw[b], s, sx);
        }
    };

    // Stage i: refill `mine` (consumed one stage ago) with the loads of stage i + 2, contract the images of stage i, then
    // turn `other` (stage i + 1, loaded one stage ago) into the other set of images.  Two stages of loads are in flight.
    auto run_stage = [&](Stage &mine, const Stage &other, int k0, int it) {
        if (k0 + 2 * C::BK < K) load_stage(mine, k0 + 2 * C::BK);
        const int buf = it & 1;
        int sw[2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
            sw[b] = *reinterpret_cast<const unsigned short *>(&simg[buf][h][32 * (nb + b) + r][0]);
        const int sx = *reinterpret_cast<const unsigned short *>(&ximgs[buf][h][tr][0]);
        step(std::integral_constant<int, 0>{}, buf, sw, sx);
        if (k0 + 64 < K) step(std::integral_constant<int, 1>{}, buf, sw, sx);
        if (k0 + C::BK < K) store_stage(other, (it + 1) & 1);      // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    };

    Stage s0, s1;
    load_stage(s0, 0);
    s1 = s0;                                                       // (K <= 128: never read)
    if (C::BK < K) load_stage(s1, C::BK);
    store_stage(s0, 0);
    __syncthreads();
    for (int k0 = 0, it = 0; k0 < K; k0 += 2 * C::BK, it += 2) {
        run_stage(s0, s1, k0, it);
        if (k0 + C::BK < K) run_stage(s1, s0, k0 + C::BK, it + 1);
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    if (!row_ok) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
#pragma unroll
    for (int b = 0; b < 2; ++b) mx4_f4_epilogue<OUT>(acc[b], out, t, N, n0 + 32 * (nb + b), h, vec, brow);
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
    auto load8 = [&](const char *p, float (&v)[8]) {               // 8 elements at p, widened
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
    };
    float v[8];
    load8(row + (size_t)k * es, v);
    if constexpr (GATED) {
        float u[8];
        load8(row + (size_t)(K + k) * es, u);
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
