// Grouped GEMM on OCP MXFP4 expert weights over fp8 (OCP e4m3) activation rows, on the block-scaled matrix cores
// (include/fql_int4.h, fql_moe_mx4_fwd_f8 / fql_moe_mx4_fwd_q8 / fql_moe_mx4_glu_fwd_q8):
//
//   out[t][n] = act_scale[t] * ( sum_k e4m3(x8[t][k]) * e2m1(code[e][n][k]) * 2^(s[e][n][k / 32] - 127) ) (+ bias[e][n])
//
// blocks [E][N][K / 2] and scales [E][N][K / 32] as fql_gemm_mx4.h reads them.  Nothing is dequantised: the packed bytes are
// the fp4 A operand of v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz = 4) and the checkpoint's E8M0 byte is its A scale; the e4m3
// bytes are the B operand (blgp = 0) with scale code 127.  The operand map, as tools/micro/mfma_f4_probe.hip measured it
// (profiles/mfma_f4_probe.txt), lane = (r = lane & 31, h = lane >> 5):
//   * fp4 A: the lane's 16 bytes (registers 0 .. 3; 4 .. 7 are ignored) are row r, k = 32 h .. 32 h + 31 in memory order, the
//     low nibble of a byte first: exactly the bytes of one scale block of a packed row.
//   * e4m3 B: the lane's bytes 0 .. 15 are column r, k = 16 h .. 16 h + 15, bytes 16 .. 31 are k = 32 + 16 h .. + 15.
//   * scale A: byte op_sel of the lane's scale register scales the lane's own 32 nibbles (row r, block h).
//   * scale code 255 makes the outputs of its row NaN (zero codes included), an e4m3 NaN byte (0x7F / 0xFF) those of its
//     column (against zero codes too): the instruction does what the project's conventions ask, nothing is flagged here.
//     Codes 0 and 254 are 2^-127 and 2^127: 1.0 * 2^-127 came back as the float32 subnormal 0x00400000 (nothing is flushed
//     inside the instruction), 1.0 * 2^127 as 0x7F000000; sums past the float32 range are infinite as in float32.
//
// mx4_f8_kernel: workgroup = 4 waves = a tile of 64 rows t x 128 columns n of one expert, the skeleton of mx4_kernel (expert
// table read on the device, blockIdx.z = expert; wave w owns rows 32 (w >> 1) .. + 31 and the 32-n blocks 2 (w & 1) and
// 2 (w & 1) + 1, which share its activation registers; a lane owns one output row t, registers 4q .. 4q+3 are 4
// consecutive n: store_out4).
//   * Stage = 128 k.  Weights: 128 n x 64 bytes, thread p copies the 16-byte pieces (row (p >> 2) + 64 i, block p & 3),
//     i = 0, 1: four threads read one 64-byte run of a packed row, and a piece is one scale block, so one scale byte goes
//     with it.  Activations: 64 t x 128 bytes, thread p copies the pieces (row (p >> 3) + 32 i, bytes 16 (p & 7) .. + 15):
//     eight threads a 128-byte line.  Both are written to LDS as loaded, double buffered (2 x 8 KiB each, 33 KiB with
//     the scale bytes): one workgroup barrier a stage.  Pieces past N or K are zero codes with scale code 127 (their scale
//     byte is not read; an absent block is never NaN) and zero activation bytes; K % 32 == 0 is all the kernel asks, so a
//     half-filled last instruction (K % 64 == 32) and a partial last stage are the normal case (gpt-oss: K = 2880 = 22.5
//     stages).  An instruction whose 64 k lie past K entirely is not issued.
//   * No padding: the 16-byte slot c of weight row n lives at slot c ^ ((n >> 2) & 3) of its 64-byte row, slot c of
//     activation row t at c ^ ((t >> 1) & 7) of its 128-byte row.  A ds_read_b128 is served in groups of 16 lanes whose rows
//     are distinct modulo 16 and which read the same c: the XOR spreads each group over the 16 slots of the 256-byte bank
//     row, so the fragment reads are conflict free.
//   * A operand of instruction s (k = k0 + 64 s .. + 63): slot 2 s + h of row 32 b + r: one ds_read_b128.  Its scale bytes
//     lie in LDS as simg[h][n][s], so one 16-bit read per block and stage gives the lane both, byte s selected by op_sel.
//   * B operand: slots 4 s + h and 4 s + 2 + h of row t: two ds_read_b128, shared by the wave's two n blocks.
//   * The loads of a stage are issued TWO stages ahead of their use, into two register sets that alternate.
//   * FIXED ORDER.  Stages in ascending k, instruction 0 then 1 inside a stage, one accumulator per output.  A row's
//     result depends on its own bytes, its scale and its expert's weights only: the grouped call equals E one-expert calls
//     bit for bit.  No atomics, every element is written once; with a table one more z-slice zeroes the rows no expert
//     covers (act_zero_uncovered).
//   * EPILOGUE, float32: v = act_scale[t] * acc (one multiplication; act_scale == NULL: v = acc), with a bias
//     v = fma(act_scale[t], acc, bias[e][n]) (one rounding), then the one rounding to out's type (store_out4).  A NaN
//     act_scale makes the whole row NaN (NaN * 0 is NaN).
//
// mx4_q8_kernel: the quantising pre-pass.  One wave a row: pass 1 takes max|v| over the row, pass 2 writes
// byte = e4m3(v / scale) (float32 division, to nearest even) with scale = max|v| / 448 in float32 (1 for an all-zero row):
// bit for bit oracle.quantize_activations_fp8.  v = the float32 or widened bfloat16 element, or (GATED)
// act_glu_mul(gate_up[t][k], gate_up[t][F + k]) in float32, evaluated in both passes (the row comes from cache the second
// time; no [T][K] float tensor exists).  A row with a non-finite v gets zero bytes and a NaN scale.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

struct Mx4F8Cfg {
    static constexpr int BT = 64, BN = 128, BK = 128;  // rows, columns and contraction depth of a stage
    static constexpr int THREADS = 256;
};

// The epilogue of one 32-n block (columns nb0 .. nb0 + 31) of the lane's row t, shared by mx4_f8_kernel and the decode
// kernel (fql_gemm_mx4_sdecode.h): registers 4q .. 4q+3 of acc are n = nb0 + 8 q + 4 h + (0 .. 3).
template <int OUT>
__device__ __forceinline__ void mx4_f8_epilogue(const v16f &acc, void *__restrict__ out, int t, int N, int nb0, int h, bool vec,
                                                const float *__restrict__ brow, const float *__restrict__ act_scale, float as)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nc = nb0 + 8 * q + 4 * h;
        if (nc >= N) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float a = acc[4 * q + c];
            if (brow != nullptr && nc + c < N) v[c] = __fmaf_rn(as, a, brow[nc + c]);
            else v[c] = act_scale == nullptr ? a : __fmul_rn(as, a);
        }
        store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
    }
}

// OUT: element type of out, rounded once in the epilogue.
template <int OUT>
__global__ __launch_bounds__(256) void mx4_f8_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const uint8_t *__restrict__ x,
    const float *__restrict__ act_scale, const float *__restrict__ bias, void *__restrict__ out,
    const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4F8Cfg;
    if ((int)blockIdx.z == E) {                                    // (with a table only) the rows no expert covers
        const int blk = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        if ((long long)blk * 256 < T) act_zero_uncovered(blk, out, OUT == 0 ? 4 : 2, N, tpe, offs, E, T);
        return;
    }
    __shared__ __attribute__((aligned(16))) uint4 wimg[2][C::BN][4];   // packed weight rows, 128 k = 64 bytes, slots swizzled
    __shared__ __attribute__((aligned(16))) uint4 ximg[2][C::BT][8];   // e4m3 rows, 128 bytes, slots swizzled
    __shared__ __attribute__((aligned(4))) uint8_t simg[2][2][C::BN][2];   // E8M0 bytes: [h][n][s] = block 2 s + h of the stage (read in pairs)

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

    // staging roles of this thread: weight pieces (row sn + 64 i, block sc of the stage), activation pieces (row xs + 32 i
    // of the tile, clamped into the expert's range: loads are unconditional; slot xq)
    const int sn = tid >> 2, sc = tid & 3, xs = tid >> 3, xq = tid & 7;
    const uint8_t *wbase[2], *sbase[2], *xrow[2];
    bool n_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        n_ok[i] = n0 + sn + 64 * i < N;
        const size_t wrow = (size_t)e * N + (n_ok[i] ? n0 + sn + 64 * i : 0);
        wbase[i] = blocks + wrow * K2 + 16 * sc;
        sbase[i] = scales + wrow * KB + sc;
        const int tx = row_lo + (t_blk + xs + 32 * i < cnt ? t_blk + xs + 32 * i : cnt - 1);
        xrow[i] = x + (size_t)tx * K + 16 * xq;
    }
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (K % 32 == 0: every row starts on a 16-byte boundary then)

    struct Stage {                                                 // what a thread holds of one stage between load and use
        uint4 w[2], x[2];
        int s[2];
    };
    auto load_stage = [&](Stage &st, int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            st.w[i] = make_uint4(0u, 0u, 0u, 0u);
            st.s[i] = 127;
            if (n_ok[i] && k0 + 32 * sc < K) {
                st.w[i] = *reinterpret_cast<const uint4 *>(wbase[i] + (k0 >> 1));
                st.s[i] = sbase[i][k0 >> 5];
            }
            st.x[i] = make_uint4(0u, 0u, 0u, 0u);
            if (k0 + 16 * xq < K) {
                const uint8_t *p = xrow[i] + k0;
                if (vec_x) {
                    st.x[i] = *reinterpret_cast<const uint4 *>(p);
                } else {
                    uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 16; ++j) wd[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
                    st.x[i] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                }
            }
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> LDS, bytes as loaded
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = sn + 64 * i, tt = xs + 32 * i;
            wimg[buf][n][sc ^ ((n >> 2) & 3)] = st.w[i];
            simg[buf][sc & 1][n][sc >> 1] = (uint8_t)st.s[i];
            ximg[buf][tt][xq ^ ((tt >> 1) & 7)] = st.x[i];
        }
    };

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    // instruction S of the stage in buffer `buf`: k = k0 + 64 S .. + 63
    auto step = [&](auto S, int buf, const int (&sw)[2]) {
        constexpr int s = decltype(S)::value;
        const int xsw = (tr >> 1) & 7;
        const uint4 x0 = ximg[buf][tr][(4 * s + h) ^ xsw], x1 = ximg[buf][tr][(4 * s + 2 + h) ^ xsw];
        const v8i bv = {(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w, (int)x1.x, (int)x1.y, (int)x1.z, (int)x1.w};
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = 32 * (nb + b) + r;
            const uint4 a = wimg[buf][n][(2 * s + h) ^ ((n >> 2) & 3)];
            const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
            acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[b], 4, 0, s, sw[b], 0, 0x7F7F7F7F);
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
        step(std::integral_constant<int, 0>{}, buf, sw);
        if (k0 + 64 < K) step(std::integral_constant<int, 1>{}, buf, sw);
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
    const float as = act_scale == nullptr ? 1.0f : act_scale[t];
#pragma unroll
    for (int b = 0; b < 2; ++b) mx4_f8_epilogue<OUT>(acc[b], out, t, N, n0 + 32 * (nb + b), h, vec, brow, act_scale, as);
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
    auto value8 = [&](int k, float (&v)[8]) {                      // v[i] of k .. k + 7
        load8(row + (size_t)k * es, v);
        if constexpr (GATED) {
            float u[8];
            load8(row + (size_t)(K + k) * es, u);
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = act_glu_mul(kind, alpha, limit, v[c], u[c]);
        }
    };
    uint32_t mu = 0u;                                              // max |v| as bits (an exponent field of 255 wins)
    for (int k = 8 * lane; k < K; k += 512) {
        float v[8];
        value8(k, v);
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
        value8(k, v);
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
