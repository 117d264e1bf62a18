// Grouped GEMM on OCP MXFP4 expert weights on the block-scaled matrix cores, over fp8 (OCP e4m3) activation rows with one
// float32 scale a row (ROWS = 1: include/fql_int4.h, fql_moe_mx4_fwd_f8 / _fwd_q8 / _glu_fwd_q8),
// over MXFP4 activation rows (ROWS = 2: fql_moe_mx4_fwd_f4 / _fwd_q4 / _glu_fwd_q4) or over MXFP6 (e2m3)
// activation rows (ROWS = 3: fql_moe_mx4_fwd_f6 / _fwd_q6 / _glu_fwd_q6):
//
//   ROWS 1: out[t][n] = act_scale[t] * ( sum_k e4m3(x8[t][k]) * e2m1(code[e][n][k]) * 2^(s[e][n][k / 32] - 127) ) (+ bias[e][n])
//   ROWS 2: out[t][n] = sum_k e2m1(xc[t][k]) 2^(xs[t][k / 32] - 127) * e2m1(code[e][n][k]) 2^(s[e][n][k / 32] - 127)  (+ bias[e][n])
//   ROWS 3: the same with e2m3(xc[t][k]): x [T][3 K / 4], element i of block b in bits 6 i .. 6 i + 5 of the 24 bytes at 24 b
//           (one little-endian 192-bit integer), code = sign << 5 | exponent << 3 | mantissa (bias 1), xscales [T][K / 32]
//
// blocks [E][N][K / 2] and scales [E][N][K / 32] as fql_gemm_mx4.h reads them; MXFP4 rows are in the SAME layout, x [T][K / 2]
// (even k in the low nibble) and xscales [T][K / 32].  Nothing is dequantised: the packed bytes are the fp4 A operand of
// v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz = 4) and the checkpoint's E8M0 byte is its A scale; the rows are the B operand, e4m3
// bytes (blgp = 0) with scale code 127, packed e2m1 (blgp = 4) or packed e2m3 (blgp = 2) with their own scale byte.  The
// operand map, as tools/micro/mfma_f4_probe.hip measured it (profiles/mfma_f4_probe.txt, profiles/mfma_f4f4_probe.txt,
// profiles/mfma_f6_probe.txt), lane = (r = lane & 31, h = lane >> 5):
//   * fp4 A: the lane's 16 bytes (registers 0 .. 3; 4 .. 7 are ignored) are row r, k = 32 h .. 32 h + 31 in memory order, the
//     low nibble of a byte first: exactly the bytes of one scale block of a packed row.
//   * e4m3 B: the lane's bytes 0 .. 15 are column r, k = 16 h .. 16 h + 15, bytes 16 .. 31 are k = 32 + 16 h .. + 15.
//   * fp4 B mirrors fp4 A (column r, one scale block of a packed row; registers 4 .. 7 ignored): the two operands share slots.
//   * e2m3 B: the lane's 24 bytes (registers 0 .. 5; 6 and 7 are ignored) are column r, k = 32 h + J in bits 6 J .. 6 J + 5 of
//     the 24 bytes read as one little-endian integer: exactly the bytes of one scale block of an MXFP6 row, so the public
//     layout is the instruction's and nothing is reordered.  Its scale is byte op_sel of the lane's own B scale register;
//     scale code 255 makes the 32 outputs of its column NaN (zero codes on both sides included) and no other, codes 0 and
//     254 are 2^-127 (the float32 subnormal comes back) and 2^127.
//   * scale A / scale B: byte op_sel (each side has its own selector) of the lane's scale register scales the lane's own 32
//     nibbles (row / column r, block h).
//   * scale code 255 makes the outputs of its row NaN (zero codes included), an e4m3 NaN byte (0x7F / 0xFF) or a B scale
//     code 255 those of its column (against zero codes too) and leaves the other columns alone: the instruction does what
//     the project's conventions ask, nothing is flagged here.  A column of the instruction is an output row t: a row whose
//     block holds a non-finite value gets scale code 255 from the quantiser and is NaN across exactly that row.
//     Codes 0 and 254 are 2^-127 and 2^127: 1.0 * 2^-127 came back as the float32 subnormal 0x00400000 (nothing is flushed
//     inside the instruction), 1.0 * 2^127 as 0x7F000000; sums past the float32 range are infinite as in float32.
//
// mx4_scaled_kernel<ROWS, OUT>: workgroup = 4 waves = a tile of 64 rows t x 128 columns n of one expert, the skeleton of
// mx4_kernel (expert table read on the device, blockIdx.z = expert; wave w owns rows 32 (w >> 1) .. + 31 and the 32-n blocks
// 2 (w & 1) and 2 (w & 1) + 1, which share its activation registers; a lane owns one output row t, registers 4q .. 4q+3 are
// 4 consecutive n: store_out4).  Its decode form is mx4_sdecode_kernel (fql_gemm_mx4_sdecode.h): the same bits.
//   * Stage = 128 k.  Weights: 128 n x 64 bytes, thread p copies the 16-byte pieces (row (p >> 2) + 64 i, block p & 3),
//     i = 0, 1: four threads read one 64-byte run of a packed row, and a piece is one scale block, so one scale byte goes
//     with it.  e4m3 rows: 64 t x 128 bytes, thread p copies the pieces (row (p >> 3) + 32 i, bytes 16 (p & 7) .. + 15):
//     eight threads a 128-byte line; a row base that is not 16-byte aligned takes byte loads.  MXFP4 rows: 64 t x 64 bytes,
//     thread p copies the ONE piece (row p >> 2, block p & 3) and its scale byte; x is 16-byte aligned and K % 32 == 0, so
//     every piece is one aligned 16-byte load.  Rows are clamped into the expert's range: loads are unconditional.  All of
//     it is written to LDS as loaded, double buffered: 2 x (8 + 8) KiB and 1 KiB of scale bytes (33 KiB) with e4m3 rows,
//     2 x (8 + 4) KiB and 1.5 KiB (25.5 KiB) with MXFP4 rows; one workgroup barrier a stage.  MXFP6 rows: 64 t x 96 bytes,
//     thread p copies the ONE block (row p >> 2, block p & 3) of 24 bytes as three 8-byte words and its scale byte: x is
//     8-byte aligned and a row is a multiple of 24 bytes, so every word is one aligned 8-byte load whatever K % 64 is (rows
//     are 16-byte aligned only when K % 64 == 0: there is one form, not two); 2 x (8 + 6.75) KiB and 1.5 KiB (31 KiB).  Pieces past N or K are zero
//     codes with scale code 127 on either side (their scale byte is not read; an absent block is never NaN) and zero e4m3
//     bytes; K % 32 == 0 is all the kernel asks, so a half-filled last instruction (K % 64 == 32) and a partial last stage
//     are the normal case (gpt-oss: K = 2880 = 22.5 stages).  An instruction whose 64 k lie past K entirely is not issued.
//   * No padding: the 16-byte slot c of a 64-byte row i (weights, MXFP4 rows) lives at slot c ^ ((i >> 2) & 3), slot c of a
//     128-byte e4m3 row t at c ^ ((t >> 1) & 7).  A ds_read_b128 is served in groups of 16 lanes which read 16 consecutive
//     rows of a fragment at the same c.  Four 64-byte rows fill a 256-byte bank row: row i of the group lies at byte
//     64 (i & 3) + 16 (c ^ ((i >> 2) & 3)), and (i & 3, (i >> 2) & 3) takes 16 distinct values; two 128-byte rows fill one,
//     and (t & 1, (t >> 1) & 7) does the same.  Either way the group covers the 16 slots once: conflict free.
//   * MXFP6 image: word j (of 3) of block c (of 4) of row t is the uint2 at [j][c][t] of a plane of 64 + 8 rows, i.e. at byte
//     576 (4 j + c) + 8 t of the buffer.  A ds_read_b64 is served in halves of 32 lanes; a half reads word j of block 2 s + h
//     of 32 consecutive rows, 256 contiguous bytes = every bank once: conflict free.  A ds_write_b64 half is threads p .. p + 31
//     = 8 consecutive rows x 4 blocks: block c lands at bank 16 (c + (t >> 3)) + 2 (t & 7) + (0, 1) mod 64 (576 bytes = 144 banks = 16 mod 64:
//     that is what the 8 rows of padding are for; unpadded the four blocks would meet in the same 16 banks, 4-way), so the
//     half covers the 64 banks once: conflict free.
//   * A operand of instruction s (k = k0 + 64 s .. + 63): slot 2 s + h of row 32 b + r: one ds_read_b128.  Scale bytes lie in
//     LDS as [h][row][s], so one 16-bit read per fragment and stage gives the lane both, byte s selected by op_sel.
//   * B operand, shared by the wave's two n blocks: e4m3 slots 4 s + h and 4 s + 2 + h of row t, two ds_read_b128; MXFP4 slot
//     2 s + h of row t, one, with the row's scale bytes read like the weights'; MXFP6 the three words of block 2 s + h of row
//     t, three ds_read_b64, the scale bytes as with MXFP4 rows.
//   * The loads of a stage are issued TWO stages ahead of their use, into two register sets that alternate.
//   * FIXED ORDER.  Stages in ascending k, instruction 0 then 1 inside a stage, one accumulator per output.  A row's
//     result depends on its own bytes, its scales and its expert's weights only: the grouped call equals E one-expert calls
//     bit for bit.  No atomics, every element is written once; with a table one more z-slice zeroes the rows no expert
//     covers (mx4_group_begin).
//   * EPILOGUE, float32 (mx4_scaled_epilogue).  e4m3 rows: v = act_scale[t] * acc (one multiplication; act_scale == NULL:
//     v = acc), with a bias v = fma(act_scale[t], acc, bias[e][n]) (one rounding); a NaN act_scale makes the whole row NaN
//     (NaN * 0 is NaN).  MXFP4 and MXFP6 rows: v = acc, with a bias v = acc + bias[e][n] (one addition).  Then the one rounding to
//     out's type (store_out4).
#pragma once
#include "fql_mx4_common.h"

struct Mx4ScaledCfg {
    static constexpr int BT = 64, BN = 128, BK = 128;  // rows, columns and contraction depth of a stage
    static constexpr int THREADS = 256;
};

// The epilogue of one 32-n block (columns nb0 .. nb0 + 31) of the lane's row t, shared by mx4_scaled_kernel and its decode
// form: registers 4q .. 4q+3 of acc are n = nb0 + 8 q + 4 h + (0 .. 3).  as: act_scale[t], or 1 without one (ROWS 1 only).
template <int ROWS, int OUT>
__device__ __forceinline__ void mx4_scaled_epilogue(const v16f &acc, void *__restrict__ out, int t, int N, int nb0, int h, bool vec,
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
            if constexpr (ROWS == 1) {
                if (brow != nullptr && nc + c < N) v[c] = __fmaf_rn(as, a, brow[nc + c]);
                else v[c] = act_scale == nullptr ? a : __fmul_rn(as, a);
            } else {
                v[c] = a;
                if (brow != nullptr && nc + c < N) v[c] = __fadd_rn(v[c], brow[nc + c]);
            }
        }
        store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
    }
}

// ROWS: 1 e4m3 rows x [T][K] (xscales unused), 2 MXFP4 rows x [T][K / 2], 3 MXFP6 rows x [T][3 K / 4] (act_scale unused);
// OUT: element type of out, rounded once in the epilogue.
template <int ROWS, int OUT>
__global__ __launch_bounds__(256) void mx4_scaled_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const uint8_t *__restrict__ x,
    const uint8_t *__restrict__ xscales, const float *__restrict__ act_scale, const float *__restrict__ bias,
    void *__restrict__ out, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4ScaledCfg;
    constexpr int XS = ROWS == 1 ? 8 : 4;                          // 16-byte slots of an activation row of a stage (ROWS 1, 2)
    constexpr int XP = C::BT + 8;                                  // rows of a plane of the MXFP6 image, padded by 64 bytes
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    __shared__ __attribute__((aligned(16))) uint4 wimg[2][C::BN][4];   // packed weight rows, 128 k = 64 bytes, slots swizzled
    __shared__ __attribute__((aligned(16))) uint4 ximg[2][C::BT][XS];  // activation rows as loaded, slots swizzled
    __shared__ __attribute__((aligned(4))) uint8_t simg[2][2][C::BN][2];   // E8M0 bytes: [h][n][s] = block 2 s + h of the stage (read in pairs)
    __shared__ __attribute__((aligned(4))) uint8_t ximgs[2][2][C::BT][2];  // MXFP4 / MXFP6 rows only (never referenced otherwise): theirs, [h][t][s]
    __shared__ __attribute__((aligned(8))) uint2 ximg6[2][3][4][XP];       // MXFP6 rows only: word j of block c of row t at [j][c][t]

    const int e = blockIdx.z;
    const int n0 = (int)blockIdx.x * C::BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nb = (wave & 1) * 2;                                 // first of this wave's two 32-n blocks
    const int tr = (wave >> 1) * 32 + r;                           // this lane's row inside the tile
    const bool row_ok = t_blk + tr < cnt;
    const int t = row_lo + t_blk + tr;
    const int K2 = K >> 1, KB = K >> 5;

    // staging roles of this thread: weight pieces (row sn + 64 i, block sc of the stage); e4m3 pieces (row xr + 32 i of the
    // tile, slot xq) or the MXFP4 piece (row sn of the tile, block sc).  Rows are clamped into the expert's range.
    const int sn = tid >> 2, sc = tid & 3, xr = tid >> 3, xq = tid & 7;
    const uint8_t *wbase[2], *sbase[2], *xbase[ROWS == 1 ? 2 : 1], *xsbase = nullptr;
    const int K34 = 3 * (K >> 2);                                  // bytes of an MXFP6 row
    bool n_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        n_ok[i] = n0 + sn + 64 * i < N;
        const size_t wrow = (size_t)e * N + (n_ok[i] ? n0 + sn + 64 * i : 0);
        wbase[i] = blocks + wrow * K2 + 16 * sc;
        sbase[i] = scales + wrow * KB + sc;
        if constexpr (ROWS == 1) {
            const int tx = row_lo + (t_blk + xr + 32 * i < cnt ? t_blk + xr + 32 * i : cnt - 1);
            xbase[i] = x + (size_t)tx * K + 16 * xq;
        }
    }
    if constexpr (ROWS == 2) {
        const size_t tx = (size_t)(row_lo + (t_blk + sn < cnt ? t_blk + sn : cnt - 1));
        xbase[0] = x + tx * K2 + 16 * sc;
        xsbase = xscales + tx * KB + sc;
    }
    if constexpr (ROWS == 3) {
        const size_t tx = (size_t)(row_lo + (t_blk + sn < cnt ? t_blk + sn : cnt - 1));
        xbase[0] = x + tx * K34 + 24 * sc;
        xsbase = xscales + tx * KB + sc;
    }
    const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0; // (e4m3 rows; K % 32 == 0: every row starts on a 16-byte boundary then)

    struct Stage {                                                 // what a thread holds of one stage between load and use
        uint4 w[2], x[ROWS == 1 ? 2 : 1];
        uint2 x6[3];                                               // (MXFP6 rows only: the three 8-byte words of the block)
        int s[2], xs;                                              // (xs: MXFP4 / MXFP6 rows only)
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
            if constexpr (ROWS == 1) {
                st.x[i] = make_uint4(0u, 0u, 0u, 0u);
                if (k0 + 16 * xq < K) {
                    const uint8_t *p = xbase[i] + k0;
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
        }
        st.xs = 127;
        if constexpr (ROWS == 2) {
            st.x[0] = make_uint4(0u, 0u, 0u, 0u);
            if (k_ok) {
                st.x[0] = *reinterpret_cast<const uint4 *>(xbase[0] + (k0 >> 1));
                st.xs = xsbase[k0 >> 5];
            }
        }
        if constexpr (ROWS == 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) st.x6[j] = make_uint2(0u, 0u);
            if (k_ok) {
                const uint2 *p = reinterpret_cast<const uint2 *>(xbase[0] + 3 * (k0 >> 2));
#pragma unroll
                for (int j = 0; j < 3; ++j) st.x6[j] = p[j];
                st.xs = xsbase[k0 >> 5];
            }
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> LDS, bytes as loaded
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = sn + 64 * i, tt = xr + 32 * i;
            wimg[buf][n][sc ^ ((n >> 2) & 3)] = st.w[i];
            simg[buf][sc & 1][n][sc >> 1] = (uint8_t)st.s[i];
            if constexpr (ROWS == 1) ximg[buf][tt][xq ^ ((tt >> 1) & 7)] = st.x[i];
        }
        if constexpr (ROWS == 2) {
            ximg[buf][sn][sc ^ ((sn >> 2) & 3)] = st.x[0];
            ximgs[buf][sc & 1][sn][sc >> 1] = (uint8_t)st.xs;
        }
        if constexpr (ROWS == 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) ximg6[buf][j][sc][sn] = st.x6[j];
            ximgs[buf][sc & 1][sn][sc >> 1] = (uint8_t)st.xs;
        }
    };

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    // instruction S of the stage in buffer `buf`: k = k0 + 64 S .. + 63; sw / sx: the stage's scale bytes of the lane's two
    // weight rows / of its MXFP4 row
    auto step = [&](auto S, int buf, const int (&sw)[2], int sx) {
        constexpr int s = decltype(S)::value;
        v8i bv;
        if constexpr (ROWS == 1) {
            const int xsw = (tr >> 1) & 7;
            const uint4 x0 = ximg[buf][tr][(4 * s + h) ^ xsw], x1 = ximg[buf][tr][(4 * s + 2 + h) ^ xsw];
            bv = v8i{(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w, (int)x1.x, (int)x1.y, (int)x1.z, (int)x1.w};
        } else if constexpr (ROWS == 2) {
            const uint4 x0 = ximg[buf][tr][(2 * s + h) ^ ((tr >> 2) & 3)];
            bv = v8i{(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w, 0, 0, 0, 0};
        } else {
            const uint2 x0 = ximg6[buf][0][2 * s + h][tr], x1 = ximg6[buf][1][2 * s + h][tr], x2 = ximg6[buf][2][2 * s + h][tr];
            bv = v8i{(int)x0.x, (int)x0.y, (int)x1.x, (int)x1.y, (int)x2.x, (int)x2.y, 0, 0};
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = 32 * (nb + b) + r;
            const uint4 a = wimg[buf][n][(2 * s + h) ^ ((n >> 2) & 3)];
            const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
            if constexpr (ROWS == 1) acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[b], 4, 0, s, sw[b], 0, 0x7F7F7F7F);
            else if constexpr (ROWS == 2) acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[b], 4, 4, s, sw[b], s, sx);
            else acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[b], 4, 2, s, sw[b], s, sx);
        }
    };

    // Stage i: refill `mine` (consumed one stage ago) with the loads of stage i + 2, contract the images of stage i, then
    // turn `other` (stage i + 1, loaded one stage ago) into the other set of images.  Two stages of loads are in flight.
    auto run_stage = [&](Stage &mine, const Stage &other, int k0, int it) {
        if (k0 + 2 * C::BK < K) load_stage(mine, k0 + 2 * C::BK);
        const int buf = it & 1;
        int sw[2], sx = 0;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            sw[b] = *reinterpret_cast<const unsigned short *>(&simg[buf][h][32 * (nb + b) + r][0]);
        if constexpr (ROWS != 1) sx = *reinterpret_cast<const unsigned short *>(&ximgs[buf][h][tr][0]);
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
    const float as = ROWS != 1 || act_scale == nullptr ? 1.0f : act_scale[t];
#pragma unroll
    for (int b = 0; b < 2; ++b) mx4_scaled_epilogue<ROWS, OUT>(acc[b], out, t, N, n0 + 32 * (nb + b), h, vec, brow, act_scale, as);
#endif
}
