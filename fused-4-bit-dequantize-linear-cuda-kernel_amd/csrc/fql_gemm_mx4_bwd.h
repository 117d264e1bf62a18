// Input gradient of the grouped GEMM on OCP MXFP4 expert weights (include/fql_int4.h, fql_moe_mx4_bwd_input):
//
//   dX[t][k] = sum_n bf16(dY[t][n]) * W_e[n][k]   over the rows t of expert e,   W_e as in fql_gemm_mx4.h
//
// The operands are the forward's blocks [E][N][K / 2] and scales [E][N][K / 32]; the contraction now runs over the weight
// ROWS n, so the packed pieces arrive as [n][32 k] while the matrix core wants 8 consecutive n for one k.  The weights are
// exact in bfloat16, the gradient rows are rounded once to bfloat16 (to nearest even) unless they already are, and the
// contraction is v_mfma_f32_32x32x16_bf16 with float32 accumulation, as in the forward.
//
// mx4_bwd_kernel: group_bwd_kernel's tiling (fql_group_bwd.h) with mx4_kernel's staging.  Workgroup = 4 waves = a tile of
// 64 rows t x 128 columns k of one expert (blockIdx.z).  The weights are the A operand (rows = k), the gradient rows the
// B operand (columns = t): a lane owns one output row t, registers 4q .. 4q+3 of an accumulator are 4 consecutive k
// (16-byte stores, store_out4).  Wave w takes the 32 rows (w >> 1) and the two 32-k blocks 2 (w & 1), 2 (w & 1) + 1.
//   * Weight stage = 64 n x 128 k.  Thread p reads ONE 16-byte piece of a packed row (row n0 + (p >> 2), the 32 k of piece
//     p & 3: one scale block, one scale byte), converts its 32 codes to bfloat16 and writes them as 4 x 16 bytes into the
//     LDS image [64 n][128 k] of bfloat16: plain 256-byte rows, double buffered (2 x 16 KiB).  The 16-byte chunk ch of row
//     n sits at chunk ch ^ (((n & 3) << 2) | ((n >> 2) & 3)) of its row (mx4_bwd_off).  Pieces past N or K are zeros.
//     A thread issues its four stores in the order (sp >> 1) | ((row & 1) << 1) XOR 0 .. 3, which spreads the 8 lanes of a
//     ds_write_b128 group over the eight 16-byte slots of a 128-byte bank row (natural order: two slots, 4-way).
//   * A operand, the transpose: lane (r = lane & 31, h = lane >> 5) needs W[n0 + 16 s + 8 h + (0 .. 7)][32 b + r] for step
//     s of block b: two ds_read_b64_tr_b16.  Each 16-lane group (g = (lane >> 4) & 1) of such a read takes the block of 4
//     rows 16 s + 8 h + 4 j .. + 3 (j = 0 | 1 for the low | high half of the operand) by the 16 columns 32 b + 16 g .. + 15;
//     lane 4 q + p of the group supplies the address of row q, elements 4 p .. 4 p + 3 of the 16 (chunk 4 b + 2 g + (p >> 1),
//     byte 8 (p & 1) in it) and lane i receives column i.  BANKS: a 32-lane half reads 4 rows x 4 chunks; the rows are 256
//     bytes apart (one bank row), so unswizzled they would hit the same 16 banks 4 ways.  With the swizzle chunk 4 b + c of
//     row q lands on chunk 4 (b ^ q) + (c ^ (2 h + j)): 16 distinct chunks = all 64 banks once.  Conflict-free.
//     The read needs EXEC all ones: every exit before the loop is uniform per workgroup and the loop's trip count is too.
//   * Gradient stage = 64 t x 64 n.  Thread p reads the 16 n of quarter p & 3 of row p >> 2 (16-byte loads when the rows are
//     16-byte aligned and N is a whole number of 16-byte pieces, element loads otherwise), rounds float32 to bfloat16 and
//     writes the second image [64 t][64 n + 8], double buffered (2 x 9 KiB).  Elements past N are zeros.
//   * B operand: the lane reads yimage[t_r][16 s + 8 h .. + 7]: one ds_read_b128, shared by its two k blocks.
//   * The loads of a stage are issued TWO stages ahead of their use, into two register sets that alternate.
//   * FIXED ORDER.  Stage n0 = 0, 64, ...; inside a stage step s = 0 .. 3 contracts n0 + 16 s .. + 15 with one instruction.
//     A row's result depends on its own gradient row and its expert's weights only: not on T, E, the table, its tile
//     neighbours or the run.  No atomics, every element is written once; with a table one more z-slice zeroes the rows no
//     expert covers (act_zero_uncovered).
//   * NON-FINITE.  A non-finite element of a gradient row makes that whole dX row NaN (the forward's exponent-field flag
//     in LDS).  A scale code 255 makes the 32 weights of its block NaN, hence dX NaN for those 32 k on the rows of that
//     expert: this falls out of the arithmetic.
//   * LORA (mx4_bwd_kernel<IN, OUT, Mx4Lora>; fql_moe_mx4_lora_bwd_input): the adapter's share of the gradient as
//     one more contraction stage behind the last weight stage,
//       dX[t][k] = sum_n bf16(dY[t][n]) W_e[n][k] + sum_{j < r} bf16(dv[t][j]) bf16(A[e][j][k]),
//     dv [T][r] float32 (the caller's s dY B), A [E][r][K] float32, r in {4, 8, 16, 32, 64}.  A's rows have the arrival
//     order [n][k] of the packed pieces: thread (sn, sp) packs A[e][sn][kbase + 32 sp .. + 31] (zeros from row r on and
//     past K) into the swizzled image through the same mx4_bwd_off and store rotation, and dv goes into yimage as dY
//     does, zeros from column r on, with the same exponent-field flag (a non-finite dv[t][j] makes the dX row NaN; A is
//     not screened).  Steps s with 16 s < r: a uniform trip count, no per-lane exit, EXEC all ones at every transposed
//     read.  No LDS beyond the two images; the kernel without the flag is the code it was.
#pragma once
#include "fql_gemm_mx4.h"

struct Mx4BwdCfg {
    static constexpr int BT = Mx4Cfg::BT, BK = 128, BN = 64;   // rows, output columns k and contraction depth n of a stage
    static constexpr int YPITCH = BN + 8;                      // bfloat16 elements of a gradient image row (144 bytes)
    static constexpr int THREADS = Mx4Cfg::THREADS;
};

typedef short mx4_v4s __attribute__((ext_vector_type(4)));

// byte offset of 16-byte chunk ch (0 .. 15) of row `row` in the [64][128] bfloat16 image
__device__ __forceinline__ int mx4_bwd_off(int row, int ch)
{
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// ds_read_b64_tr_b16 at LDS address p (8-byte aligned; EXEC must be all ones)
__device__ __forceinline__ mx4_v4s mx4_tr_read(const unsigned char *p)
{
    typedef __attribute__((address_space(3))) mx4_v4s *lds_v4s;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)p);
}

// IN: element type of dY (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of dX, rounded once in the epilogue.
// LA: nothing (mx4_bwd_kernel<IN, OUT>: the signature, the code and the bits it always had), or Mx4Lora: the LORA flag.
template <int IN, int OUT, class... LA>
__global__ __launch_bounds__(256) void mx4_bwd_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ dy,
    void *__restrict__ dx, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, int T, int K, int N,
    LA... lora)
{
    static_assert(sizeof...(LA) == 0 || (sizeof...(LA) == 1 && (std::is_same<LA, Mx4Lora>::value && ...)), "LA: nothing or Mx4Lora");
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool LORA = sizeof...(LA) == 1;
    using C = Mx4BwdCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(dx, K, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    __shared__ __attribute__((aligned(16))) unsigned char image[2][C::BN * C::BK * 2];     // weights, bfloat16, swizzled
    __shared__ __attribute__((aligned(16))) unsigned short yimage[2][C::BT][C::YPITCH];    // gradient rows, bfloat16
    __shared__ int row_bad[C::BT];                                 // != 0: the row holds a non-finite gradient

    const int e = blockIdx.z;
    const int kbase = (int)blockIdx.x * C::BK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int kb = (wave & 1) * 2;                                 // first of this wave's two 32-k blocks
    const int tr = (wave >> 1) * 32 + r;                           // this lane's row inside the tile
    const bool row_ok = t_blk + tr < cnt;
    const int t = row_lo + t_blk + tr;
    const int K2 = K >> 1, KB = K >> 5;
    constexpr int es = IN == 0 ? 4 : 2;

    // staging roles of this thread.  Weights: row sn of the stage, 16-byte piece sp (32 k = one scale block).  Gradients:
    // row ys of the tile (clamped into the expert's range: loads are unconditional), the 16 n of quarter yq.
    const int sn = tid >> 2, sp = tid & 3;
    const int kp = kbase + 32 * sp;
    const bool k_ok = kp < K;
    const uint8_t *wbase = blocks + (size_t)e * N * K2 + (kp >> 1);
    const uint8_t *sbase = scales + (size_t)e * N * KB + (kp >> 5);
    const int ys = tid >> 2, yq = tid & 3;
    const int ty = row_lo + (t_blk + ys < cnt ? t_blk + ys : cnt - 1);
    const char *yrow = reinterpret_cast<const char *>(dy) + (size_t)ty * N * es;
    // (16-byte loads: every row starts on a 16-byte boundary and ends on a piece boundary)
    const bool vec_y = (reinterpret_cast<uintptr_t>(dy) & 15) == 0 && ((size_t)N * es) % 16 == 0;

    const int wrot = (sp >> 1) | ((sn & 1) << 1);                  // this thread's order of its four 16-byte stores
    int w_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w_off[j] = mx4_bwd_off(sn, 4 * sp + (j ^ wrot));

    struct Stage {
        uint4 wq;
        int sc;
        typename std::conditional<IN == 0, float, uint32_t>::type y[IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int n0) {
        const int nw = n0 + sn;                                    // packed piece + its scale byte
        st.wq = make_uint4(0u, 0u, 0u, 0u);
        st.sc = 127;
        if (k_ok && nw < N) {
            st.wq = *reinterpret_cast<const uint4 *>(wbase + (size_t)nw * K2);
            st.sc = sbase[(size_t)nw * KB];
        }
        const int n = n0 + 16 * yq;                                // dY[ty][n .. n + 15]; zeros past N
        constexpr int NY = IN == 0 ? 16 : 8;
#pragma unroll
        for (int i = 0; i < NY; ++i) st.y[i] = 0;
        if (vec_y) {
#pragma unroll
            for (int i = 0; i < NY / 4; ++i) {
                if constexpr (IN == 0) {
                    if (n + 4 * i < N) {                           // (N % 4 == 0: a piece is inside or outside as a whole)
                        const v4f v = *reinterpret_cast<const v4f *>(yrow + (size_t)n * 4 + 16 * i);
#pragma unroll
                        for (int c = 0; c < 4; ++c) st.y[4 * i + c] = v[c];
                    }
                } else {
                    if (n + 8 * i < N) {                           // (N % 8 == 0)
                        const uint4 v = *reinterpret_cast<const uint4 *>(yrow + (size_t)n * 2 + 16 * i);
                        st.y[4 * i] = v.x; st.y[4 * i + 1] = v.y; st.y[4 * i + 2] = v.z; st.y[4 * i + 3] = v.w;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NY; ++i) {
                if constexpr (IN == 0) {
                    if (n + i < N) st.y[i] = reinterpret_cast<const float *>(yrow)[n + i];
                } else {
                    const unsigned short *p = reinterpret_cast<const unsigned short *>(yrow) + n + 2 * i;
                    uint32_t w = 0u;
                    if (n + 2 * i < N) w = p[0];
                    if (n + 2 * i + 1 < N) w |= (uint32_t)p[1] << 16;
                    st.y[i] = w;
                }
            }
        }
    };
    auto store_stage = [&](const Stage &st, int buf) {             // registers -> the two LDS images (bfloat16)
        // Dword i of the piece is k = kp + 8 i .. + 7: chunk 4 sp + i.  Store j of a thread takes dword j ^ wrot, not j: the
        // 8 lanes of a ds_write_b128 group are two rows x four pieces, and in natural order they would land on two of the
        // eight 16-byte slots of a 128-byte bank row (4-way); with the rotation they cover all eight.
        uint32_t words[4] = {st.wq.x, st.wq.y, st.wq.z, st.wq.w};
        if (wrot & 1) { const uint32_t a = words[0], b = words[2]; words[0] = words[1]; words[1] = a; words[2] = words[3]; words[3] = b; }
        if (wrot & 2) { const uint32_t a = words[0], b = words[1]; words[0] = words[2]; words[2] = a; words[1] = words[3]; words[3] = b; }
#pragma unroll
        for (int j = 0; j < 4; ++j)                                // (words[j] is dword j ^ wrot now)
            *reinterpret_cast<uint4 *>(&image[buf][w_off[j]]) = mx4_dequant8(words[j], st.sc);
        uint32_t yw[8], bad = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (IN == 0) yw[i] = mx4_pack_bf16(st.y[2 * i], st.y[2 * i + 1]);
            else yw[i] = st.y[i];
            bad |= mx4_nonfinite2(yw[i]);
        }
        *reinterpret_cast<uint4 *>(&yimage[buf][ys][16 * yq]) = make_uint4(yw[0], yw[1], yw[2], yw[3]);
        *reinterpret_cast<uint4 *>(&yimage[buf][ys][16 * yq + 8]) = make_uint4(yw[4], yw[5], yw[6], yw[7]);
        if (bad & 0x80008000u) row_bad[ys] = 1;                    // an exponent field of 255 (every writer writes 1)
    };

    // Transposed-read addresses of this lane, step 0: block b, half j of the operand (rows 8 h + 4 j + q).  Step s adds
    // 16 rows = 4096 bytes: the swizzle depends on the row through (row & 3) and ((row >> 2) & 3) only, and 16 s changes
    // neither.
    const int tg = (lane >> 4) & 1, tq = (lane >> 2) & 3, tp = lane & 3;
    int a_off[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            a_off[b][j] = mx4_bwd_off(8 * h + 4 * j + tq, 4 * (kb + b) + 2 * tg + (tp >> 1)) + 8 * (tp & 1);

    v16f acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;

    // Stage i: refill `mine` (consumed one stage ago) with the loads of stage i + 2, contract the images of stage i, then
    // turn `other` (stage i + 1, loaded one stage ago) into the other pair of images.  Two stages of loads are in flight.
    auto run_stage = [&](Stage &mine, const Stage &other, int n0, int it) {
        if (n0 + 2 * C::BN < N) load_stage(mine, n0 + 2 * C::BN);
        const unsigned char *cur = image[it & 1];
        const unsigned short(*ycur)[C::YPITCH] = yimage[it & 1];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 yb = *reinterpret_cast<const uint4 *>(&ycur[tr][16 * s + 8 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const mx4_v4s lo = mx4_tr_read(cur + a_off[b][0] + 4096 * s);
                const mx4_v4s hi = mx4_tr_read(cur + a_off[b][1] + 4096 * s);
                const v8bf a = __builtin_bit_cast(v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(v8bf, yb), acc[b], 0, 0, 0);
            }
        }
        if (n0 + C::BN < N) store_stage(other, (it + 1) & 1);      // (last read one stage ago, behind that stage's barrier)
        __syncthreads();
    };

    if (tid < C::BT) row_bad[tid] = 0;
    __syncthreads();
    Stage s0, s1;
    load_stage(s0, 0);
    s1 = s0;                                                       // (N <= 64: never read)
    if (C::BN < N) load_stage(s1, C::BN);
    store_stage(s0, 0);
    __syncthreads();
    for (int n0 = 0, it = 0; n0 < N; n0 += 2 * C::BN, it += 2) {
        run_stage(s0, s1, n0, it);
        if (n0 + C::BN < N) run_stage(s1, s0, n0 + C::BN, it + 1);
    }

    if constexpr (LORA) {
        // The adapter stage.  Every thread is behind the last stage's barrier (or, N == 0, the one before the loop), which
        // no store followed: pair 0 of the images is free (N == 0: it holds zeros, written again here).  It is written in
        // full, zeros from row `rank` on, past K and from column `rank` of dv on; then one barrier, then the steps.  Every
        // condition around a transposed read is uniform.
        const Mx4Lora la{lora...};
        const int rank = la.rank;
        const float *vrow = la.rows + (size_t)ty * rank;
        const bool a_ok = k_ok && sn < rank;
        const float *arow = la.w + ((size_t)e * rank + (a_ok ? sn : 0)) * K + (a_ok ? kp : 0);
        const bool vec_v = (reinterpret_cast<uintptr_t>(la.rows) & 15) == 0, vec_a = (reinterpret_cast<uintptr_t>(la.w) & 15) == 0;
        uint32_t yw[8], bad = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                              // dv[ty][16 yq + 4 i .. + 3]
            const int j = 16 * yq + 4 * i;
            mx4_lora_pack4(vrow + j, vec_v, j < rank, yw[2 * i], yw[2 * i + 1]);
            bad |= mx4_nonfinite2(yw[2 * i]) | mx4_nonfinite2(yw[2 * i + 1]);
        }
        *reinterpret_cast<uint4 *>(&yimage[0][ys][16 * yq]) = make_uint4(yw[0], yw[1], yw[2], yw[3]);
        *reinterpret_cast<uint4 *>(&yimage[0][ys][16 * yq + 8]) = make_uint4(yw[4], yw[5], yw[6], yw[7]);
        if (bad & 0x80008000u) row_bad[ys] = 1;                    // (read behind the barrier below)
        uint4 ch[4];                                               // chunk 4 sp + i of image row sn: A[e][sn][kp + 8 i .. + 7]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mx4_lora_pack4(arow + 8 * i, vec_a, a_ok, ch[i].x, ch[i].y);
            mx4_lora_pack4(arow + 8 * i + 4, vec_a, a_ok, ch[i].z, ch[i].w);
        }
        if (wrot & 1) { const uint4 a = ch[0], b = ch[2]; ch[0] = ch[1]; ch[1] = a; ch[2] = ch[3]; ch[3] = b; }
        if (wrot & 2) { const uint4 a = ch[0], b = ch[1]; ch[0] = ch[2]; ch[2] = a; ch[1] = ch[3]; ch[3] = b; }
#pragma unroll
        for (int j = 0; j < 4; ++j)                                // (ch[j] is chunk j ^ wrot now: store_stage's rotation)
            *reinterpret_cast<uint4 *>(&image[0][w_off[j]]) = ch[j];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (16 * s >= rank) break;                             // (uniform)
            const uint4 yb = *reinterpret_cast<const uint4 *>(&yimage[0][tr][16 * s + 8 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const mx4_v4s lo = mx4_tr_read(image[0] + a_off[b][0] + 4096 * s);
                const mx4_v4s hi = mx4_tr_read(image[0] + a_off[b][1] + 4096 * s);
                const v8bf a = __builtin_bit_cast(v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(v8bf, yb), acc[b], 0, 0, 0);
            }
        }
    }

    // D[i][j]: i = k (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are k = 8 q + 4 h + (0 .. 3) of the block.
    // (Every write of row_bad lies behind a barrier.)
    const bool row_nan = row_bad[tr] != 0;
    if (!row_ok) return;
    const bool vec = (reinterpret_cast<uintptr_t>(dx) & (OUT == 0 ? 15 : 7)) == 0;   // (K % 32 == 0)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kc = kbase + 32 * (kb + b) + 8 * q + 4 * h;
            if (kc >= K) continue;
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = row_nan ? __uint_as_float(0x7FC00000u) : acc[b][4 * q + c];
            store_out4(dx, OUT, (size_t)t * K, kc, K, vec, v);
        }
#endif
}
