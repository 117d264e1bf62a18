// Input gradient of the grouped GEMM on NVFP4 expert weights (include/fql_int4.h, fql_moe_nvfp4_bwd_input):
//
//   dX[t][k] = round_OUT( fl32(acc * global_scale[e]) ),   acc = sum_n bf16(dY[t][n]) * W_e[n][k]   over the rows t of expert e,
//   W_e[n][k] = e2m1(code[e][n][k]) * e4m3(s[e][n][k / 16])                                          as in fql_gemm_nvfp4.h
//
// The operands are the forward's blocks [E][N][K / 2], scales [E][N][K / 16] and global_scale [E] (or NULL: 1, and the result
// is acc's bits); no transposed weight copy.  The weights are exact in bfloat16 (fql_gemm_nvfp4.h), the gradient rows are
// rounded once to bfloat16 unless they already are, the contraction is v_mfma_f32_32x32x16_bf16 in ascending n.
//
// nv4_bwd_kernel: mx4_bwd_kernel's skeleton (fql_gemm_mx4_bwd.h: the 64 t x 128 k tile of 4 waves, the 64-n stage, the
// swizzled [64 n][128 k] image through mx4_bwd_off with the rotated store order, the two ds_read_b64_tr_b16 per operand, the
// [64 t][64 n + 8] gradient image, loads two stages ahead, one barrier a stage) with nv4_kernel's staging.  It lives in a
// file of its own so that mx4_bwd_kernel stays the instructions it was.  What differs from mx4_bwd_kernel:
//   * SCALE BYTES.  A staging thread's 16-byte piece is 32 k = TWO scale blocks.  It loads the two adjacent scale bytes as two
//     byte loads (no alignment is asked of `scales`) under the piece's own guard k_ok && n < N; kp + 31 < K there, so
//     (kp >> 4) + 1 <= K / 16 - 1: both bytes lie inside the row.  Absent pieces are zero codes under the byte 0x38 (1.0).
//   * CONVERSION.  Dword i of the piece (k = kp + 8 i .. + 7) converts under byte i >> 1.  The store rotation permutes the
//     dwords (store j takes dword j ^ wrot), so each dword's scale travels with it: the scales are rotated by the same two
//     swaps as the dwords, never selected by the store index.
//   * EPILOGUE.  global_scale[e] is read once per workgroup; one float32 multiply, then the one rounding to OUT.
//   * EXEC.  As mx4_bwd_kernel: every exit before the loop and the loop's trip count are uniform per workgroup, tiles are
//     padded with zeros, never masked; no per-lane return before the epilogue.
//   * NON-FINITE.  The row flag as mx4_bwd_kernel's.  A NaN scale byte (0x7F, 0xFF) makes its 16 weights NaN (nv4_scale),
//     hence dX NaN for exactly those 16 k on the rows of that expert; a negative byte negates its block.  global_scale is
//     not screened.
//   * LORA (nv4_bwd_kernel<IN, OUT, Mx4Lora>; fql_moe_nvfp4_lora_bwd_input / fql_linear_nvfp4_lora_bwd_input, DESIGN.md section
//     41): mx4_bwd_kernel's adapter stage behind the last weight stage,
//       dX[t][k] = round_OUT( S' ),   S' = fl32(acc * global_scale[e]) (+) sum_{j < r} bf16(dv[t][j]) bf16(A[e][j][k]).
//     The global scale scales the weight term only: the LORA form multiplies the accumulator registers by it behind the last
//     weight stage (one __fmul_rn each, never an FMA) and the epilogue multiplies no more.  The stage writes pair 0 of the
//     images in full, through the same mx4_bwd_off and store rotation; a uniform trip count, no per-lane exit, EXEC all
//     ones at every transposed read.  nv4_bwd_kernel<IN, OUT> is the code it was.
#pragma once
#include "fql_gemm_mx4_bwd.h"
#include "fql_gemm_nvfp4.h"

// IN: element type of dY (FQL_DTYPE_F32 or FQL_DTYPE_BF16); OUT: element type of dX, rounded once in the epilogue.
// LA: nothing (nv4_bwd_kernel<IN, OUT>: the signature, the code and the bits it always had), or Mx4Lora: the LORA flag.
template <int IN, int OUT, class... LA>
__global__ __launch_bounds__(256) void nv4_bwd_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const float *__restrict__ gscale,
    const void *__restrict__ dy, void *__restrict__ dx, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
    int E, int T, int K, int N, LA... lora)
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
    const int K2 = K >> 1, KS = K >> 4;
    constexpr int es = IN == 0 ? 4 : 2;
    const bool has_gs = gscale != nullptr;
    const float gs = has_gs ? gscale[e] : 1.0f;                    // (uniform: once per workgroup)

    // staging roles of this thread.  Weights: row sn of the stage, 16-byte piece sp (32 k = two scale blocks).  Gradients:
    // row ys of the tile (clamped into the expert's range: loads are unconditional), the 16 n of quarter yq.
    const int sn = tid >> 2, sp = tid & 3;
    const int kp = kbase + 32 * sp;
    const bool k_ok = kp < K;                                      // (K % 32 == 0: kp + 31 < K then)
    const uint8_t *wbase = blocks + (size_t)e * N * K2 + (kp >> 1);
    const uint8_t *sbase = scales + (size_t)e * N * KS + (kp >> 4);
    const int ys = tid >> 2, yq = tid & 3;
    const int ty = row_lo + (t_blk + ys < cnt ? t_blk + ys : cnt - 1);
    const char *yrow = reinterpret_cast<const char *>(dy) + (size_t)ty * N * es;
    // (16-byte loads: every row starts on a 16-byte boundary and ends on a piece boundary)
    const bool vec_y = (reinterpret_cast<uintptr_t>(dy) & 15) == 0 && ((size_t)N * es) % 16 == 0;

    const int wrot = (sp >> 1) | ((sn & 1) << 1);                  // this thread's order of its four 16-byte stores
    int w_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w_off[j] = mx4_bwd_off(sn, 4 * sp + (j ^ wrot));

    // What a thread holds of one stage between its loads and their use: its packed piece with the two scale bytes (byte 0:
    // dwords 0-1, byte 1: dwords 2-3) and its 16 gradients as loaded.
    struct Stage {
        uint4 wq;
        uint32_t sc;
        typename std::conditional<IN == 0, float, uint32_t>::type y[IN == 0 ? 16 : 8];
    };
    auto load_stage = [&](Stage &st, int n0) {
        const int nw = n0 + sn;                                    // packed piece + its two scale bytes
        st.wq = make_uint4(0u, 0u, 0u, 0u);
        st.sc = 0x3838u;
        if (k_ok && nw < N) {                                      // (both bytes lie inside the row's K / 16)
            const uint8_t *sb = sbase + (size_t)nw * KS;
            st.wq = *reinterpret_cast<const uint4 *>(wbase + (size_t)nw * K2);
            st.sc = (uint32_t)sb[0] | ((uint32_t)sb[1] << 8);
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
        // Dword i of the piece is k = kp + 8 i .. + 7: chunk 4 sp + i, scale byte i >> 1.  Store j takes dword j ^ wrot
        // (mx4_bwd_kernel's rotation); the scales go through the same two swaps, so sv[j] is the scale of words[j].
        uint32_t words[4] = {st.wq.x, st.wq.y, st.wq.z, st.wq.w};
        const float s01 = nv4_scale<0>(st.sc), s23 = nv4_scale<1>(st.sc);
        float sv[4] = {s01, s01, s23, s23};
        if (wrot & 1) { const uint32_t a = words[0], b = words[2]; words[0] = words[1]; words[1] = a; words[2] = words[3]; words[3] = b; }
        if (wrot & 2) {
            const uint32_t a = words[0], b = words[1]; words[0] = words[2]; words[2] = a; words[1] = words[3]; words[3] = b;
            const float fa = sv[0], fb = sv[1]; sv[0] = sv[2]; sv[2] = fa; sv[1] = sv[3]; sv[3] = fb;
        }                                                          // (the swap of wrot & 1 stays inside a scale block)
#pragma unroll
        for (int j = 0; j < 4; ++j)                                // (words[j] is dword j ^ wrot now, sv[j] its block's scale)
            *reinterpret_cast<uint4 *>(&image[buf][w_off[j]]) = nv4_dequant8(words[j], sv[j]);
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

    // Transposed-read addresses of this lane, step 0 (mx4_bwd_kernel's): block b, half j of the operand.
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
        // global_scale belongs to the weights alone: the finished weight sum is multiplied here, one rounding a register
        // and never an FMA, the adapter steps accumulate onto the scaled value and the epilogue multiplies no more.
        if (has_gs) {
#pragma clang fp contract(off)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[b][q] = __fmul_rn(acc[b][q], gs);
        }
        // The adapter stage (mx4_bwd_kernel's).  Every thread is behind the last stage's barrier, which no store followed:
        // pair 0 of the images is free.  It is written in full, zeros from row `rank` on, past K and from column `rank` of
        // dv on, so nothing of a weight stage, a NaN block included, meets a zero; then one barrier, then the steps.  Every
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
            for (int c = 0; c < 4; ++c) {
                v[c] = acc[b][4 * q + c];
                if (!LORA && has_gs) v[c] = __fmul_rn(v[c], gs);
                if (row_nan) v[c] = __uint_as_float(0x7FC00000u);
            }
            store_out4(dx, OUT, (size_t)t * K, kc, K, vec, v);
        }
#endif
}
