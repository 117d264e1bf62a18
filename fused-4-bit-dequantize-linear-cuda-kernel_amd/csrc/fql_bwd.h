// Input gradient of the INT4 linear / grouped ops on the CDNA4 matrix cores (v_mfma_i32_32x32x32_i8):
//
//   dX[t][k] = sum_n dY[t][n] * s[e][n] * (q[e][n][k] - zp[e][n])
//
// is the forward's exact-integer scheme with the roles of N and K swapped:
//
//   g[t][n]  = dY[t][n] * s[e][n]                          (float32, one rounding, in the pre-pass)
//   g[t][n] ~= delta[t] * sum_l 256^l a_l[t][n]            (the limb pre-pass of fql_act_quant.h, rows of length N)
//   z[n]     = clamp(rint(zp[n]), -112, 112),  f[n] = zp[n] - z[n]     (f == 0 for every quantize_weights output)
//   dX[t][k] = delta[t] * sum_l 256^l * sum_n a_l[t][n] * (q[n][k] - z[n])  -  sum_n g[t][n] * f[n]
//
// The zero point cannot be folded into a row sum here (it varies along the contraction), so the weight image holds
// q - z[n] itself: int8 in [-112, 127].  Every inner dot product is exact in i32 for N <= 2^31 / (128 * 127) = 132104
// (checked by the entry points), so a row's result does not depend on the tile shape or on the other rows of its tile.
// The float term sum_n g f comes from the pre-pass (act_rows<..., CS = true>), one value per row.
// Heavy-tailed gradient rows get the pre-pass's residual limb set (delta2 = delta + T, limbs + L planes); a tile holding
// such a row runs its contraction a second time on that set and adds delta2 * (...) for those rows only.
//
// Element types: grad_out may be float16 / bfloat16 (loaded as it is by the pre-pass, widened in registers) and grad_in
// may be stored in either (one rounding to nearest even in the GEMM's epilogue); everything in between is the float32
// path, so a 16-bit call is bit for bit the float32 call on the widened gradient, rounded once.
//
// Pre-pass (act_colscale_kernel): act_rows with CS = true: the limbs of g in the fragment-native layout of
// fql_act_quant.h, contraction index n in the place of k.  The limb order (0,2,4,6,1,3,5,7) inside every aligned
// group of 8 n is kept; the weight side follows it through the addresses of the transposed read (below).
//
// GEMM (gemm_bwd_kernel): one 8-wave workgroup per CU walks tiles of 128 rows t x 128 columns k (persistent; m-tile
// major, dealt to XCDs in contiguous ranges as in fql_gemm_i8.h), expert table on the device.  The weights are the
// MFMA's A operand (rows = k), the limbs its B operand (columns = t), so every lane owns one output row t and
// registers 4q..4q+3 of a fragment are 4 consecutive k: 16-byte stores.
//   * Weight stage = 256 n x 128 k: packed bytes (64 per row n) global -> VGPR -> nibbles unpacked to natural k order
//     and z[n] subtracted (SWAR, 4 bytes per op) -> LDS image [n][128 k] of int8, one 128-byte row per n, double
//     buffered (2 x 32 KiB).  The 32-byte chunk c of row n is stored at chunk c ^ ((n >> 1) & 3).
//   * The A operand needs 16 n for one k: a column of that image, read with ds_read_b64_tr_b8.  Per 16-lane group,
//     lane 2q+p gives the address of 8 bytes (columns 8p .. 8p+7 of the group's 16 k) of row q of an 8-row block and
//     lane i receives column i, row q in byte q.  Row q of the block is taken as n = base + (0,2,4,6,1,3,5,7)[q] --
//     the pre-pass's limb order -- so byte j of the operand pairs with byte j of the limbs without moving any data.
//     A 32-lane half reads 8 rows whose n & 7 are all different: with the chunk swizzle the 32 lanes hit 32 different
//     8-byte bank pairs (no conflict).
//   * Activation limbs: one coalesced 1 KiB buffer load per wave, k-step and limb, D k-steps ahead in a register ring.
//   * One workgroup barrier per stage.  No atomics: each dX element is written once.
#pragma once
#include "fql_common.h"
#include "fql_act_quant.h"

#ifndef FQL_BWD_MAX_N
#define FQL_BWD_MAX_N 132104        // 2^31 / (128 * 127): i32 accumulation exact (include/fql_int4.h)
#endif

// ---- pre-pass: limbs of g = dY * s[e][:] (+ the per-row correction), coverage workgroups zero the rows of grad_in
//      no expert owns
//      IN: element type of gy (FQL_DTYPE_*; 16-bit gradients are widened in registers before the multiply by s, so the
//      limbs are the bits of the float32 call on the widened gradient); gx_es: bytes per element of gx (zero fill only)
template <int L, bool VEC, int AR, int IN = 0>
__global__ __launch_bounds__(256) void act_colscale_kernel(
    const void *__restrict__ gy, float *__restrict__ delta, int32_t *__restrict__ rowsum, int8_t *__restrict__ limbs,
    int T, int N, int KB, int MBT, int rblocks, void *__restrict__ gx, int gx_es, int K, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, const float *__restrict__ scales, const float *__restrict__ zps)
{
    if ((int)blockIdx.x >= rblocks) {
        act_zero_uncovered((int)blockIdx.x - rblocks, gx, gx_es, K, tpe, offs, E, T);
        return;
    }
    act_rows<L, VEC, IN, false, false, AR, false, true>(gy, nullptr, 0, delta, rowsum, limbs, T, N, KB, MBT, rblocks, tpe,
                                                       offs, E, nullptr, (int)blockIdx.x * AR, scales, zps);
}

struct BwdCfg {
    static constexpr int WM = 4, WN = 2, NF = 2;        // 8 waves; wave (wm, wn): 32 rows x NF * 32 columns
    static constexpr int BM = 32 * WM, BN = 32 * NF * WN;
    static constexpr int THREADS = 64 * WM * WN;
    static constexpr int ROWB = BN;                     // bytes per n-row of the LDS image (int8 weights)
    static constexpr int STAGE = FQL_KB * ROWB;         // 32 KiB
    static constexpr int CPT = FQL_KB * (BN / 32) / THREADS;   // 16-byte packed chunks per thread per stage (2)
    static_assert(BN == 128, "the chunk swizzle assumes 4 chunks of 32 bytes per row");
};

// 8 packed bytes (16 k, byte j = q[2j] | q[2j+1] << 4) -> 16 bytes q - z in natural k order; zz = (-z) & 0x7f7f7f7f
// replicated, zh = (-z) & 0x80808080: a per-byte add without carries (q < 16 and 127 + 15 < 256)
__device__ __forceinline__ void bwd_unpack16(uint32_t w0, uint32_t w1, uint32_t zz, uint32_t zh, uint32_t (&o)[4])
{
    const uint32_t lo0 = w0 & 0x0F0F0F0Fu, hi0 = (w0 >> 4) & 0x0F0F0F0Fu;
    const uint32_t lo1 = w1 & 0x0F0F0F0Fu, hi1 = (w1 >> 4) & 0x0F0F0F0Fu;
    o[0] = (__builtin_amdgcn_perm(hi0, lo0, 0x05010400u) + zz) ^ zh;   // k0 k1 k2 k3
    o[1] = (__builtin_amdgcn_perm(hi0, lo0, 0x07030602u) + zz) ^ zh;   // k4 .. k7
    o[2] = (__builtin_amdgcn_perm(hi1, lo1, 0x05010400u) + zz) ^ zh;
    o[3] = (__builtin_amdgcn_perm(hi1, lo1, 0x07030602u) + zz) ^ zh;
}

// VW: K % 32 == 0 and a 16-byte aligned weight base, so every 16-byte chunk of a packed row is one aligned load;
// otherwise the chunk is read byte by byte (odd K / 2: rows are not 4-byte aligned).
// OUT: element type of `out` (FQL_DTYPE_*): the epilogue's store rounds once (store_out4, fql_common.h).
template <int L, bool VW, int OUT = 0>
__global__ __launch_bounds__(512, 2) void gemm_bwd_kernel(
    const int8_t *__restrict__ limbs, const float *__restrict__ delta, const uint8_t *__restrict__ packed,
    const float *__restrict__ zps, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N, int Np, int MBT, int m_slots, int n_tiles)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = BwdCfg;
    constexpr int NF = C::NF, WM = C::WM, KS = FQL_KB / 32;
    // A ring depth in k-steps (the byte-load path of the weights holds 16 more registers per chunk in flight: at 3 limbs
    // it keeps a 2-step ring, which fits the 2-wave-per-SIMD register budget without spilling)
    constexpr int D = (L == 3) ? (VW ? 4 : 2) : 8;
    constexpr bool RES = FQL_RES_ENABLED && L >= 2;
    constexpr int SETS = RES ? 2 : 1;
    constexpr int OOB = 0x7fff0000;
    __shared__ __attribute__((aligned(16))) char lds[2 * C::STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int l31 = lane & 31, g = lane >> 5;
    const int KB = Np / FQL_KB;
    const int a_stage = MBT * 8192, a_limb = KB * a_stage;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)limbs, 0, SETS * L * a_limb, 0x00020000);
    const size_t wbytes = (size_t)N * (size_t)(K >> 1);

    int n_real = m_slots * n_tiles;
    if (tpe != nullptr) {
        int cp = 0, ct = 0;
        for (int base = 0; base < E; base += 64) (void)expert_chunk(tpe, offs, E, T, C::BM, base, lane, cp, ct);
        n_real = __builtin_amdgcn_readfirstlane((ct < m_slots ? ct : m_slots) * n_tiles);
    }

    // transposed-read address of this lane inside a stage (fragment j, half h, k-step ks added per read):
    // 16-lane group: i = lane & 15 -> q = i >> 1 (row of the 8-row block), p = i & 1 (8 columns); gh = second 16 k
    const int tq = (lane & 15) >> 1, tp = lane & 1, gh = (lane >> 4) & 1;
    const int perm_q = 2 * (tq & 3) + (tq >> 2);                  // (0,2,4,6,1,3,5,7)[q]
    // staging: chunk c = tid + THREADS * i -> row n = c >> 2 of the stage, 16-byte packed chunk ch = c & 3 (32 k)
    for (int vb = blockIdx.x; vb < n_real; vb += gridDim.x) {
        // ---- tile
        const int tile = xcd_remap(vb, n_real);
        const int ms = tile / n_tiles, nt = tile - ms * n_tiles;
        int e = 0, row0 = ms * C::BM, prow0 = ms * C::BM, rows_valid = T - ms * C::BM;
        if (tpe != nullptr) {
            int cp = 0, ct = 0, found = 0;
            for (int base = 0; base < E && !found; base += 64) {
                const ExpertLane x = expert_chunk(tpe, offs, E, T, C::BM, base, lane, cp, ct);
                const unsigned long long hit = __ballot(ms >= x.tile_excl && ms < x.tile_excl + x.tiles);
                if (hit) {
                    const int src = __ffsll((long long)hit) - 1;
                    const int te = wave_bcast(x.tile_excl, src);
                    e = base + src;
                    row0 = wave_bcast(x.lo, src) + (ms - te) * C::BM;
                    prow0 = wave_bcast(x.pad_excl, src) + (ms - te) * C::BM;
                    rows_valid = wave_bcast(x.cnt, src) - (ms - te) * C::BM;
                    found = 1;
                }
            }
            if (!found) rows_valid = 0;
        }
        e = __builtin_amdgcn_readfirstlane(e);
        row0 = __builtin_amdgcn_readfirstlane(row0);
        prow0 = __builtin_amdgcn_readfirstlane(prow0);
        rows_valid = __builtin_amdgcn_readfirstlane(rows_valid > C::BM ? C::BM : rows_valid);
        if (rows_valid <= 0) continue;                           // (uniform over the workgroup)
        const int k0 = nt * C::BN;
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(packed + (size_t)e * wbytes), 0, (int)wbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsZ = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(zps + (size_t)e * N), 0, N * 4, 0x00020000);
        // rows of this tile with a residual limb set (delta2 != 0)?
        int res_tile = 0;
        if constexpr (RES) {
            const __amdgpu_buffer_rsrc_t rsD2 = __builtin_amdgcn_make_buffer_rsrc((void *)(delta + T), 0, T * 4, 0x00020000);
            const int v0 = __builtin_amdgcn_raw_buffer_load_b32(rsD2, lane < rows_valid ? (row0 + lane) * 4 : OOB, 0, 0);
            const int v1 = __builtin_amdgcn_raw_buffer_load_b32(rsD2, lane + 64 < rows_valid ? (row0 + lane + 64) * 4 : OOB, 0, 0);
            res_tile = __builtin_amdgcn_readfirstlane(__ballot(((v0 | v1) & 0x7fffffff) != 0) != 0ull ? 1 : 0);
        }

        v4i wr[C::CPT];
        float zr[C::CPT];
        auto load_w = [&](int kt) {                              // stage kt's packed chunks + zero points -> registers
#pragma unroll
            for (int i = 0; i < C::CPT; ++i) {
                const int c = tid + C::THREADS * i, nr = c >> 2, ch = c & 3;
                const int n = kt * FQL_KB + nr;
                const int kb = k0 + 32 * ch;                     // first k of the chunk
                const bool ok = n < N && kb < K;
                if (VW) {
                    wr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsB, ok ? n * (K >> 1) + (kb >> 1) : OOB, 0, 0);
                } else {
                    uint32_t b[4] = {0u, 0u, 0u, 0u};
                    const int ro = n * (K >> 1) + (kb >> 1);
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const bool in = ok && (kb >> 1) + j < (K >> 1);
                        const uint32_t v = __builtin_amdgcn_raw_buffer_load_b8(rsB, in ? ro + j : OOB, 0, 0);
                        b[j >> 2] |= v << (8 * (j & 3));
                    }
                    wr[i] = v4i{(int)b[0], (int)b[1], (int)b[2], (int)b[3]};
                }
                zr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsZ, n < N ? n * 4 : OOB, 0, 0));
            }
        };
        auto store_w = [&](char *buf) {                          // registers -> LDS image (q - z, natural k order)
#pragma unroll
            for (int i = 0; i < C::CPT; ++i) {
                const int c = tid + C::THREADS * i, nr = c >> 2, ch = c & 3;
                const int z = (int)fminf(fmaxf(rintf(zr[i]), -112.0f), 112.0f);
                const uint32_t nz = (uint32_t)(-z) & 0xFFu;
                const uint32_t zz = (nz & 0x7Fu) * 0x01010101u, zh = (nz & 0x80u) * 0x01010101u;
                uint32_t o0[4], o1[4];
                bwd_unpack16((uint32_t)wr[i][0], (uint32_t)wr[i][1], zz, zh, o0);
                bwd_unpack16((uint32_t)wr[i][2], (uint32_t)wr[i][3], zz, zh, o1);
                char *dst = buf + nr * C::ROWB + 32 * (ch ^ ((nr >> 1) & 3));
                *reinterpret_cast<v4i *>(dst) = v4i{(int)o0[0], (int)o0[1], (int)o0[2], (int)o0[3]};
                *reinterpret_cast<v4i *>(dst + 16) = v4i{(int)o1[0], (int)o1[1], (int)o1[2], (int)o1[3]};
            }
        };
        // A operand of fragment j at k-step ks of a stage: two transposed 8-byte reads (n blocks base and base + 8)
        auto read_frag = [&](const char *buf, int ks, int j) -> v4i {
            const int v = ks >> 1, b = ks & 1;
            const int chk = wn * NF + j;
            v2i r[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = 32 * (2 * v + g) + 16 * b + 8 * h + perm_q;
                const char *src = buf + n * C::ROWB + 32 * (chk ^ ((n >> 1) & 3)) + 16 * gh + 8 * tp;
                r[h] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i *)LDS_PTR(src));
            }
            return v4i{r[0][0], r[0][1], r[1][0], r[1][1]};
        };

        float o[NF][16];
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][r] = 0.0f;
        const int t = row0 + wm * 32 + l31;
        const bool row_ok = wm * 32 + l31 < rows_valid;

        for (int set = 0; set <= res_tile; ++set) {
            v16i acc[L][NF];
#pragma unroll
            for (int l = 0; l < L; ++l)
#pragma unroll
                for (int j = 0; j < NF; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[l][j][r] = 0;
            const int sA = ((prow0 >> 5) + wm) * 8192 + set * L * a_limb;
            auto a_off = [&](int gs) { return gs < KB * KS ? sA + (gs / KS) * a_stage + (gs % KS) * 1024 : OOB; };
            v4i afr[D][L];
            load_w(0);
#pragma unroll
            for (int s = 0; s < D; ++s)
#pragma unroll
                for (int l = 0; l < L; ++l)
                    afr[s][l] = __builtin_amdgcn_raw_buffer_load_b128(rsA, lane * 16, a_off(s) == OOB ? OOB : a_off(s) + l * a_limb, 0);
            __syncthreads();                                     // (the previous visit's last reads of the image)
            store_w(lds);
            __syncthreads();
            for (int kt = 0; kt < KB; ++kt) {
                const char *cb = lds + (kt & 1) * C::STAGE;
                const bool more = kt + 1 < KB;
                if (more) load_w(kt + 1);
                v4i bf[2][NF];
#pragma unroll
                for (int j = 0; j < NF; ++j) bf[0][j] = read_frag(cb, 0, j);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks + 1 < KS) {
#pragma unroll
                        for (int j = 0; j < NF; ++j) bf[(ks + 1) & 1][j] = read_frag(cb, ks + 1, j);
                    }
#pragma unroll
                    for (int l = 0; l < L; ++l)
#pragma unroll
                        for (int j = 0; j < NF; ++j)
                            acc[l][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[ks & 1][j], afr[ks % D][l], acc[l][j], 0, 0, 0);
                    const int gs = kt * KS + ks + D;
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        afr[ks % D][l] = __builtin_amdgcn_raw_buffer_load_b128(rsA, lane * 16, a_off(gs) == OOB ? OOB : a_off(gs) + l * a_limb, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (more) store_w(lds + ((kt + 1) & 1) * C::STAGE);
                __syncthreads();
            }
            // fold this set: delta (or delta2) * sum_l 256^l acc_l
            const float d = row_ok ? delta[(size_t)set * T + t] : 0.0f;
            if (set == 0 || d != 0.0f) {
#pragma unroll
                for (int j = 0; j < NF; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float tot = 0.0f;
#pragma unroll
                        for (int l = L - 1; l >= 0; --l) tot = fmaf(tot, 256.0f, (float)acc[l][j][r]);
                        o[j][r] = set == 0 ? tot * d : fmaf(tot, d, o[j][r]);
                    }
            }
        }
        // ---- epilogue: - sum_n g f, store rows t, columns k0 + (wn NF + j) 32 + 8 q' + 4 g + c
        if (row_ok) {
            const float cor = delta[(size_t)SETS * T + t];
            const bool vec = ((K & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0);
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int kc = k0 + (wn * NF + j) * 32 + 8 * q + 4 * g;
                    float v[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        v[c] = o[j][4 * q + c] - cor;
                        // float16: round the float32 result, never a fused multiply-add rounded straight to float16
                        // (v_fma_mixlo_f16 would: one rounding of the exact value, not Tensor.to(float16) of float32)
                        if constexpr (OUT == 1) asm volatile("" : "+v"(v[c]));
                    }
                    if (kc < K) store_out4(out, OUT, (size_t)t * K, kc, K, vec, v);
                }
        }
    }
#endif
}
