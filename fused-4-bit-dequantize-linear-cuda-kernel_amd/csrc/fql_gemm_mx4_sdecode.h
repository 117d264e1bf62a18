// The decode form of mx4_scaled_kernel (fql_gemm_mx4_scaled.h): the block-scaled grouped GEMM on MXFP4 expert weights for a
// FEW rows an expert, as fql_gemm_mx4_decode.h is the decode form of mx4_kernel.
//
// mx4_sdecode_kernel<ROWS, OUT>: ROWS = 1: e4m3 rows [T][K] with act_scale [T]; ROWS = 2: MXFP4 rows [T][K / 2] with
// in_scales [T][K / 32]; ROWS = 3: MXFP6 rows [T][3 K / 4] with in_scales [T][K / 32] (blgp = 2; a lane's fragment is the 24
// bytes of block 2 s + h, three 8-byte loads: a row is 8-byte aligned whatever K is; 12 registers a ring slot).  Workgroup = ONE wave = 32 weight rows n of one expert x one block of up to 32 rows t, for all of
// K.  No LDS, no barrier.  grid = (ceil(N / 32), ceil(T / 32), E (+ 1 with a table)); the workgroups of an expert without
// rows in that block leave at once, a count above 32 is the next row block's, so the kernel is right for every T.
//   * THE SAME BITS AS THE TILE KERNEL.  An element of the instruction's result depends on its own A row, its own B column,
//     their scales and its own accumulator only, so what has to agree is the sequence of instructions and what a lane feeds
//     them, and it does: ceil(K / 64) v_mfma_scale_f32_32x32x64_f8f6f4 in ascending k on one accumulator that starts at
//     zero, the weights as A (cbsz = 4), the rows as B (blgp = 0 with scale code 127, or blgp = 4 with the row's scale
//     byte), lane (r = lane & 31, h = lane >> 5) supplying block 2 s + h of packed row n_r with its scale byte and, of row
//     t_r, the bytes k0 + 16 h .. + 15 and k0 + 32 + 16 h .. + 15 (e4m3) or block 2 s + h with its scale byte (MXFP4).  The
//     tile kernel picks the scale byte out of a 16-bit register with op_sel; here it is byte 0 of its own register: the
//     same byte.  K % 64 == 32 ends, as there, with one instruction whose absent block is zero codes with scale code 127
//     on either side and zero row bytes past K; an instruction wholly past K is not issued.  The epilogue is the tile
//     kernel's own function (mx4_scaled_epilogue).
//   * Nothing is exchanged and nothing is converted: the 16 bytes a lane loads of a packed row ARE its operand (the operand
//     map in the header of fql_gemm_mx4_scaled.h), so a wave's weight load is 32 rows x 32 contiguous bytes with every byte
//     used, and a slot's work is one matrix instruction.  Scale code 255 and e4m3 NaN bytes are the instruction's business.
//   * Rows.  The lane loads its own fragment of row t_r from global memory (L2: the rows are a few KiB).  Rows past the
//     expert's count read its last row, weight rows past N read row N - 1; neither is stored.  Loads are unconditional.
//   * Ring.  What a lane needs for 64 k (piece, scale byte, row fragment: 13 registers with e4m3 rows, 10 with MXFP4
//     rows) is one ring slot; DEPTH slots are loaded ahead, in the order of their use, so the waits are counted ones.
//     They are refilled GROUP = 4 at a time: four pieces are 128 contiguous bytes of a packed row (fql_gemm_mx4_decode.h
//     measured that form).  The odd last block of K % 64 == 32 is loaded first of all and used last.
//   * e4m3 rows whose base is not 16-byte aligned take the same kernel with byte loads and a ring of one slot.
#pragma once
#include "fql_gemm_mx4_scaled.h"

#ifndef FQL_MX4_SDECODE_DEPTH
#define FQL_MX4_SDECODE_DEPTH 8   // ring slots (A/B knob)
#endif

struct Mx4SDecodeCfg {
    static constexpr int BT = 32, BN = 32;             // rows t and weight rows n of a workgroup (one MFMA result)
    static constexpr int THREADS = 64;
    static constexpr int DEPTH = FQL_MX4_SDECODE_DEPTH;   // 64 k a slot
    static constexpr int GROUP = 4;                    // slots refilled together: 128 contiguous bytes of a packed row
};

// One ring slot: what lane (r, h) holds of 64 k between its loads and their use.
template <int ROWS>
struct Mx4SDecodeSlot {
    uint4 wq;                                          // the 16 bytes of scale block 2 s + h of the packed weight row
    uint8_t sc;                                        // its scale code
    uint4 x[ROWS == 1 ? 2 : 1];                        // e4m3: k0 + 16 h .. + 15 and k0 + 32 + 16 h .. + 15; MXFP4: block 2 s + h
    uint2 x6[ROWS == 3 ? 3 : 1];                       // MXFP6: the three 8-byte words of block 2 s + h (x is not used then)
    uint8_t xs;                                        // MXFP4 / MXFP6 rows: that block's scale code
};

// VEC: the rows' base is 16-byte aligned (every row and every fragment is, then: K % 32 == 0; MXFP4 rows always are).
template <int ROWS, int OUT, bool VEC, int DEPTH, int GROUP>
__device__ __forceinline__ void mx4_sdecode_body(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const uint8_t *__restrict__ x,
    const uint8_t *__restrict__ xscales, const float *__restrict__ act_scale, const float *__restrict__ bias,
    void *__restrict__ out, int e, int row_lo, int cnt, int t_blk, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    static_assert(ROWS == 1 || VEC, "packed rows are 16-byte aligned (MXFP4) or read in 8-byte words (MXFP6)");
    using Slot = Mx4SDecodeSlot<ROWS>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4SDecodeCfg::BN;
    const int K2 = K >> 1, KB = K >> 5;
    // Loads are unconditional: a lane past N reads row N - 1 (its results are never stored and reach no other lane's), a
    // lane past the count reads the expert's last row.
    const size_t wrow = (size_t)e * N + (n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KB;
    const bool row_ok = t_blk + r < cnt;
    const int t = row_lo + (row_ok ? t_blk + r : cnt - 1);
    const uint8_t *xrow = x + (size_t)t * (ROWS == 1 ? K : ROWS == 2 ? K2 : 3 * (K >> 2));
    const uint8_t *xsrow = ROWS != 1 ? xscales + (size_t)t * KB : nullptr;

    auto load16 = [&](const uint8_t *p) {
        if constexpr (VEC) {
            return *reinterpret_cast<const uint4 *>(p);
        } else {
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) wd[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
            return make_uint4(wd[0], wd[1], wd[2], wd[3]);
        }
    };
    // the 64 k of instruction s; hw / hx: the block of the pair this lane takes of the weight row / of the row (h, but 0
    // for both halves where only block 2 s exists); BOTH: the e4m3 bytes k0 + 32 .. exist
    auto load_slot = [&](Slot &sl, int s, int hw, int hx, auto BOTH) {
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * s + 16 * hw);
        sl.sc = sbase[2 * s + hw];
        if constexpr (ROWS == 1) {
            sl.x[0] = load16(xrow + 64 * s + 16 * hx);
            if constexpr (decltype(BOTH)::value) sl.x[1] = load16(xrow + 64 * s + 32 + 16 * hx);
            else sl.x[1] = make_uint4(0u, 0u, 0u, 0u);
            sl.xs = 127;
        } else if constexpr (ROWS == 2) {
            sl.x[0] = *reinterpret_cast<const uint4 *>(xrow + 32 * s + 16 * hx);
            sl.xs = xsrow[2 * s + hx];
        } else {                                                   // (a block is 24 bytes at a multiple of 8: three 8-byte loads)
            const uint2 *p = reinterpret_cast<const uint2 *>(xrow + 48 * s + 24 * hx);
#pragma unroll
            for (int j = 0; j < 3; ++j) sl.x6[j] = p[j];
            sl.xs = xsrow[2 * s + hx];
        }
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;

    auto consume = [&](const Slot &sl) {                           // one instruction: k0 = 64 s
        const v8i av = {(int)sl.wq.x, (int)sl.wq.y, (int)sl.wq.z, (int)sl.wq.w, 0, 0, 0, 0};
        if constexpr (ROWS == 1) {
            const v8i bv = {(int)sl.x[0].x, (int)sl.x[0].y, (int)sl.x[0].z, (int)sl.x[0].w,
                            (int)sl.x[1].x, (int)sl.x[1].y, (int)sl.x[1].z, (int)sl.x[1].w};
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 0, 0, (int)sl.sc, 0, 0x7F7F7F7F);
        } else if constexpr (ROWS == 2) {
            const v8i bv = {(int)sl.x[0].x, (int)sl.x[0].y, (int)sl.x[0].z, (int)sl.x[0].w, 0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 4, 0, (int)sl.sc, 0, (int)sl.xs);
        } else {
            const v8i bv = {(int)sl.x6[0].x, (int)sl.x6[0].y, (int)sl.x6[1].x, (int)sl.x6[1].y, (int)sl.x6[2].x, (int)sl.x6[2].y, 0, 0};
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 2, 0, (int)sl.sc, 0, (int)sl.xs);
        }
    };

    // K % 64 == 32: the last scale block has no partner.  Both halves load it (the h = 1 lanes drop theirs below; the
    // absent block's scale byte is never read); of an e4m3 row the 32 bytes that exist are k0 + 16 h .. + 15 of both halves.
    const int pairs = K >> 6;
    const bool odd = (K & 32) != 0;
    Slot tail;
    if (odd) load_slot(tail, pairs, 0, ROWS == 1 ? h : 0, std::false_type{});
    __builtin_amdgcn_sched_barrier(0);

    // The loop that loads has no branch in it (a branch around a load makes the compiler wait for every load at the
    // join): a slot index past the last pair loads the last pair again, at most DEPTH times a wave, and is not used.
    if (pairs > 0) {
        const int last = pairs - 1;
        Slot ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {                          // (in the order of their use: the waits count on it)
            load_slot(ring[i], i < last ? i : last, h, h, std::true_type{});
            __builtin_amdgcn_sched_barrier(0);
        }
        int j = 0;
        for (; j + DEPTH <= pairs; j += DEPTH) {
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) {
                consume(ring[i]);
                // Refill the GROUP slots just used, back to back (the scheduling barriers keep the loads where they are
                // written, as in mx4_decode_kernel).
                if (i % GROUP == GROUP - 1) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = i - (GROUP - 1); q <= i; ++q) {
                        const int nx = j + q + DEPTH;
                        load_slot(ring[q], nx < last ? nx : last, h, h, std::true_type{});
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
        if (h) {
            tail.wq = make_uint4(0u, 0u, 0u, 0u);
            tail.sc = 127;
            if constexpr (ROWS == 2) { tail.x[0] = make_uint4(0u, 0u, 0u, 0u); tail.xs = 127; }
            if constexpr (ROWS == 3) {
#pragma unroll
                for (int j = 0; j < 3; ++j) tail.x6[j] = make_uint2(0u, 0u);
                tail.xs = 127;
            }
        }
        consume(tail);
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    if (!row_ok) return;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
    const float as = ROWS != 1 || act_scale == nullptr ? 1.0f : act_scale[t];
    mx4_scaled_epilogue<ROWS, OUT>(acc, out, t, N, n0, h, vec, brow, act_scale, as);
}

// ROWS, OUT as the tile kernel's.
template <int ROWS, int OUT>
__global__ __launch_bounds__(64) void mx4_sdecode_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const uint8_t *__restrict__ x,
    const uint8_t *__restrict__ xscales, const float *__restrict__ act_scale, const float *__restrict__ bias,
    void *__restrict__ out, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4SDecodeCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    const int e = blockIdx.z;
    if (ROWS != 1 || (reinterpret_cast<uintptr_t>(x) & 15) == 0)
        mx4_sdecode_body<ROWS, OUT, true, C::DEPTH, C::GROUP>(blocks, scales, x, xscales, act_scale, bias, out, e, row_lo, cnt, t_blk, K, N);
    else if constexpr (ROWS == 1)
        mx4_sdecode_body<ROWS, OUT, false, 1, 1>(blocks, scales, x, xscales, act_scale, bias, out, e, row_lo, cnt, t_blk, K, N);
#endif
}
