// The decode form of mx4_kernel (fql_gemm_mx4.h): the same grouped GEMM on MXFP4 expert weights for a FEW rows an expert,
// where the call is a weight stream and a 64 x 128 tile with a barrier every 64 k leaves most of the chip waiting.
//
// mx4_decode_kernel: workgroup = ONE wave = 32 weight rows n of one expert x one block of up to 32 rows t, for all of K.
// No LDS, no barrier.  grid = (ceil(N / 32), ceil(T / 32), E (+ 1 with a table)); the workgroups of an expert without rows
// in that block leave at once, a count above 32 is the next row block's, so the kernel is right for every T.
//   * THE SAME BITS AS mx4_kernel.  An element of an MFMA's result depends on its own A row, its own B column and its own
//     accumulator only, so what has to agree is the sequence of instructions and what a lane feeds them, and it does:
//     v_mfma_f32_32x32x16_bf16 with the weights as A and the rows as B, k0 = 0, 16, 32, ... one instruction per 16 k on an
//     accumulator that starts at zero, lane (r = lane & 31, h = lane >> 5) supplying W[n_r][k0 + 8 h .. + 7] and
//     x[t_r][k0 + 8 h .. + 7]; mx4_pair / mx4_pack_bf16 as they are; K % 64 == 32 ends, as there, with two instructions on
//     zeros (the tile kernel's last stage is 64 k deep); bias, the NaN row and store_out4 in the same order.
//   * Weights.  Lane (r, h) loads ONE 16-byte piece of packed row n_r per 64 k: the 32 k of scale block 2 j + h, so a wave's
//     load instruction is 32 rows x 32 contiguous bytes with every byte used.  Dword i of a piece is 8 k, and step s of the
//     64 k wants dword (2 s + h) & 3 of block s >> 1: lane h = 0 keeps d0, d2 of its block and needs e0, e2 of the other
//     half's, lane h = 1 keeps e1, e3 and needs d1, d3.  Two v_permlane32_swap do it: swap(x, y) leaves {d0 | d1} (step 0)
//     and {e0 | e1} (step 2), swap(z, w) leaves {d2 | d3} and {e2 | e3}; a third one on the scale byte gives both halves
//     both blocks' scales.  The 32 codes a lane feeds the matrix core are converted after the exchange, in registers.
//   * Rows.  The lane loads its own fragment x[t_r][k0 + 8 h .. + 7] from global memory (L2: the rows are a few KiB) as it
//     is, 16 bytes of bfloat16 or 32 of float32 a step.  Rows past the expert's count read its last row, so a block with
//     c live rows touches c rows' lines however many lanes load.  (mx4_kernel found this form slow at 64 live rows.)
//   * Ring.  Everything a lane needs for 64 k (piece, scale byte, four row fragments) is one ring slot; DEPTH slots are
//     loaded ahead, in the order of their use, so the waits are counted ones.  They are refilled GROUP at a time: four
//     pieces are 128 contiguous bytes of a packed row, so a row's cache line is asked for by consecutive instructions
//     and not by four that lie a slot's work apart (measured: 15 to 22 % of the call at 1 to 32 tokens).  The odd last
//     block of K % 64 == 32 is loaded first of all and used last.
//   * NON-FINITE.  The lane ORs the exponent test over the words it feeds (its half of the row's k); one more swap ORs the
//     two halves.  Scale code 255: 0x7FC0 across the block, as in mx4_kernel.
//   * Rows whose base is not 16-byte aligned take the same kernel with element loads and a ring of one slot.
#pragma once
#include "fql_gemm_mx4.h"

#ifndef FQL_MX4_DECODE_DEPTH
#define FQL_MX4_DECODE_DEPTH 8   // ring slots of the bfloat16-row kernel (A/B knob; float32 rows take half as many)
#endif

struct Mx4DecodeCfg {
    static constexpr int BT = 32, BN = 32;             // rows t and weight rows n of a workgroup (one MFMA result)
    static constexpr int THREADS = 64;
    static constexpr int DEPTH_BF16 = FQL_MX4_DECODE_DEPTH, DEPTH_F32 = DEPTH_BF16 / 2;   // 64 k a slot: 21 / 37 registers
    static constexpr int GROUP_BF16 = 4, GROUP_F32 = 2;   // slots refilled together: 4 = 128 contiguous bytes of a packed row
};

// One ring slot: what lane (r, h) holds of 64 k between its loads and their use.
template <int IN>
struct Mx4DecodeSlot {
    uint4 wq;                                                      // the 16-byte piece of scale block 2 j + h
    uint8_t sc;                                                    // its scale code (kept a byte: see consume)
    typename std::conditional<IN == 0, float, uint32_t>::type x[4][IN == 0 ? 8 : 4];   // x[t_r][64 j + 16 s + 8 h .. + 7], step s
};

// Copies of a slot's piece and scale for the lane swaps to overwrite.  The s_nop is the two wait states a VALU write needs
// before v_permlane32_swap reads it: the compiler pads its own instructions, not the inside of an asm statement.
__device__ __forceinline__ void mx4_decode_copy(const uint4 &wq, uint32_t sc, uint32_t (&w)[4], uint32_t &own)
{
    asm("v_mov_b32 %0, %5\n\tv_mov_b32 %1, %6\n\tv_mov_b32 %2, %7\n\tv_mov_b32 %3, %8\n\tv_mov_b32 %4, %9\n\ts_nop 1"
        : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(own)
        : "v"(wq.x), "v"(wq.y), "v"(wq.z), "v"(wq.w), "v"(sc));
}

// VEC: the rows' base is 16-byte aligned (every row and every fragment is, then: K % 32 == 0).
template <int IN, int OUT, bool VEC, int DEPTH, int GROUP>
__device__ __forceinline__ void mx4_decode_body(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    const float *__restrict__ bias, void *__restrict__ out, int e, int row_lo, int cnt, int t_blk, int K, int N)
{
    static_assert(DEPTH % GROUP == 0, "the ring is refilled in whole groups");
    using Slot = Mx4DecodeSlot<IN>;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int n0 = (int)blockIdx.x * Mx4DecodeCfg::BN;
    const int K2 = K >> 1, KB = K >> 5;
    constexpr int es = IN == 0 ? 4 : 2;
    // Loads are unconditional: a lane past N reads row N - 1 (its results are never stored and reach no other lane's), a
    // lane past the count reads the expert's last row.
    const size_t wrow = (size_t)e * N + (n0 + r < N ? n0 + r : N - 1);
    const uint8_t *wbase = blocks + wrow * K2;
    const uint8_t *sbase = scales + wrow * KB;
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
    auto load_slot = [&](Slot &sl, int j) {                        // the 64 k of pair j (both scale blocks exist)
        sl.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * j + 16 * h);
        sl.sc = sbase[2 * j + h];
#pragma unroll
        for (int s = 0; s < 4; ++s) load_x(sl, j, s);
    };

    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    uint32_t bad = 0u;

    auto consume = [&](const Slot &sl) {                           // four instructions: k0 = 64 j + 16 s, s = 0 .. 3
        // (The swap writes both its operands.  Handed the ring's registers, the compiler copies next round's into place at
        //  the END of the loop, i.e. waits there for every load in flight: copy here instead, where the slot is due.  The
        //  scale is a byte in the slot for the same reason: a 32-bit one is widened for all slots at the top of the loop.)
        uint32_t w[4], own;
        mx4_decode_copy(sl.wq, sl.sc, w, own);
        const auto lo = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);         // {d0 | d1}, {e0 | e1}
        const auto hi = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);         // {d2 | d3}, {e2 | e3}
        const auto sc = __builtin_amdgcn_permlane32_swap(own, own, false, false);           // block 2 j, block 2 j + 1
        const uint32_t words[4] = {lo[0], hi[0], lo[1], hi[1]};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            // (mx4_dequant8, spelled out: through the function the compiler arranges this loop otherwise, 5 % more instructions)
            const int code = (int)sc[s >> 1];
            const bool nan = code == 255;
            const int sv = nan ? 127 : code;
            uint4 a;
            a.x = mx4_pair<0>(words[s], sv);
            a.y = mx4_pair<1>(words[s], sv);
            a.z = mx4_pair<2>(words[s], sv);
            a.w = mx4_pair<3>(words[s], sv);
            if (nan) a = make_uint4(0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u);
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

    // K % 64 == 32: the last scale block has no partner.  Both halves load it (the h = 1 lanes drop theirs below) and
    // the 32 k of x that exist; the rest of the slot is the zeros mx4_kernel pads its last stage with.
    const int pairs = K >> 6;
    const bool odd = (K & 32) != 0;
    Slot tail;
    if (odd) {
        tail.wq = *reinterpret_cast<const uint4 *>(wbase + 32 * pairs);
        tail.sc = sbase[2 * pairs];
#pragma unroll
        for (int s = 0; s < 2; ++s) load_x(tail, pairs, s);
    }
    __builtin_amdgcn_sched_barrier(0);

    // The loop that loads has no branch in it (a branch around a load makes the compiler wait for every load at the
    // join): a slot index past the last pair loads the last pair again, at most DEPTH times a wave, and is not used.
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
                // Refill the GROUP slots just used, back to back.  (The scheduling barriers keep the loads where they are
                // written: left alone, the scheduler gathers a round's loads at its end and the next round's waits drain them.)
                if (i % GROUP == GROUP - 1) {
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
        if (h) { tail.wq = make_uint4(0u, 0u, 0u, 0u); tail.sc = 127; }
#pragma unroll
        for (int s = 2; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < (IN == 0 ? 8 : 4); ++i) tail.x[s][i] = 0;
        consume(tail);
    }

    // D[i][j]: i = n (A), j = t (B): the lane owns row t, registers 4q .. 4q+3 are n = 8 q + 4 h + (0 .. 3) of the block.
    const auto both = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);   // the row's other half of k
    if (!row_ok) return;
    const bool row_nan = ((both[0] | both[1]) & 0x80008000u) != 0u;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (OUT == 0 ? 15 : 7)) == 0;
    const float *brow = bias == nullptr ? nullptr : bias + (size_t)e * N;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nc = n0 + 8 * q + 4 * h;
        if (nc >= N) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = acc[4 * q + c];
            if (brow != nullptr && nc + c < N) v[c] += brow[nc + c];
            if (row_nan) v[c] = __uint_as_float(0x7FC00000u);
        }
        store_out4(out, OUT, (size_t)t * N, nc, N, vec, v);
    }
}

// IN, OUT as mx4_kernel's.
template <int IN, int OUT>
__global__ __launch_bounds__(64) void mx4_decode_kernel(
    const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const void *__restrict__ x,
    const float *__restrict__ bias, void *__restrict__ out, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, int T, int K, int N)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using C = Mx4DecodeCfg;
    int row_lo, cnt, t_blk;
    if (!mx4_group_begin<C::THREADS, OUT>(out, N, tpe, offs, E, T, C::BT, row_lo, cnt, t_blk)) return;
    const int e = blockIdx.z;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        mx4_decode_body<IN, OUT, true, IN == 0 ? C::DEPTH_F32 : C::DEPTH_BF16, IN == 0 ? C::GROUP_F32 : C::GROUP_BF16>(blocks, scales, x, bias, out, e, row_lo, cnt, t_blk, K, N);
    else
        mx4_decode_body<IN, OUT, false, 1, 1>(blocks, scales, x, bias, out, e, row_lo, cnt, t_blk, K, N);
#endif
}
