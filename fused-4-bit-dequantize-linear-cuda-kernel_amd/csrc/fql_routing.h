// Token routing either side of the grouped GEMM, on the device and in single launches (SURVEY section 8f N1 and
// the expert-parallel step of 8e): what the reference does with argsort / bincount / cumsum / index ops / a
// broadcast multiply and a sum (benchmark/moe_grouped_gemm/routing.py:117-149, 172-189).
//
//   route_plan_kernel    stable counting sort of the (token, slot) pairs by expert id: per-expert counts, their
//                        exclusive prefix (= tokens_per_expert / input_offsets of the grouped GEMM), for every
//                        sorted position the token row it reads (the gather index of fql_moe_gather_fwd_f32) and
//                        for every slot its sorted position (the un-sort index of the combine).
//   route_plan_capped_kernel  the same plan with a token mask and a per-expert capacity: a masked or overflowing slot
//                        gets no row (pos_of_slot = -1), the kept rows stay compact and in expert order.
//   combine_kernel       out[t][:] = sum_k w[t][k] * y[pos[t][k]][:]  (k ascending) + an optional per-token weighted
//                        addend (a shared expert's rows), with an element type for y and one for out (float32 /
//                        float16 / bfloat16), accesses of up to 16 bytes.
//   combine_bwd_kernel   its gradients to y, w, the addend and the addend's weight, in one launch.
//                        Both take a SPARSE flag: a slot with pos < 0 is skipped instead of clamped to row 0.
//   regroup_index_kernel expert-parallel receive side: rows arrive (source rank, local expert)-major, the GEMM
//                        wants (local expert, source rank)-major: gather index + its inverse + the expert table.
#pragma once
#include "fql_common.h"

#define ROUTE_THREADS 256
#define ROUTE_MAX_EXPERTS 128          // LDS: ROUTE_THREADS x experts counters

// One workgroup.  Thread i owns the contiguous slots [i*chunk, (i+1)*chunk): sequential inside a thread and
// threads in slot order, so equal keys keep their order (stable, like argsort(stable=True)).
__global__ __launch_bounds__(ROUTE_THREADS) void route_plan_kernel(
    const int32_t *__restrict__ expert_of_slot, int n_slots, int top_k, int E,
    int32_t *__restrict__ counts, int32_t *__restrict__ offsets, int32_t *__restrict__ token_of_sorted,
    int32_t *__restrict__ pos_of_slot)
{
    extern __shared__ int s_cnt[];                 // [ROUTE_THREADS][E], then per-expert bases at the end
    int *s_base = s_cnt + ROUTE_THREADS * E;       // [E]
    const int tid = threadIdx.x;
    const int chunk = (n_slots + ROUTE_THREADS - 1) / ROUTE_THREADS;
    const int lo = tid * chunk, hi = (lo + chunk < n_slots) ? lo + chunk : n_slots;
    for (int e = 0; e < E; ++e) s_cnt[tid * E + e] = 0;
    for (int i = lo; i < hi; ++i) {
        int e = expert_of_slot[i];
        e = e < 0 ? 0 : (e >= E ? E - 1 : e);      // ids outside [0, E) are clamped
        s_cnt[tid * E + e] += 1;
    }
    __syncthreads();
    // per expert: exclusive scan over the threads (column e), total -> counts
    for (int e = tid; e < E; e += ROUTE_THREADS) {
        int run = 0;
        for (int t = 0; t < ROUTE_THREADS; ++t) {
            const int c = s_cnt[t * E + e];
            s_cnt[t * E + e] = run;
            run += c;
        }
        counts[e] = run;
        s_base[e] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int e = 0; e < E; ++e) {
            const int c = s_base[e];
            s_base[e] = run;
            offsets[e] = run;
            run += c;
        }
    }
    __syncthreads();
    for (int i = lo; i < hi; ++i) {
        int e = expert_of_slot[i];
        e = e < 0 ? 0 : (e >= E ? E - 1 : e);
        const int pos = s_base[e] + s_cnt[tid * E + e]++;
        token_of_sorted[pos] = i / top_k;
        pos_of_slot[i] = pos;
    }
}

// ---- the plan with slots that go nowhere: a token mask and a per-expert capacity.
// Inclusive prefix sum over the 64 lanes of a wave.
__device__ __forceinline__ int wave_scan_i(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// ROUTE_BATCH consecutive slots of a thread's range [.., hi), from slot i0 on: e[j] the clamped expert id, or -1 for a slot
// that is past the range or masked out, and t[j] its token.  The loads of a batch do not depend on each other and none
// sits behind a per-lane condition, so they are in flight together; one slot at a time, the loop pays the latency of a
// global load (two, with a mask) per slot.  (tok, rem) = (i / top_k, i % top_k) of slot i = min(i0, hi - 1) on entry and of
// min(i0 + ROUTE_BATCH, hi - 1) on return: the token index walks along with the slots, no division per slot, and never
// leaves the range, so the mask byte it names exists.
#define ROUTE_BATCH 4
__device__ __forceinline__ void route_load_batch(const int32_t *__restrict__ expert_of_slot,
                                                 const uint8_t *__restrict__ token_mask, int i0, int hi, int top_k, int E,
                                                 int &tok, int &rem, int (&e)[ROUTE_BATCH], int (&t)[ROUTE_BATCH])
{
    uint8_t m[ROUTE_BATCH];
#pragma unroll
    for (int j = 0; j < ROUTE_BATCH; ++j) {
        e[j] = expert_of_slot[i0 + j < hi ? i0 + j : hi - 1];        // past the range: a valid address, the value is dropped
        t[j] = tok;
        if (i0 + j + 1 < hi && ++rem == top_k) { rem = 0; ++tok; }
    }
    if (token_mask != nullptr) {
#pragma unroll
        for (int j = 0; j < ROUTE_BATCH; ++j) m[j] = token_mask[t[j]];
    } else {
#pragma unroll
        for (int j = 0; j < ROUTE_BATCH; ++j) m[j] = 1;
    }
#pragma unroll
    for (int j = 0; j < ROUTE_BATCH; ++j)
        e[j] = (i0 + j >= hi || m[j] == 0) ? -1 : (e[j] < 0 ? 0 : (e[j] >= E ? E - 1 : e[j]));      // ids outside [0, E) are clamped
}

// One workgroup, the slot ownership of route_plan_kernel (thread i owns a contiguous range, threads in slot order), so
// a slot's rank among the eligible slots of its expert is the stable order of that kernel.  The counters are laid out
// expert-major, s_rank[e * ROUTE_THREADS + tid]: the 64 lanes of a wave touch 64 consecutive words (64 banks) whatever E
// is.  A column (one expert, ROUTE_THREADS counters) is scanned by one wave: every lane loads the four counters of
// threads 4 * lane .. 4 * lane + 3 in one 16-byte access, the lane sums are scanned across the wave, and the exclusive
// prefixes go back the same way.  A slot is kept when its rank is below `cap` (0: no limit); a slot that is masked out
// (token_mask[token] == 0) is not counted at all.
__global__ __launch_bounds__(ROUTE_THREADS) void route_plan_capped_kernel(
    const int32_t *__restrict__ expert_of_slot, int n_slots, int top_k, int E, const uint8_t *__restrict__ token_mask,
    int cap, int32_t *__restrict__ demand, int32_t *__restrict__ counts, int32_t *__restrict__ offsets,
    int32_t *__restrict__ token_of_sorted, int32_t *__restrict__ pos_of_slot)
{
    extern __shared__ __attribute__((aligned(16))) int s_rank[];      // [E][ROUTE_THREADS], then [E] bases, then the total
    int *s_base = s_rank + ROUTE_THREADS * E;                            // [E]: kept rows, then their exclusive prefix
    int *s_total = s_base + E;                                           // [1]: all kept rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = n_slots > 0 ? (n_slots - 1) / ROUTE_THREADS + 1 : 0;
    const long long lo64 = (long long)tid * chunk;
    const int lo = lo64 < n_slots ? (int)lo64 : n_slots;
    const int hi = lo64 + chunk < n_slots ? (int)(lo64 + chunk) : n_slots;
    const int limit = cap > 0 ? cap : 0x7fffffff;
    for (int e = 0; e < E; ++e) s_rank[e * ROUTE_THREADS + tid] = 0;
    int e4[ROUTE_BATCH], t4[ROUTE_BATCH];
    int tok = lo / top_k, rem = lo - tok * top_k;
    for (int i0 = lo; i0 < hi; i0 += ROUTE_BATCH) {
        route_load_batch(expert_of_slot, token_mask, i0, hi, top_k, E, tok, rem, e4, t4);
#pragma unroll
        for (int j = 0; j < ROUTE_BATCH; ++j)
            if (e4[j] >= 0) s_rank[e4[j] * ROUTE_THREADS + tid] += 1;
    }
    __syncthreads();
    // per expert: exclusive scan over the threads, one wave per column; the total is the demand
    for (int e = wave; e < E; e += ROUTE_THREADS / 64) {
        int4 *col = reinterpret_cast<int4 *>(s_rank + e * ROUTE_THREADS) + lane;
        const int4 c = *col;
        const int sum = (c.x + c.y) + (c.z + c.w);
        const int incl = wave_scan_i(sum, lane);
        const int x0 = incl - sum;
        *col = make_int4(x0, x0 + c.x, x0 + c.x + c.y, x0 + c.x + c.y + c.z);
        if (lane == 63) {
            const int kept = incl < limit ? incl : limit;
            demand[e] = incl;
            counts[e] = kept;
            s_base[e] = kept;
        }
    }
    __syncthreads();
    if (wave == 0) {                               // exclusive prefix of the kept counts: two experts per lane (E <= 128)
        const int e0 = 2 * lane, e1 = e0 + 1;
        const int c0 = e0 < E ? s_base[e0] : 0, c1 = e1 < E ? s_base[e1] : 0;
        const int incl = wave_scan_i(c0 + c1, lane);
        const int x0 = incl - (c0 + c1);
        if (e0 < E) { s_base[e0] = x0; offsets[e0] = x0; }
        if (e1 < E) { s_base[e1] = x0 + c0; offsets[e1] = x0 + c0; }
        if (lane == 63) *s_total = incl;
    }
    __syncthreads();
    tok = lo / top_k, rem = lo - tok * top_k;
    for (int i0 = lo; i0 < hi; i0 += ROUTE_BATCH) {
        route_load_batch(expert_of_slot, token_mask, i0, hi, top_k, E, tok, rem, e4, t4);
#pragma unroll
        for (int j = 0; j < ROUTE_BATCH; ++j) {
            const int i = i0 + j;
            if (i >= hi) break;
            int pos = -1;
            if (e4[j] >= 0) {
                const int rank = s_rank[e4[j] * ROUTE_THREADS + tid]++;
                if (rank < limit) {
                    pos = s_base[e4[j]] + rank;
                    token_of_sorted[pos] = t4[j];
                }
            }
            pos_of_slot[i] = pos;
        }
    }
    // the rows behind the kept ones belong to no expert: a valid gather index, row 0
    for (long long i = (long long)*s_total + tid; i < n_slots; i += ROUTE_THREADS) token_of_sorted[i] = 0;
}

// ---- the combine.  KIND is an FQL_DTYPE_* code: 0 float32, 1 float16, 2 bfloat16.  16-bit
//      elements are widened in registers on load (exact) and rounded once, to nearest even, on store.
template <int KIND> struct CombElem { using type = unsigned short; };
template <> struct CombElem<0> { using type = float; };

template <int KIND>
__device__ __forceinline__ float comb_widen(typename CombElem<KIND>::type u)
{
    if constexpr (KIND == 0) return u;
    else if constexpr (KIND == 1) {
        _Float16 h;
        __builtin_memcpy(&h, &u, 2);
        return (float)h;
    } else return __uint_as_float((uint32_t)u << 16);
}
template <int KIND>
__device__ __forceinline__ typename CombElem<KIND>::type comb_round(float v)
{
    if constexpr (KIND == 0) return v;
    else if constexpr (KIND == 1) return f32_to_f16_bits(v);
    else return f32_to_bf16_bits(v);
}

// round(w * g) of the backward: the float32 product, rounded, THEN converted, as a multiply followed by Tensor.to does.
// hipcc selects v_fma_mixlo_f16 for a float16 conversion of a product: that rounds the exact product once (another bit
// where the two roundings disagree) and computes w * g + 0 (a -0 product becomes +0).  The identity lane move between the
// multiply and the conversion keeps them two instructions.
template <int KIND>
__device__ __forceinline__ typename CombElem<KIND>::type comb_round_product(float w, float g)
{
    float p = w * g;
    if constexpr (KIND == 1) p = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(p), 0xE4, 0xF, 0xF, false));
    return comb_round<KIND>(p);
}

// A thread's V consecutive columns of a row move in one of three ways.  COMB_WIDE: accesses of up to 16 bytes (V elements,
// or two halves when V float32 make 32 bytes); needs N % V == 0 and a base aligned to the access.  COMB_PAIR: accesses of
// two elements (N even, base aligned to two elements).  COMB_SCALAR: one element at a time.  `left` = N - n columns of
// the row remain at the thread's first one; a column past the row is loaded as 0 and never stored.
enum { COMB_WIDE = 0, COMB_PAIR = 1, COMB_SCALAR = 2 };
template <int KIND, int V>
struct CombRow {
    using E = typename CombElem<KIND>::type;
    static constexpr int C = (V * (int)sizeof(E) > 16) ? 16 / (int)sizeof(E) : V;      // elements of one wide access
    typedef E EC __attribute__((ext_vector_type(C)));
    typedef E E2 __attribute__((ext_vector_type(2)));

    static __device__ __forceinline__ int mode(uintptr_t base_bits, int N)
    {
        if (N % V == 0 && (base_bits & (C * sizeof(E) - 1)) == 0) return COMB_WIDE;
        if (N % 2 == 0 && (base_bits & (2 * sizeof(E) - 1)) == 0) return COMB_PAIR;
        return COMB_SCALAR;
    }
    static __device__ __forceinline__ void load(const E *p, int mode, int left, float (&v)[V])
    {
        if (mode == COMB_WIDE) {
#pragma unroll
            for (int c0 = 0; c0 < V; c0 += C) {
                const EC r = *reinterpret_cast<const EC *>(p + c0);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c0 + c] = comb_widen<KIND>(r[c]);
            }
        } else if (mode == COMB_PAIR) {
#pragma unroll
            for (int c = 0; c < V; c += 2) {
                v[c] = v[c + 1] = 0.0f;
                if (c < left) {
                    const E2 r = *reinterpret_cast<const E2 *>(p + c);
                    v[c] = comb_widen<KIND>(r[0]);
                    v[c + 1] = comb_widen<KIND>(r[1]);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < V; ++c) v[c] = c < left ? comb_widen<KIND>(p[c]) : 0.0f;
        }
    }
    static __device__ __forceinline__ void store(E *p, int mode, int left, const float (&v)[V])
    {
        if (mode == COMB_WIDE) {
#pragma unroll
            for (int c0 = 0; c0 < V; c0 += C) {
                EC r;
#pragma unroll
                for (int c = 0; c < C; ++c) r[c] = comb_round<KIND>(v[c0 + c]);
                *reinterpret_cast<EC *>(p + c0) = r;
            }
        } else if (mode == COMB_PAIR) {
#pragma unroll
            for (int c = 0; c < V; c += 2)
                if (c < left) *reinterpret_cast<E2 *>(p + c) = E2{comb_round<KIND>(v[c]), comb_round<KIND>(v[c + 1])};
        } else {
#pragma unroll
            for (int c = 0; c < V; ++c) if (c < left) p[c] = comb_round<KIND>(v[c]);
        }
    }
};

// out[t][n] = round_out( (...((0 + y[p_0][n] * w_0) + y[p_1][n] * w_1)...) + addend[t][n] * aw[t] ): the slot terms are
// float32, multiply then add, k ascending, pos clamped to [0, R) (w == NULL: 1, and x * 1 == x: the gather-add form keeps
// the bits of pre-weighted rows); the addend term comes last (addend == NULL: none; aw == NULL: 1, the bits of "+ addend").
// grid: (ceil(N / (V * 256)), T); one thread = V consecutive columns of one token, V = 16 bytes of the input type.
// SPARSE: a slot with pos < 0 (dropped by route_plan_capped_kernel) adds nothing; neither its row nor its weight is read.
template <int IK, int OK, bool SPARSE = false>
__global__ __launch_bounds__(256) void combine_kernel(
    const void *__restrict__ y_, const int32_t *__restrict__ pos_of_slot, const float *__restrict__ w,
    const void *__restrict__ addend_, const float *__restrict__ aw, void *__restrict__ out_, int T, int top_k, int N, int R)
{
#pragma clang fp contract(off)                     // (y * w), THEN add, as the reference does: never an FMA
    constexpr int V = IK == 0 ? 4 : 8;
    using In = CombRow<IK, V>;
    using Out = CombRow<OK, V>;
    const typename In::E *y = static_cast<const typename In::E *>(y_), *addend = static_cast<const typename In::E *>(addend_);
    typename Out::E *out = static_cast<typename Out::E *>(out_);
    const int t = blockIdx.y;
    const int n = (blockIdx.x * 256 + threadIdx.x) * V;
    if (n >= N) return;
    const int left = N - n;
    const int imode = In::mode(reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(addend), N);
    const int omode = Out::mode(reinterpret_cast<uintptr_t>(out), N);
    float acc[V], v[V];
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] = 0.0f;
    for (int k = 0; k < top_k; ++k) {
        int p = pos_of_slot[t * top_k + k];
        if (SPARSE && p < 0) continue;
        p = p < 0 ? 0 : (p >= R ? R - 1 : p);
        const float wk = w != nullptr ? w[t * top_k + k] : 1.0f;
        In::load(y + (size_t)p * N + n, imode, left, v);
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = acc[c] + v[c] * wk;
    }
    if (addend != nullptr) {
        const float a = aw != nullptr ? aw[t] : 1.0f;
        In::load(addend + (size_t)t * N + n, imode, left, v);
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = acc[c] + v[c] * a;
    }
    Out::store(out + (size_t)t * N + n, omode, left, acc);
}

// Backward of combine_kernel, one workgroup per token t, no atomics (pos_of_slot is a permutation of the rows, so every
// row of gy is written by exactly one slot); gout has the type OK, y / addend / gy / gaddend the type IK, gw and gaw are
// float32.  The dot products have a fixed summation order: fmaf over n = tid, tid + 256, ..., wave_sum, then the four
// wave partials as (0 + 1) + (2 + 3):
//   gy[pos[t][k]][:] = round_in(w[t][k] * gout[t][:])         (w == NULL: gout[t][:] itself)
//   gw[t][k]         = <y[pos[t][k]][:], gout[t][:]>          (gw == NULL: skipped)
//   gaddend[t][:]    = round_in(aw[t] * gout[t][:])           (gaddend == NULL: skipped; aw == NULL: gout[t][:] itself)
//   gaw[t]           = <addend[t][:], gout[t][:]>             (gaw == NULL: skipped)
// SPARSE: pos_of_slot is an injection of the kept slots into the rows; a slot with pos < 0 writes no row of gy (the
// caller zeroes gy) and gets gw = 0.  pos is the same for the whole workgroup, so the skip is uniform.
template <int IK, int OK, bool SPARSE = false>
__global__ __launch_bounds__(256) void combine_bwd_kernel(
    const void *__restrict__ gout_, const void *__restrict__ y_, const int32_t *__restrict__ pos_of_slot,
    const float *__restrict__ w, const void *__restrict__ addend_, const float *__restrict__ aw, void *__restrict__ gy_,
    float *__restrict__ gw, void *__restrict__ gaddend_, float *__restrict__ gaw, int T, int top_k, int N, int R)
{
    using EI = typename CombElem<IK>::type;
    using EO = typename CombElem<OK>::type;
    __shared__ float s_part[4];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EO *go = static_cast<const EO *>(gout_) + (size_t)t * N;
    for (int k = 0; k < top_k; ++k) {
        int p = pos_of_slot[(size_t)t * top_k + k];
        if (SPARSE && p < 0) {
            if (gw != nullptr && tid == 0) gw[(size_t)t * top_k + k] = 0.0f;
            continue;
        }
        p = p < 0 ? 0 : (p >= R ? R - 1 : p);
        const float wk = w != nullptr ? w[(size_t)t * top_k + k] : 1.0f;
        const EI *yr = static_cast<const EI *>(y_) + (size_t)p * N;
        EI *gyr = static_cast<EI *>(gy_) + (size_t)p * N;
        float dot = 0.0f;
        for (int n = tid; n < N; n += 256) {
            const float g = comb_widen<OK>(go[n]);
            gyr[n] = w != nullptr ? comb_round_product<IK>(wk, g) : comb_round<IK>(g);
            if (gw != nullptr) dot = fmaf(comb_widen<IK>(yr[n]), g, dot);
        }
        if (gw != nullptr) {
            dot = wave_sum(dot);
            if (lane == 0) s_part[wave] = dot;
            __syncthreads();
            if (tid == 0) gw[(size_t)t * top_k + k] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
            __syncthreads();
        }
    }
    if (gaddend_ == nullptr && gaw == nullptr) return;
    const float a = aw != nullptr ? aw[t] : 1.0f;
    const EI *ar = static_cast<const EI *>(addend_) + (size_t)t * N;       // read only for gaw (the host checks the pair)
    EI *gar = static_cast<EI *>(gaddend_) + (size_t)t * N;
    float dot = 0.0f;
    for (int n = tid; n < N; n += 256) {
        const float g = comb_widen<OK>(go[n]);
        if (gaddend_ != nullptr) gar[n] = aw != nullptr ? comb_round_product<IK>(a, g) : comb_round<IK>(g);
        if (gaw != nullptr) dot = fmaf(comb_widen<IK>(ar[n]), g, dot);
    }
    if (gaw != nullptr) {
        dot = wave_sum(dot);
        if (lane == 0) s_part[wave] = dot;
        __syncthreads();
        if (tid == 0) gaw[t] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    }
}

// One workgroup.  cnt[s][e] = rows source rank s sent for local expert e (received order: s major, e minor).
// gather[d] = received row feeding expert-major position d; scatter[r] = expert-major position of received row r.
__global__ __launch_bounds__(256) void regroup_index_kernel(
    const int32_t *__restrict__ cnt, int G, int EL, int32_t *__restrict__ tpe, int32_t *__restrict__ offs,
    int32_t *__restrict__ gather, int32_t *__restrict__ scatter)
{
    extern __shared__ int s_tab[];                 // src_off[G*EL], exp_off[EL*G]
    int *src_off = s_tab, *exp_off = s_tab + G * EL;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < G * EL; ++i) { src_off[i] = run; run += cnt[i]; }
        run = 0;
        for (int e = 0; e < EL; ++e) {
            offs[e] = run;
            int tot = 0;
            for (int s = 0; s < G; ++s) { exp_off[e * G + s] = run; run += cnt[s * EL + e]; tot += cnt[s * EL + e]; }
            tpe[e] = tot;
        }
    }
    __syncthreads();
    for (int seg = 0; seg < G * EL; ++seg) {
        const int s = seg / EL, e = seg - s * EL;
        const int c = cnt[seg], so = src_off[seg], eo = exp_off[e * G + s];
        for (int i = tid; i < c; i += 256) {
            gather[eo + i] = so + i;
            scatter[so + i] = eo + i;
        }
    }
}
