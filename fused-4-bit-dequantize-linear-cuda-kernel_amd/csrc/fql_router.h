// The router in front of fql_route_plan_i32: softmax over a token's E logits, the top_k experts and their routing
// weights in ONE launch (what torch does as softmax -> topk -> sum -> div -> to(int32)), and its backward.
//
//   router_topk_fwd_kernel   logits [T][E] (float32 / float16 / bfloat16, 16-bit values widened exactly) ->
//                            indices [T][top_k] int32 (what route_plan_kernel reads), weights [T][top_k] float32 (what
//                            combine_kernel reads) and, when asked for, probs [T][E] float32 (the full softmax).
//   router_topk_bwd_kernel   grad_weights [T][top_k] and / or grad_probs [T][E] -> grad_logits [T][E] in the logits'
//                            type, rounded once.  The row's softmax is recomputed from the logits: nothing of size
//                            [T][E] is kept between the two.
//
// Semantics:
//   selection    on the LOGITS (two distinct float32 logits can round to one probability): slot j holds the j-th largest,
//                ties (-0.0 == 0.0 included) go to the lower expert id: torch.sort(-logits, stable=True).indices[:, :k].
//   softmax      q_e = expf(l_e - m), m the row maximum, s = sum_e q_e, p_e = q_e / s: float32, the accurate expf.
//   weights      renormalize: w_j = q_{e_j} / sum_i q_{e_i} (= p_{e_j} / sum_i p_{e_i} without the two roundings of the
//                division by s: all-equal logits give exactly 1 / top_k); otherwise w_j = q_{e_j} / s, the bits of
//                probs[t][e_j].
//   non-finite   a row with a NaN or an infinite logit gets NaN weights, NaN probs and indices 0 .. top_k-1 (always
//                valid ids: the plan kernel behind it is safe), a NaN row of grad_logits: the project's convention, a
//                non-finite activation makes its whole output row NaN.  This holds with both gradients NULL as well.
//   rows         a token's results depend on its own row alone: not on T, not on its neighbours in the wave.
//
// Thread mapping: a group of G = min(64, next_pow2(E)) lanes owns one token, lane g of the group the experts g and
// (E > 64) g + 64.  A wave holds 64 / G tokens, a workgroup of four waves 256 / G.  Every reduction is an xor
// butterfly inside the group (pairwise, the same tree wherever the group sits in the wave); the top_k rounds of
// arg-max carry (value, id) through the same butterfly; slot j lives in lane j of the group.  No LDS, no atomics, plain
// vector loads and stores: the same inputs give the same bits.
#pragma once
#include "fql_common.h"

#define ROUTER_THREADS 256
#define ROUTER_MAX_EXPERTS 128         // = ROUTE_MAX_EXPERTS of the plan kernel behind it
#define ROUTER_MAX_TOPK 8              // the slots of a token live in the first 8 lanes of its group

__device__ __forceinline__ float router_load(const void *p, int kind, size_t i)
{
    if (kind == 0) return reinterpret_cast<const float *>(p)[i];
    const unsigned short u = reinterpret_cast<const unsigned short *>(p)[i];
    if (kind == 1) {
        _Float16 h;
        __builtin_memcpy(&h, &u, 2);
        return (float)h;
    }
    return __uint_as_float((uint32_t)u << 16);
}
__device__ __forceinline__ void router_store(void *p, int kind, size_t i, float v)
{
    if (kind == 0) reinterpret_cast<float *>(p)[i] = v;
    else reinterpret_cast<unsigned short *>(p)[i] = (kind == 1) ? f32_to_f16_bits(v) : f32_to_bf16_bits(v);
}

// Butterfly reductions over the W lanes of an aligned group (W a power of two): every lane of the group ends with the
// same value, and the tree is the same for every group of a wave.
template <int W>
__device__ __forceinline__ float group_sum(float v)
{
    if constexpr (W == 64) return wave_sum(v);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int W>
__device__ __forceinline__ float group_max(float v)
{
    if constexpr (W == 64) return wave_max(v);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int W>
__device__ __forceinline__ int group_or(int v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// One token's row as its group holds it: l / q of the experts g + i * G (0 past E), the row maximum m, s = sum q and
// whether the row has a non-finite logit.  Lanes of a token past T load nothing and carry zeros through the shuffles.
template <int G, int NPL>
struct RouterRow {
    float l[NPL], q[NPL], m, s;
    bool bad;
};
template <int G, int NPL>
__device__ __forceinline__ RouterRow<G, NPL> router_row(const void *logits, int kind, size_t row, int E, int g, bool live)
{
    RouterRow<G, NPL> r;
    int nonfinite = 0;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int e = g + i * G;
        r.l[i] = 0.0f;
        if (live && e < E) {
            r.l[i] = router_load(logits, kind, row + e);
            nonfinite |= (__float_as_uint(r.l[i]) & 0x7F800000u) == 0x7F800000u;
            mx = fmaxf(mx, r.l[i]);
        }
    }
    r.bad = group_or<G>(nonfinite) != 0;
    r.m = group_max<G>(mx);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        r.q[i] = (live && g + i * G < E) ? expf(r.l[i] - r.m) : 0.0f;
        part += r.q[i];
    }
    r.s = group_sum<G>(part);
    return r;
}

// grid: ceil(T / (256 / G)) workgroups of 256 threads
template <int G, int NPL>
__global__ __launch_bounds__(ROUTER_THREADS) void router_topk_fwd_kernel(
    const void *__restrict__ logits, int kind, int T, int E, int top_k, int renormalize, int32_t *__restrict__ indices,
    float *__restrict__ weights, float *__restrict__ probs)
{
    constexpr int KG = G < ROUTER_MAX_TOPK ? G : ROUTER_MAX_TOPK;      // lanes of a group that can hold a slot
    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1);
    const long long t = ((long long)blockIdx.x * (ROUTER_THREADS / 64) + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = t < T;
    const size_t row = (size_t)(live ? t : 0) * E;
    const RouterRow<G, NPL> r = router_row<G, NPL>(logits, kind, row, E, g, live);

    // top_k rounds of arg-max over what is left, key (value, lower id first); slot j stays in lane j
    unsigned taken = 0;
    float slot_v = 0.0f;
    int slot_e = 0;
    for (int j = 0; j < top_k; ++j) {
        float bv = -INFINITY;
        int be = 0x7FFFFFFF;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int e = g + i * G;
            if (e < E && !((taken >> i) & 1u) && (r.l[i] > bv || (r.l[i] == bv && e < be))) {
                bv = r.l[i];
                be = e;
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oe = __shfl_xor(be, o, 64);
            if (ov > bv || (ov == bv && oe < be)) {
                bv = ov;
                be = oe;
            }
        }
#pragma unroll
        for (int i = 0; i < NPL; ++i) if (g + i * G == be) taken |= 1u << i;
        if (g == j) {
            slot_v = bv;
            slot_e = be;
        }
    }
    const float qs = g < top_k ? expf(slot_v - r.m) : 0.0f;            // the bits of the owner's q: same inputs
    const float den = renormalize ? group_sum<KG>(qs) : r.s;           // (lanes past KG hold no slot and store nothing)
    const float nan = __uint_as_float(0x7FC00000u);
    if (live && g < top_k) {
        indices[(size_t)t * top_k + g] = r.bad ? g : slot_e;
        weights[(size_t)t * top_k + g] = r.bad ? nan : qs / den;
    }
    if (probs != nullptr && live) {
#pragma unroll
        for (int i = 0; i < NPL; ++i)
            if (g + i * G < E) probs[row + g + i * G] = r.bad ? nan : r.q[i] / r.s;
    }
}

// Backward, the same mapping.  With g = grad_weights, gp = grad_probs (either may be NULL) and w, p recomputed:
//   renormalize:  dl_{e_j} = w_j * (g_j - sum_i w_i g_i), exactly 0.0 for an expert no slot names
//   otherwise:    dl_e     = p_e * ([e selected] g_e - sum_j p_{e_j} g_j)
//   grad_probs:   dl_e    += p_e * (gp_e - sum_e' p_e' gp_e')
// Sums over the slots are butterflies over the group's first 8 lanes, sums over the experts over the whole group; the
// slot terms reach their experts' lanes in slot order.  Ids outside [0, E) are clamped, as the plan kernel does.
template <int G, int NPL>
__global__ __launch_bounds__(ROUTER_THREADS) void router_topk_bwd_kernel(
    const void *__restrict__ logits, int kind, const int32_t *__restrict__ indices, const float *__restrict__ grad_weights,
    const float *__restrict__ grad_probs, void *__restrict__ grad_logits, int T, int E, int top_k, int renormalize)
{
    constexpr int KG = G < ROUTER_MAX_TOPK ? G : ROUTER_MAX_TOPK;
    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1);
    const int base = lane - g;
    const long long t = ((long long)blockIdx.x * (ROUTER_THREADS / 64) + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = t < T;
    const size_t row = (size_t)(live ? t : 0) * E;
    const RouterRow<G, NPL> r = router_row<G, NPL>(logits, kind, row, E, g, live);

    float d[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) d[i] = 0.0f;

    if (grad_weights != nullptr) {                                     // (uniform over the grid)
        int se = 0;
        float sg = 0.0f;
        if (live && g < top_k) {
            se = indices[(size_t)t * top_k + g];
            se = se < 0 ? 0 : (se >= E ? E - 1 : se);
            sg = grad_weights[(size_t)t * top_k + g];
        }
        // the slot's logit from the lane that owns its expert
        float lv = __shfl(r.l[0], base + (se & (G - 1)), 64);
        if constexpr (NPL == 2) {
            const float l1 = __shfl(r.l[1], base + (se & (G - 1)), 64);
            if (se >= G) lv = l1;
        }
        const float qs = (live && g < top_k) ? expf(lv - r.m) : 0.0f;
        const float den = renormalize ? group_sum<KG>(qs) : r.s;
        const float w = (live && g < top_k) ? qs / den : 0.0f;
        const float dot = __shfl(group_sum<KG>(w * sg), base, 64);     // sum_i w_i g_i, to every lane of the group
        const float term = renormalize ? w * (sg - dot) : sg;          // what slot g hands its expert
        float acc[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) acc[i] = 0.0f;
        for (int j = 0; j < top_k; ++j) {
            const int ej = __shfl(se, base + j, 64);
            const float tj = __shfl(term, base + j, 64);
#pragma unroll
            for (int i = 0; i < NPL; ++i) if (g + i * G == ej) acc[i] += tj;
        }
#pragma unroll
        for (int i = 0; i < NPL; ++i) d[i] = renormalize ? acc[i] : (r.q[i] / r.s) * (acc[i] - dot);
    }
    if (grad_probs != nullptr) {
        float gp[NPL], part = 0.0f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            gp[i] = (live && g + i * G < E) ? grad_probs[row + g + i * G] : 0.0f;
            part += (r.q[i] / r.s) * gp[i];
        }
        const float mean = group_sum<G>(part);
#pragma unroll
        for (int i = 0; i < NPL; ++i) d[i] += (r.q[i] / r.s) * (gp[i] - mean);
    }
    if (live) {
        const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
        for (int i = 0; i < NPL; ++i)
            if (g + i * G < E) router_store(grad_logits, kind, row + g + i * G, r.bad ? nan : d[i]);
    }
}
