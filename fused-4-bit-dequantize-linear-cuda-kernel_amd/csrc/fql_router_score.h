// The scored router: what csrc/fql_router.h does for the softmax / top-k rule, for the routing rules of DeepSeek-V2 / V3,
// GLM-4.5, Kimi-K2 and Llama-4: sigmoid or softmax scores, an optional per-expert selection bias, group-limited selection
// and a scaling factor, in ONE launch, and the backward of that in one launch.
//
//   router_score_topk_fwd_kernel   logits [T][E] -> indices [T][top_k] int32, weights [T][top_k] float32 and, when asked
//                                  for, scores [T][E] float32 (the softmax, or the sigmoids).
//   router_score_topk_bwd_kernel   grad_weights [T][top_k] and / or grad_scores [T][E] -> grad_logits [T][E] in the logits'
//                                  type, rounded once.  The scores are recomputed from the logits; the bias and the groups
//                                  are not needed (the indices are saved) and the bias gets no gradient.
//
// Semantics:
//   scores       softmax: p_e = q_e / s, the bits of router_topk's probs.  sigmoid: s_e = 1 / (1 + expf(-l_e)), float32,
//                the accurate expf; it saturates to exactly 1.0f and 0.0f.
//   key          select_bias == NULL: the logit (both scorings are monotone in it, and two logits can round to one
//                score).  Otherwise key_e = score_e + bias_e, one float32 add (its operand is the result of a division:
//                nothing can be contracted into it).  A NaN key counts as -inf, so every id written is in [0, E).
//   groups       n_group > 1: group c holds the experts [c * E / n_group, (c + 1) * E / n_group).  Its score is the
//                largest (group_top == 1) or the sum of the two largest (group_top == 2; a one-member group: its one
//                value) of score_e + bias_e (bias 0 when NULL).  The topk_group best groups are chosen, ties to the
//                lower group id; experts outside them are NEVER selected (no 0.0 fill).
//   slots        slot j holds the j-th largest key among the allowed experts, ties (-0.0 == 0.0 included) to the lower id.
//   weights      always from the unbiased scores.  softmax: (q_{e_j} / sum_i q_{e_i}) * scale renormalised, else
//                (q_{e_j} / s) * scale.  sigmoid: (s_{e_j} / (sum_i s_{e_i} + 1e-20f)) * scale renormalised, else
//                s_{e_j} * scale.  Slot sums are the butterfly over the group's first 8 lanes.
//   non-finite   a row with a non-finite logit: NaN weights, NaN scores, indices 0 .. top_k-1, a NaN row of grad_logits.
//
// Thread mapping: that of fql_router.h (G lanes own a token, lane g the experts g and g + 64; xor butterflies only; no
// LDS, no atomics).  The group stage runs one butterfly per expert group that carries the pair (largest, second
// largest) of the group's members: a lane contributes the members it holds (none, one or both of its experts, so a
// group may be any width, be split across a lane's two experts or straddle the wave's halves), max / min are exact and
// commutative, so every lane of the token ends with the same pair.  Each lane then ranks the at most 8 group scores in
// registers and masks its own experts.
#pragma once
#include "fql_router.h"

#define ROUTER_MAX_GROUPS 8

__device__ __forceinline__ float router_sigmoid(float l) { return 1.0f / (1.0f + expf(-l)); }
__device__ __forceinline__ float router_no_nan(float v) { return v != v ? -INFINITY : v; }

// The value of expert e (clamped by the caller) from the lane of the token's group that owns it
template <int G, int NPL>
__device__ __forceinline__ float router_fetch(const float (&v)[NPL], int base, int e)
{
    float r = __shfl(v[0], base + (e & (G - 1)), 64);
    if constexpr (NPL == 2) {
        const float r1 = __shfl(v[1], base + (e & (G - 1)), 64);
        if (e >= G) r = r1;
    }
    return r;
}

// grid: ceil(T / (256 / G)) workgroups of 256 threads
template <int G, int NPL>
__global__ __launch_bounds__(ROUTER_THREADS) void router_score_topk_fwd_kernel(
    const void *__restrict__ logits, int kind, int T, int E, int top_k, int scoring, const float *__restrict__ select_bias,
    int n_group, int topk_group, int group_top, int renormalize, float scale, int32_t *__restrict__ indices,
    float *__restrict__ weights, float *__restrict__ scores)
{
    constexpr int KG = G < ROUTER_MAX_TOPK ? G : ROUTER_MAX_TOPK;      // lanes of a group that can hold a slot
    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1);
    const int base = lane - g;
    const long long t = ((long long)blockIdx.x * (ROUTER_THREADS / 64) + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = t < T;
    const size_t row = (size_t)(live ? t : 0) * E;
    const RouterRow<G, NPL> r = router_row<G, NPL>(logits, kind, row, E, g, live);

    // sc: the score; num: what a slot's weight is made of (q or the sigmoid); key: what the selection orders by;
    // gv: what a group's score is made of
    float sc[NPL], num[NPL], key[NPL], gv[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int e = g + i * G;
        const bool have = e < E;
        num[i] = scoring ? (have ? router_sigmoid(r.l[i]) : 0.0f) : r.q[i];
        sc[i] = scoring ? num[i] : r.q[i] / r.s;
        gv[i] = sc[i];
        key[i] = r.l[i];
        if (select_bias != nullptr) {                                  // (uniform over the grid)
            gv[i] = router_no_nan(sc[i] + (have ? select_bias[e] : 0.0f));
            key[i] = gv[i];
        }
    }

    // the group stage: which of this lane's experts may be selected
    unsigned allowed = (1u << NPL) - 1u;
    if (n_group > 1) {
        const int per = E / n_group;
        int mine[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) mine[i] = g + i * G < E ? (g + i * G) / per : -1;
        float gs[ROUTER_MAX_GROUPS];
#pragma unroll
        for (int c = 0; c < ROUTER_MAX_GROUPS; ++c) {
            gs[c] = -INFINITY;
            if (c < n_group) {
                float m1 = -INFINITY, m2 = -INFINITY;                  // the largest and the second largest so far
#pragma unroll
                for (int i = 0; i < NPL; ++i) {
                    if (mine[i] == c) {
                        m2 = fmaxf(m2, fminf(m1, gv[i]));
                        m1 = fmaxf(m1, gv[i]);
                    }
                }
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) {
                    const float o1 = __shfl_xor(m1, o, 64);
                    const float o2 = __shfl_xor(m2, o, 64);
                    m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
                    m1 = fmaxf(m1, o1);
                }
                gs[c] = router_no_nan((group_top == 2 && per > 1) ? m1 + m2 : m1);
            }
        }
        // group c is chosen when fewer than topk_group groups come before it in the order (score, lower id first)
        unsigned chosen = 0;
#pragma unroll
        for (int c = 0; c < ROUTER_MAX_GROUPS; ++c) {
            int before = 0;
#pragma unroll
            for (int d = 0; d < ROUTER_MAX_GROUPS; ++d)
                if (d != c) before += (d < n_group) && (gs[d] > gs[c] || (gs[d] == gs[c] && d < c));
            if (c < n_group && before < topk_group) chosen |= 1u << c;
        }
        allowed = 0;
#pragma unroll
        for (int i = 0; i < NPL; ++i) if (mine[i] >= 0 && ((chosen >> mine[i]) & 1u)) allowed |= 1u << i;
    }

    // top_k rounds of arg-max over what is left and allowed, key (value, lower id first); slot j stays in lane j
    unsigned taken = ~allowed;
    int slot_e = 0;
    for (int j = 0; j < top_k; ++j) {
        float bv = -INFINITY;
        int be = 0x7FFFFFFF;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int e = g + i * G;
            if (e < E && !((taken >> i) & 1u) && (key[i] > bv || (key[i] == bv && e < be))) {
                bv = key[i];
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
        if (g == j) slot_e = be;
    }
    slot_e = slot_e < 0 ? 0 : (slot_e >= E ? E - 1 : slot_e);          // (a NaN logit is never picked: a bad row, ids g below)
    const float fetched = router_fetch<G, NPL>(num, base, slot_e);     // the owner's bits of q or of the sigmoid
    const float ns = g < top_k ? fetched : 0.0f;                       // (lanes past KG hold no slot and store nothing)
    float w;
    if (scoring) w = renormalize ? ns / (group_sum<KG>(ns) + 1e-20f) : ns;
    else w = ns / (renormalize ? group_sum<KG>(ns) : r.s);
    w *= scale;
    const float nan = __uint_as_float(0x7FC00000u);
    if (live && g < top_k) {
        indices[(size_t)t * top_k + g] = r.bad ? g : slot_e;
        weights[(size_t)t * top_k + g] = r.bad ? nan : w;
    }
    if (scores != nullptr && live) {
#pragma unroll
        for (int i = 0; i < NPL; ++i)
            if (g + i * G < E) scores[row + g + i * G] = r.bad ? nan : sc[i];
    }
}

// Backward, the same mapping.  With g_j = scale * grad_weights_j, gs = grad_scores (either may be NULL):
//   softmax      the formulas of router_topk_bwd_kernel with g; grad_scores adds p_e * (gs_e - sum_e' p_e' gs_e').
//   sigmoid      d_e = s_e * (1 - s_e), 1 - s_e taken as the sigmoid of -l_e (no cancellation for large l_e);
//                renormalised, D = sum_i s_{e_i} + 1e-20f, u_i = s_{e_i} / D: dl_{e_j} = d_{e_j} * (g_j - sum_i u_i g_i) / D;
//                otherwise dl_{e_j} = d_{e_j} * g_j; exactly 0.0 for an expert no slot names; grad_scores adds d_e * gs_e.
// Ids outside [0, E) are clamped, as the plan kernel does.
template <int G, int NPL>
__global__ __launch_bounds__(ROUTER_THREADS) void router_score_topk_bwd_kernel(
    const void *__restrict__ logits, int kind, const int32_t *__restrict__ indices, const float *__restrict__ grad_weights,
    const float *__restrict__ grad_scores, void *__restrict__ grad_logits, int T, int E, int top_k, int scoring,
    int renormalize, float scale)
{
    constexpr int KG = G < ROUTER_MAX_TOPK ? G : ROUTER_MAX_TOPK;
    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1);
    const int base = lane - g;
    const long long t = ((long long)blockIdx.x * (ROUTER_THREADS / 64) + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = t < T;
    const size_t row = (size_t)(live ? t : 0) * E;
    const RouterRow<G, NPL> r = router_row<G, NPL>(logits, kind, row, E, g, live);

    float num[NPL], dsig[NPL], d[NPL];                                 // q or the sigmoid; s (1 - s); the result
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const bool have = g + i * G < E;
        num[i] = scoring ? (have ? router_sigmoid(r.l[i]) : 0.0f) : r.q[i];
        dsig[i] = (scoring && have) ? num[i] * router_sigmoid(-r.l[i]) : 0.0f;
        d[i] = 0.0f;
    }

    if (grad_weights != nullptr) {                                     // (uniform over the grid)
        int se = 0;
        float sg = 0.0f;
        if (live && g < top_k) {
            se = indices[(size_t)t * top_k + g];
            se = se < 0 ? 0 : (se >= E ? E - 1 : se);
            sg = scale * grad_weights[(size_t)t * top_k + g];
        }
        const float fetched = router_fetch<G, NPL>(num, base, se);
        const float ns = (live && g < top_k) ? fetched : 0.0f;
        float dot, term;
        if (scoring) {
            const float D = group_sum<KG>(ns) + 1e-20f;
            const float u = ns / D;
            dot = __shfl(group_sum<KG>(u * sg), base, 64);
            term = renormalize ? (sg - dot) / D : sg;
        } else {
            const float den = renormalize ? group_sum<KG>(ns) : r.s;
            const float w = ns / den;
            dot = __shfl(group_sum<KG>(w * sg), base, 64);             // sum_i w_i g_i, to every lane of the group
            term = renormalize ? w * (sg - dot) : sg;                  // what slot g hands its expert
        }
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
        for (int i = 0; i < NPL; ++i) {
            if (scoring) d[i] = dsig[i] * acc[i];
            else d[i] = renormalize ? acc[i] : (r.q[i] / r.s) * (acc[i] - dot);
        }
    }
    if (grad_scores != nullptr) {
        float gp[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) gp[i] = (live && g + i * G < E) ? grad_scores[row + g + i * G] : 0.0f;
        if (scoring) {
#pragma unroll
            for (int i = 0; i < NPL; ++i) d[i] += dsig[i] * gp[i];
        } else {
            float part = 0.0f;
#pragma unroll
            for (int i = 0; i < NPL; ++i) part = __fmaf_rn(r.q[i] / r.s, gp[i], part);   // (router_topk_bwd_kernel's bits)
            const float mean = group_sum<G>(part);
#pragma unroll
            for (int i = 0; i < NPL; ++i) d[i] += (r.q[i] / r.s) * (gp[i] - mean);
        }
    }
    if (live) {
        const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
        for (int i = 0; i < NPL; ++i)
            if (g + i * G < E) router_store(grad_logits, kind, row + g + i * G, r.bad ? nan : d[i]);
    }
}
