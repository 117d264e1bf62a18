// Segmented (per-expert, ragged) low-rank adapter kernels: float32 VALU FMAs, float32 accumulators; the streamed [T][C]
// operand is float32, float16 or bfloat16 (below, "Element types").
//
// For the rows t of expert e (rows [lo_e, hi_e), from tokens_per_expert / input_offsets on the device; one segment of
// all T rows when the table is NULL), with rank R and a weight W_e stored [E][R][C] (FQL_LORA_RC) or [E][C][R]
// (FQL_LORA_CR):
//
//   shrink  out[t][j] = scale * sum_c in[t][c] * W_e[j][c]                   [T][C] -> [T][R]
//   expand  out[t][c] = in[t][c] + scale * sum_j V[t][j] * W_e[c][j]         [T][R] -> [T][C]   (in == out allowed)
//   grad    D_e[c][j] = scale * sum_{t in e} P[t][c] * V[t][j]               -> [E][C][R] or [E][R][C]
//
// At R <= 64 all three are bandwidth-bound (2 R FLOP per streamed float), so the design is: stream the [T][C] operand
// once with the widest load its alignment allows (VEC = 4 / 2 / 1 floats), keep 64 float32 accumulators per lane, and
// re-read the small weight from L2.
//
// Determinism.  No atomics; every output element is written once by one lane, after a reduction whose order depends
// only on the row's position inside its expert (never on T, E or the tile the row shares):
//   * shrink: lane l of the workgroup sums the VEC-column groups l, l + 512, ... of its rows; the 64 partial sums of
//     a wave are reduced by a fixed butterfly (each step halves the values a lane keeps), then the 8 waves in order.
//   * expand: one lane per output element, j ascending.
//   * grad: wave w of 8 sums the rows lo_e + w, lo_e + w + 8, ... in ascending order; the 8 partials are added by a
//     fixed tree through LDS.  An expert's result is therefore the same bits whether it is computed in a grouped call
//     or alone with E = 1.
// Rows covered by no expert: shrink writes zeros, expand copies `in` (zeros when in == NULL; nothing when in place).
//
// Element types (DT / DI / DO = FQL_DTYPE_F32 / _F16 / _BF16): the [T][C] operand -- `in` of shrink, `P` of grad, `in` and
// `out` of expand, each on its own -- may be 16-bit.  A 16-bit element is widened in registers on load (exact) and a
// 16-bit output is rounded once, to nearest even, on store (the helpers of fql_common.h, as Tensor.to(dtype) rounds).
// Only the load and the store differ: VEC counts ELEMENTS, so the column-to-lane mapping, the tiles and every reduction
// order are those of the float32 kernel at the same VEC, and a 16-bit call returns the bits of the float32 call on the
// widened operand (rounded once, for expand).  [T][r] tensors, adapter weights and their gradients are always float32.
//
// GATE (shrink and grad; any element type): the streamed operand is the [T][2C] gate|up tensor of a gated FFN expert and the value that
// enters the sums is h[t][c] = act_silu_mul(gate_up[t][c], gate_up[t][C + c]) -- the function the down GEMM's
// activation pre-pass calls (fql_common.h), so the down adapter sees the h the INT4 GEMM consumed and the [T][C]
// hidden activation is never written.  Only the operand load differs: tiles, lanes and reduction orders are the same
// code, and every promise above holds for the gated variants.
//
// swiglu_bwd_kernel: the elementwise backward of h = silu(g) * u, one streaming pass over [T][2F] + [T][F] -> [T][2F].
//
// Activation kinds other than silu (FQL_ACT_GELU_TANH, FQL_ACT_SWIGLU_CLAMP; instantiated in fql_glu.hip only): the gated
// shrink and grad kernels take one more argument, ACT = GluArgs -- the kind and its two floats, wave-uniform -- and h comes
// from act_glu_mul of fql_common.h, the function the pre-pass calls for the same kind.  The argument is a template
// parameter pack that is empty for every kernel of before, which therefore keeps its argument list and its code; only the
// operand load differs.  glu_bwd_kernel is swiglu_bwd_typed_kernel with (dg, du) = act_glu_grad.
#pragma once
#include "fql_common.h"

#define FQL_LORA_SHRINK_THREADS 512
#define FQL_LORA_EXPAND_THREADS 256
#define FQL_LORA_EXPAND_ROWS 8
#define FQL_LORA_GRAD_THREADS 512
#define FQL_LORA_COVER_ROWS 64      // rows per coverage workgroup (rows no expert owns)

namespace lora {

template <int VEC> struct vec_t;
template <> struct vec_t<4> { typedef float4 type; };
template <> struct vec_t<2> { typedef float2 type; };
template <> struct vec_t<1> { typedef float type; };

template <int VEC>
__device__ __forceinline__ void load_vec(const float *p, float (&v)[VEC])
{
    const typename vec_t<VEC>::type t = *reinterpret_cast<const typename vec_t<VEC>::type *>(p);
    if constexpr (VEC == 4) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else if constexpr (VEC == 2) { v[0] = t.x; v[1] = t.y; }
    else { v[0] = t; }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *p, const float (&v)[VEC])
{
    typename vec_t<VEC>::type t;
    if constexpr (VEC == 4) { t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; }
    else if constexpr (VEC == 2) { t.x = v[0]; t.y = v[1]; }
    else { t = v[0]; }
    *reinterpret_cast<typename vec_t<VEC>::type *>(p) = t;
}

// 16-bit elements: VEC of them in one load (8 / 4 / 2 bytes), widened / rounded in registers.
template <int DT>
__device__ __forceinline__ float widen16(unsigned short h)
{
    if constexpr (DT == 1) { _Float16 f; __builtin_memcpy(&f, &h, 2); return (float)f; }
    else return __uint_as_float((uint32_t)h << 16);
}
template <int DT>
__device__ __forceinline__ unsigned short round16(float f)
{
    if constexpr (DT == 1) {
        // the float32 value first, in a register of its own: left to itself the compiler folds the preceding fma and this
        // conversion into one v_fma_mixlo_f16, which rounds the exact fma once to float16 -- not the float32 result
        // rounded to float16 that Tensor.to(float16) gives (the two differ in double-rounding cases)
        asm volatile("" : "+v"(f));
        return f32_to_f16_bits(f);
    } else return f32_to_bf16_bits(f);
}

// VEC elements of type DT at element index i of `base` -> float32
template <int VEC, int DT>
__device__ __forceinline__ void load_elems(const void *base, size_t i, float (&v)[VEC])
{
    if constexpr (DT == 0) load_vec<VEC>(reinterpret_cast<const float *>(base) + i, v);
    else {
        const unsigned short *p = reinterpret_cast<const unsigned short *>(base) + i;
        if constexpr (VEC == 4) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p);
            v[0] = widen16<DT>((unsigned short)(t.x & 0xFFFFu)); v[1] = widen16<DT>((unsigned short)(t.x >> 16));
            v[2] = widen16<DT>((unsigned short)(t.y & 0xFFFFu)); v[3] = widen16<DT>((unsigned short)(t.y >> 16));
        } else if constexpr (VEC == 2) {
            const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
            v[0] = widen16<DT>((unsigned short)(t & 0xFFFFu)); v[1] = widen16<DT>((unsigned short)(t >> 16));
        } else { v[0] = widen16<DT>(*p); }
    }
}

// float32 -> VEC elements of type DT at element index i of `base` (16-bit: one rounding to nearest even)
template <int VEC, int DT>
__device__ __forceinline__ void store_elems(void *base, size_t i, const float (&v)[VEC])
{
    if constexpr (DT == 0) store_vec<VEC>(reinterpret_cast<float *>(base) + i, v);
    else {
        unsigned short *p = reinterpret_cast<unsigned short *>(base) + i;
        if constexpr (VEC == 4) {
            *reinterpret_cast<uint2 *>(p) = make_uint2((uint32_t)round16<DT>(v[0]) | ((uint32_t)round16<DT>(v[1]) << 16),
                                                       (uint32_t)round16<DT>(v[2]) | ((uint32_t)round16<DT>(v[3]) << 16));
        } else if constexpr (VEC == 2) {
            *reinterpret_cast<uint32_t *>(p) = (uint32_t)round16<DT>(v[0]) | ((uint32_t)round16<DT>(v[1]) << 16);
        } else { *p = round16<DT>(v[0]); }
    }
}

// VEC operand values of row t at column c: the elements of a [T][C] tensor, or with GATE the hidden activation formed
// from the gate half (columns [0, C)) and the up half ([C, 2C)) of row t of a [T][2C] gate|up tensor (16-bit halves are
// widened first: h is the float32 act_silu_mul of the widened values).
template <int VEC, bool GATE, int DT = 0>
__device__ __forceinline__ void load_operand(const void *pv, int t, int C, int c, float (&v)[VEC])
{
    if constexpr (GATE) {
        float g[VEC], u[VEC];
        load_elems<VEC, DT>(pv, (size_t)t * 2 * C + c, g);
        load_elems<VEC, DT>(pv, (size_t)t * 2 * C + C + c, u);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = act_silu_mul(g[i], u[i]);
    } else {
        load_elems<VEC, DT>(pv, (size_t)t * C + c, v);
    }
}

// ... and for an activation kind other than silu (GATE only): h = act_glu_mul(kind, alpha, limit, g, u).
struct GluArgs { int kind; float alpha, limit; };
template <int VEC, bool GATE, int DT = 0>
__device__ __forceinline__ void load_operand(const void *pv, int t, int C, int c, float (&v)[VEC], GluArgs act)
{
    static_assert(GATE, "an activation kind needs a gate|up row");
    float g[VEC], u[VEC];
    load_elems<VEC, DT>(pv, (size_t)t * 2 * C + c, g);
    load_elems<VEC, DT>(pv, (size_t)t * 2 * C + C + c, u);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = act_glu_mul(act.kind, act.alpha, act.limit, g[i], u[i]);
}

// Rows [lo, hi) of expert e, clamped into [0, T) (a table that points outside the tensor never reaches memory).
__device__ __forceinline__ void expert_rows(const int32_t *tpe, const int32_t *offs, int e, int T, int &lo, int &hi)
{
    const int cnt = tpe[e], off = offs[e];
    lo = min(max(off, 0), T);
    hi = cnt > 0 ? (int)min((long long)off + cnt, (long long)T) : lo;
    hi = max(hi, lo);
}

// Tile slot b -> (rows [row0, row0 + n) of one expert).  Experts are dealt ceil(count / TM) consecutive slots in
// order; slots past the last tile return false.  The scan is wave-uniform (scalar loads of the table).
template <int TM>
__device__ __forceinline__ bool tile_rows(const int32_t *tpe, const int32_t *offs, int E, int T, int b, int &e_out,
                                          int &row0, int &n)
{
    if (tpe == nullptr) {
        e_out = 0;
        row0 = b * TM;
        n = min(TM, T - row0);
        return row0 < T;
    }
    int acc = 0;
    for (int e = 0; e < E; ++e) {
        int lo, hi;
        expert_rows(tpe, offs, e, T, lo, hi);
        const int tiles = (hi - lo + TM - 1) / TM;
        if (b < acc + tiles) {
            e_out = e;
            row0 = lo + (b - acc) * TM;
            n = min(TM, hi - row0);
            return true;
        }
        acc += tiles;
    }
    return false;
}

// Coverage workgroup: flag[i] = 1 if row r0 + i belongs to some expert.  All writers store the same value.
__device__ __forceinline__ void cover_flags(const int32_t *tpe, const int32_t *offs, int E, int T, int r0, int *flag)
{
    for (int i = threadIdx.x; i < FQL_LORA_COVER_ROWS; i += blockDim.x) flag[i] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        int lo, hi;
        expert_rows(tpe, offs, e, T, lo, hi);
        const int a = max(lo, r0), z = min(hi, r0 + FQL_LORA_COVER_ROWS);
        for (int r = a; r < z; ++r) flag[r - r0] = 1;
    }
    __syncthreads();
}

// ---- shrink: out[t][0:R] = scale * in[t][:] . W_e^T.  One workgroup = TM = 64 / R rows of one expert, 512 lanes
//      across the columns; grid = tile slots (+ coverage workgroups when there is a table).  GATE: `in` is [T][2C].
template <int R, bool CR, int VEC, bool GATE, int DT = 0, typename... ACT>
__global__ __launch_bounds__(FQL_LORA_SHRINK_THREADS) void lora_shrink_kernel(
    const void *__restrict__ in, const float *__restrict__ w, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, float *__restrict__ out, int E, int T, int C, float scale, int slots, ACT... act)
{
    constexpr int TM = 64 / R;
    constexpr int NW = FQL_LORA_SHRINK_THREADS / FQL_WAVE;
    __shared__ float red[NW][64];
    __shared__ int flag[FQL_LORA_COVER_ROWS];
    if ((int)blockIdx.x >= slots) {                              // rows no expert owns: zeros
        const int r0 = ((int)blockIdx.x - slots) * FQL_LORA_COVER_ROWS;
        cover_flags(tpe, offs, E, T, r0, flag);
        for (int i = threadIdx.x; i < FQL_LORA_COVER_ROWS * R; i += blockDim.x) {
            const int t = r0 + i / R;
            if (t < T && !flag[i / R]) out[(size_t)t * R + i % R] = 0.f;
        }
        return;
    }
    int e, row0, n;
    if (!tile_rows<TM>(tpe, offs, E, T, (int)blockIdx.x, e, row0, n)) return;
    const float *we = w + (size_t)e * R * C;

    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
    const int nq = C / VEC;
    for (int q = threadIdx.x; q < nq; q += FQL_LORA_SHRINK_THREADS) {
        const int c = q * VEC;
        float x[TM][VEC];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i < n) load_operand<VEC, GATE, DT>(in, row0 + i, C, c, x[i], act...);
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) x[i][v] = 0.f;
            }
        }
        if constexpr (!CR) {                                     // W_e[j][c .. c + VEC)
#pragma unroll
            for (int j = 0; j < R; ++j) {
                float wv[VEC];
                load_vec<VEC>(we + (size_t)j * C + c, wv);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[i * R + j] = fmaf(x[i][v], wv[v], acc[i * R + j]);
            }
        } else {                                                 // W_e[c + v][0 .. R)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
#pragma unroll
                for (int j = 0; j < R; j += 4) {
                    float wv[4];
                    load_vec<4>(we + (size_t)(c + v) * R + j, wv);
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) acc[i * R + j + jj] = fmaf(x[i][v], wv[jj], acc[i * R + j + jj]);
                }
        }
    }
    // wave butterfly: at the step of width h, a lane keeps the half of its values selected by (lane & h) and adds the
    // partner's copy of that half; after 6 steps lane l holds the wave's sum of value l.
    const int lane = threadIdx.x & (FQL_WAVE - 1);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const bool up = (lane & h) != 0;
#pragma unroll
        for (int k = 0; k < h; ++k) {
            const float keep = up ? acc[k + h] : acc[k];
            const float send = up ? acc[k] : acc[k + h];
            acc[k] = keep + __shfl_xor(send, h, FQL_WAVE);
        }
    }
    red[threadIdx.x / FQL_WAVE][lane] = acc[0];
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = red[0][lane];
#pragma unroll
        for (int k = 1; k < NW; ++k) s += red[k][lane];
        const int i = lane / R, j = lane % R;
        if (i < n) out[(size_t)(row0 + i) * R + j] = scale * s;
    }
}

// ---- expand: out[t][c] = in[t][c] + scale * V[t][0:R] . W_e[c][0:R].  One workgroup = up to 8 rows of one expert x
//      256 * VEC columns (grid.y); V of the tile is staged in LDS and read as broadcasts.
template <int R, bool CR, int VEC, int DI = 0, int DO = 0>
__global__ __launch_bounds__(FQL_LORA_EXPAND_THREADS) void lora_expand_kernel(
    const float *__restrict__ V, const float *__restrict__ w, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, const void *in, void *out, int E, int T, int C, float scale, int slots)
{
    constexpr int TM = FQL_LORA_EXPAND_ROWS;
    __shared__ __attribute__((aligned(16))) float vs[TM][R];
    __shared__ int flag[FQL_LORA_COVER_ROWS];
    const int c = ((int)blockIdx.y * FQL_LORA_EXPAND_THREADS + (int)threadIdx.x) * VEC;
    if ((int)blockIdx.x >= slots) {                              // rows no expert owns: copy `in` (or zeros)
        const int r0 = ((int)blockIdx.x - slots) * FQL_LORA_COVER_ROWS;
        cover_flags(tpe, offs, E, T, r0, flag);
        if (c >= C || in == out) return;
        for (int i = 0; i < FQL_LORA_COVER_ROWS && r0 + i < T; ++i) {
            if (flag[i]) continue;
            float y[VEC];
            if (in) load_elems<VEC, DI>(in, (size_t)(r0 + i) * C + c, y);
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) y[v] = 0.f;
            }
            store_elems<VEC, DO>(out, (size_t)(r0 + i) * C + c, y);
        }
        return;
    }
    int e, row0, n;
    if (!tile_rows<TM>(tpe, offs, E, T, (int)blockIdx.x, e, row0, n)) return;
    for (int i = threadIdx.x; i < TM * R; i += FQL_LORA_EXPAND_THREADS)
        vs[i / R][i % R] = (i / R) < n ? V[(size_t)(row0 + i / R) * R + i % R] : 0.f;
    __syncthreads();
    if (c >= C) return;
    const float *we = w + (size_t)e * R * C;

    float acc[TM][VEC];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[i][v] = 0.f;
#pragma unroll 2
    for (int j0 = 0; j0 < R; j0 += 4) {
        float wv[4][VEC];                                        // W_e[c + v][j0 + jj]
        if constexpr (!CR) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) load_vec<VEC>(we + (size_t)(j0 + jj) * C + c, wv[jj]);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float t[4];
                load_vec<4>(we + (size_t)(c + v) * R + j0, t);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) wv[jj][v] = t[jj];
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float4 vv = *reinterpret_cast<const float4 *>(&vs[i][j0]);
            const float vj[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[i][v] = fmaf(vj[jj], wv[jj][v], acc[i][v]);
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        if (i >= n) break;
        const size_t o = (size_t)(row0 + i) * C + c;
        float y[VEC];
        if (in) load_elems<VEC, DI>(in, o, y);
        else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) y[v] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[v] = fmaf(scale, acc[i][v], y[v]);
        store_elems<VEC, DO>(out, o, y);
    }
}

// ---- grad: D_e = scale * P_e^T V_e.  grid = (column blocks, E).  A lane owns VEC columns x RJ = min(R, 16) ranks (the
//      R / RJ rank groups split the wave's lanes); the 8 waves split the expert's rows (wave w: lo + w + 8 i) and their
//      partials meet in a fixed tree through LDS.  Experts without rows write zeros.  GATE: P is [T][2C].
template <int R, bool CR, int VEC, bool GATE, int DT = 0, typename... ACT>
__global__ __launch_bounds__(FQL_LORA_GRAD_THREADS) void lora_grad_kernel(
    const void *__restrict__ P, const float *__restrict__ V, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, float *__restrict__ D, int T, int C, float scale, ACT... act)
{
    constexpr int RJ = R < 16 ? R : 16;
    constexpr int JG = R / RJ;
    constexpr int LPG = FQL_WAVE / JG;                           // lanes per rank group
    constexpr int NA = VEC * RJ;                                 // accumulators per lane
    constexpr int NW = FQL_LORA_GRAD_THREADS / FQL_WAVE;
    constexpr int U = 4;                                         // rows in flight per wave
    __shared__ float red[NW / 2][NA][FQL_WAVE];

    const int e = blockIdx.y;
    int lo = 0, hi = T;
    if (tpe != nullptr) expert_rows(tpe, offs, e, T, lo, hi);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / FQL_WAVE);
    const int lane = threadIdx.x & (FQL_WAVE - 1);
    const int jg = lane / LPG, j0 = jg * RJ;
    const int c = ((int)blockIdx.x * LPG + lane % LPG) * VEC;
    const bool live = c < C;
    const int cc = live ? c : 0;                                 // dead lanes read column 0 and never store

    float acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    int t = lo + wave;
    for (; t + (U - 1) * NW < hi; t += U * NW) {
        float p[U][VEC], v[U][RJ];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_operand<VEC, GATE, DT>(P, t + u * NW, C, cc, p[u], act...);
#pragma unroll
            for (int j = 0; j < RJ; j += 4) {
                float4 x = *reinterpret_cast<const float4 *>(V + (size_t)(t + u * NW) * R + j0 + j);
                v[u][j] = x.x; v[u][j + 1] = x.y; v[u][j + 2] = x.z; v[u][j + 3] = x.w;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int a = 0; a < VEC; ++a)
#pragma unroll
                for (int j = 0; j < RJ; ++j) acc[a * RJ + j] = fmaf(p[u][a], v[u][j], acc[a * RJ + j]);
    }
    for (; t < hi; t += NW) {
        float p[VEC], v[RJ];
        load_operand<VEC, GATE, DT>(P, t, C, cc, p, act...);
#pragma unroll
        for (int j = 0; j < RJ; j += 4) {
            float4 x = *reinterpret_cast<const float4 *>(V + (size_t)t * R + j0 + j);
            v[j] = x.x; v[j + 1] = x.y; v[j + 2] = x.z; v[j + 3] = x.w;
        }
#pragma unroll
        for (int a = 0; a < VEC; ++a)
#pragma unroll
            for (int j = 0; j < RJ; ++j) acc[a * RJ + j] = fmaf(p[a], v[j], acc[a * RJ + j]);
    }
    // fixed tree: at width h, waves [h, 2h) hand their partials to waves [0, h)
#pragma unroll
    for (int h = NW / 2; h >= 1; h >>= 1) {
        if (wave >= h && wave < 2 * h) {
#pragma unroll
            for (int i = 0; i < NA; ++i) red[wave - h][i][lane] = acc[i];
        }
        __syncthreads();
        if (wave < h) {
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i] += red[wave][i][lane];
        }
        __syncthreads();
    }
    if (wave != 0 || !live) return;
    float *de = D + (size_t)e * R * C;
    if constexpr (CR) {                                          // D_e[c + a][j0 .. j0 + RJ)
#pragma unroll
        for (int a = 0; a < VEC; ++a)
#pragma unroll
            for (int j = 0; j < RJ; j += 4) {
                const float y[4] = {scale * acc[a * RJ + j], scale * acc[a * RJ + j + 1], scale * acc[a * RJ + j + 2],
                                    scale * acc[a * RJ + j + 3]};
                store_vec<4>(de + (size_t)(c + a) * R + j0 + j, y);
            }
    } else {                                                     // D_e[j0 + j][c .. c + VEC)
#pragma unroll
        for (int j = 0; j < RJ; ++j) {
            float y[VEC];
#pragma unroll
            for (int a = 0; a < VEC; ++a) y[a] = scale * acc[a * RJ + j];
            store_vec<VEC>(de + (size_t)(j0 + j) * C + c, y);
        }
    }
}

// ---- swiglu backward: dgu[t] = [dg | du] with sigma = 1 / (1 + exp(-g)), dg = dh u sigma (1 + g (1 - sigma)),
//      du = dh g sigma.  One lane per VEC columns of one row, every row (no expert table: rows no expert covers carry
//      dh = 0 and get zeros).  g very negative: expf overflows to +inf, sigma = 0 and both gradients are (signed) zero.
#define FQL_SWIGLU_BWD_THREADS 256
template <int VEC>
__global__ __launch_bounds__(FQL_SWIGLU_BWD_THREADS) void swiglu_bwd_kernel(
    const float *__restrict__ gu, const float *__restrict__ dh, float *__restrict__ dgu, int T, int F)
{
    const int per_row = F / VEC;
    const long long q = (long long)blockIdx.x * FQL_SWIGLU_BWD_THREADS + threadIdx.x;
    if (q >= (long long)T * per_row) return;
    const int t = (int)(q / per_row), c = (int)(q % per_row) * VEC;
    const size_t o = (size_t)t * 2 * F + c;
    float g[VEC], u[VEC], d[VEC], dg[VEC], du[VEC];
    load_vec<VEC>(gu + o, g);
    load_vec<VEC>(gu + o + F, u);
    load_vec<VEC>(dh + (size_t)t * F + c, d);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float sig = 1.0f / (1.0f + expf(-g[i]));
        dg[i] = d[i] * u[i] * (sig * (1.0f + g[i] * (1.0f - sig)));
        du[i] = d[i] * (g[i] * sig);
    }
    store_vec<VEC>(dgu + o, dg);
    store_vec<VEC>(dgu + o + F, du);
}

// The same pass with an element type for each tensor (DG: gate_up, DD: dh, DO: dgate_up): typed loads, the float32
// arithmetic of swiglu_bwd_kernel term for term, one rounding on the store (store_elems pins the float32 value before a
// float16 conversion).  VEC counts elements.
template <int VEC, int DG, int DD, int DO>
__global__ __launch_bounds__(FQL_SWIGLU_BWD_THREADS) void swiglu_bwd_typed_kernel(
    const void *__restrict__ gu, const void *__restrict__ dh, void *__restrict__ dgu, int T, int F)
{
    const int per_row = F / VEC;
    const long long q = (long long)blockIdx.x * FQL_SWIGLU_BWD_THREADS + threadIdx.x;
    if (q >= (long long)T * per_row) return;
    const int t = (int)(q / per_row), c = (int)(q % per_row) * VEC;
    const size_t o = (size_t)t * 2 * F + c;
    float g[VEC], u[VEC], d[VEC], dg[VEC], du[VEC];
    load_elems<VEC, DG>(gu, o, g);
    load_elems<VEC, DG>(gu, o + F, u);
    load_elems<VEC, DD>(dh, (size_t)t * F + c, d);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float sig = 1.0f / (1.0f + expf(-g[i]));
        dg[i] = d[i] * u[i] * (sig * (1.0f + g[i] * (1.0f - sig)));
        du[i] = d[i] * (g[i] * sig);
    }
    store_elems<VEC, DO>(dgu, o, dg);
    store_elems<VEC, DO>(dgu, o + F, du);
}

// ---- the same pass for the activation kind in `act`: (dg, du) = act_glu_grad (fql_common.h), every element type.
template <int VEC, int DG, int DD, int DO>
__global__ __launch_bounds__(FQL_SWIGLU_BWD_THREADS) void glu_bwd_kernel(
    const void *__restrict__ gu, const void *__restrict__ dh, void *__restrict__ dgu, int T, int F, GluArgs act)
{
    const int per_row = F / VEC;
    const long long q = (long long)blockIdx.x * FQL_SWIGLU_BWD_THREADS + threadIdx.x;
    if (q >= (long long)T * per_row) return;
    const int t = (int)(q / per_row), c = (int)(q % per_row) * VEC;
    const size_t o = (size_t)t * 2 * F + c;
    float g[VEC], u[VEC], d[VEC], dg[VEC], du[VEC];
    load_elems<VEC, DG>(gu, o, g);
    load_elems<VEC, DG>(gu, o + F, u);
    load_elems<VEC, DD>(dh, (size_t)t * F + c, d);
#pragma unroll
    for (int i = 0; i < VEC; ++i) act_glu_grad(act.kind, act.alpha, act.limit, g[i], u[i], d[i], dg[i], du[i]);
    store_elems<VEC, DO>(dgu, o, dg);
    store_elems<VEC, DO>(dgu, o + F, du);
}

}  // namespace lora
