// libfql_int4.so, fourth translation unit: the low-rank adapter entry points (include/fql_int4.h, fql_lora_*) over
// the kernels of fql_lora.h.  Host-side validation and launches only: no allocation, no synchronisation.
#include "../../include/fql_int4.h"
#include "fql_common.h"
#include "fql_lora.h"

namespace {

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

// Widest float vector every row of the [T][C] operands allows.
inline int vec_width(int C, const void *a, const void *b)
{
    if (C % 4 == 0 && aligned(a, 16) && aligned(b, 16)) return 4;
    if (C % 2 == 0 && aligned(a, 8) && aligned(b, 8)) return 2;
    return 1;
}

// Widest float vector both halves of every [2C] gate|up row allow: gate_up, gate_up + C and the row pitch 2C (and,
// for the grad, nothing else: v and d have their own 16-byte rule).
inline int gated_vec_width(int C, const float *gate_up)
{
    for (int v = 4; v > 1; v >>= 1)
        if ((2LL * C) % v == 0 && aligned(gate_up, 4 * v) && aligned(gate_up + C, 4 * v)) return v;
    return 1;
}

// Checks shared by the entry points, in the documented order (all before any HIP call).  `gated`: the streamed operand
// is [T][2C], so 2 T C joins the size check.
inline int shape_check(int E, int T, int C, int r, int layout, bool gated = false)
{
    if (!rank_ok(r)) return FQL_ERR_BAD_SHAPE;
    if (layout != FQL_LORA_RC && layout != FQL_LORA_CR) return FQL_ERR_BAD_SHAPE;
    if (E < 0 || T < 0 || C < 0 || E > 65535) return FQL_ERR_BAD_SHAPE;
    const long long lim = (long long)1 << 31;
    if ((long long)T * C >= lim || (long long)E * C * r >= lim || (long long)T * r >= lim) return FQL_ERR_BAD_SHAPE;
    if (gated && 2LL * T * C >= lim) return FQL_ERR_BAD_SHAPE;
    return FQL_OK;
}

inline int table_check(const int32_t *tpe, const int32_t *offs, int E)
{
    if ((tpe == nullptr) != (offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (tpe == nullptr && E != 1) return FQL_ERR_NULL_POINTER;
    return FQL_OK;
}

inline int launched() { return hipGetLastError() == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH; }

inline int tile_slots(int T, int E, int TM, bool table) { return (T + TM - 1) / TM + (table ? E : 0); }
inline int cover_blocks(int T, bool table) { return table ? (T + FQL_LORA_COVER_ROWS - 1) / FQL_LORA_COVER_ROWS : 0; }

template <int R, bool CR, bool GATE = false>
int shrink_r(const float *in, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T, int C,
             float scale, int vec, hipStream_t st)
{
    const int slots = tile_slots(T, E, 64 / R, tpe != nullptr);
    const dim3 grid(slots + cover_blocks(T, tpe != nullptr));
    auto k = vec == 4 ? lora::lora_shrink_kernel<R, CR, 4, GATE>
                      : (vec == 2 ? lora::lora_shrink_kernel<R, CR, 2, GATE> : lora::lora_shrink_kernel<R, CR, 1, GATE>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_SHRINK_THREADS), 0, st, in, w, tpe, offs, out, E, T, C, scale, slots);
    return launched();
}

template <int R, bool CR>
int expand_r(const float *v, const float *w, const int32_t *tpe, const int32_t *offs, const float *in, float *out, int E,
             int T, int C, float scale, int vec, hipStream_t st)
{
    const int slots = tile_slots(T, E, FQL_LORA_EXPAND_ROWS, tpe != nullptr);
    const int cols = FQL_LORA_EXPAND_THREADS * vec;
    const dim3 grid(slots + cover_blocks(T, tpe != nullptr), (C + cols - 1) / cols);
    auto k = vec == 4 ? lora::lora_expand_kernel<R, CR, 4>
                      : (vec == 2 ? lora::lora_expand_kernel<R, CR, 2> : lora::lora_expand_kernel<R, CR, 1>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_EXPAND_THREADS), 0, st, v, w, tpe, offs, in, out, E, T, C, scale, slots);
    return launched();
}

template <int R, bool CR, bool GATE = false>
int grad_r(const float *p, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T, int C,
           float scale, int vec, hipStream_t st)
{
    constexpr int JG = R < 16 ? 1 : R / 16;
    const int cols = FQL_WAVE / JG * vec;
    const dim3 grid((C + cols - 1) / cols, E);
    auto k = vec == 4 ? lora::lora_grad_kernel<R, CR, 4, GATE>
                      : (vec == 2 ? lora::lora_grad_kernel<R, CR, 2, GATE> : lora::lora_grad_kernel<R, CR, 1, GATE>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_GRAD_THREADS), 0, st, p, v, tpe, offs, d, T, C, scale);
    return launched();
}

template <int R, bool CR>
int gated_shrink_r(const float *gu, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T,
                   int C, float scale, int vec, hipStream_t st)
{
    return shrink_r<R, CR, true>(gu, w, tpe, offs, out, E, T, C, scale, vec, st);
}

template <int R, bool CR>
int gated_grad_r(const float *gu, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T, int C,
                 float scale, int vec, hipStream_t st)
{
    return grad_r<R, CR, true>(gu, v, tpe, offs, d, E, T, C, scale, vec, st);
}

// rank x layout dispatch
#define FQL_LORA_DISPATCH(FN, CR, ...)                                                                                  \
    switch (r) {                                                                                                        \
    case 4: return CR ? FN<4, true>(__VA_ARGS__) : FN<4, false>(__VA_ARGS__);                                           \
    case 8: return CR ? FN<8, true>(__VA_ARGS__) : FN<8, false>(__VA_ARGS__);                                           \
    case 16: return CR ? FN<16, true>(__VA_ARGS__) : FN<16, false>(__VA_ARGS__);                                        \
    case 32: return CR ? FN<32, true>(__VA_ARGS__) : FN<32, false>(__VA_ARGS__);                                        \
    default: return CR ? FN<64, true>(__VA_ARGS__) : FN<64, false>(__VA_ARGS__);                                        \
    }

}  // namespace

extern "C" {

FQL_API int fql_lora_shrink_f32(const float *in, const float *w, int w_layout, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, float *out, int E, int T, int C, int r, float scale,
                                void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout);
    if (rc != FQL_OK || T == 0) return rc;
    if (!in || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16)) return FQL_ERR_ALIGNMENT;
    const int vec = vec_width(C, in, in);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(shrink_r, w_layout == FQL_LORA_CR, in, w, tokens_per_expert, input_offsets, out, E, T, C, scale,
                      vec, st)
}

FQL_API int fql_lora_expand_f32(const float *v, const float *w, int w_layout, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, const float *in, float *out, int E, int T, int C, int r,
                                float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout);
    if (rc != FQL_OK || T == 0 || C == 0) return rc;
    if (!v || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16)) return FQL_ERR_ALIGNMENT;
    const int vec = vec_width(C, out, in ? in : out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(expand_r, w_layout == FQL_LORA_CR, v, w, tokens_per_expert, input_offsets, in, out, E, T, C,
                      scale, vec, st)
}

FQL_API int fql_lora_grad_f32(const float *p, const float *v, const int32_t *tokens_per_expert,
                              const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                              float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, d_layout);
    if (rc != FQL_OK || T == 0 || C == 0 || E == 0) return rc;
    if (!p || !v || !d) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(v, 16) || !aligned(d, 16)) return FQL_ERR_ALIGNMENT;
    const int vec = vec_width(C, p, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(grad_r, d_layout == FQL_LORA_CR, p, v, tokens_per_expert, input_offsets, d, E, T, C, scale, vec,
                      st)
}

FQL_API int fql_lora_gated_shrink_f32(const float *gate_up, const float *w, int w_layout,
                                      const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                      int T, int C, int r, float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout, true);
    if (rc != FQL_OK || T == 0) return rc;
    if (!gate_up || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16)) return FQL_ERR_ALIGNMENT;
    const int vec = gated_vec_width(C, gate_up);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(gated_shrink_r, w_layout == FQL_LORA_CR, gate_up, w, tokens_per_expert, input_offsets, out, E, T,
                      C, scale, vec, st)
}

FQL_API int fql_lora_gated_grad_f32(const float *gate_up, const float *v, const int32_t *tokens_per_expert,
                                    const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                                    float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, d_layout, true);
    if (rc != FQL_OK || T == 0 || C == 0 || E == 0) return rc;
    if (!gate_up || !v || !d) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(v, 16) || !aligned(d, 16)) return FQL_ERR_ALIGNMENT;
    const int vec = gated_vec_width(C, gate_up);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(gated_grad_r, d_layout == FQL_LORA_CR, gate_up, v, tokens_per_expert, input_offsets, d, E, T, C,
                      scale, vec, st)
}

FQL_API int fql_swiglu_bwd_f32(const float *gate_up, const float *dh, float *dgate_up, int T, int F, void *stream)
{
    if (T < 0 || F < 0 || 2LL * T * F >= ((long long)1 << 31)) return FQL_ERR_BAD_SHAPE;
    if (T == 0 || F == 0) return FQL_OK;
    if (!gate_up || !dh || !dgate_up) return FQL_ERR_NULL_POINTER;
    if (dgate_up == gate_up) return FQL_ERR_BAD_SHAPE;
    const bool wide = F % 4 == 0 && aligned(gate_up, 16) && aligned(dh, 16) && aligned(dgate_up, 16);
    const long long lanes = (long long)T * (wide ? F / 4 : F);
    const dim3 grid((unsigned)((lanes + FQL_SWIGLU_BWD_THREADS - 1) / FQL_SWIGLU_BWD_THREADS));
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(wide ? lora::swiglu_bwd_kernel<4> : lora::swiglu_bwd_kernel<1>, grid,
                       dim3(FQL_SWIGLU_BWD_THREADS), 0, st, gate_up, dh, dgate_up, T, F);
    return launched();
}

}  // extern "C"
