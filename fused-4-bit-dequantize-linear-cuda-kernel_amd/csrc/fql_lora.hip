// libfql_int4.so, fourth translation unit: the float32 low-rank adapter entry points (include/fql_int4.h, fql_lora_*_f32)
// over the kernels of fql_lora.h (the typed entry points are fql_lora16.hip).  Host-side validation and launches only: no
// allocation, no synchronisation.
#include "fql_lora_launch.h"

namespace {

using namespace lora_host;

// Widest float vector both halves of every [2C] gate|up row allow: gate_up, gate_up + C and the row pitch 2C (and,
// for the grad, nothing else: v and d have their own 16-byte rule).
inline int gated_vec_width(int C, const float *gate_up)
{
    for (int v = 4; v > 1; v >>= 1)
        if ((2LL * C) % v == 0 && aligned(gate_up, 4 * v) && aligned(gate_up + C, 4 * v)) return v;
    return 1;
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
    const int vec = vec_width(C, in, FQL_DTYPE_F32, in, FQL_DTYPE_F32);
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
    const int vec = vec_width(C, out, FQL_DTYPE_F32, in ? in : out, FQL_DTYPE_F32);
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
    const int vec = vec_width(C, p, FQL_DTYPE_F32, p, FQL_DTYPE_F32);
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
