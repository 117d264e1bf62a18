// libfql_int4.so, fifth translation unit: the typed low-rank adapter entry points (include/fql_int4.h, fql_lora_shrink /
// fql_lora_expand / fql_lora_grad) -- the kernels of fql_lora.h with a float16 / bfloat16 [T][C] operand.  A translation
// unit of its own because of the number of instantiations (rank x layout x vector width x element types).  All-float32
// calls forward to the _f32 entry points of fql_lora.hip, so those kernels exist once.
// Host-side validation and launches only: no allocation, no synchronisation.
#include "fql_lora_launch.h"

namespace {

using namespace lora_host;

template <int R, bool CR>
int shrink_t(const void *in, int dt, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T,
             int C, float scale, int vec, hipStream_t st)
{
    return dt == FQL_DTYPE_F16 ? shrink_r<R, CR, false, FQL_DTYPE_F16>(in, w, tpe, offs, out, E, T, C, scale, vec, st)
                               : shrink_r<R, CR, false, FQL_DTYPE_BF16>(in, w, tpe, offs, out, E, T, C, scale, vec, st);
}

template <int R, bool CR>
int grad_t(const void *p, int dt, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T, int C,
           float scale, int vec, hipStream_t st)
{
    return dt == FQL_DTYPE_F16 ? grad_r<R, CR, false, FQL_DTYPE_F16>(p, v, tpe, offs, d, E, T, C, scale, vec, st)
                               : grad_r<R, CR, false, FQL_DTYPE_BF16>(p, v, tpe, offs, d, E, T, C, scale, vec, st);
}

// (in, out) element types: every pair but (float32, float32), which is fql_lora_expand_f32.  `di` is ignored (taken as
// float32) when in == NULL.
template <int R, bool CR>
int expand_t(const float *v, const float *w, const int32_t *tpe, const int32_t *offs, const void *in, int di, void *out,
             int dout, int E, int T, int C, float scale, int vec, hipStream_t st)
{
#define FQL_EXPAND_CASE(DI, DO)                                                                                         \
    if (di == DI && dout == DO) return expand_r<R, CR, DI, DO>(v, w, tpe, offs, in, out, E, T, C, scale, vec, st);
    FQL_EXPAND_CASE(FQL_DTYPE_F32, FQL_DTYPE_F16)
    FQL_EXPAND_CASE(FQL_DTYPE_F32, FQL_DTYPE_BF16)
    FQL_EXPAND_CASE(FQL_DTYPE_F16, FQL_DTYPE_F32)
    FQL_EXPAND_CASE(FQL_DTYPE_F16, FQL_DTYPE_F16)
    FQL_EXPAND_CASE(FQL_DTYPE_F16, FQL_DTYPE_BF16)
    FQL_EXPAND_CASE(FQL_DTYPE_BF16, FQL_DTYPE_F32)
    FQL_EXPAND_CASE(FQL_DTYPE_BF16, FQL_DTYPE_F16)
    FQL_EXPAND_CASE(FQL_DTYPE_BF16, FQL_DTYPE_BF16)
#undef FQL_EXPAND_CASE
    return FQL_ERR_DTYPE;
}

}  // namespace

extern "C" {

FQL_API int fql_lora_shrink(const void *in, int in_dtype, const float *w, int w_layout, const int32_t *tokens_per_expert,
                            const int32_t *input_offsets, float *out, int E, int T, int C, int r, float scale,
                            void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout);
    if (rc != FQL_OK) return rc;
    if (!valid_dtype(in_dtype)) return FQL_ERR_DTYPE;
    if (in_dtype == FQL_DTYPE_F32)
        return fql_lora_shrink_f32(static_cast<const float *>(in), w, w_layout, tokens_per_expert, input_offsets, out, E,
                                   T, C, r, scale, stream);
    if (T == 0) return FQL_OK;
    if (!in || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16) || !aligned(in, 2)) return FQL_ERR_ALIGNMENT;
    const int vec = vec_width(C, in, in_dtype, in, in_dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(shrink_t, w_layout == FQL_LORA_CR, in, in_dtype, w, tokens_per_expert, input_offsets, out, E, T, C,
                      scale, vec, st)
}

FQL_API int fql_lora_expand(const float *v, const float *w, int w_layout, const int32_t *tokens_per_expert,
                            const int32_t *input_offsets, const void *in, int in_dtype, void *out, int out_dtype, int E,
                            int T, int C, int r, float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout);
    if (rc != FQL_OK) return rc;
    if (!valid_dtype(out_dtype) || (in && !valid_dtype(in_dtype))) return FQL_ERR_DTYPE;
    if (in && in == out && in_dtype != out_dtype) return FQL_ERR_DTYPE;       // in place: one element type
    const int di = in ? in_dtype : FQL_DTYPE_F32;
    if (di == FQL_DTYPE_F32 && out_dtype == FQL_DTYPE_F32)
        return fql_lora_expand_f32(v, w, w_layout, tokens_per_expert, input_offsets, static_cast<const float *>(in),
                                   static_cast<float *>(out), E, T, C, r, scale, stream);
    if (T == 0 || C == 0) return FQL_OK;
    if (!v || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16) || !aligned(out, elem_bytes(out_dtype)) || (in && !aligned(in, elem_bytes(di))))
        return FQL_ERR_ALIGNMENT;
    const int vec = in ? vec_width(C, out, out_dtype, in, di) : vec_width(C, out, out_dtype, out, out_dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(expand_t, w_layout == FQL_LORA_CR, v, w, tokens_per_expert, input_offsets, in, di, out, out_dtype,
                      E, T, C, scale, vec, st)
}

FQL_API int fql_lora_grad(const void *p, int p_dtype, const float *v, const int32_t *tokens_per_expert,
                          const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r, float scale,
                          void *stream)
{
    int rc = shape_check(E, T, C, r, d_layout);
    if (rc != FQL_OK) return rc;
    if (!valid_dtype(p_dtype)) return FQL_ERR_DTYPE;
    if (p_dtype == FQL_DTYPE_F32)
        return fql_lora_grad_f32(static_cast<const float *>(p), v, tokens_per_expert, input_offsets, d, d_layout, E, T,
                                 C, r, scale, stream);
    if (T == 0 || C == 0 || E == 0) return FQL_OK;
    if (!p || !v || !d) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(v, 16) || !aligned(d, 16) || !aligned(p, 2)) return FQL_ERR_ALIGNMENT;
    const int vec = vec_width(C, p, p_dtype, p, p_dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(grad_t, d_layout == FQL_LORA_CR, p, p_dtype, v, tokens_per_expert, input_offsets, d, E, T, C, scale,
                      vec, st)
}

}  // extern "C"
