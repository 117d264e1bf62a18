// libfql_int4.so, sixth translation unit: the gated FFN experts on float16 / bfloat16 activations (include/fql_int4.h,
// fql_lora_gated_shrink / fql_lora_gated_grad / fql_swiglu_bwd, and the pre-pass behind fql_moe_gated_fwd) -- the kernels of
// fql_lora.h with GATE = true and a 16-bit gate|up operand, swiglu_bwd_typed_kernel, and act_fused_kernel<.., GATE = true>
// for a 16-bit row.  A translation unit of its own so that a parallel build is not lengthened and the other units' device
// code stays what it was.  All-float32 calls forward to the _f32 entry points of fql_lora.hip, so those kernels exist once.
// Host-side validation and launches only: no allocation, no synchronisation.
#include "fql_lora_launch.h"
#include "fql_act_quant.h"
#include "fql_ffn16_launch.h"

namespace {

using namespace lora_host;

// Widest vector, in ELEMENTS, both halves of every [2C] gate|up row allow: gate_up, gate_up + C and the row pitch 2C,
// each at 2 bytes per element (the float32 rule of fql_lora.hip at half the bytes, so an aligned tensor gets the same
// width in either type).
inline int gated_vec_width16(int C, const void *gate_up)
{
    const char *base = static_cast<const char *>(gate_up);
    for (int v = 4; v > 1; v >>= 1)
        if ((2LL * C) % v == 0 && aligned(base, 2 * v) && aligned(base + 2 * (size_t)C, 2 * v)) return v;
    return 1;
}

template <int R, bool CR>
int gated_shrink_t(const void *gu, int dt, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E,
                   int T, int C, float scale, int vec, hipStream_t st)
{
    return dt == FQL_DTYPE_F16 ? shrink_r<R, CR, true, FQL_DTYPE_F16>(gu, w, tpe, offs, out, E, T, C, scale, vec, st)
                               : shrink_r<R, CR, true, FQL_DTYPE_BF16>(gu, w, tpe, offs, out, E, T, C, scale, vec, st);
}

template <int R, bool CR>
int gated_grad_t(const void *gu, int dt, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T,
                 int C, float scale, int vec, hipStream_t st)
{
    return dt == FQL_DTYPE_F16 ? grad_r<R, CR, true, FQL_DTYPE_F16>(gu, v, tpe, offs, d, E, T, C, scale, vec, st)
                               : grad_r<R, CR, true, FQL_DTYPE_BF16>(gu, v, tpe, offs, d, E, T, C, scale, vec, st);
}

using SwigluKernel = void (*)(const void *, const void *, void *, int, int);

template <int DG, int DD, int DO>
SwigluKernel swiglu_pick(int vec)
{
    return vec == 4 ? lora::swiglu_bwd_typed_kernel<4, DG, DD, DO>
                    : (vec == 2 ? lora::swiglu_bwd_typed_kernel<2, DG, DD, DO> : lora::swiglu_bwd_typed_kernel<1, DG, DD, DO>);
}

template <int DG, int DD>
SwigluKernel swiglu_pick_out(int dout, int vec)
{
    return dout == FQL_DTYPE_F32 ? swiglu_pick<DG, DD, FQL_DTYPE_F32>(vec)
         : dout == FQL_DTYPE_F16 ? swiglu_pick<DG, DD, FQL_DTYPE_F16>(vec) : swiglu_pick<DG, DD, FQL_DTYPE_BF16>(vec);
}

template <int DG>
SwigluKernel swiglu_pick_dh(int dd, int dout, int vec)
{
    return dd == FQL_DTYPE_F32 ? swiglu_pick_out<DG, FQL_DTYPE_F32>(dout, vec)
         : dd == FQL_DTYPE_F16 ? swiglu_pick_out<DG, FQL_DTYPE_F16>(dout, vec) : swiglu_pick_out<DG, FQL_DTYPE_BF16>(dout, vec);
}

using ActKernel = void (*)(const void *, const int32_t *, int, float *, int32_t *, int8_t *, int, int, int, int, int, void *,
                           int, int, const int32_t *, const int32_t *, int, const float *);

template <int L, int IN>
ActKernel act_pick(int variant)
{
    return variant == 0 ? act_fused_kernel<L, true, IN, true, false, 1>
                        : (variant == 1 ? act_fused_kernel<L, true, IN, true, false> : act_fused_kernel<L, false, IN, true, false>);
}

}  // namespace

int fql_act_gated16_launch(int L, int variant, int in_dtype, const FqlActGatedArgs &a)
{
    if (variant < 0 || variant > 2 || (in_dtype != FQL_DTYPE_F16 && in_dtype != FQL_DTYPE_BF16)) return -1;
    ActKernel kern;
    const bool h = in_dtype == FQL_DTYPE_F16;
    if (L == 1) kern = h ? act_pick<1, FQL_DTYPE_F16>(variant) : act_pick<1, FQL_DTYPE_BF16>(variant);
    else if (L == 2) kern = h ? act_pick<2, FQL_DTYPE_F16>(variant) : act_pick<2, FQL_DTYPE_BF16>(variant);
    else if (L == 3) kern = h ? act_pick<3, FQL_DTYPE_F16>(variant) : act_pick<3, FQL_DTYPE_BF16>(variant);
    else return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(a.rblocks + a.zblocks), dim3(256), 0, a.stream, a.x, (const int32_t *)nullptr, 0, a.delta,
                       a.rowsum, a.limbs, a.T, a.K, a.KB, a.MBT, a.rblocks, a.out, a.out_es, a.N, a.tpe, a.offs, a.E,
                       a.row_weight);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" {

FQL_API int fql_lora_gated_shrink(const void *gate_up, int dtype, const float *w, int w_layout,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                  int T, int C, int r, float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, w_layout, true);
    if (rc != FQL_OK) return rc;
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (dtype == FQL_DTYPE_F32)
        return fql_lora_gated_shrink_f32(static_cast<const float *>(gate_up), w, w_layout, tokens_per_expert,
                                         input_offsets, out, E, T, C, r, scale, stream);
    if (T == 0) return FQL_OK;
    if (!gate_up || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16) || !aligned(gate_up, 2)) return FQL_ERR_ALIGNMENT;
    const int vec = gated_vec_width16(C, gate_up);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(gated_shrink_t, w_layout == FQL_LORA_CR, gate_up, dtype, w, tokens_per_expert, input_offsets, out,
                      E, T, C, scale, vec, st)
}

FQL_API int fql_lora_gated_grad(const void *gate_up, int dtype, const float *v, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                                float scale, void *stream)
{
    int rc = shape_check(E, T, C, r, d_layout, true);
    if (rc != FQL_OK) return rc;
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (dtype == FQL_DTYPE_F32)
        return fql_lora_gated_grad_f32(static_cast<const float *>(gate_up), v, tokens_per_expert, input_offsets, d,
                                       d_layout, E, T, C, r, scale, stream);
    if (T == 0 || C == 0 || E == 0) return FQL_OK;
    if (!gate_up || !v || !d) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(v, 16) || !aligned(d, 16) || !aligned(gate_up, 2)) return FQL_ERR_ALIGNMENT;
    const int vec = gated_vec_width16(C, gate_up);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FQL_LORA_DISPATCH(gated_grad_t, d_layout == FQL_LORA_CR, gate_up, dtype, v, tokens_per_expert, input_offsets, d, E, T,
                      C, scale, vec, st)
}

FQL_API int fql_swiglu_bwd(const void *gate_up, int dtype, const void *dh, int dh_dtype, void *dgate_up, int out_dtype,
                           int T, int F, void *stream)
{
    if (T < 0 || F < 0 || 2LL * T * F >= ((long long)1 << 31)) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(dtype) || !valid_dtype(dh_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (dtype == FQL_DTYPE_F32 && dh_dtype == FQL_DTYPE_F32 && out_dtype == FQL_DTYPE_F32)
        return fql_swiglu_bwd_f32(static_cast<const float *>(gate_up), static_cast<const float *>(dh),
                                  static_cast<float *>(dgate_up), T, F, stream);
    if (T == 0 || F == 0) return FQL_OK;
    if (!gate_up || !dh || !dgate_up) return FQL_ERR_NULL_POINTER;
    if (dgate_up == gate_up) return FQL_ERR_BAD_SHAPE;
    if (!aligned(gate_up, elem_bytes(dtype)) || !aligned(dh, elem_bytes(dh_dtype)) || !aligned(dgate_up, elem_bytes(out_dtype)))
        return FQL_ERR_ALIGNMENT;
    // widest vector, in elements, every access allows: the three bases aligned to v of their own elements, F % v == 0
    // (then the up half at + F and every row pitch follow)
    int vec = 1;
    for (int v = 4; v > 1; v >>= 1)
        if (F % v == 0 && aligned(gate_up, v * elem_bytes(dtype)) && aligned(dh, v * elem_bytes(dh_dtype)) &&
            aligned(dgate_up, v * elem_bytes(out_dtype))) { vec = v; break; }
    const SwigluKernel kern = dtype == FQL_DTYPE_F32 ? swiglu_pick_dh<FQL_DTYPE_F32>(dh_dtype, out_dtype, vec)
                            : dtype == FQL_DTYPE_F16 ? swiglu_pick_dh<FQL_DTYPE_F16>(dh_dtype, out_dtype, vec)
                                                     : swiglu_pick_dh<FQL_DTYPE_BF16>(dh_dtype, out_dtype, vec);
    const long long lanes = (long long)T * (F / vec);
    const dim3 grid((unsigned)((lanes + FQL_SWIGLU_BWD_THREADS - 1) / FQL_SWIGLU_BWD_THREADS));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, grid, dim3(FQL_SWIGLU_BWD_THREADS), 0, static_cast<hipStream_t>(stream), gate_up, dh, dgate_up,
                       T, F);
    return launched();
}

}  // extern "C"
