// libfql_int4.so, seventh translation unit: the gated FFN experts with an activation other than silu (include/fql_int4.h,
// fql_lora_glu_shrink / fql_lora_glu_grad / fql_glu_bwd, and the pre-pass behind fql_moe_glu_fwd) -- GeGLU (tanh form) and the
// clamped SwiGLU.  One instantiation serves both kinds: the kind and its two floats are wave-uniform kernel arguments of
// lora_shrink_kernel / lora_grad_kernel <.., GluArgs> and glu_bwd_kernel (fql_lora.h) and act_glu_kernel (fql_act_quant.h), for
// every element type, float32 included.  FQL_ACT_SILU forwards to the entry points of before, so the kernels that kind
// reaches are the ones it always reached.  A translation unit of its own so that the other units' device code stays what
// it was.  Host-side validation and launches only: no allocation, no synchronisation.
#include <cmath>

#include "fql_lora_launch.h"
#include "fql_act_quant.h"
#include "fql_glu_launch.h"

namespace {

using namespace lora_host;
using lora::GluArgs;

// activation outside FQL_ACT_*, alpha not finite, limit not finite or <= 0 (the floats of every kind but silu)
inline bool glu_args_ok(int activation, float alpha, float limit)
{
    if (activation == FQL_ACT_SILU) return true;
    if (activation != FQL_ACT_GELU_TANH && activation != FQL_ACT_SWIGLU_CLAMP) return false;
    return std::isfinite(alpha) && std::isfinite(limit) && limit > 0.0f;
}

// Widest vector, in ELEMENTS, both halves of every [2C] gate|up row allow: gate_up, gate_up + C and the row pitch 2C (the
// rule of the silu entry points in either element size, so a tensor gets the width it gets there).
inline int glu_vec_width(int C, const void *gate_up, int dtype)
{
    const char *base = static_cast<const char *>(gate_up);
    const uintptr_t es = elem_bytes(dtype);
    for (int v = 4; v > 1; v >>= 1)
        if ((2LL * C) % v == 0 && aligned(base, es * v) && aligned(base + es * (size_t)C, es * v)) return v;
    return 1;
}

template <int R, bool CR, int DT>
int glu_shrink_d(const void *gu, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T, int C,
                 float scale, int vec, hipStream_t st, GluArgs act)
{
    const int slots = tile_slots(T, E, 64 / R, tpe != nullptr);
    const dim3 grid(slots + cover_blocks(T, tpe != nullptr));
    auto k = vec == 4 ? lora::lora_shrink_kernel<R, CR, 4, true, DT, GluArgs>
                      : (vec == 2 ? lora::lora_shrink_kernel<R, CR, 2, true, DT, GluArgs> : lora::lora_shrink_kernel<R, CR, 1, true, DT, GluArgs>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_SHRINK_THREADS), 0, st, gu, w, tpe, offs, out, E, T, C, scale, slots, act);
    return launched();
}

template <int R, bool CR>
int glu_shrink_t(const void *gu, int dt, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T,
                 int C, float scale, int vec, hipStream_t st, GluArgs act)
{
    return dt == FQL_DTYPE_F32 ? glu_shrink_d<R, CR, FQL_DTYPE_F32>(gu, w, tpe, offs, out, E, T, C, scale, vec, st, act)
         : dt == FQL_DTYPE_F16 ? glu_shrink_d<R, CR, FQL_DTYPE_F16>(gu, w, tpe, offs, out, E, T, C, scale, vec, st, act)
                               : glu_shrink_d<R, CR, FQL_DTYPE_BF16>(gu, w, tpe, offs, out, E, T, C, scale, vec, st, act);
}

template <int R, bool CR, int DT>
int glu_grad_d(const void *gu, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T, int C,
               float scale, int vec, hipStream_t st, GluArgs act)
{
    constexpr int JG = R < 16 ? 1 : R / 16;
    const int cols = FQL_WAVE / JG * vec;
    const dim3 grid((C + cols - 1) / cols, E);
    auto k = vec == 4 ? lora::lora_grad_kernel<R, CR, 4, true, DT, GluArgs>
                      : (vec == 2 ? lora::lora_grad_kernel<R, CR, 2, true, DT, GluArgs> : lora::lora_grad_kernel<R, CR, 1, true, DT, GluArgs>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_GRAD_THREADS), 0, st, gu, v, tpe, offs, d, T, C, scale, act);
    return launched();
}

template <int R, bool CR>
int glu_grad_t(const void *gu, int dt, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T,
               int C, float scale, int vec, hipStream_t st, GluArgs act)
{
    return dt == FQL_DTYPE_F32 ? glu_grad_d<R, CR, FQL_DTYPE_F32>(gu, v, tpe, offs, d, E, T, C, scale, vec, st, act)
         : dt == FQL_DTYPE_F16 ? glu_grad_d<R, CR, FQL_DTYPE_F16>(gu, v, tpe, offs, d, E, T, C, scale, vec, st, act)
                               : glu_grad_d<R, CR, FQL_DTYPE_BF16>(gu, v, tpe, offs, d, E, T, C, scale, vec, st, act);
}

using GluBwdKernel = void (*)(const void *, const void *, void *, int, int, GluArgs);

template <int DG, int DD, int DO>
GluBwdKernel bwd_pick(int vec)
{
    return vec == 4 ? lora::glu_bwd_kernel<4, DG, DD, DO>
                    : (vec == 2 ? lora::glu_bwd_kernel<2, DG, DD, DO> : lora::glu_bwd_kernel<1, DG, DD, DO>);
}

template <int DG, int DD>
GluBwdKernel bwd_pick_out(int dout, int vec)
{
    return dout == FQL_DTYPE_F32 ? bwd_pick<DG, DD, FQL_DTYPE_F32>(vec)
         : dout == FQL_DTYPE_F16 ? bwd_pick<DG, DD, FQL_DTYPE_F16>(vec) : bwd_pick<DG, DD, FQL_DTYPE_BF16>(vec);
}

template <int DG>
GluBwdKernel bwd_pick_dh(int dd, int dout, int vec)
{
    return dd == FQL_DTYPE_F32 ? bwd_pick_out<DG, FQL_DTYPE_F32>(dout, vec)
         : dd == FQL_DTYPE_F16 ? bwd_pick_out<DG, FQL_DTYPE_F16>(dout, vec) : bwd_pick_out<DG, FQL_DTYPE_BF16>(dout, vec);
}

using ActGluKernel = void (*)(const void *, float *, int32_t *, int8_t *, int, int, int, int, int, void *, int, int,
                              const int32_t *, const int32_t *, int, const float *, int, float, float);

template <int L, int IN>
ActGluKernel act_pick(int variant)
{
    return variant == 0 ? act_glu_kernel<L, true, IN, 1>
                        : (variant == 1 ? act_glu_kernel<L, true, IN> : act_glu_kernel<L, false, IN>);
}

template <int L>
ActGluKernel act_pick_in(int variant, int in_dtype)
{
    return in_dtype == FQL_DTYPE_F32 ? act_pick<L, FQL_DTYPE_F32>(variant)
         : in_dtype == FQL_DTYPE_F16 ? act_pick<L, FQL_DTYPE_F16>(variant) : act_pick<L, FQL_DTYPE_BF16>(variant);
}

}  // namespace

int fql_act_glu_launch(int L, int variant, int in_dtype, const FqlActGatedArgs &a, int activation, float act_alpha,
                       float act_limit)
{
    if (variant < 0 || variant > 2 || !valid_dtype(in_dtype)) return -1;
    if (activation != FQL_ACT_GELU_TANH && activation != FQL_ACT_SWIGLU_CLAMP) return -1;
    ActGluKernel kern;
    if (L == 1) kern = act_pick_in<1>(variant, in_dtype);
    else if (L == 2) kern = act_pick_in<2>(variant, in_dtype);
    else if (L == 3) kern = act_pick_in<3>(variant, in_dtype);
    else return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(a.rblocks + a.zblocks), dim3(256), 0, a.stream, a.x, a.delta, a.rowsum, a.limbs, a.T, a.K,
                       a.KB, a.MBT, a.rblocks, a.out, a.out_es, a.N, a.tpe, a.offs, a.E, a.row_weight, activation, act_alpha,
                       act_limit);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" {

FQL_API int fql_lora_glu_shrink(const void *gate_up, int dtype, const float *w, int w_layout,
                                const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                                int C, int r, float scale, int activation, float act_alpha, float act_limit, void *stream)
{
    if (activation == FQL_ACT_SILU)
        return fql_lora_gated_shrink(gate_up, dtype, w, w_layout, tokens_per_expert, input_offsets, out, E, T, C, r, scale,
                                     stream);
    int rc = shape_check(E, T, C, r, w_layout, true);
    if (rc != FQL_OK) return rc;
    if (!glu_args_ok(activation, act_alpha, act_limit)) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (T == 0) return FQL_OK;
    if (!gate_up || !w || !out) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(w, 16) || !aligned(gate_up, elem_bytes(dtype))) return FQL_ERR_ALIGNMENT;
    const int vec = glu_vec_width(C, gate_up, dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GluArgs act{activation, act_alpha, act_limit};
    FQL_LORA_DISPATCH(glu_shrink_t, w_layout == FQL_LORA_CR, gate_up, dtype, w, tokens_per_expert, input_offsets, out, E,
                      T, C, scale, vec, st, act)
}

FQL_API int fql_lora_glu_grad(const void *gate_up, int dtype, const float *v, const int32_t *tokens_per_expert,
                              const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                              float scale, int activation, float act_alpha, float act_limit, void *stream)
{
    if (activation == FQL_ACT_SILU)
        return fql_lora_gated_grad(gate_up, dtype, v, tokens_per_expert, input_offsets, d, d_layout, E, T, C, r, scale,
                                   stream);
    int rc = shape_check(E, T, C, r, d_layout, true);
    if (rc != FQL_OK) return rc;
    if (!glu_args_ok(activation, act_alpha, act_limit)) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || C == 0 || E == 0) return FQL_OK;
    if (!gate_up || !v || !d) return FQL_ERR_NULL_POINTER;
    if ((rc = table_check(tokens_per_expert, input_offsets, E)) != FQL_OK) return rc;
    if (!aligned(v, 16) || !aligned(d, 16) || !aligned(gate_up, elem_bytes(dtype))) return FQL_ERR_ALIGNMENT;
    const int vec = glu_vec_width(C, gate_up, dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GluArgs act{activation, act_alpha, act_limit};
    FQL_LORA_DISPATCH(glu_grad_t, d_layout == FQL_LORA_CR, gate_up, dtype, v, tokens_per_expert, input_offsets, d, E, T, C,
                      scale, vec, st, act)
}

FQL_API int fql_glu_bwd(const void *gate_up, int dtype, const void *dh, int dh_dtype, void *dgate_up, int out_dtype, int T,
                        int F, int activation, float act_alpha, float act_limit, void *stream)
{
    if (activation == FQL_ACT_SILU)
        return fql_swiglu_bwd(gate_up, dtype, dh, dh_dtype, dgate_up, out_dtype, T, F, stream);
    if (T < 0 || F < 0 || 2LL * T * F >= ((long long)1 << 31)) return FQL_ERR_BAD_SHAPE;
    if (!glu_args_ok(activation, act_alpha, act_limit)) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(dtype) || !valid_dtype(dh_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
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
    const GluBwdKernel kern = dtype == FQL_DTYPE_F32 ? bwd_pick_dh<FQL_DTYPE_F32>(dh_dtype, out_dtype, vec)
                            : dtype == FQL_DTYPE_F16 ? bwd_pick_dh<FQL_DTYPE_F16>(dh_dtype, out_dtype, vec)
                                                     : bwd_pick_dh<FQL_DTYPE_BF16>(dh_dtype, out_dtype, vec);
    const long long lanes = (long long)T * (F / vec);
    const dim3 grid((unsigned)((lanes + FQL_SWIGLU_BWD_THREADS - 1) / FQL_SWIGLU_BWD_THREADS));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, grid, dim3(FQL_SWIGLU_BWD_THREADS), 0, static_cast<hipStream_t>(stream), gate_up, dh, dgate_up,
                       T, F, GluArgs{activation, act_alpha, act_limit});
    return launched();
}

}  // extern "C"
