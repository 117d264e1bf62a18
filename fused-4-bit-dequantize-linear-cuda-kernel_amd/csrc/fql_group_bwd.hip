// libfql_int4.so, the per-group input gradient (include/fql_int4.h, fql_moe_group_bwd_input) over the kernels of
// fql_group_bwd.h.  Host-side validation and launches only, as in fql_int4.hip: no allocation, no synchronisation.
#include "../../include/fql_int4.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_group_bwd.h"

namespace {

using namespace fql_host;

template <int IN, int OUT>
int launch_group_bwd(bool tiled, const void *gy, const uint8_t *packed, const float *scales, const float *zps, void *gx,
                     const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, int group, hipStream_t st)
{
    using C = GroupBwdCfg;
    if (tiled)                                               // (one more z-slice zeroes the rows no expert covers)
        return launch(group_bwd_kernel<IN, OUT>, dim3((K + C::BK - 1) / C::BK, (T + C::BT - 1) / C::BT, tpe != nullptr ? E + 1 : 1),
                      dim3(C::THREADS), 0, st, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, group);
    return launch(group_bwd_rows_kernel<IN, OUT>, dim3(T), dim3(64), 0, st, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, group);
}

template <int IN>
int launch_group_bwd_out(int out_dtype, bool tiled, const void *gy, const uint8_t *packed, const float *scales,
                         const float *zps, void *gx, const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N,
                         int group, hipStream_t st)
{
    switch (out_dtype) {
    case FQL_DTYPE_F32: return launch_group_bwd<IN, FQL_DTYPE_F32>(tiled, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, group, st);
    case FQL_DTYPE_F16: return launch_group_bwd<IN, FQL_DTYPE_F16>(tiled, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, group, st);
    default: return launch_group_bwd<IN, FQL_DTYPE_BF16>(tiled, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, group, st);
    }
}

}  // namespace

extern "C" {

// The kernels keep nothing between them: no workspace is needed today.  The query and the two arguments are part of the
// signature so that a cached [E][G][N] transpose can move in without a new entry point.
FQL_API size_t fql_moe_group_bwd_workspace_bytes(int E, int T, int K, int N, int group_size)
{
    (void)E; (void)T; (void)K; (void)N; (void)group_size;
    return 0;
}

FQL_API int fql_moe_group_bwd_input(const uint8_t *packed, const float *scales, const float *zps, const void *grad_out,
                                    int grad_out_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                    void *grad_in, int grad_in_dtype, int E, int T, int K, int N, int group_size,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (E <= 0 || T < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (K > 0 && (group_size <= 0 || (group_size & 1) || K % group_size != 0)) return FQL_ERR_BAD_SHAPE;   // even groups that tile K
    if (!valid_dtype(grad_out_dtype) || !valid_dtype(grad_in_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || K == 0) return FQL_OK;
    if (!grad_in) return FQL_ERR_NULL_POINTER;
    if (N > 0 && (!grad_out || !packed || !scales || !zps)) return FQL_ERR_NULL_POINTER;
    if ((tokens_per_expert == nullptr) != (input_offsets == nullptr)) return FQL_ERR_NULL_POINTER;
    if (tokens_per_expert == nullptr && E != 1) return FQL_ERR_BAD_SHAPE;
    if (E > 65534) return FQL_ERR_BAD_SHAPE;                          // (the grid's z: the experts and the coverage slice)
    const int ib = dtype_bytes(grad_out_dtype), ob = dtype_bytes(grad_in_dtype);
    if ((reinterpret_cast<uintptr_t>(grad_out) & (ib - 1)) || (reinterpret_cast<uintptr_t>(grad_in) & (ob - 1)) ||
        (reinterpret_cast<uintptr_t>(scales) & 3) || (reinterpret_cast<uintptr_t>(zps) & 3)) return FQL_ERR_ALIGNMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0)                                                       // empty contraction: the gradient is zero
        return hipMemsetAsync(grad_in, 0, (size_t)T * K * ob, st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    const bool tiled = K % 64 == 0 && group_size % 32 == 0 && aligned16(packed) && aligned16(grad_out) && aligned16(grad_in) &&
                       (T + GroupBwdCfg::BT - 1) / GroupBwdCfg::BT <= 65535;
    switch (grad_out_dtype) {
    case FQL_DTYPE_F32: return launch_group_bwd_out<FQL_DTYPE_F32>(grad_in_dtype, tiled, grad_out, packed, scales, zps, grad_in, tokens_per_expert, input_offsets, E, T, K, N, group_size, st);
    case FQL_DTYPE_F16: return launch_group_bwd_out<FQL_DTYPE_F16>(grad_in_dtype, tiled, grad_out, packed, scales, zps, grad_in, tokens_per_expert, input_offsets, E, T, K, N, group_size, st);
    default: return launch_group_bwd_out<FQL_DTYPE_BF16>(grad_in_dtype, tiled, grad_out, packed, scales, zps, grad_in, tokens_per_expert, input_offsets, E, T, K, N, group_size, st);
    }
}

}  // extern "C"
