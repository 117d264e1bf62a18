// libfql_int4.so, third translation unit: the input-gradient entry points (include/fql_int4.h,
// fql_linear_bwd_input[_f32] / fql_moe_bwd_input[_f32]) over the kernels of fql_bwd.h.
// Host-side validation and launches only, as in fql_int4.hip: no allocation, no synchronisation.
#include "../../include/fql_int4.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_act_quant.h"
#include "fql_bwd.h"

namespace {

using namespace fql_host;

struct BwdWorkspace {
    int8_t *limbs = nullptr;
    float *delta = nullptr;      // [sets + 1][T]: delta, delta2 (residual set), the per-row float correction
    int32_t *rowsum = nullptr;   // [sets][L][T] (written by the pre-pass; the backward GEMM does not need them)
    size_t bytes = 0;
};

inline size_t bwd_limb_bytes(int L, int T, int E, int Np) { return (size_t)L * (Np / FQL_KB) * (size_t)row_blocks(T, E) * 8192; }

inline BwdWorkspace bwd_carve(void *base, int L, int T, int E, int Np)
{
    BwdWorkspace w;
    const int sets = (FQL_RES_ENABLED && L >= 2) ? 2 : 1;
    const size_t lb = round16((size_t)sets * bwd_limb_bytes(L, T, E, Np));
    const size_t db = round16((size_t)(sets + 1) * T * sizeof(float));
    const size_t rb = round16((size_t)sets * L * T * sizeof(int32_t));
    char *p = static_cast<char *>(base);
    w.limbs = reinterpret_cast<int8_t *>(p);
    w.delta = reinterpret_cast<float *>(p + lb);
    w.rowsum = reinterpret_cast<int32_t *>(p + lb + db);
    w.bytes = lb + db + rb;
    return w;
}

// IN / OUT: element types of gy / gx (FQL_DTYPE_*)
template <int L, int IN, int OUT>
int launch_bwd(const void *gy, const uint8_t *packed, const float *scales, const float *zps, void *gx,
               const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, const BwdWorkspace &w, hipStream_t st)
{
    const int Np = padded(N);
    const int MBT = (int)row_blocks(T, E);
    // pre-pass: 4-row workgroups, or one row per workgroup when there are few rows in all (fql_int4.hip, launch_act_quant)
    const bool vec = (N % 16 == 0) && aligned16(gy) && aligned16(scales) && aligned16(zps);
    const int mblocks = (tpe == nullptr) ? (T + FQL_MB - 1) / FQL_MB : (T + FQL_MB * E) / FQL_MB;
    const bool single = vec && (long long)mblocks * FQL_MB <= 512;
    const int rblocks = single ? T : (T + ACT_ROWS - 1) / ACT_ROWS;
    const int zblocks = tpe != nullptr ? (T + 255) / 256 : 0;
    void (*pre)(const void *, float *, int32_t *, int8_t *, int, int, int, int, int, void *, int, int, const int32_t *,
                const int32_t *, int, const float *, const float *) =
        single ? act_colscale_kernel<L, true, 1, IN>
               : (vec ? act_colscale_kernel<L, true, ACT_ROWS, IN> : act_colscale_kernel<L, false, ACT_ROWS, IN>);
    if (const int rc = launch(pre, dim3(rblocks + zblocks), dim3(256), 0, st, gy, w.delta, w.rowsum, w.limbs, T, N, Np / FQL_KB, MBT,
                              rblocks, gx, dtype_bytes(OUT), K, tpe, offs, E, scales, zps))
        return rc;

    const int m_slots = (tpe == nullptr) ? (T + BwdCfg::BM - 1) / BwdCfg::BM : (T + BwdCfg::BM - 1) / BwdCfg::BM + E;
    const int n_tiles = (K + BwdCfg::BN - 1) / BwdCfg::BN;
    const long long tiles = (long long)m_slots * n_tiles;
    const int cus = device_compute_units();                  // (the real count: fql_tune_set_compute_units caps the forward only)
    const int grid = (int)(tiles < cus ? tiles : cus);
    const bool vw = (K % 32 == 0) && aligned16(packed);
    auto gemm = vw ? gemm_bwd_kernel<L, true, OUT> : gemm_bwd_kernel<L, false, OUT>;
    hipLaunchKernelGGL(gemm, dim3(grid), dim3(BwdCfg::THREADS), 0, st, w.limbs, w.delta, packed, zps, gx, tpe, offs, E, T,
                       K, N, Np, MBT, m_slots, n_tiles);
    return launched();
}

// Shape limits shared by the workspace query and the entry points: i32 exactness (N), 31-bit buffer offsets (limbs, weights),
// the tile count.
inline bool bwd_shape_ok(int L, int E, int T, int K, int N)
{
    if (N > FQL_BWD_MAX_N || E > 65535) return false;
    const size_t sets = (FQL_RES_ENABLED && L >= 2) ? 2 : 1;
    if (sets * bwd_limb_bytes(L, T, E, padded(N)) >= ((size_t)1 << 31)) return false;
    if ((size_t)N * (size_t)(K >> 1) >= ((size_t)1 << 31)) return false;
    const long long m_slots = ((long long)T + BwdCfg::BM - 1) / BwdCfg::BM + E;
    return m_slots * ((K + BwdCfg::BN - 1) / BwdCfg::BN) < ((long long)1 << 31);
}

size_t bwd_workspace_bytes(int E, int T, int K, int N, int precision)
{
    const int L = limbs_of(precision);
    if (L < 0 || E <= 0 || T <= 0 || K <= 0 || N <= 0 || (K & 1) || !bwd_shape_ok(L, E, T, K, N)) return 0;
    return bwd_carve(nullptr, L, T, E, padded(N)).bytes;
}

template <int L, int IN>
int launch_bwd_out(int out_dtype, const void *gy, const uint8_t *packed, const float *scales, const float *zps, void *gx,
                   const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, const BwdWorkspace &w, hipStream_t st)
{
    switch (out_dtype) {
    case FQL_DTYPE_F32: return launch_bwd<L, IN, FQL_DTYPE_F32>(gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    case FQL_DTYPE_F16: return launch_bwd<L, IN, FQL_DTYPE_F16>(gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    default: return launch_bwd<L, IN, FQL_DTYPE_BF16>(gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    }
}

template <int L>
int launch_bwd_types(int in_dtype, int out_dtype, const void *gy, const uint8_t *packed, const float *scales,
                     const float *zps, void *gx, const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N,
                     const BwdWorkspace &w, hipStream_t st)
{
    switch (in_dtype) {
    case FQL_DTYPE_F32: return launch_bwd_out<L, FQL_DTYPE_F32>(out_dtype, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    case FQL_DTYPE_F16: return launch_bwd_out<L, FQL_DTYPE_F16>(out_dtype, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    default: return launch_bwd_out<L, FQL_DTYPE_BF16>(out_dtype, gy, packed, scales, zps, gx, tpe, offs, E, T, K, N, w, st);
    }
}

int bwd_entry(const void *grad_out, int in_dtype, const uint8_t *packed, const float *scales, const float *zps,
              const int32_t *tpe, const int32_t *offs, void *grad_in, int out_dtype, int E, int T, int K, int N,
              int precision, void *ws, size_t ws_bytes, void *stream, bool grouped)
{
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (E < 0 || T < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (N > FQL_BWD_MAX_N || E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || K == 0) return FQL_OK;
    if (!grad_in) return FQL_ERR_NULL_POINTER;
    if (N > 0 && E > 0 && (!grad_out || !packed || !scales || !zps || (grouped && (!tpe || !offs))))
        return FQL_ERR_NULL_POINTER;
    if (N > 0 && E > 0 && !bwd_shape_ok(L, E, T, K, N)) return FQL_ERR_BAD_SHAPE;
    if (N > 0 && E > 0) {
        const size_t need = bwd_carve(nullptr, L, T, E, padded(N)).bytes;
        if (!ws || !aligned16(ws) || ws_bytes < need) return FQL_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0 || E == 0)                                     // empty contraction / no expert: the gradient is zero
        return hipMemsetAsync(grad_in, 0, (size_t)T * K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    const BwdWorkspace w = bwd_carve(ws, L, T, E, padded(N));
    return with_limbs(L, [&](auto l) {
        return launch_bwd_types<decltype(l)::value>(in_dtype, out_dtype, grad_out, packed, scales, zps, grad_in, tpe, offs, E, T, K, N, w, st);
    });
}

}  // namespace

extern "C" {

FQL_API size_t fql_linear_bwd_workspace_bytes(int B, int K, int N, int precision)
{
    return bwd_workspace_bytes(1, B, K, N, precision);
}

FQL_API int fql_linear_bwd_input_f32(const float *grad_out, const uint8_t *packed, const float *scales, const float *zps,
                                     float *grad_in, int B, int K, int N, int precision, void *ws, size_t ws_bytes,
                                     void *stream)
{
    return bwd_entry(grad_out, FQL_DTYPE_F32, packed, scales, zps, nullptr, nullptr, grad_in, FQL_DTYPE_F32, 1, B, K, N,
                     precision, ws, ws_bytes, stream, false);
}

FQL_API int fql_linear_bwd_input(const void *grad_out, int grad_out_dtype, const uint8_t *packed, const float *scales,
                                 const float *zps, void *grad_in, int grad_in_dtype, int B, int K, int N, int precision,
                                 void *ws, size_t ws_bytes, void *stream)
{
    return bwd_entry(grad_out, grad_out_dtype, packed, scales, zps, nullptr, nullptr, grad_in, grad_in_dtype, 1, B, K, N,
                     precision, ws, ws_bytes, stream, false);
}

FQL_API size_t fql_moe_bwd_workspace_bytes(int E, int T, int K, int N, int precision)
{
    return bwd_workspace_bytes(E, T, K, N, precision);
}

FQL_API int fql_moe_bwd_input_f32(const uint8_t *packed, const float *scales, const float *zps, const float *grad_out,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *grad_in, int E,
                                  int T, int K, int N, int precision, void *ws, size_t ws_bytes, void *stream)
{
    return bwd_entry(grad_out, FQL_DTYPE_F32, packed, scales, zps, tokens_per_expert, input_offsets, grad_in,
                     FQL_DTYPE_F32, E, T, K, N, precision, ws, ws_bytes, stream, true);
}

FQL_API int fql_moe_bwd_input(const uint8_t *packed, const float *scales, const float *zps, const void *grad_out,
                              int grad_out_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                              void *grad_in, int grad_in_dtype, int E, int T, int K, int N, int precision, void *ws,
                              size_t ws_bytes, void *stream)
{
    return bwd_entry(grad_out, grad_out_dtype, packed, scales, zps, tokens_per_expert, input_offsets, grad_in,
                     grad_in_dtype, E, T, K, N, precision, ws, ws_bytes, stream, true);
}

}  // extern "C"
