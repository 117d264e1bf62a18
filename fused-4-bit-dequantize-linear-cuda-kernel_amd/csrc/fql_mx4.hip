// libfql_int4.so, the MXFP4 expert weights (include/fql_int4.h, fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd /
// fql_moe_mx4_bwd_input, the fp8-row entries fql_moe_mx4_fwd_f8 / _fwd_q8 / _glu_fwd_q8 and the MXFP4-row entries
// fql_moe_mx4_fwd_f4 / _fwd_q4 / _glu_fwd_q4 / fql_mx4_quantize_rows) over the kernels of fql_gemm_mx4.h,
// fql_gemm_mx4_decode.h, fql_gemm_mx4_bwd.h, fql_gemm_mx4_f8.h, fql_gemm_mx4_f4.h and fql_gemm_mx4_sdecode.h.  Host-side validation and launches only, as in fql_int4.hip: no allocation, no synchronisation.
#include "../../include/fql_int4.h"
#include "../../include/fql_int4_tune.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_gemm_mx4.h"
#include "fql_gemm_mx4_decode.h"
#include "fql_gemm_mx4_bwd.h"
#include "fql_gemm_mx4_f8.h"
#include "fql_gemm_mx4_f4.h"
#include "fql_gemm_mx4_sdecode.h"

#include <cmath>

namespace {

using namespace fql_host;

struct Mx4Call {
    const uint8_t *blocks, *scales;
    const void *rows;                 // [T][K] of in_dtype
    const float *bias;
    const int32_t *tpe, *offs;
    void *out;
    int E, T, K, N;
    const float *act_scale = nullptr;  // [T] or NULL (the fp8-row kernel only)
    const uint8_t *row_scales = nullptr;  // [T][K / 32] E8M0 (the MXFP4-row kernel only)
};

enum { ROWS_FLOAT = 0, ROWS_E4M3 = 1, ROWS_MXFP4 = 2 };   // what c.rows holds

// The bfloat16 forward has two kernels that return the same bits (fql_gemm_mx4_decode.h): the 64 x 128 tile and, for few
// rows, the one-wave decode kernel.  The per-expert counts stay on the device, so T alone decides.
#define FQL_MX4_DECODE_MAX_ROWS 512    /* rows (T) up to which the decode kernel runs: the largest count of the sweep at which it wins */
int g_mx4_decode_max_rows = FQL_MX4_DECODE_MAX_ROWS;

bool mx4_use_decode(int T)
{
    return T > 0 && T <= g_mx4_decode_max_rows && (T + Mx4DecodeCfg::BT - 1) / Mx4DecodeCfg::BT <= 65535;
}

// The two block-scaled precisions have the same pair of kernels (fql_gemm_mx4_sdecode.h), each with a threshold of its own:
// index 0 the fp8 rows (mode 1 of the hooks), index 1 the MXFP4 rows (mode 2).
#define FQL_MX4_F8_DECODE_MAX_ROWS 8   /* rows (T) up to which the fp8-row decode kernel runs: the largest count of the sweep up to which it wins at every point of both shapes */
#define FQL_MX4_F4_DECODE_MAX_ROWS 8   /* ... the MXFP4-row decode kernel: the same rule, the same count */
int g_mx4_scaled_decode_max_rows[2] = {FQL_MX4_F8_DECODE_MAX_ROWS, FQL_MX4_F4_DECODE_MAX_ROWS};

bool mx4_scaled_use_decode(int rows_kind, int T)
{
    return T > 0 && T <= g_mx4_scaled_decode_max_rows[rows_kind - ROWS_E4M3] &&
           (T + Mx4SDecodeCfg::BT - 1) / Mx4SDecodeCfg::BT <= 65535;
}

// The decode kernel of either block-scaled precision: c.rows is what launch_mx4_f8 / launch_mx4_f4 take.
template <int ROWS>
int launch_mx4_sdecode(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using D = Mx4SDecodeCfg;                                 // (one more z-slice zeroes the rows no expert covers)
    const dim3 grid((c.N + D::BN - 1) / D::BN, (c.T + D::BT - 1) / D::BT, c.tpe != nullptr ? c.E + 1 : 1);
    auto go = [&](auto kern) {
        return launch(kern, grid, dim3(D::THREADS), 0, st, c.blocks, c.scales, static_cast<const uint8_t *>(c.rows), c.row_scales,
                      c.act_scale, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
    };
    switch (out_dtype) {
    case FQL_DTYPE_F32: return go(mx4_sdecode_kernel<ROWS, FQL_DTYPE_F32>);
    case FQL_DTYPE_F16: return go(mx4_sdecode_kernel<ROWS, FQL_DTYPE_F16>);
    default: return go(mx4_sdecode_kernel<ROWS, FQL_DTYPE_BF16>);
    }
}

template <int IN, int OUT>
int launch_mx4(const Mx4Call &c, hipStream_t st)
{
    const unsigned z = c.tpe != nullptr ? c.E + 1 : 1;       // (one more z-slice zeroes the rows no expert covers)
    if (mx4_use_decode(c.T)) {
        using D = Mx4DecodeCfg;
        return launch(mx4_decode_kernel<IN, OUT>, dim3((c.N + D::BN - 1) / D::BN, (c.T + D::BT - 1) / D::BT, z), dim3(D::THREADS), 0,
                      st, c.blocks, c.scales, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
    }
    using C = Mx4Cfg;
    return launch(mx4_kernel<IN, OUT>, dim3((c.N + C::BN - 1) / C::BN, (c.T + C::BT - 1) / C::BT, z),
                  dim3(C::THREADS), 0, st, c.blocks, c.scales, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
}

template <int IN>
int launch_mx4_out(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    switch (out_dtype) {
    case FQL_DTYPE_F32: return launch_mx4<IN, FQL_DTYPE_F32>(c, st);
    case FQL_DTYPE_F16: return launch_mx4<IN, FQL_DTYPE_F16>(c, st);
    default: return launch_mx4<IN, FQL_DTYPE_BF16>(c, st);
    }
}

int launch_mx4_in(int in_dtype, int out_dtype, const Mx4Call &c, hipStream_t st)
{
    return in_dtype == FQL_DTYPE_F32 ? launch_mx4_out<FQL_DTYPE_F32>(out_dtype, c, st)
                                     : launch_mx4_out<FQL_DTYPE_BF16>(out_dtype, c, st);
}

// The input gradient: c.rows is grad_out [T][N], c.out grad_in [T][K].
template <int IN, int OUT>
int launch_mx4_bwd(const Mx4Call &c, hipStream_t st)
{
    using C = Mx4BwdCfg;                                     // (one more z-slice zeroes the rows no expert covers)
    return launch(mx4_bwd_kernel<IN, OUT>, dim3((c.K + C::BK - 1) / C::BK, (c.T + C::BT - 1) / C::BT, c.tpe != nullptr ? c.E + 1 : 1),
                  dim3(C::THREADS), 0, st, c.blocks, c.scales, c.rows, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
}

template <int IN>
int launch_mx4_bwd_out(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    switch (out_dtype) {
    case FQL_DTYPE_F32: return launch_mx4_bwd<IN, FQL_DTYPE_F32>(c, st);
    case FQL_DTYPE_F16: return launch_mx4_bwd<IN, FQL_DTYPE_F16>(c, st);
    default: return launch_mx4_bwd<IN, FQL_DTYPE_BF16>(c, st);
    }
}

size_t mx4_h_bytes(int T, int K) { return round16((size_t)T * K * 2); }

// The checks both entry points share, in the documented order; `rows` is inputs or gate_up.  FQL_OK with *empty set: an
// empty call, nothing to launch.  rows_kind other than ROWS_FLOAT: the rows are bytes (in_dtype is not looked at); ROWS_MXFP4:
// packed rows [T][K / 2], 16-byte aligned, with c.row_scales.
int mx4_check(const Mx4Call &c, int in_dtype, int out_dtype, int in_cols, bool act_ok, bool *empty, int rows_kind = ROWS_FLOAT)
{
    const bool e4m3_rows = rows_kind != ROWS_FLOAT;
    *empty = false;
    if (c.E <= 0 || c.T < 0 || c.K <= 0 || c.N < 0 || !act_ok) return FQL_ERR_BAD_SHAPE;
    if (c.K & 1) return FQL_ERR_ODD_K;
    if (c.K % 32 != 0) return FQL_ERR_BAD_SHAPE;                      // one scale per 32 inputs
    if ((!e4m3_rows && in_dtype != FQL_DTYPE_F32 && in_dtype != FQL_DTYPE_BF16) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (c.T == 0 || c.N == 0) { *empty = true; return FQL_OK; }
    if (!c.blocks || !c.scales || !c.rows || !c.out) return FQL_ERR_NULL_POINTER;
    if (rows_kind == ROWS_MXFP4 && !c.row_scales) return FQL_ERR_NULL_POINTER;
    if ((c.tpe == nullptr) != (c.offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (c.tpe == nullptr && c.E != 1) return FQL_ERR_BAD_SHAPE;
    if (c.E > 65534) return FQL_ERR_BAD_SHAPE;                        // (the grid's z: the experts and the coverage slice)
    if ((c.T + Mx4Cfg::BT - 1) / Mx4Cfg::BT > 65535) return FQL_ERR_BAD_SHAPE;
    if ((long long)c.T * (in_cols / 8) / 256 >= 0x7FFFFFFFLL) return FQL_ERR_BAD_SHAPE;
    const int ib = e4m3_rows ? 1 : dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!aligned16(c.blocks) || (reinterpret_cast<uintptr_t>(c.rows) & (ib - 1)) || (reinterpret_cast<uintptr_t>(c.out) & (ob - 1)) ||
        (reinterpret_cast<uintptr_t>(c.bias) & 3)) return FQL_ERR_ALIGNMENT;
    if (rows_kind == ROWS_MXFP4 && !aligned16(c.rows)) return FQL_ERR_ALIGNMENT;
    return FQL_OK;
}

// ---- the fp8-row path (fql_gemm_mx4_f8.h): c.rows is [T][K] e4m3 bytes
int launch_mx4_f8(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    if (mx4_scaled_use_decode(ROWS_E4M3, c.T)) return launch_mx4_sdecode<ROWS_E4M3>(out_dtype, c, st);
    using C = Mx4F8Cfg;                                      // (one more z-slice zeroes the rows no expert covers)
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the bfloat16 kernel's row tile");
    const dim3 grid((c.N + C::BN - 1) / C::BN, (c.T + C::BT - 1) / C::BT, c.tpe != nullptr ? c.E + 1 : 1);
    auto go = [&](auto kern) {
        return launch(kern, grid, dim3(C::THREADS), 0, st, c.blocks, c.scales, static_cast<const uint8_t *>(c.rows), c.act_scale,
                      c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
    };
    switch (out_dtype) {
    case FQL_DTYPE_F32: return go(mx4_f8_kernel<FQL_DTYPE_F32>);
    case FQL_DTYPE_F16: return go(mx4_f8_kernel<FQL_DTYPE_F16>);
    default: return go(mx4_f8_kernel<FQL_DTYPE_BF16>);
    }
}

size_t mx4_q8_bytes(int T, int K) { return round16((size_t)T * K); }      // the e4m3 rows; act_scale [T] lies behind them

// Quantise c.rows (float rows [T][K], or gated: gate_up [T][2 K]) into the workspace, then the GEMM on the bytes.
int mx4_q8_run(Mx4Call c, int in_dtype, int out_dtype, bool gated, int activation, float act_alpha, float act_limit,
               void *workspace, size_t workspace_bytes, hipStream_t st)
{
    if (!workspace || !aligned16(workspace) || workspace_bytes < mx4_q8_bytes(c.T, c.K) + round16((size_t)c.T * 4))
        return FQL_ERR_WORKSPACE;
    uint8_t *q = static_cast<uint8_t *>(workspace);
    float *as = reinterpret_cast<float *>(q + mx4_q8_bytes(c.T, c.K));
    const dim3 grid((unsigned)((c.T + 3) / 4));
    auto go = [&](auto kern) { return launch(kern, grid, dim3(256), 0, st, c.rows, q, as, c.T, c.K, activation, act_alpha, act_limit); };
    const int lrc = in_dtype == FQL_DTYPE_F32 ? (gated ? go(mx4_q8_kernel<FQL_DTYPE_F32, true>) : go(mx4_q8_kernel<FQL_DTYPE_F32, false>))
                                              : (gated ? go(mx4_q8_kernel<FQL_DTYPE_BF16, true>) : go(mx4_q8_kernel<FQL_DTYPE_BF16, false>));
    if (lrc != FQL_OK) return lrc;
    c.rows = q;
    c.act_scale = as;
    return launch_mx4_f8(out_dtype, c, st);
}

// ---- the MXFP4-row path (fql_gemm_mx4_f4.h): c.rows is [T][K / 2] packed e2m1, c.row_scales [T][K / 32] E8M0
int launch_mx4_f4(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    if (mx4_scaled_use_decode(ROWS_MXFP4, c.T)) return launch_mx4_sdecode<ROWS_MXFP4>(out_dtype, c, st);
    using C = Mx4F4Cfg;                                      // (one more z-slice zeroes the rows no expert covers)
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the bfloat16 kernel's row tile");
    const dim3 grid((c.N + C::BN - 1) / C::BN, (c.T + C::BT - 1) / C::BT, c.tpe != nullptr ? c.E + 1 : 1);
    auto go = [&](auto kern) {
        return launch(kern, grid, dim3(C::THREADS), 0, st, c.blocks, c.scales, static_cast<const uint8_t *>(c.rows), c.row_scales,
                      c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
    };
    switch (out_dtype) {
    case FQL_DTYPE_F32: return go(mx4_f4_kernel<FQL_DTYPE_F32>);
    case FQL_DTYPE_F16: return go(mx4_f4_kernel<FQL_DTYPE_F16>);
    default: return go(mx4_f4_kernel<FQL_DTYPE_BF16>);
    }
}

size_t mx4_q4_bytes(int T, int K) { return round16((size_t)T * (K / 2)); }   // the packed rows; their scale bytes lie behind them

bool mx4_act_ok(int activation, float act_alpha, float act_limit)
{
    bool act_ok = activation == FQL_ACT_SILU || activation == FQL_ACT_GELU_TANH || activation == FQL_ACT_SWIGLU_CLAMP;
    if (act_ok && activation != FQL_ACT_SILU)
        act_ok = std::isfinite(act_alpha) && std::isfinite(act_limit) && act_limit > 0.0f;
    return act_ok;
}

// rows (float rows [T][K], or gated: gate_up [T][2 K]) -> qb [T][K / 2], qs [T][K / 32] (mx4_q4_kernel)
int launch_mx4_q4(const void *rows, int in_dtype, bool gated, int activation, float act_alpha, float act_limit, uint8_t *qb,
                  uint8_t *qs, int T, int K, hipStream_t st)
{
    const dim3 grid((unsigned)(((long long)T * (K / 8) + 255) / 256));
    auto go = [&](auto kern) { return launch(kern, grid, dim3(256), 0, st, rows, qb, qs, T, K, activation, act_alpha, act_limit); };
    return in_dtype == FQL_DTYPE_F32 ? (gated ? go(mx4_q4_kernel<FQL_DTYPE_F32, true>) : go(mx4_q4_kernel<FQL_DTYPE_F32, false>))
                                     : (gated ? go(mx4_q4_kernel<FQL_DTYPE_BF16, true>) : go(mx4_q4_kernel<FQL_DTYPE_BF16, false>));
}

// Quantise c.rows into the workspace, then the GEMM on the packed rows.
int mx4_q4_run(Mx4Call c, int in_dtype, int out_dtype, bool gated, int activation, float act_alpha, float act_limit,
               void *workspace, size_t workspace_bytes, hipStream_t st)
{
    if (!workspace || !aligned16(workspace) || workspace_bytes < mx4_q4_bytes(c.T, c.K) + round16((size_t)c.T * (c.K / 32)))
        return FQL_ERR_WORKSPACE;
    uint8_t *qb = static_cast<uint8_t *>(workspace), *qs = qb + mx4_q4_bytes(c.T, c.K);
    const int lrc = launch_mx4_q4(c.rows, in_dtype, gated, activation, act_alpha, act_limit, qb, qs, c.T, c.K, st);
    if (lrc != FQL_OK) return lrc;
    c.rows = qb;
    c.row_scales = qs;
    return launch_mx4_f4(out_dtype, c, st);
}

}  // namespace

extern "C" {

FQL_API size_t fql_moe_mx4_workspace_bytes(int E, int T, int K, int N, int gated)
{
    (void)E; (void)N;
    if (!gated || T <= 0 || K <= 0) return 0;
    return mx4_h_bytes(T, K);                                         // h [T][K] bfloat16
}

FQL_API int fql_moe_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                            const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                            int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    const Mx4Call c{blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4_in(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    bool act_ok = activation == FQL_ACT_SILU || activation == FQL_ACT_GELU_TANH || activation == FQL_ACT_SWIGLU_CLAMP;
    if (act_ok && activation != FQL_ACT_SILU)
        act_ok = std::isfinite(act_alpha) && std::isfinite(act_limit) && act_limit > 0.0f;
    Mx4Call c{blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, act_ok, &empty);
    if (rc != FQL_OK || empty) return rc;
    if (!workspace || !aligned16(workspace) || workspace_bytes < mx4_h_bytes(T, K)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned short *hbuf = static_cast<unsigned short *>(workspace);
    const dim3 grid((unsigned)(((long long)T * (K / 8) + 255) / 256));
    const int lrc = in_dtype == FQL_DTYPE_F32
        ? launch(mx4_glu_kernel<FQL_DTYPE_F32>, grid, dim3(256), 0, st, gate_up, hbuf, T, K, activation, act_alpha, act_limit)
        : launch(mx4_glu_kernel<FQL_DTYPE_BF16>, grid, dim3(256), 0, st, gate_up, hbuf, T, K, activation, act_alpha, act_limit);
    if (lrc != FQL_OK) return lrc;
    c.rows = hbuf;
    return launch_mx4_in(FQL_DTYPE_BF16, out_dtype, c, st);
}

FQL_API int fql_moe_mx4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                  int out_dtype, int E, int T, int K, int N, void *stream)
{
    static_assert(Mx4BwdCfg::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the forward's row tile");
    const Mx4Call c{blocks, scales_e8m0, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, true, &empty);
    if (rc != FQL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty) {
        if (T == 0) return FQL_OK;
        // N == 0: the gradient of an empty contraction.  grad_in [T][K] is zeros and no other operand is read.
        if (!grad_in) return FQL_ERR_NULL_POINTER;
        (void)hipGetLastError();
        return hipMemsetAsync(grad_in, 0, (size_t)T * K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    return in_dtype == FQL_DTYPE_F32 ? launch_mx4_bwd_out<FQL_DTYPE_F32>(out_dtype, c, st)
                                     : launch_mx4_bwd_out<FQL_DTYPE_BF16>(out_dtype, c, st);
}

FQL_API size_t fql_moe_mx4_f8_workspace_bytes(int E, int T, int K, int N, int mode)
{
    (void)E; (void)N;
    if ((mode != 1 && mode != 2) || T <= 0 || K <= 0) return 0;
    return mx4_q8_bytes(T, K) + round16((size_t)T * 4);               // e4m3 rows [T][K], act_scale [T]
}

FQL_API int fql_moe_mx4_fwd_f8(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *inputs_e4m3,
                               const float *act_scale, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    Mx4Call c{blocks, scales_e8m0, inputs_e4m3, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    c.act_scale = act_scale;
    bool empty;
    const int rc = mx4_check(c, 0, out_dtype, K, true, &empty, ROWS_E4M3);
    if (rc != FQL_OK || empty) return rc;
    if (reinterpret_cast<uintptr_t>(act_scale) & 3) return FQL_ERR_ALIGNMENT;
    return launch_mx4_f8(out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    const Mx4Call c{blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return mx4_q8_run(c, in_dtype, out_dtype, false, FQL_ACT_SILU, 0.0f, 0.0f, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_glu_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    bool act_ok = activation == FQL_ACT_SILU || activation == FQL_ACT_GELU_TANH || activation == FQL_ACT_SWIGLU_CLAMP;
    if (act_ok && activation != FQL_ACT_SILU)
        act_ok = std::isfinite(act_alpha) && std::isfinite(act_limit) && act_limit > 0.0f;
    const Mx4Call c{blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, act_ok, &empty);
    if (rc != FQL_OK || empty) return rc;
    return mx4_q8_run(c, in_dtype, out_dtype, true, activation, act_alpha, act_limit, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

FQL_API size_t fql_moe_mx4_f4_workspace_bytes(int E, int T, int K, int N, int mode)
{
    (void)E; (void)N;
    if ((mode != 1 && mode != 2) || T <= 0 || K <= 0) return 0;
    return mx4_q4_bytes(T, K) + round16((size_t)T * (K / 32));        // packed rows [T][K / 2], their scales [T][K / 32]
}

FQL_API int fql_moe_mx4_fwd_f4(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *in_blocks,
                               const uint8_t *in_scales_e8m0, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    Mx4Call c{blocks, scales_e8m0, in_blocks, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    c.row_scales = in_scales_e8m0;
    bool empty;
    const int rc = mx4_check(c, 0, out_dtype, K, true, &empty, ROWS_MXFP4);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4_f4(out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    const Mx4Call c{blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return mx4_q4_run(c, in_dtype, out_dtype, false, FQL_ACT_SILU, 0.0f, 0.0f, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_glu_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    const Mx4Call c{blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, K, mx4_act_ok(activation, act_alpha, act_limit), &empty);
    if (rc != FQL_OK || empty) return rc;
    return mx4_q4_run(c, in_dtype, out_dtype, true, activation, act_alpha, act_limit, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

FQL_API int fql_mx4_quantize_rows(const void *rows, int in_dtype, int gated, int activation, float act_alpha, float act_limit,
                                  uint8_t *out_blocks, uint8_t *out_scales, int T, int K, void *stream)
{
    // mx4_check on a call record with one expert, one column and no table: out_blocks stands for both `blocks` (non-NULL,
    // 16-byte aligned) and `out`, out_scales for `scales`; the documented order is fql_moe_mx4_fwd's.
    const Mx4Call c{out_blocks, out_scales, rows, nullptr, nullptr, nullptr, out_blocks, 1, T, K, 1};
    bool empty;
    const int rc = mx4_check(c, in_dtype, FQL_DTYPE_F32, K, !gated || mx4_act_ok(activation, act_alpha, act_limit), &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4_q4(rows, in_dtype, gated != 0, activation, act_alpha, act_limit, out_blocks, out_scales, T, K,
                         static_cast<hipStream_t>(stream));
}

FQL_API int fql_tune_set_mx4_decode_max_rows(int rows)
{
    const int old = g_mx4_decode_max_rows;
    if (rows >= 0) g_mx4_decode_max_rows = rows;
    return old;
}

FQL_API int fql_tune_mx4_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return mx4_use_decode(T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_scaled_decode_max_rows(int mode, int rows)
{
    if (mode != 1 && mode != 2) return -1;
    const int old = g_mx4_scaled_decode_max_rows[mode - 1];
    if (rows >= 0) g_mx4_scaled_decode_max_rows[mode - 1] = rows;
    return old;
}

FQL_API int fql_tune_mx4_scaled_kernel(int mode, int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    if (mode != 1 && mode != 2) return -1;
    return mx4_scaled_use_decode(mode == 1 ? ROWS_E4M3 : ROWS_MXFP4, T) ? 1 : 0;
}

}  // extern "C"
