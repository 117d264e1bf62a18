// libfql_int4.so, the MXFP4 expert weights (include/fql_int4.h): the bfloat16 entries fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd /
// fql_moe_mx4_bwd_input (fql_gemm_mx4.h, fql_gemm_mx4_decode.h, fql_gemm_mx4_bwd.h) and their adapter forms fql_moe_mx4_lora_fwd /
// fql_moe_mx4_glu_lora_fwd / fql_moe_mx4_lora_bwd_input (the LORA flag of the two tile kernels), the block-scaled entries on fp8 rows
// fql_moe_mx4_fwd_f8 / _fwd_q8 / _glu_fwd_q8, on MXFP4 rows fql_moe_mx4_fwd_f4 / _fwd_q4 / _glu_fwd_q4 and on MXFP6 rows
// fql_moe_mx4_fwd_f6 / _fwd_q6 / _glu_fwd_q6 (one tile and one decode kernel for the three, fql_gemm_mx4_scaled.h and
// fql_gemm_mx4_sdecode.h), the row pre-passes with fql_mx4_quantize_rows / fql_mx6_quantize_rows (fql_mx4_quant.h) and the dense
// linear entries fql_linear_mx4_fwd / fql_linear_mx4_glu_fwd with their split-K decode form (fql_gemm_mx4_linear.h), and the NVFP4 entries
// fql_moe_nvfp4_fwd / fql_moe_nvfp4_glu_fwd / fql_linear_nvfp4_fwd / fql_linear_nvfp4_glu_fwd (fql_gemm_nvfp4.h) and fql_moe_nvfp4_bwd_input (fql_gemm_nvfp4_bwd.h)
// with their adapter forms fql_moe_nvfp4_lora_fwd / _glu_lora_fwd / _lora_bwd_input and fql_linear_nvfp4_lora_fwd / _lora_bwd_input (the LORA flag of the two NVFP4 tile kernels).  Host-side validation and launches only, as in fql_int4.hip: no allocation, no synchronisation.
#include "../../include/fql_int4.h"
#include "../../include/fql_int4_tune.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_gemm_mx4.h"
#include "fql_gemm_mx4_decode.h"
#include "fql_gemm_mx4_linear.h"
#include "fql_gemm_mx4_bwd.h"
#include "fql_gemm_mx4_scaled.h"
#include "fql_gemm_mx4_sdecode.h"
#include "fql_mx4_quant.h"
#include "fql_gemm_nvfp4.h"
#include "fql_gemm_nvfp4_bwd.h"

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
    const float *act_scale = nullptr;  // [T] or NULL (fp8 rows only)
    const uint8_t *row_scales = nullptr;  // [T][K / 32] E8M0 (MXFP4 and MXFP6 rows only)
    bool lora = false;                 // an adapter entry (bfloat16 kernels only): the three below are its operands
    const float *lora_rows = nullptr;  // [T][rank]: v (forward) or dv (input gradient)
    const float *lora_w = nullptr;     // [E][N][rank] B (forward) or [E][rank][K] A (input gradient)
    int rank = 0;
    bool nvfp4 = false;                // an NVFP4 entry: `scales` is [E][N][K / 16] e4m3 bytes, and
    const float *gscale = nullptr;     // [E] float32 or NULL (1): the per-tensor scales
};

// c as the call of an NVFP4 entry
Mx4Call with_nvfp4(Mx4Call c, const float *global_scale)
{
    c.nvfp4 = true; c.gscale = global_scale;
    return c;
}

// c with the operands of an adapter entry
Mx4Call with_lora(Mx4Call c, const float *rows, const float *w, int rank)
{
    c.lora = true; c.lora_rows = rows; c.lora_w = w; c.rank = rank;
    return c;
}

enum { ROWS_FLOAT = 0, ROWS_E4M3 = 1, ROWS_MXFP4 = 2, ROWS_MXFP6 = 3 };   // what c.rows holds; 1 .. 3 are the kernels' ROWS, 1 and 2 the scaled hooks' mode

// f(std::integral_constant<int, OUT>) for the element type of a call's output (valid_dtype() has been checked)
template <class F>
int with_out_dtype(int out_dtype, F &&f)
{
    switch (out_dtype) {
    case FQL_DTYPE_F32: return f(std::integral_constant<int, FQL_DTYPE_F32>{});
    case FQL_DTYPE_F16: return f(std::integral_constant<int, FQL_DTYPE_F16>{});
    default: return f(std::integral_constant<int, FQL_DTYPE_BF16>{});
    }
}
// ... and for the element type of its float rows (float32 or bfloat16: mx4_check has looked)
template <class F>
int with_in_dtype(int in_dtype, F &&f)
{
    return in_dtype == FQL_DTYPE_F32 ? f(std::integral_constant<int, FQL_DTYPE_F32>{}) : f(std::integral_constant<int, FQL_DTYPE_BF16>{});
}

// The grid of a grouped kernel with tiles of bt rows x bc columns of out [T][cols]: one more z-slice zeroes the rows no
// expert covers.
dim3 mx4_grid(const Mx4Call &c, int cols, int bc, int bt)
{
    return dim3((cols + bc - 1) / bc, (c.T + bt - 1) / bt, c.tpe != nullptr ? c.E + 1 : 1);
}

// Every forward has two kernels that return the same bits: the 64 x 128 tile and, for few rows, a one-wave decode kernel
// (fql_gemm_mx4_decode.h, fql_gemm_mx4_sdecode.h).  The per-expert counts stay on the device, so T alone decides, with a
// threshold for each kind of rows.
#define FQL_MX4_DECODE_MAX_ROWS 512    /* rows (T) up to which the decode kernel runs: the largest count of the sweep at which it wins */
#define FQL_MX4_F8_DECODE_MAX_ROWS 8   /* rows (T) up to which the fp8-row decode kernel runs: the largest count of the sweep up to which it wins at every point of both shapes */
#define FQL_MX4_F4_DECODE_MAX_ROWS 8   /* ... the MXFP4-row decode kernel: the same rule, the same count */
#define FQL_MX4_F6_DECODE_MAX_ROWS 8   /* ... the MXFP6-row decode kernel: the same rule */
int g_mx4_decode_max_rows[4] = {FQL_MX4_DECODE_MAX_ROWS, FQL_MX4_F8_DECODE_MAX_ROWS, FQL_MX4_F4_DECODE_MAX_ROWS,
                                FQL_MX4_F6_DECODE_MAX_ROWS};   // by rows kind

bool mx4_use_decode(int rows_kind, int T)
{
    static_assert(Mx4DecodeCfg::BT == Mx4SDecodeCfg::BT, "one bound on the grid's y for both decode kernels");
    return T > 0 && T <= g_mx4_decode_max_rows[rows_kind] && (T - 1) / Mx4DecodeCfg::BT + 1 <= 65535;   // (no overflow at a hook's T = INT_MAX)
}

// The bfloat16 forward: c.rows is [T][K] float32 or bfloat16.  An adapter call always takes the tile kernel (training: the
// decode kernel has no adapter form).
int launch_mx4(int in_dtype, int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using C = Mx4Cfg;
    using D = Mx4DecodeCfg;
    if (c.lora)
        return with_in_dtype(in_dtype, [&](auto in) {
            return with_out_dtype(out_dtype, [&](auto o) {
                return launch(mx4_kernel<decltype(in)::value, decltype(o)::value, Mx4Lora>, mx4_grid(c, c.N, C::BN, C::BT), dim3(C::THREADS), 0, st,
                              c.blocks, c.scales, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N, Mx4Lora{c.lora_rows, c.lora_w, c.rank});
            });
        });
    const bool decode = mx4_use_decode(ROWS_FLOAT, c.T);
    const dim3 grid = decode ? mx4_grid(c, c.N, D::BN, D::BT) : mx4_grid(c, c.N, C::BN, C::BT);
    return with_in_dtype(in_dtype, [&](auto in) {
        return with_out_dtype(out_dtype, [&](auto o) {
            constexpr int IN = decltype(in)::value, OUT = decltype(o)::value;
            return launch(decode ? mx4_decode_kernel<IN, OUT> : mx4_kernel<IN, OUT>, grid, dim3(decode ? D::THREADS : C::THREADS), 0, st,
                          c.blocks, c.scales, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
        });
    });
}

// The NVFP4 forward (fql_gemm_nvfp4.h): the same pair of kernels, the same bits from both, a threshold of its own.
#define FQL_NVFP4_DECODE_MAX_ROWS 512  /* rows (T) up to which the decode kernel runs: the largest count of the sweep up to which it wins at every point of both shapes */
int g_nvfp4_decode_max_rows = FQL_NVFP4_DECODE_MAX_ROWS;

bool nvfp4_use_decode(int T)
{
    return T > 0 && T <= g_nvfp4_decode_max_rows && (T - 1) / Mx4DecodeCfg::BT + 1 <= 65535;
}

int launch_nvfp4(int in_dtype, int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using C = Mx4Cfg;
    using D = Mx4DecodeCfg;
    if (c.lora)                                                       // (always the tile kernel, as launch_mx4's adapter call)
        return with_in_dtype(in_dtype, [&](auto in) {
            return with_out_dtype(out_dtype, [&](auto o) {
                return launch(nv4_kernel<decltype(in)::value, decltype(o)::value, Mx4Lora>, mx4_grid(c, c.N, C::BN, C::BT), dim3(C::THREADS), 0, st,
                              c.blocks, c.scales, c.gscale, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N,
                              Mx4Lora{c.lora_rows, c.lora_w, c.rank});
            });
        });
    const bool decode = nvfp4_use_decode(c.T);
    const dim3 grid = decode ? mx4_grid(c, c.N, D::BN, D::BT) : mx4_grid(c, c.N, C::BN, C::BT);
    return with_in_dtype(in_dtype, [&](auto in) {
        return with_out_dtype(out_dtype, [&](auto o) {
            constexpr int IN = decltype(in)::value, OUT = decltype(o)::value;
            return launch(decode ? nv4_decode_kernel<IN, OUT> : nv4_kernel<IN, OUT>, grid, dim3(decode ? D::THREADS : C::THREADS), 0, st,
                          c.blocks, c.scales, c.gscale, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
        });
    });
}

// The bfloat16 GEMM of a call with float rows, by the format of its weights.
int launch_float_rows(int in_dtype, int out_dtype, const Mx4Call &c, hipStream_t st)
{
    return c.nvfp4 ? launch_nvfp4(in_dtype, out_dtype, c, st) : launch_mx4(in_dtype, out_dtype, c, st);
}

// The block-scaled forward: c.rows is [T][K] e4m3 bytes with c.act_scale (ROWS_E4M3), or [T][K / 2] packed e2m1 with
// c.row_scales (ROWS_MXFP4), or [T][3 K / 4] packed e2m3 with c.row_scales (ROWS_MXFP6).
template <int ROWS>
int launch_mx4_scaled(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using C = Mx4ScaledCfg;
    using D = Mx4SDecodeCfg;
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the bfloat16 kernel's row tile");
    const bool decode = mx4_use_decode(ROWS, c.T);
    const dim3 grid = decode ? mx4_grid(c, c.N, D::BN, D::BT) : mx4_grid(c, c.N, C::BN, C::BT);
    return with_out_dtype(out_dtype, [&](auto o) {
        constexpr int OUT = decltype(o)::value;
        return launch(decode ? mx4_sdecode_kernel<ROWS, OUT> : mx4_scaled_kernel<ROWS, OUT>, grid, dim3(decode ? D::THREADS : C::THREADS),
                      0, st, c.blocks, c.scales, static_cast<const uint8_t *>(c.rows), c.row_scales, c.act_scale, c.bias, c.out, c.tpe,
                      c.offs, c.E, c.T, c.K, c.N);
    });
}

// The checks every entry point shares, in the documented order; `rows` is inputs or gate_up.  FQL_OK with *empty set: an
// empty call, nothing to launch.  rows_kind other than ROWS_FLOAT: the rows are bytes (in_dtype is not looked at); ROWS_MXFP4:
// packed rows [T][K / 2], 16-byte aligned, with c.row_scales; ROWS_MXFP6: packed rows [T][3 K / 4], 8-byte aligned (a row is a
// multiple of 24 bytes, so every block of every row is), with c.row_scales.
int mx4_check(const Mx4Call &c, int in_dtype, int out_dtype, bool act_ok, bool *empty, int rows_kind = ROWS_FLOAT)
{
    const bool byte_rows = rows_kind != ROWS_FLOAT;
    *empty = false;
    if (c.E <= 0 || c.T < 0 || c.K <= 0 || c.N < 0 || !act_ok) return FQL_ERR_BAD_SHAPE;
    if (c.K & 1) return FQL_ERR_ODD_K;
    if (c.K % 32 != 0) return FQL_ERR_BAD_SHAPE;                      // one scale per 32 inputs
    if ((!byte_rows && in_dtype != FQL_DTYPE_F32 && in_dtype != FQL_DTYPE_BF16) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (c.lora && c.rank != 4 && c.rank != 8 && c.rank != 16 && c.rank != 32 && c.rank != 64) return FQL_ERR_BAD_SHAPE;
    if (c.T == 0 || c.N == 0) { *empty = true; return FQL_OK; }
    if (!c.blocks || !c.scales || !c.rows || !c.out) return FQL_ERR_NULL_POINTER;
    if (c.lora && (!c.lora_rows || !c.lora_w)) return FQL_ERR_NULL_POINTER;
    if ((rows_kind == ROWS_MXFP4 || rows_kind == ROWS_MXFP6) && !c.row_scales) return FQL_ERR_NULL_POINTER;
    if ((c.tpe == nullptr) != (c.offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (c.tpe == nullptr && c.E != 1) return FQL_ERR_BAD_SHAPE;
    if (c.E > 65534) return FQL_ERR_BAD_SHAPE;                        // (the grid's z: the experts and the coverage slice)
    if ((c.T + Mx4Cfg::BT - 1) / Mx4Cfg::BT > 65535) return FQL_ERR_BAD_SHAPE;
    if ((long long)c.T * (c.K / 8) / 256 >= 0x7FFFFFFFLL) return FQL_ERR_BAD_SHAPE;
    const int ib = byte_rows ? 1 : dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!aligned16(c.blocks) || (reinterpret_cast<uintptr_t>(c.rows) & (ib - 1)) || (reinterpret_cast<uintptr_t>(c.out) & (ob - 1)) ||
        (reinterpret_cast<uintptr_t>(c.bias) & 3)) return FQL_ERR_ALIGNMENT;
    if ((reinterpret_cast<uintptr_t>(c.lora_rows) & 3) || (reinterpret_cast<uintptr_t>(c.lora_w) & 3)) return FQL_ERR_ALIGNMENT;   // (NULL without an adapter)
    if (reinterpret_cast<uintptr_t>(c.gscale) & 3) return FQL_ERR_ALIGNMENT;                                                        // (NULL but for NVFP4)
    if (rows_kind == ROWS_MXFP4 && !aligned16(c.rows)) return FQL_ERR_ALIGNMENT;
    if (rows_kind == ROWS_MXFP6 && (reinterpret_cast<uintptr_t>(c.rows) & 7)) return FQL_ERR_ALIGNMENT;
    return FQL_OK;
}

// The activation of a gated entry: a known kind, and for the kinds that read them a finite alpha and a positive finite limit.
bool mx4_act_ok(int activation, float act_alpha, float act_limit)
{
    bool act_ok = activation == FQL_ACT_SILU || activation == FQL_ACT_GELU_TANH || activation == FQL_ACT_SWIGLU_CLAMP;
    if (act_ok && activation != FQL_ACT_SILU)
        act_ok = std::isfinite(act_alpha) && std::isfinite(act_limit) && act_limit > 0.0f;
    return act_ok;
}

struct Mx4Act {                       // the element-wise step of a pre-pass: none, or act_glu_mul of a gate_up row
    bool gated;
    int kind;
    float alpha, limit;
    bool ok() const { return !gated || mx4_act_ok(kind, alpha, limit); }
};
const Mx4Act kMx4Plain{false, FQL_ACT_SILU, 0.0f, 0.0f};

// The workspace of a pre-pass by the rows it writes: h [T][K] bfloat16 | e4m3 rows [T][K], then act_scale [T] | packed rows
// [T][K / 2], then their scales [T][K / 32].  mx4_ws_rows: the bytes of the rows, what lies behind them starts there.
size_t mx4_ws_rows(int rows_kind, int T, int K)
{
    return round16(rows_kind == ROWS_FLOAT ? (size_t)T * K * 2 : rows_kind == ROWS_E4M3 ? (size_t)T * K :
                   rows_kind == ROWS_MXFP4 ? (size_t)T * (K / 2) : (size_t)T * (K / 4) * 3);
}
size_t mx4_ws_bytes(int rows_kind, int T, int K)
{
    return mx4_ws_rows(rows_kind, T, K) + (rows_kind == ROWS_FLOAT ? 0 : round16(rows_kind == ROWS_E4M3 ? (size_t)T * 4 : (size_t)T * (K / 32)));
}

// The pre-pass that writes rows of kind ROWS: rows (float rows [T][K], or gated: gate_up [T][2 K]) -> q, with `side` what
// goes with them (act_scale, the rows' scale bytes; none with bfloat16 rows, which exist gated only).  Packed MXFP6 rows are
// [T][3 K / 4].
template <int ROWS>
int launch_mx4_quant(const void *rows, int in_dtype, const Mx4Act &a, void *q, void *side, int T, int K, hipStream_t st)
{
    const dim3 grid(ROWS == ROWS_E4M3 ? (unsigned)((T + 3) / 4) : (unsigned)(((long long)T * (K / 8) + 255) / 256));   // a wave a row | a thread 8 k
    return with_in_dtype(in_dtype, [&](auto in) {
        auto go = [&](auto gated) {
            constexpr int IN = decltype(in)::value;
            constexpr bool GATED = decltype(gated)::value;
            if constexpr (ROWS == ROWS_FLOAT)
                return launch(mx4_glu_kernel<IN>, grid, dim3(256), 0, st, rows, static_cast<unsigned short *>(q), T, K, a.kind, a.alpha, a.limit);
            else if constexpr (ROWS == ROWS_E4M3)
                return launch(mx4_q8_kernel<IN, GATED>, grid, dim3(256), 0, st, rows, static_cast<uint8_t *>(q), static_cast<float *>(side),
                              T, K, a.kind, a.alpha, a.limit);
            else if constexpr (ROWS == ROWS_MXFP6)
                return launch(mx4_q6_kernel<IN, GATED>, grid, dim3(256), 0, st, rows, static_cast<uint8_t *>(q), static_cast<uint8_t *>(side),
                              T, K, a.kind, a.alpha, a.limit);
            else
                return launch(mx4_q4_kernel<IN, GATED>, grid, dim3(256), 0, st, rows, static_cast<uint8_t *>(q), static_cast<uint8_t *>(side),
                              T, K, a.kind, a.alpha, a.limit);
        };
        return a.gated ? go(std::true_type{}) : go(std::false_type{});
    });
}

// An entry that runs a pre-pass into the workspace and then the GEMM on what it wrote: the checks, the workspace, the two
// launches.
template <int ROWS>
int mx4_quant_fwd(Mx4Call c, int in_dtype, int out_dtype, const Mx4Act &a, void *workspace, size_t workspace_bytes, void *stream)
{
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, a.ok(), &empty);
    if (rc != FQL_OK || empty) return rc;
    if (!workspace || !aligned16(workspace) || workspace_bytes < mx4_ws_bytes(ROWS, c.T, c.K)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *q = static_cast<uint8_t *>(workspace), *side = q + mx4_ws_rows(ROWS, c.T, c.K);
    const int lrc = launch_mx4_quant<ROWS>(c.rows, in_dtype, a, q, side, c.T, c.K, st);
    if (lrc != FQL_OK) return lrc;
    c.rows = q;
    if constexpr (ROWS == ROWS_FLOAT) {
        return launch_float_rows(FQL_DTYPE_BF16, out_dtype, c, st);
    } else {
        if constexpr (ROWS == ROWS_E4M3) c.act_scale = reinterpret_cast<const float *>(side);
        else c.row_scales = side;
        return launch_mx4_scaled<ROWS>(out_dtype, c, st);
    }
}

// An entry whose rows are quantised already.
template <int ROWS>
int mx4_scaled_fwd(const Mx4Call &c, int out_dtype, void *stream)
{
    bool empty;
    const int rc = mx4_check(c, 0, out_dtype, true, &empty, ROWS);
    if (rc != FQL_OK || empty) return rc;
    if (reinterpret_cast<uintptr_t>(c.act_scale) & 3) return FQL_ERR_ALIGNMENT;   // (NULL with MXFP4 rows)
    return launch_mx4_scaled<ROWS>(out_dtype, c, static_cast<hipStream_t>(stream));
}

// ---- the dense linear layer (fql_linear_mx4_fwd / fql_linear_mx4_glu_fwd): E = 1, no table, and with split_k set and few rows
//      the decode kernel cut along K (fql_gemm_mx4_linear.h) ----
#define FQL_MX4_LINEAR_DECODE_MAX_ROWS 16   /* rows (T) up to which the split form runs: the largest count of the sweep up to which it beats both grouped kernels at every shape whose S is above 1 */
#define FQL_MX4_LINEAR_MAX_SLICES 16
#define FQL_MX4_LINEAR_FILL_WAVES 640       /* the waves S(K, N) asks for: 2.5 a compute unit, from the S sweep of the same section */
int g_mx4_linear_decode_max_rows = FQL_MX4_LINEAR_DECODE_MAX_ROWS;
int g_mx4_linear_slices = 0;           // 0: the policy below; 1 / 2 / 4 / 8 / 16: forced (fql_tune_set_mx4_linear_slices)

// S(K, N): the slices of the split form, a pure function of the weights' shape (never of T or the device).  The smallest
// S of {1, 2, 4, 8, 16} with ceil(N / 32) * S >= FQL_MX4_LINEAR_FILL_WAVES, capped at max(1, P) with P = K / 64 whole
// pairs, so that no slice of the policy's is empty.  (The rule the work started from asked for 1024, a wave a SIMD; the
// sweep's winners at one row are what 640 gives on all five shapes: 4, 8, 4, 1, 4.  Past that the partial sums' traffic
// and the second launch cost more than the shorter K loop saves, and N = 28672 has 896 waves without help.)
int mx4_linear_policy_slices(int K, int N)
{
    const long long waves = ((long long)N + Mx4DecodeCfg::BN - 1) / Mx4DecodeCfg::BN;
    int S = 1;
    while (S < FQL_MX4_LINEAR_MAX_SLICES && waves * S < FQL_MX4_LINEAR_FILL_WAVES) S *= 2;
    const int P = K / 64;
    while (S > 1 && S > P) S /= 2;
    return S;
}

// The slices a call with split_k set runs now: 1 means no split form (the call goes the split_k == 0 way).
int mx4_linear_slices(int T, int K, int N)
{
    if (T <= 0 || T > g_mx4_linear_decode_max_rows || (T - 1) / Mx4DecodeCfg::BT + 1 > 65535) return 1;
    return g_mx4_linear_slices != 0 ? g_mx4_linear_slices : mx4_linear_policy_slices(K, N);
}

// The partial sums of the split form: [16][T][N] float32, sized for the largest S so that the hook cannot outgrow it.
size_t mx4_linear_partial_bytes(int T, int N, int split_k)
{
    if (!split_k || T <= 0 || N <= 0 || T > g_mx4_linear_decode_max_rows) return 0;
    return (size_t)FQL_MX4_LINEAR_MAX_SLICES * sizeof(float) * (size_t)T * (size_t)N;
}
size_t mx4_linear_h_bytes(int T, int K, int gated) { return gated && T > 0 && K > 0 ? mx4_ws_bytes(ROWS_FLOAT, T, K) : 0; }

// The two launches of the split form: the sliced decode kernel into partial [S][T][N], then the reduce kernel.
int launch_mx4_linear_split(int in_dtype, int out_dtype, const Mx4Call &c, int S, float *partial, hipStream_t st)
{
    using D = Mx4DecodeCfg;
    using R = Mx4LinearReduceCfg;
    const dim3 grid((c.N + D::BN - 1) / D::BN, (c.T + D::BT - 1) / D::BT, S);
    const int rc = with_in_dtype(in_dtype, [&](auto in) {
        return launch(mx4_linear_decode_kernel<decltype(in)::value>, grid, dim3(D::THREADS), 0, st, c.blocks, c.scales, c.rows, partial,
                      c.T, c.K, c.N);
    });
    if (rc != FQL_OK) return rc;
    const int row_blocks = (c.T + R::ROWS - 1) / R::ROWS;
    const dim3 rgrid((c.N + R::COLS - 1) / R::COLS, row_blocks < 65535 ? row_blocks : 65535);
    return with_out_dtype(out_dtype, [&](auto o) {
        constexpr int OUT = decltype(o)::value;
        auto go = [&](auto s) {
            return launch(mx4_linear_reduce_kernel<OUT, decltype(s)::value>, rgrid, dim3(R::THREADS), 0, st, partial, c.bias, c.out, c.T, c.N);
        };
        switch (S) {
        case 2: return go(std::integral_constant<int, 2>{});
        case 4: return go(std::integral_constant<int, 4>{});
        case 8: return go(std::integral_constant<int, 8>{});
        default: return go(std::integral_constant<int, 16>{});
        }
    });
}

// Both linear entries: the checks of mx4_check with E = 1 and no table, the workspace, then the launches.
int mx4_linear_fwd(Mx4Call c, int in_dtype, int out_dtype, const Mx4Act &a, int split_k, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, a.ok(), &empty);
    if (rc != FQL_OK || empty) return rc;
    const size_t h_bytes = mx4_linear_h_bytes(c.T, c.K, a.gated);
    const size_t need = h_bytes + mx4_linear_partial_bytes(c.T, c.N, split_k);
    if (need != 0 && (!workspace || !aligned16(workspace) || workspace_bytes < need)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    if (a.gated) {
        const int lrc = launch_mx4_quant<ROWS_FLOAT>(c.rows, in_dtype, a, ws, nullptr, c.T, c.K, st);
        if (lrc != FQL_OK) return lrc;
        c.rows = ws;
        in_dtype = FQL_DTYPE_BF16;
    }
    const int S = split_k ? mx4_linear_slices(c.T, c.K, c.N) : 1;
    if (S > 1) return launch_mx4_linear_split(in_dtype, out_dtype, c, S, reinterpret_cast<float *>(ws + h_bytes), st);
    return launch_float_rows(in_dtype, out_dtype, c, st);
}

}  // namespace

extern "C" {

FQL_API size_t fql_moe_mx4_workspace_bytes(int E, int T, int K, int N, int gated)
{
    (void)E; (void)N;
    if (!gated || T <= 0 || K <= 0) return 0;
    return mx4_ws_bytes(ROWS_FLOAT, T, K);                            // h [T][K] bfloat16
}

FQL_API int fql_moe_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                            const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                            int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    const Mx4Call c{blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_FLOAT>({blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                     out_dtype, {true, activation, act_alpha, act_limit}, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                  int out_dtype, int E, int T, int K, int N, void *stream)
{
    using C = Mx4BwdCfg;
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the forward's row tile");
    const Mx4Call c{blocks, scales_e8m0, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N};
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty) {
        if (T == 0) return FQL_OK;
        // N == 0: the gradient of an empty contraction.  grad_in [T][K] is zeros and no other operand is read.
        if (!grad_in) return FQL_ERR_NULL_POINTER;
        (void)hipGetLastError();
        return hipMemsetAsync(grad_in, 0, (size_t)T * K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    return with_in_dtype(in_dtype, [&](auto in) {                     // c.rows is grad_out [T][N], c.out grad_in [T][K]
        return with_out_dtype(out_dtype, [&](auto o) {
            return launch(mx4_bwd_kernel<decltype(in)::value, decltype(o)::value>, mx4_grid(c, K, C::BK, C::BT), dim3(C::THREADS), 0, st, c.blocks, c.scales, c.rows, c.out,
                          c.tpe, c.offs, c.E, c.T, c.K, c.N);
        });
    });
}

FQL_API int fql_moe_mx4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                                 const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                 const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                 int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    const Mx4Call c = with_lora({blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, lora_rows, lora_B, rank);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_mx4_glu_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                     const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                     const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                                     int E, int T, int K, int N, int activation, float act_alpha, float act_limit,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_FLOAT>(with_lora({blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                               lora_rows, lora_B, rank), in_dtype, out_dtype, {true, activation, act_alpha, act_limit},
                                     workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                       const float *lora_rows, const float *lora_A, int rank, const int32_t *tokens_per_expert,
                                       const int32_t *input_offsets, void *grad_in, int out_dtype, int E, int T, int K, int N,
                                       void *stream)
{
    using C = Mx4BwdCfg;
    const Mx4Call c = with_lora({blocks, scales_e8m0, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N}, lora_rows,
                                lora_A, rank);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK) return rc;
    if (empty) return T == 0 ? FQL_OK : FQL_ERR_BAD_SHAPE;            // (N == 0 with rows: dv A alone is not this entry's business)
    return with_in_dtype(in_dtype, [&](auto in) {                     // c.rows is grad_out [T][N], c.out grad_in [T][K]
        return with_out_dtype(out_dtype, [&](auto o) {
            return launch(mx4_bwd_kernel<decltype(in)::value, decltype(o)::value, Mx4Lora>, mx4_grid(c, K, C::BK, C::BT), dim3(C::THREADS), 0,
                          static_cast<hipStream_t>(stream), c.blocks, c.scales, c.rows, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N,
                          Mx4Lora{c.lora_rows, c.lora_w, c.rank});
        });
    });
}

FQL_API size_t fql_moe_mx4_f8_workspace_bytes(int E, int T, int K, int N, int mode)
{
    (void)E; (void)N;
    if ((mode != 1 && mode != 2) || T <= 0 || K <= 0) return 0;
    return mx4_ws_bytes(ROWS_E4M3, T, K);                             // e4m3 rows [T][K], act_scale [T]
}

FQL_API int fql_moe_mx4_fwd_f8(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *inputs_e4m3,
                               const float *act_scale, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    return mx4_scaled_fwd<ROWS_E4M3>({blocks, scales_e8m0, inputs_e4m3, bias, tokens_per_expert, input_offsets, out, E, T, K, N, act_scale},
                                     out_dtype, stream);
}

FQL_API int fql_moe_mx4_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_E4M3>({blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                    out_dtype, kMx4Plain, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_glu_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_E4M3>({blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                    out_dtype, {true, activation, act_alpha, act_limit}, workspace, workspace_bytes, stream);
}

FQL_API size_t fql_moe_mx4_f4_workspace_bytes(int E, int T, int K, int N, int mode)
{
    (void)E; (void)N;
    if ((mode != 1 && mode != 2) || T <= 0 || K <= 0) return 0;
    return mx4_ws_bytes(ROWS_MXFP4, T, K);                            // packed rows [T][K / 2], their scales [T][K / 32]
}

FQL_API int fql_moe_mx4_fwd_f4(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *in_blocks,
                               const uint8_t *in_scales_e8m0, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    return mx4_scaled_fwd<ROWS_MXFP4>({blocks, scales_e8m0, in_blocks, bias, tokens_per_expert, input_offsets, out, E, T, K, N, nullptr,
                                       in_scales_e8m0}, out_dtype, stream);
}

FQL_API int fql_moe_mx4_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_MXFP4>({blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                     out_dtype, kMx4Plain, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_glu_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_MXFP4>({blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                     out_dtype, {true, activation, act_alpha, act_limit}, workspace, workspace_bytes, stream);
}

FQL_API size_t fql_moe_mx4_f6_workspace_bytes(int E, int T, int K, int N, int mode)
{
    (void)E; (void)N;
    if ((mode != 1 && mode != 2) || T <= 0 || K <= 0) return 0;
    return mx4_ws_bytes(ROWS_MXFP6, T, K);                            // packed rows [T][3 K / 4], their scales [T][K / 32]
}

FQL_API int fql_moe_mx4_fwd_f6(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *in_codes,
                               const uint8_t *in_scales_e8m0, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    return mx4_scaled_fwd<ROWS_MXFP6>({blocks, scales_e8m0, in_codes, bias, tokens_per_expert, input_offsets, out, E, T, K, N, nullptr,
                                       in_scales_e8m0}, out_dtype, stream);
}

FQL_API int fql_moe_mx4_fwd_q6(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_MXFP6>({blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                     out_dtype, kMx4Plain, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_glu_fwd_q6(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_MXFP6>({blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype,
                                     out_dtype, {true, activation, act_alpha, act_limit}, workspace, workspace_bytes, stream);
}

FQL_API int fql_mx4_quantize_rows(const void *rows, int in_dtype, int gated, int activation, float act_alpha, float act_limit,
                                  uint8_t *out_blocks, uint8_t *out_scales, int T, int K, void *stream)
{
    // mx4_check on a call record with one expert, one column and no table: out_blocks stands for both `blocks` (non-NULL,
    // 16-byte aligned) and `out`, out_scales for `scales`; the documented order is fql_moe_mx4_fwd's.
    const Mx4Call c{out_blocks, out_scales, rows, nullptr, nullptr, nullptr, out_blocks, 1, T, K, 1};
    const Mx4Act a{gated != 0, activation, act_alpha, act_limit};
    bool empty;
    const int rc = mx4_check(c, in_dtype, FQL_DTYPE_F32, a.ok(), &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4_quant<ROWS_MXFP4>(rows, in_dtype, a, out_blocks, out_scales, T, K, static_cast<hipStream_t>(stream));
}

FQL_API int fql_mx6_quantize_rows(const void *rows, int in_dtype, int gated, int activation, float act_alpha, float act_limit,
                                  uint8_t *out_codes, uint8_t *out_scales, int T, int K, void *stream)
{
    // as fql_mx4_quantize_rows: out_codes stands for `blocks` (non-NULL, 16-byte aligned) and `out`, out_scales for `scales`
    const Mx4Call c{out_codes, out_scales, rows, nullptr, nullptr, nullptr, out_codes, 1, T, K, 1};
    const Mx4Act a{gated != 0, activation, act_alpha, act_limit};
    bool empty;
    const int rc = mx4_check(c, in_dtype, FQL_DTYPE_F32, a.ok(), &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_mx4_quant<ROWS_MXFP6>(rows, in_dtype, a, out_codes, out_scales, T, K, static_cast<hipStream_t>(stream));
}

FQL_API size_t fql_linear_mx4_workspace_bytes(int T, int K, int N, int gated, int split_k)
{
    return mx4_linear_h_bytes(T, K, gated) + mx4_linear_partial_bytes(T, N, split_k);   // h [T][K] bfloat16 | partial [16][T][N] float32
}

FQL_API int fql_linear_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, void *out, int out_dtype, int T, int K, int N, int split_k, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd({blocks, scales_e8m0, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, in_dtype, out_dtype, kMx4Plain,
                          split_k, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, void *out, int out_dtype, int T, int K, int N, int activation,
                                   float act_alpha, float act_limit, int split_k, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    return mx4_linear_fwd({blocks, scales_e8m0, gate_up, bias, nullptr, nullptr, out, 1, T, K, N}, in_dtype, out_dtype,
                          {true, activation, act_alpha, act_limit}, split_k, workspace, workspace_bytes, stream);
}

FQL_API size_t fql_moe_nvfp4_workspace_bytes(int E, int T, int K, int N, int gated)
{
    return fql_moe_mx4_workspace_bytes(E, T, K, N, gated);            // h [T][K] bfloat16, as the MXFP4 entries'
}

FQL_API int fql_moe_nvfp4_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                              int in_dtype, const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                              void *out, int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes,
                              void *stream)
{
    (void)workspace; (void)workspace_bytes;
    const Mx4Call c = with_nvfp4({blocks, scales_e4m3, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, global_scale);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_nvfp4(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_nvfp4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *gate_up,
                                  int in_dtype, const float *bias, const int32_t *tokens_per_expert,
                                  const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                                  int activation, float act_alpha, float act_limit, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    return mx4_quant_fwd<ROWS_FLOAT>(with_nvfp4({blocks, scales_e4m3, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                                global_scale), in_dtype, out_dtype, {true, activation, act_alpha, act_limit},
                                     workspace, workspace_bytes, stream);
}

FQL_API size_t fql_linear_nvfp4_workspace_bytes(int T, int K, int N, int gated)
{
    (void)N;
    return mx4_linear_h_bytes(T, K, gated);                           // h [T][K] bfloat16
}

FQL_API int fql_linear_nvfp4_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                 int in_dtype, const float *bias, void *out, int out_dtype, int T, int K, int N, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd(with_nvfp4({blocks, scales_e4m3, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale), in_dtype,
                          out_dtype, kMx4Plain, 0, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_nvfp4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                     const void *gate_up, int in_dtype, const float *bias, void *out, int out_dtype, int T, int K,
                                     int N, int activation, float act_alpha, float act_limit, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd(with_nvfp4({blocks, scales_e4m3, gate_up, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale), in_dtype,
                          out_dtype, {true, activation, act_alpha, act_limit}, 0, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_nvfp4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *grad_out,
                                    int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                    int out_dtype, int E, int T, int K, int N, void *stream)
{
    using C = Mx4BwdCfg;
    const Mx4Call c = with_nvfp4({blocks, scales_e4m3, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N}, global_scale);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty) {
        if (T == 0) return FQL_OK;
        // N == 0: the gradient of an empty contraction.  grad_in [T][K] is zeros and no other operand is read.
        if (!grad_in) return FQL_ERR_NULL_POINTER;
        (void)hipGetLastError();
        return hipMemsetAsync(grad_in, 0, (size_t)T * K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    return with_in_dtype(in_dtype, [&](auto in) {                     // c.rows is grad_out [T][N], c.out grad_in [T][K]
        return with_out_dtype(out_dtype, [&](auto o) {
            return launch(nv4_bwd_kernel<decltype(in)::value, decltype(o)::value>, mx4_grid(c, K, C::BK, C::BT), dim3(C::THREADS), 0, st, c.blocks, c.scales, c.gscale,
                          c.rows, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N);
        });
    });
}

FQL_API int fql_moe_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                   int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                   const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                   int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    const Mx4Call c = with_lora(with_nvfp4({blocks, scales_e4m3, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                           global_scale), lora_rows, lora_B, rank);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_nvfp4(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
}

FQL_API int fql_moe_nvfp4_glu_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                       const void *gate_up, int in_dtype, const float *lora_rows, const float *lora_B, int rank,
                                       const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                       void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                       float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_FLOAT>(with_lora(with_nvfp4({blocks, scales_e4m3, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                                          global_scale), lora_rows, lora_B, rank), in_dtype, out_dtype,
                                     {true, activation, act_alpha, act_limit}, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_nvfp4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                         const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A, int rank,
                                         const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                         int out_dtype, int E, int T, int K, int N, void *stream)
{
    using C = Mx4BwdCfg;
    const Mx4Call c = with_lora(with_nvfp4({blocks, scales_e4m3, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N},
                                           global_scale), lora_rows, lora_A, rank);
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK) return rc;
    if (empty) return T == 0 ? FQL_OK : FQL_ERR_BAD_SHAPE;            // (N == 0 with rows: dv A alone is not this entry's business)
    return with_in_dtype(in_dtype, [&](auto in) {                     // c.rows is grad_out [T][N], c.out grad_in [T][K]
        return with_out_dtype(out_dtype, [&](auto o) {
            return launch(nv4_bwd_kernel<decltype(in)::value, decltype(o)::value, Mx4Lora>, mx4_grid(c, K, C::BK, C::BT), dim3(C::THREADS), 0,
                          static_cast<hipStream_t>(stream), c.blocks, c.scales, c.gscale, c.rows, c.out, c.tpe, c.offs, c.E, c.T, c.K,
                          c.N, Mx4Lora{c.lora_rows, c.lora_w, c.rank});
        });
    });
}

FQL_API int fql_linear_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                      int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                      void *out, int out_dtype, int T, int K, int N, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    return mx4_linear_fwd(with_lora(with_nvfp4({blocks, scales_e4m3, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale),
                                    lora_rows, lora_B, rank), in_dtype, out_dtype, kMx4Plain, 0, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_nvfp4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                            const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A,
                                            int rank, void *grad_in, int out_dtype, int T, int K, int N, void *stream)
{
    return fql_moe_nvfp4_lora_bwd_input(blocks, scales_e4m3, global_scale, grad_out, in_dtype, lora_rows, lora_A, rank, nullptr,
                                        nullptr, grad_in, out_dtype, 1, T, K, N, stream);
}

FQL_API int fql_tune_set_nvfp4_decode_max_rows(int rows)
{
    const int old = g_nvfp4_decode_max_rows;
    if (rows >= 0) g_nvfp4_decode_max_rows = rows;
    return old;
}

FQL_API int fql_tune_nvfp4_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return nvfp4_use_decode(T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_linear_decode_max_rows(int rows)
{
    const int old = g_mx4_linear_decode_max_rows;
    if (rows >= 0) g_mx4_linear_decode_max_rows = rows;
    return old;
}

FQL_API int fql_tune_set_mx4_linear_slices(int slices)
{
    const int old = g_mx4_linear_slices;
    if (slices == 0 || slices == 1 || slices == 2 || slices == 4 || slices == 8 || slices == 16) g_mx4_linear_slices = slices;
    return old;
}

FQL_API int fql_tune_mx4_linear_kernel(int T, int K, int N)
{
    const int S = mx4_linear_slices(T, K, N);
    return (S << 8) | (S > 1 ? 2 : mx4_use_decode(ROWS_FLOAT, T) ? 1 : 0);
}

FQL_API int fql_tune_set_mx4_decode_max_rows(int rows)
{
    const int old = g_mx4_decode_max_rows[ROWS_FLOAT];
    if (rows >= 0) g_mx4_decode_max_rows[ROWS_FLOAT] = rows;
    return old;
}

FQL_API int fql_tune_mx4_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return mx4_use_decode(ROWS_FLOAT, T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_scaled_decode_max_rows(int mode, int rows)
{
    if (mode != ROWS_E4M3 && mode != ROWS_MXFP4) return -1;
    const int old = g_mx4_decode_max_rows[mode];
    if (rows >= 0) g_mx4_decode_max_rows[mode] = rows;
    return old;
}

FQL_API int fql_tune_mx4_scaled_kernel(int mode, int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    if (mode != ROWS_E4M3 && mode != ROWS_MXFP4) return -1;
    return mx4_use_decode(mode, T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_f6_decode_max_rows(int rows)
{
    const int old = g_mx4_decode_max_rows[ROWS_MXFP6];
    if (rows >= 0) g_mx4_decode_max_rows[ROWS_MXFP6] = rows;
    return old;
}

FQL_API int fql_tune_mx4_f6_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return mx4_use_decode(ROWS_MXFP6, T) ? 1 : 0;
}

}  // extern "C"
