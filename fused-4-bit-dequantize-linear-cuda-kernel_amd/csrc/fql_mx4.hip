// libfql_int4.so, the 4-bit float weight families (include/fql_int4.h).  Host-side validation and launches only, as in
// fql_int4.hip: no allocation, no synchronisation.  DESIGN.md section 47 describes how the host code below is shared.
//
//   family                      entries                                                          kernels
//   MXFP4 experts, float rows   fql_moe_mx4_fwd / _glu_fwd / _bwd_input                          fql_gemm_mx4.h, fql_gemm_mx4_decode.h,
//     with an adapter           fql_moe_mx4_lora_fwd / _glu_lora_fwd / _lora_bwd_input           fql_gemm_mx4_bwd.h (LORA: a flag of the tile kernels)
//   MXFP4 experts, scaled rows  fql_moe_mx4_fwd_f8 / _fwd_q8 / _glu_fwd_q8 (fp8 rows),           fql_gemm_mx4_scaled.h, fql_gemm_mx4_sdecode.h
//                               _fwd_f4 / _fwd_q4 / _glu_fwd_q4 (MXFP4), _f6 / _q6 (MXFP6)       (one tile and one decode kernel for the three)
//   row pre-passes              fql_mx4_quantize_rows / fql_mx6_quantize_rows                    fql_mx4_quant.h
//   MXFP4 dense                 fql_linear_mx4_fwd / _glu_fwd (split_k: the split-K decode form) fql_gemm_mx4_linear.h
//   NVFP4 experts and dense     fql_moe_nvfp4_fwd / _glu_fwd / _bwd_input,                       fql_gemm_nvfp4.h, fql_gemm_nvfp4_bwd.h
//                               fql_linear_nvfp4_fwd / _glu_fwd
//     with an adapter           fql_moe_nvfp4_lora_fwd / _glu_lora_fwd / _lora_bwd_input,        (LORA: a flag of the two tile kernels)
//                               fql_linear_nvfp4_lora_fwd / _lora_bwd_input
//     split-K decode form       fql_linear_nvfp4_split_fwd / _glu_split_fwd                      fql_gemm_nvfp4_linear.h
//   code book (NF4), dense      fql_linear_lut4_fwd / _bwd_input                                 fql_gemm_lut4.h, fql_gemm_lut4_bwd.h
//     with an adapter           fql_linear_lut4_lora_fwd / _lora_bwd_input                       (LORA: a flag of the two tile kernels)
//     split-K decode form       fql_linear_lut4_split_fwd                                        fql_gemm_lut4_decode.h
//   code book (NF4), grouped    fql_moe_lut4_fwd / _glu_fwd / _bwd_input                         fql_gemm_lut4_group.h, fql_gemm_lut4_bwd.h
//     decode forms              (the same entries, by T) / fql_moe_lut4_split_fwd / _glu_split_fwd  fql_gemm_lut4_group_decode.h
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
#include "fql_gemm_nvfp4_linear.h"
#include "fql_gemm_lut4.h"
#include "fql_gemm_lut4_bwd.h"
#include "fql_gemm_lut4_decode.h"
#include "fql_gemm_lut4_group.h"
#include "fql_gemm_lut4_group_decode.h"

#include <cmath>

namespace {

using namespace fql_host;

// The operands of an adapter entry (the tile kernels only), the same in every family's call record.
struct LoraOperands {
    bool on = false;                   // an adapter entry: the three below are its operands
    const float *rows = nullptr;       // [T][rank]: v (forward) or dv (input gradient)
    const float *w = nullptr;          // [E][N][rank] B (forward) or [E][rank][K] A (input gradient); dense: E = 1
    int rank = 0;
};

// c (an Mx4Call or a Lut4Call) with the operands of an adapter entry
template <class Call>
Call with_lora(Call c, const float *rows, const float *w, int rank)
{
    c.lora = {true, rows, w, rank};
    return c;
}

// The three tests of an adapter's operands; mx4_check and lut4_check each place them in their documented order.
bool lora_rank_bad(const LoraOperands &l) { return l.on && l.rank != 4 && l.rank != 8 && l.rank != 16 && l.rank != 32 && l.rank != 64; }
bool lora_null(const LoraOperands &l) { return l.on && (!l.rows || !l.w); }
bool lora_misaligned(const LoraOperands &l)                          // (both NULL without an adapter)
{
    return (reinterpret_cast<uintptr_t>(l.rows) & 3) || (reinterpret_cast<uintptr_t>(l.w) & 3);
}

// f(), or f(Mx4Lora) for an adapter call: the one kernel argument more of a tile kernel's LORA form
template <class F>
int with_lora_arg(const LoraOperands &l, F &&f)
{
    return l.on ? f(Mx4Lora{l.rows, l.w, l.rank}) : f();
}

struct Mx4Call {
    const uint8_t *blocks, *scales;
    const void *rows;                 // [T][K] of in_dtype
    const float *bias;
    const int32_t *tpe, *offs;
    void *out;
    int E, T, K, N;
    const float *act_scale = nullptr;  // [T] or NULL (fp8 rows only)
    const uint8_t *row_scales = nullptr;  // [T][K / 32] E8M0 (MXFP4 and MXFP6 rows only)
    LoraOperands lora;                 // (bfloat16 kernels only)
    bool nvfp4 = false;                // an NVFP4 entry: `scales` is [E][N][K / 16] e4m3 bytes, and
    const float *gscale = nullptr;     // [E] float32 or NULL (1): the per-tensor scales
};

// c as the call of an NVFP4 entry
Mx4Call with_nvfp4(Mx4Call c, const float *global_scale)
{
    c.nvfp4 = true; c.gscale = global_scale;
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
// ... and f(in, out) for both: the nest around every kernel with the two element types as template arguments
template <class F>
int with_dtypes(int in_dtype, int out_dtype, F &&f)
{
    return with_in_dtype(in_dtype, [&](auto in) { return with_out_dtype(out_dtype, [&](auto o) { return f(in, o); }); });
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
// The NVFP4 forward (fql_gemm_nvfp4.h): the same pair of kernels, the same bits from both, a threshold of its own.
#define FQL_NVFP4_DECODE_MAX_ROWS 512  /* rows (T) up to which the decode kernel runs: the largest count of the sweep up to which it wins at every point of both shapes */
int g_nvfp4_decode_max_rows = FQL_NVFP4_DECODE_MAX_ROWS;

// The row-threshold predicate of every decode kernel, one-wave or split: all of them run on row tiles of Mx4DecodeCfg::BT.
bool decode_rows(int max_rows, int T)
{
    static_assert(Mx4DecodeCfg::BT == Mx4SDecodeCfg::BT, "one bound on the grid's y for both decode kernels");
    return T > 0 && T <= max_rows && (T - 1) / Mx4DecodeCfg::BT + 1 <= 65535;   // (no overflow at a hook's T = INT_MAX)
}

// The bfloat16 GEMM of a call with float rows (float32 or bfloat16), MXFP4 or NVFP4 weights by c.nvfp4.  An adapter call
// always takes the tile kernel (training: the decode kernel has no adapter form).
int launch_float_rows(int in_dtype, int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using C = Mx4Cfg;
    using D = Mx4DecodeCfg;
    const bool decode = !c.lora.on && decode_rows(c.nvfp4 ? g_nvfp4_decode_max_rows : g_mx4_decode_max_rows[ROWS_FLOAT], c.T);
    const dim3 grid = decode ? mx4_grid(c, c.N, D::BN, D::BT) : mx4_grid(c, c.N, C::BN, C::BT);
    const dim3 block(decode ? D::THREADS : C::THREADS);
    // one launch per kernel signature: the NVFP4 kernels take the per-tensor scales behind the block scales
    auto mx = [&](auto kern, auto... la) {
        return launch(kern, grid, block, 0, st, c.blocks, c.scales, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N, la...);
    };
    auto nv = [&](auto kern, auto... la) {
        return launch(kern, grid, block, 0, st, c.blocks, c.scales, c.gscale, c.rows, c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N, la...);
    };
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        constexpr int IN = decltype(in)::value, OUT = decltype(o)::value;
        if (decode) return c.nvfp4 ? nv(nv4_decode_kernel<IN, OUT>) : mx(mx4_decode_kernel<IN, OUT>);
        return with_lora_arg(c.lora, [&](auto... la) {
            return c.nvfp4 ? nv(nv4_kernel<IN, OUT, decltype(la)...>, la...) : mx(mx4_kernel<IN, OUT, decltype(la)...>, la...);
        });
    });
}

// The block-scaled forward: c.rows is [T][K] e4m3 bytes with c.act_scale (ROWS_E4M3), or [T][K / 2] packed e2m1 with
// c.row_scales (ROWS_MXFP4), or [T][3 K / 4] packed e2m3 with c.row_scales (ROWS_MXFP6).
template <int ROWS>
int launch_mx4_scaled(int out_dtype, const Mx4Call &c, hipStream_t st)
{
    using C = Mx4ScaledCfg;
    using D = Mx4SDecodeCfg;
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the bfloat16 kernel's row tile");
    const bool decode = decode_rows(g_mx4_decode_max_rows[ROWS], c.T);
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
    if (lora_rank_bad(c.lora)) return FQL_ERR_BAD_SHAPE;
    if (c.T == 0 || c.N == 0) { *empty = true; return FQL_OK; }
    if (!c.blocks || !c.scales || !c.rows || !c.out) return FQL_ERR_NULL_POINTER;
    if (lora_null(c.lora)) return FQL_ERR_NULL_POINTER;
    if ((rows_kind == ROWS_MXFP4 || rows_kind == ROWS_MXFP6) && !c.row_scales) return FQL_ERR_NULL_POINTER;
    if ((c.tpe == nullptr) != (c.offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (c.tpe == nullptr && c.E != 1) return FQL_ERR_BAD_SHAPE;
    if (c.E > 65534) return FQL_ERR_BAD_SHAPE;                        // (the grid's z: the experts and the coverage slice)
    if ((c.T + Mx4Cfg::BT - 1) / Mx4Cfg::BT > 65535) return FQL_ERR_BAD_SHAPE;
    if ((long long)c.T * (c.K / 8) / 256 >= 0x7FFFFFFFLL) return FQL_ERR_BAD_SHAPE;
    const int ib = byte_rows ? 1 : dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!aligned16(c.blocks) || (reinterpret_cast<uintptr_t>(c.rows) & (ib - 1)) || (reinterpret_cast<uintptr_t>(c.out) & (ob - 1)) ||
        (reinterpret_cast<uintptr_t>(c.bias) & 3)) return FQL_ERR_ALIGNMENT;
    if (lora_misaligned(c.lora)) return FQL_ERR_ALIGNMENT;
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

// A grouped entry on float rows with nothing before the GEMM: the checks, the launch.
int mx4_float_fwd(const Mx4Call &c, int in_dtype, int out_dtype, void *stream)
{
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK || empty) return rc;
    return launch_float_rows(in_dtype, out_dtype, c, static_cast<hipStream_t>(stream));
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

// The input gradient of a grouped entry, MXFP4 or NVFP4 weights, with or without an adapter: c.rows is grad_out [T][N],
// c.out grad_in [T][K].
int mx4_bwd_input(const Mx4Call &c, int in_dtype, int out_dtype, void *stream)
{
    using C = Mx4BwdCfg;
    static_assert(C::BT == Mx4Cfg::BT, "mx4_check bounds the grid's y by the forward's row tile");
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, true, &empty);
    if (rc != FQL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty) {
        if (c.T == 0) return FQL_OK;
        if (c.lora.on) return FQL_ERR_BAD_SHAPE;                      // (N == 0 with rows: dv A alone is not this entry's business)
        // N == 0: the gradient of an empty contraction.  grad_in [T][K] is zeros and no other operand is read.
        if (!c.out) return FQL_ERR_NULL_POINTER;
        (void)hipGetLastError();
        return hipMemsetAsync(c.out, 0, (size_t)c.T * c.K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    const dim3 grid = mx4_grid(c, c.K, C::BK, C::BT);
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        constexpr int IN = decltype(in)::value, OUT = decltype(o)::value;
        return with_lora_arg(c.lora, [&](auto... la) {
            return c.nvfp4 ? launch(nv4_bwd_kernel<IN, OUT, decltype(la)...>, grid, dim3(C::THREADS), 0, st, c.blocks, c.scales, c.gscale,
                                    c.rows, c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N, la...)
                           : launch(mx4_bwd_kernel<IN, OUT, decltype(la)...>, grid, dim3(C::THREADS), 0, st, c.blocks, c.scales, c.rows,
                                    c.out, c.tpe, c.offs, c.E, c.T, c.K, c.N, la...);
        });
    });
}

// ---- the split-K decode form of the three dense layers: with few rows, the decode kernel cut along K into S slices of
//      partial sums and a reduce kernel (fql_gemm_mx4_linear.h, fql_gemm_nvfp4_linear.h, fql_gemm_lut4_decode.h).  One
//      policy, a record of its three numbers per family ----
#define FQL_LINEAR_MAX_SLICES 16
#define FQL_MX4_LINEAR_DECODE_MAX_ROWS 16   /* rows (T) up to which the split form runs: the largest count of the sweep up to which it beats both grouped kernels at every shape whose S is above 1 */
#define FQL_MX4_LINEAR_FILL_WAVES 640       /* the waves S(K, N) asks for: 2.5 a compute unit, from the S sweep of the same section */
#define FQL_NVFP4_LINEAR_DECODE_MAX_ROWS 32 /* rows (T) up to which the split form runs: the largest count of the sweep (1, 16, 32, 64) up to which it beats both grouped kernels by more than the windows' ranges at every shape whose S is above 1: at 64 rows 2880 -> 5120 loses at its eight slices */
#define FQL_NVFP4_LINEAR_FILL_WAVES 720     /* the waves S(K, N) asks for: MXFP4's 640 gives 2880 -> 5120 four slices where eight win at one row; 720 is the largest value that keeps 4096 -> 2880 at eight (the S sweep of the same section) */
#define FQL_LUT4_LINEAR_DECODE_MAX_ROWS 64 /* rows (T) up to which the decode form runs: the largest count of the sweep (1, 8, 16, 32, 64, 128) at which it beats the tile kernel by more than the windows' ranges on every shape; at 128 rows 8192 -> 28672 ties at its two slices */
#define FQL_LUT4_LINEAR_FILL_WAVES 1280     /* the waves S(K, N) asks for: every value in (1024, 1376] gives each of the five swept shapes the S that won its one-row sweep (16, 4, 16, 8, 2); 1280 is five waves a compute unit (the same section) */
struct SplitPolicy {
    int max_rows;                      // rows (T) up to which the split form runs (fql_tune_set_*_linear_decode_max_rows)
    int forced;                        // 0: S(K, N) below; 1 / 2 / 4 / 8 / 16: forced (fql_tune_set_*_linear_slices)
    int fill_waves;                    // the waves S(K, N) asks for
};
SplitPolicy g_mx4_linear{FQL_MX4_LINEAR_DECODE_MAX_ROWS, 0, FQL_MX4_LINEAR_FILL_WAVES};
SplitPolicy g_nvfp4_linear{FQL_NVFP4_LINEAR_DECODE_MAX_ROWS, 0, FQL_NVFP4_LINEAR_FILL_WAVES};
SplitPolicy g_lut4_linear{FQL_LUT4_LINEAR_DECODE_MAX_ROWS, 0, FQL_LUT4_LINEAR_FILL_WAVES};
// The grouped code-book experts' split form (fql_gemm_lut4_group_decode.h): S(K, N) cannot see how many experts are live.
#define FQL_LUT4_GROUP_SPLIT_MAX_ROWS 2     /* rows (T) up to which the split entries run the sliced form: the sweep has the split form at one token only (T = 2 at top-2 of 8 experts, T = 6 at top-6 of 64), and at T = 6 the 64 x 1408 -> 2048 shape ties the one-wave kernel at its sixteen slices; at T = 2 every shape whose S is above 1 wins by more than the windows' ranges */
#define FQL_LUT4_GROUP_FILL_WAVES 704       /* the waves S(K, N) asks for: every value in (688, 896] gives the four 8-expert shapes their one-token winners or a tie with them (4, 1, 8, 8); 704, the smallest multiple of 32 in it, is what costs the 64-expert shapes least (8 and 16 where 4 wins: S cannot see that six experts are live; the same section) */
SplitPolicy g_lut4_group{FQL_LUT4_GROUP_SPLIT_MAX_ROWS, 0, FQL_LUT4_GROUP_FILL_WAVES};
// The grouped code-book forward: the 128-row tile and, for few rows, the one-wave decode kernel; the same bits from both.
#define FQL_LUT4_GROUP_DECODE_MAX_ROWS 96   /* rows (T) up to which the decode kernel runs: the largest count of the sweep (2 .. 1024) below the first at which it does not beat the tile by more than the two windows' ranges at every shape: at 128 rows 11008 -> 4096 is within them */
int g_lut4_group_decode_max_rows = FQL_LUT4_GROUP_DECODE_MAX_ROWS;

// S(K, N): the slices of the split form, a pure function of the weights' shape (never of T or the device).  The smallest
// S of {1, 2, 4, 8, 16} with ceil(N / 32) * S >= fill_waves, capped at max(1, P) with P = K / 64 whole pairs, so that no
// slice of the policy's is empty.  (The rule the MXFP4 work started from asked for 1024, a wave a SIMD; the sweep's winners
// at one row are what 640 gives on all five shapes: 4, 8, 4, 1, 4.  Past that the partial sums' traffic and the second
// launch cost more than the shorter K loop saves, and N = 28672 has 896 waves without help.)
int policy_slices(int fill_waves, int K, int N)
{
    const long long waves = ((long long)N + Mx4DecodeCfg::BN - 1) / Mx4DecodeCfg::BN;
    int S = 1;
    while (S < FQL_LINEAR_MAX_SLICES && waves * S < fill_waves) S *= 2;
    const int P = K / 64;
    while (S > 1 && S > P) S /= 2;
    return S;
}

// The slices a call that asks for the split form runs now.  Past the row threshold: 1.  The MXFP4 and NVFP4 layers run the
// split form above one slice and their grouped pair of kernels at 1; the code-book layer has no one-wave kernel to fall
// back on and runs the decode form up to the threshold at S = 1 as well, so T never changes its S.
int slices(const SplitPolicy &p, int T, int K, int N)
{
    if (!decode_rows(p.max_rows, T)) return 1;
    return p.forced != 0 ? p.forced : policy_slices(p.fill_waves, K, N);
}

// The partial sums of the split form: [16][T][N] float32, sized for the largest S so that the slice hook cannot outgrow it.
size_t partial_bytes(const SplitPolicy &p, int T, int N)
{
    if (T <= 0 || N <= 0 || T > p.max_rows) return 0;
    return (size_t)FQL_LINEAR_MAX_SLICES * sizeof(float) * (size_t)T * (size_t)N;
}
size_t mx4_linear_h_bytes(int T, int K, int gated) { return gated && T > 0 && K > 0 ? mx4_ws_bytes(ROWS_FLOAT, T, K) : 0; }

// What fql_tune_{mx4,nvfp4}_linear_kernel report: slices << 8 | the kernel (2 the split form, 1 the one-wave decode kernel of
// the grouped pair, 0 its tile kernel).
int linear_kernel_code(const SplitPolicy &p, int grouped_max_rows, int T, int K, int N)
{
    const int S = slices(p, T, K, N);
    return (S << 8) | (S > 1 ? 2 : decode_rows(grouped_max_rows, T) ? 1 : 0);
}

// f(std::integral_constant<int, S>) for a slice count of {MIN_S, .., 16}: the reduce kernels have S as a template argument,
// and only the code-book one exists at S = 1.
template <int MIN_S, class F>
int with_slices(int S, F &&f)
{
    if constexpr (MIN_S == 1)
        if (S == 1) return f(std::integral_constant<int, 1>{});
    switch (S) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

// The two launches of the split form: decode(in, grid, block) is a family's sliced decode kernel into partial [S][T][N],
// reduce(out, s, grid, block) its reduce kernel.  (Three reduce kernels, not one: DESIGN.md section 45.)
template <int MIN_S, class Decode, class Reduce>
int launch_split(int in_dtype, int out_dtype, int T, int N, int S, Decode &&decode, Reduce &&reduce)
{
    using D = Mx4DecodeCfg;
    using R = Nv4LinearReduceCfg;
    static_assert(Mx4LinearReduceCfg::THREADS == R::THREADS && Mx4LinearReduceCfg::ROWS == R::ROWS && Mx4LinearReduceCfg::COLS == R::COLS,
                  "one reduce grid for the three families");
    const dim3 grid((N + D::BN - 1) / D::BN, (T + D::BT - 1) / D::BT, S);
    const int rc = with_in_dtype(in_dtype, [&](auto in) { return decode(in, grid, dim3(D::THREADS)); });
    if (rc != FQL_OK) return rc;
    const int row_blocks = (T + R::ROWS - 1) / R::ROWS;
    const dim3 rgrid((N + R::COLS - 1) / R::COLS, row_blocks < 65535 ? row_blocks : 65535);
    return with_out_dtype(out_dtype, [&](auto o) {
        return with_slices<MIN_S>(S, [&](auto s) { return reduce(o, s, rgrid, dim3(R::THREADS)); });
    });
}

// The split form of the MXFP4 and NVFP4 layers, S > 1.
int launch_linear_split(int in_dtype, int out_dtype, const Mx4Call &c, int S, float *partial, hipStream_t st)
{
    if (c.nvfp4)
        return launch_split<2>(in_dtype, out_dtype, c.T, c.N, S,
            [&](auto in, dim3 grid, dim3 block) {
                return launch(nv4_linear_decode_kernel<decltype(in)::value>, grid, block, 0, st, c.blocks, c.scales, c.rows, partial, c.T, c.K, c.N);
            },
            [&](auto o, auto s, dim3 grid, dim3 block) {
                return launch(nv4_linear_reduce_kernel<decltype(o)::value, decltype(s)::value>, grid, block, 0, st, partial, c.gscale, c.bias,
                              c.out, c.T, c.N);
            });
    return launch_split<2>(in_dtype, out_dtype, c.T, c.N, S,
        [&](auto in, dim3 grid, dim3 block) {
            return launch(mx4_linear_decode_kernel<decltype(in)::value>, grid, block, 0, st, c.blocks, c.scales, c.rows, partial, c.T, c.K, c.N);
        },
        [&](auto o, auto s, dim3 grid, dim3 block) {
            return launch(mx4_linear_reduce_kernel<decltype(o)::value, decltype(s)::value>, grid, block, 0, st, partial, c.bias, c.out, c.T, c.N);
        });
}

// Every dense MXFP4 and NVFP4 entry: the checks of mx4_check with E = 1 and no table, the workspace (last, everything before
// any HIP call), the pre-pass of a gated call, then the split form where `split` (NULL: an entry without one, or split_k
// == 0) asks for more than one slice and the grouped pair of kernels everywhere else.
int mx4_linear_fwd(Mx4Call c, int in_dtype, int out_dtype, const Mx4Act &a, const SplitPolicy *split, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    bool empty;
    const int rc = mx4_check(c, in_dtype, out_dtype, a.ok(), &empty);
    if (rc != FQL_OK || empty) return rc;
    const size_t h_bytes = mx4_linear_h_bytes(c.T, c.K, a.gated);
    const size_t need = h_bytes + (split ? partial_bytes(*split, c.T, c.N) : 0);
    if (need != 0 && (!workspace || !aligned16(workspace) || workspace_bytes < need)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    if (a.gated) {
        const int lrc = launch_mx4_quant<ROWS_FLOAT>(c.rows, in_dtype, a, ws, nullptr, c.T, c.K, st);
        if (lrc != FQL_OK) return lrc;
        c.rows = ws;
        in_dtype = FQL_DTYPE_BF16;
    }
    const int S = split ? slices(*split, c.T, c.K, c.N) : 1;
    if (S > 1) return launch_linear_split(in_dtype, out_dtype, c, S, reinterpret_cast<float *>(ws + h_bytes), st);
    return launch_float_rows(in_dtype, out_dtype, c, st);
}

// ---- 4-bit code-book weights, dense and grouped (fql_gemm_lut4.h, fql_gemm_lut4_bwd.h, fql_gemm_lut4_decode.h,
//      fql_gemm_lut4_group.h; DESIGN.md sections 44 to 46 and 48) ----
struct Lut4Call {
    const uint8_t *codes;
    const float *absmax, *book;        // book: [16] or NULL (the NF4 table)
    int block;
    const void *rows;                  // inputs [T][K] (forward) or grad_out [T][N] (input gradient)
    const float *bias;
    void *out;                         // out [T][N] or grad_in [T][K]
    int T, K, N;
    LoraOperands lora;
    bool grouped = false;              // a grouped entry: codes [E][N][K / 2], absmax [E][N][K / block], bias [E][N], and
    const int32_t *tpe = nullptr, *offs = nullptr;   // the expert table (both NULL with E == 1: one segment of all rows)
    int E = 1;
    bool act_ok = true;                // (a gated grouped entry) the activation's arguments are valid
};

// c as the call of a grouped entry
Lut4Call with_experts(Lut4Call c, const int32_t *tpe, const int32_t *offs, int E)
{
    c.grouped = true; c.tpe = tpe; c.offs = offs; c.E = E;
    return c;
}

// mx4_check's order for one dense matrix: shapes, the row and result types, (an adapter entry: the rank), the empty call,
// NULL pointers (the adapter operands with the others), the grid, then alignment.  bt: the row tile of the kernel that will
// run; `bwd`: N == 0 is not empty (grad_in is zeros; nothing but the result is dereferenced then; an adapter entry refuses
// it here).  *bshift = log2(block).  A grouped call adds mx4_check's tests of E, the activation and the expert table, each
// where mx4_check has it; a dense call (E = 1, no table) passes them all.
int lut4_check(const Lut4Call &c, int in_dtype, int out_dtype, int bt, bool bwd, bool *empty, int *bshift)
{
    *empty = false;
    if (c.E <= 0 || c.T < 0 || c.K <= 0 || c.N < 0 || !c.act_ok) return FQL_ERR_BAD_SHAPE;
    if (c.K & 1) return FQL_ERR_ODD_K;
    if (c.K % 64 != 0) return FQL_ERR_BAD_SHAPE;
    if (c.block < 64 || (c.block & (c.block - 1)) != 0 || c.K % c.block != 0) return FQL_ERR_BAD_SHAPE;
    if ((in_dtype != FQL_DTYPE_F32 && in_dtype != FQL_DTYPE_BF16) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (lora_rank_bad(c.lora)) return FQL_ERR_BAD_SHAPE;
    if (c.T == 0 || (c.N == 0 && !bwd)) { *empty = true; return FQL_OK; }
    if (c.lora.on && c.N == 0) return FQL_ERR_BAD_SHAPE;              // (the input gradient: dv A alone is not this entry's business)
    if (!c.out || (c.N != 0 && (!c.codes || !c.absmax || !c.rows))) return FQL_ERR_NULL_POINTER;
    if (lora_null(c.lora)) return FQL_ERR_NULL_POINTER;
    if ((c.tpe == nullptr) != (c.offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (c.tpe == nullptr && c.E != 1) return FQL_ERR_BAD_SHAPE;
    if (c.E > 65534) return FQL_ERR_BAD_SHAPE;                        // (the grid's z: the experts and the coverage slice)
    if ((c.T + bt - 1) / bt > 65535) return FQL_ERR_BAD_SHAPE;
    if (c.grouped && (long long)c.T * (c.K / 8) / 256 >= 0x7FFFFFFFLL) return FQL_ERR_BAD_SHAPE;   // (the pre-pass's grid, as mx4_check)
    const int ib = dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!aligned16(c.codes) || (reinterpret_cast<uintptr_t>(c.rows) & (ib - 1)) || (reinterpret_cast<uintptr_t>(c.out) & (ob - 1)) ||
        (reinterpret_cast<uintptr_t>(c.bias) & 3) || (reinterpret_cast<uintptr_t>(c.absmax) & 3) ||
        (reinterpret_cast<uintptr_t>(c.book) & 3)) return FQL_ERR_ALIGNMENT;
    if (lora_misaligned(c.lora)) return FQL_ERR_ALIGNMENT;
    int s = 6;
    while ((1 << s) < c.block) ++s;
    *bshift = s;
    return FQL_OK;
}

// The tile kernel; an adapter call runs the same tile and grid, the adapter stage behind the K loop.
int launch_lut4_tile(int in_dtype, int out_dtype, const Lut4Call &c, int bshift, hipStream_t st)
{
    using C = Lut4Cfg;
    const dim3 grid((c.N + C::BN - 1) / C::BN, (c.T + C::BT - 1) / C::BT);
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        return with_lora_arg(c.lora, [&](auto... la) {
            return launch(lut4_kernel<decltype(in)::value, decltype(o)::value, decltype(la)...>, grid, dim3(C::THREADS), 0, st,
                          c.codes, c.absmax, c.book, c.rows, c.bias, c.out, bshift, c.T, c.K, c.N, la...);
        });
    });
}

// The forward on the tile kernel, with or without an adapter: no workspace, no tune hook, never the decode form.
int lut4_tile_fwd(const Lut4Call &c, int in_dtype, int out_dtype, void *stream)
{
    bool empty;
    int bshift = 6;
    const int rc = lut4_check(c, in_dtype, out_dtype, Lut4Cfg::BT, false, &empty, &bshift);
    if (rc != FQL_OK || empty) return rc;
    return launch_lut4_tile(in_dtype, out_dtype, c, bshift, static_cast<hipStream_t>(stream));
}

// The input gradient, with or without an adapter (N == 0 with rows: lut4_check refuses the adapter entry): c.rows is
// grad_out [T][N], c.out grad_in [T][K].
int lut4_bwd_input(const Lut4Call &c, int in_dtype, int out_dtype, void *stream)
{
    using C = Mx4BwdCfg;
    bool empty;
    int bshift = 6;
    const int rc = lut4_check(c, in_dtype, out_dtype, C::BT, true, &empty, &bshift);
    if (rc != FQL_OK || empty) return rc;
    const dim3 grid((c.K + C::BK - 1) / C::BK, (c.T + C::BT - 1) / C::BT);   // (N == 0: no stage exists, every tile stores zeros)
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        return with_lora_arg(c.lora, [&](auto... la) {
            return launch(lut4_bwd_kernel<decltype(in)::value, decltype(o)::value, decltype(la)...>, grid, dim3(C::THREADS), 0,
                          static_cast<hipStream_t>(stream), c.codes, c.absmax, c.book, c.rows, c.out, bshift, c.T, c.K, c.N, la...);
        });
    });
}

// The grid of a grouped code-book kernel with tiles of bt rows x bc columns of the result [T][cols]: mx4_grid's.
dim3 lut4_group_grid(const Lut4Call &c, int cols, int bc, int bt)
{
    return dim3((cols + bc - 1) / bc, (c.T + bt - 1) / bt, c.tpe != nullptr ? c.E + 1 : 1);
}

// The grouped forward (fql_gemm_lut4_group.h, fql_gemm_lut4_group_decode.h), plain or gated: the checks, the workspace (gated:
// h; a split entry up to its row threshold: the partial sums behind it), mx4_glu_kernel's pre-pass, then
//   * `split` (an entry that has one) and T within its threshold: the sliced decode kernel on S(K, N) slices, S = 1
//     included, and the reduce kernel;
//   * else the one-wave decode kernel up to g_lut4_group_decode_max_rows rows and the 128-row tile past it: the same bits.
// lut4_check receives the tile's row block whichever kernel runs, so its grid bound and order do not move.
int lut4_group_fwd(Lut4Call c, int in_dtype, int out_dtype, const Mx4Act &a, const SplitPolicy *split, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    using C = Lut4GroupCfg;
    using D = Mx4DecodeCfg;
    bool empty;
    int bshift = 6;
    c.act_ok = a.ok();
    const int rc = lut4_check(c, in_dtype, out_dtype, C::BT, false, &empty, &bshift);
    if (rc != FQL_OK || empty) return rc;
    const bool sliced = split != nullptr && decode_rows(split->max_rows, c.T);
    if (sliced && (long long)c.E * FQL_LINEAR_MAX_SLICES > 65535) return FQL_ERR_BAD_SHAPE;   // (the sliced grid's z = E * S)
    const size_t h_bytes = a.gated ? mx4_ws_bytes(ROWS_FLOAT, c.T, c.K) : 0;                  // (a multiple of 16: K % 64 == 0)
    const size_t need = h_bytes + (sliced ? partial_bytes(*split, c.T, c.N) : 0);
    if (need != 0 && (!workspace || !aligned16(workspace) || workspace_bytes < need)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.gated) {
        const int lrc = launch_mx4_quant<ROWS_FLOAT>(c.rows, in_dtype, a, workspace, nullptr, c.T, c.K, st);
        if (lrc != FQL_OK) return lrc;
        c.rows = workspace;
        in_dtype = FQL_DTYPE_BF16;
    }
    if (sliced) {
        using R = Lut4GroupReduceCfg;
        const int S = slices(*split, c.T, c.K, c.N);
        float *partial = reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + h_bytes);
        const dim3 grid((c.N + D::BN - 1) / D::BN, (c.T + D::BT - 1) / D::BT, c.E * S);
        const int drc = with_in_dtype(in_dtype, [&](auto in) {
            return launch(lut4_group_sdecode_kernel<decltype(in)::value>, grid, dim3(D::THREADS), 0, st, c.codes, c.absmax, c.book, c.rows,
                          partial, c.tpe, c.offs, bshift, S, c.T, c.K, c.N);
        });
        if (drc != FQL_OK) return drc;
        const dim3 rgrid = lut4_group_grid(c, c.N, R::COLS, R::BT);
        return with_out_dtype(out_dtype, [&](auto o) {
            return with_slices<1>(S, [&](auto s) {
                return launch(lut4_group_reduce_kernel<decltype(o)::value, decltype(s)::value>, rgrid, dim3(R::THREADS), 0, st, partial,
                              c.bias, c.out, c.tpe, c.offs, c.E, c.T, c.N);
            });
        });
    }
    const bool decode = decode_rows(g_lut4_group_decode_max_rows, c.T);
    const dim3 grid = decode ? lut4_group_grid(c, c.N, D::BN, D::BT) : lut4_group_grid(c, c.N, C::BN, C::BT);
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        constexpr int IN = decltype(in)::value, OUT = decltype(o)::value;
        return launch(decode ? lut4_group_decode_kernel<IN, OUT> : lut4_group_kernel<IN, OUT>, grid, dim3(decode ? D::THREADS : C::THREADS),
                      0, st, c.codes, c.absmax, c.book, c.rows, c.bias, c.out, c.tpe, c.offs, bshift, c.E, c.T, c.K, c.N);
    });
}

// The grouped input gradient: c.rows is grad_out [T][N], c.out grad_in [T][K].  N == 0 with rows: grad_in is zeros (one
// memset; no other operand is read).
int lut4_group_bwd_input(const Lut4Call &c, int in_dtype, int out_dtype, void *stream)
{
    using C = Mx4BwdCfg;
    bool empty;
    int bshift = 6;
    const int rc = lut4_check(c, in_dtype, out_dtype, C::BT, true, &empty, &bshift);
    if (rc != FQL_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c.N == 0) {
        (void)hipGetLastError();
        return hipMemsetAsync(c.out, 0, (size_t)c.T * c.K * dtype_bytes(out_dtype), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    const dim3 grid = lut4_group_grid(c, c.K, C::BK, C::BT);
    return with_dtypes(in_dtype, out_dtype, [&](auto in, auto o) {
        return launch(lut4_group_bwd_kernel<decltype(in)::value, decltype(o)::value>, grid, dim3(C::THREADS), 0, st, c.codes,
                      c.absmax, c.book, c.rows, c.out, c.tpe, c.offs, bshift, c.E, c.T, c.K, c.N);
    });
}

// The code-book layer's partial sums: none where the decode form does not run, the grid's bound on T included.
size_t lut4_partial_bytes(int T, int N) { return decode_rows(g_lut4_linear.max_rows, T) ? partial_bytes(g_lut4_linear, T, N) : 0; }

// The decode form of the code-book layer (S = 1 included).
int launch_lut4_split(int in_dtype, int out_dtype, const Lut4Call &c, int bshift, int S, float *partial, hipStream_t st)
{
    return launch_split<1>(in_dtype, out_dtype, c.T, c.N, S,
        [&](auto in, dim3 grid, dim3 block) {
            return launch(lut4_decode_kernel<decltype(in)::value>, grid, block, 0, st, c.codes, c.absmax, c.book, c.rows, partial, bshift,
                          c.T, c.K, c.N);
        },
        [&](auto o, auto s, dim3 grid, dim3 block) {
            return launch(lut4_linear_reduce_kernel<decltype(o)::value, decltype(s)::value>, grid, block, 0, st, partial, c.bias, c.out, c.T,
                          c.N);
        });
}

// The two bodies of the fql_tune_set_* hooks: a negative threshold, or a slice count outside {0, 1, 2, 4, 8, 16}, changes
// nothing; the value before the call comes back.
int replace_rows(int &slot, int rows)
{
    const int old = slot;
    if (rows >= 0) slot = rows;
    return old;
}
int replace_slices(int &slot, int slices)
{
    const int old = slot;
    if (slices == 0 || slices == 1 || slices == 2 || slices == 4 || slices == 8 || slices == 16) slot = slices;
    return old;
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
    return mx4_float_fwd({blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, in_dtype, out_dtype, stream);
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
    return mx4_bwd_input({blocks, scales_e8m0, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N}, in_dtype,
                         out_dtype, stream);
}

FQL_API int fql_moe_mx4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                                 const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                 const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                 int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    return mx4_float_fwd(with_lora(Mx4Call{blocks, scales_e8m0, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                   lora_rows, lora_B, rank), in_dtype, out_dtype, stream);
}

FQL_API int fql_moe_mx4_glu_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                     const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                     const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                                     int E, int T, int K, int N, int activation, float act_alpha, float act_limit,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_quant_fwd<ROWS_FLOAT>(with_lora(Mx4Call{blocks, scales_e8m0, gate_up, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                               lora_rows, lora_B, rank), in_dtype, out_dtype, {true, activation, act_alpha, act_limit},
                                     workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_mx4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                       const float *lora_rows, const float *lora_A, int rank, const int32_t *tokens_per_expert,
                                       const int32_t *input_offsets, void *grad_in, int out_dtype, int E, int T, int K, int N,
                                       void *stream)
{
    return mx4_bwd_input(with_lora(Mx4Call{blocks, scales_e8m0, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N},
                                   lora_rows, lora_A, rank), in_dtype, out_dtype, stream);
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
    return mx4_linear_h_bytes(T, K, gated) + (split_k ? partial_bytes(g_mx4_linear, T, N) : 0);   // h [T][K] bfloat16 | partial [16][T][N] float32
}

FQL_API int fql_linear_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, void *out, int out_dtype, int T, int K, int N, int split_k, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd({blocks, scales_e8m0, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, in_dtype, out_dtype, kMx4Plain,
                          split_k ? &g_mx4_linear : nullptr, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, void *out, int out_dtype, int T, int K, int N, int activation,
                                   float act_alpha, float act_limit, int split_k, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    return mx4_linear_fwd({blocks, scales_e8m0, gate_up, bias, nullptr, nullptr, out, 1, T, K, N}, in_dtype, out_dtype,
                          {true, activation, act_alpha, act_limit}, split_k ? &g_mx4_linear : nullptr, workspace, workspace_bytes, stream);
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
    return mx4_float_fwd(with_nvfp4({blocks, scales_e4m3, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N}, global_scale),
                         in_dtype, out_dtype, stream);
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
                          out_dtype, kMx4Plain, nullptr, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_nvfp4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                     const void *gate_up, int in_dtype, const float *bias, void *out, int out_dtype, int T, int K,
                                     int N, int activation, float act_alpha, float act_limit, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd(with_nvfp4({blocks, scales_e4m3, gate_up, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale), in_dtype,
                          out_dtype, {true, activation, act_alpha, act_limit}, nullptr, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_nvfp4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *grad_out,
                                    int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                    int out_dtype, int E, int T, int K, int N, void *stream)
{
    return mx4_bwd_input(with_nvfp4({blocks, scales_e4m3, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N},
                                    global_scale), in_dtype, out_dtype, stream);
}

FQL_API int fql_moe_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                   int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                   const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                   int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    return mx4_float_fwd(with_lora(with_nvfp4({blocks, scales_e4m3, inputs, bias, tokens_per_expert, input_offsets, out, E, T, K, N},
                                              global_scale), lora_rows, lora_B, rank), in_dtype, out_dtype, stream);
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
    return mx4_bwd_input(with_lora(with_nvfp4({blocks, scales_e4m3, grad_out, nullptr, tokens_per_expert, input_offsets, grad_in, E, T, K, N},
                                              global_scale), lora_rows, lora_A, rank), in_dtype, out_dtype, stream);
}

FQL_API int fql_linear_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                      int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                      void *out, int out_dtype, int T, int K, int N, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    return mx4_linear_fwd(with_lora(with_nvfp4({blocks, scales_e4m3, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale),
                                    lora_rows, lora_B, rank), in_dtype, out_dtype, kMx4Plain, nullptr, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_nvfp4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                            const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A,
                                            int rank, void *grad_in, int out_dtype, int T, int K, int N, void *stream)
{
    return fql_moe_nvfp4_lora_bwd_input(blocks, scales_e4m3, global_scale, grad_out, in_dtype, lora_rows, lora_A, rank, nullptr,
                                        nullptr, grad_in, out_dtype, 1, T, K, N, stream);
}

FQL_API int fql_linear_lut4_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *inputs,
                                int in_dtype, const float *bias, void *out, int out_dtype, int T, int K, int N, void *stream)
{
    return lut4_tile_fwd({codes, absmax, code_book, block, inputs, bias, out, T, K, N}, in_dtype, out_dtype, stream);
}

FQL_API size_t fql_linear_lut4_split_workspace_bytes(int T, int K, int N)
{
    (void)K;
    return lut4_partial_bytes(T, N);                                      // partial [16][T][N] float32
}

FQL_API int fql_linear_lut4_split_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *inputs,
                                      int in_dtype, const float *bias, void *out, int out_dtype, int T, int K, int N,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    const Lut4Call c{codes, absmax, code_book, block, inputs, bias, out, T, K, N};
    bool empty;
    int bshift = 6;
    const int rc = lut4_check(c, in_dtype, out_dtype, Lut4Cfg::BT, false, &empty, &bshift);   // (a decode grid's y is within it)
    if (rc != FQL_OK || empty) return rc;
    const size_t need = lut4_partial_bytes(T, N);
    if (need != 0 && (!workspace || !aligned16(workspace) || workspace_bytes < need)) return FQL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!decode_rows(g_lut4_linear.max_rows, T)) return launch_lut4_tile(in_dtype, out_dtype, c, bshift, st);
    return launch_lut4_split(in_dtype, out_dtype, c, bshift, slices(g_lut4_linear, T, K, N), static_cast<float *>(workspace), st);
}

FQL_API int fql_tune_set_lut4_linear_decode_max_rows(int rows) { return replace_rows(g_lut4_linear.max_rows, rows); }
FQL_API int fql_tune_set_lut4_linear_slices(int slices) { return replace_slices(g_lut4_linear.forced, slices); }

FQL_API int fql_tune_lut4_linear_kernel(int T, int K, int N)
{
    return decode_rows(g_lut4_linear.max_rows, T) ? (slices(g_lut4_linear, T, K, N) << 8) | 2 : (1 << 8);
}

FQL_API int fql_linear_lut4_bwd_input(const uint8_t *codes, const float *absmax, const float *code_book, int block,
                                      const void *grad_out, int in_dtype, void *grad_in, int out_dtype, int T, int K, int N,
                                      void *stream)
{
    return lut4_bwd_input({codes, absmax, code_book, block, grad_out, nullptr, grad_in, T, K, N}, in_dtype, out_dtype, stream);
}

// The adapter forms of the two code-book tile kernels.
FQL_API size_t fql_moe_lut4_workspace_bytes(int E, int T, int K, int N, int gated)
{
    return fql_moe_mx4_workspace_bytes(E, T, K, N, gated);            // h [T][K] bfloat16, as the MXFP4 entries'
}

FQL_API int fql_moe_lut4_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *inputs,
                             int in_dtype, const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                             void *out, int out_dtype, int E, int T, int K, int N, void *stream)
{
    return lut4_group_fwd(with_experts({codes, absmax, code_book, block, inputs, bias, out, T, K, N}, tokens_per_expert, input_offsets, E),
                          in_dtype, out_dtype, kMx4Plain, nullptr, nullptr, 0, stream);
}

FQL_API int fql_moe_lut4_glu_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *gate_up,
                                 int in_dtype, const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                 void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                 float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return lut4_group_fwd(with_experts({codes, absmax, code_book, block, gate_up, bias, out, T, K, N}, tokens_per_expert, input_offsets, E),
                          in_dtype, out_dtype, {true, activation, act_alpha, act_limit}, nullptr, workspace, workspace_bytes, stream);
}

// The split forms of the two grouped forwards: the workspace is the gated h [T][K] bfloat16, then the
// partial sums [16][T][N] float32 where the sliced form runs.
FQL_API size_t fql_moe_lut4_split_workspace_bytes(int E, int T, int K, int N, int gated)
{
    return fql_moe_lut4_workspace_bytes(E, T, K, N, gated) + (decode_rows(g_lut4_group.max_rows, T) ? partial_bytes(g_lut4_group, T, N) : 0);
}

FQL_API int fql_moe_lut4_split_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *inputs,
                                   int in_dtype, const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    return lut4_group_fwd(with_experts({codes, absmax, code_book, block, inputs, bias, out, T, K, N}, tokens_per_expert, input_offsets, E),
                          in_dtype, out_dtype, kMx4Plain, &g_lut4_group, workspace, workspace_bytes, stream);
}

FQL_API int fql_moe_lut4_glu_split_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block,
                                       const void *gate_up, int in_dtype, const float *bias, const int32_t *tokens_per_expert,
                                       const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                                       int activation, float act_alpha, float act_limit, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return lut4_group_fwd(with_experts({codes, absmax, code_book, block, gate_up, bias, out, T, K, N}, tokens_per_expert, input_offsets, E),
                          in_dtype, out_dtype, {true, activation, act_alpha, act_limit}, &g_lut4_group, workspace, workspace_bytes, stream);
}

FQL_API int fql_tune_set_lut4_group_decode_max_rows(int rows) { return replace_rows(g_lut4_group_decode_max_rows, rows); }
FQL_API int fql_tune_lut4_group_kernel(int T) { return decode_rows(g_lut4_group_decode_max_rows, T) ? 1 : 0; }
FQL_API int fql_tune_set_lut4_group_split_max_rows(int rows) { return replace_rows(g_lut4_group.max_rows, rows); }
FQL_API int fql_tune_set_lut4_group_slices(int slices) { return replace_slices(g_lut4_group.forced, slices); }

// slices << 8 | the kernel a split entry runs: 2 the sliced form, 1 the one-wave decode kernel, 0 the tile
FQL_API int fql_tune_lut4_group_split_kernel(int T, int K, int N)
{
    return decode_rows(g_lut4_group.max_rows, T) ? (slices(g_lut4_group, T, K, N) << 8) | 2 : (1 << 8) | fql_tune_lut4_group_kernel(T);
}

FQL_API int fql_moe_lut4_bwd_input(const uint8_t *codes, const float *absmax, const float *code_book, int block,
                                   const void *grad_out, int in_dtype, const int32_t *tokens_per_expert,
                                   const int32_t *input_offsets, void *grad_in, int out_dtype, int E, int T, int K, int N,
                                   void *stream)
{
    return lut4_group_bwd_input(with_experts({codes, absmax, code_book, block, grad_out, nullptr, grad_in, T, K, N}, tokens_per_expert,
                                             input_offsets, E), in_dtype, out_dtype, stream);
}

FQL_API int fql_linear_lut4_lora_fwd(const uint8_t *codes, const float *absmax, const float *code_book, int block, const void *inputs,
                                     int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                     void *out, int out_dtype, int T, int K, int N, void *stream)
{
    return lut4_tile_fwd(with_lora(Lut4Call{codes, absmax, code_book, block, inputs, bias, out, T, K, N}, lora_rows, lora_B, rank),
                         in_dtype, out_dtype, stream);
}

FQL_API int fql_linear_lut4_lora_bwd_input(const uint8_t *codes, const float *absmax, const float *code_book, int block,
                                           const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A,
                                           int rank, void *grad_in, int out_dtype, int T, int K, int N, void *stream)
{
    return lut4_bwd_input(with_lora(Lut4Call{codes, absmax, code_book, block, grad_out, nullptr, grad_in, T, K, N}, lora_rows, lora_A, rank),
                          in_dtype, out_dtype, stream);
}

FQL_API int fql_tune_set_nvfp4_decode_max_rows(int rows) { return replace_rows(g_nvfp4_decode_max_rows, rows); }

FQL_API int fql_tune_nvfp4_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return decode_rows(g_nvfp4_decode_max_rows, T) ? 1 : 0;
}

FQL_API size_t fql_linear_nvfp4_split_workspace_bytes(int T, int K, int N, int gated)
{
    return mx4_linear_h_bytes(T, K, gated) + partial_bytes(g_nvfp4_linear, T, N);   // h [T][K] bfloat16 | partial [16][T][N] float32
}

FQL_API int fql_linear_nvfp4_split_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                       int in_dtype, const float *bias, void *out, int out_dtype, int T, int K, int N,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd(with_nvfp4({blocks, scales_e4m3, inputs, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale), in_dtype,
                          out_dtype, kMx4Plain, &g_nvfp4_linear, workspace, workspace_bytes, stream);
}

FQL_API int fql_linear_nvfp4_glu_split_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                           const void *gate_up, int in_dtype, const float *bias, void *out, int out_dtype, int T,
                                           int K, int N, int activation, float act_alpha, float act_limit, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return mx4_linear_fwd(with_nvfp4({blocks, scales_e4m3, gate_up, bias, nullptr, nullptr, out, 1, T, K, N}, global_scale), in_dtype,
                          out_dtype, {true, activation, act_alpha, act_limit}, &g_nvfp4_linear, workspace, workspace_bytes, stream);
}

FQL_API int fql_tune_set_nvfp4_linear_decode_max_rows(int rows) { return replace_rows(g_nvfp4_linear.max_rows, rows); }
FQL_API int fql_tune_set_nvfp4_linear_slices(int slices) { return replace_slices(g_nvfp4_linear.forced, slices); }
FQL_API int fql_tune_nvfp4_linear_kernel(int T, int K, int N) { return linear_kernel_code(g_nvfp4_linear, g_nvfp4_decode_max_rows, T, K, N); }

FQL_API int fql_tune_set_mx4_linear_decode_max_rows(int rows) { return replace_rows(g_mx4_linear.max_rows, rows); }
FQL_API int fql_tune_set_mx4_linear_slices(int slices) { return replace_slices(g_mx4_linear.forced, slices); }
FQL_API int fql_tune_mx4_linear_kernel(int T, int K, int N) { return linear_kernel_code(g_mx4_linear, g_mx4_decode_max_rows[ROWS_FLOAT], T, K, N); }

FQL_API int fql_tune_set_mx4_decode_max_rows(int rows) { return replace_rows(g_mx4_decode_max_rows[ROWS_FLOAT], rows); }

FQL_API int fql_tune_mx4_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return decode_rows(g_mx4_decode_max_rows[ROWS_FLOAT], T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_scaled_decode_max_rows(int mode, int rows)
{
    if (mode != ROWS_E4M3 && mode != ROWS_MXFP4) return -1;
    return replace_rows(g_mx4_decode_max_rows[mode], rows);
}

FQL_API int fql_tune_mx4_scaled_kernel(int mode, int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    if (mode != ROWS_E4M3 && mode != ROWS_MXFP4) return -1;
    return decode_rows(g_mx4_decode_max_rows[mode], T) ? 1 : 0;
}

FQL_API int fql_tune_set_mx4_f6_decode_max_rows(int rows) { return replace_rows(g_mx4_decode_max_rows[ROWS_MXFP6], rows); }

FQL_API int fql_tune_mx4_f6_kernel(int E, int T, int K, int N)
{
    (void)E; (void)K; (void)N;
    return decode_rows(g_mx4_decode_max_rows[ROWS_MXFP6], T) ? 1 : 0;
}

}  // extern "C"
