/*
 * fql_int4.h -- C ABI of libfql_int4.so: fused INT4 dequantize-linear and grouped (MoE)
 * per-expert INT4 GEMM for AMD Instinct MI355X (gfx950 / CDNA4).
 *
 * This header is the drop-in boundary.  It replaces, entry point for entry point, the two
 * pybind11/libtorch operators of the reference (paths relative to the reference repository):
 *
 *   fql_linear_fwd_f32   <- fused_quant_linear_cuda.forward(input, packed_weights, scales, zero_points)
 *                           csrc/quantized_linear.cpp:22-28, csrc/quantized_linear.h:29-34,
 *                           host wrapper csrc/quantized_linear_kernel.cu:293-378
 *   fql_moe_fwd_f32      <- moe_int4_cuda.forward(packed_weights, scales, zero_points, inputs,
 *                                                 expert_ids, tokens_per_expert, input_offsets)
 *                           csrc/moe_int4_kernel.cu:93-141, csrc/moe_int4_kernel.h:7-15
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / pybind types.  All data pointers are DEVICE
 *     pointers (hipMalloc'd or a framework's device tensor storage) unless stated otherwise.
 *   - the library owns nothing and allocates nothing: outputs and the scratch workspace are
 *     caller-allocated; `*_workspace_bytes` says how much scratch a call needs.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream), performs no host synchronisation, keeps no state between calls and is
 *     re-entrant.  It is safe to capture into a hipGraph.  (The tuning hooks of fql_int4_tune.h, which no product
 *     path calls, are the one exception: their setters change process-global dispatch thresholds.)
 *   - return value: FQL_OK (0) or a negative FQL_ERR_* code; fql_error_string() describes it.
 *     Nothing is launched when an error is returned.
 *
 * Weight format (identical to the reference; python/quantize.py:120-122, :172):
 *   packed[n][j] = (q[n][2j+1] << 4) | q[n][2j]      uint8, row-major [N][K/2]
 *   w[n][k]      = (q[n][k] - zero_points[n]) * scales[n]          per-ROW scale / zero-point
 */
#ifndef FQL_INT4_H
#define FQL_INT4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQL_VERSION 450 /* 0.4.5: low-rank adapters on the NVFP4 weights, fused into the two NVFP4 tile kernels, grouped and dense: fql_moe_nvfp4_lora_fwd / fql_moe_nvfp4_glu_lora_fwd / fql_moe_nvfp4_lora_bwd_input / fql_linear_nvfp4_lora_fwd / fql_linear_nvfp4_lora_bwd_input.  0.4.4: the input gradient of the NVFP4 weights, grouped (the dense one is its one-expert view): fql_moe_nvfp4_bwd_input.  0.4.3: NVFP4 weights (e2m1 codes, one e4m3 scale per 16 inputs, one float32 scale per tensor) on the bfloat16 matrix cores, grouped and dense: fql_moe_nvfp4_fwd / fql_moe_nvfp4_glu_fwd / fql_linear_nvfp4_fwd / fql_linear_nvfp4_glu_fwd / fql_moe_nvfp4_workspace_bytes / fql_linear_nvfp4_workspace_bytes.  0.4.2: a dense MXFP4 linear layer with a split-K decode form: fql_linear_mx4_fwd / fql_linear_mx4_glu_fwd / fql_linear_mx4_workspace_bytes.  0.4.1: low-rank adapters on the MXFP4 expert weights, fused into the bfloat16 GEMMs as one more contraction stage: fql_moe_mx4_lora_fwd / fql_moe_mx4_glu_lora_fwd / fql_moe_mx4_lora_bwd_input.  0.4.0: MXFP6 rows for the MXFP4 experts: fql_moe_mx4_fwd_f6 / fql_moe_mx4_fwd_q6 / fql_moe_mx4_glu_fwd_q6 / fql_moe_mx4_f6_workspace_bytes / fql_mx6_quantize_rows.  0.3.9: decode kernels for the fp8-row and MXFP4-row precisions of the MXFP4 experts, picked from T, the same bits as their tile kernels; no new entry point.  0.3.8: a decode kernel for the bfloat16 MXFP4 forward (few rows an expert), picked from T, the same bits as the tile kernel; no new entry point.  0.3.7: MXFP4 expert weights over MXFP4 rows (both operands e2m1 with E8M0 block scales): fql_moe_mx4_fwd_f4 / fql_moe_mx4_fwd_q4 / fql_moe_mx4_glu_fwd_q4 / fql_moe_mx4_f4_workspace_bytes / fql_mx4_quantize_rows.  0.3.6: MXFP4 expert weights on the block-scaled FP4 matrix cores over fp8 rows: fql_moe_mx4_fwd_f8 / fql_moe_mx4_fwd_q8 / fql_moe_mx4_glu_fwd_q8 / fql_moe_mx4_f8_workspace_bytes.  0.3.5: the input gradient of the MXFP4 expert weights: fql_moe_mx4_bwd_input.  0.3.4: OCP MXFP4 expert weights, forward only: fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd / fql_moe_mx4_workspace_bytes.  0.3.3: per-group scales through the typed grouped entry points and their input gradient: fql_moe_group_fwd / fql_moe_group_glu_fwd / fql_moe_group_bwd_input (+ their workspace queries).  0.3.2: expert capacity and a token mask: fql_route_plan_capped_i32 / fql_combine_sparse / fql_combine_sparse_bwd.  0.3.1: per-expert biases of the grouped GEMM and their gradient: fql_moe_bias_fwd / fql_moe_glu_bias_fwd / fql_moe_bias_grad.  0.3.0: activation kinds of the gated FFN experts (GeGLU, clamped SwiGLU): fql_moe_glu_fwd / fql_lora_glu_shrink / fql_lora_glu_grad / fql_glu_bwd.  0.2.9: the typed combine with an addend: fql_combine / fql_combine_bwd.  0.2.8: the scored router: fql_router_score_topk_fwd / fql_router_score_topk_bwd.  0.2.7: the router: fql_router_topk_fwd / fql_router_topk_bwd.  0.2.6: the gated FFN experts on float16 / bfloat16 activations: fql_moe_gated_fwd / fql_lora_gated_shrink / fql_lora_gated_grad / fql_swiglu_bwd.  0.2.4: adapters on the gated FFN experts: fql_lora_gated_shrink_f32 / fql_lora_gated_grad_f32 / fql_swiglu_bwd_f32.  0.2.3: low-rank adapter entry points fql_lora_shrink_f32 / fql_lora_expand_f32 / fql_lora_grad_f32.  0.2.2: input-gradient entry points fql_linear_bwd_input_f32 / fql_moe_bwd_input_f32 (+ their workspace queries) and fql_combine_bwd_f32.  0.2.1: fql_moe_gather_scaled_fwd_f32, fql_combine_f32 with NULL weights; the 3-limb workspace grew by one flag word per 4 rows (size it with fql_*_workspace_bytes, as always).  0.2.0: fp8 activations; residual limb set for heavy-tailed rows (two-phase buffers doubled) */

#if defined(__GNUC__)
#define FQL_API __attribute__((visibility("default")))
#else
#define FQL_API
#endif

/* error codes */
#define FQL_OK 0
#define FQL_ERR_NULL_POINTER (-1)   /* a required pointer is NULL                                  */
#define FQL_ERR_BAD_SHAPE (-2)      /* negative / zero dimension or size overflow                  */
#define FQL_ERR_ODD_K (-3)          /* K must be even (two weights per byte)                       */
#define FQL_ERR_WORKSPACE (-4)      /* workspace NULL, misaligned (16 B) or smaller than required  */
#define FQL_ERR_LAUNCH (-5)         /* hipGetLastError() reported a launch failure                 */
#define FQL_ERR_BAD_PRECISION (-6)  /* precision not one of FQL_PRECISION_*                        */
#define FQL_ERR_ALIGNMENT (-7)      /* a tensor base pointer is not aligned as documented          */
#define FQL_ERR_DTYPE (-8)          /* element type not supported on the path this shape takes     */

/* Activation precision of the MFMA path.  Weights are always exact (4-bit integers).
 * Activations are split per row into signed 8-bit limbs of a fixed-point value; the integer
 * dot products are exact (i32 MFMA accumulation), so the only error is the one rounding of
 * each activation to 2^-(8*limbs-1) of its row's maximum magnitude:
 *   FQL_PRECISION_EXACT : 3 limbs, 23-bit fixed point -> float32-class results (default;
 *                         meets the reference's own allclose(atol=1e-3) GPU tests)
 *   FQL_PRECISION_FAST  : 2 limbs, 15-bit fixed point -> ~3e-5 relative (Frobenius) error,
 *                         2/3 of the matrix-core work
 *   FQL_PRECISION_INT8  : 1 limb, 8-bit activations (per-row power-of-two scale) -> ~5e-3 relative
 *                         error, 1/3 of the matrix-core work: the "8-bit activations + INT4 weights"
 *                         serving mode (outside the 1e-3 parity claim; for weight-streaming-bound
 *                         shapes such as 64 experts x 7168 -> 18432)                          */
#define FQL_PRECISION_DEFAULT 0
#define FQL_PRECISION_INT8 1
#define FQL_PRECISION_FAST 2
#define FQL_PRECISION_EXACT 3
/*   FQL_PRECISION_FP8   : activations rounded to OCP e4m3 (4-bit significand) with one float32 scale per row
 *                         (max|x| / 448), ONE pass of the block-scaled fp8 matrix-core instruction
 *                         (v_mfma_scale_f32_32x32x64_f8f6f4, float32 accumulation) -- the "fp8 activations + INT4
 *                         weights" configuration of BASELINE.json configs[4].  ~2.7e-2 relative error on randn
 *                         activations (the format's, not the kernel's): outside the 1e-3 parity claim.  MFMA path
 *                         only: K % 32 == 0, 16-byte aligned weights and, for the linear op, more than 2 rows --
 *                         otherwise FQL_ERR_BAD_PRECISION (never a silent float32 computation); a NULL / short
 *                         workspace is FQL_ERR_WORKSPACE. */
#define FQL_PRECISION_FP8 8

/* Element types of activations and outputs for the dtype-generic entry points (fql_linear_fwd / fql_moe_fwd).
 * 16-bit inputs are widened exactly; outputs are rounded to nearest even from the float32 result, i.e. the
 * result equals `fql_*_fwd_f32(x.float()).to(dtype)` bit for bit, without the two conversion passes
 * (reference: benchmark/moe_grouped_gemm/moe_int4_module.py:70-72 runs its experts in the dtype of x). */
#define FQL_DTYPE_F32 0
#define FQL_DTYPE_F16 1
#define FQL_DTYPE_BF16 2

FQL_API int fql_version(void);
FQL_API const char *fql_error_string(int code);

/* ---------------------------------------------------------------------------------------
 * Fused INT4 dequantize-linear:  out[b][n] = sum_k x[b][k] * (q[n][k] - zp[n]) * scale[n]
 *
 *   x       [B][K] float32, contiguous          (reference: `input`, 1-D inputs are B = 1)
 *   packed  [N][K/2] uint8, contiguous
 *   scales  [N] float32,  zps [N] float32
 *   out     [B][N] float32, contiguous, fully overwritten
 *   workspace: fql_linear_workspace_bytes(B, K, N, precision) bytes, 16-byte aligned
 *              (0 bytes for B <= 2: those shapes run on the float32 GEMV kernel and never touch a workspace -- except
 *              with FQL_PRECISION_FP8, where the size is what fql_linear_fwd_f8 needs, which takes any B on the
 *              matrix cores; B = 3, 4 also run with NULL, on the slower GEMV kernel)
 * Any even K is accepted; K % 32 == 0 with 16-byte aligned `packed` takes the fast paths.
 * ------------------------------------------------------------------------------------- */
FQL_API size_t fql_linear_workspace_bytes(int B, int K, int N, int precision);

FQL_API int fql_linear_fwd_f32(const float *x, const uint8_t *packed, const float *scales,
                       const float *zps, float *out, int B, int K, int N, int precision,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Same with a per-column bias added to the result (the reference asserts `bias is None`,
 * python/module.py:84):  out[b][n] = (sum_k x[b][k] * (q[n][k] - zp[n]) * scale[n]) + bias[n],  bias [N] float32 or
 * NULL.  The add is the last operation of the kernels' epilogues (one float32 rounding after the un-biased result). */
FQL_API int fql_linear_bias_fwd_f32(const float *x, const uint8_t *packed, const float *scales,
                                    const float *zps, const float *bias, float *out, int B, int K, int N,
                                    int precision, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Grouped (MoE) INT4 GEMM over rows pre-grouped by expert:
 *   for every expert e:  out[off_e : off_e+cnt_e] = inputs[off_e : off_e+cnt_e] @ dequant(W_e)^T
 *   rows of `out` covered by no expert are set to zero (reference: torch::zeros, :109)
 *
 *   packed  [E][N][K/2] uint8;  scales, zps [E][N] float32
 *   inputs  [T][K] float32;     out [T][N] float32, fully overwritten
 *   tokens_per_expert [E] int32 (cnt_e), input_offsets [E] int32 (off_e): DEVICE arrays,
 *     consumed on the device -- no host read-back, one launch sequence for all experts.
 *     Ranges are clipped to [0, T]; they must not overlap.
 *   (`expert_ids` of the reference signature is accepted by the Python shim and ignored,
 *    exactly as the reference ignores it: csrc/moe_int4_kernel.cu:98.)
 * ------------------------------------------------------------------------------------- */
FQL_API size_t fql_moe_workspace_bytes(int E, int T, int K, int N, int precision);

FQL_API int fql_moe_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                    const float *inputs, const int32_t *tokens_per_expert,
                    const int32_t *input_offsets, float *out, int E, int T, int K, int N,
                    int precision, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Same, with the dispatch gather fused into the activation pre-pass:
 * grouped row t is read from tokens[row_index[t]] -- the sort-by-expert permutation of
 * benchmark/moe_grouped_gemm/routing.py:117-149 -- so the [T, K] gathered copy of the activations is
 * never written or re-read.  tokens [n_tokens][K] float32, row_index [T] int32 (device), values
 * clamped into [0, n_tokens).  Requires the MFMA path (K % 32 == 0, 16-byte aligned `packed`),
 * otherwise FQL_ERR_ALIGNMENT.  Workspace: fql_moe_workspace_bytes(E, T, K, N, precision).
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_moe_gather_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                                   const float *tokens, const int32_t *row_index, int n_tokens,
                                   const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   float *out, int E, int T, int K, int N, int precision,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* The same with the routing weight folded into the GEMM epilogue (second half;
 * benchmark/moe_grouped_gemm/routing.py:172-189 multiplies after the fact): out[t][:] = row_weight[t] * (grouped result).
 * row_weight [T] float32, one per GROUPED row (the weight of the (token, slot) pair the row belongs to).  One float32
 * rounding after the un-weighted result, so fql_combine_f32(..., weights = NULL), a pure gather-add of these rows, gives
 * bit for bit what fql_combine_f32 with the weights gives on the un-weighted rows (top_k <= 2).  MFMA path only. */
FQL_API int fql_moe_gather_scaled_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                                  const float *tokens, const int32_t *row_index, int n_tokens, const float *row_weight,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out,
                                  int E, int T, int K, int N, int precision, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* ---------------------------------------------------------------------------------------
 * Activations that are ALREADY fp8 (OCP e4m3fn bytes, e.g. the output of an upstream fp8 kernel or of
 * torch's .to(torch.float8_e4m3fn)), with an optional float32 scale per row:
 *
 *   out[t][n] = act_scales[t] * scale[e][n] * sum_k (q[e][n][k] - zp[e][n]) * e4m3(inputs[t][k])
 *
 *   inputs_e4m3 [T][K] uint8;  act_scales [T] float32 or NULL (= 1);  out [T][N] of out_dtype (FQL_DTYPE_*)
 * One pass of the block-scaled fp8 matrix-core instruction, float32 accumulation; the 4-bit weights are exact in
 * e4m3.  An e4m3 NaN makes its whole output row NaN.  Not in the reference (FP8 is listed as future work,
 * README.md:228); the shape is BASELINE.json configs[4].  MFMA path only: K % 32 == 0 and 16-byte aligned
 * `packed`, otherwise FQL_ERR_ALIGNMENT.  Workspace: fql_moe_workspace_bytes(E, T, K, N, FQL_PRECISION_FP8)
 * (fql_linear_workspace_bytes(B, ...) for the linear form, which takes any B >= 1).
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_moe_fwd_f8(const uint8_t *packed, const float *scales, const float *zps,
                           const uint8_t *inputs_e4m3, const float *act_scales,
                           const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                           int out_dtype, int E, int T, int K, int N, void *workspace,
                           size_t workspace_bytes, void *stream);

FQL_API int fql_linear_fwd_f8(const uint8_t *x_e4m3, const float *act_scales, const uint8_t *packed,
                              const float *scales, const float *zps, void *out, int out_dtype, int B, int K,
                              int N, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-GROUP scales and zero points along K (the layout GPTQ / AWQ-style INT4 checkpoints use;
 * NOT in the reference, whose quantisation is per output row, python/quantize.py:73-80):
 *
 *   out[t][n] = sum_k x[t][k] * (q[n][k] - zps[n][k / group_size]) * scales[n][k / group_size]   (+ bias[n])
 *
 *   scales, zps [N][K / group_size] float32 ([E][N][K / group_size] for the grouped form); group_size even, divides K.
 * Any shape, no workspace.  The weights are dequantised in registers, (q - zp) * scale as the reference kernel does per
 * element, and the contraction is float32: up to 3 rows of ONE matrix (K % 32 == 0, group_size % 32 == 0, 16-byte
 * aligned bases) on the GEMV kernel with the constants folded per 32-k chunk; 4 or more rows per group (K % 64 == 0,
 * group_size % 32 == 0, aligned bases) on the float32 matrix-core instruction; one wave per output row (float32 FMA)
 * otherwise.  The integer MFMA kernels need a single scale per output row: per-row quantisation (group_size == K) stays
 * on the faster entry points above.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_linear_group_fwd_f32(const float *x, const uint8_t *packed, const float *scales,
                                     const float *zps, const float *bias, float *out, int B, int K, int N,
                                     int group_size, void *stream);

FQL_API int fql_moe_group_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                                  const float *inputs, const int32_t *tokens_per_expert,
                                  const int32_t *input_offsets, float *out, int E, int T, int K, int N,
                                  int group_size, void *stream);

/* The same two calls WITH a workspace (fql_group_workspace_bytes bytes, 16-byte aligned): batches (40 or more rows of one
 * matrix, 8 or more rows per expert) with K % 256 == 0 and group_size % 64 == 0 then run on the INT8 matrix cores -- the activation limbs of the
 * per-row path (`precision` as there: exact / fast / int8), integer dot products and limb sums per group, folded in
 * float32 with the group's scale and zero point at the end of every group (csrc/fql_group_i8.h); 2.5-3x the per-row
 * path's time instead of 6x.  Every other shape, or a NULL / short workspace, takes the float32 paths above. */
FQL_API size_t fql_group_workspace_bytes(int E, int T, int K, int N, int group_size, int precision);

FQL_API int fql_linear_group_ws_fwd_f32(const float *x, const uint8_t *packed, const float *scales,
                                        const float *zps, const float *bias, float *out, int B, int K, int N,
                                        int group_size, int precision, void *workspace, size_t workspace_bytes,
                                        void *stream);

FQL_API int fql_moe_group_ws_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                                     const float *inputs, const int32_t *tokens_per_expert,
                                     const int32_t *input_offsets, float *out, int E, int T, int K, int N,
                                     int group_size, int precision, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* The grouped call with per-group scales as the per-row grouped entry points take theirs: rows of any element type, a
 * per-expert bias, a fused activation, a result of any element type (FQL_DTYPE_*), and the input gradient.
 *
 * fql_moe_group_fwd:     out[t][n] = sum_k x[t][k] * W_e[n][k] (+ bias[e][n]) over the rows t of expert e,
 *                        W_e[n][k] = (q[e][n][k] - zps[e][n][k / group_size]) * scales[e][n][k / group_size].
 * fql_moe_group_glu_fwd: the same on h[t][k] = act(gate_up[t][k], gate_up[t][K + k]), gate_up [T][2K], `activation` one of
 *                        FQL_ACT_* with act_alpha / act_limit (ignored for FQL_ACT_SILU) as fql_moe_glu_fwd takes them.
 *   scales, zps [E][N][K / group_size] float32; bias [E][N] float32 or NULL; inputs / gate_up in_dtype, out out_dtype.
 *   Rows no expert covers are zero.  tokens_per_expert / input_offsets: both, or both NULL with E == 1 (one segment).
 *   A 16-bit call is bit for bit the float32 call on the widened operand, rounded once (after the bias).
 *   Workspace: fql_moe_group_typed_workspace_bytes(E, T, K, N, group_size, precision), 16-byte aligned.
 *   INTEGER PATH (K % 256 == 0, group_size % 64 == 0, 8 or more rows per expert on average, 16-byte aligned packed, N >= 4):
 *   the activation pre-pass of the per-row path reads the rows as they are and forms h on the fly, csrc/fql_group_i8.h
 *   contracts on the INT8 matrix cores and rounds once: h is never stored.  Only this path keeps h out of memory.
 *   EVERY OTHER SHAPE: the float32 kernels of fql_moe_group_fwd_f32.  The entry widens 16-bit rows, or writes the
 *   float32 h, into the workspace ([T][K] float32), and a 16-bit result is written as float32 into the workspace
 *   ([T][N]) and rounded from there: two streaming kernels around the GEMM, `precision` does not enter the arithmetic.
 *   Return codes, in this order: FQL_ERR_BAD_PRECISION (unknown, or FQL_PRECISION_FP8); FQL_ERR_BAD_SHAPE (E <= 0, T < 0,
 *   K <= 0, N < 0; glu: an unknown activation, or for a kind other than silu a non-finite act_alpha / act_limit or
 *   act_limit <= 0); FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE (group_size <= 0, odd, or not dividing K); FQL_ERR_DTYPE; T == 0 or
 *   N == 0: FQL_OK with nothing launched; FQL_ERR_NULL_POINTER (packed, scales, zps, inputs, out; one of the table's two
 *   arrays alone); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65535); FQL_ERR_ALIGNMENT (inputs / out not aligned to
 *   their element); FQL_ERR_WORKSPACE (off the integer path, when something is staged: NULL, misaligned or short);
 *   FQL_ERR_LAUNCH.
 *
 * fql_moe_group_bwd_input: grad_in[t][k] = sum_n grad_out[t][n] * W_e[n][k] (csrc/fql_group_bwd.h): the weights
 *   dequantised in registers and staged through LDS, the contraction on the float32 matrix-core instruction.  grad_out
 *   [T][N] of grad_out_dtype is read as it is and widened in registers, grad_in [T][K] of grad_in_dtype is rounded once: a
 *   16-bit call is bit for bit the float32 call on the widened gradient, rounded once.  No atomics; every element of
 *   grad_in is written once, rows no expert covers as zeros by the same launch.  The sum over n runs in a fixed order
 *   (64 n at a time, inside them n0 + s then n0 + 32 + s for s = 0 .. 31), so a row's result depends on its own gradient
 *   row and its expert's weights only: the grouped call equals E one-expert calls on the same rows bit for bit, run to run
 *   and under any permutation of the table.  K % 64 == 0, group_size % 32 == 0 and 16-byte aligned packed / grad_out /
 *   grad_in: the tiled kernel; anything else one wave per row with the same order (correct, not tuned).
 *   fql_moe_group_bwd_workspace_bytes is 0 today (the kernels keep nothing between them) and the workspace may be NULL;
 *   both are part of the signature so that a cached transpose of the constants can move in later.
 *   Return codes, in this order: FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K < 0, N < 0); FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE
 *   (group_size <= 0, odd, or not dividing K); FQL_ERR_DTYPE; T == 0 or K == 0: FQL_OK with nothing launched;
 *   FQL_ERR_NULL_POINTER (grad_in; with N > 0 grad_out, packed, scales, zps; one of the table's two arrays alone);
 *   FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534); FQL_ERR_ALIGNMENT (a base not aligned to its element);
 *   N == 0: grad_in is zeroed; FQL_ERR_LAUNCH. */
FQL_API size_t fql_moe_group_typed_workspace_bytes(int E, int T, int K, int N, int group_size, int precision);
FQL_API int fql_moe_group_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                              const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                              int out_dtype, int E, int T, int K, int N, int group_size, int precision, void *workspace,
                              size_t workspace_bytes, void *stream);
FQL_API int fql_moe_group_glu_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up,
                                  int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                  const float *bias, void *out, int out_dtype, int E, int T, int K, int N, int group_size,
                                  int precision, int activation, float act_alpha, float act_limit, void *workspace,
                                  size_t workspace_bytes, void *stream);
FQL_API size_t fql_moe_group_bwd_workspace_bytes(int E, int T, int K, int N, int group_size);
FQL_API int fql_moe_group_bwd_input(const uint8_t *packed, const float *scales, const float *zps, const void *grad_out,
                                    int grad_out_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                    void *grad_in, int grad_in_dtype, int E, int T, int K, int N, int group_size,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Format helpers on the device (same unpack code path as the GEMM kernels; bit-exact).
 *   fql_unpack_u8     : q[i][2j] = packed[i][j] & 15, q[i][2j+1] = packed[i][j] >> 4
 *                       (python/quantize.py:152-163)
 *   fql_dequantize_f32: w[n][k] = (q[n][k] - zps[n]) * scales[n]   (python/quantize.py:172)
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_unpack_u8(const uint8_t *packed, uint8_t *q, size_t nbytes, void *stream);

FQL_API int fql_dequantize_f32(const uint8_t *packed, const float *scales, const float *zps, float *w,
                       int N, int K, void *stream);

/* ---------------------------------------------------------------------------------------
 * Quantisers on the device, bit-exact with the reference's host arithmetic:
 *   fql_quantize_rows_f32   : python/quantize.py:38-124  per-ROW scale / zero-point (constant-row guard,
 *                             1e-8 floor, round-half-to-even), packed [N][K/2], scales / zps [N]
 *   fql_quantize_tensor_f32 : python/moe_int4_module.py:45-76  per-TENSOR scale / zero-point broadcast to
 *                             [N] (one expert); scratch = 2*N floats of device memory
 *   w [N][K] float32 contiguous (fp16 weights are widened by the caller, as the reference does).
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_quantize_rows_f32(const float *w, uint8_t *packed, float *scales, float *zps, int N, int K,
                                  void *stream);

FQL_API int fql_quantize_tensor_f32(const float *w, uint8_t *packed, float *scales, float *zps,
                                    float *scratch, int N, int K, void *stream);

/* ---------------------------------------------------------------------------------------
 * Phase 1 of the MFMA path on its own: the activation pre-pass (also the tests' window into it).
 *   x[t][k] ~= delta[t] * sum_l 256^l * a_l[t][k],  a_l signed 8-bit ("limbs"), delta a power of two
 *   limbs   fql_act_limb_bytes(T, E, K, precision) bytes, 16-byte aligned, in MFMA-fragment order:
 *           [limb][k / 256][padded_row / 32][k-step 0..7][lane 0..63][16 B]  (see csrc/fql_act_quant.h;
 *           expert e's rows start at padded row sum_{e'<e} roundup(cnt_e', 32); K is zero-padded to
 *           fql_act_padded_k(K))
 *   delta   [T] float32, rowsum [limbs][T] int32 (sum over k of each limb)
 *   tokens_per_expert / input_offsets: device arrays as in fql_moe_fwd_f32, or both NULL with E = 1
 *   for one group covering all T rows.  Rows covered by no expert are skipped.
 *
 * Heavy-tailed rows (FQL_PRECISION_FAST / _EXACT / _DEFAULT): the limbs are per-ROW block fixed point, so one
 * outlier element coarsens the quantum of its whole row.  A row whose 8*limbs-1 bits would not carry the mode's
 * stated precision -- predicted relative output error sqrt(K/12) / ||x/delta||_2 above 1e-6 (3 limbs) or
 * 2.5e-4 (2 limbs); randn rows never are -- gets a SECOND limb set holding the rounding residual
 * (x/delta - X) * 2^(8*limbs-1), quantum delta2 = delta * 2^-(8*limbs-1), which the GEMM adds for that row
 * (16*limbs-2 bits in all).  For these precisions the buffers are therefore doubled:
 *   limbs   fql_act_limb_bytes() bytes = both sets back to back;  delta [2][T] (delta, delta2; delta2 = 0
 *   marks a row without residual);  rowsum [2][limbs][T].
 * FQL_PRECISION_INT8 / _FP8 keep one set.  With _FP8 the plane holds e4m3 bytes, delta the per-row scale
 * max|x| / 448 and rowsum[0] the float32 bits of the row sum.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_act_padded_k(int K);

FQL_API size_t fql_act_limb_bytes(int T, int E, int K, int precision);

FQL_API int fql_act_quant_f32(const float *x, int8_t *limbs, float *delta, int32_t *rowsum,
                              const int32_t *tokens_per_expert, const int32_t *input_offsets, int E,
                              int T, int K, int precision, void *stream);

/* ---------------------------------------------------------------------------------------
 * Phase 2 of the MFMA path on its own: the grouped INT4 x INT8-limb GEMM over activations that
 * fql_act_quant_f32 already converted (fql_linear_fwd_f32 / fql_moe_fwd_f32 = phase 1 + phase 2
 * back to back).  Lets a caller fuse its own gather/dispatch into phase 1, and lets bench.py
 * time the dominant kernel alone.  The expert arrays must be the ones phase 1 was given (they fix
 * the limb layout); tokens_per_expert == NULL means one group covering all T rows (E must be 1).  Requires K % 32 == 0 and a 16-byte aligned `packed`
 * (FQL_ERR_ALIGNMENT otherwise).  Rows covered by no expert are left untouched.
 * `scratch`: fql_gemm_scratch_bytes(precision) bytes, 16-byte aligned -- workgroup-private float32 partials of the
 * residual pass over tiles that hold heavy-tailed rows (see phase 1).  With scratch == NULL (or too small) that
 * pass is skipped and such rows keep the plain 8*limbs-1 bit result.
 * ------------------------------------------------------------------------------------- */
FQL_API size_t fql_gemm_scratch_bytes(int precision);

FQL_API int fql_gemm_i8_f32(const int8_t *limbs, const float *delta, const int32_t *rowsum,
                            const uint8_t *packed, const float *scales, const float *zps,
                            const int32_t *tokens_per_expert, const int32_t *input_offsets,
                            float *out, int E, int T, int K, int N, int precision, void *stream,
                            void *scratch, size_t scratch_bytes);

/* ---------------------------------------------------------------------------------------
 * Dtype-generic forms of fql_linear_fwd_f32 / fql_moe_fwd_f32 (float16 / bfloat16
 * activations and outputs, as the reference's MoE benches feed them).  Same arguments plus the element
 * types; (F32, F32) forwards to the float32 entry points.  16-bit I/O exists on the MFMA path only
 * (more than 2 rows, K % 32 == 0, 16-byte aligned packed weights): other shapes return FQL_ERR_DTYPE and
 * the caller converts.  fql_native_dtype_supported answers that question without launching anything.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_native_dtype_supported(int rows, int E, int K, int N, int precision, const void *packed,
                                       int grouped);

FQL_API int fql_linear_fwd(const void *x, int in_dtype, const uint8_t *packed, const float *scales,
                           const float *zps, void *out, int out_dtype, int B, int K, int N, int precision,
                           void *workspace, size_t workspace_bytes, void *stream);
/* fql_linear_fwd with the optional bias [N] of fql_linear_bias_fwd_f32 (NULL: none), added by the same epilogue: bit for
 * bit fql_linear_bias_fwd_f32 on the widened x, rounded once to out_dtype.  Same shapes, same errors. */
FQL_API int fql_linear_bias_fwd(const void *x, int in_dtype, const uint8_t *packed, const float *scales,
                                const float *zps, const float *bias, void *out, int out_dtype, int B, int K, int N,
                                int precision, void *workspace, size_t workspace_bytes, void *stream);

FQL_API int fql_moe_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs,
                        int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                        void *out, int out_dtype, int E, int T, int K, int N, int precision,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Second GEMM of a gated FFN expert with the activation fused in (the reference models
 * only the up projection, benchmark/moe_grouped_gemm/config.py:50-52):
 *   out[t][:] = W_e * ( silu(gate_up[t][0:K]) (.) gate_up[t][K:2K] )
 * gate_up is the [T, 2K] float32 output of the fused gate|up projection (one grouped GEMM over the stacked
 * [E, 2K, H] weights); the [T, K] hidden activation is never written.  tokens_per_expert / input_offsets as in
 * fql_moe_fwd_f32, or both NULL with E = 1 for a dense layer.  MFMA path only (K % 32 == 0, 16-byte aligned
 * packed weights): FQL_ERR_ALIGNMENT otherwise.  Workspace: fql_moe_workspace_bytes(E, T, K, N, precision).
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_moe_gated_fwd_f32(const uint8_t *packed, const float *scales, const float *zps,
                                  const float *gate_up, const int32_t *tokens_per_expert,
                                  const int32_t *input_offsets, float *out, int E, int T, int K, int N,
                                  int precision, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Routing either side of the grouped GEMM, one launch each (reference: the torch index ops of
 * benchmark/moe_grouped_gemm/routing.py:117-149 create_expert_inputs and :172-189 combine_expert_outputs).
 *
 * fql_route_plan_i32: stable counting sort of the n_slots = tokens * top_k (token, slot) pairs by expert id
 *   (expert_of_slot = expert_indices flattened, ids clamped into [0, E), E <= 128).  Outputs, all int32 on the
 *   device: counts[E] and offsets[E] (= tokens_per_expert / input_offsets), token_of_sorted[n_slots] (the
 *   row_index of fql_moe_gather_fwd_f32) and pos_of_slot[n_slots] (where each slot's result row lands).
 * fql_combine_f32: out[t][:] = sum_{k < top_k} weights[t][k] * y[pos_of_slot[t*top_k + k]][:], k ascending;
 *   y is [R, N], out [T, N] (T <= 65535).  weights == NULL: a pure gather-add of rows that already carry their
 *   weight (fql_moe_gather_scaled_fwd_f32).
 * fql_regroup_index_i32 (expert-parallel receive side): recv_counts[G][EL] rows per (source rank, local expert)
 *   in arrival order -> tokens_per_expert[EL], input_offsets[EL], gather[R] (expert-major position -> received
 *   row, the row_index of fql_moe_gather_fwd_f32) and scatter[R] (its inverse); G * EL <= 8192.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_route_plan_i32(const int32_t *expert_of_slot, int n_slots, int top_k, int E, int32_t *counts,
                               int32_t *offsets, int32_t *token_of_sorted, int32_t *pos_of_slot,
                               void *stream);

FQL_API int fql_combine_f32(const float *y, const int32_t *pos_of_slot, const float *weights, float *out,
                            int T, int top_k, int N, int R, void *stream);

/* ---------------------------------------------------------------------------------------
 * The router in front of fql_route_plan_i32 (csrc/fql_router.h): softmax over a token's logits, its top_k experts and
 * their routing weights in one launch, and the backward of that in one launch.  No workspace.
 *
 * fql_router_topk_fwd: logits [T][E] contiguous, float32 / float16 / bfloat16 (logits_dtype, an FQL_DTYPE_* code; 16-bit
 *   values are widened exactly), 1 <= E <= 128, 1 <= top_k <= min(E, 8).  Outputs: indices [T][top_k] int32 (the
 *   expert_of_slot of fql_route_plan_i32), weights [T][top_k] float32 (the weights of fql_combine_f32) and, unless
 *   probs == NULL, probs [T][E] float32, the full softmax.
 *     selection: on the logits; slot j holds the j-th largest, ties go to the lower expert id
 *                (torch.sort(-logits, stable=True).indices[:, :top_k]).
 *     p_e = exp(l_e - m) / sum_e' exp(l_e' - m), m the row maximum, float32, accurate expf, pairwise sums.
 *     renormalize != 0: weights[j] = p_{e_j} / sum_i p_{e_i} (Mixtral);  renormalize == 0: weights[j] = p_{e_j}.
 *     a row with a non-finite logit: NaN weights, NaN probs, indices 0 .. top_k-1 (always valid ids in [0, E)).
 *     a token's results depend on its own row alone (not on T or on its neighbours), and are the same bits every call.
 * fql_router_topk_bwd: grad_logits [T][E] in the logits' element type (rounded once) from the saved logits and indices
 *   and the incoming grad_weights [T][top_k] and / or grad_probs [T][E] (float32; either may be NULL, both NULL: zeros).
 *   With g = grad_weights and w, p recomputed from the logits:
 *     renormalize != 0: dl_{e_j} = w_j * (g_j - sum_i w_i g_i), exactly 0.0 for every expert no slot names;
 *     renormalize == 0: dl_e = p_e * ([e selected] g_e - sum_j p_{e_j} g_j);
 *     grad_probs: dl_e += p_e * (grad_probs_e - sum_e' p_e' grad_probs_e').
 *   Fixed summation order, no atomics.  A row with a non-finite logit gets a NaN row (also with both gradients NULL).
 * Return codes, both, in this order and all before any HIP call: FQL_ERR_DTYPE (logits_dtype); FQL_ERR_BAD_SHAPE
 *   (T < 0, E < 1, E > 128, top_k < 1, top_k > E, top_k > 8); T == 0: FQL_OK with nothing launched;
 *   FQL_ERR_NULL_POINTER (logits, indices, weights / grad_logits); then FQL_ERR_LAUNCH.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_router_topk_fwd(const void *logits, int logits_dtype, int T, int E, int top_k, int renormalize,
                                int32_t *indices, float *weights, float *probs, void *stream);
FQL_API int fql_router_topk_bwd(const void *logits, int logits_dtype, const int32_t *indices, const float *grad_weights,
                                const float *grad_probs, void *grad_logits, int T, int E, int top_k, int renormalize,
                                void *stream);

/* ---------------------------------------------------------------------------------------
 * The scored router (csrc/fql_router.h): the routing rules of DeepSeek-V2 / V3, GLM-4.5, Kimi-K2 and Llama-4 in one
 * launch, and the backward of that in one launch.  No workspace.  The thread mapping, the element types, the limits on
 * E and top_k and the outputs are those of fql_router_topk_fwd / _bwd above.
 *
 * fql_router_score_topk_fwd: logits [T][E]; scoring 0 = softmax, 1 = sigmoid; select_bias [E] float32 or NULL; the
 *   experts form n_group groups of E / n_group (1 <= n_group <= 8, E % n_group == 0) of which the topk_group best are
 *   searched (topk_group * (E / n_group) >= top_k); group_top 1 or 2; scale finite.  Outputs: indices [T][top_k] int32,
 *   weights [T][top_k] float32 and, unless scores == NULL, scores [T][E] float32.
 *     scores:    softmax p_e (the bits of fql_router_topk_fwd's probs), or s_e = 1 / (1 + expf(-l_e)), float32, accurate
 *                expf; the sigmoid saturates to exactly 1.0f and 0.0f.
 *     key:       select_bias == NULL: the logit.  Otherwise score_e + select_bias_e, one float32 add; a NaN key counts
 *                as -infinity (a non-finite bias is the caller's error; the ids stay in [0, E)).
 *     groups:    (n_group > 1) group c holds the experts [c * E / n_group, (c + 1) * E / n_group); its score is the
 *                largest (group_top == 1) or the sum of the two largest (group_top == 2; a one-member group: its single
 *                value) of score_e + select_bias_e (bias 0 when NULL); the topk_group best groups are chosen, ties to the
 *                lower group id.  Experts outside them are never selected (the Hugging Face code fills their keys with
 *                0.0 instead, so that a masked expert beats a negative key; the two agree when all keys are positive).
 *     slots:     slot j holds the j-th largest key among the allowed experts, ties (-0.0 == 0.0 included) to the lower id.
 *     weights:   from the unbiased scores.  softmax: (p_{e_j} / sum_i p_{e_i}) * scale (renormalize != 0, the formula
 *                of fql_router_topk_fwd) or p_{e_j} * scale.  sigmoid: (s_{e_j} / (sum_i s_{e_i} + 1e-20f)) * scale or
 *                s_{e_j} * scale.
 *     a row with a non-finite logit: NaN weights, NaN scores, indices 0 .. top_k-1.
 *     scoring == 0, select_bias == NULL, n_group == 1 and scale == 1: the bits of fql_router_topk_fwd.
 * fql_router_score_topk_bwd: grad_logits [T][E] in the logits' element type (rounded once) from the saved logits and
 *   indices and grad_weights [T][top_k] and / or grad_scores [T][E] (float32; either may be NULL, both NULL: zeros).  The
 *   groups and the bias do not enter (the indices are saved; the bias gets no gradient).  With g_j = scale * grad_weights_j:
 *     softmax:   the formulas of fql_router_topk_bwd with g (scale == 1: its bits).
 *     sigmoid:   d_e = s_e * (1 - s_e), 1 - s_e computed as the sigmoid of -l_e;  renormalize != 0, with
 *                D = sum_i s_{e_i} + 1e-20f and u_i = s_{e_i} / D: dl_{e_j} = d_{e_j} * (g_j - sum_i u_i g_i) / D;
 *                renormalize == 0: dl_{e_j} = d_{e_j} * g_j;  exactly 0.0 for every expert no slot names;
 *                grad_scores: dl_e += d_e * grad_scores_e.
 *   Fixed summation order, no atomics.  A row with a non-finite logit gets a NaN row (also with both gradients NULL).
 * Return codes, both, in this order and all before any HIP call: FQL_ERR_DTYPE (logits_dtype); FQL_ERR_BAD_SHAPE
 *   (T < 0, E < 1, E > 128, top_k < 1, top_k > E, top_k > 8, scoring not 0 or 1, scale not finite and, forward only:
 *   n_group < 1, n_group > 8, E % n_group != 0, topk_group < 1, topk_group > n_group, topk_group * (E / n_group) < top_k,
 *   group_top not 1 or 2); T == 0: FQL_OK with nothing launched; FQL_ERR_NULL_POINTER (logits, indices, weights /
 *   grad_logits); then FQL_ERR_LAUNCH.
 * ------------------------------------------------------------------------------------- */
FQL_API int fql_router_score_topk_fwd(const void *logits, int logits_dtype, int T, int E, int top_k, int scoring,
                                      const float *select_bias, int n_group, int topk_group, int group_top,
                                      int renormalize, float scale, int32_t *indices, float *weights, float *scores,
                                      void *stream);
FQL_API int fql_router_score_topk_bwd(const void *logits, int logits_dtype, const int32_t *indices,
                                      const float *grad_weights, const float *grad_scores, void *grad_logits, int T, int E,
                                      int top_k, int scoring, int renormalize, float scale, void *stream);

/* ---- backward (input gradients; the INT4 weights are frozen: no weight gradient) ----
 * fql_linear_bwd_input_f32: grad_in[B][K] = grad_out[B][N] @ W, W[n][k] = (q[n][k] - zps[n]) * scales[n], on the INT8
 *   matrix cores (csrc/fql_bwd.h): g = grad_out * scales (one float32 rounding) is split into `precision` limbs per row
 *   exactly as the forward splits x (3 for DEFAULT / EXACT, 2 for FAST, 1 for INT8 and FP8), the weights enter as the
 *   exact integers q - clamp(rint(zp), -112, 112), and the fractional part of non-integer zero points is applied as a
 *   float32 correction per row.  float32 gradients here; fql_linear_bwd_input / fql_moe_bwd_input (below) take
 *   float16 / bfloat16 gradients as they are, so a 16-bit caller converts nothing.  Any even K, any N in
 *   [0, FQL_BWD_MAX_N] (the i32 accumulation is exact up to 2^31 / (128 * 127) = 132104).  Every element of grad_in
 *   is written once: deterministic, no atomics.
 * fql_moe_bwd_input_f32: the grouped form: grad_in[t] = grad_out[t] @ W_e for the rows of expert e's range
 *   (tokens_per_expert / input_offsets on the device, never read back), packed [E][N][K/2], scales / zps [E][N];
 *   rows no expert covers are zeroed.
 *   Both: B / T == 0 or K == 0 -> FQL_OK with nothing done; N == 0 (or E == 0) -> grad_in zeroed; workspace at least
 *   fql_*_bwd_workspace_bytes(), 16-byte aligned.  Errors: FQL_ERR_BAD_PRECISION, FQL_ERR_BAD_SHAPE (negative
 *   dimension, N > FQL_BWD_MAX_N, E > 65535, 31-bit workspace / weight offsets exceeded), FQL_ERR_ODD_K,
 *   FQL_ERR_NULL_POINTER, FQL_ERR_WORKSPACE, FQL_ERR_LAUNCH -- in that order, all before any HIP call.
 * fql_combine_bwd_f32: gradients of fql_combine_f32 in one launch, no atomics (pos_of_slot must be a permutation of
 *   the rows of y that it names): grad_y[pos[t][k]] = weights[t][k] * grad_out[t] (weights == NULL: grad_out[t]);
 *   grad_weights[t][k] = <y[pos[t][k]], grad_out[t]> (skipped when grad_weights == NULL).  Rows of grad_y no slot
 *   names are not written.
 *
 * fql_linear_bwd_input / fql_moe_bwd_input: the same two gradients with an element type (FQL_DTYPE_*) for grad_out and
 *   one for grad_in.  The pre-pass loads a 16-bit grad_out directly and widens it in registers (exact) before the
 *   multiply by scales[n], so the limbs are those of the float32 call on the widened gradient; the GEMM's epilogue
 *   rounds grad_in once to nearest even on store.  Contract: bit for bit the _f32 entry point on the widened grad_out,
 *   rounded once to grad_in_dtype as Tensor.to(dtype) rounds (float16 overflow gives inf).  No float32 copy of a [T][N]
 *   or [T][K] tensor exists anywhere; the workspace (fql_*_bwd_workspace_bytes) is unchanged.  (float32, float32) is the
 *   _f32 entry point.  Errors: as above, with FQL_ERR_DTYPE (an element type that is not FQL_DTYPE_F32 / _F16 / _BF16)
 *   after FQL_ERR_BAD_PRECISION, FQL_ERR_BAD_SHAPE and FQL_ERR_ODD_K and before everything else: before the empty-call
 *   FQL_OK, FQL_ERR_NULL_POINTER, FQL_ERR_WORKSPACE and FQL_ERR_LAUNCH. */
#define FQL_BWD_MAX_N 132104
FQL_API size_t fql_linear_bwd_workspace_bytes(int B, int K, int N, int precision);
FQL_API int fql_linear_bwd_input_f32(const float *grad_out, const uint8_t *packed, const float *scales, const float *zps,
                                     float *grad_in, int B, int K, int N, int precision, void *ws, size_t ws_bytes,
                                     void *stream);
FQL_API size_t fql_moe_bwd_workspace_bytes(int E, int T, int K, int N, int precision);
FQL_API int fql_moe_bwd_input_f32(const uint8_t *packed, const float *scales, const float *zps, const float *grad_out,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *grad_in, int E,
                                  int T, int K, int N, int precision, void *ws, size_t ws_bytes, void *stream);
FQL_API int fql_linear_bwd_input(const void *grad_out, int grad_out_dtype, const uint8_t *packed, const float *scales,
                                 const float *zps, void *grad_in, int grad_in_dtype, int B, int K, int N, int precision,
                                 void *ws, size_t ws_bytes, void *stream);
FQL_API int fql_moe_bwd_input(const uint8_t *packed, const float *scales, const float *zps, const void *grad_out,
                              int grad_out_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                              void *grad_in, int grad_in_dtype, int E, int T, int K, int N, int precision, void *ws,
                              size_t ws_bytes, void *stream);
FQL_API int fql_combine_bwd_f32(const float *grad_out, const float *y, const int32_t *pos_of_slot, const float *weights,
                                float *grad_y, float *grad_weights, int T, int top_k, int N, int rows, void *stream);

/* ---- the typed combine with an addend (FQL_VERSION 290; csrc/fql_routing.h) ----
 * fql_combine: fql_combine_f32 with an element type (FQL_DTYPE_F32 / _F16 / _BF16) for y and one for out, and an optional
 *   per-token weighted addend (a shared expert's rows) added behind the slot terms:
 *     out[t][n] = round_out( (...((0 + y[p_0][n] * w_0) + y[p_1][n] * w_1)...) + addend[t][n] * addend_weight[t] )
 *   y [R][N] and addend [T][N] (or NULL: no term) have in_dtype, out [T][N] has out_dtype, weights [T][top_k] (or NULL:
 *   1) and addend_weight [T] (or NULL: 1, the bits of "+ addend") are float32.  The slot terms are those of
 *   fql_combine_f32: float32, multiply then add (never an FMA), k ascending, pos_of_slot clamped into [0, R).  16-bit
 *   elements are widened in registers (exact); a 16-bit out is rounded once to nearest even as Tensor.to rounds (float16
 *   overflow gives inf).  So without an addend the result is bit for bit fql_combine_f32 on the widened rows, rounded
 *   once.  T <= 65535.  (float32, float32) without an addend is fql_combine_f32 itself.
 * fql_combine_bwd: its gradients in one launch, no atomics (pos_of_slot a permutation of the rows it names).  grad_out
 *   [T][N] has out_dtype; grad_y [rows][N] and grad_addend [T][N] have in_dtype and are rounded once; grad_weights
 *   [T][top_k] and grad_addend_weight [T] are float32:
 *     grad_y[pos[t][k]] = weights[t][k] * grad_out[t] (weights == NULL: grad_out[t]); rows no slot names are not written;
 *     grad_weights[t][k] = <y[pos[t][k]], grad_out[t]>          (NULL: skipped);
 *     grad_addend[t] = addend_weight[t] * grad_out[t]           (NULL: skipped; addend_weight == NULL: grad_out[t]);
 *     grad_addend_weight[t] = <addend[t], grad_out[t]>          (NULL: skipped).
 *   Both dot products use the reduction of fql_combine_bwd_f32 (the same bits on the widened operands).  (float32,
 *   float32) with the four addend pointers NULL is fql_combine_bwd_f32 itself.
 * Return codes, both, in this order and all before any HIP call:
 *   1. FQL_ERR_BAD_SHAPE: T < 0, top_k <= 0, N < 0, R / rows < 0 (backward: rows == 0 with T > 0);
 *   2. FQL_ERR_DTYPE: in_dtype or out_dtype outside FQL_DTYPE_*;
 *   3. the empty call, FQL_OK with nothing launched: T == 0 or N == 0 (backward: T == 0, or N == 0 with grad_weights and
 *      grad_addend_weight both NULL);
 *   4. FQL_ERR_NULL_POINTER: y, pos_of_slot, out NULL or R == 0 (backward: pos_of_slot; with N > 0 grad_out, grad_y, and
 *      y when grad_weights is given); addend_weight without addend; grad_addend_weight without addend;
 *   5. FQL_ERR_BAD_SHAPE: T > 65535 (forward only);
 *   6. FQL_ERR_ALIGNMENT: a data pointer not aligned to its element size;
 *   7. FQL_ERR_LAUNCH. */
FQL_API int fql_combine(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights, const void *addend,
                        const float *addend_weight, void *out, int out_dtype, int T, int top_k, int N, int R, void *stream);
FQL_API int fql_combine_bwd(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot,
                            const float *weights, const void *addend, const float *addend_weight, int in_dtype,
                            void *grad_y, float *grad_weights, void *grad_addend, float *grad_addend_weight, int T,
                            int top_k, int N, int rows, void *stream);

/* ---- low-rank adapters (LoRA) on the INT4 layers: csrc/fql_lora.h ----
 * Segmented float32 kernels for y = W_q x + scale * B (A x), per expert e over the rows of its range.  The adapter
 * weight of a call is `w` (or the output `d` of the gradient), stored in one of two layouts:
 *   FQL_LORA_RC: [E][r][C] (lora_A, [r, K] per expert)        FQL_LORA_CR: [E][C][r] (lora_B, [N, r] per expert)
 * and read as W_e[j][c] whichever way it is stored.
 *
 * fql_lora_shrink_f32: out[t][j] = scale * sum_c in[t][c] * W_e[j][c]            in [T][C] -> out [T][r]
 *   (forward U = X A_e^T with w = lora_A, RC; backward dU = s G B_e with w = lora_B, CR).  Rows no expert covers
 *   get zeros.
 * fql_lora_expand_f32: out[t][c] = in[t][c] + scale * sum_j v[t][j] * W_e[c][j]  v [T][r] -> out [T][C]
 *   (forward Y += s U B_e^T with w = lora_B, CR; backward dX += dU A_e with w = lora_A, RC).  in == out is allowed
 *   (in place); in == NULL starts from zero.  Rows no expert covers are copied from `in` (zeroed when in == NULL,
 *   left alone in place).
 * fql_lora_grad_f32: d_e[c][j] = scale * sum_{t of e} p[t][c] * v[t][j], stored [E][C][r] (d_layout FQL_LORA_CR:
 *   dB_e = s G_e^T U_e) or [E][r][C] (FQL_LORA_RC: dA_e = dU_e^T X_e).  Experts without rows get zeros; rows no
 *   expert covers contribute nothing.
 *
 * All three: E experts, T rows, C columns (K or N), rank r in {4, 8, 16, 32, 64}; float32 operands and float32
 * accumulation on the vector FMA units.  tokens_per_expert / input_offsets are the int32 device table of the grouped
 * GEMM (never read back; ranges must not overlap and are clamped into [0, T)); both NULL with E == 1 is one segment
 * of all T rows (the linear layer: no table on the device).  No atomics and no workspace: every output element is
 * written once in a fixed order, so two runs are bitwise equal, and an expert's rows (and its d_e) equal bit for bit
 * the E == 1 call on its rows alone.  Rows of C floats are streamed 16 bytes per lane when C % 4 == 0 and the [T][C]
 * operands are 16-byte aligned (8 bytes when C % 2 == 0, else 4).
 * Errors, in this order and all before any HIP call: r not in the list, a layout other than FQL_LORA_RC /
 * FQL_LORA_CR, a negative dimension, E > 65535, or T * C, T * r or E * C * r past 2^31 -> FQL_ERR_BAD_SHAPE;
 * T == 0 -> FQL_OK with nothing done (also C == 0 for expand and grad, and E == 0 for grad); a NULL data pointer,
 * only one of the two table pointers, or no table with E != 1 -> FQL_ERR_NULL_POINTER; `w` (shrink, expand) or
 * `v` and `d` (grad) not 16-byte aligned -> FQL_ERR_ALIGNMENT; FQL_ERR_LAUNCH.  The Python surface is
 * ops.lora_shrink / lora_expand / lora_grad and the differentiable ops.linear_lora_forward / moe_lora_forward
 * (INTEGRATION.md section 6).
 *
 * fql_lora_shrink / fql_lora_expand / fql_lora_grad: the same three kernels with an element type (FQL_DTYPE_F32 / _F16 /
 * _BF16) for each streamed [T][C] operand: `in` of shrink, `p` of grad, and `in` and `out` of expand, each on its own.
 * [T][r] tensors (out of shrink, v), adapter weights and their gradients are float32, and so is every accumulator.
 * 16-bit elements are widened in registers on load (exact) and a 16-bit `out` is rounded once, to nearest even, on
 * store.  Contract: a call returns, bit for bit, what the _f32 entry point returns on the exactly widened operands,
 * (expand) rounded once to out_dtype as Tensor.to(dtype) rounds -- whenever both calls take the same vector width:
 *   vector width, in ELEMENTS: 4 when C % 4 == 0 and every [T][C] base pointer of the call is aligned to 4 of its own
 *   elements (16 bytes float32, 8 bytes 16-bit), else 2 under the same rule (8 / 4 bytes), else 1.
 * The width fixes the column-to-lane mapping and, for shrink, the order of the sum over c.  16-byte aligned bases on both
 * sides always give equal widths; a 16-bit base that is only 2- or 4-byte aligned takes a narrower width than the float32
 * call on an aligned copy and then agrees with it to rounding of the float32 sums only (expand and grad do not depend on
 * the width: one lane per output column, fixed order over j / t).  Determinism, grouped == per-expert and the handling of
 * uncovered rows are those of the _f32 entry points.  expand: in == out (in place) needs in_dtype == out_dtype; in_dtype is
 * ignored when in == NULL.  (float32[, float32]) calls are forwarded to the _f32 entry points.
 * Errors, in this order and all before any HIP call: FQL_ERR_BAD_SHAPE as above; then FQL_ERR_DTYPE: an element type
 * outside FQL_DTYPE_*, or expand with in == out and in_dtype != out_dtype; then the empty-call FQL_OK,
 * FQL_ERR_NULL_POINTER and FQL_ERR_ALIGNMENT as above (plus a [T][C] base not aligned to its element size), FQL_ERR_LAUNCH. */
#define FQL_LORA_RC 0
#define FQL_LORA_CR 1
FQL_API int fql_lora_shrink_f32(const float *in, const float *w, int w_layout, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, float *out, int E, int T, int C, int r, float scale,
                                void *stream);
FQL_API int fql_lora_expand_f32(const float *v, const float *w, int w_layout, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, const float *in, float *out, int E, int T, int C, int r,
                                float scale, void *stream);
FQL_API int fql_lora_grad_f32(const float *p, const float *v, const int32_t *tokens_per_expert,
                              const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                              float scale, void *stream);
FQL_API int fql_lora_shrink(const void *in, int in_dtype, const float *w, int w_layout, const int32_t *tokens_per_expert,
                            const int32_t *input_offsets, float *out, int E, int T, int C, int r, float scale,
                            void *stream);
FQL_API int fql_lora_expand(const float *v, const float *w, int w_layout, const int32_t *tokens_per_expert,
                            const int32_t *input_offsets, const void *in, int in_dtype, void *out, int out_dtype, int E,
                            int T, int C, int r, float scale, void *stream);
FQL_API int fql_lora_grad(const void *p, int p_dtype, const float *v, const int32_t *tokens_per_expert,
                          const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r, float scale,
                          void *stream);

/* ---- adapters on the gated FFN experts (QuantizedMoEFFN): y = W_d h + s B_d (A_d h), h = silu(g) * u ----
 * The hidden activation h [T][C] is never stored; the down adapter reads it from gate_up = [g | u] ([T][2C], the
 * output of the fused gate|up projection) exactly as fql_moe_gated_fwd_f32 does: both call one device function, so
 * the adapter and the INT4 GEMM see the same bits of h.
 *
 * fql_lora_gated_shrink_f32: fql_lora_shrink_f32 with in[t][c] = silu(gate_up[t][c]) * gate_up[t][C + c]
 *   (forward U_d = h A_d^T with w = down lora_A, RC).
 * fql_lora_gated_grad_f32: fql_lora_grad_f32 with p[t][c] formed the same way (dA_d = dU_d^T h, RC).
 *   Both: same kernels, tiles and reduction orders as the plain entry points (a compile-time flag on the operand
 *   load), so their bitwise promises hold; same arguments, checks, order and codes, with 2 * T * C added to the
 *   sizes that must stay below 2^31.  Both halves of a row are streamed once, 16 bytes per lane when gate_up,
 *   gate_up + C and the pitch 2 C allow (8 when they allow 8, else 4).
 * fql_swiglu_bwd_f32: dgate_up[t] = [dg | du] from gate_up [T][2F] and dh [T][F]:
 *   sigma = 1 / (1 + exp(-g)), dg = dh u sigma (1 + g (1 - sigma)), du = dh g sigma.  One streaming pass over every
 *   row (no expert table), 16-byte accesses when F % 4 == 0 and the three pointers are 16-byte aligned.  Finite for
 *   every finite g (g very negative: sigma = 0, both gradients 0).  Errors, in this order: T < 0, F < 0 or
 *   2 * T * F past 2^31 -> FQL_ERR_BAD_SHAPE; T == 0 or F == 0 -> FQL_OK with nothing done; a NULL pointer ->
 *   FQL_ERR_NULL_POINTER; dgate_up == gate_up -> FQL_ERR_BAD_SHAPE (not in place); FQL_ERR_LAUNCH.
 * All three: one launch, no workspace, no allocation, no host synchronisation, no atomics, graph-capturable.  The
 * Python surface is ops.lora_gated_shrink / lora_gated_grad / swiglu_backward and the differentiable
 * ops.moe_ffn_lora_forward. */
FQL_API int fql_lora_gated_shrink_f32(const float *gate_up, const float *w, int w_layout,
                                      const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                      int T, int C, int r, float scale, void *stream);
FQL_API int fql_lora_gated_grad_f32(const float *gate_up, const float *v, const int32_t *tokens_per_expert,
                                    const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                                    float scale, void *stream);
FQL_API int fql_swiglu_bwd_f32(const float *gate_up, const float *dh, float *dgate_up, int T, int F, void *stream);

/* ---- the gated FFN experts on float16 / bfloat16 activations (FQL_VERSION 260) ----
 * The four entry points above with an element type (FQL_DTYPE_F32 / _F16 / _BF16) for every [T][.] activation tensor.
 * One contract, that of the typed adapter entry points: a call returns, bit for bit, what the _f32 entry point returns
 * on the exactly widened operands, a 16-bit output rounded once to nearest even as Tensor.to(dtype) rounds (float16
 * overflow gives inf).  16-bit elements are widened in registers on load; h = silu(g) * u is the float32 act_silu_mul of
 * the widened values, so the INT4 GEMM and the down adapter still see the same bits of h.  All-float32 calls are
 * forwarded to the _f32 entry points.
 *
 * fql_moe_gated_fwd: fql_moe_gated_fwd_f32 with gate_up [T][2K] of in_dtype and out [T][N] of out_dtype.  The limbs are
 *   those of the float32 call on the widened gate_up; rows no expert covers are zeroed in out_dtype.  Workspace:
 *   fql_moe_workspace_bytes(E, T, K, N, precision), unchanged.  Errors, in this order and all before any HIP call:
 *   FQL_ERR_BAD_PRECISION (unknown, or FQL_PRECISION_FP8), FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0, N < 0),
 *   FQL_ERR_ODD_K, FQL_ERR_DTYPE (an element type outside FQL_DTYPE_*), T == 0 or N == 0 -> FQL_OK with nothing done,
 *   FQL_ERR_NULL_POINTER (a data pointer, or only one table pointer), FQL_ERR_BAD_SHAPE (no table with E != 1,
 *   E > 65535), FQL_ERR_ALIGNMENT (K % 32 != 0, packed not 16-byte aligned, gate_up not aligned to its element),
 *   FQL_ERR_WORKSPACE, FQL_ERR_LAUNCH.
 * fql_lora_gated_shrink / fql_lora_gated_grad: the _f32 entry points with gate_up [T][2C] of `dtype`; out / v / d stay
 *   float32.  The vector width, in ELEMENTS, is the widest (4, 2, 1) that gate_up, gate_up + C and the pitch 2 C all
 *   allow at the element size, so a 16-byte aligned tensor takes the same width in every type and the tiles, the
 *   column-to-lane mapping and every reduction order are those of the float32 kernel.  Errors: FQL_ERR_BAD_SHAPE as the
 *   _f32 forms, then FQL_ERR_DTYPE, then the empty-call FQL_OK, FQL_ERR_NULL_POINTER, FQL_ERR_ALIGNMENT (w, or v and d,
 *   not 16-byte aligned; gate_up not aligned to its element), FQL_ERR_LAUNCH.
 * fql_swiglu_bwd: fql_swiglu_bwd_f32 with one element type each for gate_up, dh and dgate_up.  The arithmetic is the
 *   float32 kernel's, term for term, on the widened values; a 16-bit dgate_up is rounded once.  Errors:
 *   FQL_ERR_BAD_SHAPE as the _f32 form, FQL_ERR_DTYPE, the empty-call FQL_OK, FQL_ERR_NULL_POINTER, dgate_up == gate_up
 *   -> FQL_ERR_BAD_SHAPE, a pointer not aligned to its element -> FQL_ERR_ALIGNMENT, FQL_ERR_LAUNCH. */
FQL_API int fql_moe_gated_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up,
                              int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                              int out_dtype, int E, int T, int K, int N, int precision, void *workspace,
                              size_t workspace_bytes, void *stream);
FQL_API int fql_lora_gated_shrink(const void *gate_up, int dtype, const float *w, int w_layout,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                  int T, int C, int r, float scale, void *stream);
FQL_API int fql_lora_gated_grad(const void *gate_up, int dtype, const float *v, const int32_t *tokens_per_expert,
                                const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                                float scale, void *stream);
FQL_API int fql_swiglu_bwd(const void *gate_up, int dtype, const void *dh, int dh_dtype, void *dgate_up, int out_dtype,
                           int T, int F, void *stream);

/* ---- activation kinds of the gated FFN experts (FQL_VERSION 300) ----
 * The four typed entry points above with `int activation, float act_alpha, float act_limit` in front of `workspace` /
 * `stream`.  All kinds are one family, h = g' * sigma(a) * u', float32 arithmetic on the widened operands, evaluated as
 * (g' / (1.0f + expf(-a))) * u' (the library is built with -fno-fast-math):
 *
 *   FQL_ACT_SILU          g' = g               u' = u                                   a = g                  a' = 1
 *   FQL_ACT_GELU_TANH     g' = g               u' = u                                   a = g (c0 + c1 g g)    a' = c0 + 3 c1 g g
 *   FQL_ACT_SWIGLU_CLAMP  g' = min(g, limit)   u' = min(max(u, -limit), limit) + 1      a = alpha g'           a' = alpha
 *
 * c0 = 2 sqrt(2 / pi) = 1.5957691216057308 and c1 = 0.044715 c0 = 0.0713548162726009, each rounded once to float32.
 * FQL_ACT_GELU_TANH is the tanh form of GELU ("gelu_pytorch_tanh"): g sigma(a) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715
 * g^3))), since 0.5 (1 + tanh z) = sigma(2 z).  It is written with the sigmoid because 1 + tanh z cancels for negative g and
 * the family form does not.  FQL_ACT_SWIGLU_CLAMP is gpt-oss's (alpha = 1.702, limit = 7.0 there).
 * Backward, sig = 1.0f / (1.0f + expf(-a)): dg = dh u' (sig (1 + g' a' (1 - sig))), du = dh (g' sig); the clamped kind
 * gives dg = 0 exactly where g > limit and du = 0 exactly where u < -limit or u > limit (equality passes the gradient, as
 * torch.clamp's backward does).  Every finite input gives finite outputs (expf overflow: sig = 0).
 * One device function forms h and one (dg, du) (csrc/fql_common.h) for the pre-pass, the adapter loads and the backward,
 * so the INT4 GEMM, the down adapter and the backward see the same bits of h.
 *
 * activation == FQL_ACT_SILU: the call IS the entry point above (same kernels, same bits, same return codes); act_alpha and
 * act_limit are ignored.  The other kinds run kernels of their own (csrc/fql_glu.hip; any element type, float32 included)
 * under the 16-bit contract above: bit for bit the float32 call on the widened operands, 16-bit outputs rounded once.
 * Errors: an activation outside FQL_ACT_*, an act_alpha that is not finite, or an act_limit that is not finite or <= 0
 * (checked for both non-silu kinds) -> FQL_ERR_BAD_SHAPE, reported where the sibling reports its first FQL_ERR_BAD_SHAPE;
 * every other check, its order and its code are the sibling's:
 * fql_moe_glu_fwd: FQL_ERR_BAD_PRECISION (unknown, or FQL_PRECISION_FP8), FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0, N < 0, or
 *   the activation arguments), FQL_ERR_ODD_K, FQL_ERR_DTYPE, T == 0 or N == 0 -> FQL_OK with nothing done,
 *   FQL_ERR_NULL_POINTER, FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65535), FQL_ERR_ALIGNMENT, FQL_ERR_WORKSPACE,
 *   FQL_ERR_LAUNCH.  Workspace: fql_moe_workspace_bytes(E, T, K, N, precision), unchanged.
 * fql_lora_glu_shrink / fql_lora_glu_grad: FQL_ERR_BAD_SHAPE (rank, layout, dimensions, sizes, or the activation
 *   arguments), FQL_ERR_DTYPE, the empty-call FQL_OK, FQL_ERR_NULL_POINTER, FQL_ERR_ALIGNMENT (w, or v and d, not 16-byte
 *   aligned; gate_up not aligned to its element), FQL_ERR_LAUNCH.
 * fql_glu_bwd: FQL_ERR_BAD_SHAPE (T < 0, F < 0, 2 T F past 2^31, or the activation arguments), FQL_ERR_DTYPE, the
 *   empty-call FQL_OK, FQL_ERR_NULL_POINTER, dgate_up == gate_up -> FQL_ERR_BAD_SHAPE, a pointer not aligned to its element
 *   -> FQL_ERR_ALIGNMENT, FQL_ERR_LAUNCH. */
#define FQL_ACT_SILU 0
#define FQL_ACT_GELU_TANH 1
#define FQL_ACT_SWIGLU_CLAMP 2
FQL_API int fql_moe_glu_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up, int in_dtype,
                            const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                            int E, int T, int K, int N, int precision, int activation, float act_alpha, float act_limit,
                            void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_lora_glu_shrink(const void *gate_up, int dtype, const float *w, int w_layout,
                                const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                                int C, int r, float scale, int activation, float act_alpha, float act_limit, void *stream);
FQL_API int fql_lora_glu_grad(const void *gate_up, int dtype, const float *v, const int32_t *tokens_per_expert,
                              const int32_t *input_offsets, float *d, int d_layout, int E, int T, int C, int r,
                              float scale, int activation, float act_alpha, float act_limit, void *stream);
FQL_API int fql_glu_bwd(const void *gate_up, int dtype, const void *dh, int dh_dtype, void *dgate_up, int out_dtype, int T,
                        int F, int activation, float act_alpha, float act_limit, void *stream);

/* ---- per-expert biases of the grouped GEMM (FQL_VERSION 310) ----
 * fql_moe_bias_fwd: fql_moe_fwd with `const float *bias` in front of `out`: [E][N] float32, expert e's bias is added to the
 *   rows of expert e in the GEMM's epilogue, out = dtype(fl32(acc + bias[e][n])) -- the float32 result of fql_moe_fwd plus
 *   the bias, rounded once for a 16-bit out.  Rows no expert covers stay exactly zero: the bias belongs to an expert, not
 *   to the output.  bias == NULL: the call IS fql_moe_fwd (same kernels, same bits, same return codes).  With a bias the
 *   checks, their order and their codes are fql_moe_fwd's (16-bit I/O off the MFMA path: FQL_ERR_DTYPE; float32 off it: the
 *   generic kernel, which takes the bias too), but E == 0 or K == 0 is FQL_ERR_BAD_SHAPE where the float32 call writes
 *   zeros (an empty contraction plus a bias is not a path worth a kernel; fql_linear_bias_fwd_f32 answers the same).
 * fql_moe_glu_bias_fwd: fql_moe_glu_fwd with the same `bias` in front of `out`, for every activation kind (FQL_ACT_SILU
 *   included) and every element type.  bias == NULL: the call IS fql_moe_glu_fwd.  With a bias the checks, their order and
 *   their codes are those listed for fql_moe_glu_fwd above, for every kind (FQL_ACT_SILU ignores act_alpha / act_limit).
 *   Without a table (both NULL, E == 1) the one bias row belongs to every row.
 * fql_moe_bias_grad: the gradient of such a bias,
 *     grad_bias[e][n] = sum over the rows t of expert e of grad_rows[t][n],
 *   grad_rows [T][N] of `dtype` (FQL_DTYPE_*; 16-bit elements are widened exactly), grad_bias [E][N] float32.  The expert
 *   table is fql_moe_fwd_f32's (device arrays, ranges clipped to [0, T)); both NULL with E == 1: all rows.  Every one of
 *   the E * N outputs is written: an expert without rows gets zeros, T == 0 writes all zeros.  Any N >= 1: 16-byte loads
 *   when grad_rows is 16-byte aligned and N * sizeof(element) is a multiple of 16, element loads otherwise.  float32
 *   accumulation, no atomics, no workspace.  The summation order of an expert depends on its row count alone (csrc/
 *   fql_bias.hip): not on the grid, E, the offsets, other experts' counts, the element type or the load width, so the result
 *   is run-to-run identical and unchanged when the table is permuted.
 *   Errors, in order: FQL_ERR_BAD_SHAPE (E < 0, T < 0, N < 0, E > 65535, N > 2^31 - 256), FQL_ERR_DTYPE, E == 0 or N == 0 ->
 *   FQL_OK with nothing done, FQL_ERR_NULL_POINTER (grad_bias; grad_rows when T > 0; one half of the table), FQL_ERR_BAD_SHAPE
 *   (no table with E != 1), FQL_ERR_ALIGNMENT (grad_rows not aligned to its element, grad_bias not to 4 bytes),
 *   FQL_ERR_LAUNCH. */
FQL_API int fql_moe_bias_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                             const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                             int out_dtype, int E, int T, int K, int N, int precision, void *workspace,
                             size_t workspace_bytes, void *stream);
FQL_API int fql_moe_glu_bias_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up,
                                 int in_dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                 const float *bias, void *out, int out_dtype, int E, int T, int K, int N, int precision,
                                 int activation, float act_alpha, float act_limit, void *workspace, size_t workspace_bytes,
                                 void *stream);
FQL_API int fql_moe_bias_grad(const void *grad_rows, int dtype, const int32_t *tokens_per_expert,
                              const int32_t *input_offsets, float *grad_bias, int E, int T, int N, void *stream);

/* ---- slots that go nowhere: expert capacity and a token mask (FQL_VERSION 320; INTEGRATION.md section 15, DESIGN.md
 *      section 23; csrc/fql_routing.h) ----
 * fql_route_plan_capped_i32: fql_route_plan_i32 with a token mask and a per-expert capacity.  Expert ids are clamped into
 *   [0, E), E <= 128.  Slot i belongs to token i / top_k and is ELIGIBLE when token_mask is NULL or
 *   token_mask[i / top_k] != 0 (token_mask: [n_slots / top_k] bytes on the device).  demand[e] is the number of eligible
 *   slots of expert e: the router's choice before any drop.  The eligible slots of an expert are walked in ascending slot
 *   order (the stable order of fql_route_plan_i32); a slot is KEPT when its rank in that order is < capacity, or when
 *   capacity == 0 (no limit): earlier tokens win, the "position" drop policy of GShard and Megatron-Core.
 *     counts[e]  = min(demand[e], capacity) kept slots, offsets[] their exclusive prefix: the kept rows are compact and in
 *                  expert order, S = sum of the counts <= n_slots;
 *     token_of_sorted[0, S) the token of each kept row; token_of_sorted[S, n_slots) = 0 (a valid gather index; no expert
 *                  covers those rows, so the grouped GEMM writes zeros there);
 *     pos_of_slot[i] the kept row of slot i, or -1 for a dropped or masked slot.
 *   With token_mask == NULL and capacity == 0 every output equals fql_route_plan_i32's, and demand == counts.  One
 *   workgroup, no atomics: the result is deterministic.  n_slots == 0 writes demand, counts and offsets as zeros.
 *   Return codes, in this order:
 *     1. FQL_ERR_BAD_SHAPE: n_slots < 0, top_k <= 0, E outside [1, 128], capacity < 0, n_slots % top_k != 0;
 *     2. FQL_ERR_NULL_POINTER: demand, counts or offsets NULL; with n_slots > 0 expert_of_slot, token_of_sorted or
 *        pos_of_slot NULL (token_mask may be NULL);
 *     3. FQL_ERR_LAUNCH.
 * fql_combine_sparse: fql_combine that SKIPS a slot with pos_of_slot < 0 where fql_combine clamps it to row 0: the slot
 *   adds nothing, and neither its row of y nor its weight is read.  pos_of_slot >= R is clamped to R - 1 as there.  A token
 *   whose slots are all dropped gets its addend term alone, or zeros.  For finite y the result is bit for bit fql_combine
 *   on the same inputs with the negative positions set to 0 and the dropped slots' weights set to 0 (the accumulator starts
 *   at +0 and cannot become -0).
 * fql_combine_sparse_bwd: fql_combine_bwd for it.  pos_of_slot is an injection of the kept slots into the rows.  A dropped
 *   slot writes no row of grad_y and gets grad_weights == 0; rows no kept slot names are not written, so the caller hands
 *   in a zeroed grad_y.  On the kept slots, and for the addend's two gradients, the bits are fql_combine_bwd's.
 *   Arguments, return codes and their order: those of fql_combine / fql_combine_bwd above. */
FQL_API int fql_route_plan_capped_i32(const int32_t *expert_of_slot, int n_slots, int top_k, int E, const uint8_t *token_mask,
                                      int capacity, int32_t *demand, int32_t *counts, int32_t *offsets,
                                      int32_t *token_of_sorted, int32_t *pos_of_slot, void *stream);
FQL_API int fql_combine_sparse(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights,
                               const void *addend, const float *addend_weight, void *out, int out_dtype, int T, int top_k,
                               int N, int R, void *stream);
FQL_API int fql_combine_sparse_bwd(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot,
                                   const float *weights, const void *addend, const float *addend_weight, int in_dtype,
                                   void *grad_y, float *grad_weights, void *grad_addend, float *grad_addend_weight, int T,
                                   int top_k, int N, int rows, void *stream);

/* ---- OCP MXFP4 expert weights, forward only (FQL_VERSION 340; INTEGRATION.md section 17, DESIGN.md section 25;
 *      csrc/fql_gemm_mx4.h) ----
 * A second frozen 4-bit weight format for the grouped GEMM, the one gpt-oss ships its experts in:
 *   blocks      [E][N][K / 2] uint8, two e2m1 codes a byte, even k in the low nibble (the INT4 byte layout).  Codes 0 .. 7 are
 *               0, 0.5, 1, 1.5, 2, 3, 4, 6; codes 8 .. 15 their negatives (8 is -0);
 *   scales_e8m0 [E][N][K / 32] uint8: code s in 0 .. 254 is 2^(s - 127) for weight row n and inputs 32 b .. 32 b + 31, code 255
 *               is NaN (the whole block, zeros included).
 * fql_moe_mx4_fwd:     out[t][n] = sum_k bf16(x[t][k]) * W_e[n][k] (+ bias[e][n]) over the rows t of expert e; inputs [T][K]
 *                      float32 (rounded once to bfloat16, to nearest even) or bfloat16 (read as they are).
 * fql_moe_mx4_glu_fwd: the same on h[t][k] = bf16(act(gate_up[t][k], gate_up[t][K + k])), gate_up [T][2K] float32 or bfloat16,
 *                      h evaluated in float32 (act_glu_mul, the kinds of FQL_ACT_*) and rounded once, by a streaming pre-pass
 *                      into the workspace ([T][K] bfloat16): the caller never holds it.
 *   The weights are exact in bfloat16; the contraction runs on v_mfma_f32_32x32x16_bf16 with float32 accumulation in a fixed
 *   order (64 k a stage, four instructions of 16 k each), so a row's result depends on its own activation row and its
 *   expert's weights only: the grouped call equals E one-expert calls bit for bit, under any permutation of the table and
 *   run to run.  bias [E][N] float32 or NULL is added in the epilogue, then comes the one rounding to out_dtype (float32,
 *   bfloat16 or float16).  No atomics; every element of out [T][N] is written once, rows no expert covers as zeros by the
 *   same launch.  tokens_per_expert / input_offsets: both, or both NULL with E == 1 (one segment).
 *   The table contract of every fql_moe_mx4_* entry (forward in each precision, fql_moe_mx4_bwd_input) is fql_moe_fwd_f32's:
 *   raw int32 (offset, count) pairs in any order, clipped on the device to [0, T] (a count <= 0 or an offset past T is an
 *   empty expert); the clipped ranges must not overlap; rows no expert covers are zero in the result, and as
 *   inputs they never enter a covered row's result, whatever they hold.
 *   Non-finite values: a non-finite activation (or h) makes its whole output row NaN; a scale code 255 makes exactly the
 *   outputs of its weight row NaN, for the rows of its expert.  A weight below 2^-126 in magnitude (scale codes 0 and 1 with
 *   the smallest element codes) may be flushed to zero, and one of 2^128 or more (scale code 254 with |code| >= 2) is
 *   infinite, as it is in float32.
 *   float16 inputs are refused (FQL_ERR_DTYPE): rounding them to bfloat16 would silently lose three bits.
 *   Workspace: fql_moe_mx4_workspace_bytes(E, T, K, N, gated): 0 for fql_moe_mx4_fwd (gated == 0; the arguments may be NULL
 *   / 0), the [T][K] bfloat16 h for fql_moe_mx4_glu_fwd (gated != 0), 16-byte aligned.
 *   Return codes, in this order and all before any HIP call: FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0, N < 0; glu: an unknown
 *   activation, or for a kind other than silu a non-finite act_alpha / act_limit or act_limit <= 0); FQL_ERR_ODD_K;
 *   FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE (in_dtype not FQL_DTYPE_F32 / _BF16, out_dtype outside FQL_DTYPE_*);
 *   T == 0 or N == 0: FQL_OK with nothing launched; FQL_ERR_NULL_POINTER (blocks, scales_e8m0, inputs / gate_up, out; one of
 *   the table's two arrays alone); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534, T > 4194240); FQL_ERR_ALIGNMENT
 *   (blocks not 16-byte aligned; inputs / gate_up / out not aligned to their element, bias not to 4 bytes);
 *   FQL_ERR_WORKSPACE (glu: NULL, misaligned or short); FQL_ERR_LAUNCH. */
FQL_API size_t fql_moe_mx4_workspace_bytes(int E, int T, int K, int N, int gated);
FQL_API int fql_moe_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                            const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                            int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                float act_limit, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the decode kernel of the bfloat16 MXFP4 forward (FQL_VERSION 380; INTEGRATION.md section 17, DESIGN.md section 29;
 *      csrc/fql_gemm_mx4_decode.h) ----
 * fql_moe_mx4_fwd and fql_moe_mx4_glu_fwd (the latter behind its pre-pass) run one of two kernels: the 64-row x 128-column
 * tile of FQL_VERSION 340, or, when T is at most a threshold built into the library (FQL_MX4_DECODE_MAX_ROWS in
 * csrc/fql_mx4.hip, set from a measurement; 0 disables it) and ceil(T / 32) <= 65535, a decode kernel in which one wave streams
 * 32 weight rows of one expert over all of K for a block of up to 32 rows.  Only T decides: the per-expert counts stay on the
 * device.  Signatures, checks, return codes, workspace and the non-finite rules are unchanged.
 *   The two kernels return THE SAME BITS for every element of out: both issue v_mfma_f32_32x32x16_bf16 with the weights as the
 *   A operand over k0 = 0, 16, 32, ... on an accumulator that starts at zero, feed it the same dequantised weights and the same
 *   rounded rows, and share the epilogue.  So the guarantee above (a row's result depends on its own row and its expert's
 *   weights only, not on T, E or the table) holds across the threshold.  The input gradient has the tile form only (the
 *   fp8 / MXFP4-row modes have their own decode kernel: FQL_VERSION 390, below).  fql_int4_tune.h: fql_tune_set_mx4_decode_max_rows / fql_tune_mx4_kernel force and report the
 *   choice (tools and tests). */

/* ---- the decode kernels of the fp8-row and MXFP4-row precisions (FQL_VERSION 390; INTEGRATION.md section 17, DESIGN.md
 *      section 32; csrc/fql_gemm_mx4_sdecode.h) ----
 * fql_moe_mx4_fwd_f8 / _fwd_q8 / _glu_fwd_q8 and fql_moe_mx4_fwd_f4 / _fwd_q4 / _glu_fwd_q4 (the quantising ones behind their
 * pre-pass, which is unchanged) run one of two kernels as well: the 64-row x 128-column tile of FQL_VERSION 360 / 370, or, when
 * T is at most a threshold built into the library per precision (FQL_MX4_F8_DECODE_MAX_ROWS / FQL_MX4_F4_DECODE_MAX_ROWS in
 * csrc/fql_mx4.hip, set from a measurement; 0 disables it) and ceil(T / 32) <= 65535, a decode kernel in which one wave streams
 * 32 weight rows of one expert over all of K for a block of up to 32 rows.  Only T decides.  Signatures, checks, return codes,
 * workspace sizes and the non-finite rules are unchanged.
 *   The two kernels return THE SAME BITS for every element of out: both issue ceil(K / 64) v_mfma_scale_f32_32x32x64_f8f6f4 in
 *   ascending k on an accumulator that starts at zero, the weights as A, the rows as B, every lane with the same bytes and the
 *   same scale bytes, and share the epilogue.  So a row's result does not depend on T across the threshold either.  The
 *   thresholds are independent of each other and of the bfloat16 one.  fql_int4_tune.h: the hooks with `scaled` in their names
 *   force and report the choice (tools and tests). */

/* ---- the input gradient of the MXFP4 expert weights (FQL_VERSION 350; INTEGRATION.md section 17, DESIGN.md section 26;
 *      csrc/fql_gemm_mx4_bwd.h) ----
 * fql_moe_mx4_bwd_input: grad_in[t][k] = sum_n bf16(grad_out[t][n]) * W_e[n][k] over the rows t of expert e, on the blocks and
 *   scales_e8m0 of the forward entries.  grad_out [T][N] float32 (rounded once to bfloat16, to nearest even) or bfloat16 (read
 *   as it is); float16 is refused as in the forward.  grad_in [T][K] of out_dtype (float32, bfloat16 or float16), rounded once.
 *   The transposed grouped GEMM on v_mfma_f32_32x32x16_bf16 with float32 accumulation in a fixed order (64 n a stage, four
 *   instructions of 16 n each): a row's result depends on its own gradient row and its expert's weights only, so the grouped
 *   call equals E one-expert calls bit for bit, under any permutation of the table and run to run.  No atomics, no
 *   workspace; every element of grad_in is written once, rows no expert covers as zeros by the same launch.  The table as in
 *   the forward (both arrays, or both NULL with E == 1).
 *   Non-finite values: a non-finite element of a gradient row makes that whole row of grad_in NaN; a scale code 255 makes
 *   grad_in NaN for exactly the 32 k of its block, on the rows of its expert.
 *   grad_out and grad_in need the alignment of their element only (16-byte aligned operands take the wide loads / stores).
 *   Return codes, in this order and all before any HIP call: FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0, N < 0); FQL_ERR_ODD_K;
 *   FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE (in_dtype not FQL_DTYPE_F32 / _BF16, out_dtype outside FQL_DTYPE_*);
 *   T == 0: FQL_OK with nothing launched; N == 0 (T > 0): the gradient of an empty contraction, grad_in [T][K] is set to zeros
 *   and nothing else is read or checked: FQL_ERR_NULL_POINTER (grad_in), else FQL_OK; FQL_ERR_NULL_POINTER (blocks,
 *   scales_e8m0, grad_out, grad_in; one of the table's two arrays alone); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534,
 *   T > 4194240); FQL_ERR_ALIGNMENT (blocks not 16-byte aligned; grad_out / grad_in not aligned to their element);
 *   FQL_ERR_LAUNCH. */
FQL_API int fql_moe_mx4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                  int out_dtype, int E, int T, int K, int N, void *stream);

/* ---- MXFP4 expert weights over fp8 rows, on the block-scaled FP4 matrix cores (FQL_VERSION 360; INTEGRATION.md section 17,
 *      DESIGN.md section 27; csrc/fql_gemm_mx4_scaled.h) ----
 * The opt-in second mode of the MXFP4 forward; the bfloat16 entries above and their bits are unchanged.
 *   out[t][n] = act_scale[t] * ( sum_k e4m3(x8[t][k]) * W_e[n][k] ) (+ bias[e][n]),   blocks / scales_e8m0 as above.
 * The packed bytes and the E8M0 bytes go to v_mfma_scale_f32_32x32x64_f8f6f4 as they lie in memory (fp4 A operand with its
 * block scale), the activation rows are OCP e4m3 bytes (0x7F / 0xFF: NaN) in the B operand with scale code 127; nothing is
 * dequantised.  float32 accumulation inside the instruction, 128 k a stage in ascending k, two instructions of 64 k each,
 * one accumulator per output: a row's result depends on its own bytes, its act_scale and its expert's weights only, so
 * the grouped call equals E one-expert calls bit for bit, under any permutation of the table and run to run.  Epilogue in
 * float32: act_scale[t] * acc (one multiplication; NULL: acc as it is), with a bias fma(act_scale[t], acc, bias[e][n])
 * (one rounding), then the one rounding to out_dtype.  No atomics; every element of out [T][N] is written once, rows no
 * expert covers as zeros by the same launch.  Any K % 32 == 0, any N >= 1.
 * fql_moe_mx4_fwd_f8:     inputs_e4m3 [T][K] bytes, act_scale [T] float32 or NULL (= 1).  No workspace (mode 0: 0 bytes, the
 *                         arguments may be NULL / 0).
 * fql_moe_mx4_fwd_q8:     inputs [T][K] float32 or bfloat16 (widened), quantised per row by a streaming pre-pass into the
 *                         workspace (mode 1): scale = max|x| / 448 in float32 (1 for an all-zero row), byte = e4m3(x / scale)
 *                         with a float32 division, to nearest even; then the call above on those bytes and scales.
 * fql_moe_mx4_glu_fwd_q8: the same on h[t][k] = act(gate_up[t][k], gate_up[t][K + k]) evaluated in float32 (act_glu_mul, the
 *                         kinds of FQL_ACT_*) from gate_up [T][2K] float32 or bfloat16 (mode 2); h itself is never stored.
 *   Non-finite values: an e4m3 NaN byte or a NaN act_scale makes exactly that output row NaN; a float row (or h) with a
 *   non-finite element gets a NaN scale, hence a NaN output row; a scale code 255 makes exactly the outputs of its weight row
 *   NaN, for the rows of its expert.  Scale codes 0 and 254 are 2^-127 and 2^127 as the instruction applies them (measured:
 *   1.0 * 2^-127 comes back as the float32 subnormal 0x00400000, nothing is flushed inside the instruction; sums past the
 *   float32 range are infinite).
 *   float16 rows are refused (FQL_ERR_DTYPE) as in fql_moe_mx4_fwd.
 *   Workspace: fql_moe_mx4_f8_workspace_bytes(E, T, K, N, mode), mode 0 (rows already e4m3): 0; mode 1 (float rows) and 2
 *   (gated): the e4m3 rows [T][K] and act_scale [T], each rounded up to 16 bytes; 16-byte aligned.
 *   Return codes, in this order and all before any HIP call (fql_moe_mx4_fwd's): FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0,
 *   N < 0; glu: an unknown activation, or for a kind other than silu a non-finite act_alpha / act_limit or act_limit <= 0);
 *   FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE (q8: in_dtype not FQL_DTYPE_F32 / _BF16; all: out_dtype
 *   outside FQL_DTYPE_*); T == 0 or N == 0: FQL_OK with nothing launched; FQL_ERR_NULL_POINTER (blocks, scales_e8m0, the rows,
 *   out; one of the table's two arrays alone); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534, T > 4194240);
 *   FQL_ERR_ALIGNMENT (blocks not 16-byte aligned; float rows / out not aligned to their element, bias and act_scale not to
 *   4 bytes; the e4m3 rows need none, 16-byte aligned ones take the wide loads); FQL_ERR_WORKSPACE (q8: NULL, misaligned or
 *   short); FQL_ERR_LAUNCH. */
FQL_API size_t fql_moe_mx4_f8_workspace_bytes(int E, int T, int K, int N, int mode);
FQL_API int fql_moe_mx4_fwd_f8(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *inputs_e4m3,
                               const float *act_scale, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_glu_fwd_q8(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream);

/* ---- MXFP4 expert weights over MXFP4 rows: both operands e2m1 with E8M0 block scales (FQL_VERSION 370; INTEGRATION.md
 *      section 17; csrc/fql_gemm_mx4_scaled.h) ----
 * The opt-in third mode of the MXFP4 forward (W4A4); the entries above and their bits are unchanged.
 *   out[t][n] = sum_k X[t][k] * W_e[n][k] (+ bias[e][n]),  X[t][k] = e2m1(in_blocks) * 2^(in_scales_e8m0[t][k / 32] - 127).
 * The rows lie in the weights' own layout: in_blocks [T][K / 2] (even k in the low nibble), in_scales_e8m0 [T][K / 32].  Both
 * sides go to v_mfma_scale_f32_32x32x64_f8f6f4 as they lie in memory (cbsz = 4, blgp = 4, each with its scale byte); nothing
 * is dequantised.  float32 accumulation inside the instruction, 128 k a stage in ascending k, two instructions of 64 k each,
 * one accumulator per output: a row's result depends on its own bytes, its scales and its expert's weights only, so the
 * grouped call equals E one-expert calls bit for bit, under any permutation of the table and run to run.  Epilogue in
 * float32: acc, with a bias acc + bias[e][n] (one addition), then the one rounding to out_dtype.  No atomics; every element
 * of out [T][N] is written once, rows no expert covers as zeros by the same launch.  Any K % 32 == 0, any N >= 1.
 * fql_moe_mx4_fwd_f4:     rows already MXFP4.  No workspace (mode 0: 0 bytes, the arguments may be NULL / 0).
 * fql_moe_mx4_fwd_q4:     inputs [T][K] float32 or bfloat16 (widened), quantised by a streaming pre-pass into the workspace
 *                         (mode 1) by the rule below; then the call above on those bytes.
 * fql_moe_mx4_glu_fwd_q4: the same on h[t][k] = act(gate_up[t][k], gate_up[t][K + k]) evaluated once in float32 (act_glu_mul,
 *                         the kinds of FQL_ACT_*) from gate_up [T][2K] float32 or bfloat16 (mode 2); h itself is never stored.
 * fql_mx4_quantize_rows:  the quantiser alone: rows [T][K] (gated != 0: gate_up [T][2K] with the activation arguments, which
 *                         are not looked at otherwise) -> out_blocks [T][K / 2], out_scales [T][K / 32].
 *   The rule (the OCP MX rule, quantize_mxfp4 of the Python package bit for bit, for every finite input, float32 subnormals
 *   included): per block of 32 consecutive k, shared = floor(log2(max|v|)) - 2 clamped to [-127, 127], scale code
 *   shared + 127 (127 for an all-zero block); elements v / 2^shared to nearest even on the e2m1 grid, saturated at +-6, the
 *   sign kept (a negative value that rounds to zero is code 8).
 *   Non-finite values: a block of a row that holds an inf or a NaN gets zero codes and scale code 255.  A scale code 255 on
 *   the activation side makes exactly that output row NaN, on the weight side exactly the outputs of its weight row, for the
 *   rows of its expert (the instruction does both by itself; measured, profiles/mfma_f4f4_probe.txt).  Scale codes 0 and 254
 *   are 2^-127 and 2^127 on both sides; sums past the float32 range are infinite.
 *   float16 rows are refused (FQL_ERR_DTYPE) as in fql_moe_mx4_fwd.
 *   Workspace: fql_moe_mx4_f4_workspace_bytes(E, T, K, N, mode), mode 0 (rows already MXFP4): 0; mode 1 (float rows) and 2
 *   (gated): the packed rows [T][K / 2] and their scales [T][K / 32], each rounded up to 16 bytes; 16-byte aligned.  0 for
 *   T or K of 0.
 *   Return codes, in this order and all before any HIP call (fql_moe_mx4_fwd's): FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0,
 *   N < 0; glu / gated: an unknown activation, or for a kind other than silu a non-finite act_alpha / act_limit or
 *   act_limit <= 0); FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE (q4 and quantize_rows: in_dtype not
 *   FQL_DTYPE_F32 / _BF16; the GEMMs: out_dtype outside FQL_DTYPE_*); T == 0 or N == 0: FQL_OK with nothing launched;
 *   FQL_ERR_NULL_POINTER (blocks, scales_e8m0, the rows, out; f4: in_scales_e8m0; one of the table's two arrays alone;
 *   quantize_rows: rows, out_blocks, out_scales); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534, T > 4194240);
 *   FQL_ERR_ALIGNMENT (blocks not 16-byte aligned; float rows / out not aligned to their element, bias not to 4 bytes; f4:
 *   in_blocks not 16-byte aligned, in_scales_e8m0 needs none; quantize_rows: out_blocks not 16-byte aligned);
 *   FQL_ERR_WORKSPACE (q4: NULL, misaligned or short); FQL_ERR_LAUNCH. */
FQL_API size_t fql_moe_mx4_f4_workspace_bytes(int E, int T, int K, int N, int mode);
FQL_API int fql_moe_mx4_fwd_f4(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *in_blocks,
                               const uint8_t *in_scales_e8m0, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_glu_fwd_q4(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_mx4_quantize_rows(const void *rows, int in_dtype, int gated, int activation, float act_alpha, float act_limit,
                                  uint8_t *out_blocks, uint8_t *out_scales, int T, int K, void *stream);

/* ---- MXFP4 expert weights over MXFP6 rows: e2m3 rows with E8M0 block scales (FQL_VERSION 400; INTEGRATION.md section 17,
 *      DESIGN.md section 34; csrc/fql_gemm_mx4_scaled.h) ----
 * The opt-in fourth mode of the MXFP4 forward; the entries above and their bits are unchanged.
 *   out[t][n] = sum_k X[t][k] * W_e[n][k] (+ bias[e][n]),  X[t][k] = e2m3(in_codes) * 2^(in_scales_e8m0[t][k / 32] - 127).
 * The row format: in_codes [T][3 K / 4]; block b of row t is the 24 bytes at 24 b of the row, and element i of the block
 * (k = 32 b + i) is bits 6 i .. 6 i + 5 of those 24 bytes read as one little-endian 192-bit integer.  A code is sign << 5 |
 * exponent << 3 | mantissa: e2m3 with bias 1, subnormals m / 8, largest value 7.5, no inf or NaN.  in_scales_e8m0 [T][K / 32]
 * as for MXFP4 rows.  A block goes to v_mfma_scale_f32_32x32x64_f8f6f4 as it lies in memory (weights cbsz = 4, rows blgp = 2,
 * each with its scale byte; measured, profiles/mfma_f6_probe.txt); the instruction runs at the rate of the MXFP4-row mode.
 * Order, accumulation, epilogue, the table, the decode form and the independence of rows are those of the MXFP4-row entries
 * (FQL_VERSION 370 / 390): the grouped call equals E one-expert calls bit for bit and the tile and decode kernels return the
 * same bits.  Any K % 32 == 0, any N >= 1.
 * fql_moe_mx4_fwd_f6:     rows already MXFP6.  No workspace (mode 0: 0 bytes, the arguments may be NULL / 0).
 * fql_moe_mx4_fwd_q6:     inputs [T][K] float32 or bfloat16 (widened), quantised by a streaming pre-pass into the workspace
 *                         (mode 1) by the rule below; then the call above on those bytes.
 * fql_moe_mx4_glu_fwd_q6: the same on h[t][k] = act(gate_up[t][k], gate_up[t][K + k]) evaluated once in float32 from gate_up
 *                         [T][2K] float32 or bfloat16 (mode 2); h itself is never stored.
 * fql_mx6_quantize_rows:  the quantiser alone: rows [T][K] (gated != 0: gate_up [T][2K] with the activation arguments, which
 *                         are not looked at otherwise) -> out_codes [T][3 K / 4], out_scales [T][K / 32].
 *   The rule (quantize_mxfp6 of the Python package bit for bit, for every finite input, float32 subnormals included): per
 *   block of 32 consecutive k, shared = floor(log2(max|v|)) - 2 clamped to [-127, 127], scale code shared + 127 (127 for an
 *   all-zero block); elements v / 2^shared to nearest even on the e2m3 grid, saturated at +-7.5, the sign kept (a negative
 *   value that rounds to zero is code 32).
 *   Non-finite values: a block of a row that holds an inf or a NaN gets zero codes and scale code 255.  A scale code 255 on
 *   the activation side makes exactly that output row NaN, on the weight side exactly the outputs of its weight row, for the
 *   rows of its expert.  Scale codes 0 and 254 are 2^-127 and 2^127 on both sides; sums past the float32 range are infinite.
 *   float16 rows are refused (FQL_ERR_DTYPE) as in fql_moe_mx4_fwd.
 *   Workspace: fql_moe_mx4_f6_workspace_bytes(E, T, K, N, mode), mode 0 (rows already MXFP6): 0; mode 1 (float rows) and 2
 *   (gated): the codes [T][3 K / 4] and their scales [T][K / 32], each rounded up to 16 bytes; 16-byte aligned.  0 for T or K
 *   of 0.
 *   Return codes, in this order and all before any HIP call (fql_moe_mx4_fwd's): FQL_ERR_BAD_SHAPE (E <= 0, T < 0, K <= 0,
 *   N < 0; glu / gated: an unknown activation, or for a kind other than silu a non-finite act_alpha / act_limit or
 *   act_limit <= 0); FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE (q6 and quantize_rows: in_dtype not
 *   FQL_DTYPE_F32 / _BF16; the GEMMs: out_dtype outside FQL_DTYPE_*); T == 0 or N == 0: FQL_OK with nothing launched;
 *   FQL_ERR_NULL_POINTER (blocks, scales_e8m0, the rows, out; f6: in_scales_e8m0; one of the table's two arrays alone;
 *   quantize_rows: rows, out_codes, out_scales); FQL_ERR_BAD_SHAPE (no table with E != 1, E > 65534, T > 4194240);
 *   FQL_ERR_ALIGNMENT (blocks not 16-byte aligned; float rows / out not aligned to their element, bias not to 4 bytes; f6:
 *   in_codes not 8-byte aligned (a row is a multiple of 24 bytes, so every block then is), in_scales_e8m0 needs none;
 *   quantize_rows: out_codes not 16-byte aligned); FQL_ERR_WORKSPACE (q6: NULL, misaligned or short); FQL_ERR_LAUNCH. */
FQL_API size_t fql_moe_mx4_f6_workspace_bytes(int E, int T, int K, int N, int mode);
FQL_API int fql_moe_mx4_fwd_f6(const uint8_t *blocks, const uint8_t *scales_e8m0, const uint8_t *in_codes,
                               const uint8_t *in_scales_e8m0, const float *bias, const int32_t *tokens_per_expert,
                               const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                               void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_fwd_q6(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                               int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_glu_fwd_q6(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                   void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                   float act_limit, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_mx6_quantize_rows(const void *rows, int in_dtype, int gated, int activation, float act_alpha, float act_limit,
                                  uint8_t *out_codes, uint8_t *out_scales, int T, int K, void *stream);

/* ---- low-rank adapters on the MXFP4 expert weights, fused into the bfloat16 GEMMs (FQL_VERSION 410; INTEGRATION.md
 *      section 17; csrc/fql_gemm_mx4.h, csrc/fql_gemm_mx4_bwd.h) ----
 * The adapter forms of fql_moe_mx4_fwd, fql_moe_mx4_glu_fwd and fql_moe_mx4_bwd_input: the adapter term is one more
 * contraction stage of the same kernel, behind the last weight stage, so no float32 [T][N] result is written and read back.
 * fql_moe_mx4_lora_fwd:       out[t][n] = sum_k bf16(x[t][k]) W_e[n][k] + sum_{j < rank} bf16(v[t][j]) bf16(B[e][n][j]) (+ bias[e][n])
 * fql_moe_mx4_glu_lora_fwd:   the same on h = bf16(act(gate_up)) (fql_moe_mx4_glu_fwd's pre-pass and workspace, unchanged)
 * fql_moe_mx4_lora_bwd_input: grad_in[t][k] = sum_n bf16(grad_out[t][n]) W_e[n][k] + sum_{j < rank} bf16(dv[t][j]) bf16(A[e][j][k])
 *   lora_rows [T][rank] float32: the caller's shrunk rows, v = s A x in the forward, dv = s grad_out B in the gradient (the
 *   entries take no scale); lora_B [E][N][rank] and lora_A [E][rank][K] float32, PEFT's layouts; rank one of 4, 8, 16, 32, 64.
 *   The adapter operands are rounded once to bfloat16 (to nearest even) on their way into LDS, as the rows are.  The order is
 *   fixed: the weight stages ascending as in the base entries, then j = 0 .. in steps of 16, so a row's result depends on its
 *   own rows of x and v and its expert's W and B only, and the grouped call equals E one-expert calls bit for bit.  With
 *   lora_B (lora_A) all zeros and finite lora_rows the result is the base entry's, bit for bit.
 *   These entries always run the 64-row tile kernel (no decode form: they are for training); everything else (the table, the
 *   zeroed rows no expert covers, the bias, the one rounding to out_dtype, scale code 255) is the base entry's.
 *   Non-finite values: a non-finite element of a row of lora_rows makes that whole row of the result NaN, as a non-finite x
 *   / grad_out does; lora_B / lora_A are not screened, a non-finite element gives what the arithmetic gives.
 *   lora_rows and the adapter matrix need 4-byte alignment only (16-byte aligned ones take the wide loads).
 *   Return codes: the base entry's, in its order, with FQL_ERR_BAD_SHAPE for a rank outside the five behind the dtype check
 *   (before T == 0 / N == 0 returns FQL_OK with nothing launched), FQL_ERR_NULL_POINTER for a NULL lora_rows or adapter matrix
 *   with the other pointers and FQL_ERR_ALIGNMENT for one not aligned to 4 bytes, all before any HIP call.
 *   fql_moe_mx4_lora_bwd_input with N == 0 and T > 0 is FQL_ERR_BAD_SHAPE (the base entry's empty contraction has no adapter
 *   form). */
FQL_API int fql_moe_mx4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                                 const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                 const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                 int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_glu_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                     const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                     const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                                     int E, int T, int K, int N, int activation, float act_alpha, float act_limit,
                                     void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_mx4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *grad_out, int in_dtype,
                                       const float *lora_rows, const float *lora_A, int rank, const int32_t *tokens_per_expert,
                                       const int32_t *input_offsets, void *grad_in, int out_dtype, int E, int T, int K, int N,
                                       void *stream);

/* ---- a dense MXFP4 linear layer, with a split-K decode form (FQL_VERSION 420; INTEGRATION.md section 17, DESIGN.md
 *      section 36; csrc/fql_gemm_mx4_linear.h) ----
 * One MXFP4 matrix, no experts: blocks [N][K / 2] and scales_e8m0 [N][K / 32] in the encoding of fql_moe_mx4_fwd.
 * fql_linear_mx4_fwd:     out[t][n] = sum_k bf16(x[t][k]) * W[n][k] (+ bias[n]); inputs [T][K] float32 or bfloat16, bias [N]
 *                         float32 or NULL, out [T][N] of out_dtype, rounded once.
 * fql_linear_mx4_glu_fwd: the same on h = bf16(act(gate_up[t][k], gate_up[t][K + k])), gate_up [T][2K], by
 *                         fql_moe_mx4_glu_fwd's pre-pass into the workspace.
 *   split_k == 0 is exactly fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd with E = 1 and no table: the same launchers, the same
 *   choice between the decode and the tile kernel, the same bits, and the guarantee stated there at every T.
 *   split_k != 0 applies when 0 < T <= a threshold built into the library (FQL_MX4_LINEAR_DECODE_MAX_ROWS in csrc/fql_mx4.hip,
 *   set from a measurement) and S(K, N) > 1.  S, the number of slices, is a pure function of K and N, one of 1, 2, 4, 8, 16:
 *   never of T, of the device or of any state but the tuning hook.  Then the decode kernel runs once per slice of K
 *   (slice s takes the 64-k pairs [s * ceil(P / S), min(P, (s + 1) * ceil(P / S))), P = K / 64, in ascending order on an
 *   accumulator that starts at zero; the odd block of K % 64 == 32 is the last slice's) into float32 partial sums in the
 *   workspace, and a second launch on the same stream computes
 *       out[t][n] = round( (((p_0 + p_1) + p_2) + ... + p_{S-1}) + bias[n] )
 *   in float32, in that order, with one rounding.  No atomics; launches are the only synchronisation.  Every other call
 *   with split_k set takes the split_k == 0 path.
 *   THE CONTRACT with split_k set: a row's result depends on its own row, the weights, K and N.  It does not depend on T
 *   or on the row's position; it is run-to-run identical, and every T up to the threshold gives the same bits.  It is NOT
 *   the tile kernel's bit pattern (the float32 sums are associated otherwise), so a row's bits may change as T crosses the
 *   threshold; both sides are within the float32 bound of DESIGN.md section 25 of the exact product.  split_k == 0 keeps
 *   that section's guarantee at every T.
 *   Non-finite values, float16 rows, scale codes 0, 1, 254 and 255: fql_moe_mx4_fwd's rules in both forms (a slice whose
 *   part of a row is non-finite stores NaN for the whole partial row, so the sum carries the rule).
 *   Workspace: fql_linear_mx4_workspace_bytes(T, K, N, gated, split_k), 16-byte aligned: the [T][K] bfloat16 h of a gated
 *   call (fql_moe_mx4_workspace_bytes' layout), then, with split_k set and 0 < T <= the threshold, 16 * T * N float32 of
 *   partial sums (sized for the largest S whatever S(K, N) is).  0 bytes when neither applies; then workspace may be NULL.
 *   Return codes, in fql_moe_mx4_fwd's order with E = 1 and all before any HIP call: FQL_ERR_BAD_SHAPE (T < 0, K <= 0, N < 0;
 *   glu: the activation); FQL_ERR_ODD_K; FQL_ERR_BAD_SHAPE (K % 32 != 0); FQL_ERR_DTYPE; T == 0 or N == 0: FQL_OK with nothing
 *   launched; FQL_ERR_NULL_POINTER (blocks, scales_e8m0, inputs / gate_up, out); FQL_ERR_BAD_SHAPE (T > 4194240);
 *   FQL_ERR_ALIGNMENT (blocks not 16-byte aligned; inputs / gate_up / out not aligned to their element, bias not to 4
 *   bytes); FQL_ERR_WORKSPACE (a non-empty workspace NULL, misaligned or short); FQL_ERR_LAUNCH.
 *   The input gradient is fql_moe_mx4_bwd_input with E = 1 and no table.  fql_int4_tune.h: fql_tune_set_mx4_linear_decode_max_rows,
 *   fql_tune_set_mx4_linear_slices and fql_tune_mx4_linear_kernel force and report the choice (tools and tests). */
FQL_API size_t fql_linear_mx4_workspace_bytes(int T, int K, int N, int gated, int split_k);
FQL_API int fql_linear_mx4_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *inputs, int in_dtype,
                               const float *bias, void *out, int out_dtype, int T, int K, int N, int split_k, void *workspace,
                               size_t workspace_bytes, void *stream);
FQL_API int fql_linear_mx4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e8m0, const void *gate_up, int in_dtype,
                                   const float *bias, void *out, int out_dtype, int T, int K, int N, int activation,
                                   float act_alpha, float act_limit, int split_k, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* ---- NVFP4 weights, grouped and dense, forward only (FQL_VERSION 430; INTEGRATION.md section 18, DESIGN.md section 38;
 *      csrc/fql_gemm_nvfp4.h) ----
 * The format of ModelOpt's "-FP4" / "-NVFP4" exports, as it lies in the checkpoint:
 *   blocks       [E][N][K / 2] uint8: two e2m1 codes a byte, even k in the low nibble (fql_moe_mx4_fwd's layout and code table:
 *                0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6 and 8 .. 15 their negatives);
 *   scales_e4m3  [E][N][K / 16] uint8: byte b is the OCP e4m3fn value of those bits (bias 7, subnormals, largest value 448, 0x7F
 *                and 0xFF NaN, the sign bit honoured as arithmetic gives it); it scales weight row n, inputs 16 b .. 16 b + 15;
 *   global_scale [E] float32, or NULL for 1: it MULTIPLIES (ModelOpt's weight_scale_2; compressed-tensors stores the reciprocal).
 *   W_e[n][k] = e2m1(code) * e4m3(scale byte), exact in bfloat16, and
 *   out[t][n] = round_OUT( fl32( fl32(acc * global_scale[e]) + bias[e][n] ) ),   acc = sum_k bf16(x[t][k]) * W_e[n][k]
 *   with float32 accumulation on v_mfma_f32_32x32x16_bf16 in fql_moe_mx4_fwd's fixed order (k ascending, 16 a step, an
 *   accumulator that starts at zero).  The multiply comes first, then the add, two roundings, never an FMA; with neither a
 *   global scale nor a bias the result is acc.  K % 32 == 0, any N >= 1.  inputs [T][K] float32 (rounded once to bfloat16) or
 *   bfloat16; float16 rows are refused (FQL_ERR_DTYPE).
 * fql_moe_nvfp4_fwd:     the grouped GEMM.  The table contract is fql_moe_fwd_f32's: raw pairs in any order, clipped, rows no
 *                        expert covers are zero; both table pointers NULL with E == 1 is one segment of all rows.
 * fql_moe_nvfp4_glu_fwd: the same on h = bf16(act(gate_up[t][k], gate_up[t][K + k])), gate_up [T][2K], by fql_moe_mx4_glu_fwd's
 *                        pre-pass into the workspace (fql_moe_nvfp4_workspace_bytes(E, T, K, N, 1): h [T][K] bfloat16, its layout).
 * fql_linear_nvfp4_fwd / fql_linear_nvfp4_glu_fwd: one matrix blocks [N][K / 2], scales_e4m3 [N][K / 16], global_scale [1] or
 *                        NULL, bias [N], no table: exactly the grouped launchers with E = 1.  There is no split-K form.
 *                        Workspace: fql_linear_nvfp4_workspace_bytes(T, K, N, gated).
 *   Two kernels, the 64 x 128 tile and a one-wave decode kernel, return THE SAME BITS for every element; T alone chooses
 *   (T <= FQL_NVFP4_DECODE_MAX_ROWS in csrc/fql_mx4.hip; fql_int4_tune.h: fql_tune_set_nvfp4_decode_max_rows /
 *   fql_tune_nvfp4_kernel).  No atomics, every element written once; the grouped call equals E one-expert calls bit for bit.
 *   NON-FINITE: a NaN scale byte makes its 16 weights NaN, zeros included, so every output of that weight row is NaN for the
 *   rows of that expert only; a non-finite activation makes exactly its own output row NaN; global_scale is not screened.
 *   Return codes: fql_moe_mx4_fwd's, in its order (global_scale not 4-byte aligned: FQL_ERR_ALIGNMENT); the glu and the
 *   gated linear entries then FQL_ERR_WORKSPACE. */
FQL_API size_t fql_moe_nvfp4_workspace_bytes(int E, int T, int K, int N, int gated);
FQL_API int fql_moe_nvfp4_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                              int in_dtype, const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                              void *out, int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes,
                              void *stream);
FQL_API int fql_moe_nvfp4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *gate_up,
                                  int in_dtype, const float *bias, const int32_t *tokens_per_expert,
                                  const int32_t *input_offsets, void *out, int out_dtype, int E, int T, int K, int N,
                                  int activation, float act_alpha, float act_limit, void *workspace, size_t workspace_bytes,
                                  void *stream);
FQL_API size_t fql_linear_nvfp4_workspace_bytes(int T, int K, int N, int gated);
FQL_API int fql_linear_nvfp4_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                 int in_dtype, const float *bias, void *out, int out_dtype, int T, int K, int N, void *workspace,
                                 size_t workspace_bytes, void *stream);
FQL_API int fql_linear_nvfp4_glu_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                     const void *gate_up, int in_dtype, const float *bias, void *out, int out_dtype, int T, int K,
                                     int N, int activation, float act_alpha, float act_limit, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ---- the input gradient of the NVFP4 weights (FQL_VERSION 440; INTEGRATION.md section 18, DESIGN.md section 39;
 *      csrc/fql_gemm_nvfp4_bwd.h) ----
 * fql_moe_nvfp4_bwd_input: grad_in[t][k] = round_OUT( fl32(acc * global_scale[e]) ), acc = sum_n bf16(grad_out[t][n]) * W_e[n][k]
 * over the rows t of expert e, on the blocks, scales_e4m3 and global_scale of fql_moe_nvfp4_fwd as they are (W_e as there; no
 * transposed copy, no workspace).  global_scale NULL means 1, and then the result is acc's bits.
 *   grad_out [T][N] float32 (rounded once to bfloat16, to nearest even) or bfloat16; float16 is refused (FQL_ERR_DTYPE).
 *   grad_in  [T][K] of out_dtype (float32, float16 or bfloat16), rounded once.  K % 32 == 0, any N >= 1.
 *   The contraction is v_mfma_f32_32x32x16_bf16 with float32 accumulation in fixed ascending order of n, 16 a step, from zero.
 *   No atomics, every element written once; a row's result depends on its own gradient row and its expert's weights only,
 *   and the grouped call equals E one-expert calls bit for bit.  The table contract is fql_moe_nvfp4_fwd's: with a table the
 *   rows no expert covers are zeros; both table pointers NULL with E == 1 is one segment of all rows (the dense layer's
 *   input gradient: there is no separate dense entry).
 *   T == 0 launches nothing; N == 0 with T > 0 sets grad_in to zeros (one hipMemsetAsync on the stream) and reads no other
 *   operand.
 *   NON-FINITE: a non-finite element of a gradient row makes exactly that grad_in row NaN; a NaN scale byte (0x7F, 0xFF) makes
 *   grad_in NaN for exactly its 16 k on the rows of that expert; a negative scale byte negates its block's contribution;
 *   global_scale is not screened.
 *   Return codes: fql_moe_nvfp4_fwd's, in its order (N == 0 with T > 0 and a NULL grad_in: FQL_ERR_NULL_POINTER). */
FQL_API int fql_moe_nvfp4_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                    const void *grad_out, int in_dtype, const int32_t *tokens_per_expert,
                                    const int32_t *input_offsets, void *grad_in, int out_dtype, int E, int T, int K, int N,
                                    void *stream);

/* ---- low-rank adapters on the NVFP4 weights, fused into the NVFP4 tile kernels (FQL_VERSION 450; INTEGRATION.md
 *      section 18; csrc/fql_gemm_nvfp4.h, csrc/fql_gemm_nvfp4_bwd.h) ----
 * The adapter forms of fql_moe_nvfp4_fwd, fql_moe_nvfp4_glu_fwd, fql_moe_nvfp4_bwd_input and of the dense entries: the adapter
 * term is one more contraction stage of the same kernel, behind the last weight stage, as in the fql_moe_mx4_lora_* entries.
 *   forward   out[t][n] = round_OUT( fl32( S + bias[e][n] ) ),  S  = fl32(accW * g_e)  (+) sum_{j < rank} bf16(v[t][j]) bf16(B[e][n][j])
 *   backward  dX[t][k]  = round_OUT( S' ),                      S' = fl32(accW' * g_e) (+) sum_{j < rank} bf16(dv[t][j]) bf16(A[e][j][k])
 *   accW / accW' are the base entries' accumulators (the same instructions on ascending k / n, from zero), g_e = global_scale[e]
 *   (NULL: 1, no multiply), (+) is the matrix instruction accumulating onto its C operand in ascending j, 16 a step.
 *   global_scale scales the WEIGHT term only: the accumulator is multiplied by it (one float32 rounding a register, never an
 *   FMA) behind the last weight stage and in front of the adapter stage; the epilogue then adds the bias and rounds.
 *   With lora_B (lora_A) all zeros and finite lora_rows the result equals the base entry's for any global_scale and bias (the
 *   only possible difference is the sign of a zero when g_e < 0: the adapter stage adds +0 to a -0).
 * fql_moe_nvfp4_glu_lora_fwd: the same on h = bf16(act(gate_up)) (fql_moe_nvfp4_glu_fwd's pre-pass and workspace, unchanged).
 * fql_linear_nvfp4_lora_fwd / fql_linear_nvfp4_lora_bwd_input: one matrix, global_scale [1] or NULL, no table: exactly the grouped
 *   launchers with E = 1.
 *   lora_rows [T][rank] float32, lora_B [E][N][rank], lora_A [E][rank][K] float32, rank one of 4, 8, 16, 32, 64: as
 *   fql_moe_mx4_lora_fwd's, with its rounding, order, non-finite rule (a non-finite element of a row of lora_rows makes
 *   exactly that row of the result NaN; the adapter matrices and global_scale are not screened) and alignment (4 bytes).
 *   A NaN scale byte gives what it gives in the base entries: the adapter stage overwrites the LDS images in full.
 *   These entries always run the 64-row tile kernels (no decode form: they are for training).  The grouped call equals E
 *   one-expert calls bit for bit; a row's result depends on its own rows of x and v and its expert's W, B and g only.
 *   Return codes: the base entry's, in its order, with the adapter checks of fql_moe_mx4_lora_fwd in their places
 *   (FQL_ERR_BAD_SHAPE for the rank behind the dtype check, FQL_ERR_NULL_POINTER, FQL_ERR_ALIGNMENT), all before any HIP call.
 *   The two input gradients with N == 0 and T > 0 are FQL_ERR_BAD_SHAPE. */
FQL_API int fql_moe_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                   int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                   const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E,
                                   int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_nvfp4_glu_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                       const void *gate_up, int in_dtype, const float *lora_rows, const float *lora_B, int rank,
                                       const float *bias, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                                       void *out, int out_dtype, int E, int T, int K, int N, int activation, float act_alpha,
                                       float act_limit, void *workspace, size_t workspace_bytes, void *stream);
FQL_API int fql_moe_nvfp4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                         const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A, int rank,
                                         const int32_t *tokens_per_expert, const int32_t *input_offsets, void *grad_in,
                                         int out_dtype, int E, int T, int K, int N, void *stream);
FQL_API int fql_linear_nvfp4_lora_fwd(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale, const void *inputs,
                                      int in_dtype, const float *lora_rows, const float *lora_B, int rank, const float *bias,
                                      void *out, int out_dtype, int T, int K, int N, void *workspace, size_t workspace_bytes,
                                      void *stream);
FQL_API int fql_linear_nvfp4_lora_bwd_input(const uint8_t *blocks, const uint8_t *scales_e4m3, const float *global_scale,
                                            const void *grad_out, int in_dtype, const float *lora_rows, const float *lora_A,
                                            int rank, void *grad_in, int out_dtype, int T, int K, int N, void *stream);

FQL_API int fql_regroup_index_i32(const int32_t *recv_counts, int G, int EL, int32_t *tokens_per_expert,
                                  int32_t *input_offsets, int32_t *gather, int32_t *scatter, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FQL_INT4_H */
