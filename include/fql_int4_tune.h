/* libfql_int4 -- tuning and diagnostic hooks.  NOT part of the drop-in boundary (include/fql_int4.h): nothing in the
 * product path calls them.  They exist for tools/ (A/B timing in one process), tests/ (every tile configuration must
 * return the same bits) and bench.py (labels its roofline with the kernel family the library picked).
 *
 * The setters change PROCESS-GLOBAL dispatch thresholds of the library: they are not thread-safe, and a process that calls
 * one no longer has the "no state between calls" property fql_int4.h promises -- use them from single-threaded tools only,
 * and restore the returned previous value.  The getters and fql_tune_gemm_i8_f32 / fql_tune_gemm_i8 keep no state.
 */
#ifndef FQL_INT4_TUNE_H
#define FQL_INT4_TUNE_H

#include "fql_int4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fql_gemm_i8_f32 with an explicit tile configuration id: 0.. wide 8-wave tiles, 100.. 32-row tiles, 200.. / 220.. 16-row
 * tiles, 300.. the one-wave-per-SIMD kernel.  FQL_ERR_BAD_SHAPE for an id that does not exist for the precision. */
FQL_API int fql_tune_gemm_i8_f32(int cfg, const int8_t *limbs, const float *delta, const int32_t *rowsum,
                                 const uint8_t *packed, const float *scales, const float *zps,
                                 const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                 int T, int K, int N, int precision, void *stream, void *scratch, size_t scratch_bytes);
/* fql_tune_gemm_i8_f32 with the rest of the epilogue: outputs of element type `out_dtype` (FQL_DTYPE_*), an optional
 * `bias` [E][N] (one vector per expert, as the scales) and an optional `row_weight` [T], in that order:
 * out = dtype(fl32(fl32(acc + bias) * row_weight)), one rounding per step.
 * The kernels take the bias as a pointer but read a row's weight from the [T] plane behind delta's set(s),
 * where the pre-pass of fql_moe_gather_scaled_fwd_f32 leaves it: a non-NULL `row_weight` must be that plane, i.e.
 * delta + sets * T (sets = 2 for 2 / 3 limbs, else 1), or the call returns FQL_ERR_ALIGNMENT.  Uncovered rows of a
 * grouped problem are left as they are. */
FQL_API int fql_tune_gemm_i8(int cfg, const int8_t *limbs, const float *delta, const int32_t *rowsum,
                             const uint8_t *packed, const float *scales, const float *zps,
                             const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                             const float *bias, const float *row_weight, int E, int T, int K, int N, int precision,
                             void *stream, void *scratch, size_t scratch_bytes);
/* the id the product path picks for a shape (grouped: rows are spread over E experts) */
FQL_API int fql_tune_chosen_cfg(int precision, int E, int T, int K, int N, int grouped);
FQL_API int fql_tune_num_configs(void);                 /* wide ids run 0 .. this - 1; not every id is built for every precision: */
FQL_API int fql_tune_is_config(int cfg, int precision);  /* 1 when fql_tune_gemm_i8_f32 accepts the id for the precision */
FQL_API int fql_tune_num_rows32_configs(void);
FQL_API int fql_tune_num_rows16_configs(void);
FQL_API int fql_tune_num_w4_configs(void);

/* process-global switches; each returns the previous value */
FQL_API int fql_tune_set_compute_units(int n);          /* persistent grids sized for n compute units (multiple of 8; 0: the device's); tests use it to walk many tiles per workgroup on small shapes */
FQL_API int fql_tune_set_fused(int on);                  /* 3 limbs, float32 rows, one-wave-per-SIMD kernel: pre-pass as the GEMM kernel's first phase (ONE launch) */
FQL_API int fql_tune_set_fused_spin(int polls);          /* polls before a workgroup of that launch quantises the rows it waits for itself (0: at once -- tests) */
FQL_API int fql_tune_set_w4(int on);                     /* 3 limbs, > 64 rows per group: one-wave-per-SIMD kernel (default on) */
FQL_API int fql_tune_set_balance_tiles(int on);          /* uneven column tiles that even out the persistent walk (default on) */
FQL_API int fql_tune_set_gemv_max_rows(int rows);        /* linear op: rows up to which the float32 GEMV kernel runs (default 2) */
FQL_API int fql_tune_set_act_single_rows(int rows);      /* pre-pass: one row per workgroup up to this many padded rows (512) */
FQL_API int fql_tune_set_group_mfma(int on);             /* per-group scales: float32 matrix-core kernel for batches */
FQL_API int fql_tune_set_group_i8(int on);               /* per-group scales: INT8 matrix-core kernel where eligible */
FQL_API int fql_tune_set_group_i8_min_rows(int rows);    /* ... from this many rows per group on */
FQL_API int fql_tune_set_mx4_decode_max_rows(int rows);  /* MXFP4 bfloat16 forward: rows (T) up to which the decode kernel runs; 0: always the tile kernel, INT_MAX: the decode kernel wherever its grid allows, a negative value changes nothing (same bits either way: fql_int4.h, FQL_VERSION 380) */

/* 0: fql_moe_mx4_fwd / fql_moe_mx4_glu_fwd would run the 64 x 128 tile kernel on this shape now, 1: the decode kernel.  Keeps no state. */
FQL_API int fql_tune_mx4_kernel(int E, int T, int K, int N);

/* The same pair for the block-scaled precisions (fql_int4.h, FQL_VERSION 390).  mode: 1 the fp8-row entries (fql_moe_mx4_fwd_f8 /
 * _fwd_q8 / _glu_fwd_q8), 2 the MXFP4-row ones (_fwd_f4 / _fwd_q4 / _glu_fwd_q4); each mode has a threshold of its own, and neither
 * moves with fql_tune_set_mx4_decode_max_rows.  The setter returns the mode's previous value (a negative `rows` changes nothing);
 * an unknown mode changes nothing and returns -1 from both. */
FQL_API int fql_tune_set_mx4_scaled_decode_max_rows(int mode, int rows);
/* 0: the mode's entries would run the 64 x 128 tile kernel on this shape now, 1: the decode kernel.  Keeps no state. */
FQL_API int fql_tune_mx4_scaled_kernel(int mode, int E, int T, int K, int N);

/* The pair of the MXFP6-row entries (fql_moe_mx4_fwd_f6 / _fwd_q6 / _glu_fwd_q6; fql_int4.h, FQL_VERSION 400), with a threshold of
 * its own.  (Mode 3 of the pair above stays an unknown mode.)  The setter returns the previous value; a negative `rows` changes nothing. */
FQL_API int fql_tune_set_mx4_f6_decode_max_rows(int rows);
/* 0: those entries would run the 64 x 128 tile kernel on this shape now, 1: the decode kernel.  Keeps no state. */
FQL_API int fql_tune_mx4_f6_kernel(int E, int T, int K, int N);

/* The dense MXFP4 linear entries (fql_linear_mx4_fwd / fql_linear_mx4_glu_fwd; fql_int4.h, FQL_VERSION 420) with split_k set.
 * fql_tune_set_mx4_linear_decode_max_rows: rows (T) up to which the split form runs; 0 never; returns the previous value, a
 * negative `rows` changes nothing.  fql_linear_mx4_workspace_bytes follows it. */
FQL_API int fql_tune_set_mx4_linear_decode_max_rows(int rows);
/* The slices S of the split form: 0 the library's policy S(K, N), or one of 1 / 2 / 4 / 8 / 16 to force S for every shape
 * (1: no split form).  Any other value changes nothing.  Returns the previous value. */
FQL_API int fql_tune_set_mx4_linear_slices(int slices);
/* What a call with split_k set would run on this shape now: (S << 8) | form, form 0 the 64 x 128 tile kernel, 1 the grouped
 * decode kernel (both with S = 1: the split_k == 0 path), 2 the split form with S slices.  Keeps no state. */
FQL_API int fql_tune_mx4_linear_kernel(int T, int K, int N);

/* The pair of the NVFP4 entries (fql_moe_nvfp4_fwd / _glu_fwd and fql_linear_nvfp4_fwd / _glu_fwd; fql_int4.h, FQL_VERSION 430),
 * with a threshold of its own: rows (T) up to which the decode kernel runs; 0: always the tile kernel, INT_MAX: the decode
 * kernel wherever its grid allows.  Returns the previous value; a negative `rows` changes nothing.  Same bits either way. */
FQL_API int fql_tune_set_nvfp4_decode_max_rows(int rows);
/* 0: those entries would run the 64 x 128 tile kernel on this shape now, 1: the decode kernel.  Keeps no state. */
FQL_API int fql_tune_nvfp4_kernel(int E, int T, int K, int N);

#ifdef __cplusplus
}
#endif
#endif
