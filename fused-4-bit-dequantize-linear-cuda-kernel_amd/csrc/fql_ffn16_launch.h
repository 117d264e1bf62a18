// Launch boundary between fql_int4.hip (the dispatcher) and fql_ffn16.hip, which holds the gated activation pre-pass for a
// float16 / bfloat16 gate|up tensor: act_fused_kernel<L, VEC, IN, GATE = true> of fql_act_quant.h for IN = F16 / BF16.
// The instantiations live in a translation unit of their own so that fql_int4.o's device code is what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct FqlActGatedArgs {
    const void *x;                     // [T][2K] gate|up, 16-bit elements
    float *delta;
    int32_t *rowsum;
    int8_t *limbs;
    int T, K, KB, MBT, rblocks, zblocks;
    void *out;                         // rows no expert covers are zeroed here (NULL: no table)
    int out_es, N;
    const int32_t *tpe, *offs;
    int E;
    const float *row_weight;
    hipStream_t stream;
};

// L = 1, 2, 3 limbs; variant 0: one row per workgroup, 1: ACT_ROWS rows per workgroup (both: K % 16 == 0 and a 16-byte
// aligned base), 2: element loads; in_dtype FQL_DTYPE_F16 / _BF16.  Returns 0, or -1 when the launch failed or the
// combination does not exist.
int fql_act_gated16_launch(int L, int variant, int in_dtype, const FqlActGatedArgs &a);
