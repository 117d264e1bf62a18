// Launch boundary between fql_int4.hip (the dispatcher) and fql_bias.hip, which holds the per-expert bias gradient
// moe_bias_grad_kernel<VEC, DT>.  The instantiations live in a translation unit of their own so that fql_int4.o's
// device code is what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// grad_bias[e][n] = sum over the rows t of expert e of grad_rows[t][n]: grad_rows [T][N] of `dtype` (FQL_DTYPE_*, aligned to
// its element), grad_bias [E][N] float32, every element written.  tpe / offs: the expert table on the device, or both NULL
// for one segment of all rows (E == 1).  1 <= E <= 65535, T >= 0, N >= 1 (checked by the caller).  16-byte loads when the
// base and the row pitch allow them, element loads otherwise.  Returns 0, or -1 when the launch failed.
int fql_bias_grad_launch(const void *grad_rows, int dtype, const int32_t *tpe, const int32_t *offs, float *grad_bias, int E,
                         int T, int N, hipStream_t stream);
