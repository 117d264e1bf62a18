// Launch boundary between fql_int4.hip (the dispatcher) and fql_glu.hip, which holds the gated activation pre-pass for the
// activation kinds other than silu: act_glu_kernel<L, VEC, IN> of fql_act_quant.h for IN = F32 / F16 / BF16.  The
// instantiations live in a translation unit of their own so that fql_int4.o's device code is what it was.
#pragma once
#include "fql_ffn16_launch.h"

// L = 1, 2, 3 limbs; variant 0: one row per workgroup, 1: ACT_ROWS rows per workgroup (both: K % 16 == 0 and a 16-byte
// aligned base), 2: element loads; in_dtype FQL_DTYPE_*; a.x is [T][2K] gate|up of that type.  activation: FQL_ACT_GELU_TANH
// or FQL_ACT_SWIGLU_CLAMP (checked by the caller).  Returns 0, or -1 when the launch failed or the combination does not exist.
int fql_act_glu_launch(int L, int variant, int in_dtype, const FqlActGatedArgs &a, int activation, float act_alpha,
                       float act_limit);
