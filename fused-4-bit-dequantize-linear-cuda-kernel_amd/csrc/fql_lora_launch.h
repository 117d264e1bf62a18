// Host-side pieces shared by the two translation units of the adapter entry points (fql_lora.hip: float32;
// fql_lora16.hip: typed [T][C] operands): argument checks in the documented order and the launch geometry.
#pragma once
#include "../../include/fql_int4.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_lora.h"

namespace lora_host {

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

using fql_host::valid_dtype;
inline uintptr_t elem_bytes(int d) { return d == FQL_DTYPE_F32 ? 4 : 2; }

// Widest vector, in ELEMENTS, every row of the [T][C] operands allows: 4 when C % 4 == 0 and each base is aligned to 4
// of its own elements (16 bytes float32, 8 bytes 16-bit), then 2, then 1.
inline int vec_width(int C, const void *a, int a_dtype, const void *b, int b_dtype)
{
    for (int v = 4; v > 1; v >>= 1)
        if (C % v == 0 && aligned(a, v * elem_bytes(a_dtype)) && aligned(b, v * elem_bytes(b_dtype))) return v;
    return 1;
}

// Checks shared by the entry points, in the documented order (all before any HIP call).  `gated`: the streamed operand
// is [T][2C], so 2 T C joins the size check.
inline int shape_check(int E, int T, int C, int r, int layout, bool gated = false)
{
    if (!rank_ok(r)) return FQL_ERR_BAD_SHAPE;
    if (layout != FQL_LORA_RC && layout != FQL_LORA_CR) return FQL_ERR_BAD_SHAPE;
    if (E < 0 || T < 0 || C < 0 || E > 65535) return FQL_ERR_BAD_SHAPE;
    const long long lim = (long long)1 << 31;
    if ((long long)T * C >= lim || (long long)E * C * r >= lim || (long long)T * r >= lim) return FQL_ERR_BAD_SHAPE;
    if (gated && 2LL * T * C >= lim) return FQL_ERR_BAD_SHAPE;
    return FQL_OK;
}

inline int table_check(const int32_t *tpe, const int32_t *offs, int E)
{
    if ((tpe == nullptr) != (offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (tpe == nullptr && E != 1) return FQL_ERR_NULL_POINTER;
    return FQL_OK;
}

using fql_host::launched;

inline int tile_slots(int T, int E, int TM, bool table) { return (T + TM - 1) / TM + (table ? E : 0); }
inline int cover_blocks(int T, bool table) { return table ? (T + FQL_LORA_COVER_ROWS - 1) / FQL_LORA_COVER_ROWS : 0; }

// Launchers: one instantiation per (rank, layout, vector width, element type(s)).
template <int R, bool CR, bool GATE = false, int DT = 0>
int shrink_r(const void *in, const float *w, const int32_t *tpe, const int32_t *offs, float *out, int E, int T, int C,
             float scale, int vec, hipStream_t st)
{
    const int slots = tile_slots(T, E, 64 / R, tpe != nullptr);
    const dim3 grid(slots + cover_blocks(T, tpe != nullptr));
    auto k = vec == 4 ? lora::lora_shrink_kernel<R, CR, 4, GATE, DT>
                      : (vec == 2 ? lora::lora_shrink_kernel<R, CR, 2, GATE, DT> : lora::lora_shrink_kernel<R, CR, 1, GATE, DT>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_SHRINK_THREADS), 0, st, in, w, tpe, offs, out, E, T, C, scale, slots);
    return launched();
}

template <int R, bool CR, int DI = 0, int DO = 0>
int expand_r(const float *v, const float *w, const int32_t *tpe, const int32_t *offs, const void *in, void *out, int E,
             int T, int C, float scale, int vec, hipStream_t st)
{
    const int slots = tile_slots(T, E, FQL_LORA_EXPAND_ROWS, tpe != nullptr);
    const int cols = FQL_LORA_EXPAND_THREADS * vec;
    const dim3 grid(slots + cover_blocks(T, tpe != nullptr), (C + cols - 1) / cols);
    auto k = vec == 4 ? lora::lora_expand_kernel<R, CR, 4, DI, DO>
                      : (vec == 2 ? lora::lora_expand_kernel<R, CR, 2, DI, DO> : lora::lora_expand_kernel<R, CR, 1, DI, DO>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_EXPAND_THREADS), 0, st, v, w, tpe, offs, in, out, E, T, C, scale, slots);
    return launched();
}

template <int R, bool CR, bool GATE = false, int DT = 0>
int grad_r(const void *p, const float *v, const int32_t *tpe, const int32_t *offs, float *d, int E, int T, int C,
           float scale, int vec, hipStream_t st)
{
    constexpr int JG = R < 16 ? 1 : R / 16;
    const int cols = FQL_WAVE / JG * vec;
    const dim3 grid((C + cols - 1) / cols, E);
    auto k = vec == 4 ? lora::lora_grad_kernel<R, CR, 4, GATE, DT>
                      : (vec == 2 ? lora::lora_grad_kernel<R, CR, 2, GATE, DT> : lora::lora_grad_kernel<R, CR, 1, GATE, DT>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, grid, dim3(FQL_LORA_GRAD_THREADS), 0, st, p, v, tpe, offs, d, T, C, scale);
    return launched();
}

}  // namespace lora_host

// rank x layout dispatch
#define FQL_LORA_DISPATCH(FN, CR, ...)                                                                                  \
    switch (r) {                                                                                                        \
    case 4: return CR ? FN<4, true>(__VA_ARGS__) : FN<4, false>(__VA_ARGS__);                                           \
    case 8: return CR ? FN<8, true>(__VA_ARGS__) : FN<8, false>(__VA_ARGS__);                                           \
    case 16: return CR ? FN<16, true>(__VA_ARGS__) : FN<16, false>(__VA_ARGS__);                                        \
    case 32: return CR ? FN<32, true>(__VA_ARGS__) : FN<32, false>(__VA_ARGS__);                                        \
    default: return CR ? FN<64, true>(__VA_ARGS__) : FN<64, false>(__VA_ARGS__);                                        \
    }
