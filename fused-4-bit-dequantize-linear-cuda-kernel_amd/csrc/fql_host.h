// Host-side helpers shared by every translation unit of libfql_int4.so: alignment and padding arithmetic, the
// precision -> limbs map, element types, the per-device compute-unit count and the "launch, then report" helper.
// Host code only (no kernel lives here); each unit takes the names with `using namespace fql_host`.
#pragma once
#include "../../include/fql_int4.h"
#include "fql_common.h"
#include <utility>

namespace fql_host {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
inline int padded(int n) { return (n + FQL_KB - 1) / FQL_KB * FQL_KB; }
// 32-row blocks of the limb workspace: every expert starts on a block boundary (<= 31 pad rows each) and a
// tile may run up to 128 rows past the last expert.
inline long long row_blocks(int T, int E) { return ((long long)T + (long long)FQL_MB * E + 128 + FQL_MB - 1) / FQL_MB; }

// Limbs of a precision: 3 (default / exact), 2 (fast), 1 (int8, and fp8: one byte plane of e4m3 values forward; the
// gradient of an fp8 layer is a 1-limb integer plane)
inline int limbs_of(int precision)
{
    if (precision == FQL_PRECISION_DEFAULT) return 3;
    if (precision == FQL_PRECISION_INT8 || precision == FQL_PRECISION_FAST || precision == FQL_PRECISION_EXACT)
        return precision;
    if (precision == FQL_PRECISION_FP8) return 1;
    return -1;
}
// f(std::integral_constant<int, L>) for the limb count L of a call (1, 2 or 3: limbs_of() has been checked)
template <class F>
inline int with_limbs(int L, F &&f)
{
    if (L == 1) return f(std::integral_constant<int, 1>{});
    if (L == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

inline bool valid_dtype(int dt) { return dt == FQL_DTYPE_F32 || dt == FQL_DTYPE_F16 || dt == FQL_DTYPE_BF16; }
inline int dtype_bytes(int dt) { return dt == FQL_DTYPE_F32 ? 4 : 2; }

// Per-device caches (a process may drive several GPUs): indexed by the current device, idempotent -- a race only repeats
// the same query / attribute call.
constexpr int FQL_MAX_DEVICES = 64;
inline int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev < FQL_MAX_DEVICES ? dev : FQL_MAX_DEVICES - 1;
}
// Compute units of the current device, rounded down to a multiple of 8 (keeps vb % 8 == blockIdx % 8: XCD grouping)
inline int device_compute_units()
{
    static int cached[FQL_MAX_DEVICES] = {};
    const int dev = current_device();
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;                                         // MI355X
        n -= n % 8;
        cached[dev] = n > 0 ? n : 8;
    }
    return cached[dev];
}

// After a launch: did it take?  (The caller has cleared the error state before the launch, see launch().)
inline int launched() { return hipGetLastError() == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH; }
// Launch, then report.  The clear comes first: a stale error of another library must not read as ours.
template <class... P, class... A>
inline int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...args)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, grid, block, lds, st, static_cast<P>(std::forward<A>(args))...);
    return launched();
}

}  // namespace fql_host
