// libfql_int4.so, eighth translation unit: the gradient of the per-expert biases of the grouped GEMM (include/fql_int4.h,
// fql_moe_bias_grad),
//
//   grad_bias[e][n] = sum over the rows t of expert e of grad_rows[t][n]        [T][N] -> [E][N] float32.
//
// A streaming reduction of T * N elements, shaped after lora_grad_kernel (fql_lora.h): grid = (column strips, E), the
// workgroup's row slots take the expert's rows round-robin, the partial sums meet in a fixed tree.  No atomics, no
// workspace, float32 accumulation; a 16-bit element is widened in registers on load (exact).
//
// Strip width.  A lane loads 16 bytes (VEC = 4 float32 or 8 16-bit elements; VEC = 1 on the element path), and a row
// segment is LPR = 16 lanes = 256 bytes, two whole cache lines, so one wave-instruction covers 4 rows and the workgroup's
// 8 waves 32 rows: SLOTS = 32 row slots.  A strip is 64 float32 / 128 16-bit columns.  A full-wave strip (256 / 512 columns)
// would leave N = 4096 with 16 strips per expert: under skewed routing the expert that owns half the rows would be
// streamed by 16 workgroups.  The narrow strip gives it 64, and every load is still 16 bytes per lane and whole lines.
// 4 rows are in flight per lane (U): 32 KiB per workgroup, and at < 48 registers four workgroups share a CU.
//
// Summation order.  Row lo_e + r of expert e belongs to slot r % 32.  A slot adds its rows in ascending order, starting from
// 0.0f; the four slots of a wave meet as (s0 + s2) + (s1 + s3) (two lane exchanges), then the 8 waves in the tree of
// lora_grad_kernel through LDS.  The order is a function of the expert's row count alone: not of the grid, E, the offsets,
// other experts, the element type or the load width -- run-to-run identical, unchanged when the table is permuted, and
// the vector and the element path return the same bits.
// Experts without rows (and T == 0) write zeros.  Host-side launches only: no allocation, no synchronisation.
#include "fql_host.h"
#include "fql_lora.h"
#include "fql_bias_launch.h"

#define FQL_BIAS_GRAD_THREADS 512
#define FQL_BIAS_GRAD_LPR 16           // lanes per row segment

namespace {

using namespace fql_host;

// VEC elements of type DT at element index i of `base` -> float32.  VEC > 1: one 16-byte load.
template <int VEC, int DT>
__device__ __forceinline__ void load_row(const void *base, size_t i, float (&v)[VEC])
{
    if constexpr (DT == FQL_DTYPE_F32) {
        static_assert(VEC == 4 || VEC == 1, "float32: 16 bytes or one element");
        lora::load_vec<VEC>(reinterpret_cast<const float *>(base) + i, v);
    } else {
        static_assert(VEC == 8 || VEC == 1, "16-bit: 16 bytes or one element");
        const unsigned short *p = reinterpret_cast<const unsigned short *>(base) + i;
        if constexpr (VEC == 8) {
            const uint4 t = *reinterpret_cast<const uint4 *>(p);
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = lora::widen16<DT>((unsigned short)(w[k] & 0xFFFFu));
                v[2 * k + 1] = lora::widen16<DT>((unsigned short)(w[k] >> 16));
            }
        } else v[0] = lora::widen16<DT>(*p);
    }
}

template <int VEC, int DT>
__global__ __launch_bounds__(FQL_BIAS_GRAD_THREADS) void moe_bias_grad_kernel(
    const void *__restrict__ G, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
    float *__restrict__ out, int T, int N)
{
    constexpr int LPR = FQL_BIAS_GRAD_LPR;
    constexpr int NW = FQL_BIAS_GRAD_THREADS / FQL_WAVE;
    constexpr int SLOTS = NW * (FQL_WAVE / LPR);                 // rows per workgroup step
    constexpr int U = 4;                                         // rows in flight per lane
    __shared__ float red[NW / 2][VEC][FQL_WAVE];

    const int e = blockIdx.y;
    int lo = 0, hi = T;
    if (tpe != nullptr) lora::expert_rows(tpe, offs, e, T, lo, hi);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / FQL_WAVE);
    const int lane = threadIdx.x & (FQL_WAVE - 1);
    const int grp = lane / LPR;
    const int c = ((int)blockIdx.x * LPR + lane % LPR) * VEC;
    const bool live = c < N;
    const size_t cc = live ? c : 0;                              // dead lanes read column 0 and never store

    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    long long t = (long long)lo + wave * (FQL_WAVE / LPR) + grp; // (64-bit: T may sit next to INT_MAX)
    for (; t + (U - 1) * SLOTS < hi; t += U * SLOTS) {
        float g[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) load_row<VEC, DT>(G, (size_t)(t + u * SLOTS) * N + cc, g[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += g[u][i];
    }
    for (; t < hi; t += SLOTS) {
        float g[VEC];
        load_row<VEC, DT>(G, (size_t)t * N + cc, g);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += g[i];
    }
    // the four slots of a wave: (s0 + s2) + (s1 + s3), the same bits in each of the four lanes that hold a column
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        acc[i] += __shfl_xor(acc[i], 2 * LPR);
        acc[i] += __shfl_xor(acc[i], LPR);
    }
    // fixed tree: at width h, waves [h, 2h) hand their partials to waves [0, h)
#pragma unroll
    for (int h = NW / 2; h >= 1; h >>= 1) {
        if (wave >= h && wave < 2 * h) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) red[wave - h][i][lane] = acc[i];
        }
        __syncthreads();
        if (wave < h) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += red[wave][i][lane];
        }
        __syncthreads();
    }
    if (wave != 0 || grp != 0 || !live) return;
    float *oe = out + (size_t)e * N + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) oe[i] = acc[i];                // (VEC > 1: N % VEC == 0, the lane's columns all exist)
}

template <int VEC, int DT>
int bias_grad_launch(const void *g, const int32_t *tpe, const int32_t *offs, float *out, int E, int T, int N, hipStream_t st)
{
    const int cols = FQL_BIAS_GRAD_LPR * VEC;
    return launch(moe_bias_grad_kernel<VEC, DT>, dim3((unsigned)(((long long)N + cols - 1) / cols), E),
                  dim3(FQL_BIAS_GRAD_THREADS), 0, st, g, tpe, offs, out, T, N);
}

}  // namespace

int fql_bias_grad_launch(const void *grad_rows, int dtype, const int32_t *tpe, const int32_t *offs, float *grad_bias, int E,
                         int T, int N, hipStream_t stream)
{
    // 16-byte loads: every row starts on a 16-byte boundary (the base does, and the row pitch is a multiple of 16 bytes)
    const bool vec = aligned16(grad_rows) && ((long long)N * dtype_bytes(dtype)) % 16 == 0;
    int rc;
    if (dtype == FQL_DTYPE_F32)
        rc = vec ? bias_grad_launch<4, FQL_DTYPE_F32>(grad_rows, tpe, offs, grad_bias, E, T, N, stream)
                 : bias_grad_launch<1, FQL_DTYPE_F32>(grad_rows, tpe, offs, grad_bias, E, T, N, stream);
    else if (dtype == FQL_DTYPE_F16)
        rc = vec ? bias_grad_launch<8, FQL_DTYPE_F16>(grad_rows, tpe, offs, grad_bias, E, T, N, stream)
                 : bias_grad_launch<1, FQL_DTYPE_F16>(grad_rows, tpe, offs, grad_bias, E, T, N, stream);
    else if (dtype == FQL_DTYPE_BF16)
        rc = vec ? bias_grad_launch<8, FQL_DTYPE_BF16>(grad_rows, tpe, offs, grad_bias, E, T, N, stream)
                 : bias_grad_launch<1, FQL_DTYPE_BF16>(grad_rows, tpe, offs, grad_bias, E, T, N, stream);
    else return -1;
    return rc == FQL_OK ? 0 : -1;
}
