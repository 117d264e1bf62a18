// libfql_int4.so -- C ABI (include/fql_int4.h) over the gfx950 kernels.
//
// Host-side dispatch only: argument validation, kernel selection, launches on the caller's
// stream.  No allocation, no synchronisation, no state.
#include "../../include/fql_int4.h"
#include "../../include/fql_int4_tune.h"
#include "fql_common.h"
#include "fql_host.h"
#include "fql_act_quant.h"
#include "fql_act_f8.h"
#include "fql_gemm_i8.h"
#include "fql_gemm_rows32.h"
#include "fql_gemm_rows16.h"
#include "fql_gemv.h"
#include "fql_group.h"
#include "fql_group_i8.h"
#include "fql_generic.h"
#include "fql_quantize.h"
#include "fql_routing.h"
#include "fql_router.h"
#include "fql_w4_launch.h"
#include "fql_ffn16_launch.h"
#include "fql_glu_launch.h"
#include "fql_bias_launch.h"
#include <atomic>
#include <random>

namespace {
using namespace fql_host;

// Batches up to this many rows take the float32 GEMV kernel, larger ones the MFMA path (measured on MI355X, 4096 -> 11008,
// product call in a hipGraph: GEMV 9.3 / 12.1 / 19.7 us at B = 1 / 2 / 3, MFMA path 16.4 / 16.5 / 16.1 us at
// B = 2 / 3 / 4 and 16.2-16.5 us at B = 5..16: profiles/r02_linear_batch_sweep.txt).  Tuning hook below.
int g_gemv_max_rows = 2;
int g_group_i8 = 1;                    // per-group scales: the INT8 matrix-core kernel where eligible (A/B hook below)
int g_group_i8_min_rows = 40;          // ... from this many rows on for one matrix (below: the float32 matrix-core kernel; measured
int g_group_i8_min_rows_grouped = 8;   //     crossover 32..48), and from 8 rows per expert on for grouped calls (190 vs 230 us at 8 x 8 rows)
int g_group_mfma = 1;                  // per-group scales: the float32 matrix-core kernel for batches (A/B hook below)
int g_use_w4 = 1;                      // 3 limbs, > 64 rows per group: the one-wave-per-SIMD kernel (fql_gemm_w4.h) instead of the 8-wave 128 x 192 one (A/B hook below)
int g_act_single_rows = 512;          // pre-pass: one row per workgroup up to this many padded rows (tuning hook below)

inline bool is_f8(int precision) { return precision == FQL_PRECISION_FP8; }

struct PerDeviceFlag {
    bool set[FQL_MAX_DEVICES] = {};
};
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device
inline bool ensure_lds_attr(PerDeviceFlag &flag, const void *kern, int bytes)
{
    const int dev = current_device();
    if (!flag.set[dev]) {
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
        flag.set[dev] = true;
    }
    return true;
}
int g_cu_cap = 0;              // tuning hook (tests): pretend the device has this many compute units (multiple of 8; 0 = real count)
inline int compute_units() { return g_cu_cap > 0 ? g_cu_cap : device_compute_units(); }

inline int compute_units_hint() { const int n = compute_units(); return n < 256 ? 256 : n; }

struct Workspace {            // (every member has a default: a hand-filled Workspace must not carry garbage pointers into a launch)
    int8_t *limbs = nullptr;
    float *delta = nullptr;
    int32_t *rowsum = nullptr;
    float *scratch = nullptr;          // workgroup-private float32 partials of the residual pass (heavy-tailed rows), or nullptr
    unsigned long long *flags = nullptr;   // one-launch form (fql_gemm_w4.h, FUSED): one word per group of 4 grouped rows
    size_t bytes = 0;
};

// Modes with a residual limb set for heavy-tailed rows (csrc/fql_act_quant.h pass 3, csrc/fql_gemm_i8.h): 2 and 3 limbs.
inline bool has_residual(int L, bool f8) { return L >= 2 && !f8; }
// Upper bound of the residual-pass scratch over every tile configuration: workgroups x tile floats
// (8 waves x <= 4 fragments x 4 KiB per workgroup and CU; the small skinny-tile workgroups share a CU's budget).
inline size_t res_scratch_bytes() { return (size_t)compute_units_hint() * 8 * 4 * 4096; }

inline size_t limb_bytes(int L, int T, int E, int Kp) { return (size_t)L * (Kp / FQL_KB) * (size_t)row_blocks(T, E) * 8192; }

inline Workspace carve(void *base, int L, int T, int E, int Kp, bool res)
{
    Workspace w;
    const int sets = res ? 2 : 1;
    const size_t lb = round16(sets * limb_bytes(L, T, E, Kp));
    const size_t db = round16((size_t)(sets + 1) * T * sizeof(float));       // + the row-weight plane (fql_moe_gather_scaled_fwd_f32)
    const size_t rb = round16((size_t)sets * L * T * sizeof(int32_t));
    const size_t fb = (L == 3 && res) ? round16(((size_t)T + 3) / 4 * sizeof(unsigned long long)) : 0;   // row-group flags of the one-launch form
    char *p = static_cast<char *>(base);
    w.limbs = reinterpret_cast<int8_t *>(p);
    w.delta = reinterpret_cast<float *>(p + lb);
    w.rowsum = reinterpret_cast<int32_t *>(p + lb + db);
    w.flags = fb ? reinterpret_cast<unsigned long long *>(p + lb + db + rb) : nullptr;
    w.scratch = res ? reinterpret_cast<float *>(p + lb + db + rb + fb) : nullptr;
    w.bytes = lb + db + rb + fb + (res ? res_scratch_bytes() : 0);
    return w;
}

// One op on the matrix-core path: what the pre-pass reads, what the GEMM reads and writes, and the workspace between them.
// An entry point fills it once; every launcher takes it by const reference.
struct Call {
    const void *x = nullptr;               // activation rows [n_src or T][K] ([T][2K] gate|up when gated), or the GEMM alone (NULL)
    int in_dtype = FQL_DTYPE_F32;
    const int32_t *gather = nullptr;       // optional: grouped row t is row gather[t] of x
    int n_src = 0;
    bool gated = false;                    // the pre-pass applies silu(gate) * up
    int act = FQL_ACT_SILU;                // ... or (gated) another kind of FQL_ACT_*, with its two floats
    float act_alpha = 0.0f, act_limit = 0.0f;
    bool f8 = false;                       // the pre-pass writes one e4m3 plane, the GEMM is the fp8 form
    const uint8_t *packed = nullptr;
    const float *scales = nullptr;
    const float *zps = nullptr;
    void *out = nullptr;
    int out_dtype = FQL_DTYPE_F32;
    const float *bias = nullptr;           // optional per-column bias [N] added to the final outputs
    const float *row_weight = nullptr;     // optional per-row output weight [T] (caller's array: the pre-pass copies it into the plane behind delta)
    const int32_t *tpe = nullptr;          // expert table (both or neither: one group of all rows)
    const int32_t *offs = nullptr;
    int E = 1;
    int T = 0, K = 0, Kp = 0, MBT = 0, N = 0;
    hipStream_t st = nullptr;
    Workspace ws;

    // (after the entry point's addressability checks: MBT is narrowed here)
    void set_shape(int E_, int T_, int K_, int N_) { E = E_; T = T_; K = K_; N = N_; Kp = padded(K_); MBT = (int)row_blocks(T_, E_); }
    bool grouped() const { return tpe != nullptr; }
    int out_kind() const { return out_dtype | (row_weight != nullptr ? 8 : 0); }   // the GEMM kernels' element type + "scale rows" bit
};

// ---- MFMA tile configurations (see fql_gemm_i8.h): 8 waves as WM x WN, NF 32-column fragments per wave.
// X(id, WM, WN, NF, A-ring depth in k-steps, weight stages in flight)
// (ids 4, 10, 14, 15, 16 and 17 were tuning experiments that lost and were built for no limb count: 64 x 256, a 64 x 384 variant
//  and the 4-wave 128 x 96 / 64 x 192 / 128 x 64 tiles, 133.6 / 143.5 against 130.4 us in DESIGN.md 4.2.  The ids stay reserved.)
#define FQL_CFG_LIST(X)                                                                                            \
    X(0, 4, 2, 3, 2, 1)        /* 128 x 192 (3 limbs: 2-step A ring is what the register budget allows) */ \
    X(1, 4, 2, 2, 4, 1)        /* 128 x 128 */ \
    X(2, 4, 2, 4, 2, 1)        /* 128 x 256 (2-limb register budget) */ \
    X(3, 4, 2, 3, 4, 1)        /* 128 x 192, 4-step A ring (2-limb register budget) */ \
    X(5, 1, 8, 1, 4, 1)        /*  32 x 256 (fp8 form only) */ \
    X(6, 4, 1, 2, 8, 4)        /* 128 x  64, 4 waves (fp8 form only): skinny tiles for few rows (HBM-bound: many small */ \
    X(7, 2, 2, 1, 8, 4)        /*  64 x  64, 4 waves   workgroups per CU, 4 weight stages in flight, deep */ \
    X(8, 1, 2, 1, 8, 4)        /*  32 x  64, 2 waves   A ring to cover L2 latency) */ \
    X(9, 2, 4, 3, 2, 1)        /*  64 x 384: 64-row groups with the A-fragment reuse of the 128 x 192 tile */ \
    X(11, 2, 4, 3, 8, 2)       /*  64 x 384, full-stage A ring (every load one stage ahead), 2 weight stages */ \
    X(12, 4, 2, 3, 8, 2)       /* 128 x 192, full-stage A ring, 2 weight stages */ \
    X(13, 4, 1, 2, 4, 8)       /* 128 x  64, 4 waves, 8 weight stages in flight (few tall tiles: HBM-latency bound) */
constexpr int FQL_NUM_CFG = 18;                              // one past the largest id (fql_tune_num_configs: callers walk range(n))
// Short row groups (fql_gemm_rows32.h): 32-row tiles, K split KG ways inside the workgroup.  ids 100 + i.
// R(i, NF, KG, A-ring depth in k-steps, weight stages in flight per wave, waves per SIMD)
#define FQL_ROWS32_LIST(R)                                                                                         \
    R(0, 2, 4, 2, 2, 2)        /* 32 x 128 */ \
    R(1, 2, 8, 2, 1, 2)        /* 32 x  64 */ \
    R(2, 2, 2, 2, 2, 2)        /* 32 x 256 */ \
    R(3, 2, 4, 2, 1, 2)        /* 32 x 128, one weight stage in flight */ \
    R(4, 1, 4, 4, 2, 2)        /* 32 x  64, one fragment per wave */ \
    R(5, 1, 4, 2, 1, 4)        /* 32 x  64, <= 128 registers: two workgroups per CU hide each other's HBM waits */ \
    R(6, 1, 8, 2, 1, 4)        /* 32 x  32, two workgroups per CU */ \
    R(7, 1, 2, 2, 1, 4)        /* 32 x 128, two workgroups per CU */
constexpr int FQL_NUM_ROWS32 = 8;
// Decode-size row groups (fql_gemm_rows16.h): 16-row tiles on v_mfma_i32_16x16x64_i8, every load one stage ahead.
// ids 200 + i.  S(i, NF, KG, weight stages in flight)
#define FQL_ROWS16_LIST(S)                                                                                         \
    S(0, 4, 4, 2)              /* 16 x 128 */ \
    S(1, 4, 2, 2)              /* 16 x 256 */ \
    S(2, 4, 4, 1)              /* 16 x 128, one weight stage in flight */ \
    S(3, 4, 8, 1)              /* 16 x  64 */ \
    S(4, 8, 4, 1)              /* 16 x 256, 8 fragments per wave */ \
    S(5, 4, 8, 2)              /* 16 x  64, both weight stages of a 4096-k row in flight from the start */ \
    S(6, 3, 8, 2)              /* 16 x  48 */ \
    S(7, 3, 8, 1)              /* 16 x  48, one weight stage in flight */ \
    S(8, 2, 8, 2)              /* 16 x  32 */
constexpr int FQL_NUM_ROWS16 = 9;
// (round 3: 16 x 192 and 16 x 160 -- two tiles per workgroup at the decode shape instead of three -- were built and timed: 47.1 / 49.4 us
//  against 46.1 us for id 2, at 253-256 registers; profiles/r03_decode_phase_trace.txt.  Not kept.)
// the same kernel as 4-wave workgroups, two per CU.  ids 220 + i.  S4(i, NF, KG, weight stages in flight)
#define FQL_ROWS16_W4_LIST(S4)                                                                                     \
    S4(0, 4, 4, 1)             /* 16 x  64, K split 4 ways */ \
    S4(1, 4, 4, 2)             /* 16 x  64, two weight stages in flight */ \
    S4(2, 4, 2, 1)             /* 16 x 128, K split 2 ways */ \
    S4(3, 8, 4, 1)             /* 16 x 128, 8 fragments per wave */
constexpr int FQL_NUM_ROWS16_W4 = 4;
// One wave per SIMD (fql_gemm_w4.h, its own translation unit): 128 x 192 tiles, 4 waves of 32 x 192.  ids 300 + i:
// W(i, limbs, fragments per wave, activation ring depth in k-steps)
#define FQL_W4_LIST(W)                                                                                             \
    W(0, 3, 6, 8)              /* 3 limbs, full-stage activation ring */ \
    W(1, 3, 6, 4)              /* 3 limbs, 4-step ring */
constexpr int FQL_NUM_W4 = 2;
// Which wide configurations are BUILT for which limb count: the ones choose_cfg() can return for it, plus the previous
// headline configuration (0 at 3 limbs: the bit-identity baseline of the tests and A/B tools).  The register budgets of
// another limb count (up to 1273 spilled registers) are not instantiated.
constexpr bool wide_cfg_built(int L, int id)
{
    return L == 3 ? (id == 0 || id == 1 || id == 7 || id == 8 || id == 9 || id == 13)
         : L == 2 ? (id == 1 || id == 2 || id == 3 || id == 7 || id == 8 || id == 11 || id == 13)
                  : (id == 1 || id == 2 || id == 7 || id == 8 || id == 11 || id == 12 || id == 13);
}
// ... and for the fp8-activation form (gemm_i8_kernel<1, ..., F8 = true>): the ones choose_cfg_f8() can return, plus 128 x 128
constexpr bool wide_cfg_built_f8(int id) { return id == 1 || id == 5 || id == 6 || id == 7 || id == 8 || id == 11 || id == 12; }
inline bool valid_cfg(int cfg, int L) { return (cfg >= 300 && cfg < 300 + FQL_NUM_W4 && L == 3) || (cfg >= 0 && cfg < FQL_NUM_CFG && wide_cfg_built(L, cfg)) ||
           (cfg >= 100 && cfg < 100 + FQL_NUM_ROWS32) || (cfg >= 200 && cfg < 200 + FQL_NUM_ROWS16) || (cfg >= 220 && cfg < 220 + FQL_NUM_ROWS16_W4);
}
inline bool valid_cfg_f8(int cfg) { return wide_cfg_built_f8(cfg); }

// The MFMA path addresses its operands through 32-bit buffer offsets.
inline bool mfma_addressable(int L, int T, int E, int K, int N, bool f8 = false)
{
    const size_t a = (has_residual(L, f8) ? 2 : 1) * limb_bytes(L, T, E, padded(K));   // (with the residual limb set where there is one)
    const size_t b = ((size_t)N + 256) * (size_t)(K >> 1);
    return a < ((size_t)1 << 31) && b < ((size_t)1 << 31);
}

inline bool mfma_eligible(int L, int T, int E, int K, int N, const uint8_t *packed)
{
    return (K % 32 == 0) && aligned16(packed) && mfma_addressable(L, T, E, K, N);
}

// The expert table comes as a pair or not at all, and without one there is one group of all rows.
inline int table_check(const int32_t *tpe, const int32_t *offs, int E)
{
    if ((tpe == nullptr) != (offs == nullptr)) return FQL_ERR_NULL_POINTER;
    if (tpe == nullptr && E != 1) return FQL_ERR_BAD_SHAPE;
    return FQL_OK;
}

// The pre-pass: c.x -> limbs, delta, rowsum of c.ws (and, with a table, zeroes the rows of c.out no expert covers).
template <int L>
int launch_act_quant(const Call &c)
{
    const int T = c.T, K = c.K;
    void *zero_out = c.grouped() ? c.out : nullptr;
    // ACT_ROWS-row workgroups over the grouped rows (each finds its rows' padded positions itself), plus (MoE entry
    // point) the workgroups that zero the rows of `out` no expert covers
    const int mblocks = !c.grouped() ? (T + FQL_MB - 1) / FQL_MB : (T + FQL_MB * c.E) / FQL_MB;   // (upper bound of the padded row blocks)
    const bool vec = (K % 16 == 0) && aligned16(c.x);
    // few rows in all (at most two single-row workgroups per CU; measured: 16 rows 6.3 -> 4.6 us, 1280 padded rows 12.5 -> 16.5 us): one row per workgroup -- the pre-pass is a latency
    // chain there and a row spread over 256 threads shortens every link of it (fql_act_quant.h)
    const bool single = vec && mblocks * FQL_MB <= g_act_single_rows;
    const int rblocks = single ? T : (T + ACT_ROWS - 1) / ACT_ROWS;
    const int zblocks = zero_out != nullptr ? (T + 255) / 256 : 0;
    if (c.gated && !c.f8 && c.act != FQL_ACT_SILU) {           // another activation kind: the instantiations of fql_glu.hip
        if (c.gather != nullptr) return FQL_ERR_DTYPE;
        FqlActGatedArgs a{c.x, c.ws.delta, c.ws.rowsum, c.ws.limbs, T, K, c.Kp / FQL_KB, c.MBT, rblocks, zblocks, zero_out,
                          dtype_bytes(c.out_dtype), c.N, c.tpe, c.offs, c.E, c.row_weight, c.st};
        return fql_act_glu_launch(L, single ? 0 : (vec ? 1 : 2), c.in_dtype, a, c.act, c.act_alpha, c.act_limit) == 0 ? FQL_OK : FQL_ERR_LAUNCH;
    }
    if (c.gated && !c.f8 && c.in_dtype != FQL_DTYPE_F32) {     // 16-bit gate|up rows: the instantiations of fql_ffn16.hip
        if (c.gather != nullptr) return FQL_ERR_DTYPE;
        FqlActGatedArgs a{c.x, c.ws.delta, c.ws.rowsum, c.ws.limbs, T, K, c.Kp / FQL_KB, c.MBT, rblocks, zblocks, zero_out,
                          dtype_bytes(c.out_dtype), c.N, c.tpe, c.offs, c.E, c.row_weight, c.st};
        return fql_act_gated16_launch(L, single ? 0 : (vec ? 1 : 2), c.in_dtype, a) == 0 ? FQL_OK : FQL_ERR_LAUNCH;
    }
    void (*kern)(const void *, const int32_t *, int, float *, int32_t *, int8_t *, int, int, int, int, int, void *, int,
                 int, const int32_t *, const int32_t *, int, const float *);
#define FQL_ACT_PICK(l, in, gate, f8) \
    (single ? act_fused_kernel<l, true, in, gate, f8, 1> : (vec ? act_fused_kernel<l, true, in, gate, f8> : act_fused_kernel<l, false, in, gate, f8>))
    if (c.f8) {
        if constexpr (L == 1) {
            switch (c.in_dtype) {
            case FQL_DTYPE_F16: kern = FQL_ACT_PICK(1, 1, false, true); break;
            case FQL_DTYPE_BF16: kern = FQL_ACT_PICK(1, 2, false, true); break;
            default: kern = FQL_ACT_PICK(1, 0, false, true); break;
            }
        } else return FQL_ERR_BAD_PRECISION;
    } else if (c.gated) kern = FQL_ACT_PICK(L, 0, true, false);
    else switch (c.in_dtype) {
    case FQL_DTYPE_F16: kern = FQL_ACT_PICK(L, 1, false, false); break;
    case FQL_DTYPE_BF16: kern = FQL_ACT_PICK(L, 2, false, false); break;
    default: kern = FQL_ACT_PICK(L, 0, false, false); break;
    }
#undef FQL_ACT_PICK
    return launch(kern, dim3(rblocks + zblocks), dim3(256), 0, c.st, c.x, c.gather, c.n_src, c.ws.delta, c.ws.rowsum, c.ws.limbs,
                  T, K, c.Kp / FQL_KB, c.MBT, rblocks, zero_out, dtype_bytes(c.out_dtype), c.N, c.tpe, c.offs, c.E, c.row_weight);
}

// Column tiles per row block of the wide kernel.  The fewest that cover N (every tile at most `fpt` fragments of 32
// columns) is the plain tiling; a few more, narrower tiles are chosen when that evens out what each persistent
// workgroup walks (fql_gemm_i8.h, tile_params).  Cost model: a tile costs its fragments + 1 (prologue / epilogue),
// the launch costs what its busiest workgroup walks; `m_tiles` is the row-block count under even routing (the real
// count lives on the device).  Exact replay of the kernel's tile order, cached per shape.
int g_balance_tiles = 1;
inline int host_xcd_remap(int bid, int nblk)
{
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}
inline int balanced_n_tiles(int N, int fpt, long long m_tiles, int wgs, int frag = 32, int overhead = 1, int min_base = -1)
{
    if (min_base < 0) min_base = fpt - 1;                    // wide kernel: its K loop has a form for one fragment less than a full tile, not fewer
    const int F = (N + frag - 1) / frag;
    const int tmin = (F + fpt - 1) / fpt;
    if (!g_balance_tiles || m_tiles <= 0 || wgs <= 0 || wgs > 4096 || m_tiles * tmin > 8192) return tmin;
    struct Key { int N, fpt, wgs, frag; long long m_tiles; int result; };
    static thread_local Key cache[8] = {};
    static thread_local int next_slot = 0;
    for (const Key &k : cache)
        if (k.result > 0 && k.N == N && k.fpt == fpt && k.wgs == wgs && k.frag == frag && k.m_tiles == m_tiles) return k.result;
    auto busiest = [&](int t) -> long long {
        const long long n_real = m_tiles * t;
        const int base = F / t, rem = F - base * t;
        const int G = n_real < wgs ? (int)n_real : wgs;
        static thread_local int cost[4096];
        for (int i = 0; i < G; ++i) cost[i] = 0;
        for (int vb = 0; vb < (int)n_real; ++vb) {
            const int i = host_xcd_remap(vb, (int)n_real) % t;
            cost[vb % G] += base + (i < rem ? 1 : 0) + overhead;
        }
        int mx = 0;
        for (int i = 0; i < G; ++i) mx = cost[i] > mx ? cost[i] : mx;
        return mx;
    };
    int best = tmin;
    long long best_cost = busiest(tmin);
    // candidates: tile counts that make the launch a whole number of rounds
    for (long long rounds = (m_tiles * tmin + wgs - 1) / wgs; rounds <= (m_tiles * tmin + wgs - 1) / wgs + 1; ++rounds) {
        if ((rounds * wgs) % m_tiles != 0) continue;
        const long long t = rounds * wgs / m_tiles;
        if (t <= tmin || t > F || F / t < min_base) continue;
        const long long c = busiest((int)t);
        if (c < best_cost) { best_cost = c; best = (int)t; }
    }
    cache[next_slot] = Key{N, fpt, wgs, frag, m_tiles, best};
    next_slot = (next_slot + 1) & 7;
    return best;
}

// ---- The persistent grid of a tile kernel: BM x BN tiles walked by at most `wg_per_cu` workgroups per compute unit.
// Balance: the kernel can also split N into `n_alt` uneven column tiles (balanced_n_tiles) and picks between the two
// tilings from the real row-block count; frag = 0 for a kernel without that form.
struct Balance { int frag, overhead, min_base; };            // fragment width in columns, per-tile overhead, fewest fragments per tile (< 0: one less than a full tile)
constexpr Balance NO_BALANCE{0, 0, 0};
constexpr Balance WIDE_BALANCE{32, 1, -1};                   // fql_gemm_i8.h (NF >= 2, integer limbs) and fql_gemm_w4.h
constexpr Balance ROWS16_BALANCE{16, 2, 1};                  // fql_gemm_rows16.h
struct GridPlan {
    int n_tiles;               // the fewest column tiles that cover N ...
    int n_alt;                 // ... and the balanced alternative (0: none)
    int m_slots;               // upper bound of the row blocks (the real count is on the device)
    long long worst;           // worst-case tile count
    unsigned blocks;           // workgroups launched
};
inline int plan_grid(int BM, int BN, int wg_per_cu, Balance bal, const Call &c, GridPlan &p)
{
    const int wgs = compute_units() * wg_per_cu;
    p.n_tiles = (c.N + BN - 1) / BN;
    p.m_slots = !c.grouped() ? (c.T + BM - 1) / BM : c.T / BM + c.E;
    p.n_alt = 0;
    if (bal.frag != 0) {
        const int groups = !c.grouped() ? 1 : c.E;
        const long long m_even = (long long)groups * (((c.T + groups - 1) / groups + BM - 1) / BM);   // row blocks if evenly routed
        p.n_alt = balanced_n_tiles(c.N, BN / bal.frag, m_even, wgs, bal.frag, bal.overhead, bal.min_base);
        if (p.n_alt == p.n_tiles) p.n_alt = 0;
    }
    p.worst = (long long)(p.n_alt > p.n_tiles ? p.n_alt : p.n_tiles) * p.m_slots;
    if (p.worst <= 0 || p.worst > 0x7fffffffLL) return FQL_ERR_BAD_SHAPE;
    p.blocks = (unsigned)(p.worst > wgs ? wgs : p.worst);
    return FQL_OK;
}

// A new tile family plugs in here: its launcher names its kernel (the LDS flag is one per instantiation: `static` in
// the launcher template), asks plan_grid() for the grid and passes the plan on; launch_gemm() gets its id range.
template <int L, int WM, int WN, int NF, int DEPTH, int BDEPTH, bool F8 = false>
int launch_gemm_cfg(const Call &c)
{
    using C = GemmCfg<L, WM, WN, NF, DEPTH, BDEPTH>;
    auto kern = gemm_i8_kernel<L, WM, WN, NF, DEPTH, BDEPTH, F8>;
    static PerDeviceFlag attr;
    if (!ensure_lds_attr(attr, reinterpret_cast<const void *>(kern), C::LDS_BYTES)) return FQL_ERR_LAUNCH;
    // persistent: the 8-wave workgroups fill a CU alone; the small skinny-tile workgroups share it 4 / 8 ways (2 waves per SIMD either way)
    GridPlan p;
    if (const int rc = plan_grid(C::BM, C::BN, C::NW >= 8 ? 1 : (C::NW == 4 ? 2 : 4), (NF >= 2 && !F8) ? WIDE_BALANCE : NO_BALANCE, c, p)) return rc;
    return launch(kern, dim3(p.blocks), dim3(C::THREADS), C::LDS_BYTES, c.st, c.ws.limbs, c.ws.delta, c.ws.rowsum, c.packed, c.scales,
                  c.zps, c.out, c.out_kind(), c.tpe, c.offs, c.E, c.T, c.K, c.Kp, c.MBT, c.N, p.n_tiles, p.m_slots, c.ws.scratch, c.bias, p.n_alt);
}

template <int L, int NF, int KG, int DEPTH, int BDEPTH, int OCC>
int launch_rows32_cfg(const Call &c)
{
    using C = Rows32Cfg<L, NF, KG, DEPTH, BDEPTH, OCC>;
    auto kern = gemm_i8_rows32_kernel<L, NF, KG, DEPTH, BDEPTH, OCC>;
    static PerDeviceFlag attr;
    if (!ensure_lds_attr(attr, reinterpret_cast<const void *>(kern), C::LDS_BYTES)) return FQL_ERR_LAUNCH;
    GridPlan p;                                              // persistent: WG_PER_CU 8-wave workgroups per CU
    if (const int rc = plan_grid(C::BM, C::BN, C::WG_PER_CU, NO_BALANCE, c, p)) return rc;
    return launch(kern, dim3(p.blocks), dim3(C::THREADS), C::LDS_BYTES, c.st, c.ws.limbs, c.ws.delta, c.ws.rowsum, c.packed, c.scales,
                  c.zps, c.out, c.out_kind(), c.tpe, c.offs, c.E, c.T, c.K, c.Kp, c.MBT, c.N, p.n_tiles, p.m_slots, c.ws.scratch, c.bias);
}

template <int L, int NF, int KG, int BDEPTH, int NWAVES = 8>
int launch_rows16_cfg(const Call &c)
{
    using C = Rows16Cfg<L, NF, KG, BDEPTH, NWAVES>;
    auto kern = gemm_i8_rows16_kernel<L, NF, KG, BDEPTH, NWAVES>;
    static PerDeviceFlag attr;
    if (!ensure_lds_attr(attr, reinterpret_cast<const void *>(kern), C::LDS_BYTES)) return FQL_ERR_LAUNCH;
    GridPlan p;                                              // persistent: one 8-wave or two 4-wave workgroups per CU
    if (const int rc = plan_grid(C::BM, C::BN, 8 / C::NW, ROWS16_BALANCE, c, p)) return rc;
    return launch(kern, dim3(p.blocks), dim3(C::THREADS), C::LDS_BYTES, c.st, c.ws.limbs, c.ws.delta, c.ws.rowsum, c.packed, c.scales,
                  c.zps, c.out, c.out_kind(), c.tpe, c.offs, c.E, c.T, c.K, c.Kp, c.MBT, c.N, p.n_tiles, p.m_slots, c.ws.scratch, c.bias, p.n_alt);
}

// One launch for pre-pass + GEMM (fql_gemm_w4.h, FUSED): tuning switch, the polls a workgroup spends on another one's rows
// before it quantises them itself, and the launch token (unique per launch: a flag word of an earlier launch, or of
// whatever the workspace held before, never equals it -- 2^-64 for arbitrary memory).
int g_fused = 0;
int g_fused_spin = 20000;
inline unsigned long long next_fused_token()
{
    static const unsigned long long salt = ((unsigned long long)std::random_device{}() << 32) | 0x100000000ull;
    static std::atomic<unsigned> counter{1};
    return salt ^ (unsigned long long)counter.fetch_add(1, std::memory_order_relaxed);
}
// The one-wave-per-SIMD kernel: same tiles and column split as the wide kernel's 128 x 192 configuration, one workgroup per CU.
inline int plan_w4(int L, int nf, const Call &c, GridPlan &p) { return plan_grid(128, fql_w4_bn(L, nf), 1, WIDE_BALANCE, c, p); }
// The one-launch form keeps its tile list in the 16-entry LDS table: every workgroup must get by with one table.
inline bool w4_fusable(int L, int nf, const Call &c)
{
    GridPlan p;
    return plan_w4(L, nf, c, p) == FQL_OK && (p.worst + p.blocks - 1) / p.blocks <= 16;
}

// `fused`: the kernel quantises the rows of c.x itself, no pre-pass launch came before (w4_fusable() said it may)
int launch_w4_cfg(int L, int nf, int depth, const Call &c, bool fused)
{
    if (c.Kp < 2 * FQL_KB) return FQL_ERR_BAD_SHAPE;         // its pipeline runs two weight stages ahead
    GridPlan p;
    if (const int rc = plan_w4(L, nf, c, p)) return rc;
    FqlW4Args a;
    a.limbs = c.ws.limbs; a.delta = c.ws.delta; a.rowsum = c.ws.rowsum;
    a.packed = c.packed; a.scales = c.scales; a.zps = c.zps;
    a.out = c.out; a.out_kind = c.out_kind();
    a.tpe = c.tpe; a.offs = c.offs;
    a.E = c.E; a.T = c.T; a.K = c.K; a.Kp = c.Kp; a.MBT = c.MBT; a.N = c.N;
    a.n_tiles = p.n_tiles; a.m_slots = p.m_slots; a.n_alt = p.n_alt;
    a.scratch = c.ws.scratch; a.bias = c.bias;
    a.blocks = p.blocks; a.stream = c.st;
    if (fused) {
        a.fused = true;
        a.fz = FqlW4Fused{c.x, c.gather, c.n_src, c.row_weight, c.ws.flags, next_fused_token(), g_fused_spin};
    }
    const int rc = fql_w4_launch(L, nf, depth, a);
    return rc == 0 ? FQL_OK : (rc == -2 ? FQL_ERR_BAD_SHAPE : FQL_ERR_LAUNCH);
}

template <int L>
int launch_gemm(int cfg, const Call &c, bool fused = false)
{
    switch (cfg) {
#define W(i, l, nf, d)                                                                                            \
    case 300 + i: return L == l ? launch_w4_cfg(l, nf, d, c, fused) : FQL_ERR_BAD_SHAPE;
        FQL_W4_LIST(W)
#undef W
#define X(id, wm, wn, nf, d, bp)                                                                                  \
    case id:                                                                                                      \
        if constexpr (wide_cfg_built(L, id)) return launch_gemm_cfg<L, wm, wn, nf, d, bp>(c);                     \
        else return FQL_ERR_BAD_SHAPE;
        FQL_CFG_LIST(X)
#undef X
#define R(i, nf, kg, d, bd, occ) case 100 + i: return launch_rows32_cfg<L, nf, kg, d, bd, occ>(c);
        FQL_ROWS32_LIST(R)
#undef R
#define S(i, nf, kg, bd) case 200 + i: return launch_rows16_cfg<L, nf, kg, bd>(c);
        FQL_ROWS16_LIST(S)
#undef S
#define S4(i, nf, kg, bd) case 220 + i: return launch_rows16_cfg<L, nf, kg, bd, 4>(c);
        FQL_ROWS16_W4_LIST(S4)
#undef S4
    default: return FQL_ERR_BAD_SHAPE;
    }
}

// fp8-activation form of the wide kernel
int launch_gemm_f8(int cfg, const Call &c)
{
    switch (cfg) {
#define X(id, wm, wn, nf, d, bp)                                                                                  \
    case id:                                                                                                      \
        if constexpr (wide_cfg_built_f8(id)) return launch_gemm_cfg<1, wm, wn, nf, d, bp, true>(c);               \
        else return FQL_ERR_BAD_SHAPE;
        FQL_CFG_LIST(X)
#undef X
    default: return FQL_ERR_BAD_SHAPE;
    }
}

// Tile choice of the fp8 form: weight-streaming bound at every shape it is meant for (one MFMA pass).
inline int choose_cfg_f8(int E, int T, int N, bool grouped)
{
    const int groups = grouped ? (E > 0 ? E : 1) : 1;
    const int m = (T + groups - 1) / groups;
    const long long wide_tiles = (long long)groups * ((m + 127) / 128) * ((N + 255) / 256);
    if (wide_tiles < 128 && m <= 128) return m <= 32 ? 8 : (m <= 64 ? 7 : 6);
    if (m <= 32) return 5;
    if (m <= 64) return 11;
    return 12;
}

// Heuristic tile choice for the product path (MI355X: 256 CUs, one workgroup per CU).
//   rows per group decide the tile height (32 / 64 / 128-row tiles: a short group must not pay for
//   128 rows of MFMA work); the tile width is the one that needs the least "rounds x width" of the
//   256 CUs -- e.g. 8 experts x 128 rows x N = 11008: 128 x 192 tiles give 464 tiles = 2 rounds x 192,
//   128 x 128 give 688 = 3 rounds x 128 (equal), 128 x 256 give 344 = 2 rounds x 256 (worse).
inline int choose_cfg(int L, int E, int T, int K, int N, bool grouped)
{
    (void)K;
    const int groups = grouped ? (E > 0 ? E : 1) : 1;
    const int m = (T + groups - 1) / groups;                 // rows per group if evenly routed
    // few rows in total: the op is HBM-bound, what matters is enough tiles to have every CU streaming
    // weights (N / 64 tiles per row block instead of N / 256)
    const long long wide_tiles = (long long)groups * ((m + 127) / 128) * ((N + 255) / 256);
    if (wide_tiles < 128 && m <= 128) {
        if (m <= 16) return 207;                             //  16 x 48 decode tiles, K split 8 ways (fql_gemm_rows16.h)
        if (m <= 32) return 8;                               //  32 x 64, 2 waves
        if (m <= 64) return 7;                               //  64 x 64, 4 waves
        // 65..128 rows: 128 x 64, 4 waves, 8 weight stages in flight; at 3 limbs the 128 x 128 tile of the wide kernel is
        // 8-10 % faster (96 rows 38.1 vs 41.3 us, 128 rows 40.3 vs 44.5 us, 4096 -> 11008, profiles/r03_small_groups.txt)
        return L == 3 ? 1 : 13;
    }
    if (m <= 16) return 202;                                 //  16 x 128 decode tiles: every load one stage ahead
    if (m <= 32) return 103;                                 //  32 x 128, K split 4 ways inside the workgroup
    if (m <= 64) {                                           //  64 x 384 (1 / 2 limbs: full-stage activation ring) ...
        // ... 3 limbs: the one-wave-per-SIMD kernel's 33..64-row tile class (two row blocks x two fragment halves per
        // workgroup): 79.7 vs 89.3 us at 8 x 64 rows (profiles/r03_small_groups.txt); at 32 rows the 32-row kernel stays (67 vs 70)
        if (L == 3 && g_use_w4 && padded(K) >= 2 * FQL_KB) return 301;
        return (L <= 2) ? 11 : 9;
    }
    const int mt = groups * ((m + 127) / 128);
    struct Cand { int cfg, bn; };
    // 3 limbs: 128 x 192 with a 2-step A ring (register budget) / 128 x 128; 2 limbs: 4-step ring, + 128 x 256
    const Cand c3[2] = {{0, 192}, {1, 128}};
    const Cand c2[3] = {{3, 192}, {1, 128}, {2, 256}};
    const Cand c1[3] = {{12, 192}, {1, 128}, {2, 256}};      // 1 limb: registers allow the full-stage activation ring
    const Cand *cands = (L == 1) ? c1 : (L == 2) ? c2 : c3;
    const int nc = (L <= 2) ? 3 : 2;
    int best = cands[0].cfg;
    long long best_cost = -1;
    for (int i = 0; i < nc; ++i) {
        const long long tiles = (long long)mt * ((N + cands[i].bn - 1) / cands[i].bn);
        const long long rounds = (tiles + 255) / 256;
        const long long cost = rounds * (cands[i].bn + 24);  // +24: per-tile prologue / epilogue
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = cands[i].cfg; }
    }
    // the same 128 x 192 tiles at one wave per SIMD (measured: 124.7 vs 134.4 us at configs[2], 182.6 vs 204.4 us under
    // skewed routing, profiles/r03_w4_vs_wide.txt); its pipeline runs two 256-k weight stages ahead
    if (best == 0 && g_use_w4 && padded(K) >= 2 * FQL_KB) best = 301;
    return best;
}

// Pre-pass + GEMM of a call whose workspace is carved.
int run_mfma(int L, const Call &c)
{
    if (c.f8) {                                              // float rows -> e4m3 with a per-row scale, one fp8 MFMA pass
        if (c.gated) return FQL_ERR_BAD_PRECISION;
        const int rc = launch_act_quant<1>(c);
        return rc != FQL_OK ? rc : launch_gemm_f8(choose_cfg_f8(c.E, c.T, c.N, c.grouped()), c);
    }
    const int cfg = choose_cfg(L, c.E, c.T, c.K, c.N, c.grouped());
    // one launch: no pre-pass, it is the GEMM kernel's first phase
    const bool fused = L == 3 && g_fused && cfg == 301 && c.in_dtype == FQL_DTYPE_F32 && !c.gated && c.ws.flags != nullptr &&
                       (c.K % 16 == 0) && aligned16(c.x) && w4_fusable(3, 6, c);
    return with_limbs(L, [&](auto l) {
        constexpr int LL = decltype(l)::value;
        if (!fused)
            if (const int rc = launch_act_quant<LL>(c)) return rc;
        return launch_gemm<LL>(cfg, c, fused);
    });
}
// ... of a call whose shape is set: carves the caller's workspace into the record first
int run_mfma(int L, Call &c, void *workspace, size_t workspace_bytes)
{
    if (workspace == nullptr || !aligned16(workspace)) return FQL_ERR_WORKSPACE;
    c.ws = carve(workspace, L, c.T, c.E, c.Kp, has_residual(L, c.f8));
    if (workspace_bytes < c.ws.bytes) return FQL_ERR_WORKSPACE;
    return run_mfma(L, static_cast<const Call &>(c));
}

int run_generic(const float *x, const uint8_t *packed, const float *scales, const float *zps, float *out,
                const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, hipStream_t st,
                const float *bias = nullptr)
{
    if (tpe != nullptr) {
        hipLaunchKernelGGL(zero_uncovered_rows_kernel, dim3(T), dim3(256), 0, st, out, tpe, offs, E, T, N);
        if (hipGetLastError() != hipSuccess) return FQL_ERR_LAUNCH;
    }
    hipLaunchKernelGGL((fused_rows_kernel<4>), dim3((N + 3) / 4, E), dim3(256), 0, st, x, packed, scales, zps,
                       out, tpe, offs, T, K, N, bias);
    return launched();
}

size_t gemv_lds_bytes(int B, int K) { return ((size_t)B * (K >> 5) * GEMV_SEG + (size_t)B * 4) * sizeof(float); }

template <int B, bool GROUPED = false>
int launch_gemv(const float *x, const uint8_t *packed, const float *scales, const float *zps, float *out,
                int K, int N, hipStream_t st, const float *bias, int group = 0)
{
    const int groups = (N + GEMV_ROWS - 1) / GEMV_ROWS;
    int blocks = (groups + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    const size_t lds = gemv_lds_bytes(B, K);
    if (lds > 48 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&gemv_kernel<B, GROUPED>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return FQL_ERR_LAUNCH;
    }
    return launch(gemv_kernel<B, GROUPED>, dim3(blocks), dim3(256), lds, st, x, packed, scales, zps, out, K, N, bias, group);
}

// The router's group width for E experts: f(std::integral_constant<int, G>, std::integral_constant<int, NPL>) with
// G = min(64, next_pow2(E)) lanes per token and NPL = 2 experts per lane past 64 (csrc/fql_router.h)
template <class F>
int with_router_group(int E, F &&f)
{
    using std::integral_constant;
    if (E > 64) return f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
    if (E > 32) return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    if (E > 16) return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    if (E > 8) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    if (E > 4) return f(integral_constant<int, 8>{}, integral_constant<int, 1>{});
    if (E > 2) return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    if (E > 1) return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
}
int router_shape_check(int dtype, int T, int E, int top_k)
{
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (T < 0 || E < 1 || E > ROUTER_MAX_EXPERTS || top_k < 1 || top_k > E || top_k > ROUTER_MAX_TOPK) return FQL_ERR_BAD_SHAPE;
    return FQL_OK;
}
// The scored router's arguments on top of router_shape_check (the backward has no groups: n_group = topk_group = 1)
int router_score_shape_check(int dtype, int T, int E, int top_k, int scoring, int n_group, int topk_group, int group_top,
                             float scale)
{
    if (const int rc = router_shape_check(dtype, T, E, top_k)) return rc;
    if (scoring < 0 || scoring > 1 || n_group < 1 || n_group > ROUTER_MAX_GROUPS || E % n_group != 0 || topk_group < 1 ||
        topk_group > n_group || topk_group * (E / n_group) < top_k || group_top < 1 || group_top > 2 || !std::isfinite(scale))
        return FQL_ERR_BAD_SHAPE;
    return FQL_OK;
}

// One launch of the router for arguments the entry points have checked.  The plain rule (softmax, no bias, one group,
// scale 1) takes the forward instantiation that has the other rules compiled out: the same bits, fewer registers.
int launch_router_fwd(const void *logits, int dtype, int T, int E, int top_k, int scoring, const float *select_bias,
                      int n_group, int topk_group, int group_top, int renormalize, float scale, int32_t *indices,
                      float *weights, float *scores, hipStream_t st)
{
    const bool plain = scoring == 0 && select_bias == nullptr && n_group == 1 && scale == 1.0f;
    return with_router_group(E, [&](auto G, auto NPL) {
        const unsigned blocks = (unsigned)(((long long)T + ROUTER_THREADS / G.value - 1) / (ROUTER_THREADS / G.value));
        return launch(plain ? router_topk_fwd_kernel<G.value, NPL.value, false> : router_topk_fwd_kernel<G.value, NPL.value, true>,
                      dim3(blocks), dim3(ROUTER_THREADS), 0, st, logits, dtype, T, E, top_k, scoring, select_bias, n_group,
                      topk_group, group_top, renormalize, scale, indices, weights, scores);
    });
}
int launch_router_bwd(const void *logits, int dtype, const int32_t *indices, const float *grad_weights,
                      const float *grad_scores, void *grad_logits, int T, int E, int top_k, int scoring, int renormalize,
                      float scale, hipStream_t st)
{
    return with_router_group(E, [&](auto G, auto NPL) {
        const unsigned blocks = (unsigned)(((long long)T + ROUTER_THREADS / G.value - 1) / (ROUTER_THREADS / G.value));
        return launch(router_topk_bwd_kernel<G.value, NPL.value>, dim3(blocks), dim3(ROUTER_THREADS), 0, st, logits, dtype,
                      indices, grad_weights, grad_scores, grad_logits, T, E, top_k, scoring, renormalize, scale);
    });
}

// The combine's element types: f(std::integral_constant<int, kind>) for a code that valid_dtype() has accepted
template <class F>
int with_dtype(int dt, F &&f)
{
    if (dt == FQL_DTYPE_F16) return f(std::integral_constant<int, FQL_DTYPE_F16>{});
    if (dt == FQL_DTYPE_BF16) return f(std::integral_constant<int, FQL_DTYPE_BF16>{});
    return f(std::integral_constant<int, FQL_DTYPE_F32>{});
}
bool elem_aligned(const void *p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// One launch of the combine / of its backward for arguments the entry points have checked (T <= 65535: grid.y).
// `sparse`: the instantiation that skips a slot with pos < 0 (fql_combine_sparse / fql_combine_sparse_bwd).
int launch_combine(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights, const void *addend,
                   const float *addend_weight, void *out, int out_dtype, int T, int top_k, int N, int R, hipStream_t st,
                   bool sparse = false)
{
    const unsigned cols = in_dtype == FQL_DTYPE_F32 ? 1024 : 2048;       // 256 threads x 16 bytes of the input type
    return with_dtype(in_dtype, [&](auto ik) {
        return with_dtype(out_dtype, [&](auto ok) {
            return launch(sparse ? combine_kernel<ik.value, ok.value, true> : combine_kernel<ik.value, ok.value, false>,
                          dim3((N + cols - 1) / cols, T), dim3(256), 0, st, y, pos_of_slot, weights, addend, addend_weight, out,
                          T, top_k, N, R);
        });
    });
}
int launch_combine_bwd(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot, const float *weights,
                       const void *addend, const float *addend_weight, int in_dtype, void *grad_y, float *grad_weights,
                       void *grad_addend, float *grad_addend_weight, int T, int top_k, int N, int rows, hipStream_t st,
                       bool sparse = false)
{
    return with_dtype(in_dtype, [&](auto ik) {
        return with_dtype(out_dtype, [&](auto ok) {
            return launch(sparse ? combine_bwd_kernel<ik.value, ok.value, true> : combine_bwd_kernel<ik.value, ok.value, false>,
                          dim3(T), dim3(256), 0, st, grad_out, y, pos_of_slot, weights, addend, addend_weight, grad_y,
                          grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows);
        });
    });
}

// fql_combine / fql_combine_sparse and their backwards: one set of checks, in the order include/fql_int4.h freezes
int combine_entry(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights, const void *addend,
                  const float *addend_weight, void *out, int out_dtype, int T, int top_k, int N, int R, void *stream,
                  bool sparse)
{
    if (T < 0 || top_k <= 0 || N < 0 || R < 0) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!y || !pos_of_slot || !out || R == 0) return FQL_ERR_NULL_POINTER;
    if (addend_weight != nullptr && addend == nullptr) return FQL_ERR_NULL_POINTER;
    if (T > 65535) return FQL_ERR_BAD_SHAPE;                 // grid.y
    const int ib = dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!elem_aligned(y, ib) || !elem_aligned(addend, ib) || !elem_aligned(out, ob) || !elem_aligned(pos_of_slot, 4) ||
        !elem_aligned(weights, 4) || !elem_aligned(addend_weight, 4))
        return FQL_ERR_ALIGNMENT;
    return launch_combine(y, in_dtype, pos_of_slot, weights, addend, addend_weight, out, out_dtype, T, top_k, N, R,
                          static_cast<hipStream_t>(stream), sparse);
}
int combine_bwd_entry(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot, const float *weights,
                      const void *addend, const float *addend_weight, int in_dtype, void *grad_y, float *grad_weights,
                      void *grad_addend, float *grad_addend_weight, int T, int top_k, int N, int rows, void *stream,
                      bool sparse)
{
    if (T < 0 || top_k <= 0 || N < 0 || rows < 0 || (T > 0 && rows == 0)) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || (N == 0 && grad_weights == nullptr && grad_addend_weight == nullptr)) return FQL_OK;
    if (!pos_of_slot) return FQL_ERR_NULL_POINTER;
    if (N > 0 && (!grad_out || !grad_y)) return FQL_ERR_NULL_POINTER;
    if (grad_weights != nullptr && N > 0 && !y) return FQL_ERR_NULL_POINTER;
    if ((addend_weight != nullptr || grad_addend_weight != nullptr) && addend == nullptr) return FQL_ERR_NULL_POINTER;
    const int ib = dtype_bytes(in_dtype), ob = dtype_bytes(out_dtype);
    if (!elem_aligned(grad_out, ob) || !elem_aligned(y, ib) || !elem_aligned(addend, ib) || !elem_aligned(grad_y, ib) ||
        !elem_aligned(grad_addend, ib) || !elem_aligned(pos_of_slot, 4) || !elem_aligned(weights, 4) ||
        !elem_aligned(addend_weight, 4) || !elem_aligned(grad_weights, 4) || !elem_aligned(grad_addend_weight, 4))
        return FQL_ERR_ALIGNMENT;
    return launch_combine_bwd(grad_out, out_dtype, y, pos_of_slot, weights, addend, addend_weight, in_dtype, grad_y,
                              grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows,
                              static_cast<hipStream_t>(stream), sparse);
}

}  // namespace

extern "C" {

int fql_version(void) { return FQL_VERSION; }

const char *fql_error_string(int code)
{
    switch (code) {
    case FQL_OK: return "ok";
    case FQL_ERR_NULL_POINTER: return "a required pointer is NULL";
    case FQL_ERR_BAD_SHAPE: return "bad shape: dimensions must be positive and fit the addressable range";
    case FQL_ERR_ODD_K: return "input_dim (K) must be even: two 4-bit weights per packed byte";
    case FQL_ERR_WORKSPACE: return "workspace is NULL, not 16-byte aligned, or smaller than *_workspace_bytes()";
    case FQL_ERR_LAUNCH: return "kernel launch failed (hipGetLastError)";
    case FQL_ERR_BAD_PRECISION: return "precision must be FQL_PRECISION_DEFAULT, _INT8 (1), _FAST (2), _EXACT (3) or _FP8 (8), and is supported by this entry point";
    case FQL_ERR_DTYPE: return "element type not supported on this path (16-bit input / output exists on the MFMA path only)";
    case FQL_ERR_ALIGNMENT: return "tensor base pointer not aligned as documented";
    default: return "unknown error code";
    }
}

int fql_act_padded_k(int K) { return K > 0 ? padded(K) : 0; }

size_t fql_linear_workspace_bytes(int B, int K, int N, int precision)
{
    (void)N;
    const int L = limbs_of(precision);
    if (L < 0 || (B <= g_gemv_max_rows && !is_f8(precision)) || B <= 0 || K <= 0 || (K % 32) != 0) return 0;   // (GEMV shapes use no workspace; fql_linear_fwd_f8 takes any B on the MFMA path)
    Workspace w = carve(nullptr, L, B, 1, padded(K), has_residual(L, is_f8(precision)));
    return w.bytes;
}

size_t fql_moe_workspace_bytes(int E, int T, int K, int N, int precision)
{
    (void)N;
    const int L = limbs_of(precision);
    if (L < 0 || T <= 0 || E <= 0 || K <= 0 || (K % 32) != 0) return 0;
    Workspace w = carve(nullptr, L, T, E, padded(K), has_residual(L, is_f8(precision)));
    return w.bytes;
}

static int linear_f32_core(const float *x, const uint8_t *packed, const float *scales, const float *zps, const float *bias,
                           float *out, int B, int K, int N, int precision, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (B < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (B == 0 || N == 0) return FQL_OK;
    if (!x || !packed || !scales || !zps || !out) return FQL_ERR_NULL_POINTER;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K == 0) {                                     // empty contraction: out = 0 (+ bias: the caller adds it; not a path worth a kernel)
        if (bias != nullptr) return FQL_ERR_BAD_SHAPE;
        return hipMemsetAsync(out, 0, (size_t)B * N * sizeof(float), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    const bool mfma_small = B > g_gemv_max_rows && mfma_eligible(L, B, 1, K, N, packed) && workspace != nullptr;
    if (is_f8(precision) && (B <= g_gemv_max_rows || !mfma_eligible(L, B, 1, K, N, packed)))
        return FQL_ERR_BAD_PRECISION;                 // fp8 exists on the MFMA path only: no silent float32 fallback
    if (is_f8(precision) && !mfma_small) return FQL_ERR_WORKSPACE;
    if (B <= 4 && !mfma_small) {
        if ((K % 32 == 0) && aligned16(packed) && aligned16(x) && gemv_lds_bytes(B, K) <= 150 * 1024) {
            switch (B) {
            case 1: return launch_gemv<1>(x, packed, scales, zps, out, K, N, st, bias);
            case 2: return launch_gemv<2>(x, packed, scales, zps, out, K, N, st, bias);
            case 3: return launch_gemv<3>(x, packed, scales, zps, out, K, N, st, bias);
            default: return launch_gemv<4>(x, packed, scales, zps, out, K, N, st, bias);
            }
        }
        return run_generic(x, packed, scales, zps, out, nullptr, nullptr, 1, B, K, N, st, bias);
    }
    if (mfma_eligible(L, B, 1, K, N, packed)) {
        Call c;
        c.x = x; c.f8 = is_f8(precision);
        c.packed = packed; c.scales = scales; c.zps = zps;
        c.out = out; c.bias = bias; c.st = st;
        c.set_shape(1, B, K, N);
        return run_mfma(L, c, workspace, workspace_bytes);
    }
    return run_generic(x, packed, scales, zps, out, nullptr, nullptr, 1, B, K, N, st, bias);
}

int fql_linear_fwd_f32(const float *x, const uint8_t *packed, const float *scales, const float *zps,
                       float *out, int B, int K, int N, int precision, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    return linear_f32_core(x, packed, scales, zps, nullptr, out, B, K, N, precision, workspace, workspace_bytes, stream);
}

int fql_linear_bias_fwd_f32(const float *x, const uint8_t *packed, const float *scales, const float *zps,
                            const float *bias, float *out, int B, int K, int N, int precision, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    return linear_f32_core(x, packed, scales, zps, bias, out, B, K, N, precision, workspace, workspace_bytes, stream);
}


static int moe_entry(const uint8_t *packed, const float *scales, const float *zps, const float *inputs,
                     const int32_t *row_index, int n_src, const int32_t *tokens_per_expert,
                     const int32_t *input_offsets, float *out, int E, int T, int K, int N, int precision,
                     void *workspace, size_t workspace_bytes, void *stream, const float *row_weight = nullptr,
                     const float *bias = nullptr)            // bias [E][N]: added to expert e's rows in the epilogue
{
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (E < 0 || T < 0 || K < 0 || N < 0 || (row_index != nullptr && n_src <= 0)) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (T == 0 || N == 0) return FQL_OK;
    if (!out) return FQL_ERR_NULL_POINTER;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (E == 0 || K == 0) {                           // nothing contributes: all rows zero
        if (bias != nullptr) return FQL_ERR_BAD_SHAPE;    // (as linear_f32_core: not a path worth a kernel)
        return hipMemsetAsync(out, 0, (size_t)T * N * sizeof(float), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    }
    if (!packed || !scales || !zps || !inputs || !tokens_per_expert || !input_offsets) return FQL_ERR_NULL_POINTER;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (mfma_eligible(L, T, E, K, N, packed)) {
        Call c;
        c.x = inputs; c.gather = row_index; c.n_src = n_src; c.f8 = is_f8(precision);
        c.packed = packed; c.scales = scales; c.zps = zps;
        c.out = out; c.bias = bias; c.row_weight = row_weight; c.st = st;
        c.tpe = tokens_per_expert; c.offs = input_offsets;
        c.set_shape(E, T, K, N);
        return run_mfma(L, c, workspace, workspace_bytes);
    }
    if (row_index != nullptr || is_f8(precision) || row_weight != nullptr) return FQL_ERR_ALIGNMENT;     // the fused gather / row weights / fp8 exist on the MFMA path only
    return run_generic(inputs, packed, scales, zps, out, tokens_per_expert, input_offsets, E, T, K, N, st, bias);
}

int fql_moe_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *inputs,
                    const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                    int K, int N, int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    return moe_entry(packed, scales, zps, inputs, nullptr, 0, tokens_per_expert, input_offsets, out, E, T, K, N,
                     precision, workspace, workspace_bytes, stream);
}

int fql_moe_gather_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *tokens,
                           const int32_t *row_index, int n_tokens, const int32_t *tokens_per_expert,
                           const int32_t *input_offsets, float *out, int E, int T, int K, int N, int precision,
                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (!row_index) return FQL_ERR_NULL_POINTER;
    return moe_entry(packed, scales, zps, tokens, row_index, n_tokens, tokens_per_expert, input_offsets, out, E, T, K,
                     N, precision, workspace, workspace_bytes, stream);
}


int fql_moe_gather_scaled_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *tokens,
                                  const int32_t *row_index, int n_tokens, const float *row_weight,
                                  const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                                  int K, int N, int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!row_index || !row_weight) return FQL_ERR_NULL_POINTER;
    if (is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    return moe_entry(packed, scales, zps, tokens, row_index, n_tokens, tokens_per_expert, input_offsets, out, E, T, K,
                     N, precision, workspace, workspace_bytes, stream, row_weight);
}

int fql_native_dtype_supported(int rows, int E, int K, int N, int precision, const void *packed, int grouped)
{
    const int L = limbs_of(precision);
    if (L < 0 || rows <= 0 || E <= 0) return 0;
    if (!grouped && rows <= g_gemv_max_rows) return 0;       // the GEMV path is float32 only
    return mfma_eligible(L, rows, E, K, N, static_cast<const uint8_t *>(packed)) ? 1 : 0;
}

int fql_linear_fwd(const void *x, int in_dtype, const uint8_t *packed, const float *scales, const float *zps, void *out,
                   int out_dtype, int B, int K, int N, int precision, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    return fql_linear_bias_fwd(x, in_dtype, packed, scales, zps, nullptr, out, out_dtype, B, K, N, precision, workspace,
                               workspace_bytes, stream);
}

// fql_linear_fwd with the optional bias of fql_linear_bias_fwd_f32 (the same epilogue add: the kernels take it already)
int fql_linear_bias_fwd(const void *x, int in_dtype, const uint8_t *packed, const float *scales, const float *zps,
                        const float *bias, void *out, int out_dtype, int B, int K, int N, int precision, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    if (in_dtype == FQL_DTYPE_F32 && out_dtype == FQL_DTYPE_F32)
        return bias != nullptr
                   ? fql_linear_bias_fwd_f32(static_cast<const float *>(x), packed, scales, zps, bias,
                                             static_cast<float *>(out), B, K, N, precision, workspace, workspace_bytes, stream)
                   : fql_linear_fwd_f32(static_cast<const float *>(x), packed, scales, zps, static_cast<float *>(out), B,
                                        K, N, precision, workspace, workspace_bytes, stream);
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (B < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (B == 0 || N == 0) return FQL_OK;
    if (!x || !packed || !scales || !zps || !out) return FQL_ERR_NULL_POINTER;
    if (B <= g_gemv_max_rows || !mfma_eligible(L, B, 1, K, N, packed)) return FQL_ERR_DTYPE;   // 16-bit I/O exists on the MFMA path only
    Call c;
    c.x = x; c.in_dtype = in_dtype; c.f8 = is_f8(precision);
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.bias = bias; c.st = static_cast<hipStream_t>(stream);
    c.set_shape(1, B, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

// fql_moe_fwd and, with a bias [E][N], fql_moe_bias_fwd: one body, the bias a member of the call record
static int moe_typed_entry(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                           const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                           int out_dtype, int E, int T, int K, int N, int precision, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    if (in_dtype == FQL_DTYPE_F32 && out_dtype == FQL_DTYPE_F32)
        return moe_entry(packed, scales, zps, static_cast<const float *>(inputs), nullptr, 0, tokens_per_expert,
                         input_offsets, static_cast<float *>(out), E, T, K, N, precision, workspace, workspace_bytes, stream,
                         nullptr, bias);
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !inputs || !tokens_per_expert || !input_offsets || !out) return FQL_ERR_NULL_POINTER;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(L, T, E, K, N, packed)) return FQL_ERR_DTYPE;
    Call c;
    c.x = inputs; c.in_dtype = in_dtype; c.f8 = is_f8(precision);
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.bias = bias; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tokens_per_expert; c.offs = input_offsets;
    c.set_shape(E, T, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

int fql_moe_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E, int T,
                int K, int N, int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    return moe_typed_entry(packed, scales, zps, inputs, in_dtype, tokens_per_expert, input_offsets, nullptr, out, out_dtype,
                           E, T, K, N, precision, workspace, workspace_bytes, stream);
}

// fql_moe_fwd with a per-expert bias [E][N] float32 in the GEMM's epilogue (NULL: fql_moe_fwd exactly)
int fql_moe_bias_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                     const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                     int out_dtype, int E, int T, int K, int N, int precision, void *workspace, size_t workspace_bytes,
                     void *stream)
{
    return moe_typed_entry(packed, scales, zps, inputs, in_dtype, tokens_per_expert, input_offsets, bias, out, out_dtype, E,
                           T, K, N, precision, workspace, workspace_bytes, stream);
}

// ---- rows that are already OCP e4m3 (BASELINE.json configs[4]): re-layout pre-pass + one fp8 MFMA pass
static int f8_entry(const uint8_t *packed, const float *scales, const float *zps, const uint8_t *x8, const float *act_scales,
                    const int32_t *tpe, const int32_t *offs, void *out, int out_dtype, int E, int T, int K, int N,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (!valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !x8 || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tpe, offs, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(1, T, E, K, N, packed)) return FQL_ERR_ALIGNMENT;      // K % 32 == 0, 16-byte aligned weights
    Call c;
    c.x = x8; c.f8 = true;
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tpe; c.offs = offs;
    c.set_shape(E, T, K, N);
    if (workspace == nullptr || !aligned16(workspace)) return FQL_ERR_WORKSPACE;
    c.ws = carve(workspace, 1, T, E, c.Kp, false);
    if (workspace_bytes < c.ws.bytes) return FQL_ERR_WORKSPACE;
    const int mblocks = (tpe == nullptr) ? (T + FQL_MB - 1) / FQL_MB : (T + FQL_MB * E) / FQL_MB;
    const int rblocks = mblocks * (FQL_MB / ACT_ROWS);
    const int zblocks = (tpe != nullptr) ? (T + 255) / 256 : 0;
    const int vec = ((K % 16) == 0 && aligned16(x8)) ? 1 : 0;
    const int rc = launch(act_f8_relayout_kernel, dim3(rblocks + zblocks), dim3(256), 0, c.st, x8, act_scales, nullptr, 0, c.ws.delta,
                          c.ws.rowsum, c.ws.limbs, T, K, c.Kp / FQL_KB, c.MBT, rblocks, out, dtype_bytes(out_dtype), N, tpe, offs, E, vec);
    return rc != FQL_OK ? rc : launch_gemm_f8(choose_cfg_f8(E, T, N, tpe != nullptr), c);
}

int fql_moe_fwd_f8(const uint8_t *packed, const float *scales, const float *zps, const uint8_t *inputs_e4m3,
                   const float *act_scales, const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out,
                   int out_dtype, int E, int T, int K, int N, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!tokens_per_expert || !input_offsets) return FQL_ERR_NULL_POINTER;
    return f8_entry(packed, scales, zps, inputs_e4m3, act_scales, tokens_per_expert, input_offsets, out, out_dtype, E, T, K, N,
                    workspace, workspace_bytes, stream);
}

int fql_linear_fwd_f8(const uint8_t *x_e4m3, const float *act_scales, const uint8_t *packed, const float *scales,
                      const float *zps, void *out, int out_dtype, int B, int K, int N, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    return f8_entry(packed, scales, zps, x_e4m3, act_scales, nullptr, nullptr, out, out_dtype, 1, B, K, N, workspace,
                    workspace_bytes, stream);
}

// ---- per-group scales along K (functional path: csrc/fql_generic.h)
static int group_entry(const float *x, const uint8_t *packed, const float *scales, const float *zps, const float *bias,
                       float *out, const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, int group,
                       void *stream)
{
    if (E <= 0 || T < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (group <= 0 || (group & 1) || K % group != 0) return FQL_ERR_BAD_SHAPE;     // even groups that tile K
    if (T == 0 || N == 0) return FQL_OK;
    if (!x || !packed || !scales || !zps || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tpe, offs, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K == 0) return hipMemsetAsync(out, 0, (size_t)T * N * sizeof(float), st) == hipSuccess ? FQL_OK : FQL_ERR_LAUNCH;
    (void)hipGetLastError();
    if (tpe != nullptr) {
        hipLaunchKernelGGL(zero_uncovered_rows_kernel, dim3(T), dim3(256), 0, st, out, tpe, offs, E, T, N);
        if (hipGetLastError() != hipSuccess) return FQL_ERR_LAUNCH;
    }
    // batches: the float32 matrix-core kernel (fql_group.h); a few rows per group: one wave per output row (fql_generic.h)
    const int groups = tpe == nullptr ? 1 : E;
    const bool batch = g_group_mfma && (T + groups - 1) / groups >= 4 && K % 64 == 0 && group % 32 == 0 &&
                       (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(packed) % 16 == 0) &&
                       (T + 63) / 64 <= 65535;
    const int per = (T + groups - 1) / groups;
    if (tpe == nullptr && T <= 3 && K % 32 == 0 && group % 32 == 0 && aligned16(packed) && aligned16(x) &&
        gemv_lds_bytes(T, K) <= 150 * 1024) {                     // a few rows of one matrix: the GEMV kernel, constants per group
        switch (T) {
        case 1: return launch_gemv<1, true>(x, packed, scales, zps, out, K, N, st, bias, group);
        case 2: return launch_gemv<2, true>(x, packed, scales, zps, out, K, N, st, bias, group);
        default: return launch_gemv<3, true>(x, packed, scales, zps, out, K, N, st, bias, group);
        }
    }
    if (batch && per <= 128 && K % 256 == 0 && (T + 31) / 32 <= 65535)   // few rows per group: 32 x 32 blocks, K split over the waves
        hipLaunchKernelGGL((group_mfma_kernel<true, 1>), dim3((N + 31) / 32, (T + 31) / 32, E), dim3(256), 0, st, x, packed, scales,
                           zps, out, tpe, offs, T, K, N, group, bias);
    else if (batch && (long long)((N + 127) / 128) * ((per + 63) / 64) * groups >= 2LL * compute_units())
        hipLaunchKernelGGL((group_mfma_kernel<false, 2>), dim3((N + 127) / 128, (T + 63) / 64, E), dim3(256), 0, st, x, packed,
                           scales, zps, out, tpe, offs, T, K, N, group, bias);
    else if (batch)
        hipLaunchKernelGGL((group_mfma_kernel<false, 1>), dim3((N + 63) / 64, (T + 63) / 64, E), dim3(256), 0, st, x, packed,
                           scales, zps, out, tpe, offs, T, K, N, group, bias);
    else
        hipLaunchKernelGGL((fused_rows_group_kernel<4>), dim3((N + 3) / 4, E), dim3(256), 0, st, x, packed, scales, zps, out,
                           tpe, offs, T, K, N, group, bias);
    return launched();
}

// ---- per-group scales on the INTEGER matrix cores (csrc/fql_group_i8.h): needs the activation workspace of the per-row
//      path plus a [E][G][N] transpose of the scales and zero points
static bool group_i8_eligible(int L, int E, int T, int K, int N, int group, const void *x, const void *packed, bool grouped)
{
    const int groups = grouped ? E : 1;
    return g_group_i8 && L >= 1 && L <= 3 && K % FQL_KB == 0 && group % 64 == 0 && K % group == 0 && (T + groups - 1) / groups >= (grouped ? g_group_i8_min_rows_grouped : g_group_i8_min_rows) &&
           aligned16(packed) && (reinterpret_cast<uintptr_t>(x) % 4 == 0) && N >= 4 && (T + FQL_MB - 1) / FQL_MB + 1 <= 65535 && E <= 65535;
}

size_t fql_group_workspace_bytes(int E, int T, int K, int N, int group_size, int precision)
{
    const int L = limbs_of(precision);
    if (L < 1 || is_f8(precision) || E <= 0 || T <= 0 || K <= 0 || N <= 0 || group_size <= 0 || K % group_size != 0 || (K % 32) != 0) return 0;
    const Workspace w = carve(nullptr, L, T, E, padded(K), has_residual(L, false));
    return round16(w.bytes) + 2 * round16((size_t)E * N * (K / group_size) * sizeof(float));
}

// The integer path of the per-group entry points for a call record that names the rows (their type, gate|up, activation),
// the output (its type), the bias and the table: the per-row path's pre-pass, the [E][G][N] transpose of the constants behind
// the limb workspace, then group_i8_kernel.  `workspace` holds fql_group_workspace_bytes() bytes.
static int run_group_i8(int L, Call &c, const float *scales, const float *zps, int group, void *workspace)
{
    c.ws = carve(workspace, L, c.T, c.E, c.Kp, has_residual(L, false));
    const int E = c.E, T = c.T, K = c.K, N = c.N, G = K / group;
    float *st_t = reinterpret_cast<float *>(static_cast<char *>(workspace) + round16(c.ws.bytes));
    float *zt_t = reinterpret_cast<float *>(reinterpret_cast<char *>(st_t) + round16((size_t)E * N * G * sizeof(float)));
    return with_limbs(L, [&](auto l) {
        constexpr int LL = decltype(l)::value;
        if (const int rc = launch_act_quant<LL>(c)) return rc;
        const size_t total = (size_t)E * N * G;
        if (const int rc = launch(transpose_ng_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.st, scales, zps, st_t, zt_t, N, G, total))
            return rc;
        return launch(group_i8_kernel<LL>, dim3((N + 127) / 128, (T + FQL_MB - 1) / FQL_MB, E), dim3(256), 0, c.st, c.ws.limbs, c.ws.delta,
                      c.packed, st_t, zt_t, c.out, c.tpe, c.offs, E, T, K, c.MBT, N, group, c.bias, has_residual(L, false) ? 1 : 0, c.out_dtype);
    });
}

static int group_ws_entry(const float *x, const uint8_t *packed, const float *scales, const float *zps, const float *bias,
                          float *out, const int32_t *tpe, const int32_t *offs, int E, int T, int K, int N, int group,
                          int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K < 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (group <= 0 || K <= 0 || K % group != 0) return (K == 0) ? group_entry(x, packed, scales, zps, bias, out, tpe, offs, E, T, K, N, group > 0 ? group : 2, stream) : FQL_ERR_BAD_SHAPE;
    const bool ok = workspace != nullptr && aligned16(workspace) && x && packed && scales && zps && out && T > 0 && N > 0 &&
                    ((tpe == nullptr) == (offs == nullptr)) && (tpe != nullptr || E == 1) &&
                    group_i8_eligible(L, E, T, K, N, group, x, packed, tpe != nullptr) &&
                    workspace_bytes >= fql_group_workspace_bytes(E, T, K, N, group, precision);
    if (!ok) return group_entry(x, packed, scales, zps, bias, out, tpe, offs, E, T, K, N, group, stream);   // float32 paths (and their checks)
    Call c;                                                  // (the pre-pass's view of the call: the GEMM is this path's own)
    c.x = x; c.packed = packed; c.out = out; c.bias = bias; c.tpe = tpe; c.offs = offs; c.st = static_cast<hipStream_t>(stream);
    c.set_shape(E, T, K, N);
    return run_group_i8(L, c, scales, zps, group, workspace);
}

// ---- the typed grouped entry points for per-group scales (fql_moe_group_fwd / fql_moe_group_glu_fwd): float32 / float16 /
//      bfloat16 rows or gate|up rows in, a per-expert bias, any of the three types out.  On the integer path (the
//      eligibility of group_ws_entry) the pre-pass takes the rows as they are and forms h on the fly, as it does for the
//      per-row GEMM, and group_i8_kernel rounds once after the bias.  Off it the float32 kernels of group_entry run between
//      two staging kernels (fql_group.h): widened rows / the float32 h and a float32 result live in the workspace.
size_t fql_moe_group_typed_workspace_bytes(int E, int T, int K, int N, int group_size, int precision)
{
    const int L = limbs_of(precision);
    if (L < 1 || is_f8(precision) || E <= 0 || T <= 0 || K <= 0 || N <= 0 || group_size <= 0 || K % group_size != 0) return 0;
    const size_t stage = round16((size_t)T * K * sizeof(float)) + round16((size_t)T * N * sizeof(float));
    const size_t i8 = fql_group_workspace_bytes(E, T, K, N, group_size, precision);
    return stage > i8 ? stage : i8;
}

static int group_typed_entry(const uint8_t *packed, const float *scales, const float *zps, const void *x, int in_dtype,
                             bool gated, int act, float act_alpha, float act_limit, const int32_t *tpe, const int32_t *offs,
                             const float *bias, void *out, int out_dtype, int E, int T, int K, int N, int group, int precision,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (gated && act != FQL_ACT_SILU &&
        ((act != FQL_ACT_GELU_TANH && act != FQL_ACT_SWIGLU_CLAMP) || !std::isfinite(act_alpha) || !std::isfinite(act_limit) ||
         !(act_limit > 0.0f))) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (group <= 0 || (group & 1) || K % group != 0) return FQL_ERR_BAD_SHAPE;     // even groups that tile K
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !x || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tpe, offs, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!elem_aligned(x, dtype_bytes(in_dtype)) || !elem_aligned(out, dtype_bytes(out_dtype))) return FQL_ERR_ALIGNMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool i8 = workspace != nullptr && aligned16(workspace) && group_i8_eligible(L, E, T, K, N, group, x, packed, tpe != nullptr) &&
                    workspace_bytes >= fql_group_workspace_bytes(E, T, K, N, group, precision);
    if (i8) {
        Call c;
        c.x = x; c.in_dtype = in_dtype; c.gated = gated;
        if (gated && act != FQL_ACT_SILU) { c.act = act; c.act_alpha = act_alpha; c.act_limit = act_limit; }
        c.packed = packed; c.out = out; c.out_dtype = out_dtype; c.bias = bias; c.tpe = tpe; c.offs = offs; c.st = st;
        c.set_shape(E, T, K, N);
        return run_group_i8(L, c, scales, zps, group, workspace);
    }
    // float32 kernels: stage what they cannot read or write themselves
    const bool stage_x = gated || in_dtype != FQL_DTYPE_F32, stage_o = out_dtype != FQL_DTYPE_F32;
    const size_t xb = stage_x ? round16((size_t)T * K * sizeof(float)) : 0, ob = stage_o ? round16((size_t)T * N * sizeof(float)) : 0;
    if (xb + ob > 0 && (workspace == nullptr || !aligned16(workspace) || workspace_bytes < xb + ob)) return FQL_ERR_WORKSPACE;
    float *xf = stage_x ? static_cast<float *>(workspace) : const_cast<float *>(static_cast<const float *>(x));
    float *of = stage_o ? reinterpret_cast<float *>(static_cast<char *>(workspace) + xb) : static_cast<float *>(out);
    auto blocks = [](size_t total) { const size_t b = (total + 255) / 256; return dim3((unsigned)(b < 65536 ? b : 65536)); };
    if (stage_x) {
        const size_t total = (size_t)T * K;
        const int rc = with_dtype(in_dtype, [&](auto d) {
            constexpr int IN = decltype(d)::value;
            return gated ? launch(group_stage_rows_kernel<IN, true>, blocks(total), dim3(256), 0, st, x, xf, K, total, act, act_alpha, act_limit)
                         : launch(group_stage_rows_kernel<IN, false>, blocks(total), dim3(256), 0, st, x, xf, K, total, act, act_alpha, act_limit);
        });
        if (rc) return rc;
    }
    if (const int rc = group_entry(xf, packed, scales, zps, bias, of, tpe, offs, E, T, K, N, group, stream)) return rc;
    if (stage_o) {
        const size_t total = (size_t)T * N;
        return launch(group_round_rows_kernel, blocks(total), dim3(256), 0, st, of, static_cast<unsigned short *>(out), total, out_dtype);
    }
    return FQL_OK;
}

int fql_moe_group_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *inputs, int in_dtype,
                      const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                      int out_dtype, int E, int T, int K, int N, int group_size, int precision, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    return group_typed_entry(packed, scales, zps, inputs, in_dtype, false, FQL_ACT_SILU, 0.0f, 0.0f, tokens_per_expert,
                             input_offsets, bias, out, out_dtype, E, T, K, N, group_size, precision, workspace, workspace_bytes,
                             stream);
}

int fql_moe_group_glu_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up, int in_dtype,
                          const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                          int out_dtype, int E, int T, int K, int N, int group_size, int precision, int activation,
                          float act_alpha, float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    return group_typed_entry(packed, scales, zps, gate_up, in_dtype, true, activation, act_alpha, act_limit, tokens_per_expert,
                             input_offsets, bias, out, out_dtype, E, T, K, N, group_size, precision, workspace, workspace_bytes,
                             stream);
}

int fql_linear_group_ws_fwd_f32(const float *x, const uint8_t *packed, const float *scales, const float *zps,
                                const float *bias, float *out, int B, int K, int N, int group_size, int precision,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    return group_ws_entry(x, packed, scales, zps, bias, out, nullptr, nullptr, 1, B, K, N, group_size, precision, workspace,
                          workspace_bytes, stream);
}

int fql_moe_group_ws_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *inputs,
                             const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                             int K, int N, int group_size, int precision, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    if (!tokens_per_expert || !input_offsets) return FQL_ERR_NULL_POINTER;
    return group_ws_entry(inputs, packed, scales, zps, nullptr, out, tokens_per_expert, input_offsets, E, T, K, N, group_size,
                          precision, workspace, workspace_bytes, stream);
}

int fql_linear_group_fwd_f32(const float *x, const uint8_t *packed, const float *scales, const float *zps,
                             const float *bias, float *out, int B, int K, int N, int group_size, void *stream)
{
    return group_entry(x, packed, scales, zps, bias, out, nullptr, nullptr, 1, B, K, N, group_size, stream);
}

int fql_moe_group_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *inputs,
                          const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                          int K, int N, int group_size, void *stream)
{
    if (!tokens_per_expert || !input_offsets) return FQL_ERR_NULL_POINTER;
    return group_entry(inputs, packed, scales, zps, nullptr, out, tokens_per_expert, input_offsets, E, T, K, N, group_size,
                       stream);
}

int fql_moe_gated_fwd_f32(const uint8_t *packed, const float *scales, const float *zps, const float *gate_up,
                          const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E, int T,
                          int K, int N, int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !gate_up || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(L, T, E, K, N, packed)) return FQL_ERR_ALIGNMENT;   // the fused activation exists on the MFMA path only
    Call c;
    c.x = gate_up; c.gated = true;
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tokens_per_expert; c.offs = input_offsets;
    c.set_shape(E, T, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

// fql_moe_gated_fwd_f32 with an element type for gate_up and one for out: the pre-pass loads 16-bit gate|up rows as they are
// (fql_ffn16.hip), the GEMM's epilogue rounds a 16-bit out once.
int fql_moe_gated_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up, int in_dtype,
                      const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E, int T,
                      int K, int N, int precision, void *workspace, size_t workspace_bytes, void *stream)
{
    if (in_dtype == FQL_DTYPE_F32 && out_dtype == FQL_DTYPE_F32)
        return fql_moe_gated_fwd_f32(packed, scales, zps, static_cast<const float *>(gate_up), tokens_per_expert, input_offsets,
                                     static_cast<float *>(out), E, T, K, N, precision, workspace, workspace_bytes, stream);
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !gate_up || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(L, T, E, K, N, packed)) return FQL_ERR_ALIGNMENT;   // the fused activation exists on the MFMA path only
    if ((reinterpret_cast<uintptr_t>(gate_up) & (dtype_bytes(in_dtype) - 1)) != 0) return FQL_ERR_ALIGNMENT;
    Call c;
    c.x = gate_up; c.in_dtype = in_dtype; c.gated = true;
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tokens_per_expert; c.offs = input_offsets;
    c.set_shape(E, T, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

// fql_moe_gated_fwd with an activation kind: silu is that call; the other kinds take the pre-pass of fql_glu.hip (any element
// type, float32 included) and the same GEMM.
int fql_moe_glu_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up, int in_dtype,
                    const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype, int E, int T,
                    int K, int N, int precision, int activation, float act_alpha, float act_limit, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    if (activation == FQL_ACT_SILU)
        return fql_moe_gated_fwd(packed, scales, zps, gate_up, in_dtype, tokens_per_expert, input_offsets, out, out_dtype, E, T,
                                 K, N, precision, workspace, workspace_bytes, stream);
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if ((activation != FQL_ACT_GELU_TANH && activation != FQL_ACT_SWIGLU_CLAMP) || !std::isfinite(act_alpha) ||
        !std::isfinite(act_limit) || !(act_limit > 0.0f)) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !gate_up || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(L, T, E, K, N, packed)) return FQL_ERR_ALIGNMENT;   // the fused activation exists on the MFMA path only
    if ((reinterpret_cast<uintptr_t>(gate_up) & (dtype_bytes(in_dtype) - 1)) != 0) return FQL_ERR_ALIGNMENT;
    Call c;
    c.x = gate_up; c.in_dtype = in_dtype; c.gated = true;
    c.act = activation; c.act_alpha = act_alpha; c.act_limit = act_limit;
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tokens_per_expert; c.offs = input_offsets;
    c.set_shape(E, T, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

// fql_moe_glu_fwd with a per-expert bias [E][N] float32 in the GEMM's epilogue, for every activation kind (silu included)
// and every element type: the checks of fql_moe_glu_fwd in its order, then the same call record plus the bias.  The record
// decides the pre-pass as it always does (silu: the kernels of fql_act_quant.h / fql_ffn16.hip, the others: fql_glu.hip).
int fql_moe_glu_bias_fwd(const uint8_t *packed, const float *scales, const float *zps, const void *gate_up, int in_dtype,
                         const int32_t *tokens_per_expert, const int32_t *input_offsets, const float *bias, void *out,
                         int out_dtype, int E, int T, int K, int N, int precision, int activation, float act_alpha,
                         float act_limit, void *workspace, size_t workspace_bytes, void *stream)
{
    if (bias == nullptr)
        return fql_moe_glu_fwd(packed, scales, zps, gate_up, in_dtype, tokens_per_expert, input_offsets, out, out_dtype, E, T,
                               K, N, precision, activation, act_alpha, act_limit, workspace, workspace_bytes, stream);
    const int L = limbs_of(precision);
    if (L < 0 || is_f8(precision)) return FQL_ERR_BAD_PRECISION;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (activation != FQL_ACT_SILU &&
        ((activation != FQL_ACT_GELU_TANH && activation != FQL_ACT_SWIGLU_CLAMP) || !std::isfinite(act_alpha) ||
         !std::isfinite(act_limit) || !(act_limit > 0.0f))) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (!valid_dtype(in_dtype) || !valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!packed || !scales || !zps || !gate_up || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (E > 65535) return FQL_ERR_BAD_SHAPE;
    if (!mfma_eligible(L, T, E, K, N, packed)) return FQL_ERR_ALIGNMENT;   // the fused activation exists on the MFMA path only
    if ((reinterpret_cast<uintptr_t>(gate_up) & (dtype_bytes(in_dtype) - 1)) != 0) return FQL_ERR_ALIGNMENT;
    Call c;
    c.x = gate_up; c.in_dtype = in_dtype; c.gated = true;
    if (activation != FQL_ACT_SILU) { c.act = activation; c.act_alpha = act_alpha; c.act_limit = act_limit; }
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.bias = bias; c.st = static_cast<hipStream_t>(stream);
    c.tpe = tokens_per_expert; c.offs = input_offsets;
    c.set_shape(E, T, K, N);
    return run_mfma(L, c, workspace, workspace_bytes);
}

// grad_bias[e][n] = sum over the rows of expert e of grad_rows[t][n] (csrc/fql_bias.hip): every output written
int fql_moe_bias_grad(const void *grad_rows, int dtype, const int32_t *tokens_per_expert, const int32_t *input_offsets,
                      float *grad_bias, int E, int T, int N, void *stream)
{
    if (E < 0 || T < 0 || N < 0 || E > 65535 || N > 0x7fffff00) return FQL_ERR_BAD_SHAPE;
    if (!valid_dtype(dtype)) return FQL_ERR_DTYPE;
    if (E == 0 || N == 0) return FQL_OK;
    if (!grad_bias || (T > 0 && !grad_rows)) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (!elem_aligned(grad_rows, dtype_bytes(dtype)) || !elem_aligned(grad_bias, 4)) return FQL_ERR_ALIGNMENT;
    return fql_bias_grad_launch(grad_rows, dtype, tokens_per_expert, input_offsets, grad_bias, E, T, N,
                                static_cast<hipStream_t>(stream)) == 0 ? FQL_OK : FQL_ERR_LAUNCH;
}

int fql_route_plan_i32(const int32_t *expert_of_slot, int n_slots, int top_k, int E, int32_t *counts,
                       int32_t *offsets, int32_t *token_of_sorted, int32_t *pos_of_slot, void *stream)
{
    if (n_slots < 0 || top_k <= 0 || E <= 0 || E > ROUTE_MAX_EXPERTS) return FQL_ERR_BAD_SHAPE;
    if (!counts || !offsets) return FQL_ERR_NULL_POINTER;
    if (n_slots > 0 && (!expert_of_slot || !token_of_sorted || !pos_of_slot)) return FQL_ERR_NULL_POINTER;
    const size_t lds = (size_t)(ROUTE_THREADS * E + E) * sizeof(int);
    static PerDeviceFlag attr;
    if (!ensure_lds_attr(attr, reinterpret_cast<const void *>(route_plan_kernel),
                         (ROUTE_THREADS * ROUTE_MAX_EXPERTS + ROUTE_MAX_EXPERTS) * (int)sizeof(int)))
        return FQL_ERR_LAUNCH;
    return launch(route_plan_kernel, dim3(1), dim3(ROUTE_THREADS), lds, static_cast<hipStream_t>(stream), expert_of_slot, n_slots,
                  top_k, E, counts, offsets, token_of_sorted, pos_of_slot);
}

int fql_combine_f32(const float *y, const int32_t *pos_of_slot, const float *weights, float *out, int T, int top_k,
                    int N, int R, void *stream)
{
    if (T < 0 || top_k <= 0 || N < 0 || R < 0) return FQL_ERR_BAD_SHAPE;
    if (T == 0 || N == 0) return FQL_OK;
    if (!y || !pos_of_slot || !out || R == 0) return FQL_ERR_NULL_POINTER;      // weights == NULL: rows already weighted, pure gather-add
    if (T > 65535) return FQL_ERR_BAD_SHAPE;                 // grid.y
    return launch_combine(y, FQL_DTYPE_F32, pos_of_slot, weights, nullptr, nullptr, out, FQL_DTYPE_F32, T, top_k, N, R,
                          static_cast<hipStream_t>(stream));
}

int fql_combine_bwd_f32(const float *grad_out, const float *y, const int32_t *pos_of_slot, const float *weights,
                        float *grad_y, float *grad_weights, int T, int top_k, int N, int rows, void *stream)
{
    if (T < 0 || top_k <= 0 || N < 0 || rows < 0) return FQL_ERR_BAD_SHAPE;
    if (T == 0) return FQL_OK;
    if (rows == 0) return FQL_ERR_BAD_SHAPE;                 // slots with no rows to point at
    if (!pos_of_slot) return FQL_ERR_NULL_POINTER;
    if (N > 0 && (!grad_out || !grad_y)) return FQL_ERR_NULL_POINTER;
    if (grad_weights != nullptr && N > 0 && !y) return FQL_ERR_NULL_POINTER;
    if (N == 0 && grad_weights == nullptr) return FQL_OK;
    return launch_combine_bwd(grad_out, FQL_DTYPE_F32, y, pos_of_slot, weights, nullptr, nullptr, FQL_DTYPE_F32, grad_y,
                              grad_weights, nullptr, nullptr, T, top_k, N, rows, static_cast<hipStream_t>(stream));
}

// fql_combine_f32 with an element type for y / addend and one for out, and an optional weighted addend behind the slot
// terms (csrc/fql_routing.h, combine_kernel).  The order of the return codes is part of the ABI (include/fql_int4.h).
int fql_combine(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights, const void *addend,
                const float *addend_weight, void *out, int out_dtype, int T, int top_k, int N, int R, void *stream)
{
    return combine_entry(y, in_dtype, pos_of_slot, weights, addend, addend_weight, out, out_dtype, T, top_k, N, R, stream,
                         false);
}

int fql_combine_bwd(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot, const float *weights,
                    const void *addend, const float *addend_weight, int in_dtype, void *grad_y, float *grad_weights,
                    void *grad_addend, float *grad_addend_weight, int T, int top_k, int N, int rows, void *stream)
{
    return combine_bwd_entry(grad_out, out_dtype, y, pos_of_slot, weights, addend, addend_weight, in_dtype, grad_y,
                             grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows, stream, false);
}

// The plan and the combine pair with slots that go nowhere (FQL_VERSION 320; include/fql_int4.h)
int fql_route_plan_capped_i32(const int32_t *expert_of_slot, int n_slots, int top_k, int E, const uint8_t *token_mask,
                              int capacity, int32_t *demand, int32_t *counts, int32_t *offsets, int32_t *token_of_sorted,
                              int32_t *pos_of_slot, void *stream)
{
    if (n_slots < 0 || top_k <= 0 || E <= 0 || E > ROUTE_MAX_EXPERTS || capacity < 0 || n_slots % top_k != 0)
        return FQL_ERR_BAD_SHAPE;
    if (!demand || !counts || !offsets) return FQL_ERR_NULL_POINTER;
    if (n_slots > 0 && (!expert_of_slot || !token_of_sorted || !pos_of_slot)) return FQL_ERR_NULL_POINTER;
    const size_t lds = (size_t)(ROUTE_THREADS * E + E + 1) * sizeof(int);
    static PerDeviceFlag attr;
    if (!ensure_lds_attr(attr, reinterpret_cast<const void *>(route_plan_capped_kernel),
                         (ROUTE_THREADS * ROUTE_MAX_EXPERTS + ROUTE_MAX_EXPERTS + 1) * (int)sizeof(int)))
        return FQL_ERR_LAUNCH;
    return launch(route_plan_capped_kernel, dim3(1), dim3(ROUTE_THREADS), lds, static_cast<hipStream_t>(stream), expert_of_slot,
                  n_slots, top_k, E, token_mask, capacity, demand, counts, offsets, token_of_sorted, pos_of_slot);
}

int fql_combine_sparse(const void *y, int in_dtype, const int32_t *pos_of_slot, const float *weights, const void *addend,
                       const float *addend_weight, void *out, int out_dtype, int T, int top_k, int N, int R, void *stream)
{
    return combine_entry(y, in_dtype, pos_of_slot, weights, addend, addend_weight, out, out_dtype, T, top_k, N, R, stream,
                         true);
}

int fql_combine_sparse_bwd(const void *grad_out, int out_dtype, const void *y, const int32_t *pos_of_slot,
                           const float *weights, const void *addend, const float *addend_weight, int in_dtype, void *grad_y,
                           float *grad_weights, void *grad_addend, float *grad_addend_weight, int T, int top_k, int N,
                           int rows, void *stream)
{
    return combine_bwd_entry(grad_out, out_dtype, y, pos_of_slot, weights, addend, addend_weight, in_dtype, grad_y,
                             grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows, stream, true);
}

int fql_router_topk_fwd(const void *logits, int logits_dtype, int T, int E, int top_k, int renormalize, int32_t *indices,
                        float *weights, float *probs, void *stream)
{
    if (const int rc = router_shape_check(logits_dtype, T, E, top_k)) return rc;
    if (T == 0) return FQL_OK;
    if (!logits || !indices || !weights) return FQL_ERR_NULL_POINTER;                 // probs == NULL: not wanted
    return launch_router_fwd(logits, logits_dtype, T, E, top_k, 0, nullptr, 1, 1, 1, renormalize, 1.0f, indices, weights, probs,
                             static_cast<hipStream_t>(stream));
}

int fql_router_topk_bwd(const void *logits, int logits_dtype, const int32_t *indices, const float *grad_weights,
                        const float *grad_probs, void *grad_logits, int T, int E, int top_k, int renormalize, void *stream)
{
    if (const int rc = router_shape_check(logits_dtype, T, E, top_k)) return rc;
    if (T == 0) return FQL_OK;
    if (!logits || !indices || !grad_logits) return FQL_ERR_NULL_POINTER;             // either gradient may be NULL
    return launch_router_bwd(logits, logits_dtype, indices, grad_weights, grad_probs, grad_logits, T, E, top_k, 0, renormalize,
                             1.0f, static_cast<hipStream_t>(stream));
}

int fql_router_score_topk_fwd(const void *logits, int logits_dtype, int T, int E, int top_k, int scoring,
                              const float *select_bias, int n_group, int topk_group, int group_top, int renormalize,
                              float scale, int32_t *indices, float *weights, float *scores, void *stream)
{
    if (const int rc = router_score_shape_check(logits_dtype, T, E, top_k, scoring, n_group, topk_group, group_top, scale))
        return rc;
    if (T == 0) return FQL_OK;
    if (!logits || !indices || !weights) return FQL_ERR_NULL_POINTER;     // select_bias, scores == NULL: none / not wanted
    return launch_router_fwd(logits, logits_dtype, T, E, top_k, scoring, select_bias, n_group, topk_group, group_top,
                             renormalize, scale, indices, weights, scores, static_cast<hipStream_t>(stream));
}

int fql_router_score_topk_bwd(const void *logits, int logits_dtype, const int32_t *indices, const float *grad_weights,
                              const float *grad_scores, void *grad_logits, int T, int E, int top_k, int scoring,
                              int renormalize, float scale, void *stream)
{
    if (const int rc = router_score_shape_check(logits_dtype, T, E, top_k, scoring, 1, 1, 1, scale)) return rc;
    if (T == 0) return FQL_OK;
    if (!logits || !indices || !grad_logits) return FQL_ERR_NULL_POINTER;             // either gradient may be NULL
    return launch_router_bwd(logits, logits_dtype, indices, grad_weights, grad_scores, grad_logits, T, E, top_k, scoring,
                             renormalize, scale, static_cast<hipStream_t>(stream));
}

int fql_regroup_index_i32(const int32_t *recv_counts, int G, int EL, int32_t *tokens_per_expert,
                          int32_t *input_offsets, int32_t *gather, int32_t *scatter, void *stream)
{
    if (G <= 0 || EL <= 0 || (size_t)G * EL > 8192) return FQL_ERR_BAD_SHAPE;
    if (!recv_counts || !tokens_per_expert || !input_offsets || !gather || !scatter) return FQL_ERR_NULL_POINTER;
    hipLaunchKernelGGL(regroup_index_kernel, dim3(1), dim3(256), (size_t)2 * G * EL * sizeof(int),
                       static_cast<hipStream_t>(stream), recv_counts, G, EL, tokens_per_expert, input_offsets, gather,
                       scatter);
    return launched();
}

int fql_unpack_u8(const uint8_t *packed, uint8_t *q, size_t nbytes, void *stream)
{
    if (nbytes == 0) return FQL_OK;
    if (!packed || !q) return FQL_ERR_NULL_POINTER;
    size_t blocks = (nbytes / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(unpack_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       packed, q, nbytes);
    return launched();
}

int fql_dequantize_f32(const uint8_t *packed, const float *scales, const float *zps, float *w, int N, int K,
                       void *stream)
{
    if (N < 0 || K < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (N == 0 || K == 0) return FQL_OK;
    if (!packed || !scales || !zps || !w) return FQL_ERR_NULL_POINTER;
    hipLaunchKernelGGL(dequantize_kernel, dim3((N + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), packed,
                       scales, zps, w, N, K);
    return launched();
}

size_t fql_act_limb_bytes(int T, int E, int K, int precision)
{
    const int L = limbs_of(precision);
    if (L < 0 || T <= 0 || E <= 0 || K <= 0) return 0;
    return (has_residual(L, is_f8(precision)) ? 2 : 1) * limb_bytes(L, T, E, padded(K));
}

size_t fql_gemm_scratch_bytes(int precision)
{
    const int L = limbs_of(precision);
    return (L >= 0 && has_residual(L, is_f8(precision))) ? res_scratch_bytes() : 0;
}

int fql_act_quant_f32(const float *x, int8_t *limbs, float *delta, int32_t *rowsum,
                      const int32_t *tokens_per_expert, const int32_t *input_offsets, int E, int T, int K,
                      int precision, void *stream)
{
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (T < 0 || K <= 0 || E <= 0) return FQL_ERR_BAD_SHAPE;
    if (T == 0) return FQL_OK;
    if (!x || !limbs || !delta || !rowsum) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if (!aligned16(limbs)) return FQL_ERR_ALIGNMENT;
    Call c;
    c.x = x; c.f8 = is_f8(precision); c.tpe = tokens_per_expert; c.offs = input_offsets; c.st = static_cast<hipStream_t>(stream);
    c.set_shape(E, T, K, 0);
    c.ws.limbs = limbs; c.ws.delta = delta; c.ws.rowsum = rowsum;
    return with_limbs(L, [&](auto l) { return launch_act_quant<decltype(l)::value>(c); });
}

int fql_quantize_rows_f32(const float *w, uint8_t *packed, float *scales, float *zps, int N, int K, void *stream)
{
    if (N < 0 || K < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (N == 0 || K == 0) return FQL_OK;
    if (!w || !packed || !scales || !zps) return FQL_ERR_NULL_POINTER;
    hipLaunchKernelGGL(quantize_rows_kernel, dim3(N), dim3(256), 0, static_cast<hipStream_t>(stream), w, N, K, packed,
                       scales, zps);
    return launched();
}

int fql_quantize_tensor_f32(const float *w, uint8_t *packed, float *scales, float *zps, float *scratch, int N, int K,
                            void *stream)
{
    if (N < 0 || K < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (N == 0 || K == 0) return FQL_OK;
    if (!w || !packed || !scales || !zps || !scratch) return FQL_ERR_NULL_POINTER;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(row_minmax_kernel, dim3(N), dim3(256), 0, st, w, N, K, scratch, scratch + N);
    hipLaunchKernelGGL(tensor_scale_kernel, dim3(1), dim3(256), 0, st, scratch, scratch + N, N, scales, zps);
    hipLaunchKernelGGL(quantize_given_kernel, dim3(N), dim3(256), 0, st, w, N, K, scales, zps, packed);
    return launched();
}

// `bias` [E][N] and `row_weight` [T] are optional.  The kernels take the bias as a pointer, but read a row's weight from the
// plane behind delta's set(s), where the pre-pass of the product path leaves it: `row_weight` must BE that plane.
static int gemm_i8_entry(int cfg, const int8_t *limbs, const float *delta, const int32_t *rowsum,
                         const uint8_t *packed, const float *scales, const float *zps,
                         const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                         const float *bias, const float *row_weight, int E, int T,
                         int K, int N, int precision, void *stream, void *scratch, size_t scratch_bytes)
{
    const int L = limbs_of(precision);
    if (L < 0) return FQL_ERR_BAD_PRECISION;
    if (!valid_dtype(out_dtype)) return FQL_ERR_DTYPE;
    if (E <= 0 || T < 0 || K <= 0 || N < 0) return FQL_ERR_BAD_SHAPE;
    if (K & 1) return FQL_ERR_ODD_K;
    if (T == 0 || N == 0) return FQL_OK;
    if (!limbs || !delta || !rowsum || !packed || !scales || !zps || !out) return FQL_ERR_NULL_POINTER;
    if (const int rc = table_check(tokens_per_expert, input_offsets, E)) return rc;
    if ((K % 32) != 0 || !aligned16(packed) || !aligned16(limbs)) return FQL_ERR_ALIGNMENT;
    if (!mfma_addressable(L, T, E, K, N)) return FQL_ERR_BAD_SHAPE;
    if (row_weight != nullptr && row_weight != delta + (size_t)(has_residual(L, is_f8(precision)) ? 2 : 1) * T) return FQL_ERR_ALIGNMENT;
    if (is_f8(precision)) {
        if (cfg < 0) cfg = choose_cfg_f8(E, T, N, tokens_per_expert != nullptr);
        if (!valid_cfg_f8(cfg)) return FQL_ERR_BAD_SHAPE;
    } else {
        if (cfg < 0) cfg = choose_cfg(L, E, T, K, N, tokens_per_expert != nullptr);
        if (!valid_cfg(cfg, L)) return FQL_ERR_BAD_SHAPE;
    }
    Call c;
    c.packed = packed; c.scales = scales; c.zps = zps;
    c.out = out; c.out_dtype = out_dtype; c.bias = bias; c.row_weight = row_weight;
    c.tpe = tokens_per_expert; c.offs = input_offsets; c.st = static_cast<hipStream_t>(stream);
    c.set_shape(E, T, K, N);
    c.ws.limbs = const_cast<int8_t *>(limbs);
    c.ws.delta = const_cast<float *>(delta);
    c.ws.rowsum = const_cast<int32_t *>(rowsum);
    // without (enough) scratch the residual pass of heavy-tailed rows is skipped: the result is then the plain 8L-1 bit one
    c.ws.scratch = (has_residual(L, is_f8(precision)) && scratch != nullptr && aligned16(scratch) && scratch_bytes >= res_scratch_bytes())
                       ? static_cast<float *>(scratch) : nullptr;
    if (is_f8(precision)) return launch_gemm_f8(cfg, c);
    return with_limbs(L, [&](auto l) { return launch_gemm<decltype(l)::value>(cfg, c); });
}

int fql_gemm_i8_f32(const int8_t *limbs, const float *delta, const int32_t *rowsum, const uint8_t *packed,
                    const float *scales, const float *zps, const int32_t *tokens_per_expert,
                    const int32_t *input_offsets, float *out, int E, int T, int K, int N, int precision,
                    void *stream, void *scratch, size_t scratch_bytes)
{
    return gemm_i8_entry(-1, limbs, delta, rowsum, packed, scales, zps, tokens_per_expert, input_offsets, out, FQL_DTYPE_F32,
                         nullptr, nullptr, E, T, K, N, precision, stream, scratch, scratch_bytes);
}

// Tuning hooks (include/fql_int4_tune.h, not part of the drop-in boundary): the same call with an explicit tile configuration id.
FQL_API int fql_tune_gemm_i8_f32(int cfg, const int8_t *limbs, const float *delta, const int32_t *rowsum,
                                 const uint8_t *packed, const float *scales, const float *zps,
                                 const int32_t *tokens_per_expert, const int32_t *input_offsets, float *out, int E,
                                 int T, int K, int N, int precision, void *stream, void *scratch, size_t scratch_bytes)
{
    if (!(precision == FQL_PRECISION_FP8 ? valid_cfg_f8(cfg) : valid_cfg(cfg, limbs_of(precision)))) return FQL_ERR_BAD_SHAPE;
    return gemm_i8_entry(cfg, limbs, delta, rowsum, packed, scales, zps, tokens_per_expert, input_offsets, out, FQL_DTYPE_F32,
                         nullptr, nullptr, E, T, K, N, precision, stream, scratch, scratch_bytes);
}

// ... and with the whole epilogue: output element type, optional bias [E][N], optional row weight [T] (the plane behind delta)
FQL_API int fql_tune_gemm_i8(int cfg, const int8_t *limbs, const float *delta, const int32_t *rowsum,
                             const uint8_t *packed, const float *scales, const float *zps,
                             const int32_t *tokens_per_expert, const int32_t *input_offsets, void *out, int out_dtype,
                             const float *bias, const float *row_weight, int E, int T, int K, int N, int precision,
                             void *stream, void *scratch, size_t scratch_bytes)
{
    if (!(precision == FQL_PRECISION_FP8 ? valid_cfg_f8(cfg) : valid_cfg(cfg, limbs_of(precision)))) return FQL_ERR_BAD_SHAPE;
    return gemm_i8_entry(cfg, limbs, delta, rowsum, packed, scales, zps, tokens_per_expert, input_offsets, out, out_dtype,
                         bias, row_weight, E, T, K, N, precision, stream, scratch, scratch_bytes);
}

#if defined(FQL_TRACE)
FQL_API int fql_debug_trace_act(unsigned long long *dst)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fql_trace_act), sizeof(unsigned long long) * 16 * 16) == hipSuccess ? 0 : -1;
}
FQL_API int fql_debug_trace_wide(unsigned long long *dst)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fql_trace_wide), sizeof(unsigned long long) * 8 * 64) == hipSuccess ? 0 : -1;
}
FQL_API int fql_debug_trace(unsigned long long *dst)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fql_trace_buf), sizeof(unsigned long long) * 8 * 64) == hipSuccess ? 0 : -1;
}
#endif
FQL_API int fql_tune_set_act_single_rows(int rows) { const int old = g_act_single_rows; if (rows >= 0) g_act_single_rows = rows; return old; }
FQL_API int fql_tune_set_balance_tiles(int on) { const int old = g_balance_tiles; g_balance_tiles = on ? 1 : 0; return old; }
FQL_API int fql_tune_set_group_mfma(int on) { const int old = g_group_mfma; g_group_mfma = on ? 1 : 0; return old; }
FQL_API int fql_tune_set_group_i8_min_rows(int rows) { const int old = g_group_i8_min_rows; if (rows >= 1) { g_group_i8_min_rows = rows; g_group_i8_min_rows_grouped = rows; } return old; }
FQL_API int fql_tune_set_group_i8(int on) { const int old = g_group_i8; g_group_i8 = on ? 1 : 0; return old; }
FQL_API int fql_tune_set_gemv_max_rows(int rows) { const int old = g_gemv_max_rows; if (rows >= 0 && rows <= 4) g_gemv_max_rows = rows; return old; }
FQL_API int fql_tune_num_configs(void) { return FQL_NUM_CFG; }
FQL_API int fql_tune_is_config(int cfg, int precision)
{
    const int L = limbs_of(precision);
    if (L < 0) return 0;
    return (is_f8(precision) ? valid_cfg_f8(cfg) : valid_cfg(cfg, L)) ? 1 : 0;
}
FQL_API int fql_tune_num_rows32_configs(void) { return FQL_NUM_ROWS32; }
FQL_API int fql_tune_num_rows16_configs(void) { return FQL_NUM_ROWS16; }
FQL_API int fql_tune_num_w4_configs(void) { return FQL_NUM_W4; }
// which tile configuration the product path picks for a shape (ids as in fql_tune_gemm_i8_f32; bench.py labels its roofline with it)
FQL_API int fql_tune_chosen_cfg(int precision, int E, int T, int K, int N, int grouped)
{
    const int L = limbs_of(precision);
    if (L < 0) return -1;
    return is_f8(precision) ? choose_cfg_f8(E, T, N, grouped != 0) : choose_cfg(L, E, T, K, N, grouped != 0);
}
FQL_API int fql_tune_set_compute_units(int n) { const int old = g_cu_cap; g_cu_cap = n > 0 ? (n < 8 ? 8 : n - n % 8) : 0; return old; }
FQL_API int fql_tune_set_fused(int on) { const int old = g_fused; g_fused = on ? 1 : 0; return old; }
FQL_API int fql_tune_set_fused_spin(int polls) { const int old = g_fused_spin; if (polls >= 0) g_fused_spin = polls; return old; }
FQL_API int fql_tune_set_w4(int on) { const int old = g_use_w4; g_use_w4 = on ? 1 : 0; return old; }


}  // extern "C"
