// Activation pre-pass of the MFMA path: float32 rows -> signed 8-bit limbs of a per-row
// fixed-point value, written in the layout the GEMM's matrix-core A operand wants.
//
//   x[t][k] ~= delta[t] * X[t][k],   X = sum_l 256^l * a_l,   a_l in [-128, 127]  (balanced digits)
//   delta[t] = 2^e, the smallest power of two with rint(max_k |x[t][k]| / 2^e) <= LIM(L)
//   rowsum[l][t] = sum_k a_l[t][k]      (folds the zero-point: sum_k (q-zp) a = sum q a - zp * rowsum)
//
// Limb layout ("fragment native"):  limbs[l][kb][mb][ks][lane][16 B]
//   kb  = k / 256                      weight-stage block (FQL_KB)
//   mb  = p / 32, p = padded row       expert e's rows start at pbase_e = sum_{e'<e} roundup(cnt_e', 32)
//   ks  = 0..7                         the 32-deep MFMA k-step inside the block
//   lane = g*32 + (p & 31)             exactly the lane that supplies row p to v_mfma_i32_32x32x32_i8
//   so one wave's A fragment for (l, kb, mb, ks) is 1 KiB contiguous: a single coalesced
//   buffer_load_dwordx4, no LDS.  Which 16 k a lane holds follows the weight side: lane group g of
//   step ks = 2v+b pairs with bytes [8b, 8b+8) of 16-byte chunk c = 2v+g of the weight row's 128-byte
//   stage segment, i.e. k = 32c + 16b + [0,16) of the block; inside every aligned group of 8 the order
//   is (0,2,4,6,1,3,5,7), the order the in-register nibble unpack (unpack8) produces.
//   Columns K..Kp-1 are zero.
//
// HBM-bound: reads T*K*4 bytes once, writes L*T*Kp bytes as full 128-byte lines.  One launch.
#pragma once
#include "fql_common.h"
#include <math.h>

// Fused dispatch: when `gather` is given, grouped row t is read from token row
// gather[t] of x (the sort-by-expert permutation of routing.py:117-149), so the [T*top_k, K] gathered
// copy of the activations is never materialised.  Indices are clamped into [0, n_src).
__device__ __forceinline__ int source_row(const int32_t *gather, int n_src, int t)
{
    if (gather == nullptr) return t;
    int s = gather[t];
    s = s < 0 ? 0 : s;
    return s < n_src ? s : n_src - 1;
}

template <int L> struct LimbLimit;
template <> struct LimbLimit<1> { static constexpr int value = 127; };
template <> struct LimbLimit<2> { static constexpr int value = 127 * 256 + 127; };
template <> struct LimbLimit<3> { static constexpr int value = 127 * 65536 + 127 * 256 + 127; };

template <int L>
__device__ __forceinline__ int act_exponent(float m)
{
    if (m == 0.0f) return 0;
    int ex;
    (void)frexpf(m, &ex);                 // m = f * 2^ex, f in [0.5, 1)
    int e = (ex - 1) - (8 * L - 2);       // m * 2^-e in [2^(8L-2), 2^(8L-1))
    e = e < -126 ? -126 : e;              // keep 2^e and 2^-e normal
    if (rintf(m * ldexpf(1.0f, -e)) > (float)LimbLimit<L>::value) e += 1;
    return e;
}

// ---- single-launch pre-pass.  One 256-thread workgroup owns ACT_ROWS (4) consecutive GROUPED rows t end to end:
//      thread t holds row r = t % ACT_ROWS and the 16-float chunks ch = t / ACT_ROWS + ACT_COLS j of that row
//      (K <= 4096: the workgroup's whole 64 KiB of x sits in registers, read from HBM exactly once, all loads in
//      flight together).  The order of the prologue is the point (in-kernel clock stamps, tools/trace_step.py: the
//      workgroup is a latency chain): the expert table's two loads are issued first, then ALL loads of x, and only
//      then the table is scanned for the padded row p of each grouped row (p = padded rows of the earlier experts +
//      t - first row of t's expert) -- the lookup used to sit in front of the loads (1.3 of 7.1 us).  Padding rows
//      (an expert's rows are padded to a multiple of 32) are never written: a matrix-core output row depends on its
//      own activation row only, and the GEMM stores valid rows only.
//      Row max -> DPP rotations inside the 16-lane rows + one LDS combine -> delta; then every 16-float chunk
//      becomes one 16-byte limb chunk per limb: k = 16 ch of the row IS lane group g / k-step ks of the fragment
//      layout (see the header comment), and the rows of a workgroup are neighbouring lanes of the fragment, so
//      each group of ACT_ROWS threads stores ACT_ROWS x 16 contiguous bytes.  No LDS staging of data, no second
//      launch.
//      Limb row sums by v_dot4 against 0x01010101, reduced the same way as the max.
//      Rows longer than 4096 are processed in 4096-k slabs: pass 1 streams all slabs for the max, pass 2
//      re-reads them (L2 hits: the workgroup just read them).
//      Workgroups with blockIdx.x >= rblocks (MoE entry point only) zero-fill the rows of `out` no expert
//      covers (reference semantics: torch::zeros, csrc/moe_int4_kernel.cu:109).
#ifndef ACT_ROWS
#define ACT_ROWS 4                  // measured: 8 rows 15.0 us, 4 rows 12.4 us, 2 rows 12.4 us at configs[2]
#endif
#define ACT_COLS (256 / ACT_ROWS)   // chunk columns of the 256 threads
#define ACT_CH (256 / ACT_COLS)     // chunks per thread per slab: ACT_COLS x ACT_CH = 256 chunks = 4096 k

// IN: element type of x (FQL_DTYPE_F32 / _F16 / _BF16); 16-bit inputs are widened in registers (exact), so the
// limbs are the ones the float32 copy of x would give.  out_es: bytes per element of `out` (zero fill only).
template <int IN>
__device__ __forceinline__ float act_widen(unsigned short h)
{
    if (IN == 1) { _Float16 f; __builtin_memcpy(&f, &h, 2); return (float)f; }
    return __uint_as_float((uint32_t)h << 16);
}

// GATE: the source row is [gate (K) | up (K)] and the value that gets quantised is
// silu(gate[k]) * up[k] -- the elementwise step between the two GEMMs of a gated FFN expert fused into the
// second GEMM's pre-pass, so the [T, K] hidden activation is never materialised.
// A 16-bit gate|up row is widened in registers first, so the limbs are those of the float32 call on the widened row.
// (act_silu_mul itself lives in fql_common.h: the adapter kernels of fql_lora.h form the same h from the same function.)
// GLU (with GATE): the value is act_glu_mul(kind, alpha, limit, gate[k], up[k]) instead, the kind and its two floats
// wave-uniform kernel arguments (act_glu_kernel): GeGLU and the clamped SwiGLU, one instantiation for both.

// ---- pieces shared by the pre-pass kernels (this file and fql_act_f8.h)
// Coverage workgroups (MoE entry points only): zero-fill the rows of `out` no expert covers, 256 rows each
// (reference semantics: torch::zeros, csrc/moe_int4_kernel.cu:109).  ROWS: the threads of the workgroup, one row each.
template <int ROWS = 256>
__device__ __forceinline__ void act_zero_uncovered(int block, void *__restrict__ out, int out_es, int N,
                                                   const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
                                                   int E, int T)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = block * ROWS + tid;
    bool covered = false;
    int cp = 0, ct = 0;
    for (int base = 0; base < E; base += 64) {
        const ExpertLane xl = expert_chunk(tpe, offs, E, T, FQL_MB, base, lane, cp, ct);
        const int ne = (E - base) < 64 ? (E - base) : 64;
        for (int i = 0; i < ne; ++i) {
            const int lo = __shfl(xl.lo, i, 64), cnt = __shfl(xl.cnt, i, 64);
            covered |= (t >= lo && t < lo + cnt);
        }
    }
    if (t < T && !covered) {                             // rare path: rows no expert owns
        if (out_es == 4) {
            float *orow = reinterpret_cast<float *>(out) + (size_t)t * N;
            for (int i = 0; i < N; ++i) orow[i] = 0.0f;
        } else {
            unsigned short *orow = reinterpret_cast<unsigned short *>(out) + (size_t)t * N;
            for (int i = 0; i < N; ++i) orow[i] = 0;
        }
    }
}

// (fql_act_f8.h: workgroups in PADDED-row order)  Token row of each of the workgroup's ACT_ROWS padded rows p0 .. (-1: padding) into s_tok; returns the number of
// padded rows in use.  The caller synchronises before reading s_tok.
struct ActLookupShared { int lo[64], cnt[64], pad[64], total; };
__device__ __forceinline__ int act_token_rows(int p0, int rows, int *s_tok, ActLookupShared &sh,
                                              const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
                                              int E, int T)
{
    const int tid = threadIdx.x;
    int total;
    if (tpe == nullptr) {
        if (tid < rows) s_tok[tid] = (p0 + tid < T) ? p0 + tid : -1;
        total = (T + FQL_MB - 1) / FQL_MB * FQL_MB;
    } else {
        int t_found = -1;
        int cp = 0, ct = 0;
        total = 0;
        for (int base = 0; base < E; base += 64) {
            if (tid < 64) {
                const ExpertLane xl = expert_chunk(tpe, offs, E, T, FQL_MB, base, tid, cp, ct);
                sh.lo[tid] = xl.lo; sh.cnt[tid] = xl.cnt; sh.pad[tid] = xl.pad_excl;
                if (tid == 0) sh.total = cp;              // running padded-row total
            }
            __syncthreads();
            if (tid < rows && t_found < 0) {
                const int p = p0 + tid;
                const int ne = (E - base) < 64 ? (E - base) : 64;
                for (int i = 0; i < ne; ++i) {
                    const int rel = p - sh.pad[i];
                    if (rel >= 0 && rel < sh.cnt[i]) { t_found = sh.lo[i] + rel; break; }
                }
            }
            total = sh.total;
            __syncthreads();
        }
        if (tid < rows) s_tok[tid] = t_found;
    }
    return total;
}

// Padded row p of each of the workgroup's grouped rows t0 .. t0 + rows - 1 into s_p (-1: no expert owns the row, or it is
// past T).  Wave 0 only; lane i owns expert base + i, (off_raw, cnt_raw) are the first chunk's table entries, loaded by the
// caller (expert_chunk_load) before its loads of x.  One ballot per row instead of a serial walk over the experts.
// s_e (optional): the expert of each row (0 for the linear op, -1 where s_p is -1).
// The caller synchronises before reading s_p.
__device__ __forceinline__ void act_padded_rows(int t0, int rows, int *s_p, int off_raw, int cnt_raw,
                                                const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
                                                int E, int T, int lane, int *s_e = nullptr)
{
    if (lane < rows) s_p[lane] = (tpe == nullptr && t0 + lane < T) ? t0 + lane : -1;
    if (s_e != nullptr && lane < rows) s_e[lane] = (tpe == nullptr && t0 + lane < T) ? 0 : -1;
    if (tpe == nullptr) return;
    int cp = 0, ct = 0;
    for (int base = 0; base < E; base += 64) {
        if (base > 0) expert_chunk_load(tpe, offs, E, base, lane, off_raw, cnt_raw);
        const ExpertLane xl = expert_chunk_scan(off_raw, cnt_raw, T, FQL_MB, lane, cp, ct);
        for (int rr = 0; rr < rows; ++rr) {
            const int t = t0 + rr, rel = t - xl.lo;
            const unsigned long long hit = __ballot(t < T && rel >= 0 && rel < xl.cnt);
            if (hit) {                                        // (ranges do not overlap: at most one expert per row)
                const int src = __ffsll((long long)hit) - 1;
                const int pv = wave_bcast(xl.pad_excl + rel, src);
                if (lane == 0) s_p[rr] = pv;
                if (s_e != nullptr && lane == 0) s_e[rr] = base + src;
            }
        }
    }
}

// Reduction over the lanes of one wave that hold the same row (lanes = r mod R): rotations inside the 16-lane DPP rows
// (R <= 8: every lane of a row ends with the result of its residue class), leaving one partial per 16-lane row.
template <int R, typename Op>
__device__ __forceinline__ int act_row16_reduce(int v, Op op)
{
    if (R <= 8) v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));   // row_ror:8
    if (R <= 4) v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));   // row_ror:4
    if (R <= 2) v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false));   // row_ror:2
    if (R <= 1) v = op(v, __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false));   // row_ror:1
    return v;
}

// F8OUT (L = 1): the row is scaled by 448 / max|x| and rounded to OCP e4m3 (round to nearest even) instead of being
// split into int8 limbs -- the "fp8 activations" mode (FQL_PRECISION_FP8, BASELINE.json configs[4]).  delta[t] is the
// float32 quotient max|x| / 448, the stored byte the conversion of the float32 quotient x / delta[t]; rowsum[0][t]
// holds sum_k of the ROUNDED values as float32 bits (summed exactly as integers in units of 2^-9).
// Debug builds (-DFQL_TRACE, tools/trace_step.py): thread 0 of the first and the last 8 workgroups stamps the 100 MHz
// clock at the phase boundaries of the pre-pass.
#if defined(FQL_TRACE)
static __device__ unsigned long long fql_trace_act[16 * 16];   // (one copy per translation unit that includes this header)
#define FQL_ASTAMP(i) do { const int sl_ = (int)blockIdx.x < 8 ? (int)blockIdx.x : ((int)blockIdx.x + 8 >= rblocks && (int)blockIdx.x < rblocks ? 8 + (int)blockIdx.x - (rblocks - 8) : -1); \
    if (sl_ >= 0 && sl_ < 16 && threadIdx.x == 0) fql_trace_act[sl_ * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FQL_ASTAMP(i) do { } while (0)
#endif

// The pre-pass of ONE group of AR grouped rows t0 .. t0 + AR - 1 by a 256-thread workgroup: the body of act_fused_kernel, and
// (round 3) the first phase of the one-launch form of pre-pass + GEMM (fql_gemm_w4.h, FUSED).  Static LDS only; a caller that
// runs it more than once synchronises in between.
// WT: every global store goes straight to device-coherent memory (sc1): the one-launch form's consumers sit on other XCDs,
// whose L2s are not coherent with this one's, and a release fence instead (L2 write-back) cost 10-20 us per workgroup.
// CS (the backward pre-pass of fql_bwd.h; any input type, widened first): every loaded element is first multiplied by the column
// scale cs_scale[e][k] of its row's expert e (one float32 rounding), and the row's float correction
// sum_k x[k] * cs_scale[e][k] * f[e][k], f = zp - clamp(rint(zp), -112, 112) (cs_zp = the zero points), is written to
// the plane delta[DSETS * T + t] (the row-weight plane of the forward, unused by the backward).  The expert of each row is
// looked up BEFORE the loads of x here (the loads need it).
template <int L, bool VEC, int IN, bool GATE = false, bool F8OUT = false, int AR = ACT_ROWS, bool WT = false, bool CS = false, bool GLU = false>
__device__ __forceinline__ void act_rows(
    const void *__restrict__ xin, const int32_t *__restrict__ gather, int n_src, float *__restrict__ delta,
    int32_t *__restrict__ rowsum, int8_t *__restrict__ limbs, int T, int K, int KB, int MBT, int rblocks,
    const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs, int E, const float *__restrict__ row_weight, int t0,
    const float *__restrict__ cs_scale = nullptr, const float *__restrict__ cs_zp = nullptr, int act_kind = 0,
    float act_alpha = 0.0f, float act_limit = 0.0f)
{
    (void)rblocks;
    static_assert(!GLU || GATE, "an activation kind needs a gate|up row");
    // the hidden activation of a gate|up pair: silu(g) * u, or (GLU) the kind the kernel was handed (fql_common.h)
    auto gated_h = [&](float g, float u) {
        if constexpr (GLU) return act_glu_mul(act_kind, act_alpha, act_limit, g, u);
        else return act_silu_mul(g, u);
    };
    constexpr int ES = (IN == 0) ? 4 : 2;
    // row_weight (optional): per grouped row, copied into the plane behind delta's set(s) for the GEMM's epilogue
    constexpr int DSETS = (L >= 2 && !F8OUT && FQL_RES_ENABLED) ? 2 : 1;         // bytes per element of x
    // AR rows per workgroup: 4 at throughput sizes (measured best at configs[2]); 1 when there are only a few rows in
    // all (decode / small-batch linear), where the pre-pass is a latency chain and a row spread over 256 threads
    // (16 values each) shortens every link of it
    constexpr int R_ = AR, COLS_ = 256 / AR, CH_ = 256 / COLS_;
    static_assert(AR == 1 || AR == 2 || AR == 4 || AR == 8, "rows per workgroup");
    __shared__ int s_p[R_];
    __shared__ __attribute__((aligned(16))) uint32_t s_max[R_][16];     // [row][wave * 4 + 16-lane row of the wave]
    __shared__ __attribute__((aligned(16))) int s_sum[R_][L][16];
    __shared__ long long s_sum8[4][R_];
    __shared__ __attribute__((aligned(16))) float s_ssq[R_][16];
    __shared__ int s_flag[R_];
    static_assert(!F8OUT || L == 1, "fp8 activations are one byte plane");
    static_assert(!CS || (!GATE && !F8OUT && !WT), "column-scaled rows: plain input, int8 limbs");
    __shared__ int s_e[CS ? R_ : 1];
    __shared__ __attribute__((aligned(16))) float s_cor[CS ? R_ : 1][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FQL_ASTAMP(0);

    // ---- this workgroup's grouped rows t0 .. t0 + R_ - 1 (the last group may hold rows past T: they re-read row
    //      T - 1 and store nothing)
    if (t0 >= T) return;
    const int r = tid & (R_ - 1), col = tid / R_;   // row of the workgroup, chunk column
    const int trow = t0 + r;
    // the expert table's first 64 entries: loaded now, scanned when the loads of x are on their way
    int off_raw = 0, cnt_raw = 0;
    if (tpe != nullptr && wave == 0) expert_chunk_load(tpe, offs, E, 0, lane, off_raw, cnt_raw);
    const char *xr = reinterpret_cast<const char *>(xin) +
                     (size_t)source_row(gather, n_src, trow < T ? trow : T - 1) * K * ES * (GATE ? 2 : 1);
    const int nch = KB * 16;                      // 16-float chunks per padded row
    const int slabs = (nch + COLS_ * CH_ - 1) / (COLS_ * CH_);
    int tok = trow < T ? trow : -1;               // (-1 once the lookup finds no expert for the row either)
    const float *csr = nullptr, *czr = nullptr;   // CS: this row's column scales / zero points
    if constexpr (CS) {
        if (wave == 0) act_padded_rows(t0, R_, s_p, off_raw, cnt_raw, tpe, offs, E, T, lane, s_e);
        __syncthreads();
        const int ce = s_e[r % (CS ? R_ : 1)] < 0 ? 0 : s_e[r % (CS ? R_ : 1)];
        csr = cs_scale + (size_t)ce * K;
        czr = cs_zp + (size_t)ce * K;
    }
    float cor = 0.0f;                             // CS: this thread's part of the row's float correction
    auto cs_frac = [](float z) { return z - fminf(fmaxf(rintf(z), -112.0f), 112.0f); };

    // VEC (K % 16 == 0, x 16-byte aligned; host-checked): every load is unconditional.  A chunk past K (the
    // zero padding up to a multiple of 256) or a padding row re-reads valid data -- duplicates do not move the
    // row max -- and is masked to +0.0f in pass 2.
    v4f xv[CH_][4];
    auto chunk_ok = [&](int slab, int j) { return tok >= 0 && (slab * COLS_ * CH_ + col + COLS_ * j) * 16 < K; };
    auto load_slab = [&](int slab, bool first) {
        (void)first;
#pragma unroll
        for (int j = 0; j < CH_; ++j) {
            const int k0 = (slab * COLS_ * CH_ + col + COLS_ * j) * 16;
            if (VEC) {
                const char *src = xr + (size_t)(k0 < K ? k0 : 0) * ES;
                if (IN == 0 && GATE) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4f gq = *reinterpret_cast<const v4f *>(src + 16 * q);
                        const v4f uq = *reinterpret_cast<const v4f *>(src + (size_t)K * 4 + 16 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) xv[j][q][i] = gated_h(gq[i], uq[i]);
                    }
                } else if (IN == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xv[j][q] = *reinterpret_cast<const v4f *>(src + 16 * q);
                } else if (GATE) {                // 16 halves of gate and 16 of up = two 16-byte loads each
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const v4i gr = *reinterpret_cast<const v4i *>(src + 16 * h);
                        const v4i ur = *reinterpret_cast<const v4i *>(src + (size_t)K * 2 + 16 * h);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            xv[j][2 * h + (i >> 1)][2 * (i & 1)] =
                                gated_h(act_widen<IN>((unsigned short)((uint32_t)gr[i] & 0xFFFFu)), act_widen<IN>((unsigned short)((uint32_t)ur[i] & 0xFFFFu)));
                            xv[j][2 * h + (i >> 1)][2 * (i & 1) + 1] =
                                gated_h(act_widen<IN>((unsigned short)((uint32_t)gr[i] >> 16)), act_widen<IN>((unsigned short)((uint32_t)ur[i] >> 16)));
                        }
                    }
                } else {                          // 16 halves = two 16-byte loads
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const v4i raw = *reinterpret_cast<const v4i *>(src + 16 * h);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            xv[j][2 * h + (i >> 1)][2 * (i & 1)] = act_widen<IN>((unsigned short)((uint32_t)raw[i] & 0xFFFFu));
                            xv[j][2 * h + (i >> 1)][2 * (i & 1) + 1] = act_widen<IN>((unsigned short)((uint32_t)raw[i] >> 16));
                        }
                    }
                }
                if constexpr (CS) {               // column scale (and the float correction) on the widened values
                    const int kc = k0 < K ? k0 : 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4f s4 = *reinterpret_cast<const v4f *>(csr + kc + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) xv[j][q][i] = xv[j][q][i] * s4[i];
                        if (first && k0 < K) {
                            const v4f z4 = *reinterpret_cast<const v4f *>(czr + kc + 4 * q);
#pragma unroll
                            for (int i = 0; i < 4; ++i) cor = fmaf(xv[j][q][i], cs_frac(z4[i]), cor);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int k = k0 + 4 * q + i;
                        float v = 0.0f;
                        if (k < K) {
                            if (IN == 0 && GATE) v = gated_h(reinterpret_cast<const float *>(xr)[k], reinterpret_cast<const float *>(xr)[K + k]);
                            else if (IN == 0) v = reinterpret_cast<const float *>(xr)[k];
                            else if (GATE) v = gated_h(act_widen<IN>(reinterpret_cast<const unsigned short *>(xr)[k]), act_widen<IN>(reinterpret_cast<const unsigned short *>(xr)[K + k]));
                            else v = act_widen<IN>(reinterpret_cast<const unsigned short *>(xr)[k]);
                            if constexpr (CS) {
                                v = v * csr[k];
                                if (first) cor = fmaf(v, cs_frac(czr[k]), cor);
                            }
                        }
                        xv[j][q][i] = v;
                    }
            }
        }
    };

    // ---- all loads of the first slab, then the padded row of every grouped row (wave 0; the others go on to the maximum)
    load_slab(0, true);
    __builtin_amdgcn_sched_barrier(0);
    if (!CS && wave == 0) act_padded_rows(t0, R_, s_p, off_raw, cnt_raw, tpe, offs, E, T, lane);
    __builtin_amdgcn_sched_barrier(0);
    FQL_ASTAMP(1);

    // ---- pass 1: row maximum, on the bit patterns: |x| as an unsigned integer orders finite < Inf < NaN, so one
    //      integer max finds the magnitude and flags a non-finite row
    uint32_t mu = 0u;
    for (int slab = 0; slab < slabs; ++slab) {
        if (slab > 0) load_slab(slab, true);
#pragma unroll
        for (int j = 0; j < CH_; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t u = __float_as_uint(xv[j][q][i]) & 0x7FFFFFFFu;
                    mu = u > mu ? u : mu;
                }
    }
    mu = (uint32_t)act_row16_reduce<R_>((int)mu, [](int a, int b) { return (int)((uint32_t)a > (uint32_t)b ? (uint32_t)a : (uint32_t)b); });
    if ((lane & 15) < R_) s_max[lane & 15][wave * 4 + (lane >> 4)] = mu;
    __syncthreads();
    {
        mu = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v4i q = reinterpret_cast<const v4i *>(s_max[r])[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) mu = (uint32_t)q[c] > mu ? (uint32_t)q[c] : mu;
        }
    }
    // (the same barrier published the lookup)
    const int p = s_p[r];
    tok = p >= 0 ? tok : -1;
    const int mb = p >> 5, r32 = p & 31;
    const bool bad = mu >= 0x7F800000u;
    const float m = __uint_as_float(mu);
    FQL_ASTAMP(2);
    if constexpr (F8OUT) {
        // ---- pass 2 (fp8): y = x / scale rounded to e4m3, scale = max|x| / 448 (1 for an all-zero row)
        const float scale = (bad || m == 0.0f) ? 1.0f : m / 448.0f;
        if (tid < R_ && tok >= 0) { delta[tok] = bad ? __builtin_nanf("") : scale; if (row_weight != nullptr) delta[(size_t)DSETS * T + tok] = row_weight[tok]; }
        long long sum8 = 0;
        for (int slab = 0; slab < slabs; ++slab) {
            if (slabs > 1) load_slab(slab, false);
#pragma unroll
            for (int j = 0; j < CH_; ++j) {
                const int ch = slab * COLS_ * CH_ + col + COLS_ * j;
                if (ch >= nch) continue;
                const uint32_t keep = (chunk_ok(slab, j) && !bad) ? 0xFFFFFFFFu : 0u;
                uint32_t nat[4];                               // e4m3 bytes of k = 4 dw .. 4 dw + 3, natural order
                int part = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float y[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] = __uint_as_float(__float_as_uint(xv[j][q][i]) & keep) / scale;
                    int v = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
                    v = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], v, true);
                    nat[q] = (uint32_t)v;
                    part += (int)(__builtin_amdgcn_cvt_f32_fp8(v, 0) * 512.0f) + (int)(__builtin_amdgcn_cvt_f32_fp8(v, 1) * 512.0f)
                          + (int)(__builtin_amdgcn_cvt_f32_fp8(v, 2) * 512.0f) + (int)(__builtin_amdgcn_cvt_f32_fp8(v, 3) * 512.0f);
                }
                sum8 += part;
                // same byte order as the limbs: (0,2,4,6) then (1,3,5,7) of every group of 8
                const uint32_t w0 = __builtin_amdgcn_perm(nat[1], nat[0], 0x06040200u), w1 = __builtin_amdgcn_perm(nat[1], nat[0], 0x07050301u);
                const uint32_t w2 = __builtin_amdgcn_perm(nat[3], nat[2], 0x06040200u), w3 = __builtin_amdgcn_perm(nat[3], nat[2], 0x07050301u);
                const int kb = ch >> 4, c16 = ch & 15;
                const int ks = 2 * (c16 >> 2) + (c16 & 1), g = (c16 >> 1) & 1;
                int8_t *dst = limbs + (((size_t)kb) * MBT + mb) * 8192 + ((ks * 64) + g * 32 + r32) * 16;
                if (tok >= 0) *reinterpret_cast<v4i *>(dst) = v4i{(int)w0, (int)w1, (int)w2, (int)w3};
            }
        }
#pragma unroll
        for (int o = R_; o < 64; o <<= 1) sum8 += __shfl_xor(sum8, o, 64);
        if (lane < R_) s_sum8[wave][lane] = sum8;
        __syncthreads();
        if (tid < R_ && tok >= 0) {
            const long long tot = (s_sum8[0][tid] + s_sum8[1][tid]) + (s_sum8[2][tid] + s_sum8[3][tid]);
            rowsum[tok] = __float_as_int((float)tot * 0x1p-9f);
        }
        return;
    }
    const int e = act_exponent<L>(bad ? 0.0f : m);
    const float inv = bad ? 0.0f : ldexpf(1.0f, -e);           // non-finite row: limbs 0, delta NaN -> outputs NaN
    auto put_f = [&](float *ptr, float v) { if (WT) __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *ptr = v; };
    auto put_i = [&](int32_t *ptr, int v) { if (WT) __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *ptr = v; };
    if (tid < R_ && tok >= 0) { put_f(delta + tok, bad ? __builtin_nanf("") : ldexpf(1.0f, e)); if (row_weight != nullptr) put_f(delta + (size_t)DSETS * T + tok, row_weight[tok]); }

    // ---- pass 2: quantise and store.  Pass 3 (rows flagged as heavy-tailed only, L >= 2): the RESIDUAL of pass 2's
    //      rounding, r = x / delta - X in [-1/2, 1/2] (exact in float32), as a second fixed-point value
    //      R = rint(r * 2^(8L-1)) with quantum delta2 = delta * 2^-(8L-1), into the second limb set
    //      (limbs + L planes, delta2 = delta + T, rowsum2 = rowsum + L*T).  The GEMM adds
    //      delta2 * (sum_k q R - zp * rowsum2) for those rows (fql_gemm_i8.h), which takes the per-row block
    //      fixed point from 8L-1 to 16L-2 bits: one outlier channel no longer coarsens the rest of its row.
    //      A row is flagged when the predicted relative error of its 8L-1 bits, sqrt(K / 12) / ||x / delta||_2,
    //      exceeds 1e-6 (L = 3) / 2.5e-4 (L = 2): half of the stated bound of the mode (tests/helpers.py) resp. a
    //      quarter of the north-star 1e-3.  randn rows are never flagged.  The prediction is relative to the row's
    //      input norm; it is the output row's relative error when that row does not cancel, and a row whose result
    //      cancels (||x_t W|| << ||x_t|| ||W||_F / sqrt(K), e.g. a zero-point term far from the centre of q that
    //      nearly vanishes for that row) shows it amplified by that ratio, as any rounding of the inputs would.
    constexpr bool RES = (L >= 2);
    constexpr int RBITS = 8 * L - 1;
    auto emit = [&](auto resid_tag, int (&sums)[L], float &ssq, bool store) {
        constexpr bool RESID = decltype(resid_tag)::value;
        int8_t *base = limbs + (RESID ? (size_t)L * KB * MBT * 8192 : (size_t)0);
        for (int slab = 0; slab < slabs; ++slab) {
            if (slabs > 1) load_slab(slab, false);
#pragma unroll
            for (int j = 0; j < CH_; ++j) {
                const int ch = slab * COLS_ * CH_ + col + COLS_ * j;
                if (ch >= nch) continue;
                // All L balanced digits of X at once: Y = X + sum_{l<L-1} 128*256^l has plain base-256 digits
                // d_l + 128 in its low bytes and the top digit above them, so byte l of Z = Y ^ 0x..8080 is limb l.
                // (the conversion of bytes l < L-1 from d_l + 128 to two's complement, the XOR, is done on the transposed
                //  dwords below: 4 bytes at a time)
                constexpr int BIAS = (L == 3) ? 0x8080 : (L == 2) ? 0x80 : 0;
                // padding (a chunk past K, re-read data): scaled by zero -> digits 0 whatever was read (the rows are
                // finite here: a non-finite row has inv = 0 as a whole, and NaN converts to 0)
                const float inv_c = chunk_ok(slab, j) ? inv : 0.0f;
                uint32_t Z[16];
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float xq = xv[j][q][i] * inv_c;
                        const float xr = rintf(xq);
                        int v;
                        if (RESID) v = (int)rintf((xq - xr) * (float)(1 << RBITS));
                        else { v = (int)xr; ssq = fmaf(xq, xq, ssq); }
                        Z[4 * q + i] = (uint32_t)(v + BIAS);
                    }
                // byte transpose into the limb dwords; inside an 8-group the byte order is (0,2,4,6,1,3,5,7):
                // dword 2h = k (0,2,4,6) of 8-group h, dword 2h+1 = k (1,3,5,7)
                uint32_t w[L][4];
#pragma unroll
                for (int dw = 0; dw < 4; ++dw) {
                    const int kbase = 8 * (dw >> 1) + (dw & 1);
                    const uint32_t za = Z[kbase], zb = Z[kbase + 2], zc = Z[kbase + 4], zd = Z[kbase + 6];
                    const uint32_t lo_ab = __builtin_amdgcn_perm(zb, za, 0x05010400u);      // a0 b0 a1 b1
                    const uint32_t lo_cd = __builtin_amdgcn_perm(zd, zc, 0x05010400u);
                    w[0][dw] = __builtin_amdgcn_perm(lo_cd, lo_ab, 0x05040100u) ^ (L > 1 ? 0x80808080u : 0u);   // a0 b0 c0 d0
                    if (L > 1) w[1 % L][dw] = __builtin_amdgcn_perm(lo_cd, lo_ab, 0x07060302u) ^ (L > 2 ? 0x80808080u : 0u);   // a1 b1 c1 d1
                    if (L > 2) {
                        const uint32_t hi_ab = __builtin_amdgcn_perm(zb, za, 0x07030602u);  // a2 b2 a3 b3
                        const uint32_t hi_cd = __builtin_amdgcn_perm(zd, zc, 0x07030602u);
                        w[2 % L][dw] = __builtin_amdgcn_perm(hi_cd, hi_ab, 0x05040100u);    // a2 b2 c2 d2
                    }
                }
                const int kb = ch >> 4, c16 = ch & 15;    // k = 32 (2v+g) + 16 b  ->  c16 = 2 (2v+g) + b
                const int ks = 2 * (c16 >> 2) + (c16 & 1), g = (c16 >> 1) & 1;
#pragma unroll
                for (int l = 0; l < L; ++l) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) sums[l] = __builtin_amdgcn_sdot4((int)w[l][i], 0x01010101, sums[l], false);
                    int8_t *dst = base + (((size_t)l * KB + kb) * MBT + mb) * 8192 + ((ks * 64) + g * 32 + r32) * 16;
                    if (store && tok >= 0) {
                        if (FQL_LIMB_WT || WT) store16_wt(dst, v4i{(int)w[l][0], (int)w[l][1], (int)w[l][2], (int)w[l][3]});
                        else *reinterpret_cast<v4i *>(dst) = v4i{(int)w[l][0], (int)w[l][1], (int)w[l][2], (int)w[l][3]};
                    }
                }
            }
        }
    };
    auto reduce_sums = [&](int (&sums)[L]) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            sums[l] = act_row16_reduce<R_>(sums[l], [](int a, int b) { return a + b; });
            if ((lane & 15) < R_) s_sum[lane & 15][l][wave * 4 + (lane >> 4)] = sums[l];
        }
    };
    auto total_sum = [&](int row, int l) -> int {              // (fixed order: the result does not depend on timing)
        int tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v4i q = reinterpret_cast<const v4i *>(s_sum[row][l])[i];
            tot += (q[0] + q[1]) + (q[2] + q[3]);
        }
        return tot;
    };
    int sums[L];
#pragma unroll
    for (int l = 0; l < L; ++l) sums[l] = 0;
    float ssq = 0.0f;
    emit(std::false_type{}, sums, ssq, true);
    FQL_ASTAMP(3);
    reduce_sums(sums);
    if (RES) {
        ssq = __int_as_float(act_row16_reduce<R_>(__float_as_int(ssq), [](int a, int b) { return __float_as_int(__int_as_float(a) + __int_as_float(b)); }));
        if ((lane & 15) < R_) s_ssq[lane & 15][wave * 4 + (lane >> 4)] = ssq;
    }
    if (CS) {
        cor = __int_as_float(act_row16_reduce<R_>(__float_as_int(cor), [](int a, int b) { return __float_as_int(__int_as_float(a) + __int_as_float(b)); }));
        if ((lane & 15) < R_) s_cor[(lane & 15) % (CS ? R_ : 1)][wave * 4 + (lane >> 4)] = cor;
    }
    __syncthreads();
    if (tid < R_) {
        int flag = 0;
        if (CS && tok >= 0) {                                                  // (fixed order, as the limb sums)
            float tot = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const v4f q = reinterpret_cast<const v4f *>(s_cor[tid % (CS ? R_ : 1)])[i];
                tot += (q[0] + q[1]) + (q[2] + q[3]);
            }
            put_f(delta + (size_t)DSETS * T + tok, tot);
        }
        if (tok >= 0) {
#pragma unroll
            for (int l = 0; l < L; ++l) put_i(rowsum + (size_t)l * T + tok, total_sum(tid, l));
            if (RES) {
                float tot = 0.0f;                                                      // ||x / delta||^2
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const v4f q = reinterpret_cast<const v4f *>(s_ssq[tid])[i];
                    tot += (q[0] + q[1]) + (q[2] + q[3]);
                }
                const float lim = (float)K * (L == 3 ? 8.3333e10f : 1.3333e6f);                    // K / (12 P^2)
                flag = (!bad && m != 0.0f && tot < lim && e - RBITS >= -126) ? 1 : 0;
                put_f(delta + (size_t)T + tok, flag ? ldexpf(1.0f, e - RBITS) : 0.0f);
            }
        }
        if (RES) s_flag[tid] = flag;
    }
    FQL_ASTAMP(4);
    if (!RES) return;
    __syncthreads();
    {
        int any = 0;
#pragma unroll
        for (int i = 0; i < R_; ++i) any |= s_flag[i];
        if (any == 0) { FQL_ASTAMP(5); return; }
    }
#pragma unroll
    for (int l = 0; l < L; ++l) sums[l] = 0;
    emit(std::true_type{}, sums, ssq, s_flag[r] != 0);
    reduce_sums(sums);
    __syncthreads();
    if (tid < R_ && tok >= 0 && s_flag[tid]) {
#pragma unroll
        for (int l = 0; l < L; ++l) put_i(rowsum + (size_t)(L + l) * T + tok, total_sum(tid, l));
    }
}

template <int L, bool VEC, int IN, bool GATE = false, bool F8OUT = false, int AR = ACT_ROWS>
__global__ __launch_bounds__(256) void act_fused_kernel(
    const void *__restrict__ xin, const int32_t *__restrict__ gather, int n_src, float *__restrict__ delta,
    int32_t *__restrict__ rowsum, int8_t *__restrict__ limbs, int T, int K, int KB, int MBT, int rblocks,
    void *__restrict__ out, int out_es, int N, const int32_t *__restrict__ tpe, const int32_t *__restrict__ offs,
    int E, const float *__restrict__ row_weight)
{
    if ((int)blockIdx.x >= rblocks) {             // ---- coverage workgroups: 256 rows of `out` each
        act_zero_uncovered((int)blockIdx.x - rblocks, out, out_es, N, tpe, offs, E, T);
        return;
    }
    act_rows<L, VEC, IN, GATE, F8OUT, AR>(xin, gather, n_src, delta, rowsum, limbs, T, K, KB, MBT, rblocks, tpe, offs, E, row_weight,
                                          (int)blockIdx.x * AR);
}

// The gated pre-pass for an activation kind other than silu (FQL_ACT_GELU_TANH / FQL_ACT_SWIGLU_CLAMP): act_fused_kernel<L, VEC,
// IN, GATE = true> with the kind and its two floats as arguments.  Instantiated in fql_glu.hip only.
template <int L, bool VEC, int IN, int AR = ACT_ROWS>
__global__ __launch_bounds__(256) void act_glu_kernel(
    const void *__restrict__ xin, float *__restrict__ delta, int32_t *__restrict__ rowsum, int8_t *__restrict__ limbs, int T,
    int K, int KB, int MBT, int rblocks, void *__restrict__ out, int out_es, int N, const int32_t *__restrict__ tpe,
    const int32_t *__restrict__ offs, int E, const float *__restrict__ row_weight, int act_kind, float act_alpha,
    float act_limit)
{
    if ((int)blockIdx.x >= rblocks) {             // ---- coverage workgroups: 256 rows of `out` each
        act_zero_uncovered((int)blockIdx.x - rblocks, out, out_es, N, tpe, offs, E, T);
        return;
    }
    act_rows<L, VEC, IN, true, false, AR, false, false, true>(xin, nullptr, 0, delta, rowsum, limbs, T, K, KB, MBT, rblocks, tpe, offs, E,
                                                              row_weight, (int)blockIdx.x * AR, nullptr, nullptr, act_kind,
                                                              act_alpha, act_limit);
}
