// Probe of the fp4 (e2m1) A operand of v_mfma_scale_f32_32x32x64_f8f6f4 against an e4m3 B operand (cbsz = 4, blgp = 0), for
// the MXFP4 fp8-row path (csrc/fql_gemm_mx4_f8.h).  One instruction on asymmetric exact data; every hypothesis is scored by
// its count of mismatching outputs, so exactly one line per question reads "0 / 1024":
//   1. which (row, k) each nibble of a lane's 16 bytes holds, and how those 32 k pair with the 32 bytes of the B operand;
//   2. which lane's scale byte applies to which row and block, and what op_sel selects;
//   3. what comes back for scale codes 0, 254, 255 and for an e4m3 NaN byte in B.
// hipcc --offload-arch=gfx950 -O3 -o mfma_f4_probe mfma_f4_probe.hip && ./mfma_f4_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

static float e4m3_to_float(uint8_t b)
{
    const int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
    float v;
    if (e == 0) v = ldexpf((float)m, -9);
    else if (e == 15 && m == 7) v = NAN;
    else v = ldexpf(1.0f + m / 8.0f, e - 7);
    return s ? -v : v;
}
static float e2m1_to_float(int c)
{
    static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return (c & 8) ? -mag[c & 7] : mag[c & 7];
}

// a: 64 lanes x 16 bytes of fp4 (registers 4 .. 7 of the operand are filled with `junk`), b: 64 lanes x 32 bytes of e4m3,
// sa: one dword of four scale bytes a lane; the B scale is code 127 in every byte.
template <int OPSEL>
__global__ void one32(const uint8_t *a, const uint8_t *b, const uint32_t *sa, float *d, int junk)
{
    const int l = threadIdx.x;
    v8i av, bv;
    for (int i = 0; i < 4; ++i) { av[i] = ((const int *)a)[l * 4 + i]; av[4 + i] = junk; }
    for (int i = 0; i < 8; ++i) bv[i] = ((const int *)b)[l * 8 + i];
    v16f acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 0, OPSEL, (int)sa[l], 0, 0x7F7F7F7F);
    for (int r = 0; r < 16; ++r) d[l * 16 + r] = acc[r];
}

static std::vector<float> run32(const std::vector<uint8_t> &A, const std::vector<uint8_t> &B, const std::vector<uint32_t> &S,
                                int opsel, int junk)
{
    uint8_t *da, *db; uint32_t *ds; float *dd;
    hipMalloc(&da, 1024); hipMalloc(&db, 2048); hipMalloc(&ds, 256); hipMalloc(&dd, 64 * 16 * 4);
    hipMemcpy(da, A.data(), 1024, hipMemcpyHostToDevice); hipMemcpy(db, B.data(), 2048, hipMemcpyHostToDevice);
    hipMemcpy(ds, S.data(), 256, hipMemcpyHostToDevice);
    switch (opsel) {
    case 0: hipLaunchKernelGGL(one32<0>, dim3(1), dim3(64), 0, 0, da, db, ds, dd, junk); break;
    case 1: hipLaunchKernelGGL(one32<1>, dim3(1), dim3(64), 0, 0, da, db, ds, dd, junk); break;
    case 2: hipLaunchKernelGGL(one32<2>, dim3(1), dim3(64), 0, 0, da, db, ds, dd, junk); break;
    default: hipLaunchKernelGGL(one32<3>, dim3(1), dim3(64), 0, 0, da, db, ds, dd, junk); break;
    }
    std::vector<float> D(64 * 16);
    if (hipMemcpy(D.data(), dd, 64 * 16 * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error\n"); exit(1); }
    hipFree(da); hipFree(db); hipFree(ds); hipFree(dd);
    return D;
}

// Output D[lane][reg]: column (B side) = lane & 31, row (A side) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), as for every
// 32x32 MFMA.  pair[H][J] = 32 h + j: nibble J of A lane (H, row) meets byte j of B lane (h, col), as derive_map() found it.
// Nibble J of a lane is the low half of byte J / 2 for even J (hi_first: the high half); the scale of an A lane's 32
// nibbles is byte sbyte of lane slane(row, H, col).
static int score(const std::vector<float> &D, const std::vector<uint8_t> &A, const std::vector<uint8_t> &B,
                 const std::vector<uint32_t> &S, const int pair[2][32], bool hi_first, int lane_rule, int sbyte)
{
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
        const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        double ref = 0;
        for (int h = 0; h < 2; ++h) {
            const int sl = lane_rule == 0 ? h * 32 + row : lane_rule == 1 ? row : lane_rule == 2 ? 32 + row : h * 32 + col;
            const int code = (S[sl] >> (8 * sbyte)) & 255;
            double part = 0;
            for (int j = 0; j < 32; ++j) {
                const uint8_t byte = A[(h * 32 + row) * 16 + (j >> 1)];
                const int nib = ((j & 1) != (int)hi_first) ? byte >> 4 : byte & 15;
                const int pb = pair[h][j];
                part += (double)e2m1_to_float(nib) * (double)e4m3_to_float(B[((pb >> 5) * 32 + col) * 32 + (pb & 31)]);
            }
            ref += ldexp(part, code - 127);
        }
        if (ref != (double)D[l * 16 + r]) ++bad;
    }
    return bad;
}

// One-hot map: B lane (h, col) byte j holds the e4m3 byte 0x08 + 32 h + j (64 distinct positive values, the same in every
// column); A row `row` of half H holds 1.0 (code 2) in the low nibble position J = row only, unit scales.  D[row][0] is
// then the value of the B slot that nibble J of half H meets.
static void derive_map(int pair[2][32], bool hi_first)
{
    std::vector<uint8_t> B(2048);
    std::vector<uint32_t> S(64, 0x7F7F7F7Fu);
    for (int l = 0; l < 64; ++l) for (int j = 0; j < 32; ++j) B[l * 32 + j] = (uint8_t)(0x08 + 32 * (l >> 5) + j);
    for (int H = 0; H < 2; ++H) {
        std::vector<uint8_t> A(1024, 0);
        for (int row = 0; row < 32; ++row) A[(H * 32 + row) * 16 + (row >> 1)] = (uint8_t)(0x02 << (4 * ((row & 1) != (int)hi_first)));
        const std::vector<float> D = run32(A, B, S, 0, 0);
        for (int row = 0; row < 32; ++row) {
            // (column 0 lives in lanes 0 and 32)
            const int l = (row >> 2) & 1 ? 32 : 0, r = (row & 3) + 4 * (row >> 3);
            const float v = D[l * 16 + r];
            pair[H][row] = -1;
            for (int c = 0; c < 64; ++c) if (e4m3_to_float((uint8_t)(0x08 + c)) == v) pair[H][row] = c;
        }
    }
}

int main()
{
    srand(11);
    int pair[2][32];
    derive_map(pair, false);
    for (int H = 0; H < 2; ++H) {
        printf("fp4 lane half %d, nibble J (low half of byte J / 2 for even J) meets B (half h, byte j):", H);
        for (int J = 0; J < 32; ++J) {
            if (J % 8 == 0) printf("\n   ");
            if (pair[H][J] < 0) printf(" J%-2d ->  ??  ", J); else printf(" J%-2d -> h%d j%-2d", J, pair[H][J] >> 5, pair[H][J] & 31);
        }
        printf("\n");
    }
    for (int H = 0; H < 2; ++H) for (int J = 0; J < 32; ++J) if (pair[H][J] < 0) pair[H][J] = 32 * H + J;

    // e4m3 codes of 0, 1, 2, 3, 4 with random signs; all 16 fp4 codes; a different scale code 125 .. 129 in every byte
    const uint8_t code[5] = {0x00, 0x38, 0x40, 0x44, 0x48};
    std::vector<uint8_t> A(1024), B(2048);
    std::vector<uint32_t> S(64);
    for (auto &v : A) v = (uint8_t)(rand() & 255);
    for (auto &v : B) v = (uint8_t)(code[rand() % 5] | ((rand() & 1) << 7));
    for (auto &v : S) { v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)(125 + rand() % 5) << (8 * i); }

    static const char *rules[4] = {"lane 32 h + row", "lane row", "lane 32 + row", "lane 32 h + col"};
    for (int opsel = 0; opsel < 4; ++opsel) {
        const std::vector<float> D = run32(A, B, S, opsel, 0x5A5A5A5A);
        int best = 1025;
        for (int hi = 0; hi < 2; ++hi) for (int rule = 0; rule < 4; ++rule) for (int sb = 0; sb < 4; ++sb) {
            const int bad = score(D, A, B, S, pair, hi != 0, rule, sb);
            if (bad < best) best = bad;
            if (bad < 64)
                printf("op_sel %d: %s nibble first, scale = byte %d of %-16s mismatches %4d / 1024\n", opsel,
                       hi ? "high" : "low", sb, rules[rule], bad);
        }
        printf("op_sel %d: best hypothesis has %d mismatches\n", opsel, best);
        if (opsel == 0) {
            const std::vector<float> D2 = run32(A, B, S, 0, 0x13572468);
            int diff = 0;
            for (int i = 0; i < 1024; ++i) diff += D[i] != D2[i];
            printf("registers 4 .. 7 of the fp4 operand changed: %d outputs differ\n", diff);
        }
    }

    // specials: A = 1.0 (code 2) at nibble 0 of lane `row 0, half 0` only, zero elsewhere; B = 1.0 everywhere
    auto special = [&](const char *name, uint32_t scode, bool zero_a, int b_nan_lane) {
        std::vector<uint8_t> a(1024, 0), b(2048, 0x38);
        std::vector<uint32_t> s(64, 0x7F7F7F7Fu);
        if (!zero_a) a[0] = 0x02;
        s[0] = scode * 0x01010101u;
        if (b_nan_lane >= 0) b[b_nan_lane * 32 + 5] = 0x7F;
        const std::vector<float> D = run32(a, b, s, 0, 0);
        int nans = 0, nan_row0 = 0, nan_col = 0;
        for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
            const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            if (std::isnan(D[l * 16 + r])) { ++nans; nan_row0 += row == 0; nan_col += b_nan_lane >= 0 && col == (b_nan_lane & 31); }
        }
        uint32_t bits0, bits1;
        memcpy(&bits0, &D[0], 4); memcpy(&bits1, &D[1], 4);
        printf("%-58s D[row0][col0] = %g (0x%08x)  D[row1][col0] = %g   NaNs %d (in row 0: %d, in the NaN column: %d)\n",
               name, D[0], bits0, D[1], nans, nan_row0, nan_col);
    };
    special("scale 127, A[0][0] = 1", 127, false, -1);
    special("scale 0,   A[0][0] = 1", 0, false, -1);
    special("scale 1,   A[0][0] = 1", 1, false, -1);
    special("scale 254, A[0][0] = 1", 254, false, -1);
    special("scale 255, A[0][0] = 1", 255, false, -1);
    special("scale 255, A row 0 all zero codes", 255, true, -1);
    special("scale 127, e4m3 NaN byte in B lane 3 (col 3, half 0), k 5", 127, false, 3);
    special("scale 127, NaN byte in B lane 35 (col 3, half 1), A all zero", 127, true, 35);
    return 0;
}
