// Probe of the fp4 (e2m1) A operand of v_mfma_scale_f32_32x32x64_f8f6f4 against an e4m3 B operand (cbsz = 4, blgp = 0), for
// the MXFP4 fp8-row path (csrc/fql_gemm_mx4_scaled.h).  One instruction on asymmetric exact data; every hypothesis is scored by
// its count of mismatching outputs, so exactly one line per question reads "0 / 1024":
//   1. which (row, k) each nibble of a lane's 16 bytes holds, and how those 32 k pair with the 32 bytes of the B operand;
//   2. which lane's scale byte applies to which row and block, and what op_sel selects;
//   3. what comes back for scale codes 0, 254, 255 and for an e4m3 NaN byte in B.
// hipcc --offload-arch=gfx950 -O3 -o mfma_f4_probe mfma_f4_probe.hip && ./mfma_f4_probe
//
// ./mfma_f4_probe f4f4: the same instruction with BOTH operands fp4 (cbsz = 4, blgp = 4), for the MXFP4-row path
// (csrc/fql_gemm_mx4_scaled.h), in the same style.  The A operand's map is the one measured above; the questions are B's:
//   1. which (column, k) each nibble of a B lane's 16 bytes holds;
//   2. which byte of the B scale register op_sel selects, which lane's, and which block it scales;
//   3. what B scale codes 0, 254 and 255 return, and whether 255 makes exactly the 32 outputs of its column NaN.
//
// ./mfma_f4_probe f4f6: the fp4 A operand against a 6-bit B operand (cbsz = 4, blgp = 2: e2m3), for the MXFP6-row path
// (csrc/fql_gemm_mx4_scaled.h).  B is six registers a lane, 192 bits = 32 fields of 6.  The questions are B's again:
//   1. which (column, k) the field at bits 6 J .. 6 J + 5 of a B lane's 24 bytes (one little-endian integer) holds;
//   2. which byte of the B scale register op_sel selects, which lane's, and which block it scales;
//   3. what B scale codes 0, 254 and 255 return, and whether 255 makes exactly the 32 outputs of its column NaN.
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

static int main_f4f4();
static int main_f4f6();

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "f4f4")) return main_f4f4();
    if (argc > 1 && !strcmp(argv[1], "f4f6")) return main_f4f6();
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

// ---------------------------------------------------------------------------------------------------------------------
// fp4 x fp4 (cbsz = 4, blgp = 4).  a, b: 64 lanes x 16 bytes each (registers 4 .. 7 of both operands are `junk`); sa, sb: one
// dword of four scale bytes a lane for each side.
template <int OPA, int OPB>
__global__ void one44(const uint8_t *a, const uint8_t *b, const uint32_t *sa, const uint32_t *sb, float *d, int junk)
{
    const int l = threadIdx.x;
    v8i av, bv;
    for (int i = 0; i < 4; ++i) { av[i] = ((const int *)a)[l * 4 + i]; av[4 + i] = junk; }
    for (int i = 0; i < 4; ++i) { bv[i] = ((const int *)b)[l * 4 + i]; bv[4 + i] = junk; }
    v16f acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 4, OPA, (int)sa[l], OPB, (int)sb[l]);
    for (int r = 0; r < 16; ++r) d[l * 16 + r] = acc[r];
}

// op_sel of A is (opb + 1) & 3: the two selectors are shown to be independent.
static std::vector<float> run44(const std::vector<uint8_t> &A, const std::vector<uint8_t> &B, const std::vector<uint32_t> &SA,
                                const std::vector<uint32_t> &SB, int opb, int junk)
{
    uint8_t *da, *db; uint32_t *dsa, *dsb; float *dd;
    hipMalloc(&da, 1024); hipMalloc(&db, 1024); hipMalloc(&dsa, 256); hipMalloc(&dsb, 256); hipMalloc(&dd, 64 * 16 * 4);
    hipMemcpy(da, A.data(), 1024, hipMemcpyHostToDevice); hipMemcpy(db, B.data(), 1024, hipMemcpyHostToDevice);
    hipMemcpy(dsa, SA.data(), 256, hipMemcpyHostToDevice); hipMemcpy(dsb, SB.data(), 256, hipMemcpyHostToDevice);
    switch (opb) {
    case 0: hipLaunchKernelGGL((one44<1, 0>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    case 1: hipLaunchKernelGGL((one44<2, 1>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    case 2: hipLaunchKernelGGL((one44<3, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    default: hipLaunchKernelGGL((one44<0, 3>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    }
    std::vector<float> D(64 * 16);
    if (hipMemcpy(D.data(), dd, 64 * 16 * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error\n"); exit(1); }
    hipFree(da); hipFree(db); hipFree(dsa); hipFree(dsb); hipFree(dd);
    return D;
}

// A as measured: lane (row, H) holds k = 32 H + J, low nibble first, scaled by byte opa of its own scale register.
// B hypothesis: nibble J of lane (col, h) is k = bmap[h][J] (hi_first: the high half of a byte first); the scale of that
// nibble is byte sbyte of lane  0: 32 h + col (the lane's own)  1: col  2: 32 + col  3: 32 (k >> 5) + col (the lane of k's block).
static int score44(const std::vector<float> &D, const std::vector<uint8_t> &A, const std::vector<uint8_t> &B,
                   const std::vector<uint32_t> &SA, const std::vector<uint32_t> &SB, int opa, const int bmap[2][32],
                   bool hi_first, int lane_rule, int sbyte)
{
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
        const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        double av[64], bv[64];
        for (int H = 0; H < 2; ++H) for (int J = 0; J < 32; ++J) {
            const uint8_t ab = A[(H * 32 + row) * 16 + (J >> 1)];
            av[32 * H + J] = ldexp((double)e2m1_to_float((J & 1) ? ab >> 4 : ab & 15), (int)((SA[H * 32 + row] >> (8 * opa)) & 255) - 127);
            const uint8_t bb = B[(H * 32 + col) * 16 + (J >> 1)];
            const int nib = ((J & 1) != (int)hi_first) ? bb >> 4 : bb & 15, k = bmap[H][J];
            const int sl = lane_rule == 0 ? H * 32 + col : lane_rule == 1 ? col : lane_rule == 2 ? 32 + col : 32 * (k >> 5) + col;
            bv[k] = ldexp((double)e2m1_to_float(nib), (int)((SB[sl] >> (8 * sbyte)) & 255) - 127);
        }
        double ref = 0;
        for (int k = 0; k < 64; ++k) ref += av[k] * bv[k];
        if (ref != (double)D[l * 16 + r]) ++bad;
    }
    return bad;
}

// One-hot map of B.  A row i holds 1.0 (code 2) at k = 32 H + i alone (nibble i of lane (i, H), by A's measured map); B
// column c holds 1.0 in nibble J = c of its lane of half h alone.  D[row i][col c] is then 1 exactly where nibble c of a
// B lane of half h is k = 32 H + i.
static void derive_bmap(int bmap[2][32])
{
    const std::vector<uint32_t> S(64, 0x7F7F7F7Fu);
    for (int h = 0; h < 2; ++h) for (int J = 0; J < 32; ++J) bmap[h][J] = -1;
    for (int h = 0; h < 2; ++h) for (int H = 0; H < 2; ++H) {
        std::vector<uint8_t> A(1024, 0), B(1024, 0);
        for (int i = 0; i < 32; ++i) A[(H * 32 + i) * 16 + (i >> 1)] = (uint8_t)(0x02 << (4 * (i & 1)));
        for (int c = 0; c < 32; ++c) B[(h * 32 + c) * 16 + (c >> 1)] = (uint8_t)(0x02 << (4 * (c & 1)));
        const std::vector<float> D = run44(A, B, S, S, 0, 0);
        for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
            const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            if (D[l * 16 + r] == 1.0f) bmap[h][col] = bmap[h][col] == -1 ? 32 * H + row : -2;       // (-2: met twice)
            else if (D[l * 16 + r] != 0.0f) bmap[h][col] = -2;
        }
    }
}

static int main_f4f4()
{
    srand(23);
    int bmap[2][32];
    derive_bmap(bmap);
    for (int h = 0; h < 2; ++h) {
        printf("fp4 B lane half %d, nibble J (low half of byte J / 2 for even J) is k:", h);
        for (int J = 0; J < 32; ++J) {
            if (J % 16 == 0) printf("\n   ");
            if (bmap[h][J] < 0) printf(" J%-2d->?? ", J); else printf(" J%-2d->%-2d", J, bmap[h][J]);
        }
        printf("\n");
    }
    bool mirror = true;
    for (int h = 0; h < 2; ++h) for (int J = 0; J < 32; ++J) {
        mirror = mirror && bmap[h][J] == 32 * h + J;
        if (bmap[h][J] < 0) bmap[h][J] = 32 * h + J;
    }
    printf("B mirrors A (lane (r, h) holds column r, k = 32 h + J): %s\n", mirror ? "yes" : "NO");

    // all 16 codes on both sides; a different scale code 125 .. 129 in every byte of every lane's two scale registers
    std::vector<uint8_t> A(1024), B(1024);
    std::vector<uint32_t> SA(64), SB(64);
    for (auto &v : A) v = (uint8_t)(rand() & 255);
    for (auto &v : B) v = (uint8_t)(rand() & 255);
    for (auto &v : SA) { v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)(125 + rand() % 5) << (8 * i); }
    for (auto &v : SB) { v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)(125 + rand() % 5) << (8 * i); }
    static const char *rules[4] = {"lane 32 h + col", "lane col", "lane 32 + col", "lane 32 (k >> 5) + col"};
    for (int opb = 0; opb < 4; ++opb) {
        const int opa = (opb + 1) & 3;
        const std::vector<float> D = run44(A, B, SA, SB, opb, 0x5A5A5A5A);
        int best = 1025;
        for (int hi = 0; hi < 2; ++hi) for (int rule = 0; rule < 4; ++rule) for (int sb = 0; sb < 4; ++sb) {
            if (mirror && rule == 3) continue;                    // (the same hypothesis as rule 0 under the mirror map)
            const int bad = score44(D, A, B, SA, SB, opa, bmap, hi != 0, rule, sb);
            if (bad < best) best = bad;
            if (bad < 64)
                printf("op_sel A %d B %d: B %s nibble first, B scale = byte %d of %-22s mismatches %4d / 1024\n", opa, opb,
                       hi ? "high" : "low", sb, rules[rule], bad);
        }
        printf("op_sel A %d B %d: best hypothesis has %d mismatches\n", opa, opb, best);
        if (opb == 0) {
            const std::vector<float> D2 = run44(A, B, SA, SB, 0, 0x13572468);
            int diff = 0;
            for (int i = 0; i < 1024; ++i) diff += D[i] != D2[i];
            printf("registers 4 .. 7 of both fp4 operands changed: %d outputs differ\n", diff);
        }
    }

    // specials: B = 1.0 (code 2) at nibble 0 of lane `col 0, half 0` only, zero elsewhere; A = 1.0 everywhere, unit scales;
    // the B scale code under test in every byte of lane 0's B scale register
    auto special = [&](const char *name, uint32_t scode, bool zero_b, bool zero_a, int lane) {
        std::vector<uint8_t> a(1024, zero_a ? 0x00 : 0x22), b(1024, 0);
        std::vector<uint32_t> sa(64, 0x7F7F7F7Fu), sb(64, 0x7F7F7F7Fu);
        if (!zero_b) b[0] = 0x02;
        sb[lane] = scode * 0x01010101u;
        const std::vector<float> D = run44(a, b, sa, sb, 0, 0);
        int nans = 0, nan_col = 0;
        for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r)
            if (std::isnan(D[l * 16 + r])) { ++nans; nan_col += (l & 31) == (lane & 31); }
        uint32_t bits0;
        memcpy(&bits0, &D[0], 4);
        printf("%-62s D[row0][col0] = %g (0x%08x)  D[row0][col1] = %g   NaNs %d (in the column of the code: %d)\n", name, D[0], bits0,
               D[16], nans, nan_col);
    };
    special("B scale 127, B[col 0][k 0] = 1", 127, false, false, 0);
    special("B scale 0,   B[col 0][k 0] = 1", 0, false, false, 0);
    special("B scale 1,   B[col 0][k 0] = 1", 1, false, false, 0);
    special("B scale 254, B[col 0][k 0] = 1", 254, false, false, 0);
    special("B scale 255, B[col 0][k 0] = 1", 255, false, false, 0);
    special("B scale 255, B col 0 all zero codes", 255, true, false, 0);
    special("B scale 255, B col 0 all zero codes, A all zero codes", 255, true, true, 0);
    special("B scale 255 in lane 37 (col 5, half 1), all codes zero", 255, true, true, 37);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fp4 x e2m3 (cbsz = 4, blgp = 2).  a: 64 lanes x 16 bytes (registers 4 .. 7 are `junk`), b: 64 lanes x 24 bytes (registers
// 6 and 7 are `junk`); sa, sb: one dword of four scale bytes a lane for each side.
template <int OPA, int OPB>
__global__ void one46(const uint8_t *a, const uint8_t *b, const uint32_t *sa, const uint32_t *sb, float *d, int junk)
{
    const int l = threadIdx.x;
    v8i av, bv;
    for (int i = 0; i < 4; ++i) { av[i] = ((const int *)a)[l * 4 + i]; av[4 + i] = junk; }
    for (int i = 0; i < 6; ++i) bv[i] = ((const int *)b)[l * 6 + i];
    bv[6] = junk; bv[7] = junk;
    v16f acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 2, OPA, (int)sa[l], OPB, (int)sb[l]);
    for (int r = 0; r < 16; ++r) d[l * 16 + r] = acc[r];
}

static std::vector<float> run46(const std::vector<uint8_t> &A, const std::vector<uint8_t> &B, const std::vector<uint32_t> &SA,
                                const std::vector<uint32_t> &SB, int opb, int junk)
{
    uint8_t *da, *db; uint32_t *dsa, *dsb; float *dd;
    hipMalloc(&da, 1024); hipMalloc(&db, 1536); hipMalloc(&dsa, 256); hipMalloc(&dsb, 256); hipMalloc(&dd, 64 * 16 * 4);
    hipMemcpy(da, A.data(), 1024, hipMemcpyHostToDevice); hipMemcpy(db, B.data(), 1536, hipMemcpyHostToDevice);
    hipMemcpy(dsa, SA.data(), 256, hipMemcpyHostToDevice); hipMemcpy(dsb, SB.data(), 256, hipMemcpyHostToDevice);
    switch (opb) {
    case 0: hipLaunchKernelGGL((one46<1, 0>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    case 1: hipLaunchKernelGGL((one46<2, 1>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    case 2: hipLaunchKernelGGL((one46<3, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    default: hipLaunchKernelGGL((one46<0, 3>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd, junk); break;
    }
    std::vector<float> D(64 * 16);
    if (hipMemcpy(D.data(), dd, 64 * 16 * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error\n"); exit(1); }
    hipFree(da); hipFree(db); hipFree(dsa); hipFree(dsb); hipFree(dd);
    return D;
}

static float e2m3_to_float(int c)
{
    const int e = (c >> 3) & 3, m = c & 7;
    const float v = e == 0 ? m / 8.0f : ldexpf(1.0f + m / 8.0f, e - 1);
    return (c & 32) ? -v : v;
}
// field J (bits 6 J .. 6 J + 5 of the 24 bytes at p read as one little-endian integer)
static int get6(const uint8_t *p, int J)
{
    const int bit = 6 * J, w = p[bit >> 3] | (bit + 8 < 192 ? p[(bit >> 3) + 1] << 8 : 0);
    return (w >> (bit & 7)) & 63;
}
static void set6(uint8_t *p, int J, int c)
{
    const int bit = 6 * J, lo = bit & 7;
    p[bit >> 3] = (uint8_t)((p[bit >> 3] & ~(63 << lo)) | (c << lo));
    if (lo > 2) p[(bit >> 3) + 1] = (uint8_t)((p[(bit >> 3) + 1] & ~(63 >> (8 - lo))) | (c >> (8 - lo)));
}

// A as measured.  B hypothesis: field J of lane (col, h) is k = bmap[h][J]; its scale is byte sbyte of lane
//   0: 32 h + col (the lane's own)  1: col  2: 32 + col  3: 32 (k >> 5) + col (the lane of k's block).
static int score46(const std::vector<float> &D, const std::vector<uint8_t> &A, const std::vector<uint8_t> &B,
                   const std::vector<uint32_t> &SA, const std::vector<uint32_t> &SB, int opa, const int bmap[2][32],
                   int lane_rule, int sbyte)
{
    int bad = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
        const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        double av[64], bv[64];
        for (int H = 0; H < 2; ++H) for (int J = 0; J < 32; ++J) {
            const uint8_t ab = A[(H * 32 + row) * 16 + (J >> 1)];
            av[32 * H + J] = ldexp((double)e2m1_to_float((J & 1) ? ab >> 4 : ab & 15), (int)((SA[H * 32 + row] >> (8 * opa)) & 255) - 127);
            const int k = bmap[H][J];
            const int sl = lane_rule == 0 ? H * 32 + col : lane_rule == 1 ? col : lane_rule == 2 ? 32 + col : 32 * (k >> 5) + col;
            bv[k] = ldexp((double)e2m3_to_float(get6(&B[(H * 32 + col) * 24], J)), (int)((SB[sl] >> (8 * sbyte)) & 255) - 127);
        }
        double ref = 0;
        for (int k = 0; k < 64; ++k) ref += av[k] * bv[k];
        if (ref != (double)D[l * 16 + r]) ++bad;
    }
    return bad;
}

// One-hot map of B, as derive_bmap: A row i holds 1.0 at k = 32 H + i alone; B column c holds 1.0 (e2m3 code 8) in field
// J = c of its lane of half h alone.  D[row i][col c] is 1 exactly where field c of a B lane of half h is k = 32 H + i; any
// other value (a field that straddles the instruction's own boundaries reads as another number) marks the field -2.
static void derive_bmap6(int bmap[2][32])
{
    const std::vector<uint32_t> S(64, 0x7F7F7F7Fu);
    for (int h = 0; h < 2; ++h) for (int J = 0; J < 32; ++J) bmap[h][J] = -1;
    for (int h = 0; h < 2; ++h) for (int H = 0; H < 2; ++H) {
        std::vector<uint8_t> A(1024, 0), B(1536, 0);
        for (int i = 0; i < 32; ++i) A[(H * 32 + i) * 16 + (i >> 1)] = (uint8_t)(0x02 << (4 * (i & 1)));
        for (int c = 0; c < 32; ++c) set6(&B[(h * 32 + c) * 24], c, 8);
        const std::vector<float> D = run46(A, B, S, S, 0, 0);
        for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
            const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            if (D[l * 16 + r] == 1.0f) bmap[h][col] = bmap[h][col] == -1 ? 32 * H + row : -2;       // (-2: met twice)
            else if (D[l * 16 + r] != 0.0f) bmap[h][col] = -2;
        }
    }
}

static int main_f4f6()
{
    srand(37);
    int bmap[2][32];
    derive_bmap6(bmap);
    for (int h = 0; h < 2; ++h) {
        printf("e2m3 B lane half %d, field J (bits 6 J .. 6 J + 5 of the lane's 24 bytes, little endian) is k:", h);
        for (int J = 0; J < 32; ++J) {
            if (J % 16 == 0) printf("\n   ");
            if (bmap[h][J] < 0) printf(" J%-2d->?? ", J); else printf(" J%-2d->%-2d", J, bmap[h][J]);
        }
        printf("\n");
    }
    bool mirror = true;
    for (int h = 0; h < 2; ++h) for (int J = 0; J < 32; ++J) {
        mirror = mirror && bmap[h][J] == 32 * h + J;
        if (bmap[h][J] < 0) bmap[h][J] = 32 * h + J;
    }
    printf("B lane (r, h) holds column r, k = 32 h + J in field J: %s\n", mirror ? "yes" : "NO");

    // every code on both sides (16 of e2m1, 64 of e2m3); a different scale code 125 .. 129 in every byte of every lane's two
    // scale registers.  A product is a multiple of 2^-4, a scaled one of 2^-8, and 64 of them stay below 2^24 of those:
    // every float32 sum is exact in any order.
    std::vector<uint8_t> A(1024), B(1536);
    std::vector<uint32_t> SA(64), SB(64);
    for (auto &v : A) v = (uint8_t)(rand() & 255);
    for (auto &v : B) v = (uint8_t)(rand() & 255);
    for (auto &v : SA) { v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)(125 + rand() % 5) << (8 * i); }
    for (auto &v : SB) { v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)(125 + rand() % 5) << (8 * i); }
    static const char *rules[4] = {"lane 32 h + col", "lane col", "lane 32 + col", "lane 32 (k >> 5) + col"};
    for (int opb = 0; opb < 4; ++opb) {
        const int opa = (opb + 1) & 3;
        const std::vector<float> D = run46(A, B, SA, SB, opb, 0x5A5A5A5A);
        int best = 1025;
        for (int rule = 0; rule < 4; ++rule) for (int sb = 0; sb < 4; ++sb) {
            if (mirror && rule == 3) continue;                    // (the same hypothesis as rule 0 under this map)
            const int bad = score46(D, A, B, SA, SB, opa, bmap, rule, sb);
            if (bad < best) best = bad;
            if (bad < 64)
                printf("op_sel A %d B %d: B scale = byte %d of %-22s mismatches %4d / 1024\n", opa, opb, sb, rules[rule], bad);
        }
        printf("op_sel A %d B %d: best hypothesis has %d mismatches\n", opa, opb, best);
        if (opb == 0) {
            const std::vector<float> D2 = run46(A, B, SA, SB, 0, 0x13572468);
            int diff = 0;
            for (int i = 0; i < 1024; ++i) diff += D[i] != D2[i];
            printf("registers 4 .. 7 of the fp4 operand and 6, 7 of the e2m3 operand changed: %d outputs differ\n", diff);
        }
    }

    // specials: B = 1.0 (code 8) in field 0 of lane `col 0, half 0` only, zero elsewhere; A = 1.0 everywhere, unit scales;
    // the B scale code under test in every byte of one lane's B scale register
    auto special = [&](const char *name, uint32_t scode, bool zero_b, bool zero_a, int lane) {
        std::vector<uint8_t> a(1024, zero_a ? 0x00 : 0x22), b(1536, 0);
        std::vector<uint32_t> sa(64, 0x7F7F7F7Fu), sb(64, 0x7F7F7F7Fu);
        if (!zero_b) set6(&b[0], 0, 8);
        sb[lane] = scode * 0x01010101u;
        const std::vector<float> D = run46(a, b, sa, sb, 0, 0);
        int nans = 0, nan_col = 0;
        for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r)
            if (std::isnan(D[l * 16 + r])) { ++nans; nan_col += (l & 31) == (lane & 31); }
        uint32_t bits0;
        memcpy(&bits0, &D[0], 4);
        printf("%-62s D[row0][col0] = %g (0x%08x)  D[row0][col1] = %g   NaNs %d (in the column of the code: %d)\n", name, D[0], bits0,
               D[16], nans, nan_col);
    };
    special("B scale 127, B[col 0][k 0] = 1", 127, false, false, 0);
    special("B scale 0,   B[col 0][k 0] = 1", 0, false, false, 0);
    special("B scale 1,   B[col 0][k 0] = 1", 1, false, false, 0);
    special("B scale 254, B[col 0][k 0] = 1", 254, false, false, 0);
    special("B scale 255, B[col 0][k 0] = 1", 255, false, false, 0);
    special("B scale 255, B col 0 all zero codes", 255, true, false, 0);
    special("B scale 255, B col 0 all zero codes, A all zero codes", 255, true, true, 0);
    special("B scale 255 in lane 37 (col 5, half 1), all codes zero", 255, true, true, 37);
    return 0;
}
