/* Plain-C consumer of the FILTERED searches of the C ABI (include/mips_hip.h, mips_search_wide_sel / mips_range_search_sel): no
 * Python, no torch, host buffers and a HOST bitmap.  Built and run by tests/test_gpu_filtered.py::test_c_abi_sel_from_plain_c:
 *     gcc tests/c_abi_sel_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Index: n x d lattice values from a tiny LCG (exact in bf16, sums exact in fp32 / fp64), so the expected results are computed
 * right here with integer arithmetic and compared bit for bit.  The bitmap speaks about n + 13 rows and the index's rows start
 * at its bit 13 (sel_bit0 = 13, not a multiple of 8). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mips_last_error());   \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static unsigned lcg(unsigned* s) { return *s = *s * 1664525u + 1013904223u; }

int main(void) {
    const int64_t n = 3001, d = 128, nq = 9, bit0 = 13, nbits = n + bit0;
    const int k = 40;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    int* xi = malloc(sizeof(int) * n * d);
    int* qi = malloc(sizeof(int) * nq * d);
    float* x = malloc(sizeof(float) * n * d);
    float* q = malloc(sizeof(float) * nq * d);
    unsigned s = 97531u;
    for (int64_t i = 0; i < n * d; ++i) { xi[i] = (int)((lcg(&s) >> 16) % 255) - 127; x[i] = xi[i] / 64.0f; }
    for (int64_t i = 0; i < nq * d; ++i) { qi[i] = (int)((lcg(&s) >> 16) % 255) - 127; q[i] = qi[i] / 64.0f; }
    /* the selector: about one row in three, none of rows 1024 .. 1535 (four empty tiles), row n - 1 in */
    uint8_t* bits = calloc((nbits + 7) / 8, 1);
    char* on = calloc(n, 1);
    for (int64_t r = 0; r < n; ++r) {
        on[r] = ((lcg(&s) >> 16) % 3 == 0 && !(r >= 1024 && r < 1536)) || r == n - 1;
        if (on[r]) bits[(r + bit0) >> 3] |= (uint8_t)(1u << ((r + bit0) & 7));
    }
    for (int64_t b = 0; b < bit0; ++b) bits[b >> 3] |= (uint8_t)(1u << (b & 7)); /* bits before bit0 belong to other rows: all set */

    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP));
    CHECK(mips_index_add(ix, x, n, MIPS_DTYPE_F32, 0, NULL));

    long* val = malloc(sizeof(long) * nq * n); /* dot products in units of 1/4096 */
    for (int64_t a = 0; a < nq; ++a)
        for (int64_t r = 0; r < n; ++r) {
            long v = 0;
            for (int64_t c = 0; c < d; ++c) v += (long)qi[a * d + c] * xi[r * d + c];
            val[a * n + r] = v;
        }

    int bad = 0;
    /* ---- filtered wide search: the k best selected rows by (score descending, row ascending) */
    float* S = malloc(sizeof(float) * nq * k);
    int64_t* I = malloc(sizeof(int64_t) * nq * k);
    CHECK(mips_search_wide_sel(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 500, 0, bits, nbits, bit0, NULL));
    if (strstr(mips_index_last_kernel(ix), "masked_scan_kernel") == NULL) { fprintf(stderr, "last kernel is not the masked one\n"); return 1; }
    int64_t f = -1, rs = -1, u = -1;
    CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
    if (u != 0 || f != rs) { fprintf(stderr, "filtered wide search left queries unresolved\n"); return 1; }
    char* used = malloc(n);
    for (int64_t a = 0; a < nq; ++a) {
        memset(used, 0, n);
        for (int t = 0; t < k; ++t) {
            int64_t best = -1;
            for (int64_t r = 0; r < n; ++r)
                if (on[r] && !used[r] && (best < 0 || val[a * n + r] > val[a * n + best])) best = r;
            used[best] = 1;
            if (I[a * k + t] != best + 500 || S[a * k + t] != (float)((double)val[a * n + best] / 4096.0)) ++bad;
        }
    }
    /* ---- filtered range search: radius on the 25th selected value of each query (strict: it and its ties are out) */
    float* radii = malloc(sizeof(float) * nq);
    int64_t* elims = calloc(nq + 1, sizeof(int64_t));
    for (int64_t a = 0; a < nq; ++a) {
        radii[a] = S[a * k + 24];
        int64_t c = 0;
        for (int64_t r = 0; r < n; ++r) c += on[r] && (float)((double)val[a * n + r] / 4096.0) > radii[a];
        elims[a + 1] = elims[a] + c;
    }
    const int64_t total = elims[nq];
    int64_t* lims = malloc(sizeof(int64_t) * (nq + 1));
    float* D = malloc(sizeof(float) * (total + 1));
    int64_t* J = malloc(sizeof(int64_t) * (total + 1));
    CHECK(mips_range_search_sel(ix, q, MIPS_DTYPE_F32, nq, radii, lims, NULL, NULL, 0, 0, 0, bits, nbits, bit0, NULL)); /* counting call */
    for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
    CHECK(mips_range_search_sel(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, J, total, 500, 0, bits, nbits, bit0, NULL));
    for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
    for (int64_t a = 0; a < nq && bad == 0; ++a) {
        int64_t o = elims[a];
        for (int64_t r = 0; r < n; ++r) {
            const float v = (float)((double)val[a * n + r] / 4096.0);
            if (on[r] && v > radii[a]) {
                if (J[o] != r + 500 || D[o] != v) ++bad;
                ++o;
            }
        }
    }
    CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
    if (f != 0 || rs != 0 || u != 0) { fprintf(stderr, "margin stats of the range search not 0 / 0 / 0\n"); return 1; }
    /* ---- NULL bitmap: the unfiltered call, under its own kernel name */
    float* S0 = malloc(sizeof(float) * nq * k);
    int64_t* I0 = malloc(sizeof(int64_t) * nq * k);
    CHECK(mips_search_wide_sel(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL, 0, 0, NULL));
    CHECK(mips_search_wide(ix, q, MIPS_DTYPE_F32, nq, k, S0, I0, 0, 0, NULL));
    if (strncmp(mips_index_last_kernel(ix), "mips::wide_scan_kernel", 22) != 0) { fprintf(stderr, "unfiltered kernel name\n"); return 1; }
    bad += memcmp(S, S0, sizeof(float) * nq * k) != 0 || memcmp(I, I0, sizeof(int64_t) * nq * k) != 0;
    /* ---- a bitmap that does not cover the rows, a negative first bit */
    int rc = mips_search_wide_sel(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, bits, nbits - 1, bit0, NULL);
    if (rc != MIPS_E_INVALID || strlen(mips_last_error()) == 0) { fprintf(stderr, "too short a bitmap not rejected (wide)\n"); return 1; }
    rc = mips_range_search_sel(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, J, total, 0, 0, bits, n, bit0, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "too short a bitmap not rejected (range)\n"); return 1; }
    rc = mips_search_wide_sel(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, bits, nbits, -1, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "negative sel_bit0 not rejected\n"); return 1; }
    CHECK(mips_index_destroy(ix));
    printf("c_abi_sel_smoke: %lld queries x %lld docs, top-%d and %lld range hits\n", (long long)nq, (long long)n, k, (long long)total);
    printf("c_abi_sel_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
