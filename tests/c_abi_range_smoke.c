/* Plain-C consumer of the RANGE search of the C ABI (include/mips_hip.h, mips_range_search): no Python, no torch, host buffers only.
 * Built and run by tests/test_gpu_range.py::test_c_abi_range_from_plain_c:
 *     gcc tests/c_abi_range_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Index: n x d lattice values from a tiny LCG (exact in bf16, sums exact in fp32 / fp64), so the expected sets are computed right here
 * with integer arithmetic and compared bit for bit.  Radii sit ON the score of one of the query's own rows (strict: that row and its
 * ties are out) or one integer step on the permissive side of it (they are in).  The capacity protocol is exercised as a caller
 * would: a counting call (cap = 0, NULL arrays), a call with too small a cap, the repeat with the exact size. */
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

static long idot(const int* a, const int* b, int64_t d) {
    long s = 0;
    for (int64_t c = 0; c < d; ++c) s += (long)a[c] * b[c];
    return s;
}

int main(void) {
    const int64_t n = 9001, d = 768, nq = 37;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    int* xi = malloc(sizeof(int) * n * d);
    int* qi = malloc(sizeof(int) * nq * d);
    float* x = malloc(sizeof(float) * n * d);
    float* q = malloc(sizeof(float) * nq * d);
    unsigned s = 4321u;
    for (int64_t i = 0; i < n * d; ++i) { xi[i] = (int)((lcg(&s) >> 16) % 255) - 127; x[i] = xi[i] / 64.0f; }
    for (int64_t i = 0; i < nq * d; ++i) { qi[i] = (int)((lcg(&s) >> 16) % 255) - 127; q[i] = qi[i] / 64.0f; }
    memcpy(x + 17 * d, x + 8500 * d, sizeof(float) * d); /* a duplicate row: an exact tie in every query */
    memcpy(xi + 17 * d, xi + 8500 * d, sizeof(int) * d);

    long phi = 0; /* max |x|^2 in units of 1/4096 */
    for (int64_t r = 0; r < n; ++r) {
        const long v = idot(xi + r * d, xi + r * d, d);
        if (v > phi) phi = v;
    }

    int bad = 0;
    for (int metric = 0; metric < 2; ++metric) {
        mips_index_t* ix = NULL;
        CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, metric));
        CHECK(mips_index_add(ix, x, 3000, MIPS_DTYPE_F32, 0, NULL));
        CHECK(mips_index_add(ix, x + 3000 * d, n - 3000, MIPS_DTYPE_F32, 0, NULL));

        /* output value of every pair in units of 1/4096, the radii and the expected CSR */
        long* val = malloc(sizeof(long) * nq * n);
        long* rad = malloc(sizeof(long) * nq);
        float* radii = malloc(sizeof(float) * nq);
        int64_t* elims = calloc(nq + 1, sizeof(int64_t));
        for (int64_t a = 0; a < nq; ++a) {
            const long qq = idot(qi + a * d, qi + a * d, d);
            for (int64_t r = 0; r < n; ++r) {
                const long dot = idot(qi + a * d, xi + r * d, d);
                val[a * n + r] = metric ? qq + phi - 2 * dot : dot;
            }
            /* the query's 40th best value by a partial selection, then on it (even queries) or one step permissive (odd); query 5
             * sits on the duplicated pair */
            long* tmp = malloc(sizeof(long) * n);
            memcpy(tmp, val + a * n, sizeof(long) * n);
            for (int t = 0; t < 40; ++t) {
                int64_t best = t;
                for (int64_t r = t + 1; r < n; ++r)
                    if (metric ? tmp[r] < tmp[best] : tmp[r] > tmp[best]) best = r;
                const long sw = tmp[t]; tmp[t] = tmp[best]; tmp[best] = sw;
            }
            rad[a] = a == 5 ? val[a * n + 17] : tmp[39];
            free(tmp);
            /* one step: 4096 units keep the radius exact in float32 for L2 values beyond 2^24 units as well */
            if (a & 1) rad[a] += metric ? 4096 : -4096;
            radii[a] = (float)((double)rad[a] / 4096.0);
            if ((double)radii[a] * 4096.0 != (double)rad[a]) { fprintf(stderr, "radius %lld is not exact in float32\n", (long long)a); return 1; }
        }
        /* membership is decided on the float32 value of the score against the float32 radius */
        for (int64_t a = 0; a < nq; ++a) {
            int64_t c = 0;
            for (int64_t r = 0; r < n; ++r) {
                const float v = (float)((double)val[a * n + r] / 4096.0);
                c += metric ? v < radii[a] : v > radii[a];
            }
            elims[a + 1] = elims[a] + c;
        }
        const int64_t total = elims[nq];

        int64_t* lims = malloc(sizeof(int64_t) * (nq + 1));
        CHECK(mips_range_search(ix, q, MIPS_DTYPE_F32, nq, radii, lims, NULL, NULL, 0, 0, 0, NULL)); /* counting call */
        for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
        float* D = malloc(sizeof(float) * (total + 1));
        int64_t* I = malloc(sizeof(int64_t) * (total + 1));
        memset(lims, 0xff, sizeof(int64_t) * (nq + 1));
        CHECK(mips_range_search(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, I, total / 2, 0, 0, NULL)); /* too small: counts stay true */
        for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
        CHECK(mips_range_search(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, I, total, 1000, 0, NULL));  /* exact size, ids offset */
        for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
        for (int64_t a = 0; a < nq && bad == 0; ++a) {
            int64_t o = elims[a];
            for (int64_t r = 0; r < n; ++r) {
                const float v = (float)((double)val[a * n + r] / 4096.0);
                if (metric ? v < radii[a] : v > radii[a]) {
                    if (I[o] != r + 1000 || D[o] != v) ++bad;
                    ++o;
                }
            }
        }
        int64_t f = -1, rs = -1, u = -1;
        CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
        if (f != 0 || rs != 0 || u != 0) { fprintf(stderr, "margin stats not 0 / 0 / 0\n"); return 1; }
        if (strstr(mips_index_last_kernel(ix), "wide_scan_kernel") == NULL) { fprintf(stderr, "last kernel not named\n"); return 1; }
        int rc = mips_range_search(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, I, total, 0, MIPS_OUT_DEVICE | MIPS_OUT_PACKED, NULL);
        if (rc != MIPS_E_INVALID || strlen(mips_last_error()) == 0) { fprintf(stderr, "MIPS_OUT_PACKED not rejected\n"); return 1; }
        radii[3] = NAN;
        rc = mips_range_search(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, I, total, 0, 0, NULL);
        if (rc != MIPS_E_INVALID) { fprintf(stderr, "NaN radius not rejected\n"); return 1; }
        CHECK(mips_index_destroy(ix));
        printf("c_abi_range_smoke: metric %d, %lld queries x %lld docs, %lld hits\n", metric, (long long)nq, (long long)n, (long long)total);
        free(val); free(rad); free(radii); free(elims); free(lims); free(D); free(I);
    }
    printf("c_abi_range_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
