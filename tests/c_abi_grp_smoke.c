/* Plain-C consumer of the GROUPED searches of the C ABI (include/mips_hip.h: mips_index_set_labels / mips_index_read_labels /
 * mips_search_wide_grp / mips_range_search_grp): no Python, no torch, host buffers, HOST labels and a HOST bitmap.  Built and run
 * by tests/test_gpu_grouped.py::test_c_abi_grp_from_plain_c:
 *     gcc tests/c_abi_grp_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Index: n x d lattice values from a tiny LCG (exact in bf16, sums exact in fp32 / fp64), so the expected results are computed
 * right here with integer arithmetic and compared bit for bit. */
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

static int admits(int32_t lab, int32_t ql, int mode) { return ql == MIPS_LABEL_NONE || ((lab == ql) == (mode == MIPS_GRP_ONLY)); }

int main(void) {
    const int64_t n = 3001, d = 128, nq = 9;
    const int k = 40;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    int* xi = malloc(sizeof(int) * n * d);
    int* qi = malloc(sizeof(int) * nq * d);
    float* x = malloc(sizeof(float) * n * d);
    float* q = malloc(sizeof(float) * nq * d);
    unsigned s = 24680u;
    for (int64_t i = 0; i < n * d; ++i) { xi[i] = (int)((lcg(&s) >> 16) % 255) - 127; x[i] = xi[i] / 64.0f; }
    for (int64_t i = 0; i < nq * d; ++i) { qi[i] = (int)((lcg(&s) >> 16) % 255) - 127; q[i] = qi[i] / 64.0f; }
    /* row labels 0 .. 6, but group 3 is small (30 rows: fewer than k); query labels: present ones, an absent one, NONE */
    int32_t* lab = malloc(sizeof(int32_t) * n);
    int small = 0;
    for (int64_t r = 0; r < n; ++r) {
        lab[r] = (int32_t)((lcg(&s) >> 16) % 7);
        if (lab[r] == 3 && ++small > 30) lab[r] = 4;
    }
    lab[n - 1] = MIPS_LABEL_NONE; /* a row may carry it: a group no query can name */
    int32_t ql[9] = {0, 1, 2, 3, 4, 5, 6, 100, MIPS_LABEL_NONE};
    /* the bitmap of the combined call: about one row in two, none of rows 1024 .. 1535 (four empty tiles) */
    uint8_t* bits = calloc((n + 7) / 8, 1);
    char* on = calloc(n, 1);
    for (int64_t r = 0; r < n; ++r) {
        on[r] = (lcg(&s) >> 16) % 2 == 0 && !(r >= 1024 && r < 1536);
        if (on[r]) bits[r >> 3] |= (uint8_t)(1u << (r & 7));
    }

    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP));
    CHECK(mips_index_add(ix, x, 2000, MIPS_DTYPE_F32, 0, NULL));
    float* S = malloc(sizeof(float) * nq * k);
    int64_t* I = malloc(sizeof(int64_t) * nq * k);
    /* never labelled: refused; labels in two batches around an add; a gap is refused */
    int rc = mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL, 0, 0, ql, MIPS_GRP_EXCLUDE, NULL);
    if (rc != MIPS_E_INVALID || strlen(mips_last_error()) == 0) { fprintf(stderr, "a never-labelled index was searched by group\n"); return 1; }
    CHECK(mips_index_set_labels(ix, lab, 0, 1500, 0, NULL));
    if (mips_index_set_labels(ix, lab + 1600, 1600, 100, 0, NULL) != MIPS_E_INVALID) { fprintf(stderr, "label gap not rejected\n"); return 1; }
    if (mips_index_set_labels(ix, lab + 1500, 1500, 501, 0, NULL) != MIPS_E_INVALID) { fprintf(stderr, "labels past ntotal not rejected\n"); return 1; }
    CHECK(mips_index_set_labels(ix, lab + 1500, 1500, 500, 0, NULL));
    CHECK(mips_index_add(ix, x + 2000 * d, n - 2000, MIPS_DTYPE_F32, 0, NULL));
    rc = mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL, 0, 0, ql, MIPS_GRP_EXCLUDE, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "rows added after labelling were searched by group\n"); return 1; }
    CHECK(mips_index_set_labels(ix, lab + 1990, 1990, n - 1990, 0, NULL)); /* (rewrites ten labelled rows) */
    int32_t* back = malloc(sizeof(int32_t) * n);
    CHECK(mips_index_read_labels(ix, 0, n, back, NULL));
    int bad = memcmp(back, lab, sizeof(int32_t) * n) != 0;
    if (mips_index_read_labels(ix, 1, n, back, NULL) != MIPS_E_INVALID) { fprintf(stderr, "read past the labelled rows not rejected\n"); return 1; }

    long* val = malloc(sizeof(long) * nq * n); /* dot products in units of 1/4096 */
    for (int64_t a = 0; a < nq; ++a)
        for (int64_t r = 0; r < n; ++r) {
            long v = 0;
            for (int64_t c = 0; c < d; ++c) v += (long)qi[a * d + c] * xi[r * d + c];
            val[a * n + r] = v;
        }

    /* ---- grouped wide search, both modes, without and with the bitmap: the k best admitted rows by (score descending, row
     * ascending), -1 / -inf once the admitted rows run out */
    char* used = malloc(n);
    int64_t f = -1, rs = -1, u = -1;
    for (int mode = 0; mode < 2; ++mode)
        for (int with_bits = 0; with_bits < 2; ++with_bits) {
            CHECK(mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 500, 0, with_bits ? bits : NULL, n, 0, ql, mode, NULL));
            if (strcmp(mips_index_last_kernel(ix), "mips::grouped_scan_kernel") != 0) { fprintf(stderr, "last kernel is not the grouped one\n"); return 1; }
            CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
            if (u != 0 || f != rs) { fprintf(stderr, "grouped wide search left queries unresolved\n"); return 1; }
            for (int64_t a = 0; a < nq; ++a) {
                memset(used, 0, n);
                for (int t = 0; t < k; ++t) {
                    int64_t best = -1;
                    for (int64_t r = 0; r < n; ++r)
                        if ((!with_bits || on[r]) && admits(lab[r], ql[a], mode) && !used[r] && (best < 0 || val[a * n + r] > val[a * n + best])) best = r;
                    if (best < 0) {
                        if (I[a * k + t] != -1 || !(S[a * k + t] == -INFINITY)) ++bad;
                        continue;
                    }
                    used[best] = 1;
                    if (I[a * k + t] != best + 500 || S[a * k + t] != (float)((double)val[a * n + best] / 4096.0)) ++bad;
                }
            }
        }
    /* ---- grouped range search (exclude mode, with the bitmap): radius on the 25th result of the unfiltered search */
    CHECK(mips_search_wide(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL));
    float* radii = malloc(sizeof(float) * nq);
    int64_t* elims = calloc(nq + 1, sizeof(int64_t));
    for (int64_t a = 0; a < nq; ++a) {
        radii[a] = S[a * k + 24];
        int64_t c = 0;
        for (int64_t r = 0; r < n; ++r) c += on[r] && admits(lab[r], ql[a], MIPS_GRP_EXCLUDE) && (float)((double)val[a * n + r] / 4096.0) > radii[a];
        elims[a + 1] = elims[a] + c;
    }
    const int64_t total = elims[nq];
    int64_t* lims = malloc(sizeof(int64_t) * (nq + 1));
    float* D = malloc(sizeof(float) * (total + 1));
    int64_t* J = malloc(sizeof(int64_t) * (total + 1));
    CHECK(mips_range_search_grp(ix, q, MIPS_DTYPE_F32, nq, radii, lims, NULL, NULL, 0, 0, 0, bits, n, 0, ql, MIPS_GRP_EXCLUDE, NULL)); /* counting call */
    for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
    CHECK(mips_range_search_grp(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, J, total, 500, 0, bits, n, 0, ql, MIPS_GRP_EXCLUDE, NULL));
    if (strcmp(mips_index_last_kernel(ix), "mips::grouped_scan_kernel") != 0) { fprintf(stderr, "range: last kernel is not the grouped one\n"); return 1; }
    for (int64_t a = 0; a <= nq; ++a) bad += lims[a] != elims[a];
    for (int64_t a = 0; a < nq && bad == 0; ++a) {
        int64_t o = elims[a];
        for (int64_t r = 0; r < n; ++r) {
            const float v = (float)((double)val[a * n + r] / 4096.0);
            if (on[r] && admits(lab[r], ql[a], MIPS_GRP_EXCLUDE) && v > radii[a]) {
                if (J[o] != r + 500 || D[o] != v) ++bad;
                ++o;
            }
        }
    }
    CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
    if (f != 0 || rs != 0 || u != 0) { fprintf(stderr, "margin stats of the range search not 0 / 0 / 0\n"); return 1; }
    /* ---- NULL q_labels: the _sel call (here: the unfiltered one), under its own kernel name */
    float* S0 = malloc(sizeof(float) * nq * k);
    int64_t* I0 = malloc(sizeof(int64_t) * nq * k);
    CHECK(mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S0, I0, 0, 0, NULL, 0, 0, NULL, 7, NULL));
    if (strncmp(mips_index_last_kernel(ix), "mips::wide_scan_kernel", 22) != 0) { fprintf(stderr, "unfiltered kernel name\n"); return 1; }
    bad += memcmp(S, S0, sizeof(float) * nq * k) != 0 || memcmp(I, I0, sizeof(int64_t) * nq * k) != 0;
    /* ---- a mode that does not exist; reset clears the labels */
    rc = mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL, 0, 0, ql, 2, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "grp_mode 2 not rejected (wide)\n"); return 1; }
    rc = mips_range_search_grp(ix, q, MIPS_DTYPE_F32, nq, radii, lims, D, J, total, 0, 0, NULL, 0, 0, ql, -1, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "grp_mode -1 not rejected (range)\n"); return 1; }
    CHECK(mips_index_reset(ix));
    CHECK(mips_index_add(ix, x, 100, MIPS_DTYPE_F32, 0, NULL));
    rc = mips_search_wide_grp(ix, q, MIPS_DTYPE_F32, nq, k, S, I, 0, 0, NULL, 0, 0, ql, MIPS_GRP_ONLY, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "labels survived mips_index_reset\n"); return 1; }
    CHECK(mips_index_destroy(ix));
    printf("c_abi_grp_smoke: %lld queries x %lld docs, top-%d and %lld range hits\n", (long long)nq, (long long)n, k, (long long)total);
    printf("c_abi_grp_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
