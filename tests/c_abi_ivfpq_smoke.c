/* Plain-C consumer of include/mips_hip_ivfpq.h: no Python, no torch, host buffers.  Compiled against the header by
 * tests/test_ivfpq_host.py (gcc -c) and built and run by tests/test_gpu_ivfpq.py::test_c_abi_ivfpq_from_plain_c:
 *     gcc tests/c_abi_ivfpq_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Planted centroids, codebook, codes and assignments: probe, table, score and ranking are restated here in C as the header words
 * them and compared exactly; then rows are added and their assignments, residual codes and decoded values are restated. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_ivfpq.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mips_last_error());   \
            return 1;                                                            \
        }                                                                        \
    } while (0)
#define REFUSED(call, code, what)                                                \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != (code) || strlen(mips_last_error()) == 0) {                   \
            fprintf(stderr, "%s: got %d, expected %d\n", what, rc_, (code));     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static unsigned lcg(unsigned* s) { return *s = *s * 1664525u + 1013904223u; }
static float unit(unsigned* s) { return (float)(lcg(s) >> 8) / 16777216.0f; } /* [0, 1) */

enum { N = 1500, D = 24, M = 8, DSUB = 3, NLIST = 6, NPROBE = 2, NQ = 5, K = 5, KSUB = 256 };

static float cen[NLIST * D], got_cen[NLIST * D], cb[M * KSUB * DSUB], got_cb[M * KSUB * DSUB], q[NQ * D], x[N * D], rec[K * D];
static uint8_t codes[N * M], got_codes[N * M];
static int32_t assign[N], got_assign[N], lists[NQ * NPROBE];
static float lut[M][KSUB], coarse[NLIST], score[N], T[NQ * NPROBE];

static float dot(const float* a, const float* b, int n) { /* the canonical score */
    double acc = 0.0;
    for (int t = 0; t < n; ++t) acc += (double)a[t] * (double)b[t];
    return (float)acc;
}

static int nearest(const float* v, const float* c) { /* strict: ties to the lowest centroid */
    int best = 0;
    double e_best = 0.0;
    for (int j = 0; j < KSUB; ++j) {
        double e = 0.0;
        for (int t = 0; t < DSUB; ++t) {
            const float u = v[t] - c[j * DSUB + t];
            e += (double)u * (double)u;
        }
        if (j == 0 || e < e_best) {
            best = j;
            e_best = e;
        }
    }
    return best;
}

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    unsigned s = 24680u;
    for (int i = 0; i < NLIST * D; ++i) cen[i] = 4.0f * (unit(&s) - 0.5f);
    for (int i = 0; i < M * KSUB * DSUB; ++i) cb[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    for (int i = 0; i < N * D; ++i) x[i] = cen[(i / D % NLIST) * D + i % D] + unit(&s) - 0.5f;
    for (int i = 0; i < N * M; ++i) codes[i] = (uint8_t)(lcg(&s) >> 24);
    for (int i = 0; i < N; ++i) assign[i] = (int32_t)((lcg(&s) >> 16) % NLIST);
    memcpy(codes + 9 * M, codes + 4 * M, M); /* row 9 = row 4, same list: a tie */
    assign[9] = assign[4];

    mips_ivfpq_t* ix = NULL;
    REFUSED(mips_ivfpq_create(&ix, 0, D, NLIST, M, 8, 1, MIPS_METRIC_L2), MIPS_E_UNSUPPORTED, "L2 create");
    if (strstr(mips_last_error(), "inner product") == NULL) { fprintf(stderr, "L2 refusal does not say why\n"); return 1; }
    REFUSED(mips_ivfpq_create(&ix, 0, D, NLIST, M, 4, 1, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "nbits 4");
    REFUSED(mips_ivfpq_create(&ix, 0, 2048, NLIST, M, 8, 1, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "d > 1024");
    REFUSED(mips_ivfpq_create(&ix, 0, 516, NLIST, 129, 8, 1, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "M > 128");
    REFUSED(mips_ivfpq_create(&ix, 0, D, 0, M, 8, 1, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "nlist 0");
    REFUSED(mips_ivfpq_create(&ix, 0, D, 65537, M, 8, 1, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "nlist > 65536");
    REFUSED(mips_ivfpq_create(&ix, 0, D, NLIST, 7, 8, 1, MIPS_METRIC_IP), MIPS_E_INVALID, "d % M != 0");
    CHECK(mips_ivfpq_create(&ix, 0, D, NLIST, M, 8, 1, MIPS_METRIC_IP));
    if (mips_ivfpq_is_trained(ix) != 0 || mips_ivfpq_m(ix) != M || mips_ivfpq_nlist(ix) != NLIST || mips_ivfpq_ntotal(ix) != 0) {
        fprintf(stderr, "fresh index\n");
        return 1;
    }
    REFUSED(mips_ivfpq_add_codes(ix, codes, assign, N, 0, NULL), MIPS_E_INVALID, "add_codes before train");
    REFUSED(mips_ivfpq_train(ix, x, KSUB - 1, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "n < 256");
    x[17 * D + 9] = INFINITY;
    REFUSED(mips_ivfpq_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on an infinity");
    x[17 * D + 9] = 0.125f;
    CHECK(mips_ivfpq_set_param(ix, "ivf_niter", 1));
    CHECK(mips_ivfpq_set_param(ix, "pq_niter", 1));
    REFUSED(mips_ivfpq_set_param(ix, "no_such", 2), MIPS_E_INVALID, "unknown parameter");
    CHECK(mips_ivfpq_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL));
    if (mips_ivfpq_is_trained(ix) != 1) { fprintf(stderr, "train left the index untrained\n"); return 1; }
    CHECK(mips_ivfpq_set_centroids(ix, cen));
    CHECK(mips_ivfpq_set_codebook(ix, cb));
    CHECK(mips_ivfpq_get_centroids(ix, got_cen));
    CHECK(mips_ivfpq_get_codebook(ix, got_cb));
    int bad = memcmp(cen, got_cen, sizeof cen) != 0 || memcmp(cb, got_cb, sizeof cb) != 0;

    assign[700] = NLIST;
    REFUSED(mips_ivfpq_add_codes(ix, codes, assign, N, 0, NULL), MIPS_E_INVALID, "an assignment outside [0, nlist)");
    assign[700] = 3;
    CHECK(mips_ivfpq_add_codes(ix, codes, assign, 700, 0, NULL));
    CHECK(mips_ivfpq_add_codes(ix, codes + 700 * M, assign + 700, N - 700, 0, NULL));
    REFUSED(mips_ivfpq_set_centroids(ix, cen), MIPS_E_INVALID, "set_centroids on a filled index");
    REFUSED(mips_ivfpq_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on a filled index");
    CHECK(mips_ivfpq_read_codes(ix, 0, N, got_codes, NULL));
    CHECK(mips_ivfpq_read_assign(ix, 0, N, got_assign, NULL));
    bad += memcmp(codes, got_codes, sizeof codes) != 0 || memcmp(assign, got_assign, sizeof assign) != 0;
    int64_t sizes[NLIST];
    CHECK(mips_ivfpq_list_sizes(ix, sizes, NULL));
    for (int l = 0; l < NLIST; ++l) {
        int64_t c = 0;
        for (int i = 0; i < N; ++i) c += assign[i] == l;
        bad += sizes[l] != c;
    }

    float S[NQ * K], S2[NQ * K];
    int64_t I[NQ * K];
    REFUSED(mips_ivfpq_search(ix, q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K + 1, NPROBE, S, I, 0, 0, NULL), MIPS_E_INVALID, "k > MIPS_MAX_K");
    REFUSED(mips_ivfpq_search(ix, q, MIPS_DTYPE_F32, NQ, K, 0, S, I, 0, 0, NULL), MIPS_E_INVALID, "nprobe 0");
    CHECK(mips_ivfpq_probe(ix, q, MIPS_DTYPE_F32, NQ, NPROBE, lists, T, 0, NULL));
    CHECK(mips_ivfpq_search(ix, q, MIPS_DTYPE_F32, NQ, K, NPROBE, S, I, 1000, 0, NULL));
    for (int j = 0; j < NQ; ++j) {
        int probed[NLIST] = {0};
        for (int l = 0; l < NLIST; ++l) coarse[l] = dot(q + j * D, cen + l * D, D);
        for (int u = 0; u < NPROBE; ++u) { /* the u-th nearest list: highest score, ties to the lowest list */
            int best = -1;
            for (int l = 0; l < NLIST; ++l)
                if (!probed[l] && (best < 0 || coarse[l] > coarse[best])) best = l;
            probed[best] = 1;
            bad += lists[j * NPROBE + u] != best || memcmp(&T[j * NPROBE + u], &coarse[best], 4) != 0;
        }
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < KSUB; ++c) lut[m][c] = dot(q + j * D + m * DSUB, cb + (m * KSUB + c) * DSUB, DSUB);
        for (int i = 0; i < N; ++i) {
            float acc = coarse[assign[i]];
            for (int m = 0; m < M; ++m) acc = acc + lut[m][codes[i * M + m]];
            score[i] = probed[assign[i]] ? acc : NAN;
        }
        for (int t = 0; t < K; ++t) { /* the t-th best probed row: highest score, ties to the lowest row */
            int best = -1;
            for (int i = 0; i < N; ++i)
                if (!isnan(score[i]) && (best < 0 || score[i] > score[best])) best = i;
            bad += I[j * K + t] != best + 1000 || memcmp(&S[j * K + t], &score[best], 4) != 0;
            score[best] = NAN; /* taken */
        }
    }
    CHECK(mips_ivfpq_score_subset(ix, q, MIPS_DTYPE_F32, NQ, I, K, S2, 1000, 0, NULL));
    bad += memcmp(S, S2, sizeof S) != 0;
    CHECK(mips_ivfpq_reconstruct(ix, I, K, 1000, rec, MIPS_DTYPE_F32, D, 0, NULL));
    for (int t = 0; t < K; ++t) {
        const int r = (int)(I[t] - 1000);
        for (int c = 0; c < D; ++c) {
            const float want = cen[assign[r] * D + c] + cb[((c / DSUB) * KSUB + codes[r * M + c / DSUB]) * DSUB + c % DSUB];
            bad += memcmp(rec + t * D + c, &want, 4) != 0;
        }
    }

    CHECK(mips_ivfpq_reset(ix));
    if (mips_ivfpq_is_trained(ix) != 1 || mips_ivfpq_ntotal(ix) != 0) { fprintf(stderr, "reset dropped the training or kept rows\n"); return 1; }
    CHECK(mips_ivfpq_search(ix, q, MIPS_DTYPE_F32, 1, K, NPROBE, S, I, 0, 0, NULL)); /* an empty index: padding */
    for (int t = 0; t < K; ++t) bad += I[t] != -1 || !(S[t] == -INFINITY);
    CHECK(mips_ivfpq_add(ix, x, N, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_ivfpq_read_codes(ix, 0, N, got_codes, NULL));
    CHECK(mips_ivfpq_read_assign(ix, 0, N, got_assign, NULL));
    for (int i = 0; i < N; ++i) {
        int best = 0;
        float r[D];
        for (int l = 0; l < NLIST; ++l) coarse[l] = dot(x + i * D, cen + l * D, D);
        for (int l = 1; l < NLIST; ++l)
            if (coarse[l] > coarse[best]) best = l;
        bad += got_assign[i] != best;
        for (int c = 0; c < D; ++c) r[c] = x[i * D + c] - cen[best * D + c];
        for (int m = 0; m < M; ++m) bad += got_codes[i * M + m] != nearest(r + m * DSUB, cb + m * KSUB * DSUB);
    }
    CHECK(mips_ivfpq_destroy(ix));
    printf("c_abi_ivfpq_smoke: %d rows x %d, %d lists, M = %d, %d queries, nprobe %d, top-%d\n", N, D, NLIST, M, NQ, NPROBE, K);
    printf("c_abi_ivfpq_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
