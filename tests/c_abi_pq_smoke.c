/* Plain-C consumer of include/mips_hip_pq.h: no Python, no torch, host buffers.  Compiled against the header by
 * tests/test_pq_host.py (gcc -c) and built and run by tests/test_gpu_pq.py::test_c_abi_pq_from_plain_c:
 *     gcc tests/c_abi_pq_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * A planted codebook and planted codes: table, score and ranking are restated here in C as the header words them and compared
 * exactly; then the same rows are encoded by the library and by the restatement. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_pq.h"
#include "mips_hip_rows.h"

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

enum { N = 1500, D = 24, M = 8, DSUB = 3, NQ = 5, K = 5, KSUB = 256 };

static float cb[M * KSUB * DSUB], got_cb[M * KSUB * DSUB], q[NQ * D], x[N * D], rec[K * D];
static uint8_t codes[N * M], got_codes[N * M];
static float lut[NQ][M][KSUB], score[N];

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
    unsigned s = 13579u;
    for (int i = 0; i < M * KSUB * DSUB; ++i) cb[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    for (int i = 0; i < N * D; ++i) x[i] = unit(&s) - 0.5f;
    for (int i = 0; i < N * M; ++i) codes[i] = (uint8_t)(lcg(&s) >> 24);
    memcpy(codes + 9 * M, codes + 4 * M, M); /* row 9 = row 4: a tie */

    mips_pq_t* pq = NULL;
    REFUSED(mips_pq_create(&pq, 0, D, M, 8, MIPS_METRIC_L2), MIPS_E_UNSUPPORTED, "L2 create");
    if (strstr(mips_last_error(), "inner product") == NULL) { fprintf(stderr, "L2 refusal does not say why\n"); return 1; }
    REFUSED(mips_pq_create(&pq, 0, D, M, 4, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "nbits 4");
    REFUSED(mips_pq_create(&pq, 0, 2048, M, 8, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "d > 1024");
    REFUSED(mips_pq_create(&pq, 0, 516, 129, 8, MIPS_METRIC_IP), MIPS_E_UNSUPPORTED, "M > 128");
    REFUSED(mips_pq_create(&pq, 0, D, 7, 8, MIPS_METRIC_IP), MIPS_E_INVALID, "d % M != 0");
    CHECK(mips_pq_create(&pq, 0, D, M, 8, MIPS_METRIC_IP));
    if (mips_pq_is_trained(pq) != 0 || mips_pq_m(pq) != M || mips_pq_ntotal(pq) != 0) { fprintf(stderr, "fresh index\n"); return 1; }
    REFUSED(mips_pq_add_codes(pq, codes, N, 0, NULL), MIPS_E_INVALID, "add_codes before train");
    REFUSED(mips_pq_train(pq, x, KSUB - 1, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "n < 256");
    x[17 * D + 9] = INFINITY;
    REFUSED(mips_pq_train(pq, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on an infinity");
    x[17 * D + 9] = 0.125f;
    CHECK(mips_pq_set_param(pq, "pq_niter", 1));
    REFUSED(mips_pq_set_param(pq, "no_such", 2), MIPS_E_INVALID, "unknown parameter");
    CHECK(mips_pq_train(pq, x, N, MIPS_DTYPE_F32, 0, NULL));
    if (mips_pq_is_trained(pq) != 1) { fprintf(stderr, "train left the index untrained\n"); return 1; }
    CHECK(mips_pq_set_codebook(pq, cb));
    CHECK(mips_pq_get_codebook(pq, got_cb));
    int bad = memcmp(cb, got_cb, sizeof cb) != 0;

    CHECK(mips_pq_add_codes(pq, codes, 700, 0, NULL));
    CHECK(mips_pq_add_codes(pq, codes + 700 * M, N - 700, 0, NULL));
    REFUSED(mips_pq_set_codebook(pq, cb), MIPS_E_INVALID, "set_codebook on a filled index");
    REFUSED(mips_pq_train(pq, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on a filled index");
    CHECK(mips_pq_read_codes(pq, 0, N, got_codes, NULL));
    bad += memcmp(codes, got_codes, sizeof codes) != 0;

    float S[NQ * K], S2[NQ * K];
    int64_t I[NQ * K];
    REFUSED(mips_pq_search(pq, q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K + 1, S, I, 0, 0, NULL), MIPS_E_INVALID, "k > MIPS_MAX_K");
    CHECK(mips_pq_search(pq, q, MIPS_DTYPE_F32, NQ, K, S, I, 1000, 0, NULL));
    for (int j = 0; j < NQ; ++j) {
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < KSUB; ++c) {
                double acc = 0.0;
                for (int t = 0; t < DSUB; ++t) acc += (double)q[j * D + m * DSUB + t] * (double)cb[(m * KSUB + c) * DSUB + t];
                lut[j][m][c] = (float)acc;
            }
        for (int i = 0; i < N; ++i) {
            float acc = lut[j][0][codes[i * M]];
            for (int m = 1; m < M; ++m) acc = acc + lut[j][m][codes[i * M + m]];
            score[i] = acc;
        }
        for (int t = 0; t < K; ++t) { /* the t-th best: highest score, ties to the lowest row */
            int best = -1;
            for (int i = 0; i < N; ++i)
                if (!isnan(score[i]) && (best < 0 || score[i] > score[best])) best = i;
            bad += I[j * K + t] != best + 1000 || memcmp(&S[j * K + t], &score[best], 4) != 0;
            score[best] = NAN; /* taken */
        }
    }
    CHECK(mips_pq_score_subset(pq, q, MIPS_DTYPE_F32, NQ, I, K, S2, 1000, 0, NULL));
    bad += memcmp(S, S2, sizeof S) != 0;
    CHECK(mips_pq_reconstruct(pq, I, K, 1000, rec, MIPS_DTYPE_F32, D, 0, NULL));
    for (int t = 0; t < K; ++t)
        for (int m = 0; m < M; ++m)
            bad += memcmp(rec + t * D + m * DSUB, cb + (m * KSUB + codes[(I[t] - 1000) * M + m]) * DSUB, sizeof(float) * DSUB) != 0;

    CHECK(mips_pq_reset(pq));
    if (mips_pq_is_trained(pq) != 1 || mips_pq_ntotal(pq) != 0) { fprintf(stderr, "reset dropped the codebook or kept rows\n"); return 1; }
    CHECK(mips_pq_search(pq, q, MIPS_DTYPE_F32, 1, K, S, I, 0, 0, NULL)); /* an empty index: padding */
    for (int t = 0; t < K; ++t) bad += I[t] != -1 || !(S[t] == -INFINITY);
    CHECK(mips_pq_add(pq, x, N, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_pq_read_codes(pq, 0, N, got_codes, NULL));
    for (int i = 0; i < N; ++i)
        for (int m = 0; m < M; ++m) bad += got_codes[i * M + m] != nearest(x + i * D + m * DSUB, cb + m * KSUB * DSUB);
    CHECK(mips_pq_destroy(pq));
    printf("c_abi_pq_smoke: %d rows x %d, M = %d, %d queries, top-%d\n", N, D, M, NQ, K);
    printf("c_abi_pq_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
