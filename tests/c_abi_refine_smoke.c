/* Plain-C consumer of include/mips_hip_refine.h: no Python, no torch, host buffers.  Compiled against the header by
 * tests/test_refine_host.py (gcc -c) and built and run by tests/test_gpu_refine.py::test_c_abi_refine_from_plain_c:
 *     gcc tests/c_abi_refine_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * A PQ index with a planted codebook and planted codes in front of an fp32-exact flat index of rows a little off their decoding: the candidates
 * (k = 40 > MIPS_MAX_K) and their re-ranking are restated here in C as the header words them and compared exactly. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_refine.h"

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

enum { N = 700, D = 8, M = 2, DSUB = 4, NQ = 3, KC = 40, K = 5, KSUB = 256 };

static float cb[M * KSUB * DSUB], q[NQ * D], x[N * D], lut[M][KSUB], adc[N], exact[N];
static uint8_t codes[N * M];
static float cand_d[NQ * KC], out_d[NQ * K], back[NQ * K];
static int64_t cand_i[NQ * KC], out_i[NQ * K];

static float dot(const float* a, const float* b, int n) { /* the canonical score */
    double acc = 0.0;
    for (int t = 0; t < n; ++t) acc += (double)a[t] * (double)b[t];
    return (float)acc;
}

/* the rank of row i under (score descending, row ascending) */
static int rank_of(const float* s, int i, const int64_t* among, int n) {
    int r = 0;
    for (int u = 0; u < n; ++u) {
        const int o = (int)among[u];
        if (o >= 0 && o != i && (s[o] > s[i] || (s[o] == s[i] && o < i))) ++r;
    }
    return r;
}

int main(void) {
    unsigned seed = 12345u;
    mips_pq_t* pq = NULL;
    mips_index_t* flat = NULL;
    static int64_t every[N];
    for (int i = 0; i < M * KSUB * DSUB; ++i) cb[i] = unit(&seed) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&seed) - 0.5f;
    for (int i = 0; i < N; ++i) {
        every[i] = i;
        for (int m = 0; m < M; ++m) {
            codes[i * M + m] = (uint8_t)(lcg(&seed) >> 24);
            /* the store holds the row a little off its decoding: the two stages rank differently */
            for (int t = 0; t < DSUB; ++t) x[i * D + m * DSUB + t] = cb[(m * KSUB + codes[i * M + m]) * DSUB + t] + 0.05f * (unit(&seed) - 0.5f);
        }
    }
    CHECK(mips_pq_create(&pq, 0, D, M, 8, MIPS_METRIC_IP));
    CHECK(mips_pq_set_codebook(pq, cb));
    CHECK(mips_pq_add_codes(pq, codes, N, 0, NULL));
    CHECK(mips_index_create(&flat, 0, D, MIPS_DTYPE_F32, MIPS_METRIC_IP));
    CHECK(mips_index_add(flat, x, N, MIPS_DTYPE_F32, 0, NULL));

    REFUSED(mips_pq_search_candidates(pq, q, MIPS_DTYPE_F32, NQ, 0, cand_d, cand_i, 0, 0, NULL), MIPS_E_INVALID, "k = 0");
    REFUSED(mips_pq_search_candidates(pq, q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K_WIDE + 1, cand_d, cand_i, 0, 0, NULL), MIPS_E_INVALID, "k = 1025");
    REFUSED(mips_index_rerank(flat, q, MIPS_DTYPE_F32, NQ, cand_i, KC, KC + 1, out_d, out_i, 0, 0, NULL), MIPS_E_INVALID, "k > kc");
    CHECK(mips_pq_search_candidates(pq, q, MIPS_DTYPE_F32, NQ, KC, cand_d, cand_i, 0, 0, NULL));
    cand_i[KC - 1] = cand_i[0]; /* a repeat and two ids that name no row: query 0 has KC - 3 distinct candidates */
    cand_i[KC - 2] = -1;
    cand_i[KC - 3] = N;
    CHECK(mips_index_rerank(flat, q, MIPS_DTYPE_F32, NQ, cand_i, KC, K, out_d, out_i, 0, 0, NULL));
    CHECK(mips_score_subset(flat, q, MIPS_DTYPE_F32, NQ, out_i, K, back, 0, 0, NULL));
    for (int j = 0; j < NQ; ++j) {
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < KSUB; ++c) lut[m][c] = dot(q + j * D + m * DSUB, cb + (m * KSUB + c) * DSUB, DSUB);
        for (int i = 0; i < N; ++i) {
            float acc = lut[0][codes[i * M]];
            for (int m = 1; m < M; ++m) acc = acc + lut[m][codes[i * M + m]];
            adc[i] = acc;
            exact[i] = dot(q + j * D, x + i * D, D);
        }
        if (j > 0) /* (query 0's candidates were edited above) */
            for (int u = 0; u < KC; ++u) {
                const int i = (int)cand_i[j * KC + u];
                if (i < 0 || i >= N || rank_of(adc, i, every, N) != u || memcmp(&cand_d[j * KC + u], &adc[i], 4) != 0) {
                    fprintf(stderr, "candidates: query %d slot %d\n", j, u);
                    return 1;
                }
            }
        for (int u = 0; u < K; ++u) {
            const int i = (int)out_i[j * K + u];
            if (i < 0 || i >= N || rank_of(exact, i, cand_i + j * KC, KC - (j == 0 ? 3 : 0)) != u || memcmp(&out_d[j * K + u], &exact[i], 4) != 0 ||
                memcmp(&out_d[j * K + u], &back[j * K + u], 4) != 0) {
                fprintf(stderr, "rerank: query %d slot %d\n", j, u);
                return 1;
            }
        }
    }
    CHECK(mips_pq_destroy(pq));
    CHECK(mips_index_destroy(flat));
    printf("c_abi_refine_smoke ok\n");
    return 0;
}
