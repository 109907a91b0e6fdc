/* Plain-C consumer of include/mips_hip_ivf.h: no Python, no torch, host buffers.  Compiled against the header by
 * tests/test_ivf_host.py (gcc -c) and built and run by tests/test_gpu_ivf.py::test_c_abi_ivf_from_plain_c:
 *     gcc tests/c_abi_ivf_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * An fp32-exact IVF index with planted centroids (the unit vectors): lists, assignments and probes are restated here in C as the
 * header words them and compared exactly. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_ivf.h"

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

enum { N = 1500, D = 100, NQ = 6, K = 5, NLIST = 4 };

static float score(const float* a, const float* b) {
    double acc = 0.0;
    for (int c = 0; c < D; ++c) acc += (double)a[c] * (double)b[c];
    return (float)acc;
}

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    static float x[N * D], q[NQ * D], cen[NLIST * D], got_cen[NLIST * D];
    static int32_t assign[N], got_assign[N], probes[NQ * NLIST];
    unsigned s = 24680u;
    for (int i = 0; i < N * D; ++i) x[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    for (int l = 0; l < NLIST; ++l) cen[l * D + l] = 1.0f;
    memcpy(x + 9 * D, x + 4 * D, sizeof(float) * D); /* row 9 = row 4: a tie, and ... */
    for (int c = 0; c < D; ++c) q[c] = x[4 * D + c];  /* ... query 0 points at both */

    mips_ivf_t* iv = NULL;
    REFUSED(mips_ivf_create(&iv, 0, D, MIPS_DTYPE_F32, MIPS_METRIC_L2, NLIST), MIPS_E_UNSUPPORTED, "L2 create");
    if (strstr(mips_last_error(), "inner product") == NULL) { fprintf(stderr, "L2 refusal does not say why\n"); return 1; }
    REFUSED(mips_ivf_create(&iv, 0, 2000, MIPS_DTYPE_F32, MIPS_METRIC_IP, NLIST), MIPS_E_UNSUPPORTED, "d > 1024");
    REFUSED(mips_ivf_create(&iv, 0, D, MIPS_DTYPE_FP8_E4M3, MIPS_METRIC_IP, NLIST), MIPS_E_UNSUPPORTED, "e4m3 storage");
    REFUSED(mips_ivf_create(&iv, 0, D, MIPS_DTYPE_F32, MIPS_METRIC_IP, 0), MIPS_E_UNSUPPORTED, "nlist 0");
    REFUSED(mips_ivf_create(&iv, 0, D, MIPS_DTYPE_F32, MIPS_METRIC_IP, 65537), MIPS_E_UNSUPPORTED, "nlist 65537");
    CHECK(mips_ivf_create(&iv, 0, D, MIPS_DTYPE_F32, MIPS_METRIC_IP, NLIST));
    if (mips_ivf_is_trained(iv) != 0 || mips_ivf_nlist(iv) != NLIST) { fprintf(stderr, "fresh index\n"); return 1; }
    REFUSED(mips_ivf_add(iv, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "add before train");
    REFUSED(mips_ivf_train(iv, x, NLIST - 1, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "n < nlist");
    x[17 * D + 9] = INFINITY;
    REFUSED(mips_ivf_train(iv, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on an infinity");
    x[17 * D + 9] = 0.125f;
    CHECK(mips_ivf_set_param(iv, "ivf_niter", 2));
    REFUSED(mips_ivf_set_param(iv, "no_such", 2), MIPS_E_INVALID, "unknown parameter");
    CHECK(mips_ivf_train(iv, x, N, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_ivf_set_centroids(iv, cen));
    CHECK(mips_ivf_get_centroids(iv, got_cen));
    int bad = memcmp(cen, got_cen, sizeof cen) != 0;

    int64_t sizes[NLIST], want_sizes[NLIST] = {0, 0, 0, 0};
    uint8_t codes[D];
    memset(codes, 0, sizeof codes);
    REFUSED(mips_ivf_add(iv, codes, 1, MIPS_DTYPE_SQ8, 0, NULL), MIPS_E_UNSUPPORTED, "raw codes as rows");
    CHECK(mips_ivf_add(iv, x, 700, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_ivf_add(iv, x + 700 * D, N - 700, MIPS_DTYPE_F32, 0, NULL));
    REFUSED(mips_ivf_set_centroids(iv, cen), MIPS_E_INVALID, "set_centroids on a filled index");
    REFUSED(mips_ivf_train(iv, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on a filled index");
    for (int r = 0; r < N; ++r) { /* the nearest list: highest score, ties to the lowest list */
        int best = 0;
        for (int l = 1; l < NLIST; ++l)
            if (score(x + r * D, cen + l * D) > score(x + r * D, cen + best * D)) best = l;
        assign[r] = best;
        ++want_sizes[best];
    }
    CHECK(mips_ivf_read_assign(iv, 0, N, got_assign, NULL));
    CHECK(mips_ivf_list_sizes(iv, sizes, NULL));
    bad += memcmp(assign, got_assign, sizeof assign) != 0 || memcmp(sizes, want_sizes, sizeof sizes) != 0;
    if (mips_index_ntotal(mips_ivf_flat(iv)) != N) { fprintf(stderr, "flat ntotal\n"); return 1; }

    for (int np = 1; np <= NLIST; np += NLIST - 1) { /* nprobe = 1 and nprobe = nlist */
        CHECK(mips_ivf_probe(iv, q, MIPS_DTYPE_F32, NQ, np, probes, 0, NULL));
        for (int j = 0; j < NQ; ++j) {
            char probed[NLIST];
            memset(probed, 0, sizeof probed);
            for (int t = 0; t < np; ++t) { /* the t-th nearest list not taken yet */
                int best = -1;
                for (int l = 0; l < NLIST; ++l)
                    if (!probed[l] && (best < 0 || score(q + j * D, cen + l * D) > score(q + j * D, cen + best * D))) best = l;
                probed[best] = 1;
                bad += probes[j * np + t] != best;
            }
        }
    }
    REFUSED(mips_ivf_probe(iv, q, MIPS_DTYPE_F32, NQ, 0, probes, 0, NULL), MIPS_E_INVALID, "nprobe 0");
    { /* the inner index holds the rows in arrival order and searches them exactly: row 9 = row 4 tie, lowest first */
        float S[NQ * K];
        int64_t I[NQ * K];
        CHECK(mips_search(mips_ivf_flat(iv), q, MIPS_DTYPE_F32, NQ, K, S, I, 0, 0, NULL));
        bad += !(I[0] == 4 && I[1] == 9 && S[0] == S[1]);
    }
    CHECK(mips_ivf_reset(iv));
    CHECK(mips_ivf_list_sizes(iv, sizes, NULL));
    for (int l = 0; l < NLIST; ++l) bad += sizes[l] != 0;
    if (mips_ivf_is_trained(iv) != 1) { fprintf(stderr, "reset dropped the centroids\n"); return 1; }
    CHECK(mips_ivf_destroy(iv));
    printf("c_abi_ivf_smoke: %d rows x %d, %d lists, %d queries, top-%d\n", N, D, NLIST, NQ, K);
    printf("c_abi_ivf_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
