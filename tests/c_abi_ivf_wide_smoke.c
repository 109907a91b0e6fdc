/* Plain-C consumer of mips_ivf_search_wide / _grp (include/mips_hip_ivf.h): no Python, no torch, host buffers.  Compiled against the
 * header by tests/test_ivf_wide_host.py (gcc -std=c11 -Wall -Werror -c) and built and run by
 * tests/test_gpu_ivf_wide.py::test_c_abi_ivf_wide_from_plain_c:
 *     gcc tests/c_abi_ivf_wide_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * An SQ8 and an fp32-exact IVF index are trained, filled and searched at k = 100; checked without any restatement, by the
 * identities of the definition: the first K0 columns are mips_ivf_search's, scoring the returned rows with mips_score_subset on the
 * inner index gives the returned scores bit for bit, every returned row lies in a probed list and no row comes twice, nprobe = nlist
 * on the fp32 index gives mips_search_wide's result on the inner index bit for bit, the _grp entry without a filter is the
 * unfiltered call, a group filter keeps the excluded label out, and the refusals answer with their codes. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_ivf.h"
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

enum { N = 3000, D = 100, NQ = 7, K = 100, K0 = 5, NLIST = 8 };

static float x[N * D], q[NQ * D];
static int32_t assign[N], labels[N], qlab[NQ], probes[NQ * NLIST];
static float S[NQ * K], S2[NQ * K], S0[NQ * K0];
static int64_t I[NQ * K], I2[NQ * K], I0[NQ * K0];
static char seen[N];

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    unsigned s = 24680u;
    for (int i = 0; i < N * D; ++i) x[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    memcpy(x + 1900 * D, x + 40 * D, sizeof(float) * D); /* row 1900 = row 40: a tie, and ... */
    for (int c = 0; c < D; ++c) q[c] = x[40 * D + c];     /* ... query 0 points at both */
    for (int i = 0; i < N; ++i) labels[i] = i % 10;
    for (int j = 0; j < NQ; ++j) qlab[j] = j == 3 ? MIPS_LABEL_NONE : j;
    int bad = 0;
    const int dtypes[2] = {MIPS_DTYPE_SQ8, MIPS_DTYPE_F32};
    for (int t = 0; t < 2; ++t) {
        mips_ivf_t* iv = NULL;
        CHECK(mips_ivf_create(&iv, 0, D, dtypes[t], MIPS_METRIC_IP, NLIST));
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 2, S, I, 0, 0, NULL), MIPS_E_INVALID, "search before train");
        CHECK(mips_ivf_set_param(iv, "ivf_niter", 3));
        CHECK(mips_ivf_train(iv, x, N, MIPS_DTYPE_F32, 0, NULL));
        /* an empty index: padding */
        CHECK(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 2, S, I, 0, 0, NULL));
        for (int e = 0; e < NQ * K; ++e) bad += !(I[e] == -1 && S[e] == -INFINITY);
        CHECK(mips_ivf_add(iv, x, N, MIPS_DTYPE_F32, 0, NULL));
        CHECK(mips_ivf_read_assign(iv, 0, N, assign, NULL));
        mips_index_t* flat = mips_ivf_flat(iv);
        CHECK(mips_index_set_labels(flat, labels, 0, N, 0, NULL));
        for (int np = 1; np <= 3; np += 2) {
            CHECK(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, np, S, I, 0, 0, NULL));
            CHECK(mips_ivf_search(iv, q, MIPS_DTYPE_F32, NQ, K0, np, S0, I0, 0, 0, NULL));
            CHECK(mips_ivf_probe(iv, q, MIPS_DTYPE_F32, NQ, np, probes, 0, NULL));
            CHECK(mips_score_subset(flat, q, MIPS_DTYPE_F32, NQ, I, K, S2, 0, 0, NULL));
            bad += memcmp(S, S2, sizeof S) != 0; /* (padding scores -inf on both sides) */
            for (int j = 0; j < NQ; ++j) {
                memset(seen, 0, sizeof seen);
                for (int e = 0; e < K0; ++e) bad += !(I[j * K + e] == I0[j * K0 + e] && memcmp(&S[j * K + e], &S0[j * K0 + e], 4) == 0); /* the prefix */
                for (int e = 0; e < K; ++e) {
                    const int64_t id = I[j * K + e];
                    if (id < 0) continue;
                    int in = 0;
                    for (int u = 0; u < np; ++u) in |= probes[j * np + u] == assign[id];
                    bad += !in || seen[id];
                    seen[id] = 1;
                    if (e > 0) bad += !(I[j * K + e - 1] >= 0 && S[j * K + e - 1] >= S[j * K + e]); /* padding last, scores descending */
                }
            }
            /* the _grp entry without a filter is the unfiltered call; with one, the excluded label stays out */
            CHECK(mips_ivf_search_wide_grp(iv, q, MIPS_DTYPE_F32, NQ, K, np, S2, I2, 0, 0, NULL, 0, 0, NULL, 0, NULL));
            bad += memcmp(S, S2, sizeof S) != 0 || memcmp(I, I2, sizeof I) != 0;
            CHECK(mips_ivf_search_wide_grp(iv, q, MIPS_DTYPE_F32, NQ, K, np, S2, I2, 0, 0, NULL, 0, 0, qlab, MIPS_GRP_EXCLUDE, NULL));
            for (int j = 0; j < NQ; ++j)
                for (int e = 0; e < K; ++e) {
                    const int64_t id = I2[j * K + e];
                    if (j == 3) bad += !(id == I[j * K + e]);
                    else if (id >= 0) bad += labels[id] == qlab[j];
                }
        }
        /* every list probed: an offset on the rows, and (fp32) the flat index's wide search */
        CHECK(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, NLIST, S, I, 0, 0, NULL));
        bad += !(I[0] == 40 && I[1] == 1900 && S[0] == S[1]);
        CHECK(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 1000, S2, I2, 7000, 0, NULL)); /* nprobe > nlist */
        for (int e = 0; e < NQ * K; ++e) bad += !(I2[e] == I[e] + 7000 && S2[e] == S[e]);
        if (dtypes[t] == MIPS_DTYPE_F32) {
            CHECK(mips_search_wide(flat, q, MIPS_DTYPE_F32, NQ, K, S2, I2, 0, 0, NULL));
            bad += memcmp(S, S2, sizeof S) != 0 || memcmp(I, I2, sizeof I) != 0;
        }
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, 0, 2, S, I, 0, 0, NULL), MIPS_E_INVALID, "k = 0");
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K_WIDE + 1, 2, S, I, 0, 0, NULL), MIPS_E_UNSUPPORTED, "k = 1025");
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 0, S, I, 0, 0, NULL), MIPS_E_INVALID, "nprobe = 0");
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 2, S, NULL, 0, 0, NULL), MIPS_E_INVALID, "NULL output");
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_SQ8, NQ, K, 2, S, I, 0, 0, NULL), MIPS_E_INVALID, "queries as codes");
        REFUSED(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, 2, S, I, 0, MIPS_OUT_PACKED, NULL), MIPS_E_INVALID, "MIPS_OUT_PACKED");
        REFUSED(mips_ivf_search(iv, q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K + 1, 2, S, I, 0, 0, NULL), MIPS_E_INVALID, "mips_ivf_search at k = 30, as before");
        CHECK(mips_ivf_search_wide(iv, NULL, MIPS_DTYPE_F32, 0, K, 2, NULL, NULL, 0, 0, NULL)); /* nq = 0 */
        CHECK(mips_ivf_destroy(iv));
    }
    printf("c_abi_ivf_wide_smoke: %d rows x %d, %d lists, %d queries, top-%d, SQ8 and F32\n", N, D, NLIST, NQ, K);
    printf("c_abi_ivf_wide_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
