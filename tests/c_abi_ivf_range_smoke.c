/* Plain-C consumer of mips_ivf_range_search / _grp (include/mips_hip_ivf_range.h): no Python, no torch, host buffers.  Compiled
 * against the header by tests/test_ivf_range_host.py (gcc -std=c11 -Wall -Werror -c) and built and run by
 * tests/test_gpu_ivf_range.py::test_c_abi_ivf_range_from_plain_c:
 *     gcc tests/c_abi_ivf_range_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * An SQ8 and an fp32-exact IVF index are trained, filled and searched with per-query radii taken from a top-K search; checked
 * without any restatement, by the identities of the definition: a counting call gives the limits of the full call; the hits of a
 * query ascend in row number, lie in probed lists and score above its radius; scoring them with mips_score_subset on the inner
 * index gives the returned scores bit for bit; the hits are exactly the entries of mips_ivf_search_wide above the radius; a capacity
 * one short still reports the true limits and leaves the guard entries alone; nprobe = nlist on the fp32 index gives
 * mips_range_search's result on the inner index bit for bit; the _grp entry without a filter is the unfiltered call and with one it
 * keeps the excluded label out; and the refusals answer with their codes. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_ivf_range.h"
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

enum { N = 3000, D = 100, NQ = 7, K = 100, NLIST = 8, CAP = N * NQ, GUARD = 4 };

static float x[N * D], q[NQ * D], radii[NQ];
static int32_t assign[N], labels[N], qlab[NQ], probes[NQ * NLIST];
static float S[NQ * K], RS[CAP + GUARD], RS2[CAP + GUARD];
static int64_t I[NQ * K], RI[CAP + GUARD], RI2[CAP + GUARD], lims[NQ + 1], lims2[NQ + 1];

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    unsigned s = 13579u;
    for (int i = 0; i < N * D; ++i) x[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    for (int i = 0; i < N; ++i) labels[i] = i % 10;
    for (int j = 0; j < NQ; ++j) qlab[j] = j == 3 ? MIPS_LABEL_NONE : j;
    int bad = 0;
    const int dtypes[2] = {MIPS_DTYPE_SQ8, MIPS_DTYPE_F32};
    for (int t = 0; t < 2; ++t) {
        mips_ivf_t* iv = NULL;
        CHECK(mips_ivf_create(&iv, 0, D, dtypes[t], MIPS_METRIC_IP, NLIST));
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, RI, CAP, 0, 0, NULL), MIPS_E_INVALID, "search before train");
        CHECK(mips_ivf_set_param(iv, "ivf_niter", 3));
        CHECK(mips_ivf_train(iv, x, N, MIPS_DTYPE_F32, 0, NULL));
        memset(lims, 0xff, sizeof lims); /* an empty index: all-zero limits */
        CHECK(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, RI, CAP, 0, 0, NULL));
        for (int j = 0; j <= NQ; ++j) bad += lims[j] != 0;
        CHECK(mips_ivf_add(iv, x, N, MIPS_DTYPE_F32, 0, NULL));
        CHECK(mips_ivf_read_assign(iv, 0, N, assign, NULL));
        mips_index_t* flat = mips_ivf_flat(iv);
        CHECK(mips_index_set_labels(flat, labels, 0, N, 0, NULL));
        for (int np = 1; np <= 3; np += 2) {
            /* radii from the wide search: query j gets the score of its (5 j + 2)-th best, query 6 +inf, query 5 -inf */
            CHECK(mips_ivf_search_wide(iv, q, MIPS_DTYPE_F32, NQ, K, np, S, I, 0, 0, NULL));
            CHECK(mips_ivf_probe(iv, q, MIPS_DTYPE_F32, NQ, np, probes, 0, NULL));
            for (int j = 0; j < NQ; ++j) radii[j] = S[j * K + 5 * j + 2];
            radii[6] = INFINITY;
            radii[5] = -INFINITY;
            CHECK(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, np, lims2, NULL, NULL, 0, 0, 0, NULL)); /* counting */
            for (int e = 0; e < CAP + GUARD; ++e) RS[e] = -7.f, RI[e] = -7;
            CHECK(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, np, lims, RS, RI, CAP, 0, 0, NULL));
            bad += memcmp(lims, lims2, sizeof lims) != 0 || lims[0] != 0 || lims[NQ] > CAP;
            for (int e = CAP; e < CAP + GUARD; ++e) bad += !(RI[e] == -7 && RS[e] == -7.f);
            bad += lims[7] != lims[6]; /* +inf: nothing */
            for (int j = 0; j < NQ; ++j) {
                const int64_t n = lims[j + 1] - lims[j];
                int above = 0;
                for (int e = 0; e < K; ++e) above += I[j * K + e] >= 0 && S[j * K + e] > radii[j];
                if (j != 5) bad += n != above; /* fewer than K hits: exactly the wide search's entries above the radius */
                for (int64_t e = lims[j]; e < lims[j + 1]; ++e) {
                    int in = 0, found = j == 5;
                    for (int u = 0; u < np; ++u) in |= probes[j * np + u] == assign[RI[e]];
                    for (int u = 0; u < K && !found; ++u) found = I[j * K + u] == RI[e] && memcmp(&S[j * K + u], &RS[e], 4) == 0;
                    bad += !in || !found || !(RS[e] > radii[j]) || (e > lims[j] && RI[e - 1] >= RI[e]);
                }
                if (n > 0) { /* scores by id */
                    CHECK(mips_score_subset(flat, q + j * D, MIPS_DTYPE_F32, 1, RI + lims[j], n, RS2, 0, 0, NULL));
                    bad += memcmp(RS2, RS + lims[j], (size_t)n * sizeof(float)) != 0;
                }
            }
            /* a capacity one short: true limits, nothing outside the arrays */
            if (lims[NQ] > 0) {
                const int64_t cap = lims[NQ] - 1;
                for (int e = 0; e < CAP + GUARD; ++e) RS2[e] = -9.f, RI2[e] = -9;
                CHECK(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, np, lims2, RS2, RI2, cap, 0, 0, NULL));
                bad += memcmp(lims, lims2, sizeof lims) != 0;
                for (int e = 0; e < GUARD; ++e) bad += !(RI2[cap + e] == -9 && RS2[cap + e] == -9.f);
            }
            /* the _grp entry without a filter is the unfiltered call (an offset on the rows); with one, the excluded label stays out */
            CHECK(mips_ivf_range_search_grp(iv, q, MIPS_DTYPE_F32, NQ, radii, np, lims2, RS2, RI2, CAP, 7000, 0, NULL, 0, 0, NULL, 0, NULL));
            bad += memcmp(lims, lims2, sizeof lims) != 0 || memcmp(RS, RS2, (size_t)lims[NQ] * sizeof(float)) != 0;
            for (int64_t e = 0; e < lims[NQ]; ++e) bad += RI2[e] != RI[e] + 7000;
            CHECK(mips_ivf_range_search_grp(iv, q, MIPS_DTYPE_F32, NQ, radii, np, lims2, RS2, RI2, CAP, 0, 0, NULL, 0, 0, qlab, MIPS_GRP_EXCLUDE, NULL));
            bad += lims2[4] - lims2[3] != lims[4] - lims[3]; /* MIPS_LABEL_NONE: unfiltered */
            for (int j = 0; j < NQ; ++j)
                for (int64_t e = lims2[j]; e < lims2[j + 1]; ++e) bad += j != 3 && labels[RI2[e]] == qlab[j];
        }
        /* every list probed: (fp32) the flat index's range search */
        if (dtypes[t] == MIPS_DTYPE_F32) {
            for (int j = 0; j < NQ; ++j) radii[j] = 0.3f * (float)j;
            CHECK(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 1000, lims, RS, RI, CAP, 0, 0, NULL)); /* nprobe > nlist */
            CHECK(mips_range_search(flat, q, MIPS_DTYPE_F32, NQ, radii, lims2, RS2, RI2, CAP, 0, 0, NULL));
            bad += memcmp(lims, lims2, sizeof lims) != 0 || lims[1] == 0;
            bad += memcmp(RS, RS2, (size_t)lims[NQ] * sizeof(float)) != 0 || memcmp(RI, RI2, (size_t)lims[NQ] * sizeof(int64_t)) != 0;
        }
        radii[2] = NAN;
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, RI, CAP, 0, 0, NULL), MIPS_E_INVALID, "a NaN radius");
        radii[2] = 0.f;
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 0, lims, RS, RI, CAP, 0, 0, NULL), MIPS_E_INVALID, "nprobe = 0");
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, NULL, RS, RI, CAP, 0, 0, NULL), MIPS_E_INVALID, "NULL lims");
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, NULL, CAP, 0, 0, NULL), MIPS_E_INVALID, "NULL output");
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, RI, -1, 0, 0, NULL), MIPS_E_INVALID, "cap < 0");
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_SQ8, NQ, radii, 2, lims, RS, RI, CAP, 0, 0, NULL), MIPS_E_INVALID, "queries as codes");
        REFUSED(mips_ivf_range_search(iv, q, MIPS_DTYPE_F32, NQ, radii, 2, lims, RS, RI, CAP, 0, MIPS_OUT_PACKED, NULL), MIPS_E_INVALID, "MIPS_OUT_PACKED");
        lims[0] = 5;
        CHECK(mips_ivf_range_search(iv, NULL, MIPS_DTYPE_F32, 0, NULL, 2, lims, NULL, NULL, 0, 0, 0, NULL)); /* nq = 0 */
        bad += lims[0] != 0;
        CHECK(mips_ivf_destroy(iv));
    }
    printf("c_abi_ivf_range_smoke: %d rows x %d, %d lists, %d queries, SQ8 and F32\n", N, D, NLIST, NQ);
    printf("c_abi_ivf_range_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
