/* Plain-C consumer of include/mips_hip_ivf_sharded.h: no Python, no torch.  Compiled against the header by
 * tests/test_ivf_sharded_host.py (gcc -std=c11 -Wall -Werror -c) and built and run by
 * tests/test_gpu_ivf_sharded.py::test_c_abi_ivf_sharded_from_plain_c:
 *     gcc tests/c_abi_ivf_sharded_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -L/opt/rocm/lib -lamdhip64 -lm
 * An SQ8 and an fp32-exact IVF index are trained on all the rows; THREE parts get the centroids (and the range) of the whole index and
 * the rows of their ranges (the last part is empty).  Every part is searched with mips_ivf_search_part (host form), the payloads are
 * laid end to end as an all-gather leaves them, and mips_ivf_merge_parts must give mips_ivf_search_wide's result on the whole index
 * bit for bit -- plain and under a global bitmap read from bit `lo` with query labels.  The refusals answer with their codes. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_ivf_sharded.h"
#include "mips_hip_sq8.h"

int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */
int hipDeviceSynchronize(void);

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

enum { N = 1000, D = 64, NQ = 5, K = 40, NLIST = 4, PARTS = 3, NBYTES = (N + 7) / 8 };
static const int64_t LO[PARTS + 1] = {0, 500, 1000, 1000}; /* the last part is empty */

static float x[N * D], q[NQ * D], cen[NLIST * D], vmin[D], vdiff[D];
static int32_t labels[N], qlab[NQ];
static uint8_t bits[NBYTES];
static float S[NQ * K], S2[NQ * K];
static int64_t I[NQ * K], I2[NQ * K];
static int64_t gathered[PARTS * NQ * K * 2];
static double bias[PARTS][NQ];

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    unsigned s = 13579u;
    for (int i = 0; i < N * D; ++i) x[i] = unit(&s) - 0.5f;
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    memcpy(x + 500 * D, x + 499 * D, sizeof(float) * D); /* rows 499 | 500: equal scores on both sides of the border, and ... */
    for (int c = 0; c < D; ++c) q[c] = x[499 * D + c];    /* ... query 0 points at both */
    for (int i = 0; i < N; ++i) labels[i] = i % 7;
    for (int j = 0; j < NQ; ++j) qlab[j] = j == 2 ? MIPS_LABEL_NONE : j;
    for (int i = 0; i < N; ++i)
        if (i % 3 != 1) bits[i >> 3] |= (uint8_t)(1u << (i & 7));
    int64_t* d_g = NULL;
    double* d_b = NULL;
    float* d_s = NULL;
    int64_t* d_i = NULL;
    if (hipMalloc((void**)&d_g, sizeof gathered) || hipMalloc((void**)&d_b, sizeof(double) * NQ) || hipMalloc((void**)&d_s, sizeof S) ||
        hipMalloc((void**)&d_i, sizeof I)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    int bad = 0;
    const int dtypes[2] = {MIPS_DTYPE_SQ8, MIPS_DTYPE_F32};
    for (int t = 0; t < 2; ++t) {
        const int sq8 = dtypes[t] == MIPS_DTYPE_SQ8;
        mips_ivf_t *full = NULL, *part[PARTS];
        CHECK(mips_ivf_create(&full, 0, D, dtypes[t], MIPS_METRIC_IP, NLIST));
        CHECK(mips_ivf_set_param(full, "ivf_niter", 3));
        CHECK(mips_ivf_train(full, x, N, MIPS_DTYPE_F32, 0, NULL));
        CHECK(mips_ivf_get_centroids(full, cen));
        if (sq8) CHECK(mips_index_sq8_get_params(mips_ivf_flat(full), vmin, vdiff));
        CHECK(mips_ivf_add(full, x, N, MIPS_DTYPE_F32, 0, NULL));
        CHECK(mips_index_set_labels(mips_ivf_flat(full), labels, 0, N, 0, NULL));
        for (int p = 0; p < PARTS; ++p) {
            const int64_t n = LO[p + 1] - LO[p];
            CHECK(mips_ivf_create(&part[p], 0, D, dtypes[t], MIPS_METRIC_IP, NLIST));
            CHECK(mips_ivf_set_centroids(part[p], cen));
            if (sq8) CHECK(mips_index_sq8_set_params(mips_ivf_flat(part[p]), vmin, vdiff));
            if (n > 0) {
                CHECK(mips_ivf_add(part[p], x + LO[p] * D, n, MIPS_DTYPE_F32, 0, NULL));
                CHECK(mips_index_set_labels(mips_ivf_flat(part[p]), labels + LO[p], 0, n, 0, NULL));
            }
        }
        for (int filtered = 0; filtered < 2; ++filtered)
            for (int np = 1; np <= NLIST; np += 3) {
                const uint8_t* sel = filtered ? bits : NULL;
                const int32_t* ql = filtered ? qlab : NULL;
                CHECK(mips_ivf_search_wide_grp(full, q, MIPS_DTYPE_F32, NQ, K, np, S, I, 0, 0, sel, 8 * NBYTES, 0, ql, MIPS_GRP_EXCLUDE, NULL));
                for (int p = 0; p < PARTS; ++p)
                    CHECK(mips_ivf_search_part(part[p], q, MIPS_DTYPE_F32, NQ, K, np, gathered + (size_t)p * NQ * K * 2, sq8 ? bias[p] : NULL, LO[p], 0, sel,
                                               8 * NBYTES, LO[p], ql, MIPS_GRP_EXCLUDE, NULL));
                if (sq8) bad += memcmp(bias[0], bias[1], sizeof bias[0]) != 0 || memcmp(bias[0], bias[2], sizeof bias[0]) != 0; /* B_q is replicated */
                for (int e = 0; e < NQ * K; ++e) { /* the empty part: padding, the offset not added */
                    const int64_t* w = gathered + ((size_t)2 * NQ * K + e) * 2;
                    float f;
                    const uint32_t u = (uint32_t)w[0];
                    memcpy(&f, &u, 4);
                    bad += !(w[1] == -1 && f == -INFINITY && (w[0] >> 32) == 0);
                }
                if (hipMemcpy(d_g, gathered, sizeof gathered, 1) || (sq8 && hipMemcpy(d_b, bias[1], sizeof bias[1], 1))) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
                CHECK(mips_ivf_merge_parts(d_g, PARTS, NQ, K, sq8 ? d_b : NULL, d_s, d_i, 0, NULL));
                hipDeviceSynchronize();
                hipMemcpy(S2, d_s, sizeof S2, 2);
                hipMemcpy(I2, d_i, sizeof I2, 2);
                bad += memcmp(S, S2, sizeof S) != 0 || memcmp(I, I2, sizeof I) != 0;
                if (!filtered && np == NLIST) bad += !(I2[0] == 499 && I2[1] == 500 && S2[0] == S2[1]); /* the tie across the border: lowest global row first */
            }
        REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, 0, 2, gathered, bias[0], 0, 0, NULL, 0, 0, NULL, 0, NULL), MIPS_E_INVALID, "k = 0");
        REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, MIPS_MAX_K_WIDE + 1, 2, gathered, bias[0], 0, 0, NULL, 0, 0, NULL, 0, NULL),
                MIPS_E_UNSUPPORTED, "k = 1025");
        REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, K, 0, gathered, bias[0], 0, 0, NULL, 0, 0, NULL, 0, NULL), MIPS_E_INVALID, "nprobe = 0");
        REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, K, 2, NULL, bias[0], 0, 0, NULL, 0, 0, NULL, 0, NULL), MIPS_E_INVALID, "NULL payload");
        REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, K, 2, gathered, bias[0], 0, MIPS_OUT_PACKED, NULL, 0, 0, NULL, 0, NULL), MIPS_E_INVALID,
                "MIPS_OUT_PACKED");
        if (sq8)
            REFUSED(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, K, 2, gathered, NULL, 0, 0, NULL, 0, 0, NULL, 0, NULL), MIPS_E_INVALID, "SQ8 without out_bias");
        else
            CHECK(mips_ivf_search_part(part[0], q, MIPS_DTYPE_F32, NQ, K, 2, gathered, NULL, 0, 0, NULL, 0, 0, NULL, 0, NULL)); /* no bias to write */
        CHECK(mips_ivf_search_part(part[0], NULL, MIPS_DTYPE_F32, 0, K, 2, NULL, NULL, 0, 0, NULL, 0, 0, NULL, 0, NULL)); /* nq = 0 */
        CHECK(mips_ivf_destroy(full));
        for (int p = 0; p < PARTS; ++p) CHECK(mips_ivf_destroy(part[p]));
    }
    REFUSED(mips_ivf_merge_parts(d_g, 0, NQ, K, NULL, d_s, d_i, 0, NULL), MIPS_E_INVALID, "parts = 0");
    REFUSED(mips_ivf_merge_parts(d_g, PARTS, NQ, 0, NULL, d_s, d_i, 0, NULL), MIPS_E_INVALID, "merge k = 0");
    REFUSED(mips_ivf_merge_parts(NULL, PARTS, NQ, K, NULL, d_s, d_i, 0, NULL), MIPS_E_INVALID, "NULL gathered");
    REFUSED(mips_ivf_merge_parts(d_g, 65, NQ, 1024, NULL, d_s, d_i, 0, NULL), MIPS_E_UNSUPPORTED, "parts * k > 65536");
    REFUSED(mips_ivf_merge_parts(d_g, 1, NQ, MIPS_MAX_K_WIDE + 1, NULL, d_s, d_i, 0, NULL), MIPS_E_UNSUPPORTED, "merge k = 1025");
    CHECK(mips_ivf_merge_parts(NULL, PARTS, 0, K, NULL, NULL, NULL, 0, NULL)); /* nq = 0 */
    hipFree(d_g);
    hipFree(d_b);
    hipFree(d_s);
    hipFree(d_i);
    printf("c_abi_ivf_sharded_smoke: %d rows x %d in %d parts, %d lists, %d queries, top-%d, SQ8 and F32\n", N, D, PARTS, NLIST, NQ, K);
    printf("c_abi_ivf_sharded_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
