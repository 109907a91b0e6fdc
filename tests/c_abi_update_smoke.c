/* Plain-C consumer of mips_index_update and mips_ivf_update (include/mips_hip_write.h): no Python, no torch, host buffers.  Built
 * and run by tests/test_gpu_update.py::test_c_abi_update_from_plain_c:
 *     gcc tests/c_abi_update_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Rows are small integers (exact in bf16), so everything expected here is integer arithmetic: the rows after the update are
 * those of the sequential loop run in C, read back and compared element by element; a search for an updated row finds it under
 * its OLD number with the integer score |x|^2; the IVF index moves a row between two lists whose centroids are axis vectors. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_write.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mips_last_error());   \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static unsigned lcg(unsigned* s) { return *s = *s * 1664525u + 1013904223u; }
static uint16_t bf16_of(float v) { uint32_t u; memcpy(&u, &v, 4); return (uint16_t)(u >> 16); } /* small integers: the upper half */

int main(void) {
    const int64_t n = 3001, d = 100, m = 700, off = ((int64_t)1 << 33) + 11;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    float* x = malloc(sizeof(float) * n * d);
    float* y = malloc(sizeof(float) * m * d);
    int64_t* ids = malloc(sizeof(int64_t) * m);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t c = 0; c < d; ++c) x[r * d + c] = (float)((r * 7 + c * 3) % 15 - 7);
    unsigned s = 97531u;
    for (int64_t p = 0; p < m; ++p) {
        for (int64_t c = 0; c < d; ++c) y[p * d + c] = (float)((p * 5 + c * 11) % 13 - 6);
        ids[p] = off + (int64_t)((lcg(&s) >> 8) % (unsigned)n); /* random rows: some twice */
    }
    ids[0] = off + n - 1, ids[1] = off;                     /* both ends */
    ids[3] = ids[4] = ids[255] = ids[256] = ids[m - 1] = off + 1717; /* five copies across the workgroups of both passes */
    ids[10] = -1, ids[11] = off + n, ids[12] = off + ((int64_t)1 << 32) + 3, ids[13] = off - 1, ids[14] = 3; /* none names a row */
    /* the sequential loop */
    float* want = malloc(sizeof(float) * n * d);
    char* hit = calloc(n, 1);
    memcpy(want, x, sizeof(float) * n * d);
    int64_t distinct = 0;
    for (int64_t p = 0; p < m; ++p) {
        const int64_t local = ids[p] - off; /* (no overflow for these ids) */
        if (local < 0 || local >= n) continue;
        memcpy(want + local * d, y + p * d, sizeof(float) * d);
        distinct += !hit[local];
        hit[local] = 1;
    }
    int bad = 0;
    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP));
    CHECK(mips_index_add(ix, x, n, MIPS_DTYPE_F32, 0, NULL));
    int64_t count = -7;
    /* refusals first: they must leave the index alone */
    if (mips_index_update(NULL, ids, m, off, y, MIPS_DTYPE_F32, 0, &count, NULL) != MIPS_E_INVALID || strlen(mips_last_error()) == 0) ++bad;
    if (mips_index_update(ix, ids, -1, off, y, MIPS_DTYPE_F32, 0, &count, NULL) != MIPS_E_INVALID) ++bad;
    if (mips_index_update(ix, NULL, m, off, y, MIPS_DTYPE_F32, 0, &count, NULL) != MIPS_E_INVALID) ++bad;
    if (mips_index_update(ix, ids, m, off, NULL, MIPS_DTYPE_F32, 0, &count, NULL) != MIPS_E_INVALID) ++bad;
    if (mips_index_update(ix, ids, m, off, y, MIPS_DTYPE_FP8_E4M3, 0, &count, NULL) != MIPS_E_INVALID) ++bad; /* bytes into a bf16 index */
    if (mips_index_update(ix, ids, (int64_t)1 << 31, off, y, MIPS_DTYPE_F32, 0, &count, NULL) != MIPS_E_UNSUPPORTED) ++bad;
    CHECK(mips_index_update(ix, NULL, 0, off, NULL, MIPS_DTYPE_F32, 0, &count, NULL)); /* n == 0 */
    bad += count != 0;
    uint16_t* got = malloc(sizeof(uint16_t) * n * d);
    CHECK(mips_index_read_rows(ix, 0, n, got, NULL));
    for (int64_t t = 0; t < n * d; ++t) bad += got[t] != bf16_of(x[t]);

    CHECK(mips_index_update(ix, ids, m, off, y, MIPS_DTYPE_F32, 0, &count, NULL));
    bad += count != distinct || mips_index_ntotal(ix) != n;
    CHECK(mips_index_read_rows(ix, 0, n, got, NULL));
    for (int64_t t = 0; t < n * d; ++t) bad += got[t] != bf16_of(want[t]);
    CHECK(mips_index_update(ix, ids, m, off, y, MIPS_DTYPE_F32, 0, NULL, NULL)); /* no count asked for; the same rows again */
    CHECK(mips_index_read_rows(ix, 0, n, got, NULL));
    for (int64_t t = 0; t < n * d; ++t) bad += got[t] != bf16_of(want[t]);
    /* one row becomes 9 times the last update row: the search finds it under its old number, score 9 |y|^2 -- an integer
     * no other row can reach (|x| <= 7 sqrt(d)) */
    float* big = malloc(sizeof(float) * d);
    int64_t yy = 0;
    for (int64_t c = 0; c < d; ++c) {
        big[c] = 9.0f * y[(m - 1) * d + c];
        yy += (int64_t)y[(m - 1) * d + c] * (int64_t)y[(m - 1) * d + c];
    }
    const int64_t one = off + 2000;
    CHECK(mips_index_update(ix, &one, 1, off, big, MIPS_DTYPE_F32, 0, &count, NULL));
    float S[2];
    int64_t I[2];
    CHECK(mips_search(ix, y + (m - 1) * d, MIPS_DTYPE_F32, 1, 1, S, I, off, 0, NULL));
    bad += count != 1 || I[0] != off + 2000 || S[0] != (float)(9 * yy);
    CHECK(mips_index_destroy(ix));

    /* the IVF index: two lists, centroids e_0 and e_1; rows alternate between them; row 5 moves from list 1 to list 0 */
    const int64_t dv = 64, nv = 40;
    float* cent = calloc(2 * dv, sizeof(float));
    float* xv = calloc(nv * dv, sizeof(float));
    cent[0] = 1.0f, cent[dv + 1] = 1.0f;
    for (int64_t r = 0; r < nv; ++r) xv[r * dv + (r & 1)] = (float)(r + 1), xv[r * dv + 7] = 1.0f;
    mips_ivf_t* v = NULL;
    CHECK(mips_ivf_create(&v, 0, dv, MIPS_DTYPE_F32, MIPS_METRIC_IP, 2));
    CHECK(mips_ivf_set_centroids(v, cent));
    CHECK(mips_ivf_add(v, xv, nv, MIPS_DTYPE_F32, 0, NULL));
    float* moved = calloc(2 * dv, sizeof(float));
    moved[0] = 50.0f;        /* position 0: list 0 ...            */
    moved[dv + 0] = 100.0f;  /* position 1, the same row: it wins */
    const int64_t vid[3] = {5, 5, -1};
    float three[3 * 64];
    memset(three, 0, sizeof three);
    memcpy(three, moved, sizeof(float) * 2 * dv);
    uint8_t codes[64] = {0};
    if (mips_ivf_update(v, vid, 1, 0, codes, MIPS_DTYPE_SQ8, 0, &count, NULL) != MIPS_E_UNSUPPORTED) ++bad; /* raw codes */
    CHECK(mips_ivf_update(v, vid, 3, 0, three, MIPS_DTYPE_F32, 0, &count, NULL));
    int32_t as[40];
    int64_t sizes[2];
    CHECK(mips_ivf_read_assign(v, 0, nv, as, NULL));
    CHECK(mips_ivf_list_sizes(v, sizes, NULL));
    bad += count != 1 || sizes[0] != nv / 2 + 1 || sizes[1] != nv / 2 - 1;
    for (int64_t r = 0; r < nv; ++r) bad += as[r] != (r == 5 ? 0 : (int32_t)(r & 1));
    float q[64] = {0};
    q[0] = 1.0f;
    CHECK(mips_ivf_search(v, q, MIPS_DTYPE_F32, 1, 2, 1, S, I, 0, 0, NULL)); /* nprobe 1: list 0 only */
    bad += I[0] != 5 || S[0] != 100.0f || I[1] != 38 || S[1] != 39.0f;
    CHECK(mips_ivf_destroy(v));
    printf("c_abi_update_smoke: %lld positions, %lld distinct rows written\n", (long long)m, (long long)distinct);
    printf("c_abi_update_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
