/* Plain-C consumer of the second header of the C ABI (include/mips_hip_sharded.h, mips_range_merge_records): no Python, no torch.
 * Built and run by tests/test_gpu_range_sharded.py::test_c_abi_range_merge_from_plain_c:
 *     gcc tests/c_abi_range_merge_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -L/opt/rocm/lib -lamdhip64 -lm
 * The entry point takes DEVICE pointers only, so this program needs four calls of the HIP runtime -- allocate, copy in, copy out,
 * synchronise -- which it declares itself (their C signatures are stable) instead of including the HIP headers.
 * Two hand-written records of 3 queries (stride 5, odd: the score region ends in half a word) are merged; the expected CSR triple is
 * written out below.  Then the capacity protocol: a counting call (cap = 0, NULL arrays), a cap below the total (counts stay true,
 * nothing at or past cap is written), and the refusals. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mips_hip_sharded.h"

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

#define NQ 3
#define STRIDE 5
#define PARTS 2
#define WORDS MIPS_RANGE_RECORD_WORDS(NQ, STRIDE)

static void fill(int64_t* rec, const int64_t* lims, const int64_t* ids, const float* scores, int m) {
    float sc[STRIDE + 1];
    for (int i = 0; i <= NQ; ++i) rec[i] = lims[i];
    for (int i = 0; i < STRIDE; ++i) rec[NQ + 1 + i] = i < m ? ids[i] : -7;   /* unused entries: a sentinel id and NaN */
    for (int i = 0; i <= STRIDE; ++i) sc[i] = i < m ? scores[i] : NAN;
    memcpy(rec + NQ + 1 + STRIDE, sc, sizeof(sc));
}

int main(void) {
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    if (WORDS != 4 + 5 + 3) { fprintf(stderr, "MIPS_RANGE_RECORD_WORDS(3, 5) != 12\n"); return 1; }
    /* part 0: rows below 1000; query 1 has no hit.  part 1: rows from 1000 on (beyond int32 in one id); query 0 has no hit */
    const int64_t lims0[] = {0, 2, 2, 5}, ids0[] = {3, 90, 7, 8, 999};
    const float sc0[] = {0.5f, 1.5f, -2.0f, 3.25f, 4.0f};
    const int64_t lims1[] = {0, 0, 3, 4}, ids1[] = {1000, 1001, ((int64_t)1 << 33) + 5, 1500};
    const float sc1[] = {10.0f, 11.0f, 12.0f, 13.0f};
    const int64_t elims[] = {0, 2, 5, 9};
    const int64_t eids[] = {3, 90, 1000, 1001, ((int64_t)1 << 33) + 5, 7, 8, 999, 1500};
    const float esc[] = {0.5f, 1.5f, 10.0f, 11.0f, 12.0f, -2.0f, 3.25f, 4.0f, 13.0f};
    enum { TOTAL = 9, GUARD = 4 };

    int64_t host[PARTS * WORDS];
    fill(host, lims0, ids0, sc0, 5);
    fill(host + WORDS, lims1, ids1, sc1, 4);

    int64_t *d_rec, *d_lims, *d_idx, *d_work;
    float* d_sc;
    if (hipMalloc((void**)&d_rec, sizeof(host)) || hipMalloc((void**)&d_lims, sizeof(int64_t) * (NQ + 1)) ||
        hipMalloc((void**)&d_idx, sizeof(int64_t) * (TOTAL + GUARD)) || hipMalloc((void**)&d_sc, sizeof(float) * (TOTAL + GUARD)) ||
        hipMalloc((void**)&d_work, sizeof(int64_t) * PARTS * NQ)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    if (hipMemcpy(d_rec, host, sizeof(host), 1)) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }

    int bad = 0;
    int64_t lims[NQ + 1], idx[TOTAL + GUARD];
    float sc[TOTAL + GUARD];

    /* the counting call */
    CHECK(mips_range_merge_records(d_rec, PARTS, NQ, STRIDE, d_lims, NULL, NULL, 0, d_work, 0, NULL));
    hipDeviceSynchronize();
    hipMemcpy(lims, d_lims, sizeof(lims), 2);
    for (int i = 0; i <= NQ; ++i) bad += lims[i] != elims[i];

    /* the merge, with a guard behind the exact capacity */
    for (int i = 0; i < TOTAL + GUARD; ++i) { idx[i] = -99; sc[i] = 123.0f; }
    hipMemcpy(d_idx, idx, sizeof(idx), 1);
    hipMemcpy(d_sc, sc, sizeof(sc), 1);
    CHECK(mips_range_merge_records(d_rec, PARTS, NQ, STRIDE, d_lims, d_sc, d_idx, TOTAL, d_work, 0, NULL));
    hipDeviceSynchronize();
    hipMemcpy(lims, d_lims, sizeof(lims), 2);
    hipMemcpy(idx, d_idx, sizeof(idx), 2);
    hipMemcpy(sc, d_sc, sizeof(sc), 2);
    for (int i = 0; i <= NQ; ++i) bad += lims[i] != elims[i];
    for (int i = 0; i < TOTAL; ++i) bad += idx[i] != eids[i] || memcmp(&sc[i], &esc[i], sizeof(float)) != 0;
    for (int i = TOTAL; i < TOTAL + GUARD; ++i) bad += idx[i] != -99 || sc[i] != 123.0f;

    /* cap below the total: the counts stay true, nothing at or past cap is written */
    for (int i = 0; i < TOTAL + GUARD; ++i) { idx[i] = -99; sc[i] = 123.0f; }
    hipMemcpy(d_idx, idx, sizeof(idx), 1);
    hipMemcpy(d_sc, sc, sizeof(sc), 1);
    CHECK(mips_range_merge_records(d_rec, PARTS, NQ, STRIDE, d_lims, d_sc, d_idx, 4, d_work, 0, NULL));
    hipDeviceSynchronize();
    hipMemcpy(lims, d_lims, sizeof(lims), 2);
    hipMemcpy(idx, d_idx, sizeof(idx), 2);
    hipMemcpy(sc, d_sc, sizeof(sc), 2);
    for (int i = 0; i <= NQ; ++i) bad += lims[i] != elims[i];
    for (int i = 4; i < TOTAL + GUARD; ++i) bad += idx[i] != -99 || sc[i] != 123.0f;

    /* refusals */
    if (mips_range_merge_records(d_rec, 0, NQ, STRIDE, d_lims, d_sc, d_idx, TOTAL, d_work, 0, NULL) != MIPS_E_INVALID ||
        strlen(mips_last_error()) == 0) { fprintf(stderr, "parts = 0 not rejected\n"); return 1; }
    if (mips_range_merge_records(d_rec, PARTS, NQ, STRIDE, d_lims, NULL, d_idx, TOTAL, d_work, 0, NULL) != MIPS_E_INVALID) {
        fprintf(stderr, "NULL scores with cap > 0 not rejected\n"); return 1; }
    if (mips_range_merge_records(d_rec, PARTS, NQ, STRIDE, d_lims, d_sc, d_idx, TOTAL, NULL, 0, NULL) != MIPS_E_INVALID) {
        fprintf(stderr, "NULL workspace not rejected\n"); return 1; }
    if (mips_range_merge_records(d_rec, PARTS, ((int64_t)1 << 24) + 1, STRIDE, d_lims, d_sc, d_idx, TOTAL, d_work, 0, NULL) != MIPS_E_UNSUPPORTED) {
        fprintf(stderr, "nq > 2^24 not refused\n"); return 1; }
    /* nq = 0: one limit, 0 */
    lims[0] = -1;
    hipMemcpy(d_lims, lims, sizeof(int64_t), 1);
    CHECK(mips_range_merge_records(d_rec, PARTS, 0, 0, d_lims, NULL, NULL, 0, NULL, 0, NULL));
    hipDeviceSynchronize();
    hipMemcpy(lims, d_lims, sizeof(int64_t), 2);
    bad += lims[0] != 0;

    hipFree(d_rec); hipFree(d_lims); hipFree(d_idx); hipFree(d_sc); hipFree(d_work);
    printf("c_abi_range_merge_smoke: %d parts, %d queries, %d hits\n", PARTS, NQ, TOTAL);
    printf("c_abi_range_merge_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
