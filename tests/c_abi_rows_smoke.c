/* Plain-C consumer of include/mips_hip_rows.h: no Python, no torch, HOST ids and HOST output.  Built and run by
 * tests/test_gpu_rows.py::test_c_abi_rows_from_plain_c:
 *     gcc tests/c_abi_rows_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Rows are small integers (exact in bf16) that name their row, so what comes back is checked right here: rows at a row pitch
 * wider than d (the elements between the rows must stay as they were), raw bf16 bits, the NaN row of a -1 id, labels, the
 * refusal of an id past the index, and the scores of a search's ids against its distances, bit for bit. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_rows.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mips_last_error());   \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(void) {
    enum { N = 3001, D = 100, LD = 104, NIDS = 300, NLAB = 2000, NQ = 7, K = 5 };
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    float* x = malloc(sizeof(float) * N * D);
    int32_t* lab = malloc(sizeof(int32_t) * N);
    for (int64_t r = 0; r < N; ++r) {
        for (int64_t c = 0; c < D; ++c) x[r * D + c] = (float)((r * 7 + c * 3) % 255 - 127);
        lab[r] = (int32_t)(r % 11);
    }
    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, D, MIPS_DTYPE_BF16, MIPS_METRIC_L2));
    CHECK(mips_index_add(ix, x, N, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_index_set_labels(ix, lab, 0, NLAB, 0, NULL)); /* a partial labelled prefix */

    /* ids in global numbering of a shard that starts at row 1000: every 10th row backwards, a -1 and an id below the shard */
    const int64_t off = 1000;
    int64_t ids[NIDS];
    for (int i = 0; i < NIDS; ++i) ids[i] = off + (N - 1) - 10 * (int64_t)i;
    ids[17] = -1;
    ids[18] = off - 1;
    int bad = 0;

    float* out = malloc(sizeof(float) * NIDS * LD);
    for (int i = 0; i < NIDS * LD; ++i) out[i] = -777.0f;
    CHECK(mips_index_reconstruct(ix, ids, NIDS, off, out, MIPS_DTYPE_F32, LD, 0, NULL));
    for (int i = 0; i < NIDS; ++i) {
        const int64_t r = ids[i] - off;
        for (int c = 0; c < LD; ++c) {
            const uint32_t got = bits_of(out[i * LD + c]);
            if (c >= D) bad += got != bits_of(-777.0f);                 /* between the rows: untouched */
            else if (i == 17 || i == 18) bad += got != 0x7FC00000u;     /* no row: quiet NaN */
            else bad += got != bits_of(x[r * D + c]);
        }
    }
    uint16_t* raw = malloc(sizeof(uint16_t) * NIDS * D);
    CHECK(mips_index_reconstruct(ix, ids, NIDS, off, raw, MIPS_DTYPE_BF16, D, MIPS_ROWS_ZERO_MISSING, NULL));
    for (int i = 0; i < NIDS; ++i)
        for (int c = 0; c < D; ++c) {
            const int64_t r = ids[i] - off;
            const uint16_t want = (i == 17 || i == 18) ? 0 : (uint16_t)(bits_of(x[r * D + c]) >> 16); /* small integers: bf16 is the upper half */
            bad += raw[i * D + c] != want;
        }
    int32_t got_lab[NIDS];
    CHECK(mips_index_gather_labels(ix, ids, NIDS, off, got_lab, 0, NULL));
    for (int i = 0; i < NIDS; ++i) {
        const int64_t r = ids[i] - off;
        const int32_t want = (i == 17 || i == 18 || r >= NLAB) ? MIPS_LABEL_NONE : lab[r];
        bad += got_lab[i] != want;
    }

    /* refusals: nothing may be written */
    for (int i = 0; i < NIDS * LD; ++i) out[i] = -777.0f;
    ids[5] = off + N; /* one row past the index */
    int rc = mips_index_reconstruct(ix, ids, NIDS, off, out, MIPS_DTYPE_F32, LD, 0, NULL);
    if (rc != MIPS_E_INVALID || strlen(mips_last_error()) == 0) { fprintf(stderr, "an id past the index was not rejected\n"); return 1; }
    for (int i = 0; i < NIDS * LD; ++i) bad += bits_of(out[i]) != bits_of(-777.0f);
    if (mips_index_gather_labels(ix, ids, NIDS, off, got_lab, 0, NULL) != MIPS_E_INVALID) ++bad;
    ids[5] = (1ll << 32) + 3 + off; /* not row 3 */
    if (mips_index_reconstruct(ix, ids, NIDS, off, out, MIPS_DTYPE_F32, LD, 0, NULL) != MIPS_E_INVALID) ++bad;
    ids[5] = off + 3;
    if (mips_index_reconstruct(ix, ids, NIDS, off, out, MIPS_DTYPE_F32, D - 1, 0, NULL) != MIPS_E_INVALID) ++bad;          /* pitch below d */
    if (mips_index_reconstruct(ix, ids, NIDS, off, out, MIPS_DTYPE_FP8_E4M3, LD, 0, NULL) != MIPS_E_INVALID) ++bad;        /* not this storage */
    if (mips_index_reconstruct(ix, NULL, NIDS, off, out, MIPS_DTYPE_F32, LD, 0, NULL) != MIPS_E_INVALID) ++bad;
    CHECK(mips_index_reconstruct(ix, ids, 0, off, NULL, MIPS_DTYPE_F32, LD, 0, NULL));                                   /* n = 0: nothing to do */

    /* scoring the ids of a search gives its distances (an L2 index: distances, and inner products with MIPS_FORCE_IP) */
    float S[NQ * K], T[NQ * K];
    int64_t I[NQ * K];
    for (int flags = 0; flags <= MIPS_FORCE_IP; flags += MIPS_FORCE_IP) {
        CHECK(mips_search(ix, x + 40 * D, MIPS_DTYPE_F32, NQ, K, S, I, off, flags, NULL));
        CHECK(mips_score_subset(ix, x + 40 * D, MIPS_DTYPE_F32, NQ, I, K, T, off, flags, NULL));
        bad += memcmp(S, T, sizeof S) != 0;
        for (int t = 0; t < NQ * K; ++t) bad += I[t] < off || I[t] >= off + N;
    }
    I[3] = -1;
    CHECK(mips_score_subset(ix, x + 40 * D, MIPS_DTYPE_F32, NQ, I, K, T, off, 0, NULL));
    bad += !(T[3] > 3.0e38f); /* +inf for no row on an L2 index */
    I[3] = off + N;
    if (mips_score_subset(ix, x + 40 * D, MIPS_DTYPE_F32, NQ, I, K, T, off, 0, NULL) != MIPS_E_INVALID) ++bad;
    CHECK(mips_score_subset(ix, x, MIPS_DTYPE_F32, NQ, I, 0, T, off, 0, NULL));                                          /* k = 0 */
    CHECK(mips_index_destroy(ix));
    printf("c_abi_rows_smoke: %d ids, %d queries\n", (int)NIDS, (int)NQ);
    printf("c_abi_rows_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
