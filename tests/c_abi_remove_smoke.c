/* Plain-C consumer of mips_index_remove (include/mips_hip_update.h): no Python, no torch, host buffers and a HOST bitmap whose
 * bit 13 speaks about row 0.  Built and run by tests/test_gpu_remove.py::test_c_abi_remove_from_plain_c:
 *     gcc tests/c_abi_remove_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Rows are small integers (exact in bf16) that name their row, so what the index holds afterwards is checked right here:
 * rows and labels are read back and compared with a compaction done in C, and a search must find a surviving row under its
 * NEW number. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_update.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mips_last_error());   \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static unsigned lcg(unsigned* s) { return *s = *s * 1664525u + 1013904223u; }

int main(void) {
    const int64_t n = 3001, d = 100, bit0 = 13, nbits = n + bit0 + 5, nlab = 2000;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    float* x = malloc(sizeof(float) * n * d);
    int32_t* lab = malloc(sizeof(int32_t) * n);
    for (int64_t r = 0; r < n; ++r) {
        for (int64_t c = 0; c < d; ++c) x[r * d + c] = (float)((r * 7 + c * 3) % 255 - 127);
        lab[r] = (int32_t)(r % 11);
    }
    /* the removal: about one row in three, all of rows 1024 .. 1535, the first and the last row */
    unsigned s = 2468u;
    uint8_t* bits = malloc((nbits + 7) / 8);
    memset(bits, 0xff, (nbits + 7) / 8); /* bits that speak about other rows are all set */
    char* gone = calloc(n, 1);
    for (int64_t r = 0; r < n; ++r) {
        gone[r] = (lcg(&s) >> 16) % 3 == 0 || (r >= 1024 && r < 1536) || r == 0 || r == n - 1;
        if (!gone[r]) bits[(r + bit0) >> 3] &= (uint8_t)~(1u << ((r + bit0) & 7));
    }
    int64_t left = 0, lab_left = 0;
    for (int64_t r = 0; r < n; ++r) {
        left += !gone[r];
        lab_left += !gone[r] && r < nlab;
    }

    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP));
    CHECK(mips_index_add(ix, x, n, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_index_set_labels(ix, lab, 0, nlab, 0, NULL)); /* a partial labelled prefix */
    CHECK(mips_index_set_param(ix, "remove_window_rows", 384));
    int64_t counts[2] = {-1, -1};
    /* refusals first: they must leave the index alone */
    int rc = mips_index_remove(ix, bits, n + bit0 - 1, bit0, 0, counts, NULL);
    if (rc != MIPS_E_INVALID || strlen(mips_last_error()) == 0) { fprintf(stderr, "too short a bitmap not rejected\n"); return 1; }
    rc = mips_index_remove(ix, bits, nbits, -1, 0, counts, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "negative sel_bit0 not rejected\n"); return 1; }
    rc = mips_index_remove(ix, NULL, nbits, bit0, 0, counts, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "NULL bitmap not rejected\n"); return 1; }
    if (mips_index_set_param(ix, "remove_window_rows", 100) != MIPS_E_INVALID) { fprintf(stderr, "window 100 not rejected\n"); return 1; }
    if (mips_index_ntotal(ix) != n) { fprintf(stderr, "a refused call changed ntotal\n"); return 1; }

    CHECK(mips_index_remove(ix, bits, nbits, bit0, 0, counts, NULL));
    int bad = 0;
    bad += counts[0] != n - left || counts[1] != lab_left || mips_index_ntotal(ix) != left;
    uint16_t* got = malloc(sizeof(uint16_t) * left * d);
    int32_t* got_lab = malloc(sizeof(int32_t) * (lab_left + 1));
    CHECK(mips_index_read_rows(ix, 0, left, got, NULL));
    CHECK(mips_index_read_labels(ix, 0, lab_left, got_lab, NULL));
    if (mips_index_read_labels(ix, 0, lab_left + 1, got_lab, NULL) != MIPS_E_INVALID) ++bad; /* the labelled prefix ends there */
    int64_t o = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (gone[r]) continue;
        for (int64_t c = 0; c < d; ++c) {
            float v = x[r * d + c];
            uint32_t u;
            memcpy(&u, &v, 4);
            if (got[o * d + c] != (uint16_t)(u >> 16)) ++bad; /* small integers: bf16 is the upper half, exactly */
        }
        if (r < nlab && got_lab[o] != lab[r]) ++bad;
        ++o;
    }
    /* the index stays searchable and no result names a row past the new ntotal (what the results ARE is the Python tests' matter) */
    float S[5];
    int64_t I[5];
    CHECK(mips_search(ix, x + 5 * d, MIPS_DTYPE_F32, 1, 5, S, I, 0, 0, NULL));
    for (int t = 0; t < 5; ++t) bad += I[t] < 0 || I[t] >= left;
    /* an add appends at the new end */
    CHECK(mips_index_add(ix, x, 2, MIPS_DTYPE_F32, 0, NULL));
    bad += mips_index_ntotal(ix) != left + 2;
    CHECK(mips_index_read_rows(ix, left, 2, got, NULL));
    for (int64_t c = 0; c < 2 * d; ++c) {
        uint32_t u;
        memcpy(&u, &x[c], 4);
        if (got[c] != (uint16_t)(u >> 16)) ++bad;
    }
    /* nothing selected: nothing happens */
    memset(bits, 0, (nbits + 7) / 8);
    CHECK(mips_index_remove(ix, bits, nbits, bit0, 0, counts, NULL));
    bad += counts[0] != 0 || counts[1] != lab_left || mips_index_ntotal(ix) != left + 2;
    CHECK(mips_index_destroy(ix));
    printf("c_abi_remove_smoke: %lld of %lld rows left, %lld labelled\n", (long long)left, (long long)n, (long long)lab_left);
    printf("c_abi_remove_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
