/* Plain-C consumer of include/mips_hip_sq8.h: no Python, no torch, host buffers.  Built and run by
 * tests/test_gpu_sq8.py::test_c_abi_sq8_from_plain_c:
 *     gcc -ffp-contract=off tests/c_abi_sq8_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -lm
 * Everything the device computes is restated here in float32 / double C as the header words it -- training, encoding, decoding,
 * q', B_q, S, D, ties to the lowest row -- and compared bit for bit. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_rows.h"
#include "mips_hip_sq8.h"

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

static float bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}

int main(void) {
    enum { N = 700, D = 100, NQ = 3, K = 5 };
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    static float x[N * D], q[NQ * D], vmin[D], vdiff[D], gmin[D], gdiff[D], dec[N * D];
    static uint8_t code[N * D], got_code[N * D];
    unsigned s = 97531u;
    for (int c = 0; c < D; ++c)
        for (int r = 0; r < N; ++r) x[r * D + c] = c == 3 ? 0.75f : (unit(&s) - 0.5f) * (0.1f + 0.05f * (float)c) + 0.01f * (float)(c - 50);
    for (int i = 0; i < NQ * D; ++i) q[i] = unit(&s) - 0.5f;
    for (int c = 0; c < D; ++c)
        if (c != 3) x[5 * D + c] *= 3.0f;             /* the longest row by far: the best match of its own direction ... */
    memcpy(x + 11 * D, x + 5 * D, sizeof(float) * D); /* ... and row 11 = row 5: a tie */

    mips_index_t* ix = NULL;
    REFUSED(mips_index_create(&ix, 0, D, MIPS_DTYPE_SQ8, MIPS_METRIC_L2), MIPS_E_UNSUPPORTED, "L2 create");
    CHECK(mips_index_create(&ix, 0, D, MIPS_DTYPE_SQ8, MIPS_METRIC_IP));
    if (mips_index_sq8_is_trained(ix) != 0 || mips_index_sq8_is_trained(NULL) != -1) { fprintf(stderr, "is_trained before training\n"); return 1; }
    REFUSED(mips_index_add(ix, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "add before train");
    REFUSED(mips_index_sq8_get_params(ix, gmin, gdiff), MIPS_E_INVALID, "get_params before train");
    REFUSED(mips_index_sq8_train(ix, x, 0, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on no rows");
    x[17 * D + 9] = INFINITY;
    REFUSED(mips_index_sq8_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on an infinity");
    x[17 * D + 9] = 0.125f;
    if (mips_index_sq8_is_trained(ix) != 0) { fprintf(stderr, "a refused training trained the index\n"); return 1; }
    CHECK(mips_index_sq8_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_index_sq8_get_params(ix, gmin, gdiff));

    int bad = 0;
    for (int c = 0; c < D; ++c) {
        float lo = x[c], hi = x[c];
        for (int r = 1; r < N; ++r) {
            lo = fminf(lo, x[r * D + c]);
            hi = fmaxf(hi, x[r * D + c]);
        }
        vmin[c] = lo;
        vdiff[c] = hi - lo;
        bad += gmin[c] != vmin[c] || gdiff[c] != vdiff[c];
    }
    bad += vdiff[3] != 0.0f;
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < D; ++c) {
            float t = vdiff[c] != 0.0f ? (x[r * D + c] - vmin[c]) / vdiff[c] : 0.0f;
            t = fminf(fmaxf(t, 0.0f), 1.0f);
            code[r * D + c] = (uint8_t)(int)(255.0f * t);
            dec[r * D + c] = vmin[c] + (((float)code[r * D + c] + 0.5f) / 255.0f) * vdiff[c];
        }
    CHECK(mips_index_add(ix, x, N, MIPS_DTYPE_F32, 0, NULL));
    REFUSED(mips_index_sq8_train(ix, x, N, MIPS_DTYPE_F32, 0, NULL), MIPS_E_INVALID, "train on a filled index");
    CHECK(mips_index_read_rows(ix, 0, N, got_code, NULL));
    bad += memcmp(got_code, code, sizeof code) != 0;

    /* reconstruct: decoded values and raw codes of rows 699, 0, "no row", 11 */
    const int64_t ids[4] = {N - 1, 0, -1, 11};
    static float rec[4 * D];
    static uint8_t rec_raw[4 * D];
    CHECK(mips_index_reconstruct(ix, ids, 4, 0, rec, MIPS_DTYPE_F32, D, 0, NULL));
    CHECK(mips_index_reconstruct(ix, ids, 4, 0, rec_raw, MIPS_DTYPE_SQ8, D, 0, NULL));
    REFUSED(mips_index_reconstruct(ix, ids, 4, 0, rec_raw, MIPS_DTYPE_FP8_E4M3, D, 0, NULL), MIPS_E_INVALID, "e4m3 as the raw type");
    for (int i = 0; i < 4; ++i)
        for (int c = 0; c < D; ++c) {
            if (ids[i] < 0) bad += rec[i * D + c] == rec[i * D + c] || rec_raw[i * D + c] != 0; /* NaN row, zero codes */
            else bad += memcmp(&rec[i * D + c], &dec[ids[i] * D + c], 4) != 0 || rec_raw[i * D + c] != code[ids[i] * D + c];
        }

    /* search against the restatement: S in the code domain, ties to the lowest row, D = S + B_q */
    float S[NQ * K], S2[NQ * K];
    int64_t I[NQ * K];
    memcpy(q, dec + 5 * D, sizeof(float) * D); /* query 0 points at rows 5 and 11 */
    CHECK(mips_search(ix, q, MIPS_DTYPE_F32, NQ, K, S, I, 0, 0, NULL));
    for (int j = 0; j < NQ; ++j) {
        float qp[D];
        double bq = 0.0;
        for (int c = 0; c < D; ++c) {
            const float sc = vdiff[c] / 255.0f;
            const float oc = vmin[c] + 0.5f * sc;
            qp[c] = bf16_rne(q[j * D + c] * sc);
            bq += (double)q[j * D + c] * (double)oc;
        }
        static float score[N];
        static char taken[N];
        memset(taken, 0, sizeof taken);
        for (int r = 0; r < N; ++r) {
            double acc = 0.0;
            for (int c = 0; c < D; ++c) acc += (double)qp[c] * (double)code[r * D + c];
            score[r] = (float)acc;
        }
        for (int t = 0; t < K; ++t) {
            int best = -1;
            for (int r = 0; r < N; ++r)
                if (!taken[r] && (best < 0 || score[r] > score[best])) best = r;
            taken[best] = 1;
            const float dv = (float)((double)score[best] + bq);
            bad += I[j * K + t] != best || memcmp(&S[j * K + t], &dv, 4) != 0;
        }
    }
    bad += !(I[0] == 5 && I[1] == 11 && S[0] == S[1]);
    CHECK(mips_score_subset(ix, q, MIPS_DTYPE_F32, NQ, I, K, S2, 0, 0, NULL));
    bad += memcmp(S, S2, sizeof S) != 0;

    /* what is not served */
    REFUSED(mips_search_wide(ix, q, MIPS_DTYPE_F32, NQ, 40, S, I, 0, 0, NULL), MIPS_E_UNSUPPORTED, "wide search");
    int64_t lims[NQ + 1];
    const float radii[NQ] = {0.f, 0.f, 0.f};
    REFUSED(mips_range_search(ix, q, MIPS_DTYPE_F32, NQ, radii, lims, S, I, NQ * K, 0, 0, NULL), MIPS_E_UNSUPPORTED, "range search");
    REFUSED(mips_search(ix, code, MIPS_DTYPE_SQ8, NQ, K, S, I, 0, 0, NULL), MIPS_E_INVALID, "codes as queries");
    REFUSED(mips_index_add(ix, code, 1, MIPS_DTYPE_FP8_E4M3, 0, NULL), MIPS_E_INVALID, "e4m3 bytes as rows");

    /* raw codes as rows; set_params on a fresh index makes it trained */
    mips_index_t* iy = NULL;
    CHECK(mips_index_create(&iy, 0, D, MIPS_DTYPE_SQ8, MIPS_METRIC_IP));
    gdiff[7] = -1.0f;
    REFUSED(mips_index_sq8_set_params(iy, gmin, gdiff), MIPS_E_INVALID, "negative vdiff");
    gdiff[7] = vdiff[7];
    CHECK(mips_index_sq8_set_params(iy, gmin, gdiff));
    if (mips_index_sq8_is_trained(iy) != 1) { fprintf(stderr, "set_params did not train\n"); return 1; }
    CHECK(mips_index_add(iy, code, N, MIPS_DTYPE_SQ8, 0, NULL));
    int64_t I2[NQ * K];
    CHECK(mips_search(iy, q, MIPS_DTYPE_F32, NQ, K, S2, I2, 0, 0, NULL));
    bad += memcmp(S, S2, sizeof S) != 0 || memcmp(I, I2, sizeof I) != 0;
    CHECK(mips_index_destroy(iy));
    CHECK(mips_index_destroy(ix));
    printf("c_abi_sq8_smoke: %d rows x %d, %d queries, top-%d\n", N, D, NQ, K);
    printf("c_abi_sq8_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
