/* Plain-C consumer of include/mips_hip_hook.h (mips_search_fused_grp): no Python, no torch.  Built and run by
 * tests/test_gpu_hook_groups.py::test_c_abi_hook_grp_from_plain_c:
 *     gcc tests/c_abi_hook_grp_smoke.c -Iinclude -L<lib dir> -lmips_hip -Wl,-rpath,<lib dir> -L/opt/rocm/lib -lamdhip64 -lm
 * The entry point takes DEVICE queries and outputs, so this program needs four calls of the HIP runtime -- allocate, copy in,
 * copy out, synchronise -- which it declares itself (their C signatures are stable) instead of including the HIP headers.
 * Index: n x d lattice values from a tiny LCG (exact in bf16, sums exact in fp32 / fp64), so the expected results are computed
 * right here with integer arithmetic and compared bit for bit: both modes, HOST and DEVICE labels, with and without the ignore
 * filter, the one-launch form (8 queries) and the general form (17 queries), and the refusals by return code. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mips_hip_hook.h"

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

#define NQ_MAX 17
#define K_MAX 6

static unsigned lcg(unsigned* s) { return *s = *s * 1664525u + 1013904223u; }

static int admits(int32_t lab, int32_t ql, int mode) { return ql == MIPS_LABEL_NONE || ((lab == ql) == (mode == MIPS_GRP_ONLY)); }

int main(void) {
    const int64_t n = 3001, d = 128;
    if (mips_abi_version() != MIPS_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    int* xi = malloc(sizeof(int) * n * d);
    int* qi = malloc(sizeof(int) * NQ_MAX * d);
    float* x = malloc(sizeof(float) * n * d);
    float* q = malloc(sizeof(float) * NQ_MAX * d);
    unsigned s = 13579u;
    for (int64_t i = 0; i < n * d; ++i) { xi[i] = (int)((lcg(&s) >> 16) % 255) - 127; x[i] = xi[i] / 64.0f; }
    for (int64_t i = 0; i < NQ_MAX * d; ++i) { qi[i] = (int)((lcg(&s) >> 16) % 255) - 127; q[i] = qi[i] / 64.0f; }
    /* row labels 0 .. 6, but group 3 is small (4 rows: fewer than k); query labels: present ones, an absent one, NONE */
    int32_t* lab = malloc(sizeof(int32_t) * n);
    int small = 0;
    for (int64_t r = 0; r < n; ++r) {
        lab[r] = (int32_t)((lcg(&s) >> 16) % 7);
        if (lab[r] == 3 && ++small > 4) lab[r] = 4;
    }
    int32_t ql[NQ_MAX];
    const int32_t cyc[9] = {0, 1, 2, 3, 4, 5, 6, 100, MIPS_LABEL_NONE};
    for (int a = 0; a < NQ_MAX; ++a) ql[a] = cyc[a % 9];
    long* val = malloc(sizeof(long) * NQ_MAX * n); /* dot products in units of 1/4096 */
    for (int64_t a = 0; a < NQ_MAX; ++a)
        for (int64_t r = 0; r < n; ++r) {
            long v = 0;
            for (int64_t c = 0; c < d; ++c) v += (long)qi[a * d + c] * xi[r * d + c];
            val[a * n + r] = v;
        }

    float *q_dev = NULL, *s_dev = NULL;
    int64_t *i_dev = NULL, *ign_dev = NULL;
    int32_t* ql_dev = NULL;
    if (hipMalloc((void**)&q_dev, sizeof(float) * NQ_MAX * d) || hipMalloc((void**)&s_dev, sizeof(float) * NQ_MAX * K_MAX) ||
        hipMalloc((void**)&i_dev, sizeof(int64_t) * NQ_MAX * K_MAX) || hipMalloc((void**)&ign_dev, sizeof(int64_t) * NQ_MAX) ||
        hipMalloc((void**)&ql_dev, sizeof(int32_t) * NQ_MAX)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    if (hipMemcpy(q_dev, q, sizeof(float) * NQ_MAX * d, 1) || hipMemcpy(ql_dev, ql, sizeof(ql), 1)) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }

    mips_index_t* ix = NULL;
    CHECK(mips_index_create(&ix, 0, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP));
    CHECK(mips_index_add(ix, x, n, MIPS_DTYPE_F32, 0, NULL));
    int rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, ql, MIPS_GRP_EXCLUDE, 0, NULL);
    if (rc != MIPS_E_INVALID || strstr(mips_last_error(), "mips_index_set_labels") == NULL) { fprintf(stderr, "a never-labelled index was searched by group\n"); return 1; }
    CHECK(mips_index_set_labels(ix, lab, 0, n, 0, NULL));

    float S[NQ_MAX * K_MAX];
    int64_t I[NQ_MAX * K_MAX], banned[NQ_MAX], E[K_MAX + 1];
    char* used = malloc(n);
    int bad = 0, calls = 0;
    int64_t f = -1, rs = -1, u = -1;
    for (int form = 0; form < 2; ++form) {          /* 0: one launch (8 queries), 1: general form (17 queries) */
        const int64_t nq = form ? 17 : 8;
        for (int mode = 0; mode < 2; ++mode)
            for (int with_ignore = 0; with_ignore < 2; ++with_ignore)
                for (int dev_labels = 0; dev_labels < 2; ++dev_labels) {
                    const int k = with_ignore ? 5 : (mode ? 6 : 1);
                    const int kf = k + with_ignore;
                    const int64_t off = 500;
                    /* expected k + with_ignore best admitted rows; the second one (if any) is banned */
                    for (int64_t a = 0; a < nq; ++a) banned[a] = -77;
                    if (with_ignore) {
                        for (int64_t a = 0; a < nq; ++a) {
                            int64_t b1 = -1, b2 = -1;
                            for (int64_t r = 0; r < n; ++r)
                                if (admits(lab[r], ql[a], mode)) {
                                    if (b1 < 0 || val[a * n + r] > val[a * n + b1]) { b2 = b1; b1 = r; }
                                    else if (b2 < 0 || val[a * n + r] > val[a * n + b2]) b2 = r;
                                }
                            if (b2 >= 0) banned[a] = b2 + off;
                        }
                        if (hipMemcpy(ign_dev, banned, sizeof(int64_t) * nq, 1)) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
                    }
                    CHECK(mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, nq, k, 0, with_ignore ? ign_dev : NULL, s_dev, i_dev, off,
                                                dev_labels ? ql_dev : ql, mode, dev_labels ? MIPS_GRP_DEVICE : 0, NULL));
                    ++calls;
                    const char* want = form ? "mips::grouped_scan_kernel" : "mips::hook_grouped_kernel<false, false>";
                    if (strcmp(mips_index_last_kernel(ix), want) != 0) { fprintf(stderr, "last kernel %s, expected %s\n", mips_index_last_kernel(ix), want); return 1; }
                    if (hipDeviceSynchronize() || hipMemcpy(S, s_dev, sizeof(float) * nq * k, 2) || hipMemcpy(I, i_dev, sizeof(int64_t) * nq * k, 2)) { fprintf(stderr, "copy out failed\n"); return 1; }
                    if (!(form && with_ignore)) { /* (behind the general form's ignore filter the report is the nested search's) */
                        CHECK(mips_index_margin_stats(ix, &f, &rs, &u, 1, NULL));
                        if (u != 0) { fprintf(stderr, "queries left unresolved\n"); return 1; }
                    }
                    for (int64_t a = 0; a < nq; ++a) {
                        memset(used, 0, n);
                        int w = 0;
                        for (int t = 0; t < kf; ++t) {
                            int64_t best = -1;
                            for (int64_t r = 0; r < n; ++r)
                                if (admits(lab[r], ql[a], mode) && !used[r] && (best < 0 || val[a * n + r] > val[a * n + best])) best = r;
                            if (best >= 0) used[best] = 1;
                            if (best >= 0 && best + off == banned[a]) continue;
                            if (w < k) E[w++] = best;
                        }
                        for (int t = 0; t < k; ++t) {
                            const int64_t e = t < w ? E[t] : -1;
                            if (e < 0) bad += I[a * k + t] != -1 || !(S[a * k + t] == -INFINITY);
                            else bad += I[a * k + t] != e + off || S[a * k + t] != (float)((double)val[a * n + e] / 4096.0);
                        }
                    }
                }
    }
    /* ---- NULL q_labels IS mips_search_fused: same results, its kernel name; grp_mode and flags are not looked at */
    float S0[8 * 5];
    int64_t I0[8 * 5];
    CHECK(mips_search_fused(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, NULL));
    if (hipDeviceSynchronize() || hipMemcpy(S0, s_dev, sizeof(S0), 2) || hipMemcpy(I0, i_dev, sizeof(I0), 2)) return 1;
    CHECK(mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, NULL, 7, 12345, NULL));
    if (strncmp(mips_index_last_kernel(ix), "mips::tiny_search_kernel", 24) != 0) { fprintf(stderr, "ungrouped kernel name\n"); return 1; }
    if (hipDeviceSynchronize() || hipMemcpy(S, s_dev, sizeof(S0), 2) || hipMemcpy(I, i_dev, sizeof(I0), 2)) return 1;
    bad += memcmp(S, S0, sizeof(S0)) != 0 || memcmp(I, I0, sizeof(I0)) != 0;
    /* ---- refusals */
    rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, ql, 2, 0, NULL);
    if (rc != MIPS_E_INVALID || strstr(mips_last_error(), "grp_mode") == NULL) { fprintf(stderr, "grp_mode 2 not rejected\n"); return 1; }
    rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, ql, -1, 0, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "grp_mode -1 not rejected\n"); return 1; }
    rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, MIPS_MAX_K, 0, ign_dev, s_dev, i_dev, 0, ql, 0, 0, NULL);
    if (rc != MIPS_E_UNSUPPORTED) { fprintf(stderr, "k + 1 > MIPS_MAX_K not rejected\n"); return 1; }
    rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_BF16, 8, 5, 1, NULL, s_dev, i_dev, 0, ql, 0, 0, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "normalize with bf16 queries not rejected\n"); return 1; }
    CHECK(mips_index_add(ix, x, 10, MIPS_DTYPE_F32, 0, NULL));
    rc = mips_search_fused_grp(ix, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, ql, 0, 0, NULL);
    if (rc != MIPS_E_INVALID) { fprintf(stderr, "rows added after labelling were searched by group\n"); return 1; }
    mips_index_t* f8 = NULL;
    CHECK(mips_index_create(&f8, 0, d, MIPS_DTYPE_FP8_E4M3, MIPS_METRIC_IP));
    CHECK(mips_index_add(f8, x, 300, MIPS_DTYPE_F32, 0, NULL));
    CHECK(mips_index_set_labels(f8, lab, 0, 300, 0, NULL));
    rc = mips_search_fused_grp(f8, q_dev, MIPS_DTYPE_F32, 8, 5, 0, NULL, s_dev, i_dev, 0, ql, 0, 0, NULL);
    if (rc != MIPS_E_UNSUPPORTED) { fprintf(stderr, "e4m3 storage not refused (%d)\n", rc); return 1; }
    CHECK(mips_index_destroy(f8));
    CHECK(mips_index_destroy(ix));
    hipFree(q_dev); hipFree(s_dev); hipFree(i_dev); hipFree(ign_dev); hipFree(ql_dev);
    printf("c_abi_hook_grp_smoke: %d grouped calls on %lld docs\n", calls, (long long)n);
    printf("c_abi_hook_grp_smoke: mismatches: %d\n", bad);
    return bad != 0;
}
