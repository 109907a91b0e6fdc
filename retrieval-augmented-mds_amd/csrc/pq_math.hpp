// Arithmetic of the product-quantised index (include/mips_hip_pq.h), one text for the kernels, the host and a
// stand-alone check (tests/pq_math_check.cpp includes this file and nothing else of the library).  Every step is one IEEE operation.
// The only products are (double)a * (double)b of two float32 values, which are EXACT in fp64 (48 significant bits), so contracting
// such a product into the sum that follows changes nothing; the fp32 sum of the score has no product in it at all.
//   score     s(a, b) = (float) sum_t (double)a_t (double)b_t, sequential in ascending t          (the project's canonical score)
//   distance  u_t = x_t - c_t (ONE float32 subtraction);  e(x, c) = sum_t (double)u_t (double)u_t, sequential in ascending t
//   nearest   scan j = 0 .. 255 with best = 0; j replaces best iff e_j < e_best (strict): ties to the lowest j, a NaN never wins
//   mean      (float)(S / count), S the sequential fp64 sum of the members in ascending row order
//   D(q, i)   acc = LUT[0][code_0]; acc = acc + LUT[m][code_m] for m = 1 .. M - 1: float32 additions in ascending m
// and the integer arithmetic of a search: the row segments of the scan, their number, the waves of a workgroup, the LDS it asks for.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PQ_HD __host__ __device__ __forceinline__
#else
#define PQ_HD inline
#endif

namespace pq {

constexpr int kSub = 256;             // centroids of a sub-quantiser (8 bits per code)
constexpr int kMaxM = 128;            // sub-quantisers at most: the query's table is M KiB of LDS
constexpr int64_t kTrainRows = 65536; // rows the trainer looks at
constexpr int kCodeAlign = 16;        // the row pitch of the codes is M rounded up to this many bytes
constexpr int kListSlots = 32;        // slots of a wave's sorted list in LDS (k <= MIPS_MAX_K = 29)
constexpr int64_t kMergeLimit = 65536; // entries per query mips_merge_topk_sorted_packed takes (S * k)

PQ_HD double sum_step(double acc, float a, float b) { return acc + (double)a * (double)b; }

PQ_HD float score(const float* a, const float* b, int64_t d) {
    double acc = 0.0;
    for (int64_t t = 0; t < d; ++t) acc = sum_step(acc, a[t], b[t]);
    return (float)acc;
}

PQ_HD double dist_step(double acc, float x, float c) {
    const float u = x - c;
    return acc + (double)u * (double)u;
}

PQ_HD double dist(const float* x, const float* c, int dsub) {
    double acc = 0.0;
    for (int t = 0; t < dsub; ++t) acc = dist_step(acc, x[t], c[t]);
    return acc;
}

// does centroid j with distance e replace the best so far?  (strict: ties stay with the lower j; a NaN never wins)
PQ_HD bool closer(double e, double e_best) { return e < e_best; }

// the code of sub-vector x among the 256 centroids cb [256][dsub]
PQ_HD int nearest(const float* x, const float* cb, int dsub) {
    int best = 0;
    double e_best = dist(x, cb, dsub);
    for (int j = 1; j < kSub; ++j) {
        const double e = dist(x, cb + (int64_t)j * dsub, dsub);
        if (closer(e, e_best)) {
            best = j;
            e_best = e;
        }
    }
    return best;
}

PQ_HD float mean(double sum, int64_t count) { return (float)(sum / (double)count); }

// row i of the m rows the trainer looks at, and the first row of centroid j:  floor(i n / m)
PQ_HD int64_t pick(int64_t i, int64_t n, int64_t m) { return i * n / m; }

PQ_HD float adc_step(float acc, float v) { return acc + v; }

// D(q, i): lut [M][256] of the query, code [M] of the row
PQ_HD float adc(const float* lut, const uint8_t* code, int M) {
    float acc = lut[code[0]];
    for (int m = 1; m < M; ++m) acc = adc_step(acc, lut[(int64_t)m * kSub + code[m]]);
    return acc;
}

PQ_HD int code_pitch(int M) { return (M + kCodeAlign - 1) / kCodeAlign * kCodeAlign; }

// ---- the scan's launch arithmetic: everything from (ns, k, M, ntotal, compute units) alone
// waves of a workgroup: a table of more than 32 KiB leaves room for few workgroups on a compute unit, so one large workgroup
// shares it (16 waves: four per SIMD, what ds_read_b32 needs to reach its rate); small tables get 4-wave workgroups
PQ_HD int scan_waves(int M) { return M > 32 ? 16 : 4; }

// bytes of LDS a workgroup asks for: the table, then the waves' lists (keys, rows) and their counts
PQ_HD int64_t scan_lds_bytes(int M) {
    const int w = scan_waves(M);
    return (int64_t)M * kSub * 4 + (int64_t)w * kListSlots * 8 + (int64_t)w * 4;
}

// workgroups one compute unit holds (160 KiB of LDS, 32 waves)
PQ_HD int scan_blocks_per_cu(int M) {
    const int64_t by_lds = ((int64_t)160 << 10) / scan_lds_bytes(M);
    const int64_t by_waves = 32 / scan_waves(M);
    const int64_t b = by_lds < by_waves ? by_lds : by_waves;
    return (int)(b < 1 ? 1 : b);
}

// first row of segment s of S (s = S: ntotal).  0 <= n < 2^31, 0 <= s <= S <= 65536: no overflow in int64
PQ_HD int64_t seg_bound(int64_t n, int64_t s, int64_t S) { return n * s / S; }

// S: enough workgroups for two rounds on every compute unit, no segment shorter than one pass of the workgroup (unless there is
// one segment), S * k within what the merge takes
PQ_HD int choose_segments(int64_t ns, int64_t k, int M, int64_t ntotal, int64_t cus) {
    const int64_t want = 2 * cus * scan_blocks_per_cu(M);
    int64_t S = (want + ns - 1) / ns;
    const int64_t pass = 64 * scan_waves(M);
    const int64_t most = (ntotal + pass - 1) / pass;
    if (S > most) S = most;
    if (S * k > kMergeLimit) S = kMergeLimit / k;
    return (int)(S < 1 ? 1 : S);
}

} // namespace pq
