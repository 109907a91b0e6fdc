// Arithmetic of the IVF index over PQ codes (include/mips_hip_ivfpq.h), one text for the kernels, the host and a
// stand-alone check (tests/ivfpq_math_check.cpp includes this file and, through it, pq_math.hpp -- nothing else of the library).
// Every step is one IEEE operation:
//   residual     r_t = x_t - c_t                                                                       (ONE float32 subtraction)
//   score        acc = T; acc = acc + LUT[m][code_m] for m = 0 .. M - 1 in ascending m               (float32 additions, in order)
//                by_residual = 0: pq::adc, no coarse term.  Started from -0.0f the same loop IS pq::adc: -0 + t is t bit for bit.
//   reconstruct  v_t = c_t + C[m][code_m][t]                                                           (ONE float32 addition)
// and the integer arithmetic of a search: the segments of the concatenation of a query's probed lists, their number, the list a
// position falls into, the LDS a workgroup asks for.
#pragma once
#include "pq_math.hpp"

namespace ivfpq {

constexpr int kMaxProbe = 1024;        // lists one query probes at most
constexpr int64_t kAddChunk = 65536;   // rows one assignment + encode pass of add() carries

PQ_HD float residual(float x, float c) { return x - c; }
PQ_HD float recon(float c, float v) { return c + v; }

// where the sum of a row's table entries starts: the coarse term, or -0.0f (then the first step IS "acc = LUT[0][code_0]")
PQ_HD float score_start(float T, bool by_residual) { return by_residual ? T : -0.0f; }

// the score of a row: lut [M][256] of the query, code [M] of the row, T the coarse term of the row's list
PQ_HD float score(float T, const float* lut, const uint8_t* code, int M, bool by_residual) {
    float acc = score_start(T, by_residual);
    for (int m = 0; m < M; ++m) acc = pq::adc_step(acc, lut[(int64_t)m * pq::kSub + code[m]]);
    return acc;
}

// ---- the scan's launch arithmetic: everything from (ns, k, M, p, nlist, ntotal, compute units) alone
// bytes of LDS a workgroup asks for: what the PQ scan asks for, then the prefix of the p list sizes [p + 1], the lists' first
// positions in list_rows [p] and their coarse terms [p]
PQ_HD int64_t scan_lds_bytes(int M, int p) { return pq::scan_lds_bytes(M) + ((int64_t)3 * p + 1) * 4; }

// rows a query is expected to score: the p / nlist share of the index, rounded up (never a value read from the device)
PQ_HD int64_t expected_rows(int64_t ntotal, int64_t p, int64_t nlist) { return (ntotal * p + nlist - 1) / nlist; }

// S, forced (0 < forced) or chosen as pq::choose_segments chooses it for an index of expected_rows rows; S * k within the merge
PQ_HD int choose_segments(int64_t ns, int64_t k, int M, int64_t ntotal, int64_t p, int64_t nlist, int64_t cus, int64_t forced) {
    if (forced <= 0) return pq::choose_segments(ns, k, M, expected_rows(ntotal, p, nlist), cus);
    int64_t S = forced;
    if (S * k > pq::kMergeLimit) S = pq::kMergeLimit / k;
    return (int)(S < 1 ? 1 : S);
}

// the probed list a position of the concatenation falls into: the u in [0, p) with pre[u] <= pos < pre[u + 1], pre [p + 1]
// non-decreasing with pre[0] = 0 and pos < pre[p]; empty lists are stepped over
PQ_HD int locate(const int* pre, int p, int64_t pos) {
    int lo = 0, hi = p; // pre[lo] <= pos < pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if ((int64_t)pre[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

} // namespace ivfpq
