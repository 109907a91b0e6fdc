// Integer arithmetic of the IVF search (include/mips_hip_ivf.h: mips_ivf_search), one text for the host, the kernels and a
// stand-alone check (tests/ivf_search_math_check.cpp includes this file and nothing else of the library).
//   segments   a probed list of L rows is cut into S segments; segment s holds the list positions [floor(L s / S), floor(L (s + 1) / S)):
//              consecutive, disjoint, covering [0, L), none longer than ceil(L / S)
//   S          a power of two chosen from the SIZES of a call alone (queries, probed lists per query, k, compute units): the smallest
//              that puts two workgroups on every compute unit, at most 32, halved while p S k exceeds what the merge takes
//   slice      queries one pass serves: bounded so that the partial lists [p S][slice][k] stay within a fixed budget
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFS_HD __host__ __device__ __forceinline__
#else
#define IVFS_HD inline
#endif

namespace ivf {

constexpr int kMaxSegments = 32;
constexpr int64_t kMergeLimit = 65536;          // entries per query mips_merge_topk_sorted_packed takes (parts * k)
constexpr int64_t kSliceQueries = 4096;         // queries of one pass at most
constexpr int64_t kPartsBudget = (int64_t)256 << 20; // bytes of partial lists of one pass with S = 1

// first list position of segment s of S (s = S: the list's length).  0 <= L < 2^31, 0 <= s <= S <= 32: no overflow
IVFS_HD int64_t seg_bound(int64_t L, int64_t s, int64_t S) { return L * s / S; }

IVFS_HD int choose_segments(int64_t nq, int64_t p, int64_t k, int64_t cus) {
    int64_t S = 1;
    while (S < kMaxSegments && nq * p * S < 2 * cus) S *= 2;
    while (S > 1 && p * S * k > kMergeLimit) S /= 2;
    return (int)S;
}

IVFS_HD int64_t slice_queries(int64_t p, int64_t k) {
    int64_t ns = kPartsBudget / (p * k * 16);
    if (ns < 1) ns = 1;
    return ns < kSliceQueries ? ns : kSliceQueries;
}

} // namespace ivf
