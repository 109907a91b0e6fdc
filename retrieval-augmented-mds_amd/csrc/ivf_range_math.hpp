// Integer arithmetic of the range search over the probed lists (include/mips_hip_ivf_range.h: mips_ivf_range_search), one text for
// the kernels and a stand-alone check (tests/ivf_range_math_check.cpp includes this file and nothing else of the library).  Every
// index that addresses the staging buffer, the caller's arrays or a sort partner is computed here.
//   staging    a wave whose lanes `mask` hold hits reserves popcount(mask) records behind `base` (one atomic add on the cursor); lane
//              order is kept inside the block.  A record whose slot is not below `cap` is dropped, the cursor counts on, so the
//              place pass walks min(cursor, cap) records.
//   place      the c-th placed record of a query whose stretch begins at lims[j] goes to lims[j] + c when that is below `cap`.
//   stretch    what of [lims[j], lims[j + 1]) lies below `cap`: the entries the ordering step sorts by row.
//   order      a sorting network of compare-exchanges that ALL put the smaller row at the lower index: merge blocks of k = 2, 4, ...
//              up to the size class (the smallest power of two >= n); the first step of a block pairs i with its mirror image
//              i ^ (k - 1), the steps after it pair i with i ^ j for j = k / 4, ..., 1.  Because no exchange moves a larger entry
//              down, n need not be a power of two: a pair whose partner is not below n is skipped -- it would meet the +inf padding
//              of the full network, which never moves.  Stretches of at most kRangeSortLds entries are sorted in LDS, longer ones
//              by the same network in global memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFR_HD __host__ __device__ __forceinline__
#else
#define IVFR_HD inline
#endif

namespace ivf {

constexpr int kRangeSortLds = 4096;         // entries of a stretch the ordering step sorts in LDS at most
constexpr int64_t kRangeSlice = 4096;       // queries of one pass at most (range_lims_kernel takes one slice)

// slot of lane `lane`'s record when the lanes of `mask` append behind `base`
IVFR_HD uint64_t range_slot(uint64_t base, uint64_t mask, int lane) { return base + (uint64_t)__builtin_popcountll(mask & (((uint64_t)1 << lane) - 1)); }

// is slot `slot` inside a staging buffer (or an output array) of `cap` entries?  cap >= 0
IVFR_HD bool range_keeps(uint64_t slot, int64_t cap) { return slot < (uint64_t)cap; }

// records the place pass walks: what the cursor counted, clamped at the capacity
IVFR_HD uint64_t range_staged(uint64_t cursor, int64_t cap) { return cursor < (uint64_t)cap ? cursor : (uint64_t)cap; }

// index in the caller's arrays of the c-th placed record of a stretch that begins at lim0; -1: dropped (not below cap)
IVFR_HD int64_t range_place_slot(int64_t lim0, int64_t c, int64_t cap) {
    const int64_t dst = lim0 + c;
    return dst >= 0 && dst < cap ? dst : -1;
}

// entries of [lim0, lim1) below cap
IVFR_HD int64_t range_stretch(int64_t lim0, int64_t lim1, int64_t cap) {
    const int64_t end = lim1 < cap ? lim1 : cap;
    return end > lim0 ? end - lim0 : 0;
}

// size class of a stretch of n >= 1 entries: the smallest power of two >= n
IVFR_HD int64_t range_sort_class(int64_t n) {
    int64_t P = 1;
    while (P < n) P *= 2;
    return P;
}

IVFR_HD bool range_sort_in_lds(int64_t n) { return n <= kRangeSortLds; }

// the lower index of the t-th pair of a step of distance j (a power of two): t with a zero bit inserted at j's position
IVFR_HD int64_t bitonic_lower(int64_t t, int64_t j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// partner (> i) of lower index i in the step of distance j of merge block k; the smaller row goes to i
IVFR_HD int64_t bitonic_partner(int64_t i, int64_t k, int64_t j) { return j == (k >> 1) ? (i ^ (k - 1)) : (i ^ j); }

} // namespace ivf
