// The rules of mips_index_update (include/mips_hip_write.h) that host and kernels share, without a HIP type: which local row an id
// names, which of several positions that name one row writes it, and the host restatement of both (the count of a host-id call,
// and what tests/update_math_check.cpp runs under the sanitizers).
//
// update(ids[n], x[n, d], idx_offset) is the sequential loop "for p = 0 .. n - 1: if ids[p] names a row, that row becomes x[p]".
// What the loop leaves behind: every named row holds the x[p] of the HIGHEST position p that names it.  The kernels
// (update_kernels.hpp) find that position with an integer maximum, which does not depend on the order of its operands.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define UPD_HD __host__ __device__ __forceinline__
#else
#define UPD_HD inline
#endif

namespace upd {

constexpr int64_t kMaxPositions = 0x7fffffff; // a position is an int32 of the owner array: n > 2^31 - 1 is refused
constexpr int kNoOwner = -1;                  // what the owner array holds between calls

// the local row of an id, or -1: "no row" (the rule of mips_hip_rows.h).  id >= idx_offset makes the true difference
// non-negative, and then the wrapping unsigned subtraction is the true difference -- no signed overflow for INT64_MIN or a
// negative offset, and nothing of an id above 2^32 is cut off.
UPD_HD int64_t local_row(int64_t id, int64_t idx_offset, int64_t ntotal) {
    if (id < idx_offset) return -1;
    const uint64_t local = (uint64_t)id - (uint64_t)idx_offset;
    return local < (uint64_t)ntotal ? (int64_t)local : -1;
}

// pass A folds every position into its row's owner with this (the device: atomicMax, the same function of two ints)
UPD_HD int fold_owner(int owner, int p) { return p > owner ? p : owner; }

// passes B and C: position p writes its row iff it is the row's owner when pass A is complete
UPD_HD bool wins(int owner, int p) { return owner == p; }

inline bool count_ok(int64_t n) { return n >= 0 && n <= kMaxPositions; }

// Host restatement over host ids: winners[p] = 1 iff position p writes its row; returns the number of distinct rows written.
// O(n log n) in n alone (never O(ntotal)): the (row, position) pairs of the valid positions, sorted.
inline int64_t host_winners(const int64_t* ids, int64_t n, int64_t idx_offset, int64_t ntotal, std::vector<unsigned char>* winners = nullptr) {
    std::vector<std::pair<int64_t, int64_t>> named; // (local row, position)
    for (int64_t p = 0; p < n; ++p) {
        const int64_t row = local_row(ids[p], idx_offset, ntotal);
        if (row >= 0) named.emplace_back(row, p);
    }
    std::sort(named.begin(), named.end());
    if (winners) winners->assign((size_t)n, 0);
    int64_t distinct = 0;
    for (size_t i = 0; i < named.size(); ++i) {
        if (i + 1 < named.size() && named[i + 1].first == named[i].first) continue; // a higher position names the same row
        ++distinct;
        if (winners) (*winners)[(size_t)named[i].second] = 1;
    }
    return distinct;
}

} // namespace upd
