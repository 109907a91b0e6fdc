// Pool arithmetic of the wide IVF search (include/mips_hip_ivf.h: mips_ivf_search_wide), one text for the kernel and a stand-alone
// check (tests/ivf_wide_math_check.cpp includes this file and nothing else of the library).  Every index that addresses a pool
// comes from here.
//   pool       a wave of the wide list scan keeps its best k candidates (key float, row int) in a pool of KP slots in LDS, KP the
//              smallest of 64, 256, 1024 with KP >= k.  The order is (key descending, row ascending): total over distinct rows.
//   fill       while the pool holds cnt < k entries, the candidates of a scoring pass (the lanes of a ballot mask) are appended
//              unsorted in lane order at slots cnt, cnt + 1, ...; candidates for which no room is left below k stay with their lanes
//   sort       a bitonic network over the first n slots, n = sort_span(cnt) the smallest power of two >= cnt (>= 2, <= KP), the
//              slots [cnt, n) padded with (-inf, kNoRow) first: afterwards slot u < cnt holds the pool's u-th best.  Run once when
//              the pool reaches k, or once at the end of a pool that never does
//   threshold  from then on slot k - 1 is the threshold: only a candidate that ranks before it is inserted
//   insert     at = count_before(pool[0, k), candidate) by binary search; the slots [at, k - 1) move one up in chunks of 64 from
//              the top (chunk c: destination k - 1 - 64 c - lane while that is > at, source one below; a chunk reads before it
//              writes and never reads what an earlier chunk wrote), the candidate goes to slot `at`, the old slot k - 1 is dropped
//   final      the four sorted pools of a workgroup hold distinct rows; entry u of pool w has rank u + sum over the other pools of
//              count_before(that pool, entry): every rank below the total is taken exactly once
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFW_HD __host__ __device__ __forceinline__
#else
#define IVFW_HD inline
#endif

namespace ivf {

constexpr int kWideLanes = 64;           // lanes of a wave: candidates of one scoring pass, slots one shift chunk moves
constexpr int kWideWaves = 4;            // pools of a workgroup (IVF_SCAN_WAVES)
constexpr int kWideMaxK = 1024;          // MIPS_MAX_K_WIDE
constexpr int kNoRow = 0x7fffffff;       // the row of a padding slot: ranks behind every row at equal key

// (key descending, row ascending)
IVFW_HD bool wide_before(float k1, int r1, float k2, int r2) { return k1 > k2 || (k1 == k2 && r1 < r2); }

// slots of a pool that serves k (1 <= k <= kWideMaxK)
IVFW_HD int pool_class(int k) { return k <= 64 ? 64 : k <= 256 ? 256 : 1024; }

// ---- fill: cnt < k entries in the pool, the lanes of `mask` carry candidates
// candidates this pass appends
IVFW_HD int fill_take(int cnt, int k, uint64_t mask) {
    const int have = __builtin_popcountll(mask), room = k - cnt;
    return have < room ? have : room;
}

// slot of lane `lane`'s candidate, or -1 when the lane carries none or no room below k is left for it (lane order is kept)
IVFW_HD int fill_slot(int cnt, int k, uint64_t mask, int lane) {
    if (((mask >> lane) & 1u) == 0) return -1;
    const int at = cnt + __builtin_popcountll(mask & (((uint64_t)1 << lane) - 1));
    return at < k ? at : -1;
}

// ---- sort: a bitonic network over the first n slots
IVFW_HD int sort_span(int cnt, int KP) {
    int n = 2;
    while (n < cnt) n *= 2;
    return n < KP ? n : KP;
}

// pair t (0 <= t < n / 2) of a stage with partner distance `stride`: its low and its high slot
IVFW_HD int bitonic_low(int t, int stride) { return 2 * t - (t & (stride - 1)); }
IVFW_HD int bitonic_high(int t, int stride) { return bitonic_low(t, stride) + stride; }

// direction of the pair whose low slot is `low` in the stages of run length `size`: true = the entry that ranks before goes low
IVFW_HD bool bitonic_best_low(int low, int size) { return (low & size) == 0; }

// ---- threshold
IVFW_HD int threshold_slot(int k) { return k - 1; }

// entries of the sorted run pk / pr [0, n) that rank before (key, row): the insertion rank, and a term of the final rank
IVFW_HD int count_before(const float* pk, const int* pr, int n, float key, int row) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wide_before(pk[mid], pr[mid], key, row)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- insert at `at` (0 <= at < k) into a full pool: [at, k - 1) moves one slot up
IVFW_HD int shift_chunks(int at, int k) { return (k - 1 - at + kWideLanes - 1) / kWideLanes; }

// destination of lane `lane` in chunk c; it moves iff the destination is > at, from the slot below
IVFW_HD int shift_dst(int k, int c, int lane) { return k - 1 - kWideLanes * c - lane; }

// ---- final: entry e of the workgroup's kWideWaves * KP slots
IVFW_HD int merge_pool(int e, int KP) { return e / KP; }
IVFW_HD int merge_slot(int e, int KP) { return e % KP; }

} // namespace ivf
