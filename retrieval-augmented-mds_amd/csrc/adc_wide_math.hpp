// Launch arithmetic of the candidate search on PQ codes (include/mips_hip_refine.h: mips_pq_search_candidates /
// mips_ivfpq_search_candidates, MIPS_MAX_K < k <= MIPS_MAX_K_WIDE), one text for the host, the kernels and a
// stand-alone check (tests/adc_wide_math_check.cpp includes this file and, through it, ivfpq_math.hpp and ivf_wide_math.hpp -- nothing
// else of the library, and no HIP).  The pool itself -- fill, sort, threshold, insert, final rank -- is ivf_wide_math.hpp as it is.
//
//   LDS of a workgroup   the query's table [M][256] float32, then P pools of KP slots (keys float32 [P][KP], rows int32 [P][KP]),
//                        the pools' counts [kMaxPools], and for the list scan the prefix of the p probed list sizes [p + 1], the
//                        lists' first positions [p] and their coarse terms [p] (p = 0: the flat scan, none of the three)
//   pools P              as many as the base scan has waves (pq::scan_waves: 16 behind a table of more than 32 KiB, else 4), cut to
//                        what fits into 160 KiB beside the table and the prefix; never fewer than one -- at M = 128, KP = 1024,
//                        p = 1024 two pools of 8 KiB fit
//   waves                P: a pool belongs to ONE wave, so its steps are ordered by wave barriers alone and no wave waits for
//                        another inside the scan loop; a large table under wide pools is scanned by fewer waves
//   segments S           as pq::choose_segments chooses them, from the pools' own workgroups per compute unit and rows per pass;
//                        S * k within what the merge takes (65536 entries per query: S <= 64 at k = 1024)
#pragma once
#include "ivf_wide_math.hpp"
#include "ivfpq_math.hpp"

namespace adcw {

constexpr int64_t kLdsBudget = (int64_t)160 << 10; // LDS of a compute unit, and the most one workgroup asks for
constexpr int kMaxPools = 16;                      // pq::scan_waves at most
constexpr int kMinK = 30;                          // below: the register lists of the base scans (MIPS_MAX_K = 29)

// bytes of one pool: a float32 key and an int32 row per slot
PQ_HD int64_t pool_bytes(int KP) { return (int64_t)KP * 8; }

// bytes beside the pools: the table, the pools' counts, the three arrays of the probed lists (p > 0)
PQ_HD int64_t fixed_bytes(int M, int p) { return (int64_t)M * pq::kSub * 4 + (int64_t)kMaxPools * 4 + (p > 0 ? ((int64_t)3 * p + 1) * 4 : 0); }

// pools of a workgroup (KP = ivf::pool_class(k); p = 0 for the flat scan)
PQ_HD int pools(int M, int KP, int p) {
    const int64_t fit = (kLdsBudget - fixed_bytes(M, p)) / pool_bytes(KP);
    const int64_t most = pq::scan_waves(M);
    const int64_t P = fit < most ? fit : most;
    return (int)(P < 1 ? 1 : P);
}

// waves of a workgroup: one per pool
PQ_HD int waves(int M, int KP, int p) { return pools(M, KP, p); }

// dynamic LDS a workgroup asks for
PQ_HD int64_t lds_bytes(int M, int KP, int p) { return fixed_bytes(M, p) + (int64_t)pools(M, KP, p) * pool_bytes(KP); }

// workgroups one compute unit holds (160 KiB of LDS, 32 waves)
PQ_HD int blocks_per_cu(int M, int KP, int p) {
    const int64_t by_lds = kLdsBudget / lds_bytes(M, KP, p);
    const int64_t by_waves = 32 / waves(M, KP, p);
    const int64_t b = by_lds < by_waves ? by_lds : by_waves;
    return (int)(b < 1 ? 1 : b);
}

// S, forced (0 < forced) or: two rounds of workgroups on every compute unit, no segment shorter than one pass of the workgroup
// over `rows` rows (unless there is one segment); S * k within the merge either way.  rows: ntotal, or ivfpq::expected_rows
PQ_HD int choose_segments(int64_t ns, int64_t k, int M, int p, int64_t rows, int64_t cus, int64_t forced) {
    const int KP = ivf::pool_class((int)k);
    int64_t S = forced;
    if (forced <= 0) {
        const int64_t want = 2 * cus * blocks_per_cu(M, KP, p);
        S = (want + ns - 1) / ns;
        const int64_t pass = (int64_t)ivf::kWideLanes * waves(M, KP, p);
        const int64_t most = (rows + pass - 1) / pass;
        if (S > most) S = most;
    }
    if (S * k > pq::kMergeLimit) S = pq::kMergeLimit / k;
    return (int)(S < 1 ? 1 : S);
}

// ---- the final rank inside a workgroup: entry e of its P * KP slots
PQ_HD int rank_pool(int e, int KP) { return ivf::merge_pool(e, KP); }
PQ_HD int rank_slot(int e, int KP) { return ivf::merge_slot(e, KP); }

// rank of entry `slot` of sorted pool w among the union of the P sorted pools (distinct rows: every rank below the total is taken
// once); stops counting at `stop` (the caller drops ranks >= k).  pk / pr [P][KP], cnt [P]
PQ_HD int union_rank(const float* pk, const int* pr, const int* cnt, int P, int KP, int w, int slot, int stop) {
    const float key = pk[(int64_t)w * KP + slot];
    const int row = pr[(int64_t)w * KP + slot];
    int rank = slot;
    for (int w2 = 0; w2 < P && rank < stop; ++w2)
        if (w2 != w) rank += ivf::count_before(pk + (int64_t)w2 * KP, pr + (int64_t)w2 * KP, cnt[w2], key, row);
    return rank;
}

// ---- the re-ranking select (mips_index_rerank): one workgroup sorts kc <= 1024 (score, id) pairs by (score descending, id ascending)
constexpr int kRerankMax = 1024;                   // MIPS_MAX_K_WIDE
constexpr int64_t kNoId = 0x7fffffffffffffffll;    // the id of an entry that is no row: ranks behind every id at equal score

PQ_HD bool rerank_before(float s1, int64_t i1, float s2, int64_t i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// is id a row of an index of ntotal rows?  (the rule of include/mips_hip_rows.h)
PQ_HD bool rerank_valid(int64_t id, int64_t idx_offset, int64_t ntotal) {
    if (id == kNoId || id < idx_offset) return false;
    return (uint64_t)id - (uint64_t)idx_offset < (uint64_t)ntotal; // (id >= idx_offset: the difference is exact in 64 unsigned bits)
}

// after the sort: entry u is kept iff it is a row and its id differs from the entry before it (equal ids are adjacent: they carry
// equal scores)
PQ_HD bool rerank_keep(const int64_t* ids, int u) { return ids[u] != kNoId && (u == 0 || ids[u - 1] != ids[u]); }

} // namespace adcw
