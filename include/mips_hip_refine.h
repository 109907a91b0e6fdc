/* mips_hip_refine.h -- the two-stage search on PQ codes (faiss IndexRefineFlat / IndexIVFPQR): a candidate search of up to 1024 rows
 * on a PQ or IVFPQ index, and the exact re-ranking of candidate ids against a flat index.
 *
 * A PQ index ranks by a quantised score: its best 5 are rarely the true best 5, its best few hundred usually contain them.  So it is
 * used as a candidate generator -- ask it for kc = k * k_factor rows -- in front of a store that holds the rows themselves and scores
 * the candidates exactly.  Additive to mips_hip.h, mips_hip_rows.h, mips_hip_pq.h and mips_hip_ivfpq.h: same library, same
 * conventions (return codes, mips_last_error, streams, flags, -1 / -inf padding), no version of its own.
 *
 *   search_candidates(q, k)   the definition of mips_pq_search / mips_ivfpq_search, unchanged, for 1 <= k <= MIPS_MAX_K_WIDE: every
 *                    row of the index (of the p = min(nprobe, nlist) probed lists) is scored; the score is the float32 sum of the
 *                    query's table entries at the row's codes in ascending m (behind the coarse term T, by_residual); the result is
 *                    the best k by (score descending, row ascending), padding -1 / -inf, idx_offset added.  For k' <= k the first
 *                    k' columns are the result for k'.  For k <= MIPS_MAX_K the call IS the narrow entry point (the same launches):
 *                    the results are those of mips_pq_search / mips_ivfpq_search bit for bit.
 *   rerank(q, ids [nq, kc], k)   the best k of the SET of valid ids of each query's row of ids.  An id is valid iff
 *                    0 <= id - idx_offset < ntotal (the rule of mips_hip_rows.h); every other value -- the -1 padding of a search
 *                    among them -- is no row, on the host and on the device alike (nothing is refused); an id that occurs more
 *                    than once counts once.  The score of an id is what mips_score_subset reports for it (the library calls it), so
 *                    mips_score_subset on out_idx reproduces out_scores bit for bit; an id whose score is a NaN is dropped like an
 *                    invalid one.  Order: (score descending, id ascending); padding -1 / -inf; out_idx carries the ids as given
 *                    (idx_offset is not added again).  Inner-product indexes of every storage; on an SQ8 index the order is that of
 *                    the reported scores D = S + B_q rounded to float32, which need not be the order in which mips_search ranks
 *                    the integer sums S.
 *
 * Launches.  A candidate search with k > MIPS_MAX_K enqueues per slice of queries what the narrow search enqueues -- (probe,)
 * tables, ONE scan launch of ns * S workgroups, the merge of the S sorted partials, the finishing pass -- with the pool instance of
 * the scan: a wave keeps its best k in a pool of KP = 64, 256 or 1024 slots in LDS (the pool of mips_ivf_search_wide), a workgroup
 * has as many waves as pools fit beside the query's table in 160 KiB (16 .. 1; two at M = 128, KP = 1024, p = 1024), S * k <= 65536.
 * mips_index_rerank enqueues mips_score_subset into scratch and ONE select launch of nq workgroups.  Every grid, block, LDS size,
 * pointer and host loop bound comes from (ns, k, kc, M, d, p, nlist, ntotal, the compute units) and the indexes' parameters alone;
 * list numbers, bounds, rows and ids are read and range-checked on the device.  So with MIPS_Q_DEVICE | MIPS_OUT_DEVICE (and
 * MIPS_IDS_DEVICE) no call synchronises, and in steady state each may be captured into a HIP graph under the capture contract of
 * mips_ivfpq_search (mips_hip_ivfpq.h); for mips_index_rerank the graph stays valid until the flat index changes or a call of a larger
 * shape arrives.
 */
#ifndef MIPS_HIP_REFINE_H
#define MIPS_HIP_REFINE_H

#include "mips_hip.h"
#include "mips_hip_rows.h"
#include "mips_hip_pq.h"
#include "mips_hip_ivfpq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mips_pq_search; 1 <= k <= MIPS_MAX_K_WIDE.  MIPS_E_INVALID: what mips_pq_search refuses, with the wider bound on k. */
int mips_pq_search_candidates(mips_pq_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset,
                              int flags, void* hip_stream);

/* The arguments of mips_ivfpq_search; 1 <= k <= MIPS_MAX_K_WIDE.  "scan_segments" forces S here too, clipped to S * k <= 65536. */
int mips_ivfpq_search_candidates(mips_ivfpq_t* ix, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores,
                                 int64_t* out_idx, int64_t idx_offset, int flags, void* hip_stream);

/* The arguments of mips_score_subset with ids int64 [nq, kc], then k and the outputs out_scores float32 / out_idx int64 [nq, k];
 * 1 <= k <= kc <= MIPS_MAX_K_WIDE.  q host or device (MIPS_Q_DEVICE), ids host or device (MIPS_IDS_DEVICE), outputs host or device
 * (MIPS_OUT_DEVICE).  A host buffer synchronises.  MIPS_E_INVALID: k or kc outside their range, a bad q_dtype, an untrained SQ8 index,
 * NULL buffers with nq > 0.  MIPS_E_UNSUPPORTED: an L2 index.  nq == 0: MIPS_OK, nothing written. */
int mips_index_rerank(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int kc, int k, float* out_scores, int64_t* out_idx,
                      int64_t idx_offset, int flags, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_REFINE_H */
