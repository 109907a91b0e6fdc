/* mips_hip_ivfpq.h -- the IVF index over PQ codes (faiss IndexIVFPQ): k-means lists, nprobe, M one-byte codes per row, ADC search.
 *
 * The two halves exist on their own: mips_hip_ivf.h (lists over the rows of a flat index) and mips_hip_pq.h (M one-byte codes per
 * row, every search reads every code).  Here a search reads only the codes of nprobe of nlist lists, and a row is coded as the
 * RESIDUAL against its list's centroid, so the 256 centroids of a sub-quantiser cover a cluster's spread and not the whole data
 * set's.  For inner product the combination is exact to define:  <q, c_l + r> = <q, c_l> + <q, r>  -- the first term is the score the
 * probe computed, the second the ordinary ADC sum, and the lookup table depends on the query alone, not on the list.
 * Additive to mips_hip.h: same library, same conventions (return codes, mips_last_error, streams, flags, ties to the lowest row,
 * -1 / -inf padding), no version of its own.
 *
 * Everything here is exact and deterministic (the arithmetic is the one text of csrc/ivfpq_math.hpp over csrc/pq_math.hpp, compiled
 * for host and device); every step is one IEEE operation in a fixed order:
 *   canonical score  s(a, b) = (float) of the sequential fp64 sum over ascending t of (double)a_t (double)b_t
 *   coarse quantiser the rule of mips_hip_ivf.h word for word: nlist float32 centroids in an internal fp32-exact inner-product
 *                    index; "the nearest lists of x" are the top entries of ITS certified search on the float32 vector x (highest
 *                    s(x, c_l), ties to the lowest l) -- in training, in add and in the probe alike
 *   residual         r_t = x_t - c_{l,t}: ONE float32 subtraction per column, l the row's nearest list, taken on the float32 input
 *                    (bf16 widened exactly).  With by_residual = 0 a row is coded as it is.
 *   train(x [n, d])  the centroids are exactly those mips_ivf_train produces on the same x (its subsample rule, spherical k-means,
 *                    "ivf_niter", a list without members keeps its centroid: the library calls that trainer).  Then R = the PQ
 *                    subsample of x (all rows if n <= 65536, else x[floor(i n / 65536)]) with every row replaced by its residual
 *                    (by_residual = 0: as it is), and the codebook is exactly what mips_pq_train produces on R ("pq_niter").
 *                    MIPS_E_INVALID: n < max(nlist, 256), a NaN or an infinity in x, a residual that overflows, an index that
 *                    holds rows.  Training again is allowed while the index is empty.
 *   add(x)           assign_i = the nearest list of row i; code[i][m] = the nearest centroid (pq::nearest of pq_math.hpp) of
 *                    sub-vector m of the row's residual; rows get ids in arrival order; the list table (list_offsets [nlist + 1],
 *                    list_rows [ntotal], ascending inside each list) is rebuilt.
 *   add_codes        codes [n, M] and assign [n] stored as given; assign must lie in [0, nlist).
 *   lookup table     LUT_j[m][c] = s(q_j^m, C[m][c]), float32: the table of mips_hip_pq.h
 *   coarse term      T_{j,l} = s(q_j, c_l): what the coarse index's search reports for list l
 *   score of row i of probed list l for query j
 *                    acc = T_{j,l}; then for m = 0 .. M - 1 in ascending order: acc = acc + LUT_j[m][code[i][m]] -- each step ONE
 *                    float32 addition, never re-associated.  by_residual = 0: acc = LUT_j[0][code[i][0]], then m = 1 .. M - 1 (the
 *                    score of mips_hip_pq.h; there is no coarse term).
 *   search(q, k, nprobe)  P(q_j) = the p = min(nprobe, nlist) nearest lists of q_j; the result is the best k rows among those
 *                    whose list is in P(q_j), by (score descending, row ascending); padding -1 / -inf; idx_offset added;
 *                    1 <= k <= MIPS_MAX_K; p <= 1024
 *   reconstruct      row i = c_{assign_i,t} + C[m][code[i][m]][t]: ONE float32 addition per column (by_residual = 0: a plain decode)
 *   score_subset     the score text above with l = assign_id, whether or not that list would have been probed: scoring a search's
 *                    rows reproduces its scores bit for bit
 * Refused with MIPS_E_UNSUPPORTED: MIPS_METRIC_L2, nbits != 8, M > 128, d > 1024, nlist outside 1 .. 65536, min(nprobe, nlist) >
 * 1024.  MIPS_E_INVALID: M < 1, d % M != 0.  Not served at all: k > MIPS_MAX_K, range search, selectors and groups, removal and
 * update by id, sharding, OPQ.
 */
#ifndef MIPS_HIP_IVFPQ_H
#define MIPS_HIP_IVFPQ_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mips_ivfpq mips_ivfpq_t;

/* nbits: 8; by_residual: 0 or 1; metric: MIPS_METRIC_IP. */
int mips_ivfpq_create(mips_ivfpq_t** out, int device, int64_t d, int64_t nlist, int64_t M, int nbits, int by_residual, int metric);
int mips_ivfpq_destroy(mips_ivfpq_t* ix);

/* x: [n, d] float32 or bf16 (x_dtype), host or device (MIPS_Q_DEVICE in flags).  Synchronises. */
int mips_ivfpq_train(mips_ivfpq_t* ix, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream);
int mips_ivfpq_is_trained(const mips_ivfpq_t* ix);

/* HOST float32 [nlist, d] / [M][256][dsub], stored as given.  The index is trained once both are set.  MIPS_E_INVALID on non-finite
 * values and on an index that holds rows; get: MIPS_E_INVALID while that half is not set.  All synchronise. */
int mips_ivfpq_set_centroids(mips_ivfpq_t* ix, const float* centroids);
int mips_ivfpq_get_centroids(mips_ivfpq_t* ix, float* out_centroids);
int mips_ivfpq_set_codebook(mips_ivfpq_t* ix, const float* codebook);
int mips_ivfpq_get_codebook(mips_ivfpq_t* ix, float* out_codebook);

/* rows [n, d] float32 or bf16 (src_dtype), host or device (src_is_device): assigned, encoded and appended, 65536 rows at a time.
 * add_codes: dense codes [n, M] bytes and assign int32 [n], both host or both device, appended as they are.  Both rebuild the list
 * table.  MIPS_E_INVALID on an untrained index and on an assignment outside [0, nlist); MIPS_E_UNSUPPORTED past 2^31 - 256 rows. */
int mips_ivfpq_add(mips_ivfpq_t* ix, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream);
int mips_ivfpq_add_codes(mips_ivfpq_t* ix, const uint8_t* codes, const int32_t* assign, int64_t n, int src_is_device, void* hip_stream);

/* out_codes HOST [n, M], out_assign HOST int32 [n]: rows [row0, row0 + n).  out_sizes HOST int64 [nlist].  All synchronise. */
int mips_ivfpq_read_codes(mips_ivfpq_t* ix, int64_t row0, int64_t n, uint8_t* out_codes, void* hip_stream);
int mips_ivfpq_read_assign(mips_ivfpq_t* ix, int64_t row0, int64_t n, int32_t* out_assign, void* hip_stream);
int mips_ivfpq_list_sizes(mips_ivfpq_t* ix, int64_t* out_sizes, void* hip_stream);

/* P(q) and the coarse terms: out_lists int32 [nq, p], out_scores float32 [nq, p] (NULL: not wanted), p = min(nprobe, nlist), nearest
 * first; out_scores[j][u] = T_{j, out_lists[j][u]}.  Host outputs synchronise; with MIPS_OUT_DEVICE both are device memory and the
 * call follows the capture contract of mips_ivfpq_search. */
int mips_ivfpq_probe(mips_ivfpq_t* ix, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int32_t* out_lists, float* out_scores, int flags,
                     void* hip_stream);

/* q [nq, d] MIPS_DTYPE_F32 or MIPS_DTYPE_BF16, host or device (MIPS_Q_DEVICE); out_scores float32 / out_idx int64 [nq, k], host or
 * device (MIPS_OUT_DEVICE); 1 <= k <= MIPS_MAX_K; nprobe >= 1.  Host outputs synchronise; a device-in / device-out call never does.
 * MIPS_E_INVALID: an untrained index, a bad q_dtype, k outside 1 .. MIPS_MAX_K, nprobe < 1, NULL buffers with nq > 0.
 * MIPS_E_UNSUPPORTED: min(nprobe, nlist) > 1024.  nq == 0: MIPS_OK, nothing written.  An empty index: padding.  A query with a NaN
 * or an infinity may get any result; it reads nothing outside the index.
 *
 * What a call enqueues per slice of ns <= "pq_query_slice" queries (default 256) is a fixed sequence -- the probe (the coarse
 * index's own certified search: list numbers AND T), the tables LUT [ns][M][256], ONE scan launch of ns * S workgroups, the merge
 * of the S sorted partial lists, a finishing pass over [ns, k].  Workgroup (j, s) copies LUT_j into LDS once, builds the prefix of
 * the sizes of query j's p probed lists in LDS, and serves segment s of their concatenation in probe order: positions
 * [floor(N_j s / S), floor(N_j (s + 1) / S)), N_j the sum of the probed list sizes -- one lane per row, list by list, so T and the
 * list bounds are uniform over a wave.  List numbers, list bounds and row numbers are read and range-checked on the device: a bad
 * value reads nothing outside the index.  Every grid, block, LDS size, pointer and host loop bound comes from (ns, k, M, d, p, nlist,
 * ntotal, the compute units) and "scan_segments" alone, never from the values of the queries; the scratch grows only when a call
 * asks for more.  So in steady state a device-in / device-out search issues only stream operations and may be captured into a HIP
 * graph and replayed with other queries; the graph stays valid until mips_ivfpq_add, _add_codes, _train, _set_centroids,
 * _set_codebook, _set_param, _reset or _destroy, or a call of a larger shape. */
int mips_ivfpq_search(mips_ivfpq_t* ix, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                      int64_t idx_offset, int flags, void* hip_stream);

/* The arguments and the "no row" rule of mips_pq_reconstruct / mips_pq_score_subset (mips_hip_pq.h): an id is valid iff
 * 0 <= id - idx_offset < ntotal; any other id is a quiet-NaN row (MIPS_ROWS_ZERO_MISSING: zero bytes) / a score of -inf; a HOST id
 * >= 0 whose local row is >= ntotal returns MIPS_E_INVALID before anything is enqueued. */
int mips_ivfpq_reconstruct(mips_ivfpq_t* ix, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld, int flags,
                           void* hip_stream);
int mips_ivfpq_score_subset(mips_ivfpq_t* ix, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores,
                            int64_t idx_offset, int flags, void* hip_stream);

/* Drop all rows; centroids and codebook stay. */
int mips_ivfpq_reset(mips_ivfpq_t* ix);

/* "ivf_niter" / "pq_niter": k-means iterations of the two trainers (default 10, 0 .. 1000); "pq_query_slice": queries one pass of a
 * search serves (default 256, 1 .. 4096); "scan_segments": 0 = S chosen by the library, any other value (1 .. 65536) forces the
 * scan's S, clipped so that S * k stays within what the merge takes (65536 entries per query). */
int mips_ivfpq_set_param(mips_ivfpq_t* ix, const char* name, int64_t value);

int64_t mips_ivfpq_ntotal(const mips_ivfpq_t* ix);
int64_t mips_ivfpq_nlist(const mips_ivfpq_t* ix);
int64_t mips_ivfpq_m(const mips_ivfpq_t* ix);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_IVFPQ_H */
