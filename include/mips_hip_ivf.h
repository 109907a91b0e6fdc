/* mips_hip_ivf.h -- the IVF index: an inverted file (k-means lists, nprobe) over the rows of a flat index.
 *
 * The reference ships `mips_string_factory: IVF256,SQ8`, `mips_nprobe`, `mips_train_size` (sotasum/config.yaml:94-97,
 * sotasum/mips.py:333-345).  The call it makes -- a handful of queries against the whole knowledge base, once per training step --
 * is bound by the bytes of the rows; an inverted file that scores only the rows of nprobe of nlist lists reads nprobe / nlist of
 * them.  Additive to mips_hip.h: same library, same conventions (return codes, mips_last_error, streams, ties to the lowest row,
 * -1 / -inf padding), no version of its own.
 *
 * Everything here is exact and deterministic:
 *   canonical score  s(a, b) = (float) of the sequential fp64 sum over ascending j of (double)a_j (double)b_j
 *   normalise(v)     t = sequential fp64 sum of (double)v_j^2; t == 0: v stays; else v_j = (float)((double)v_j / sqrt(t))
 *   coarse quantiser nlist float32 centroids in an internal fp32-exact inner-product index; "the nearest lists of x" are the top
 *                    entries of ITS certified search on the float32 vector x (highest s(x, c_l), ties to the lowest l) -- in
 *                    training, in add and in probe alike
 *   train(x [n, d])  T = x if n <= 256 nlist, else the m = 256 nlist rows x[floor(i n / m)];  c_l = normalise(T[floor(l m / nlist)]);
 *                    "ivf_niter" (default 10, 0 allowed) times: a_i = the nearest list of T_i; every list with members:
 *                    mean_lj = (float)(S / count), S the sequential fp64 sum of (double)T_ij over its members in ascending i,
 *                    c_l = normalise(mean_l); a list without members keeps its centroid.  An SQ8 index also trains its per-column
 *                    range on the whole x (mips_index_sq8_train).  MIPS_E_INVALID: n < nlist, a NaN or an infinity in x, an index
 *                    that holds rows.  Training again is allowed while the index is empty.
 *   add(x)           assign_i = the nearest list of the row as float32 INPUT (before any storage rounding); the rows go into the
 *                    inner flat index in arrival order, so row ids are the flat ids; the list table (list_offsets [nlist + 1],
 *                    list_rows [ntotal], ascending inside each list) is rebuilt.  Rows are float32 or bf16 values: raw codes are
 *                    MIPS_E_UNSUPPORTED.
 *   probe(q, nprobe) P(q) = the p = min(nprobe, nlist) nearest lists of the float32 query, nearest first.
 *   search(q, k, nprobe)  for query j: A_j = the rows i with assign_i in P(q_j); the result is what the flat index's mips_search
 *                    returns for q_j on an index from which the rows outside A_j were deleted, row numbers kept: the flat storage's
 *                    canonical score (bf16: stored bf16 rows, queries staged to bf16; F32: the caller's float32 rows and queries;
 *                    SQ8: ranked by S(q, i), reported as D(q, i) = (float)((double)S + B_q) of mips_hip_sq8.h -- ranked and merged
 *                    on S, converted to D once the order is fixed, so two rows with different S and equal D keep the order of S),
 *                    order by (score descending, row ascending), -1 / -inf padding when |A_j| < k, idx_offset added to the rows.
 *                    Hence: mips_score_subset on mips_ivf_flat of the returned rows gives the returned scores bit for bit, and
 *                    nprobe >= nlist gives mips_search's result on mips_ivf_flat bit for bit.  Every row of the probed lists is
 *                    scored exactly (the sequential fp64 sum); nothing is approximated and nothing needs a certificate.
 * Refused: MIPS_METRIC_L2 (the index ranks by inner product), d > 1024, the e4m3 storages, nlist outside 1 .. 65536, p > 1024.
 * The range form -- every probed, admitted row above a per-query radius, in CSR form -- is declared in mips_hip_ivf_range.h.
 * Overwriting stored rows by id, with their assignments following (faiss IndexIVF::update_vectors), is mips_ivf_update in
 * mips_hip_write.h; like mips_ivf_add it ends the validity of a captured search.
 */
#ifndef MIPS_HIP_IVF_H
#define MIPS_HIP_IVF_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mips_ivf mips_ivf_t;

/* doc_dtype: MIPS_DTYPE_BF16, MIPS_DTYPE_F32 or MIPS_DTYPE_SQ8 (the storage of the inner flat index); metric: MIPS_METRIC_IP. */
int mips_ivf_create(mips_ivf_t** out, int device, int64_t d, int doc_dtype, int metric, int64_t nlist);
int mips_ivf_destroy(mips_ivf_t* ivf);

/* The inner flat index, BORROWED (it goes with the IVF index): for mips_index_reconstruct, mips_index_read_rows, labels,
 * mips_score_subset, the SQ8 parameters.  Adding to it or removing from it directly breaks the list table. */
mips_index_t* mips_ivf_flat(mips_ivf_t* ivf);

/* x: [n, d] float32 or bf16 (x_dtype), host or device (MIPS_Q_DEVICE in flags).  Synchronises. */
int mips_ivf_train(mips_ivf_t* ivf, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream);
int mips_ivf_is_trained(const mips_ivf_t* ivf);

/* HOST float32 [nlist, d].  set: stored as given (not normalised) and makes the index trained (an SQ8 index needs its range too:
 * mips_index_sq8_set_params on mips_ivf_flat); MIPS_E_INVALID on non-finite values and on an index that holds rows. */
int mips_ivf_set_centroids(mips_ivf_t* ivf, const float* centroids);
int mips_ivf_get_centroids(mips_ivf_t* ivf, float* out_centroids);

int mips_ivf_add(mips_ivf_t* ivf, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream);

/* P(q): q [nq, d] float32 or bf16, host or device (MIPS_Q_DEVICE in flags); out_lists HOST int32 [nq, min(nprobe, nlist)], nearest
 * first.  nprobe >= 1, min(nprobe, nlist) <= 1024 (up to MIPS_MAX_K lists through mips_search, more through mips_search_wide: both
 * certified).  Synchronises.  With MIPS_OUT_DEVICE in flags out_lists is DEVICE int32 [nq, p] and the call never synchronises (it
 * writes through the scratch of mips_ivf_search and follows its capture contract, below). */
int mips_ivf_probe(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int32_t* out_lists, int flags, void* hip_stream);

/* The search over the probed lists (the definition: "search" above).  q [nq, d] MIPS_DTYPE_F32 or MIPS_DTYPE_BF16, host or device
 * (MIPS_Q_DEVICE); out_scores float32 / out_idx int64 [nq, k], host or device (MIPS_OUT_DEVICE); 1 <= k <= MIPS_MAX_K; nprobe as
 * mips_ivf_probe.  Host outputs synchronise; a device-in / device-out call never does.
 * MIPS_E_INVALID: an untrained index, a bad q_dtype, k outside 1 .. MIPS_MAX_K, nprobe < 1, NULL buffers with nq > 0.
 * MIPS_E_UNSUPPORTED: min(nprobe, nlist) > 1024.  nq == 0: MIPS_OK, nothing written.  An empty index: padding (-1 / -inf).
 * A query with a NaN or an infinity may get any result; it reads nothing outside the index.
 *
 * What a call enqueues is a fixed sequence -- the probe (the coarse index's own certified search), the staging of the queries as
 * the flat index stages them, ONE list-scan launch of nq * p * S workgroups (S = segments per probed list, a power of two <= 32
 * chosen from nq, p, k and the device's compute units), the merge of the sorted partial lists, a finishing pass over [nq, k] -- in
 * which no grid, pointer, size or loop bound depends on the VALUES of the queries: list numbers, list bounds and row numbers are
 * read and range-checked on the device.  Its scratch (probe buffer, staged queries, partial lists) is the search's own and grows
 * only when a search asks for a larger (nq, p, S, k).  So in steady state a device-in / device-out search issues only stream
 * operations and may be captured into a HIP graph and replayed with other queries; the captured graph stays valid until a search
 * (or a device-output probe) of a larger shape, or until mips_ivf_train, _set_centroids, _add, _remove, _set_assign, _reset or
 * _destroy (add also grows the coarse index's scratch and may move the rows and the list table). */
int mips_ivf_search(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                    int64_t idx_offset, int flags, void* hip_stream);

/* The search over the probed lists under a filter: a bitmap over the rows (_sel), and per-query group labels on top of it (_grp).
 * Row i is ADMITTED for query j iff both hold:
 *   - sel_bits == NULL, or bit sel_bit0 + i of the bitmap is set (least significant bit of a byte first);
 *   - q_labels == NULL, or the group rule holds: q_labels[j] == MIPS_LABEL_NONE, or label[i] != q_labels[j] under
 *     MIPS_GRP_EXCLUDE, or label[i] == q_labels[j] under MIPS_GRP_ONLY.
 * Layout, flags (MIPS_SEL_DEVICE: sel_bits is device memory; MIPS_GRP_DEVICE: q_labels [nq] is device memory) and labels are those
 * of mips_search_wide_sel / _grp (mips_hip.h); label[i] is the label of the inner flat index (mips_index_set_labels on
 * mips_ivf_flat), which follows its row through mips_ivf_remove.
 * The result for query j is what mips_ivf_search returns for j on an index from which the rows not admitted for j were deleted,
 * row numbers kept: the best k of A_j n admitted_j by the storage's canonical score (SQ8 ranked and merged on S, turned into D once
 * the order is fixed), order (score descending, row ascending), -1 / -inf padding, idx_offset added.  Everything stays exact.
 * Hence: with sel_bits == NULL and q_labels == NULL the call IS mips_ivf_search (same launches, same bits); on a BF16 or F32 index
 * with nprobe >= nlist the result is the first k columns of mips_search_wide_grp(k = 30) under the same filter, bit for bit; and
 * mips_score_subset on mips_ivf_flat reproduces the scores.  A filtered top-k cannot be had by fetching more and dropping: a group
 * has no bounded size.  The rule is applied inside the list scan, where a row number is read; the bytes of a row that is not
 * admitted are never requested, and the admitted rows are compacted before they are scored, so a sparse filter costs what it admits.
 * mips_ivf_search_sel is mips_ivf_search_grp with q_labels == NULL.
 * MIPS_E_INVALID: what mips_ivf_search refuses; sel_bit0 < 0 or sel_bit0 + ntotal > sel_nbits; a grp_mode other than 0 / 1; a
 * grouped call on an index whose labelled prefix is not exactly ntotal.  nq == 0: MIPS_OK.  Limits: those of mips_ivf_search.
 * A host bitmap (the bytes that cover the index's rows) and host q_labels travel by the stream's asynchronous copy into the
 * search's own scratch.  With device queries, outputs, bitmap and labels the call issues only stream operations, and no grid,
 * pointer, size or loop bound depends on the VALUES of the queries, the query labels or the bitmap: the capture contract of
 * mips_ivf_search holds, and a captured graph replays with other queries, other q_labels contents and other bitmap contents of
 * the same size. */
int mips_ivf_search_sel(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                        int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, void* hip_stream);
int mips_ivf_search_grp(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                        int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                        int grp_mode, void* hip_stream);

/* The WIDE search over the probed lists: mips_ivf_search / _sel / _grp with 1 <= k <= MIPS_MAX_K_WIDE -- for measuring recall@100
 * against the flat index when choosing nprobe, for retrieve-then-rerank, and for mining hard negatives ("the best 64 rows that are
 * not of my article": q_labels with MIPS_GRP_EXCLUDE) at IVF cost.  The definition is the one above, word for word: P(q_j), A_j,
 * admitted_j, the best k of A_j n admitted_j by the storage's canonical score (SQ8 ranked and merged on S, turned into D once the
 * order is fixed), order (score descending, row ascending), -1 / -inf padding, idx_offset added.  Nothing is approximated and
 * nothing is certified: every probed row is scored exactly, so unlike mips_search_wide on a flat index the call needs no
 * approximate pass, no candidate pool and no certificate -- only a wider exact selection inside the list scan.  Hence:
 *   - prefix: for k' <= k the first k' columns equal the call with k', bit for bit; for k' <= MIPS_MAX_K they equal
 *     mips_ivf_search / _sel / _grp with k' (for k <= MIPS_MAX_K the call issues exactly their launches);
 *   - every list probed: on a BF16 or F32 index with nprobe >= nlist the result is mips_search_wide / _sel / _grp on mips_ivf_flat
 *     under the same filter, bit for bit;
 *   - scores by id: mips_score_subset on mips_ivf_flat reproduces the scores;
 *   - no filter: with sel_bits == NULL and q_labels == NULL, mips_ivf_search_wide_grp IS mips_ivf_search_wide (same launches, same
 *     bits).  A bitmap alone is q_labels == NULL: there is no third entry point.
 * Arguments, flags, host / device forms and synchronisation are those of mips_ivf_search / mips_ivf_search_grp.
 * MIPS_E_INVALID: what mips_ivf_search_grp refuses, k < 1, MIPS_OUT_PACKED (it would serve a sharded IVF index, which does not
 * exist).  MIPS_E_UNSUPPORTED: k > MIPS_MAX_K_WIDE, min(nprobe, nlist) > 1024, and min(nprobe, nlist) * k > 65536 -- the entries
 * per query mips_merge_topk_sorted_packed takes.  nq == 0: MIPS_OK.  An empty index: padding.
 * The launch sequence is that of mips_ivf_search -- probe, staging, ONE list-scan launch of nq * p * S workgroups, the merge of the
 * p * S sorted partial lists of k entries, the finishing pass -- with, for k > MIPS_MAX_K, the wide list scan as its third launch:
 * every wave keeps its best k in a pool in LDS (64, 256 or 1024 slots, the smallest that holds k) instead of in registers.  The
 * capture contract of mips_ivf_search / _grp holds unchanged. */
int mips_ivf_search_wide(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                         int64_t idx_offset, int flags, void* hip_stream);
int mips_ivf_search_wide_grp(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                             int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                             int grp_mode, void* hip_stream);

/* mips_index_remove on the inner index, the same order-preserving compaction of the assignments, the list table rebuilt.
 * Arguments as mips_index_remove (include/mips_hip_update.h); out_counts[0] = rows removed. */
int mips_ivf_remove(mips_ivf_t* ivf, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, int flags, int64_t out_counts[2],
                    void* hip_stream);

/* Drop all rows; centroids (and an SQ8 range) stay. */
int mips_ivf_reset(mips_ivf_t* ivf);

/* out_sizes HOST int64 [nlist]; out_assign HOST int32 [n], the lists of rows [row0, row0 + n).  Both synchronise. */
int mips_ivf_list_sizes(mips_ivf_t* ivf, int64_t* out_sizes, void* hip_stream);
int mips_ivf_read_assign(mips_ivf_t* ivf, int64_t row0, int64_t n, int32_t* out_assign, void* hip_stream);

/* load(): the assignments of ALL the rows the inner index holds (added to it directly, in their stored form), HOST int32
 * [ntotal] with values in [0, nlist); rebuilds the list table. */
int mips_ivf_set_assign(mips_ivf_t* ivf, const int32_t* assign, int64_t n, void* hip_stream);

/* "ivf_niter": k-means iterations of mips_ivf_train (default 10, >= 0). */
int mips_ivf_set_param(mips_ivf_t* ivf, const char* name, int64_t value);

int64_t mips_ivf_nlist(const mips_ivf_t* ivf);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_IVF_H */
