/* mips_hip_pq.h -- the product-quantised index (faiss IndexPQ): M one-byte codes per row, asymmetric-distance (ADC) search.
 *
 * A row of d columns is cut into M sub-vectors of dsub = d / M columns; each is replaced by the number of the nearest of 256
 * trained centroids of ITS sub-quantiser.  A row costs M bytes: at M = d / 8 a sixteenth of bf16 and an eighth of SQ8.  A query is
 * not quantised: its inner products with all M * 256 centroids form a lookup table, and the score of a row is the sum of the M
 * table entries its codes select.  Additive to mips_hip.h: same library, same conventions (return codes, mips_last_error, streams,
 * flags, ties to the lowest row, -1 / -inf padding), no version of its own.
 *
 * Everything here is exact and deterministic (the one text of csrc/pq_math.hpp, compiled for host and device):
 *   canonical score  s(a, b) = (float) of the sequential fp64 sum over ascending t of (double)a_t (double)b_t
 *   distance         u_t = x_t - c_t is ONE float32 subtraction; e(x, c) = the sequential fp64 sum over ascending t of (double)u_t^2
 *   nearest centroid scan j = 0 .. 255 with best = 0; j replaces best iff e_j < e_best (strict): ties go to the lowest j, a NaN
 *                    distance never wins, so every input has a defined code (an all-NaN or all-infinite sub-vector: code 0)
 *   train(x [n, d])  T = x if n <= 65536, else the 65536 rows x[floor(i n / 65536)].  The sub-quantisers train independently:
 *                    C[m][j] = T[floor(j |T| / 256)] restricted to sub-vector m, as given; then "pq_niter" (default 10, 0 allowed)
 *                    times: a_i = the nearest centroid of T_i^m; every centroid with members becomes (float)(S_t / count) per
 *                    column, S_t the sequential fp64 sum of (double)T_it over its members in ascending i; a centroid without
 *                    members keeps its value.  MIPS_E_INVALID: n < 256, a NaN or an infinity in x, an index that holds rows.
 *                    Training again is allowed while the index is empty.
 *   add(x)           code[i][m] = the nearest centroid of the row's sub-vector m, taken on the float32 input (bf16 widened exactly);
 *                    rows get ids in arrival order.  add_codes stores caller-supplied [n, M] bytes as they are.
 *   lookup table     LUT[m][c] = s(q^m, C[m][c]), float32
 *   score D(q, i)    acc = LUT[0][code[i][0]]; for m = 1 .. M - 1: acc = acc + LUT[m][code[i][m]] -- each step ONE float32 addition,
 *                    in ascending m, never re-associated, never widened.  A code is an unsigned byte.  (The other storages sum in
 *                    fp64; here the addends are float32 already and the fixed order makes the sum just as reproducible.)
 *   search           the best k rows (1 <= k <= MIPS_MAX_K) by (D descending, row ascending); padding -1 / -inf when ntotal < k;
 *                    idx_offset added to the rows
 *   reconstruct      row i = the concatenation of C[m][code[i][m]]: a bit move
 *   score_subset     D(q_j, id) by the text above: scoring a search's rows reproduces its scores bit for bit
 * Refused: MIPS_METRIC_L2, nbits != 8, M > 128 (MIPS_E_UNSUPPORTED), d > 1024 (MIPS_E_UNSUPPORTED), M < 1 or d % M != 0
 * (MIPS_E_INVALID).  Not served at all: k > MIPS_MAX_K, range search, selectors and groups, removal and update by id, sharding,
 * OPQ.  IVF over PQ codes is an index of its own: mips_hip_ivfpq.h.
 */
#ifndef MIPS_HIP_PQ_H
#define MIPS_HIP_PQ_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mips_pq mips_pq_t;

/* nbits: 8; metric: MIPS_METRIC_IP. */
int mips_pq_create(mips_pq_t** out, int device, int64_t d, int64_t M, int nbits, int metric);
int mips_pq_destroy(mips_pq_t* pq);

/* x: [n, d] float32 or bf16 (x_dtype), host or device (MIPS_Q_DEVICE in flags).  Synchronises. */
int mips_pq_train(mips_pq_t* pq, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream);
int mips_pq_is_trained(const mips_pq_t* pq);

/* HOST float32 [M][256][dsub].  set: stored as given and makes the index trained; MIPS_E_INVALID on non-finite values and on an
 * index that holds rows.  get: MIPS_E_INVALID on an untrained index.  Both synchronise. */
int mips_pq_set_codebook(mips_pq_t* pq, const float* codebook);
int mips_pq_get_codebook(mips_pq_t* pq, float* out_codebook);

/* rows [n, d] float32 or bf16 (src_dtype), host or device (src_is_device): encoded and appended.  codes: dense [n, M] bytes, host
 * or device, appended as they are.  read_codes: out HOST [n, M], the codes of rows [row0, row0 + n); synchronises.  The internal
 * row pitch is the library's own.  MIPS_E_INVALID on an untrained index; MIPS_E_UNSUPPORTED past 2^31 - 256 rows. */
int mips_pq_add(mips_pq_t* pq, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream);
int mips_pq_add_codes(mips_pq_t* pq, const uint8_t* codes, int64_t n, int src_is_device, void* hip_stream);
int mips_pq_read_codes(mips_pq_t* pq, int64_t row0, int64_t n, uint8_t* out_codes, void* hip_stream);

/* q [nq, d] MIPS_DTYPE_F32 or MIPS_DTYPE_BF16, host or device (MIPS_Q_DEVICE); out_scores float32 / out_idx int64 [nq, k], host or
 * device (MIPS_OUT_DEVICE); 1 <= k <= MIPS_MAX_K.  Host outputs synchronise; a device-in / device-out call never does.
 * MIPS_E_INVALID: an untrained index, a bad q_dtype, k outside 1 .. MIPS_MAX_K, NULL buffers with nq > 0.  nq == 0: MIPS_OK, nothing
 * written.  An empty index: padding.  A query with a NaN or an infinity may get any result; it reads nothing outside the index.
 *
 * What a call enqueues per slice of "pq_query_slice" queries (default 256: at most 32 MiB of tables) is a fixed sequence -- the
 * tables LUT [ns][M][256], ONE scan launch of ns * S workgroups (S row segments [floor(n s / S), floor(n (s + 1) / S)); the
 * workgroup copies its query's table into LDS and scores its segment, one lane per row), the merge of the S sorted partial lists,
 * a finishing pass over [ns, k] -- in which every grid, block, LDS size, pointer and loop bound comes from (ns, k, M, d, ntotal, the
 * compute units) alone, never from the values of the queries.  The scratch (staged host queries, tables, partial lists) grows only
 * when a search asks for more.  So in steady state a device-in / device-out search issues only stream operations and may be
 * captured into a HIP graph and replayed with other queries; the captured graph stays valid until mips_pq_add, _add_codes,
 * _train, _set_codebook, _reset or _destroy, or a search of a larger shape.
 * Large query batches are served, but are not what the index is for: the scan costs nq * ntotal * M table reads and shares nothing
 * between queries. */
int mips_pq_search(mips_pq_t* pq, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset,
                   int flags, void* hip_stream);

/* The arguments of mips_index_reconstruct / mips_score_subset (mips_hip_rows.h), on the codes: out[i, 0:d] = the decoded row
 * ids[i] - idx_offset at a pitch of out_ld elements, out_dtype MIPS_DTYPE_F32 only; out_scores[j, t] = D(q[j], row ids[j, t] -
 * idx_offset), ids and out_scores [nq][k], any k >= 0.  An id is valid iff 0 <= id - idx_offset < ntotal; any other id is "no row":
 * a quiet-NaN row (MIPS_ROWS_ZERO_MISSING: zero bytes) / a score of -inf.  A HOST id >= 0 whose local row is >= ntotal returns
 * MIPS_E_INVALID before anything is enqueued.  flags: MIPS_IDS_DEVICE, MIPS_OUT_DEVICE, MIPS_ROWS_ZERO_MISSING / MIPS_Q_DEVICE.
 * With device ids, output (and queries) nothing synchronises. */
int mips_pq_reconstruct(mips_pq_t* pq, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld, int flags,
                        void* hip_stream);
int mips_pq_score_subset(mips_pq_t* pq, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores, int64_t idx_offset,
                         int flags, void* hip_stream);

/* Drop all rows; the codebook stays. */
int mips_pq_reset(mips_pq_t* pq);

/* "pq_niter": k-means iterations of mips_pq_train (default 10, 0 .. 1000); "pq_query_slice": queries one pass of a search serves
 * (default 256, 1 .. 4096). */
int mips_pq_set_param(mips_pq_t* pq, const char* name, int64_t value);

int64_t mips_pq_ntotal(const mips_pq_t* pq);
int64_t mips_pq_m(const mips_pq_t* pq);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_PQ_H */
