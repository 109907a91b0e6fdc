/* mips_hip_rows.h -- entry points that give stored rows back by id, or score rows the caller names.
 *
 * Everything a search returns is (D, I); these calls lead from I back to the index: the stored vectors, their labels, and
 * the canonical score of chosen (query, row) pairs.  Conventions, error codes and the error text are those of
 * mips_hip.h; the same libmips_hip.so exports everything and there is one ABI version, defined there.
 *
 * Common to the three calls
 *   ids          int64, host memory unless MIPS_IDS_DEVICE.  The local row of an id is id - idx_offset; an id is VALID iff
 *                0 <= id - idx_offset < ntotal, compared as int64 (2^32 + 3 is not row 3).  Every other id means "no row":
 *                search pads with -1, a row shard is handed ids of other shards.
 *   host ids     are checked before anything is enqueued: an id >= 0 whose local row is >= ntotal returns MIPS_E_INVALID
 *                and nothing is written.  Negative ids and ids below idx_offset are allowed ("no row").  Device ids are
 *                never read by the host; an invalid one is "no row".
 *   launches     one kernel launch per call, whatever n is (mips_score_subset: plus the query staging of mips_search).
 *   ordering     as every call on the index: behind the calls before it on any stream.  With MIPS_IDS_DEVICE and
 *                MIPS_OUT_DEVICE (mips_score_subset: and MIPS_Q_DEVICE) nothing synchronises and no memory outside the
 *                index, the ids and the output is read.  Host ids, host queries or host output synchronise hip_stream.
 *   mutation     nothing is cached between calls: the calls follow reserve, growth, reset + add and mips_index_remove.
 */
#ifndef MIPS_HIP_ROWS_H
#define MIPS_HIP_ROWS_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of this header (bits no other header uses); MIPS_Q_DEVICE, MIPS_OUT_DEVICE and MIPS_FORCE_IP are mips_hip.h's */
#define MIPS_IDS_DEVICE 64         /* ids is device memory */
#define MIPS_ROWS_ZERO_MISSING 128 /* mips_index_reconstruct: "no row" gives all-zero bytes instead of NaN */

/* out[i, 0:d] = stored row ids[i] - idx_offset, at a row pitch of out_ld ELEMENTS (out_ld >= d); columns d .. out_ld - 1
 * of the output are never written, the padding columns of the storage never appear.
 *
 * out_dtype  MIPS_DTYPE_F32: the decoded values.  Decoding is exact and involves no arithmetic: a bf16 value becomes the
 *            float32 whose upper half is the stored bits, an e4m3 value its exact float32; a MIPS_DTYPE_F32 index returns
 *            the float32 values it was given bit for bit (-0.0, denormals and NaN payloads included).
 *            The storage's element type (MIPS_DTYPE_BF16 for a bf16 index, MIPS_DTYPE_FP8_E4M3 for both e4m3 storages):
 *            the raw bits, 2 or 1 bytes per element.  Anything else: MIPS_E_INVALID.
 * no row     float32 output: a quiet-NaN row (0x7FC00000); raw output: 0x7FC0 (bf16) / 0x7F (e4m3).  With
 *            MIPS_ROWS_ZERO_MISSING: all-zero bytes (a row shard: the shards' outputs then add up to the rows).
 * flags      MIPS_IDS_DEVICE, MIPS_OUT_DEVICE, MIPS_ROWS_ZERO_MISSING.
 * MIPS_E_INVALID: NULL index, n < 0, out_ld < d, NULL ids or out while n > 0, a bad out_dtype, a host id past the index. */
int mips_index_reconstruct(mips_index_t* index, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype,
                           int64_t out_ld, int flags, void* hip_stream);

/* out[i] = the label (mips_index_set_labels) of row ids[i] - idx_offset; "no row" and rows past the labelled prefix give
 * MIPS_LABEL_NONE.  flags: MIPS_IDS_DEVICE, MIPS_OUT_DEVICE. */
int mips_index_gather_labels(mips_index_t* index, const int64_t* ids, int64_t n, int64_t idx_offset, int32_t* out, int flags,
                             void* hip_stream);

/* out_scores[j, t] = the canonical score of (q[j], row ids[j, t] - idx_offset), ids and out_scores [nq][k], in the caller's
 * order, nothing ranked.  The queries are staged exactly as mips_search stages them for this index (rounded to bf16, kept
 * as float32, or quantised to e4m3); the score is (float) of the sequential fp64 sum of q.x over the stored values, on an
 * L2 index without MIPS_FORCE_IP the distance (float)(|q|^2 + phi - 2 q.x) with |q|^2 the same kind of sum and phi as the
 * searches use it (mips_index_phi: computed with one synchronisation when it is not known).  For any (D, I) that
 * mips_search, mips_search_wide or mips_range_search returned, scoring I gives D bit for bit.
 * "No row" scores -inf (inner product) / +inf (L2).  Any k >= 0 (MIPS_MAX_K does not apply), every d and every storage.
 * flags: MIPS_Q_DEVICE, MIPS_OUT_DEVICE, MIPS_IDS_DEVICE, MIPS_FORCE_IP. */
int mips_score_subset(mips_index_t* index, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores,
                      int64_t idx_offset, int flags, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_ROWS_H */
