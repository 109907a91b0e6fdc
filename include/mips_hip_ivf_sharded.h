/* mips_hip_ivf_sharded.h -- the IVF search cut at its merge: what a ROW-SHARDED IVF index needs (ShardedIvfIndex).
 *
 * One logical IVF index whose rows are split contiguously over parts (ranks), every part an mips_ivf_t with the SAME centroids (and,
 * for SQ8, the same per-column range) that holds the rows of its range.  Then the lists of a part are the global lists restricted to
 * its rows (the list of a row depends on the float32 row and the centroids only), the probe P(q) is the same on every part (it
 * depends on the query and the centroids only), and the best k of the union are the best k of the parts' best k.  mips_ivf_search
 * already ends in "merge p * S sorted partial lists, then finish"; the sharded search is that search cut behind its merge, with ONE
 * all-gather in the cut:
 *     every part      mips_ivf_search_part  -> the payload int64 [nq, k, 2] (+ B_q of an SQ8 index)
 *     the exchange    an all-gather of the payloads: gathered [parts, nq, k, 2], part p holding lower global rows than part p + 1
 *     every part      mips_ivf_merge_parts  -> out_scores / out_idx [nq, k]
 * and the result is, bit for bit, what mips_ivf_search_wide_grp returns on the one unsharded index that holds all the rows in global
 * order: scores, rows, order (score descending, global row ascending), -1 / -inf padding.  SQ8 is ranked and merged on S ACROSS the
 * parts too and turned into D = (float)((double)S + B_q) only once the cross-part order is fixed, so two rows with different S and
 * equal D keep the order of S wherever they are stored.
 * Additive to mips_hip_ivf.h: same library, same conventions, no version of its own.  What mips_ivf_search* accept is unchanged.
 * The range search needs nothing from here: mips_ivf_range_search_grp writes (lims, D, I) with idx_offset into a part record and
 * mips_range_merge_records (mips_hip_sharded.h) lays the records end to end -- SQ8 hits are decided on D per row, nothing is
 * compared across parts.
 */
#ifndef MIPS_HIP_IVF_SHARDED_H
#define MIPS_HIP_IVF_SHARDED_H

#include "mips_hip_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The part search: mips_ivf_search_wide_grp up to and including the merge of its p * S partial lists, 1 <= k <= MIPS_MAX_K_WIDE,
 * sel_bits == NULL and q_labels == NULL meaning unfiltered.  In the place of out_scores / out_idx:
 *   out_packed  int64 [nq, k, 2], the payload mips_merge_topk_sorted_packed reads: entry t of query j is {the float32 bits of the
 *               score in the RANKING domain, zero-extended (SQ8: S, not D); row + idx_offset}, in result order; a padding entry is
 *               {the bits of -inf, -1}, idx_offset not added
 *   out_bias    float64 [nq], B_q of every query: written on an SQ8 index (where it must not be NULL), untouched otherwise (NULL is
 *               fine).  It is the call's only other result: NOTHING of a part search is kept in the index for the merge.
 * Both are host memory, or device memory under MIPS_OUT_DEVICE.  Arguments, flags, host / device forms, synchronisation and
 * refusals are those of mips_ivf_search_wide_grp (MIPS_OUT_PACKED stays MIPS_E_INVALID: the payload is this call's only form; a NULL
 * out_packed, or a NULL out_bias on an SQ8 index, with nq > 0: MIPS_E_INVALID).  nq == 0: MIPS_OK.  An empty part: padding.
 * The call enqueues mips_ivf_search's own launches with a packing pass in the place of the finishing pass -- no grid, pointer or size
 * depends on the values of the queries -- so the capture contract of mips_ivf_search / _grp holds unchanged.  One thing to know: the
 * merged lists pass through scratch of the search ([nq, k] scores and rows) also in the device form, which a device-form
 * mips_ivf_search* never sizes; so the warm-up call that precedes a capture must be a mips_ivf_search_part of that shape itself. */
int mips_ivf_search_part(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, int64_t* out_packed, double* out_bias,
                         int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                         int grp_mode, void* hip_stream);

/* The merge of the gathered payloads, without an index handle: mips_merge_topk_sorted_packed over the `parts` lists of every query
 * (order: score descending, row ascending, padding last; equal entries by part), then, when bias != NULL, the finishing pass
 * S -> D = (float)((double)S + bias[j]) on every entry that names a row.  bias: float64 [nq], any part's out_bias (B_q depends on
 * the query and the shared range only).  All pointers are DEVICE memory; everything is enqueued on hip_stream, nothing synchronises.
 * MIPS_E_INVALID: parts < 1, nq < 0, k < 1, NULL gathered / out_scores / out_idx with nq > 0.  MIPS_E_UNSUPPORTED: k >
 * MIPS_MAX_K_WIDE, parts * k > 65536 (the entries per query the merge takes).  nq == 0: MIPS_OK, nothing written. */
int mips_ivf_merge_parts(const int64_t* gathered, int parts, int64_t nq, int k, const double* bias, float* out_scores, int64_t* out_idx,
                         int device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_IVF_SHARDED_H */
