/* mips_hip_ivf_range.h -- range search over the probed lists of an IVF index: every probed, admitted row above a per-query radius.
 *
 * The fixed-k searches of mips_hip_ivf.h answer "the best k"; this call answers "everything above a threshold" -- all memories with
 * similarity above t, duplicate clusters (a cluster of 65 copies overflows any k), counting neighbours to choose a radius -- at IVF
 * cost: it reads nprobe / nlist of the rows in ONE scan launch where mips_range_search on the flat index walks all of them chunk by
 * chunk.  Additive to mips_hip_ivf.h: same library, same conventions, no version of its own.
 *
 * Definition.  P(q_j), A_j (the rows whose list lies in P(q_j)) and "admitted" are those of mips_ivf_search_grp (mips_hip_ivf.h).
 * Row i is a HIT of query j iff all three hold:
 *   - i is in A_j;
 *   - i is admitted for j (sel_bits == NULL or bit sel_bit0 + i set; q_labels == NULL or the group rule holds);
 *   - the score the search would REPORT for (j, i) is strictly above radii[j], compared as float32.  BF16 and F32: the storage's
 *     canonical score.  SQ8: D(q, i) = (float)((double)S + B_q) of mips_hip_sq8.h -- D, not S: two rows with different S and equal D
 *     are both hits or both not.
 * Inner product only, as the index is.  Every probed row is scored exactly (the sequential fp64 sum) and the rule is applied to that
 * score, so nothing is approximated, no threshold is lowered and nothing is filtered afterwards.
 *
 * The result is CSR, as mips_range_search (mips_hip.h) defines it: out_lims int64 [nq + 1] with out_lims[0] = 0; the hits of query
 * j lie at [out_lims[j], out_lims[j + 1]) of out_scores (float32, the reported values) and out_idx (int64, row + idx_offset) IN
 * ASCENDING ROW ORDER.  The probed lists interleave in row number, so the call ends with a per-query ordering step; rows are distinct
 * within a query, so the order is total, and neither the order in which rows are scored nor the order in which atomics arrive shows
 * in the result.  out_lims always holds the TRUE counts: when out_lims[nq] > cap the call still returns MIPS_OK, out_scores /
 * out_idx [cap] are unspecified, nothing is written outside them, and the caller repeats with cap >= out_lims[nq].  cap = 0 with
 * NULL arrays is a counting call.
 * Hence: on a BF16 or F32 index with nprobe >= nlist the result is mips_range_search / _sel / _grp on mips_ivf_flat under the same
 * filter, bit for bit; mips_score_subset on mips_ivf_flat reproduces the scores; for a radius with fewer than k hits, the hits
 * re-sorted by (score descending, row ascending) are the entries of mips_ivf_search_wide with a score above the radius; and with
 * sel_bits == NULL and q_labels == NULL mips_ivf_range_search_grp IS mips_ivf_range_search (same launches, same bits).  A bitmap
 * alone is q_labels == NULL: there is no _sel entry.
 *
 * Arguments.  q [nq, d] MIPS_DTYPE_F32 or MIPS_DTYPE_BF16, host or device (MIPS_Q_DEVICE).  radii [nq] float32, HOST memory by
 * default: a NaN is MIPS_E_INVALID, +inf (no hit) and -inf (every probed admitted row with a score above -inf) are legal, and they
 * travel by the stream's asynchronous copy into the search's scratch.  With MIPS_RADII_DEVICE radii is DEVICE memory and nothing
 * of it is read on the host; a NaN radius there makes that query hit nothing.  The three outputs are all host or all device
 * (MIPS_OUT_DEVICE); host outputs synchronise, a device-in / device-out call never does.  sel_bits, sel_nbits, sel_bit0, q_labels,
 * grp_mode, MIPS_SEL_DEVICE and MIPS_GRP_DEVICE: as mips_ivf_search_grp.
 * MIPS_E_INVALID: what mips_ivf_search_grp refuses (an untrained index, a bad q_dtype, nprobe < 1, the bitmap bounds, a grp_mode
 * other than 0 / 1, a labelled prefix that is not ntotal), cap < 0, NULL out_lims, NULL radii with nq > 0, NULL arrays with
 * cap > 0, MIPS_OUT_PACKED.  MIPS_E_UNSUPPORTED: min(nprobe, nlist) > 1024.  nq == 0 and an empty index: all-zero out_lims.
 *
 * What a call enqueues is a fixed sequence per slice of 4096 queries -- the probe and the staging of mips_ivf_search, ONE range-scan
 * launch of nq * p * S workgroups (the list scan's decomposition; S from nq, p and the compute units), the prefix sum of the
 * per-query counts into out_lims, a pass that places the staged hits at out_lims[j] + a per-query cursor, and the ordering step,
 * one workgroup per query.  The capture contract of mips_ivf_search_grp holds in the same words: with device queries, radii,
 * outputs, bitmap and labels the call issues only stream operations, and no grid, pointer, size or loop bound depends on the VALUES
 * of the queries, the radii, the labels or the bitmap -- how many hits there are, where they land and how long a stretch is exist
 * on the device only.  Its scratch grows only when a call asks for a larger (nq, p, S, cap), so a captured call replays with other
 * queries, other radii and other filter contents of the same sizes; it stays valid until what ends a captured mips_ivf_search. */
#ifndef MIPS_HIP_IVF_RANGE_H
#define MIPS_HIP_IVF_RANGE_H

#include "mips_hip_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPS_RADII_DEVICE 256 /* radii is device memory (64 and 128 are taken by mips_hip_rows.h) */

int mips_ivf_range_search(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims,
                          float* out_scores, int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, void* hip_stream);
int mips_ivf_range_search_grp(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims,
                              float* out_scores, int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits,
                              int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPS_HIP_IVF_RANGE_H */
