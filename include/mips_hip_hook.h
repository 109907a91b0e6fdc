/* mips_hip_hook.h -- the device-resident scoring hook (mips_search_fused of mips_hip.h) under a per-query group filter.
 *
 * Conventions, constants (MIPS_GRP_EXCLUDE / MIPS_GRP_ONLY, MIPS_LABEL_NONE, MIPS_GRP_DEVICE), error codes and mips_last_error()
 * are those of mips_hip.h; the same libmips_hip.so exports everything and there is one ABI version, defined there.
 */
#ifndef MIPS_HIP_HOOK_H
#define MIPS_HIP_HOOK_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mips_search_fused with the group rule of mips_search_wide_grp: the arguments of mips_search_fused, then
 *   q_labels   int32 [nq], one label per query, tested against the row labels of mips_index_set_labels; host memory, or device
 *              memory with MIPS_GRP_DEVICE in flags (host labels travel by the stream's asynchronous copy and must stay valid
 *              until the call returns; device labels until the work enqueued by the call has run)
 *   grp_mode   MIPS_GRP_EXCLUDE: every row of the query's group stays out of its result (leak-free retrieval, hard negatives);
 *              MIPS_GRP_ONLY: the search runs inside the group.  A query labelled MIPS_LABEL_NONE is not filtered
 *   flags      MIPS_GRP_DEVICE or 0
 * The result for query j is what mips_search_fused returns for j on an index from which the rows not admitted for j were
 * deleted, row numbers, phi and maximal norm kept; short results are padded with (-inf | +inf, -1).  The single-id filter
 * ignore_device applies on top, after the group rule: k + 1 admitted hits are fetched, the banned one dropped, k kept.
 *
 * Where mips_search_fused is one launch (nq <= 16, bf16 or fp32-exact index of <= 65536 rows, k + 1 <= 6, row pitch a multiple
 * of 128 up to 1024) so is this call: the grouped instance of that kernel (mips_index_last_kernel:
 * "mips::hook_grouped_kernel<L2, F32>") tests the rule in its scan, and the stream-ordered exact pass behind it settles the
 * queries it flagged under the same rule.  Nothing synchronises; "margin_check" = 2 synchronises as it does for
 * mips_search_fused.  Everywhere else the call is the general form: query normalisation, mips_search_wide_grp with k (or k + 1)
 * and mips_filter_ignore.  Both forms are exact, hence bit-identical.
 *
 * q_labels == NULL IS mips_search_fused (grp_mode and flags are not looked at).  MIPS_E_INVALID: grp_mode other than 0 / 1, an
 * index whose labelled prefix is not exactly ntotal (mips_index_set_labels), normalize with queries that are not float32.
 * MIPS_E_UNSUPPORTED: k + (ignore_device ? 1 : 0) > MIPS_MAX_K and what mips_search_wide_grp refuses -- e4m3 storage, rows of
 * more than 1024 columns. */
int mips_search_fused_grp(mips_index_t* index, const void* q_device, int q_dtype, int64_t nq, int k, int normalize,
                          const int64_t* ignore_device, float* out_scores_device, int64_t* out_idx_device, int64_t idx_offset,
                          const int32_t* q_labels, int grp_mode, int flags, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_HOOK_H */
