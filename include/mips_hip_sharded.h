/* mips_hip_sharded.h -- helpers of the shard exchange that take no index handle.
 *
 * A row-sharded index (ShardedMipsIndex) searches every shard with the entry points of mips_hip.h and
 * brings the shards' results together with ONE collective followed by a replicated merge.  For the top-k searches the merges
 * are mips_merge_topk* in mips_hip.h.  This header holds what a result of VARIABLE size -- the CSR triple of the range search --
 * needs: the layout of the record a shard sends, and the merge of the gathered records.  Conventions, error codes and
 * mips_last_error() are those of mips_hip.h; the same libmips_hip.so exports everything.
 */
#ifndef MIPS_HIP_SHARDED_H
#define MIPS_HIP_SHARDED_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The part record: a shard's range-search result for nq queries with room for `stride` hits, as ONE contiguous int64 buffer
 *     words [0, nq + 1)                out_lims of mips_range_search* (int64; the true counts, whatever `stride` is)
 *     words [nq + 1, nq + 1 + stride)  out_idx (int64; called with idx_offset = the shard's first global row)
 *     the rest                         out_scores: `stride` float32, padded to a whole word
 * The three regions are what mips_range_search* takes as out_lims, out_idx and out_scores with cap = stride and MIPS_OUT_DEVICE:
 * a shard searches straight into its record and no pack step exists.  Records of one (nq, stride) have one size, so an
 * all-gather of them is the merge's input as it arrives. */
#define MIPS_RANGE_RECORD_WORDS(nq, stride) ((int64_t)(nq) + 1 + (int64_t)(stride) + ((int64_t)(stride) + 1) / 2)

/* Merge of `parts` gathered records (gathered[p] at word p * MIPS_RANGE_RECORD_WORDS(nq, stride)) into one CSR result.  Part p
 * must hold lower global rows than part p + 1 and list every query's hits in ascending row order (what mips_range_search*
 * writes): the merged hits of query j are then the parts' segments of j laid end to end, in ascending row order again.
 *     out_lims [nq + 1]   always the true global counts, out_lims[j] = sum over the parts of lims_p[j]
 *     out_scores, out_idx [cap]   the merged hits; when out_lims[nq] > cap their contents are unspecified and nothing at or past
 *                         `cap` is written (the caller repeats with larger arrays); cap = 0 with NULL arrays is a counting call
 *     workspace           parts * nq int64 words (may be NULL when nq == 0)
 * A part whose own total lims_p[nq] exceeds `stride` is a truncated part: nothing past its `stride` entries is read, the merged
 * scores and ids are then unspecified, the counts stay true and the call returns MIPS_OK.
 * All pointers are DEVICE memory; everything is enqueued on hip_stream and nothing synchronises.  nq == 0 writes out_lims[0] = 0.
 * MIPS_E_INVALID: parts < 1, negative nq, stride or cap, NULL gathered or out_lims, NULL outputs with cap > 0, NULL workspace
 * with nq > 0.  MIPS_E_UNSUPPORTED: nq > 2^24, parts > 65535.  Nothing in the reference corresponds (it replicates its index). */
int mips_range_merge_records(const int64_t* gathered, int parts, int64_t nq, int64_t stride, int64_t* out_lims, float* out_scores,
                             int64_t* out_idx, int64_t cap, int64_t* workspace, int device, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_SHARDED_H */
