/* mips_hip_sq8.h -- the trained 8-bit scalar quantiser of an index created with MIPS_DTYPE_SQ8 (faiss "SQ8":
 * ScalarQuantizer QT_8bit, range statistic min/max with argument 0).
 *
 * Conventions, error codes and the error text are those of mips_hip.h; the same libmips_hip.so exports everything and there
 * is one ABI version, defined there.
 *
 * Storage    one byte per element.  Parameters per column j: vmin_j and vdiff_j = max_j - vmin_j of the training rows.
 *            All of the following is IEEE float32, one rounding per operation, no fused multiply-add:
 *   encode   t = vdiff_j != 0 ? (x - vmin_j) / vdiff_j : 0;  t = fminf(fmaxf(t, 0), 1);  code = (uint8_t)(int)(255 * t)
 *            (the cast truncates; NaN encodes as 0, +inf as 255, -inf as 0; values outside the trained range clamp)
 *   decode   vmin_j + ((code + 0.5f) / 255.0f) * vdiff_j            -- what mips_index_reconstruct returns as float32
 * Scores     s_j = vdiff_j / 255, o_j = vmin_j + 0.5f * s_j, q'_j = bf16(q_j * s_j) (bf16 queries are widened first).
 *            Rows are RANKED by S(q, i) = (float) of the sequential fp64 sum over ascending j of q'_j * code_ij, ties to the
 *            lowest row; the score REPORTED is D(q, i) = (float)((double)S(q, i) + B_q), B_q = the sequential fp64 sum of
 *            (double)q_j * (double)o_j: the inner product of the query with the decoded row up to the bf16 rounding of q'.
 *            D is monotone in S, so the rows come out in non-increasing D.  -1 padding keeps -inf, poisoned outputs NaN.
 * Served     mips_index_add (after training; float32 / bf16 rows, or raw codes as MIPS_DTYPE_SQ8), mips_search (k <=
 *            MIPS_MAX_K, with MIPS_OUT_PACKED too), mips_search_split, mips_score_subset (scores D: scoring a search's I gives
 *            its D bit for bit), mips_index_reconstruct (float32: decoded; MIPS_DTYPE_SQ8: the codes; "no row": NaN / code 0), mips_index_remove,
 *            labels, reserve, growth, reset (the parameters stay).  Before training: mips_index_add and mips_score_subset return
 *            MIPS_E_INVALID; mips_search answers as an empty index does (-1 / -inf), reconstruct finds no row.
 * Not served mips_search_wide*, mips_range_search*, mips_search_fused_grp and the sel / grp forms: MIPS_E_UNSUPPORTED, as for
 *            the e4m3 storages.  MIPS_METRIC_L2: refused by mips_index_create.  d <= 1024. */
#ifndef MIPS_HIP_SQ8_H
#define MIPS_HIP_SQ8_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Train on x [n, d] (MIPS_DTYPE_F32 or MIPS_DTYPE_BF16; flags: MIPS_Q_DEVICE = x is device memory): vmin_j = min_i x_ij,
 * vdiff_j = max_i x_ij - vmin_j, computed on the device (deterministic: min and max do not depend on the order).  Synchronises
 * hip_stream.  MIPS_E_INVALID: n <= 0, a NaN or infinity in x (the parameters then stay as they were), an index that is not
 * SQ8, an index that already holds rows (training again replaces the parameters only while the index is empty). */
int mips_index_sq8_train(mips_index_t* index, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream);

/* The parameters as HOST float32 arrays of d.  set: the index becomes trained (MIPS_E_INVALID: a non-finite value, vdiff_j < 0,
 * an index that holds rows); get: MIPS_E_INVALID on an untrained index. */
int mips_index_sq8_set_params(mips_index_t* index, const float* vmin, const float* vdiff);
int mips_index_sq8_get_params(mips_index_t* index, float* vmin, float* vdiff);

/* 1 / 0; -1: NULL or not an SQ8 index */
int mips_index_sq8_is_trained(const mips_index_t* index);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_SQ8_H */
