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
 * NOT IN THIS HEADER YET: the search over the probed lists (the flat index's mips_search restricted to the rows whose assignment
 * lies in P(q)).  What is here builds and maintains everything that search reads; until it exists, the rows are searched exactly
 * through mips_ivf_flat.
 * Refused: MIPS_METRIC_L2 (the index ranks by inner product), d > 1024, the e4m3 storages, nlist outside 1 .. 65536, p > 1024.
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
 * certified).  Synchronises. */
int mips_ivf_probe(mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int32_t* out_lists, int flags, void* hip_stream);

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
