/* mips_hip_write.h -- overwrite stored rows in place, by id: the missing quarter of append / remove / read / WRITE.
 *
 * mips_hip.h appends and resets, mips_hip_update.h removes, mips_hip_rows.h reads rows back by id; this header gives rows a new
 * value.  A model that trains its retrieval encoder re-encodes a few dozen rows per step and writes them back: row numbers,
 * labels and the list layout of every other row stay, and the call costs what the written rows cost.  (The reference rebuilds its
 * whole index every mips_rebuild_every steps; faiss has the call for its IVF index, IndexIVF::update_vectors.)
 * Conventions, error codes and mips_last_error() are those of mips_hip.h; the same libmips_hip.so exports everything and there is
 * one ABI version, defined there.  The two calls live in a header of their own because the sets of functions that
 * mips_hip_update.h and mips_hip_ivf.h declare are fixed.
 *
 * Semantics.  update(ids[n], x[n, d], idx_offset) is the sequential loop
 *     for p = 0 .. n - 1:  local = ids[p] - idx_offset;  if 0 <= local < ntotal (as int64, the rule of mips_hip_rows.h):  row[local] = x[p]
 * where x[p] is converted exactly as mips_index_add converts a row of src_dtype into the index's storage.  Every other id names
 * no row and is skipped: negative ids (the -1 padding of a search), ids of another shard, ids past the index.  Of several positions
 * that name one row the HIGHEST wins -- what the loop leaves behind.  ntotal, row numbers, labels and capacity do not change.
 * THE CONTRACT: afterwards the index cannot be told from a fresh index of the same type that was given the final rows in order --
 * stored bytes (mips_index_read_rows, mips_index_reconstruct) and the (scores, ids) of every search path match bit for bit.  No
 * byte of another row changes, padding columns included, and nothing past ntotal.
 */
#ifndef MIPS_HIP_WRITE_H
#define MIPS_HIP_WRITE_H

#include "mips_hip.h"
#include "mips_hip_ivf.h"
#include "mips_hip_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ids [n] int64, host or device (MIPS_IDS_DEVICE); rows [n, d] of src_dtype, host or device (MIPS_Q_DEVICE, as mips_ivf_train
 * uses it); out_updated: NULL, or one int64 in host or device memory (MIPS_OUT_DEVICE) that receives the number of DISTINCT local
 * rows written.  src_dtype: whatever mips_index_add accepts for this storage -- MIPS_DTYPE_F32 / MIPS_DTYPE_BF16, raw
 * MIPS_DTYPE_FP8_E4M3 bytes on the e4m3 storages, raw MIPS_DTYPE_SQ8 codes on an SQ8 index.  Every storage and every d that
 * mips_index_add accepts is served: the call works on storage, not on a search path.
 *
 * What a call enqueues: three launches over the n positions ("Updating rows") -- A: owner[row] = max(owner[row], p)
 * for every position that names a row (an integer atomic maximum: order-free, deterministic); B: the wave of each row's owner
 * converts x[p] and stores it over the row (an fp32-exact index: its two bf16 planes, the fp32 original and, where the bf16 image
 * of the two-stage search exists, the image); C: the owners fold their stored row into the row-norm bounds, count themselves and
 * put the touched owners back to -1.  O(n), never O(ntotal).  owner is one int32 per row of capacity; it is allocated by the first
 * call and again by the first call after the index has grown.
 *
 * Synchronisation and capture.  Ordering is that of every call on the index: behind the calls before it on any stream, and a
 * search enqueued behind it sees the new rows.  With device ids, device rows and a device or NULL count the call NEVER
 * synchronises on an inner-product index, and no grid, pointer, size or loop bound depends on the VALUES of the ids.  Behind one
 * warm-up call (which allocates owner) it may be captured into a HIP graph and replayed with other ids and other rows in the same
 * buffers; the graph stays valid until the index grows (mips_index_add, _reserve), or until a search has extended the bf16 image
 * of an fp32-exact index over rows added since the capture.  Host ids, host rows or a host count synchronise hip_stream once.
 *
 * Cached scalars.  The row-norm maxima the margin checks use stay valid as UPPER bounds (the written rows are folded in; a row
 * that shrank leaves the bound where it was -- too large only flags more queries, and every path settles those exactly).  phi is
 * part of the reported L2 distances and is recomputed from the stored rows by the next call that needs it (that call
 * synchronises), unless it was set by mips_index_set_phi: an override stays until the caller renews it, as after mips_index_remove.
 * Labels are untouched.
 *
 * MIPS_E_INVALID: NULL index, n < 0, NULL ids or rows with n > 0, a src_dtype mips_index_add refuses for this storage, an
 * untrained SQ8 index.  NaN and infinities in rows are stored as mips_index_add stores them (no check, as there).
 * MIPS_E_UNSUPPORTED: n > 2^31 - 1.  n == 0: MIPS_OK, nothing is touched, every cached scalar stays, the count is 0.
 *
 * On mips_ivf_flat(ivf) the call is allowed: the row changes and its list does not, so the IVF searches stay exact on what they
 * read but the row is found through the list of its OLD value.  mips_ivf_update moves it. */
int mips_index_update(mips_index_t* index, const int64_t* ids, int64_t n, int64_t idx_offset, const void* rows, int src_dtype, int flags,
                      int64_t* out_updated, void* hip_stream);

/* mips_index_update on the inner flat index, and every written row gets the assignment mips_ivf_add would give it: the nearest
 * list of the float32 INPUT by the coarse index's certified search; of several positions that name one row the highest decides
 * the list as it decides the row.  The list table is rebuilt.  Afterwards the index equals a fresh IVF index with the same
 * centroids that was given the final rows: assignments, list sizes and every search, bit for bit.
 * Arguments as mips_index_update; src_dtype MIPS_DTYPE_F32 or MIPS_DTYPE_BF16 -- raw codes are MIPS_E_UNSUPPORTED, as in
 * mips_ivf_add.  MIPS_E_INVALID also on an untrained index.  The call may synchronise where mips_ivf_add does, and it ends the
 * validity of captured IVF searches as mips_ivf_add does (mips_hip_ivf.h). */
int mips_ivf_update(mips_ivf_t* ivf, const int64_t* ids, int64_t n, int64_t idx_offset, const void* rows, int src_dtype, int flags,
                    int64_t* out_updated, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_WRITE_H */
