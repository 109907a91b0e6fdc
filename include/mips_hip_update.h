/* mips_hip_update.h -- entry points that change the rows an index already holds.
 *
 * mips_hip.h appends (mips_index_add*) and forgets everything (mips_index_reset); this header takes single rows out, and
 * mips_hip_write.h gives stored rows a new value in place (mips_index_update, mips_ivf_update: row numbers and labels stay).
 * Conventions, error codes and mips_last_error() are those of mips_hip.h; the same libmips_hip.so exports everything and
 * there is one ABI version, defined there.
 */
#ifndef MIPS_HIP_UPDATE_H
#define MIPS_HIP_UPDATE_H

#include "mips_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Removes the local rows whose bit is set and closes the gaps: the surviving rows keep their order and are renumbered
 * 0 .. ntotal' - 1 (faiss IndexFlat::remove_ids).  Bitmap, sel_nbits, sel_bit0, MIPS_SEL_DEVICE: as in the _sel searches
 * (bit sel_bit0 + i speaks about LOCAL row i).  out_counts[0] = rows removed, out_counts[1] = labelled rows left.
 *
 * Every storage and every d the index accepts is served (the call works on storage, not on a search path).  The rows are
 * compacted IN PLACE, window by window ("Removing rows"): no second copy of the index exists at any time; the
 * scratch is one window of rows, allocated for the call and released after it.
 *
 * Ordering: as every call on the index, behind the calls before it on any stream.  THE CALL SYNCHRONISES hip_stream ONCE:
 * ntotal lives on the host, so the number of surviving rows (one count per window) is read back before the rows move.  The
 * moves themselves are enqueued; a search enqueued behind the call sees the new index.
 *
 * Nothing is removed (out_counts[0] = 0): nothing is touched and every cached scalar (phi, the row-norm maxima) stays valid.
 * Otherwise ntotal drops; the labels of the labelled prefix are compacted with their rows and the labelled prefix becomes the
 * surviving rows that carried a label; phi is recomputed from the surviving rows by the next call that needs it, unless it was
 * set by mips_index_set_phi (an override stays until the caller renews it, as after mips_index_add).  Storage past the new
 * ntotal keeps old bytes, as after mips_index_reset; mips_index_add appends at the new end.
 *
 * MIPS_E_INVALID: NULL index or out_counts, sel_bit0 < 0, sel_bit0 + ntotal > sel_nbits, a NULL bitmap while ntotal > 0.
 * "remove_window_rows" (mips_index_set_param; a multiple of 128, 0 = automatic) sets the window: a test knob, the result does
 * not depend on it.  Nothing in the reference corresponds (it rebuilds its index). */
int mips_index_remove(mips_index_t* index, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, int flags,
                      int64_t out_counts[2], void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MIPS_HIP_UPDATE_H */
