// Payload arithmetic of the row-sharded IVF search (include/mips_hip_ivf_sharded.h), one text for the kernel, the host entry points
// and a stand-alone check (tests/ivf_sharded_math_check.cpp includes this file and nothing else of the library).
//   payload    a part's result for nq queries is int64 [nq][k][2]: word 0 of an entry holds the float32 bits of the score in the
//              RANKING domain (an SQ8 part: S, never D), zero-extended -- mips_merge_topk_sorted_packed reads the low 32 bits, so a
//              negative score must not smear its sign over the word --; word 1 the global row, the part's row + idx_offset.  A
//              negative row (-1: padding) stays as it is: the merge ranks every id < 0 behind every row at an equal score.
//   merge      `parts` sorted lists of k entries per query; the merge takes parts * k <= kPartsMergeLimit entries per query.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFS_HD __host__ __device__ __forceinline__
#else
#define IVFS_HD inline
#endif

namespace ivf {

constexpr int64_t kPartsMergeLimit = 65536; // entries per query mips_merge_topk_sorted_packed takes (kMergeLimit of ivf_search_math.hpp)
constexpr int kPartsMaxK = 1024;            // MIPS_MAX_K_WIDE

// word 0 of an entry from the score's bits, and back
IVFS_HD int64_t packed_score_word(uint32_t score_bits) { return (int64_t)score_bits; }
IVFS_HD uint32_t packed_score_bits(int64_t word) { return (uint32_t)word; }

// word 1 of an entry: the global row of a part's row; padding (any negative id) passes through
IVFS_HD int64_t packed_row_word(int64_t row, int64_t idx_offset) { return row < 0 ? row : row + idx_offset; }

// first word of entry t of query j in a payload of k entries per query
IVFS_HD int64_t packed_entry(int64_t j, int k, int t) { return (j * (int64_t)k + t) * 2; }

// words of a payload
IVFS_HD int64_t packed_words(int64_t nq, int k) { return nq * (int64_t)k * 2; }

// whether `parts` lists of k entries fit one merge (parts >= 1, 1 <= k <= kPartsMaxK; no overflow for any int parts)
IVFS_HD bool parts_fit_merge(int parts, int k) { return (int64_t)parts * (int64_t)k <= kPartsMergeLimit; }

} // namespace ivf
