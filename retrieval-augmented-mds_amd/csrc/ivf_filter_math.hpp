// The element-wise rule of the filtered IVF search (include/mips_hip_ivf.h: mips_ivf_search_sel / _grp) and the bookkeeping of the
// list scan's compacting queue, one text for the kernel and a stand-alone check (tests/ivf_filter_math_check.cpp includes this file
// and nothing else of the library).
//   admission  row i answers query j iff its bit is set (when a bitmap is given) and the group rule holds (when query labels are
//              given): the query carries MIPS_LABEL_NONE, or label[i] != q_label under exclude, or label[i] == q_label under only
//   queue      a wave collects the admitted row numbers of successive 64-position windows of its list segment in a queue of
//              kQueueSlots = 128 entries: a window appends its admitted rows in lane order (ballot + prefix popcount) behind the
//              `queued` entries already there, a scoring pass takes the first 64 when at least 64 are queued, and the remainder
//              moves to the front.  Between windows 0 <= queued < 64, so an append never writes past slot 126.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFF_HD __host__ __device__ __forceinline__
#else
#define IVFF_HD inline
#endif

namespace ivf {

constexpr int32_t kLabelNone = INT32_MIN; // MIPS_LABEL_NONE
constexpr int kGrpExclude = 0, kGrpOnly = 1; // MIPS_GRP_EXCLUDE, MIPS_GRP_ONLY
constexpr int kQueuePass = 64;            // rows one scoring pass takes (a wave)
constexpr int kQueueSlots = 128;          // slots of a wave's queue

// the group rule for one (row label, query label) pair
IVFF_HD bool group_admits(int32_t label, int32_t q_label, int mode) {
    if (q_label == kLabelNone) return true;
    return mode == kGrpOnly ? label == q_label : label != q_label;
}

// bit `bit` (>= 0) of a bitmap stored least significant bit first
IVFF_HD bool bit_is_set(const uint8_t* bits, int64_t bit) { return ((bits[bit >> 3] >> (bit & 7)) & 1u) != 0; }

// slot of lane `lane`'s row when the lanes of `mask` append behind `queued` entries (lane order is kept)
IVFF_HD int queue_slot(int queued, uint64_t mask, int lane) { return queued + __builtin_popcountll(mask & (((uint64_t)1 << lane) - 1)); }

IVFF_HD int queue_after_append(int queued, uint64_t mask) { return queued + __builtin_popcountll(mask); }

IVFF_HD bool queue_has_pass(int queued) { return queued >= kQueuePass; }

// entries left once a pass took the first kQueuePass; they move from slot kQueuePass + u to slot u
IVFF_HD int queue_after_pass(int queued) { return queued - kQueuePass; }

} // namespace ivf
