// Merge of the range-search results of row shards (mips_range_merge_records, include/mips_hip_sharded.h).
//
// Every part arrives as ONE int64 record of W = (nq + 1) + stride + (stride + 1) / 2 words, the records end to end as an
// all-gather leaves them:
//
//   words [0, nq + 1)              lims of the part (true counts, as mips_range_search writes them)
//   words [nq + 1, nq + 1 + stride)  ids, already global
//   the rest                       stride float32 scores, padded to a whole word
//
// Within a query the hits of a part are in ascending row order and the parts are ascending row ranges, so the merged result
// is the parts' segments laid end to end per query: nothing is compared, the merge is two index computations and a copy.
//
//   range_merge_lims_kernel   one thread per j in [0, nq]: out_lims[j] = sum over the parts of lims_p[j] (prefix sums are linear,
//                             no scan), and for j < nq the first destination of every part's segment of query j,
//                             base[p][j] = out_lims[j] + sum over p' < p of (lims_p'[j + 1] - lims_p'[j]).
//   range_merge_copy_kernel   source-major: a wave takes 128 consecutive entries of one part's payload, whatever queries they belong
//                             to -- a query with 10^6 hits is copied by thousands of waves, 10^6 empty queries cost nothing.  The
//                             query of an entry e is j = upper_bound(lims_p, e) - 1; lanes 0 and 1 find it for the two ends of the
//                             wave's span over all nq + 1 words, every lane then searches between those two.  Reads are contiguous
//                             (8 B of scores and 16 B of ids per lane), writes contiguous within a query's segment.  An entry is
//                             stored iff its destination lies in [0, cap); nothing past min(lims_p[nq], stride) is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mips {

constexpr int RANGE_MERGE_THREADS = 256;
constexpr int RANGE_MERGE_SPAN = 128;        // entries of one wave step: two per lane
constexpr int RANGE_MERGE_MAX_BLOCKS = 2048; // per part: 8 workgroups on each of 256 CUs, the rest in grid strides

struct RangeMergeArgs {
    const int64_t* gathered; // [parts][W]
    int parts;
    int nq;
    int64_t stride;
    int64_t W;
    int64_t* out_lims;  // [nq + 1]
    float* out_s;       // [cap]
    int64_t* out_i;     // [cap]
    int64_t cap;
    int64_t* base;      // [parts][nq]
};

__global__ __launch_bounds__(RANGE_MERGE_THREADS) void range_merge_lims_kernel(RangeMergeArgs a) {
    const int64_t j = (int64_t)blockIdx.x * RANGE_MERGE_THREADS + threadIdx.x;
    if (j > a.nq) return;
    int64_t sum = 0;
    for (int p = 0; p < a.parts; ++p) sum += a.gathered[p * a.W + j];
    a.out_lims[j] = sum;
    if (j == a.nq) return;
    for (int p = 0; p < a.parts; ++p) {
        const int64_t* lims = a.gathered + p * a.W;
        a.base[(int64_t)p * a.nq + j] = sum;
        sum += lims[j + 1] - lims[j];
    }
}

// largest j in [lo, hi] with lims[j] <= e; lims[lo] <= e is the caller's
__device__ __forceinline__ int range_merge_owner(const int64_t* lims, int lo, int hi, int64_t e) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (lims[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(RANGE_MERGE_THREADS) void range_merge_copy_kernel(RangeMergeArgs a) {
    const int p = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t* lims = a.gathered + p * a.W;
    const int64_t* ids = lims + a.nq + 1;
    const float* scores = reinterpret_cast<const float*>(ids + a.stride); // 8-byte aligned: entry pairs load as one float2
    const int64_t* base = a.base + (int64_t)p * a.nq;
    int64_t n = lims[a.nq];                                               // a truncated part holds `stride` entries, not its total
    n = n < a.stride ? n : a.stride;
    const bool ids16 = (reinterpret_cast<uintptr_t>(ids) & 15) == 0;      // (the record's parity decides, uniformly)
    const bool out16 = (reinterpret_cast<uintptr_t>(a.out_i) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.out_s) & 7) == 0;
    const int64_t wave0 = (int64_t)blockIdx.x * (RANGE_MERGE_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * (RANGE_MERGE_THREADS / 64) * RANGE_MERGE_SPAN;
    for (int64_t e0 = wave0 * RANGE_MERGE_SPAN; e0 < n; e0 += step) {
        const int64_t last = (e0 + RANGE_MERGE_SPAN < n ? e0 + RANGE_MERGE_SPAN : n) - 1;
        // the span's ends: the full search once per wave (lims[0] = 0 <= e < lims[nq], so the owner lies in [0, nq - 1])
        const int end = range_merge_owner(lims, 0, a.nq - 1, (lane & 1) ? last : e0);
        const int jlo = __shfl(end, 0), jhi = __shfl(end, 1);
        const int64_t e = e0 + 2 * lane;
        if (e > last) continue;
        const bool two = e < last;
        const int j0 = range_merge_owner(lims, jlo, jhi, e);
        const int64_t l0 = lims[j0];
        int j1 = j0;
        int64_t l1 = l0;
        if (two && j0 < jhi && lims[j0 + 1] <= e + 1) {
            j1 = range_merge_owner(lims, j0 + 1, jhi, e + 1);
            l1 = lims[j1];
        }
        float s0, s1 = 0.f;
        int64_t i0, i1 = 0;
        if (two) {
            const float2 sv = *reinterpret_cast<const float2*>(scores + e);
            s0 = sv.x;
            s1 = sv.y;
            if (ids16) {
                const longlong2 iv = *reinterpret_cast<const longlong2*>(ids + e);
                i0 = iv.x;
                i1 = iv.y;
            } else {
                i0 = ids[e];
                i1 = ids[e + 1];
            }
        } else {
            s0 = scores[e];
            i0 = ids[e];
        }
        const int64_t d0 = base[j0] + (e - l0);
        const int64_t d1 = base[j1] + (e + 1 - l1);
        const bool ok0 = (uint64_t)d0 < (uint64_t)a.cap;
        const bool ok1 = two && (uint64_t)d1 < (uint64_t)a.cap;
        if (ok0 && ok1 && out16 && d1 == d0 + 1 && (d0 & 1) == 0) {
            *reinterpret_cast<float2*>(a.out_s + d0) = make_float2(s0, s1);
            longlong2 iv;
            iv.x = i0;
            iv.y = i1;
            *reinterpret_cast<longlong2*>(a.out_i + d0) = iv;
        } else {
            if (ok0) {
                a.out_s[d0] = s0;
                a.out_i[d0] = i0;
            }
            if (ok1) {
                a.out_s[d1] = s1;
                a.out_i[d1] = i1;
            }
        }
    }
}

} // namespace mips
