// Kernels of the range search over the probed lists (include/mips_hip_ivf_range.h: mips_ivf_range_search / _grp).
//
//   ivf_range_scan_kernel   grid = nq * p * S workgroups of IVF_SCAN_WAVES waves; workgroup (j, t, s) is that of ivf_list_scan_kernel
//                           (ivf_search_kernels.hpp), text for text: the list number, the list's bounds and every row number are
//                           read and range-checked here, the canonical score is ivf_gathered_dot, and the FILT instance admits a
//                           row where its number is read and compacts the admitted rows through the per-wave queue.  What differs
//                           is what happens to a score: the REPORTED value (the canonical score; SQ8: D = (float)((double)S + B_q),
//                           ivf_finish_kernel's arithmetic) is compared with the query's radius, strictly, as float32.  The hits of
//                           a pass are appended to the staging buffer: a ballot, a prefix popcount, and lane 0 reserves the block
//                           with ONE atomic add on the cursor and advances the query's count with another.  Records past the
//                           capacity are dropped; cursor and counts go on, so the counts are true whatever the capacity.  No
//                           __syncthreads() in the loop, no workgroup waits for another.  A NaN radius compares false: no hit.
//   (mips::range_lims_kernel of range_kernels.hpp, as it is: the slice's counts -> out_lims, carried over slices in a device word)
//   ivf_range_place_kernel  the staged records of the slice, scattered to lims[j] + (a per-query cursor) of the caller's arrays.
//   ivf_range_order_kernel  one workgroup per query: the stretch [lims[j], min(lims[j + 1], cap)) into ascending row order by the
//                           sorting network of ivf_range_math.hpp -- in LDS up to kRangeSortLds entries, in global memory beyond --
//                           then idx_offset on the rows.  Rows are distinct within a query, so the order is total and neither the
//                           order in which rows were scored nor the order in which the atomics arrived shows in the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_range_math.hpp"
#include "ivf_search_kernels.hpp"

namespace mips {

constexpr int IVF_RANGE_THREADS = 256; // of the place and order kernels

struct IvfRangeArgs {
    IvfScanArgs a;               // the list scan's arguments (k and parts are not looked at)
    const float* radii;          // [nq] of the slice
    const double* bias;          // [nq] B_q of an SQ8 index, else nullptr
    unsigned long long* cursor;  // staging records reserved so far (this slice)
    int* qcnt;                   // [nq] hits of every query, zeroed per slice
    int64_t cap;                 // records the staging buffer holds
    int* stage_q;                // [cap] query of the slice
    int* stage_r;                // [cap] row
    float* stage_s;              // [cap] reported score
};

// One pass: lane `lane` scores row `id` (id < 0: none); the hits of the wave go to the staging buffer in lane order.
template <typename EL>
__device__ __forceinline__ void ivf_score_stage(const typename EL::type* rows, int ld, int id, int lane, u32x4* tile, const double* yd, const IvfRangeArgs& g,
                                                int j, float radius, bool sq8, double bq) {
    const float key = (float)ivf_gathered_dot<EL>(rows, ld, id, lane, tile, yd);
    float rep = key;
    if (sq8 && fabsf(key) < INFINITY) rep = (float)((double)key + bq);
    const bool hit = id >= 0 && rep > radius; // strict, on the float32 value
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) return; // (uniform over the wave)
    unsigned lo = 0u, hi = 0u;
    if (lane == 0) {
        const int n = __popcll(m);
        const unsigned long long base = atomicAdd(g.cursor, (unsigned long long)n);
        atomicAdd(g.qcnt + j, n);
        lo = (unsigned)base;
        hi = (unsigned)(base >> 32);
    }
    lo = __shfl(lo, 0);
    hi = __shfl(hi, 0);
    const unsigned long long slot = ivf::range_slot(((unsigned long long)hi << 32) | lo, m, lane);
    if (hit && ivf::range_keeps(slot, g.cap)) {
        g.stage_q[slot] = j;
        g.stage_r[slot] = id;
        g.stage_s[slot] = rep;
    }
}

// EL: element type of the rows; ELQ: of the staged queries (bf16 for SQ8 codes); FILT: the filtered instance
template <typename EL, typename ELQ, bool FILT>
__global__ __launch_bounds__(64 * IVF_SCAN_WAVES) void ivf_range_scan_kernel(IvfRangeArgs g) {
    __shared__ __attribute__((aligned(16))) double yd[IVF_SCAN_MAX_LD];
    __shared__ __attribute__((aligned(16))) u32x4 tiles[IVF_SCAN_WAVES * 64 * (IVF_SCAN_TCH + 1)];
    __shared__ int fq[FILT ? IVF_SCAN_WAVES * ivf::kQueueSlots : 1]; // the waves' queues of admitted row numbers
    const IvfScanArgs& a = g.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int s = (int)(b % a.S);
    const int t = (int)((b / a.S) % a.p);
    const int64_t j = b / ((int64_t)a.S * a.p);
    if (j >= a.nq) return;
    // the list and its bounds: read here, checked here
    const int64_t l = a.probe[j * a.p + t];
    int64_t beg = 0, L = 0;
    if (l >= 0 && l < a.nlist) {
        const int64_t o0 = a.offsets[l], o1 = a.offsets[l + 1];
        if (o0 >= 0 && o0 <= o1 && o1 <= a.ntotal) {
            beg = o0;
            L = o1 - o0;
        }
    }
    const int64_t lo = beg + ivf::seg_bound(L, s, a.S), hi = beg + ivf::seg_bound(L, s + 1, a.S);
    if (lo >= hi) return; // (uniform over the workgroup)

    constexpr int PERQ = ELQ::PER16;
    const typename ELQ::type* ys = reinterpret_cast<const typename ELQ::type*>(a.y) + (size_t)j * a.ld;
    for (int c = tid; c < a.ld / PERQ; c += 64 * IVF_SCAN_WAVES) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ys + (size_t)c * PERQ);
#pragma unroll
        for (int e = 0; e < PERQ; ++e) yd[c * PERQ + e] = (double)ELQ::get(v, e);
    }
    __syncthreads();
    const typename EL::type* rows = reinterpret_cast<const typename EL::type*>(a.rows);
    u32x4* tile = tiles + wave * 64 * (IVF_SCAN_TCH + 1);
    int* queue = fq + (FILT ? wave * ivf::kQueueSlots : 0);
    int queued = 0; // entries of the wave's queue, < 64 between windows
    const int qlab = FILT && a.q_labels != nullptr ? a.q_labels[j] : ivf::kLabelNone;
    const float radius = g.radii[j];
    const bool sq8 = g.bias != nullptr;
    const double bq = sq8 ? g.bias[j] : 0.0;
    for (int64_t r0 = lo + (int64_t)wave * 64; r0 < hi; r0 += 64 * IVF_SCAN_WAVES) {
        const int64_t pos = r0 + lane;
        int id = -1;
        if (pos < hi) {
            const int r = a.list_rows[pos];
            if (r >= 0 && r < a.ntotal) id = r;
        }
        if constexpr (FILT) {
            // admission where the row number is read: bit and label of an in-range row only, then the queue
            if (id >= 0) {
                bool ok = a.sel_bits == nullptr || ivf::bit_is_set(a.sel_bits, a.sel_bit0 + id);
                if (ok && a.q_labels != nullptr) ok = ivf::group_admits(a.row_labels[id], qlab, a.grp_mode);
                if (!ok) id = -1;
            }
            const unsigned long long adm = __ballot(id >= 0);
            if (id >= 0) queue[ivf::queue_slot(queued, adm, lane)] = id;
            queued = ivf::queue_after_append(queued, adm);
            __builtin_amdgcn_wave_barrier(); // (one wave: LDS operations complete in order)
            if (!ivf::queue_has_pass(queued)) continue; // (uniform over the wave)
            id = queue[lane];
            queued = ivf::queue_after_pass(queued);
            const int next = lane < queued ? queue[ivf::kQueuePass + lane] : -1;
            __builtin_amdgcn_wave_barrier();
            if (lane < queued) queue[lane] = next;
            __builtin_amdgcn_wave_barrier();
        }
        ivf_score_stage<EL>(rows, a.ld, id, lane, tile, yd, g, (int)j, radius, sq8, bq);
    }
    if constexpr (FILT) {
        if (queued > 0) ivf_score_stage<EL>(rows, a.ld, lane < queued ? queue[lane] : -1, lane, tile, yd, g, (int)j, radius, sq8, bq); // the remainder
    }
}

struct IvfRangePlaceArgs {
    const unsigned long long* cursor; // records the scan reserved (this slice)
    int64_t cap;                      // of the staging buffer and of the caller's arrays
    const int* stage_q;
    const int* stage_r;
    const float* stage_s;
    int* qcur;                        // [ns] records placed so far, zeroed per slice
    int ns;
    int64_t s0;
    const int64_t* lims;              // [nq + 1]
    float* out_s;                     // [cap]
    int64_t* out_i;                   // [cap] rows, without idx_offset
};

__global__ __launch_bounds__(IVF_RANGE_THREADS) void ivf_range_place_kernel(IvfRangePlaceArgs a) {
    const uint64_t staged = ivf::range_staged(*a.cursor, a.cap);
    for (uint64_t e = blockIdx.x * (uint64_t)IVF_RANGE_THREADS + threadIdx.x; e < staged; e += (uint64_t)gridDim.x * IVF_RANGE_THREADS) {
        const int j = a.stage_q[e];
        if (j < 0 || j >= a.ns) continue; // (the scan writes queries of the slice only)
        const int c = atomicAdd(a.qcur + j, 1);
        const int64_t dst = ivf::range_place_slot(a.lims[a.s0 + j], c, a.cap);
        if (dst >= 0) {
            a.out_s[dst] = a.stage_s[e];
            a.out_i[dst] = (int64_t)a.stage_r[e];
        }
    }
}

struct IvfRangeOrderArgs {
    const int64_t* lims; // [nq + 1]
    int ns;
    int64_t s0;
    int64_t cap;
    float* out_s;        // [cap]
    int64_t* out_i;      // [cap]
    int64_t idx_offset;
};

__global__ __launch_bounds__(IVF_RANGE_THREADS) void ivf_range_order_kernel(IvfRangeOrderArgs a) {
    __shared__ int sr[ivf::kRangeSortLds];
    __shared__ float sv[ivf::kRangeSortLds];
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x;
    if (j >= a.ns) return;
    const int64_t lim0 = a.lims[a.s0 + j];
    const int64_t n = ivf::range_stretch(lim0, a.lims[a.s0 + j + 1], a.cap);
    if (n <= 0 || lim0 < 0) return; // (uniform over the workgroup)
    float* S = a.out_s + lim0;
    int64_t* I = a.out_i + lim0;
    const int64_t P = ivf::range_sort_class(n);
    if (ivf::range_sort_in_lds(n)) {
        const int m = (int)n;
        for (int i = tid; i < m; i += IVF_RANGE_THREADS) {
            sr[i] = (int)I[i];
            sv[i] = S[i];
        }
        __syncthreads();
        for (int k = 2; k <= (int)P; k <<= 1)
            for (int jj = k >> 1; jj >= 1; jj >>= 1) {
                for (int t = tid; t < (int)(P >> 1); t += IVF_RANGE_THREADS) {
                    const int i = (int)ivf::bitonic_lower(t, jj), u = (int)ivf::bitonic_partner(i, k, jj);
                    if (u < m && sr[u] < sr[i]) {
                        const int r = sr[i];
                        const float v = sv[i];
                        sr[i] = sr[u];
                        sv[i] = sv[u];
                        sr[u] = r;
                        sv[u] = v;
                    }
                }
                __syncthreads();
            }
        for (int i = tid; i < m; i += IVF_RANGE_THREADS) {
            I[i] = (int64_t)sr[i] + a.idx_offset;
            S[i] = sv[i];
        }
        return;
    }
    // the long stretch: the same network on the caller's arrays (slow, reached by radii that admit a large part of the index)
    __syncthreads();
    for (int64_t k = 2; k <= P; k <<= 1)
        for (int64_t jj = k >> 1; jj >= 1; jj >>= 1) {
            for (int64_t t = tid; t < (P >> 1); t += IVF_RANGE_THREADS) {
                const int64_t i = ivf::bitonic_lower(t, jj), u = ivf::bitonic_partner(i, k, jj);
                if (u < n && I[u] < I[i]) {
                    const int64_t r = I[i];
                    const float v = S[i];
                    I[i] = I[u];
                    S[i] = S[u];
                    I[u] = r;
                    S[u] = v;
                }
            }
            __syncthreads(); // (one workgroup: its global writes are visible to it behind the barrier)
        }
    for (int64_t i = tid; i < n; i += IVF_RANGE_THREADS) I[i] += a.idx_offset;
}

} // namespace mips
