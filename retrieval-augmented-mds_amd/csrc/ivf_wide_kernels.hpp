// The list scan of the wide IVF search (include/mips_hip_ivf.h: mips_ivf_search_wide / _grp, MIPS_MAX_K < k <= MIPS_MAX_K_WIDE;
// DESIGN.md section 4j).
//
//   ivf_list_scan_wide_kernel   ivf_list_scan_kernel (ivf_search_kernels.hpp) with another selection.  Unchanged: the grid of
//                          nq * p * S workgroups (j, t, s), the range checks of list number, list bounds and row numbers where they
//                          are read, ivf_gathered_dot, the admission of a filtered instance where the row number is read and its
//                          per-wave queue, the packed layout [p * S][nq][k][2] of the sorted partial.
//                          New: a wave's best k live in a POOL of KP slots in LDS (KP = 64, 256 or 1024, the smallest >= k;
//                          ivf_wide_math.hpp holds every index that addresses one) instead of lanes 0 .. k - 1 of two registers.
//                          Fill, then threshold: candidates are appended unsorted until the pool holds k, the wave sorts it once (a
//                          bitonic network over the smallest power of two >= k), from then on slot k - 1 is the threshold and only
//                          a row that ranks before it is inserted (binary search for the rank, the tail shifted in chunks of 64
//                          from the top).  A pool that never fills is sorted once at the end.  A pool belongs to ONE wave: its
//                          steps are ordered by wave barriers, so no workgroup barrier sits in the scan loop (under a filter the
//                          waves run different numbers of passes) and no workgroup waits for another.  Behind the one final
//                          barrier all four waves rank the union: entry u of pool w has rank u + the entries of the other three
//                          sorted pools that rank before it (binary searches; the rows are distinct, so every rank is taken once).
//                          The order (key descending, row ascending) is total, so neither the order in which rows are scored nor
//                          the order in which they were appended shows in the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_search_kernels.hpp"
#include "ivf_wide_math.hpp"

namespace mips {

static_assert(ivf::kWideWaves == IVF_SCAN_WAVES, "pools per workgroup");

// orders the LDS operations of ONE wave's lanes among themselves (they complete in order; the compiler keeps them in order too)
__device__ __forceinline__ void ivf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// slot u < cnt of the pool holds its u-th best afterwards (cnt <= KP)
template <int KP>
__device__ __forceinline__ void ivf_pool_sort(float* pk, int* pr, int cnt, int lane) {
    const int n = ivf::sort_span(cnt, KP);
    for (int u = cnt + lane; u < n; u += ivf::kWideLanes) {
        pk[u] = -INFINITY;
        pr[u] = ivf::kNoRow;
    }
    ivf_wave_sync();
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < n / 2; t += ivf::kWideLanes) { // (the pairs of a stage are disjoint)
                const int lo = ivf::bitonic_low(t, stride), hi = ivf::bitonic_high(t, stride);
                const float ka = pk[lo], kb = pk[hi];
                const int ra = pr[lo], rb = pr[hi];
                const bool swap = ivf::bitonic_best_low(lo, size) ? ivf::wide_before(kb, rb, ka, ra) : ivf::wide_before(ka, ra, kb, rb);
                if (swap) {
                    pk[lo] = kb;
                    pr[lo] = rb;
                    pk[hi] = ka;
                    pr[hi] = ra;
                }
            }
            ivf_wave_sync();
        }
}

// One scoring pass: lane `lane` scores row `id` (id < 0: none) and the wave takes what ranks among its best K into its pool
// (pk, pr, cnt): cnt < K -- unsorted; cnt == K -- sorted, slot K - 1 the threshold.
template <typename EL, int KP>
__device__ __forceinline__ void ivf_score_pool(const typename EL::type* rows, int ld, int id, int lane, u32x4* tile, const double* yd, int K, float* pk,
                                               int* pr, int& cnt) {
    const float key = (float)ivf_gathered_dot<EL>(rows, ld, id, lane, tile, yd);
    unsigned long long m = __ballot(id >= 0);
    if (cnt < K) { // fill (uniform over the wave)
        const int slot = ivf::fill_slot(cnt, K, m, lane);
        if (slot >= 0) {
            pk[slot] = key;
            pr[slot] = id;
        }
        cnt += ivf::fill_take(cnt, K, m);
        m = __ballot(id >= 0 && slot < 0); // candidates that found the pool full
        ivf_wave_sync();
        if (cnt < K) return;
        ivf_pool_sort<KP>(pk, pr, cnt, lane);
    }
    const int ts = ivf::threshold_slot(K);
    float tk = pk[ts];
    int tr = pr[ts];
    m = __ballot(((m >> lane) & 1ull) != 0ull && ivf::wide_before(key, id, tk, tr));
    while (m != 0ull) { // one candidate at a time, the whole wave on it
        const int c = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const float nk = __shfl(key, c);
        const int ni = __shfl(id, c);
        if (!ivf::wide_before(nk, ni, tk, tr)) continue; // (the threshold has moved since the ballot)
        const int at = ivf::count_before(pk, pr, K, nk, ni); // < K: the threshold ranks behind the candidate
        const int chunks = ivf::shift_chunks(at, K);
        for (int ch = 0; ch < chunks; ++ch) {
            const int dst = ivf::shift_dst(K, ch, lane);
            const bool mv = dst > at;
            float vk = 0.f;
            int vr = 0;
            if (mv) {
                vk = pk[dst - 1];
                vr = pr[dst - 1];
            }
            ivf_wave_sync();
            if (mv) {
                pk[dst] = vk;
                pr[dst] = vr;
            }
            ivf_wave_sync();
        }
        if (lane == 0) {
            pk[at] = nk;
            pr[at] = ni;
        }
        ivf_wave_sync();
        tk = pk[ts];
        tr = pr[ts];
    }
}

// EL, ELQ, FILT: as ivf_list_scan_kernel; KP: slots of a wave's pool, ivf::pool_class(a.k)
template <typename EL, typename ELQ, bool FILT, int KP>
__global__ __launch_bounds__(64 * IVF_SCAN_WAVES) void ivf_list_scan_wide_kernel(IvfScanArgs a) {
    __shared__ __attribute__((aligned(16))) double yd[IVF_SCAN_MAX_LD];
    __shared__ __attribute__((aligned(16))) u32x4 tiles[IVF_SCAN_WAVES * 64 * (IVF_SCAN_TCH + 1)];
    __shared__ float poolk[IVF_SCAN_WAVES * KP];
    __shared__ int poolr[IVF_SCAN_WAVES * KP];
    __shared__ int fq[FILT ? IVF_SCAN_WAVES * ivf::kQueueSlots : 1]; // the waves' queues of admitted row numbers
    __shared__ int mc[IVF_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.k; // <= KP: the host chose the instance
    const int64_t b = blockIdx.x;
    const int s = (int)(b % a.S);
    const int t = (int)((b / a.S) % a.p);
    const int64_t j = b / ((int64_t)a.S * a.p);
    if (j >= a.nq || K < 1 || K > KP) return;
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

    float* pk = poolk + wave * KP; // the wave's pool
    int* pr = poolr + wave * KP;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
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
            ivf_score_pool<EL, KP>(rows, a.ld, id, lane, tile, yd, K, pk, pr, cnt);
        }
        if constexpr (FILT) {
            if (queued > 0) ivf_score_pool<EL, KP>(rows, a.ld, lane < queued ? queue[lane] : -1, lane, tile, yd, K, pk, pr, cnt); // the remainder
        }
        if (cnt > 1 && cnt < K) ivf_pool_sort<KP>(pk, pr, cnt, lane); // a pool that never filled
    }
    if (lane == 0) mc[wave] = cnt;
    __syncthreads();
    // all four waves rank the union of the sorted pools (distinct rows: every rank below the total is taken once)
    int64_t* out = a.parts + (((int64_t)t * a.S + s) * a.nq + j) * K * 2;
    int total = 0;
#pragma unroll
    for (int w = 0; w < IVF_SCAN_WAVES; ++w) total += mc[w];
    for (int e = tid; e < IVF_SCAN_WAVES * KP; e += 64 * IVF_SCAN_WAVES) {
        const int w = ivf::merge_pool(e, KP), u = ivf::merge_slot(e, KP);
        if (u >= mc[w]) continue;
        const float ck = poolk[e];
        const int ci = poolr[e];
        int rank = u;
        for (int w2 = 0; w2 < IVF_SCAN_WAVES && rank < K; ++w2)
            if (w2 != w) rank += ivf::count_before(poolk + w2 * KP, poolr + w2 * KP, mc[w2], ck, ci);
        if (rank < K) {
            out[2 * rank] = (int64_t)__float_as_uint(ck);
            out[2 * rank + 1] = (int64_t)ci;
        }
    }
    for (int u = total + tid; u < K; u += 64 * IVF_SCAN_WAVES) {
        out[2 * u] = (int64_t)__float_as_uint(-INFINITY);
        out[2 * u + 1] = -1;
    }
}

} // namespace mips
