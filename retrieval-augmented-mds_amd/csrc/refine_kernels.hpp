// Kernels of the two-stage search on PQ codes (include/mips_hip_refine.h): the candidate scans (30 <= k <= 1024)
// and the select pass of the exact re-ranking.  The launch arithmetic is csrc/adc_wide_math.hpp, every pool index csrc/ivf_wide_math.hpp.
//
//   cand_flat_scan_kernel   pq_adc_scan_kernel (pq_kernels.hpp) with another selection.  Unchanged: the grid of ns * S workgroups
//                           (j, s), query fastest, the table copy, one lane per row, pq_adc_chunk with the next 16-byte chunk in
//                           flight, the sorted partial [S][ns][k][2].
//   cand_list_scan_kernel   ivfadc_scan_kernel (ivfpq_kernels.hpp) likewise: the LDS prefix of the probed list sizes (list numbers,
//                           bounds and rows read and range-checked here), ivfpq::locate, the 64-row tiles dealt round robin across
//                           list boundaries, the coarse term in front of the sum.
//                           New in both: a wave's best k live in a POOL of KP slots in LDS (64, 256 or 1024) -- fill, one bitonic
//                           sort, then slot k - 1 is the threshold and a row that ranks before it is inserted at its binary-search
//                           rank (ivf_pool_sort and the pool indices are those of the wide IVF scan).  The workgroup has as many
//                           waves as pools fit beside the table (adcw::pools: 16 .. 1), one pool per wave, so no wave waits for
//                           another inside the scan loop.  Behind the one final barrier every wave ranks the union of the P sorted
//                           pools (adcw::union_rank, any P).
//   rerank_select_kernel    one workgroup per query: kc <= 1024 (score, id) pairs, an id that names no row and a NaN score replaced
//                           by (-inf, no id), one bitonic sort in LDS by (score descending, id ascending) with the same index
//                           functions, equal ids (adjacent, equal scores) dropped but the first, the first k written, padding last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adc_wide_math.hpp"
#include "ivf_wide_kernels.hpp"
#include "ivfpq_kernels.hpp"

namespace mips {

// the wave takes what ranks among its best K into its pool (pk, pr, cnt): cnt < K -- unsorted; cnt == K -- sorted, slot K - 1 the
// threshold.  id < 0: this lane has no row
template <int KP>
__device__ __forceinline__ void cand_pool_take(float key, int id, int lane, int K, float* pk, int* pr, int& cnt) {
    unsigned long long m = __ballot(id >= 0);
    if (m == 0ull) return;
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

// behind the workgroup's final barrier: the sorted partial of K entries out of the P sorted pools, padding (-inf, -1) last
__device__ __forceinline__ void cand_write_partial(const float* poolk, const int* poolr, const int* mc, int P, int KP, int K, int tid, int64_t* out) {
    int total = 0;
    for (int w = 0; w < P; ++w) total += mc[w];
    for (int e = tid; e < P * KP; e += 64 * P) {
        const int w = adcw::rank_pool(e, KP), u = adcw::rank_slot(e, KP);
        if (u >= mc[w]) continue;
        const int rank = adcw::union_rank(poolk, poolr, mc, P, KP, w, u, K);
        if (rank < K) {
            out[2 * rank] = (int64_t)__float_as_uint(poolk[e]);
            out[2 * rank + 1] = (int64_t)poolr[e];
        }
    }
    for (int u = total + tid; u < K; u += 64 * P) {
        out[2 * u] = (int64_t)__float_as_uint(-INFINITY);
        out[2 * u + 1] = -1;
    }
}

// grid = ns * S workgroups of P = adcw::waves(M, KP, 0) waves, query fastest; dynamic LDS = adcw::lds_bytes(M, KP, 0)
template <int KP>
__global__ __launch_bounds__(64 * adcw::kMaxPools) void cand_flat_scan_kernel(PqScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_flat_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = (int)(blockDim.x >> 6);
    float* tab = reinterpret_cast<float*>(cand_flat_lds);      // [M][256]
    float* poolk = tab + (size_t)a.M * pq::kSub;               // [P][KP]
    int* poolr = reinterpret_cast<int*>(poolk + P * KP);       // [P][KP]
    int* mc = poolr + P * KP;                                  // [kMaxPools]
    const int K = a.k; // <= KP: the host chose the instance
    const int64_t b = blockIdx.x;
    const int64_t j = b % a.ns;
    const int s = (int)(b / a.ns);
    if (s >= a.S || K < 1 || K > KP || P > adcw::kMaxPools) return;
    const int64_t lo = pq::seg_bound(a.ntotal, s, a.S), hi = pq::seg_bound(a.ntotal, s + 1, a.S);

    float* pk = poolk + wave * KP; // the wave's pool
    int* pr = poolr + wave * KP;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
        const u32x4* src = reinterpret_cast<const u32x4*>(a.lut + (size_t)j * a.M * pq::kSub);
        u32x4* dst = reinterpret_cast<u32x4*>(tab);
        for (int c = tid; c < a.M * (pq::kSub / 4); c += 64 * P) dst[c] = src[c];
        __syncthreads();
        const int nch = a.pitch / 16;
        for (int64_t r0 = lo + (int64_t)wave * 64; r0 < hi; r0 += 64 * P) {
            const int64_t row = r0 + lane;
            const bool have = row < hi;
            // (a lane without a row reads row lo: inside the index)
            const u32x4* cp = reinterpret_cast<const u32x4*>(a.codes + (size_t)(have ? row : lo) * a.pitch);
            float acc = -0.0f;
            u32x4 cur = cp[0];
            for (int c = 0; c < nch; ++c) {
                const u32x4 nxt = c + 1 < nch ? cp[c + 1] : cur; // the next chunk is in flight while this one is summed
                acc = pq_adc_chunk(acc, cur, tab, 16 * c, a.M);
                cur = nxt;
            }
            cand_pool_take<KP>(acc, have ? (int)row : -1, lane, K, pk, pr, cnt);
        }
        if (cnt > 1 && cnt < K) ivf_pool_sort<KP>(pk, pr, cnt, lane); // a pool that never filled
    }
    if (lane == 0) mc[wave] = cnt;
    __syncthreads();
    cand_write_partial(poolk, poolr, mc, P, KP, K, tid, a.parts + ((int64_t)s * a.ns + j) * K * 2);
}

// grid = ns * S workgroups of P = adcw::waves(M, KP, p) waves, query fastest; dynamic LDS = adcw::lds_bytes(M, KP, p)
template <int KP>
__global__ __launch_bounds__(64 * adcw::kMaxPools) void cand_list_scan_kernel(IvfAdcScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_list_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = (int)(blockDim.x >> 6);
    const int K = a.k, p = a.p;
    float* tab = reinterpret_cast<float*>(cand_list_lds);      // [M][256]
    float* poolk = tab + (size_t)a.M * pq::kSub;               // [P][KP]
    int* poolr = reinterpret_cast<int*>(poolk + P * KP);       // [P][KP]
    int* mc = poolr + P * KP;                                  // [kMaxPools]
    int* pre = mc + adcw::kMaxPools;                           // [p + 1] first position of every probed list; pre[p] = N_j
    int* first = pre + p + 1;                                  // [p] where the list starts in list_rows
    float* tq = reinterpret_cast<float*>(first + p);           // [p] T
    const int64_t b = blockIdx.x;
    const int64_t j = b % a.ns;
    const int s = (int)(b / a.ns);
    if (s >= a.S || K < 1 || K > KP || P > adcw::kMaxPools) return;

    // the probed lists of query j: sizes (into pre[u + 1]), starts, coarse terms; everything range-checked
    for (int u = tid; u < p; u += 64 * P) {
        const int64_t l = a.probe[j * p + u];
        int beg = 0, size = 0;
        if (l >= 0 && l < a.nlist) {
            const int b0 = a.offsets[l], b1 = a.offsets[l + 1];
            if (b0 >= 0 && b0 <= b1 && (int64_t)b1 <= a.ntotal) {
                beg = b0;
                size = b1 - b0;
            }
        }
        pre[u + 1] = size;
        first[u] = beg;
        tq[u] = a.coarse[j * p + u];
    }
    if (tid == 0) pre[0] = 0;
    __syncthreads();
    if (wave == 0) { // inclusive prefix of pre[1 .. p]: a run of consecutive entries per lane, then the lanes' totals
        const int per = (p + 63) / 64;
        const int u0 = lane * per < p ? lane * per : p;
        const int u1 = u0 + per < p ? u0 + per : p;
        long long run = 0;
        for (int u = u0; u < u1; ++u) run += pre[u + 1];
        long long before = run; // inclusive scan over the lanes
        for (int o = 1; o < 64; o <<= 1) {
            const long long v = __shfl_up(before, o);
            if (lane >= o) before += v;
        }
        before -= run;
        for (int u = u0; u < u1; ++u) {
            before += pre[u + 1];
            pre[u + 1] = (int)(before > a.ntotal ? a.ntotal : before); // (sizes of distinct lists sum to <= ntotal; a repeated list is capped)
        }
    }
    __syncthreads();
    const int64_t Nj = pre[p];
    const int64_t lo = pq::seg_bound(Nj, s, a.S), hi = pq::seg_bound(Nj, s + 1, a.S);

    float* pk = poolk + wave * KP; // the wave's pool
    int* pr = poolr + wave * KP;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
        const u32x4* src = reinterpret_cast<const u32x4*>(a.lut + (size_t)j * a.M * pq::kSub);
        u32x4* dst = reinterpret_cast<u32x4*>(tab);
        for (int c = tid; c < a.M * (pq::kSub / 4); c += 64 * P) dst[c] = src[c];
        __syncthreads();
        const int nch = a.pitch / 16;
        int tile0 = 0; // 64-row tiles of the lists before this one, modulo P: tiles go to the waves round robin
        for (int u = ivfpq::locate(pre, p, lo); u < p && (int64_t)pre[u] < hi; ++u) {
            const int64_t pa = lo > pre[u] ? lo : (int64_t)pre[u], pb = hi < pre[u + 1] ? hi : (int64_t)pre[u + 1];
            if (pa >= pb) continue; // an empty list
            const float acc0 = ivfpq::score_start(tq[u], a.by_residual != 0);
            const int64_t base = (int64_t)first[u] - pre[u]; // list_rows[base + pos]: the row at position pos of the concatenation
            const int ntile = (int)((pb - pa + 63) / 64);
            for (int t = (wave - tile0 + P) % P; t < ntile; t += P) {
                const int64_t pos = pa + (int64_t)t * 64 + lane;
                int row = pos < pb ? a.list_rows[base + pos] : -1;
                if (row < 0 || (int64_t)row >= a.ntotal) row = -1; // (a bad row number scores nothing)
                // (a lane without a row reads row 0: inside the index, ntotal > 0 here)
                const u32x4* cp = reinterpret_cast<const u32x4*>(a.codes + (size_t)(row >= 0 ? row : 0) * a.pitch);
                float acc = acc0;
                u32x4 cur = cp[0];
                for (int c = 0; c < nch; ++c) {
                    const u32x4 nxt = c + 1 < nch ? cp[c + 1] : cur; // the next chunk is in flight while this one is summed
                    acc = pq_adc_chunk(acc, cur, tab, 16 * c, a.M);
                    cur = nxt;
                }
                cand_pool_take<KP>(acc, row, lane, K, pk, pr, cnt);
            }
            tile0 = (tile0 + ntile) % P;
        }
        if (cnt > 1 && cnt < K) ivf_pool_sort<KP>(pk, pr, cnt, lane); // a pool that never filled
    }
    if (lane == 0) mc[wave] = cnt;
    __syncthreads();
    cand_write_partial(poolk, poolr, mc, P, KP, K, tid, a.parts + ((int64_t)s * a.ns + j) * K * 2);
}

// ------------------------------------------------------------------------------------------------------------------ re-ranking
struct RerankArgs {
    const float* scores;  // [nq][kc] what mips_score_subset reported
    const int64_t* ids;   // [nq][kc] as the caller gave them
    int kc, k;            // 1 <= k <= kc <= adcw::kRerankMax
    int64_t ntotal, idx_offset;
    float* out_s;         // [nq][k]
    int64_t* out_i;       // [nq][k]
};

constexpr int RERANK_THREADS = 256;
static_assert(RERANK_THREADS * 4 == adcw::kRerankMax, "four consecutive entries per thread in the compaction");

// grid = nq workgroups
__global__ __launch_bounds__(RERANK_THREADS) void rerank_select_kernel(RerankArgs a) {
    __shared__ float sk[adcw::kRerankMax];
    __shared__ int64_t si[adcw::kRerankMax];
    __shared__ int wsum[RERANK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j = blockIdx.x;
    if (a.kc < 1 || a.kc > adcw::kRerankMax || a.k < 1 || a.k > a.kc) return;
    const int n = ivf::sort_span(a.kc, adcw::kRerankMax);
    for (int u = tid; u < n; u += RERANK_THREADS) {
        float s = -INFINITY;
        int64_t id = adcw::kNoId;
        if (u < a.kc) {
            const int64_t g = a.ids[j * a.kc + u];
            const float v = a.scores[j * a.kc + u];
            if (adcw::rerank_valid(g, a.idx_offset, a.ntotal) && v == v) { // (a NaN score is dropped like an id that names no row)
                s = v;
                id = g;
            }
        }
        sk[u] = s;
        si[u] = id;
    }
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < n / 2; t += RERANK_THREADS) { // (the pairs of a stage are disjoint)
                const int lo = ivf::bitonic_low(t, stride), hi = ivf::bitonic_high(t, stride);
                const float ka = sk[lo], kb = sk[hi];
                const int64_t ia = si[lo], ib = si[hi];
                const bool swap = ivf::bitonic_best_low(lo, size) ? adcw::rerank_before(kb, ib, ka, ia) : adcw::rerank_before(ka, ia, kb, ib);
                if (swap) {
                    sk[lo] = kb;
                    si[lo] = ib;
                    sk[hi] = ka;
                    si[hi] = ia;
                }
            }
            __syncthreads();
        }
    // compaction: thread t owns entries 4 t .. 4 t + 3; its kept entries go behind those of the threads before it
    bool keep[4];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int u = 4 * tid + e;
        keep[e] = u < n && adcw::rerank_keep(si, u);
        mine += keep[e] ? 1 : 0;
    }
    int incl = mine; // inclusive scan over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int pos = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < RERANK_THREADS / 64; ++w) {
        if (w < wave) pos += wsum[w];
        total += wsum[w];
    }
    float* os = a.out_s + j * a.k;
    int64_t* oi = a.out_i + j * a.k;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!keep[e]) continue;
        if (pos < a.k) {
            os[pos] = sk[4 * tid + e];
            oi[pos] = si[4 * tid + e];
        }
        ++pos;
    }
    for (int u = total + tid; u < a.k; u += RERANK_THREADS) {
        os[u] = -INFINITY;
        oi[u] = -1;
    }
}

} // namespace mips
