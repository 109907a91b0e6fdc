// Kernels of the product-quantised index (include/mips_hip_pq.h).  The arithmetic is csrc/pq_math.hpp.
//
//   training  pq_init_codebook_kernel, pq_assign_kernel (every row x sub-quantiser against its 256 centroids), the list table per
//             sub-quantiser (pq_hist_kernel / pq_offsets_kernel / pq_list_fill_kernel: the IVF trainer's, restated for M tables of
//             256 lists) and pq_centroid_mean_kernel (one thread per (sub-quantiser, centroid, column) walks its members in
//             ascending row order).  Build-time code: deterministic, not tuned.
//   encode    pq_assign_kernel writes the codes (the same kernel, other strides).
//   search    pq_lut_kernel writes LUT [ns][M][256]; pq_adc_scan_kernel is the hot path: workgroup (j, s) copies query j's table
//             into LDS and streams the codes of row segment s, one lane per row, M table reads and M float32 additions per row in
//             ascending m; every wave keeps a sorted top k by (score descending, row ascending) in its lanes 0 .. k - 1 (the lists of
//             ivf_list_scan_kernel); the waves' lists meet in LDS and wave 0 writes the workgroup's sorted partial of k entries,
//             padding (-inf, -1) last, in the MIPS_OUT_PACKED layout [S][ns][k][2] that merge_topk_sorted_packed_kernel reads.
//             pq_finish_kernel adds idx_offset behind the merge.
//   by id     pq_rows_kernel (reconstruct: a bit move out of the codebook), pq_score_subset_kernel (D(q_j, id) from the table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "pq_math.hpp"

namespace mips {

template <typename T>
__device__ __forceinline__ float pq_widen(T v);
template <>
__device__ __forceinline__ float pq_widen<float>(float v) { return v; }
template <>
__device__ __forceinline__ float pq_widen<uint16_t>(uint16_t v) { return bf16_bits_to_f32(v); }

// ------------------------------------------------------------------------------------------------------------------ training
// C[m][j] = T[floor(j rows / 256)] restricted to sub-vector m; one thread per element of the codebook [M][256][dsub]
__global__ void pq_init_codebook_kernel(const float* T, int64_t rows, int d, int M, float* cb) {
    const int dsub = d / M;
    const int64_t total = (int64_t)pq::kSub * d;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(e % dsub);
        const int j = (int)((e / dsub) % pq::kSub);
        const int m = (int)(e / ((int64_t)dsub * pq::kSub));
        cb[e] = T[(size_t)pq::pick(j, rows, pq::kSub) * d + (size_t)m * dsub + t];
    }
}

// The code of every (row, sub-quantiser): grid.y = m, one thread per row (the centroid reads are uniform over a wave).
// out[i * row_stride + m * m_stride]: the codes of an index (row_stride = pitch, m_stride = 1) or the trainer's [M][n] (1, n).
template <typename T>
__global__ __launch_bounds__(256) void pq_assign_kernel(const T* x, int64_t n, int d, int M, const float* cb, uint8_t* out, int64_t row_stride,
                                                        int64_t m_stride) {
    const int dsub = d / M;
    const int m = blockIdx.y;
    const float* c = cb + (size_t)m * pq::kSub * dsub;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T* xs = x + (size_t)i * d + (size_t)m * dsub;
        int best = 0;
        double e_best = 0.0;
        for (int j = 0; j < pq::kSub; ++j) {
            double e = 0.0;
            for (int t = 0; t < dsub; ++t) e = pq::dist_step(e, pq_widen<T>(xs[t]), c[(size_t)j * dsub + t]);
            if (j == 0) e_best = e;
            else if (pq::closer(e, e_best)) {
                best = j;
                e_best = e;
            }
        }
        out[(size_t)i * row_stride + (size_t)m * m_stride] = (uint8_t)best;
    }
}

// count [M][256] zeroed by the host; assign [M][n]
__global__ void pq_hist_kernel(const uint8_t* assign, int64_t n, int M, int* count) {
    const int64_t total = n * M;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&count[(e / n) * pq::kSub + assign[e]], 1);
}

// one workgroup of 256 threads per sub-quantiser: offsets [M][257]
__global__ __launch_bounds__(256) void pq_offsets_kernel(const int* count, int* offsets) {
    __shared__ int c[pq::kSub];
    const int m = blockIdx.x, j = threadIdx.x;
    c[j] = count[m * pq::kSub + j];
    __syncthreads();
    int base = 0;
    for (int u = 0; u < j; ++u) base += c[u];
    offsets[m * (pq::kSub + 1) + j] = base;
    if (j == pq::kSub - 1) offsets[m * (pq::kSub + 1) + pq::kSub] = base + c[j];
}

// one wave per (sub-quantiser, centroid): its members in ascending row order -> list_rows [M][n]
__global__ __launch_bounds__(256) void pq_list_fill_kernel(const uint8_t* assign, int64_t n, int M, const int* offsets, int* list_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t w = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (w >= (int64_t)M * pq::kSub) return;
    const int m = (int)(w / pq::kSub), j = (int)(w % pq::kSub);
    int pos = offsets[m * (pq::kSub + 1) + j];
    const int end = offsets[m * (pq::kSub + 1) + j + 1];
    if (pos == end) return;
    const uint8_t* as = assign + (size_t)m * n;
    int* rows = list_rows + (size_t)m * n;
    for (int64_t r0 = 0; r0 < n; r0 += 64) {
        const int64_t r = r0 + lane;
        const bool mine = r < n && as[r] == j;
        const unsigned long long b = __ballot(mine);
        const int at = pos + __popcll(b & ((1ull << lane) - 1ull));
        if (mine && at < end) rows[at] = (int)r;
        pos += __popcll(b);
    }
}

// one thread per (sub-quantiser, centroid, column); a centroid without members keeps its value
__global__ void pq_centroid_mean_kernel(const float* T, int64_t n, int d, int M, const int* offsets, const int* list_rows, float* cb) {
    const int dsub = d / M;
    const int64_t total = (int64_t)pq::kSub * d;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(e % dsub);
        const int j = (int)((e / dsub) % pq::kSub);
        const int m = (int)(e / ((int64_t)dsub * pq::kSub));
        const int beg = offsets[m * (pq::kSub + 1) + j], end = offsets[m * (pq::kSub + 1) + j + 1];
        if (end == beg) continue;
        const int* rows = list_rows + (size_t)m * n;
        double s = 0.0;
        for (int u = beg; u < end; ++u) s += (double)T[(size_t)rows[u] * d + (size_t)m * dsub + t]; // ascending rows
        cb[e] = pq::mean(s, end - beg);
    }
}

// -------------------------------------------------------------------------------------------------------------------- search
// LUT[j][m][c] = s(q_j^m, C[m][c]); one thread per entry
template <typename T>
__global__ void pq_lut_kernel(const T* q, int64_t ns, int d, int M, const float* cb, float* lut) {
    const int dsub = d / M;
    const int64_t total = ns * M * pq::kSub;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / ((int64_t)M * pq::kSub);
        const int mc = (int)(e - j * M * pq::kSub); // m * 256 + c
        const T* qs = q + (size_t)j * d + (size_t)(mc / pq::kSub) * dsub;
        const float* c = cb + (size_t)mc * dsub;
        double acc = 0.0;
        for (int t = 0; t < dsub; ++t) acc = pq::sum_step(acc, pq_widen<T>(qs[t]), c[t]);
        lut[e] = (float)acc;
    }
}

struct PqScanArgs {
    const uint8_t* codes; // [ntotal][pitch], pitch a multiple of 16, the bytes behind column M - 1 zero
    int pitch;
    int M;
    int64_t ntotal;
    const float* lut;     // [ns][M][256]
    int64_t ns;
    int S, k;
    int64_t* parts;       // [S][ns][k][2]
};

// the wave inserts what ranks among its best K into its sorted list (lk, li, cnt): lane u < cnt holds the wave's u-th best by
// (key descending, row ascending).  id < 0: this lane has no row
__device__ __forceinline__ void pq_list_insert(float key, int id, int lane, int K, float& lk, int& li, int& cnt) {
    const float wk = __shfl(lk, K - 1);
    const int wi = __shfl(li, K - 1);
    unsigned long long m = __ballot(id >= 0 && (cnt < K || ranks_before(key, id, wk, wi)));
    while (m != 0ull) { // one candidate at a time, the whole wave on it
        const int c = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const float nk = __shfl(key, c);
        const int ni = __shfl(id, c);
        const int at = __popcll(__ballot(lane < cnt && ranks_before(lk, li, nk, ni)));
        if (at < K) {
            const int from = lane > 0 ? lane - 1 : 0;
            const float uk = __shfl(lk, from);
            const int ui = __shfl(li, from);
            if (lane > at) {
                lk = uk;
                li = ui;
            } else if (lane == at) {
                lk = nk;
                li = ni;
            }
            cnt = cnt < K ? cnt + 1 : K;
        }
    }
}

// 16 codes of one row (columns 16 c .. 16 c + 15, those below M) against the table: float32 additions in ascending m.  The caller
// starts from -0.0f: -0 + t is t bit for bit for every t, so the first step IS "acc = LUT[0][code_0]" of pq::adc
__device__ __forceinline__ float pq_adc_chunk(float acc, const u32x4& v, const float* tab, int m0, int M) {
    if (m0 + 16 <= M) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned code = (v[e >> 2] >> ((e & 3) * 8)) & 0xffu;
            const float t = tab[(m0 + e) * pq::kSub + code];
            acc = pq::adc_step(acc, t);
        }
    } else {
        for (int e = 0; m0 + e < M; ++e) {
            const unsigned code = (v[e >> 2] >> ((e & 3) * 8)) & 0xffu;
            const float t = tab[(m0 + e) * pq::kSub + code];
            acc = pq::adc_step(acc, t);
        }
    }
    return acc;
}

// grid = ns * S workgroups of WAVES waves, query fastest (the workgroups of one segment run together and share its codes in L2);
// dynamic LDS = pq::scan_lds_bytes(M)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void pq_adc_scan_kernel(PqScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_lds[];
    float* tab = reinterpret_cast<float*>(pq_lds);             // [M][256]
    float* mk = tab + (size_t)a.M * pq::kSub;                  // [WAVES][kListSlots]
    int* mi = reinterpret_cast<int*>(mk + WAVES * pq::kListSlots);
    int* mc = mi + WAVES * pq::kListSlots;                     // [WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.k;
    const int64_t b = blockIdx.x;
    const int64_t j = b % a.ns;
    const int s = (int)(b / a.ns);
    if (s >= a.S) return;
    const int64_t lo = pq::seg_bound(a.ntotal, s, a.S), hi = pq::seg_bound(a.ntotal, s + 1, a.S);

    float lk = -INFINITY; // the wave's list: lane u < cnt holds its u-th best
    int li = IDX_NONE;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
        const u32x4* src = reinterpret_cast<const u32x4*>(a.lut + (size_t)j * a.M * pq::kSub);
        u32x4* dst = reinterpret_cast<u32x4*>(tab);
        for (int c = tid; c < a.M * (pq::kSub / 4); c += 64 * WAVES) dst[c] = src[c];
        __syncthreads();
        const int nch = a.pitch / 16;
        for (int64_t r0 = lo + (int64_t)wave * 64; r0 < hi; r0 += 64 * WAVES) {
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
            pq_list_insert(acc, have ? (int)row : -1, lane, K, lk, li, cnt);
        }
    }
    if (lane < cnt) {
        mk[wave * pq::kListSlots + lane] = lk;
        mi[wave * pq::kListSlots + lane] = li;
    }
    if (lane == 0) mc[wave] = cnt;
    __syncthreads();
    if (wave != 0) return;
    // wave 0 ranks the union (<= WAVES * k entries with distinct rows: every rank is taken once)
    int64_t* out = a.parts + ((int64_t)s * a.ns + j) * K * 2;
    int total = 0;
    for (int w = 0; w < WAVES; ++w) total += mc[w];
    for (int u = 0; u < WAVES * pq::kListSlots / 64; ++u) {
        const int e = lane + 64 * u, w = e / pq::kListSlots;
        if (e % pq::kListSlots >= mc[w]) continue;
        const float ck = mk[e];
        const int ci = mi[e];
        int rank = 0;
        for (int w2 = 0; w2 < WAVES; ++w2)
            for (int u2 = 0; u2 < mc[w2]; ++u2) rank += ranks_before(mk[w2 * pq::kListSlots + u2], mi[w2 * pq::kListSlots + u2], ck, ci) ? 1 : 0;
        if (rank < K) {
            out[2 * rank] = (int64_t)__float_as_uint(ck);
            out[2 * rank + 1] = (int64_t)ci;
        }
    }
    if (lane < K && lane >= total) {
        out[2 * lane] = (int64_t)__float_as_uint(-INFINITY);
        out[2 * lane + 1] = -1;
    }
}

// behind the merge, over [nq][k]: idx_offset added to the rows; padding stays (-inf, -1)
__global__ void pq_finish_kernel(int64_t* out_i, int64_t total, int64_t idx_offset) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = out_i[t];
        if (id >= 0) out_i[t] = id + idx_offset;
    }
}

// --------------------------------------------------------------------------------------------------------------------- by id
// out[i][0:d] = the concatenation of C[m][code[id][m]]; an id that names no row: a quiet-NaN row, or zero bytes
__global__ void pq_rows_kernel(const uint8_t* codes, int pitch, int64_t ntotal, const float* cb, int d, int M, const int64_t* ids, int64_t n,
                               int64_t idx_offset, float* out, int64_t out_ld, int zero_missing) {
    const int dsub = d / M;
    const int64_t total = n * d;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / d;
        const int col = (int)(e - i * d);
        const int64_t id = ids[i];
        const int64_t r = id - idx_offset;
        float v;
        if (r < 0 || r >= ntotal) v = zero_missing ? 0.0f : __uint_as_float(0x7FC00000u);
        else {
            const int m = col / dsub;
            v = cb[((size_t)m * pq::kSub + codes[(size_t)r * pitch + m]) * dsub + (col - m * dsub)];
        }
        out[(size_t)i * out_ld + col] = v;
    }
}

// out[j][t] = D(q_j, ids[j][t] - idx_offset) for the ns queries of a slice; "no row": -inf
__global__ void pq_score_subset_kernel(const uint8_t* codes, int pitch, int64_t ntotal, const float* lut, int M, const int64_t* ids, int64_t ns, int k,
                                       int64_t idx_offset, float* out) {
    const int64_t total = ns * k;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[e];
        const int64_t r = id - idx_offset;
        if (r < 0 || r >= ntotal) {
            out[e] = -INFINITY;
            continue;
        }
        out[e] = pq::adc(lut + (size_t)(e / k) * M * pq::kSub, codes + (size_t)r * pitch, M);
    }
}

} // namespace mips
