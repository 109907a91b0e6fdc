// Kernels of the IVF index over PQ codes (include/mips_hip_ivfpq.h).  The arithmetic is csrc/ivfpq_math.hpp.
// Every kernel of this file is named ivfadc_*: the tables, the trainers and the list table are the kernels of pq_kernels.hpp and
// ivf_kernels.hpp, launched as they are.
//
//   build     ivfadc_residual_kernel: out[i] = (float32)x[i] - c[assign[i]], one float32 subtraction per column.
//   search    ivfadc_scan_kernel is the hot path.  Workgroup (j, s) of ns * S, query fastest, copies query j's table into LDS,
//             builds in LDS the prefix of the sizes of j's p probed lists (list numbers and bounds read and range-checked here: a
//             bad one counts as an empty list), and serves positions [floor(N_j s / S), floor(N_j (s + 1) / S)) of their
//             concatenation in probe order -- list by list, so the coarse term T and the list bounds are uniform over a wave;
//             64-row tiles are dealt to the waves round robin ACROSS lists, so short lists do not idle waves.  A lane gathers the
//             codes of its row list_rows[pos] in 16-byte chunks, the next in flight while the current one is summed
//             (pq_adc_chunk), from T (by_residual) or -0.0f.  The per-wave sorted best k, their union in LDS and the sorted
//             partial [S][ns][k][2] are those of pq_adc_scan_kernel.  ivfadc_finish_kernel adds idx_offset behind the merge.
//   by id     ivfadc_rows_kernel (centroid + decode), ivfadc_score_subset_kernel (T of the row's OWN list, computed here as the
//             canonical score, then the same sum).
//   probe     ivfadc_lists_kernel narrows the coarse search's int64 list numbers to the caller's int32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivfpq_math.hpp"
#include "pq_kernels.hpp"

namespace mips {

// out [n][d] = the residual of row i against centroid assign[i] (by_residual), or the widened row.  A list number outside
// [0, nlist) reads centroid 0 (it cannot come out of ivf_to_assign_kernel, which clamps).
template <typename T>
__global__ void ivfadc_residual_kernel(const T* x, int64_t n, int d, const int* assign, int nlist, const float* cent, int by_residual, float* out) {
    const int64_t total = n * d;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / d;
        const int t = (int)(e - i * d);
        const float v = pq_widen<T>(x[e]);
        if (!by_residual) {
            out[e] = v;
            continue;
        }
        int l = assign[i];
        if (l < 0 || l >= nlist) l = 0;
        out[e] = ivfpq::residual(v, cent[(size_t)l * d + t]);
    }
}

struct IvfAdcScanArgs {
    const uint8_t* codes;    // [ntotal][pitch], pitch a multiple of 16, the bytes behind column M - 1 zero
    int pitch;
    int M;
    int64_t ntotal;
    const float* lut;        // [ns][M][256]
    const int64_t* probe;    // [ns][p] list numbers, nearest first
    const float* coarse;     // [ns][p] T
    const int* offsets;      // [nlist + 1]
    const int* list_rows;    // [ntotal]
    int nlist;
    int p;
    int by_residual;
    int64_t ns;
    int S, k;
    int64_t* parts;          // [S][ns][k][2]
};

// grid = ns * S workgroups of WAVES waves, query fastest; dynamic LDS = ivfpq::scan_lds_bytes(M, p)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void ivfadc_scan_kernel(IvfAdcScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivfadc_lds[];
    float* tab = reinterpret_cast<float*>(ivfadc_lds);         // [M][256]
    float* mk = tab + (size_t)a.M * pq::kSub;                  // [WAVES][kListSlots]
    int* mi = reinterpret_cast<int*>(mk + WAVES * pq::kListSlots);
    int* mc = mi + WAVES * pq::kListSlots;                     // [WAVES]
    int* pre = mc + WAVES;                                     // [p + 1] first position of every probed list; pre[p] = N_j
    int* first = pre + a.p + 1;                                // [p] where the list starts in list_rows
    float* tq = reinterpret_cast<float*>(first + a.p);         // [p] T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.k, p = a.p;
    const int64_t b = blockIdx.x;
    const int64_t j = b % a.ns;
    const int s = (int)(b / a.ns);
    if (s >= a.S) return;

    // the probed lists of query j: sizes (into pre[u + 1]), starts, coarse terms; everything range-checked
    for (int u = tid; u < p; u += 64 * WAVES) {
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

    float lk = -INFINITY; // the wave's list: lane u < cnt holds its u-th best
    int li = IDX_NONE;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
        const u32x4* src = reinterpret_cast<const u32x4*>(a.lut + (size_t)j * a.M * pq::kSub);
        u32x4* dst = reinterpret_cast<u32x4*>(tab);
        for (int c = tid; c < a.M * (pq::kSub / 4); c += 64 * WAVES) dst[c] = src[c];
        __syncthreads();
        const int nch = a.pitch / 16;
        int tile0 = 0; // 64-row tiles of the lists before this one, modulo WAVES: tiles go to the waves round robin
        for (int u = ivfpq::locate(pre, p, lo); u < p && (int64_t)pre[u] < hi; ++u) {
            const int64_t pa = lo > pre[u] ? lo : (int64_t)pre[u], pb = hi < pre[u + 1] ? hi : (int64_t)pre[u + 1];
            if (pa >= pb) continue; // an empty list
            const float acc0 = ivfpq::score_start(tq[u], a.by_residual != 0);
            const int64_t base = (int64_t)first[u] - pre[u]; // list_rows[base + pos]: the row at position pos of the concatenation
            const int ntile = (int)((pb - pa + 63) / 64);
            for (int t = (wave - tile0 + WAVES) % WAVES; t < ntile; t += WAVES) {
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
                pq_list_insert(acc, row, lane, K, lk, li, cnt);
            }
            tile0 = (tile0 + ntile) % WAVES;
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

// behind the merge, over [ns][k]: idx_offset added to the rows; padding stays (-inf, -1)
__global__ void ivfadc_finish_kernel(int64_t* out_i, int64_t total, int64_t idx_offset) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = out_i[t];
        if (id >= 0) out_i[t] = id + idx_offset;
    }
}

// the coarse search's list numbers [total] int64 -> int32 (a number outside [0, nlist): -1)
__global__ void ivfadc_lists_kernel(const int64_t* idx, int64_t total, int nlist, int* out) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = idx[t];
        out[t] = l >= 0 && l < nlist ? (int)l : -1;
    }
}

// --------------------------------------------------------------------------------------------------------------------- by id
// out[i][0:d] = c[assign[id]] + the concatenation of C[m][code[id][m]] (by_residual: one float32 addition per column); an id that
// names no row: a quiet-NaN row, or zero bytes
__global__ void ivfadc_rows_kernel(const uint8_t* codes, int pitch, int64_t ntotal, const float* cb, int d, int M, const int* assign, int nlist,
                                   const float* cent, int by_residual, const int64_t* ids, int64_t n, int64_t idx_offset, float* out, int64_t out_ld,
                                   int zero_missing) {
    const int dsub = d / M;
    const int64_t total = n * d;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / d;
        const int col = (int)(e - i * d);
        const int64_t r = ids[i] - idx_offset;
        float v;
        if (r < 0 || r >= ntotal) v = zero_missing ? 0.0f : __uint_as_float(0x7FC00000u);
        else {
            const int m = col / dsub;
            v = cb[((size_t)m * pq::kSub + codes[(size_t)r * pitch + m]) * dsub + (col - m * dsub)];
            if (by_residual) {
                int l = assign[r];
                if (l < 0 || l >= nlist) l = 0;
                v = ivfpq::recon(cent[(size_t)l * d + col], v);
            }
        }
        out[(size_t)i * out_ld + col] = v;
    }
}

// out[j][t] = the score of row ids[j][t] - idx_offset for query j of a slice, with the coarse term of the row's own list:
// T = s(q_j, c_l), the canonical score; "no row": -inf
template <typename T>
__global__ void ivfadc_score_subset_kernel(const uint8_t* codes, int pitch, int64_t ntotal, const float* lut, int M, const int* assign, int nlist,
                                           const float* cent, int d, int by_residual, const T* q, const int64_t* ids, int64_t ns, int k, int64_t idx_offset,
                                           float* out) {
    const int64_t total = ns * k;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = ids[e] - idx_offset;
        if (r < 0 || r >= ntotal) {
            out[e] = -INFINITY;
            continue;
        }
        const int64_t j = e / k;
        float coarse = 0.0f;
        if (by_residual) {
            int l = assign[r];
            if (l < 0 || l >= nlist) l = 0;
            const T* qs = q + (size_t)j * d;
            const float* c = cent + (size_t)l * d;
            double acc = 0.0;
            for (int t = 0; t < d; ++t) acc = pq::sum_step(acc, pq_widen<T>(qs[t]), c[t]);
            coarse = (float)acc;
        }
        out[e] = ivfpq::score(coarse, lut + (size_t)j * M * pq::kSub, codes + (size_t)r * pitch, M, by_residual != 0);
    }
}

} // namespace mips
