// Exact range search (mips_range_search): every row whose canonical score lies beyond a per-query radius, in CSR form.
//
// The index is walked in row chunks of at most RANGE_CHUNK rows with the wide search's geometry (scan_kernel_wide.hpp):
//
//   range_tau_kernel      once per query slice: |q|^2 as the canonical sum and the scan threshold tau of every query -- the
//                         radius's image in the dot domain, lowered by the bound on the scan's error, rounded DOWN to float32.
//                         tau never moves during the call, so the rows the scan appends are a superset of the members
//                          and nothing has to be certified or settled afterwards.
//   wide_scan_kernel      as it is: appends every row whose MFMA score beats tau to the segments of (query, split, lane half).
//   range_filter_kernel   one workgroup per query after each chunk: leaves at once when nothing was appended; otherwise computes
//                         the canonical score of every appended row (arithmetic and column order of wide_rescore_kernel), applies
//                         the strict float32 rule and marks the members in a bitmap over the chunk's rows, their scores in an
//                         array indexed by row-in-chunk, both in LDS.  A popcount prefix sum over the bitmap words then gives
//                         every member its rank in ascending row order -- no sort.  The members go into a block of the staging
//                         buffer reserved with ONE atomic add on a global cursor; (offset, count) is recorded for (query, chunk).
//                         Entries past the staging capacity are dropped, the counts stay true.
//   range_lims_kernel     prefix sum of the slice's per-query totals into out_lims, continued from the slices before it.
//   range_compact_kernel  one wave per query: copies the query's blocks in chunk order to [lims[q], lims[q + 1]) of the caller's
//                         arrays (writes past `cap` are dropped: the caller sees lims[nq] > cap and repeats the call).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel_wide.hpp"

namespace mips {

constexpr int RANGE_CHUNK = 8192;                 // rows per chunk at most: what the filter's LDS bitmap + score array hold
constexpr int RANGE_THREADS = RANGE_CHUNK / 32;   // one bitmap word per thread
constexpr int RANGE_LIMS_THREADS = 1024;          // x 4 queries per thread = one slice
static_assert(RANGE_THREADS == WIDE_MAX_SEG, "the filter's segment scan takes one segment counter per thread");

struct RangeTauArgs {
    const void* y;       // canonical staged queries of the slice (bf16 rows / fp32 rows), pitch ld
    int ld;
    int nq, nq_pad;
    const float* radii;  // [nq]
    int l2;
    double phi;
    const double* xmax2;
    const double* dres2; // fp32-exact index (with qerr2), else nullptr
    const double* qerr2;
    double err_c;
    float* tau;          // [nq_pad] out: the scan's threshold (+inf for pad queries: nothing passes)
    double* qq;          // [nq] out: |q|^2 as the canonical sum
};

template <typename EL>
__global__ __launch_bounds__(256) void range_tau_kernel(RangeTauArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nq_pad) return;
    if (q >= a.nq) {
        a.tau[q] = INFINITY;
        return;
    }
    const typename EL::type* y = reinterpret_cast<const typename EL::type*>(a.y) + (size_t)q * a.ld;
    double s = 0.0;
    for (int c = 0; c < a.ld; c += EL::PER16) { // sequential in the column index like the dot products
        const u32x4 v = *reinterpret_cast<const u32x4*>(y + c);
#pragma unroll
        for (int e = 0; e < EL::PER16; ++e) {
            const double t = (double)EL::get(v, e);
            s += t * t;
        }
    }
    a.qq[q] = s;
    const float rf = a.radii[q];
    float tau;
    if (isinf(rf)) { // everything or nothing: IP members score ABOVE the radius, L2 members lie BELOW it
        tau = ((rf > 0.f) == (a.l2 != 0)) ? -INFINITY : INFINITY;
    } else {
        // Every member's canonical dot lies beyond `image`: rounding to float32 is monotone, so (float)dot > r needs dot > r, and
        // (float)(|q|^2 + phi - 2 dot) < r needs dot > (|q|^2 + phi - r) / 2 up to the fp64 rounding of that expression; `slack`
        // (an ulp of float32 on the magnitudes involved) covers both many times over.  The scan's score a obeys dot <= a + e.
        const double r = (double)rf;
        const double c = s + a.phi;
        const double image = a.l2 ? 0.5 * (c - r) : r;
        const double slack = 1.1920928955078125e-07 * (a.l2 ? fabs(c) + fabs(r) : fabs(r));
        const double qn = sqrt(s), xm = sqrt(*a.xmax2);
        double e = a.err_c * qn * xm;
        if (a.qerr2 != nullptr) {
            const double dr = sqrt(*a.dres2);
            e += dr * qn + (xm + dr) * sqrt(a.qerr2[q]);
        }
        const double t = image - slack - e * 1.000000001 - 1e-300;
        tau = (float)t;
        if ((double)tau > t) tau = nextafterf(tau, -INFINITY); // round DOWN: tau <= t
        if (!(t == t)) tau = -INFINITY;                        // (non-finite data: keep the superset)
    }
    a.tau[q] = tau;
}

struct RangeFilterArgs {
    const wkey_t* seg;   // [queries][nseg][segcap]
    int nseg, segcap;
    const int* cnt;      // [queries][nseg]: written by every scan launch
    const void* rows;    // canonical rows, pitch ld
    const void* y;       // canonical staged queries, pitch ld
    int ld;
    const double* qq;    // [queries]
    double phi;
    const float* radii;  // [queries]
    int row0;            // first row of the chunk
    int chunk, nchunks;
    unsigned long long* cursor; // staging entries reserved so far (this slice)
    long long stage_cap;
    float* stage_s;      // [stage_cap]
    int* stage_r;        // [stage_cap] row numbers
    unsigned long long* blk_off; // [queries][nchunks]
    int* blk_cnt;        // [queries][nchunks], zeroed per slice: written only where a chunk has members
    int* qtot;           // [queries] members so far
};

template <typename EL, bool L2>
__global__ __launch_bounds__(RANGE_THREADS) void range_filter_kernel(RangeFilterArgs a) {
    __shared__ double yd[1024];
    __shared__ float sc[RANGE_CHUNK];
    __shared__ unsigned bm[RANGE_THREADS];
    __shared__ int off[RANGE_THREADS + 1];
    __shared__ unsigned long long base_s;
    constexpr int PER = EL::PER16;
    const int q = blockIdx.x, tid = threadIdx.x;
    int c = tid < a.nseg ? a.cnt[(size_t)q * a.nseg + tid] : 0;
    if (c > a.segcap) c = a.segcap;
    off[tid + 1] = c;
    if (tid == 0) off[0] = 0;
    __syncthreads();
    for (int d = 1; d < RANGE_THREADS; d <<= 1) { // inclusive scan
        const int v = tid >= d ? off[tid + 1 - d] : 0;
        __syncthreads();
        off[tid + 1] += v;
        __syncthreads();
    }
    const int total = off[RANGE_THREADS];
    if (total == 0) return;

    bm[tid] = 0u;
    const typename EL::type* ys = reinterpret_cast<const typename EL::type*>(a.y) + (size_t)q * a.ld;
    const int nchunk = a.ld / PER;
    for (int ch = tid; ch < nchunk; ch += RANGE_THREADS) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ys + (size_t)ch * PER);
#pragma unroll
        for (int e = 0; e < PER; ++e) yd[ch * PER + e] = (double)EL::get(v, e);
    }
    __syncthreads();
    const double qq = L2 ? a.qq[q] : 0.0;
    const float r = a.radii[q];
    const wkey_t* segs = a.seg + (size_t)q * a.nseg * a.segcap;
    for (int v = tid; v < total; v += RANGE_THREADS) {
        int lo = 0, hi = a.nseg; // the segment holding flat position v: largest s with off[s] <= v
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= v) lo = mid;
            else hi = mid;
        }
        const int row = wide_row(segs[(size_t)lo * a.segcap + (v - off[lo])]);
        const typename EL::type* x = reinterpret_cast<const typename EL::type*>(a.rows) + (size_t)row * a.ld;
        double dot = 0.0;
        for (int c0 = 0; c0 < nchunk; c0 += 8) { // (nchunk is a multiple of 8: rows are whole 128-byte segments)
            u32x4 w[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) w[t] = *reinterpret_cast<const u32x4*>(x + (size_t)(c0 + t) * PER);
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int e = 0; e < PER; ++e) dot += (double)EL::get(w[t], e) * yd[(c0 + t) * PER + e]; // sequential in the column index
        }
        const float outv = L2 ? (float)(qq + a.phi - 2.0 * dot) : (float)dot;
        const unsigned ric = (unsigned)(row - a.row0);
        if ((L2 ? outv < r : outv > r) && ric < (unsigned)RANGE_CHUNK) { // strict, on the float32 value
            sc[ric] = outv;
            atomicOr(&bm[ric >> 5], 1u << (ric & 31));
        }
    }
    __syncthreads();
    unsigned word = bm[tid];
    off[tid + 1] = __popc(word);
    __syncthreads();
    for (int d = 1; d < RANGE_THREADS; d <<= 1) {
        const int v = tid >= d ? off[tid + 1 - d] : 0;
        __syncthreads();
        off[tid + 1] += v;
        __syncthreads();
    }
    const int members = off[RANGE_THREADS];
    if (members == 0) return;
    if (tid == 0) {
        const unsigned long long o = atomicAdd(a.cursor, (unsigned long long)members);
        base_s = o;
        a.blk_off[(size_t)q * a.nchunks + a.chunk] = o;
        a.blk_cnt[(size_t)q * a.nchunks + a.chunk] = members;
        a.qtot[q] += members; // (one workgroup per query and launch; launches are ordered by the stream)
    }
    __syncthreads();
    long long pos = (long long)base_s + off[tid]; // members before this thread's word, in row order
    while (word != 0u) {
        const int b = __ffs((int)word) - 1;
        word &= word - 1u;
        const int ric = tid * 32 + b;
        if (pos < a.stage_cap) {
            a.stage_s[pos] = sc[ric];
            a.stage_r[pos] = a.row0 + ric;
        }
        ++pos;
    }
}

struct RangeLimsArgs {
    const int* qtot;  // [ns]
    int ns;
    int64_t s0;       // first query of the slice
    int64_t* lims;    // [nq + 1]
    unsigned long long* base; // members of the slices before this one; advanced here
};

__global__ __launch_bounds__(RANGE_LIMS_THREADS) void range_lims_kernel(RangeLimsArgs a) {
    __shared__ long long part[RANGE_LIMS_THREADS];
    const int tid = threadIdx.x;
    const long long base = (long long)*a.base;
    int v[4];
    long long sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid * 4 + i;
        v[i] = q < a.ns ? a.qtot[q] : 0;
        sum += v[i];
    }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < RANGE_LIMS_THREADS; d <<= 1) { // inclusive scan
        const long long t = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    long long run = base + part[tid] - sum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid * 4 + i;
        run += v[i];
        if (q < a.ns) a.lims[a.s0 + q + 1] = run;
    }
    if (tid == 0 && a.s0 == 0) a.lims[0] = 0;
    if (tid == RANGE_LIMS_THREADS - 1) *a.base = (unsigned long long)(base + part[tid]); // (every thread read it before the first barrier)
}

struct RangeCompactArgs {
    const unsigned long long* blk_off; // [ns][nchunks]
    const int* blk_cnt;
    int nchunks;
    int ns;
    int64_t s0;
    const int64_t* lims;
    const float* stage_s;
    const int* stage_r;
    long long stage_cap;
    float* out_s;      // [cap]
    int64_t* out_i;
    int64_t cap;
    int64_t idx_offset;
};

__global__ __launch_bounds__(256) void range_compact_kernel(RangeCompactArgs a) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.ns) return;
    long long pos = a.lims[a.s0 + q];
    const int* cnts = a.blk_cnt + (size_t)q * a.nchunks;
    const unsigned long long* offs = a.blk_off + (size_t)q * a.nchunks;
    for (int c0 = 0; c0 < a.nchunks; c0 += 64) {
        const int mine = c0 + lane < a.nchunks ? cnts[c0 + lane] : 0;
        unsigned long long mask = __ballot(mine > 0);
        while (mask != 0ull) { // chunks with members, in chunk order
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            const int n = __shfl(mine, b);
            const long long o = (long long)offs[c0 + b];
            for (int i = lane; i < n; i += 64) {
                const long long src = o + i, dst = pos + i;
                if (src < a.stage_cap && dst < a.cap) {
                    a.out_s[dst] = a.stage_s[src];
                    a.out_i[dst] = (int64_t)a.stage_r[src] + a.idx_offset;
                }
            }
            pos += n;
        }
    }
}

} // namespace mips
