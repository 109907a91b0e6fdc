// Wide top-k (k up to MIPS_MAX_K_WIDE = 1024): threshold scan + streaming select + exact re-score + exact settlement.
//
// The list kernels keep per-lane register lists of at most 32 entries; nothing of that shape reaches k = 1000.  Here a query
// owns a POOL of k' = k + slack candidates in global memory and a threshold tau = the approximate score of the pool's worst
// member once the pool is full.  The index is walked in row chunks:
//
//   wide_scan_kernel     the 32x32x16 MFMA loop of scan_kernel.hpp (query on the lane, 16 accumulators = 16 documents), its
//                        list-insert epilogue replaced by an APPEND: a lane compares its accumulators with its query's tau and
//                        writes the rows that pass as 64-bit entries {order-preserving score key, ~row} into the segment of
//                        (query, split, lane half).  The write cursor is a register, stored once; no atomics.  A segment holds
//                        every row its lane half sees in a chunk, so a chunk in which everything passes (the dense first chunk,
//                        sorted data) is as correct as any other.
//   wide_select_kernel   one workgroup per query after each chunk: leaves at once when nothing was appended, otherwise streams
//                        pool + new entries through an LDS buffer (bitonic sort whenever it holds more than k' entries), keeps
//                        the best k' and raises tau.  Entries order as unsigned 64-bit integers: score descending, row ascending.
//   wide_rescore_kernel  canonical scores (sequential fp64 sum on the stored values) of the pool, ranked in LDS by (float32 key,
//                        row); writes the top k and the padding, and decides the certificate: everything outside the pool has
//                        an approximate score <= tau, hence a canonical KEY no better than key(tau + error bound); unless that
//                        is strictly worse than the k-th result's key the query is flagged.
//   wide_exact_kernel    settlement of flagged queries: canonical scores of every row by brute force (exact_dots of
//                        resolve_kernels.hpp, 8 queries per pass), rows beating the query's exact threshold appended to the same
//                        segments, selected by the same select kernel with k' = k, written by wide_finalize_kernel.
// Flag list and count live on the device; workgroups past the count leave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "resolve_kernels.hpp"

namespace mips {

typedef unsigned long long wkey_t; // {key : 32, ~row : 32}; larger = ranks earlier; 0 = no entry

constexpr int WIDE_POOL = 2048;    // largest k' (pool entries per query)
constexpr int WIDE_BUF = 4096;     // LDS entries of the select: pool + one batch of new entries
constexpr int WIDE_THREADS = 256;
constexpr int WIDE_MAX_SEG = 256;  // segments per query (2 per split)

__device__ __forceinline__ wkey_t wide_pack(unsigned key, int row) { return ((wkey_t)key << 32) | (wkey_t)(~(unsigned)row); }
__device__ __forceinline__ int wide_row(wkey_t c) { return (int)(~(unsigned)(c & 0xffffffffull)); }
__device__ __forceinline__ unsigned wide_hi(wkey_t c) { return (unsigned)(c >> 32); }
// key of an OUTPUT value: inner product (larger is better) or L2 distance (smaller is better); -0 and +0 are one key
template <bool L2>
__device__ __forceinline__ unsigned wide_enc(float outv) {
    const unsigned k = thr_encode(outv + 0.0f);
    return L2 ? ~k : k;
}
template <bool L2>
__device__ __forceinline__ float wide_dec(unsigned key) { return thr_decode(L2 ? ~key : key); }

struct WideScanArgs {
    const uint16_t* docs; // [capacity][ld] bf16 bits
    const uint16_t* qbuf; // [nqt * TN][ld] bf16 bits, pad rows zero
    int64_t ntotal;
    int ld, ksteps;
    int tile0, tile_end;  // document tiles of this chunk
    int tiles_per_split;
    int nsplit;           // multiple of 8
    int nqt;
    const float* tau;     // [nqt * TN]: rows scoring above it are appended (+inf for pad queries)
    wkey_t* seg;          // [nqt * TN][2 nsplit][segcap]
    int segcap;           // >= 64 * tiles_per_split
    int* cnt;             // [nqt * TN][2 nsplit]
    const unsigned* sel;  // masked_scan_kernel: staged selector, 4 words per tile (16-byte aligned); wide_scan_kernel: unused
    const int* rlab;      // grouped_scan_kernel: one label per row, allocated in whole tiles (16-byte aligned)
    const int* qlab;      // grouped_scan_kernel: [nqt * TN] one label per query (LABEL_NONE: the query is not group-filtered)
    int grp_only;         // grouped_scan_kernel: 1 = only the rows of the query's group answer, 0 = every row but those
};

constexpr int LABEL_NONE = -2147483647 - 1; // MIPS_LABEL_NONE

// The group rule of mips_search_wide_grp / mips_range_search_grp: may a row labelled `lab` answer a query labelled `ql`?
__device__ __forceinline__ bool group_admits(int lab, int ql, int only) { return ql == LABEL_NONE || ((lab == ql) == (only != 0)); }

// SEL: the masked instance (masked_scan_kernel below).  p.sel holds four 32-bit words per tile (select_kernels.hpp): a tile whose
// words are all zero is never loaded, and a row whose bit is clear never passes the threshold test.
// GRP (with SEL): the grouped instance (grouped_scan_kernel).  A lane owns one query, so its label is one register; the labels of
// the sixteen rows of an accumulator block are four aligned 16-byte loads, made only for a block in which some lane passes the
// threshold, and a row is appended only if the group rule admits it for the lane's query.
template <bool SEL, bool GRP = false>
__device__ __forceinline__ void wide_scan_body(const WideScanArgs& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int h = lane >> 5;
    const int l31 = lane & 31;

    // blocks with equal (blockIdx & 7) share an XCD: all query tiles of one split run there, so the split's documents are
    // fetched from HBM once and served to the other query tiles from that XCD's L2
    const int xcd = blockIdx.x & 7;
    const int j = blockIdx.x >> 3;
    const int qt = j % p.nqt;
    const int split = xcd * (p.nsplit >> 3) + j / p.nqt;

    const int t0 = p.tile0 + split * p.tiles_per_split;
    int t1 = t0 + p.tiles_per_split;
    if (t1 > p.tile_end) t1 = p.tile_end;
    const int nt = t1 > t0 ? t1 - t0 : 0;

    const int q = qt * TN + wave * 32 + l31;
    const float tau = p.tau[q];
    int ql = 0;
    if constexpr (GRP) ql = p.qlab[q];
    const size_t segno = (size_t)q * (2 * p.nsplit) + 2 * split + h;
    wkey_t* myseg = p.seg + segno * p.segcap;
    int cur = 0;

    const int srow = tid >> 3;
    const int schunk = tid & 7;
    const int st_off = srow * 128 + ((schunk ^ ((srow >> 1) & 7)) << 4);
    const int rd_swz = (l31 >> 1) & 7;

    const uint16_t* qbase = p.qbuf + (int64_t)qt * TN * p.ld + schunk * 8 + (int64_t)srow * p.ld;
    const uint16_t* dbase = p.docs + schunk * 8 + (int64_t)srow * p.ld;
    const int64_t row32 = (int64_t)32 * p.ld;

    u32x4 ra[4], rb[4];
    auto gload = [&](int tile, int ks) {
        const uint16_t* a = dbase + (int64_t)tile * TM * p.ld + ks * BK;
        const uint16_t* b = qbase + ks * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = *reinterpret_cast<const u32x4*>(a + i * row32);
            rb[i] = *reinterpret_cast<const u32x4*>(b + i * row32);
        }
    };
    auto swrite = [&](int buf) {
        unsigned char* sa = smem + buf * ((TM + TN) * BK * 2);
        unsigned char* sb = sa + TM * BK * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<u32x4*>(sa + st_off + i * 32 * 128) = ra[i];
            *reinterpret_cast<u32x4*>(sb + st_off + i * 32 * 128) = rb[i];
        }
    };

    f32x16 acc[4];
    auto compute = [&](int buf) {
        const unsigned char* sa = smem + buf * ((TM + TN) * BK * 2);
        const unsigned char* sb = sa + TM * BK * 2;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int coff = ((2 * kk + h) ^ rd_swz) << 4;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(sb + (wave * 32 + l31) * 128 + coff);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(sa + (m * 32 + l31) * 128 + coff);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[m], 0, 0, 0);
            }
        }
    };

    // first tile at or after t that holds a selected row, or t1 (the words are wave-uniform: every wave walks the same tiles)
    auto next_tile = [&](int t) {
        if constexpr (SEL) {
            const u32x4* sel4 = reinterpret_cast<const u32x4*>(p.sel);
            while (t < t1) {
                const u32x4 w = sel4[t];
                if (__builtin_amdgcn_readfirstlane((int)(w[0] | w[1] | w[2] | w[3])) != 0) break;
                ++t;
            }
        }
        return t;
    };

    auto epilogue = [&](int tile) {
        const int base = tile * TM + 4 * h;
        if constexpr (SEL) { // rows past ntotal are clear bits of the staged words: no test of the ragged tile
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const unsigned wm = (unsigned)__builtin_amdgcn_readfirstlane((int)p.sel[4 * tile + m]);
                if (wm != 0xffffffffu) {
                    const unsigned ws = wm >> (4 * h);
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (((ws >> ((r & 3) + 8 * (r >> 2))) & 1u) == 0u) acc[m][r] = -INFINITY;
                }
            }
        } else if ((int64_t)(tile + 1) * TM > p.ntotal) { // ragged last tile: rows past ntotal never pass
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((int64_t)(base + m * 32 + (r & 3) + 8 * (r >> 2)) >= p.ntotal) acc[m][r] = -INFINITY;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float mx = acc[m][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[m][r]);
            if (__ballot(mx > tau) != 0ull) {
                unsigned adm = 0xffffu; // bit r: row r of the block may answer this lane's query
                if constexpr (GRP) {
                    const u32x4* lab4 = reinterpret_cast<const u32x4*>(p.rlab + (int64_t)base + m * 32);
                    adm = 0u;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const u32x4 lb = lab4[2 * g];
#pragma unroll
                        for (int c = 0; c < 4; ++c) adm |= group_admits((int)lb[c], ql, p.grp_only) ? 1u << (4 * g + c) : 0u;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = acc[m][r];
                    if (s > tau && (!GRP || ((adm >> r) & 1u) != 0u) && cur < p.segcap) {
                        myseg[cur] = wide_pack(thr_encode(s + 0.0f), base + m * 32 + (r & 3) + 8 * (r >> 2));
                        ++cur;
                    }
                }
            }
        }
    };

    if constexpr (SEL) {
        // the same flattened (tile, k-step) pipeline over the NON-EMPTY tiles of the split: the prefetch of the step after a
        // tile's last k-step addresses the next non-empty tile, and a split without one stores a zero counter and leaves
        int tile = next_tile(t0), ks = 0, buf = 0;
        if (tile < t1) gload(tile, 0);
        while (tile < t1) {
            swrite(buf);
            __syncthreads();
            int ntile = tile, nks = ks + 1;
            if (nks == p.ksteps) {
                nks = 0;
                ntile = next_tile(tile + 1);
            }
            if (ntile < t1) gload(ntile, nks);
            if (ks == 0) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
            }
            compute(buf);
            if (ks == p.ksteps - 1) epilogue(tile);
            tile = ntile;
            ks = nks;
            buf ^= 1;
        }
        p.cnt[segno] = cur;
        return;
    }
    const int total = nt * p.ksteps;
    if (total > 0) gload(t0, 0);
    int tile = t0, ks = 0;
    for (int step = 0; step < total; ++step) {
        const int buf = step & 1;
        swrite(buf);
        __syncthreads();
        int ntile = tile, nks = ks + 1;
        if (nks == p.ksteps) {
            nks = 0;
            ++ntile;
        }
        if (step + 1 < total) gload(ntile, nks);
        if (ks == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        }
        compute(buf);
        if (ks == p.ksteps - 1) epilogue(tile);
        tile = ntile;
        ks = nks;
    }
    p.cnt[segno] = cur;
}

__global__ __launch_bounds__(SCAN_THREADS, 2) void wide_scan_kernel(WideScanArgs p) { wide_scan_body<false>(p); }
// the instance of the filtered searches (its name stays outside the census of scan instances, tests/scan_recipes.py)
__global__ __launch_bounds__(SCAN_THREADS, 2) void masked_scan_kernel(WideScanArgs p) { wide_scan_body<true>(p); }
// the instance of the grouped searches (outside the census too): always reads staged selector words, all ones without a bitmap
__global__ __launch_bounds__(SCAN_THREADS, 2) void grouped_scan_kernel(WideScanArgs p) { wide_scan_body<true, true>(p); }

// ------------------------------------------------------------------------------------------------------------- select
// descending bitonic sort of buf[0 .. n) in LDS by the whole workgroup (n <= WIDE_BUF; pads with 0 = "no entry")
__device__ __forceinline__ void wide_sort_desc(wkey_t* buf, int n, int tid) {
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += WIDE_THREADS) buf[i] = 0ull;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += WIDE_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const wkey_t a = buf[i], b = buf[o];
                    const bool desc = (i & k2) == 0;
                    if (desc ? a < b : a > b) {
                        buf[i] = b;
                        buf[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

struct WideSelArgs {
    const wkey_t* seg; // [slots][nseg][segcap]
    int nseg, segcap;
    int* cnt;          // [slots][nseg]; cleared here once consumed
    wkey_t* pool;      // [slots][pool_stride]
    int pool_stride;
    int* pool_n;       // [slots]
    wkey_t* tau_c;     // [slots] entries must be > tau_c to matter
    float* tau_f;      // [slots] or nullptr: the scan's threshold (score of the k'-th entry, -inf while the pool is not full)
    int kp;            // entries kept
    const int* n_dev;  // or nullptr: slots slot0 + blockIdx.x >= *n_dev leave
    int slot0;
};

__global__ __launch_bounds__(WIDE_THREADS) void wide_select_kernel(WideSelArgs a) {
    __shared__ wkey_t buf[WIDE_BUF];
    __shared__ int off[WIDE_MAX_SEG + 1];
    __shared__ int fill_s;
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (a.n_dev != nullptr && a.slot0 + slot >= *a.n_dev) return;
    int c = tid < a.nseg ? a.cnt[(size_t)slot * a.nseg + tid] : 0;
    if (c > a.segcap) c = a.segcap;
    off[tid + 1] = c;
    if (tid == 0) off[0] = 0;
    __syncthreads();
    for (int d = 1; d < WIDE_THREADS; d <<= 1) { // inclusive scan
        const int v = tid >= d ? off[tid + 1 - d] : 0;
        __syncthreads();
        off[tid + 1] += v;
        __syncthreads();
    }
    const int total = off[WIDE_THREADS];
    if (total == 0) return;
    if (tid < a.nseg) a.cnt[(size_t)slot * a.nseg + tid] = 0;
    const wkey_t* segs = a.seg + (size_t)slot * a.nseg * a.segcap;
    wkey_t* pool = a.pool + (size_t)slot * a.pool_stride;
    int fill = a.pool_n[slot];
    if (fill > a.kp) fill = a.kp;
    wkey_t tau = a.tau_c[slot];
    for (int i = tid; i < fill; i += WIDE_THREADS) buf[i] = pool[i];
    if (tid == 0) fill_s = fill;
    constexpr int BATCH = WIDE_BUF - WIDE_POOL;
    for (int v0 = 0; v0 < total; v0 += BATCH) {
        __syncthreads();
        const int v1 = v0 + BATCH < total ? v0 + BATCH : total;
        for (int v = v0 + tid; v < v1; v += WIDE_THREADS) {
            int lo = 0, hi = a.nseg; // the segment holding flat position v: largest s with off[s] <= v
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= v) lo = mid;
                else hi = mid;
            }
            const wkey_t e = segs[(size_t)lo * a.segcap + (v - off[lo])];
            if (e > tau) {
                const int pos = atomicAdd(&fill_s, 1);
                if (pos < WIDE_BUF) buf[pos] = e;
            }
        }
        __syncthreads();
        fill = fill_s < WIDE_BUF ? fill_s : WIDE_BUF;
        __syncthreads();
        if (fill >= a.kp) {
            wide_sort_desc(buf, fill, tid);
            fill = a.kp;
            tau = buf[a.kp - 1];
            if (tid == 0) fill_s = fill;
        }
    }
    __syncthreads();
    for (int i = tid; i < fill; i += WIDE_THREADS) pool[i] = buf[i];
    if (tid == 0) {
        a.pool_n[slot] = fill;
        a.tau_c[slot] = tau;
        if (a.tau_f != nullptr) a.tau_f[slot] = fill >= a.kp ? thr_decode(wide_hi(tau)) : -INFINITY;
    }
}

// per query slice: empty pools, thresholds that pass everything (pad queries: nothing)
__global__ void wide_init_kernel(int nq, int nq_pad, int* pool_n, wkey_t* tau_c, float* tau_f) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    pool_n[q] = 0;
    tau_c[q] = 0ull;
    tau_f[q] = q < nq ? -INFINITY : INFINITY;
}

// ------------------------------------------------------------------------------------------- exact re-score, rank, certificate
// One result slot: the plain pair of arrays, or the packed all-gather payload [nq][k][2] = {float32 bits (zero-extended), id}.
__device__ __forceinline__ void wide_write(float* out_s, int64_t* out_i, int64_t* out_packed, size_t o, float s, int64_t id) {
    if (out_packed) {
        out_packed[2 * o] = (int64_t)__float_as_uint(s);
        out_packed[2 * o + 1] = id;
    } else {
        out_s[o] = s;
        out_i[o] = id;
    }
}

struct WideRescoreArgs {
    const wkey_t* pool;
    int pool_stride;
    const int* pool_n;
    int kp;
    const void* rows;  // canonical rows (bf16 index rows / fp32 rows), pitch ld
    const void* y;     // canonical staged queries, pitch ld
    int ld;
    int64_t ntotal;
    int k;
    double phi;
    int64_t idx_offset;
    float* out_s;      // [nq][k]
    int64_t* out_i;
    int64_t* out_packed; // or [nq][k][2] (MIPS_OUT_PACKED)
    unsigned char* flag; // [nq]
    unsigned* nflag;     // running count of flagged queries of the call
    double* qq;          // [nq] out: |q|^2 as the canonical sum
    wkey_t* seed;        // [nq] out: the k-th result as an exact entry (0: fewer than k results)
    const double* xmax2;
    const double* dres2; // fp32-exact index (with qerr2), else nullptr
    const double* qerr2;
    double err_c;
    const unsigned long long* nsel; // SEL: number of selected rows (select_kernels.hpp), a device word
};

// SEL: a filtered search.  The rows that can be results are the nsel selected ones, so the two uses of ntotal in the certificate
// read that count instead.
// GRP: a grouped search.  The rows admitted for a query are not counted anywhere.  A pool short of k' entries IS the query's whole
// admitted set (wide_select_kernel keeps tau_f at -inf until a pool holds k' entries, and under -inf the scan appends every
// admitted row), so such a query is certified outright; a full pool takes the bound check whatever lies outside it.
template <typename EL, bool L2, bool SEL = false, bool GRP = false>
__global__ __launch_bounds__(WIDE_THREADS) void wide_rescore_kernel(WideRescoreArgs a) {
    __shared__ double yd[1024];
    __shared__ double dd[WIDE_POOL];
    __shared__ wkey_t buf[WIDE_POOL];
    __shared__ unsigned minhi_s;
    __shared__ double qq_s;
    constexpr int PER = EL::PER16;
    const int q = blockIdx.x, tid = threadIdx.x;
    int n = a.pool_n[q];
    if (n > a.kp) n = a.kp;
    const typename EL::type* ys = reinterpret_cast<const typename EL::type*>(a.y) + (size_t)q * a.ld;
    const int nchunk = a.ld / PER;
    for (int c = tid; c < nchunk; c += WIDE_THREADS) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ys + (size_t)c * PER);
#pragma unroll
        for (int e = 0; e < PER; ++e) yd[c * PER + e] = (double)EL::get(v, e);
    }
    if (tid == 0) minhi_s = 0xffffffffu;
    __syncthreads();
    if (tid == WIDE_THREADS - 1) { // |q|^2, sequential in the column index like the dot products
        double s = 0.0;
        for (int c = 0; c < a.ld; ++c) s += yd[c] * yd[c];
        qq_s = s;
    }
    const wkey_t* pool = a.pool + (size_t)q * a.pool_stride;
    unsigned mh = 0xffffffffu;
    for (int i = tid; i < n; i += WIDE_THREADS) {
        const wkey_t c = pool[i];
        const unsigned hi = wide_hi(c);
        mh = hi < mh ? hi : mh;
        const typename EL::type* x = reinterpret_cast<const typename EL::type*>(a.rows) + (size_t)wide_row(c) * a.ld;
        double dot = 0.0;
        for (int c0 = 0; c0 < nchunk; c0 += 8) { // (nchunk is a multiple of 8: rows are whole 128-byte segments)
            u32x4 v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = *reinterpret_cast<const u32x4*>(x + (size_t)(c0 + t) * PER);
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int e = 0; e < PER; ++e) dot += (double)EL::get(v[t], e) * yd[(c0 + t) * PER + e]; // sequential in the column index
        }
        dd[i] = dot;
    }
    if (mh != 0xffffffffu) atomicMin(&minhi_s, mh);
    __syncthreads();
    const double qq = qq_s;
    for (int i = tid; i < n; i += WIDE_THREADS) {
        const float outv = L2 ? (float)(qq + a.phi - 2.0 * dd[i]) : (float)dd[i];
        buf[i] = wide_pack(wide_enc<L2>(outv), wide_row(pool[i]));
    }
    __syncthreads();
    if (n > 1) wide_sort_desc(buf, n, tid);
    __syncthreads();
    for (int i = tid; i < a.k; i += WIDE_THREADS) {
        const size_t o = (size_t)q * a.k + i;
        if (i < n) wide_write(a.out_s, a.out_i, a.out_packed, o, wide_dec<L2>(wide_hi(buf[i])), (int64_t)wide_row(buf[i]) + a.idx_offset);
        else wide_write(a.out_s, a.out_i, a.out_packed, o, L2 ? INFINITY : -INFINITY, -1);
    }
    if (tid == 0) {
        // Certificate.  Every row outside the pool has an approximate score <= B = the score of the pool's worst member, so a
        // canonical dot <= ub = B + e; the canonical key is a monotone function of the dot, so its key is no better than
        // key(ub).  Only if that is STRICTLY worse than the k-th result's key can no such row enter the top k (an equal float32
        // key could still win on the row number).
        const int64_t nrows = SEL ? (int64_t)*a.nsel : a.ntotal;
        const int64_t need = nrows < (int64_t)a.kp ? nrows : (int64_t)a.kp;
        bool fl = false;
        if (GRP ? false : (int64_t)n < need) {
            fl = true;
        } else if (GRP ? n >= a.kp : nrows > (int64_t)n) {
            const double B = (double)thr_decode(minhi_s);
            const double qn = sqrt(qq), xm = sqrt(*a.xmax2);
            double e = a.err_c * qn * xm;
            if (a.qerr2 != nullptr) {
                const double dr = sqrt(*a.dres2);
                e += dr * qn + (xm + dr) * sqrt(a.qerr2[q]);
            }
            const double ub = B + e * 1.000000001 + 1e-300;
            const float outk = wide_dec<L2>(wide_hi(buf[a.k - 1]));
            if (L2) fl = !((float)(qq + a.phi - 2.0 * ub) > outk);
            else fl = !((float)ub < outk);
        }
        a.qq[q] = qq;
        a.seed[q] = n >= a.k ? buf[a.k - 1] : 0ull;
        a.flag[q] = fl ? 1 : 0;
        if (fl) atomicAdd(a.nflag, 1u);
    }
}

// ------------------------------------------------------------------------------------------------- exact settlement
struct WideExactArgs {
    const void* rows;  // canonical rows, pitch ld
    const void* y;     // canonical staged queries of the slice, pitch ld
    int ld;
    int64_t ntotal;
    int64_t r0, r1;    // rows of this chunk
    const int* ids;    // flagged query numbers, ascending
    const int* n_dev;  // their count
    int slot0, nslots; // this round settles flagged positions slot0 .. slot0 + nslots - 1 (slot = position - slot0)
    const double* qq;  // [nq]
    double phi;
    const wkey_t* seed; // [nq]
    wkey_t* tau_c;     // [slots]
    int* pool_n;       // [slots]
    wkey_t* pool;
    int pool_stride;
    wkey_t* seg;       // [slots][segcap]
    int segcap;
    int* cnt;          // [slots]
    int k;
    int64_t idx_offset;
    float* out_s;
    int64_t* out_i;
    int64_t* out_packed;
    const unsigned* sel; // SEL: staged selector words (bit r & 31 of word r >> 5 = local row r), zero past ntotal
    const int* rlab;     // GRP: one label per row
    const int* qlab;     // GRP: one label per query of the slice (indexed like y)
    int grp_only;        // GRP: 1 = only mode, 0 = exclude mode
};

// start of a round: empty pools; a row must reach the k-th result of the first pass to matter
__global__ void wide_exact_init_kernel(WideExactArgs a) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.nslots || a.slot0 + slot >= *a.n_dev) return;
    const wkey_t s = a.seed[a.ids[a.slot0 + slot]];
    a.pool_n[slot] = 0;
    a.tau_c[slot] = s != 0ull ? s - 1ull : 0ull;
    a.cnt[slot] = 0;
}

// SEL: a filtered search.  An unselected row is never appended (the settlement must not bring back what the scan left out), and a
// wave's 64 rows are not scored at all when none of them is selected.
// GRP (with SEL): a grouped search.  Each of the RESOLVE_QB queries of a pass has its own label, so the group rule is tested per
// (query, row) next to the threshold; the wave-level skip stays on the bitmap alone.
template <typename EL, bool L2, bool SEL = false, bool GRP = false>
__global__ __launch_bounds__(64 * RESOLVE_WAVES) void wide_exact_kernel(WideExactArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = *a.n_dev;
    if (a.slot0 >= n) return;
    const int jend = n < a.slot0 + a.nslots ? n : a.slot0 + a.nslots;
    constexpr int TCH = 8;
    constexpr int PER = EL::PER16;
    double* yd = reinterpret_cast<double*>(smem);                             // [RESOLVE_QB][ld]
    unsigned char* tiles = smem + (size_t)RESOLVE_QB * a.ld * sizeof(double); // [waves][64 rows][TCH + 1 chunks]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32x4* tile = reinterpret_cast<u32x4*>(tiles) + wave * 64 * (TCH + 1);
    const typename EL::type* rows = reinterpret_cast<const typename EL::type*>(a.rows);
    const typename EL::type* ys = reinterpret_cast<const typename EL::type*>(a.y);
    const int nchunk = a.ld / PER;
    for (int j0 = a.slot0; j0 < jend; j0 += RESOLVE_QB) {
        __syncthreads();
        for (int t = tid; t < RESOLVE_QB * nchunk; t += 64 * RESOLVE_WAVES) {
            const int j = t / nchunk, c = t % nchunk;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (j0 + j < jend) v = *reinterpret_cast<const u32x4*>(ys + (size_t)a.ids[j0 + j] * a.ld + (size_t)c * PER);
#pragma unroll
            for (int e = 0; e < PER; ++e) yd[(size_t)j * a.ld + c * PER + e] = j0 + j < jend ? (double)EL::get(v, e) : 0.0;
        }
        __syncthreads();
        wkey_t tau[RESOLVE_QB];
        double qn[RESOLVE_QB];
        int ql[RESOLVE_QB];
#pragma unroll
        for (int j = 0; j < RESOLVE_QB; ++j) {
            const bool on = j0 + j < jend;
            tau[j] = on ? a.tau_c[j0 + j - a.slot0] : ~0ull;
            qn[j] = on && L2 ? a.qq[a.ids[j0 + j]] : 0.0;
            ql[j] = LABEL_NONE;
            if constexpr (GRP) ql[j] = on ? a.qlab[a.ids[j0 + j]] : LABEL_NONE;
        }
        for (int64_t r0 = a.r0 + ((int64_t)blockIdx.x * RESOLVE_WAVES + wave) * 64; r0 < a.r1; r0 += (int64_t)gridDim.x * 64 * RESOLVE_WAVES) {
            const int64_t row = r0 + lane;
            bool on = true;
            if constexpr (SEL) {
                on = row < a.r1 && ((a.sel[row >> 5] >> (int)(row & 31)) & 1u) != 0u;
                if (__ballot(on) == 0ull) continue;
            }
            double acc[RESOLVE_QB];
            exact_dots<EL>(rows, a.ld, a.ntotal, r0, lane, tile, yd, acc);
            if (row < a.r1 && on) {
                int lab = 0;
                if constexpr (GRP) lab = a.rlab[row];
#pragma unroll
                for (int j = 0; j < RESOLVE_QB; ++j) {
                    const float outv = L2 ? (float)(qn[j] + a.phi - 2.0 * acc[j]) : (float)acc[j];
                    const wkey_t c = wide_pack(wide_enc<L2>(outv), (int)row);
                    if ((!GRP || group_admits(lab, ql[j], a.grp_only)) && c > tau[j]) {
                        const int slot = j0 + j - a.slot0;
                        const int pos = atomicAdd(&a.cnt[slot], 1);
                        if (pos < a.segcap) a.seg[(size_t)slot * a.segcap + pos] = c;
                    }
                }
            }
        }
    }
}

// end of a round: the slot's pool is the query's exact top k
template <bool L2>
__global__ __launch_bounds__(WIDE_THREADS) void wide_finalize_kernel(WideExactArgs a) {
    __shared__ wkey_t buf[WIDE_POOL];
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (a.slot0 + slot >= *a.n_dev) return;
    const int q = a.ids[a.slot0 + slot];
    int n = a.pool_n[slot];
    if (n > a.k) n = a.k;
    const wkey_t* pool = a.pool + (size_t)slot * a.pool_stride;
    for (int i = tid; i < n; i += WIDE_THREADS) buf[i] = pool[i];
    __syncthreads();
    if (n > 1) wide_sort_desc(buf, n, tid);
    __syncthreads();
    for (int i = tid; i < a.k; i += WIDE_THREADS) {
        const size_t o = (size_t)q * a.k + i;
        if (i < n) wide_write(a.out_s, a.out_i, a.out_packed, o, wide_dec<L2>(wide_hi(buf[i])), (int64_t)wide_row(buf[i]) + a.idx_offset);
        else wide_write(a.out_s, a.out_i, a.out_packed, o, L2 ? INFINITY : -INFINITY, -1);
    }
}

} // namespace mips
