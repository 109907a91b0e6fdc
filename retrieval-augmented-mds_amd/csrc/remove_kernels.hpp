// Row removal (mips_index_remove): an in-place, order-preserving compaction of the stored rows, one window of W rows per launch
// (remove_plan.hpp says which window goes where and why no workgroup ever waits for another).
//
//   remove_stage_kernel          the caller's REMOVAL bitmap (the layout of select_kernels.hpp) becomes KEEP words: keep[w] bit b = 1
//                                iff local row 32 w + b exists and is not removed.  One workgroup per window (W = 32 * wwords rows);
//                                it also writes kept[window], the window's surviving rows, and adds the survivors among the rows
//                                below `nlabelled` to *lab_kept (zeroed before the launch).
//   remove_gather_kernel         one window of an array of 16-byte chunks (cpr per row).  Workgroup x takes a tile of 128 source rows:
//                                it counts the survivors of the window's tiles before its own (prefix), ranks its own survivors in
//                                LDS, and then moves them as ONE contiguous run of destination chunks -- lane l of an instruction
//                                stores chunk c + l, so a wave's store is 1 KiB of consecutive destination bytes and its load the
//                                same bytes of whole source rows (one or two rows from a 1 KiB pitch on, eight full 128-byte rows
//                                at the smallest pitch), never one row per lane.  Workgroup y takes a segment of `seg` chunks of
//                                every row (long rows).  dst is where the window's FIRST survivor goes: its home, or a bounce buffer.
//   remove_gather_labels_kernel  the same for the one int32 label of a row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select_kernels.hpp"

namespace mips {

constexpr int REM_THREADS = 256;
constexpr int REM_TILE = 128;   // source rows per workgroup: four keep words
constexpr int REM_UNROLL = 8;   // 16-byte loads a lane has in flight
typedef unsigned rem_u4 __attribute__((ext_vector_type(4))); // 16 bytes, one dwordx4 load or store

__global__ __launch_bounds__(REM_THREADS) void remove_stage_kernel(const uint8_t* bits, int64_t nbytes, int64_t bit0, int64_t ntotal, int64_t nlabelled,
                                                                   int wwords, unsigned* keep, int* kept, int64_t nwindows,
                                                                   unsigned long long* lab_kept) {
    __shared__ int s_sum[2][REM_THREADS / 64];
    for (int64_t win = blockIdx.x; win < nwindows; win += gridDim.x) {
        int mine = 0, lab = 0;
        const int64_t w0 = win * wwords;
        for (int i = threadIdx.x; i < wwords; i += REM_THREADS) {
            const int64_t w = w0 + i;
            const int64_t left = ntotal - 32 * w, left_lab = nlabelled - 32 * w;
            const unsigned exist = left >= 32 ? ~0u : left > 0 ? (1u << (int)left) - 1u : 0u;
            const unsigned v = ~selector_word(bits, nbytes, bit0, ntotal, w) & exist;
            keep[w] = v;
            mine += __popc(v);
            lab += __popc(left_lab >= 32 ? v : left_lab > 0 ? v & ((1u << (int)left_lab) - 1u) : 0u);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mine += __shfl_xor(mine, o);
            lab += __shfl_xor(lab, o);
        }
        if ((threadIdx.x & 63) == 0) {
            s_sum[0][threadIdx.x >> 6] = mine;
            s_sum[1][threadIdx.x >> 6] = lab;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int k = 0, l = 0;
#pragma unroll
            for (int i = 0; i < REM_THREADS / 64; ++i) {
                k += s_sum[0][i];
                l += s_sum[1][i];
            }
            kept[win] = k;
            if (l != 0) atomicAdd(lab_kept, (unsigned long long)l);
        }
        __syncthreads();
    }
}

// keep word w restricted to the rows below nvalid (the labels are compacted over the labelled prefix only)
__device__ inline unsigned keep_word(const unsigned* keep, int64_t w, int64_t nvalid) {
    const int64_t left = nvalid - 32 * w;
    if (left <= 0) return 0u;
    const unsigned v = keep[w];
    return left < 32 ? v & ((1u << (int)left) - 1u) : v;
}

// For tile `tile` of the window that starts at row0 (a multiple of 128): `prefix` = survivors of the window's tiles before it,
// `kept` = its own survivors, s_src[r] = the tile-local source row of its r-th survivor.  Ends with a barrier.
__device__ inline void tile_ranks(const unsigned* keep, int64_t row0, int tile, int64_t nvalid, unsigned short* s_src, int* s_red, int& prefix,
                                  int& kept) {
    const int64_t w0 = row0 >> 5;
    int mine = 0;
    for (int i = threadIdx.x; i < tile * (REM_TILE / 32); i += REM_THREADS) mine += __popc(keep_word(keep, w0 + i, nvalid));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mine;
    const int64_t tw = w0 + (int64_t)tile * (REM_TILE / 32);
    const unsigned k0 = keep_word(keep, tw, nvalid), k1 = keep_word(keep, tw + 1, nvalid), k2 = keep_word(keep, tw + 2, nvalid),
                   k3 = keep_word(keep, tw + 3, nvalid);
    const int p0 = __popc(k0), p1 = __popc(k1), p2 = __popc(k2), p3 = __popc(k3);
    if (threadIdx.x < REM_TILE) {
        const int j = threadIdx.x >> 5, b = threadIdx.x & 31;
        const unsigned wd = j == 0 ? k0 : j == 1 ? k1 : j == 2 ? k2 : k3;
        if ((wd >> b) & 1u) {
            const int before = (j > 0 ? p0 : 0) + (j > 1 ? p1 : 0) + (j > 2 ? p2 : 0);
            s_src[before + __popc(wd & ((1u << b) - 1u))] = (unsigned short)threadIdx.x;
        }
    }
    __syncthreads();
    prefix = 0;
#pragma unroll
    for (int i = 0; i < REM_THREADS / 64; ++i) prefix += s_red[i];
    kept = p0 + p1 + p2 + p3;
}

// src: row 0 of the array; grid.x = the 128-row tiles of the window; dst: where the window's first survivor goes
__global__ __launch_bounds__(REM_THREADS) void remove_gather_kernel(const unsigned* keep, int64_t row0, int64_t nvalid, const rem_u4* src, rem_u4* dst,
                                                                    int cpr, int seg) {
    __shared__ unsigned short s_src[REM_TILE];
    __shared__ int s_red[REM_THREADS / 64];
    int prefix, kept;
    tile_ranks(keep, row0, (int)blockIdx.x, nvalid, s_src, s_red, prefix, kept);
    const int c0 = (int)blockIdx.y * seg;
    const int ncol = min(seg, cpr - c0);
    const int total = kept * ncol; // <= 128 * seg chunks
    const rem_u4* s = src + ((row0 + (int64_t)blockIdx.x * REM_TILE) * cpr + c0);
    rem_u4* d = dst + ((int64_t)prefix * cpr + c0);
    int c = threadIdx.x;
    for (; c + (REM_UNROLL - 1) * REM_THREADS < total; c += REM_UNROLL * REM_THREADS) { // every load issued before the first store
        rem_u4 v[REM_UNROLL];
        int64_t to[REM_UNROLL];
#pragma unroll
        for (int u = 0; u < REM_UNROLL; ++u) {
            const int cc = c + u * REM_THREADS;
            const int r = cc / ncol, col = cc - r * ncol;
            v[u] = s[(int64_t)s_src[r] * cpr + col];
            to[u] = (int64_t)r * cpr + col;
        }
#pragma unroll
        for (int u = 0; u < REM_UNROLL; ++u) d[to[u]] = v[u];
    }
    for (; c < total; c += REM_THREADS) {
        const int r = c / ncol, col = c - r * ncol;
        d[(int64_t)r * cpr + col] = s[(int64_t)s_src[r] * cpr + col];
    }
}

__global__ __launch_bounds__(REM_THREADS) void remove_gather_labels_kernel(const unsigned* keep, int64_t row0, int64_t nvalid, const int* src, int* dst) {
    __shared__ unsigned short s_src[REM_TILE];
    __shared__ int s_red[REM_THREADS / 64];
    int prefix, kept;
    tile_ranks(keep, row0, (int)blockIdx.x, nvalid, s_src, s_red, prefix, kept);
    if ((int)threadIdx.x < kept) dst[prefix + threadIdx.x] = src[row0 + (int64_t)blockIdx.x * REM_TILE + s_src[threadIdx.x]];
}

} // namespace mips
