// Kernels of the IVF index (include/mips_hip_ivf.h): what builds an inverted file over the rows of a flat index.
//
//   list table     ivf_hist_kernel / ivf_offsets_kernel / ivf_list_fill_kernel: list_offsets [nlist + 1] and list_rows [n] from the
//                  rows' list numbers, ascending inside each list.  Counting (integer atomics: the sums do not depend on their
//                  order), one workgroup's scan, then one wave per list that walks the assignments 64 rows at a time and compacts
//                  its members by ballot and popcount.  No workgroup waits for another.
//   training       ivf_gather_rows_kernel (the training set as float32), ivf_finite_kernel, ivf_init_centroids_kernel,
//                  ivf_centroid_sum_kernel (one thread per (list, column): sequential fp64 sum of the members in ascending row
//                  order), ivf_normalise_kernel (one thread per list).  The arithmetic is csrc/ivf_math.hpp.
// The scan of the probed lists: ivf_search_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "ivf_math.hpp"

namespace mips {

constexpr int IVF_SCAN_THREADS = 1024; // the one workgroup of a scan over the lists
constexpr int IVF_MAX_PROBE = 1024;

// ---------------------------------------------------------------------------------------------------------------- list table
__global__ void ivf_to_assign_kernel(const int64_t* idx, int64_t n, int nlist, int* assign) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = idx[t];
        assign[t] = l >= 0 && l < nlist ? (int)l : -1;
    }
}

// count zeroed by the host
__global__ void ivf_hist_kernel(const int* assign, int64_t n, int nlist, int* count) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int l = assign[t];
        if (l >= 0 && l < nlist) atomicAdd(&count[l], 1);
    }
}

// one workgroup: thread t owns the lists [t per, (t + 1) per)
__global__ __launch_bounds__(IVF_SCAN_THREADS) void ivf_offsets_kernel(const int* count, int nlist, int* offsets) {
    __shared__ int part[IVF_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (nlist + IVF_SCAN_THREADS - 1) / IVF_SCAN_THREADS;
    const int l0 = t * per < nlist ? t * per : nlist;
    const int l1 = l0 + per < nlist ? l0 + per : nlist;
    int s = 0;
    for (int l = l0; l < l1; ++l) s += count[l];
    part[t] = s;
    __syncthreads();
    int base = 0;
    for (int u = 0; u < t; ++u) base += part[u];
    for (int l = l0; l < l1; ++l) {
        offsets[l] = base;
        base += count[l];
    }
    if (t == IVF_SCAN_THREADS - 1) offsets[nlist] = base;
}

// one wave per list
__global__ __launch_bounds__(256) void ivf_list_fill_kernel(const int* assign, int64_t n, int nlist, const int* offsets, int* list_rows) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= nlist) return;
    int pos = offsets[l];
    const int end = offsets[l + 1];
    if (pos == end) return;
    for (int64_t r0 = 0; r0 < n; r0 += 64) {
        const int64_t r = r0 + lane;
        const bool m = r < n && assign[r] == l;
        const unsigned long long b = __ballot(m);
        const int at = pos + __popcll(b & ((1ull << lane) - 1ull));
        if (m && at < end) list_rows[at] = (int)r;
        pos += __popcll(b);
    }
}

// ------------------------------------------------------------------------------------------------------------------ training
template <typename T>
__device__ __forceinline__ float ivf_widen(T v);
template <>
__device__ __forceinline__ float ivf_widen<float>(float v) { return v; }
template <>
__device__ __forceinline__ float ivf_widen<uint16_t>(uint16_t v) { return bf16_bits_to_f32(v); }

// out [m][d] float32: row i = x[floor(i n / m)]
template <typename T>
__global__ void ivf_gather_rows_kernel(const T* x, int64_t n, int64_t m, int d, float* out) {
    const int64_t total = m * d;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / d;
        const int j = (int)(t - i * d);
        out[t] = ivf_widen<T>(x[(size_t)ivf::pick(i, n, m) * d + j]);
    }
}

// *flag = 1 if a value is NaN or infinite (flag zeroed by the host)
template <typename T>
__global__ void ivf_finite_kernel(const T* x, int64_t total, int* flag) {
    bool bad = false;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const float v = ivf_widen<T>(x[t]);
        bad = bad || !(fabsf(v) < INFINITY);
    }
    if (bad) atomicOr(flag, 1);
}

// c_l = normalise(T[floor(l m / nlist)])
__global__ void ivf_init_centroids_kernel(const float* T, int64_t m, int d, int nlist, float* cent) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlist) return;
    const float* src = T + (size_t)ivf::pick(l, m, nlist) * d;
    float* c = cent + (size_t)l * d;
    for (int j = 0; j < d; ++j) c[j] = src[j];
    ivf::normalise(c, d);
}

// one thread per (list, column); a list without members keeps its centroid
__global__ void ivf_centroid_sum_kernel(const float* T, int d, const int* offsets, const int* list_rows, int nlist, float* cent) {
    const int64_t total = (int64_t)nlist * d;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(t / d);
        const int j = (int)(t - (int64_t)l * d);
        const int beg = offsets[l], end = offsets[l + 1];
        if (end == beg) continue;
        double s = 0.0;
        for (int u = beg; u < end; ++u) s += (double)T[(size_t)list_rows[u] * d + j]; // ascending rows
        cent[t] = ivf::mean(s, end - beg);
    }
}

__global__ void ivf_normalise_kernel(float* cent, int d, const int* offsets, int nlist) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlist || offsets[l + 1] == offsets[l]) return;
    ivf::normalise(cent + (size_t)l * d, d);
}

} // namespace mips
