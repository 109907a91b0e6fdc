// Rows overwritten in place by id (include/mips_hip_write.h; DESIGN.md, "Updating rows").  Three launches, each O(n) in the
// positions of the call and none in the rows of the index; no grid, pointer or loop bound depends on the VALUE of an id.
//
//   update_mark_kernel     pass A, one thread per position: owner[row] = max(owner[row], p) for every position p whose id names a
//                          row (upd::local_row).  An integer maximum: whatever order the atomics land in, owner[row] ends as the
//                          HIGHEST position that names the row -- the one the sequential loop of assignments leaves standing.
//   update_scatter_kernel  pass B, one WAVE per position: the wave of the owner converts x[p] and stores it over the row, 16 bytes
//                          per lane and store (plain vector stores); every other wave leaves.  Element by element the conversion
//                          is the text of the kernels behind mips_index_add (convert_rows_kernel, convert_rows_f8_kernel,
//                          split_rows_kernel's split_hi_lo, sq8_encode_rows_kernel's sq8::encode), so a row comes out
//                          byte-identical to an added one, padding columns included.  An fp32-exact index gets its [hi | lo]
//                          planes, the fp32 original and -- for rows below hi_rows, where the bf16 image of the two-stage search
//                          already exists -- the image's row.
//   update_finish_kernel   pass C, one thread per position: the owner folds |x|^2 (and |x - bf16 x|^2) of the STORED row into
//                          the index's row-norm bounds with the 64-bit atomicMax of row_sumsq_max_kernel, counts itself, hands
//                          an int32 that travels with the row (the IVF index: its list) to aux_dst[row], and puts owner[row] back
//                          to -1.  A loser p' < p of the same row reads owner[row] = p or -1, neither is p': no order needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "sq8_quant.hpp"
#include "update_math.hpp"

namespace mips {

constexpr int UPD_THREADS = 256;
constexpr int UPD_WAVES = UPD_THREADS / 64;

enum { UPD_BF16 = 0, UPD_F32X = 1, UPD_F8 = 2, UPD_SQ8 = 3 }; // the storage a scatter writes

struct UpdateArgs {
    const int64_t* ids; // [n]
    int n;
    int64_t idx_offset, ntotal;
    int* owner;         // [>= ntotal], -1 outside a call
    const void* src;    // [n][d] of the source type
    int d;
    uint8_t* rows;      // the index rows, pitch ld elements
    int ld;
    float* rows_f32;    // fp32-exact index: the originals at pitch plane, and the bf16 image at pitch hp up to hi_rows
    int plane;
    uint16_t* rows_hi;
    int hp;
    int64_t hi_rows;
    const float* sq8_params; // [vmin | vdiff | ...], ld floats each
};

__global__ __launch_bounds__(UPD_THREADS) void update_mark_kernel(const int64_t* __restrict__ ids, int n, int64_t idx_offset, int64_t ntotal, int* owner) {
    for (int64_t p = blockIdx.x * (int64_t)UPD_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * UPD_THREADS) {
        const int64_t row = upd::local_row(ids[p], idx_offset, ntotal);
        if (row >= 0) atomicMax(&owner[row], (int)p); // upd::fold_owner, atomically
    }
}

// the source element at column c as the float32 it stands for (bf16 bits: the exact up-cast)
template <typename SRC>
__device__ __forceinline__ float upd_value(const SRC* s, int c) {
    if constexpr (sizeof(SRC) == 4) return ((const float*)s)[c];
    else return bf16_bits_to_f32(((const uint16_t*)s)[c]);
}

template <typename SRC, int STORE>
__global__ __launch_bounds__(UPD_THREADS) void update_scatter_kernel(UpdateArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t p = blockIdx.x * (int64_t)UPD_WAVES + (threadIdx.x >> 6); p < a.n; p += (int64_t)gridDim.x * UPD_WAVES) {
        const int64_t row = upd::local_row(a.ids[p], a.idx_offset, a.ntotal);
        if (row < 0 || !upd::wins(a.owner[row], (int)p)) continue; // (the same for every lane of the wave)
        const SRC* s = reinterpret_cast<const SRC*>(a.src) + (size_t)p * a.d;
        if constexpr (STORE == UPD_BF16) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(a.rows) + (size_t)row * a.ld;
            for (int c0 = lane * 8; c0 < a.ld; c0 += 64 * 8) {
                uint16_t v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = c0 + e;
                    if (c < a.d) {
                        if constexpr (sizeof(SRC) == 4) v[e] = f32_to_bf16_rne(((const float*)s)[c]);
                        else v[e] = ((const uint16_t*)s)[c];
                    } else {
                        v[e] = 0;
                    }
                }
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = v[2 * e] | ((uint32_t)v[2 * e + 1] << 16);
                *reinterpret_cast<u32x4*>(dst + c0) = o;
            }
        } else if constexpr (STORE == UPD_F32X) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(a.rows) + (size_t)row * 2 * a.plane;
            float* keep = a.rows_f32 + (size_t)row * a.plane;
            const bool image = row < a.hi_rows;
            uint16_t* img = a.rows_hi + (image ? (size_t)row * a.hp : 0);
            const int width = image && a.hp > a.plane ? a.hp : a.plane; // (the image's columns >= plane are zero, as ensure_hi writes them)
            for (int c0 = lane * 8; c0 < width; c0 += 64 * 8) {
                u32x4 oh = {0u, 0u, 0u, 0u}, ol = {0u, 0u, 0u, 0u}, k0 = {0u, 0u, 0u, 0u}, k1 = {0u, 0u, 0u, 0u};
                if (c0 < a.plane) {
                    uint16_t hi[8], lo[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int c = c0 + e;
                        const float x = c < a.d ? upd_value(s, c) : 0.f;
                        split_hi_lo(x, hi[e], lo[e]);
                        if (e < 4) k0[e & 3] = __float_as_uint(x);
                        else k1[e & 3] = __float_as_uint(x);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        oh[e] = hi[2 * e] | ((uint32_t)hi[2 * e + 1] << 16);
                        ol[e] = lo[2 * e] | ((uint32_t)lo[2 * e + 1] << 16);
                    }
                    *reinterpret_cast<u32x4*>(dst + c0) = oh;
                    *reinterpret_cast<u32x4*>(dst + a.plane + c0) = ol;
                    *reinterpret_cast<u32x4*>(keep + c0) = k0;
                    *reinterpret_cast<u32x4*>(keep + c0 + 4) = k1;
                }
                if (image && c0 < a.hp) *reinterpret_cast<u32x4*>(img + c0) = oh; // bf16(x): what convert_rows_kernel makes of the fp32 row
            }
        } else {
            uint8_t* dst = a.rows + (size_t)row * a.ld;
            for (int c0 = lane * 16; c0 < a.ld; c0 += 64 * 16) {
                u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int c = c0 + e;
                    uint32_t b = 0;
                    if (c < a.d) {
                        if constexpr (sizeof(SRC) == 1) b = ((const uint8_t*)s)[c]; // raw e4m3 bytes / raw codes
                        else if constexpr (STORE == UPD_F8) b = f32_to_e4m3(upd_value(s, c));
                        else b = sq8::encode(upd_value(s, c), a.sq8_params[c], a.sq8_params[a.ld + c]);
                    }
                    o[e >> 2] |= b << ((e & 3) * 8);
                }
                *reinterpret_cast<u32x4*>(dst + c0) = o;
            }
        }
    }
}

struct UpdateFinishArgs {
    const int64_t* ids;
    int n;
    int64_t idx_offset, ntotal;
    int* owner;
    const void* canon;  // the rows the norm bound speaks about (ensure_xmax2), pitch cld elements
    int cld;
    unsigned long long* xmax2; // NULL: the bound is not valid, nothing to keep
    const float* rows_f32;     // with dres2: the fp32 rows at pitch plane
    int plane;
    unsigned long long* dres2; // NULL likewise
    unsigned long long* count; // NULL: nobody asked
    const int* aux_src;        // [n] or NULL
    int* aux_dst;              // [>= ntotal]
};

template <typename EL>
__global__ __launch_bounds__(UPD_THREADS) void update_finish_kernel(UpdateFinishArgs a) {
    // (every wave runs the same number of rounds: the reductions below see whole waves)
    for (int64_t base = blockIdx.x * (int64_t)UPD_THREADS; base < a.n; base += (int64_t)gridDim.x * UPD_THREADS) {
        const int64_t p = base + threadIdx.x;
        double s2 = 0.0, r2 = 0.0; // a maximum of non-negative values: 0 from whoever does not write
        int won = 0;
        if (p < a.n) {
            const int64_t row = upd::local_row(a.ids[p], a.idx_offset, a.ntotal);
            if (row >= 0 && upd::wins(a.owner[row], (int)p)) {
                won = 1;
                if (a.xmax2) s2 = row_sumsq<EL>(reinterpret_cast<const typename EL::type*>(a.canon) + (size_t)row * a.cld, a.cld);
                if (a.dres2) r2 = row_resid_sumsq(a.rows_f32 + (size_t)row * a.plane, a.plane);
                if (a.aux_dst) a.aux_dst[row] = a.aux_src[p];
                a.owner[row] = upd::kNoOwner;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s2 = fmax(s2, __shfl_xor(s2, off));
            r2 = fmax(r2, __shfl_xor(r2, off));
            won += __shfl_xor(won, off);
        }
        if ((threadIdx.x & 63) == 0 && won > 0) {
            if (a.xmax2) atomicMax(a.xmax2, (unsigned long long)__double_as_longlong(s2));
            if (a.dres2) atomicMax(a.dres2, (unsigned long long)__double_as_longlong(r2));
            if (a.count) atomicAdd(a.count, (unsigned long long)won);
        }
    }
}

} // namespace mips
