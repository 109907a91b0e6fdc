// 8-bit scalar-quantised storage (MIPS_DTYPE_SQ8, faiss "SQ8"; DESIGN.md, "8-bit scalar-quantised storage"): one byte per element,
// 256 uniform levels between each column's trained minimum and maximum (sq8_quant.hpp).  Ranking happens in the CODE domain:
//   <q, decode(c_i)> = sum_j (q_j s_j) c_ij + sum_j q_j o_j,   s_j = vdiff_j / 255,  o_j = vmin_j + s_j / 2
// so a search stages q'_j = bf16(q_j s_j), scans the rows as the integers 0 .. 255 against q' (every product is exact in fp32, all
// of 0 .. 255 are bf16 values: scan_kernel_e8's plan with another conversion step), ranks by the canonical score S = the
// sequential fp64 sum of q'_j c_ij, and reports D = (float)(S + B_q), B_q = sum_j q_j o_j in fp64 (sq8_bias_kernel).
//   sq8_minmax_kernel / sq8_minmax_final_kernel   training: column min / max over row parts, then over the parts (no atomics:
//                                                 min and max do not depend on the order); a non-finite value raises a flag
//   sq8_derive_kernel                             s, o from vmin, vdiff
//   sq8_encode_rows_kernel                        float32 / bf16 rows (or raw codes) -> [rows][ld] codes, padding columns code 0
//   sq8_stage_queries_kernel                      q' as bf16 [nq_pad][ld] + B_q; folds the memsets convert_rows_kernel folds
//   sq8_bias_kernel                               D = S + B_q over a finished [nq][k] result
//   sq8_decode_rows_kernel                        reconstruct: codes gathered as float32 -> decoded values, in place
// The scan itself is sq8_scan_kernel.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "rows_kernels.hpp"
#include "sq8_quant.hpp"

namespace mips {

constexpr int SQ8_PARTS = 64; // row parts of the training reduction

template <typename SRC>
__device__ __forceinline__ float sq8_load(const SRC* src, int64_t at) {
    if constexpr (sizeof(SRC) == 4) return ((const float*)src)[at];
    else return bf16_bits_to_f32(((const uint16_t*)src)[at]);
}

// grid (ceil(d / 256), parts): thread (column c, part p) folds rows p, p + parts, ... of this chunk into ITS slot [p][c] of the
// partial arrays (first: the slot starts at +inf / -inf / 0; later chunks of the same training continue it).  Signed zeros: fminf /
// fmaxf may return either of -0.0 and +0.0 when both occur, so a column whose extremum is a zero of both signs has vmin = +-0.0 as
// the order has it -- equal as numbers, and so are vdiff and every code; only the bit pattern get_params reports may differ
template <typename SRC>
__global__ __launch_bounds__(256) void sq8_minmax_kernel(const SRC* __restrict__ src, int64_t n, int d, float* pmin, float* pmax, unsigned char* pflag,
                                                         int first) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const size_t slot = (size_t)blockIdx.y * d + c;
    float lo = first ? INFINITY : pmin[slot], hi = first ? -INFINITY : pmax[slot];
    unsigned char bad = first ? 0 : pflag[slot];
    for (int64_t r = blockIdx.y; r < n; r += gridDim.y) {
        const float x = sq8_load(src, r * d + c);
        lo = fminf(lo, x);
        hi = fmaxf(hi, x);
        if (!(fabsf(x) < INFINITY)) bad = 1; // NaN or +-inf
    }
    pmin[slot] = lo;
    pmax[slot] = hi;
    pflag[slot] = bad;
}

// one thread per padded column: vmin / vdiff [ld] (columns >= d: 0); *bad = 1 if any value was not finite
__global__ __launch_bounds__(256) void sq8_minmax_final_kernel(const float* pmin, const float* pmax, const unsigned char* pflag, int parts, int d, int ld,
                                                               float* vmin, float* vdiff, unsigned* bad) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ld) return;
    float lo = 0.f, hi = 0.f;
    if (c < d) {
        lo = INFINITY, hi = -INFINITY;
        unsigned char b = 0;
        for (int p = 0; p < parts; ++p) {
            lo = fminf(lo, pmin[(size_t)p * d + c]);
            hi = fmaxf(hi, pmax[(size_t)p * d + c]);
            b |= pflag[(size_t)p * d + c];
        }
        if (b) *bad = 1u; // (every writer stores the same value)
    }
    vmin[c] = lo;
    vdiff[c] = sq8::sub(hi, lo);
}

// params = [vmin | vdiff | s | o], ld floats each
__global__ __launch_bounds__(256) void sq8_derive_kernel(float* params, int ld) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ld) return;
    params[2 * ld + c] = sq8::scale(params[ld + c]);
    params[3 * ld + c] = sq8::offset(params[c], params[ld + c]);
}

// one thread per 16 output bytes; SRC = float, uint16_t (bf16 bits) or uint8_t (raw codes)
template <typename SRC>
__global__ void sq8_encode_rows_kernel(const SRC* __restrict__ src, int64_t n, int d, const float* __restrict__ params, uint8_t* dst, int ld) {
    const int chunks = ld / 16;
    const int64_t total = n * chunks;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / chunks;
        const int c0 = (int)(t % chunks) * 16;
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = c0 + e;
            uint32_t b = 0;
            if (c < d) {
                if constexpr (sizeof(SRC) == 1) b = ((const uint8_t*)src)[row * d + c];
                else b = sq8::encode(sq8_load(src, row * d + c), params[c], params[ld + c]);
            }
            o[e >> 2] |= b << ((e & 3) * 8);
        }
        *reinterpret_cast<u32x4*>(dst + row * ld + c0) = o;
    }
}

// q' = bf16(q s) into dst [n_out][ld] (columns >= d and rows n .. n_out - 1 zero), `zero_words` words at `zero` cleared (the
// scan's insert bounds), and bias[row] = B_q = the sequential fp64 sum of q_j o_j in ascending j (one thread per query; each
// product of two float32 values is exact in fp64, so contraction cannot change the sum)
template <typename SRC>
__global__ void sq8_stage_queries_kernel(const SRC* __restrict__ src, int64_t n, int d, const float* __restrict__ params, uint16_t* dst, int ld,
                                         int64_t n_out, uint32_t* zero, int64_t zero_words, double* bias) {
    const int chunks = ld / 8;
    const int64_t total = (n_out > n ? n_out : n) * chunks;
    const float* s = params + 2 * ld;
    const float* o = params + 3 * ld;
    zero_words_grid_stride(zero, zero_words);
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / chunks;
        const int c0 = (int)(t % chunks) * 8;
        uint16_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            v[e] = (c < d && row < n) ? f32_to_bf16_rne(sq8::mul(sq8_load(src, row * d + c), s[c])) : (uint16_t)0;
        }
        u32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = v[2 * e] | ((uint32_t)v[2 * e + 1] << 16);
        *reinterpret_cast<u32x4*>(dst + row * ld + c0) = w;
    }
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        double b = 0.0;
        for (int c = 0; c < d; ++c) b += (double)sq8_load(src, row * d + c) * (double)o[c];
        bias[row] = b;
    }
}

// D = (float)((double)S + B_q) over a finished result [nq][k] (plain or packed).  Slots that carry no score stay as they are:
// the -1 padding (-inf), "no row" of a subset score (-inf), poisoned outputs (NaN).
__global__ void sq8_bias_kernel(float* out_s, int64_t* out_packed, const double* bias, int64_t nq, int k) {
    const int64_t total = nq * k;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const float sc = out_packed ? __uint_as_float((unsigned)out_packed[2 * t]) : out_s[t];
        if (!(fabsf(sc) < INFINITY)) continue;
        const float dv = (float)((double)sc + bias[t / k]);
        if (out_packed) out_packed[2 * t] = (int64_t)__float_as_uint(dv);
        else out_s[t] = dv;
    }
}

// reconstruct: out [n][out_ld] holds the codes of the rows that exist as float32 (rows_gather_kernel<ElemU8, false>); decode them
// in place.  Rows of ids that name no row keep their fill.
__global__ void sq8_decode_rows_kernel(float* out, int64_t out_ld, const int64_t* ids, int64_t n, int d, int64_t idx_offset, int64_t ntotal,
                                       const float* __restrict__ params, int ld) {
    const int64_t total = n * d;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / d;
        const int c = (int)(t % d);
        if (rows_local(ids[i], idx_offset, ntotal) < 0) continue;
        float* p = out + i * out_ld + c;
        *p = sq8::decode((uint8_t)*p, params[c], params[ld + c]);
    }
}

} // namespace mips
