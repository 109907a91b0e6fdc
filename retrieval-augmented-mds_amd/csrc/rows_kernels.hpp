// Rows by id (include/mips_hip_rows.h): the stored rows, their labels and the canonical score of chosen (query, row) pairs.
//
//   rows_gather_kernel         one WAVE per output row.  Lane l loads the 16-byte chunks l, l + 64, ... of the padded source row
//                              (the row pitch is a multiple of 128 bytes, so a chunk that holds a column < d is read whole), all
//                              of a batch before the first is used, and writes them decoded (float32: a bit move, bf16 bits << 16,
//                              the exact e4m3 value) or raw.  A chunk whose destination is 16-byte aligned and that lies wholly
//                              below column d leaves as 16-byte stores; an unaligned destination (odd d or out_ld, a strided view)
//                              and the row's tail leave as element stores.  Columns >= d of the output are never written.
//   rows_gather_labels_kernel  one thread per id.
//   rows_score_kernel          one THREAD per (query, id) pair: the sequential fp64 sum over the stored values, in the column
//                              order, element traits and arithmetic of rescore_rank_kernel / wide_rescore_kernel (each product is
//                              exact in fp64, so FMA contraction cannot change the sum).  Nothing is ranked.
//
// Ids are int64 throughout; local = id - idx_offset is valid iff 0 <= local < ntotal as int64 (rows_local).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "aux_kernels.hpp"

namespace mips {

constexpr int ROWS_THREADS = 256;
constexpr int ROWS_WAVES = ROWS_THREADS / 64;
constexpr int ROWS_UNROLL = 4;  // 16-byte loads a lane of the gather has in flight (one batch: 4 KiB of a row per wave)
constexpr int ROWS_SCORE_PF = 8; // 16-byte row chunks a thread of the score kernel loads before it sums them

// the local row of an id, or -1: "no row".  id >= idx_offset makes the true difference non-negative, and then the wrapping
// unsigned subtraction is the true difference (below 2^64) -- no signed overflow for INT64_MIN or a negative offset.
__device__ __forceinline__ int64_t rows_local(int64_t id, int64_t idx_offset, int64_t ntotal) {
    if (id < idx_offset) return -1;
    const uint64_t local = (uint64_t)id - (uint64_t)idx_offset;
    return local < (uint64_t)ntotal ? (int64_t)local : -1;
}

struct RowsGatherArgs {
    const void* rows;   // canonical rows: the index rows (bf16 / e4m3) or the fp32 originals of an fp32-exact index
    int ld;             // their pitch in elements
    int d;
    int64_t ntotal;
    const int64_t* ids; // [n]
    int64_t n;
    int64_t idx_offset;
    void* out;          // [n][out_ld] elements of the output type
    int64_t out_ld;
    unsigned fill;      // what an element of "no row" is (the output type's bits)
};

// the raw bits of element e of a 16-byte chunk
template <typename EL>
__device__ __forceinline__ unsigned rows_raw_bits(const u32x4& v, int e) {
    if constexpr (EL::PER16 == 4) return v[e];
    else if constexpr (EL::PER16 == 8) return (v[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
    else return (v[e >> 2] >> ((e & 3) * 8)) & 0xffu;
}

// EL: element traits of the source rows.  RAW: the output has the source's element type (a byte copy of columns 0 .. d - 1);
// otherwise it is float32 and every element is EL::get's exact up-cast, moved as its bit pattern.
template <typename EL, bool RAW>
__global__ __launch_bounds__(ROWS_THREADS) void rows_gather_kernel(RowsGatherArgs a) {
    constexpr int PER = EL::PER16;
    typedef typename std::conditional<RAW, typename EL::type, float>::type OUT;
    typedef typename std::conditional<sizeof(OUT) == 4, uint32_t, typename std::conditional<sizeof(OUT) == 2, uint16_t, uint8_t>::type>::type OBITS;
    const int lane = threadIdx.x & 63;
    const int nchunk = (a.d + PER - 1) / PER; // chunks that hold a column < d
    for (int64_t i = blockIdx.x * (int64_t)ROWS_WAVES + (threadIdx.x >> 6); i < a.n; i += (int64_t)gridDim.x * ROWS_WAVES) {
        const int64_t local = rows_local(a.ids[i], a.idx_offset, a.ntotal);
        OBITS* o = reinterpret_cast<OBITS*>(a.out) + i * a.out_ld;
        if (local < 0) {
            for (int c = lane; c < a.d; c += 64) o[c] = (OBITS)a.fill;
            continue;
        }
        const typename EL::type* x = reinterpret_cast<const typename EL::type*>(a.rows) + (size_t)local * a.ld;
        for (int c0 = 0; c0 < nchunk; c0 += 64 * ROWS_UNROLL) {
            u32x4 v[ROWS_UNROLL];
#pragma unroll
            for (int u = 0; u < ROWS_UNROLL; ++u) {
                const int c = c0 + 64 * u + lane;
                v[u] = u32x4{0u, 0u, 0u, 0u};
                if (c < nchunk) v[u] = *reinterpret_cast<const u32x4*>(x + (size_t)c * PER);
            }
#pragma unroll
            for (int u = 0; u < ROWS_UNROLL; ++u) {
                const int c = c0 + 64 * u + lane;
                if (c >= nchunk) continue;
                const int col0 = c * PER;
                OBITS* dst = o + col0;
                if (col0 + PER <= a.d && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                    if constexpr (RAW || PER == 4) {
                        *reinterpret_cast<u32x4*>(dst) = v[u];
                    } else {
#pragma unroll
                        for (int g = 0; g < PER / 4; ++g) {
                            u32x4 w;
#pragma unroll
                            for (int e = 0; e < 4; ++e) w[e] = __float_as_uint(EL::get(v[u], 4 * g + e));
                            *reinterpret_cast<u32x4*>(dst + 4 * g) = w;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < PER; ++e)
                        if (col0 + e < a.d) dst[e] = RAW ? (OBITS)rows_raw_bits<EL>(v[u], e) : (OBITS)__float_as_uint(EL::get(v[u], e));
                }
            }
        }
    }
}

__global__ __launch_bounds__(ROWS_THREADS) void rows_gather_labels_kernel(const int* labels, int64_t nlabelled, int64_t ntotal, const int64_t* ids,
                                                                          int64_t n, int64_t idx_offset, int* out, int none) {
    for (int64_t i = blockIdx.x * (int64_t)ROWS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROWS_THREADS) {
        const int64_t local = rows_local(ids[i], idx_offset, ntotal);
        out[i] = local >= 0 && local < nlabelled ? labels[local] : none;
    }
}

struct RowsScoreArgs {
    const void* rows;   // canonical rows, pitch ld elements
    const void* y;      // canonical staged queries, pitch ld elements of the query type
    int ld;
    int64_t ntotal;
    const int64_t* ids; // [nq][k]
    int64_t npairs;     // nq * k
    int k;
    int64_t idx_offset;
    double phi;
    float* out;         // [nq][k]
};

// ELQ: element type of the staged queries (= EL except for the e4m3-documents / bf16-queries index, where one 16-byte chunk of a
// row meets two of the query)
template <typename EL, bool L2, typename ELQ = EL>
__global__ __launch_bounds__(ROWS_THREADS) void rows_score_kernel(RowsScoreArgs a) {
    static_assert(EL::PER16 == ELQ::PER16 || EL::PER16 == 2 * ELQ::PER16, "queries at most twice as wide as the rows");
    constexpr int R = EL::PER16 / ELQ::PER16;
    constexpr int PF = ROWS_SCORE_PF / R;
    const int nchunk = a.ld / EL::PER16;
    for (int64_t p = blockIdx.x * (int64_t)ROWS_THREADS + threadIdx.x; p < a.npairs; p += (int64_t)gridDim.x * ROWS_THREADS) {
        const int64_t local = rows_local(a.ids[p], a.idx_offset, a.ntotal);
        float outv = L2 ? INFINITY : -INFINITY;
        if (local >= 0) {
            const typename EL::type* x = reinterpret_cast<const typename EL::type*>(a.rows) + (size_t)local * a.ld;
            const typename ELQ::type* y = reinterpret_cast<const typename ELQ::type*>(a.y) + (size_t)(p / a.k) * a.ld;
            double dot = 0.0, qq = 0.0;
            for (int c0 = 0; c0 < nchunk; c0 += PF) {
                u32x4 xv[PF], yv[PF][R];
#pragma unroll
                for (int t = 0; t < PF; ++t) {
                    const int c = c0 + t < nchunk ? c0 + t : nchunk - 1;
                    xv[t] = *reinterpret_cast<const u32x4*>(x + (size_t)c * EL::PER16);
#pragma unroll
                    for (int r = 0; r < R; ++r) yv[t][r] = *reinterpret_cast<const u32x4*>(y + (size_t)c * EL::PER16 + r * ELQ::PER16);
                }
#pragma unroll
                for (int t = 0; t < PF; ++t) {
                    if (c0 + t < nchunk) {
#pragma unroll
                        for (int e = 0; e < EL::PER16; ++e) { // sequential in the column index
                            const double xe = (double)EL::get(xv[t], e);
                            const double ye = (double)ELQ::get(yv[t][e / ELQ::PER16], e % ELQ::PER16);
                            dot += xe * ye;
                            if (L2) qq += ye * ye;
                        }
                    }
                }
            }
            outv = L2 ? (float)(qq + a.phi - 2.0 * dot) : (float)dot;
        }
        a.out[p] = outv;
    }
}

} // namespace mips
