// Kernels of the IVF search (include/mips_hip_ivf.h: mips_ivf_search).
//
//   ivf_list_scan_kernel   grid = nq * p * S workgroups of IVF_SCAN_WAVES waves; workgroup (j, t, s) scores segment s of the t-th
//                          probed list of query j.  Everything that depends on the queries is read HERE and range-checked before
//                          it becomes an address: the list number probe[j][t] (outside [0, nlist): an empty list), the list's
//                          bounds list_offsets[l], list_offsets[l + 1] (not 0 <= o0 <= o1 <= ntotal: an empty list), every row
//                          number of list_rows (outside [0, ntotal): no row).  The host passes sizes only.
//                          The canonical score is computed directly -- one lane per row, the sequential fp64 sum over ascending
//                          column, the query as fp64 in LDS, rows brought in coalesced through a per-wave LDS transpose: the
//                          arrangement of exact_dots (resolve_kernels.hpp) over GATHERED rows, one accumulator.  Every wave keeps
//                          a sorted top k by (key descending, row ascending) in its lanes 0 .. k - 1 (the lists of
//                          resolve_overflow_kernel); the waves' lists meet in LDS and wave 0 writes the workgroup's sorted partial
//                          of k entries, padding (-inf, -1) last, in the MIPS_OUT_PACKED layout [p * S][nq][k][2] that
//                          merge_topk_sorted_packed_kernel reads.
//                          FILT (mips_ivf_search_sel / _grp): the lane that reads a row number also reads the row's bit and label
//                          and drops a row that is not admitted there, before any of its bytes is requested; the admitted row
//                          numbers are compacted through a per-wave queue in LDS (ivf_filter_math.hpp) and scored 64 at a time,
//                          so a sparse filter costs passes for the rows it admits, not for the positions it walks.  The order
//                          (key descending, row ascending) is total, so the order in which rows are scored does not show in the
//                          result.  FILT = false compiles the unfiltered kernel: no queue, no extra LDS, the same registers.
//   ivf_finish_kernel      behind the merge, over [nq][k]: SQ8 scores S -> D = (float)((double)S + B_q) (sq8_bias_kernel's
//                          arithmetic), idx_offset added to the rows; padding stays (-inf, -1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "ivf_filter_math.hpp"
#include "ivf_search_math.hpp"

namespace mips {

constexpr int IVF_SCAN_WAVES = 4;
constexpr int IVF_SCAN_TCH = 8;       // 16-byte chunks per row per tile step: 128 bytes
constexpr int IVF_SCAN_MAX_LD = 1024; // elements of a staged query at most (d <= 1024)
constexpr int IVF_SCAN_KSLOT = 32;    // slots of a wave's list in LDS (k <= MIPS_MAX_K = 29)

struct IvfScanArgs {
    const void* rows;       // canonical rows of the flat index: bf16 rows, rows_f32, SQ8 codes
    const void* y;          // staged queries [nq][ld] of the query element type
    int ld;                 // elements per row and per staged query; ld / PER16 is a multiple of IVF_SCAN_TCH
    int64_t ntotal;
    const int64_t* probe;   // [nq][p] list numbers, as the coarse search wrote them
    const int* offsets;     // [nlist + 1]
    const int* list_rows;   // [>= ntotal]
    int nlist;
    int64_t nq;
    int p, S, k;
    int64_t* parts;         // [p * S][nq][k][2]
    // the filtered instances only (FILT); a null pointer switches that half of the rule off
    const uint8_t* sel_bits; // bit sel_bit0 + i decides row i
    int64_t sel_bit0;
    const int* row_labels;   // [ntotal] the flat index's labels
    const int* q_labels;     // [nq]
    int grp_mode;            // MIPS_GRP_EXCLUDE / MIPS_GRP_ONLY
};

// The canonical dot product of row `id` of this lane (id < 0: no row; the lane reads row 0 and the caller drops the result) with
// the query in yd.  8 lanes cover a 128-byte segment of one row, 8 rows per load instruction, through the wave's LDS tile
// ([64 rows][TCH + 1 chunks]); the next segment's loads are in flight while this one is summed.
template <typename EL>
__device__ __forceinline__ double ivf_gathered_dot(const typename EL::type* rows, int ld, int id, int lane, u32x4* tile, const double* yd) {
    constexpr int PER = EL::PER16;
    constexpr int TCH = IVF_SCAN_TCH;
    const int nchunk = ld / PER;
    const typename EL::type* src[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int rr = __shfl(id, 8 * i + (lane >> 3));
        if (rr < 0) rr = 0;
        src[i] = rows + (size_t)rr * ld + (size_t)(lane & 7) * PER;
    }
    u32x4 in[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = *reinterpret_cast<const u32x4*>(src[i]);
    double acc = 0.0;
    for (int c0 = 0; c0 < nchunk; c0 += TCH) {
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[(8 * i + (lane >> 3)) * (TCH + 1) + (lane & 7)] = in[i];
        if (c0 + TCH < nchunk) {
#pragma unroll
            for (int i = 0; i < 8; ++i) in[i] = *reinterpret_cast<const u32x4*>(src[i] + (size_t)(c0 + TCH) * PER);
        }
        __builtin_amdgcn_wave_barrier(); // (one wave: LDS operations complete in order)
#pragma unroll
        for (int c = 0; c < TCH; ++c) {
            const u32x4 v = tile[lane * (TCH + 1) + c];
            const double* yy = yd + (size_t)(c0 + c) * PER;
#pragma unroll
            for (int e = 0; e < PER; ++e) acc += (double)EL::get(v, e) * yy[e]; // sequential in the column index
        }
        __builtin_amdgcn_wave_barrier();
    }
    return acc;
}

// One scoring pass: lane `lane` scores row `id` (id < 0: none) and the wave inserts what ranks among its best K into its sorted list
// (lk, li, cnt): lane u < cnt holds the wave's u-th best by (key descending, row ascending).
template <typename EL>
__device__ __forceinline__ void ivf_score_insert(const typename EL::type* rows, int ld, int id, int lane, u32x4* tile, const double* yd, int K, float& lk,
                                                 int& li, int& cnt) {
    const float key = (float)ivf_gathered_dot<EL>(rows, ld, id, lane, tile, yd);
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

// EL: element type of the rows; ELQ: of the staged queries (bf16 for SQ8 codes); FILT: the filtered instance
template <typename EL, typename ELQ, bool FILT = false>
__global__ __launch_bounds__(64 * IVF_SCAN_WAVES) void ivf_list_scan_kernel(IvfScanArgs a) {
    __shared__ __attribute__((aligned(16))) double yd[IVF_SCAN_MAX_LD];
    __shared__ __attribute__((aligned(16))) u32x4 tiles[IVF_SCAN_WAVES * 64 * (IVF_SCAN_TCH + 1)];
    __shared__ float mk[IVF_SCAN_WAVES * IVF_SCAN_KSLOT];
    __shared__ int mi[IVF_SCAN_WAVES * IVF_SCAN_KSLOT];
    __shared__ int fq[FILT ? IVF_SCAN_WAVES * ivf::kQueueSlots : 1]; // the waves' queues of admitted row numbers
    __shared__ int mc[IVF_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.k;
    const int64_t b = blockIdx.x;
    const int s = (int)(b % a.S);
    const int t = (int)((b / a.S) % a.p);
    const int64_t j = b / ((int64_t)a.S * a.p);
    if (j >= a.nq) return;
    // the list and its bounds: read here, checked here
    const int64_t l = a.probe[j * a.p + t];
    int64_t beg = 0, L = 0;
    if (l >= 0 && l < a.nlist) {
        const int64_t o0 = a.offsets[l], o1 = a.offsets[l + 1];
        if (o0 >= 0 && o0 <= o1 && o1 <= a.ntotal) {
            beg = o0;
            L = o1 - o0;
        }
    }
    const int64_t lo = beg + ivf::seg_bound(L, s, a.S), hi = beg + ivf::seg_bound(L, s + 1, a.S);

    float lk = -INFINITY; // the wave's list: lane u < cnt holds its u-th best
    int li = IDX_NONE;
    int cnt = 0;
    if (lo < hi) { // (uniform over the workgroup)
        constexpr int PERQ = ELQ::PER16;
        const typename ELQ::type* ys = reinterpret_cast<const typename ELQ::type*>(a.y) + (size_t)j * a.ld;
        for (int c = tid; c < a.ld / PERQ; c += 64 * IVF_SCAN_WAVES) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(ys + (size_t)c * PERQ);
#pragma unroll
            for (int e = 0; e < PERQ; ++e) yd[c * PERQ + e] = (double)ELQ::get(v, e);
        }
        __syncthreads();
        const typename EL::type* rows = reinterpret_cast<const typename EL::type*>(a.rows);
        u32x4* tile = tiles + wave * 64 * (IVF_SCAN_TCH + 1);
        int* queue = fq + (FILT ? wave * ivf::kQueueSlots : 0);
        int queued = 0; // entries of the wave's queue, < 64 between windows
        const int qlab = FILT && a.q_labels != nullptr ? a.q_labels[j] : ivf::kLabelNone;
        for (int64_t r0 = lo + (int64_t)wave * 64; r0 < hi; r0 += 64 * IVF_SCAN_WAVES) {
            const int64_t pos = r0 + lane;
            int id = -1;
            if (pos < hi) {
                const int r = a.list_rows[pos];
                if (r >= 0 && r < a.ntotal) id = r;
            }
            if constexpr (FILT) {
                // admission where the row number is read: bit and label of an in-range row only, then the queue
                if (id >= 0) {
                    bool ok = a.sel_bits == nullptr || ivf::bit_is_set(a.sel_bits, a.sel_bit0 + id);
                    if (ok && a.q_labels != nullptr) ok = ivf::group_admits(a.row_labels[id], qlab, a.grp_mode);
                    if (!ok) id = -1;
                }
                const unsigned long long adm = __ballot(id >= 0);
                if (id >= 0) queue[ivf::queue_slot(queued, adm, lane)] = id;
                queued = ivf::queue_after_append(queued, adm);
                __builtin_amdgcn_wave_barrier(); // (one wave: LDS operations complete in order)
                if (!ivf::queue_has_pass(queued)) continue; // (uniform over the wave)
                id = queue[lane];
                queued = ivf::queue_after_pass(queued);
                const int next = lane < queued ? queue[ivf::kQueuePass + lane] : -1;
                __builtin_amdgcn_wave_barrier();
                if (lane < queued) queue[lane] = next;
                __builtin_amdgcn_wave_barrier();
            }
            ivf_score_insert<EL>(rows, a.ld, id, lane, tile, yd, K, lk, li, cnt);
        }
        if constexpr (FILT) {
            if (queued > 0) ivf_score_insert<EL>(rows, a.ld, lane < queued ? queue[lane] : -1, lane, tile, yd, K, lk, li, cnt); // the remainder
        }
    }
    if (lane < cnt) {
        mk[wave * IVF_SCAN_KSLOT + lane] = lk;
        mi[wave * IVF_SCAN_KSLOT + lane] = li;
    }
    if (lane == 0) mc[wave] = cnt;
    __syncthreads();
    if (wave != 0) return;
    // wave 0 ranks the union (<= IVF_SCAN_WAVES * k entries with distinct rows: every rank is taken once)
    int64_t* out = a.parts + (((int64_t)t * a.S + s) * a.nq + j) * K * 2;
    int total = 0;
#pragma unroll
    for (int w = 0; w < IVF_SCAN_WAVES; ++w) total += mc[w];
#pragma unroll
    for (int u = 0; u < IVF_SCAN_WAVES * IVF_SCAN_KSLOT / 64; ++u) {
        const int e = lane + 64 * u, w = e / IVF_SCAN_KSLOT;
        if (e % IVF_SCAN_KSLOT >= mc[w]) continue;
        const float ck = mk[e];
        const int ci = mi[e];
        int rank = 0;
        for (int w2 = 0; w2 < IVF_SCAN_WAVES; ++w2)
            for (int u2 = 0; u2 < mc[w2]; ++u2) rank += ranks_before(mk[w2 * IVF_SCAN_KSLOT + u2], mi[w2 * IVF_SCAN_KSLOT + u2], ck, ci) ? 1 : 0;
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

__global__ void ivf_finish_kernel(float* out_s, int64_t* out_i, const double* bias, int64_t nq, int k, int64_t idx_offset) {
    const int64_t total = nq * k;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = out_i[t];
        if (id < 0) continue;
        if (bias != nullptr) {
            const float sc = out_s[t];
            if (fabsf(sc) < INFINITY) out_s[t] = (float)((double)sc + bias[t / k]);
        }
        out_i[t] = id + idx_offset;
    }
}

} // namespace mips
