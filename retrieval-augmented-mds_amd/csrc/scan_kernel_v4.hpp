// scan_kernel_v4: the query-stationary scan of scan_kernel_v3 on the 16x16x32 bf16 MFMA shape.
//
// Why: under this load the chip is power-limited.  tools/mfma_ceiling.hip (profiles/r1_class_maxima): a bare
// LDS-fed single-chain loop sustains 1.51-1.59 PFLOP/s on random bf16 data with 32x32x16 and 1.71-1.74 with
// 16x16x32 at the same bytes and flops per wave -- the chip holds a higher clock on the smaller shape.
//
// Mapping (v_mfma_f32_16x16x32_bf16: lane l -> c = l & 15, g = l >> 4; A[row c][k = 8 g + j],
// B[k = 8 g + j][col c], C/D col = c, row = 4 g + reg):
//   * a wave still owns 32 stationary queries = two 16-query column blocks n = 0, 1 (192 fragment VGPRs);
//   * a 32-document block is scored as two 16-document halves; per half and k32-step ONE A fragment feeds
//     two MFMAs (one per query block), 4 accumulator registers each -> 8 accumulator VGPRs instead of 16,
//     which pays for the second running list a lane now needs (lane (c, g) sees documents 4 g .. 4 g + 3 of
//     each half for queries c and 16 + c); the half-block epilogue is a handful of instructions unless a
//     document passes (16 accumulators and one epilogue per block do not fit next to lists of 6: 13+ spilled
//     registers -- the pitch-768 shared-block instance runs them next to lists of 4, see ONE_PASS below);
//   * four lanes (g = 0..3) share a query, so a (query, split) pair has 4 sub-lists of KL entries.  A
//     document of global rank r can only be pushed out of its sub-list by KL better documents of the same
//     sub-list, so ranks 1 .. KL survive for certain (KL = 6 = k + 1 for k <= 5), the re-score pool is the
//     8 best of the union;
//   * shared insert bounds as scan_kernel_v3's class words: every sub-list publishes its best score (PUB = 1; its PUB-th best
//     in general) into class word (4 split + g) & 7 of its query, the bound is the minimum of the 8 words, re-read
//     sparsely: 8 PUB distinct documents score at least the bound, so nothing below it belongs to a pool of 8 PUB.
//     PUB = 4 serves the "optimistic" pools of 32 (mips_hip.hip): the lists still keep 6 entries each, the margin
//     check decides per query whether the pool selected from them was wide enough.
// Everything else (LDS-DMA ring, counted vmcnt, split barrier, strict-'>' tie rule) is scan_kernel_v3's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.hpp"
#include "scan_kernel_v3.hpp"

namespace mips {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// lane id the compiler cannot hoist out of a loop (so that values derived from it are re-derived where they
// are used instead of living in -- or being spilled from -- a register across the MFMA chain)
__device__ __forceinline__ unsigned lane_id_here() {
    unsigned ln = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
#endif
    return ln;
}

// max(a, b, c) of raw MFMA results.  fmaxf() makes the compiler canonicalise every input it cannot prove canonical (one
// v_max_f32 x, x, x per accumulator); the instruction itself needs none.  An asm statement gets no hazard padding: the caller
// places it at least 8 wait states after the MFMA that wrote an operand (what hipcc pads a VALU read of this MFMA shape with).
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r = a;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
#else
    (void)b; (void)c;
#endif
    return r;
}

// NT_DOCS: non-temporal document DMA -- for searches of ONE query tile, where every document block has a single reader
// (the fourth slot held a diagnostic axis, retired; it stays in the parameter list so that the instance names remain the ones
// profiles/, latest_traffic.json and the tests know)
template <int KL, int KS32, int AD, int = 0, bool NT_DOCS = false, int PUB = 1>
__global__ __launch_bounds__(512, 2) void scan_kernel_v4(ScanArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WAVES = 8;
    constexpr int TN = WAVES * 32;
    constexpr int STAGES = 3;
    constexpr int STAGE_BYTES = V3_DB * KS32 * 64; // 32 rows x (32 KS32) k x 2 B
    constexpr int PIECES = STAGE_BYTES / 1024;
    constexpr int PPW = PIECES / WAVES;
    static_assert(PIECES % WAVES == 0, "every wave must issue the same number of DMA pieces");
    static_assert(KL <= 8, "8 class words vouch for 8 documents");
    static_assert(PUB >= 1 && PUB <= KL, "a sub-list publishes one of its entries");
    constexpr int STEPS = 2 * KS32; // k32-steps per block (two halves)
    // ONE_PASS (the pitch-768 shared-block instance with pools of 8): the accumulators of BOTH halves stay live through the
    // chain and the block runs one pre-test, one ballot and one branch instead of two.  The eight extra accumulator registers
    // are paid for by keeping the sub-lists KLI = 4 deep in registers; the record a lane writes still has KL slots (below).
    // A list of 4 may drop a true top-5 member: its 4th score then bounds what it dropped, the margin check flags the query
    // and the exact pass settles it, exactly as for any other pool that was not provably wide enough.
    constexpr bool ONE_PASS = KL == 6 && KS32 == 24 && !NT_DOCS && PUB == 1;
    constexpr int KLI = ONE_PASS ? 4 : KL; // entries a sub-list keeps while it scans
    static_assert(PUB <= KLI, "a sub-list publishes one of the entries it keeps");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15;
    const int g = lane >> 4;

    const int xcd = blockIdx.x & 7;
    const int j = blockIdx.x >> 3;
    const int qt = (xcd % p.qgroups) + p.qgroups * (j % p.qt_per_group);
    const int split = (xcd / p.qgroups) * p.splits_per_group + j / p.qt_per_group;
    if (qt >= p.nqt) return;
    if (p.spin_limit < 0 && tid == 0) *p.err = 1u; // test-only: force the scan-error path (include/mips_hip.h, "spin_limit")
    const bool idle_wave = (qt * TN + wave * 32) >= p.nq;

    const int b0 = split * p.tiles_per_split;
    int b1 = b0 + p.tiles_per_split;
    if (b1 > p.ntiles) b1 = p.ntiles;
    const int nb = b1 > b0 ? b1 - b0 : 0;

    // ---- stationary query fragments: lane holds Q[q0 + 16 n + c][32 s + 8 g .. +8)
    bf16x8 bq[2][KS32];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const uint16_t* qrow = p.qbuf + ((int64_t)qt * TN + wave * 32 + n * 16 + c) * p.ld + 8 * g;
#pragma unroll
        for (int s = 0; s < KS32; ++s) bq[n][s] = *reinterpret_cast<const bf16x8*>(qrow + 32 * s);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int s = 0; s < KS32; ++s) asm volatile("" : "+v"(bq[n][s]));
#endif
    }

    float ls[2][KLI];
    int li[2][KLI];
    float thr[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        thr[n] = -INFINITY;
#pragma unroll
        for (int i = 0; i < KLI; ++i) {
            ls[n][i] = -INFINITY;
            li[n][i] = IDX_NONE;
        }
    }

    // ---- shared insert bounds (scan_kernel_v3.hpp, "shared per-query thresholds"): p.gthr = [query tile][wave][32 queries][8 words]
    constexpr unsigned THR_AREA = STAGES * STAGE_BYTES;
    constexpr unsigned THR_WAVE = 1024u;
    constexpr unsigned DUMP_AREA = THR_AREA + WAVES * THR_WAVE;
    static_assert(THR_AREA % 1024 == 0, "the wave areas are recovered from thr_addr by masking");
    // this lane's DMA chunk = LDS slot = voffset; re-derived from the lane id wherever it is needed
    auto thr_addr_of = [&](unsigned ln) { return THR_AREA + wave * THR_WAVE + ln * 16u; };
    *reinterpret_cast<uint4*>(smem + thr_addr_of(lane)) = make_uint4(0u, 0u, 0u, 0u);
    const __amdgpu_buffer_rsrc_t thr_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<unsigned char*>(p.gthr) + (int64_t)qt * (WAVES * THR_WAVE) - (int64_t)THR_AREA), 0,
        (int)(THR_AREA + WAVES * THR_WAVE), 0x00020000);
    // ONE_PASS keeps this value in a register (opaque, as lane_off_kept below), so that the bound fetch at the head of a block
    // costs no vector instruction
    unsigned thr_addr_kept = 0u;
    if constexpr (ONE_PASS) {
        thr_addr_kept = thr_addr_of((unsigned)lane);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(thr_addr_kept));
#endif
    }
    auto refresh_thresholds = [&](bool real) { // !real: out-of-range dummy into the dump area (uniform vmcnt count)
        lds_void* dst = (lds_void*)(smem + (real ? THR_AREA + wave * THR_WAVE : DUMP_AREA));
        const unsigned thr_addr = ONE_PASS ? thr_addr_kept : thr_addr_of(lane_id_here());
        __builtin_amdgcn_raw_ptr_buffer_load_lds(thr_rsrc, dst, 16, real ? thr_addr : (thr_addr | 0x40000000u), 0, 0, 16);
    };

    // ---- LDS-DMA map (as v3): piece pc = slab * 4 + rg, 8 rows x 128 B
    const unsigned char* docs_b = reinterpret_cast<const unsigned char*>(p.docs);
    const int64_t row_bytes = (int64_t)p.ld * 2;
    // ONE_PASS keeps the per-lane source offset of issue_piece in a register (the shorter lists leave room for it); the asm
    // makes the value opaque, so that it is not re-derived from the lane id at each of the six pieces of a block
    unsigned lane_off_kept = 0u;
    if constexpr (ONE_PASS) {
        lane_off_kept = ((unsigned)lane >> 3) * (unsigned)row_bytes + ((((unsigned)lane & 7u) ^ (((unsigned)lane >> 4) & 7u)) << 4);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(lane_off_kept));
#endif
    }
    auto issue_piece = [&](const unsigned char* blk_base, int stage, int i) {
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void*)blk_base, 0, (int)(V3_DB * row_bytes), 0x00020000);
        const int pc = wave + WAVES * i;
        const int slab = pc >> 2, rg = pc & 3;
        // per-lane source offset: row lane >> 3 of the piece, chunk slot (lane & 7) ^ ((row >> 1) & 7) = (lane & 7) ^
        // ((4 rg + (lane >> 4)) & 7).  Recomputed per piece from the lane id where the kernel has no VGPR to spare
        unsigned lane_off0 = lane_off_kept;
        if constexpr (!ONE_PASS) {
            const unsigned ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            lane_off0 = (ln >> 3) * (unsigned)row_bytes + (((ln & 7u) ^ ((ln >> 4) & 7u)) << 4);
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(smem + stage * STAGE_BYTES + pc * 1024), 16,
                                                 (rg & 1) ? (lane_off0 ^ 64u) : lane_off0,
                                                 rg * 8 * (int)row_bytes + slab * 128, 0, NT_DOCS ? 2 : 0);
    };
    auto issue = [&](const unsigned char* blk_base, int stage) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) issue_piece(blk_base, stage, i);
    };

    // ---- A-fragment read addresses: row = 16 half + c, chunk 4 (s & 1) + g of slab s >> 1, slot chunk ^ swz
    auto rd0_of = [&](unsigned ln) { // (s & 1) == 0; the odd step is this ^ 64 (chunk + 4)
        const unsigned cc = ln & 15u, gg = ln >> 4;
        return (int)(cc * 128u + ((gg ^ ((cc >> 1) & 7u)) << 4));
    };
    // ONE_PASS keeps it (opaque); the two read addresses of a block, stage base + rd0 and stage base + (rd0 ^ 64), are made from
    // it under the last MFMAs of the block before and cross the block boundary in registers
    unsigned rd0_kept = 0u, rd_even = 0u, rd_odd = 0u;
    auto set_read_addresses = [&](int stage) {
        // two instructions, the stage base from an SGPR; as asm, so that the compiler neither keeps rd0 ^ 64 in a register of
        // its own nor moves the pair to the head of the next block
        const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(size_t)(lds_void*)smem + (unsigned)(stage * STAGE_BYTES)));
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("v_add_u32 %0, %3, %2\n\tv_xad_u32 %1, %2, 64, %3" : "=&v"(rd_even), "=v"(rd_odd) : "v"(rd0_kept), "s"(base));
#else
        (void)base;
#endif
    };
    if constexpr (ONE_PASS) {
        rd0_kept = (unsigned)rd0_of((unsigned)lane);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(rd0_kept));
#endif
        set_read_addresses(0);
    }

    // ---- split barrier (see scan_kernel_v3.hpp)
    const unsigned cnt_lds = (unsigned)(size_t)(lds_void*)(smem + DUMP_AREA + 1024);
    unsigned arrivals_needed = 0;
    // A wave issues PPW document pieces per block, and one bound fetch before them: in every block where DUMMY_FETCH (a fetch of
    // out-of-range zeros into the dump area stands in on the blocks that refresh nothing), in the refresh blocks alone otherwise.
    // arrive(fetched) says whether THIS block had the fetch.  The invariant: vmcnt(N) with N = the operations the wave issued in
    // this block leaves only those outstanding (loads retire in issue order), so everything issued in the block before
    // -- the pieces of the stage that the next block reads -- has landed when the wave adds itself to the arrival count.
    // The prologue (one bound fetch + PPW pieces per ring stage) and the idle waves' loop count the same way.
    static_assert(STAGES == 3, "arrive() lets the operations of one block stay in flight");
    constexpr bool DUMMY_FETCH = !ONE_PASS;
    auto arrive = [&](int fetched) { // 0 or 1, uniform
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (ONE_PASS) {
            // one straight statement: lane 0 alone adds (every lane of the wave is active here), without the compiler's branch
            // around a masked-off region.  The wait of a block that fetched nothing is skipped by a branch that only the refresh
            // blocks take; vmcnt(PPW + 1) after vmcnt(PPW) waits for nothing.
            uint64_t exec_kept;
            asm volatile("s_cmp_lg_u32 %3, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt vmcnt(%4)\n1:\n\ts_waitcnt vmcnt(%5)\n\t"
                         "s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_add_u32 %1, %2\n\ts_mov_b64 exec, %0"
                         : "=&s"(exec_kept) : "v"(cnt_lds), "v"(1u), "s"(fetched), "n"(PPW), "n"(PPW + 1) : "memory", "scc");
            return;
        }
#endif
        if (fetched) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW + 1) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
#if defined(__HIP_DEVICE_COMPILE__)
        if (lane == 0) asm volatile("ds_add_u32 %0, %1" ::"v"(cnt_lds), "v"(1u) : "memory");
#endif
    };
    auto wait_all = [&]() {
        arrivals_needed += WAVES;
        for (int spin = 0;; ++spin) {
            unsigned v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(cnt_lds) : "memory");
#endif
            if (__builtin_amdgcn_readfirstlane(v) >= arrivals_needed) break;
            if (spin > p.spin_limit) {
                if (lane == 0) *p.err = 1u;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    // ONE_PASS: the same polls in the same order, laid out so that "count reached" at the first poll falls through into the
    // block; the sleeping polls and the spin-limit error path stand aside
    auto reached = [&]() {
        unsigned v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(cnt_lds) : "memory");
#endif
        return __builtin_amdgcn_readfirstlane(v) >= arrivals_needed;
    };
    auto wait_all_straight = [&]() {
        arrivals_needed += WAVES;
        if (__builtin_expect(!reached(), 0)) {
            for (int spin = 0;; ++spin) {
                if (spin > p.spin_limit) {
                    if (lane == 0) *p.err = 1u;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                if (reached()) break;
            }
        }
    };

    // epilogue of one 16-document half: the 8 accumulator registers of a lane are documents base .. base + 3
    // against queries c (n = 0) and 16 + c (n = 1).  No synchronisation in here: at mid-block the partner
    // wave's MFMAs keep the matrix pipe busy while this wave runs the few instructions of the pre-test.
    auto epilogue_half = [&](f32x4 (&acc)[2], int blk, int half) {
        // fast path: 6 max, 2 compares, one branch -- everything else is derived only if a document passes
        const float mx0 = fmaxf(fmaxf(acc[0][0], acc[0][1]), fmaxf(acc[0][2], acc[0][3]));
        const float mx1 = fmaxf(fmaxf(acc[1][0], acc[1][1]), fmaxf(acc[1][2], acc[1][3]));
        if (__ballot(mx0 > thr[0] || mx1 > thr[1]) != 0ull) {
            const unsigned thr_addr = thr_addr_of(lane_id_here());
            const int base = blk * V3_DB + 16 * half + (int)((thr_addr >> 6) & 12u); // + 4 g, from the lane bits
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const float mark = ls[n][PUB - 1];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = acc[n][r];
                    if (s > thr[n]) {
                        list_insert<KLI>(ls[n], li[n], s, base + r);
                        thr[n] = fmaxf(thr[n], ls[n][KLI - 1]);
                    }
                }
                if (ls[n][PUB - 1] > mark) { // new PUB-th best of this sub-list: raise its class word, (4 split + g) & 7
                    const unsigned cls = (4u * (unsigned)split + ((thr_addr >> 8) & 3u)) & 7u;
                    publish_umax(thr_encode(ls[n][PUB - 1]), (thr_addr & ~0x3FFu) + ((thr_addr & 0xF0u) << 1) + 512u * n + 4u * cls, thr_rsrc);
                }
            }
        }
    };

    // ONE_PASS: epilogue of the whole 32-document block.  acc[half][n] = documents 16 half + 4 g .. + 3 against query 16 n + c.
    // mx0, mx1 = the largest of the lane's eight accumulators for query c and for query 16 + c (block(): half_max, block_max).
    // The fast path (2 compares, one branch) falls through; the insert path is one loop per query that visits only the
    // accumulators above the bound, lowest document first (the order the strict-'>' tie rule needs), through ONE copy of
    // list_insert -- a select chain picks the score, so the path stays a few hundred bytes instead of sixteen inlined inserts.
    auto epilogue_block = [&](f32x4 (&acc)[2][2], int blk, float mx0, float mx1) {
        if (__builtin_expect(__ballot((int)(mx0 > thr[0]) | (int)(mx1 > thr[1])) != 0ull, 0)) { // '|': no lane-level short circuit
            const unsigned thr_addr = thr_addr_of(lane_id_here());
            const int base = blk * V3_DB + (int)((thr_addr >> 6) & 12u); // + 4 g, from the lane bits
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const float mark = ls[n][PUB - 1];
                unsigned m = 0u; // bit 4 half + r: that accumulator is above the bound
#pragma unroll
                for (int e = 0; e < 8; ++e) m |= acc[e >> 2][n][e & 3] > thr[n] ? 1u << e : 0u;
                while (m != 0u) {
                    const int e = __ffs(m) - 1;
                    m &= m - 1u;
                    float s = acc[0][n][0];
#pragma unroll
                    for (int x = 1; x < 8; ++x) s = e == x ? acc[x >> 2][n][x & 3] : s;
                    if (s > thr[n]) { // the bound may have risen since the mask was taken
                        list_insert<KLI>(ls[n], li[n], s, base + 16 * (e >> 2) + (e & 3));
                        thr[n] = fmaxf(thr[n], ls[n][KLI - 1]);
                    }
                }
                if (ls[n][PUB - 1] > mark) { // new PUB-th best of this sub-list: raise its class word, (4 split + g) & 7
                    const unsigned cls = (4u * (unsigned)split + ((thr_addr >> 8) & 3u)) & 7u;
                    publish_umax(thr_encode(ls[n][PUB - 1]), (thr_addr & ~0x3FFu) + ((thr_addr & 0xF0u) << 1) + 512u * n + 4u * cls, thr_rsrc);
                }
            }
        }
    };

    // first block of the index that holds rows past its end: (blk + 1) * 32 > ntotal <=> blk >= ntotal / 32 (uniform, scalar)
    const int first_ragged = (int)(p.ntotal / V3_DB < 0x7fffffff ? p.ntotal / V3_DB : 0x7fffffff);
    auto block = [&](int refresh_word, int blk, int stage, const unsigned char* pbase, int pstage) { // refresh_word: 0 or 1
        const bool refresh = refresh_word != 0;
        if constexpr (!ONE_PASS) {
            if (idle_wave) { // all of this wave's queries are padding (scan_kernel_v3.hpp): bring the documents, skip the arithmetic
                refresh_thresholds(false);
                issue(pbase, pstage);
                arrive(1);
                return;
            }
        }
        const unsigned char* sa = smem + stage * STAGE_BYTES;
        const int rd0 = ONE_PASS ? 0 : rd0_of(lane_id_here());
        // flattened step t = half * KS32 + s
        auto lds_frag = [&](int t) {
            const int half = t / KS32, s = t % KS32;
            if constexpr (ONE_PASS) { // the kept addresses are LDS byte addresses, stage base included: the rest is the immediate
                typedef const __attribute__((address_space(3))) bf16x8 lds_frag_t;
                return *(lds_frag_t*)(size_t)(((s & 1) ? rd_odd : rd_even) + (unsigned)(half * 2048 + (s >> 1) * 4096));
            }
            const int off = half * 2048 + (s >> 1) * 4096 + ((s & 1) ? (rd0 ^ 64) : rd0);
            return *reinterpret_cast<const bf16x8*>(sa + off);
        };
        // ONE_PASS: the head of a block is its first two fragment reads, from addresses that are already in registers; no
        // vector instruction stands between the poll and them, and the MFMA chain starts as soon as they land
        bf16x8 ar[AD];
#pragma unroll
        for (int t = 0; t < AD; ++t) ar[t] = lds_frag(t);
        if constexpr (DUMMY_FETCH) {
            refresh_thresholds(refresh); // first VMEM op of the block
        } else {
            if (__builtin_expect(refresh, 0)) refresh_thresholds(true); // first VMEM op of a refresh block; the others fetch nothing
        }
        __builtin_amdgcn_sched_barrier(0);
        const bool ragged = ONE_PASS ? blk >= first_ragged : (int64_t)(blk + 1) * V3_DB > p.ntotal; // uniform
        auto mask_ragged = [&](f32x4 (&a)[2], int half) { // last block of the index only: rows past the end score -inf
            const int base = blk * V3_DB + 16 * half + 4 * (int)(lane_id_here() >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if ((int64_t)(base + r) >= p.ntotal) {
                    a[0][r] = -INFINITY;
                    a[1][r] = -INFINITY;
                }
        };
        f32x4 accs[2][2]; // [half][n]; without ONE_PASS a half's accumulators die in its own epilogue
        // ONE_PASS pre-test: the largest of a lane's 8 accumulators per query, 4 v_max3_f32 each.  The two that reduce half 0
        // run under the MFMAs of half 1 (5 and 7 steps after the last MFMA of half 0: its results have long landed)
        float mh[2] = {0.f, 0.f};
        auto half_max = [&](const f32x4& a) { return max3_raw(max3_raw(a[0], a[1], a[2]), a[3], a[3]); };
        auto block_max = [&](float m, const f32x4& a) { return max3_raw(max3_raw(m, a[0], a[1]), a[2], a[3]); };
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4(&acc)[2] = accs[half];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[n][r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS32; ++s) {
                const int t = half * KS32 + s;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ar[t % AD], bq[0][s], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ar[t % AD], bq[1][s], acc[1], 0, 0, 0);
                if (t + AD < STEPS) ar[t % AD] = lds_frag(t + AD);
                if ((t % (STEPS / PPW)) == (STEPS / PPW) / 2) issue_piece(pbase, pstage, t / (STEPS / PPW));
                if constexpr (ONE_PASS) {
                    if (t == KS32 + 5) mh[0] = half_max(accs[0][0]);
                    if (t == KS32 + 7) mh[1] = half_max(accs[0][1]);
                    // the last fragment read of this block is issued: the next block's read addresses take the registers over
                    if (t == STEPS - AD) set_read_addresses(stage == STAGES - 1 ? 0 : stage + 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // all LDS reads of this block are done: arrive; the epilogue runs un-synchronised
            if (half == 1) arrive(DUMMY_FETCH ? 1 : refresh_word);
            if (half == 1 && (ONE_PASS ? __builtin_expect(refresh, 0) : refresh)) {
                // minimum of the 8 class words of queries c and 16 + c (what an earlier block's DMA brought, or 0);
                // inline asm, one query at a time: see scan_kernel_v3.hpp
                unsigned thr_addr = ONE_PASS ? thr_addr_kept : thr_addr_of(lane_id_here());
#if defined(__HIP_DEVICE_COMPILE__)
                if constexpr (ONE_PASS) asm volatile("" : "+v"(thr_addr)); // (derive a0 here, not in a register kept for it)
#endif
                const unsigned a0 = (unsigned)(size_t)(lds_void*)smem + (thr_addr & ~0x3FFu) + ((thr_addr & 0xF0u) << 1);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    u32x4 w0 = {0u, 0u, 0u, 0u}, w1 = w0;
#if defined(__HIP_DEVICE_COMPILE__)
                    if (n == 0)
                        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                                     : "=&v"(w0), "=&v"(w1) : "v"(a0) : "memory");
                    else
                        asm volatile("ds_read_b128 %0, %2 offset:512\n\tds_read_b128 %1, %2 offset:528\n\ts_waitcnt lgkmcnt(0)"
                                     : "=&v"(w0), "=&v"(w1) : "v"(a0) : "memory");
#endif
                    const unsigned key = min(min(min(w0[0], w0[1]), min(w0[2], w0[3])), min(min(w1[0], w1[1]), min(w1[2], w1[3])));
                    thr[n] = fmaxf(thr[n], key > 1u ? thr_decode(key - 1u) : -INFINITY);
                }
            }
            if constexpr (!ONE_PASS) {
                if (ragged) mask_ragged(acc, half);
                epilogue_half(acc, blk, half);
            }
        }
        if constexpr (ONE_PASS) { // after arrive() and the bound refresh: one top-k pass over both halves
            if (__builtin_expect(ragged, 0)) {
                mask_ragged(accs[0], 0);
                mask_ragged(accs[1], 1);
                mh[0] = half_max(accs[0][0]); // of the masked values
                mh[1] = half_max(accs[0][1]);
            }
            // The last two MFMAs wrote accs[1][0] and accs[1][1].  An asm statement gets no hazard padding, and the compiler pads
            // a VALU read of this MFMA shape with 8 wait states: arrive() stands in between (volatile asm keeps its order; its
            // statement is 7 instructions on its shortest path), the s_nop adds 4, query 16 + c waits 2 more.
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("s_nop 3" ::: "memory");
#endif
            const float mx0 = block_max(mh[0], accs[1][0]);
            const float mx1 = block_max(mh[1], accs[1][1]);
            epilogue_block(accs, blk, mx0, mx1);
        }
    };

    const unsigned char* first = docs_b + (int64_t)b0 * V3_DB * row_bytes;
    const unsigned char* last = docs_b + (int64_t)(b1 - 1) * V3_DB * row_bytes;
    const int64_t blk_bytes = V3_DB * row_bytes;
    constexpr int AHEAD = STAGES - 1;
    if (nb > 0) {
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) { // same operation sequence as a refresh block (vmcnt arithmetic)
            refresh_thresholds(true);
            issue(a < nb ? first + a * blk_bytes : last, a);
        }
    }
    const unsigned char* pbase = nb > AHEAD ? first + AHEAD * blk_bytes : last;
    int stage = 0, pstage = AHEAD;
    if (tid == 0) *reinterpret_cast<unsigned*>(smem + DUMP_AREA + 1024) = 0u;
    __syncthreads();
    if (nb > 0) arrive(1);
    auto advance = [&](int i) {
        if (i + AHEAD + 1 < nb) pbase += blk_bytes;
        stage = stage == STAGES - 1 ? 0 : stage + 1;
        pstage = pstage == STAGES - 1 ? 0 : pstage + 1;
    };
    if constexpr (ONE_PASS) {
        // idle_wave is constant per wave: decided once, outside the block loop.  An idle wave (all of its queries are padding,
        // scan_kernel_v3.hpp) brings its share of the documents and takes part in the block barrier, nothing else
        if (idle_wave) {
            for (int i = 0; i < nb; ++i) {
                wait_all_straight();
                issue(pbase, pstage);
                arrive(0);
                advance(i);
            }
        } else {
            for (int i = 0; i < nb; ++i) {
                wait_all_straight();
                // refresh schedule (scan_kernel_v3.hpp): i < 8 || (i & 7) == 0, as a word made by scalar arithmetic and kept in
                // an SGPR, so that arrive() reads it there and no lane mask of it is turned into a word after the chain
                int refresh_word = (int)(((unsigned)(i - 8) >> 31) | ((unsigned)((i & 7) - 1) >> 31));
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" : "+s"(refresh_word));
#endif
                block(refresh_word, b0 + i, stage, pbase, pstage);
                advance(i);
            }
        }
    } else {
        for (int i = 0; i < nb; ++i) {
            wait_all();
            block(i < 8 || (i & 7) == 0 ? 1 : 0, b0 + i, stage, pbase, pstage); // refresh schedule: scan_kernel_v3.hpp
            advance(i);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int q = qt * TN + wave * 32 + n * 16 + c;
        const size_t o = (((size_t)q * p.nsplit + split) * 4 + g) * KL;
        // The record keeps KL slots per list.  A list of KLI < KL entries repeats its last entry in the slots it does not
        // have.  What merge_select_body (aux_kernels.hpp) makes of that:
        //   * its bound on what a full list dropped is the list's LAST slot when that slot holds a row: here the KLI-th
        //     score of a list that filled -- every row this list pushed out or refused scored no more than that -- and
        //     (-inf, IDX_NONE) for a list that never filled, which dropped nothing and leaves the bound alone;
        //   * the repeats add no candidate: the slots of one list go to consecutive lanes of the merge, so the copies of
        //     an entry sit in different lanes' lists; when the entry is the wave-wide best every lane that holds it has it
        //     at its head and pops it in the same round, and the round counts once.  The pool holds each row once.
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            p.part_s[o + i] = ls[n][i < KLI ? i : KLI - 1];
            p.part_i[o + i] = li[n][i < KLI ? i : KLI - 1];
        }
    }
}

} // namespace mips
