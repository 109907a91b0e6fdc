// Host side of libmips_hip.so, part 2 of 3 (included by mips_hip.hip): which scan kernel answers which search -- the instance
// tables (one row per shipped scan-kernel instance, every family), pool_policy (no HIP calls: the ONE place that decides which
// pool the first scan of a search selects from -- K', two-stage, optimistic -- and counts fast_skip down) and launch_search<K'>
// in three steps with a plain struct between them: choose_scan (no HIP calls: kernel row, tiles, lists, splits, XCD groups, grid),
// launch_scan (the ONE place that launches a scan kernel) and launch_tail (merge_select -> rescore_rank with the margin check).
// All of them read the launch's view of the index, its staged queries and its switches from the SearchCall they are handed,
// and write nothing on the index but scratch, the event ring and last_kernel.  DESIGN.md section 4, "Dispatch".
#pragma once

namespace {

// ---- The shipped scan-kernel instances, ONE ROW EACH: what selects an instance (row pitch, document cache policy and, as the
// family needs, published rank and query tile), what it needs (threads, dynamic LDS bytes), its entry point, the name rocprofv3
// prints, and which by-value argument struct the entry takes.  choose_scan looks the row up; a new pitch / list length / policy
// is one more row here.  The name is spelled from the same tokens as the entry point, so the two cannot drift apart.
enum class ScanArgKind { Bf16, F8, E8 }; // mips::ScanArgs / ScanArgsF8 / ScanArgsE8
struct ScanInstance {
    int ld;            // row pitch in elements
    bool nt;           // non-temporal document DMA (searches of one query tile: every block has a single reader)
    int pub;           // rank every sub-list publishes (scan_kernel_v4 / k3 / e8: pools of 8 pub); 0 where the family has no such axis
    int tile;          // scan_kernel_e8: 16-query column blocks per workgroup (1 / 2 / 4); 0 elsewhere
    int threads;       // per workgroup
    int lds;           // dynamic LDS bytes
    const void* fn;    // __global__ entry taking its argument struct by value
    const char* name;  // printf format; the rows of per-K' tables (scan_kernel_v3 / f8 / generic) take K' as their one %d
    ScanArgKind args;
};
inline const ScanInstance* find_instance(const ScanInstance* t, int n, int ld, bool nt, int pub = 0, int tile = 0) {
    for (int i = 0; i < n; ++i)
        if (t[i].ld == ld && t[i].nt == nt && t[i].pub == pub && t[i].tile == tile) return &t[i];
    return nullptr;
}
#define MIPS_TABLE_END(t) *n = (int)(sizeof t / sizeof t[0]); return t

// scan_kernel_v3 / v4: ring + class-word copies (1 KiB per wave) + dump area + arrival counter
constexpr int ring_scan_lds(int ld, int waves, int stages) { return stages * mips::V3_DB * ld * 2 + waves * 1024 + 1024 + 16; }
// scan_kernel_v4: 16x16x32 MFMA, 8 waves x 32 queries, 3-stage ring, 4 sub-lists of 6 per (query, split)
#define MIPS_V4_ROW(KS, NT, PUB)                                                                                   \
    {KS * 32, NT, PUB, 0, 512, ring_scan_lds(KS * 32, 8, 3), (const void*)mips::scan_kernel_v4<6, KS, 2, 0, NT, PUB>, \
     "mips::scan_kernel_v4<6, " #KS ", 2, 0, " #NT ", " #PUB ">", ScanArgKind::Bf16}
#define MIPS_V4_PITCH(KS) MIPS_V4_ROW(KS, false, 1), MIPS_V4_ROW(KS, true, 1), MIPS_V4_ROW(KS, false, 4), MIPS_V4_ROW(KS, true, 4)
inline const ScanInstance* v4_instances(int* n) {
    static const ScanInstance t[] = {MIPS_V4_PITCH(12), MIPS_V4_PITCH(16), MIPS_V4_PITCH(20), MIPS_V4_PITCH(24)};
    MIPS_TABLE_END(t);
}
// scan_kernel_v3: 32x32x16 MFMA, true K'-entry lists.  K' <= 10 at pitch <= 768: 8 waves (two per SIMD), 3-stage ring; K' = 16 /
// 32 there: 4 waves (one per SIMD, 512 registers), 3-stage ring; pitch 1024 (256 fragment registers): 4 waves, 2 stages of 64 KiB
#define MIPS_V3_ROW8(KS16, NT)                                                                                     \
    {KS16 * 16, NT, 0, 0, 512, ring_scan_lds(KS16 * 16, 8, 3), (const void*)mips::scan_kernel_v3<KL, KS16, 1, 2, true, 0, 2, 8, 3, true, NT>, \
     "mips::scan_kernel_v3<%d, " #KS16 ", 1, 2, true, 0, 2, 8, 3, true, " #NT ", 8>", ScanArgKind::Bf16}
#define MIPS_V3_ROW4(KS16, NT)                                                                                     \
    {KS16 * 16, NT, 0, 0, 256, ring_scan_lds(KS16 * 16, 4, 3), (const void*)mips::scan_kernel_v3<KL, KS16, 1, 4, true, 0, 2, 4, 3, true, NT>, \
     "mips::scan_kernel_v3<%d, " #KS16 ", 1, 4, true, 0, 2, 4, 3, true, " #NT ", 8>", ScanArgKind::Bf16}
#define MIPS_V3_ROW1024(NT)                                                                                        \
    {1024, NT, 0, 0, 256, ring_scan_lds(1024, 4, 2), (const void*)mips::scan_kernel_v3<KL, 64, 1, 4, false, 0, 2, 4, 2, true, NT>, \
     "mips::scan_kernel_v3<%d, 64, 1, 4, false, 0, 2, 4, 2, true, " #NT ", 8>", ScanArgKind::Bf16}
template <int KL>
const ScanInstance* v3_instances(int* n) {
    if constexpr (KL <= 10) {
        static const ScanInstance t[] = {MIPS_V3_ROW8(8, false),  MIPS_V3_ROW8(8, true),  MIPS_V3_ROW8(16, false), MIPS_V3_ROW8(16, true),
                                         MIPS_V3_ROW8(24, false), MIPS_V3_ROW8(24, true), MIPS_V3_ROW8(32, false), MIPS_V3_ROW8(32, true),
                                         MIPS_V3_ROW8(40, false), MIPS_V3_ROW8(40, true), MIPS_V3_ROW8(48, false), MIPS_V3_ROW8(48, true),
                                         MIPS_V3_ROW1024(false),  MIPS_V3_ROW1024(true)};
        MIPS_TABLE_END(t);
    } else {
        static const ScanInstance t[] = {MIPS_V3_ROW4(16, false), MIPS_V3_ROW4(16, true), MIPS_V3_ROW4(32, false), MIPS_V3_ROW4(32, true),
                                         MIPS_V3_ROW4(48, false), MIPS_V3_ROW4(48, true), MIPS_V3_ROW1024(false), MIPS_V3_ROW1024(true)};
        MIPS_TABLE_END(t);
    }
}

// scan_kernel_k3 (pitch 1024, 4 wave pairs x 48 queries, 8 sub-lists of 4): ring + the pairs' class-word copies + exchange slots +
// counters (+ 256 bytes that no longer have a user: the byte count the kernel was measured and tuned with)
constexpr int k3_lds() { return 2 * mips::V3_DB * 1024 * 2 + 4 * 1536 + 8 * 3072 + 64 + 256; }
// pool of 8 PUB candidates: every sub-list vouches for its PUB-th best
#define MIPS_K3_ROW(PUB) \
    {1024, false, PUB, 0, 512, k3_lds(), (const void*)mips::scan_kernel_k3<4, 32, 2, 0, PUB>, "mips::scan_kernel_k3<4, 32, 2, 0, " #PUB ">", ScanArgKind::Bf16}
inline const ScanInstance* k3_instances(int* n) {
    static const ScanInstance t[] = {MIPS_K3_ROW(1), MIPS_K3_ROW(2), MIPS_K3_ROW(4)};
    MIPS_TABLE_END(t);
}

// all-e4m3 index.  Both kernels: ring + threshold words + dump area + arrival counter
// scan_kernel_f8x: 16x16x128 MFMA, 64-document blocks, 4 sub-lists of 6 (k <= 5, row pitches up to 768 bytes)
constexpr int f8x_lds(int ld) { return 3 * mips::F8X_DB * ld + 8 * 1024 + 1024 + 16; }
#define MIPS_F8X_ROW(LD, NT) \
    {LD, NT, 0, 0, 512, f8x_lds(LD), (const void*)mips::scan_kernel_f8x<6, LD, 2, 0, NT>, "mips::scan_kernel_f8x<6, " #LD ", 2, 0, " #NT ">", ScanArgKind::F8}
inline const ScanInstance* f8x_instances(int* n) {
    static const ScanInstance t[] = {MIPS_F8X_ROW(256, false), MIPS_F8X_ROW(256, true), MIPS_F8X_ROW(512, false),
                                     MIPS_F8X_ROW(512, true),  MIPS_F8X_ROW(768, false), MIPS_F8X_ROW(768, true)};
    MIPS_TABLE_END(t);
}
// scan_kernel_f8: 32x32x64 MFMA, 32-document blocks, true K'-entry lists (K' <= 16)
constexpr int f8_lds(int ld) { return 3 * mips::V3_DB * ld + 8 * 1024 + 1024 + 16; }
#define MIPS_F8_ROW(LD, NT) \
    {LD, NT, 0, 0, 512, f8_lds(LD), (const void*)mips::scan_kernel_f8<KL, LD, 2, NT>, "mips::scan_kernel_f8<%d, " #LD ", 2, " #NT ">", ScanArgKind::F8}
template <int KL>
const ScanInstance* f8_instances(int* n) {
    if constexpr (KL <= 16) {
        static const ScanInstance t[] = {MIPS_F8_ROW(256, false), MIPS_F8_ROW(256, true), MIPS_F8_ROW(512, false),  MIPS_F8_ROW(512, true),
                                         MIPS_F8_ROW(768, false), MIPS_F8_ROW(768, true), MIPS_F8_ROW(1024, false), MIPS_F8_ROW(1024, true)};
        MIPS_TABLE_END(t);
    } else {
        *n = 0;
        return nullptr;
    }
}

// scan_kernel_e8 (e4m3 documents x bf16 queries): instance by row pitch, query tile, document cache policy and pool.
// Tiles of 16 / 32 / 64 queries (ncb = 1 / 2 / 4).  K parts (kw): 8 for the 16-query tile, 4 beyond (half the partial sums
// through LDS: two slot buffers -- one barrier per block -- then fit for every tile but 64 queries at pitch 1024); ring depth 4
// where 160 KiB allow it.  The tile follows from the query count alone:
inline int e8_ncb(int64_t nq) { return nq <= 16 ? 1 : nq <= 32 ? 2 : 4; }
// ring + slot buffer(s) + class words + dump + counters
constexpr int e8_lds(int ld, int ncb, int stages, bool pipe, int kw) {
    return stages * mips::V3_DB * ld + (pipe ? 2 : 1) * kw * (2 * ncb) * 1024 + 2048 + 1024 + 64;
}
#define MIPS_E8_ROW(LDB, NCB, STG, NT, PUB, PIPE, KW)                                                                             \
    {LDB, NT, PUB, NCB, 512, e8_lds(LDB, NCB, STG, PIPE, KW), (const void*)mips::scan_kernel_e8<6, LDB, NCB, STG, NT, PUB, PIPE, KW>, \
     "mips::scan_kernel_e8<6, " #LDB ", " #NCB ", " #STG ", " #NT ", " #PUB ", " #PIPE ", " #KW ">", ScanArgKind::E8}
// The 16- and 32-query tiles hold the whole search (e8_ncb ties the tile to nq), so their document blocks always have a single
// reader: only the non-temporal instance exists.  Shared blocks (nt = false) are the 64-query tile's alone.
#define MIPS_E8_PITCH(LDB, PUB)  /* pitch <= 768 */                                                          \
    MIPS_E8_ROW(LDB, 1, 4, true, PUB, true, 8), MIPS_E8_ROW(LDB, 2, 4, true, PUB, true, 4),                  \
    MIPS_E8_ROW(LDB, 4, 3, true, PUB, true, 4), MIPS_E8_ROW(LDB, 4, 3, false, PUB, true, 4)
#define MIPS_E8_PITCH_1024(PUB)  /* 3-stage ring throughout, one slot buffer under the 64-query tile */      \
    MIPS_E8_ROW(1024, 1, 3, true, PUB, true, 8), MIPS_E8_ROW(1024, 2, 3, true, PUB, true, 4),                \
    MIPS_E8_ROW(1024, 4, 3, true, PUB, false, 4), MIPS_E8_ROW(1024, 4, 3, false, PUB, false, 4)
#define MIPS_E8_POOL(PUB) MIPS_E8_PITCH(256, PUB), MIPS_E8_PITCH(512, PUB), MIPS_E8_PITCH(768, PUB), MIPS_E8_PITCH_1024(PUB)
inline const ScanInstance* e8_instances(int* n) {
    static const ScanInstance t[] = {MIPS_E8_POOL(1), MIPS_E8_POOL(2), MIPS_E8_POOL(4)};
    MIPS_TABLE_END(t);
}

// sq8_scan_kernel (8-bit codes x bf16 queries, MIPS_DTYPE_SQ8): scan_kernel_e8's plan and instance set -- same pitches, tiles,
// pools, ring depths and LDS bytes -- with the conversion step u8 -> bf16
#define MIPS_SQ8_ROW(LDB, NCB, STG, NT, PUB, PIPE, KW)                                                                             \
    {LDB, NT, PUB, NCB, 512, e8_lds(LDB, NCB, STG, PIPE, KW), (const void*)mips::sq8_scan_kernel<6, LDB, NCB, STG, NT, PUB, PIPE, KW>, \
     "mips::sq8_scan_kernel<6, " #LDB ", " #NCB ", " #STG ", " #NT ", " #PUB ", " #PIPE ", " #KW ">", ScanArgKind::E8}
#define MIPS_SQ8_PITCH(LDB, PUB)                                                                               \
    MIPS_SQ8_ROW(LDB, 1, 4, true, PUB, true, 8), MIPS_SQ8_ROW(LDB, 2, 4, true, PUB, true, 4),                  \
    MIPS_SQ8_ROW(LDB, 4, 3, true, PUB, true, 4), MIPS_SQ8_ROW(LDB, 4, 3, false, PUB, true, 4)
#define MIPS_SQ8_PITCH_1024(PUB)                                                                               \
    MIPS_SQ8_ROW(1024, 1, 3, true, PUB, true, 8), MIPS_SQ8_ROW(1024, 2, 3, true, PUB, true, 4),                \
    MIPS_SQ8_ROW(1024, 4, 3, true, PUB, false, 4), MIPS_SQ8_ROW(1024, 4, 3, false, PUB, false, 4)
#define MIPS_SQ8_POOL(PUB) MIPS_SQ8_PITCH(256, PUB), MIPS_SQ8_PITCH(512, PUB), MIPS_SQ8_PITCH(768, PUB), MIPS_SQ8_PITCH_1024(PUB)
inline const ScanInstance* sq8_instances(int* n) {
    static const ScanInstance t[] = {MIPS_SQ8_POOL(1), MIPS_SQ8_POOL(2), MIPS_SQ8_POOL(4)};
    MIPS_TABLE_END(t);
}

// generic scan_kernel<K'>: any row pitch (a multiple of 64), the [hi | lo] planes of the fp32-exact index
template <int KL>
const ScanInstance* generic_instance() {
    static const ScanInstance row = {0,  false, 0, 0, mips::SCAN_THREADS, mips::SCAN_LDS_BYTES, (const void*)mips::scan_kernel<KL>,
                                     "mips::scan_kernel<%d>", ScanArgKind::Bf16};
    return &row;
}

// ---- What choose_scan decides and the other two steps carry out
struct ScanPlan {
    const ScanInstance* row; // the kernel
    bool stationary;         // a query-stationary kernel: shares insert bounds through the class words (ix->cur.gthr)
    bool f32x;               // fp32-exact mode: generic kernel over the [hi | lo] planes, three k segments
    int tn, tm;              // queries per workgroup, documents per scheduling unit ("tile")
    int lists, list_len;     // running lists per (query, split), entries of each
    int nqt, ntiles;         // query tiles, document tiles
    int nsplit, tps;         // index splits (a multiple of 8), document tiles per split
    int qgroups, qt_per_group;
    int grid;
    int64_t nq_pad;
    size_t ncand;            // candidates per query in the lists: nsplit * lists * list_len
};

// ---- Which pool a search selects from: ONE policy, no HIP calls.  pool_policy maps (index, nq, k, outputs, split, margin mode,
// knobs, fast_skip) to the list length K' of the first scan and to what is optimistic about it; search_impl switches on K',
// choose_scan reads SearchCall::optimistic and only picks the instance.
struct PoolPolicy {
    int kl;          // K' = 8 / 10 / 16 / 32 >= k + 3: the pool merge_select hands to the exact re-score
    bool fast;       // stage 1 of the two-stage search of an fp32-exact index (scan of the bf16 rows_hi)
    bool optimistic; // the scan takes its pool from sub-lists (scan_kernel_v4 / k3), not from true K'-entry lists
    bool recheck;    // fast or a pool picked for optimism: flagged queries get a second scan with true K' = 32 lists whatever K'
                     // was, and a synchronising call that flags too many of them starts the fast_skip countdown
};
// row pitches of scan_kernel_v4 (16x16x32 MFMA shape, sub-lists of 6): 384 .. 768 (at 256 the shorter chain no longer pays:
// 2.03 vs 2.00 ms).  With pitch 1024 beyond 256 queries (scan_kernel_k3) these are the optimistic pitch windows
inline bool v4_pitch(int ld) { return ld % 128 == 0 && ld >= 384 && ld <= 768; }

// The MFMA scores only SELECT a pool of K' candidates that is then re-scored exactly.  What is GUARANTEED
// to reach the pool per (query, split): the 32x32 kernels (scan_kernel_v3 / f8 / generic) keep lists of K' entries, so MFMA
// ranks 1 .. K'; the 16x16 kernels (scan_kernel_v4 / f8x: bf16 pitch 384 .. 768 or fp8 pitch <= 768, k <= 5, more than one
// query tile) keep 4 sub-lists of 6, so MFMA ranks 1 .. 6 = k + 1 for certain and 7 .. 8 unless 6 better documents share the
// sub-list (rows congruent mod 16 within a split).  Queries whose k-th exact score is too close to what the pool may have lost
// are detected by the re-score and settled by finish_margin.
inline PoolPolicy pool_policy(mips_index* ix, int64_t nq, int k, bool out_dev, bool split, int margin) {
    const bool certifies = call_certifies(margin, out_dev) && !split; // (split tail: the certificate, if any, is part of the tail)
    const bool bf16_rows = ix->plane == 0 && ix->esize == 2 && !ix->mixed;
    const bool knob = ix->opt_f32_fast != 0; // "f32_fast" / "optimistic": one switch for all three below
    // fp32-exact index: two-stage search when the call may synchronise anyway (see mips_index: rows_hi), or always
    // ("f32_fast" = 2).  Stage 1 keeps K' = 32 lists where the bf16 kernels have them (pitch 256 / 512 / 768): the pool's bound
    // is then the ~33rd best score, far enough below the k-th for the widened margin to certify nearly every query on
    // well-separated data (with K' = 8 pools 44 % of the queries of a Gaussian test set went to the second stage).
    // (round 3: row pitch 1024 has true K' = 32 lists as well -- with pools of 8, all it had before, 46 % of a Gaussian test set
    // went to the second stage and stage 1 did not pay)
    // k <= 13 only: the pool is 32 wide whatever k, and the widened margin (representation error of bf16(x) . bf16(q)) has to
    // fit between the k-th and the 33rd score -- at k = 20 .. 29 nearly every query of a Gaussian test set was flagged, and an
    // exact pass per 8 flagged queries costs far more than the three-segment scan saves.
    // (pools of 32, not 16: with the 16th best score as the bound 30 of 4096 Gaussian queries went to the second stage, and a
    // second stage of even one query tile costs more than stage 1 saved -- 22 ms per call instead of 5.4)
    const bool fast = ix->plane > 0 && ix->hp > 0 && ix->hp <= 1024 && k <= 13 && knob && margin != 0 && !split &&
                      (ix->opt_f32_fast == 2 || certifies);
    // bf16 rows at pitch 1024, k <= 5, a large index, a call that certifies: pool of 16 (scan_kernel_k3 with every sub-list
    // vouching for its 2nd best).  The MFMA error bound at K = 1024 (0.14 on unit-variance data) reaches from the 5th exact score
    // to the 8th best approximate one for one Gaussian query in ~3000 at 2^22 rows, and each flagged query costs a pass over the
    // index (3 ms there); the 16th best is out of reach.  Small indexes keep the pool of 8 (their exact pass is cheap), and so
    // do forced kernels.
    const bool deep_1024 = k <= 5 && bf16_rows && ix->ld == 1024 && nq > 256 && ix->ntotal >= (1ll << 21) && certifies && knob &&
                           ix->opt_variant == 0;
    // bf16 index, a call that certifies, 8 <= k <= 29: pool of 32 out of the 16x16x32 kernel's sub-lists (round 3: k = 14 .. 29
    // as well -- the class words vouch for 32 documents, what the sub-lists of 6 may have dropped is bounded, the margin check
    // decides per query; at pitch 1024 out of scan_kernel_k3's, every sub-list vouching for its 4th best).
    const bool opt = k > 7 && bf16_rows && certifies && knob && (v4_pitch(ix->ld) || (ix->ld == 1024 && nq > 256));
    // At most one of the three holds (fp32-exact index / k <= 5 / k >= 8).  The optimistic scan pays while few queries need the
    // second one: a call that sent too many there (scan_and_finish) has the next ones skip it -- "f32_fast" = 2 never counts down
    // (setting the knob clears fast_skip, and scan_and_finish does not arm it then)
    bool recheck = fast || deep_1024 || opt;
    if (recheck && ix->opt_f32_fast == 1 && ix->fast_skip > 0) {
        --ix->fast_skip;
        recheck = false;
    }
    PoolPolicy p;
    p.fast = fast && recheck;
    p.recheck = recheck;
    // sub-list pools exist at the optimistic pitch windows of the SCANNED rows, and forced kernels ("variant") keep true lists
    const int pitch = p.fast ? ix->hp : ix->ld;
    p.optimistic = recheck && ix->opt_variant == 0 && (v4_pitch(pitch) || (pitch == 1024 && nq > 256));
    // k + 1 = 6 is what Mips.search fetches for top_k = 5 with ignore_indexes (mips.py:388-398): K' = 10 serves k <= 7
    p.kl = p.fast ? 32 : k <= 5 ? (recheck ? 16 : 8) : k <= 7 ? 10 : (recheck || k > 13) ? 32 : 16;
    return p;
}

// Step 1, no HIP calls: the kernel row and the launch geometry of a search of nq queries for pools of K'
template <int KL>
int choose_scan(const mips_index* ix, const SearchCall& c, int64_t nq, ScanPlan& pl) {
    // variant 3 (query-stationary, LDS-DMA): the whole K of a wave's 32 queries lives in its VGPRs, so it
    // exists for a few row lengths only: 256 / 512 / 768 (8 waves, 2 per SIMD) and 1024 (4 waves, 1 per SIMD)
    int variant = ix->opt_variant;
    // scan_kernel_v4 (16x16x32 MFMA shape, 4 sub-lists of 6): row pitch 384 .. 768, k <= 5, bf16 storage.  It is the default
    // there when more than one query tile shares the document stream (the MFMA-bound regime, where the shape's
    // higher clock pays: 4.54 vs 4.78 ms at BASELINE config 2); single-tile searches are HBM-bound and keep
    // scan_kernel_v3's non-temporal document DMA.  "variant" = 3 / 4 forces one of the two.  Optimistic pools (K' = 16 / 32,
    // pool_policy) come from it as well
    const bool v4_opt = c.optimistic && c.ld != 1024;
    const bool v4_shape = v4_pitch(c.ld) && (KL == 8 || v4_opt) && ix->esize == 2 && c.plane == 0;
    const bool v4_forced = variant == 4 && v4_shape;
    const bool v4_auto = variant == 0 && v4_shape;
    if (variant != 1 && variant != 3) variant = 3; // (4 was decided above; the rest of the function only knows 1 and 3)
    const bool v3_dim = (c.ld % 128 == 0 && c.ld <= 768) || c.ld == 1024;
    const bool v3_long = c.ld == 256 || c.ld == 512 || c.ld == 768 || c.ld == 1024; // pitches with K' = 16 / 32 instances
    constexpr bool kl_short = KL <= 10; // K' = 8 / 10 lists fit the 8-wave (two per SIMD) configuration
    const bool f8 = ix->esize == 1; // e4m3 index: scan_kernel_f8 only (row lengths 256..1024, K' <= 16)
    const bool f32x = c.plane > 0; // fp32-exact mode: generic kernel over the [hi | lo] planes, three k segments
    // e4m3 documents x bf16 queries (MIPS_DTYPE_FP8_E4M3_DOCS): scan_kernel_e8, tiles of 32 queries (up to 32 queries, and at
    // row pitch 1024) or 64; pools of 8 / 10 / 16 / 32 out of 8 sub-lists of 6 per (query, split), the class words vouching for
    // 8 PUB documents
    // (MIPS_DTYPE_SQ8: the same plan over 8-bit codes, sq8_scan_kernel)
    const bool e8 = ix->mixed;
    if (e8) {
        if (c.ld % 256 != 0 || c.ld > 1024) return fail(MIPS_E_UNSUPPORTED, "one-byte rows x bf16 queries: d must pad to 256/512/768/1024");
        variant = 3;
    } else if (f8) {
        if (c.ld % 256 != 0 || c.ld > 1024 || KL > 16) return fail(MIPS_E_UNSUPPORTED, "fp8 index: d must pad to 256/512/768/1024 and k <= 13");
        variant = 3;
    } else if (f32x || !v3_dim || (!kl_short && !v3_long && !v4_opt)) {
        variant = 1; // no query-stationary configuration: generic tiles
    }
    // K' = 8 / 10 (k <= 7) at d <= 768: 8 waves, two per SIMD (256 registers each, no spill up to K' = 10).
    // Longer lists or d = 1024 do not fit next to the fragments there: 4 waves, one per SIMD, 512 registers,
    // 128 queries per workgroup.
    const int v3_waves = (!f8 && !v4_opt && (c.ld == 1024 || !kl_short)) ? 4 : 8;
    // fp8: scan_kernel_f8x (16x16x128 MFMA shape, 64-document blocks, 4 sub-lists of 6) for k <= 5 and row pitches
    // up to 768 bytes; scan_kernel_f8 (32x32x64, 32-document blocks) otherwise or when "variant" = 3 asks for it
    const bool want_f8x = f8 && !e8 && KL == 8 && c.ld <= 768 && ix->opt_variant != 3;
    // scan_kernel_k3: row pitch 1024, K split over wave pairs of 48 queries each -- 192 stationary queries per CU, a third less
    // L2 -> LDS fill per flop than the 128-query configuration of scan_kernel_v3, which is what bounds pitch 1024 (measured
    // 30.6 vs 31.3 ms at 2^22 x 1024 for a pair kernel with 128 queries: profiles/r2_pitch1024 -- both sat on that fill).
    // Default there once several 192-query tiles share the document stream (the MFMA-bound regime); smaller searches keep the
    // 128-query configuration ("variant" = 7 / 3 force one).
    // (round 3, later: pools of 16 / 32 out of scan_kernel_k3's sub-lists, every sub-list vouching for its 2nd / 4th best -- the
    // "optimistic" pools of scan_kernel_v4 at this pitch: first stage of the fp32-exact search at d in (768, 1024], bf16 searches
    // with 8 <= k <= 29, and k <= 5 on large indexes, where the MFMA error bound at K = 1024 reaches the 8th best score of one
    // query in a few thousand and a flagged query costs a pass over the index)
    const bool k3_opt = c.optimistic && c.ld == 1024;
    const bool k3_shape = c.ld == 1024 && (KL == 8 || k3_opt) && ix->esize == 2 && c.plane == 0;
    const bool want_k3 = k3_opt || (k3_shape && (ix->opt_variant == 7 || (ix->opt_variant == 0 && nq > 256)));
    constexpr int K3_KLL = 4; // entries per sub-list (the third accumulator set is paid for with shorter lists)
    // (a variant on 16-document stages -- 4-stage ring, three blocks in flight, one barrier per 16 documents -- was built and
    // measured 18 % SLOWER, 34.8 vs 29.5 ms at 2^22 x 1024: profiles/r3_pitch1024/README.md; what parks the waves is the barrier
    // itself, not the landing of the pieces)
    const int tm = variant == 1 ? mips::TM : want_f8x ? mips::F8X_DB : mips::V3_DB; // documents per scheduling unit ("tile")
    const int tn = variant == 1 ? mips::TN : e8 ? 16 * e8_ncb(nq) : want_k3 ? 192 : v3_waves * 32; // queries per workgroup
    const int wg_target = variant == 1 ? 512 : 256;                   // resident workgroups on 256 CUs
    const int nqt = (int)((nq + tn - 1) / tn);
    // One query tile (round 2): with non-temporal document DMA the 16x16x32 kernel ties scan_kernel_v3 in the HBM-bound
    // regime on large indexes (3.80 vs 3.82 ms at Q = 64 on 2^24 rows), loses 3-8 % on short streams at Q = 8 (0.315 vs
    // 0.304 ms at 2^20 rows, 0.091 vs 0.084 at 2^17) and wins once several waves multiply (3.89 vs 4.15 ms at Q = 128,
    // 5.57 vs 5.98 at Q = 256; profiles/r2_final/ab_single_tile.md): scan_kernel_v3 up to 64 queries, v4 beyond
    const bool want_v4 = v4_forced || v4_opt || (v4_auto && (nqt > 1 || nq > 64));

    // ---- the kernel row.  One query tile: every document block has a single reader -> non-temporal document DMA (HBM-bound
    // regime: 5.5 -> 5.9 TB/s at pitch 768)
    const bool nt = nqt == 1;
    int nrow = 0;
    const ScanInstance* rows = nullptr;
    if (e8) { // pools of 8 PUB: K' = 8 / 10, 16 / 32
        rows = ix->sq8 ? sq8_instances(&nrow) : e8_instances(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, nt, KL <= 8 ? 1 : KL <= 16 ? 2 : 4, e8_ncb(nq));
    } else if (want_k3) { // pool of 8 PUB candidates: every sub-list vouches for its PUB-th best
        rows = k3_instances(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, false, KL / 8);
    } else if (want_v4) { // pools of 8 (PUB 1) or, optimistic, of 16 / 32: every sub-list vouches for its 4th best (8 x 4 = 32 documents)
        rows = v4_instances(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, nt, v4_opt ? 4 : 1);
    } else if (want_f8x) {
        rows = f8x_instances(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, nt);
    } else if (f8) {
        rows = f8_instances<KL>(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, nt);
    } else if (variant == 1) {
        pl.row = generic_instance<KL>();
    } else {
        // K' = 8 / 10; true K' = 16 / 32 lists: pitches 256 / 512 / 768 and (round 3) 1024 -- k = 8 .. 29 and stage 1 of the
        // two-stage fp32 search at Longformer-large width no longer fall back to the generic kernel there
        rows = v3_instances<KL>(&nrow);
        pl.row = find_instance(rows, nrow, c.ld, nt);
    }
    if (pl.row == nullptr) return fail(MIPS_E_UNSUPPORTED, "no scan-kernel instance for row pitch %d, K' = %d", c.ld, KL);
    pl.stationary = variant == 3;
    pl.f32x = f32x;
    pl.tn = tn;
    pl.tm = tm;
    pl.nqt = nqt;
    pl.nq_pad = query_pad(ix, nq);
    pl.lists = (want_k3 || e8) ? 8 : (want_v4 || want_f8x) ? 4 : 2; // running lists per (query, split)
    // scan_kernel_v4 / f8x / e8 keep sub-lists of 6 per (query, split); each needs k (<= 5) + 1 entries only, the re-score pool
    // is still the K' best of their union
    constexpr int V4_KLL = 6;
    pl.list_len = want_k3 ? K3_KLL : (want_v4 || want_f8x || e8) ? V4_KLL : KL; // entries per running list
    const int ntiles = (int)((ix->ntotal + tm - 1) / tm);
    // Index splits (a multiple of 8: one XCD group each).  The grid nqt x nsplit should come in whole
    // "rounds" of wg_target resident workgroups: among the multiples of 8 up to 64 take the one whose last
    // round is fullest (ties: fewer splits = longer streams, fewer lists to merge).
    int nsplit;
    if (c.nsplit > 0) {
        nsplit = (int)round_up(c.nsplit, 8);
    } else {
        nsplit = (int)round_up(std::max(1, (wg_target + nqt - 1) / nqt), 8);
        double best = -1.0;
        for (int cand = 8; cand <= 64 && (int64_t)nqt * cand <= 16 * (int64_t)wg_target; cand += 8) {
            const int64_t wgs = (int64_t)nqt * cand;
            if (wgs < wg_target && cand < nsplit) continue; // never leave CUs idle on purpose
            const double eff = (double)wgs / (double)(((wgs + wg_target - 1) / wg_target) * wg_target);
            if (eff > best + 0.02) {
                best = eff;
                nsplit = cand;
            }
        }
    }
    nsplit = (int)std::min<int64_t>(nsplit, round_up(ntiles, 8));
    const int tps = (ntiles + nsplit - 1) / nsplit;
    // query-tile groups per XCD.  Variant 1 re-reads its query tiles from L2 for every document tile:
    // keep an XCD's query working set at <= 8 tiles (1.5 MiB of its 4 MiB L2).  Variant 3 holds the
    // queries in registers: give every XCD as many query tiles of ONE split as possible instead, so a
    // document block is fetched from HBM once and served to the other tiles from that XCD's L2.
    int qgroups = ix->opt_qgroups;
    if (qgroups != 1 && qgroups != 2 && qgroups != 4 && qgroups != 8) {
        if (variant == 1) qgroups = nqt <= 8 ? 1 : nqt <= 16 ? 2 : nqt <= 32 ? 4 : 8;
        else qgroups = nqt <= 32 ? 1 : nqt <= 64 ? 2 : nqt <= 128 ? 4 : 8;
    }
    const int qt_per_group = (nqt + qgroups - 1) / qgroups;
    pl.ntiles = ntiles;
    pl.nsplit = nsplit;
    pl.tps = tps;
    pl.qgroups = qgroups;
    pl.qt_per_group = qt_per_group;
    pl.grid = qt_per_group * qgroups * nsplit;
    pl.ncand = (size_t)nsplit * pl.lists * pl.list_len;
    return MIPS_OK;
}

// Step 2: the ONE place that launches a scan kernel.  `a`: the common arguments; the e4m3 families wrap them
inline int launch_scan(mips_index* ix, const SearchCall& c, const ScanPlan& pl, const mips::ScanArgs& a, int name_arg, hipStream_t st) {
    const ScanInstance& e = *pl.row;
    mips::ScanArgsF8 f8a;
    mips::ScanArgsE8 e8a;
    const void* arg = &a;
    if (e.args == ScanArgKind::F8) {
        f8a.docs = c.rows;
        f8a.qbuf = (const uint8_t*)c.qbuf;
        f8a.c = a;
        arg = &f8a;
    } else if (e.args == ScanArgKind::E8) {
        e8a.docs = c.rows;
        e8a.c = a;
        arg = &e8a;
    }
    const int slot = ix->ev_next;
    const bool timed = c.timed && ix->timing_armed; // (the bench's event window times the first scan of a search only)
    HIP_TRY(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, e.lds));
    if (timed) HIP_TRY(hipEventRecord(ix->ev0[slot], st));
    void* kargs[] = {const_cast<void*>(arg)};
    HIP_TRY(hipLaunchKernel(e.fn, dim3((unsigned)pl.grid), dim3((unsigned)e.threads), kargs, (size_t)e.lds, st));
    if (c.timed) set_kernel_name(ix, e.name, name_arg);
    HIP_TRY(hipGetLastError());
    if (timed) {
        HIP_TRY(hipEventRecord(ix->ev1[slot], st));
        ix->ev_next = (slot + 1) % mips_index::kEvRing;
        if (++ix->ev_count == mips_index::kEvRing) ix->timing_armed = false; // window full
    }
    return MIPS_OK;
}

// Step 3: the tail behind the scan -- (1) K' best candidates per query by MFMA score, (2) lane-packed exact re-score + final
// order, with the margin check's buffers.  tail_st: stream of the two launches when `split` (else the scan's own).
// *nflag_dev: where the re-score counts the queries it flags (nullptr: the margin check is off)
template <int KL>
int launch_tail(mips_index* ix, const SearchCall& c, const ScanPlan& pl, const mips::ScanArgs& a, int64_t nq, int k, float* d_out_s, int64_t* d_out_i,
                int64_t* d_out_packed, int64_t idx_offset, hipStream_t st, unsigned** nflag_dev, hipStream_t tail_st, bool split) {
    const bool f32x = pl.f32x, e8 = ix->mixed, f8 = ix->esize == 1;
    int rc;
    mips::MergeArgs m;
    m.part_s = a.part_s;
    m.part_i = a.part_i;
    m.ncand = (int)pl.ncand;
    const bool f32r = f32x || c.stage1; // exact re-score on the fp32 rows (stage 1 of the two-stage search included)
    m.docs = f32r ? (const void*)ix->rows_f32.p : (const void*)c.rows;
    m.qbuf = f32r ? c.qf32 : (const void*)a.qbuf;
    m.ld = c.stage1 ? c.rescore_ld : f32x ? c.plane : c.ld;
    m.k = k;
    m.metric = c.metric;
    m.phi = ix->phi;
    m.idx_offset = idx_offset;
    m.out_s = d_out_s;
    m.out_i = d_out_i;
    m.out_packed = d_out_packed;
    m.err = a.err;
    m.sticky = ix->sticky_dev;
    m.ll = pl.list_len;
    m.pre_bnd = nullptr;
    m.npre = 0;
    m.bnd = nullptr;
    m.flag = nullptr;
    m.nflag = nullptr;
    m.xmax2 = ix->xmax2_dev;
    *nflag_dev = nullptr;
    // MFMA score = fp32 accumulation of exact products (bf16 x bf16 and e4m3 x e4m3 fit fp32): |error| <= (terms) u
    // sum |q_j x_j| <= d 2^-23 |q| |x| (u = 2^-23 allows truncating adders).  fp32-exact mode scans hi.qhi + hi.qlo +
    // lo.qhi of bf16 splits: the dropped lo.qlo term adds 2^-16 |q| |x|, and there are three times the terms.
    m.err_c = f32x ? (3.0 * (double)ix->d * 1.1920928955078125e-07 + 1.52587890625e-05) : (double)ix->d * 1.1920928955078125e-07;
    m.nq_dev = c.nq_dev;
    if (c.stage1) { // the scan's operands are bf16(q), bf16(x): norms within 2^-8 of |q|, |x|
        m.err_c *= 1.01;
        m.dres2 = ix->dres2_dev;
        m.qerr2 = (const double*)ix->qerr2.p;
    }
    if (c.margin != 0) {
        rc = ix->cur.mbnd.ensure((size_t)nq * sizeof(float));
        if (rc) return rc;
        rc = ix->cur.mflag.ensure((size_t)nq);
        if (rc) return rc;
        rc = ensure_xmax2(ix, st);
        if (rc) return rc;
        m.xmax2 = ix->xmax2_dev;
        m.bnd = (float*)ix->cur.mbnd.p;
        m.flag = (unsigned char*)ix->cur.mflag.p;
        m.nflag = (unsigned*)ix->cur.gthr.p + (size_t)pl.nq_pad * 8 + 1; // zeroed with the insert bounds by the query staging
        *nflag_dev = m.nflag;
        if (!c.rescan) { // what the exact resolution of flagged queries starts from (resolve_kernels.hpp)
            rc = ix->keyk.ensure((size_t)nq * sizeof(float));
            if (rc) return rc;
            rc = ix->qqv.ensure((size_t)nq * sizeof(double));
            if (rc) return rc;
            m.keyk = (float*)ix->keyk.p;
            m.qq_out = (double*)ix->qqv.p;
        }
    }
    // (1) K' best candidates per query by MFMA score, (2) lane-packed exact re-score + final order
    rc = ix->cur.cand.ensure((size_t)nq * KL * sizeof(int));
    if (rc) return rc;
    int* cand = (int*)ix->cur.cand.p;
    const hipStream_t scan_st = st;
    if (split) { // the tail goes to its own stream, behind the scan
        HIP_TRY(hipEventRecord(ix->scan_done, scan_st));
        HIP_TRY(hipStreamWaitEvent(tail_st, ix->scan_done, 0));
        st = tail_st;
    }
    mips::merge_select_kernel<KL><<<(int)nq, 64, 0, st>>>(m, cand);
    HIP_TRY(hipGetLastError());
    const bool l2 = c.metric == MIPS_METRIC_L2;
    const int rgrid = (int)((nq + (64 / KL) - 1) / (64 / KL));
    if (f32r && l2) mips::rescore_rank_kernel<KL, mips::ElemF32, true><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (f32r) mips::rescore_rank_kernel<KL, mips::ElemF32, false><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (ix->sq8) mips::rescore_rank_kernel<KL, mips::ElemU8, false, mips::ElemBF16><<<rgrid, 64, 0, st>>>(m, cand, nq); // (inner product only)
    else if (e8 && l2) mips::rescore_rank_kernel<KL, mips::ElemF8, true, mips::ElemBF16><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (e8) mips::rescore_rank_kernel<KL, mips::ElemF8, false, mips::ElemBF16><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (f8 && l2) mips::rescore_rank_kernel<KL, mips::ElemF8, true><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (f8) mips::rescore_rank_kernel<KL, mips::ElemF8, false><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else if (l2) mips::rescore_rank_kernel<KL, mips::ElemBF16, true><<<rgrid, 64, 0, st>>>(m, cand, nq);
    else mips::rescore_rank_kernel<KL, mips::ElemBF16, false><<<rgrid, 64, 0, st>>>(m, cand, nq);
    HIP_TRY(hipGetLastError());
    if (split) {
        HIP_TRY(hipEventRecord(ix->cur.tail_done, st));
        ix->cur.tail_pending = true;
    }
    return MIPS_OK;
}

// tail_st: stream of the select + exact re-score launches (nullptr or == st: the scan's own stream)
template <int KL>
int launch_search(mips_index* ix, const SearchCall& c, int64_t nq, int k, float* d_out_s, int64_t* d_out_i, int64_t* d_out_packed,
                  int64_t idx_offset, hipStream_t st, unsigned** nflag_dev, hipStream_t tail_st = nullptr, bool split = false) {
    ScanPlan pl;
    int rc = choose_scan<KL>(ix, c, nq, pl);
    if (rc) return rc;
    rc = ix->cur.part_s.ensure((size_t)pl.nq_pad * pl.ncand * sizeof(float));
    if (rc) return rc;
    rc = ix->cur.part_i.ensure((size_t)pl.nq_pad * pl.ncand * sizeof(int));
    if (rc) return rc;

    mips::ScanArgs a;
    a.docs = (const uint16_t*)c.rows;
    a.qbuf = (const uint16_t*)c.qbuf;
    a.ntotal = ix->ntotal;
    a.ld = c.ld;
    a.ksteps = pl.f32x ? 3 * c.plane / mips::BK : c.ld / mips::BK;
    a.plane = c.plane;
    a.ntiles = pl.ntiles;
    a.tiles_per_split = pl.tps;
    a.nsplit = pl.nsplit;
    a.nqt = pl.nqt;
    a.nq = (int)nq;
    a.nq_dev = c.nq_dev;
    a.qgroups = pl.qgroups;
    a.qt_per_group = pl.qt_per_group;
    a.splits_per_group = pl.nsplit / (8 / pl.qgroups);
    a.part_s = (float*)ix->cur.part_s.p;
    a.part_i = (int*)ix->cur.part_i.p;
    a.gthr = nullptr;
    a.err = nullptr;
    a.spin_limit = ix->opt_spin_limit != 0 ? ix->opt_spin_limit : (1 << 22);
    if (pl.stationary) {
        // shared insert bounds: 8 class words per query (2 lane-half words in the older layouts) + error word
        const size_t thr_words = (size_t)pl.nq_pad * 8;
        // (allocated and cleared by mips_search together with the query staging)
        a.gthr = (unsigned*)ix->cur.gthr.p;
        a.err = a.gthr + thr_words;
    }
    rc = launch_scan(ix, c, pl, a, KL, st);
    if (rc) return rc;
    return launch_tail<KL>(ix, c, pl, a, nq, k, d_out_s, d_out_i, d_out_packed, idx_offset, st, nflag_dev, tail_st, split);
}

#undef MIPS_TABLE_END
#undef MIPS_SQ8_ROW
#undef MIPS_SQ8_PITCH
#undef MIPS_SQ8_PITCH_1024
#undef MIPS_SQ8_POOL

} // namespace
