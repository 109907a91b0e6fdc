// Host side of libmips_hip.so, part 1 of 3 (included by mips_hip.hip, one translation unit): error reporting, device / stream
// helpers, the types that own a device resource, the index object (what PERSISTS between calls: storage in HBM, scratch, the
// caller's options, the report of the last search), the value that describes ONE call in progress (SearchCall: passed by
// reference, never stored on the index) and what keeps the index consistent (growth, rows_changed, phi, row norms, the bf16
// image of an fp32-exact index, stream ordering, the two scratch sets).
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? MIPS_E_NOMEM : MIPS_E_HIP, "%s failed: %s", \
                        #expr, hipGetErrorString(e_));                                         \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
constexpr int64_t kRowAlign = 256;   // index capacity granule: the largest document tile of any scan variant
constexpr int64_t kQueryAlign = 256; // query staging buffer granule: the largest power-of-two query tile of any scan variant

// ---- What owns a device resource of the index.  Each frees what it holds when it goes (errors of the frees are ignored),
// cannot be copied and can be moved, so std::swap exchanges two of them; `delete ix` is the whole of mips_index_destroy.
// A handle released by Free: the exact-size device arrays (sizes are the caller's: never through Buffer::ensure), the pinned host
// words and the events.  Converts to the handle it holds.
template <class H, auto Free>
struct Owned {
    H p = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
    Owned& operator=(Owned&& o) noexcept { // (what this held leaves with o)
        std::swap(p, o.p);
        return *this;
    }
    ~Owned() {
        if (p) (void)Free(p);
    }
    operator H() const { return p; }
};
template <class T>
using DeviceArray = Owned<T*, hipFree>;
using PinnedWords = Owned<unsigned*, hipHostFree>; // 64 bytes of pinned host memory
using Event = Owned<hipEvent_t, hipEventDestroy>;
inline hipError_t create_event(Event& e, bool timing) {
    return timing ? hipEventCreate(&e.p) : hipEventCreateWithFlags(&e.p, hipEventDisableTiming);
}

// Growable device scratch: grows by a quarter over what is asked for, never shrinks
struct Buffer {
    void* p = nullptr;
    size_t bytes = 0;
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    Buffer& operator=(Buffer&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~Buffer() {
        if (p) (void)hipFree(p);
    }
    int ensure(size_t need) {
        if (need <= bytes) return MIPS_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(MIPS_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        bytes = want;
        return MIPS_OK;
    }
};

// The scratch a search's scan and tail share.  Split-tail searches (mips_search_split) run the scan on one stream and select +
// exact re-score on another, so the NEXT search's scan can start behind this one's: two sets alternate, and each carries the
// event its tail records and whether a tail may still be reading it.
struct ScratchSet {
    Buffer qbuf, qf32, gthr, part_s, part_i, cand, mbnd, mflag;
    Buffer qbias; // SQ8 index: B_q of the staged queries, one double each (SearchCall::qbias)
    Event tail_done;
    bool tail_pending = false;
};

int grid_for(int64_t items, int block) {
    int64_t g = (items + block - 1) / block;
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, 256 * 16));
}

} // namespace

struct mips_index {
    int device = 0;
    int64_t d = 0;
    int ld = 0;    // row length in elements: d padded to a multiple of 64 (bf16) or 256 (fp8)
    int esize = 2; // bytes per stored element
    int qsize = 2; // bytes per STAGED query element: esize, except MIPS_DTYPE_FP8_E4M3_DOCS (e4m3 rows, bf16 queries: `mixed`)
    bool mixed = false;
    // 8-bit scalar-quantised storage (MIPS_DTYPE_SQ8; host_sq8.hpp).  `mixed` holds as well: one-byte rows, bf16 staged queries.
    // sq8_params = [vmin | vdiff | s | o], ld floats each (columns >= d zero): what encode, query staging and decode read
    bool sq8 = false;
    bool sq8_trained = false;
    DeviceArray<float> sq8_params;
    Buffer sq8_part; // training: the row parts' minima / maxima / flags, and the candidate parameters
    int doc_dtype = MIPS_DTYPE_BF16;
    int metric = MIPS_METRIC_IP;
    int64_t ntotal = 0;
    int64_t capacity = 0; // rows allocated, multiple of TM
    DeviceArray<uint8_t> rows; // [capacity][ld] elements of esize bytes
    // fp32-exact mode (doc_dtype F32): rows = bf16 planes [hi | lo] (ld = 2 * plane) for the scan,
    // rows_f32 = the fp32 originals [capacity][plane] for the exact re-score; qf32 = staged fp32 queries
    int plane = 0;
    DeviceArray<float> rows_f32;
    // two-stage search of the fp32-exact index ("f32_fast", d <= 1024): rows_hi = bf16(x) alone at a row pitch the
    // query-stationary kernels take ([capacity][hp]; converted lazily from rows_f32 up to hi_rows).  Stage 1 scans it
    // like a bf16 index and re-scores on the fp32 rows; the margin check, widened by the representation error
    // |x - bf16 x| |q| + |bf16 x| |q - bf16 q|, sends the queries it cannot certify to the three-segment scan.
    DeviceArray<uint8_t> rows_hi;
    int hp = 0;
    int64_t hi_rows = 0;
    DeviceArray<double> dres2_dev; // max_i |x_i - bf16 x_i|^2
    bool dres2_valid = false;
    int opt_f32_fast = 1;        // 0 off, 1 when the call may synchronise (host buffers / margin_check = 2), 2 always
    int fast_skip = 0;           // calls left to skip stage 1 for: set by a SYNCHRONISING call that flagged too many queries for the
                                 // optimistic scan to pay (its count is known when it returns; stream-ordered calls never set it,
                                 // so what a search does depends on the calls before it, not on when a device store lands)
    bool phi_valid = false;
    bool phi_override = false; // phi was set from outside (global maximum of a sharded index): adds do not reset it
    double phi = 0.0;
    ScratchSet cur, alt; // the scratch set in use and the other one (swap_scratch_sets)
    Buffer stage, out_s, out_i, scalar;
    // ring of HIP event pairs around the scan kernel (bench.py reads the average launch duration)
    static constexpr int kEvRing = 128;
    // tuning knobs (mips_index_set_param); 0 = automatic
    int opt_nsplit = 0;
    int opt_qgroups = 0;
    int opt_spin_limit = 0; // test-only: polls of the split barrier before a wave gives up (0 = 1 << 22, < 0 = flag forced)
    // sticky scan-error flag: one pinned, mapped host word.  The exact re-score sets it (system-scope store) when
    // the scan kernel of its call gave up on the split barrier; the host reads it without a device round trip.
    PinnedWords sticky_host;
    unsigned* sticky_dev = nullptr; // (the same words as the device sees them)
    char last_kernel[96] = ""; // instance mips_search dispatched last (mips_index_last_kernel)
    // margin check.  0 = off, 1 = flag and count on the device (never synchronises), 2 = certify:
    // synchronise, re-scan the flagged queries with the widest lists.  Host-output searches always certify (they
    // synchronise anyway) unless the check is off.  This is the caller's knob: a call acts on margin_mode() of it.
    int opt_margin = 1;
    Buffer qbuf2, qf32b, tmp_s, tmp_i, ids, qhi, qerr2, keyk, qqv, hit_d, hit_i, hit_n, qnorm;
    // wide top-k (mips_search_wide, host_wide.hpp): candidate segments (fixed budget), pools [queries][k'], segment counters,
    // per-query thresholds / seeds / flags
    Buffer w_seg, w_pool, w_cnt, w_misc;
    // range search (mips_range_search, host_range.hpp; it shares w_seg / w_cnt): staging of the members in O(cap), the
    // (offset, count) of every (query, chunk) block, per-query thresholds / totals / radii, and the CSR arrays of a host-output call
    Buffer r_stage, r_blk, r_misc, r_lims;
    // filtered searches (mips_search_wide_sel / mips_range_search_sel): the device copy of a host bitmap, and the staged selector
    // ([0] the number of selected rows, from byte 16 on four 32-bit words per 128-row tile; select_kernels.hpp)
    Buffer sel_raw, sel_words;
    // row removal (mips_index_remove, host_remove.hpp; it stages into sel_raw / sel_words): "remove_window_rows", rows a gather
    // launch compacts (a multiple of 128; 0 = automatic, host_remove.hpp)
    int64_t opt_remove_window = 0;
    // rows by id (include/mips_hip_rows.h, host_rows.hpp): the device copy of host ids, and the device result of a host-output call
    Buffer row_ids, row_out;
    // exact re-ranking (include/mips_hip_refine.h, host_refine.hpp): the candidates' scores, and host ids / host results on the device
    Buffer rr_scores, rr_ids, rr_out_s, rr_out_i;
    // rows overwritten by id (include/mips_hip_write.h, host_update.hpp; host ids stage into row_ids, host rows into stage): one
    // int32 per row of `capacity`, -1 between calls (the position that writes the row while a call runs), and the call's count
    DeviceArray<int> upd_owner;
    int64_t upd_owner_cap = 0;
    Buffer upd_count;
    // grouped searches (mips_search_wide_grp / mips_range_search_grp): one int32 label per row in storage of its own, allocated in
    // whole 128-row tiles for at least `capacity` rows (mips_index_set_labels grows it and keeps what it held, so it survives the
    // growth of the rows); rows [0, nlabelled) carry a label.  grp_q: the staged per-query labels of the call in flight.
    DeviceArray<int> labels;
    int64_t labels_cap = 0, nlabelled = 0;
    Buffer grp_q;
    int opt_resolve = 1; // flagged queries: 1 = exact brute-force resolution (resolve_kernels.hpp; 2 = its plain form, no MFMA pre-filter), 0 = re-scan with the widest lists
    int resolve_budget = 0; // "resolve_budget" > 0: flagged queries a search resolves at most (0 = RESOLVE_MAX); a search that flags
                            // more keeps its first results (counted unresolved) -- or, if its first scan was an optimistic one,
                            // goes through the stream-ordered re-scan with true K' = 32 lists
    DeviceArray<double> xmax2_dev; // max_i |x_i|^2 of the LOCAL rows, on the device (no host copy: never synchronises)
    bool xmax2_valid = false;
    PinnedWords nflag_host; // flagged-query counts a certifying search reads back (allocated on first use: ensure_nflag_host)
    SearchReport report;    // what the last search call flagged and settled (search_report.hpp; mips_index_margin_stats)
    Event scan_done;        // split-tail searches: the tail stream waits for the scan (ScratchSet)
    int opt_tiny = 1;              // 1 = searches of <= 16 queries over a small bf16 index take the one-launch kernel
    DeviceArray<unsigned> tiny_words; // [0] ticket (reset by the kernel's last workgroup), [1] flag counter
    int opt_variant = 0; // 0 = automatic, 1 = scan_kernel (128x128 tiles), 3 = scan_kernel_v3 (32x32x16), 4 = scan_kernel_v4 (16x16x32)
    Event ev0[kEvRing], ev1[kEvRing];
    int ev_count = 0; // pairs recorded since the last reset (saturates at kEvRing)
    bool timing_armed = false; // event pairs are recorded only inside a measurement window (mips_scan_timing reset):
                               // an event record costs ~5.7 us of stream time on this part, 11 us per search
    int ev_next = 0;
    // The scratch buffers are shared by every call on this index.  Calls on ONE stream are ordered by the
    // stream; a call arriving on another stream first waits for `busy`, recorded at the end of the last call.
    Event busy;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
};

// What ONE launch of a search sees beyond the index: the view of the rows it scans, its staged queries and the switches of the
// call in progress.  A plain value, built by the entry point (begin_call), passed by reference down to the kernel launch and
// never stored on the index; a nested launch (stage 1 of the two-stage fp32 search, a re-scan) gets a modified COPY.
struct SearchCall {
    const uint8_t* rows = nullptr; // the scanned rows, [capacity][ld]
    int ld = 0, plane = 0;         // their pitch; plane > 0: the [hi | lo] planes of the fp32-exact index
    // stage 1 of the two-stage fp32 search: rows = the bf16 rows_hi at pitch hp, scanned like a bf16 index (plane = 0); the
    // exact re-score and the margin check still run on rows_f32, rescore_ld columns wide
    bool stage1 = false;
    int rescore_ld = 0;
    const void* qbuf = nullptr;    // staged queries: the scan's operand ...
    const void* qf32 = nullptr;    // ... and the fp32 originals of an fp32-exact index
    // "Optimistic" scan (calls that certify, i.e. may synchronise): pools of 16 / 32 candidates selected from the sub-lists of
    // scan_kernel_v4 / k3 instead of from true K'-entry lists.  What the pool may have excluded is bounded all the same
    // (merge_select: sub-lists' last entries), so the margin check decides per query; flagged queries are re-scanned with true
    // K' = 32 lists.  Decided by pool_policy, read by choose_scan.
    bool optimistic = false;
    bool rescan = false;           // the second scan of flagged queries (widest lists): nothing is prepared for a third
    // stream-ordered re-scan: the query count lives on the device -- the launches are sized for all queries and the workgroups
    // past the count leave
    const int* nq_dev = nullptr;
    int nsplit = 0;                // index splits asked for (0 = automatic): "nsplit", or a re-scan's own choice
    bool timed = true;             // the scan may record its event pair and names itself in last_kernel (a nested launch: no)
    int metric = MIPS_METRIC_IP;   // index metric unless MIPS_FORCE_IP
    int margin = 0;                // margin_mode() of this call
    const double* qbias = nullptr; // SQ8 index: B_q per staged query, added where the call's final scores stand (sq8_finish)
};

namespace {

// "margin_check" as the caller set it -> the mode one call acts on:
//   1 (default, "auto")  device outputs: 3 = certify on the stream; host buffers: they synchronise anyway and certify
//   4 ("count only")     1: device outputs count flagged queries, nothing more
// 0 / 2 / 3 as they are.
inline int margin_mode(const mips_index* ix, bool out_dev) {
    if (ix->opt_margin == 1 && out_dev) return 3;
    return ix->opt_margin == 4 ? 1 : ix->opt_margin;
}
// The call settles the queries it flags: host buffers (they synchronise anyway), "margin_check" = 2, or on the stream (3)
inline bool call_certifies(int margin, bool out_dev) { return margin != 0 && (!out_dev || margin >= 2); }

// Rows the per-query buffers (staged queries, insert bounds, partial lists) are padded to: whole query tiles of every kernel that
// may take the search -- 256 (128 / 256-query tiles), and at bf16 row pitch 1024 also scan_kernel_k3's 192-query tiles
inline int64_t query_pad(const mips_index* ix, int64_t n) {
    const bool pitch_1024 = ix->esize == 2 && (ix->ld == 1024 || ix->hp == 1024);
    return round_up(n, pitch_1024 ? 768 : kQueryAlign);
}

// Orders the calls on one index across streams (see mips_index::busy).  Nothing is recorded per call (an event
// record costs ~5.7 us of stream time here): when a call arrives on ANOTHER stream than the previous one, the
// event is recorded on the previous stream at that moment and the new stream waits for it.  A stream handed to
// the library must therefore stay valid until the next call on the index (torch's pooled streams do).
struct StreamOrder {
    mips_index* ix;
    hipStream_t st;
    bool ok = true;
    StreamOrder(mips_index* ix_, hipStream_t st_) : ix(ix_), st(st_) {
        if (ix->has_last && ix->last_stream != st)
            ok = hipEventRecord(ix->busy, ix->last_stream) == hipSuccess && hipStreamWaitEvent(st, ix->busy, 0) == hipSuccess;
    }
    ~StreamOrder() {
        ix->last_stream = st;
        ix->has_last = true;
    }
};
#define ORDER_ON(ix, st)             \
    StreamOrder order_guard(ix, st); \
    if (!order_guard.ok) return fail(MIPS_E_HIP, "hipStreamWaitEvent failed")

// A scan kernel whose split barrier timed out poisons its call's output and raises the sticky flag; whoever looks
// first (the next call on the index, mips_index_check_error, a host-output search) reports and clears it.
int take_scan_error(mips_index* ix, const char* who) {
    if (ix->sticky_host == nullptr) return MIPS_OK;
    if (__atomic_load_n(ix->sticky_host.p, __ATOMIC_ACQUIRE) == 0u) return MIPS_OK;
    __atomic_store_n(ix->sticky_host.p, 0u, __ATOMIC_RELEASE);
    return fail(MIPS_E_SCAN_TIMEOUT,
                "%s: a scan kernel on this index gave up on its block barrier (spin bound reached); the results of "
                "that search were poisoned (idx %d, NaN scores) and must be discarded", who, MIPS_IDX_POISON);
}

void set_kernel_name(mips_index* ix, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ix->last_kernel, sizeof ix->last_kernel, fmt, ap);
    va_end(ap);
}

// exact = false: geometric growth for repeated adds; true: mips_index_reserve's exact reservation
int grow(mips_index* ix, int64_t need_rows, hipStream_t st, bool exact = false) {
    if (need_rows <= ix->capacity) return MIPS_OK;
    int64_t cap = exact ? need_rows : std::max<int64_t>(need_rows, ix->capacity + ix->capacity / 2);
    cap = round_up(cap, kRowAlign);
    DeviceArray<uint8_t> fresh, fresh_hi; // (swapped into the index at the end: the old storage goes with them, behind the
    DeviceArray<float> fresh32;           // synchronisation below; on an error return what was allocated goes)
    const size_t row_bytes = (size_t)ix->ld * ix->esize;
    const size_t bytes = (size_t)cap * row_bytes;
    const size_t b32 = (size_t)cap * ix->plane * sizeof(float);
    hipError_t e = hipMalloc((void**)&fresh.p, bytes);
    if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the index failed: %s", bytes, hipGetErrorString(e));
    if (ix->plane > 0) {
        e = hipMalloc((void**)&fresh32.p, b32);
        if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the fp32 rows failed: %s", b32, hipGetErrorString(e));
    }
    const size_t bhi = (size_t)cap * ix->hp * 2;
    if (ix->plane > 0 && ix->hp > 0) {
        e = hipMalloc((void**)&fresh_hi.p, bhi);
        if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the bf16 rows of the fp32 index failed: %s", bhi, hipGetErrorString(e));
    }
    // copy the rows in use; rows past ntotal are read by the last (ragged) tile: keep them defined
    const size_t used = (size_t)ix->ntotal * row_bytes;
    const size_t u32 = (size_t)ix->ntotal * ix->plane * sizeof(float);
    if (used) e = hipMemcpyAsync(fresh, ix->rows, used, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(fresh + used, 0, bytes - used, st);
    if (e == hipSuccess && fresh32 && u32) e = hipMemcpyAsync(fresh32, ix->rows_f32, u32, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && fresh32) e = hipMemsetAsync((char*)fresh32.p + u32, 0, b32 - u32, st);
    const size_t uhi = (size_t)ix->hi_rows * ix->hp * 2;
    if (e == hipSuccess && fresh_hi && uhi) e = hipMemcpyAsync(fresh_hi, ix->rows_hi, uhi, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && fresh_hi) e = hipMemsetAsync(fresh_hi + uhi, 0, bhi - uhi, st);
    if (e == hipSuccess && ix->rows) e = hipStreamSynchronize(st); // the old storage is freed when this returns
    if (e != hipSuccess) return fail(MIPS_E_HIP, "growing the index to %lld rows failed: %s", (long long)cap, hipGetErrorString(e));
    std::swap(ix->rows, fresh);
    std::swap(ix->rows_f32, fresh32);
    std::swap(ix->rows_hi, fresh_hi);
    ix->capacity = cap;
    return MIPS_OK;
}

// convert [n][d] of src_dtype (host or device) into dst [n][ld] of the index element type on the device
// pad_rows / zero / zero_words: query staging only -- that many zero rows behind the last converted one and a
// word range to clear, both done by the launch that converts the last chunk (bf16 and fp8 storage)
// out_esize: bytes per OUTPUT element (0 = the index storage's; query staging passes ix->qsize)
int convert_into(mips_index* ix, const void* src, int64_t n, int src_dtype, int src_is_device, uint8_t* dst,
                 hipStream_t st, float* keep_f32 = nullptr, int64_t pad_rows = 0, uint32_t* zero = nullptr,
                 int64_t zero_words = 0, int out_esize = 0, double* sq8_bias = nullptr) {
    const int d = (int)ix->d, ld = ix->ld;
    if (out_esize == 0) out_esize = ix->esize;
    const size_t esz = src_dtype == MIPS_DTYPE_F32 ? 4 : src_dtype == MIPS_DTYPE_BF16 ? 2 : 1;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)(d * esz));
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t nr = std::min(chunk_rows, n - r0);
        const void* s = (const char*)src + (size_t)r0 * d * esz;
        if (!src_is_device) {
            int rc = ix->stage.ensure((size_t)nr * d * esz);
            if (rc) return rc;
            // the staging buffer is reused by the next chunk: this copy is synchronous for pageable memory
            HIP_TRY(hipMemcpyAsync(ix->stage.p, s, (size_t)nr * d * esz, hipMemcpyHostToDevice, st));
            s = ix->stage.p;
        }
        uint8_t* out = dst + (size_t)r0 * ld * out_esize;
        if (ix->plane > 0) { // fp32-exact mode: bf16 planes [hi | lo] + the fp32 originals
            const int64_t items = nr * (ix->plane / 8);
            float* keep = keep_f32 ? keep_f32 + (size_t)r0 * ix->plane : nullptr;
            if (src_dtype == MIPS_DTYPE_F32)
                mips::split_rows_kernel<float><<<grid_for(items, 256), 256, 0, st>>>((const float*)s, nr, d, d, (uint16_t*)out, ix->plane, keep);
            else
                mips::split_rows_kernel<uint16_t><<<grid_for(items, 256), 256, 0, st>>>((const uint16_t*)s, nr, d, d, (uint16_t*)out, ix->plane, keep);
        } else {
            // (both SQ8 branches below read the trained parameters on the device: no launch without them, whoever calls)
            if (ix->sq8 && !ix->sq8_trained) return fail(MIPS_E_INVALID, "the SQ8 index is not trained (mips_index_sq8_train)");
            const bool last = r0 + nr == n;
            const int64_t n_out = nr + (last ? pad_rows : 0);
            uint32_t* z = last ? zero : nullptr;
            const int64_t zw = last ? zero_words : 0;
            if (ix->sq8 && out_esize == 2) { // query staging of an SQ8 index: q' = bf16(q s), B_q (chunks: the launch of the last
                const int64_t items = n_out * (ld / 8); // one pads and clears; every launch writes its own queries' B_q)
                if (src_dtype != MIPS_DTYPE_F32 && src_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "SQ8 index: queries are float32 or bf16");
                uint16_t* qo = (uint16_t*)out;
                if (src_dtype == MIPS_DTYPE_F32)
                    mips::sq8_stage_queries_kernel<float><<<grid_for(items, 256), 256, 0, st>>>((const float*)s, nr, d, ix->sq8_params, qo, ld, n_out, z, zw, sq8_bias + r0);
                else
                    mips::sq8_stage_queries_kernel<uint16_t><<<grid_for(items, 256), 256, 0, st>>>((const uint16_t*)s, nr, d, ix->sq8_params, qo, ld, n_out, z, zw, sq8_bias + r0);
            } else if (ix->sq8) { // rows of an SQ8 index: encode (or copy raw codes)
                const int64_t items = nr * (ld / 16);
                if (src_dtype == MIPS_DTYPE_F32)
                    mips::sq8_encode_rows_kernel<float><<<grid_for(items, 256), 256, 0, st>>>((const float*)s, nr, d, ix->sq8_params, out, ld);
                else if (src_dtype == MIPS_DTYPE_BF16)
                    mips::sq8_encode_rows_kernel<uint16_t><<<grid_for(items, 256), 256, 0, st>>>((const uint16_t*)s, nr, d, ix->sq8_params, out, ld);
                else
                    mips::sq8_encode_rows_kernel<uint8_t><<<grid_for(items, 256), 256, 0, st>>>((const uint8_t*)s, nr, d, ix->sq8_params, out, ld);
            } else if (out_esize == 2) {
                const int64_t items = n_out * (ld / 8);
                if (src_dtype == MIPS_DTYPE_FP8_E4M3) return fail(MIPS_E_INVALID, "e4m3 bytes cannot be staged as bf16 rows");
                if (src_dtype == MIPS_DTYPE_F32)
                    mips::convert_rows_kernel<float><<<grid_for(items, 256), 256, 0, st>>>((const float*)s, nr, d, (uint16_t*)out, ld, n_out, z, zw);
                else
                    mips::convert_rows_kernel<uint16_t><<<grid_for(items, 256), 256, 0, st>>>((const uint16_t*)s, nr, d, (uint16_t*)out, ld, n_out, z, zw);
            } else {
                const int64_t items = n_out * (ld / 16);
                if (src_dtype == MIPS_DTYPE_F32)
                    mips::convert_rows_f8_kernel<float><<<grid_for(items, 256), 256, 0, st>>>((const float*)s, nr, d, out, ld, n_out, z, zw);
                else if (src_dtype == MIPS_DTYPE_BF16)
                    mips::convert_rows_f8_kernel<uint16_t><<<grid_for(items, 256), 256, 0, st>>>((const uint16_t*)s, nr, d, out, ld, n_out, z, zw);
                else
                    mips::convert_rows_f8_kernel<uint8_t><<<grid_for(items, 256), 256, 0, st>>>((const uint8_t*)s, nr, d, out, ld, n_out, z, zw);
            }
        }
        HIP_TRY(hipGetLastError());
        if (!src_is_device) HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

// for_query: queries of an e4m3-documents / bf16-queries index are float32 or bf16 (raw e4m3 bytes are rows only)
bool src_dtype_ok(const mips_index* ix, int t, bool for_query = false) {
    return t == MIPS_DTYPE_F32 || t == MIPS_DTYPE_BF16 || (t == MIPS_DTYPE_SQ8 && ix->sq8 && !for_query) || // (raw codes: rows only)
           (t == MIPS_DTYPE_FP8_E4M3 && ix->esize == 1 && ix->plane == 0 && !ix->sq8 && !(for_query && ix->mixed));
}

int compute_phi(mips_index* ix, hipStream_t st) {
    if (ix->phi_valid) return MIPS_OK;
    int rc = ix->scalar.ensure(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix->scalar.p, 0, 8, st));
    if (ix->ntotal > 0) {
        const int grid = (int)((ix->ntotal + 255) / 256);
        if (ix->plane > 0)
            mips::row_sumsq_max_kernel<mips::ElemF32><<<grid, 256, 0, st>>>(ix->rows_f32, ix->ntotal, ix->plane,
                                                                             (unsigned long long*)ix->scalar.p);
        else if (ix->esize == 2)
            mips::row_sumsq_max_kernel<mips::ElemBF16><<<grid, 256, 0, st>>>((const uint16_t*)ix->rows.p, ix->ntotal, ix->ld,
                                                                              (unsigned long long*)ix->scalar.p);
        else if (ix->sq8)
            mips::row_sumsq_max_kernel<mips::ElemU8><<<grid, 256, 0, st>>>(ix->rows, ix->ntotal, ix->ld,
                                                                            (unsigned long long*)ix->scalar.p);
        else
            mips::row_sumsq_max_kernel<mips::ElemF8><<<grid, 256, 0, st>>>(ix->rows, ix->ntotal, ix->ld,
                                                                            (unsigned long long*)ix->scalar.p);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, ix->scalar.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(&ix->phi, &bits, 8);
    ix->phi_valid = true;
    return MIPS_OK;
}

// max_i |x_i|^2 of the local rows into a device scalar, stream-ordered, no host copy (the margin check's error bound)
int ensure_xmax2(mips_index* ix, hipStream_t st) {
    if (ix->xmax2_valid) return MIPS_OK;
    if (!ix->xmax2_dev) HIP_TRY(hipMalloc((void**)&ix->xmax2_dev.p, 8));
    HIP_TRY(hipMemsetAsync(ix->xmax2_dev, 0, 8, st));
    if (ix->ntotal > 0) {
        const int grid = (int)((ix->ntotal + 255) / 256);
        unsigned long long* out = (unsigned long long*)ix->xmax2_dev.p;
        if (ix->plane > 0) mips::row_sumsq_max_kernel<mips::ElemF32><<<grid, 256, 0, st>>>(ix->rows_f32, ix->ntotal, ix->plane, out);
        else if (ix->esize == 2) mips::row_sumsq_max_kernel<mips::ElemBF16><<<grid, 256, 0, st>>>((const uint16_t*)ix->rows.p, ix->ntotal, ix->ld, out);
        else if (ix->sq8) mips::row_sumsq_max_kernel<mips::ElemU8><<<grid, 256, 0, st>>>(ix->rows, ix->ntotal, ix->ld, out); // (the norm of the codes)
        else mips::row_sumsq_max_kernel<mips::ElemF8><<<grid, 256, 0, st>>>(ix->rows, ix->ntotal, ix->ld, out);
        HIP_TRY(hipGetLastError());
    }
    ix->xmax2_valid = true;
    return MIPS_OK;
}

// two-stage fp32-exact search: bf16 rows of the rows added since the last call, and the residual bound
int ensure_hi(mips_index* ix, hipStream_t st) {
    if (ix->hi_rows < ix->ntotal) {
        const int64_t nr = ix->ntotal - ix->hi_rows;
        const int64_t items = nr * (ix->hp / 8);
        mips::convert_rows_kernel<float><<<grid_for(items, 256), 256, 0, st>>>(ix->rows_f32 + (size_t)ix->hi_rows * ix->plane, nr, ix->plane,
                                                                               (uint16_t*)ix->rows_hi.p + (size_t)ix->hi_rows * ix->hp, ix->hp);
        HIP_TRY(hipGetLastError());
        ix->hi_rows = ix->ntotal;
    }
    if (!ix->dres2_valid) {
        if (!ix->dres2_dev) HIP_TRY(hipMalloc((void**)&ix->dres2_dev.p, 8));
        HIP_TRY(hipMemsetAsync(ix->dres2_dev, 0, 8, st));
        if (ix->ntotal > 0) {
            mips::row_resid_sumsq_max_kernel<<<(int)((ix->ntotal + 255) / 256), 256, 0, st>>>(ix->rows_f32, ix->ntotal, ix->plane,
                                                                                             (unsigned long long*)ix->dres2_dev.p);
            HIP_TRY(hipGetLastError());
        }
        ix->dres2_valid = true;
    }
    return MIPS_OK;
}

void swap_scratch_sets(mips_index* ix) { std::swap(ix->cur, ix->alt); }

// A tail of a split-tail search may still be reading its scratch set (staged queries, lists) and the stored rows from its tail
// stream: what is enqueued on st from here on comes behind it.  both_sets: the other set's tail as well (calls that move rows)
int wait_for_tail(mips_index* ix, hipStream_t st, bool both_sets) {
    for (ScratchSet* s : {&ix->cur, &ix->alt}) {
        if (s == &ix->alt && !both_sets) break;
        if (s->tail_pending) {
            HIP_TRY(hipStreamWaitEvent(st, s->tail_done, 0));
            s->tail_pending = false;
        }
    }
    return MIPS_OK;
}

// The pinned words a certifying search reads its counts back into
int ensure_nflag_host(mips_index* ix) {
    if (!ix->nflag_host) HIP_TRY(hipHostMalloc((void**)&ix->nflag_host.p, 64, hipHostMallocDefault));
    return MIPS_OK;
}

// The stored rows from first_changed_row on changed (added, moved, gone): what is derived from them is computed again when next
// needed -- the bf16 image of an fp32-exact index from that row on, phi unless it was set from outside, the row-norm bounds
void rows_changed(mips_index* ix, int64_t first_changed_row) {
    ix->hi_rows = std::min(ix->hi_rows, first_changed_row);
    if (!ix->phi_override) ix->phi_valid = false;
    ix->xmax2_valid = false;
    ix->dres2_valid = false;
}

} // namespace
