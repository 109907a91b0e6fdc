// Host side of mips_search_wide (included by mips_hip.hip behind host_search.hpp): query slices, chunk geometry, launches and
// the scratch of the wide top-k path (scan_kernel_wide.hpp).  Everything is enqueued on the caller's stream; the only
// synchronisation is the one a host-output call ends with.
#pragma once

namespace {

constexpr int64_t kWideBudget = 1ll << 25;   // segment entries (8 bytes each): the scratch that does NOT grow with ntotal
constexpr int64_t kWideSlice = 4096;         // queries per slice
constexpr int64_t kWideMaxChunkRows = 1 << 17;
constexpr int kWideExactSlots = 256;         // flagged queries one settlement round takes
static_assert(kWideSlice % mips::TN == 0, "a slice reads the staged query labels at its offset: whole query tiles");

// k' - k.  The pool must reach past the k-th result by the error of the scores that selected it: d 2^-23 |q| max|x| on a bf16
// index (a few ranks on Gaussian data), the representation error of bf16(x) . bf16(q) on the fp32-exact index (~0.1 sigma:
// hundreds of ranks at k = 1000 over 2^20 rows).  Queries it does not reach are settled exactly, so this is speed only.
inline int wide_slack(const mips_index* ix, int k) { return ix->plane > 0 ? 256 + k / 4 : 64; }

struct WideScratch {
    int* cnt;
    int* pool_n;
    mips::wkey_t* tau_c;
    float* tau_f;
    mips::wkey_t* seed;
    double* qq;
    int* ids;        // [slice + 4]: flagged list, then its count
    unsigned char* flag;
    unsigned* words; // [0] flagged queries of the call, [1] always 0 (unresolved)
};

// A caller's row selector (bits == nullptr: none) and, once staged, what the kernels read.
struct Selector {
    const uint8_t* bits = nullptr;
    int64_t nbits = 0, bit0 = 0;
    bool dev = false;                          // bits is device memory (MIPS_SEL_DEVICE)
    const unsigned* words = nullptr;           // staged: four words per 128-row tile
    const unsigned long long* nsel = nullptr;  // staged: number of selected rows
    // a grouped call (qlab != nullptr): one label per query, tested against the index's row labels
    const int32_t* qlab = nullptr;
    bool qlab_dev = false;                     // qlab is device memory (MIPS_GRP_DEVICE)
    int grp_only = 0;                          // MIPS_GRP_ONLY
    const int* qlab_staged = nullptr;          // staged: [round_up(nq, TN)], MIPS_LABEL_NONE behind the caller's nq
};

// Runs once per call, before the first slice: the bitmap (a host one is copied with the stream's async copy) becomes the
// shifted, cleared and padded words of select_kernels.hpp, and their popcount.  Nothing is read back.
// A grouped call without a bitmap stages all ones over [0, ntotal), and every grouped call stages its query labels: a slice reads
// them at its offset (a multiple of the query tile), the last one up to the pad.
// The caller's bitmap as the staging kernels take it (device bytes, their number, the bit of local row 0): a host bitmap is
// copied with the stream's async copy (the removal's staging, host_remove.hpp, starts the same way)
int bitmap_on_device(mips_index* ix, const uint8_t* bits, int64_t nbits, int64_t sel_bit0, bool dev, hipStream_t st, const uint8_t*& src,
                     int64_t& bit0, int64_t& nbytes) {
    src = bits;
    bit0 = sel_bit0;
    nbytes = (nbits + 7) >> 3;
    if (bits == nullptr) {
        bit0 = 0;
        nbytes = 0;
    } else if (!dev) { // only the bytes that hold bits bit0 .. bit0 + ntotal - 1 travel
        const int64_t b0 = sel_bit0 >> 3, b1 = (sel_bit0 + ix->ntotal + 7) >> 3;
        int rc = ix->sel_raw.ensure((size_t)(b1 - b0));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(ix->sel_raw.p, bits + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, st));
        src = (const uint8_t*)ix->sel_raw.p;
        bit0 = sel_bit0 & 7;
        nbytes = b1 - b0;
    }
    return MIPS_OK;
}

int stage_selector(mips_index* ix, Selector& sel, int64_t nq, hipStream_t st) {
    const int64_t ntiles = (ix->ntotal + mips::TM - 1) / mips::TM;
    const int64_t nwords = ntiles * (mips::TM / 32);
    int rc = ix->sel_words.ensure(16 + (size_t)nwords * sizeof(unsigned));
    if (rc) return rc;
    const uint8_t* src;
    int64_t bit0, nbytes;
    rc = bitmap_on_device(ix, sel.bits, sel.nbits, sel.bit0, sel.dev, st, src, bit0, nbytes);
    if (rc) return rc;
    unsigned long long* nsel = (unsigned long long*)ix->sel_words.p;
    unsigned* words = (unsigned*)((unsigned char*)ix->sel_words.p + 16);
    HIP_TRY(hipMemsetAsync(nsel, 0, 16, st));
    mips::selector_stage_kernel<<<grid_for(nwords, mips::SEL_THREADS), mips::SEL_THREADS, 0, st>>>(src, nbytes, bit0, ix->ntotal, words, nwords, nsel);
    HIP_TRY(hipGetLastError());
    sel.words = words;
    sel.nsel = nsel;
    if (sel.qlab != nullptr) {
        const int64_t nq_pad = round_up(nq, mips::TN);
        rc = ix->grp_q.ensure((size_t)nq_pad * sizeof(int));
        if (rc) return rc;
        int* ql = (int*)ix->grp_q.p;
        HIP_TRY(hipMemcpyAsync(ql, sel.qlab, (size_t)nq * sizeof(int), sel.qlab_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (nq_pad > nq) mips::label_pad_kernel<<<(int)((nq_pad - nq + 127) / 128), 128, 0, st>>>(ql, nq, nq_pad);
        HIP_TRY(hipGetLastError());
        sel.qlab_staged = ql;
    }
    return MIPS_OK;
}

// packed: d_i is the MIPS_OUT_PACKED payload [nq][k][2] and d_s is not written (it may be NULL)
// sel.bits != nullptr: a filtered search (masked scan, certificate on the selected count, masked settlement)
// sel.qlab != nullptr: a grouped search (grouped scan, certificate without a count, settlement that tests the labels)
int wide_search(mips_index* ix, SearchReport& rep, const void* q, int q_dtype, int64_t nq, int k, float* d_s, int64_t* d_i, bool packed, int64_t idx_offset, bool q_dev,
                Selector sel, int metric, hipStream_t st) {
    const bool grouped = sel.qlab != nullptr;
    const bool masked = sel.bits != nullptr && !grouped;
    const bool f32x = ix->plane > 0;
    const bool l2 = metric == MIPS_METRIC_L2;
    const int sld = f32x ? ix->hp : ix->ld;    // row pitch of the scanned bf16 rows
    const int cld = f32x ? ix->plane : ix->ld; // row pitch of the canonical rows and queries
    const int kp = std::min<int>(mips::WIDE_POOL, k + wide_slack(ix, k));
    int rc;
    if (l2) {
        rc = compute_phi(ix, st);
        if (rc) return rc;
    }
    rc = ensure_xmax2(ix, st);
    if (rc) return rc;
    if (f32x) {
        rc = ensure_hi(ix, st);
        if (rc) return rc;
    }

    // ---- geometry, fixed for the call (slices only differ in their query count)
    const int64_t slice = std::min<int64_t>(nq, kWideSlice);
    const int64_t slice_pad = round_up(slice, mips::TN);
    const int nqt_max = (int)(slice_pad / mips::TN);
    const int64_t ntiles = (ix->ntotal + mips::TM - 1) / mips::TM;
    int nsplit = (int)round_up((512 + nqt_max - 1) / nqt_max, 8);
    nsplit = std::min(nsplit, mips::WIDE_MAX_SEG / 2);
    nsplit = (int)std::min<int64_t>(nsplit, round_up(ntiles, 8));
    const int64_t max_rows = std::max<int64_t>(mips::TM, std::min<int64_t>(kWideMaxChunkRows, kWideBudget / slice_pad));
    const int tps_max = (int)std::max<int64_t>(1, std::min<int64_t>(max_rows / mips::TM / nsplit, (ntiles + nsplit - 1) / nsplit));
    const int segcap = tps_max * (mips::TM / 2);
    const int nseg = 2 * nsplit;
    // settlement: kWideExactSlots flagged queries per round, one segment each
    const int xslots = (int)std::min<int64_t>(slice, kWideExactSlots);
    const int64_t xrows = std::max<int64_t>(512, std::min<int64_t>(round_up(ix->ntotal, 512), kWideBudget / xslots));

    const size_t seg_entries = std::max<size_t>((size_t)slice_pad * nseg * segcap, (size_t)xslots * xrows);
    rc = ix->w_seg.ensure(seg_entries * sizeof(mips::wkey_t));
    if (rc) return rc;
    rc = ix->w_pool.ensure((size_t)slice_pad * kp * sizeof(mips::wkey_t));
    if (rc) return rc;
    rc = ix->w_cnt.ensure((size_t)slice_pad * nseg * sizeof(int));
    if (rc) return rc;
    const size_t P = (size_t)slice_pad;
    rc = ix->w_misc.ensure(P * (8 + 8 + 8 + 4 + 4 + 4 + 1) + 256);
    if (rc) return rc;
    WideScratch w;
    {
        unsigned char* b = (unsigned char*)ix->w_misc.p;
        w.tau_c = (mips::wkey_t*)b;
        b += P * 8;
        w.seed = (mips::wkey_t*)b;
        b += P * 8;
        w.qq = (double*)b;
        b += P * 8;
        w.tau_f = (float*)b;
        b += P * 4;
        w.pool_n = (int*)b;
        b += P * 4;
        w.ids = (int*)b;
        b += P * 4;
        w.words = (unsigned*)b; // (ids spill-over: count at ids[slice] lives in its own words below)
        b += 64;
        w.flag = b;
    }
    w.cnt = (int*)ix->w_cnt.p;
    int* const nflag_slice = (int*)(w.words + 4); // flagged count of the slice in flight
    HIP_TRY(hipMemsetAsync(w.words, 0, 64, st));

    const size_t qesz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    const double err_c = (double)ix->d * 1.1920928955078125e-07 * (f32x ? 1.01 : 1.0);
    const int scan_lds = mips::SCAN_LDS_BYTES;
    if (grouped || masked) {
        const void* scan = grouped ? (const void*)mips::grouped_scan_kernel : (const void*)mips::masked_scan_kernel;
        HIP_TRY(hipFuncSetAttribute(scan, hipFuncAttributeMaxDynamicSharedMemorySize, scan_lds));
        rc = stage_selector(ix, sel, nq, st);
        if (rc) return rc;
    } else {
        HIP_TRY(hipFuncSetAttribute((const void*)mips::wide_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, scan_lds));
    }

    for (int64_t s0 = 0; s0 < nq; s0 += slice) {
        const int64_t ns = std::min(slice, nq - s0);
        const int64_t ns_pad = round_up(ns, mips::TN);
        const int nqt = (int)(ns_pad / mips::TN);
        const void* qs = (const char*)q + (size_t)s0 * ix->d * qesz;
        const int* qlab_s = grouped ? sel.qlab_staged + s0 : nullptr; // (s0 is a multiple of the query tile)
        float* out_s = packed ? nullptr : d_s + (size_t)s0 * k;
        int64_t* out_i = packed ? nullptr : d_i + (size_t)s0 * k;
        int64_t* out_packed = packed ? d_i + (size_t)s0 * k * 2 : nullptr;

        // ---- stage the slice's queries: canonical form (bf16 rows / fp32 rows) and, fp32-exact index, bf16(q) for the scan
        const int64_t nq_padq = query_pad(ix, ns);
        const size_t row_bytes = (size_t)ix->ld * ix->qsize;
        rc = ix->cur.qbuf.ensure((size_t)nq_padq * row_bytes);
        if (rc) return rc;
        if (f32x) {
            rc = ix->cur.qf32.ensure((size_t)nq_padq * ix->plane * sizeof(float));
            if (rc) return rc;
            rc = convert_into(ix, qs, ns, q_dtype, q_dev ? 1 : 0, (uint8_t*)ix->cur.qbuf.p, st, (float*)ix->cur.qf32.p);
            if (rc) return rc;
            rc = ix->qhi.ensure((size_t)nq_padq * ix->hp * 2);
            if (rc) return rc;
            rc = ix->qerr2.ensure((size_t)ns * sizeof(double));
            if (rc) return rc;
            mips::convert_rows_kernel<float><<<grid_for(nq_padq * (int64_t)(ix->hp / 8), 256), 256, 0, st>>>((const float*)ix->cur.qf32.p, ns, ix->plane,
                                                                                                           (uint16_t*)ix->qhi.p, ix->hp, nq_padq);
            mips::query_resid_kernel<<<(int)((ns + 3) / 4), 256, 0, st>>>((const float*)ix->cur.qf32.p, ns, ix->plane, (double*)ix->qerr2.p);
            HIP_TRY(hipGetLastError());
        } else {
            rc = convert_into(ix, qs, ns, q_dtype, q_dev ? 1 : 0, (uint8_t*)ix->cur.qbuf.p, st, nullptr, nq_padq - ns, nullptr, 0, ix->qsize);
            if (rc) return rc;
        }
        mips::wide_init_kernel<<<(int)((ns_pad + 255) / 256), 256, 0, st>>>((int)ns, (int)ns_pad, w.pool_n, w.tau_c, w.tau_f);
        HIP_TRY(hipGetLastError());

        // ---- threshold scan + select, chunk by chunk (chunks double up to the budget: a pool's expected intake per chunk is
        // k' ln(rows after / rows before))
        mips::WideScanArgs sa;
        sa.docs = f32x ? (const uint16_t*)ix->rows_hi.p : (const uint16_t*)ix->rows.p;
        sa.qbuf = f32x ? (const uint16_t*)ix->qhi.p : (const uint16_t*)ix->cur.qbuf.p;
        sa.ntotal = ix->ntotal;
        sa.ld = sld;
        sa.ksteps = sld / mips::BK;
        sa.nsplit = nsplit;
        sa.nqt = nqt;
        sa.tau = w.tau_f;
        sa.seg = (mips::wkey_t*)ix->w_seg.p;
        sa.segcap = segcap;
        sa.cnt = w.cnt;
        sa.sel = sel.words;
        sa.rlab = ix->labels;
        sa.qlab = qlab_s;
        sa.grp_only = sel.grp_only;
        mips::WideSelArgs se;
        se.seg = sa.seg;
        se.nseg = nseg;
        se.segcap = segcap;
        se.cnt = w.cnt;
        se.pool = (mips::wkey_t*)ix->w_pool.p;
        se.pool_stride = kp;
        se.pool_n = w.pool_n;
        se.tau_c = w.tau_c;
        se.tau_f = w.tau_f;
        se.kp = kp;
        se.n_dev = nullptr;
        se.slot0 = 0;
        int tps = 1;
        int64_t tile = 0;
        for (int chunk = 0; tile < ntiles; ++chunk) {
            if (chunk >= 2) tps = std::min(tps * 2, tps_max);
            sa.tile0 = (int)tile;
            sa.tile_end = (int)std::min<int64_t>(ntiles, tile + (int64_t)tps * nsplit);
            sa.tiles_per_split = tps;
            if (grouped) mips::grouped_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            else if (masked) mips::masked_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            else mips::wide_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            mips::wide_select_kernel<<<(int)ns, mips::WIDE_THREADS, 0, st>>>(se);
            HIP_TRY(hipGetLastError());
            tile = sa.tile_end;
        }

        // ---- canonical scores of the pools, ranking, certificate
        mips::WideRescoreArgs ra;
        ra.pool = se.pool;
        ra.pool_stride = kp;
        ra.pool_n = w.pool_n;
        ra.kp = kp;
        ra.rows = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
        ra.y = f32x ? (const void*)ix->cur.qf32.p : (const void*)ix->cur.qbuf.p;
        ra.ld = cld;
        ra.ntotal = ix->ntotal;
        ra.k = k;
        ra.phi = ix->phi;
        ra.idx_offset = idx_offset;
        ra.out_s = out_s;
        ra.out_i = out_i;
        ra.out_packed = out_packed;
        ra.flag = w.flag;
        ra.nflag = w.words;
        ra.qq = w.qq;
        ra.seed = w.seed;
        ra.xmax2 = ix->xmax2_dev;
        ra.dres2 = f32x ? ix->dres2_dev : nullptr;
        ra.qerr2 = f32x ? (const double*)ix->qerr2.p : nullptr;
        ra.err_c = err_c;
        ra.nsel = sel.nsel;
        if (grouped) {
            if (f32x) {
                if (l2) mips::wide_rescore_kernel<mips::ElemF32, true, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
                else mips::wide_rescore_kernel<mips::ElemF32, false, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            } else {
                if (l2) mips::wide_rescore_kernel<mips::ElemBF16, true, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
                else mips::wide_rescore_kernel<mips::ElemBF16, false, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            }
        } else if (masked) {
            if (f32x) {
                if (l2) mips::wide_rescore_kernel<mips::ElemF32, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
                else mips::wide_rescore_kernel<mips::ElemF32, false, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            } else {
                if (l2) mips::wide_rescore_kernel<mips::ElemBF16, true, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
                else mips::wide_rescore_kernel<mips::ElemBF16, false, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            }
        } else if (f32x) {
            if (l2) mips::wide_rescore_kernel<mips::ElemF32, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            else mips::wide_rescore_kernel<mips::ElemF32, false><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
        } else {
            if (l2) mips::wide_rescore_kernel<mips::ElemBF16, true><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
            else mips::wide_rescore_kernel<mips::ElemBF16, false><<<(int)ns, mips::WIDE_THREADS, 0, st>>>(ra);
        }
        HIP_TRY(hipGetLastError());

        // ---- exact settlement of the flagged queries, sized on the device: rounds of xslots flagged queries, each round a walk
        // over the rows in chunks of xrows; launches past the flagged count leave at once
        mips::compact_flags_kernel<<<1, 256, 0, st>>>(w.flag, (int)ns, w.ids, nflag_slice);
        HIP_TRY(hipGetLastError());
        mips::WideExactArgs xa;
        xa.rows = ra.rows;
        xa.y = ra.y;
        xa.ld = cld;
        xa.ntotal = ix->ntotal;
        xa.ids = w.ids;
        xa.n_dev = nflag_slice;
        xa.qq = w.qq;
        xa.phi = ix->phi;
        xa.seed = w.seed;
        xa.tau_c = w.tau_c;
        xa.pool_n = w.pool_n;
        xa.pool = se.pool;
        xa.pool_stride = kp;
        xa.seg = sa.seg;
        xa.segcap = (int)xrows;
        xa.cnt = w.cnt;
        xa.k = k;
        xa.idx_offset = idx_offset;
        xa.out_s = out_s;
        xa.out_i = out_i;
        xa.out_packed = out_packed;
        xa.sel = sel.words;
        xa.rlab = ix->labels;
        xa.qlab = qlab_s;
        xa.grp_only = sel.grp_only;
        mips::WideSelArgs xe = se;
        xe.nseg = 1;
        xe.segcap = (int)xrows;
        xe.tau_f = nullptr;
        xe.kp = k;
        xe.n_dev = nflag_slice;
        const int xlds = mips::RESOLVE_QB * cld * (int)sizeof(double) + mips::RESOLVE_WAVES * 64 * 9 * 16;
        auto producer = [&](auto kern, int grid) -> int {
            HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, xlds));
            kern<<<grid, 64 * mips::RESOLVE_WAVES, xlds, st>>>(xa);
            return MIPS_OK;
        };
        for (int64_t r = 0; r < ns; r += xslots) {
            xa.slot0 = (int)r;
            xa.nslots = (int)std::min<int64_t>(xslots, ns - r);
            xe.slot0 = (int)r;
            mips::wide_exact_init_kernel<<<(xa.nslots + 255) / 256, 256, 0, st>>>(xa);
            for (int64_t r0 = 0; r0 < ix->ntotal; r0 += xrows) {
                xa.r0 = r0;
                xa.r1 = std::min(ix->ntotal, r0 + xrows);
                const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(512, (xa.r1 - xa.r0 + 511) / 512));
                if (grouped && f32x) rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemF32, true, true, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemF32, false, true, true>, grid);
                else if (grouped) rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemBF16, true, true, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemBF16, false, true, true>, grid);
                else if (masked && f32x) rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemF32, true, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemF32, false, true>, grid);
                else if (masked) rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemBF16, true, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemBF16, false, true>, grid);
                else if (f32x) rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemF32, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemF32, false>, grid);
                else rc = l2 ? producer(mips::wide_exact_kernel<mips::ElemBF16, true>, grid) : producer(mips::wide_exact_kernel<mips::ElemBF16, false>, grid);
                if (rc) return rc;
                mips::wide_select_kernel<<<xa.nslots, mips::WIDE_THREADS, 0, st>>>(xe);
            }
            if (l2) mips::wide_finalize_kernel<true><<<xa.nslots, mips::WIDE_THREADS, 0, st>>>(xa);
            else mips::wide_finalize_kernel<false><<<xa.nslots, mips::WIDE_THREADS, 0, st>>>(xa);
            HIP_TRY(hipGetLastError());
        }
    }
    set_kernel_name(ix, grouped ? "mips::grouped_scan_kernel" : masked ? "mips::masked_scan_kernel" : "mips::wide_scan_kernel");
    // the report: flagged = settled exactly; nothing is ever left unresolved.  (The counts stay on the device:
    // mips_index_margin_stats fetches the two words when asked)
    rep = SearchReport();
    rep.first_dev = (const int*)w.words;
    rep.last_dev = w.words + 1;
    return MIPS_OK;
}

} // namespace
