// Host side of mips_range_search (included by mips_hip.hip behind host_wide.hpp): query slices, chunk geometry, launches and the
// scratch of the range search (range_kernels.hpp).  Everything is enqueued on the caller's stream; the only synchronisation is the
// one a host-output call ends with (in the entry point).
#pragma once

namespace {

static_assert(kWideSlice == 4 * mips::RANGE_LIMS_THREADS, "range_lims_kernel takes one slice: 4 queries per thread");

// d_lims [nq + 1], d_s / d_i [cap] are DEVICE buffers; radii is the caller's HOST array.  nq > 0 and ntotal > 0.
int range_search(mips_index* ix, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t* d_lims, float* d_s, int64_t* d_i, int64_t cap,
                 int64_t idx_offset, bool q_dev, Selector sel, int metric, hipStream_t st) {
    // a filtered or grouped search: only the scan changes, the filter sees appended rows alone
    const bool grouped = sel.qlab != nullptr;
    const bool masked = sel.bits != nullptr && !grouped;
    const bool f32x = ix->plane > 0;
    const bool l2 = metric == MIPS_METRIC_L2;
    const int sld = f32x ? ix->hp : ix->ld;    // row pitch of the scanned bf16 rows
    const int cld = f32x ? ix->plane : ix->ld; // row pitch of the canonical rows and queries
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

    // ---- geometry, fixed for the call: the wide search's slices and segments, chunks capped at what the filter's LDS holds
    const int64_t slice = std::min<int64_t>(nq, kWideSlice);
    const int64_t slice_pad = round_up(slice, mips::TN);
    const int nqt_max = (int)(slice_pad / mips::TN);
    const int64_t ntiles = (ix->ntotal + mips::TM - 1) / mips::TM;
    constexpr int kChunkTiles = mips::RANGE_CHUNK / mips::TM;
    int nsplit = (int)round_up((512 + nqt_max - 1) / nqt_max, 8);
    nsplit = std::min(nsplit, kChunkTiles);
    nsplit = (int)std::min<int64_t>(nsplit, round_up(ntiles, 8));
    const int tps = (int)std::max<int64_t>(1, std::min<int64_t>(kChunkTiles / nsplit, (ntiles + nsplit - 1) / nsplit));
    const int64_t chunk_tiles = (int64_t)tps * nsplit;   // <= kChunkTiles
    const int nchunks = (int)((ntiles + chunk_tiles - 1) / chunk_tiles);
    const int segcap = tps * (mips::TM / 2);
    const int nseg = 2 * nsplit;                         // <= 128; nseg * segcap = rows of a chunk <= RANGE_CHUNK

    rc = ix->w_seg.ensure((size_t)slice_pad * nseg * segcap * sizeof(mips::wkey_t)); // <= kWideBudget entries
    if (rc) return rc;
    rc = ix->w_cnt.ensure((size_t)slice_pad * nseg * sizeof(int));
    if (rc) return rc;
    rc = ix->r_stage.ensure((size_t)cap * (sizeof(float) + sizeof(int)));
    if (rc) return rc;
    rc = ix->r_blk.ensure((size_t)slice * nchunks * (sizeof(unsigned long long) + sizeof(int)));
    if (rc) return rc;
    const size_t P = (size_t)slice_pad;
    rc = ix->r_misc.ensure(64 + P * (8 + 4 + 4) + (size_t)nq * sizeof(float));
    if (rc) return rc;
    unsigned long long* const words = (unsigned long long*)ix->r_misc.p; // [0] staging cursor of the slice, [1] members of the slices before
    double* const qq = (double*)((unsigned char*)ix->r_misc.p + 64);
    float* const tau = (float*)(qq + P);
    int* const qtot = (int*)(tau + P);
    float* const radii_dev = (float*)(qtot + P);
    float* const stage_s = (float*)ix->r_stage.p;
    int* const stage_r = (int*)(stage_s + cap);
    unsigned long long* const blk_off = (unsigned long long*)ix->r_blk.p;
    int* const blk_cnt = (int*)(blk_off + (size_t)slice * nchunks);
    HIP_TRY(hipMemsetAsync(words, 0, 64, st));
    HIP_TRY(hipMemcpyAsync(radii_dev, radii, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st));

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
        const void* rows_c = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
        const void* y_c = f32x ? (const void*)ix->cur.qf32.p : (const void*)ix->cur.qbuf.p;

        // ---- the thresholds of the slice, fixed from here on; empty staging, no members yet
        mips::RangeTauArgs ta;
        ta.y = y_c;
        ta.ld = cld;
        ta.nq = (int)ns;
        ta.nq_pad = (int)ns_pad;
        ta.radii = radii_dev + s0;
        ta.l2 = l2 ? 1 : 0;
        ta.phi = ix->phi;
        ta.xmax2 = ix->xmax2_dev;
        ta.dres2 = f32x ? ix->dres2_dev : nullptr;
        ta.qerr2 = f32x ? (const double*)ix->qerr2.p : nullptr;
        ta.err_c = err_c;
        ta.tau = tau;
        ta.qq = qq;
        if (f32x) mips::range_tau_kernel<mips::ElemF32><<<(int)((ns_pad + 255) / 256), 256, 0, st>>>(ta);
        else mips::range_tau_kernel<mips::ElemBF16><<<(int)((ns_pad + 255) / 256), 256, 0, st>>>(ta);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(words, 0, 8, st));
        HIP_TRY(hipMemsetAsync(qtot, 0, (size_t)ns * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(blk_cnt, 0, (size_t)ns * nchunks * sizeof(int), st));

        // ---- threshold scan + exact filter, chunk by chunk
        mips::WideScanArgs sa;
        sa.docs = f32x ? (const uint16_t*)ix->rows_hi.p : (const uint16_t*)ix->rows.p;
        sa.qbuf = f32x ? (const uint16_t*)ix->qhi.p : (const uint16_t*)ix->cur.qbuf.p;
        sa.ntotal = ix->ntotal;
        sa.ld = sld;
        sa.ksteps = sld / mips::BK;
        sa.nsplit = nsplit;
        sa.nqt = nqt;
        sa.tau = tau;
        sa.seg = (mips::wkey_t*)ix->w_seg.p;
        sa.segcap = segcap;
        sa.cnt = (int*)ix->w_cnt.p;
        sa.tiles_per_split = tps;
        sa.sel = sel.words;
        sa.rlab = ix->labels;
        sa.qlab = grouped ? sel.qlab_staged + s0 : nullptr; // (s0 is a multiple of the query tile)
        sa.grp_only = sel.grp_only;
        mips::RangeFilterArgs fa;
        fa.seg = sa.seg;
        fa.nseg = nseg;
        fa.segcap = segcap;
        fa.cnt = sa.cnt;
        fa.rows = rows_c;
        fa.y = y_c;
        fa.ld = cld;
        fa.qq = qq;
        fa.phi = ix->phi;
        fa.radii = radii_dev + s0;
        fa.nchunks = nchunks;
        fa.cursor = words;
        fa.stage_cap = (long long)cap;
        fa.stage_s = stage_s;
        fa.stage_r = stage_r;
        fa.blk_off = blk_off;
        fa.blk_cnt = blk_cnt;
        fa.qtot = qtot;
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            sa.tile0 = (int)(chunk * chunk_tiles);
            sa.tile_end = (int)std::min<int64_t>(ntiles, sa.tile0 + chunk_tiles);
            fa.row0 = sa.tile0 * mips::TM;
            fa.chunk = chunk;
            if (grouped) mips::grouped_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            else if (masked) mips::masked_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            else mips::wide_scan_kernel<<<nqt * nsplit, mips::SCAN_THREADS, scan_lds, st>>>(sa);
            if (f32x) {
                if (l2) mips::range_filter_kernel<mips::ElemF32, true><<<(int)ns, mips::RANGE_THREADS, 0, st>>>(fa);
                else mips::range_filter_kernel<mips::ElemF32, false><<<(int)ns, mips::RANGE_THREADS, 0, st>>>(fa);
            } else {
                if (l2) mips::range_filter_kernel<mips::ElemBF16, true><<<(int)ns, mips::RANGE_THREADS, 0, st>>>(fa);
                else mips::range_filter_kernel<mips::ElemBF16, false><<<(int)ns, mips::RANGE_THREADS, 0, st>>>(fa);
            }
            HIP_TRY(hipGetLastError());
        }

        // ---- CSR: limits of the slice, then its blocks in chunk order
        mips::RangeLimsArgs la;
        la.qtot = qtot;
        la.ns = (int)ns;
        la.s0 = s0;
        la.lims = d_lims;
        la.base = words + 1;
        mips::range_lims_kernel<<<1, mips::RANGE_LIMS_THREADS, 0, st>>>(la);
        if (cap > 0) {
            mips::RangeCompactArgs ca;
            ca.blk_off = blk_off;
            ca.blk_cnt = blk_cnt;
            ca.nchunks = nchunks;
            ca.ns = (int)ns;
            ca.s0 = s0;
            ca.lims = d_lims;
            ca.stage_s = stage_s;
            ca.stage_r = stage_r;
            ca.stage_cap = (long long)cap;
            ca.out_s = d_s;
            ca.out_i = d_i;
            ca.cap = cap;
            ca.idx_offset = idx_offset;
            mips::range_compact_kernel<<<(int)((ns + 3) / 4), 256, 0, st>>>(ca);
        }
        HIP_TRY(hipGetLastError());
    }
    set_kernel_name(ix, grouped ? "mips::grouped_scan_kernel" : masked ? "mips::masked_scan_kernel" : "mips::wide_scan_kernel");
    return MIPS_OK;
}

} // namespace
