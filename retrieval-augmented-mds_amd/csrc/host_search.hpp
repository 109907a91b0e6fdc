// Host side of libmips_hip.so, part 3 of 3 (included by mips_hip.hip): what a search does around its scan -- the one-launch
// kernel for the reference's own call shape, the exact pass of flagged queries (resolve_flagged), the ONE re-scan of flagged
// queries (rescan_flagged) behind its stream-ordered and its synchronising caller, the certificate (finish_margin) and the
// optimistic / two-stage first scans (scan_and_finish).  A nested launch -- stage 1, a re-scan -- is a modified COPY of the
// SearchCall; the index is not touched to describe it.
#pragma once

namespace {

// One-launch search for the reference's own call shape (tiny_search.hpp): <= 16 queries, bf16 index of at most
// kTinyMaxRows rows, k_fetch <= 6.  q must be device memory.
constexpr int64_t kTinyMaxRows = 1 << 16;
// certifies: the call settles the queries it flags (host buffers, "margin_check" = 2, or stream-ordered).  The fp32-exact
// index takes the one-launch kernel only then: its scan sees bf16(x) . bf16(q) (stage 1 of the two-stage search), which is
// admissible because of the certificate alone
bool tiny_eligible(const mips_index* ix, int64_t nq, int k_fetch, bool certifies) {
    if (!(ix->opt_tiny != 0 && nq >= 1 && nq <= 16 && k_fetch <= mips::TINY_MAXK && ix->ntotal > 0 && ix->ntotal <= kTinyMaxRows &&
          ix->esize == 2))
        return false;
    if (ix->plane > 0) return certifies && ix->opt_f32_fast != 0 && ix->hp > 0 && ix->hp <= 1024 && ix->hp % 128 == 0;
    return ix->ld <= 1024 && ix->ld % 128 == 0;
}

int ensure_resolve_buffers(mips_index* ix, int64_t nq) {
    int rc = ix->ids.ensure((size_t)(nq + 4) * sizeof(int));
    if (rc) return rc;
    rc = ix->hit_d.ensure((size_t)mips::RESOLVE_MAX * mips::RESOLVE_CAP * sizeof(double));
    if (rc) return rc;
    rc = ix->hit_i.ensure((size_t)mips::RESOLVE_MAX * mips::RESOLVE_CAP * sizeof(int));
    if (rc) return rc;
    rc = ix->hit_n.ensure((size_t)mips::RESOLVE_MAX * sizeof(int));
    if (rc) return rc;
    rc = ix->keyk.ensure((size_t)nq * sizeof(float));
    if (rc) return rc;
    return ix->qqv.ensure((size_t)nq * sizeof(double));
}

// handoff: prepare the stream-ordered exact pass (resolve_flagged with skip_compact) -- the kernel's last workgroup writes
// the flag list, clears the hit counters and copies the staged queries out when something was flagged (c.qbuf / c.qf32: where to).
// *nflag_dev: where the kernel counts the queries it flags (nullptr: the margin check is off)
// qlab_dev != nullptr: the grouped form (mips_search_fused_grp) -- [nq] query labels on the device, tested against the index's
// row labels; hook_grouped_kernel instead of tiny_search_kernel
int tiny_search(mips_index* ix, SearchCall& c, const void* q_dev, int q_dtype, int64_t nq, int k_fetch, int k_out, int normalize, const int64_t* ignore_dev,
                float* d_s, int64_t* d_i, bool packed, int64_t idx_offset, hipStream_t st, bool handoff, unsigned** nflag_dev,
                const int* qlab_dev = nullptr, int grp_only = 0) {
    const bool f32x = ix->plane > 0;
    const int tld = f32x ? ix->hp : ix->ld; // row pitch of the scanned bf16 rows
    if (f32x) { // bf16 rows + residual bound up to date, max |x|^2 on the fp32 rows
        int rc0 = ensure_hi(ix, st);
        if (rc0) return rc0;
    }
    if (!ix->tiny_words) {
        HIP_TRY(hipMalloc((void**)&ix->tiny_words.p, 64));
        HIP_TRY(hipMemsetAsync(ix->tiny_words, 0, 64, st)); // the ticket starts at 0; the kernel's last workgroup resets it
    }
    const int ntiles = (int)((ix->ntotal + 15) / 16);
    // one tile per wave, 8 waves per workgroup, while the chip has the CUs for it (more workgroups = more candidates for
    // the last one to sift; spreading thinner did not make the first tiles arrive sooner)
    const int nwg = (int)std::max<int64_t>(1, std::min<int64_t>(mips::TINY_MAX_WG, (ntiles + mips::TINY_WAVES - 1) / mips::TINY_WAVES));
    mips::TinyArgs a;
    a.docs = (const uint16_t*)(f32x ? ix->rows_hi.p : ix->rows.p);
    a.rows_f32 = ix->rows_f32;
    a.plane = ix->plane;
    a.q = q_dev;
    a.q_is_f32 = q_dtype == MIPS_DTYPE_F32 ? 1 : 0;
    a.normalize = normalize;
    a.nq = (int)nq;
    a.d = (int)ix->d;
    a.ld = tld;
    a.ntotal = ix->ntotal;
    a.res_ids = nullptr;
    a.res_cnt = nullptr;
    a.res_hit_n = nullptr;
    a.res_unres = nullptr;
    a.q_out = nullptr;
    a.ntiles = ntiles;
    a.nwaves = nwg * mips::TINY_WAVES;
    a.force_slow = ix->opt_tiny == 2 ? 1 : 0;
    a.ticket = ix->tiny_words;
    a.ignore = ignore_dev;
    a.k_out = k_out;
    a.out_s = d_s;
    a.out_i = d_i;
    a.out_packed = packed ? d_i : nullptr;
    a.rlab = nullptr;
    a.qlab = qlab_dev;
    a.grp_only = grp_only;
    if (qlab_dev != nullptr) { // (a lane loads the four labels of its rows of a 16-row tile: the storage covers whole tiles)
        if (ix->labels_cap < (int64_t)ntiles * 16) return fail(MIPS_E_INVALID, "tiny_search: the row labels do not cover the index (mips_index_set_labels)");
        a.rlab = ix->labels;
    }
    const size_t ncand = (size_t)nwg * mips::TINY_POOL; // per query: the 8 best of every workgroup
    int rc = ix->cur.part_s.ensure(16 * (ncand + nwg) * sizeof(float)); // + the workgroups' bounds behind the candidates
    if (rc) return rc;
    rc = ix->cur.part_i.ensure(16 * ncand * sizeof(int));
    if (rc) return rc;
    mips::MergeArgs& m = a.m;
    m.part_s = (const float*)ix->cur.part_s.p;
    m.part_i = (const int*)ix->cur.part_i.p;
    m.ncand = (int)ncand;
    m.pre_bnd = (const float*)ix->cur.part_s.p + 16 * ncand;
    m.npre = nwg;
    m.docs = a.docs;
    m.qbuf = nullptr;
    m.ld = tld;
    m.k = k_fetch;
    m.metric = c.metric;
    m.phi = ix->phi;
    m.idx_offset = idx_offset;
    m.out_s = nullptr;
    m.out_i = nullptr;
    m.out_packed = nullptr;
    m.err = nullptr;
    m.sticky = ix->sticky_dev;
    m.ll = 0x7fffffff; // final level: no "last entry of a full list" rule, the workgroups' bounds carry that
    m.bnd = nullptr;
    m.flag = nullptr;
    m.nflag = nullptr;
    m.xmax2 = ix->xmax2_dev;
    m.err_c = (double)ix->d * 1.1920928955078125e-07 * (f32x ? 1.01 : 1.0); // (F32: the scan's operands are bf16(q), bf16(x))
    m.dres2 = ix->dres2_dev;
    *nflag_dev = nullptr;
    if (c.margin != 0) {
        rc = ix->cur.mbnd.ensure(16 * sizeof(float));
        if (rc) return rc;
        rc = ix->cur.mflag.ensure(16);
        if (rc) return rc;
        rc = ensure_xmax2(ix, st);
        if (rc) return rc;
        m.xmax2 = ix->xmax2_dev;
        m.bnd = (float*)ix->cur.mbnd.p;
        m.flag = (unsigned char*)ix->cur.mflag.p;
        m.nflag = ix->tiny_words + 1;
        *nflag_dev = m.nflag;
        if (handoff) {
            rc = ensure_resolve_buffers(ix, nq);
            if (rc) return rc;
            if (f32x) rc = ix->cur.qf32.ensure((size_t)16 * ix->plane * sizeof(float));
            else rc = ix->cur.qbuf.ensure((size_t)16 * ix->ld * 2);
            if (rc) return rc;
            a.res_ids = (int*)ix->ids.p;
            a.res_cnt = a.res_ids + nq;
            a.res_unres = (unsigned*)(a.res_ids + nq + 1);
            a.res_hit_n = (int*)ix->hit_n.p;
            a.q_out = f32x ? ix->cur.qf32.p : ix->cur.qbuf.p;
            if (f32x) c.qf32 = a.q_out; // (the exact pass reads the flagged queries from there)
            else c.qbuf = a.q_out;
            m.keyk = (float*)ix->keyk.p;
            m.qq_out = (double*)ix->qqv.p;
        }
    } else if (f32x) {
        return fail(MIPS_E_INVALID, "tiny_search: the fp32-exact index needs the margin check");
    }
    const int lds = mips::tiny_lds_bytes(tld, ix->plane);
    auto go = [&](auto kern) -> int {
        if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        kern<<<nwg, mips::TINY_THREADS, lds, st>>>(a);
        return MIPS_OK;
    };
    const bool l2m = c.metric == MIPS_METRIC_L2;
    const bool grp = qlab_dev != nullptr;
    if (grp) {
        if (f32x) rc = l2m ? go(mips::hook_grouped_kernel<true, true>) : go(mips::hook_grouped_kernel<false, true>);
        else rc = l2m ? go(mips::hook_grouped_kernel<true, false>) : go(mips::hook_grouped_kernel<false, false>);
    } else if (f32x) rc = l2m ? go(mips::tiny_search_kernel<true, true>) : go(mips::tiny_search_kernel<false, true>);
    else rc = l2m ? go(mips::tiny_search_kernel<true, false>) : go(mips::tiny_search_kernel<false, false>);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    set_kernel_name(ix, grp ? "mips::hook_grouped_kernel<%s, %s>" : "mips::tiny_search_kernel<%s, %s>", l2m ? "true" : "false", f32x ? "true" : "false");
    return MIPS_OK;
}

// Exact resolution of the flagged queries (resolve_kernels.hpp): flag list + count on the device, one pass over the stored
// rows per 8 flagged queries computing canonical scores, the hit lists ranked over the first results.
// certify_now: the call synchronises anyway (host buffers / "margin_check" = 2): the count is read first, and a search that
// flagged more than RESOLVE_MAX queries is handed to the tile re-scan (return value kUseRescan).  Otherwise everything is
// enqueued blind and the report names the two device words (the flagged count, what is still unresolved).
// rep: the call's report -- on entry "unknown", with the first scan's counter in last_dev.
constexpr int kUseRescan = 1;
// skip_compact: the flag list, its count and the cleared counters are already on the device (the one-launch kernel's hand-off).
// ignore / k_out: the fused hook call's ignore filter (ResolveArgs), d_s / d_i then are [nq][k_out].
// qlab_dev / grp_only: the flagging search was the grouped hook call -- the same rule decides what becomes a hit.
int resolve_flagged(mips_index* ix, const SearchCall& c, SearchReport& rep, int64_t nq, int k, float* d_s, int64_t* d_i, bool packed, int64_t idx_offset, hipStream_t st, bool certify_now,
                    bool skip_compact = false, const int64_t* ignore = nullptr, int k_out = 0, const int* qlab_dev = nullptr, int grp_only = 0) {
    if (k > mips::RESOLVE_OVF_K) return fail(MIPS_E_UNSUPPORTED, "resolve_flagged: k = %d exceeds RESOLVE_OVF_K", k);
    int rc = ensure_resolve_buffers(ix, nq); // (never reallocates behind a hand-off: same sizes as tiny_search asked for)
    if (rc) return rc;
    int* ids = (int*)ix->ids.p;
    int* cnt = ids + nq;
    unsigned* unres = (unsigned*)(ids + nq + 1);
    rc = ensure_nflag_host(ix);
    if (rc) return rc;
    const int max_n = ix->resolve_budget > 0 ? std::min(ix->resolve_budget, mips::RESOLVE_MAX) : mips::RESOLVE_MAX;
    if (!skip_compact)
        mips::compact_flags_kernel<<<1, 256, 0, st>>>((const unsigned char*)ix->cur.mflag.p, (int)nq, ids, cnt, (int*)ix->hit_n.p, mips::RESOLVE_MAX, unres);
    if (certify_now) {
        HIP_TRY(hipMemcpyAsync(&ix->nflag_host[0], cnt, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t n = (int64_t)ix->nflag_host[0];
        rep.flagged = n;
        if (n == 0) return MIPS_OK;
        if (n > max_n && !skip_compact) return kUseRescan; // (the one-launch kernel's <= 16 queries have no tile re-scan to go to)
    }
    mips::ResolveArgs a;
    const bool f32x = ix->plane > 0;
    a.rows = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
    a.y = f32x ? c.qf32 : c.qbuf;
    a.ld = f32x ? ix->plane : ix->ld;
    a.ntotal = ix->ntotal;
    a.ids = ids;
    a.n_dev = cnt;
    a.max_n = max_n;
    rep.max_n = max_n;
    a.keyk = (const float*)ix->keyk.p;
    a.qq = (const double*)ix->qqv.p;
    a.phi = ix->phi;
    a.hit_d = (double*)ix->hit_d.p;
    a.hit_i = (int*)ix->hit_i.p;
    a.hit_n = (int*)ix->hit_n.p;
    a.k = k;
    a.idx_offset = idx_offset;
    a.out_s = d_s;
    a.out_i = d_i;
    a.out_packed = packed ? d_i : nullptr;
    a.unresolved = unres;
    a.ignore = ignore;
    a.k_out = ignore ? k_out : 0;
    if (qlab_dev != nullptr) {
        a.rlab = ix->labels;
        a.qlab = qlab_dev;
        a.grp_only = grp_only;
    }
    int lds = mips::RESOLVE_QB * a.ld * (int)sizeof(double) + mips::RESOLVE_WAVES * 64 * 9 * 16;
    const int rows_per_wg = 64 * mips::RESOLVE_WAVES;
    int grid = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (ix->ntotal + rows_per_wg - 1) / rows_per_wg));
    const bool l2 = c.metric == MIPS_METRIC_L2;
    auto go = [&](auto kern) -> int {
        HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        kern<<<grid, 64 * mips::RESOLVE_WAVES, lds, st>>>(a);
        return MIPS_OK;
    };
    // bf16-stored rows and the fp32-exact index: the same pass behind an MFMA pre-filter (16 flagged queries per pass, canonical
    // evaluation of the few rows whose approximate score comes within the error bound of the k-th key; "resolve" = 2 keeps the
    // plain form -- tests compare the two)
    const int ffld = f32x ? ix->hp : ix->ld;
    const bool mfma_filter = ix->opt_resolve == 1 && (f32x ? (ix->hp > 0 && ix->rows_hi != nullptr) : (ix->esize == 2 && !ix->mixed)) &&
                             ffld % 64 == 0 && ffld <= 1024 && a.ld <= 1024;
    if (mfma_filter) {
        if (f32x) {
            rc = ensure_hi(ix, st);
            if (rc) return rc;
        }
        rc = ensure_xmax2(ix, st);
        if (rc) return rc;
        a.frows = (const uint16_t*)(f32x ? ix->rows_hi.p : ix->rows.p);
        a.fld = ffld;
        a.xmax2 = ix->xmax2_dev;
        a.dres2 = ix->dres2_dev;
        a.err_c = (double)ix->d * 1.1920928955078125e-07 * (f32x ? 1.01 : 1.0);
        // query image (row pitch + 16 B) + the waves' product staging + statistics / thresholds / keys / ids
        lds = ((mips::RESOLVE_QM * (ffld * 2 + 16) + 15) & ~15) + mips::RESOLVE_WAVES * 64 * 8 * 8 + 2 * mips::RESOLVE_QM * 8 + 3 * mips::RESOLVE_QM * 4;
        const int64_t tiles = (ix->ntotal + 15) / 16;
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(512, (tiles + mips::RESOLVE_WAVES - 1) / mips::RESOLVE_WAVES));
        if (f32x) rc = l2 ? go(mips::exact_filter_mfma_kernel<true, true>) : go(mips::exact_filter_mfma_kernel<false, true>);
        else rc = l2 ? go(mips::exact_filter_mfma_kernel<true, false>) : go(mips::exact_filter_mfma_kernel<false, false>);
    } else if (f32x) rc = l2 ? go(mips::exact_filter_kernel<mips::ElemF32, true>) : go(mips::exact_filter_kernel<mips::ElemF32, false>);
    else if (ix->sq8) rc = go(mips::exact_filter_kernel<mips::ElemU8, false, mips::ElemBF16>);
    else if (ix->mixed) rc = l2 ? go(mips::exact_filter_kernel<mips::ElemF8, true, mips::ElemBF16>) : go(mips::exact_filter_kernel<mips::ElemF8, false, mips::ElemBF16>);
    else if (ix->esize == 1) rc = l2 ? go(mips::exact_filter_kernel<mips::ElemF8, true>) : go(mips::exact_filter_kernel<mips::ElemF8, false>);
    else rc = l2 ? go(mips::exact_filter_kernel<mips::ElemBF16, true>) : go(mips::exact_filter_kernel<mips::ElemBF16, false>);
    if (rc) return rc;
    const int fgrid = (int)std::min<int64_t>(nq, certify_now ? (int64_t)ix->nflag_host[0] : (int64_t)a.max_n); // (at least one block: it counts an over-budget search)
    if (l2) mips::resolve_finalize_kernel<true><<<fgrid, 64, 0, st>>>(a);
    else mips::resolve_finalize_kernel<false><<<fgrid, 64, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    // floods (more hits than a hit list holds): one workgroup per RESOLVE_QB flagged slots ranks them over the whole index; the
    // workgroups of batches without one read RESOLVE_QB counters and leave
    grid = (fgrid + mips::RESOLVE_QB - 1) / mips::RESOLVE_QB;
    lds = mips::RESOLVE_QB * a.ld * (int)sizeof(double) + mips::RESOLVE_WAVES * 64 * 9 * 16; // (the plain pass's layout; the lists
                                                                                            // meet over the tiles)
    if (f32x) rc = l2 ? go(mips::resolve_overflow_kernel<mips::ElemF32, true>) : go(mips::resolve_overflow_kernel<mips::ElemF32, false>);
    else if (ix->sq8) rc = go(mips::resolve_overflow_kernel<mips::ElemU8, false, mips::ElemBF16>);
    else if (ix->mixed) rc = l2 ? go(mips::resolve_overflow_kernel<mips::ElemF8, true, mips::ElemBF16>) : go(mips::resolve_overflow_kernel<mips::ElemF8, false, mips::ElemBF16>);
    else if (ix->esize == 1) rc = l2 ? go(mips::resolve_overflow_kernel<mips::ElemF8, true>) : go(mips::resolve_overflow_kernel<mips::ElemF8, false>);
    else rc = l2 ? go(mips::resolve_overflow_kernel<mips::ElemBF16, true>) : go(mips::resolve_overflow_kernel<mips::ElemBF16, false>);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    rep.first_dev = cnt;
    rep.last_dev = unres;
    if (certify_now) {
        HIP_TRY(hipMemcpyAsync(&ix->nflag_host[1], unres, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rep.rescanned = rep.settled();
        rep.unresolved = (int64_t)ix->nflag_host[1];
    } // (else device only: mips_index_margin_stats fetches the two counters when asked)
    return MIPS_OK;
}

// Widest lists this storage type has (K' = 32; 16 on an fp8 index), or 0 when the first scan already kept them.  recheck: the
// first scan was stage 1 of the two-stage fp32 search or took its pool from sub-lists (PoolPolicy::recheck) -- the second is
// the three-segment scan / true K' = 32 lists whatever K' was
template <int KL>
int widest_lists(const mips_index* ix, bool recheck) {
    return ix->esize == 1 ? (KL < 16 ? 16 : 0) : (KL < 32 || recheck ? 32 : 0);
}

// The second scan of flagged queries, both forms: the staged rows of the queries listed in ids (device) are gathered into a
// compact query buffer, the insert bounds cleared, the compact queries searched with the widest lists -- a nested launch that
// is neither timed nor named and prepares nothing for a third scan -- and its rows scattered over the first results.
//   synchronising form:  n = the flagged count as the host read it, cnt = nullptr
//   stream-ordered form: n = ALL queries (what the launches are sized for), cnt = the count on the device: workgroups past it
//                        leave (ScanArgs::nq_dev), select, re-score and the scatter do the same
// nsplit: few flagged queries = few query tiles, so each tile's scan is spread over more splits than the automatic choice makes
// (0 = that choice; the caller's heuristic, which "nsplit" overrides)
// rep.last_dev becomes the re-scan's own counter: the queries still flagged on the widest lists
int rescan_flagged(mips_index* ix, const SearchCall& c, SearchReport& rep, int wide, const int* ids, int64_t n, const int* cnt, int nsplit, int k, float* d_s,
                   int64_t* d_i, bool packed, int64_t idx_offset, hipStream_t st) {
    const int64_t n_pad = query_pad(ix, n);
    const size_t row_bytes = (size_t)c.ld * ix->qsize;
    int rc = ix->qbuf2.ensure((size_t)n_pad * row_bytes);
    if (rc) return rc;
    rc = ix->tmp_s.ensure((size_t)n * k * sizeof(float));
    if (rc) return rc;
    rc = ix->tmp_i.ensure((size_t)n * k * sizeof(int64_t) * 2);
    if (rc) return rc;
    SearchCall r = c;
    r.qbuf = ix->qbuf2.p;
    mips::gather_rows_kernel<<<grid_for(n_pad * (int64_t)(row_bytes / 16), 256), 256, 0, st>>>((const unsigned char*)c.qbuf, ids, n, n_pad, (int)row_bytes,
                                                                                              (unsigned char*)ix->qbuf2.p, cnt);
    if (c.plane > 0) {
        const size_t rb32 = (size_t)c.plane * sizeof(float);
        rc = ix->qf32b.ensure((size_t)n_pad * rb32);
        if (rc) return rc;
        r.qf32 = ix->qf32b.p;
        mips::gather_rows_kernel<<<grid_for(n_pad * (int64_t)(rb32 / 16), 256), 256, 0, st>>>((const unsigned char*)c.qf32, ids, n, n_pad, (int)rb32,
                                                                                            (unsigned char*)ix->qf32b.p, cnt);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(ix->cur.gthr.p, 0, (size_t)(n_pad * 8 + 4) * sizeof(unsigned), st)); // insert bounds, error word, flag counter
    r.optimistic = false;
    r.rescan = true;
    r.nq_dev = cnt;
    r.nsplit = c.nsplit != 0 ? c.nsplit : nsplit;
    r.timed = false; // the bench's event window times the first scan only, and last_kernel keeps naming it
    float* ts = (float*)ix->tmp_s.p;
    int64_t* ti = (int64_t*)ix->tmp_i.p;
    if (wide == 32) rc = launch_search<32>(ix, r, n, k, ts, ti, packed ? ti : nullptr, idx_offset, st, &rep.last_dev);
    else rc = launch_search<16>(ix, r, n, k, ts, ti, packed ? ti : nullptr, idx_offset, st, &rep.last_dev);
    if (rc) return rc;
    if (packed) {
        mips::scatter_i64_kernel<<<grid_for(n * 2 * k, 256), 256, 0, st>>>(ti, ids, n, 2 * k, d_i, cnt);
    } else {
        mips::scatter_i64_kernel<<<grid_for(n * k, 256), 256, 0, st>>>(ti, ids, n, k, d_i, cnt);
        mips::scatter_f32_kernel<<<grid_for(n * k, 256), 256, 0, st>>>(ts, ids, n, k, d_s, cnt);
    }
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

// "margin_check" = 3, device outputs: the re-scan without a synchronisation.  The flags of the first scan are compacted into a
// list + count ON THE DEVICE and rescan_flagged runs in its stream-ordered form.  With nothing flagged this costs a handful of
// empty launches (tens of microseconds); mips_index_margin_stats reads both counters when asked.
// gate_above >= 0: the fall-back behind the exact pass for searches whose first scan was an optimistic one (PoolPolicy::recheck):
// the exact pass leaves a search that flagged more than gate_above queries alone, and first results selected by bf16 scores /
// short sub-lists must not stand uncertified -- so this re-scan runs exactly then (its launches are sized by a count that is 0
// otherwise) and its own still-flagged count replaces the exact pass's "unresolved".
template <int KL>
int rescan_on_stream(mips_index* ix, const SearchCall& c, SearchReport& rep, int64_t nq, int k, float* d_s, int64_t* d_i, bool packed, int64_t idx_offset, hipStream_t st,
                     bool recheck, int gate_above = -1) {
    const int wide = widest_lists<KL>(ix, recheck);
    if (wide == 0) return MIPS_OK; // already on the widest lists: counted only (rep.last_dev: the first scan's counter)
    int rc = ix->ids.ensure((size_t)(nq + 4) * sizeof(int));
    if (rc) return rc;
    int* ids = (int*)ix->ids.p;
    int* cnt = ids + nq + (gate_above >= 0 ? 2 : 0); // (gated: the exact pass's own count and unresolved counter stay where they are)
    unsigned* const exact_unres = (unsigned*)(ids + nq + 1);
    mips::compact_flags_kernel<<<1, 256, 0, st>>>((const unsigned char*)ix->cur.mflag.p, (int)nq, ids, cnt, nullptr, 0, nullptr, gate_above);
    // the flagged queries are few: spread each of their tiles over many CUs
    rc = rescan_flagged(ix, c, rep, wide, ids, nq, cnt, nq <= 4096 ? 128 : nq <= 8192 ? 64 : 0, k, d_s, d_i, packed, idx_offset, st);
    if (rc) return rc;
    if (gate_above >= 0) { // statistics stay the exact pass's; if this re-scan ran, what IT still flags is what is unresolved
        mips::adopt_rescan_count_kernel<<<1, 1, 0, st>>>(cnt, rep.last_dev, exact_unres);
        HIP_TRY(hipGetLastError());
        rep.last_dev = exact_unres; // (first_dev, max_n: as the exact pass left them)
        rep.fallback = true;
        return MIPS_OK;
    }
    rep.first_dev = cnt; // (last_dev: the re-scan's own counter)
    return MIPS_OK;
}

// Margin check, host side.  The re-score flagged every query whose k-th exact score is within the MFMA error bound of
// what the candidate pool may have excluded (aux_kernels.hpp).  Flagged queries are settled exactly, by brute force on the
// canonical scores (resolve_flagged: rows of up to 1024 columns); beyond that, with "resolve" = 0 and when more are flagged
// than the exact pass takes, they are re-scanned with the widest lists -- on the stream ("margin_check" = 3, device outputs) or,
// when the call may synchronise (host buffers, "margin_check" = 2), here: the flag list is read back and rescan_flagged runs in
// its synchronising form.  Queries still flagged after that are counted as unresolved (mips_index_margin_stats).
template <int KL>
int finish_margin(mips_index* ix, const SearchCall& c, SearchReport& rep, int64_t nq, int k, float* d_s, int64_t* d_i, bool packed, int64_t idx_offset, bool out_dev,
                  hipStream_t st, bool recheck) {
    if (!call_certifies(c.margin, out_dev)) return MIPS_OK; // off, or counted on the device only
    const bool stream_ordered = out_dev && c.margin == 3;
    if (ix->opt_resolve != 0 && (c.plane > 0 ? c.plane : c.ld) <= 1024) {
        const int r = resolve_flagged(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, st, !stream_ordered);
        if (r == MIPS_OK && stream_ordered && recheck) {
            const int max_n = ix->resolve_budget > 0 ? std::min(ix->resolve_budget, mips::RESOLVE_MAX) : mips::RESOLVE_MAX;
            if (nq > max_n) return rescan_on_stream<KL>(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, st, recheck, max_n);
        }
        if (r != kUseRescan) return r; // (else more flagged than the exact pass takes: the tile re-scan below, which synchronises)
    } else if (stream_ordered) {
        return rescan_on_stream<KL>(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, st, recheck);
    }
    int rc = ensure_nflag_host(ix);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->nflag_host, rep.last_dev, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n = (int64_t)ix->nflag_host[0];
    rep.flagged = n;
    if (n == 0) return MIPS_OK;
    const int wide = widest_lists<KL>(ix, recheck);
    if (wide == 0) { // already on the widest lists this storage type has
        rep.unresolved = n;
        return MIPS_OK;
    }
    // flagged query numbers
    std::string flags((size_t)nq, '\0');
    HIP_TRY(hipMemcpyAsync(&flags[0], ix->cur.mflag.p, (size_t)nq, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> ids_h;
    for (int64_t q = 0; q < nq && (int64_t)ids_h.size() < n; ++q)
        if (flags[(size_t)q]) ids_h.push_back((int)q);
    if ((int64_t)ids_h.size() != n)
        return fail(MIPS_E_HIP, "margin check: flag count %lld does not match the flag array (%lld)", (long long)n, (long long)ids_h.size());
    rc = ix->ids.ensure((size_t)n * sizeof(int));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->ids.p, ids_h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    // (the automatic split choice stops at 64; one 128-query tile of the three-segment scan on 64 workgroups took 17 ms at
    // 2^20 x 768)
    const int nsplit = n <= 1024 ? (int)std::max<int64_t>(64, std::min<int64_t>(256, round_up(512 / ((n + 127) / 128), 8))) : 0;
    rc = rescan_flagged(ix, c, rep, wide, (const int*)ix->ids.p, n, nullptr, nsplit, k, d_s, d_i, packed, idx_offset, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->nflag_host, rep.last_dev, 4, hipMemcpyDeviceToHost, st)); // still flagged on the widest lists
    HIP_TRY(hipStreamSynchronize(st));
    rep.rescanned = n;
    rep.unresolved = (int64_t)ix->nflag_host[0];
    return MIPS_OK;
}

// One scan + select + exact re-score + margin finish at list length KL = pol.kl.  pol.fast: stage 1 of the two-stage search of an
// fp32-exact index -- the launch gets a COPY of the call that views the index as the bf16 index rows_hi (pitch hp) with the bf16
// queries qhi; the re-score and the margin check still run on the fp32 rows (SearchCall::stage1).  Queries the widened margin
// cannot certify are settled by finish_margin, which sees the call as it came in.
template <int KL>
int scan_and_finish(mips_index* ix, const SearchCall& c, SearchReport& rep, const PoolPolicy& pol, int64_t nq, int k, float* d_s, int64_t* d_i, bool packed,
                    int64_t idx_offset, bool out_dev, hipStream_t st, hipStream_t tail_st, bool split) {
    SearchCall first = c;
    first.optimistic = pol.optimistic;
    if (pol.fast) {
        first.rows = ix->rows_hi;
        first.ld = ix->hp;
        first.plane = 0;
        first.stage1 = true;
        first.rescore_ld = c.plane;
        first.qbuf = ix->qhi.p;
    }
    int rc = launch_search<KL>(ix, first, nq, k, d_s, d_i, packed ? d_i : nullptr, idx_offset, st, &rep.last_dev, tail_st, split);
    if (rc) return rc;
    if (split) { // scan on st, tail on tail_st: the certificate, when asked for, is part of the tail
        if (c.margin == 3 && out_dev && ix->opt_resolve != 0 && (c.plane > 0 ? c.plane : c.ld) <= 1024) {
            rc = resolve_flagged(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, tail_st, false);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(ix->cur.tail_done, tail_st)); // (supersedes the record behind the re-score: the exact
            ix->cur.tail_pending = true;                         // pass reads this set's staged queries)
        }
        return MIPS_OK;
    }
    rc = finish_margin<KL>(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, out_dev, st, pol.recheck);
    // the optimistic scan pays while few queries need the second one: after a synchronising call that sent more than an eighth
    // (and at least 64) there, pool_policy skips it for the next 8 calls
    if (!rc && pol.recheck && ix->opt_f32_fast != 2 && rep.flagged >= 64 && rep.flagged * 8 > nq) ix->fast_skip = 8;
    return rc;
}

} // namespace
