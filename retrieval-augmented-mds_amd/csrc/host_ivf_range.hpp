// Host side of the range search over the probed lists (include/mips_hip_ivf_range.h; the kernels: ivf_range_kernels.hpp).  Included
// behind host_ivf.hpp.  mips_ivf_range_search is a fixed launch sequence on the caller's stream -- probe, stage, range scan, lims,
// place, order -- in which every grid, pointer, size and loop bound comes from (nq, p, d, nlist, cap, the CU count) and the index
// object: how many hits there are, where they land and how long a stretch is exist on the device only.
#pragma once

namespace {

int ivf_range_impl(const char* who, mips_ivf* v, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims,
                   float* out_scores, int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits,
                   int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream) {
    int rc = ivf_check(who, v);
    if (rc) return rc;
    if (mips_ivf_is_trained(v) != 1) return fail(MIPS_E_INVALID, "%s: the IVF index is not trained (mips_ivf_train / mips_ivf_set_centroids)", who);
    int p = 0;
    if ((rc = ivf_query_args(who, v, q, q_dtype, nq, nprobe, &p))) return rc;
    if (cap < 0) return fail(MIPS_E_INVALID, "%s: negative cap", who);
    if (flags & MIPS_OUT_PACKED) return fail(MIPS_E_INVALID, "%s: MIPS_OUT_PACKED does not apply to a CSR result", who);
    if (!out_lims || (nq > 0 && !radii) || (cap > 0 && (!out_scores || !out_idx))) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    mips_index* ix = v->flat;
    const bool filtered = sel_bits != nullptr || q_labels != nullptr;
    Selector sel;
    if (filtered && (rc = make_selector(who, ix, flags, sel_bits, sel_nbits, sel_bit0, q_labels, grp_mode, sel))) return rc;
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0, radii_dev = (flags & MIPS_RADII_DEVICE) != 0;
    if (!radii_dev)
        for (int64_t j = 0; j < nq; ++j)
            if (radii[j] != radii[j]) return fail(MIPS_E_INVALID, "%s: radii[%lld] is NaN", who, (long long)j);
    const bool f32x = ix->plane > 0;
    const int ld = f32x ? ix->plane : ix->ld; // elements per canonical row and per staged query
    const int per16 = f32x ? 4 : ix->esize == 2 ? 8 : 16;
    if (ld > mips::IVF_SCAN_MAX_LD || ld % (per16 * mips::IVF_SCAN_TCH) != 0) return fail(MIPS_E_UNSUPPORTED, "%s: row pitch %d is not served", who, ld);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st); // (the staging below is the flat index's; the coarse index orders its own calls)
    IvfSearchScratch& ss = v->ss;
    IvfRangeScratch& rs = v->rs;
    int64_t* d_lims = out_lims;
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    if (!out_dev) {
        if ((rc = rs.lims.ensure((size_t)(nq + 1) * sizeof(int64_t)))) return rc;
        d_lims = (int64_t*)rs.lims.p;
        if (cap > 0) {
            if ((rc = rs.out_s.ensure((size_t)cap * sizeof(float)))) return rc;
            if ((rc = rs.out_i.ensure((size_t)cap * sizeof(int64_t)))) return rc;
            d_s = (float*)rs.out_s.p;
            d_i = (int64_t*)rs.out_i.p;
        }
    }
    if (nq == 0 || ix->ntotal == 0) { // no hits: every limit is 0
        HIP_TRY(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
    } else {
        // a host bitmap, host query labels and host radii travel by the stream's asynchronous copy into the search's scratch; device
        // ones are read where they are
        const uint8_t* d_bits = sel_bits;
        int64_t d_bit0 = sel_bit0;
        const int* d_qlab = (const int*)q_labels;
        if (sel_bits && !sel.dev) {
            const int64_t b0 = sel_bit0 >> 3, b1 = (sel_bit0 + ix->ntotal + 7) >> 3;
            if ((rc = ss.sel.ensure((size_t)(b1 - b0)))) return rc;
            HIP_TRY(hipMemcpyAsync(ss.sel.p, sel_bits + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, st));
            d_bits = (const uint8_t*)ss.sel.p;
            d_bit0 = sel_bit0 & 7;
        }
        if (q_labels && !sel.qlab_dev) {
            if ((rc = ss.qlab.ensure((size_t)nq * sizeof(int)))) return rc;
            HIP_TRY(hipMemcpyAsync(ss.qlab.p, q_labels, (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
            d_qlab = (const int*)ss.qlab.p;
        }
        const float* d_radii = radii;
        if (!radii_dev) {
            if ((rc = rs.radii.ensure((size_t)nq * sizeof(float)))) return rc;
            HIP_TRY(hipMemcpyAsync(rs.radii.p, radii, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st));
            d_radii = (const float*)rs.radii.p;
        }
        const int64_t slice = std::min<int64_t>(nq, ivf::kRangeSlice);
        if ((rc = rs.words.ensure(64))) return rc;
        if ((rc = rs.counts.ensure((size_t)2 * slice * sizeof(int)))) return rc;
        if (cap > 0 && (rc = rs.stage.ensure((size_t)cap * (2 * sizeof(int) + sizeof(float))))) return rc;
        unsigned long long* const words = (unsigned long long*)rs.words.p;
        int* const qcnt = (int*)rs.counts.p;
        int* const qcur = qcnt + slice;
        int* const stage_q = (int*)rs.stage.p; // (never addressed when cap == 0)
        int* const stage_r = stage_q + cap;
        float* const stage_s = (float*)(stage_r + cap);
        HIP_TRY(hipMemsetAsync(words, 0, 64, st));
        const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
        for (int64_t s0 = 0; s0 < nq; s0 += slice) {
            const int64_t ns = std::min(slice, nq - s0);
            const void* qs = (const char*)q + (size_t)s0 * v->d * esz;
            const int S = ivf::choose_segments(ns, p, 1, v->cus);
            // 1. the probe: the coarse index's own certified search, into the search's buffer
            if ((rc = ivf_probe_slice(v, qs, q_dtype, ns, p, q_dev, ss.ps, ss.pi, st))) return rc;
            // 2. the queries, staged as the flat index stages them for its storage
            if ((rc = ss.qbuf.ensure((size_t)ns * ix->ld * ix->qsize))) return rc;
            if (f32x) {
                if ((rc = ss.qf32.ensure((size_t)ns * ix->plane * sizeof(float)))) return rc;
                rc = convert_into(ix, qs, ns, q_dtype, q_dev, (uint8_t*)ss.qbuf.p, st, (float*)ss.qf32.p);
            } else {
                if (ix->sq8 && (rc = ss.qbias.ensure((size_t)ns * sizeof(double)))) return rc;
                rc = convert_into(ix, qs, ns, q_dtype, q_dev, (uint8_t*)ss.qbuf.p, st, nullptr, 0, nullptr, 0, ix->qsize, (double*)ss.qbias.p);
            }
            if (rc) return rc;
            // 3. the range scan: one workgroup per (query, probed list, segment); an empty staging buffer, no hits yet
            HIP_TRY(hipMemsetAsync(words, 0, 8, st));
            HIP_TRY(hipMemsetAsync(qcnt, 0, (size_t)2 * slice * sizeof(int), st));
            mips::IvfRangeArgs ra;
            mips::IvfScanArgs& a = ra.a;
            a.rows = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
            a.y = f32x ? ss.qf32.p : ss.qbuf.p;
            a.ld = ld;
            a.ntotal = ix->ntotal;
            a.probe = (const int64_t*)ss.pi.p;
            a.offsets = v->offsets;
            a.list_rows = v->list_rows;
            a.nlist = v->nlist;
            a.nq = ns;
            a.p = p;
            a.S = S;
            a.k = 0;
            a.parts = nullptr;
            a.sel_bits = d_bits;
            a.sel_bit0 = d_bit0;
            a.row_labels = ix->labels;
            a.q_labels = d_qlab ? d_qlab + s0 : nullptr;
            a.grp_mode = sel.grp_only ? MIPS_GRP_ONLY : MIPS_GRP_EXCLUDE;
            ra.radii = d_radii + s0;
            ra.bias = ix->sq8 ? (const double*)ss.qbias.p : nullptr;
            ra.cursor = words;
            ra.qcnt = qcnt;
            ra.cap = cap;
            ra.stage_q = stage_q;
            ra.stage_r = stage_r;
            ra.stage_s = stage_s;
            const unsigned grid = (unsigned)(ns * p * S); // <= 4096 * 1024, or < 2 * cus * 32
            constexpr int threads = 64 * mips::IVF_SCAN_WAVES;
            if (filtered) {
                if (f32x) mips::ivf_range_scan_kernel<mips::ElemF32, mips::ElemF32, true><<<grid, threads, 0, st>>>(ra);
                else if (ix->sq8) mips::ivf_range_scan_kernel<mips::ElemU8, mips::ElemBF16, true><<<grid, threads, 0, st>>>(ra);
                else mips::ivf_range_scan_kernel<mips::ElemBF16, mips::ElemBF16, true><<<grid, threads, 0, st>>>(ra);
            } else if (f32x) mips::ivf_range_scan_kernel<mips::ElemF32, mips::ElemF32, false><<<grid, threads, 0, st>>>(ra);
            else if (ix->sq8) mips::ivf_range_scan_kernel<mips::ElemU8, mips::ElemBF16, false><<<grid, threads, 0, st>>>(ra);
            else mips::ivf_range_scan_kernel<mips::ElemBF16, mips::ElemBF16, false><<<grid, threads, 0, st>>>(ra);
            HIP_TRY(hipGetLastError());
            // 4. the limits of the slice, continued from the slices before it
            mips::RangeLimsArgs la;
            la.qtot = qcnt;
            la.ns = (int)ns;
            la.s0 = s0;
            la.lims = d_lims;
            la.base = words + 1;
            mips::range_lims_kernel<<<1, mips::RANGE_LIMS_THREADS, 0, st>>>(la);
            HIP_TRY(hipGetLastError());
            if (cap == 0) continue; // a counting call
            // 5. place the staged records, 6. put every query's stretch into ascending row order and add idx_offset
            mips::IvfRangePlaceArgs pa;
            pa.cursor = words;
            pa.cap = cap;
            pa.stage_q = stage_q;
            pa.stage_r = stage_r;
            pa.stage_s = stage_s;
            pa.qcur = qcur;
            pa.ns = (int)ns;
            pa.s0 = s0;
            pa.lims = d_lims;
            pa.out_s = d_s;
            pa.out_i = d_i;
            mips::ivf_range_place_kernel<<<grid_for(cap, mips::IVF_RANGE_THREADS), mips::IVF_RANGE_THREADS, 0, st>>>(pa);
            mips::IvfRangeOrderArgs oa;
            oa.lims = d_lims;
            oa.ns = (int)ns;
            oa.s0 = s0;
            oa.cap = cap;
            oa.out_s = d_s;
            oa.out_i = d_i;
            oa.idx_offset = idx_offset;
            mips::ivf_range_order_kernel<<<(unsigned)ns, mips::IVF_RANGE_THREADS, 0, st>>>(oa);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_lims, d_lims, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (cap > 0) {
            HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)cap * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)cap * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

} // namespace

extern "C" {

int mips_ivf_range_search(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims, float* out_scores,
                          int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, void* hip_stream) {
    return ivf_range_impl("mips_ivf_range_search", v, q, q_dtype, nq, radii, nprobe, out_lims, out_scores, out_idx, cap, idx_offset, flags, nullptr, 0, 0, nullptr,
                          0, hip_stream);
}

int mips_ivf_range_search_grp(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims, float* out_scores,
                              int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0,
                              const int32_t* q_labels, int grp_mode, void* hip_stream) {
    return ivf_range_impl("mips_ivf_range_search_grp", v, q, q_dtype, nq, radii, nprobe, out_lims, out_scores, out_idx, cap, idx_offset, flags, sel_bits, sel_nbits,
                          sel_bit0, q_labels, grp_mode, hip_stream);
}

} // extern "C"
