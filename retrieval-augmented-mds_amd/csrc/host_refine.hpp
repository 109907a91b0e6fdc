// Host side of the two-stage search on PQ codes (include/mips_hip_refine.h; the kernels: refine_kernels.hpp; the launch arithmetic:
// adc_wide_math.hpp).  Included last by mips_hip.hip: the candidate searches are the launch sequences of mips_pq_search /
// mips_ivfpq_search -- probe, tables, scan, merge, finish -- with the pool instance of the scan for k > MIPS_MAX_K (k <= MIPS_MAX_K: the
// narrow entry point itself), and the re-ranking is mips_score_subset into scratch behind which ONE select launch sits.  Every grid,
// block, LDS size, pointer and loop bound comes from (ns, k, kc, M, d, p, nlist, ntotal, the CU count) and the objects: nothing is read
// back from the device.
#pragma once

namespace {

template <typename Kern, typename Args>
int cand_launch_one(Kern kern, const Args& a, unsigned grid, int waves, int lds, hipStream_t st) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    kern<<<grid, 64 * waves, lds, st>>>(a);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int cand_launch_flat(const mips::PqScanArgs& a, unsigned grid, hipStream_t st) {
    const int KP = ivf::pool_class(a.k), waves = adcw::waves(a.M, KP, 0), lds = (int)adcw::lds_bytes(a.M, KP, 0);
    if (KP == 64) return cand_launch_one(mips::cand_flat_scan_kernel<64>, a, grid, waves, lds, st);
    if (KP == 256) return cand_launch_one(mips::cand_flat_scan_kernel<256>, a, grid, waves, lds, st);
    return cand_launch_one(mips::cand_flat_scan_kernel<1024>, a, grid, waves, lds, st);
}

int cand_launch_list(const mips::IvfAdcScanArgs& a, unsigned grid, hipStream_t st) {
    const int KP = ivf::pool_class(a.k), waves = adcw::waves(a.M, KP, a.p), lds = (int)adcw::lds_bytes(a.M, KP, a.p);
    if (KP == 64) return cand_launch_one(mips::cand_list_scan_kernel<64>, a, grid, waves, lds, st);
    if (KP == 256) return cand_launch_one(mips::cand_list_scan_kernel<256>, a, grid, waves, lds, st);
    return cand_launch_one(mips::cand_list_scan_kernel<1024>, a, grid, waves, lds, st);
}

} // namespace

extern "C" {

int mips_pq_search_candidates(mips_pq_t* p, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset,
                              int flags, void* hip_stream) {
    const char* who = "mips_pq_search_candidates";
    int rc = pq_check(who, p);
    if (rc) return rc;
    if (k >= 1 && k <= MIPS_MAX_K) return mips_pq_search(p, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, hip_stream);
    if ((rc = pq_query_args(who, p, q, q_dtype, nq))) return rc;
    if (k < 1 || k > MIPS_MAX_K_WIDE) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K_WIDE, k);
    if (nq == 0) return MIPS_OK;
    if (!out_scores || !out_idx) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    if (!out_dev) {
        if ((rc = p->out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
        if ((rc = p->out_i.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
        d_s = (float*)p->out_s.p;
        d_i = (int64_t*)p->out_i.p;
    }
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    for (int64_t s0 = 0; s0 < nq; s0 += p->query_slice) {
        const int64_t ns = std::min(p->query_slice, nq - s0);
        // 1. the tables
        const void* qs = nullptr;
        if ((rc = pq_stage_queries(p, (const char*)q + (size_t)s0 * p->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        if ((rc = pq_tables(p, qs, q_dtype, ns, st))) return rc;
        // 2. the scan: one workgroup per (query, row segment), one pool per wave
        const int S = adcw::choose_segments(ns, k, p->M, 0, p->ntotal, p->cus, 0);
        if ((rc = p->parts.ensure((size_t)S * ns * k * 2 * sizeof(int64_t)))) return rc;
        mips::PqScanArgs a;
        a.codes = p->codes;
        a.pitch = p->pitch;
        a.M = p->M;
        a.ntotal = p->ntotal;
        a.lut = (const float*)p->lut.p;
        a.ns = ns;
        a.S = S;
        a.k = k;
        a.parts = (int64_t*)p->parts.p;
        if ((rc = cand_launch_flat(a, (unsigned)(ns * S), st))) return rc; // grid <= 4096 * 65536 / k
        // 3. the merge of the sorted partials (score descending, row ascending, padding last), 4. idx_offset
        if ((rc = mips_merge_topk_sorted_packed(a.parts, ns, S, k, MIPS_METRIC_IP, d_s + (size_t)s0 * k, d_i + (size_t)s0 * k, p->device, st))) return rc;
        mips::pq_finish_kernel<<<grid_for(ns * k, 256), 256, 0, st>>>(d_i + (size_t)s0 * k, ns * k, idx_offset);
        HIP_TRY(hipGetLastError());
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

int mips_ivfpq_search_candidates(mips_ivfpq_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                                 int64_t idx_offset, int flags, void* hip_stream) {
    const char* who = "mips_ivfpq_search_candidates";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if (k >= 1 && k <= MIPS_MAX_K) return mips_ivfpq_search(v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags, hip_stream);
    if ((rc = ivfpq_query_args(who, v, q, q_dtype, nq))) return rc;
    int p = 0;
    if ((rc = ivfpq_probe_args(who, v, nprobe, &p))) return rc;
    if (k < 1 || k > MIPS_MAX_K_WIDE) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K_WIDE, k);
    if (nq == 0) return MIPS_OK;
    if (!out_scores || !out_idx) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    mips_pq* pqx = v->pq;
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    if (!out_dev) {
        if ((rc = v->out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
        if ((rc = v->out_i.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
        d_s = (float*)v->out_s.p;
        d_i = (int64_t*)v->out_i.p;
    }
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    for (int64_t s0 = 0; s0 < nq; s0 += v->query_slice) {
        const int64_t ns = std::min(v->query_slice, nq - s0);
        const void* qs = nullptr;
        if ((rc = ivfpq_stage_queries(v, (const char*)q + (size_t)s0 * v->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        // 1. the probe: list numbers and T, the coarse index's own certified search
        if ((rc = ivfpq_probe_slice(v, qs, q_dtype, ns, p, st))) return rc;
        // 2. the tables
        if ((rc = pq_tables(pqx, qs, q_dtype, ns, st))) return rc;
        // 3. the scan: one workgroup per (query, segment of the concatenation of its probed lists), one pool per wave
        const int S = adcw::choose_segments(ns, k, v->M, p, ivfpq::expected_rows(pqx->ntotal, p, v->nlist), v->cus, v->scan_segments);
        if ((rc = v->parts.ensure((size_t)S * ns * k * 2 * sizeof(int64_t)))) return rc;
        mips::IvfAdcScanArgs a;
        a.codes = pqx->codes;
        a.pitch = pqx->pitch;
        a.M = v->M;
        a.ntotal = pqx->ntotal;
        a.lut = (const float*)pqx->lut.p;
        a.probe = (const int64_t*)v->pi.p;
        a.coarse = (const float*)v->ps.p;
        a.offsets = v->offsets;
        a.list_rows = v->list_rows;
        a.nlist = v->nlist;
        a.p = p;
        a.by_residual = v->by_residual ? 1 : 0;
        a.ns = ns;
        a.S = S;
        a.k = k;
        a.parts = (int64_t*)v->parts.p;
        if ((rc = cand_launch_list(a, (unsigned)(ns * S), st))) return rc; // grid <= 4096 * 65536 / k
        // 4. the merge of the sorted partials (score descending, row ascending, padding last), 5. idx_offset
        if ((rc = mips_merge_topk_sorted_packed(a.parts, ns, S, k, MIPS_METRIC_IP, d_s + (size_t)s0 * k, d_i + (size_t)s0 * k, v->device, st))) return rc;
        mips::ivfadc_finish_kernel<<<grid_for(ns * k, 256), 256, 0, st>>>(d_i + (size_t)s0 * k, ns * k, idx_offset);
        HIP_TRY(hipGetLastError());
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

int mips_index_rerank(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int kc, int k, float* out_scores, int64_t* out_idx,
                      int64_t idx_offset, int flags, void* hip_stream) {
    const char* who = "mips_index_rerank";
    if (!ix) return fail(MIPS_E_INVALID, "%s: index is NULL", who);
    if (ix->metric != MIPS_METRIC_IP) return fail(MIPS_E_UNSUPPORTED, "%s: an inner-product index only (the order is score descending)", who);
    if (nq < 0) return fail(MIPS_E_INVALID, "%s: negative nq", who);
    if (kc < 1 || kc > adcw::kRerankMax || k < 1 || k > kc) return fail(MIPS_E_INVALID, "%s: 1 <= k <= kc <= %d, got k = %d, kc = %d", who, adcw::kRerankMax, k, kc);
    if (nq == 0) return MIPS_OK;
    if (!q || !ids || !out_scores || !out_idx) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0, ids_dev = (flags & MIPS_IDS_DEVICE) != 0;
    const hipStream_t st = (hipStream_t)hip_stream;
    const int64_t npairs = nq * kc;
    const int64_t* d_ids = ids;
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    int rc;
    {
        DeviceGuard g(ix->device);
        if ((rc = ix->rr_scores.ensure((size_t)npairs * sizeof(float)))) return rc;
        if (!ids_dev) { // any id may come in: what names no row is dropped here, not refused
            if ((rc = ix->rr_ids.ensure((size_t)npairs * sizeof(int64_t)))) return rc;
            HIP_TRY(hipMemcpyAsync(ix->rr_ids.p, ids, (size_t)npairs * sizeof(int64_t), hipMemcpyHostToDevice, st));
            d_ids = (const int64_t*)ix->rr_ids.p;
        }
        if (!out_dev) {
            if ((rc = ix->rr_out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
            if ((rc = ix->rr_out_i.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
            d_s = (float*)ix->rr_out_s.p;
            d_i = (int64_t*)ix->rr_out_i.p;
        }
    }
    // 1. the scores, stated once: mips_score_subset on the device ids into scratch
    const int sflags = (q_dev ? MIPS_Q_DEVICE : 0) | MIPS_IDS_DEVICE | MIPS_OUT_DEVICE;
    if ((rc = mips_score_subset(ix, q, q_dtype, nq, d_ids, kc, (float*)ix->rr_scores.p, idx_offset, sflags, hip_stream))) return rc;
    // 2. the select: one workgroup per query
    DeviceGuard g(ix->device);
    mips::RerankArgs a;
    a.scores = (const float*)ix->rr_scores.p;
    a.ids = d_ids;
    a.kc = kc;
    a.k = k;
    a.ntotal = ix->ntotal;
    a.idx_offset = idx_offset;
    a.out_s = d_s;
    a.out_i = d_i;
    mips::rerank_select_kernel<<<(unsigned)nq, mips::RERANK_THREADS, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (!out_dev || !ids_dev || !q_dev) HIP_TRY(hipStreamSynchronize(st)); // (the caller's host buffers are free again)
    return MIPS_OK;
}

} // extern "C"
