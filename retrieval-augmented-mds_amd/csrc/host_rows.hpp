// Host side of include/mips_hip_rows.h (included by mips_hip.hip behind host_remove.hpp): check host ids before anything is
// enqueued, bring ids / queries to the device where they are host data, and enqueue the one launch of rows_kernels.hpp.  Every
// pointer into the index is read from the index object in the call itself: reserve, growth and removal move them.
#pragma once

namespace {

// Host ids: an id that names a row past the index is the caller's error (negative ids and ids below idx_offset mean "no row")
int rows_check_host_ids(const char* who, const mips_index* ix, const int64_t* ids, int64_t n, int64_t idx_offset) {
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id < 0 || id < idx_offset) continue;
        const uint64_t local = (uint64_t)id - (uint64_t)idx_offset; // the true difference: id >= idx_offset
        if (local >= (uint64_t)ix->ntotal)
            return fail(MIPS_E_INVALID, "%s: ids[%lld] = %lld names row %llu of an index of %lld", who, (long long)i, (long long)id,
                        (unsigned long long)local, (long long)ix->ntotal);
    }
    return MIPS_OK;
}

// ids on the device: the caller's pointer, or a copy of the host array (the call then synchronises: the array may go on return)
int rows_ids_on_device(mips_index* ix, const int64_t* ids, int64_t n, bool ids_dev, hipStream_t st, const int64_t*& d_ids) {
    d_ids = ids;
    if (ids_dev) return MIPS_OK;
    int rc = ix->row_ids.ensure((size_t)n * sizeof(int64_t));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->row_ids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    d_ids = (const int64_t*)ix->row_ids.p;
    return MIPS_OK;
}

inline int rows_grid(int64_t items, int per_block) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, 1 << 20)); }

int index_reconstruct(mips_index* ix, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld, int flags,
                      hipStream_t st) {
    const bool ids_dev = (flags & MIPS_IDS_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const bool f32x = ix->plane > 0;
    const bool raw = out_dtype != MIPS_DTYPE_F32; // (an fp32-exact index: the decoded values ARE the raw bits)
    const size_t osize = raw ? (size_t)ix->esize : 4;
    int rc;
    if (!ids_dev) {
        rc = rows_check_host_ids("mips_index_reconstruct", ix, ids, n, idx_offset);
        if (rc) return rc;
    }
    const int64_t* d_ids;
    rc = rows_ids_on_device(ix, ids, n, ids_dev, st, d_ids);
    if (rc) return rc;
    mips::RowsGatherArgs a;
    a.rows = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
    a.ld = f32x ? ix->plane : ix->ld;
    a.d = (int)ix->d;
    a.ntotal = ix->ntotal;
    a.ids = d_ids;
    a.n = n;
    a.idx_offset = idx_offset;
    a.out = out;
    a.out_ld = out_ld;
    a.fill = (flags & MIPS_ROWS_ZERO_MISSING) ? 0u : !raw ? 0x7fc00000u : ix->esize == 2 ? 0x7fc0u : ix->sq8 ? 0u : 0x7fu; // (SQ8 has no NaN code)
    if (!out_dev) { // compute into a packed device buffer; only columns 0 .. d - 1 of the caller's rows are written
        rc = ix->row_out.ensure((size_t)n * ix->d * osize);
        if (rc) return rc;
        a.out = ix->row_out.p;
        a.out_ld = ix->d;
    }
    const int grid = rows_grid(n, mips::ROWS_WAVES);
    if (f32x) mips::rows_gather_kernel<mips::ElemF32, false><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    else if (ix->esize == 2 && raw) mips::rows_gather_kernel<mips::ElemBF16, true><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    else if (ix->esize == 2) mips::rows_gather_kernel<mips::ElemBF16, false><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    else if (ix->sq8 && raw) mips::rows_gather_kernel<mips::ElemU8, true><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    else if (ix->sq8) { // the codes as float32, decoded in place behind the gather (rows of "no row" keep their fill)
        mips::rows_gather_kernel<mips::ElemU8, false><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
        if (ix->sq8_trained) // (an untrained index holds no row: every id is "no row" and keeps its fill)
            mips::sq8_decode_rows_kernel<<<grid_for(n * ix->d, 256), 256, 0, st>>>((float*)a.out, a.out_ld, d_ids, n, (int)ix->d, idx_offset, ix->ntotal,
                                                                            ix->sq8_params, ix->ld);
    } else if (raw) mips::rows_gather_kernel<mips::ElemF8, true><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    else mips::rows_gather_kernel<mips::ElemF8, false><<<grid, mips::ROWS_THREADS, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    if (!out_dev)
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_ld * osize, a.out, (size_t)ix->d * osize, (size_t)ix->d * osize, (size_t)n, hipMemcpyDeviceToHost, st));
    if (!out_dev || !ids_dev) HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int index_gather_labels(mips_index* ix, const int64_t* ids, int64_t n, int64_t idx_offset, int32_t* out, int flags, hipStream_t st) {
    const bool ids_dev = (flags & MIPS_IDS_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    int rc;
    if (!ids_dev) {
        rc = rows_check_host_ids("mips_index_gather_labels", ix, ids, n, idx_offset);
        if (rc) return rc;
    }
    const int64_t* d_ids;
    rc = rows_ids_on_device(ix, ids, n, ids_dev, st, d_ids);
    if (rc) return rc;
    int* d_out = out;
    if (!out_dev) {
        rc = ix->row_out.ensure((size_t)n * sizeof(int));
        if (rc) return rc;
        d_out = (int*)ix->row_out.p;
    }
    mips::rows_gather_labels_kernel<<<rows_grid(n, mips::ROWS_THREADS), mips::ROWS_THREADS, 0, st>>>(ix->labels, ix->nlabelled, ix->ntotal, d_ids, n,
                                                                                                  idx_offset, d_out, MIPS_LABEL_NONE);
    HIP_TRY(hipGetLastError());
    if (!out_dev) HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (!out_dev || !ids_dev) HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int index_score_subset(mips_index* ix, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores, int64_t idx_offset,
                       int flags, hipStream_t st) {
    const bool ids_dev = (flags & MIPS_IDS_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0, q_dev = (flags & MIPS_Q_DEVICE) != 0;
    const bool l2 = ix->metric == MIPS_METRIC_L2 && !(flags & MIPS_FORCE_IP);
    const bool f32x = ix->plane > 0;
    const int64_t npairs = nq * k;
    int rc;
    if (!ids_dev) {
        rc = rows_check_host_ids("mips_score_subset", ix, ids, npairs, idx_offset);
        if (rc) return rc;
    }
    // the staged queries of the current scratch set may still be read by the tail of a split-tail search
    rc = wait_for_tail(ix, st, /*both_sets=*/false);
    if (rc) return rc;
    if (l2 && ix->ntotal > 0) {
        rc = compute_phi(ix, st);
        if (rc) return rc;
    }
    // the queries, staged as mips_search stages them (no padding rows: one thread reads one query row)
    const size_t row_bytes = (size_t)ix->ld * ix->qsize;
    rc = ix->cur.qbuf.ensure((size_t)nq * row_bytes);
    if (rc) return rc;
    if (f32x) {
        rc = ix->cur.qf32.ensure((size_t)nq * ix->plane * sizeof(float));
        if (rc) return rc;
        rc = convert_into(ix, q, nq, q_dtype, q_dev, (uint8_t*)ix->cur.qbuf.p, st, (float*)ix->cur.qf32.p);
    } else {
        if (ix->sq8) {
            rc = ix->cur.qbias.ensure((size_t)nq * sizeof(double));
            if (rc) return rc;
        }
        rc = convert_into(ix, q, nq, q_dtype, q_dev, (uint8_t*)ix->cur.qbuf.p, st, nullptr, 0, nullptr, 0, ix->qsize, (double*)ix->cur.qbias.p);
    }
    if (rc) return rc;
    const int64_t* d_ids;
    rc = rows_ids_on_device(ix, ids, npairs, ids_dev, st, d_ids);
    if (rc) return rc;
    mips::RowsScoreArgs a;
    a.rows = f32x ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
    a.y = f32x ? ix->cur.qf32.p : ix->cur.qbuf.p;
    a.ld = f32x ? ix->plane : ix->ld;
    a.ntotal = ix->ntotal;
    a.ids = d_ids;
    a.npairs = npairs;
    a.k = k;
    a.idx_offset = idx_offset;
    a.phi = ix->phi;
    a.out = out_scores;
    if (!out_dev) {
        rc = ix->row_out.ensure((size_t)npairs * sizeof(float));
        if (rc) return rc;
        a.out = (float*)ix->row_out.p;
    }
    const int grid = rows_grid(npairs, mips::ROWS_THREADS);
    auto go = [&](auto kern) { kern<<<grid, mips::ROWS_THREADS, 0, st>>>(a); };
    if (f32x) l2 ? go(mips::rows_score_kernel<mips::ElemF32, true>) : go(mips::rows_score_kernel<mips::ElemF32, false>);
    else if (ix->sq8) { // S on the codes and q', then D = S + B_q as the searches report it
        go(mips::rows_score_kernel<mips::ElemU8, false, mips::ElemBF16>);
        mips::sq8_bias_kernel<<<grid_for(npairs, 256), 256, 0, st>>>(a.out, nullptr, (const double*)ix->cur.qbias.p, nq, k);
    } else if (ix->mixed) l2 ? go(mips::rows_score_kernel<mips::ElemF8, true, mips::ElemBF16>) : go(mips::rows_score_kernel<mips::ElemF8, false, mips::ElemBF16>);
    else if (ix->esize == 1) l2 ? go(mips::rows_score_kernel<mips::ElemF8, true>) : go(mips::rows_score_kernel<mips::ElemF8, false>);
    else l2 ? go(mips::rows_score_kernel<mips::ElemBF16, true>) : go(mips::rows_score_kernel<mips::ElemBF16, false>);
    HIP_TRY(hipGetLastError());
    if (!out_dev) HIP_TRY(hipMemcpyAsync(out_scores, a.out, (size_t)npairs * sizeof(float), hipMemcpyDeviceToHost, st));
    if (!out_dev || !ids_dev) HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

} // namespace
