// Host side of mips_index_update (include/mips_hip_write.h; included by mips_hip.hip behind host_rows.hpp): bring host ids / rows
// to the device, enqueue the three launches of update_kernels.hpp and keep the cached scalars of the index true (DESIGN.md section
// 4b).  With device ids, device rows and a device or NULL count nothing here waits for the device once the owner array exists, and
// nothing enqueued depends on the value of an id.
#pragma once

namespace {

// one int32 per row of capacity, -1.  The array that goes held -1 everywhere (every call puts back what it touched), so nothing
// is carried over; hipFree waits for what may still read it.
int update_ensure_owner(mips_index* ix, hipStream_t st) {
    if (ix->upd_owner_cap >= ix->capacity && ix->upd_owner) return MIPS_OK;
    DeviceArray<int> fresh;
    const size_t bytes = (size_t)ix->capacity * sizeof(int);
    hipError_t e = hipMalloc((void**)&fresh.p, bytes);
    if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the update owners failed: %s", bytes, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(fresh, 0xff, bytes, st));
    std::swap(ix->upd_owner, fresh);
    ix->upd_owner_cap = ix->capacity;
    return MIPS_OK;
}

template <int STORE>
int update_launch_scatter(const mips::UpdateArgs& a, int src_dtype, int grid, hipStream_t st) {
    if (src_dtype == MIPS_DTYPE_F32) mips::update_scatter_kernel<float, STORE><<<grid, mips::UPD_THREADS, 0, st>>>(a);
    else if (src_dtype == MIPS_DTYPE_BF16) mips::update_scatter_kernel<uint16_t, STORE><<<grid, mips::UPD_THREADS, 0, st>>>(a);
    else if constexpr (STORE == mips::UPD_F8 || STORE == mips::UPD_SQ8) mips::update_scatter_kernel<uint8_t, STORE><<<grid, mips::UPD_THREADS, 0, st>>>(a);
    else return fail(MIPS_E_INVALID, "mips_index_update: one-byte rows go into one-byte storage only");
    return MIPS_OK;
}

// aux_src [n] / aux_dst [>= ntotal]: an int32 per position that the row's winner hands to its row (mips_ivf_update: the list)
int index_update(mips_index* ix, const int64_t* ids, int64_t n, int64_t idx_offset, const void* rows, int src_dtype, int flags,
                 int64_t* out_updated, hipStream_t st, const int* aux_src = nullptr, int* aux_dst = nullptr) {
    const bool ids_dev = (flags & MIPS_IDS_DEVICE) != 0, rows_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    if (n == 0 || ix->ntotal == 0) { // no position names a row: nothing of the index is touched
        if (out_updated && out_dev) HIP_TRY(hipMemsetAsync(out_updated, 0, sizeof(int64_t), st));
        else if (out_updated) *out_updated = 0;
        return MIPS_OK;
    }
    // a split-tail search may still re-score on the rows from its tail stream
    int rc = wait_for_tail(ix, st, /*both_sets=*/true);
    if (rc) return rc;
    if ((rc = update_ensure_owner(ix, st))) return rc;
    const int64_t* d_ids;
    if ((rc = rows_ids_on_device(ix, ids, n, ids_dev, st, d_ids))) return rc;
    const void* d_rows = rows;
    if (!rows_dev) {
        const size_t bytes = (size_t)n * ix->d * (src_dtype == MIPS_DTYPE_F32 ? 4 : src_dtype == MIPS_DTYPE_BF16 ? 2 : 1);
        if ((rc = ix->stage.ensure(bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(ix->stage.p, rows, bytes, hipMemcpyHostToDevice, st));
        d_rows = ix->stage.p;
    }
    // the count: straight into the caller's device word; a host count of host ids is the host restatement (update_math.hpp),
    // a host count of device ids is read back
    const bool count_host_ids = out_updated && !out_dev && !ids_dev, count_readback = out_updated && !out_dev && ids_dev;
    unsigned long long* d_count = out_updated && out_dev ? (unsigned long long*)out_updated : nullptr;
    if (count_readback) {
        if ((rc = ix->upd_count.ensure(8))) return rc;
        d_count = (unsigned long long*)ix->upd_count.p;
    }
    if (d_count) HIP_TRY(hipMemsetAsync(d_count, 0, 8, st));

    mips::UpdateArgs a;
    a.ids = d_ids;
    a.n = (int)n;
    a.idx_offset = idx_offset;
    a.ntotal = ix->ntotal;
    a.owner = ix->upd_owner;
    a.src = d_rows;
    a.d = (int)ix->d;
    a.rows = ix->rows;
    a.ld = ix->ld;
    a.rows_f32 = ix->rows_f32;
    a.plane = ix->plane;
    a.rows_hi = (uint16_t*)ix->rows_hi.p;
    a.hp = ix->hp;
    a.hi_rows = ix->rows_hi ? ix->hi_rows : 0;
    a.sq8_params = ix->sq8_params;
    mips::update_mark_kernel<<<rows_grid(n, mips::UPD_THREADS), mips::UPD_THREADS, 0, st>>>(d_ids, a.n, idx_offset, a.ntotal, a.owner);
    HIP_TRY(hipGetLastError());
    const int grid = rows_grid(n, mips::UPD_WAVES);
    if (ix->plane > 0) rc = update_launch_scatter<mips::UPD_F32X>(a, src_dtype, grid, st);
    else if (ix->esize == 2) rc = update_launch_scatter<mips::UPD_BF16>(a, src_dtype, grid, st);
    else if (ix->sq8) rc = update_launch_scatter<mips::UPD_SQ8>(a, src_dtype, grid, st);
    else rc = update_launch_scatter<mips::UPD_F8>(a, src_dtype, grid, st);
    if (rc) return rc; // (unreachable behind src_dtype_ok: the entry points check the type before anything is enqueued)
    HIP_TRY(hipGetLastError());

    // The cached scalars.  The row-norm bounds stay UPPER bounds without a pass over the index: the written rows are folded in
    // (a bound too large flags more queries, which every path settles exactly; one too small would certify wrong answers).  phi is
    // part of the reported L2 distances and must be exact: it is recomputed when next needed, unless it was set from outside.
    mips::UpdateFinishArgs f;
    f.ids = d_ids;
    f.n = a.n;
    f.idx_offset = idx_offset;
    f.ntotal = a.ntotal;
    f.owner = a.owner;
    f.canon = ix->plane > 0 ? (const void*)ix->rows_f32.p : (const void*)ix->rows.p;
    f.cld = ix->plane > 0 ? ix->plane : ix->ld;
    f.xmax2 = ix->xmax2_valid ? (unsigned long long*)ix->xmax2_dev.p : nullptr;
    f.rows_f32 = ix->rows_f32;
    f.plane = ix->plane;
    f.dres2 = ix->plane > 0 && ix->dres2_valid ? (unsigned long long*)ix->dres2_dev.p : nullptr;
    f.count = d_count;
    f.aux_src = aux_src;
    f.aux_dst = aux_dst;
    const int fgrid = rows_grid(n, mips::UPD_THREADS);
    if (ix->plane > 0) mips::update_finish_kernel<mips::ElemF32><<<fgrid, mips::UPD_THREADS, 0, st>>>(f);
    else if (ix->esize == 2) mips::update_finish_kernel<mips::ElemBF16><<<fgrid, mips::UPD_THREADS, 0, st>>>(f);
    else if (ix->sq8) mips::update_finish_kernel<mips::ElemU8><<<fgrid, mips::UPD_THREADS, 0, st>>>(f);
    else mips::update_finish_kernel<mips::ElemF8><<<fgrid, mips::UPD_THREADS, 0, st>>>(f);
    HIP_TRY(hipGetLastError());
    if (!ix->phi_override) ix->phi_valid = false;

    unsigned long long counted = 0;
    if (count_readback) HIP_TRY(hipMemcpyAsync(&counted, d_count, 8, hipMemcpyDeviceToHost, st));
    if (!ids_dev || !rows_dev || count_readback) HIP_TRY(hipStreamSynchronize(st)); // the one synchronisation of a call with host data
    if (count_readback) *out_updated = (int64_t)counted;
    if (count_host_ids) *out_updated = upd::host_winners(ids, n, idx_offset, ix->ntotal);
    return MIPS_OK;
}

} // namespace
