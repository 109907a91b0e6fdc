// Host side of the IVF index (include/mips_hip_ivf.h; the kernels: ivf_kernels.hpp).  Included last by mips_hip.hip: the object owns
// two ordinary indexes -- `flat` holds the rows in arrival order, `coarse` (fp32-exact, inner product) holds the centroids and answers
// every "nearest lists of x" through mips_search / mips_search_wide -- plus the rows' list numbers and the list table.  Device
// resources are owned by type (DeviceArray, Buffer): `delete ivf` behind the two inner destroys leaves nothing.
// mips_ivf_search (at the end) is a fixed launch sequence -- probe, stage, list scan, merge, finish -- in which every grid, pointer,
// size and loop bound comes from (nq, p, k, d, nlist, the CU count) and the index object: nothing is read back from the device,
// and everything that depends on the queries is read and range-checked by the kernels (ivf_search_kernels.hpp).
#pragma once

// What a search over the probed lists writes between its launches.  Its own: `cs` / `ci` below are resized by add and training,
// these grow only when a search asks for a larger (nq, p, S, k) -- so a captured search stays valid across smaller ones.
struct IvfSearchScratch {
    Buffer ps, pi;            // the probe [ns][p]: scores, list numbers (int64)
    Buffer qbuf, qf32, qbias; // staged queries as the flat index stages them (+ B_q of an SQ8 index)
    Buffer parts;             // [p * S][ns][k][2] sorted partial lists
    Buffer out_s, out_i;      // [nq][k] of a host-output call, and the merged lists of a part search before they are packed
    Buffer packed;            // [nq][k][2] of a host-output part search (mips_ivf_search_part)
    Buffer sel, qlab;         // a host bitmap and host query labels of a filtered call (mips_ivf_search_sel / _grp)
};

// What a range search over the probed lists (host_ivf_range.hpp) writes between its launches, beside the probe and the staged
// queries above.  It grows only when a call asks for a larger (nq, cap).
struct IvfRangeScratch {
    Buffer words;             // [0] staging cursor of the slice, [1] hits of the slices before it
    Buffer counts;            // [2][ns] hits and placed records of every query of the slice
    Buffer radii;             // [nq] host radii
    Buffer stage;             // [cap] records: query, row, score
    Buffer lims, out_s, out_i; // [nq + 1], [cap], [cap] of a host-output call
};

struct mips_ivf {
    int device = 0;
    int64_t d = 0;
    int nlist = 0;
    int niter = 10;
    bool trained = false;
    mips_index* flat = nullptr;
    mips_index* coarse = nullptr;
    DeviceArray<float> cent;    // [nlist][d] the centroids as the coarse index holds them
    DeviceArray<int> assign;    // [assign_cap] list of every row
    int64_t assign_cap = 0;
    DeviceArray<int> offsets;   // [nlist + 1]
    DeviceArray<int> list_rows; // [rows_cap]
    int64_t rows_cap = 0;
    Buffer count;               // [nlist] histogram of a table build
    Buffer cs, ci;              // coarse results [nq][p]
    Buffer train_rows, train_assign, train_off, train_list, flag;
    Buffer upd_assign;          // mips_ivf_update: the list of every position's row [n]
    IvfSearchScratch ss;        // mips_ivf_search, and the device-output form of mips_ivf_probe
    IvfRangeScratch rs;         // mips_ivf_range_search
    int cus = 1;                // compute units of the device (sizes the list scan)
    ~mips_ivf() {
        if (flat) (void)mips_index_destroy(flat);
        if (coarse) (void)mips_index_destroy(coarse);
    }
};

namespace {

constexpr int64_t kIvfAssignChunk = 65536; // rows one coarse search assigns

// lists of n rows (float32 / bf16, host or device) -> out (device int32)
int ivf_assign_rows(mips_ivf* v, const void* x, int64_t n, int dtype, bool is_dev, int* out, hipStream_t st) {
    const size_t esz = dtype == MIPS_DTYPE_F32 ? 4 : 2;
    int rc = v->cs.ensure((size_t)std::min(n, kIvfAssignChunk) * sizeof(float));
    if (rc) return rc;
    rc = v->ci.ensure((size_t)std::min(n, kIvfAssignChunk) * sizeof(int64_t));
    if (rc) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += kIvfAssignChunk) {
        const int64_t nr = std::min(kIvfAssignChunk, n - r0);
        rc = mips_search(v->coarse, (const char*)x + (size_t)r0 * v->d * esz, dtype, nr, 1, (float*)v->cs.p, (int64_t*)v->ci.p, 0,
                         (is_dev ? MIPS_Q_DEVICE : 0) | MIPS_OUT_DEVICE, st);
        if (rc) return rc;
        mips::ivf_to_assign_kernel<<<grid_for(nr, 256), 256, 0, st>>>((const int64_t*)v->ci.p, nr, v->nlist, out + r0);
        HIP_TRY(hipGetLastError());
    }
    return MIPS_OK;
}

// offsets [nlist + 1], rows [n] from assign [n]
int ivf_build_table(mips_ivf* v, const int* assign, int64_t n, int* offsets, int* rows, hipStream_t st) {
    int rc = v->count.ensure((size_t)v->nlist * sizeof(int));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(v->count.p, 0, (size_t)v->nlist * sizeof(int), st));
    if (n > 0) mips::ivf_hist_kernel<<<grid_for(n, 256), 256, 0, st>>>(assign, n, v->nlist, (int*)v->count.p);
    mips::ivf_offsets_kernel<<<1, mips::IVF_SCAN_THREADS, 0, st>>>((const int*)v->count.p, v->nlist, offsets);
    if (n > 0) mips::ivf_list_fill_kernel<<<(v->nlist + 3) / 4, 256, 0, st>>>(assign, n, v->nlist, offsets, rows);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int ivf_rebuild(mips_ivf* v, hipStream_t st) {
    const int64_t n = v->flat->ntotal;
    if (v->rows_cap < n) {
        HIP_TRY(hipStreamSynchronize(st)); // (nothing in flight reads the table that goes)
        DeviceArray<int> fresh;
        const int64_t cap = round_up(std::max<int64_t>(n, v->rows_cap + v->rows_cap / 2), 256);
        hipError_t e = hipMalloc((void**)&fresh.p, (size_t)cap * sizeof(int));
        if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the list table failed: %s", (size_t)cap * sizeof(int), hipGetErrorString(e));
        std::swap(v->list_rows, fresh);
        v->rows_cap = cap;
    }
    return ivf_build_table(v, v->assign, n, v->offsets, v->list_rows, st);
}

int ivf_reserve_assign(mips_ivf* v, int64_t need, hipStream_t st) {
    if (need <= v->assign_cap) return MIPS_OK;
    const int64_t cap = round_up(std::max<int64_t>(need, v->assign_cap + v->assign_cap / 2), 256);
    DeviceArray<int> fresh;
    hipError_t e = hipMalloc((void**)&fresh.p, (size_t)cap * sizeof(int));
    if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the assignments failed: %s", (size_t)cap * sizeof(int), hipGetErrorString(e));
    const int64_t used = v->flat->ntotal;
    if (used > 0) HIP_TRY(hipMemcpyAsync(fresh, v->assign, (size_t)used * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the old storage is freed when this returns
    std::swap(v->assign, fresh);
    v->assign_cap = cap;
    return MIPS_OK;
}

// the centroids in v->cent -> the coarse index
int ivf_load_coarse(mips_ivf* v, hipStream_t st) {
    int rc = mips_index_reset(v->coarse);
    if (rc) return rc;
    return mips_index_add(v->coarse, v->cent, v->nlist, MIPS_DTYPE_F32, 1, st);
}

bool ivf_host_finite(const void* x, int64_t total, int dtype) {
    if (dtype == MIPS_DTYPE_F32) {
        const float* f = (const float*)x;
        for (int64_t t = 0; t < total; ++t)
            if (!std::isfinite(f[t])) return false;
    } else {
        const uint16_t* h = (const uint16_t*)x;
        for (int64_t t = 0; t < total; ++t)
            if ((h[t] & 0x7f80u) == 0x7f80u) return false;
    }
    return true;
}

int ivf_check(const char* who, const mips_ivf* v) {
    if (!v) return fail(MIPS_E_INVALID, "%s: the IVF index is NULL", who);
    return MIPS_OK;
}

// P(q) of a query slice: ci [ns][p] on the device (cs / ci: the index's coarse results, or the search's own probe buffers)
int ivf_probe_slice(mips_ivf* v, const void* q, int q_dtype, int64_t ns, int p, bool q_dev, Buffer& cs, Buffer& ci, hipStream_t st) {
    int rc = cs.ensure((size_t)ns * p * sizeof(float));
    if (rc) return rc;
    rc = ci.ensure((size_t)ns * p * sizeof(int64_t));
    if (rc) return rc;
    const int flags = (q_dev ? MIPS_Q_DEVICE : 0) | MIPS_OUT_DEVICE;
    if (p <= MIPS_MAX_K) return mips_search(v->coarse, q, q_dtype, ns, p, (float*)cs.p, (int64_t*)ci.p, 0, flags, st);
    return mips_search_wide(v->coarse, q, q_dtype, ns, p, (float*)cs.p, (int64_t*)ci.p, 0, flags, st);
}

int ivf_query_args(const char* who, const mips_ivf* v, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int* p) {
    if (!v->trained) return fail(MIPS_E_INVALID, "%s: the IVF index is not trained (mips_ivf_train / mips_ivf_set_centroids)", who);
    if (q_dtype != MIPS_DTYPE_F32 && q_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: q_dtype must be F32 or BF16", who);
    if (nq < 0 || (nq > 0 && !q)) return fail(MIPS_E_INVALID, "%s: bad q / nq", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    if (nprobe < 1) return fail(MIPS_E_INVALID, "%s: nprobe must be >= 1, got %lld", who, (long long)nprobe);
    const int64_t pp = std::min<int64_t>(nprobe, v->nlist);
    if (pp > mips::IVF_MAX_PROBE) return fail(MIPS_E_UNSUPPORTED, "%s: min(nprobe, nlist) = %lld exceeds %d", who, (long long)pp, mips::IVF_MAX_PROBE);
    *p = (int)pp;
    return MIPS_OK;
}

// launch 3 of a wide search (MIPS_MAX_K < k <= MIPS_MAX_K_WIDE): the instance whose pools hold KP >= k entries
template <int KP>
void ivf_launch_wide_scan(bool filtered, bool f32x, bool sq8, unsigned grid, hipStream_t st, const mips::IvfScanArgs& a) {
    constexpr int threads = 64 * mips::IVF_SCAN_WAVES;
    if (filtered) {
        if (f32x) mips::ivf_list_scan_wide_kernel<mips::ElemF32, mips::ElemF32, true, KP><<<grid, threads, 0, st>>>(a);
        else if (sq8) mips::ivf_list_scan_wide_kernel<mips::ElemU8, mips::ElemBF16, true, KP><<<grid, threads, 0, st>>>(a);
        else mips::ivf_list_scan_wide_kernel<mips::ElemBF16, mips::ElemBF16, true, KP><<<grid, threads, 0, st>>>(a);
    } else if (f32x) mips::ivf_list_scan_wide_kernel<mips::ElemF32, mips::ElemF32, false, KP><<<grid, threads, 0, st>>>(a);
    else if (sq8) mips::ivf_list_scan_wide_kernel<mips::ElemU8, mips::ElemBF16, false, KP><<<grid, threads, 0, st>>>(a);
    else mips::ivf_list_scan_wide_kernel<mips::ElemBF16, mips::ElemBF16, false, KP><<<grid, threads, 0, st>>>(a);
}

// What mips_ivf_search_part (host_ivf_sharded.hpp) takes in the place of out_scores / out_idx: the payload [nq][k][2] and, of an SQ8
// index, B_q [nq] -- host or device as the flags say.
struct IvfPartOut {
    int64_t* packed;
    double* bias;
};

// mips_ivf_search (sel_bits == nullptr and q_labels == nullptr: the unfiltered launch sequence, nothing else is touched) and
// mips_ivf_search_sel / _grp: the same sequence with the filtered instance of the list scan.  wide (mips_ivf_search_wide / _grp):
// k up to MIPS_MAX_K_WIDE; the same sequence again, with the wide list scan as launch 3 when k > MIPS_MAX_K.  part (wide only): the
// search cut behind its merge -- ivf_part_pack_kernel in the place of ivf_finish_kernel, B_q handed to the caller, nothing kept
int ivf_search_impl(const char* who, bool wide, mips_ivf* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                    int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode,
                    void* hip_stream, const IvfPartOut* part = nullptr) {
    int rc = ivf_check(who, v);
    if (rc) return rc;
    if (mips_ivf_is_trained(v) != 1) return fail(MIPS_E_INVALID, "%s: the IVF index is not trained (mips_ivf_train / mips_ivf_set_centroids)", who);
    int p = 0;
    if ((rc = ivf_query_args(who, v, q, q_dtype, nq, nprobe, &p))) return rc;
    if (wide) {
        if (k < 1) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K_WIDE, k);
        if (flags & MIPS_OUT_PACKED) return fail(MIPS_E_INVALID, "%s: MIPS_OUT_PACKED is not served on an IVF index", who);
        if (k > MIPS_MAX_K_WIDE) return fail(MIPS_E_UNSUPPORTED, "%s: k = %d exceeds MIPS_MAX_K_WIDE = %d", who, k, MIPS_MAX_K_WIDE);
        if ((int64_t)p * k > ivf::kMergeLimit)
            return fail(MIPS_E_UNSUPPORTED, "%s: min(nprobe, nlist) * k = %d * %d exceeds %lld, the entries per query the merge of the partial lists takes", who,
                        p, k, (long long)ivf::kMergeLimit);
    } else if (k < 1 || k > MIPS_MAX_K) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K, k);
    mips_index* ix = v->flat;
    const bool filtered = sel_bits != nullptr || q_labels != nullptr;
    Selector sel;
    if (filtered && (rc = make_selector(who, ix, flags, sel_bits, sel_nbits, sel_bit0, q_labels, grp_mode, sel))) return rc;
    if (nq == 0) return MIPS_OK;
    if (part ? !part->packed || (ix->sq8 && !part->bias) : !out_scores || !out_idx) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const bool f32x = ix->plane > 0;
    const int ld = f32x ? ix->plane : ix->ld; // elements per canonical row and per staged query
    const int per16 = f32x ? 4 : ix->esize == 2 ? 8 : 16;
    if (ld > mips::IVF_SCAN_MAX_LD || ld % (per16 * mips::IVF_SCAN_TCH) != 0)
        return fail(MIPS_E_UNSUPPORTED, "%s: row pitch %d is not served", who, ld);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st); // (the staging below is the flat index's; the coarse index orders its own calls)
    IvfSearchScratch& ss = v->ss;
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    if (!out_dev || part) {
        if ((rc = ss.out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
        if ((rc = ss.out_i.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
        d_s = (float*)ss.out_s.p;
        d_i = (int64_t*)ss.out_i.p;
    }
    // a part search: the payload and B_q of ALL the queries go to the caller's device buffers, or to scratch on their way to the host
    int64_t* d_pk = nullptr;
    double* d_b = nullptr;
    if (part) {
        d_pk = part->packed;
        d_b = part->bias;
        if (!out_dev) {
            if ((rc = ss.packed.ensure((size_t)ivf::packed_words(nq, k) * sizeof(int64_t)))) return rc;
            d_pk = (int64_t*)ss.packed.p;
            if (ix->sq8 && (rc = ss.qbias.ensure((size_t)nq * sizeof(double)))) return rc;
            d_b = (double*)ss.qbias.p;
        }
    }
    // a host bitmap (the bytes that hold bits sel_bit0 .. sel_bit0 + ntotal - 1) and host query labels travel by the stream's
    // asynchronous copy into the search's scratch; device ones are read where they are
    const uint8_t* d_bits = sel_bits;
    int64_t d_bit0 = sel_bit0;
    const int* d_qlab = (const int*)q_labels;
    if (sel_bits && !sel.dev && ix->ntotal > 0) {
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
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    const int64_t slice = ivf::slice_queries(p, k);
    for (int64_t s0 = 0; s0 < nq; s0 += slice) {
        const int64_t ns = std::min(slice, nq - s0);
        const void* qs = (const char*)q + (size_t)s0 * v->d * esz;
        const int S = ivf::choose_segments(ns, p, k, v->cus);
        // 1. the probe: the coarse index's own certified search, into the search's buffer
        if ((rc = ivf_probe_slice(v, qs, q_dtype, ns, p, q_dev, ss.ps, ss.pi, st))) return rc;
        // 2. the queries, staged as the flat index stages them for its storage
        if ((rc = ss.qbuf.ensure((size_t)ns * ix->ld * ix->qsize))) return rc;
        if (f32x) {
            if ((rc = ss.qf32.ensure((size_t)ns * ix->plane * sizeof(float)))) return rc;
            rc = convert_into(ix, qs, ns, q_dtype, q_dev, (uint8_t*)ss.qbuf.p, st, (float*)ss.qf32.p);
        } else {
            if (ix->sq8 && !part && (rc = ss.qbias.ensure((size_t)ns * sizeof(double)))) return rc;
            rc = convert_into(ix, qs, ns, q_dtype, q_dev, (uint8_t*)ss.qbuf.p, st, nullptr, 0, nullptr, 0, ix->qsize,
                              part ? (d_b ? d_b + s0 : nullptr) : (double*)ss.qbias.p);
        }
        if (rc) return rc;
        // 3. the list scan: one workgroup per (query, probed list, segment)
        const int parts = p * S;
        if ((rc = ss.parts.ensure((size_t)parts * ns * k * 2 * sizeof(int64_t)))) return rc;
        mips::IvfScanArgs a;
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
        a.k = k;
        a.parts = (int64_t*)ss.parts.p;
        a.sel_bits = d_bits;
        a.sel_bit0 = d_bit0;
        a.row_labels = ix->labels;
        a.q_labels = d_qlab ? d_qlab + s0 : nullptr;
        a.grp_mode = sel.grp_only ? MIPS_GRP_ONLY : MIPS_GRP_EXCLUDE;
        const unsigned grid = (unsigned)(ns * parts); // <= 4096 * 1024, or < 2 * cus * 32
        constexpr int threads = 64 * mips::IVF_SCAN_WAVES;
        if (k > MIPS_MAX_K) { // (wide only) the pool class of k: ivf::pool_class
            const int kp = ivf::pool_class(k);
            if (kp == 64) ivf_launch_wide_scan<64>(filtered, f32x, ix->sq8, grid, st, a);
            else if (kp == 256) ivf_launch_wide_scan<256>(filtered, f32x, ix->sq8, grid, st, a);
            else ivf_launch_wide_scan<1024>(filtered, f32x, ix->sq8, grid, st, a);
        } else if (filtered) {
            if (f32x) mips::ivf_list_scan_kernel<mips::ElemF32, mips::ElemF32, true><<<grid, threads, 0, st>>>(a);
            else if (ix->sq8) mips::ivf_list_scan_kernel<mips::ElemU8, mips::ElemBF16, true><<<grid, threads, 0, st>>>(a);
            else mips::ivf_list_scan_kernel<mips::ElemBF16, mips::ElemBF16, true><<<grid, threads, 0, st>>>(a);
        } else if (f32x) mips::ivf_list_scan_kernel<mips::ElemF32, mips::ElemF32><<<grid, threads, 0, st>>>(a);
        else if (ix->sq8) mips::ivf_list_scan_kernel<mips::ElemU8, mips::ElemBF16><<<grid, threads, 0, st>>>(a);
        else mips::ivf_list_scan_kernel<mips::ElemBF16, mips::ElemBF16><<<grid, threads, 0, st>>>(a);
        HIP_TRY(hipGetLastError());
        // 4. the merge of the sorted partials (score descending, row ascending, padding last), then S -> D and idx_offset -- or, of a
        //    part search, the payload: the ranking score as it is, idx_offset added
        if ((rc = mips_merge_topk_sorted_packed(a.parts, ns, parts, k, MIPS_METRIC_IP, d_s + (size_t)s0 * k, d_i + (size_t)s0 * k, v->device, st))) return rc;
        if (part)
            mips::ivf_part_pack_kernel<<<grid_for(ns * k, 256), 256, 0, st>>>(d_s + (size_t)s0 * k, d_i + (size_t)s0 * k, ns, k, idx_offset,
                                                                             d_pk + ivf::packed_words(s0, k));
        else
            mips::ivf_finish_kernel<<<grid_for(ns * k, 256), 256, 0, st>>>(d_s + (size_t)s0 * k, d_i + (size_t)s0 * k, ix->sq8 ? (const double*)ss.qbias.p : nullptr, ns,
                                                                          k, idx_offset);
        HIP_TRY(hipGetLastError());
    }
    if (part) {
        if (!out_dev) {
            HIP_TRY(hipMemcpyAsync(part->packed, d_pk, (size_t)ivf::packed_words(nq, k) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (ix->sq8) HIP_TRY(hipMemcpyAsync(part->bias, d_b, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return MIPS_OK;
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

} // namespace

extern "C" {

int mips_ivf_create(mips_ivf_t** out, int device, int64_t d, int doc_dtype, int metric, int64_t nlist) {
    if (!out) return fail(MIPS_E_INVALID, "mips_ivf_create: out is NULL");
    *out = nullptr;
    if (metric == MIPS_METRIC_L2)
        return fail(MIPS_E_UNSUPPORTED, "mips_ivf_create: an IVF index ranks by inner product only (the index's L2 is the MIPS->L2 reduction, whose "
                                        "constant is not a property of a list)");
    if (metric != MIPS_METRIC_IP) return fail(MIPS_E_INVALID, "mips_ivf_create: metric must be 0 (inner product), got %d", metric);
    if (doc_dtype == MIPS_DTYPE_FP8_E4M3 || doc_dtype == MIPS_DTYPE_FP8_E4M3_DOCS)
        return fail(MIPS_E_UNSUPPORTED, "mips_ivf_create: the e4m3 storages are not served (BF16, F32 or SQ8)");
    if (doc_dtype != MIPS_DTYPE_BF16 && doc_dtype != MIPS_DTYPE_F32 && doc_dtype != MIPS_DTYPE_SQ8)
        return fail(MIPS_E_INVALID, "mips_ivf_create: storage dtype must be BF16, F32 or SQ8, got %d", doc_dtype);
    if (d <= 0) return fail(MIPS_E_INVALID, "mips_ivf_create: bad dimension %lld", (long long)d);
    if (d > 1024) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_create: rows of more than 1024 columns are not served");
    if (nlist < 1 || nlist > 65536) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_create: nlist must be 1 .. 65536, got %lld", (long long)nlist);
    std::unique_ptr<mips_ivf> v(new (std::nothrow) mips_ivf());
    if (!v) return fail(MIPS_E_NOMEM, "out of host memory");
    v->device = device;
    v->d = d;
    v->nlist = (int)nlist;
    int rc = mips_index_create(&v->flat, device, d, doc_dtype, MIPS_METRIC_IP);
    if (rc) return rc;
    rc = mips_index_create(&v->coarse, device, d, MIPS_DTYPE_F32, MIPS_METRIC_IP);
    if (rc) return rc;
    DeviceGuard g(device);
    HIP_TRY(hipDeviceGetAttribute(&v->cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipMalloc((void**)&v->cent.p, (size_t)nlist * d * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&v->offsets.p, (size_t)(nlist + 1) * sizeof(int)));
    HIP_TRY(hipMemset(v->offsets.p, 0, (size_t)(nlist + 1) * sizeof(int)));
    *out = v.release();
    return MIPS_OK;
}

int mips_ivf_destroy(mips_ivf_t* v) {
    if (!v) return MIPS_OK;
    DeviceGuard g(v->device);
    (void)hipDeviceSynchronize();
    delete v;
    return MIPS_OK;
}

mips_index_t* mips_ivf_flat(mips_ivf_t* v) { return v ? v->flat : nullptr; }
int mips_ivf_is_trained(const mips_ivf_t* v) { return v ? (v->trained && (!v->flat->sq8 || v->flat->sq8_trained) ? 1 : 0) : -1; }
int64_t mips_ivf_nlist(const mips_ivf_t* v) { return v ? v->nlist : -1; }

int mips_ivf_set_param(mips_ivf_t* v, const char* name, int64_t value) {
    int rc = ivf_check("mips_ivf_set_param", v);
    if (rc) return rc;
    if (name && std::strcmp(name, "ivf_niter") == 0) {
        if (value < 0 || value > 1000) return fail(MIPS_E_INVALID, "mips_ivf_set_param: ivf_niter must be 0 .. 1000");
        v->niter = (int)value;
        return MIPS_OK;
    }
    return fail(MIPS_E_INVALID, "mips_ivf_set_param: unknown parameter '%s'", name ? name : "(null)");
}

int mips_ivf_train(mips_ivf_t* v, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream) {
    int rc = ivf_check("mips_ivf_train", v);
    if (rc) return rc;
    if (x_dtype != MIPS_DTYPE_F32 && x_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_ivf_train: x_dtype must be F32 or BF16");
    if (v->flat->ntotal > 0) return fail(MIPS_E_INVALID, "mips_ivf_train: the index holds %lld rows", (long long)v->flat->ntotal);
    if (!x || n < v->nlist) return fail(MIPS_E_INVALID, "mips_ivf_train: %lld training rows for %d lists", (long long)n, v->nlist);
    if (n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_train: more than 2^31 training rows");
    const bool is_dev = (flags & MIPS_Q_DEVICE) != 0;
    const int d = (int)v->d, nlist = v->nlist;
    const int64_t m = n > (int64_t)256 * nlist ? (int64_t)256 * nlist : n;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = v->train_rows.ensure((size_t)m * d * sizeof(float)))) return rc;
    if ((rc = v->train_assign.ensure((size_t)m * sizeof(int)))) return rc;
    if ((rc = v->train_off.ensure((size_t)(nlist + 1) * sizeof(int)))) return rc;
    if ((rc = v->train_list.ensure((size_t)m * sizeof(int)))) return rc;
    float* T = (float*)v->train_rows.p;
    if (is_dev) {
        if ((rc = v->flag.ensure(sizeof(int)))) return rc;
        HIP_TRY(hipMemsetAsync(v->flag.p, 0, sizeof(int), st));
        if (x_dtype == MIPS_DTYPE_F32) {
            mips::ivf_finite_kernel<float><<<grid_for(n * d, 256), 256, 0, st>>>((const float*)x, n * d, (int*)v->flag.p);
            mips::ivf_gather_rows_kernel<float><<<grid_for(m * d, 256), 256, 0, st>>>((const float*)x, n, m, d, T);
        } else {
            mips::ivf_finite_kernel<uint16_t><<<grid_for(n * d, 256), 256, 0, st>>>((const uint16_t*)x, n * d, (int*)v->flag.p);
            mips::ivf_gather_rows_kernel<uint16_t><<<grid_for(m * d, 256), 256, 0, st>>>((const uint16_t*)x, n, m, d, T);
        }
        HIP_TRY(hipGetLastError());
        int bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, v->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return fail(MIPS_E_INVALID, "mips_ivf_train: the training rows hold a NaN or an infinity");
    } else {
        if (!ivf_host_finite(x, n * d, x_dtype)) return fail(MIPS_E_INVALID, "mips_ivf_train: the training rows hold a NaN or an infinity");
        std::vector<float> h((size_t)m * d);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t r = ivf::pick(i, n, m);
            if (x_dtype == MIPS_DTYPE_F32) std::memcpy(&h[(size_t)i * d], (const float*)x + (size_t)r * d, (size_t)d * sizeof(float));
            else
                for (int j = 0; j < d; ++j) {
                    const uint32_t u = (uint32_t)((const uint16_t*)x)[(size_t)r * d + j] << 16;
                    std::memcpy(&h[(size_t)i * d + j], &u, 4);
                }
        }
        HIP_TRY(hipMemcpyAsync(T, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    v->trained = false;
    mips::ivf_init_centroids_kernel<<<(nlist + 255) / 256, 256, 0, st>>>(T, m, d, nlist, v->cent);
    HIP_TRY(hipGetLastError());
    if ((rc = ivf_load_coarse(v, st))) return rc;
    for (int it = 0; it < v->niter; ++it) {
        if ((rc = ivf_assign_rows(v, T, m, MIPS_DTYPE_F32, true, (int*)v->train_assign.p, st))) return rc;
        if ((rc = ivf_build_table(v, (const int*)v->train_assign.p, m, (int*)v->train_off.p, (int*)v->train_list.p, st))) return rc;
        mips::ivf_centroid_sum_kernel<<<grid_for((int64_t)nlist * d, 256), 256, 0, st>>>(T, d, (const int*)v->train_off.p, (const int*)v->train_list.p, nlist,
                                                                                        v->cent);
        mips::ivf_normalise_kernel<<<(nlist + 255) / 256, 256, 0, st>>>(v->cent, d, (const int*)v->train_off.p, nlist);
        HIP_TRY(hipGetLastError());
        if ((rc = ivf_load_coarse(v, st))) return rc;
    }
    if (v->flat->sq8 && (rc = mips_index_sq8_train(v->flat, x, n, x_dtype, is_dev ? MIPS_Q_DEVICE : 0, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    v->trained = true;
    return MIPS_OK;
}

int mips_ivf_set_centroids(mips_ivf_t* v, const float* c) {
    int rc = ivf_check("mips_ivf_set_centroids", v);
    if (rc) return rc;
    if (!c) return fail(MIPS_E_INVALID, "mips_ivf_set_centroids: NULL array");
    if (v->flat->ntotal > 0) return fail(MIPS_E_INVALID, "mips_ivf_set_centroids: the index holds %lld rows", (long long)v->flat->ntotal);
    if (!ivf_host_finite(c, (int64_t)v->nlist * v->d, MIPS_DTYPE_F32)) return fail(MIPS_E_INVALID, "mips_ivf_set_centroids: a NaN or an infinity");
    DeviceGuard g(v->device);
    HIP_TRY(hipMemcpyAsync(v->cent, c, (size_t)v->nlist * v->d * sizeof(float), hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = ivf_load_coarse(v, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    v->trained = true;
    return MIPS_OK;
}

int mips_ivf_get_centroids(mips_ivf_t* v, float* out) {
    int rc = ivf_check("mips_ivf_get_centroids", v);
    if (rc) return rc;
    if (!out) return fail(MIPS_E_INVALID, "mips_ivf_get_centroids: NULL array");
    if (!v->trained) return fail(MIPS_E_INVALID, "mips_ivf_get_centroids: the index is not trained");
    DeviceGuard g(v->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, v->cent, (size_t)v->nlist * v->d * sizeof(float), hipMemcpyDeviceToHost));
    return MIPS_OK;
}

int mips_ivf_add(mips_ivf_t* v, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream) {
    int rc = ivf_check("mips_ivf_add", v);
    if (rc) return rc;
    if (src_dtype == MIPS_DTYPE_SQ8 || src_dtype == MIPS_DTYPE_FP8_E4M3)
        return fail(MIPS_E_UNSUPPORTED, "mips_ivf_add: raw codes cannot be assigned to a list (float32 or bf16 rows)");
    if (src_dtype != MIPS_DTYPE_F32 && src_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_ivf_add: src_dtype must be F32 or BF16");
    if (n < 0 || (n > 0 && !rows)) return fail(MIPS_E_INVALID, "mips_ivf_add: bad rows / n");
    if (mips_ivf_is_trained(v) != 1) return fail(MIPS_E_INVALID, "mips_ivf_add: the IVF index is not trained (mips_ivf_train)");
    if (n == 0) return MIPS_OK;
    const int64_t n0 = v->flat->ntotal;
    if (n0 + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_add: more than 2^31 rows on one GPU");
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = ivf_reserve_assign(v, n0 + n, st))) return rc;
    if ((rc = ivf_assign_rows(v, rows, n, src_dtype, src_is_device != 0, v->assign + n0, st))) return rc;
    if ((rc = mips_index_add(v->flat, rows, n, src_dtype, src_is_device, st))) return rc;
    return ivf_rebuild(v, st);
}

int mips_ivf_reset(mips_ivf_t* v) {
    int rc = ivf_check("mips_ivf_reset", v);
    if (rc) return rc;
    DeviceGuard g(v->device);
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = mips_index_reset(v->flat))) return rc;
    HIP_TRY(hipMemset(v->offsets.p, 0, (size_t)(v->nlist + 1) * sizeof(int)));
    return MIPS_OK;
}

int mips_ivf_list_sizes(mips_ivf_t* v, int64_t* out, void* hip_stream) {
    int rc = ivf_check("mips_ivf_list_sizes", v);
    if (rc) return rc;
    if (!out) return fail(MIPS_E_INVALID, "mips_ivf_list_sizes: NULL array");
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int> h((size_t)v->nlist + 1);
    HIP_TRY(hipMemcpyAsync(h.data(), v->offsets, h.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int l = 0; l < v->nlist; ++l) out[l] = (int64_t)h[l + 1] - h[l];
    return MIPS_OK;
}

int mips_ivf_read_assign(mips_ivf_t* v, int64_t row0, int64_t n, int32_t* out, void* hip_stream) {
    int rc = ivf_check("mips_ivf_read_assign", v);
    if (rc) return rc;
    if (row0 < 0 || n < 0 || row0 + n > v->flat->ntotal || (n > 0 && !out))
        return fail(MIPS_E_INVALID, "mips_ivf_read_assign: bad range [%lld, +%lld) of %lld rows", (long long)row0, (long long)n, (long long)v->flat->ntotal);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemcpyAsync(out, v->assign + row0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int mips_ivf_set_assign(mips_ivf_t* v, const int32_t* assign, int64_t n, void* hip_stream) {
    int rc = ivf_check("mips_ivf_set_assign", v);
    if (rc) return rc;
    if (n != v->flat->ntotal || (n > 0 && !assign))
        return fail(MIPS_E_INVALID, "mips_ivf_set_assign: %lld assignments for %lld rows", (long long)n, (long long)v->flat->ntotal);
    for (int64_t i = 0; i < n; ++i)
        if (assign[i] < 0 || assign[i] >= v->nlist) return fail(MIPS_E_INVALID, "mips_ivf_set_assign: row %lld names list %d of %d", (long long)i, assign[i], v->nlist);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t keep = v->flat->ntotal;
    v->flat->ntotal = 0; // (nothing of the old assignments is carried over)
    rc = ivf_reserve_assign(v, n, st);
    v->flat->ntotal = keep;
    if (rc) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(v->assign, assign, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = ivf_rebuild(v, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int mips_ivf_remove(mips_ivf_t* v, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, int flags, int64_t out_counts[2], void* hip_stream) {
    int rc = ivf_check("mips_ivf_remove", v);
    if (rc) return rc;
    const int64_t n = v->flat->ntotal;
    if (!out_counts) return fail(MIPS_E_INVALID, "mips_ivf_remove: out_counts is NULL");
    if (sel_bit0 < 0 || sel_nbits < 0 || sel_bit0 > sel_nbits || n > sel_nbits - sel_bit0 || (!sel_bits && n > 0))
        return fail(MIPS_E_INVALID, "mips_ivf_remove: the bitmap's %lld bits from bit %lld on do not cover the index's %lld rows", (long long)sel_nbits,
                    (long long)sel_bit0, (long long)n);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    // the assignments follow their rows: the same order-preserving compaction, on the host (the call synchronises anyway)
    std::vector<uint8_t> bits((size_t)(sel_nbits + 7) / 8);
    std::vector<int> as((size_t)n);
    if (n > 0) {
        if (flags & MIPS_SEL_DEVICE) HIP_TRY(hipMemcpyAsync(bits.data(), sel_bits, bits.size(), hipMemcpyDeviceToHost, st));
        else std::memcpy(bits.data(), sel_bits, bits.size());
        HIP_TRY(hipMemcpyAsync(as.data(), v->assign, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if ((rc = mips_index_remove(v->flat, sel_bits, sel_nbits, sel_bit0, flags, out_counts, st))) return rc;
    int64_t w = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t b = sel_bit0 + i;
        if (!((bits[(size_t)(b >> 3)] >> (b & 7)) & 1)) as[(size_t)w++] = as[(size_t)i];
    }
    if (w != v->flat->ntotal) return fail(MIPS_E_HIP, "mips_ivf_remove: %lld assignments survive, %lld rows do", (long long)w, (long long)v->flat->ntotal);
    if (w > 0) HIP_TRY(hipMemcpyAsync(v->assign, as.data(), (size_t)w * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = ivf_rebuild(v, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

// include/mips_hip_write.h: the rows by id through the flat index, the list of every written row with them, the table again
int mips_ivf_update(mips_ivf_t* v, const int64_t* ids, int64_t n, int64_t idx_offset, const void* rows, int src_dtype, int flags, int64_t* out_updated,
                    void* hip_stream) {
    int rc = ivf_check("mips_ivf_update", v);
    if (rc) return rc;
    if (src_dtype == MIPS_DTYPE_SQ8 || src_dtype == MIPS_DTYPE_FP8_E4M3)
        return fail(MIPS_E_UNSUPPORTED, "mips_ivf_update: raw codes cannot be assigned to a list (float32 or bf16 rows)");
    if (src_dtype != MIPS_DTYPE_F32 && src_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_ivf_update: src_dtype must be F32 or BF16");
    if (n < 0 || (n > 0 && (!ids || !rows))) return fail(MIPS_E_INVALID, "mips_ivf_update: bad ids / rows / n");
    if (mips_ivf_is_trained(v) != 1) return fail(MIPS_E_INVALID, "mips_ivf_update: the IVF index is not trained (mips_ivf_train)");
    if (!upd::count_ok(n)) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_update: more than 2^31 - 1 positions in one call");
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    mips_index* ix = v->flat;
    if (n == 0 || ix->ntotal == 0) return mips_index_update(ix, ids, n, idx_offset, rows, src_dtype, flags, out_updated, st);
    if ((rc = v->upd_assign.ensure((size_t)n * sizeof(int)))) return rc;
    if ((rc = ivf_assign_rows(v, rows, n, src_dtype, (flags & MIPS_Q_DEVICE) != 0, (int*)v->upd_assign.p, st))) return rc;
    {
        ORDER_ON(ix, st);
        if ((rc = index_update(ix, ids, n, idx_offset, rows, src_dtype, flags, out_updated, st, (const int*)v->upd_assign.p, v->assign))) return rc;
    }
    return ivf_rebuild(v, st);
}

int mips_ivf_probe(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int32_t* out_lists, int flags, void* hip_stream) {
    int rc = ivf_check("mips_ivf_probe", v);
    if (rc) return rc;
    int p = 0;
    if ((rc = ivf_query_args("mips_ivf_probe", v, q, q_dtype, nq, nprobe, &p))) return rc;
    if (nq == 0) return MIPS_OK;
    if (!out_lists) return fail(MIPS_E_INVALID, "mips_ivf_probe: NULL buffer");
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    if (flags & MIPS_OUT_DEVICE) { // into the search's probe buffer, then int32 to the caller: stream operations only
        for (int64_t s0 = 0; s0 < nq; s0 += 4096) {
            const int64_t ns = std::min<int64_t>(4096, nq - s0);
            if ((rc = ivf_probe_slice(v, (const char*)q + (size_t)s0 * v->d * esz, q_dtype, ns, p, (flags & MIPS_Q_DEVICE) != 0, v->ss.ps, v->ss.pi, st)))
                return rc;
            mips::ivf_to_assign_kernel<<<grid_for(ns * p, 256), 256, 0, st>>>((const int64_t*)v->ss.pi.p, ns * p, v->nlist, out_lists + (size_t)s0 * p);
            HIP_TRY(hipGetLastError());
        }
        return MIPS_OK;
    }
    std::vector<int64_t> h;
    for (int64_t s0 = 0; s0 < nq; s0 += 4096) {
        const int64_t ns = std::min<int64_t>(4096, nq - s0);
        if ((rc = ivf_probe_slice(v, (const char*)q + (size_t)s0 * v->d * esz, q_dtype, ns, p, (flags & MIPS_Q_DEVICE) != 0, v->cs, v->ci, st))) return rc;
        h.resize((size_t)ns * p);
        HIP_TRY(hipMemcpyAsync(h.data(), v->ci.p, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t t = 0; t < h.size(); ++t) out_lists[(size_t)s0 * p + t] = (int32_t)h[t];
    }
    return MIPS_OK;
}

int mips_ivf_search(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx, int64_t idx_offset,
                    int flags, void* hip_stream) {
    return ivf_search_impl("mips_ivf_search", false, v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags, nullptr, 0, 0, nullptr, 0, hip_stream);
}

int mips_ivf_search_sel(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                        int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, void* hip_stream) {
    return ivf_search_impl("mips_ivf_search_sel", false, v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags, sel_bits, sel_nbits, sel_bit0, nullptr,
                           0, hip_stream);
}

int mips_ivf_search_grp(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                        int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode,
                        void* hip_stream) {
    return ivf_search_impl(q_labels ? "mips_ivf_search_grp" : "mips_ivf_search_sel", false, v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags,
                           sel_bits, sel_nbits, sel_bit0, q_labels, grp_mode, hip_stream);
}

int mips_ivf_search_wide(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                         int64_t idx_offset, int flags, void* hip_stream) {
    return ivf_search_impl("mips_ivf_search_wide", true, v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags, nullptr, 0, 0, nullptr, 0,
                           hip_stream);
}

int mips_ivf_search_wide_grp(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                             int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                             int grp_mode, void* hip_stream) {
    return ivf_search_impl("mips_ivf_search_wide_grp", true, v, q, q_dtype, nq, k, nprobe, out_scores, out_idx, idx_offset, flags, sel_bits, sel_nbits, sel_bit0,
                           q_labels, grp_mode, hip_stream);
}

} // extern "C"
