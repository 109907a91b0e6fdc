// Host side of the IVF index over PQ codes (include/mips_hip_ivfpq.h; the kernels: ivfpq_kernels.hpp; the arithmetic:
// ivfpq_math.hpp).  Included by mips_hip.hip behind host_ivf.hpp and host_pq.hpp, whose entry points it calls as they are: the
// object owns `coarse` (an fp32-exact inner-product mips_index over the centroids, which answers every "nearest lists of x" through
// mips_search / mips_search_wide), `pq` (a mips_pq: codebook, codes and table scratch; rows are trained on and encoded through
// mips_pq_train / mips_pq_add on device residual buffers), the rows' list numbers, the list table (the IVF index's table kernels)
// and its own search scratch.  The centroids come from mips_ivf_train on a temporary empty mips_ivf: k-means is stated once.
// mips_ivfpq_search is a fixed launch sequence -- probe, tables, scan, merge, finish -- in which every grid, block, LDS size, pointer
// and loop bound comes from (ns, k, M, d, p, nlist, ntotal, the CU count) and the object: nothing is read back from the device.
#pragma once

struct mips_ivfpq {
    int device = 0;
    int d = 0, nlist = 0, M = 0;
    bool by_residual = true;
    int ivf_niter = 10;
    int64_t query_slice = 256; // queries one pass of a search serves
    int64_t scan_segments = 0; // 0: chosen by ivfpq::choose_segments
    bool have_cent = false;
    int cus = 1;
    mips_index* coarse = nullptr;
    mips_pq* pq = nullptr;
    DeviceArray<float> cent;    // [nlist][d] the centroids as the coarse index holds them
    DeviceArray<int> assign;    // [assign_cap] list of every row
    int64_t assign_cap = 0;
    DeviceArray<int> offsets;   // [nlist + 1]
    DeviceArray<int> list_rows; // [rows_cap]
    int64_t rows_cap = 0;
    Buffer count;               // [nlist] histogram of a table build
    Buffer cs, ci;              // coarse results of an assignment [chunk]
    Buffer stage, resid;        // host rows of an add, one chunk; the float32 residuals of a chunk / of the PQ training rows
    Buffer train_assign, flag;
    // a search's own: they grow only when a search asks for more (the tables are pq->lut)
    Buffer qbuf, ps, pi, parts, out_s, out_i, out_l;
    // by id
    Buffer ids, row_out;
    ~mips_ivfpq() {
        if (coarse) (void)mips_index_destroy(coarse);
        if (pq) (void)mips_pq_destroy(pq);
    }
};

namespace {

int ivfpq_check(const char* who, const mips_ivfpq* v) {
    if (!v) return fail(MIPS_E_INVALID, "%s: the IVFPQ index is NULL", who);
    return MIPS_OK;
}

bool ivfpq_trained(const mips_ivfpq* v) { return v->have_cent && v->pq->trained; }

// ivfpq_assign_rows, ivfpq_rebuild, ivfpq_reserve_assign and ivfpq_load_coarse below are the twins of ivf_assign_rows,
// ivf_build_table + ivf_rebuild, ivf_reserve_assign and ivf_load_coarse of host_ivf.hpp, which take a mips_ivf* (rows in its flat
// index) where these take a mips_ivfpq* (rows in its mips_pq): a fix in one belongs in the other.

// lists of n device rows (float32 / bf16) -> out (device int32), at most ivfpq::kAddChunk rows
int ivfpq_assign_rows(mips_ivfpq* v, const void* x_dev, int64_t n, int dtype, int* out, hipStream_t st) {
    int rc = v->cs.ensure((size_t)n * sizeof(float));
    if (rc) return rc;
    if ((rc = v->ci.ensure((size_t)n * sizeof(int64_t)))) return rc;
    if ((rc = mips_search(v->coarse, x_dev, dtype, n, 1, (float*)v->cs.p, (int64_t*)v->ci.p, 0, MIPS_Q_DEVICE | MIPS_OUT_DEVICE, st))) return rc;
    mips::ivf_to_assign_kernel<<<grid_for(n, 256), 256, 0, st>>>((const int64_t*)v->ci.p, n, v->nlist, out);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

// the list table of the rows the index holds
int ivfpq_rebuild(mips_ivfpq* v, hipStream_t st) {
    const int64_t n = v->pq->ntotal;
    if (v->rows_cap < n) {
        HIP_TRY(hipStreamSynchronize(st)); // (nothing in flight reads the table that goes)
        DeviceArray<int> fresh;
        const int64_t cap = round_up(std::max<int64_t>(n, v->rows_cap + v->rows_cap / 2), 256);
        hipError_t e = hipMalloc((void**)&fresh.p, (size_t)cap * sizeof(int));
        if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the list table failed: %s", (size_t)cap * sizeof(int), hipGetErrorString(e));
        std::swap(v->list_rows, fresh);
        v->rows_cap = cap;
    }
    int rc = v->count.ensure((size_t)v->nlist * sizeof(int));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(v->count.p, 0, (size_t)v->nlist * sizeof(int), st));
    if (n > 0) mips::ivf_hist_kernel<<<grid_for(n, 256), 256, 0, st>>>(v->assign, n, v->nlist, (int*)v->count.p);
    mips::ivf_offsets_kernel<<<1, mips::IVF_SCAN_THREADS, 0, st>>>((const int*)v->count.p, v->nlist, v->offsets);
    if (n > 0) mips::ivf_list_fill_kernel<<<(v->nlist + 3) / 4, 256, 0, st>>>(v->assign, n, v->nlist, v->offsets, v->list_rows);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int ivfpq_reserve_assign(mips_ivfpq* v, int64_t need, hipStream_t st) {
    if (need <= v->assign_cap) return MIPS_OK;
    const int64_t cap = round_up(std::max<int64_t>(need, v->assign_cap + v->assign_cap / 2), 256);
    DeviceArray<int> fresh;
    hipError_t e = hipMalloc((void**)&fresh.p, (size_t)cap * sizeof(int));
    if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the assignments failed: %s", (size_t)cap * sizeof(int), hipGetErrorString(e));
    const int64_t used = v->pq->ntotal;
    if (used > 0) HIP_TRY(hipMemcpyAsync(fresh, v->assign, (size_t)used * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the old storage is freed when this returns
    std::swap(v->assign, fresh);
    v->assign_cap = cap;
    return MIPS_OK;
}

// the centroids in v->cent -> the coarse index
int ivfpq_load_coarse(mips_ivfpq* v, hipStream_t st) {
    int rc = mips_index_reset(v->coarse);
    if (rc) return rc;
    return mips_index_add(v->coarse, v->cent, v->nlist, MIPS_DTYPE_F32, 1, st);
}

template <typename T>
void ivfpq_launch_residual(const mips_ivfpq* v, const void* x, int64_t n, const int* assign, float* out, hipStream_t st) {
    mips::ivfadc_residual_kernel<T><<<grid_for(n * v->d, 256), 256, 0, st>>>((const T*)x, n, v->d, assign, v->nlist, v->cent, v->by_residual ? 1 : 0, out);
}

int ivfpq_query_args(const char* who, const mips_ivfpq* v, const void* q, int q_dtype, int64_t nq) {
    if (!ivfpq_trained(v)) return fail(MIPS_E_INVALID, "%s: the IVFPQ index is not trained (mips_ivfpq_train, or _set_centroids and _set_codebook)", who);
    if (q_dtype != MIPS_DTYPE_F32 && q_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: q_dtype must be F32 or BF16", who);
    if (nq < 0 || (nq > 0 && !q)) return fail(MIPS_E_INVALID, "%s: bad q / nq", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    return MIPS_OK;
}

int ivfpq_probe_args(const char* who, const mips_ivfpq* v, int64_t nprobe, int* p) {
    if (nprobe < 1) return fail(MIPS_E_INVALID, "%s: nprobe must be >= 1, got %lld", who, (long long)nprobe);
    const int64_t pp = std::min<int64_t>(nprobe, v->nlist);
    if (pp > ivfpq::kMaxProbe) return fail(MIPS_E_UNSUPPORTED, "%s: min(nprobe, nlist) = %lld exceeds %d", who, (long long)pp, ivfpq::kMaxProbe);
    *p = (int)pp;
    return MIPS_OK;
}

// a slice of queries where the kernels read them: device queries as they are, host queries through v->qbuf
int ivfpq_stage_queries(mips_ivfpq* v, const void* qs, int64_t ns, size_t esz, bool q_dev, const void** out, hipStream_t st) {
    *out = qs;
    if (q_dev) return MIPS_OK;
    int rc = v->qbuf.ensure((size_t)ns * v->d * esz);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(v->qbuf.p, qs, (size_t)ns * v->d * esz, hipMemcpyHostToDevice, st));
    *out = v->qbuf.p;
    return MIPS_OK;
}

// P(q) and T of ns device queries -> v->ps [ns][p], v->pi [ns][p]: the coarse index's own certified search
int ivfpq_probe_slice(mips_ivfpq* v, const void* q_dev, int q_dtype, int64_t ns, int p, hipStream_t st) {
    int rc = v->ps.ensure((size_t)ns * p * sizeof(float));
    if (rc) return rc;
    if ((rc = v->pi.ensure((size_t)ns * p * sizeof(int64_t)))) return rc;
    const int flags = MIPS_Q_DEVICE | MIPS_OUT_DEVICE;
    if (p <= MIPS_MAX_K) return mips_search(v->coarse, q_dev, q_dtype, ns, p, (float*)v->ps.p, (int64_t*)v->pi.p, 0, flags, st);
    return mips_search_wide(v->coarse, q_dev, q_dtype, ns, p, (float*)v->ps.p, (int64_t*)v->pi.p, 0, flags, st);
}

// ids [n] where the kernels read them; host ids are checked first (an id >= 0 whose local row is past the index: MIPS_E_INVALID)
int ivfpq_stage_ids(const char* who, mips_ivfpq* v, const int64_t* ids, int64_t n, int64_t idx_offset, bool ids_dev, const int64_t** out, hipStream_t st) {
    *out = ids;
    if (ids_dev) return MIPS_OK;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= 0 && ids[i] - idx_offset >= v->pq->ntotal)
            return fail(MIPS_E_INVALID, "%s: id %lld (position %lld) names row %lld of %lld", who, (long long)ids[i], (long long)i,
                        (long long)(ids[i] - idx_offset), (long long)v->pq->ntotal);
    int rc = v->ids.ensure((size_t)n * sizeof(int64_t));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(v->ids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    *out = (const int64_t*)v->ids.p;
    return MIPS_OK;
}

} // namespace

extern "C" {

int mips_ivfpq_create(mips_ivfpq_t** out, int device, int64_t d, int64_t nlist, int64_t M, int nbits, int by_residual, int metric) {
    if (!out) return fail(MIPS_E_INVALID, "mips_ivfpq_create: out is NULL");
    *out = nullptr;
    if (metric == MIPS_METRIC_L2)
        return fail(MIPS_E_UNSUPPORTED, "mips_ivfpq_create: an IVFPQ index ranks by inner product only (coarse term plus a table of inner products)");
    if (metric != MIPS_METRIC_IP) return fail(MIPS_E_INVALID, "mips_ivfpq_create: metric must be 0 (inner product), got %d", metric);
    if (nlist < 1 || nlist > 65536) return fail(MIPS_E_UNSUPPORTED, "mips_ivfpq_create: nlist must be 1 .. 65536, got %lld", (long long)nlist);
    if (by_residual != 0 && by_residual != 1) return fail(MIPS_E_INVALID, "mips_ivfpq_create: by_residual must be 0 or 1, got %d", by_residual);
    std::unique_ptr<mips_ivfpq> v(new (std::nothrow) mips_ivfpq());
    if (!v) return fail(MIPS_E_NOMEM, "out of host memory");
    int rc = mips_pq_create(&v->pq, device, d, M, nbits, metric); // (refuses nbits != 8, M > 128, d > 1024, d % M != 0)
    if (rc) return rc;
    if ((rc = mips_index_create(&v->coarse, device, d, MIPS_DTYPE_F32, MIPS_METRIC_IP))) return rc;
    v->device = device;
    v->d = (int)d;
    v->nlist = (int)nlist;
    v->M = (int)M;
    v->by_residual = by_residual != 0;
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    HIP_TRY(hipDeviceGetAttribute(&v->cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipMalloc((void**)&v->cent.p, (size_t)nlist * d * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&v->offsets.p, (size_t)(nlist + 1) * sizeof(int)));
    HIP_TRY(hipMemset(v->offsets.p, 0, (size_t)(nlist + 1) * sizeof(int)));
    *out = v.release();
    return MIPS_OK;
}

int mips_ivfpq_destroy(mips_ivfpq_t* v) {
    if (!v) return MIPS_OK;
    DeviceGuard g(v->device);
    (void)hipDeviceSynchronize();
    delete v;
    return MIPS_OK;
}

int mips_ivfpq_is_trained(const mips_ivfpq_t* v) { return v ? (ivfpq_trained(v) ? 1 : 0) : -1; }
int64_t mips_ivfpq_ntotal(const mips_ivfpq_t* v) { return v ? v->pq->ntotal : -1; }
int64_t mips_ivfpq_nlist(const mips_ivfpq_t* v) { return v ? v->nlist : -1; }
int64_t mips_ivfpq_m(const mips_ivfpq_t* v) { return v ? v->M : -1; }

int mips_ivfpq_set_param(mips_ivfpq_t* v, const char* name, int64_t value) {
    int rc = ivfpq_check("mips_ivfpq_set_param", v);
    if (rc) return rc;
    if (name && std::strcmp(name, "ivf_niter") == 0) {
        if (value < 0 || value > 1000) return fail(MIPS_E_INVALID, "mips_ivfpq_set_param: ivf_niter must be 0 .. 1000");
        v->ivf_niter = (int)value;
        return MIPS_OK;
    }
    if (name && std::strcmp(name, "pq_niter") == 0) return mips_pq_set_param(v->pq, "pq_niter", value);
    if (name && std::strcmp(name, "pq_query_slice") == 0) {
        if (value < 1 || value > 4096) return fail(MIPS_E_INVALID, "mips_ivfpq_set_param: pq_query_slice must be 1 .. 4096");
        v->query_slice = value;
        return MIPS_OK;
    }
    if (name && std::strcmp(name, "scan_segments") == 0) {
        if (value < 0 || value > 65536) return fail(MIPS_E_INVALID, "mips_ivfpq_set_param: scan_segments must be 0 (automatic) .. 65536");
        v->scan_segments = value;
        return MIPS_OK;
    }
    return fail(MIPS_E_INVALID, "mips_ivfpq_set_param: unknown parameter '%s'", name ? name : "(null)");
}

int mips_ivfpq_train(mips_ivfpq_t* v, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream) {
    const char* who = "mips_ivfpq_train";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if (x_dtype != MIPS_DTYPE_F32 && x_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: x_dtype must be F32 or BF16", who);
    if (v->pq->ntotal > 0) return fail(MIPS_E_INVALID, "%s: the index holds %lld rows", who, (long long)v->pq->ntotal);
    if (!x || n < std::max<int64_t>(v->nlist, pq::kSub))
        return fail(MIPS_E_INVALID, "%s: %lld training rows for %d lists and %d centroids per sub-quantiser", who, (long long)n, v->nlist, pq::kSub);
    if (n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^31 training rows", who);
    const bool is_dev = (flags & MIPS_Q_DEVICE) != 0;
    const int d = v->d;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    // 1. the centroids: the IVF index's trainer on a temporary empty IVF index (it refuses a NaN or an infinity in x)
    {
        mips_ivf_t* tmp = nullptr;
        if ((rc = mips_ivf_create(&tmp, v->device, d, MIPS_DTYPE_BF16, MIPS_METRIC_IP, v->nlist))) return rc;
        std::unique_ptr<mips_ivf, int (*)(mips_ivf_t*)> own(tmp, mips_ivf_destroy); // (synchronises the device, then frees)
        if ((rc = mips_ivf_set_param(tmp, "ivf_niter", v->ivf_niter))) return rc;
        if ((rc = mips_ivf_train(tmp, x, n, x_dtype, is_dev ? MIPS_Q_DEVICE : 0, st))) return rc;
        v->have_cent = false;
        HIP_TRY(hipMemcpyAsync(v->cent, tmp->cent, (size_t)v->nlist * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if ((rc = ivfpq_load_coarse(v, st))) return rc;
    // 2. R: the PQ subsample of x as float32 on the device, every row replaced by its residual
    const int64_t m = n > pq::kTrainRows ? pq::kTrainRows : n;
    const size_t esz = x_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    if ((rc = v->resid.ensure((size_t)m * d * sizeof(float)))) return rc;
    float* R = (float*)v->resid.p;
    if (is_dev) {
        if (x_dtype == MIPS_DTYPE_F32) mips::ivf_gather_rows_kernel<float><<<grid_for(m * d, 256), 256, 0, st>>>((const float*)x, n, m, d, R);
        else mips::ivf_gather_rows_kernel<uint16_t><<<grid_for(m * d, 256), 256, 0, st>>>((const uint16_t*)x, n, m, d, R);
        HIP_TRY(hipGetLastError());
    } else {
        std::vector<float> h((size_t)m * d);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t r = pq::pick(i, n, m);
            if (x_dtype == MIPS_DTYPE_F32) std::memcpy(&h[(size_t)i * d], (const char*)x + (size_t)r * d * esz, (size_t)d * sizeof(float));
            else
                for (int j = 0; j < d; ++j) {
                    const uint32_t u = (uint32_t)((const uint16_t*)x)[(size_t)r * d + j] << 16;
                    std::memcpy(&h[(size_t)i * d + j], &u, 4);
                }
        }
        HIP_TRY(hipMemcpyAsync(R, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (v->by_residual) {
        if ((rc = v->train_assign.ensure((size_t)m * sizeof(int)))) return rc;
        if ((rc = ivfpq_assign_rows(v, R, m, MIPS_DTYPE_F32, (int*)v->train_assign.p, st))) return rc;
        ivfpq_launch_residual<float>(v, R, m, (const int*)v->train_assign.p, R, st); // (in place: element e reads and writes e)
        HIP_TRY(hipGetLastError());
    }
    // 3. the codebook: the PQ trainer on R (m <= 65536: it looks at every row; it refuses a residual that overflowed)
    if ((rc = mips_pq_train(v->pq, R, m, MIPS_DTYPE_F32, MIPS_Q_DEVICE, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    v->have_cent = true;
    return MIPS_OK;
}

int mips_ivfpq_set_centroids(mips_ivfpq_t* v, const float* c) {
    int rc = ivfpq_check("mips_ivfpq_set_centroids", v);
    if (rc) return rc;
    if (!c) return fail(MIPS_E_INVALID, "mips_ivfpq_set_centroids: NULL array");
    if (v->pq->ntotal > 0) return fail(MIPS_E_INVALID, "mips_ivfpq_set_centroids: the index holds %lld rows", (long long)v->pq->ntotal);
    if (!pq_host_finite(c, (int64_t)v->nlist * v->d, MIPS_DTYPE_F32)) return fail(MIPS_E_INVALID, "mips_ivfpq_set_centroids: a NaN or an infinity");
    DeviceGuard g(v->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(v->cent, c, (size_t)v->nlist * v->d * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = ivfpq_load_coarse(v, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    v->have_cent = true;
    return MIPS_OK;
}

int mips_ivfpq_get_centroids(mips_ivfpq_t* v, float* out) {
    int rc = ivfpq_check("mips_ivfpq_get_centroids", v);
    if (rc) return rc;
    if (!out) return fail(MIPS_E_INVALID, "mips_ivfpq_get_centroids: NULL array");
    if (!v->have_cent) return fail(MIPS_E_INVALID, "mips_ivfpq_get_centroids: the index has no centroids");
    DeviceGuard g(v->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, v->cent, (size_t)v->nlist * v->d * sizeof(float), hipMemcpyDeviceToHost));
    return MIPS_OK;
}

int mips_ivfpq_set_codebook(mips_ivfpq_t* v, const float* c) {
    int rc = ivfpq_check("mips_ivfpq_set_codebook", v);
    if (rc) return rc;
    return mips_pq_set_codebook(v->pq, c);
}

int mips_ivfpq_get_codebook(mips_ivfpq_t* v, float* out) {
    int rc = ivfpq_check("mips_ivfpq_get_codebook", v);
    if (rc) return rc;
    return mips_pq_get_codebook(v->pq, out);
}

int mips_ivfpq_add(mips_ivfpq_t* v, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream) {
    const char* who = "mips_ivfpq_add";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if (src_dtype != MIPS_DTYPE_F32 && src_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: src_dtype must be F32 or BF16 (codes: mips_ivfpq_add_codes)", who);
    if (n < 0 || (n > 0 && !rows)) return fail(MIPS_E_INVALID, "%s: bad rows / n", who);
    if (!ivfpq_trained(v)) return fail(MIPS_E_INVALID, "%s: the IVFPQ index is not trained (mips_ivfpq_train)", who);
    if (n == 0) return MIPS_OK;
    const int64_t n0 = v->pq->ntotal;
    if (n0 + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^31 - 256 rows on one GPU", who);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = ivfpq_reserve_assign(v, n0 + n, st))) return rc;
    const size_t esz = src_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    const int64_t chunk = std::min(n, ivfpq::kAddChunk);
    if (!src_is_device && (rc = v->stage.ensure((size_t)chunk * v->d * esz))) return rc;
    if (v->by_residual && (rc = v->resid.ensure((size_t)chunk * v->d * sizeof(float)))) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* src = (const char*)rows + (size_t)r0 * v->d * esz;
        if (!src_is_device) {
            HIP_TRY(hipMemcpyAsync(v->stage.p, src, (size_t)nr * v->d * esz, hipMemcpyHostToDevice, st));
            src = v->stage.p;
        }
        int* as = v->assign + n0 + r0;
        if ((rc = ivfpq_assign_rows(v, src, nr, src_dtype, as, st))) return rc;
        if (v->by_residual) {
            if (src_dtype == MIPS_DTYPE_F32) ivfpq_launch_residual<float>(v, src, nr, as, (float*)v->resid.p, st);
            else ivfpq_launch_residual<uint16_t>(v, src, nr, as, (float*)v->resid.p, st);
            HIP_TRY(hipGetLastError());
            rc = mips_pq_add(v->pq, v->resid.p, nr, MIPS_DTYPE_F32, 1, st);
        } else rc = mips_pq_add(v->pq, src, nr, src_dtype, 1, st);
        if (rc) { // the rows of this call go again: codes and assignments stay in step
            v->pq->ntotal = n0;
            return rc;
        }
        if (!src_is_device) HIP_TRY(hipStreamSynchronize(st)); // (the staging buffer is free again)
    }
    return ivfpq_rebuild(v, st);
}

int mips_ivfpq_add_codes(mips_ivfpq_t* v, const uint8_t* codes, const int32_t* assign, int64_t n, int src_is_device, void* hip_stream) {
    const char* who = "mips_ivfpq_add_codes";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!codes || !assign))) return fail(MIPS_E_INVALID, "%s: bad codes / assign / n", who);
    if (!ivfpq_trained(v)) return fail(MIPS_E_INVALID, "%s: the IVFPQ index is not trained (mips_ivfpq_train, or _set_centroids and _set_codebook)", who);
    if (n == 0) return MIPS_OK;
    const int64_t n0 = v->pq->ntotal;
    if (n0 + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^31 - 256 rows on one GPU", who);
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    // the assignments are checked on the host (the call synchronises anyway)
    std::vector<int32_t> h;
    const int32_t* ha = assign;
    if (src_is_device) {
        h.resize((size_t)n);
        HIP_TRY(hipMemcpyAsync(h.data(), assign, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ha = h.data();
    }
    for (int64_t i = 0; i < n; ++i)
        if (ha[i] < 0 || ha[i] >= v->nlist) return fail(MIPS_E_INVALID, "%s: row %lld names list %d of %d", who, (long long)i, ha[i], v->nlist);
    if ((rc = ivfpq_reserve_assign(v, n0 + n, st))) return rc;
    HIP_TRY(hipMemcpyAsync(v->assign + n0, assign, (size_t)n * sizeof(int32_t), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = mips_pq_add_codes(v->pq, codes, n, src_is_device, st))) return rc;
    return ivfpq_rebuild(v, st);
}

int mips_ivfpq_read_codes(mips_ivfpq_t* v, int64_t row0, int64_t n, uint8_t* out, void* hip_stream) {
    int rc = ivfpq_check("mips_ivfpq_read_codes", v);
    if (rc) return rc;
    return mips_pq_read_codes(v->pq, row0, n, out, hip_stream);
}

int mips_ivfpq_read_assign(mips_ivfpq_t* v, int64_t row0, int64_t n, int32_t* out, void* hip_stream) {
    int rc = ivfpq_check("mips_ivfpq_read_assign", v);
    if (rc) return rc;
    if (row0 < 0 || n < 0 || row0 + n > v->pq->ntotal || (n > 0 && !out))
        return fail(MIPS_E_INVALID, "mips_ivfpq_read_assign: bad range [%lld, +%lld) of %lld rows", (long long)row0, (long long)n, (long long)v->pq->ntotal);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemcpyAsync(out, v->assign + row0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int mips_ivfpq_list_sizes(mips_ivfpq_t* v, int64_t* out, void* hip_stream) {
    int rc = ivfpq_check("mips_ivfpq_list_sizes", v);
    if (rc) return rc;
    if (!out) return fail(MIPS_E_INVALID, "mips_ivfpq_list_sizes: NULL array");
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int> h((size_t)v->nlist + 1);
    HIP_TRY(hipMemcpyAsync(h.data(), v->offsets, h.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int l = 0; l < v->nlist; ++l) out[l] = (int64_t)h[l + 1] - h[l];
    return MIPS_OK;
}

int mips_ivfpq_reset(mips_ivfpq_t* v) {
    int rc = ivfpq_check("mips_ivfpq_reset", v);
    if (rc) return rc;
    DeviceGuard g(v->device);
    if ((rc = mips_pq_reset(v->pq))) return rc; // (synchronises the device)
    HIP_TRY(hipMemset(v->offsets.p, 0, (size_t)(v->nlist + 1) * sizeof(int)));
    return MIPS_OK;
}

int mips_ivfpq_probe(mips_ivfpq_t* v, const void* q, int q_dtype, int64_t nq, int64_t nprobe, int32_t* out_lists, float* out_scores, int flags,
                     void* hip_stream) {
    const char* who = "mips_ivfpq_probe";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if ((rc = ivfpq_query_args(who, v, q, q_dtype, nq))) return rc;
    int p = 0;
    if ((rc = ivfpq_probe_args(who, v, nprobe, &p))) return rc;
    if (nq == 0) return MIPS_OK;
    if (!out_lists) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    int* d_l = out_lists;
    if (!out_dev) {
        if ((rc = v->out_l.ensure((size_t)nq * p * sizeof(int)))) return rc;
        if (out_scores && (rc = v->out_s.ensure((size_t)nq * p * sizeof(float)))) return rc;
        d_l = (int*)v->out_l.p;
    }
    float* d_s = out_dev ? out_scores : (float*)v->out_s.p;
    for (int64_t s0 = 0; s0 < nq; s0 += v->query_slice) {
        const int64_t ns = std::min(v->query_slice, nq - s0);
        const void* qs = nullptr;
        if ((rc = ivfpq_stage_queries(v, (const char*)q + (size_t)s0 * v->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        if ((rc = ivfpq_probe_slice(v, qs, q_dtype, ns, p, st))) return rc;
        mips::ivfadc_lists_kernel<<<grid_for(ns * p, 256), 256, 0, st>>>((const int64_t*)v->pi.p, ns * p, v->nlist, d_l + (size_t)s0 * p);
        HIP_TRY(hipGetLastError());
        if (out_scores) HIP_TRY(hipMemcpyAsync(d_s + (size_t)s0 * p, v->ps.p, (size_t)ns * p * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_lists, d_l, (size_t)nq * p * sizeof(int), hipMemcpyDeviceToHost, st));
        if (out_scores) HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * p * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MIPS_OK;
}

int mips_ivfpq_search(mips_ivfpq_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx,
                      int64_t idx_offset, int flags, void* hip_stream) {
    const char* who = "mips_ivfpq_search";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if ((rc = ivfpq_query_args(who, v, q, q_dtype, nq))) return rc;
    int p = 0;
    if ((rc = ivfpq_probe_args(who, v, nprobe, &p))) return rc;
    if (k < 1 || k > MIPS_MAX_K) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K, k);
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
    const int waves = pq::scan_waves(v->M);
    const int lds = (int)ivfpq::scan_lds_bytes(v->M, p);
    for (int64_t s0 = 0; s0 < nq; s0 += v->query_slice) {
        const int64_t ns = std::min(v->query_slice, nq - s0);
        const void* qs = nullptr;
        if ((rc = ivfpq_stage_queries(v, (const char*)q + (size_t)s0 * v->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        // 1. the probe: list numbers and T, the coarse index's own certified search
        if ((rc = ivfpq_probe_slice(v, qs, q_dtype, ns, p, st))) return rc;
        // 2. the tables
        if ((rc = pq_tables(pqx, qs, q_dtype, ns, st))) return rc;
        // 3. the scan: one workgroup per (query, segment of the concatenation of its probed lists)
        const int S = ivfpq::choose_segments(ns, k, v->M, pqx->ntotal, p, v->nlist, v->cus, v->scan_segments);
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
        const unsigned grid = (unsigned)(ns * S); // <= 4096 * 65536 / k
        if (waves == 16) {
            HIP_TRY(hipFuncSetAttribute((const void*)mips::ivfadc_scan_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            mips::ivfadc_scan_kernel<16><<<grid, 64 * 16, lds, st>>>(a);
        } else {
            mips::ivfadc_scan_kernel<4><<<grid, 64 * 4, lds, st>>>(a);
        }
        HIP_TRY(hipGetLastError());
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

int mips_ivfpq_reconstruct(mips_ivfpq_t* v, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld, int flags,
                           void* hip_stream) {
    const char* who = "mips_ivfpq_reconstruct";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if (!ivfpq_trained(v)) return fail(MIPS_E_INVALID, "%s: the IVFPQ index is not trained", who);
    if (out_dtype != MIPS_DTYPE_F32) return fail(MIPS_E_INVALID, "%s: out_dtype must be F32 (the codes themselves: mips_ivfpq_read_codes)", who);
    if (n < 0 || out_ld < v->d || (n > 0 && (!ids || !out))) return fail(MIPS_E_INVALID, "%s: bad ids / out / n / out_ld", who);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    const bool out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const int64_t* d_ids = nullptr;
    if ((rc = ivfpq_stage_ids(who, v, ids, n, idx_offset, (flags & MIPS_IDS_DEVICE) != 0, &d_ids, st))) return rc;
    float* d_out = (float*)out;
    int64_t ld = out_ld;
    if (!out_dev) {
        if ((rc = v->row_out.ensure((size_t)n * v->d * sizeof(float)))) return rc;
        d_out = (float*)v->row_out.p;
        ld = v->d;
    }
    mips::ivfadc_rows_kernel<<<grid_for(n * v->d, 256), 256, 0, st>>>(v->pq->codes, v->pq->pitch, v->pq->ntotal, v->pq->cb, v->d, v->M, v->assign, v->nlist, v->cent,
                                                                      v->by_residual ? 1 : 0, d_ids, n, idx_offset, d_out, ld,
                                                                      (flags & MIPS_ROWS_ZERO_MISSING) ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (!out_dev) {
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_ld * sizeof(float), d_out, (size_t)v->d * sizeof(float), (size_t)v->d * sizeof(float), (size_t)n,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else if (!(flags & MIPS_IDS_DEVICE)) HIP_TRY(hipStreamSynchronize(st)); // (the caller's ids are free again)
    return MIPS_OK;
}

int mips_ivfpq_score_subset(mips_ivfpq_t* v, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores, int64_t idx_offset,
                            int flags, void* hip_stream) {
    const char* who = "mips_ivfpq_score_subset";
    int rc = ivfpq_check(who, v);
    if (rc) return rc;
    if ((rc = ivfpq_query_args(who, v, q, q_dtype, nq))) return rc;
    if (k < 0) return fail(MIPS_E_INVALID, "%s: k must be >= 0, got %d", who, k);
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!ids || !out_scores) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0, ids_dev = (flags & MIPS_IDS_DEVICE) != 0;
    DeviceGuard g(v->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    mips_pq* pqx = v->pq;
    const int64_t* d_ids = nullptr;
    if ((rc = ivfpq_stage_ids(who, v, ids, nq * k, idx_offset, ids_dev, &d_ids, st))) return rc;
    float* d_s = out_scores;
    if (!out_dev) {
        if ((rc = v->out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
        d_s = (float*)v->out_s.p;
    }
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    for (int64_t s0 = 0; s0 < nq; s0 += v->query_slice) {
        const int64_t ns = std::min(v->query_slice, nq - s0);
        const void* qs = nullptr;
        if ((rc = ivfpq_stage_queries(v, (const char*)q + (size_t)s0 * v->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        if ((rc = pq_tables(pqx, qs, q_dtype, ns, st))) return rc;
        const int grid = grid_for(ns * k, 256);
        if (q_dtype == MIPS_DTYPE_F32)
            mips::ivfadc_score_subset_kernel<float><<<grid, 256, 0, st>>>(pqx->codes, pqx->pitch, pqx->ntotal, (const float*)pqx->lut.p, v->M, v->assign, v->nlist, v->cent,
                                                                          v->d, v->by_residual ? 1 : 0, (const float*)qs, d_ids + (size_t)s0 * k, ns, k, idx_offset,
                                                                          d_s + (size_t)s0 * k);
        else
            mips::ivfadc_score_subset_kernel<uint16_t><<<grid, 256, 0, st>>>(pqx->codes, pqx->pitch, pqx->ntotal, (const float*)pqx->lut.p, v->M, v->assign, v->nlist,
                                                                             v->cent, v->d, v->by_residual ? 1 : 0, (const uint16_t*)qs, d_ids + (size_t)s0 * k, ns, k,
                                                                             idx_offset, d_s + (size_t)s0 * k);
        HIP_TRY(hipGetLastError());
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else if (!q_dev || !ids_dev) HIP_TRY(hipStreamSynchronize(st)); // (the caller's host buffers are free again)
    return MIPS_OK;
}

} // extern "C"
