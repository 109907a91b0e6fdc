// Host side of the product-quantised index (include/mips_hip_pq.h; the kernels: pq_kernels.hpp; the arithmetic: pq_math.hpp).
// Included last by mips_hip.hip.  The object owns the codebook [M][256][dsub], the codes [capacity][pitch] and its scratch; device
// resources are owned by type (DeviceArray, Buffer): `delete pq` leaves nothing.  mips_pq_search is a fixed launch sequence --
// tables, scan, merge, finish -- in which every grid, block, LDS size, pointer and loop bound comes from (ns, k, M, d, ntotal, the CU
// count) and the object: nothing is read back from the device.
#pragma once

struct mips_pq {
    int device = 0;
    int d = 0, M = 0, dsub = 0;
    int pitch = 0;             // bytes per stored row: M rounded up to pq::kCodeAlign, the tail zero
    int niter = 10;
    int64_t query_slice = 256; // queries one pass of a search serves
    bool trained = false;
    int64_t ntotal = 0, capacity = 0;
    int cus = 1;
    DeviceArray<float> cb;      // [M][256][dsub]
    DeviceArray<uint8_t> codes; // [capacity][pitch]
    // training: the rows the trainer looks at, their codes [M][rows], the list tables
    Buffer train_rows, train_assign, train_count, train_off, train_list, flag;
    Buffer stage;               // host rows / host codes of an add, one chunk
    // a search's own: they grow only when a search asks for more
    Buffer qbuf, lut, parts, out_s, out_i;
    // by id
    Buffer ids, row_out;
};

namespace {

constexpr int64_t kPqAddChunk = 65536; // host rows one staging copy carries

int pq_check(const char* who, const mips_pq* p) {
    if (!p) return fail(MIPS_E_INVALID, "%s: the PQ index is NULL", who);
    return MIPS_OK;
}

bool pq_host_finite(const void* x, int64_t total, int dtype) {
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

// room for `need` rows; what the index holds is kept
int pq_reserve(mips_pq* p, int64_t need, hipStream_t st) {
    if (need <= p->capacity) return MIPS_OK;
    const int64_t cap = round_up(std::max<int64_t>(need, p->capacity + p->capacity / 2), 256);
    DeviceArray<uint8_t> fresh;
    hipError_t e = hipMalloc((void**)&fresh.p, (size_t)cap * p->pitch);
    if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the codes failed: %s", (size_t)cap * p->pitch, hipGetErrorString(e));
    if (p->ntotal > 0) HIP_TRY(hipMemcpyAsync(fresh, p->codes, (size_t)p->ntotal * p->pitch, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the old storage is freed when this returns
    std::swap(p->codes, fresh);
    p->capacity = cap;
    return MIPS_OK;
}

template <typename T>
void pq_launch_assign(const mips_pq* p, const T* x, int64_t n, uint8_t* out, int64_t row_stride, int64_t m_stride, hipStream_t st) {
    const dim3 grid((unsigned)grid_for(n, 256), (unsigned)p->M);
    mips::pq_assign_kernel<T><<<grid, 256, 0, st>>>(x, n, p->d, p->M, p->cb, out, row_stride, m_stride);
}

// the tables of ns device queries -> p->lut
int pq_tables(mips_pq* p, const void* q_dev, int q_dtype, int64_t ns, hipStream_t st) {
    int rc = p->lut.ensure((size_t)ns * p->M * pq::kSub * sizeof(float));
    if (rc) return rc;
    const int64_t total = ns * p->M * pq::kSub;
    if (q_dtype == MIPS_DTYPE_F32) mips::pq_lut_kernel<float><<<grid_for(total, 256), 256, 0, st>>>((const float*)q_dev, ns, p->d, p->M, p->cb, (float*)p->lut.p);
    else mips::pq_lut_kernel<uint16_t><<<grid_for(total, 256), 256, 0, st>>>((const uint16_t*)q_dev, ns, p->d, p->M, p->cb, (float*)p->lut.p);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

// a slice of queries where the kernels read them: device queries as they are, host queries through p->qbuf
int pq_stage_queries(mips_pq* p, const void* qs, int64_t ns, size_t esz, bool q_dev, const void** out, hipStream_t st) {
    *out = qs;
    if (q_dev) return MIPS_OK;
    int rc = p->qbuf.ensure((size_t)ns * p->d * esz);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p->qbuf.p, qs, (size_t)ns * p->d * esz, hipMemcpyHostToDevice, st));
    *out = p->qbuf.p;
    return MIPS_OK;
}

int pq_query_args(const char* who, const mips_pq* p, const void* q, int q_dtype, int64_t nq) {
    if (!p->trained) return fail(MIPS_E_INVALID, "%s: the PQ index is not trained (mips_pq_train / mips_pq_set_codebook)", who);
    if (q_dtype != MIPS_DTYPE_F32 && q_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: q_dtype must be F32 or BF16", who);
    if (nq < 0 || (nq > 0 && !q)) return fail(MIPS_E_INVALID, "%s: bad q / nq", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    return MIPS_OK;
}

// ids [n] where the kernels read them; host ids are checked first (an id >= 0 whose local row is past the index: MIPS_E_INVALID)
int pq_stage_ids(const char* who, mips_pq* p, const int64_t* ids, int64_t n, int64_t idx_offset, bool ids_dev, const int64_t** out, hipStream_t st) {
    *out = ids;
    if (ids_dev) return MIPS_OK;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= 0 && ids[i] - idx_offset >= p->ntotal)
            return fail(MIPS_E_INVALID, "%s: id %lld (position %lld) names row %lld of %lld", who, (long long)ids[i], (long long)i,
                        (long long)(ids[i] - idx_offset), (long long)p->ntotal);
    int rc = p->ids.ensure((size_t)n * sizeof(int64_t));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p->ids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    *out = (const int64_t*)p->ids.p;
    return MIPS_OK;
}

} // namespace

extern "C" {

int mips_pq_create(mips_pq_t** out, int device, int64_t d, int64_t M, int nbits, int metric) {
    if (!out) return fail(MIPS_E_INVALID, "mips_pq_create: out is NULL");
    *out = nullptr;
    if (metric == MIPS_METRIC_L2) return fail(MIPS_E_UNSUPPORTED, "mips_pq_create: a PQ index ranks by inner product only (the lookup table holds inner products)");
    if (metric != MIPS_METRIC_IP) return fail(MIPS_E_INVALID, "mips_pq_create: metric must be 0 (inner product), got %d", metric);
    if (nbits != 8) return fail(MIPS_E_UNSUPPORTED, "mips_pq_create: %d bits per code are not served (8: 256 centroids per sub-quantiser)", nbits);
    if (d <= 0) return fail(MIPS_E_INVALID, "mips_pq_create: bad dimension %lld", (long long)d);
    if (d > 1024) return fail(MIPS_E_UNSUPPORTED, "mips_pq_create: rows of more than 1024 columns are not served");
    if (M < 1) return fail(MIPS_E_INVALID, "mips_pq_create: M must be >= 1, got %lld", (long long)M);
    if (M > pq::kMaxM) return fail(MIPS_E_UNSUPPORTED, "mips_pq_create: M = %lld exceeds %d (the query's table is M KiB of LDS)", (long long)M, pq::kMaxM);
    if (d % M != 0) return fail(MIPS_E_INVALID, "mips_pq_create: d = %lld is not a multiple of M = %lld", (long long)d, (long long)M);
    std::unique_ptr<mips_pq> p(new (std::nothrow) mips_pq());
    if (!p) return fail(MIPS_E_NOMEM, "out of host memory");
    p->device = device;
    p->d = (int)d;
    p->M = (int)M;
    p->dsub = (int)(d / M);
    p->pitch = pq::code_pitch((int)M);
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipMalloc((void**)&p->cb.p, (size_t)pq::kSub * d * sizeof(float)));
    *out = p.release();
    return MIPS_OK;
}

int mips_pq_destroy(mips_pq_t* p) {
    if (!p) return MIPS_OK;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    delete p;
    return MIPS_OK;
}

int mips_pq_is_trained(const mips_pq_t* p) { return p ? (p->trained ? 1 : 0) : -1; }
int64_t mips_pq_ntotal(const mips_pq_t* p) { return p ? p->ntotal : -1; }
int64_t mips_pq_m(const mips_pq_t* p) { return p ? p->M : -1; }

int mips_pq_set_param(mips_pq_t* p, const char* name, int64_t value) {
    int rc = pq_check("mips_pq_set_param", p);
    if (rc) return rc;
    if (name && std::strcmp(name, "pq_niter") == 0) {
        if (value < 0 || value > 1000) return fail(MIPS_E_INVALID, "mips_pq_set_param: pq_niter must be 0 .. 1000");
        p->niter = (int)value;
        return MIPS_OK;
    }
    if (name && std::strcmp(name, "pq_query_slice") == 0) {
        if (value < 1 || value > 4096) return fail(MIPS_E_INVALID, "mips_pq_set_param: pq_query_slice must be 1 .. 4096");
        p->query_slice = value;
        return MIPS_OK;
    }
    return fail(MIPS_E_INVALID, "mips_pq_set_param: unknown parameter '%s'", name ? name : "(null)");
}

int mips_pq_train(mips_pq_t* p, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream) {
    int rc = pq_check("mips_pq_train", p);
    if (rc) return rc;
    if (x_dtype != MIPS_DTYPE_F32 && x_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_pq_train: x_dtype must be F32 or BF16");
    if (p->ntotal > 0) return fail(MIPS_E_INVALID, "mips_pq_train: the index holds %lld rows", (long long)p->ntotal);
    if (!x || n < pq::kSub) return fail(MIPS_E_INVALID, "mips_pq_train: %lld training rows for %d centroids", (long long)n, pq::kSub);
    if (n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_pq_train: more than 2^31 training rows");
    const bool is_dev = (flags & MIPS_Q_DEVICE) != 0;
    const int d = p->d, M = p->M;
    const int64_t m = n > pq::kTrainRows ? pq::kTrainRows : n;
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = p->train_rows.ensure((size_t)m * d * sizeof(float)))) return rc;
    if ((rc = p->train_assign.ensure((size_t)m * M))) return rc;
    if ((rc = p->train_count.ensure((size_t)M * pq::kSub * sizeof(int)))) return rc;
    if ((rc = p->train_off.ensure((size_t)M * (pq::kSub + 1) * sizeof(int)))) return rc;
    if ((rc = p->train_list.ensure((size_t)m * M * sizeof(int)))) return rc;
    float* T = (float*)p->train_rows.p;
    if (is_dev) { // (the finite check and the evenly spaced gather of the IVF trainer: the same rule with nlist -> 256)
        if ((rc = p->flag.ensure(sizeof(int)))) return rc;
        HIP_TRY(hipMemsetAsync(p->flag.p, 0, sizeof(int), st));
        if (x_dtype == MIPS_DTYPE_F32) {
            mips::ivf_finite_kernel<float><<<grid_for(n * d, 256), 256, 0, st>>>((const float*)x, n * d, (int*)p->flag.p);
            mips::ivf_gather_rows_kernel<float><<<grid_for(m * d, 256), 256, 0, st>>>((const float*)x, n, m, d, T);
        } else {
            mips::ivf_finite_kernel<uint16_t><<<grid_for(n * d, 256), 256, 0, st>>>((const uint16_t*)x, n * d, (int*)p->flag.p);
            mips::ivf_gather_rows_kernel<uint16_t><<<grid_for(m * d, 256), 256, 0, st>>>((const uint16_t*)x, n, m, d, T);
        }
        HIP_TRY(hipGetLastError());
        int bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, p->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return fail(MIPS_E_INVALID, "mips_pq_train: the training rows hold a NaN or an infinity");
    } else {
        if (!pq_host_finite(x, n * d, x_dtype)) return fail(MIPS_E_INVALID, "mips_pq_train: the training rows hold a NaN or an infinity");
        std::vector<float> h((size_t)m * d);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t r = pq::pick(i, n, m);
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
    p->trained = false;
    const int64_t cb_total = (int64_t)pq::kSub * d;
    mips::pq_init_codebook_kernel<<<grid_for(cb_total, 256), 256, 0, st>>>(T, m, d, M, p->cb);
    HIP_TRY(hipGetLastError());
    uint8_t* as = (uint8_t*)p->train_assign.p;
    for (int it = 0; it < p->niter; ++it) {
        pq_launch_assign<float>(p, T, m, as, 1, m, st);
        HIP_TRY(hipMemsetAsync(p->train_count.p, 0, (size_t)M * pq::kSub * sizeof(int), st));
        mips::pq_hist_kernel<<<grid_for(m * M, 256), 256, 0, st>>>(as, m, M, (int*)p->train_count.p);
        mips::pq_offsets_kernel<<<M, pq::kSub, 0, st>>>((const int*)p->train_count.p, (int*)p->train_off.p);
        mips::pq_list_fill_kernel<<<M * pq::kSub / 4, 256, 0, st>>>(as, m, M, (const int*)p->train_off.p, (int*)p->train_list.p);
        mips::pq_centroid_mean_kernel<<<grid_for(cb_total, 256), 256, 0, st>>>(T, m, d, M, (const int*)p->train_off.p, (const int*)p->train_list.p, p->cb);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    p->trained = true;
    return MIPS_OK;
}

int mips_pq_set_codebook(mips_pq_t* p, const float* c) {
    int rc = pq_check("mips_pq_set_codebook", p);
    if (rc) return rc;
    if (!c) return fail(MIPS_E_INVALID, "mips_pq_set_codebook: NULL array");
    if (p->ntotal > 0) return fail(MIPS_E_INVALID, "mips_pq_set_codebook: the index holds %lld rows", (long long)p->ntotal);
    if (!pq_host_finite(c, (int64_t)pq::kSub * p->d, MIPS_DTYPE_F32)) return fail(MIPS_E_INVALID, "mips_pq_set_codebook: a NaN or an infinity");
    DeviceGuard g(p->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(p->cb, c, (size_t)pq::kSub * p->d * sizeof(float), hipMemcpyHostToDevice));
    p->trained = true;
    return MIPS_OK;
}

int mips_pq_get_codebook(mips_pq_t* p, float* out) {
    int rc = pq_check("mips_pq_get_codebook", p);
    if (rc) return rc;
    if (!out) return fail(MIPS_E_INVALID, "mips_pq_get_codebook: NULL array");
    if (!p->trained) return fail(MIPS_E_INVALID, "mips_pq_get_codebook: the index is not trained");
    DeviceGuard g(p->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, p->cb, (size_t)pq::kSub * p->d * sizeof(float), hipMemcpyDeviceToHost));
    return MIPS_OK;
}

int mips_pq_add(mips_pq_t* p, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream) {
    int rc = pq_check("mips_pq_add", p);
    if (rc) return rc;
    if (src_dtype != MIPS_DTYPE_F32 && src_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_pq_add: src_dtype must be F32 or BF16 (codes: mips_pq_add_codes)");
    if (n < 0 || (n > 0 && !rows)) return fail(MIPS_E_INVALID, "mips_pq_add: bad rows / n");
    if (!p->trained) return fail(MIPS_E_INVALID, "mips_pq_add: the PQ index is not trained (mips_pq_train / mips_pq_set_codebook)");
    if (n == 0) return MIPS_OK;
    if (p->ntotal + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_pq_add: more than 2^31 - 256 rows on one GPU");
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = pq_reserve(p, p->ntotal + n, st))) return rc;
    const size_t esz = src_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    // the tail of every new row (columns M .. pitch - 1) is zero: the scan reads whole 16-byte chunks
    HIP_TRY(hipMemsetAsync(p->codes + (size_t)p->ntotal * p->pitch, 0, (size_t)n * p->pitch, st));
    const int64_t chunk = src_is_device ? n : std::min(n, kPqAddChunk);
    if (!src_is_device && (rc = p->stage.ensure((size_t)chunk * p->d * esz))) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* src = (const char*)rows + (size_t)r0 * p->d * esz;
        if (!src_is_device) {
            HIP_TRY(hipMemcpyAsync(p->stage.p, src, (size_t)nr * p->d * esz, hipMemcpyHostToDevice, st));
            src = p->stage.p;
        }
        uint8_t* dst = p->codes + (size_t)(p->ntotal + r0) * p->pitch;
        if (src_dtype == MIPS_DTYPE_F32) pq_launch_assign<float>(p, (const float*)src, nr, dst, p->pitch, 1, st);
        else pq_launch_assign<uint16_t>(p, (const uint16_t*)src, nr, dst, p->pitch, 1, st);
        HIP_TRY(hipGetLastError());
    }
    if (!src_is_device) HIP_TRY(hipStreamSynchronize(st)); // (the caller's rows and the staging buffer are free again)
    p->ntotal += n;
    return MIPS_OK;
}

int mips_pq_add_codes(mips_pq_t* p, const uint8_t* codes, int64_t n, int src_is_device, void* hip_stream) {
    int rc = pq_check("mips_pq_add_codes", p);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !codes)) return fail(MIPS_E_INVALID, "mips_pq_add_codes: bad codes / n");
    if (!p->trained) return fail(MIPS_E_INVALID, "mips_pq_add_codes: the PQ index is not trained (mips_pq_train / mips_pq_set_codebook)");
    if (n == 0) return MIPS_OK;
    if (p->ntotal + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_pq_add_codes: more than 2^31 - 256 rows on one GPU");
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = pq_reserve(p, p->ntotal + n, st))) return rc;
    uint8_t* dst = p->codes + (size_t)p->ntotal * p->pitch;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n * p->pitch, st));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)p->pitch, codes, (size_t)p->M, (size_t)p->M, (size_t)n, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!src_is_device) HIP_TRY(hipStreamSynchronize(st));
    p->ntotal += n;
    return MIPS_OK;
}

int mips_pq_read_codes(mips_pq_t* p, int64_t row0, int64_t n, uint8_t* out, void* hip_stream) {
    int rc = pq_check("mips_pq_read_codes", p);
    if (rc) return rc;
    if (row0 < 0 || n < 0 || row0 + n > p->ntotal || (n > 0 && !out))
        return fail(MIPS_E_INVALID, "mips_pq_read_codes: bad range [%lld, +%lld) of %lld rows", (long long)row0, (long long)n, (long long)p->ntotal);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)p->M, p->codes + (size_t)row0 * p->pitch, (size_t)p->pitch, (size_t)p->M, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int mips_pq_reset(mips_pq_t* p) {
    int rc = pq_check("mips_pq_reset", p);
    if (rc) return rc;
    DeviceGuard g(p->device);
    HIP_TRY(hipDeviceSynchronize());
    p->ntotal = 0;
    return MIPS_OK;
}

int mips_pq_search(mips_pq_t* p, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset, int flags,
                   void* hip_stream) {
    const char* who = "mips_pq_search";
    int rc = pq_check(who, p);
    if (rc) return rc;
    if ((rc = pq_query_args(who, p, q, q_dtype, nq))) return rc;
    if (k < 1 || k > MIPS_MAX_K) return fail(MIPS_E_INVALID, "%s: k must be 1 .. %d, got %d", who, MIPS_MAX_K, k);
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
    const int waves = pq::scan_waves(p->M);
    const int lds = (int)pq::scan_lds_bytes(p->M);
    for (int64_t s0 = 0; s0 < nq; s0 += p->query_slice) {
        const int64_t ns = std::min(p->query_slice, nq - s0);
        // 1. the tables
        const void* qs = nullptr;
        if ((rc = pq_stage_queries(p, (const char*)q + (size_t)s0 * p->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        if ((rc = pq_tables(p, qs, q_dtype, ns, st))) return rc;
        // 2. the scan: one workgroup per (query, row segment)
        const int S = pq::choose_segments(ns, k, p->M, p->ntotal, p->cus);
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
        const unsigned grid = (unsigned)(ns * S); // <= 4096 * 65536 / k
        if (waves == 16) {
            HIP_TRY(hipFuncSetAttribute((const void*)mips::pq_adc_scan_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            mips::pq_adc_scan_kernel<16><<<grid, 64 * 16, lds, st>>>(a);
        } else {
            mips::pq_adc_scan_kernel<4><<<grid, 64 * 4, lds, st>>>(a);
        }
        HIP_TRY(hipGetLastError());
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

int mips_pq_reconstruct(mips_pq_t* p, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld, int flags,
                        void* hip_stream) {
    const char* who = "mips_pq_reconstruct";
    int rc = pq_check(who, p);
    if (rc) return rc;
    if (!p->trained) return fail(MIPS_E_INVALID, "%s: the PQ index is not trained", who);
    if (out_dtype != MIPS_DTYPE_F32) return fail(MIPS_E_INVALID, "%s: out_dtype must be F32 (the codes themselves: mips_pq_read_codes)", who);
    if (n < 0 || out_ld < p->d || (n > 0 && (!ids || !out))) return fail(MIPS_E_INVALID, "%s: bad ids / out / n / out_ld", who);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    const bool out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const int64_t* d_ids = nullptr;
    if ((rc = pq_stage_ids(who, p, ids, n, idx_offset, (flags & MIPS_IDS_DEVICE) != 0, &d_ids, st))) return rc;
    float* d_out = (float*)out;
    int64_t ld = out_ld;
    if (!out_dev) {
        if ((rc = p->row_out.ensure((size_t)n * p->d * sizeof(float)))) return rc;
        d_out = (float*)p->row_out.p;
        ld = p->d;
    }
    mips::pq_rows_kernel<<<grid_for(n * p->d, 256), 256, 0, st>>>(p->codes, p->pitch, p->ntotal, p->cb, p->d, p->M, d_ids, n, idx_offset, d_out, ld,
                                                                  (flags & MIPS_ROWS_ZERO_MISSING) ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (!out_dev) {
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_ld * sizeof(float), d_out, (size_t)p->d * sizeof(float), (size_t)p->d * sizeof(float), (size_t)n,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else if (!(flags & MIPS_IDS_DEVICE)) HIP_TRY(hipStreamSynchronize(st)); // (the caller's ids are free again)
    return MIPS_OK;
}

int mips_pq_score_subset(mips_pq_t* p, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores, int64_t idx_offset, int flags,
                         void* hip_stream) {
    const char* who = "mips_pq_score_subset";
    int rc = pq_check(who, p);
    if (rc) return rc;
    if ((rc = pq_query_args(who, p, q, q_dtype, nq))) return rc;
    if (k < 0) return fail(MIPS_E_INVALID, "%s: k must be >= 0, got %d", who, k);
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!ids || !out_scores) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0, out_dev = (flags & MIPS_OUT_DEVICE) != 0, ids_dev = (flags & MIPS_IDS_DEVICE) != 0;
    DeviceGuard g(p->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    const int64_t* d_ids = nullptr;
    if ((rc = pq_stage_ids(who, p, ids, nq * k, idx_offset, ids_dev, &d_ids, st))) return rc;
    float* d_s = out_scores;
    if (!out_dev) {
        if ((rc = p->out_s.ensure((size_t)nq * k * sizeof(float)))) return rc;
        d_s = (float*)p->out_s.p;
    }
    const size_t esz = q_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    for (int64_t s0 = 0; s0 < nq; s0 += p->query_slice) {
        const int64_t ns = std::min(p->query_slice, nq - s0);
        const void* qs = nullptr;
        if ((rc = pq_stage_queries(p, (const char*)q + (size_t)s0 * p->d * esz, ns, esz, q_dev, &qs, st))) return rc;
        if ((rc = pq_tables(p, qs, q_dtype, ns, st))) return rc;
        mips::pq_score_subset_kernel<<<grid_for(ns * k, 256), 256, 0, st>>>(p->codes, p->pitch, p->ntotal, (const float*)p->lut.p, p->M, d_ids + (size_t)s0 * k, ns, k,
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
