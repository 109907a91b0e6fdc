// Host side of include/mips_hip_sq8.h (included by mips_hip.hip behind host_state.hpp): the trained parameters of an SQ8 index --
// training on the device, set / get from the host -- and the epilogue that turns the code-domain scores S of a finished result
// into the reported D = S + B_q.  Encoding and query staging are branches of convert_into (host_state.hpp), the scan's instance
// table is host_launch.hpp's, the exact tail takes mips::ElemU8 where the e4m3-documents index takes ElemF8.
#pragma once

namespace {

int sq8_check(const char* who, const mips_index* ix) {
    if (!ix) return fail(MIPS_E_INVALID, "%s: index is NULL", who);
    if (!ix->sq8) return fail(MIPS_E_INVALID, "%s: not an SQ8 index (mips_index_create with MIPS_DTYPE_SQ8)", who);
    return MIPS_OK;
}

int sq8_ensure_params(mips_index* ix) {
    if (!ix->sq8_params) HIP_TRY(hipMalloc((void**)&ix->sq8_params.p, (size_t)4 * ix->ld * sizeof(float)));
    return MIPS_OK;
}

// vmin | vdiff [2][ld] on the device (columns >= d zero) become the index's parameters; s and o follow
int sq8_adopt(mips_index* ix, const float* cand_dev, hipStream_t st) {
    int rc = sq8_ensure_params(ix);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->sq8_params, cand_dev, (size_t)2 * ix->ld * sizeof(float), hipMemcpyDeviceToDevice, st));
    mips::sq8_derive_kernel<<<(ix->ld + 255) / 256, 256, 0, st>>>(ix->sq8_params, ix->ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st)); // (the candidate buffer is scratch of the next training)
    ix->sq8_trained = true;
    return MIPS_OK;
}

int sq8_train(mips_index* ix, const void* x, int64_t n, int x_dtype, bool x_dev, hipStream_t st) {
    const int d = (int)ix->d, ld = ix->ld;
    const size_t slots = (size_t)mips::SQ8_PARTS * d;
    // [pmin | pmax] floats, the candidate vmin | vdiff [2][ld], the flag word, the parts' flags
    const size_t cand_off = 2 * slots * sizeof(float), bad_off = cand_off + (size_t)2 * ld * sizeof(float), flag_off = bad_off + 16;
    int rc = ix->sq8_part.ensure(flag_off + slots);
    if (rc) return rc;
    char* base = (char*)ix->sq8_part.p;
    float* pmin = (float*)base;
    float* pmax = pmin + slots;
    float* cand = (float*)(base + cand_off);
    unsigned* bad = (unsigned*)(base + bad_off);
    unsigned char* pflag = (unsigned char*)(base + flag_off);
    HIP_TRY(hipMemsetAsync(bad, 0, 16, st));
    const size_t esz = x_dtype == MIPS_DTYPE_F32 ? 4 : 2;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)(d * esz));
    const dim3 grid((unsigned)((d + 255) / 256), (unsigned)mips::SQ8_PARTS);
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t nr = std::min(chunk_rows, n - r0);
        const void* s = (const char*)x + (size_t)r0 * d * esz;
        if (!x_dev) {
            rc = ix->stage.ensure((size_t)nr * d * esz);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(ix->stage.p, s, (size_t)nr * d * esz, hipMemcpyHostToDevice, st));
            s = ix->stage.p;
        }
        if (x_dtype == MIPS_DTYPE_F32) mips::sq8_minmax_kernel<float><<<grid, 256, 0, st>>>((const float*)s, nr, d, pmin, pmax, pflag, r0 == 0);
        else mips::sq8_minmax_kernel<uint16_t><<<grid, 256, 0, st>>>((const uint16_t*)s, nr, d, pmin, pmax, pflag, r0 == 0);
        HIP_TRY(hipGetLastError());
        if (!x_dev) HIP_TRY(hipStreamSynchronize(st)); // the staging buffer is reused by the next chunk
    }
    mips::sq8_minmax_final_kernel<<<(ld + 255) / 256, 256, 0, st>>>(pmin, pmax, pflag, mips::SQ8_PARTS, d, ld, cand, cand + ld, bad);
    HIP_TRY(hipGetLastError());
    unsigned bad_h = 0;
    HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad_h) return fail(MIPS_E_INVALID, "mips_index_sq8_train: the training rows hold a NaN or an infinity");
    return sq8_adopt(ix, cand, st);
}

// The call's final scores stand in d_s [nq][k] (packed: in d_i): S -> D = S + B_q.  One launch on the stream that wrote them.
int sq8_finish(const SearchCall& c, float* d_s, int64_t* d_i, bool packed, int64_t nq, int k, hipStream_t st) {
    mips::sq8_bias_kernel<<<grid_for(nq * k, 256), 256, 0, st>>>(d_s, packed ? d_i : nullptr, c.qbias, nq, k);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

} // namespace

extern "C" {

int mips_index_sq8_train(mips_index_t* ix, const void* x, int64_t n, int x_dtype, int flags, void* hip_stream) {
    int rc = sq8_check("mips_index_sq8_train", ix);
    if (rc) return rc;
    if (n <= 0 || !x) return fail(MIPS_E_INVALID, "mips_index_sq8_train: no training rows");
    if (x_dtype != MIPS_DTYPE_F32 && x_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_index_sq8_train: x_dtype must be F32 or BF16");
    if (ix->ntotal > 0) return fail(MIPS_E_INVALID, "mips_index_sq8_train: the index holds %lld rows (training replaces the parameters of an empty index only)", (long long)ix->ntotal);
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    rc = wait_for_tail(ix, st, /*both_sets=*/true);
    if (rc) return rc;
    return sq8_train(ix, x, n, x_dtype, (flags & MIPS_Q_DEVICE) != 0, st);
}

int mips_index_sq8_set_params(mips_index_t* ix, const float* vmin, const float* vdiff) {
    int rc = sq8_check("mips_index_sq8_set_params", ix);
    if (rc) return rc;
    if (!vmin || !vdiff) return fail(MIPS_E_INVALID, "mips_index_sq8_set_params: NULL array");
    if (ix->ntotal > 0) return fail(MIPS_E_INVALID, "mips_index_sq8_set_params: the index holds %lld rows", (long long)ix->ntotal);
    for (int64_t j = 0; j < ix->d; ++j)
        if (!std::isfinite(vmin[j]) || !std::isfinite(vdiff[j]) || vdiff[j] < 0.0f)
            return fail(MIPS_E_INVALID, "mips_index_sq8_set_params: column %lld: vmin and vdiff must be finite, vdiff >= 0", (long long)j);
    DeviceGuard g(ix->device);
    ORDER_ON(ix, nullptr);
    rc = wait_for_tail(ix, nullptr, /*both_sets=*/true);
    if (rc) return rc;
    std::vector<float> h((size_t)2 * ix->ld, 0.0f);
    std::copy(vmin, vmin + ix->d, h.begin());
    std::copy(vdiff, vdiff + ix->d, h.begin() + ix->ld);
    rc = ix->sq8_part.ensure(h.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ix->sq8_part.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, nullptr));
    return sq8_adopt(ix, (const float*)ix->sq8_part.p, nullptr);
}

int mips_index_sq8_get_params(mips_index_t* ix, float* vmin, float* vdiff) {
    int rc = sq8_check("mips_index_sq8_get_params", ix);
    if (rc) return rc;
    if (!vmin || !vdiff) return fail(MIPS_E_INVALID, "mips_index_sq8_get_params: NULL array");
    if (!ix->sq8_trained) return fail(MIPS_E_INVALID, "mips_index_sq8_get_params: the index is not trained");
    DeviceGuard g(ix->device);
    ORDER_ON(ix, nullptr);
    HIP_TRY(hipMemcpyAsync(vmin, ix->sq8_params, (size_t)ix->d * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(vdiff, ix->sq8_params + ix->ld, (size_t)ix->d * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MIPS_OK;
}

int mips_index_sq8_is_trained(const mips_index_t* ix) { return ix && ix->sq8 ? (ix->sq8_trained ? 1 : 0) : -1; }

} // extern "C"
