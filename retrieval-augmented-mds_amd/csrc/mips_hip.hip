// C ABI of the MI355X MIPS backend (include/mips_hip.h), gfx950 only.  ONE translation unit: the kernels (*.hpp), the host side
// in three parts -- host_state.hpp (the index object; search_report.hpp: the report of a search call), host_launch.hpp (which kernel
// answers which search), host_search.hpp (what a search does around its scan) -- and, below, the extern "C" entry points themselves.
// The search entry points validate their arguments and then share one prologue (run_call), which hands their body the SearchCall
// of the whole index and the call's SearchReport.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include <cstdlib>

#include "../../include/mips_hip.h"
#include "../../include/mips_hip_sharded.h"
#include "../../include/mips_hip_update.h"
#include "../../include/mips_hip_rows.h"
#include "../../include/mips_hip_hook.h"
#include "../../include/mips_hip_sq8.h"
#include "../../include/mips_hip_ivf.h"
#include "../../include/mips_hip_ivf_range.h"
#include "../../include/mips_hip_ivf_sharded.h"
#include "../../include/mips_hip_write.h"
#include "../../include/mips_hip_pq.h"
#include "../../include/mips_hip_ivfpq.h"
#include "../../include/mips_hip_refine.h"
#include "aux_kernels.hpp"
#include "scan_kernel.hpp"
#include "scan_kernel_v3.hpp"
#include "scan_kernel_f8.hpp"
#include "scan_kernel_f8x.hpp"
#include "scan_kernel_v4.hpp"
#include "scan_kernel_k3.hpp"
#include "scan_kernel_e8.hpp"
#include "tiny_search.hpp"
#include "resolve_kernels.hpp"
#include "scan_kernel_wide.hpp"
#include "range_kernels.hpp"
#include "range_merge_kernels.hpp"
#include "select_kernels.hpp"
#include "remove_kernels.hpp"
#include "rows_kernels.hpp"
#include "sq8_kernels.hpp"
#include "sq8_scan_kernel.hpp"
#include "ivf_kernels.hpp"
#include "ivf_search_kernels.hpp"
#include "ivf_wide_kernels.hpp"
#include "ivf_range_kernels.hpp"
#include "ivf_sharded_kernels.hpp"
#include "update_kernels.hpp"
#include "pq_kernels.hpp"
#include "ivfpq_kernels.hpp"
#include "refine_kernels.hpp"

#include "search_report.hpp"
#include "host_state.hpp"
#include "host_sq8.hpp"
#include "host_launch.hpp"
#include "host_search.hpp"
#include "host_wide.hpp"
#include "host_range.hpp"
#include "host_range_merge.hpp"
#include "remove_plan.hpp"
#include "host_remove.hpp"
#include "host_rows.hpp"
#include "host_update.hpp"

extern "C" {

int mips_abi_version(void) { return MIPS_ABI_VERSION; }

const char* mips_last_error(void) { return g_err.c_str(); }

int mips_index_create(mips_index_t** out, int device, int64_t d, int doc_dtype, int metric) {
    if (!out) return fail(MIPS_E_INVALID, "mips_index_create: out is NULL");
    *out = nullptr;
    if (d <= 0 || d > (1 << 20)) return fail(MIPS_E_INVALID, "mips_index_create: bad dimension %lld", (long long)d);
    if (metric != MIPS_METRIC_IP && metric != MIPS_METRIC_L2)
        return fail(MIPS_E_INVALID, "mips_index_create: metric must be 0 (inner product) or 1 (L2), got %d", metric);
    const bool sq8 = doc_dtype == MIPS_DTYPE_SQ8;
    if (doc_dtype != MIPS_DTYPE_BF16 && doc_dtype != MIPS_DTYPE_FP8_E4M3 && doc_dtype != MIPS_DTYPE_F32 && doc_dtype != MIPS_DTYPE_FP8_E4M3_DOCS && !sq8)
        return fail(MIPS_E_INVALID, "mips_index_create: index storage dtype must be BF16, FP8_E4M3, FP8_E4M3_DOCS, SQ8 or F32, got %d", doc_dtype);
    // (one-byte storages share row pitch, element size and the d limit; SQ8 is "e4m3 documents" with another element decode)
    const bool f8_storage = doc_dtype == MIPS_DTYPE_FP8_E4M3 || doc_dtype == MIPS_DTYPE_FP8_E4M3_DOCS || sq8;
    if (f8_storage && d > 1024)
        return fail(MIPS_E_UNSUPPORTED, "mips_index_create: one-byte storage (fp8 e4m3, SQ8) supports d <= 1024 in this build");
    if (sq8 && metric != MIPS_METRIC_IP)
        return fail(MIPS_E_UNSUPPORTED, "mips_index_create: an SQ8 index ranks by inner product only (the L2 rule |q|^2 + phi - 2 q.x presumes rows of "
                                        "constant norm, which decoded SQ8 rows are not)");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(MIPS_E_INVALID, "mips_index_create: no HIP device %d (have %d)", device, count);
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    // (declared behind the device guard: a failure below frees what the index holds with its device still current)
    std::unique_ptr<mips_index> ix(new (std::nothrow) mips_index());
    if (!ix) return fail(MIPS_E_NOMEM, "out of host memory");
    ix->device = device;
    ix->d = d;
    ix->esize = f8_storage ? 1 : 2;
    ix->sq8 = sq8;
    ix->mixed = doc_dtype == MIPS_DTYPE_FP8_E4M3_DOCS || sq8;
    ix->qsize = ix->mixed ? 2 : ix->esize;
    // Row pitch.  bf16: the query-stationary kernels exist for pitches of 128 .. 768 (multiples of 128) and
    // 1024, so every d <= 1024 is padded to one of those (zero columns); beyond that the generic kernel
    // takes multiples of 64.  fp8: multiples of 256 bytes.  fp32-exact: generic kernel over two planes.
    if (f8_storage) ix->ld = (int)round_up(d, 256);
    else if (doc_dtype == MIPS_DTYPE_F32 || d > 1024) ix->ld = (int)round_up(d, mips::BK);
    else ix->ld = d > 768 ? 1024 : (int)round_up(d, 128);
    if (doc_dtype == MIPS_DTYPE_F32) {
        ix->plane = ix->ld;
        ix->ld = 2 * ix->plane;
        // a pitch at which the query-stationary kernels serve pools of 32: 256 (true K' = 32 lists), 384 .. 768 (16x16x32
        // kernel, optimistic pools); 1024: K' <= 10 only
        if (d <= 1024) ix->hp = d <= 256 ? 256 : d <= 768 ? (int)round_up(d, 128) : 1024;
    }
    ix->doc_dtype = doc_dtype;
    ix->metric = metric;
    for (int e = 0; e < mips_index::kEvRing; ++e)
        if (create_event(ix->ev0[e], true) != hipSuccess || create_event(ix->ev1[e], true) != hipSuccess) return fail(MIPS_E_HIP, "hipEventCreate failed");
    if (create_event(ix->busy, false) != hipSuccess || create_event(ix->scan_done, false) != hipSuccess ||
        create_event(ix->cur.tail_done, false) != hipSuccess || create_event(ix->alt.tail_done, false) != hipSuccess)
        return fail(MIPS_E_HIP, "hipEventCreate failed");
    // the sticky scan-error word: pinned host memory the device writes to (coherent, mapped)
    if (hipHostMalloc((void**)&ix->sticky_host.p, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&ix->sticky_dev, ix->sticky_host, 0) != hipSuccess)
        return fail(MIPS_E_HIP, "hipHostMalloc for the scan-error word failed");
    for (int w = 0; w < 16; ++w) ix->sticky_host[w] = 0u; // [0] scan error, [2..3] resolve statistics of the last stream-ordered search
    *out = ix.release();
    return MIPS_OK;
}

int mips_index_destroy(mips_index_t* ix) {
    if (!ix) return MIPS_OK;
    DeviceGuard g(ix->device);
    (void)hipDeviceSynchronize();
    delete ix; // (every member that holds a device resource frees it: host_state.hpp)
    return MIPS_OK;
}

int mips_index_reserve(mips_index_t* ix, int64_t n) {
    if (!ix || n < 0) return fail(MIPS_E_INVALID, "mips_index_reserve: bad argument");
    if (n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_index_reserve: more than 2^31 rows on one GPU");
    DeviceGuard g(ix->device);
    ORDER_ON(ix, nullptr);
    return grow(ix, n, nullptr, /*exact=*/true);
}

int mips_index_add(mips_index_t* ix, const void* rows, int64_t n, int src_dtype, int src_is_device, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_add: index is NULL");
    if (n < 0 || (n > 0 && !rows)) return fail(MIPS_E_INVALID, "mips_index_add: bad rows / n");
    if (!src_dtype_ok(ix, src_dtype))
        return fail(MIPS_E_INVALID, "mips_index_add: src_dtype must be F32 or BF16 (or FP8_E4M3 bytes for an fp8 index, SQ8 codes for an SQ8 index)");
    if (ix->sq8 && !ix->sq8_trained) return fail(MIPS_E_INVALID, "mips_index_add: the SQ8 index is not trained (mips_index_sq8_train)");
    if (n == 0) return MIPS_OK;
    if (ix->ntotal + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "mips_index_add: more than 2^31 rows on one GPU");
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    int rc = grow(ix, ix->ntotal + n, st);
    if (rc) return rc;
    rc = convert_into(ix, rows, n, src_dtype, src_is_device, ix->rows + (size_t)ix->ntotal * ix->ld * ix->esize, st,
                      ix->plane > 0 ? ix->rows_f32 + (size_t)ix->ntotal * ix->plane : nullptr);
    if (rc) return rc;
    rows_changed(ix, ix->ntotal);
    ix->ntotal += n;
    return MIPS_OK;
}

int mips_index_reset(mips_index_t* ix) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_reset: index is NULL");
    ix->ntotal = 0;
    ix->nlabelled = 0;
    ix->phi_override = false;
    rows_changed(ix, 0);
    return MIPS_OK;
}

int mips_index_set_labels(mips_index_t* ix, const int32_t* labels, int64_t row0, int64_t n, int src_is_device, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_set_labels: index is NULL");
    if (row0 < 0 || n < 0 || (n > 0 && !labels) || row0 + n > ix->ntotal)
        return fail(MIPS_E_INVALID, "mips_index_set_labels: bad range [%lld, +%lld) of %lld rows", (long long)row0, (long long)n, (long long)ix->ntotal);
    if (row0 > ix->nlabelled)
        return fail(MIPS_E_INVALID, "mips_index_set_labels: row0 = %lld leaves a gap behind the %lld labelled rows", (long long)row0,
                    (long long)ix->nlabelled);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    const int64_t need = round_up(std::max(ix->capacity, ix->ntotal), mips::TM); // whole tiles: the grouped scan loads a tile's labels
    if (ix->labels_cap < need) {
        DeviceArray<int> fresh; // (swapped in below: the old storage goes with it when the block ends, behind the synchronisation)
        hipError_t e = hipMalloc((void**)&fresh.p, (size_t)need * sizeof(int));
        if (e != hipSuccess) return fail(MIPS_E_NOMEM, "hipMalloc(%zu) for the row labels failed: %s", (size_t)need * sizeof(int), hipGetErrorString(e));
        e = hipMemsetAsync(fresh, 0, (size_t)need * sizeof(int), st);
        if (e == hipSuccess && ix->nlabelled > 0)
            e = hipMemcpyAsync(fresh, ix->labels, (size_t)ix->nlabelled * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && ix->labels) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(MIPS_E_HIP, "growing the row labels to %lld rows failed: %s", (long long)need, hipGetErrorString(e));
        std::swap(ix->labels, fresh);
        ix->labels_cap = need;
    }
    HIP_TRY(hipMemcpyAsync(ix->labels + row0, labels, (size_t)n * sizeof(int), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!src_is_device) HIP_TRY(hipStreamSynchronize(st)); // the caller's array may go once the call returns
    ix->nlabelled = std::max(ix->nlabelled, row0 + n);
    return MIPS_OK;
}

int mips_index_read_labels(mips_index_t* ix, int64_t row0, int64_t n, int32_t* out_host, void* hip_stream) {
    if (!ix || row0 < 0 || n < 0 || row0 + n > ix->nlabelled || (n > 0 && !out_host))
        return fail(MIPS_E_INVALID, "mips_index_read_labels: bad range [%lld, +%lld) of %lld labelled rows", (long long)row0, (long long)n,
                    ix ? (long long)ix->nlabelled : -1LL);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    HIP_TRY(hipMemcpyAsync(out_host, ix->labels + row0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int64_t mips_index_ntotal(const mips_index_t* ix) { return ix ? ix->ntotal : -1; }
int64_t mips_index_dim(const mips_index_t* ix) { return ix ? ix->d : -1; }
int mips_index_metric(const mips_index_t* ix) { return ix ? ix->metric : -1; }

int mips_index_phi(mips_index_t* ix, double* out_phi, void* hip_stream) {
    if (!ix || !out_phi) return fail(MIPS_E_INVALID, "mips_index_phi: bad argument");
    DeviceGuard g(ix->device);
    ORDER_ON(ix, (hipStream_t)hip_stream);
    int rc = compute_phi(ix, (hipStream_t)hip_stream);
    if (rc) return rc;
    *out_phi = ix->phi;
    return MIPS_OK;
}

int mips_index_set_phi(mips_index_t* ix, double phi) {
    if (!ix || phi != phi) return fail(MIPS_E_INVALID, "mips_index_set_phi: bad argument");
    if (phi < 0.0) { // drop the override: the next mips_index_phi / L2 search recomputes the local maximum
        ix->phi_override = false;
        ix->phi_valid = false;
        return MIPS_OK;
    }
    ix->phi = phi;
    ix->phi_valid = true;
    ix->phi_override = true;
    return MIPS_OK;
}

int mips_index_read_rows(mips_index_t* ix, int64_t row0, int64_t n, void* out_host_u16, void* hip_stream) {
    if (!ix || row0 < 0 || n < 0 || row0 + n > ix->ntotal || (n > 0 && !out_host_u16))
        return fail(MIPS_E_INVALID, "mips_index_read_rows: bad range [%lld, +%lld) of %lld", (long long)row0, (long long)n,
                    ix ? (long long)ix->ntotal : -1LL);
    if (n == 0) return MIPS_OK;
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    if (ix->plane > 0) { // fp32-exact mode: the fp32 originals
        HIP_TRY(hipMemcpy2DAsync(out_host_u16, (size_t)ix->d * 4, ix->rows_f32 + (size_t)row0 * ix->plane, (size_t)ix->plane * 4,
                                 (size_t)ix->d * 4, (size_t)n, hipMemcpyDeviceToHost, st));
    } else {
        const size_t es = (size_t)ix->esize;
        HIP_TRY(hipMemcpy2DAsync(out_host_u16, (size_t)ix->d * es, ix->rows + (size_t)row0 * ix->ld * es, (size_t)ix->ld * es,
                                 (size_t)ix->d * es, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MIPS_OK;
}

int mips_index_add_synthetic(mips_index_t* ix, int64_t n, int64_t row0, uint64_t seed, int kind, void* hip_stream) {
    if (!ix || n < 0 || row0 < 0) return fail(MIPS_E_INVALID, "mips_index_add_synthetic: bad argument");
    if (kind < 0 || kind > 2) return fail(MIPS_E_INVALID, "mips_index_add_synthetic: unknown kind %d", kind);
    if (ix->sq8) return fail(MIPS_E_UNSUPPORTED, "mips_index_add_synthetic: not served on an SQ8 index (mips_synth_fill + mips_index_add)");
    if (n == 0) return MIPS_OK;
    if (ix->ntotal + n > (int64_t)0x7fffff00) return fail(MIPS_E_UNSUPPORTED, "more than 2^31 rows on one GPU");
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    int rc = grow(ix, ix->ntotal + n, st);
    if (rc) return rc;
    if (ix->plane > 0) {
        float* f32 = ix->rows_f32 + (size_t)ix->ntotal * ix->plane;
        const int64_t items = n * (ix->plane / 8);
        mips::synth_fill_kernel<<<grid_for(items, 256), 256, 0, st>>>(f32, n, (int)ix->d, ix->plane, row0, seed, kind, 1);
        mips::split_rows_kernel<float><<<grid_for(items, 256), 256, 0, st>>>(
            f32, n, (int)ix->d, ix->plane, (uint16_t*)(ix->rows + (size_t)ix->ntotal * ix->ld * 2), ix->plane, nullptr);
    } else {
        const int64_t items = n * (ix->ld / 8);
        mips::synth_fill_kernel<<<grid_for(items, 256), 256, 0, st>>>(ix->rows + (size_t)ix->ntotal * ix->ld * ix->esize, n,
                                                                      (int)ix->d, ix->ld, row0, seed, kind, ix->esize == 1 ? 2 : 0);
    }
    HIP_TRY(hipGetLastError());
    rows_changed(ix, ix->ntotal); // (as mips_index_add: a phi set from outside stays until the caller renews it)
    ix->ntotal += n;
    return MIPS_OK;
}

int mips_synth_fill(void* out_device, int64_t n, int64_t d, int64_t row0, uint64_t seed, int kind, int dtype, int device,
                    void* hip_stream) {
    if (!out_device || n < 0 || d <= 0 || d % 8 != 0)
        return fail(MIPS_E_INVALID, "mips_synth_fill: bad argument (d must be a positive multiple of 8)");
    if (kind < 0 || kind > 2) return fail(MIPS_E_INVALID, "mips_synth_fill: unknown kind %d", kind);
    if (dtype != MIPS_DTYPE_F32 && dtype != MIPS_DTYPE_BF16 && dtype != MIPS_DTYPE_FP8_E4M3)
        return fail(MIPS_E_INVALID, "mips_synth_fill: dtype must be F32, BF16 or FP8_E4M3");
    if (n == 0) return MIPS_OK;
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    const int64_t items = n * (d / 8);
    mips::synth_fill_kernel<<<grid_for(items, 256), 256, 0, (hipStream_t)hip_stream>>>(out_device, n, (int)d, (int)d, row0, seed,
                                                                                      kind, dtype == MIPS_DTYPE_F32 ? 1 : dtype == MIPS_DTYPE_FP8_E4M3 ? 2 : 0);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

} // extern "C"

namespace {

// The call value of a search over the whole index as it stands (scan_and_finish and rescan_flagged derive their nested
// launches' views from it); the staged query buffers are filled in once they are staged
SearchCall index_call(const mips_index* ix, int flags) {
    SearchCall c;
    c.rows = ix->rows;
    c.ld = ix->ld;
    c.plane = ix->plane;
    c.nsplit = ix->opt_nsplit;
    c.metric = (flags & MIPS_FORCE_IP) ? MIPS_METRIC_IP : ix->metric;
    c.margin = margin_mode(ix, (flags & MIPS_OUT_DEVICE) != 0);
    return c;
}

// What mips_search, the wide and the range search do between validating their arguments and their own work, in this order:
// make the index's device current; report an earlier device-output search on this index whose scan timed out (no
// synchronisation: the word lives in host memory) before anything new is enqueued; order the call behind the last one on
// another stream; split-tail form: take the other scratch set, so that this scan may run while the previous search's tail still
// reads its lists; whichever set is about to be used, a tail still pending on it (it reads the set's staged queries) comes
// first.  body(c, rep) is the rest of the call; it fills in the call's report, which becomes the index's when the call
// succeeds -- until then, and after an error, the index reports "unknown".
template <class Body>
int run_call(const char* who, mips_index* ix, int flags, hipStream_t st, bool split, Body body) {
    DeviceGuard g(ix->device);
    const int prev = take_scan_error(ix, who);
    if (prev) return prev;
    ORDER_ON(ix, st);
    if (split) swap_scratch_sets(ix);
    int rc = wait_for_tail(ix, st, /*both_sets=*/false);
    if (rc) return rc;
    ix->report = SearchReport();
    SearchCall c = index_call(ix, flags);
    SearchReport rep;
    rc = body(c, rep);
    if (rc == MIPS_OK) ix->report = rep;
    return rc;
}

// Host-output calls compute into the index's own device buffers (n scores and indices), copied out when the call ends
int device_outputs(mips_index* ix, bool out_dev, int64_t n, float*& d_s, int64_t*& d_i) {
    if (out_dev) return MIPS_OK;
    int rc = ix->out_s.ensure((size_t)n * sizeof(float));
    if (rc) return rc;
    rc = ix->out_i.ensure((size_t)n * sizeof(int64_t));
    if (rc) return rc;
    d_s = (float*)ix->out_s.p;
    d_i = (int64_t*)ix->out_i.p;
    return MIPS_OK;
}

// mips_search / mips_search_split behind run_call: the one-launch kernel or stage queries -> pool_policy -> scan_and_finish<K'>
int search_call(mips_index* ix, SearchCall& c, SearchReport& rep, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset,
                int flags, hipStream_t st, hipStream_t tail_st) {
    const bool out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const bool packed = (flags & MIPS_OUT_PACKED) != 0;
    const bool q_dev = (flags & MIPS_Q_DEVICE) != 0;
    const bool split = tail_st != st;
    if (packed && !out_dev) return fail(MIPS_E_INVALID, "mips_search: MIPS_OUT_PACKED requires MIPS_OUT_DEVICE");
    float* d_s = out_scores;
    int64_t* d_i = out_idx;
    int rc = device_outputs(ix, out_dev, nq * k, d_s, d_i);
    if (rc) return rc;
    if (ix->ntotal > 0 && c.metric == MIPS_METRIC_L2) {
        rc = compute_phi(ix, st);
        if (rc) return rc;
    }
    const bool certifies = call_certifies(c.margin, out_dev);
    if (ix->ntotal == 0) {
        const int64_t total = nq * k;
        mips::fill_empty_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(d_s, d_i, packed ? d_i : nullptr, total, c.metric);
        HIP_TRY(hipGetLastError());
        rep = SearchReport::all_certified();
    } else if (tiny_eligible(ix, nq, k, certifies)) {
        // the reference's own call shape (<= 16 queries, small knowledge base): one launch (tiny_search.hpp)
        const void* qd = q;
        if (!q_dev) {
            const size_t qbytes = (size_t)nq * ix->d * (q_dtype == MIPS_DTYPE_F32 ? 4 : 2);
            rc = ix->stage.ensure(qbytes);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(ix->stage.p, q, qbytes, hipMemcpyHostToDevice, st));
            qd = ix->stage.p;
        }
        rc = tiny_search(ix, c, qd, q_dtype, nq, k, k, 0, nullptr, d_s, d_i, packed, idx_offset, st, certifies, &rep.last_dev);
        if (rc) return rc;
        if (certifies) {
            // the exact pass behind the one launch (the kernel, and with it its results, live on the scan stream even in the
            // split-tail form).  Device outputs: enqueued blind, it leaves at once when nothing was flagged; host buffers and
            // "margin_check" = 2 synchronise, read the count and skip it when that is 0
            rc = resolve_flagged(ix, c, rep, nq, k, d_s, d_i, packed, idx_offset, st, /*certify_now=*/!(out_dev && c.margin == 3), /*skip_compact=*/true);
            if (rc < 0) return rc; // (kUseRescan cannot happen: <= 16 queries)
        }
    } else {
        // stage the queries: converted to the scan's operand type, zero-padded to whole query tiles; the fp32 originals of an
        // fp32-exact index next to them; the scan's shared insert bounds (8 class words per query + the error word) cleared
        const int64_t nq_pad = query_pad(ix, nq);
        const size_t row_bytes = (size_t)ix->ld * ix->qsize;
        rc = ix->cur.qbuf.ensure((size_t)nq_pad * row_bytes);
        if (rc) return rc;
        uint8_t* qb = (uint8_t*)ix->cur.qbuf.p;
        const int64_t thr_words = nq_pad * 8 + 4;
        rc = ix->cur.gthr.ensure((size_t)thr_words * sizeof(unsigned));
        if (rc) return rc;
        if (ix->plane > 0) { // fp32-exact staging has its own kernel: clear with plain memsets
            rc = ix->cur.qf32.ensure((size_t)nq_pad * ix->plane * sizeof(float));
            if (rc) return rc;
            rc = convert_into(ix, q, nq, q_dtype, q_dev, qb, st, (float*)ix->cur.qf32.p);
            if (rc) return rc;
            if (nq_pad > nq) HIP_TRY(hipMemsetAsync(qb + (size_t)nq * row_bytes, 0, (size_t)(nq_pad - nq) * row_bytes, st));
            HIP_TRY(hipMemsetAsync(ix->cur.gthr.p, 0, (size_t)thr_words * sizeof(unsigned), st));
        } else { // one launch converts the queries, zero-pads to the tile multiple and clears the bounds
            if (ix->sq8) { // (the same launch writes B_q of every query)
                rc = ix->cur.qbias.ensure((size_t)nq * sizeof(double));
                if (rc) return rc;
                c.qbias = (const double*)ix->cur.qbias.p;
            }
            rc = convert_into(ix, q, nq, q_dtype, q_dev, qb, st, nullptr, nq_pad - nq, (uint32_t*)ix->cur.gthr.p, thr_words, ix->qsize,
                              (double*)ix->cur.qbias.p);
            if (rc) return rc;
        }
        c.qbuf = ix->cur.qbuf.p;
        c.qf32 = ix->cur.qf32.p;
        const PoolPolicy pol = pool_policy(ix, nq, k, out_dev, split, c.margin);
        if (pol.fast) { // bf16(q) at the bf16 kernels' row pitch, |q - bf16 q|^2, bf16 rows and residual bound up to date
            rc = ix->qhi.ensure((size_t)nq_pad * ix->hp * 2);
            if (rc) return rc;
            rc = ix->qerr2.ensure((size_t)nq * sizeof(double));
            if (rc) return rc;
            mips::convert_rows_kernel<float><<<grid_for(nq_pad * (int64_t)(ix->hp / 8), 256), 256, 0, st>>>((const float*)ix->cur.qf32.p, nq, ix->plane,
                                                                                                           (uint16_t*)ix->qhi.p, ix->hp, nq_pad);
            mips::query_resid_kernel<<<(int)((nq + 3) / 4), 256, 0, st>>>((const float*)ix->cur.qf32.p, nq, ix->plane, (double*)ix->qerr2.p);
            HIP_TRY(hipGetLastError());
            rc = ensure_hi(ix, st);
            if (rc) return rc;
            rc = ensure_xmax2(ix, st); // (on the fp32 rows)
            if (rc) return rc;
        }
        switch (pol.kl) {
        case 8: rc = scan_and_finish<8>(ix, c, rep, pol, nq, k, d_s, d_i, packed, idx_offset, out_dev, st, tail_st, split); break;
        case 10: rc = scan_and_finish<10>(ix, c, rep, pol, nq, k, d_s, d_i, packed, idx_offset, out_dev, st, tail_st, split); break;
        case 16: rc = scan_and_finish<16>(ix, c, rep, pol, nq, k, d_s, d_i, packed, idx_offset, out_dev, st, tail_st, split); break;
        default: rc = scan_and_finish<32>(ix, c, rep, pol, nq, k, d_s, d_i, packed, idx_offset, out_dev, st, tail_st, split); break;
        }
        if (rc) return rc;
        if (ix->sq8) { // every writer of the [nq, k] scores is done on the stream of the tail: S -> D = S + B_q there
            rc = sq8_finish(c, d_s, d_i, packed, nq, k, tail_st);
            if (rc) return rc;
            if (split) HIP_TRY(hipEventRecord(ix->cur.tail_done, tail_st)); // (supersedes the record behind the re-score)
        }
    }
    if (!out_dev) {
        HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // host buffers: the stream is drained, so a timed-out scan of THIS call is known now
        const int bad = take_scan_error(ix, "mips_search");
        if (bad) return bad;
    }
    return MIPS_OK;
}

int search_impl(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx, int64_t idx_offset, int flags,
                void* hip_stream, void* tail_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_search: index is NULL");
    if (nq < 0 || k < 0) return fail(MIPS_E_INVALID, "mips_search: negative nq or k");
    if (k > MIPS_MAX_K) return fail(MIPS_E_UNSUPPORTED, "mips_search: k = %d exceeds MIPS_MAX_K = %d", k, MIPS_MAX_K);
    if (!src_dtype_ok(ix, q_dtype, true)) return fail(MIPS_E_INVALID, "mips_search: q_dtype must be F32 or BF16 (or FP8_E4M3 bytes for an all-e4m3 index)");
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!q || !out_idx || (!out_scores && !(flags & MIPS_OUT_PACKED))) return fail(MIPS_E_INVALID, "mips_search: NULL buffer");
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "mips_search: more than 2^24 queries in one call");
    const hipStream_t st = (hipStream_t)hip_stream, tail_st = (hipStream_t)tail_stream;
    return run_call("mips_search", ix, flags, st, tail_st != st, [&](SearchCall& c, SearchReport& rep) {
        return search_call(ix, c, rep, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, st, tail_st);
    });
}

// ---- The wide and the range search (and their filtered / grouped forms) validate the same way and build the same Selector
// what both serve: bf16 and fp32-exact indexes of up to 1024 columns, float32 or bf16 queries
int check_served(const char* who, const mips_index* ix, int q_dtype) {
    if (ix->sq8) return fail(MIPS_E_UNSUPPORTED, "%s: SQ8 storage is not served (bf16 and fp32-exact indexes only)", who);
    if (ix->esize == 1) return fail(MIPS_E_UNSUPPORTED, "%s: e4m3 storage is not served (bf16 and fp32-exact indexes only)", who);
    if ((ix->plane > 0 ? ix->plane : ix->ld) > 1024 || ix->d > 1024)
        return fail(MIPS_E_UNSUPPORTED, "%s: stored rows of more than 1024 columns are not served", who);
    if (q_dtype != MIPS_DTYPE_F32 && q_dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: q_dtype must be F32 or BF16", who);
    return MIPS_OK;
}
// sel_bits == NULL: the unfiltered search (sel_nbits and sel_bit0 are not looked at); q_labels == NULL: no group filter
int make_selector(const char* who, const mips_index* ix, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0,
                  const int32_t* q_labels, int grp_mode, Selector& sel) {
    if (sel_bits && (sel_bit0 < 0 || sel_nbits < 0 || sel_bit0 > sel_nbits || ix->ntotal > sel_nbits - sel_bit0))
        return fail(MIPS_E_INVALID, "%s: the selector's %lld bits from bit %lld on do not cover the index's %lld rows", who, (long long)sel_nbits,
                    (long long)sel_bit0, (long long)ix->ntotal);
    if (q_labels) {
        if (grp_mode != MIPS_GRP_EXCLUDE && grp_mode != MIPS_GRP_ONLY) return fail(MIPS_E_INVALID, "%s: grp_mode must be 0 (exclude) or 1 (only), got %d", who, grp_mode);
        if (ix->nlabelled != ix->ntotal)
            return fail(MIPS_E_INVALID, "%s: %lld of the index's %lld rows carry a label (mips_index_set_labels)", who, (long long)ix->nlabelled,
                        (long long)ix->ntotal);
    }
    sel.bits = sel_bits;
    sel.nbits = sel_nbits;
    sel.bit0 = sel_bit0;
    sel.dev = (flags & MIPS_SEL_DEVICE) != 0;
    sel.qlab = q_labels;
    sel.qlab_dev = (flags & MIPS_GRP_DEVICE) != 0;
    sel.grp_only = grp_mode == MIPS_GRP_ONLY ? 1 : 0;
    return MIPS_OK;
}

int search_wide_impl(const char* who, mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                     int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, void* hip_stream,
                     const int32_t* q_labels = nullptr, int grp_mode = 0) {
    if (!ix) return fail(MIPS_E_INVALID, "%s: index is NULL", who);
    if (nq < 0 || k < 0) return fail(MIPS_E_INVALID, "%s: negative nq or k", who);
    if (k > MIPS_MAX_K_WIDE) return fail(MIPS_E_UNSUPPORTED, "%s: k = %d exceeds MIPS_MAX_K_WIDE = %d", who, k, MIPS_MAX_K_WIDE);
    int rc = check_served(who, ix, q_dtype);
    if (rc) return rc;
    Selector sel;
    rc = make_selector(who, ix, flags, sel_bits, sel_nbits, sel_bit0, q_labels, grp_mode, sel);
    if (rc) return rc;
    if (nq == 0 || k == 0) return MIPS_OK;
    const bool out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const bool packed = (flags & MIPS_OUT_PACKED) != 0;
    if (packed && !out_dev) return fail(MIPS_E_INVALID, "%s: MIPS_OUT_PACKED requires MIPS_OUT_DEVICE", who);
    if (!q || !out_idx || (!out_scores && !packed)) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    const hipStream_t st = (hipStream_t)hip_stream;
    return run_call(who, ix, flags, st, false, [&](SearchCall& c, SearchReport& rep) {
        float* d_s = out_scores;
        int64_t* d_i = out_idx;
        int rc = device_outputs(ix, out_dev, nq * k, d_s, d_i);
        if (rc) return rc;
        if (ix->ntotal == 0) {
            const int64_t total = nq * k;
            mips::fill_empty_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(d_s, d_i, packed ? d_i : nullptr, total, c.metric);
            HIP_TRY(hipGetLastError());
            rep = SearchReport::all_certified();
        } else {
            rc = wide_search(ix, rep, q, q_dtype, nq, k, d_s, d_i, packed, idx_offset, (flags & MIPS_Q_DEVICE) != 0, sel, c.metric, st);
            if (rc) return rc;
        }
        if (!out_dev) {
            rc = ensure_nflag_host(ix);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (rep.first_dev) HIP_TRY(hipMemcpyAsync(ix->nflag_host, rep.first_dev, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (rep.first_dev) { // (the stream is drained: the flagged count is known, and every flagged query was settled)
                rep.flagged = (int64_t)ix->nflag_host[0];
                rep.rescanned = rep.settled();
            }
        }
        return (int)MIPS_OK;
    });
}

int range_search_impl(const char* who, mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t* out_lims,
                      float* out_scores, int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits,
                      int64_t sel_nbits, int64_t sel_bit0, void* hip_stream, const int32_t* q_labels = nullptr, int grp_mode = 0) {
    if (!ix) return fail(MIPS_E_INVALID, "%s: index is NULL", who);
    if (nq < 0 || cap < 0) return fail(MIPS_E_INVALID, "%s: negative nq or cap", who);
    if (flags & MIPS_OUT_PACKED) return fail(MIPS_E_INVALID, "%s: MIPS_OUT_PACKED does not apply to a CSR result", who);
    int rc = check_served(who, ix, q_dtype);
    if (rc) return rc;
    if (!out_lims || (nq > 0 && (!q || !radii)) || (cap > 0 && (!out_scores || !out_idx))) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    Selector sel;
    rc = make_selector(who, ix, flags, sel_bits, sel_nbits, sel_bit0, q_labels, grp_mode, sel);
    if (rc) return rc;
    for (int64_t j = 0; j < nq; ++j)
        if (radii[j] != radii[j]) return fail(MIPS_E_INVALID, "%s: radii[%lld] is NaN", who, (long long)j);
    const bool out_dev = (flags & MIPS_OUT_DEVICE) != 0;
    const hipStream_t st = (hipStream_t)hip_stream;
    return run_call(who, ix, flags, st, false, [&](SearchCall& c, SearchReport& rep) {
        int64_t* d_lims = out_lims;
        float* d_s = out_scores;
        int64_t* d_i = out_idx;
        int rc = device_outputs(ix, out_dev, cap, d_s, d_i);
        if (rc) return rc;
        if (!out_dev) {
            rc = ix->r_lims.ensure((size_t)(nq + 1) * sizeof(int64_t));
            if (rc) return rc;
            d_lims = (int64_t*)ix->r_lims.p;
        }
        if (nq == 0 || ix->ntotal == 0) { // no hits: every limit is 0
            HIP_TRY(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        } else {
            rc = range_search(ix, q, q_dtype, nq, radii, d_lims, d_s, d_i, cap, idx_offset, (flags & MIPS_Q_DEVICE) != 0, sel, c.metric, st);
            if (rc) return rc;
        }
        // nothing is ever uncertified: the candidates are a provable superset and the filter decides on the canonical score
        rep = SearchReport::all_certified();
        if (!out_dev) {
            HIP_TRY(hipMemcpyAsync(out_lims, d_lims, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (cap > 0) {
                HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)cap * sizeof(float), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(out_idx, d_i, (size_t)cap * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(hipStreamSynchronize(st));
        }
        return (int)MIPS_OK;
    });
}

} // namespace

extern "C" {

int mips_search(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                int64_t idx_offset, int flags, void* hip_stream) {
    return search_impl(ix, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, hip_stream, hip_stream);
}

int mips_search_split(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                      int64_t idx_offset, int flags, void* scan_stream, void* tail_stream) {
    if (!(flags & MIPS_OUT_DEVICE)) return fail(MIPS_E_INVALID, "mips_search_split: device outputs only (MIPS_OUT_DEVICE)");
    return search_impl(ix, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, scan_stream, tail_stream);
}

int mips_search_wide(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                     int64_t idx_offset, int flags, void* hip_stream) {
    return search_wide_impl("mips_search_wide", ix, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, nullptr, 0, 0, hip_stream);
}

int mips_search_wide_sel(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                         int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, void* hip_stream) {
    return search_wide_impl("mips_search_wide_sel", ix, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags, sel_bits, sel_nbits, sel_bit0,
                            hip_stream);
}

int mips_range_search(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t* out_lims, float* out_scores,
                      int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, void* hip_stream) {
    return range_search_impl("mips_range_search", ix, q, q_dtype, nq, radii, out_lims, out_scores, out_idx, cap, idx_offset, flags, nullptr, 0, 0,
                             hip_stream);
}

int mips_range_search_sel(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t* out_lims, float* out_scores,
                          int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits,
                          int64_t sel_bit0, void* hip_stream) {
    return range_search_impl("mips_range_search_sel", ix, q, q_dtype, nq, radii, out_lims, out_scores, out_idx, cap, idx_offset, flags, sel_bits,
                             sel_nbits, sel_bit0, hip_stream);
}

int mips_search_wide_grp(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, int k, float* out_scores, int64_t* out_idx,
                         int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                         int grp_mode, void* hip_stream) {
    return search_wide_impl(q_labels ? "mips_search_wide_grp" : "mips_search_wide_sel", ix, q, q_dtype, nq, k, out_scores, out_idx, idx_offset, flags,
                            sel_bits, sel_nbits, sel_bit0, hip_stream, q_labels, grp_mode);
}

int mips_range_search_grp(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t* out_lims, float* out_scores,
                          int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits,
                          int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream) {
    return range_search_impl(q_labels ? "mips_range_search_grp" : "mips_range_search_sel", ix, q, q_dtype, nq, radii, out_lims, out_scores, out_idx, cap,
                             idx_offset, flags, sel_bits, sel_nbits, sel_bit0, hip_stream, q_labels, grp_mode);
}

// mips_search_fused and, with q_labels, mips_search_fused_grp (include/mips_hip_hook.h): q_labels == nullptr is the ungrouped call,
// grp_mode and flags are not looked at then
static int search_fused_impl(const char* who, mips_index_t* ix, const void* q_device, int q_dtype, int64_t nq, int k, int normalize,
                             const int64_t* ignore_device, float* out_scores_device, int64_t* out_idx_device, int64_t idx_offset,
                             const int32_t* q_labels, int grp_mode, int flags, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "%s: index is NULL", who);
    if (nq < 0 || k < 0) return fail(MIPS_E_INVALID, "%s: negative nq or k", who);
    const int k_fetch = k + (ignore_device ? 1 : 0);
    if (k_fetch > MIPS_MAX_K) return fail(MIPS_E_UNSUPPORTED, "%s: k = %d exceeds MIPS_MAX_K = %d", who, k_fetch, MIPS_MAX_K);
    if (!src_dtype_ok(ix, q_dtype, true)) return fail(MIPS_E_INVALID, "%s: q_dtype must be F32 or BF16", who);
    if (normalize && q_dtype != MIPS_DTYPE_F32) return fail(MIPS_E_INVALID, "%s: normalize needs float32 queries", who);
    Selector sel;
    if (q_labels) { // what the wide search refuses is refused here, whichever form would serve the call
        int rc = check_served(who, ix, q_dtype);
        if (rc) return rc;
        rc = make_selector(who, ix, flags, nullptr, 0, 0, q_labels, grp_mode, sel);
        if (rc) return rc;
    }
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!q_device || !out_idx_device || !out_scores_device) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    DeviceGuard g(ix->device);
    hipStream_t st = (hipStream_t)hip_stream;
    {   // (both forms below touch the index's scratch: an earlier scan error is reported, and a call on another stream ordered,
        // before anything is enqueued)
        const int prev = take_scan_error(ix, who);
        if (prev) return prev;
    }
    ORDER_ON(ix, st);
    ix->report = SearchReport(); // (as run_call: "unknown" until a form below has succeeded)
    {
        SearchCall c = index_call(ix, MIPS_OUT_DEVICE);
        SearchReport rep;
        const bool certifies = call_certifies(c.margin, /*out_dev=*/true);
        if (tiny_eligible(ix, nq, k_fetch, certifies)) {
            if (c.metric == MIPS_METRIC_L2) {
                int rc = compute_phi(ix, st);
                if (rc) return rc;
            }
            const int* qlab_dev = nullptr; // the query labels on the device: the caller's, or a host array staged as stage_selector does
            if (q_labels) {
                qlab_dev = (const int*)q_labels;
                if (!sel.qlab_dev) {
                    int rc = ix->grp_q.ensure((size_t)nq * sizeof(int));
                    if (rc) return rc;
                    HIP_TRY(hipMemcpyAsync(ix->grp_q.p, q_labels, (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
                    qlab_dev = (const int*)ix->grp_q.p;
                }
            }
            int rc = tiny_search(ix, c, q_device, q_dtype, nq, k_fetch, k, normalize, ignore_device, out_scores_device, out_idx_device, false,
                                 idx_offset, st, certifies, &rep.last_dev, qlab_dev, sel.grp_only);
            if (rc) return rc;
            // certified: the exact pass behind the one launch ranks the hits of a flagged query and applies the same ignore
            // filter -- without a synchronisation by default (it leaves at once when nothing was flagged); "margin_check" = 2
            // synchronises to read the counts.  ("margin_check" = 4 / 0: flagged queries are counted, or not even that)
            if (certifies)
                rc = resolve_flagged(ix, c, rep, nq, k_fetch, out_scores_device, out_idx_device, false, idx_offset, st, /*certify_now=*/c.margin == 2,
                                     /*skip_compact=*/true, ignore_device, k, qlab_dev, sel.grp_only);
            if (rc < 0) return rc;
            ix->report = rep;
            return MIPS_OK;
        }
    }
    // general form: the same steps as separate launches
    const void* qsrc = q_device;
    if (normalize) { // (a buffer of its own: the searches' scratch -- qf32 / qf32b -- is rewritten by the nested call)
        const size_t qbytes = (size_t)nq * ix->d * sizeof(float);
        int rc = ix->qnorm.ensure(qbytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(ix->qnorm.p, q_device, qbytes, hipMemcpyDeviceToDevice, st));
        rc = mips_l2_normalize((float*)ix->qnorm.p, nq, ix->d, ix->device, hip_stream);
        if (rc) return rc;
        qsrc = ix->qnorm.p;
    }
    // (grouped: the wide search under the same rule -- exact like the one launch, so the two forms agree bit for bit)
    const int oflags = MIPS_Q_DEVICE | MIPS_OUT_DEVICE;
    auto nested = [&](int kk, float* os, int64_t* oi) -> int {
        if (q_labels)
            return mips_search_wide_grp(ix, qsrc, q_dtype, nq, kk, os, oi, idx_offset, oflags | (flags & MIPS_GRP_DEVICE), nullptr, 0, 0, q_labels, grp_mode,
                                        hip_stream);
        return mips_search(ix, qsrc, q_dtype, nq, kk, os, oi, idx_offset, oflags, hip_stream);
    };
    if (!ignore_device) return nested(k, out_scores_device, out_idx_device);
    int rc = ix->out_s.ensure((size_t)nq * k_fetch * sizeof(float));
    if (rc) return rc;
    rc = ix->out_i.ensure((size_t)nq * k_fetch * sizeof(int64_t));
    if (rc) return rc;
    rc = nested(k_fetch, (float*)ix->out_s.p, (int64_t*)ix->out_i.p);
    if (rc) return rc;
    return mips_filter_ignore((const float*)ix->out_s.p, (const int64_t*)ix->out_i.p, ignore_device, nq, k_fetch, k, out_scores_device,
                              out_idx_device, ix->device, hip_stream);
}

int mips_search_fused(mips_index_t* ix, const void* q_device, int q_dtype, int64_t nq, int k, int normalize, const int64_t* ignore_device,
                      float* out_scores_device, int64_t* out_idx_device, int64_t idx_offset, void* hip_stream) {
    return search_fused_impl("mips_search_fused", ix, q_device, q_dtype, nq, k, normalize, ignore_device, out_scores_device, out_idx_device, idx_offset,
                             nullptr, 0, 0, hip_stream);
}

int mips_search_fused_grp(mips_index_t* ix, const void* q_device, int q_dtype, int64_t nq, int k, int normalize, const int64_t* ignore_device,
                          float* out_scores_device, int64_t* out_idx_device, int64_t idx_offset, const int32_t* q_labels, int grp_mode, int flags,
                          void* hip_stream) {
    return search_fused_impl(q_labels ? "mips_search_fused_grp" : "mips_search_fused", ix, q_device, q_dtype, nq, k, normalize, ignore_device,
                             out_scores_device, out_idx_device, idx_offset, q_labels, grp_mode, flags, hip_stream);
}

int mips_merge_topk(const float* cand_s, const int64_t* cand_i, int64_t nq, int parts, int k, int metric, float* out_s,
                    int64_t* out_i, int device, void* hip_stream) {
    if (nq < 0 || parts <= 0 || k < 0) return fail(MIPS_E_INVALID, "mips_merge_topk: bad sizes");
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!cand_s || !cand_i || !out_s || !out_i) return fail(MIPS_E_INVALID, "mips_merge_topk: NULL buffer");
    if ((int64_t)parts * k > 65536) return fail(MIPS_E_UNSUPPORTED, "mips_merge_topk: parts * k too large");
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    mips::merge_topk_kernel<<<(int)nq, 64, 0, (hipStream_t)hip_stream>>>(cand_s, cand_i, parts * k, k, metric, out_s, out_i);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_merge_topk_packed(const int64_t* gathered, int64_t nq, int parts, int k, int metric, float* out_s,
                           int64_t* out_i, int device, void* hip_stream) {
    if (nq < 0 || parts <= 0 || k < 0) return fail(MIPS_E_INVALID, "mips_merge_topk_packed: bad sizes");
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!gathered || !out_s || !out_i) return fail(MIPS_E_INVALID, "mips_merge_topk_packed: NULL buffer");
    if ((int64_t)parts * k > 65536) return fail(MIPS_E_UNSUPPORTED, "mips_merge_topk_packed: parts * k too large");
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    mips::merge_topk_packed_kernel<<<(int)nq, 64, 0, (hipStream_t)hip_stream>>>(gathered, nq, parts, k, metric, out_s, out_i);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_merge_topk_sorted_packed(const int64_t* gathered, int64_t nq, int parts, int k, int metric, float* out_s,
                                  int64_t* out_i, int device, void* hip_stream) {
    if (nq < 0 || parts <= 0 || k < 0) return fail(MIPS_E_INVALID, "mips_merge_topk_sorted_packed: bad sizes");
    if (k > MIPS_MAX_K_WIDE) return fail(MIPS_E_UNSUPPORTED, "mips_merge_topk_sorted_packed: k = %d exceeds MIPS_MAX_K_WIDE = %d", k, MIPS_MAX_K_WIDE);
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!gathered || !out_s || !out_i) return fail(MIPS_E_INVALID, "mips_merge_topk_sorted_packed: NULL buffer");
    if ((int64_t)parts * k > 65536) return fail(MIPS_E_UNSUPPORTED, "mips_merge_topk_sorted_packed: parts * k too large");
    if (nq > INT32_MAX) return fail(MIPS_E_UNSUPPORTED, "mips_merge_topk_sorted_packed: more than 2^31 - 1 queries in one call");
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    const int c = parts * k;
    // one thread per candidate up to the largest workgroup; beyond that in strides
    const int threads = c <= 64 ? 64 : c <= 128 ? 128 : c <= 256 ? 256 : c <= 512 ? 512 : 1024;
    // the lists go to LDS while the payload of one query (16 bytes per entry) is at most 128 KiB of the CU's 160 KiB (8 x 1024:
    // the staged form is 12 bytes per entry, 96 KiB); larger merges search the L2-resident payload
    if ((size_t)c * 16 <= (128u << 10)) {
        const int lds = c * 12;
        HIP_TRY(hipFuncSetAttribute((const void*)mips::merge_topk_sorted_packed_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        mips::merge_topk_sorted_packed_kernel<true><<<(int)nq, threads, lds, (hipStream_t)hip_stream>>>(gathered, nq, parts, k, metric, out_s, out_i);
    } else {
        mips::merge_topk_sorted_packed_kernel<false><<<(int)nq, threads, 0, (hipStream_t)hip_stream>>>(gathered, nq, parts, k, metric, out_s, out_i);
    }
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_range_merge_records(const int64_t* gathered, int parts, int64_t nq, int64_t stride, int64_t* out_lims, float* out_scores,
                             int64_t* out_idx, int64_t cap, int64_t* workspace, int device, void* hip_stream) {
    return range_merge_records(gathered, parts, nq, stride, out_lims, out_scores, out_idx, cap, workspace, device, (hipStream_t)hip_stream);
}

int mips_index_remove(mips_index_t* ix, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, int flags, int64_t out_counts[2],
                      void* hip_stream) {
    if (!ix || !out_counts) return fail(MIPS_E_INVALID, "mips_index_remove: index or out_counts is NULL");
    if (sel_bit0 < 0 || sel_nbits < 0 || sel_bit0 > sel_nbits || ix->ntotal > sel_nbits - sel_bit0)
        return fail(MIPS_E_INVALID, "mips_index_remove: the bitmap's %lld bits from bit %lld on do not cover the index's %lld rows",
                    (long long)sel_nbits, (long long)sel_bit0, (long long)ix->ntotal);
    if (!sel_bits && ix->ntotal > 0) return fail(MIPS_E_INVALID, "mips_index_remove: the bitmap is NULL");
    DeviceGuard g(ix->device);
    const int prev = take_scan_error(ix, "mips_index_remove");
    if (prev) return prev;
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    return index_remove(ix, sel_bits, sel_nbits, sel_bit0, (flags & MIPS_SEL_DEVICE) != 0, out_counts, st);
}

// ---- include/mips_hip_write.h
int mips_index_update(mips_index_t* ix, const int64_t* ids, int64_t n, int64_t idx_offset, const void* rows, int src_dtype, int flags,
                      int64_t* out_updated, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_update: index is NULL");
    if (n < 0 || (n > 0 && (!ids || !rows))) return fail(MIPS_E_INVALID, "mips_index_update: bad ids / rows / n");
    if (!src_dtype_ok(ix, src_dtype))
        return fail(MIPS_E_INVALID, "mips_index_update: src_dtype must be F32 or BF16 (or FP8_E4M3 bytes for an fp8 index, SQ8 codes for an SQ8 index)");
    if (ix->sq8 && !ix->sq8_trained) return fail(MIPS_E_INVALID, "mips_index_update: the SQ8 index is not trained (mips_index_sq8_train)");
    if (!upd::count_ok(n)) return fail(MIPS_E_UNSUPPORTED, "mips_index_update: more than 2^31 - 1 positions in one call");
    DeviceGuard g(ix->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    return index_update(ix, ids, n, idx_offset, rows, src_dtype, flags, out_updated, st);
}

// ---- include/mips_hip_rows.h
int mips_index_reconstruct(mips_index_t* ix, const int64_t* ids, int64_t n, int64_t idx_offset, void* out, int out_dtype, int64_t out_ld,
                           int flags, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_reconstruct: index is NULL");
    if (n < 0 || out_ld < ix->d) return fail(MIPS_E_INVALID, "mips_index_reconstruct: n = %lld, out_ld = %lld for rows of %lld columns", (long long)n,
                                             (long long)out_ld, (long long)ix->d);
    const int raw_dtype = ix->plane > 0 ? MIPS_DTYPE_F32 : ix->esize == 2 ? MIPS_DTYPE_BF16 : ix->sq8 ? MIPS_DTYPE_SQ8 : MIPS_DTYPE_FP8_E4M3;
    if (out_dtype != MIPS_DTYPE_F32 && out_dtype != raw_dtype)
        return fail(MIPS_E_INVALID, "mips_index_reconstruct: out_dtype must be F32 (decoded) or the storage's element type %d (raw), got %d", raw_dtype,
                    out_dtype);
    if (n == 0) return MIPS_OK;
    if (!ids || !out) return fail(MIPS_E_INVALID, "mips_index_reconstruct: NULL buffer");
    DeviceGuard g(ix->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    return index_reconstruct(ix, ids, n, idx_offset, out, out_dtype, out_ld, flags, st);
}

int mips_index_gather_labels(mips_index_t* ix, const int64_t* ids, int64_t n, int64_t idx_offset, int32_t* out, int flags, void* hip_stream) {
    if (!ix || n < 0) return fail(MIPS_E_INVALID, "mips_index_gather_labels: bad argument");
    if (n == 0) return MIPS_OK;
    if (!ids || !out) return fail(MIPS_E_INVALID, "mips_index_gather_labels: NULL buffer");
    DeviceGuard g(ix->device);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    return index_gather_labels(ix, ids, n, idx_offset, out, flags, st);
}

int mips_score_subset(mips_index_t* ix, const void* q, int q_dtype, int64_t nq, const int64_t* ids, int k, float* out_scores, int64_t idx_offset,
                      int flags, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_score_subset: index is NULL");
    if (nq < 0 || k < 0) return fail(MIPS_E_INVALID, "mips_score_subset: negative nq or k");
    if (!src_dtype_ok(ix, q_dtype, true)) return fail(MIPS_E_INVALID, "mips_score_subset: q_dtype must be F32 or BF16 (or FP8_E4M3 bytes for an all-e4m3 index)");
    if (ix->sq8 && !ix->sq8_trained) return fail(MIPS_E_INVALID, "mips_score_subset: the SQ8 index is not trained (mips_index_sq8_train)");
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!q || !ids || !out_scores) return fail(MIPS_E_INVALID, "mips_score_subset: NULL buffer");
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "mips_score_subset: more than 2^24 queries in one call");
    DeviceGuard g(ix->device);
    const int prev = take_scan_error(ix, "mips_score_subset"); // (the call rewrites the searches' staged queries)
    if (prev) return prev;
    const hipStream_t st = (hipStream_t)hip_stream;
    ORDER_ON(ix, st);
    return index_score_subset(ix, q, q_dtype, nq, ids, k, out_scores, idx_offset, flags, st);
}

int mips_filter_ignore(const float* scores, const int64_t* idx, const int64_t* ignore, int64_t nq, int k_fetched, int k,
                       float* out_s, int64_t* out_i, int device, void* hip_stream) {
    if (nq < 0 || k < 0 || k_fetched < k) return fail(MIPS_E_INVALID, "mips_filter_ignore: bad sizes");
    if (nq == 0 || k == 0) return MIPS_OK;
    if (!scores || !idx || !ignore || !out_s || !out_i) return fail(MIPS_E_INVALID, "mips_filter_ignore: NULL buffer");
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    mips::filter_ignore_kernel<<<(int)((nq + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(scores, idx, ignore, nq, k_fetched,
                                                                                          k, out_s, out_i);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

static int cosine_rescore_impl(const char* who, const void* query, const void* cls, int dtype, int64_t b, int k, int64_t d,
                               float* out, int64_t mem_len, float* bias, int device, void* hip_stream) {
    if (b < 0 || k < 0 || d <= 0 || mem_len < 0) return fail(MIPS_E_INVALID, "%s: bad sizes", who);
    if (dtype != MIPS_DTYPE_F32 && dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "%s: dtype must be F32 or BF16", who);
    if (b == 0 || k == 0) return MIPS_OK;
    if (!query || !cls || !out || (mem_len > 0 && !bias)) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    const int64_t pairs = b * k;
    const int grid = (int)((pairs + 3) / 4);
    float* bias_arg = mem_len > 0 ? bias : nullptr;
    if (dtype == MIPS_DTYPE_F32)
        mips::cosine_rescore_kernel<float><<<grid, 256, 0, (hipStream_t)hip_stream>>>((const float*)query, (const float*)cls, pairs, k, (int)d, out, mem_len, bias_arg);
    else
        mips::cosine_rescore_kernel<uint16_t><<<grid, 256, 0, (hipStream_t)hip_stream>>>((const uint16_t*)query, (const uint16_t*)cls, pairs, k, (int)d, out, mem_len, bias_arg);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_cosine_rescore(const void* query, const void* cls, int dtype, int64_t b, int k, int64_t d, float* out, int device,
                        void* hip_stream) {
    return cosine_rescore_impl("mips_cosine_rescore", query, cls, dtype, b, k, d, out, 0, nullptr, device, hip_stream);
}

int mips_cosine_rescore_bias(const void* query, const void* cls, int dtype, int64_t b, int k, int64_t d, float* out,
                             int64_t memory_seq_len, float* memory_bias, int device, void* hip_stream) {
    return cosine_rescore_impl("mips_cosine_rescore_bias", query, cls, dtype, b, k, d, out, memory_seq_len, memory_bias, device,
                               hip_stream);
}

int mips_cosine_rescore_backward(const void* query, const void* cls, int dtype, int64_t b, int k, int64_t d, const float* grad_scores,
                                 const float* grad_memory_bias, int64_t memory_seq_len, float* grad_query, float* grad_cls, int device,
                                 void* hip_stream) {
    if (b < 0 || k < 0 || d <= 0 || memory_seq_len < 0) return fail(MIPS_E_INVALID, "mips_cosine_rescore_backward: bad sizes");
    if (k > 64) return fail(MIPS_E_UNSUPPORTED, "mips_cosine_rescore_backward: k = %d > 64", k);
    if (dtype != MIPS_DTYPE_F32 && dtype != MIPS_DTYPE_BF16) return fail(MIPS_E_INVALID, "mips_cosine_rescore_backward: dtype must be F32 or BF16");
    if (b == 0 || k == 0) return MIPS_OK;
    if (!query || !cls || !grad_query || !grad_cls || (!grad_scores && !grad_memory_bias))
        return fail(MIPS_E_INVALID, "mips_cosine_rescore_backward: NULL buffer");
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    const float* gb = memory_seq_len > 0 ? grad_memory_bias : nullptr;
    if (dtype == MIPS_DTYPE_F32)
        mips::cosine_rescore_bwd_kernel<float><<<(int)b, 256, 0, (hipStream_t)hip_stream>>>((const float*)query, (const float*)cls, k, (int)d, grad_scores, gb, memory_seq_len, grad_query, grad_cls);
    else
        mips::cosine_rescore_bwd_kernel<uint16_t><<<(int)b, 256, 0, (hipStream_t)hip_stream>>>((const uint16_t*)query, (const uint16_t*)cls, k, (int)d, grad_scores, gb, memory_seq_len, grad_query, grad_cls);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_l2_normalize(float* x_device, int64_t n, int64_t d, int device, void* hip_stream) {
    if (n < 0 || d <= 0 || (n > 0 && !x_device)) return fail(MIPS_E_INVALID, "mips_l2_normalize: bad argument");
    if (n == 0) return MIPS_OK;
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    mips::l2_normalize_kernel<<<(int)((n + 3) / 4), 256, 0, (hipStream_t)hip_stream>>>(x_device, n, (int)d);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_rows_max_sumsq(const float* x_device, int64_t n, int64_t d, double* out_host, int device, void* hip_stream) {
    if (n < 0 || d <= 0 || (n > 0 && !x_device) || !out_host) return fail(MIPS_E_INVALID, "mips_rows_max_sumsq: bad argument");
    *out_host = 0.0;
    if (n == 0) return MIPS_OK;
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    hipStream_t st = (hipStream_t)hip_stream;
    // one 8-byte result slot per (host thread, device), allocated once: the rebuild path calls this per build
    // (mips.py:298-304), and a hipMalloc / hipFree pair per call serialises the device
    constexpr int kMaxDev = 64;
    thread_local unsigned long long* slots[kMaxDev] = {};
    if (device < 0 || device >= kMaxDev) return fail(MIPS_E_INVALID, "mips_rows_max_sumsq: device %d out of range", device);
    if (!slots[device]) HIP_TRY(hipMalloc((void**)&slots[device], 8));
    unsigned long long* slot = slots[device];
    hipError_t e = hipMemsetAsync(slot, 0, 8, st);
    if (e == hipSuccess) {
        mips::f32_rows_max_sumsq_kernel<<<(int)std::min<int64_t>((n + 3) / 4, 256 * 16), 256, 0, st>>>(x_device, n, (int)d, slot);
        e = hipGetLastError();
    }
    unsigned long long bits = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bits, slot, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(MIPS_E_HIP, "mips_rows_max_sumsq: %s", hipGetErrorString(e));
    std::memcpy(out_host, &bits, 8);
    return MIPS_OK;
}

int mips_rows_max_sumsq_device(const float* x_device, int64_t n, int64_t d, double* acc_device, int device, void* hip_stream) {
    if (n < 0 || d <= 0 || (n > 0 && !x_device) || !acc_device) return fail(MIPS_E_INVALID, "mips_rows_max_sumsq_device: bad argument");
    if (n == 0) return MIPS_OK;
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    // (non-negative doubles order like their bit patterns: the kernel's atomicMax on the 64-bit word IS the running maximum)
    mips::f32_rows_max_sumsq_kernel<<<(int)std::min<int64_t>((n + 3) / 4, 256 * 16), 256, 0, (hipStream_t)hip_stream>>>(
        x_device, n, (int)d, (unsigned long long*)acc_device);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

int mips_index_set_param(mips_index_t* ix, const char* name, int64_t value) {
    if (!ix || !name) return fail(MIPS_E_INVALID, "mips_index_set_param: bad argument");
    const std::string n(name);
    if (n == "nsplit") ix->opt_nsplit = (int)value;
    else if (n == "qgroups") ix->opt_qgroups = (int)value;
    else if (n == "variant") {
        ix->opt_variant = (int)value;
        if (value == 5 || value == 6) ix->opt_variant = 0; // (kernels of the retired A/B build: the automatic choice answers)
    }
    else if (n == "tiny") ix->opt_tiny = value == 2 ? 2 : value != 0 ? 1 : 0; // 2: one launch, fall-back paths forced (tests)
    else if (n == "resolve") ix->opt_resolve = value < 0 ? 0 : value > 2 ? 2 : (int)value; // 2: exact pass without the MFMA pre-filter
    else if (n == "f32_fast" || n == "optimistic") { // (one switch: two-stage fp32 search and optimistic pools, include/mips_hip.h)
        if (value < 0 || value > 2) return fail(MIPS_E_INVALID, "mips_index_set_param: f32_fast / optimistic must be 0, 1 or 2");
        ix->opt_f32_fast = (int)value;
        ix->fast_skip = 0;
    } else if (n == "margin_check") {
        if (value < 0 || value > 4) return fail(MIPS_E_INVALID, "mips_index_set_param: margin_check must be 0, 1, 2, 3 or 4");
        ix->opt_margin = (int)value;
    } else if (n == "resolve_budget") {
        if (value < 0) return fail(MIPS_E_INVALID, "mips_index_set_param: resolve_budget must be >= 0");
        ix->resolve_budget = (int)std::min<int64_t>(value, mips::RESOLVE_MAX);
    } else if (n == "remove_window_rows") {
        if (value < 0 || value % mips::REM_TILE != 0 || value > (1ll << 30))
            return fail(MIPS_E_INVALID, "mips_index_set_param: remove_window_rows must be a multiple of %d (0 = automatic)", mips::REM_TILE);
        ix->opt_remove_window = value;
    } else if (n == "spin_limit") ix->opt_spin_limit = (int)std::max<int64_t>(-1, std::min<int64_t>(value, 1 << 30));
    else if (n == "sub") {
        if (value != 0)
            return fail(MIPS_E_UNSUPPORTED, "mips_index_set_param: 'sub' selected experimental kernel instances of the A/B build, "
                                            "which was retired; rebuild them from commit 29d81a6 (the last one that carries them)");
    } else return fail(MIPS_E_INVALID, "mips_index_set_param: unknown parameter '%s'", name);
    return MIPS_OK;
}

int mips_index_check_error(mips_index_t* ix, int synchronize, void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_check_error: index is NULL");
    if (synchronize) {
        DeviceGuard g(ix->device);
        HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
        for (ScratchSet* s : {&ix->cur, &ix->alt}) // split-tail searches raise the sticky word from their tail stream
            if (s->tail_pending) HIP_TRY(hipEventSynchronize(s->tail_done));
    }
    return take_scan_error(ix, "mips_index_check_error");
}

const char* mips_index_last_kernel(const mips_index_t* ix) { return ix ? ix->last_kernel : ""; }

int mips_index_margin_stats(mips_index_t* ix, int64_t* flagged, int64_t* rescanned, int64_t* unresolved, int synchronize,
                            void* hip_stream) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_index_margin_stats: index is NULL");
    SearchReport& r = ix->report;
    if (synchronize && ix->cur.tail_pending) { // a split-tail search writes its counters on the tail stream
        DeviceGuard g(ix->device);
        HIP_TRY(hipEventSynchronize(ix->cur.tail_done));
    }
    if (r.flagged < 0 && synchronize && r.last_dev != nullptr) {
        // the last search left its counts on the device (search_report.hpp): fetch the one or two words now
        DeviceGuard g(ix->device);
        unsigned n[2] = {0, 0};
        if (r.first_dev) HIP_TRY(hipMemcpyAsync(&n[0], r.first_dev, 4, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
        HIP_TRY(hipMemcpyAsync(&n[1], r.last_dev, 4, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
        r.read_back(n[0], n[1]);
    }
    if (flagged) *flagged = r.flagged;
    if (rescanned) *rescanned = r.rescanned;
    if (unresolved) *unresolved = r.unresolved;
    return MIPS_OK;
}

int mips_scan_timing(mips_index_t* ix, float* out_sum_ms, int* out_count, int reset) {
    if (!ix) return fail(MIPS_E_INVALID, "mips_scan_timing: index is NULL");
    DeviceGuard g(ix->device);
    float sum = 0.f;
    int n = 0;
    for (int t = 0; t < ix->ev_count; ++t) {
        const int slot = ((ix->ev_next - 1 - t) % mips_index::kEvRing + mips_index::kEvRing) % mips_index::kEvRing;
        float ms = 0.f;
        hipError_t e = hipEventElapsedTime(&ms, ix->ev0[slot], ix->ev1[slot]);
        if (e == hipErrorNotReady) return fail(MIPS_E_HIP, "mips_scan_timing: a scan is still running; synchronise the stream first");
        if (e != hipSuccess) return fail(MIPS_E_HIP, "hipEventElapsedTime failed: %s", hipGetErrorString(e));
        sum += ms;
        ++n;
    }
    if (out_sum_ms) *out_sum_ms = sum;
    if (out_count) *out_count = n;
    if (reset) {
        ix->ev_count = 0;
        ix->timing_armed = true;
    }
    return MIPS_OK;
}

} // extern "C"

#include "host_ivf.hpp" // the IVF index (include/mips_hip_ivf.h): its own entry points, behind everything they call
#include "host_ivf_range.hpp" // its range search (include/mips_hip_ivf_range.h)
#include "host_ivf_sharded.hpp" // its search cut at the merge, for row shards (include/mips_hip_ivf_sharded.h)
#include "host_pq.hpp" // the product-quantised index (include/mips_hip_pq.h): an object of its own
#include "host_ivfpq.hpp" // the IVF index over PQ codes (include/mips_hip_ivfpq.h): lists of the one, codes and tables of the other
#include "host_refine.hpp" // the two-stage search on PQ codes (include/mips_hip_refine.h): candidates and exact re-ranking
