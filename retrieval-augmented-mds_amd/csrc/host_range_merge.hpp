// Host side of mips_range_merge_records (included by mips_hip.hip behind host_range.hpp): argument checks and the two launches of
// range_merge_kernels.hpp.  No index handle, no scratch of the library's own: the caller brings the workspace.  Everything is
// enqueued on the caller's stream and nothing synchronises.
#pragma once

namespace {

int range_merge_records(const int64_t* gathered, int parts, int64_t nq, int64_t stride, int64_t* out_lims, float* out_scores, int64_t* out_idx,
                        int64_t cap, int64_t* workspace, int device, hipStream_t st) {
    const char* who = "mips_range_merge_records";
    if (parts < 1) return fail(MIPS_E_INVALID, "%s: parts = %d", who, parts);
    if (nq < 0 || stride < 0 || cap < 0) return fail(MIPS_E_INVALID, "%s: negative nq, stride or cap", who);
    if (!gathered || !out_lims || (cap > 0 && (!out_scores || !out_idx)) || (nq > 0 && !workspace)) return fail(MIPS_E_INVALID, "%s: NULL buffer", who);
    if (nq > (1 << 24)) return fail(MIPS_E_UNSUPPORTED, "%s: more than 2^24 queries in one call", who);
    if (parts > 65535) return fail(MIPS_E_UNSUPPORTED, "%s: more than 65535 parts", who); // (the copy's gridDim.y)
    DeviceGuard g(device);
    if (!g.ok) return fail(MIPS_E_HIP, "hipSetDevice(%d) failed", device);
    if (nq == 0) {
        HIP_TRY(hipMemsetAsync(out_lims, 0, sizeof(int64_t), st));
        return MIPS_OK;
    }
    mips::RangeMergeArgs a;
    a.gathered = gathered;
    a.parts = parts;
    a.nq = (int)nq;
    a.stride = stride;
    a.W = MIPS_RANGE_RECORD_WORDS(nq, stride);
    a.out_lims = out_lims;
    a.out_s = out_scores;
    a.out_i = out_idx;
    a.cap = cap;
    a.base = workspace;
    constexpr int T = mips::RANGE_MERGE_THREADS;
    mips::range_merge_lims_kernel<<<(int)((nq + 1 + T - 1) / T), T, 0, st>>>(a);
    if (cap > 0 && stride > 0) {
        // the parts' totals are device data: the grid covers the payload's capacity, a workgroup past a part's entries leaves at once
        constexpr int64_t per_block = (int64_t)(T / 64) * mips::RANGE_MERGE_SPAN;
        const int64_t blocks = std::min<int64_t>((stride + per_block - 1) / per_block, mips::RANGE_MERGE_MAX_BLOCKS);
        mips::range_merge_copy_kernel<<<dim3((unsigned)blocks, (unsigned)parts), T, 0, st>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

} // namespace
