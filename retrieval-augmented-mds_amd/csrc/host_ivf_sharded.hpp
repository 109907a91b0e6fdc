// Host side of the row-sharded IVF search (include/mips_hip_ivf_sharded.h; the kernel: ivf_sharded_kernels.hpp).  Included behind
// host_ivf.hpp.  The part search is ivf_search_impl with an IvfPartOut: the launches of mips_ivf_search_wide_grp with the packing
// pass in the place of the finishing pass.  The merge of the parts takes no index: the gathered payload, B_q and the outputs are
// the caller's, so nothing passes from one call to the other through an object.
#pragma once

static_assert(ivf::kPartsMergeLimit == ivf::kMergeLimit, "the merge of the parts and the merge of the partial lists are one merge");
static_assert(ivf::kPartsMaxK == MIPS_MAX_K_WIDE, "ivf_sharded_math.hpp restates MIPS_MAX_K_WIDE");

extern "C" {

int mips_ivf_search_part(mips_ivf_t* v, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, int64_t* out_packed, double* out_bias,
                         int64_t idx_offset, int flags, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels,
                         int grp_mode, void* hip_stream) {
    const IvfPartOut part{out_packed, out_bias};
    return ivf_search_impl("mips_ivf_search_part", true, v, q, q_dtype, nq, k, nprobe, nullptr, nullptr, idx_offset, flags, sel_bits, sel_nbits, sel_bit0,
                           q_labels, grp_mode, hip_stream, &part);
}

int mips_ivf_merge_parts(const int64_t* gathered, int parts, int64_t nq, int k, const double* bias, float* out_scores, int64_t* out_idx, int device,
                         void* hip_stream) {
    if (parts < 1 || nq < 0 || k < 1) return fail(MIPS_E_INVALID, "mips_ivf_merge_parts: bad sizes (parts %d, nq %lld, k %d)", parts, (long long)nq, k);
    if (k > MIPS_MAX_K_WIDE) return fail(MIPS_E_UNSUPPORTED, "mips_ivf_merge_parts: k = %d exceeds MIPS_MAX_K_WIDE = %d", k, MIPS_MAX_K_WIDE);
    if (!ivf::parts_fit_merge(parts, k))
        return fail(MIPS_E_UNSUPPORTED, "mips_ivf_merge_parts: parts * k = %d * %d exceeds %lld, the entries per query the merge takes", parts, k,
                    (long long)ivf::kPartsMergeLimit);
    if (nq == 0) return MIPS_OK;
    if (!gathered || !out_scores || !out_idx) return fail(MIPS_E_INVALID, "mips_ivf_merge_parts: NULL buffer");
    int rc = mips_merge_topk_sorted_packed(gathered, nq, parts, k, MIPS_METRIC_IP, out_scores, out_idx, device, hip_stream);
    if (rc || !bias) return rc;
    DeviceGuard g(device);
    mips::ivf_finish_kernel<<<grid_for(nq * k, 256), 256, 0, (hipStream_t)hip_stream>>>(out_scores, out_idx, bias, nq, k, 0);
    HIP_TRY(hipGetLastError());
    return MIPS_OK;
}

} // extern "C"
