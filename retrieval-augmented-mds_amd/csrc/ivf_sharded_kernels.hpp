// Kernel of the part search of a row-sharded IVF index (include/mips_hip_ivf_sharded.h: mips_ivf_search_part).
//
//   ivf_part_pack_kernel   behind the merge of a part's p * S partial lists, in the place of ivf_finish_kernel, over [nq][k]: the
//                          merged (score, row) pairs leave as the payload int64 [nq][k][2] that merge_topk_sorted_packed_kernel
//                          reads -- the score's bits AS THEY ARE (an SQ8 part hands over S; the bias is applied once, behind the
//                          merge of the parts, by ivf_finish_kernel), the row with idx_offset added, padding (-inf, -1) unchanged.
//                          The packed tail of the inner merge and the offset half of the finishing pass read the same [nq][k]
//                          entries, so they are one pass and one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_sharded_math.hpp"

namespace mips {

__global__ void ivf_part_pack_kernel(const float* s, const int64_t* id, int64_t nq, int k, int64_t idx_offset, int64_t* out_packed) {
    const int64_t total = nq * k;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t w = ivf::packed_entry(t / k, k, (int)(t % k));
        out_packed[w] = ivf::packed_score_word(__float_as_uint(s[t]));
        out_packed[w + 1] = ivf::packed_row_word(id[t], idx_offset);
    }
}

} // namespace mips
