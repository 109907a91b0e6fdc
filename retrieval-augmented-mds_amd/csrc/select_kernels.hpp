// Row selectors (mips_search_wide_sel / mips_range_search_sel): the caller's bitmap in the FAISS IDSelectorBitmap layout (row i is
// selected iff bits[i >> 3] >> (i & 7) & 1), staged once per call into the form the kernels read.
//
//   selector_stage_kernel   words[w] bit b = caller's bit bit0 + 32 w + b for LOCAL rows 32 w + b < ntotal, 0 for every other bit
//                           of the nwords = 4 * (128-row tiles) words: the masked scan reads the four words of a tile whole and the
//                           ragged last tile needs no test of its own.  The popcount of the words is summed into *nsel (zeroed
//                           before the launch); the certificate of the wide search reads it on the device.  bits == nullptr
//                           stages "every row": what a grouped call without a bitmap scans under.
//   label_pad_kernel        the staged per-query labels of a grouped call (mips_search_wide_grp / mips_range_search_grp) behind the
//                           caller's nq: MIPS_LABEL_NONE up to the next whole query tile (pad queries never append anyway)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mips {

constexpr int SEL_THREADS = 256;

// bits: the caller's bytes, nbytes of them (bytes past that are never read); bit0 >= 0 and bit0 + ntotal <= 8 * nbytes;
// or nullptr: all rows selected
// word w of the staged form (shared with the removal's staging, remove_kernels.hpp)
__device__ inline unsigned selector_word(const uint8_t* bits, int64_t nbytes, int64_t bit0, int64_t ntotal, int64_t w) {
    const int64_t left = ntotal - 32 * w; // rows of this word that exist
    unsigned v = 0u;
    if (left > 0) {
        const int64_t b = bit0 + 32 * w;
        const int64_t byte0 = b >> 3;
        const int sh = (int)(b & 7);
        unsigned long long acc = bits == nullptr ? ~0ull : 0ull;
        if (bits != nullptr) {
#pragma unroll
            for (int i = 0; i < 5; ++i)
                if (byte0 + i < nbytes) acc |= (unsigned long long)bits[byte0 + i] << (8 * i);
        }
        v = (unsigned)(acc >> sh);
        if (left < 32) v &= (1u << (int)left) - 1u;
    }
    return v;
}

__global__ __launch_bounds__(SEL_THREADS) void selector_stage_kernel(const uint8_t* bits, int64_t nbytes, int64_t bit0, int64_t ntotal,
                                                                     unsigned* words, int64_t nwords, unsigned long long* nsel) {
    unsigned long long mine = 0ull;
    for (int64_t w = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * SEL_THREADS) {
        const unsigned v = selector_word(bits, nbytes, bit0, ntotal, w);
        words[w] = v;
        mine += (unsigned long long)__popc(v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine != 0ull) atomicAdd(nsel, mine);
}

__global__ void label_pad_kernel(int* qlab, int64_t nq, int64_t nq_pad) {
    const int64_t i = nq + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq_pad) qlab[i] = -2147483647 - 1;
}

} // namespace mips
