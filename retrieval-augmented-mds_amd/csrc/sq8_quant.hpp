// The 8-bit scalar quantiser (faiss ScalarQuantizer QT_8bit, range statistic min/max with argument 0) as plain fp32 arithmetic,
// one text for the kernels and for host checks (tests/sq8_quant_check.cpp includes this file and nothing else of the library).
// Every operation is a single IEEE fp32 operation, rounded to nearest, and none may be contracted into a fused multiply-add
// (decode is a multiply feeding an add): under clang -- hipcc, host and device -- each helper switches contraction off for its
// own statement, which holds after inlining; any other compiler must be given -ffp-contract=off.  (HIP's __fmul_rn / __fadd_rn
// are plain operators and do not prevent it.)
//   train   vmin_j = min_i x_ij, vdiff_j = max_i x_ij - vmin_j
//   encode  t = vdiff != 0 ? (x - vmin) / vdiff : 0;  t = fminf(fmaxf(t, 0), 1);  code = (uint8_t)(int)(255 t)   (truncation)
//           NaN encodes as 0 (fmaxf returns its other operand), +inf as 255, -inf as 0, values outside the range clamp
//   decode  vmin + ((code + 0.5) / 255) vdiff
//   score   s = vdiff / 255, o = vmin + 0.5 s:  <q, decode(c)> = sum_j (q_j s_j) c_j + sum_j q_j o_j up to rounding
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SQ8_HD __host__ __device__ __forceinline__
#else
#define SQ8_HD inline
#endif
#if defined(__clang__)
#define SQ8_EXACT _Pragma("clang fp contract(off)")
#else
#define SQ8_EXACT
#endif

namespace sq8 {

SQ8_HD float mul(float a, float b) {
    SQ8_EXACT
    return a * b;
}
SQ8_HD float add(float a, float b) {
    SQ8_EXACT
    return a + b;
}
SQ8_HD float sub(float a, float b) {
    SQ8_EXACT
    return a - b;
}
SQ8_HD float div(float a, float b) { return a / b; } // (correctly rounded on the device: hipcc's default for float32 division)

SQ8_HD uint8_t encode(float x, float vmin, float vdiff) {
    float t = vdiff != 0.0f ? div(sub(x, vmin), vdiff) : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return (uint8_t)(int)mul(255.0f, t);
}
SQ8_HD float decode(uint8_t code, float vmin, float vdiff) { return add(vmin, mul(div(add((float)code, 0.5f), 255.0f), vdiff)); }
SQ8_HD float scale(float vdiff) { return div(vdiff, 255.0f); }
SQ8_HD float offset(float vmin, float vdiff) { return add(vmin, mul(0.5f, scale(vdiff))); }

} // namespace sq8
