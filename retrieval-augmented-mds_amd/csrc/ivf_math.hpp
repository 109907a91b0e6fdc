// Element-wise arithmetic of the IVF index (include/mips_hip_ivf.h), one text for the kernels and for host checks
// (tests/ivf_math_check.cpp includes this file and nothing else of the library).  Every step is one IEEE operation.  The only
// products are (double)a * (double)b of two float32 values, which are EXACT in fp64 (48 significant bits), so contracting such a
// product into the sum that follows changes nothing; fp64 division and square root are correctly rounded on host and device.
//   score      s(a, b)  = (float) sum_j (double)a_j (double)b_j, sequential in ascending j     (the project's canonical score)
//   normalise  t = sum_j (double)v_j^2 (sequential);  t == 0: v stays;  else v_j = (float)((double)v_j / sqrt(t))
//   mean       (float)(S / count), S the sequential fp64 sum of the members in ascending row order
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IVF_HD __host__ __device__ __forceinline__
#else
#define IVF_HD inline
#endif

namespace ivf {

IVF_HD double sum_step(double acc, float a, float b) { return acc + (double)a * (double)b; }

IVF_HD float score(const float* a, const float* b, int64_t d) {
    double acc = 0.0;
    for (int64_t j = 0; j < d; ++j) acc = sum_step(acc, a[j], b[j]);
    return (float)acc;
}

// in place; stride between the elements of v (1 for a row)
IVF_HD void normalise(float* v, int64_t d) {
    double t = 0.0;
    for (int64_t j = 0; j < d; ++j) t = sum_step(t, v[j], v[j]);
    if (t == 0.0) return;
    const double r = sqrt(t);
    for (int64_t j = 0; j < d; ++j) v[j] = (float)((double)v[j] / r);
}

IVF_HD float mean(double sum, int64_t count) { return (float)(sum / (double)count); }

// first row of the training set / of the initial centroid l:  floor(i n / m)
IVF_HD int64_t pick(int64_t i, int64_t n, int64_t m) { return i * n / m; }

} // namespace ivf
