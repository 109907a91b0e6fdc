// Stand-alone check of csrc/ivf_math.hpp (the text the IVF kernels compile), built with -fsanitize=address,undefined and run as its
// own process by tests/test_ivf_host.py.  Properties are checked here; normalise / score / mean of the vectors in the input file
// are printed as bit patterns for the test to compare with the NumPy restatement (tests/ivf_cases.py).
//   input:  "n d" then n * d float32 bit patterns (hex);  output: "ok <checks>" then n lines of d normalised bit patterns, one line of
//           n - 1 scores s(row i, row i + 1), one line of d means over all rows
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_math.hpp"

static uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float bits_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static long checks = 0;
#define REQUIRE(c)                                                  \
    do {                                                            \
        ++checks;                                                   \
        if (!(c)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);     \
            return 1;                                               \
        }                                                           \
    } while (0)

int main(int argc, char** argv) {
    // the evenly spaced pick
    REQUIRE(ivf::pick(0, 1000, 10) == 0 && ivf::pick(9, 1000, 10) == 900 && ivf::pick(2, 7, 3) == 4);
    REQUIRE(ivf::pick((int64_t)1 << 23, (int64_t)1 << 31, (int64_t)1 << 24) == ((int64_t)1 << 30)); // (no 32-bit overflow)
    // normalise: a zero vector stays, a unit vector stays, the result has norm 1 up to rounding
    float z[5] = {0, 0, 0, 0, 0}, u[5] = {0, 0, -1, 0, 0}, w[5] = {3, 4, 0, -12, 1e-30f};
    ivf::normalise(z, 5);
    ivf::normalise(u, 5);
    ivf::normalise(w, 5);
    for (int j = 0; j < 5; ++j) REQUIRE(z[j] == 0.0f && u[j] == (j == 2 ? -1.0f : 0.0f));
    REQUIRE(w[0] == (float)(3.0 / 13.0) && w[3] == (float)(-12.0 / 13.0) && std::fabs(ivf::score(w, w, 5) - 1.0f) < 1e-6f);
    REQUIRE(ivf::mean(10.0, 4) == 2.5f && ivf::mean(1.0, 3) == (float)(1.0 / 3.0));
    if (argc < 2) {
        std::printf("ok %ld\n", checks);
        return 0;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long n = 0, d = 0;
    if (std::fscanf(f, "%ld %ld", &n, &d) != 2 || n < 2 || d < 1) return 2;
    std::vector<float> x((size_t)n * d);
    for (size_t t = 0; t < x.size(); ++t) {
        unsigned bits = 0;
        if (std::fscanf(f, "%x", &bits) != 1) return 2;
        x[t] = bits_float(bits);
    }
    std::fclose(f);
    std::printf("ok %ld\n", checks);
    std::vector<float> v((size_t)d);
    for (long i = 0; i < n; ++i) {
        for (long j = 0; j < d; ++j) v[(size_t)j] = x[(size_t)(i * d + j)];
        ivf::normalise(v.data(), d);
        for (long j = 0; j < d; ++j) std::printf("%08x ", float_bits(v[(size_t)j]));
        std::printf("\n");
    }
    for (long i = 0; i + 1 < n; ++i) std::printf("%08x ", float_bits(ivf::score(&x[(size_t)(i * d)], &x[(size_t)((i + 1) * d)], d)));
    std::printf("\n");
    for (long j = 0; j < d; ++j) {
        double s = 0.0;
        for (long i = 0; i < n; ++i) s += (double)x[(size_t)(i * d + j)];
        std::printf("%08x ", float_bits(ivf::mean(s, n)));
    }
    std::printf("\n");
    return 0;
}
