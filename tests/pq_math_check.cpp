// Stand-alone check of csrc/pq_math.hpp (the text the PQ kernels and their host side compile), built with
// -fsanitize=address,undefined and run as its own process by tests/test_pq_host.py.  Properties are checked here; codes, tables and
// scores of the vectors in the input file are printed for the test to compare with the NumPy restatement (tests/pq_cases.py).
//   input:  "M dsub n nq" then float32 bit patterns (hex): the codebook [M][256][dsub], n rows [n][M dsub], nq queries
//   output: "ok <checks>", one line of n * M codes, nq lines of M * 256 table entries (bits), nq lines of n scores (bits)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/pq_math.hpp"

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
    REQUIRE(pq::pick(0, 1000, 10) == 0 && pq::pick(9, 1000, 10) == 900 && pq::pick(2, 7, 3) == 4);
    REQUIRE(pq::pick(65535, (int64_t)0x7fffff00, 65536) == (int64_t)65535 * 0x7fffff00 / 65536); // (no 32-bit overflow)
    REQUIRE(pq::mean(10.0, 4) == 2.5f && pq::mean(1.0, 3) == (float)(1.0 / 3.0));
    // nearest: strict, so ties stay with the lowest centroid and a NaN never wins
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    REQUIRE(pq::closer(1.0, 2.0) && !pq::closer(2.0, 2.0) && !pq::closer(nan, 2.0) && !pq::closer(1.0, nan) && !pq::closer(inf, inf));
    {
        std::vector<float> cb((size_t)pq::kSub * 2, 5.0f); // every centroid equal: code 0
        const float x[2] = {1.0f, 2.0f}, bad[2] = {NAN, 1.0f}, far[2] = {INFINITY, INFINITY};
        REQUIRE(pq::nearest(x, cb.data(), 2) == 0 && pq::nearest(bad, cb.data(), 2) == 0 && pq::nearest(far, cb.data(), 2) == 0);
        cb[2 * 200] = 1.0f, cb[2 * 200 + 1] = 2.0f;
        cb[2 * 201] = 1.0f, cb[2 * 201 + 1] = 2.0f; // 200 and 201 tie at distance 0
        REQUIRE(pq::nearest(x, cb.data(), 2) == 200);
        REQUIRE(pq::dist(x, cb.data(), 2) == 16.0 + 9.0);
    }
    // the float32 difference of the distance: 2^70 - 11 is 2^70 as float32
    REQUIRE(pq::dist_step(0.0, 0x1p70f, 11.0f) == 0x1p140);
    // the score sums in float32, in ascending m: (2^24 + 1) + 1 loses the first 1, 1 + 1 + 2^24 does not
    {
        std::vector<float> lut((size_t)3 * pq::kSub, 0.0f);
        lut[7] = 0x1p24f, lut[pq::kSub + 255] = 1.0f, lut[2 * pq::kSub + 0] = 1.0f;
        const uint8_t code[3] = {7, 255, 0};
        REQUIRE(pq::adc(lut.data(), code, 3) == 0x1p24f + 1.0f && pq::adc(lut.data(), code, 3) != 16777218.0f);
        lut[7] = -0.0f;
        REQUIRE(float_bits(pq::adc(lut.data(), code, 1)) == 0x80000000u); // the first entry as it is, not 0 + entry
    }
    // the launch arithmetic
    REQUIRE(pq::code_pitch(1) == 16 && pq::code_pitch(16) == 16 && pq::code_pitch(17) == 32 && pq::code_pitch(96) == 96 && pq::code_pitch(128) == 128);
    for (int M = 1; M <= pq::kMaxM; ++M) {
        REQUIRE(pq::scan_lds_bytes(M) <= ((int64_t)160 << 10));
        REQUIRE(pq::scan_waves(M) == 4 || pq::scan_waves(M) == 16);
        REQUIRE(pq::scan_blocks_per_cu(M) >= 1 && pq::scan_blocks_per_cu(M) * pq::scan_lds_bytes(M) <= ((int64_t)160 << 10));
        REQUIRE(pq::scan_blocks_per_cu(M) * pq::scan_waves(M) <= 32);
    }
    REQUIRE(pq::scan_blocks_per_cu(128) == 1 && pq::scan_blocks_per_cu(81) == 1 && pq::scan_blocks_per_cu(4) == 8);
    const int64_t ns_[] = {1, 3, 8, 17, 256, 4096}, n_[] = {0, 1, 63, 64, 65, 1000, 4097, (int64_t)1 << 24, (int64_t)0x7fffff00};
    for (int64_t ns : ns_)
        for (int64_t n : n_)
            for (int k : {1, 5, 29})
                for (int M : {1, 4, 32, 33, 96, 128}) {
                    const int S = pq::choose_segments(ns, k, M, n, 256);
                    REQUIRE(S >= 1 && (int64_t)S * k <= pq::kMergeLimit && ns * S <= (int64_t)4096 * 65536);
                    REQUIRE(S == 1 || (n + S - 1) / S >= 64 * pq::scan_waves(M) / 2); // no crowd of nearly empty segments
                    REQUIRE(pq::seg_bound(n, 0, S) == 0 && pq::seg_bound(n, S, S) == n);
                    for (int s = 0; s < S; s += (S > 64 ? S / 7 : 1)) {
                        const int64_t lo = pq::seg_bound(n, s, S), hi = pq::seg_bound(n, s + 1, S);
                        REQUIRE(0 <= lo && lo <= hi && hi <= n && hi - lo <= (n + S - 1) / S);
                    }
                }
    REQUIRE(pq::choose_segments(8, 5, 96, (int64_t)1 << 24, 256) == 64 && pq::choose_segments(3, 5, 4, 4097, 256) == 17);
    if (argc < 2) {
        std::printf("ok %ld\n", checks);
        return 0;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long M = 0, dsub = 0, n = 0, nq = 0;
    if (std::fscanf(f, "%ld %ld %ld %ld", &M, &dsub, &n, &nq) != 4 || M < 1 || M > pq::kMaxM || dsub < 1 || n < 1 || nq < 1) return 2;
    const long d = M * dsub;
    std::vector<float> cb((size_t)M * pq::kSub * dsub), x((size_t)n * d), q((size_t)nq * d);
    for (std::vector<float>* v : {&cb, &x, &q})
        for (size_t t = 0; t < v->size(); ++t) {
            unsigned bits = 0;
            if (std::fscanf(f, "%x", &bits) != 1) return 2;
            (*v)[t] = bits_float(bits);
        }
    std::fclose(f);
    std::printf("ok %ld\n", checks);
    std::vector<uint8_t> codes((size_t)n * M);
    for (long i = 0; i < n; ++i)
        for (long m = 0; m < M; ++m) {
            codes[(size_t)(i * M + m)] = (uint8_t)pq::nearest(&x[(size_t)(i * d + m * dsub)], &cb[(size_t)(m * pq::kSub * dsub)], (int)dsub);
            std::printf("%d ", (int)codes[(size_t)(i * M + m)]);
        }
    std::printf("\n");
    std::vector<float> lut((size_t)nq * M * pq::kSub);
    for (long j = 0; j < nq; ++j) {
        for (long mc = 0; mc < M * pq::kSub; ++mc) {
            lut[(size_t)(j * M * pq::kSub + mc)] = pq::score(&q[(size_t)(j * d + (mc / pq::kSub) * dsub)], &cb[(size_t)(mc * dsub)], dsub);
            std::printf("%08x ", float_bits(lut[(size_t)(j * M * pq::kSub + mc)]));
        }
        std::printf("\n");
    }
    for (long j = 0; j < nq; ++j) {
        for (long i = 0; i < n; ++i) std::printf("%08x ", float_bits(pq::adc(&lut[(size_t)(j * M * pq::kSub)], &codes[(size_t)(i * M)], (int)M)));
        std::printf("\n");
    }
    return 0;
}
