// Stand-alone check of csrc/sq8_quant.hpp (the text the kernels compile): built by tests/test_sq8_host.py with
// -ffp-contract=off -fsanitize=address,undefined and run on the CPU.  Prints "ok <checks>" and returns 0, or says what failed.
//   sq8_quant_check [file]   file: lines "x vmin vdiff" as float32 bit patterns (hex); the codes are printed one per line behind
//                            the "ok" line, so the test can compare them with the NumPy restatement
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/sq8_quant.hpp"

static long checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        ++checks;                         \
        if (!(cond)) {                    \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");   \
            return 1;                     \
        }                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() { // splitmix64 -> [0, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

int main(int argc, char** argv) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float ranges[][2] = {{0.0f, 1.0f}, {-1.0f, 2.0f}, {-3.5f, 0.001f}, {100.0f, 0.25f}, {-1e-3f, 2e-3f}, {1e6f, 1e4f}, {-0.37f, 7.77f}};
    for (const auto& r : ranges) {
        const float vmin = r[0], vdiff = r[1], vmax = vmin + vdiff;
        // the clamps, the ends of the range, NaN and the infinities
        CHECK(sq8::encode(vmin, vmin, vdiff) == 0, "vmin does not encode as 0");
        CHECK(sq8::encode(vmax, vmin, vdiff) == 255 || vmax - vmin != vdiff, "vmin + vdiff does not encode as 255");
        CHECK(sq8::encode(vmin - 10.0f * vdiff - 1.0f, vmin, vdiff) == 0, "below the range: no clamp to 0");
        CHECK(sq8::encode(vmax + 10.0f * vdiff + 1.0f, vmin, vdiff) == 255, "above the range: no clamp to 255");
        CHECK(sq8::encode(nan, vmin, vdiff) == 0, "NaN does not encode as 0");
        CHECK(sq8::encode(inf, vmin, vdiff) == 255, "+inf does not encode as 255");
        CHECK(sq8::encode(-inf, vmin, vdiff) == 0, "-inf does not encode as 0");
        // round trip and monotonicity over the range (and a little beyond)
        int prev = -1;
        float prev_x = -inf;
        for (int i = 0; i <= 20000; ++i) {
            const float x = vmin + (float)((i / 20000.0) * 1.2 - 0.1) * vdiff;
            if (x < prev_x) continue; // (float rounding of the sweep itself)
            const int c = sq8::encode(x, vmin, vdiff);
            CHECK(c >= 0 && c <= 255, "code %d outside 0 .. 255", c);
            CHECK(c >= prev, "encode is not monotone: %d after %d at x = %a", c, prev, x);
            prev = c, prev_x = x;
            if (x >= vmin && x <= vmax) {
                const float back = sq8::decode((uint8_t)c, vmin, vdiff);
                // half a level (vdiff / 510) plus one ulp of the largest magnitude in the range (the float32 roundings of encode
                // and decode); the top of the range (t = 1 -> 255) decodes half a level above it
                const float top = std::fmax(std::fabs(vmin), std::fabs(vmax));
                const float ulp = std::nextafter(top, inf) - top;
                CHECK(std::fabs(back - x) <= vdiff / 510.0f + ulp, "round trip error %g > %g at x = %a (vmin %g vdiff %g)", std::fabs(back - x),
                      vdiff / 510.0f + ulp, x, vmin, vdiff);
            }
        }
        // (int)(255 t) never exceeds 255 (a 256 would wrap to code 0): just below the top of the range the code is 254 or 255
        for (int i = 0; i < 20000; ++i) {
            const float x = vmax - (float)(uniform() * 1e-5) * vdiff;
            const int c = sq8::encode(x, vmin, vdiff);
            CHECK(c == 254 || c == 255, "code %d near the top of the range", c);
        }
    }
    // vdiff = 0: every value encodes as 0 and decodes as vmin
    for (float x : {-1.0f, 0.0f, 3.0f, inf, -inf, nan}) {
        CHECK(sq8::encode(x, 3.0f, 0.0f) == 0, "vdiff = 0: code is not 0");
    }
    CHECK(sq8::decode(0, 3.0f, 0.0f) == 3.0f, "vdiff = 0: decode is not vmin");
    // every code decodes into its own level
    for (int c = 0; c < 256; ++c) {
        CHECK(sq8::encode(sq8::decode((uint8_t)c, -0.37f, 7.77f), -0.37f, 7.77f) == c, "decode(%d) does not encode back", c);
    }
    // s and o: decode(c) = o + c s up to rounding
    for (int c = 0; c < 256; ++c) {
        const float s = sq8::scale(7.77f), o = sq8::offset(-0.37f, 7.77f);
        CHECK(std::fabs((o + c * s) - sq8::decode((uint8_t)c, -0.37f, 7.77f)) <= 4e-6f, "o + c s differs from decode(%d)", c);
    }
    std::vector<int> codes;
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "r");
        CHECK(f != nullptr, "cannot open %s", argv[1]);
        unsigned bx, bm, bd;
        while (std::fscanf(f, "%x %x %x", &bx, &bm, &bd) == 3) {
            float x, vmin, vdiff;
            std::memcpy(&x, &bx, 4), std::memcpy(&vmin, &bm, 4), std::memcpy(&vdiff, &bd, 4);
            codes.push_back(sq8::encode(x, vmin, vdiff));
        }
        std::fclose(f);
    }
    std::printf("ok %ld\n", checks);
    for (int c : codes) std::printf("%d\n", c);
    return 0;
}
