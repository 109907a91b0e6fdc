// Stand-alone check of csrc/ivf_search_math.hpp -- the integer arithmetic the host and the list-scan kernel of the IVF search share
// (segments of a probed list, the number of segments, the query slice).  Built by tests/test_ivf_search_host.py with
// -fsanitize=address,undefined and run on the host: it includes that header and nothing else of the library.
//   usage: ivf_search_math_check <file>      lines "S nq p k cus" -> "S <segments> <slice>";  lines "L len S" -> the S + 1 bounds
// Before reading the file it walks a grid of sizes and checks the properties the kernel relies on; "ok <checks>" is the first line.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_search_math.hpp"

static long g_checks = 0;
#define REQUIRE(cond)                                                       \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int properties() {
    const int64_t lens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 100, 200, 2500, 4096, 1000003, ((int64_t)1 << 31) - 256};
    for (int64_t L : lens)
        for (int64_t S = 1; S <= ivf::kMaxSegments; S *= 2) {
            std::vector<int64_t> b((size_t)S + 1);
            for (int64_t s = 0; s <= S; ++s) b[(size_t)s] = ivf::seg_bound(L, s, S);
            REQUIRE(b[0] == 0 && b[(size_t)S] == L);                        // the segments cover [0, L) ...
            for (int64_t s = 0; s < S; ++s) {
                REQUIRE(b[(size_t)s] <= b[(size_t)s + 1]);                  // ... in order, without overlap ...
                REQUIRE(b[(size_t)s + 1] - b[(size_t)s] <= (L + S - 1) / S); // ... and none is longer than ceil(L / S)
            }
        }
    const int64_t cus[] = {1, 8, 64, 256, 304, 4096, 100000};
    const int64_t nqs[] = {1, 2, 8, 12, 16, 100, 1024, 4096};
    const int64_t ps[] = {1, 2, 3, 8, 29, 30, 40, 256, 1024};
    const int64_t ks[] = {1, 2, 5, 29};
    for (int64_t cu : cus)
        for (int64_t nq : nqs)
            for (int64_t p : ps)
                for (int64_t k : ks) {
                    const int64_t S = ivf::choose_segments(nq, p, k, cu);
                    REQUIRE(S >= 1 && S <= ivf::kMaxSegments && (S & (S - 1)) == 0);
                    REQUIRE(p * S * k <= ivf::kMergeLimit);                 // what the merge takes
                    // two workgroups per compute unit, unless the cap or the merge's limit stopped it
                    REQUIRE(nq * p * S >= 2 * cu || S == ivf::kMaxSegments || p * (2 * S) * k > ivf::kMergeLimit);
                    REQUIRE(S == 1 || nq * p * (S / 2) < 2 * cu);           // and no more segments than that takes
                    const int64_t ns = ivf::slice_queries(p, k);
                    REQUIRE(ns >= 1 && ns <= ivf::kSliceQueries);
                    REQUIRE(ns == 1 || p * ns * k * 16 <= ivf::kPartsBudget);
                }
    REQUIRE(ivf::choose_segments(8, 1, 2, 256) == 32);      // the reference's call at nprobe = 1: the cap
    REQUIRE(ivf::choose_segments(16, 32, 2, 256) == 1);     // enough workgroups without segments
    REQUIRE(ivf::choose_segments(1, 1024, 29, 100000) == 2); // cut by the merge's limit: 1024 * 2 * 29 <= 65536 < 1024 * 4 * 29
    return 0;
}

int main(int argc, char** argv) {
    if (properties()) return 1;
    std::printf("ok %ld\n", g_checks);
    if (argc < 2) return 0;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char tag;
    while (std::fscanf(f, " %c", &tag) == 1) {
        if (tag == 'S') {
            int64_t nq, p, k, cu;
            if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &nq, &p, &k, &cu) != 4) return 3;
            std::printf("S %d %" PRId64 "\n", ivf::choose_segments(nq, p, k, cu), ivf::slice_queries(p, k));
        } else if (tag == 'L') {
            int64_t L, S;
            if (std::fscanf(f, "%" SCNd64 " %" SCNd64, &L, &S) != 2 || S < 1 || S > ivf::kMaxSegments) return 3;
            std::printf("L");
            for (int64_t s = 0; s <= S; ++s) std::printf(" %" PRId64, ivf::seg_bound(L, s, S));
            std::printf("\n");
        } else {
            return 3;
        }
    }
    std::fclose(f);
    return 0;
}
