// Stand-alone check of csrc/ivf_filter_math.hpp -- the admission rule and the queue bookkeeping of the filtered list scan of the IVF
// search.  Built by tests/test_ivf_filter_host.py with -fsanitize=address,undefined and run on the host: it includes that header
// and nothing else of the library.  The queue is walked as a wave walks it -- window by window, every lane's slot from the ballot
// mask, a pass whenever 64 rows are queued, one more for the remainder -- into an array of exactly kQueueSlots entries, so a slot
// outside it is an AddressSanitizer report.
//   usage: ivf_filter_math_check [seed]      prints "ok <checks>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_filter_math.hpp"

static long g_checks = 0;
#define REQUIRE(cond)                                                       \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static uint64_t g_state = 1;
static uint64_t next_u64() { // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int rule() {
    const int32_t none = ivf::kLabelNone;
    const int32_t labs[] = {none, -1, 0, 1, 7, INT32_MAX};
    for (int32_t a : labs)
        for (int32_t b : labs) {
            REQUIRE(ivf::group_admits(a, b, ivf::kGrpExclude) == (b == none || a != b));
            REQUIRE(ivf::group_admits(a, b, ivf::kGrpOnly) == (b == none || a == b));
        }
    REQUIRE(ivf::group_admits(none, none, ivf::kGrpOnly) && ivf::group_admits(none, none, ivf::kGrpExclude)); // no rule at all
    std::vector<uint8_t> bits(37);
    for (auto& b : bits) b = (uint8_t)next_u64();
    for (int64_t t = 0; t < (int64_t)bits.size() * 8; ++t) REQUIRE(ivf::bit_is_set(bits.data(), t) == (((bits[(size_t)(t / 8)] >> (t % 8)) & 1) == 1));
    return 0;
}

// one wave's walk over `windows` ballot masks; `density` of 256 is every lane
static int walk(int windows, int density) {
    std::vector<int> queue((size_t)ivf::kQueueSlots, -1), scored, want;
    int queued = 0, row = 0;
    for (int w = 0; w < windows; ++w) {
        uint64_t mask = 0;
        for (int lane = 0; lane < 64; ++lane)
            if ((int)(next_u64() & 255) < density) mask |= (uint64_t)1 << lane;
        REQUIRE(queued >= 0 && queued < ivf::kQueuePass); // between windows
        for (int lane = 0; lane < 64; ++lane, ++row)
            if ((mask >> lane) & 1) {
                const int slot = ivf::queue_slot(queued, mask, lane);
                REQUIRE(slot >= queued && slot < ivf::kQueueSlots - 1);
                queue[(size_t)slot] = row;
                want.push_back(row);
            }
        queued = ivf::queue_after_append(queued, mask);
        REQUIRE(queued < ivf::kQueueSlots);
        if (ivf::queue_has_pass(queued)) {
            for (int lane = 0; lane < ivf::kQueuePass; ++lane) scored.push_back(queue[(size_t)lane]);
            const int left = ivf::queue_after_pass(queued);
            for (int lane = 0; lane < left; ++lane) queue[(size_t)lane] = queue[(size_t)(ivf::kQueuePass + lane)];
            queued = left;
        }
    }
    for (int lane = 0; lane < queued; ++lane) scored.push_back(queue[(size_t)lane]); // the remainder
    REQUIRE(scored == want); // every admitted row once, in list order
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) g_state = std::strtoull(argv[1], nullptr, 10);
    if (rule()) return 1;
    const int densities[] = {0, 1, 4, 16, 128, 255, 256};
    const int lengths[] = {0, 1, 2, 3, 79, 313};
    for (int rep = 0; rep < 20; ++rep)
        for (int den : densities)
            for (int len : lengths)
                if (walk(len, den)) return 1;
    REQUIRE(ivf::queue_slot(63, ~(uint64_t)0, 63) == 126); // the furthest slot an append reaches
    REQUIRE(ivf::queue_after_append(63, ~(uint64_t)0) == 127 && ivf::queue_after_pass(127) == 63);
    std::printf("ok %ld\n", g_checks);
    return 0;
}
