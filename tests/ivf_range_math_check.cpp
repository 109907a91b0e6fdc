// Stand-alone check of csrc/ivf_range_math.hpp (every index of the range search over the probed lists that addresses the staging
// buffer, the caller's arrays or a sort partner), built by tests/test_ivf_range_host.py with -fsanitize=address,undefined and run
// directly.  It plays the launches of csrc/ivf_range_kernels.hpp on the host with every index taken from the header and every buffer
// a heap array of EXACTLY the size the library allocates (a slot outside it is a sanitizer report and a failed check):
//   staging  waves of 64 lanes with random hit masks reserve blocks behind a cursor and write records of `cap` slots; the cursor and
//            the per-query counts go on past the capacity;
//   lims     the prefix sum of the counts;
//   place    min(cursor, cap) records go to lims[j] + a per-query cursor of arrays of `cap` entries;
//   order    every stretch [lims[j], min(lims[j + 1], cap)) is sorted by the network -- a stage reads all its pairs before the next
//            begins, every entry is in at most one pair of a stage, every partner lies above its lower index --
// for capacities of 0, the total - 1, the total and more, and for stretch lengths 0 .. 600 and around every size class up to
// kRangeSortLds + 1 and beyond.  With cap >= total the result must be every query's hits in ascending row order.
//   usage: ivf_range_math_check [seed]      prints "ok <checks>"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_range_math.hpp"

namespace {

long long checks = 0;

#define CHECK(c)                                                            \
    do {                                                                    \
        ++checks;                                                           \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

uint64_t rng_state = 1;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// the ordering step on a stretch of n entries that live in a heap array of exactly n entries
void order(int64_t* rows, float* vals, int64_t n) {
    const int64_t P = ivf::range_sort_class(n);
    CHECK(P >= n && (P & (P - 1)) == 0 && (P == 1 || P / 2 < n));
    CHECK(ivf::range_sort_in_lds(n) == (n <= ivf::kRangeSortLds));
    std::vector<char> touched;
    for (int64_t k = 2; k <= P; k <<= 1)
        for (int64_t j = k >> 1; j >= 1; j >>= 1) {
            touched.assign((size_t)n, 0);
            for (int64_t t = 0; t < (P >> 1); ++t) {
                const int64_t i = ivf::bitonic_lower(t, j), u = ivf::bitonic_partner(i, k, j);
                CHECK(i >= 0 && i < P && u > i && u < P && (i & j) == 0 && (i / k) == (u / k));
                if (u >= n) continue; // the padding of the full network: never moves
                CHECK(!touched[(size_t)i] && !touched[(size_t)u]);
                touched[(size_t)i] = touched[(size_t)u] = 1;
                if (rows[u] < rows[i]) {
                    std::swap(rows[u], rows[i]);
                    std::swap(vals[u], vals[i]);
                }
            }
        }
}

void check_order(int64_t n) {
    int64_t* rows = new int64_t[(size_t)n];
    float* vals = new float[(size_t)n];
    std::vector<int64_t> want((size_t)n);
    for (int64_t i = 0; i < n; ++i) want[(size_t)i] = (int64_t)(rnd() % 4u) + 4 * i; // distinct
    for (int64_t i = n - 1; i > 0; --i) std::swap(want[(size_t)i], want[(size_t)(rnd() % (uint32_t)(i + 1))]);
    for (int64_t i = 0; i < n; ++i) rows[i] = want[(size_t)i], vals[i] = (float)want[(size_t)i] * 0.5f;
    if (n > 0) order(rows, vals, n);
    std::sort(want.begin(), want.end());
    for (int64_t i = 0; i < n; ++i) CHECK(rows[i] == want[(size_t)i] && vals[i] == (float)rows[i] * 0.5f);
    delete[] rows;
    delete[] vals;
}

// one whole call: nq queries, `waves` wave passes with random hit masks, a capacity
void check_call(int nq, int waves, int64_t cap, int density) {
    int* stage_q = new int[(size_t)cap];
    int* stage_r = new int[(size_t)cap];
    float* stage_s = new float[(size_t)cap];
    float* out_s = new float[(size_t)cap];
    int64_t* out_i = new int64_t[(size_t)cap];
    for (int64_t e = 0; e < cap; ++e) out_i[e] = -777, out_s[e] = -1.f;
    std::vector<int> qcnt((size_t)nq, 0), qcur((size_t)nq, 0);
    std::vector<std::vector<int>> truth((size_t)nq);
    uint64_t cursor = 0;
    int next_row = 1 << 20;
    for (int w = 0; w < waves; ++w) {
        const int j = (int)(rnd() % (uint32_t)nq);
        uint64_t mask = 0;
        for (int lane = 0; lane < 64; ++lane)
            if ((int)(rnd() % 100u) < density) mask |= (uint64_t)1 << lane;
        if (mask == 0) continue;
        const uint64_t base = cursor; // lane 0's atomic add
        cursor += (uint64_t)__builtin_popcountll(mask);
        qcnt[(size_t)j] += __builtin_popcountll(mask);
        uint64_t prev = base;
        for (int lane = 0; lane < 64; ++lane) {
            if (!((mask >> lane) & 1)) continue;
            const uint64_t slot = ivf::range_slot(base, mask, lane);
            CHECK(slot >= base && slot < cursor && (lane == __builtin_ctzll(mask) ? slot == base : slot == prev + 1));
            prev = slot;
            const int row = next_row - 3 * (w * 64 + lane); // rows arrive in descending order: the order step has work to do
            truth[(size_t)j].push_back(row);
            if (ivf::range_keeps(slot, cap)) {
                CHECK(slot < (uint64_t)cap);
                stage_q[slot] = j, stage_r[slot] = row, stage_s[slot] = (float)row;
            }
        }
    }
    std::vector<int64_t> lims((size_t)nq + 1, 0);
    for (int j = 0; j < nq; ++j) lims[(size_t)j + 1] = lims[(size_t)j] + qcnt[(size_t)j];
    const int64_t total = lims[(size_t)nq];
    CHECK((uint64_t)total == cursor);
    const uint64_t staged = ivf::range_staged(cursor, cap);
    CHECK(staged <= (uint64_t)cap && staged <= cursor && (staged == cursor || staged == (uint64_t)cap));
    for (uint64_t e = 0; e < staged; ++e) {
        const int j = stage_q[e];
        const int c = qcur[(size_t)j]++;
        const int64_t dst = ivf::range_place_slot(lims[(size_t)j], c, cap);
        CHECK(dst == -1 || (dst >= lims[(size_t)j] && dst < lims[(size_t)j + 1] && dst < cap));
        if (dst >= 0) out_s[dst] = stage_s[e], out_i[dst] = stage_r[e];
    }
    for (int j = 0; j < nq; ++j) {
        const int64_t n = ivf::range_stretch(lims[(size_t)j], lims[(size_t)j + 1], cap);
        CHECK(n >= 0 && n <= qcnt[(size_t)j] && (n == 0 || lims[(size_t)j] + n <= cap));
        if (n == 0) continue;
        // the stretch as a heap array of its own: nothing of the network may leave it
        int64_t* rows = new int64_t[(size_t)n];
        float* vals = new float[(size_t)n];
        for (int64_t i = 0; i < n; ++i) rows[i] = out_i[lims[(size_t)j] + i], vals[i] = out_s[lims[(size_t)j] + i];
        order(rows, vals, n);
        for (int64_t i = 1; i < n; ++i) CHECK(rows[i - 1] <= rows[i]);
        if (total <= cap) {
            std::vector<int>& t = truth[(size_t)j];
            std::sort(t.begin(), t.end());
            CHECK((int64_t)t.size() == n);
            for (int64_t i = 0; i < n; ++i) CHECK(rows[i] == t[(size_t)i] && vals[i] == (float)t[(size_t)i]);
        }
        delete[] rows;
        delete[] vals;
    }
    delete[] stage_q;
    delete[] stage_r;
    delete[] stage_s;
    delete[] out_s;
    delete[] out_i;
}

} // namespace

int main(int argc, char** argv) {
    rng_state = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    for (int64_t n = 0; n <= 600; ++n) check_order(n);
    for (int64_t P = 1024; P <= 2 * ivf::kRangeSortLds; P *= 2)
        for (int64_t n = P - 1; n <= P + 1; ++n) check_order(n);
    check_order(3 * ivf::kRangeSortLds + 17);
    CHECK(ivf::range_sort_in_lds(ivf::kRangeSortLds) && !ivf::range_sort_in_lds(ivf::kRangeSortLds + 1));
    CHECK(ivf::range_sort_class(1) == 1 && ivf::range_sort_class(2) == 2 && ivf::range_sort_class(3) == 4 && ivf::range_sort_class(4097) == 8192);
    CHECK(ivf::range_place_slot(5, 0, 5) == -1 && ivf::range_place_slot(4, 0, 5) == 4 && ivf::range_stretch(3, 9, 5) == 2 && ivf::range_stretch(7, 9, 5) == 0);
    CHECK(!ivf::range_keeps(0, 0) && ivf::range_keeps(4, 5) && !ivf::range_keeps(5, 5) && ivf::range_staged(9, 5) == 5 && ivf::range_staged(3, 5) == 3);
    for (int round = 0; round < 40; ++round) {
        const int nq = 1 + (int)(rnd() % 9u), waves = (int)(rnd() % 120u), density = (int)(rnd() % 101u);
        // the total of this round, found by a dry run with the same random stream
        const uint64_t keep = rng_state;
        uint64_t total = 0;
        {
            for (int w = 0; w < waves; ++w) {
                (void)rnd();
                for (int lane = 0; lane < 64; ++lane) total += (int)(rnd() % 100u) < density;
            }
        }
        const int64_t caps[5] = {0, (int64_t)total > 0 ? (int64_t)total - 1 : 0, (int64_t)total, (int64_t)total + 1 + (int64_t)(rnd() % 50u), (int64_t)(total / 2)};
        const uint64_t after = rng_state;
        for (int64_t cap : caps) {
            rng_state = keep;
            check_call(nq, waves, cap, density);
        }
        rng_state = after;
    }
    std::printf("ok %lld\n", checks);
    return 0;
}
