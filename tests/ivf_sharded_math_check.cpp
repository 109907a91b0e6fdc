// Stand-alone check of csrc/ivf_sharded_math.hpp (the payload arithmetic of the row-sharded IVF search), built by
// tests/test_ivf_sharded_host.py with -fsanitize=address,undefined and run directly.  It packs sorted part lists with the header's
// functions into heap payloads of exactly packed_words(nq, k) words (a word outside is a sanitizer report and a failed check) --
// scores of either sign, zeros of either sign, infinities, ties across parts, padding, row offsets up to 2^40 --, reads them back
// the way merge_topk_sorted_packed_kernel does (the low 32 bits of word 0, word 1 with every negative id as INT64_MAX) and merges
// them by that kernel's total order (score descending; id; part; position): the result must equal a reference sort of the union
// with global rows, cut at k, and the merge limit must hold for every (parts, k) without overflow.
//   usage: ivf_sharded_math_check [seed]      prints "ok <checks>"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_sharded_math.hpp"

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

uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
float float_of(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

struct Entry {
    float score;
    int64_t row; // global; -1: padding
};

// (score descending, row ascending, padding last): the order of the definition
bool before(const Entry& a, const Entry& b) {
    const int64_t ia = a.row < 0 ? INT64_MAX : a.row, ib = b.row < 0 ? INT64_MAX : b.row;
    return a.score > b.score || (a.score == b.score && ia < ib);
}

float draw_score(int flavour) {
    switch (flavour) {
    case 0: return (float)((int)(rnd() % 7) - 3);                       // heavy ties, both signs, +0
    case 1: return rnd() % 2 ? 0.0f : -0.0f;                            // zeros of either sign: equal scores, different bits
    case 2: return -(float)(rnd() % 1000) * 0.125f - 1.0f;              // all negative: the sign bit is set in every word
    case 3: return rnd() % 4 == 0 ? -INFINITY : (float)(rnd() % 50);    // -inf scores on real rows
    default: return (float)(rnd() % 100000) * 1e-3f - 50.0f;
    }
}

void run(int parts, int k, int64_t nq, int flavour, int64_t base) {
    CHECK(ivf::parts_fit_merge(parts, k));
    const int64_t words = ivf::packed_words(nq, k);
    CHECK(words == nq * k * 2);
    std::vector<int64_t*> payload((size_t)parts);
    std::vector<std::vector<Entry>> all((size_t)nq);
    const int64_t per = 1000;
    for (int p = 0; p < parts; ++p) {
        payload[(size_t)p] = new int64_t[(size_t)words];
        const int64_t idx_offset = base + p * per; // the part's first global row
        for (int64_t j = 0; j < nq; ++j) {
            // the part's local result: have <= k distinct local rows, sorted by the definition's order, then padding
            const int have = flavour == 3 && p == parts - 1 ? 0 : (int)(rnd() % (uint32_t)(k + 1));
            std::vector<Entry> loc;
            for (int t = 0; t < have; ++t) loc.push_back({draw_score(flavour), (int64_t)(rnd() % 20) + 20 * t}); // distinct local rows < 1000 for k <= 50
            std::sort(loc.begin(), loc.end(), before);
            for (int t = 0; t < k; ++t) {
                const int64_t w = ivf::packed_entry(j, k, t);
                CHECK(w >= 0 && w + 1 < words);
                const Entry e = t < have ? loc[(size_t)t] : Entry{-INFINITY, -1};
                payload[(size_t)p][w] = ivf::packed_score_word(bits_of(e.score));
                payload[(size_t)p][w + 1] = ivf::packed_row_word(e.row, idx_offset);
                CHECK(payload[(size_t)p][w] >= 0 && (payload[(size_t)p][w] >> 32) == 0);        // zero-extended: no sign smear
                CHECK(ivf::packed_score_bits(payload[(size_t)p][w]) == bits_of(e.score));       // the bits come back, -0.0 included
                CHECK(payload[(size_t)p][w + 1] == (e.row < 0 ? -1 : e.row + idx_offset));      // padding: the offset not added
                if (t < have) all[(size_t)j].push_back({e.score, e.row + idx_offset});
            }
        }
    }
    for (int64_t j = 0; j < nq; ++j) {
        // the merge as merge_topk_sorted_packed_kernel ranks: every candidate's rank by (key, id, part, position)
        std::vector<Entry> out((size_t)k, Entry{NAN, -99});
        std::vector<char> taken((size_t)k, 0);
        const int c = parts * k;
        for (int a = 0; a < c; ++a) {
            const int pa = a / k;
            const int64_t* ea = payload[(size_t)pa] + ivf::packed_entry(j, k, a % k);
            const float sa = float_of((uint32_t)ea[0]);
            const int64_t ia = ea[1] < 0 ? INT64_MAX : ea[1];
            int rank = 0;
            for (int b = 0; b < c; ++b) {
                const int pb = b / k;
                const int64_t* eb = payload[(size_t)pb] + ivf::packed_entry(j, k, b % k);
                const float sb = float_of((uint32_t)eb[0]);
                const int64_t ib = eb[1] < 0 ? INT64_MAX : eb[1];
                rank += (sb > sa || (sb == sa && (ib < ia || (ib == ia && b < a)))) ? 1 : 0;
            }
            if (rank < k) {
                CHECK(!taken[(size_t)rank]); // every rank once
                taken[(size_t)rank] = 1;
                out[(size_t)rank] = {sa, ea[1]};
            }
        }
        std::vector<Entry>& want = all[(size_t)j];
        std::stable_sort(want.begin(), want.end(), before);
        for (int t = 0; t < k; ++t) {
            CHECK(taken[(size_t)t]);
            if (t < (int)want.size()) {
                CHECK(out[(size_t)t].row == want[(size_t)t].row && out[(size_t)t].score == want[(size_t)t].score);
            } else CHECK(out[(size_t)t].row == -1 && out[(size_t)t].score == -INFINITY); // padding survives the merge, last
        }
    }
    for (int p = 0; p < parts; ++p) delete[] payload[(size_t)p];
}

} // namespace

int main(int argc, char** argv) {
    rng_state = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    // the merge limit: parts * k <= 65536, for any int parts without overflow
    for (int k = 1; k <= ivf::kPartsMaxK; ++k) {
        const int most = (int)(ivf::kPartsMergeLimit / k);
        CHECK(ivf::parts_fit_merge(most, k) && !ivf::parts_fit_merge(most + 1, k));
        CHECK(!ivf::parts_fit_merge(INT_MAX, k));
    }
    CHECK(ivf::parts_fit_merge(64, 1024) && !ivf::parts_fit_merge(65, 1024) && ivf::parts_fit_merge(65536, 1));
    // words and entries: no 32-bit overflow at the largest shapes
    CHECK(ivf::packed_words((int64_t)1 << 24, 1024) == ((int64_t)1 << 35));
    CHECK(ivf::packed_entry(((int64_t)1 << 24) - 1, 1024, 1023) == ((int64_t)1 << 35) - 2);
    // rows: offsets past 2^31 and 2^40, padding and the poison id pass through
    CHECK(ivf::packed_row_word(0x7ffffeff, (int64_t)1 << 40) == ((int64_t)1 << 40) + 0x7ffffeff);
    CHECK(ivf::packed_row_word(-1, (int64_t)1 << 40) == -1 && ivf::packed_row_word(-2, 12345) == -2 && ivf::packed_row_word(0, 0) == 0);
    // every class of float bits round-trips through word 0
    const uint32_t specials[] = {0u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x00000001u, 0x80000001u, 0x7f7fffffu, 0xff7fffffu};
    for (uint32_t u : specials) CHECK(ivf::packed_score_bits(ivf::packed_score_word(u)) == u && ivf::packed_score_word(u) == (int64_t)(uint64_t)u);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t u = rnd() ^ (rnd() << 16);
        CHECK(ivf::packed_score_bits(ivf::packed_score_word(u)) == u && (ivf::packed_score_word(u) >> 32) == 0);
    }
    for (int parts : {1, 2, 3, 8})
        for (int k : {1, 5, 29, 30, 50})
            for (int flavour = 0; flavour < 5; ++flavour)
                for (int64_t base : {(int64_t)0, (int64_t)1 << 31, (int64_t)1 << 40}) run(parts, k, 3, flavour, base);
    std::printf("ok %lld\n", checks);
    return 0;
}
