// Stand-alone check of csrc/adc_wide_math.hpp (the text the candidate scans and the re-ranking select compile), built by
// tests/test_refine_host.py with -fsanitize=address,undefined.  It includes that header and, through it, ivfpq_math.hpp and
// ivf_wide_math.hpp -- nothing else of the library.  Prints "ok <checks>" and, for the table of DESIGN.md 4n, the pools of a few shapes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/adc_wide_math.hpp"

static long checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main() {
    const int KPS[3] = {64, 256, 1024};
    const int PS[4] = {0, 1, 8, 1024}; // 0: the flat scan
    // ---- the LDS rule: every (M, KP, p) is served within 160 KiB
    for (int M = 1; M <= pq::kMaxM; ++M)
        for (int KP : KPS)
            for (int p : PS) {
                const int P = adcw::pools(M, KP, p), W = adcw::waves(M, KP, p);
                const int64_t lds = adcw::lds_bytes(M, KP, p);
                CHECK(lds <= 163840 && adcw::kLdsBudget == 163840);
                CHECK(P >= 1 && P <= adcw::kMaxPools && P <= pq::scan_waves(M));
                CHECK(W >= P && 64 * W <= 1024);
                CHECK(lds == (int64_t)M * 1024 + 64 + (p > 0 ? (3 * (int64_t)p + 1) * 4 : 0) + (int64_t)P * KP * 8);
                // one more pool would not fit (or the base scan has no more waves)
                CHECK(P == pq::scan_waves(M) || lds + adcw::pool_bytes(KP) > adcw::kLdsBudget);
                CHECK(adcw::blocks_per_cu(M, KP, p) >= 1 && adcw::blocks_per_cu(M, KP, p) * lds <= std::max<int64_t>(lds, adcw::kLdsBudget));
                for (int k : {KP == 64 ? 30 : KP == 256 ? 65 : 257, KP})
                    for (int64_t ns : {1, 3, 256, 4096})
                        for (int64_t rows : {0, 1, 5000, 1 << 20})
                            for (int64_t forced : {0, 1, 2, 7, 64, 65536}) {
                                CHECK(ivf::pool_class(k) == KP);
                                const int S = adcw::choose_segments(ns, k, M, p, rows, 256, forced);
                                CHECK(S >= 1 && (int64_t)S * k <= 65536);
                                if (forced > 0 && forced * k <= 65536) CHECK(S == forced);
                                if (k == 1024) CHECK(S <= 64);
                            }
            }
    // the worst case of the issue: M = 128, KP = 1024, p = 1024 -> two pools
    CHECK(adcw::fixed_bytes(128, 1024) == 131072 + 12292 + 64);
    CHECK(adcw::pools(128, 1024, 1024) == 2 && adcw::pools(128, 1024, 0) == 3 && adcw::pools(128, 64, 1024) == 16);
    CHECK(adcw::pools(96, 1024, 0) == 7 && adcw::pools(96, 256, 0) == 16 && adcw::pools(4, 1024, 1024) == 4 && adcw::pools(32, 1024, 1024) == 4);

    // ---- the final rank over ANY number of pools: a permutation of [0, total)
    std::mt19937 rng(7);
    for (int P : {1, 2, 3, 4, 5, 7, 16})
        for (int KP : {64, 256})
            for (int rep = 0; rep < 4; ++rep) {
                std::vector<float> pk((size_t)P * KP, 0.f);
                std::vector<int> pr((size_t)P * KP, 0), cnt(P);
                int row = 0, total = 0;
                std::vector<std::pair<float, int>> all;
                for (int w = 0; w < P; ++w) {
                    cnt[w] = rep == 0 ? KP : (int)(rng() % (KP + 1));
                    std::vector<std::pair<float, int>> e;
                    for (int u = 0; u < cnt[w]; ++u) e.push_back({(float)(rng() % 7), row += 1 + (int)(rng() % 3)}); // few keys: ties
                    std::shuffle(e.begin(), e.end(), rng);
                    std::sort(e.begin(), e.end(), [](auto& a, auto& b) { return ivf::wide_before(a.first, a.second, b.first, b.second); });
                    for (int u = 0; u < cnt[w]; ++u) {
                        pk[(size_t)w * KP + u] = e[u].first;
                        pr[(size_t)w * KP + u] = e[u].second;
                        all.push_back(e[u]);
                    }
                    total += cnt[w];
                }
                std::sort(all.begin(), all.end(), [](auto& a, auto& b) { return ivf::wide_before(a.first, a.second, b.first, b.second); });
                std::vector<int> hit(total, 0);
                for (int e = 0; e < P * KP; ++e) {
                    const int w = adcw::rank_pool(e, KP), u = adcw::rank_slot(e, KP);
                    CHECK(w >= 0 && w < P && u >= 0 && u < KP && w * KP + u == e);
                    if (u >= cnt[w]) continue;
                    const int r = adcw::union_rank(pk.data(), pr.data(), cnt.data(), P, KP, w, u, total + 1);
                    CHECK(r >= 0 && r < total);
                    CHECK(all[r].first == pk[e] && all[r].second == pr[e]);
                    ++hit[r];
                    const int stop = total / 2;
                    const int r2 = adcw::union_rank(pk.data(), pr.data(), cnt.data(), P, KP, w, u, stop);
                    CHECK(r < stop ? r2 == r : r2 >= stop); // (an early stop never moves a rank below the stop)
                }
                for (int r = 0; r < total; ++r) CHECK(hit[r] == 1);
            }

    // ---- the re-ranking select
    const int64_t MIN64 = INT64_MIN, MAX64 = INT64_MAX;
    CHECK(adcw::rerank_valid(0, 0, 1) && !adcw::rerank_valid(1, 0, 1) && !adcw::rerank_valid(-1, 0, 1) && !adcw::rerank_valid(0, 0, 0));
    CHECK(adcw::rerank_valid(7, 7, 1) && !adcw::rerank_valid(6, 7, 1) && adcw::rerank_valid(-3, -5, 3) && !adcw::rerank_valid(-2, -5, 3));
    CHECK(!adcw::rerank_valid(MIN64, 0, 100) && !adcw::rerank_valid(MIN64, 5, 100) && !adcw::rerank_valid(MAX64, 0, MAX64) && !adcw::rerank_valid(MAX64, -5, 100));
    CHECK(adcw::rerank_valid(MAX64 - 1, MAX64 - 1, 1) && !adcw::rerank_valid(((int64_t)1 << 32) + 3, 0, 100) && adcw::rerank_valid(MIN64 + 1, MIN64, 2));
    CHECK(adcw::rerank_before(1.f, 5, 0.f, 1) && adcw::rerank_before(1.f, 1, 1.f, 5) && !adcw::rerank_before(1.f, 5, 1.f, 5) && adcw::rerank_before(-0.f, 1, 0.f, 2));
    CHECK(adcw::rerank_before(-INFINITY, 5, -INFINITY, adcw::kNoId)); // a row that scores -inf still ranks before what is no row
    for (int kc : {1, 2, 63, 64, 65, 1000, 1024}) {
        // the select, restated on the host with the header's functions, against a std::sort of the set
        std::vector<float> sk(1024);
        std::vector<int64_t> si(1024);
        const int n = ivf::sort_span(kc, adcw::kRerankMax);
        CHECK(n >= kc && n <= 1024 && (n & (n - 1)) == 0);
        std::vector<std::pair<float, int64_t>> want;
        for (int u = 0; u < n; ++u) {
            const int64_t id = u < kc ? (int64_t)(rng() % 40) - 4 : adcw::kNoId; // repeats, and ids that name no row
            const bool ok = u < kc && adcw::rerank_valid(id, 0, 30);
            sk[u] = ok ? (float)(id % 5) : -INFINITY; // (equal ids carry equal scores)
            si[u] = ok ? id : adcw::kNoId;
            if (ok && std::find(want.begin(), want.end(), std::make_pair(sk[u], id)) == want.end()) want.push_back({sk[u], id});
        }
        for (int size = 2; size <= n; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1)
                for (int t = 0; t < n / 2; ++t) {
                    const int lo = ivf::bitonic_low(t, stride), hi = ivf::bitonic_high(t, stride);
                    CHECK(lo >= 0 && hi < n && hi == lo + stride);
                    const bool swap = ivf::bitonic_best_low(lo, size) ? adcw::rerank_before(sk[hi], si[hi], sk[lo], si[lo])
                                                                      : adcw::rerank_before(sk[lo], si[lo], sk[hi], si[hi]);
                    if (swap) {
                        std::swap(sk[lo], sk[hi]);
                        std::swap(si[lo], si[hi]);
                    }
                }
        std::sort(want.begin(), want.end(), [](auto& a, auto& b) { return adcw::rerank_before(a.first, a.second, b.first, b.second); });
        size_t pos = 0;
        for (int u = 0; u < n; ++u) {
            if (!adcw::rerank_keep(si.data(), u)) continue;
            CHECK(pos < want.size() && want[pos].first == sk[u] && want[pos].second == si[u]);
            ++pos;
        }
        CHECK(pos == want.size());
    }
    std::printf("ok %ld\n", checks);
    for (int M : {4, 32, 40, 96, 128})
        for (int KP : KPS)
            for (int p : {0, 1024})
                std::printf("M %d KP %d p %d pools %d lds %lld blocks %d\n", M, KP, p, adcw::pools(M, KP, p), (long long)adcw::lds_bytes(M, KP, p),
                            adcw::blocks_per_cu(M, KP, p));
    return 0;
}
