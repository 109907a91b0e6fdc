// Stand-alone check of csrc/ivf_wide_math.hpp (the pool arithmetic of the wide IVF list scan), built by tests/test_ivf_wide_host.py
// with -fsanitize=address,undefined and run directly.  It walks a wave of 64 lanes in lock step through the steps of
// ivf_score_pool / ivf_pool_sort / the final ranking of csrc/ivf_wide_kernels.hpp -- fill, sort, threshold, insert, final -- with
// every pool index taken from the header, on pools that are heap arrays of exactly KP entries (a slot >= KP is a sanitizer report and
// a failed check), for k in {1, 29, 30, 63, 64, 65, 255, 256, 257, 1023, 1024} and streams of 0, 1, k - 1, k, k + 1 and 3 k
// candidates with tied keys, -inf keys and rows in no order.  After every pass the pool must equal the first k of the reference
// sort by (key descending, row ascending) of everything seen so far.
//   usage: ivf_wide_math_check [seed]      prints "ok <checks>"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/ivf_wide_math.hpp"

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

struct Cand {
    float key;
    int row;
};

bool before(const Cand& a, const Cand& b) { return ivf::wide_before(a.key, a.row, b.key, b.row); }

uint64_t rng_state = 1;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// a wave's pool: exactly KP entries on the heap
struct Pool {
    int KP, k, cnt = 0;
    float* pk;
    int* pr;
    Pool(int k_) : KP(ivf::pool_class(k_)), k(k_), pk(new float[KP]), pr(new int[KP]) {
        for (int u = 0; u < KP; ++u) pk[u] = NAN, pr[u] = -12345; // garbage: nothing may depend on it
    }
    ~Pool() {
        delete[] pk;
        delete[] pr;
    }
    int slot(int u) const {
        CHECK(u >= 0 && u < KP);
        return u;
    }
};

// ivf_pool_sort, lanes in lock step: every stage reads all its pairs before the next stage begins
void pool_sort(Pool& p) {
    const int n = ivf::sort_span(p.cnt, p.KP);
    CHECK(n >= 2 && n <= p.KP && n >= p.cnt && (n & (n - 1)) == 0 && (n == 2 || n / 2 < p.cnt || n == p.KP));
    for (int lane = 0; lane < ivf::kWideLanes; ++lane)
        for (int u = p.cnt + lane; u < n; u += ivf::kWideLanes) p.pk[p.slot(u)] = -INFINITY, p.pr[p.slot(u)] = ivf::kNoRow;
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            std::vector<char> touched((size_t)n, 0);
            for (int lane = 0; lane < ivf::kWideLanes; ++lane)
                for (int t = lane; t < n / 2; t += ivf::kWideLanes) {
                    const int lo = p.slot(ivf::bitonic_low(t, stride)), hi = p.slot(ivf::bitonic_high(t, stride));
                    CHECK(lo < hi && hi < n && !touched[lo] && !touched[hi]); // the pairs of a stage are disjoint
                    touched[lo] = touched[hi] = 1;
                    const float ka = p.pk[lo], kb = p.pk[hi];
                    const int ra = p.pr[lo], rb = p.pr[hi];
                    const bool swap = ivf::bitonic_best_low(lo, size) ? ivf::wide_before(kb, rb, ka, ra) : ivf::wide_before(ka, ra, kb, rb);
                    if (swap) p.pk[lo] = kb, p.pr[lo] = rb, p.pk[hi] = ka, p.pr[hi] = ra;
                }
            for (int u = 0; u < n; ++u) CHECK(touched[u]);
        }
    for (int u = 0; u + 1 < n; ++u) CHECK(!ivf::wide_before(p.pk[u + 1], p.pr[u + 1], p.pk[u], p.pr[u]));
    for (int u = p.cnt; u < n; ++u) CHECK(p.pr[u] == ivf::kNoRow); // padding last
}

// ivf_score_pool behind the scoring: the lanes of `valid` carry (key[lane], row[lane])
void pool_pass(Pool& p, const float* key, const int* row, uint64_t valid) {
    uint64_t m = valid;
    const int K = p.k;
    if (p.cnt < K) {
        const int take = ivf::fill_take(p.cnt, K, m);
        uint64_t rest = 0;
        int written = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int s = ivf::fill_slot(p.cnt, K, m, lane);
            if (s >= 0) {
                CHECK(s >= p.cnt && s < K && s == p.cnt + written); // lane order, no gap
                p.pk[p.slot(s)] = key[lane];
                p.pr[p.slot(s)] = row[lane];
                ++written;
            } else if ((m >> lane) & 1) rest |= (uint64_t)1 << lane;
        }
        CHECK(written == take && take + __builtin_popcountll(rest) == __builtin_popcountll(m));
        p.cnt += take;
        m = rest;
        if (p.cnt < K) {
            CHECK(m == 0);
            return;
        }
        pool_sort(p);
    }
    const int ts = p.slot(ivf::threshold_slot(K));
    float tk = p.pk[ts];
    int tr = p.pr[ts];
    uint64_t in = 0;
    for (int lane = 0; lane < 64; ++lane)
        if (((m >> lane) & 1) && ivf::wide_before(key[lane], row[lane], tk, tr)) in |= (uint64_t)1 << lane;
    while (in) {
        const int c = __builtin_ctzll(in);
        in &= in - 1;
        const float nk = key[c];
        const int ni = row[c];
        if (!ivf::wide_before(nk, ni, tk, tr)) continue;
        const int at = ivf::count_before(p.pk, p.pr, K, nk, ni);
        CHECK(at >= 0 && at < K);
        const int chunks = ivf::shift_chunks(at, K);
        int moved = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            float vk[64];
            int vr[64];
            for (int lane = 0; lane < 64; ++lane) { // every lane reads ...
                const int dst = ivf::shift_dst(K, ch, lane);
                if (dst > at) vk[lane] = p.pk[p.slot(dst - 1)], vr[lane] = p.pr[p.slot(dst - 1)];
            }
            for (int lane = 0; lane < 64; ++lane) { // ... before any lane writes
                const int dst = ivf::shift_dst(K, ch, lane);
                if (dst > at) p.pk[p.slot(dst)] = vk[lane], p.pr[p.slot(dst)] = vr[lane], ++moved;
            }
        }
        CHECK(moved == K - 1 - at); // [at, K - 1) moved, each slot once
        CHECK(ivf::shift_dst(K, chunks, 0) <= at); // no chunk was left out
        p.pk[p.slot(at)] = nk;
        p.pr[p.slot(at)] = ni;
        tk = p.pk[ts];
        tr = p.pr[ts];
    }
}

void pool_finish(Pool& p) {
    if (p.cnt > 1 && p.cnt < p.k) pool_sort(p);
}

std::vector<Cand> make_stream(int n, int flavour) {
    std::vector<int> rows((size_t)n);
    const int base = (int)(rnd() % 1000);
    for (int i = 0; i < n; ++i) rows[(size_t)i] = base + 3 * i; // distinct
    if (flavour != 1)
        for (int i = n - 1; i > 0; --i) std::swap(rows[(size_t)i], rows[(size_t)(rnd() % (uint32_t)(i + 1))]);
    std::vector<Cand> s((size_t)n);
    for (int i = 0; i < n; ++i) {
        float key;
        switch (flavour) {
        case 0: key = (float)(rnd() % 7); break;                       // heavy ties
        case 1: key = (float)i; break;                                 // ascending: every candidate is inserted at the front
        case 2: key = (float)-i; break;                                // descending: none after the fill
        case 3: key = 5.0f; break;                                     // one key: the row decides everything
        default: key = rnd() % 5 == 0 ? -INFINITY : (float)(rnd() % 1000) * 0.25f; break;
        }
        s[(size_t)i] = {key, rows[(size_t)i]};
    }
    return s;
}

void check_pool_against(const Pool& p, std::vector<Cand> seen, bool sorted_now) {
    std::sort(seen.begin(), seen.end(), before);
    const int want = (int)std::min<size_t>(seen.size(), (size_t)p.k);
    CHECK(p.cnt == want);
    std::vector<Cand> got;
    for (int u = 0; u < p.cnt; ++u) got.push_back({p.pk[u], p.pr[u]});
    if (!sorted_now) std::sort(got.begin(), got.end(), before);
    for (int u = 0; u < want; ++u) CHECK(got[(size_t)u].row == seen[(size_t)u].row && (got[(size_t)u].key == seen[(size_t)u].key));
}

void run_stream(int k, int len, int flavour) {
    Pool p(k);
    CHECK(p.KP >= k && (p.KP == 64 || p.KP == 256 || p.KP == 1024) && (p.KP == 64 || ivf::pool_class(k) / 4 < k));
    const std::vector<Cand> s = make_stream(len, flavour);
    std::vector<Cand> seen;
    size_t next = 0;
    do {
        float key[64];
        int row[64];
        uint64_t valid = 0;
        const int dense = (int)(rnd() % 3); // full passes, sparse passes, mixed
        for (int lane = 0; lane < 64; ++lane) {
            key[lane] = NAN;
            row[lane] = -1;
            if (next < s.size() && (dense == 0 || rnd() % (dense == 1 ? 4 : 2) == 0)) {
                key[lane] = s[next].key;
                row[lane] = s[next].row;
                seen.push_back(s[next++]);
                valid |= (uint64_t)1 << lane;
            }
        }
        pool_pass(p, key, row, valid);
        check_pool_against(p, seen, p.cnt == k);
    } while (next < s.size());
    pool_finish(p);
    check_pool_against(p, seen, true);
}

// the final ranking of a workgroup: four sorted pools with distinct rows
void run_final(int k, const int lens[4], int flavour) {
    const int KP = ivf::pool_class(k);
    std::vector<float> poolk((size_t)ivf::kWideWaves * KP, NAN);
    std::vector<int> poolr((size_t)ivf::kWideWaves * KP, -777);
    int mc[4], total = 0;
    std::vector<Cand> all;
    for (int w = 0; w < 4; ++w) {
        Pool p(k);
        std::vector<Cand> s = make_stream(lens[w], flavour);
        for (auto& c : s) c.row = c.row * 4 + w; // distinct across the pools
        for (size_t i = 0; i < s.size(); i += 64) {
            float key[64];
            int row[64];
            uint64_t valid = 0;
            for (int lane = 0; lane < 64 && i + lane < s.size(); ++lane) key[lane] = s[i + lane].key, row[lane] = s[i + lane].row, valid |= (uint64_t)1 << lane;
            pool_pass(p, key, row, valid);
        }
        pool_finish(p);
        mc[w] = p.cnt;
        total += p.cnt;
        for (int u = 0; u < p.cnt; ++u) poolk[(size_t)w * KP + u] = p.pk[u], poolr[(size_t)w * KP + u] = p.pr[u], all.push_back({p.pk[u], p.pr[u]});
    }
    std::sort(all.begin(), all.end(), before);
    std::vector<int> out((size_t)k, -1);
    for (int tid = 0; tid < 256; ++tid)
        for (int e = tid; e < ivf::kWideWaves * KP; e += 256) {
            const int w = ivf::merge_pool(e, KP), u = ivf::merge_slot(e, KP);
            CHECK(w >= 0 && w < 4 && u >= 0 && u < KP && w * KP + u == e);
            if (u >= mc[w]) continue;
            int rank = u;
            for (int w2 = 0; w2 < 4 && rank < k; ++w2)
                if (w2 != w) rank += ivf::count_before(poolk.data() + (size_t)w2 * KP, poolr.data() + (size_t)w2 * KP, mc[w2], poolk[(size_t)e], poolr[(size_t)e]);
            if (rank < k) {
                CHECK(out[(size_t)rank] == -1); // every rank once
                out[(size_t)rank] = poolr[(size_t)e];
            }
        }
    for (int u = 0; u < k; ++u) CHECK(out[(size_t)u] == (u < total ? all[(size_t)u].row : -1));
}

} // namespace

int main(int argc, char** argv) {
    rng_state = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int ks[] = {1, 29, 30, 63, 64, 65, 255, 256, 257, 1023, 1024};
    for (int k = 1; k <= ivf::kWideMaxK; ++k) {
        const int kp = ivf::pool_class(k);
        CHECK(kp >= k && (kp == 64 || kp == 256 || kp == 1024) && (kp == 64 || kp / 4 < k)); // the smallest class that holds k
    }
    // the sort alone: every pool class, every count around the spans, ties and -inf keys
    for (int kp : {64, 256, 1024})
        for (int cnt : {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024}) {
            if (cnt > kp) continue;
            for (int flavour : {0, 3, 4}) {
                Pool p(kp);
                std::vector<Cand> s = make_stream(cnt, flavour);
                for (int u = 0; u < cnt; ++u) p.pk[u] = s[(size_t)u].key, p.pr[u] = s[(size_t)u].row;
                p.cnt = cnt;
                pool_sort(p);
                std::sort(s.begin(), s.end(), before);
                for (int u = 0; u < cnt; ++u) CHECK(p.pr[u] == s[(size_t)u].row && p.pk[u] == s[(size_t)u].key);
            }
        }
    for (int k : ks) {
        const int lens[] = {0, 1, k - 1, k, k + 1, 3 * k};
        for (int len : lens)
            for (int flavour = 0; flavour < 5; ++flavour) run_stream(k, len, flavour);
        const int mixes[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {k, k, k, k}, {3 * k, 1, k - 1, k + 1}, {k - 1, k - 1, 0, 2}, {3 * k, 3 * k, 3 * k, 3 * k}};
        for (const auto& mix : mixes)
            for (int flavour : {0, 3, 4}) run_final(k, mix, flavour);
    }
    std::printf("ok %lld\n", checks);
    return 0;
}
