// csrc/update_math.hpp -- the text the update kernels and the host compile -- as a stand-alone program for the sanitizers:
//   update_math_check cases.txt      one case per line: ntotal idx_offset n id_0 .. id_{n-1}   (n == 0: nothing follows)
// For every case the sequential loop of assignments (the definition) is run on a row -> position table and compared with
//   - upd::host_winners (winners and the count of distinct rows), and
//   - the three passes as the kernels run them: fold_owner over the positions in ascending, descending and a scrambled order (the
//     atomic maximum may land in any), wins() per position, and the owners put back to kNoOwner by the winners alone.
// Prints "ok <cases> <positions> <winners>"; exit status 1 on the first difference.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/update_math.hpp"

static int fail(const std::string& what, size_t line) {
    std::printf("FAIL line %zu: %s\n", line, what.c_str());
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    // the id rule at the ends of int64: no signed overflow (UBSan watches), nothing cut off
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    if (upd::local_row(lo, 0, 10) != -1 || upd::local_row(hi, 0, 10) != -1 || upd::local_row(hi, lo, hi) != -1) return fail("extremes", 0);
    if (upd::local_row(lo + 3, lo, 10) != 3 || upd::local_row(hi, hi - 2, 3) != 2 || upd::local_row(hi, hi - 3, 3) != -1) return fail("offsets", 0);
    if (upd::local_row((int64_t(1) << 32) + 3, 0, 10) != -1 || upd::local_row(-1, -2, 5) != 1 || upd::local_row(5, 5, 0) != -1) return fail("ids", 0);
    if (!upd::count_ok(0) || !upd::count_ok(0x7fffffff) || upd::count_ok(0x80000000LL) || upd::count_ok(-1)) return fail("count_ok", 0);
    if (upd::fold_owner(upd::kNoOwner, 0) != 0 || upd::fold_owner(7, 3) != 7 || !upd::wins(4, 4) || upd::wins(upd::kNoOwner, 0)) return fail("owner rule", 0);

    std::ifstream in(argv[1]);
    std::string text;
    size_t line = 0, cases = 0, positions = 0, nwin = 0;
    while (std::getline(in, text)) {
        ++line;
        std::istringstream ss(text);
        int64_t ntotal, off, n;
        if (!(ss >> ntotal >> off >> n) || ntotal < 0 || n < 0) return fail("malformed case", line);
        std::vector<int64_t> ids((size_t)n);
        for (auto& v : ids)
            if (!(ss >> v)) return fail("too few ids", line);
        // the definition: the loop, on a table row -> last position that wrote it
        std::vector<int64_t> last((size_t)ntotal, -1);
        for (int64_t p = 0; p < n; ++p) {
            const int64_t id = ids[(size_t)p];
            if (id < off) continue;
            const uint64_t local = (uint64_t)id - (uint64_t)off;
            if (local < (uint64_t)ntotal) last[(size_t)local] = p;
        }
        std::vector<unsigned char> want((size_t)n, 0);
        int64_t distinct = 0;
        for (int64_t r = 0; r < ntotal; ++r)
            if (last[(size_t)r] >= 0) want[(size_t)last[(size_t)r]] = 1, ++distinct;
        std::vector<unsigned char> got;
        if (upd::host_winners(ids.data(), n, off, ntotal, &got) != distinct || got != want) return fail("host_winners differs from the loop", line);
        if (upd::host_winners(ids.data(), n, off, ntotal) != distinct) return fail("host_winners without the list", line);
        // the three passes, pass A in three orders
        std::vector<int> owner((size_t)ntotal, upd::kNoOwner);
        for (int order = 0; order < 3; ++order) {
            for (int64_t t = 0; t < n; ++t) {
                const int64_t p = order == 0 ? t : order == 1 ? n - 1 - t : (t * 7919 + 13) % n; // (7919 is prime: a permutation unless it divides n)
                const int64_t r = upd::local_row(ids[(size_t)p], off, ntotal);
                if (r >= 0) owner[(size_t)r] = upd::fold_owner(owner[(size_t)r], (int)p);
            }
            if (order == 2 && n % 7919 == 0) // (not a permutation: finish the fold)
                for (int64_t p = 0; p < n; ++p) {
                    const int64_t r = upd::local_row(ids[(size_t)p], off, ntotal);
                    if (r >= 0) owner[(size_t)r] = upd::fold_owner(owner[(size_t)r], (int)p);
                }
            for (int64_t p = 0; p < n; ++p) { // pass B reads, writes nothing to owner
                const int64_t r = upd::local_row(ids[(size_t)p], off, ntotal);
                if ((r >= 0 && upd::wins(owner[(size_t)r], (int)p)) != (want[(size_t)p] != 0)) return fail("the owner passes differ from the loop", line);
            }
            for (int64_t p = n - 1; p >= 0; --p) { // pass C, in an order of its own: only the winner resets
                const int64_t r = upd::local_row(ids[(size_t)p], off, ntotal);
                if (r >= 0 && upd::wins(owner[(size_t)r], (int)p)) owner[(size_t)r] = upd::kNoOwner;
            }
            for (int v : owner)
                if (v != upd::kNoOwner) return fail("an owner was not put back", line);
        }
        ++cases, positions += (size_t)n, nwin += (size_t)distinct;
    }
    std::printf("ok %zu %zu %zu\n", cases, positions, nwin);
    return 0;
}
