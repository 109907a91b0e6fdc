// Stand-alone check of the removal plan (csrc/remove_plan.hpp), built with -fsanitize=address,undefined and run on the CPU by
// tests/test_remove_host.py.  Input (a file named on the command line): one case per line, "W n mask" with mask a string of n
// characters '0' / '1' ('1' = the row leaves; "-" for n = 0).  For every case the plan is made from the per-window counts alone,
// as the library makes it, and then
//   * its invariants are checked: the destinations tile [first_row, n_new) in order without a gap or an overlap, every
//     destination ends at or before its window's end, `direct` exactly where the destination is disjoint from the window, no
//     window before first_row loses a row;
//   * it is EXECUTED on an array of row numbers, window by window in order -- a direct move writes in place while the check
//     asserts that it never writes a row of its own window it has yet to read, a bounce move goes through a buffer of exactly
//     the size the library allocates -- and the result is compared with the plain compaction.
// Prints "ok <cases> <moves> <direct> <bounce>" and exits 0, or names the first violated invariant and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../retrieval-augmented-mds_amd/csrc/remove_plan.hpp"

#define REQUIRE(cond, what)                                                                                   \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            std::fprintf(stderr, "case %ld (W %ld, n %ld): %s\n", (long)ncase, (long)W, (long)n, what);      \
            return 1;                                                                                         \
        }                                                                                                     \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    long ncase = 0, nmoves = 0, ndirect = 0, nbounce = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        int64_t W = 0, n = 0;
        std::string mask;
        ls >> W >> n >> mask;
        ++ncase;
        REQUIRE(W > 0 && W % 128 == 0 && n >= 0 && (n == 0 || (int64_t)mask.size() == n), "malformed case");
        const int64_t nw = (n + W - 1) / W;
        std::vector<int> kept((size_t)nw, 0);
        std::vector<int64_t> want;
        for (int64_t i = 0; i < n; ++i)
            if (mask[(size_t)i] == '0') {
                ++kept[(size_t)(i / W)];
                want.push_back(i);
            }
        const mips_remove::Plan p = mips_remove::make_plan(kept, W, n);
        REQUIRE(p.n_new == (int64_t)want.size(), "n_new is not the number of surviving rows");
        REQUIRE(p.first_row >= 0 && p.first_row <= p.n_new, "first_row out of range");
        for (int64_t i = 0; i < p.first_row; ++i) REQUIRE(mask[(size_t)i] == '0', "a row before first_row is removed");
        REQUIRE(p.first_row == p.n_new || p.first_row % W == 0, "first_row is not a window start");
        int64_t at = p.first_row, last_window = -1, bounce_rows = 0;
        for (const mips_remove::Move& m : p.moves) {
            const int64_t start = m.window * W, rows = mips_remove::window_rows(n, W, m.window);
            REQUIRE(m.window > last_window && m.window < nw, "moves are not in ascending window order");
            REQUIRE(m.kept > 0 && m.kept == kept[(size_t)m.window], "a move's count is not its window's");
            REQUIRE(m.base == at, "destinations leave a gap or overlap");
            REQUIRE(m.base <= start && m.base + m.kept <= start + rows, "a destination reaches past its window");
            REQUIRE(m.direct == (m.base + m.kept <= start), "direct is not 'the destination is disjoint from the window'");
            if (!m.direct && m.kept > bounce_rows) bounce_rows = m.kept;
            at += m.kept;
            last_window = m.window;
            ++nmoves;
            ++(m.direct ? ndirect : nbounce);
        }
        REQUIRE(at == p.n_new, "destinations do not end at n_new");
        // execution on row numbers; `bounce` is exactly as large as the library's
        std::vector<int64_t> rows((size_t)n), bounce((size_t)bounce_rows);
        for (int64_t i = 0; i < n; ++i) rows[(size_t)i] = i;
        for (const mips_remove::Move& m : p.moves) {
            const int64_t start = m.window * W, end = start + mips_remove::window_rows(n, W, m.window);
            int64_t r = 0;
            for (int64_t i = start; i < end; ++i) {
                if (mask[(size_t)i] != '0') continue;
                if (m.direct) {
                    REQUIRE(m.base + r < start, "a direct move writes into its own window");
                    rows[(size_t)(m.base + r)] = rows[(size_t)i];
                } else {
                    bounce[(size_t)r] = rows[(size_t)i];
                }
                ++r;
            }
            REQUIRE(r == m.kept, "a window holds another number of survivors than planned");
            if (!m.direct)
                for (int64_t j = 0; j < r; ++j) rows[(size_t)(m.base + j)] = bounce[(size_t)j];
        }
        for (int64_t i = 0; i < p.n_new; ++i) REQUIRE(rows[(size_t)i] == want[(size_t)i], "the executed plan is not the compaction");
    }
    std::printf("ok %ld %ld %ld %ld\n", ncase, nmoves, ndirect, nbounce);
    return 0;
}
