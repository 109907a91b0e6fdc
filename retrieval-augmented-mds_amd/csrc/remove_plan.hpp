// The plan of an in-place row removal (mips_index_remove, host_remove.hpp): plain host code on vectors, no HIP call, so that a
// stand-alone program can run it under the sanitizers (tests/remove_plan_check.cpp).
//
// The rows [0, n) are cut into windows of W rows (the last one ragged); kept[w] is the number of rows of window w that survive.
// The surviving rows of window w go to [base, base + kept[w]), base = the number of survivors before the window: base <= start
// (= w * W) and base + kept[w] <= the window's own end.  The windows are moved one launch each, in ascending order on one
// stream.  What a launch writes is never read by a LATER launch (those read rows >= their own start >= this window's end) and an
// EARLIER launch is complete, so the only hazard is inside one launch: a workgroup writing a destination row that another
// workgroup of the same launch has not read yet.  That needs the destination to reach into the window's own rows:
//     base + kept[w] <= start   the destination is disjoint from everything the launch reads: write it directly
//     otherwise                 gather into a bounce buffer of one window; a device-to-device copy behind the launch carries it home
// Windows before the first one that loses a row stay where they are; a window that keeps nothing needs no launch.
#pragma once

#include <cstdint>
#include <vector>

namespace mips_remove {

struct Move {
    int64_t window; // rows [window * W, min(n, (window + 1) * W)) are read
    int64_t base;   // first destination row
    int64_t kept;   // > 0: destination rows
    bool direct;    // true: written in place by the gather; false: through the bounce buffer
};

struct Plan {
    int64_t first_row = 0; // start of the first window that loses a row (= n_new when nothing is removed): rows before it stay
    int64_t n_new = 0;     // surviving rows
    std::vector<Move> moves;
};

inline int64_t window_rows(int64_t n, int64_t W, int64_t w) {
    const int64_t left = n - w * W;
    return left < W ? left : W;
}

// kept.size() == ceil(n / W) and 0 <= kept[w] <= window_rows(n, W, w)
inline Plan make_plan(const std::vector<int>& kept, int64_t W, int64_t n) {
    Plan p;
    const int64_t nw = (int64_t)kept.size();
    int64_t w = 0, base = 0;
    while (w < nw && kept[w] == window_rows(n, W, w)) base += kept[w++];
    p.first_row = base; // (every window before w is whole: base == w * W, or == n when the loop ran to the end)
    for (; w < nw; ++w) {
        const int64_t k = kept[w], start = w * W;
        if (k > 0) p.moves.push_back(Move{w, base, k, base + k <= start});
        base += k;
    }
    p.n_new = base;
    return p;
}

} // namespace mips_remove
