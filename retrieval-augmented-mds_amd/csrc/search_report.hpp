// What ONE search call flagged and settled (mips_index_margin_stats), and its rules.  Plain C++, no HIP: the two device words are
// only named here.  A call builds its own report and passes it down by reference; the entry point stores it on the index once,
// when the call succeeds (mips_index::report), so no function learns from the index what another one of the same call did.
#pragma once

#include <cstdint>

struct SearchReport {
    // the default is "unknown": a call that returned an error, or one that ran without the margin check, reports (-1, 0, 0)
    int64_t flagged = -1;    // queries the margin check could not certify; -1 = counted on the device, not read back yet
    int64_t rescanned = 0;   // of those, settled: exactly, or by a second scan with the widest lists
    int64_t unresolved = 0;  // still flagged after that
    int max_n = 0;           // flagged queries the exact pass resolves at most (0 = no such limit applied)
    bool fallback = false;   // the gated re-scan was enqueued behind the exact pass: it takes what is over that limit
    // While flagged = -1, where the counts are: a call that settles on the stream leaves first_dev (flagged) and last_dev
    // (unresolved); one that only counts leaves last_dev (flagged = unresolved); neither: nothing was counted
    const int* first_dev = nullptr;
    unsigned* last_dev = nullptr;

    // nothing can be uncertified: range search (the candidates are a provable superset), an empty index
    static SearchReport all_certified() {
        SearchReport r;
        r.flagged = 0;
        return r;
    }
    // flagged queries that were settled.  Over the exact pass's limit it leaves every first result alone, so unless the
    // fall-back re-scan stands behind it nothing was settled
    int64_t settled() const { return (max_n > 0 && flagged > max_n && !fallback) ? 0 : flagged; }
    // the counts as read from the device words (flagged_word: first_dev's, looked at only if there is one)
    void read_back(unsigned flagged_word, unsigned last_word) {
        flagged = first_dev ? flagged_word : last_word;
        unresolved = last_word;
        rescanned = first_dev ? settled() : 0;
    }
};
