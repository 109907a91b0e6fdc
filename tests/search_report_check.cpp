// The rules of csrc/search_report.hpp on the host (the header includes no HIP): compiled and run by test_search_report_host.py.
#include <cstdio>

#include "../retrieval-augmented-mds_amd/csrc/search_report.hpp"

static int bad = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);      \
            ++bad;                                              \
        }                                                       \
    } while (0)

int main() {
    SearchReport r; // "unknown": an error, or a call without the margin check
    CHECK(r.flagged == -1 && r.rescanned == 0 && r.unresolved == 0 && r.max_n == 0 && !r.fallback && !r.first_dev && !r.last_dev);
    const SearchReport c = SearchReport::all_certified();
    CHECK(c.flagged == 0 && c.rescanned == 0 && c.unresolved == 0 && !c.first_dev && !c.last_dev);

    // settled: every flagged query, unless the exact pass was over its limit with no fall-back behind it
    r.flagged = 7;
    CHECK(r.settled() == 7);            // no limit applied (re-scans, the wide search)
    r.max_n = 7;
    CHECK(r.settled() == 7);            // at the limit
    r.max_n = 6;
    CHECK(r.settled() == 0);            // over it: the first results stand
    r.fallback = true;
    CHECK(r.settled() == 7);            // over it, the gated re-scan takes them

    // counts fetched from the device: two words (settled on the stream) or one (counted only)
    int first_word = 0;
    unsigned last_word = 0;
    SearchReport two;
    two.first_dev = &first_word;
    two.last_dev = &last_word;
    two.max_n = 4;
    two.read_back(9, 9);
    CHECK(two.flagged == 9 && two.rescanned == 0 && two.unresolved == 9);
    two.fallback = true;
    two.read_back(9, 2);
    CHECK(two.flagged == 9 && two.rescanned == 9 && two.unresolved == 2);
    SearchReport one;
    one.last_dev = &last_word;
    one.read_back(123, 5); // (the first word is not looked at)
    CHECK(one.flagged == 5 && one.rescanned == 0 && one.unresolved == 5);
    std::printf(bad ? "failed %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
