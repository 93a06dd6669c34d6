// `Matcher::match_list_top_indices` of the C++ host side (include/frizbee_hip.hpp) for Single and Multi matchers.  Without an argument: the
// host-only part (the call compiles and links; without a device it fails loudly, never quietly).  With "gpu": the result is the head of
// `match_list_indices`' list over the whole corpus with `index` = the corpus index, `found` its length.
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "frizbee_hip.hpp"

using namespace frizbee;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                              \
        }                                                                            \
    } while (0)

static std::vector<MatchIndices> head(const std::vector<MatchIndices>& v, size_t limit) {
    return std::vector<MatchIndices>(v.begin(), v.begin() + (std::ptrdiff_t)std::min(limit, v.size()));
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && !strcmp(argv[1], "gpu");
    std::vector<std::string> hs;
    for (int i = 0; i < 20000; i++) {
        std::string h = "src/" + std::to_string(i * 7919 % 10007) + "/";
        if (i % 3 == 0) h += "linux/";
        if (i % 5 == 0) h += "test_";
        h += i % 7 == 0 ? "lin_file.cc" : "file.cc";
        hs.push_back(h);
    }
    if (!gpu) {
        int threw = 0;
        for (int multi = 0; multi < 2; multi++) {
            try {
                Matcher m = multi ? Matcher::from_query("src linux !test") : Matcher("linux");
                size_t found = 0;
                (void)m.match_list_top_indices(hs, 10, &found);
            } catch (const Error& e) {
                threw++;
            }
        }
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) CHECK(threw == 2);
        if (failures) return 1;
        printf("test_facade_top_indices: ok (host)\n");
        return 0;
    }
    try {
        Corpus corpus(hs);
        for (int multi = 0; multi < 2; multi++) {
            for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::ScoreThenIndexDesc, SortStrategy::IndexDesc}) {
                Matcher m = multi ? Matcher::from_query("src linux !test", Config().sort(sort)) : Matcher("linux", Config().sort(sort).max_typos(1));
                // (the whole corpus as the list: `index` of match_list_indices is the corpus index)
                const std::vector<MatchIndices> all = m.match_list_indices(corpus);
                CHECK(all.size() > 1000);
                m.reserve_top_indices(corpus, 100, 16);
                for (size_t limit : {(size_t)0, (size_t)1, (size_t)100, (size_t)3000, all.size(), all.size() * 2}) {
                    size_t found = 0;
                    CHECK(m.match_list_top_indices(corpus, limit, &found) == head(all, limit) && found == all.size());
                }
                CHECK(m.match_list_top_indices(corpus, 5) == head(all, 5));  // `found` is optional
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_top_indices: ok\n");
    return 0;
}
