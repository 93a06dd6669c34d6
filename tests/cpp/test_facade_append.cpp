// A corpus that grows, through the C++ host side (include/frizbee_hip.hpp): Corpus::append / reserve / truncate / info.  Without an
// argument: the host-only part (the calls compile and link, NULL is refused before a device is touched).  With "gpu": a list appended in
// batches answers like one upload of it.
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

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && !strcmp(argv[1], "gpu");
    std::vector<std::string> hs;
    for (int i = 0; i < 20000; i++) {
        std::string h = "src/" + std::to_string(i * 7919 % 10007) + "/";
        if (i % 3 == 0) h += "linux/";
        if (i % 5 == 0) h += "test_";
        if (i % 7 == 0) h += "a/rather/longer/directory/name/that/goes/beyond/thirty-two/bytes/";
        h += "file.cc";
        hs.push_back(h);
    }
    if (!gpu) {
        const uint8_t byte = 'a';
        const uint64_t end = 1;
        uint64_t info[12];
        size_t got = 0;
        CHECK(fzb_corpus_append(nullptr, &byte, &end, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_reserve(nullptr, 1, 16) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_truncate(nullptr, 0) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_info(nullptr, info) == FZB_ERR_INVALID);
        CHECK(fzb_debug_corpus_read(nullptr, 0, nullptr, 0, &got) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) {
            int threw = 0;
            try {
                Corpus c(std::vector<std::string>{"a"});
                c.append(std::vector<std::string>{"b"});
            } catch (const Error& e) {
                threw++;
            }
            CHECK(threw == 1);
        }
        if (failures) return 1;
        printf("test_facade_append: ok (host)\n");
        return 0;
    }
    try {
        Corpus whole(hs);
        Corpus grown(std::vector<std::string>{});
        const size_t batches[] = {1, 63, 1024, 1025, 5000};
        size_t at = 0, b = 0;
        while (at < hs.size()) {
            const size_t n = std::min(batches[b++ % 5], hs.size() - at);
            grown.append(std::vector<std::string>(hs.begin() + (std::ptrdiff_t)at, hs.begin() + (std::ptrdiff_t)(at + n)));
            at += n;
        }
        CHECK(grown.len() == whole.len());
        const Corpus::Info gi = grown.info(), wi = whole.info();
        CHECK(gi.items == wi.items && gi.bytes == wi.bytes && gi.max_len == wi.max_len && gi.uniform_len == wi.uniform_len);
        CHECK(gi.has_view == wi.has_view && gi.view_nv == wi.view_nv && gi.outliers == wi.outliers);
        for (int multi = 0; multi < 2; multi++) {
            for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::IndexDesc}) {
                Matcher m = multi ? Matcher::from_query("src linux !test", Config().sort(sort)) : Matcher("linux", Config().sort(sort));
                const std::vector<Match> all = m.match_list(whole);
                CHECK(all.size() > 1000);
                CHECK(m.match_list(grown) == all);
                size_t found = 0;
                CHECK(m.match_list_top(grown, 100, &found) == std::vector<Match>(all.begin(), all.begin() + 100) && found == all.size());
            }
        }
        grown.truncate(1500);
        Corpus prefix(std::vector<std::string>(hs.begin(), hs.begin() + 1500));
        Matcher m("linux");
        CHECK(grown.len() == 1500 && m.match_list(grown) == m.match_list(prefix));
        grown.reserve(4000, 4000 * 128);
        const uint64_t regrows = grown.info().regrows;
        grown.append(std::vector<std::string>(hs.begin() + 1500, hs.begin() + 3000));
        Corpus longer(std::vector<std::string>(hs.begin(), hs.begin() + 3000));
        CHECK(grown.info().regrows == regrows && m.match_list(grown) == m.match_list(longer));
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_append: ok\n");
    return 0;
}
