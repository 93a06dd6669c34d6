// A corpus that is edited, through the C++ host side (include/frizbee_hip.hpp): Corpus::remove / remove_device / replace / edit_info.
// Without an argument: the host-only part (the calls compile and link, bad arguments are refused before a device is touched).  With
// "gpu": a list with haystacks removed and replaced answers like one upload of the edited list.
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
        const uint32_t idx = 0;
        uint64_t info[4];
        fzb_corpus* fake = (fzb_corpus*)64;  // never dereferenced: the argument checks come first
        CHECK(fzb_corpus_remove(nullptr, &idx, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove(fake, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove_device(nullptr, &idx, 4, &idx, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove_device(fake, nullptr, 4, &idx, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove_device(fake, &idx, 4, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove_device(fake, &idx, 0, &idx, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_remove_device(fake, &idx, 6, &idx, 1) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "stride_bytes") != nullptr);
        CHECK(fzb_corpus_replace(nullptr, &idx, 1, &byte, &end) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_replace(fake, nullptr, 1, &byte, &end) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_replace(fake, &idx, 1, &byte, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_edit_info(nullptr, info) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_edit_info(fake, nullptr) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) {
            int threw = 0;
            try {
                Corpus c(std::vector<std::string>{"a"});
                c.remove({0});
                c.replace({0}, std::vector<std::string>{"b"});
                (void)c.edit_info();
            } catch (const Error& e) {
                threw++;
            }
            CHECK(threw == 1);
        }
        if (failures) return 1;
        printf("test_facade_edit: ok (host)\n");
        return 0;
    }
    try {
        Corpus cp(hs);
        CHECK(cp.edit_info().first == 0 && cp.edit_info().bytes_written == 0);
        // every third haystack from 5000 on goes, two are renamed
        std::vector<std::string> want;
        std::vector<uint32_t> drop;
        for (size_t i = 0; i < hs.size(); i++) {
            if (i >= 5000 && i % 3 == 0) drop.push_back((uint32_t)i);
            else want.push_back(hs[i]);
        }
        cp.remove(drop);
        CHECK(cp.len() == want.size() && cp.edit_info().first == drop.front());
        want[17] = "src/linux/renamed_to_something_much_longer_than_it_was_before/file.cc";
        want[9000] = "";
        cp.replace({9000, 17}, std::vector<std::string>{want[9000], want[17]});
        CHECK(cp.edit_info().first == 17);
        Corpus fresh(want);
        const Corpus::Info gi = cp.info(), wi = fresh.info();
        CHECK(gi.items == wi.items && gi.bytes == wi.bytes && gi.max_len == wi.max_len && gi.uniform_len == wi.uniform_len);
        CHECK(gi.has_view == wi.has_view && gi.view_nv == wi.view_nv && gi.outliers == wi.outliers);
        for (int multi = 0; multi < 2; multi++) {
            for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::IndexDesc}) {
                Matcher m = multi ? Matcher::from_query("src linux !test", Config().sort(sort)) : Matcher("linux", Config().sort(sort));
                const std::vector<Match> all = m.match_list(fresh);
                CHECK(all.size() > 1000);
                CHECK(m.match_list(cp) == all);
                size_t found = 0;
                CHECK(m.match_list_top(cp, 100, &found) == std::vector<Match>(all.begin(), all.begin() + 100) && found == all.size());
            }
        }
        int threw = 0;
        try {
            cp.remove({(uint32_t)cp.len()});
        } catch (const Error& e) {
            threw += e.code == FZB_ERR_INVALID;
        }
        CHECK(threw == 1 && cp.len() == want.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_edit: ok\n");
    return 0;
}
