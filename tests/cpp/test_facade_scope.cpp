// Per-haystack tags and a visibility scope, through the C++ host side (include/frizbee_hip.hpp): Corpus::set_tags / update_tags /
// clear_tags / set_scope / scope_info.  Without an argument: the host-only part (the calls compile and link, bad arguments are refused
// before a device is touched).  With "gpu": the contract sentence itself - a scoped corpus answers like a second Corpus made of the
// visible haystacks alone, every index mapped back to the full list.
#include <algorithm>
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
    if (!gpu) {
        const uint16_t val = 5;
        const uint32_t idx = 0;
        uint64_t info[4];
        fzb_corpus* fake = (fzb_corpus*)64;  // never dereferenced: the argument checks come first
        CHECK(fzb_corpus_set_tags(nullptr, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_set_tags(fake, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_tags(nullptr, &idx, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_tags(fake, nullptr, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_tags(fake, &idx, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_clear_tags(nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_set_scope(nullptr, 1, 2) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_scope_info(nullptr, info) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_scope_info(fake, nullptr) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) {
            int threw = 0;
            try {
                Corpus c(std::vector<std::string>{"a"});
                c.set_tags({1});
                c.update_tags({0}, {2});
                c.set_scope(1, 0);
                c.clear_tags();
                (void)c.scope_info();
            } catch (const Error& e) {
                threw++;
            }
            CHECK(threw == 1);
        }
        if (failures) return 1;
        printf("test_facade_scope: ok (host)\n");
        return 0;
    }
    try {
        std::vector<std::string> hs;
        for (int i = 0; i < 20000; i++) {
            std::string h = "src/" + std::to_string(i * 7919 % 10007) + "/";
            if (i % 3 == 0) h += "linux/";
            if (i % 5 == 0) h += "test_";
            h += "file.cc";
            hs.push_back(h);
        }
        std::vector<uint16_t> tags(hs.size());
        for (size_t i = 0; i < hs.size(); i++) tags[i] = (uint16_t)((i % 4 == 0 ? 1 : 0) | (i % 7 == 0 ? 2 : 0) | (i * 31 % 5 == 0 ? 0x8000 : 0));
        Corpus cp(hs);
        CHECK(cp.scope_info().active == 0 && cp.scope_info().capacity == 0);
        cp.set_tags(tags);
        CHECK(cp.scope_info().active == 0 && cp.scope_info().capacity >= hs.size());
        const uint16_t scopes[3][2] = {{0, 1}, {2, 0x8000}, {1, 1}};  // hide bit 0; require bit 1 without bit 15; a bit in both masks: nothing visible
        for (const auto& sc : scopes) {
            std::vector<std::string> vis;
            std::vector<uint32_t> map;
            for (size_t i = 0; i < hs.size(); i++)
                if ((tags[i] & sc[0]) == sc[0] && (tags[i] & sc[1]) == 0) {
                    vis.push_back(hs[i]);
                    map.push_back((uint32_t)i);
                }
            Corpus sub(vis);
            for (int multi = 0; multi < 2; multi++) {
                for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::ScoreThenIndexDesc, SortStrategy::IndexDesc}) {
                    Matcher m = multi ? Matcher::from_query("src linux !test", Config().sort(sort)) : Matcher("linux", Config().sort(sort));
                    cp.set_scope(0, 0);
                    const std::vector<Match> plain = m.match_list(cp);
                    std::vector<Match> want = m.match_list(sub);
                    for (Match& r : want) r.index = map[r.index];
                    cp.set_scope(sc[0], sc[1]);
                    CHECK(cp.scope_info().active == 1 && cp.scope_info().require() == sc[0] && cp.scope_info().exclude() == sc[1]);
                    CHECK(vis.empty() ? want.empty() : (want.size() > 100 && want.size() < plain.size()));
                    CHECK(m.match_list(cp) == want);
                    size_t found = 0;
                    const size_t head = std::min<size_t>(100, want.size());
                    CHECK(m.match_list_top(cp, 100, &found) == std::vector<Match>(want.begin(), want.begin() + head) && found == want.size());
                    const std::vector<MatchIndices> top = m.match_list_top_indices(cp, 10, &found);
                    CHECK(top.size() == std::min<size_t>(10, want.size()) && found == want.size());
                    for (size_t k = 0; k < top.size(); k++) CHECK(top[k].index == want[k].index && top[k].score == want[k].score);
                    cp.set_scope();
                    CHECK(cp.scope_info().active == 0);
                    CHECK(m.match_list(cp) == plain);
                }
            }
        }
        cp.update_tags({3, 17}, {4, 4});
        cp.set_scope(4, 0);
        CHECK(Matcher("", Config()).match_list(cp).size() == 2);
        int threw = 0;
        try {
            cp.update_tags({3, 3}, {1, 2});
        } catch (const Error& e) {
            threw += e.code == FZB_ERR_INVALID;
        }
        try {
            cp.set_tags(std::vector<uint16_t>(3, 0));
        } catch (const Error& e) {
            threw += e.code == FZB_ERR_INVALID;
        }
        CHECK(threw == 2 && cp.scope_info().require() == 4);
        cp.clear_tags();
        CHECK(cp.scope_info().active == 0 && cp.scope_info().scope == 0 && cp.scope_info().capacity >= hs.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_scope: ok\n");
    return 0;
}
