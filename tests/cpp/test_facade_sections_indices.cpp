// Sectioned top-`limit` with matched positions through the C++ host side (include/frizbee_hip.hpp): Matcher::match_list_top_sections_indices.
// Without an argument: the host-only part (the calls compile and link, bad arguments and the stated limits are refused before a device is
// touched).  With "gpu": the heads of a query against heads made here from the same list - a haystack matches "linux" exactly when this test
// put "linux/" into it, at bytes 10..14 behind "src/" and five digits, every match has the same score, so a section's head is its first
// (last, for the *Desc strategies) `limit` members, each with the positions 14, 13, 12, 11, 10.
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
    static_assert(FZB_SECTIONS_MAX == 8 && FZB_SECTION_LIMIT_MAX == 1024, "the limits the header states");
    if (!gpu) {
        fzb_matcher* m = (fzb_matcher*)64;  // never dereferenced: the argument checks come first
        fzb_multi_matcher* mm = (fzb_multi_matcher*)64;
        const fzb_corpus* c = (const fzb_corpus*)64;
        fzb_section secs[9] = {};
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        fzb_match_indices* dev = (fzb_match_indices*)64;
        uint32_t* words = (uint32_t*)64;
        size_t lens[9];
        uint64_t found[9];
        CHECK(fzb_match_list_top_sections_indices(m, c, secs, 9, 10, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID && out == nullptr && pos == nullptr);
        CHECK(strstr(fzb_last_error(), "FZB_SECTIONS_MAX") != nullptr);
        CHECK(fzb_match_list_top_sections_indices(m, c, secs, 8, 1025, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "FZB_SECTION_LIMIT_MAX") != nullptr);
        CHECK(fzb_match_list_top_sections_indices(nullptr, c, secs, 1, 1, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices(m, nullptr, secs, 1, 1, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices(m, c, nullptr, 1, 1, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices(m, c, secs, 1, 1, nullptr, nullptr, nullptr, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices(m, c, secs, 1, 1, nullptr, nullptr, &out, nullptr, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices(m, c, secs, 1, 1, nullptr, nullptr, &out, lens, nullptr, found) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_sections_indices(mm, c, secs, 9, 10, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_sections_indices(mm, c, secs, 2, 1025, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_sections_indices(nullptr, c, secs, 1, 1, nullptr, nullptr, &out, lens, &pos, found) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(m, c, secs, 9, 10, nullptr, nullptr, dev, 90, words, 900, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(m, c, secs, 8, 1025, nullptr, nullptr, dev, 8200, words, 82000, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(m, c, secs, 1, 1, nullptr, nullptr, nullptr, 1, words, 8, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(m, c, secs, 1, 1, nullptr, nullptr, dev, 1, nullptr, 8, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(m, c, secs, 1, 1, nullptr, nullptr, dev, 1, words, 8, nullptr, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_match_list_top_sections_indices_device(nullptr, c, secs, 1, 1, nullptr, nullptr, dev, 1, words, 8, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_sections_indices_device(mm, c, secs, 9, 10, nullptr, nullptr, dev, 90, words, 900, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_sections_indices_device(mm, nullptr, secs, 1, 1, nullptr, nullptr, dev, 1, words, 8, words, nullptr) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        if (failures) return 1;
        printf("test_facade_sections_indices: ok (host)\n");
        return 0;
    }
    try {
        std::vector<std::string> hs;
        std::vector<uint16_t> tags;
        for (int i = 0; i < 20000; i++) {
            std::string h = "src/" + std::to_string(10000 + i * 7919 % 10007) + "/";
            if (i % 3 == 0) h += "linux/";
            h += "file.cc";
            hs.push_back(h);
            tags.push_back((uint16_t)((i % 4 == 0 ? 1 : 0) | (i % 7 == 0 ? 2 : 0) | (i * 31 % 5 == 0 ? 0x8000 : 0)));
        }
        Corpus cp(hs);
        cp.set_tags(tags);
        cp.set_scope(0, 0x8000);
        const std::vector<fzb_section> sections = {{1, 0}, {2, 1}, {0, 0}, {1, 1}, {3, 0}};
        const std::vector<uint32_t> where = {14, 13, 12, 11, 10};
        for (int desc = 0; desc < 2; desc++) {
            Config cfg;
            cfg.sort_ = desc ? SortStrategy::ScoreThenIndexDesc : SortStrategy::ScoreThenIndexAsc;
            for (int multi = 0; multi < 2; multi++) {
                Matcher m = multi ? Matcher::from_query("linux !zzz", cfg) : Matcher(Pattern("linux"), cfg);
                for (size_t limit : {(size_t)0, (size_t)7, (size_t)1024}) {
                    const auto heads = m.match_list_top_sections_indices(cp, sections, limit);
                    CHECK(heads.size() == sections.size());
                    for (size_t s = 0; s < heads.size(); s++) {
                        std::vector<uint32_t> members;
                        for (size_t i = 0; i < hs.size(); i += 3) {  // the haystacks that hold "linux/"
                            const uint16_t t = tags[i];
                            if ((t & 0x8000) == 0 && (t & sections[s].require) == sections[s].require && (t & sections[s].exclude) == 0) members.push_back((uint32_t)i);
                        }
                        CHECK(heads[s].found == members.size());
                        const size_t kept = members.size() < limit ? members.size() : limit;
                        CHECK(heads[s].matches.size() == kept);
                        for (size_t k = 0; k < kept && k < heads[s].matches.size(); k++) {
                            CHECK(heads[s].matches[k].index == (desc ? members[members.size() - 1 - k] : members[k]));
                            CHECK(heads[s].matches[k].indices == where);
                        }
                    }
                }
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("test_facade_sections_indices: ok\n");
    return 0;
}
