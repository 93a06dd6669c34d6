// Any-of groups (`a | b`) through the C++ host side (include/frizbee_hip.hpp): Pattern::parse_query_groups and Matcher::from_pattern_groups.
// Without an argument: the host-only part (the calls compile and link, the parser's table, bad groupings refused before a device is touched).
// With "gpu": `rs$ | py$ !test` over a list made here - a haystack matches exactly when this test gave it one of the two endings and no
// "test", and a literal suffix scores the same for every haystack, so the expected records are known without another matcher.
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

static bool parsed(const char* query, const std::vector<std::string>& needles, const std::vector<uint32_t>& ids) {
    std::vector<uint32_t> got_ids;
    const std::vector<Pattern> pats = Pattern::parse_query_groups(query, &got_ids);
    if (pats.size() != needles.size() || got_ids != ids) return false;
    for (size_t i = 0; i < pats.size(); i++)
        if (pats[i].needle != needles[i]) return false;
    return true;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && !strcmp(argv[1], "gpu");
    static_assert(FZB_GROUP_ALTS_MAX == 8, "the limit the header states");
    if (!gpu) {
        CHECK(parsed("a | b", {"a", "b"}, {0, 0}));
        CHECK(parsed("a | b | c", {"a", "b", "c"}, {0, 0, 0}));
        CHECK(parsed("a | !b", {"a", "|", "b"}, {0, 1, 2}));
        CHECK(parsed("| a", {"|", "a"}, {0, 1}));
        CHECK(parsed("a |", {"a", "|"}, {0, 1}));
        CHECK(parsed("a | | b", {"a", "|", "|", "b"}, {0, 1, 2, 3}));
        CHECK(parsed("\\|", {"|"}, {0}));
        CHECK(parsed("a|b", {"a|b"}, {0}));
        CHECK(parsed("^src rs$ | py$ | go$ !test", {"src", "rs", "py", "go", "test"}, {0, 1, 1, 1, 2}));
        fzb_config cfg;
        fzb_config_default(&cfg);
        std::vector<fzb_pattern> pats(9);
        for (auto& p : pats) {
            memset(&p, 0, sizeof(p));
            p.needle_utf8 = (const uint8_t*)"ab";
            p.needle_len = 2;
            p.casing = p.unicode = p.matching = -1;
        }
        const uint32_t one_group[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, apart[3] = {0, 1, 0}, pair[2] = {5, 5};
        fzb_multi_matcher* mm = nullptr;
        CHECK(fzb_multi_matcher_create_groups(&cfg, pats.data(), 9, one_group, &mm) == FZB_ERR_INVALID && mm == nullptr);
        CHECK(strstr(fzb_last_error(), "FZB_GROUP_ALTS_MAX") != nullptr);
        CHECK(fzb_multi_matcher_create_groups(&cfg, pats.data(), 3, apart, &mm) == FZB_ERR_INVALID && strstr(fzb_last_error(), "adjacent") != nullptr);
        pats[1].negated = 1;
        CHECK(fzb_multi_matcher_create_groups(&cfg, pats.data(), 2, pair, &mm) == FZB_ERR_INVALID && strstr(fzb_last_error(), "negated") != nullptr);
        pats[1].negated = 0;
        CHECK(fzb_multi_matcher_create_groups(nullptr, pats.data(), 2, pair, &mm) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_create_groups(&cfg, nullptr, 2, pair, &mm) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_create_groups(&cfg, pats.data(), 2, pair, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_set_pattern_groups(nullptr, pats.data(), 2, pair) == FZB_ERR_INVALID && strstr(fzb_last_error(), "null") != nullptr);
        CHECK(fzb_multi_matcher_create_groups(&cfg, pats.data(), 8, one_group, &mm) == FZB_OK && mm != nullptr && fzb_multi_matcher_len(mm) == 8);
        CHECK(fzb_multi_matcher_set_pattern_groups(mm, pats.data(), 9, one_group) == FZB_ERR_INVALID && fzb_multi_matcher_len(mm) == 8);  // answers as before
        CHECK(fzb_multi_matcher_set_pattern_groups(mm, pats.data(), 2, pair) == FZB_OK && fzb_multi_matcher_len(mm) == 2);
        fzb_multi_matcher_free(mm);
        bool threw = false;
        try {
            Matcher::from_pattern_groups({Pattern("a"), Pattern("b")}, {0});
        } catch (const Error& e) {
            threw = e.code == FZB_ERR_INVALID;
        }
        CHECK(threw);
        Matcher grouped = Matcher::from_query_groups("rs$ | py$ !test");
        CHECK(grouped.patterns().size() == 3);
        if (failures) return 1;
        printf("test_facade_anyof: ok (host)\n");
        return 0;
    }
    try {
        std::vector<std::string> hs;
        const char* ends[] = {".rs", ".py", ".go", ".md"};
        for (int i = 0; i < 5000; i++) hs.push_back("src/" + std::string(i % 5 == 0 ? "test_" : "lib_") + std::to_string(i * 7919 % 10007) + ends[i % 4 == 3 ? 3 : (i / 3) % 3]);
        Corpus cp(hs);
        Matcher m = Matcher::from_query_groups("rs$ | py$ !test", Config().sort(SortStrategy::IndexAsc));
        const std::vector<Match> got = m.match_list(cp);
        std::vector<uint32_t> want;
        for (size_t i = 0; i < hs.size(); i++) {
            const std::string& h = hs[i];
            const std::string end = h.substr(h.size() - 3);
            if ((end == ".rs" || end == ".py") && h.find("test") == std::string::npos) want.push_back((uint32_t)i);
        }
        CHECK(want.size() > 1000 && want.size() < hs.size());
        CHECK(got.size() == want.size());
        for (size_t k = 0; k < got.size() && k < want.size(); k++) CHECK(got[k].index == want[k] && got[k].score == got[0].score && !got[k].exact);
        bool refused = false;
        try {
            m.match_list_top_indices(cp, 5);
        } catch (const Error& e) {
            refused = e.code == FZB_ERR_INVALID && strstr(e.what(), "any-of group") != nullptr;
        }
        CHECK(refused);
        CHECK(m.match_list(cp).size() == want.size());  // still answers
        m.set_patterns(Pattern::parse_query("rs$ !test"));  // single terms again
        CHECK(m.match_list(cp).size() < want.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("test_facade_anyof: ok\n");
    return 0;
}
