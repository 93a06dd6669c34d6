// Tag facets through the C++ host side (include/frizbee_hip.hpp): Facets, Matcher::set_facets.  Without an argument: the host-only part
// (the calls compile and link, bad arguments are refused before a device is touched).  With "gpu": the counts of a query against a count
// made here from the same list - a haystack matches "linux" exactly when this test put "linux/" into it.
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
    static_assert(FZB_FACET_WORDS == 34, "matched, visible, two rows of 16");
    if (!gpu) {
        uint32_t words[FZB_FACET_WORDS];
        fzb_facets* f = nullptr;
        fzb_facets* fake = (fzb_facets*)64;  // never dereferenced: the argument checks come first
        CHECK(fzb_facets_create(nullptr, &f) == FZB_ERR_INVALID && f == nullptr);
        CHECK(fzb_facets_create((const fzb_corpus*)64, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_facets_read(nullptr, words) == FZB_ERR_INVALID);
        CHECK(fzb_facets_read(fake, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_facets_device(nullptr) == nullptr);
        CHECK(fzb_matcher_set_facets(nullptr, fake) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_set_facets(nullptr, nullptr) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        fzb_facets_free(nullptr);
        Matcher m(Pattern("linux"));
        m.set_facets(nullptr);  // detaching what was never attached is fine, with either form of the matcher
        Matcher q = Matcher::from_query("li nux !x");
        q.set_facets(nullptr);
        if (failures) return 1;
        printf("test_facade_facets: ok (host)\n");
        return 0;
    }
    try {
        std::vector<std::string> hs;
        std::vector<uint16_t> tags;
        for (int i = 0; i < 20000; i++) {
            std::string h = "src/" + std::to_string(i * 7919 % 10007) + "/";
            if (i % 3 == 0) h += "linux/";
            h += "file.cc";
            hs.push_back(h);
            tags.push_back((uint16_t)((i % 4 == 0 ? 1 : 0) | (i % 7 == 0 ? 2 : 0) | (i * 31 % 5 == 0 ? 0x8000 : 0)));
        }
        Corpus cp(hs);
        cp.set_tags(tags);
        Facets sink(cp);
        Matcher m(Pattern("linux"));
        m.set_facets(&sink);
        const uint16_t scopes[3][2] = {{0, 0}, {2, 1}, {1, 1}};
        for (const auto& sc : scopes) {
            cp.set_scope(sc[0], sc[1]);
            Facets::Counts want{};
            for (size_t i = 0; i < hs.size(); i += 3) {  // the haystacks that hold "linux/"
                const uint16_t t = tags[i];
                const bool vis = (t & sc[0]) == sc[0] && (t & sc[1]) == 0;
                want.matched++;
                want.visible += vis;
                for (int b = 0; b < 16; b++) {
                    want.all_by_bit[b] += (t >> b) & 1;
                    want.visible_by_bit[b] += vis ? (t >> b) & 1 : 0;
                }
            }
            size_t found = 0;
            (void)m.match_list_top(cp, 10, &found);
            const Facets::Counts got = sink.read();
            CHECK(got.matched == want.matched && got.visible == want.visible && got.visible == found);
            CHECK(got.all_by_bit == want.all_by_bit && got.visible_by_bit == want.visible_by_bit);
            CHECK(m.match_list(cp).size() == found && sink.read().matched == want.matched);
        }
        CHECK(sink.device() != nullptr);
        // the sink follows the matcher into its other form
        m.set_patterns(Pattern::parse_query("linux !zzz"));
        cp.set_scope(0, 0);
        size_t found = 0;
        (void)m.match_list_top(cp, 10, &found);
        CHECK(sink.read().matched == found && found == (hs.size() + 2) / 3);
        m.set_facets(nullptr);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("test_facade_facets: ok\n");
    return 0;
}
