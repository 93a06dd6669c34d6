// The device-fused `match_list_top_indices` of a `from_patterns` matcher through the C++ host side (include/frizbee_hip.hpp) and the C ABI
// under it.  Without an argument: the host-only part (the calls compile and link; NULL arguments are refused; without a device the query fails
// loudly, never quietly).  With "gpu": the fused result is the head of `match_list_indices`' list over the whole corpus, and equals the host
// composition fzb_multi_match_list_top_indices record by record, also after set_patterns and reserve_top_indices.
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

// the two C entry points side by side on one matcher: records, positions and `found`
static bool same_as_host_composition(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit) {
    fzb_match_indices *a = nullptr, *b = nullptr;
    uint32_t *pa = nullptr, *pb = nullptr;
    size_t na = 0, nb = 0;
    uint64_t fa = 0, fb = 0;
    if (fzb_multi_match_list_top_indices(mm, c, limit, &a, &na, &pa, &fa) != FZB_OK) return false;
    if (fzb_multi_match_list_top_indices_fused(mm, c, limit, &b, &nb, &pb, &fb) != FZB_OK) {
        fzb_match_indices_free(a, pa);
        return false;
    }
    bool same = na == nb && fa == fb;
    for (size_t i = 0; same && i < na; i++) {
        same = a[i].index == b[i].index && a[i].score == b[i].score && (a[i].exact != 0) == (b[i].exact != 0) && a[i].positions_len == b[i].positions_len &&
               !memcmp(pa + a[i].positions_begin, pb + b[i].positions_begin, 4 * (size_t)a[i].positions_len);
    }
    fzb_match_indices_free(a, pa);
    fzb_match_indices_free(b, pb);
    return same;
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
    const fzb_config cfg = Config().raw();
    fzb_pattern* pats = nullptr;
    size_t npats = 0;
    const char* q = "src lin !test";
    CHECK(fzb_parse_query((const uint8_t*)q, strlen(q), &pats, &npats) == FZB_OK && npats == 3);
    fzb_multi_matcher* mm = nullptr;
    CHECK(fzb_multi_matcher_create(&cfg, pats, npats, &mm) == FZB_OK);
    if (!gpu) {
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        uint32_t words[4];
        const fzb_corpus* fake = (const fzb_corpus*)(uintptr_t)64;  // never dereferenced: the NULL checks come first
        CHECK(fzb_multi_match_list_top_indices_fused(nullptr, fake, 1, &out, &n, &pos, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_indices_fused(mm, nullptr, 1, &out, &n, &pos, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_indices_device(mm, nullptr, 1, out, 0, pos, 0, words, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_match_list_top_indices_device(mm, fake, 1, out, 0, pos, 0, nullptr, nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_reserve_top_indices(nullptr, fake, 1, 8) == FZB_ERR_INVALID);
        CHECK(fzb_multi_matcher_reserve_top_indices(mm, nullptr, 1, 8) == FZB_ERR_INVALID);
        int threw = 0;
        try {
            Matcher m = Matcher::from_query("src lin !test");
            size_t found = 0;
            (void)m.match_list_top_indices(hs, 10, &found);
        } catch (const Error& e) {
            threw++;
        }
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) CHECK(threw == 1);
        fzb_multi_matcher_free(mm);
        fzb_patterns_free(pats, npats);
        if (failures) return 1;
        printf("test_facade_multi_top_indices: ok (host)\n");
        return 0;
    }
    try {
        Corpus corpus(hs);
        for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::IndexDesc}) {
            Matcher m = Matcher::from_query("src lin !test", Config().sort(sort));
            m.reserve_top_indices(corpus, 3000, 16);
            for (const char* query : {"src lin !test", "lin", "src 'linux ^src file.cc$", "!test !linux"}) {
                m.set_patterns(Pattern::parse_query(query));
                const std::vector<MatchIndices> all = m.match_list_indices(corpus);  // (the whole corpus as the list: `index` is the corpus index)
                CHECK(all.size() > 1000);
                for (size_t limit : {(size_t)0, (size_t)1, (size_t)100, (size_t)3000, all.size(), all.size() * 2}) {
                    size_t found = 0;
                    CHECK(m.match_list_top_indices(corpus, limit, &found) == head(all, limit) && found == all.size());
                }
            }
        }
        for (size_t limit : {(size_t)0, (size_t)7, (size_t)2500, (size_t)20000}) CHECK(same_as_host_composition(mm, corpus.raw(), limit));
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    fzb_multi_matcher_free(mm);
    fzb_patterns_free(pats, npats);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_multi_top_indices: ok\n");
    return 0;
}
