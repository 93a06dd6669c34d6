// A per-haystack score bias, through the C++ host side (include/frizbee_hip.hpp): Corpus::set_bias / update_bias / clear_bias / bias_info.
// Without an argument: the host-only part (the calls compile and link, bad arguments are refused before a device is touched).  With
// "gpu": a biased corpus answers like the unbiased list with the bias added and the list ordered again on the host.
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

// what a caller without the device-side bias does: add, clamp, reverse for *Desc, stable sort by descending score
static std::vector<Match> host_biased(std::vector<Match> index_asc, const std::vector<int16_t>& bias, SortStrategy sort) {
    for (Match& m : index_asc) m.score = (uint16_t)std::min(65535, std::max(0, (int)m.score + (int)bias[m.index]));
    if (sort == SortStrategy::IndexDesc || sort == SortStrategy::ScoreThenIndexDesc) std::reverse(index_asc.begin(), index_asc.end());
    if (sort == SortStrategy::ScoreThenIndexAsc || sort == SortStrategy::ScoreThenIndexDesc)
        std::stable_sort(index_asc.begin(), index_asc.end(), [](const Match& a, const Match& b) { return a.score > b.score; });
    return index_asc;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && !strcmp(argv[1], "gpu");
    if (!gpu) {
        const int16_t val = 5;
        const uint32_t idx = 0;
        uint64_t info[4];
        fzb_corpus* fake = (fzb_corpus*)64;  // never dereferenced: the argument checks come first
        CHECK(fzb_corpus_set_bias(nullptr, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_set_bias(fake, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_bias(nullptr, &idx, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_bias(fake, nullptr, &val, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_update_bias(fake, &idx, nullptr, 1) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_clear_bias(nullptr) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_bias_info(nullptr, info) == FZB_ERR_INVALID);
        CHECK(fzb_corpus_bias_info(fake, nullptr) == FZB_ERR_INVALID);
        CHECK(strstr(fzb_last_error(), "null") != nullptr);
        int have = 0;
        if (fzb_device_count(&have) != FZB_OK || have == 0) {
            int threw = 0;
            try {
                Corpus c(std::vector<std::string>{"a"});
                c.set_bias({1});
                c.update_bias({0}, {2});
                c.clear_bias();
                (void)c.bias_info();
            } catch (const Error& e) {
                threw++;
            }
            CHECK(threw == 1);
        }
        if (failures) return 1;
        printf("test_facade_bias: ok (host)\n");
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
        std::vector<int16_t> bias(hs.size());
        for (size_t i = 0; i < hs.size(); i++) bias[i] = (int16_t)(i % 11 == 0 ? 300 : i % 7 == 0 ? -32768 : (int)(i * 31 % 81) - 40);
        Corpus cp(hs);
        CHECK(cp.bias_info().has_bias == 0);
        for (int multi = 0; multi < 2; multi++) {
            for (SortStrategy sort : {SortStrategy::ScoreThenIndexAsc, SortStrategy::ScoreThenIndexDesc, SortStrategy::IndexDesc}) {
                cp.clear_bias();
                Matcher plain = multi ? Matcher::from_query("src linux !test", Config().sort(SortStrategy::IndexAsc)) : Matcher("linux", Config().sort(SortStrategy::IndexAsc));
                Matcher m = multi ? Matcher::from_query("src linux !test", Config().sort(sort)) : Matcher("linux", Config().sort(sort));
                const std::vector<Match> unbiased = m.match_list(cp);
                const std::vector<Match> want = host_biased(plain.match_list(cp), bias, sort);
                CHECK(want.size() > 1000);
                cp.set_bias(bias);
                CHECK(cp.bias_info().has_bias == 1 && cp.bias_info().bias_hi == 300 && cp.bias_info().capacity >= hs.size());
                CHECK(m.match_list(cp) == want);
                size_t found = 0;
                CHECK(m.match_list_top(cp, 100, &found) == std::vector<Match>(want.begin(), want.begin() + 100) && found == want.size());
                const std::vector<MatchIndices> top = m.match_list_top_indices(cp, 10, &found);
                CHECK(top.size() == 10 && found == want.size());
                for (size_t k = 0; k < top.size(); k++) CHECK(top[k].index == want[k].index && top[k].score == want[k].score);
                cp.clear_bias();
                CHECK(cp.bias_info().has_bias == 0 && cp.bias_info().bias_hi == 0);
                CHECK(m.match_list(cp) == unbiased);
            }
        }
        cp.update_bias({3, 17}, {1000, -5});
        CHECK(cp.bias_info().has_bias == 1 && cp.bias_info().bias_hi == 1000);
        int threw = 0;
        try {
            cp.update_bias({3, 3}, {1, 2});
        } catch (const Error& e) {
            threw += e.code == FZB_ERR_INVALID;
        }
        try {
            cp.set_bias(std::vector<int16_t>(3, 0));
        } catch (const Error& e) {
            threw += e.code == FZB_ERR_INVALID;
        }
        CHECK(threw == 2 && cp.bias_info().bias_hi == 1000);
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_bias: ok\n");
    return 0;
}
