// The multi-pattern matcher through the C++ host side (include/frizbee_hip.hpp): `from_query` -> `set_patterns` (in place: the
// sub-matchers are rebuilt, their device buffers kept) -> `match_list_parallel(ShardedCorpus)` (the composition per shard, gathered and
// ordered on the root) must return `match_list`'s list and never throw.  Needs a GPU; the shards share it (oversubscribed).
#include <cstdio>
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

int main() {
    std::vector<std::string> hs;
    for (int i = 0; i < 20000; i++) {
        std::string h = "src/" + std::to_string(i * 7919 % 10007) + "/";
        if (i % 3 == 0) h += "linux/";
        if (i % 5 == 0) h += "test_";
        if (i % 7 == 0) h += "deadbeef";
        h += "file.cc";
        hs.push_back(h);
    }
    try {
        Corpus corpus(hs);
        ShardedCorpus sharded(hs, 3, /*by_bytes=*/true, /*oversubscribe=*/true);
        Matcher m = Matcher::from_query("src linux !test", Config().sort(SortStrategy::ScoreThenIndexDesc));
        const std::vector<Match> first = m.match_list_parallel(sharded);
        CHECK(!first.empty() && first == m.match_list(corpus));
        int checked = 0;
        for (const char* q : {"src li", "src linux", "src linux !t", "dead !x file", "!linux", "src linux !test", "", "linux"}) {
            m.set_patterns(Pattern::parse_query(q));
            const std::vector<Match> want = m.match_list(corpus);
            const std::vector<Match> got = m.match_list_parallel(sharded);
            CHECK(got == want);
            CHECK(got.size() == Matcher::from_query(q, m.config()).match_list(corpus).size());
            if (std::string(q).find(' ') != std::string::npos) CHECK(m.shard_report().find("shard 2 on device") != std::string::npos);
            checked++;
        }
        m.set_config(Config().sort(SortStrategy::IndexAsc));
        m.set_patterns(Pattern::parse_query("file !x"));
        CHECK(m.match_list_parallel(sharded) == m.match_list(corpus));
        CHECK(checked == 8);
    } catch (const std::exception& e) {
        fprintf(stderr, "threw: %s\n", e.what());
        return 1;
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("test_facade_multi: ok\n");
    return 0;
}
