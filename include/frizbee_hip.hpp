// frizbee_hip.hpp - C++ host side over the C ABI of frizbee_hip.h, mirroring the reference crate's public interface for the
// list-matching path (the reference is Rust; there is no Rust toolchain in the build image, so the host-language mirror is C++):
// same type names, field names, defaults, method names and argument meaning, and the reference's panics become exceptions with
// the reference's panic text.  Header-only; link with -lfrizbee_hip.
//
//   reference                                            here
//   ---------------------------------------------------  ---------------------------------------------------------------
//   Scoring, Config (+ builder methods)   src/lib.rs:236-271, 439-478     frizbee::Scoring, frizbee::Config
//   CaseMatching / UnicodeMatching / SortStrategy / Matching  src/lib.rs:311-427   enum classes of the same names
//   Match { index, score, exact }          src/lib.rs:141-153             frizbee::Match
//   Pattern, PatternConfig, parse_query    src/pattern.rs:9-18, 186-262   frizbee::Pattern, frizbee::PatternConfig
//   Matcher::new / from_patterns / from_query / set_pattern / set_config / match_list / match_list_parallel / match_list_indices
//                                          src/matcher/mod.rs:90-222, parallel.rs:18-89          frizbee::Matcher
//   (the borrowed &[S: AsRef<str>])                                        frizbee::Corpus: the list packed once, resident in HBM
#pragma once
#include <cstdint>
#include <array>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "frizbee_hip.h"

namespace frizbee {

// The reference panics (assert!) in these situations; the message is the reference's panic text.
struct Panic : std::runtime_error { using std::runtime_error::runtime_error; };
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc == FZB_OK) return;
    const std::string msg = fzb_last_error();
    if (rc == FZB_ERR_PANIC) throw Panic(msg);
    throw Error(rc, msg);
}

enum class CaseMatching { Ignore = FZB_CASE_IGNORE, Smart = FZB_CASE_SMART, Respect = FZB_CASE_RESPECT };
enum class UnicodeMatching { Ignore = FZB_UNICODE_IGNORE, Smart = FZB_UNICODE_SMART, Always = FZB_UNICODE_ALWAYS };
enum class SortStrategy {
    ScoreThenIndexAsc = FZB_SORT_SCORE_THEN_INDEX_ASC,
    ScoreThenIndexDesc = FZB_SORT_SCORE_THEN_INDEX_DESC,
    IndexAsc = FZB_SORT_INDEX_ASC,
    IndexDesc = FZB_SORT_INDEX_DESC
};
enum class Matching { Fuzzy = FZB_MATCH_FUZZY, Exact = FZB_MATCH_EXACT, Prefix = FZB_MATCH_PREFIX, Suffix = FZB_MATCH_SUFFIX, Substring = FZB_MATCH_SUBSTRING };

struct Scoring {  // defaults: src/const.rs:1-10
    uint16_t match_score = 12, mismatch_penalty = 6, gap_open_penalty = 5, gap_extend_penalty = 1;
    uint16_t prefix_bonus = 12, capitalization_bonus = 4, matching_case_bonus = 4, exact_match_bonus = 8, delimiter_bonus = 4;
    fzb_scoring raw() const {
        return fzb_scoring{match_score, mismatch_penalty, gap_open_penalty, gap_extend_penalty, prefix_bonus, capitalization_bonus, matching_case_bonus, exact_match_bonus, delimiter_bonus};
    }
    bool operator==(const Scoring& o) const {
        return match_score == o.match_score && mismatch_penalty == o.mismatch_penalty && gap_open_penalty == o.gap_open_penalty && gap_extend_penalty == o.gap_extend_penalty &&
               prefix_bonus == o.prefix_bonus && capitalization_bonus == o.capitalization_bonus && matching_case_bonus == o.matching_case_bonus &&
               exact_match_bonus == o.exact_match_bonus && delimiter_bonus == o.delimiter_bonus;
    }
};

struct Config {  // src/lib.rs:236-271; the builder methods take and return by value like the Rust ones
    std::optional<uint16_t> max_typos_ = 0;
    CaseMatching casing_ = CaseMatching::Smart;
    UnicodeMatching unicode_ = UnicodeMatching::Smart;
    Matching matching_ = Matching::Fuzzy;
    SortStrategy sort_ = SortStrategy::ScoreThenIndexAsc;
    Scoring scoring_;
    // Not in the reference: which reference CPU backend the results are bit-exact against (see frizbee_hip.h). 0 / 0 = the one
    // frizbee would select on this host.
    uint16_t pf_lanes = 0, sw_lanes = 0;

    Config max_typos(std::optional<uint16_t> v) const { Config c = *this; c.max_typos_ = v; return c; }
    Config casing(CaseMatching v) const { Config c = *this; c.casing_ = v; return c; }
    Config unicode(UnicodeMatching v) const { Config c = *this; c.unicode_ = v; return c; }
    Config matching(Matching v) const { Config c = *this; c.matching_ = v; return c; }
    Config sort(SortStrategy v) const { Config c = *this; c.sort_ = v; return c; }
    Config scoring(const Scoring& v) const { Config c = *this; c.scoring_ = v; return c; }
    Config lanes(uint16_t pf, uint16_t sw = 0) const { Config c = *this; c.pf_lanes = pf; c.sw_lanes = sw; return c; }

    fzb_config raw() const {
        fzb_config r{};
        r.max_typos = max_typos_ ? (int32_t)*max_typos_ : -1;
        r.casing = (int32_t)casing_;
        r.unicode = (int32_t)unicode_;
        r.sort = (int32_t)sort_;
        r.scoring = scoring_.raw();
        r.pf_lanes = pf_lanes;
        r.sw_lanes = sw_lanes;
        r.matching = (int32_t)matching_;
        return r;
    }
};

struct Match {  // src/lib.rs:141-153
    uint32_t index;
    uint16_t score;
    bool exact;
    bool operator==(const Match& o) const { return index == o.index && score == o.score && exact == o.exact; }
};

struct MatchIndices {  // src/lib.rs:189-199
    uint16_t score;
    uint32_t index;
    bool exact;
    std::vector<uint32_t> indices;  // matched haystack byte positions, reverse order
    bool operator==(const MatchIndices& o) const { return index == o.index && score == o.score && exact == o.exact && indices == o.indices; }
};

struct PatternConfig {  // src/pattern.rs:230-244: every field optional, nullopt inherits the matcher's Config
    std::optional<uint16_t> max_typos;
    std::optional<CaseMatching> casing;
    std::optional<UnicodeMatching> unicode;
    std::optional<Matching> matching;
    std::optional<Scoring> scoring;
};

struct Pattern {  // src/pattern.rs:9-18
    std::string needle;
    bool negated = false;
    PatternConfig config;

    Pattern() = default;
    Pattern(const char* n) : needle(n) {}  // `impl From<&str> for Pattern`: matched literally, no syntax
    Pattern(std::string n, PatternConfig c = {}) : needle(std::move(n)), config(std::move(c)) {}
    Pattern with_negated(bool v) const { Pattern p = *this; p.negated = v; return p; }
    Pattern max_typos(std::optional<uint16_t> v) const { Pattern p = *this; p.config.max_typos = v; return p; }
    Pattern matching(std::optional<Matching> v) const { Pattern p = *this; p.config.matching = v; return p; }
    Pattern casing(std::optional<CaseMatching> v) const { Pattern p = *this; p.config.casing = v; return p; }

    // `Pattern::parse_query(query)` (src/pattern.rs:186-222): `^foo` prefix, `foo$` suffix, `^foo$` exact, `'foo` substring, `!foo`
    // negated (substring unless anchored), backslash escapes, atoms with an empty needle dropped
    static std::vector<Pattern> parse_query(std::string_view query) {
        fzb_pattern* arr = nullptr;
        size_t n = 0;
        check(fzb_parse_query((const uint8_t*)query.data(), query.size(), &arr, &n));
        std::vector<Pattern> out;
        for (size_t i = 0; i < n; i++) {
            Pattern p(std::string((const char*)arr[i].needle_utf8, arr[i].needle_len));
            p.negated = arr[i].negated != 0;
            if (arr[i].matching >= 0) p.config.matching = (Matching)arr[i].matching;
            out.push_back(std::move(p));
        }
        fzb_patterns_free(arr, n);
        return out;
    }
    // parse_query with the any-of operator (fzb_parse_query_groups): an atom that is exactly `|` joins the atoms around it into one group;
    // group_of[i] = the term id of pattern i, for Matcher::from_pattern_groups
    static std::vector<Pattern> parse_query_groups(std::string_view query, std::vector<uint32_t>* group_of) {
        fzb_pattern* arr = nullptr;
        uint32_t* ids = nullptr;
        size_t n = 0;
        check(fzb_parse_query_groups((const uint8_t*)query.data(), query.size(), &arr, &ids, &n));
        std::vector<Pattern> out;
        if (group_of) group_of->assign(ids, ids + n);
        for (size_t i = 0; i < n; i++) {
            Pattern p(std::string((const char*)arr[i].needle_utf8, arr[i].needle_len));
            p.negated = arr[i].negated != 0;
            if (arr[i].matching >= 0) p.config.matching = (Matching)arr[i].matching;
            out.push_back(std::move(p));
        }
        fzb_query_groups_free(arr, ids, n);
        return out;
    }
};

// The haystack list `match_list(&haystacks)` borrows: packed and uploaded once, it stays resident in HBM across queries.
class Corpus {
  public:
    template <typename Strings>  // any range of things convertible to std::string_view
    explicit Corpus(const Strings& haystacks) {
        std::string bytes;
        std::vector<uint64_t> ends;
        for (const auto& h : haystacks) {
            const std::string_view v(h);
            bytes.append(v.data(), v.size());
            ends.push_back(bytes.size());
        }
        fzb_corpus* c = nullptr;
        check(fzb_corpus_upload((const uint8_t*)bytes.data(), ends.data(), ends.size(), &c));
        h_.reset(c);
    }
    size_t len() const { return fzb_corpus_len(h_.get()); }
    const fzb_corpus* raw() const { return h_.get(); }
    // A corpus that grows (fzb_corpus_append and friends): the batch becomes haystacks len() .. of the resident list, only the batch
    // crosses the link.  `Corpus(std::vector<std::string>{})` followed by appends is how a picker starts.
    template <typename Strings>
    void append(const Strings& batch) {
        std::string bytes;
        std::vector<uint64_t> ends;
        for (const auto& h : batch) {
            const std::string_view v(h);
            bytes.append(v.data(), v.size());
            ends.push_back(bytes.size());
        }
        check(fzb_corpus_append(h_.get(), (const uint8_t*)bytes.data(), ends.data(), ends.size()));
    }
    // room for `items` haystacks and `bytes` padded bytes (<= raw bytes + 15 per haystack): appends within it allocate nothing
    void reserve(size_t items, uint64_t bytes) { check(fzb_corpus_reserve(h_.get(), items, bytes)); }
    void truncate(size_t n) { check(fzb_corpus_truncate(h_.get(), n)); }  // keep the first n haystacks; capacity is kept
    struct Info {
        uint64_t items, item_capacity, bytes, byte_capacity, max_len, uniform_len, has_view, view_nv, outliers, ends_u64, regrows, h2d_bytes;
    };
    Info info() const {
        uint64_t o[12] = {};
        check(fzb_corpus_info(h_.get(), o));
        return Info{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11]};
    }
    // the signatures' bit-planes of a list of short haystacks (fzb_corpus_signature_planes_info): device bytes, 0 without them
    uint64_t signature_planes_bytes() const {
        int built = 0;
        uint64_t bytes = 0;
        check(fzb_corpus_signature_planes_info(h_.get(), &built, &bytes));
        return built ? bytes : 0;
    }
    // the repeat planes beside them (fzb_corpus_signature_repeat_planes_info): device bytes, 0 without them
    uint64_t signature_repeat_planes_bytes() const {
        int built = 0;
        uint64_t bytes = 0;
        check(fzb_corpus_signature_repeat_planes_info(h_.get(), &built, &bytes));
        return built ? bytes : 0;
    }
    // A corpus that is edited (fzb_corpus_remove and friends): the other haystacks keep their order and are renumbered, as Vec::retain
    // would; only the indices - and a replace's new bytes - cross the link, nothing in front of the first touched haystack moves.
    void remove(const std::vector<uint32_t>& indices) { check(fzb_corpus_remove(h_.get(), indices.data(), indices.size())); }
    // the index list in HBM: entry k = the uint32 at byte k * stride_bytes, min(*dev_count, max_count) entries (stride 8: the records of
    // Matcher::match_list_device over the whole corpus - "drop everything that matches")
    void remove_device(const void* dev_indices, size_t stride_bytes, const uint32_t* dev_count, size_t max_count) {
        check(fzb_corpus_remove_device(h_.get(), dev_indices, stride_bytes, dev_count, max_count));
    }
    // batch item k becomes the content of haystack indices[k] (unique indices, any order)
    template <typename Strings>
    void replace(const std::vector<uint32_t>& indices, const Strings& batch) {
        std::string bytes;
        std::vector<uint64_t> ends;
        for (const auto& h : batch) {
            const std::string_view v(h);
            bytes.append(v.data(), v.size());
            ends.push_back(bytes.size());
        }
        if (ends.size() != indices.size()) throw Error(FZB_ERR_INVALID, "Corpus::replace: one haystack per index");
        check(fzb_corpus_replace(h_.get(), indices.data(), indices.size(), (const uint8_t*)bytes.data(), ends.data()));
    }
    struct EditInfo {
        uint64_t first, bytes_written, view_tiles, temp_bytes;
    };
    EditInfo edit_info() const {
        uint64_t o[4] = {};
        check(fzb_corpus_edit_info(h_.get(), o));
        return EditInfo{o[0], o[1], o[2], o[3]};
    }
    // A per-haystack score bias (fzb_corpus_set_bias and friends): one int16 per haystack, added on the device to every record's score before
    // anything selects or orders - reported score = clamp(score + bias[index], 0, 65535).  It belongs to the list: it survives set_pattern
    // and follows append / truncate / remove / replace.
    void set_bias(const std::vector<int16_t>& values) { check(fzb_corpus_set_bias(h_.get(), values.data(), values.size())); }
    // bias[indices[k]] = values[k] (unique indices in range); a corpus without a bias gets an all-zero one first
    void update_bias(const std::vector<uint32_t>& indices, const std::vector<int16_t>& values) {
        if (indices.size() != values.size()) throw Error(FZB_ERR_INVALID, "Corpus::update_bias: one value per index");
        check(fzb_corpus_update_bias(h_.get(), indices.data(), values.data(), indices.size()));
    }
    void clear_bias() { check(fzb_corpus_clear_bias(h_.get())); }
    struct BiasInfo {
        uint64_t has_bias, capacity, bias_hi, device_bytes;
    };
    BiasInfo bias_info() const {
        uint64_t o[4] = {};
        check(fzb_corpus_bias_info(h_.get(), o));
        return BiasInfo{o[0], o[1], o[2], o[3]};
    }
    // Per-haystack tags and a visibility scope (fzb_corpus_set_tags and friends): one uint16 of caller-defined bits per haystack; haystack i
    // is visible iff (tags[i] & require) == require && (tags[i] & exclude) == 0, and a query returns what it returns over the visible
    // haystacks alone, every index that of the full list.  The tags belong to the list; set_scope is host-only (the toggle keystroke).
    void set_tags(const std::vector<uint16_t>& values) { check(fzb_corpus_set_tags(h_.get(), values.data(), values.size())); }
    void update_tags(const std::vector<uint32_t>& indices, const std::vector<uint16_t>& values) {
        if (indices.size() != values.size()) throw Error(FZB_ERR_INVALID, "Corpus::update_tags: one value per index");
        check(fzb_corpus_update_tags(h_.get(), indices.data(), values.data(), indices.size()));
    }
    void clear_tags() { check(fzb_corpus_clear_tags(h_.get())); }
    void set_scope(uint16_t require = 0, uint16_t exclude = 0) { check(fzb_corpus_set_scope(h_.get(), require, exclude)); }
    struct ScopeInfo {
        uint64_t active, capacity, scope, device_bytes;
        uint16_t require() const { return (uint16_t)(scope & 0xFFFF); }
        uint16_t exclude() const { return (uint16_t)(scope >> 16); }
    };
    ScopeInfo scope_info() const {
        uint64_t o[4] = {};
        check(fzb_corpus_scope_info(h_.get(), o));
        return ScopeInfo{o[0], o[1], o[2], o[3]};
    }

    // the list's generation: + 1 for every append / truncate / remove / replace that changed it (what a Subset is checked against)
    uint64_t generation() const {
        uint64_t g = 0;
        check(fzb_corpus_generation(h_.get(), &g));
        return g;
    }

  private:
    struct Del { void operator()(fzb_corpus* c) const { fzb_corpus_free(c); } };
    std::unique_ptr<fzb_corpus, Del> h_;
};

// A candidate set of one resident Corpus (fzb_subset): strictly ascending haystack indices in HBM - the input or the captured match set of
// Matcher::match_list / match_list_top / match_list_top_device / match_list_top_indices with a Subset.  A query over a subset returns what it
// returns over an upload of those haystacks alone, every index that of the full list.  The reference has no counterpart.  The corpus must
// outlive the subset.
class Subset {
  public:
    explicit Subset(const Corpus& corpus) : corpus_(corpus.raw()) {
        fzb_subset* s = nullptr;
        check(fzb_subset_create(corpus_, &s));
        h_.reset(s);
    }
    void set_indices(const std::vector<uint32_t>& ascending) { check(fzb_subset_set_indices(h_.get(), ascending.data(), ascending.size())); }
    void from_scope(uint16_t require = 0, uint16_t exclude = 0) { check(fzb_subset_from_scope(h_.get(), corpus_, require, exclude)); }
    struct Info {
        uint64_t known, count, capacity, generation;
    };
    Info info() const {
        uint64_t o[4] = {};
        check(fzb_subset_info(h_.get(), o));
        return Info{o[0], o[1], o[2], o[3]};
    }
    size_t len() const { return (size_t)info().count; }  // (synchronises when the last capture left the count on the device only)
    std::vector<uint32_t> read() const {
        std::vector<uint32_t> v(len());
        size_t n = 0;
        check(fzb_subset_read(h_.get(), v.data(), v.size(), &n));
        v.resize(n);
        return v;
    }
    fzb_subset* raw() const { return h_.get(); }

  private:
    struct Del { void operator()(fzb_subset* s) const { fzb_subset_free(s); } };
    const fzb_corpus* corpus_;
    std::unique_ptr<fzb_subset, Del> h_;
};

// A facet sink of one resident Corpus (fzb_facets): the per-tag match counts of a query, counted on the device.  Attached with
// Matcher::set_facets / MultiMatcher::set_facets, it is filled by every query that honours it; read() returns the counts of the last such
// query's match set (what a capture would hold: before scope, bias, limit and ordering).  The reference has no counterpart.  The corpus
// must outlive the sink, and the sink every matcher it is attached to.
class Facets {
  public:
    struct Counts {
        uint32_t matched, visible;
        std::array<uint32_t, 16> all_by_bit, visible_by_bit;  // all_by_bit counts hidden matches too: a chip for an excluded bit shows what it hides
    };
    explicit Facets(const Corpus& corpus) {
        fzb_facets* f = nullptr;
        check(fzb_facets_create(corpus.raw(), &f));
        h_.reset(f);
    }
    Counts read() const {  // (after a _device form: waits for that form's stream)
        uint32_t w[FZB_FACET_WORDS] = {};
        check(fzb_facets_read(h_.get(), w));
        Counts c{w[0], w[1], {}, {}};
        for (int b = 0; b < 16; b++) {
            c.all_by_bit[b] = w[2 + b];
            c.visible_by_bit[b] = w[18 + b];
        }
        return c;
    }
    const uint32_t* device() const { return fzb_facets_device(h_.get()); }  // FZB_FACET_WORDS uint32 in device memory
    fzb_facets* raw() const { return h_.get(); }

  private:
    struct Del { void operator()(fzb_facets* f) const { fzb_facets_free(f); } };
    std::unique_ptr<fzb_facets, Del> h_;
};

// The list cut into one contiguous shard per GPU (fzb_corpus_upload_sharded): the devices of a node in the role of
// `match_list_parallel`'s worker threads (src/matcher/parallel.rs:18-89).  `gpus == 0`: every visible device.
class ShardedCorpus {
  public:
    template <typename Strings>
    explicit ShardedCorpus(const Strings& haystacks, int gpus = 0, bool by_bytes = false, bool oversubscribe = false) {
        std::string bytes;
        std::vector<uint64_t> ends;
        for (const auto& h : haystacks) {
            const std::string_view v(h);
            bytes.append(v.data(), v.size());
            ends.push_back(bytes.size());
        }
        if (gpus == 0) check(fzb_device_count(&gpus));
        fzb_sharded_corpus* c = nullptr;
        check(fzb_corpus_upload_sharded((const uint8_t*)bytes.data(), ends.data(), ends.size(), gpus,
                                        (by_bytes ? FZB_SHARD_BY_BYTES : 0) | (oversubscribe ? FZB_SHARD_OVERSUBSCRIBE : 0), &c));
        h_.reset(c);
    }
    size_t len() const { return fzb_sharded_corpus_len(h_.get()); }
    int shards() const { return fzb_sharded_corpus_shards(h_.get()); }
    const fzb_sharded_corpus* raw() const { return h_.get(); }

  private:
    struct Del { void operator()(fzb_sharded_corpus* c) const { fzb_sharded_corpus_free(c); } };
    std::unique_ptr<fzb_sharded_corpus, Del> h_;
};

// One process per GPU (fzb_shard_comm, csrc/host_rccl.hip): the ranks in the role of `match_list_parallel`'s worker threads, the runs moved by
// RCCL below the C ABI.  `ShardComm::unique_id()` on rank 0, its 128 bytes to the other ranks by whatever started them, then the constructor
// on every rank (collective) with the rank's GPU current.
class ShardComm {
  public:
    using Id = std::array<uint8_t, FZB_RCCL_ID_BYTES>;
    static Id unique_id() {
        Id id{};
        check(fzb_rccl_unique_id(id.data()));
        return id;
    }
    ShardComm(const Id& id, int rank, int world) {
        fzb_shard_comm* c = nullptr;
        check(fzb_shard_comm_create(id.data(), rank, world, &c));
        h_.reset(c);
    }
    int rank() const { return fzb_shard_comm_rank(h_.get()); }
    int world() const { return fzb_shard_comm_world(h_.get()); }
    fzb_shard_comm* raw() const { return h_.get(); }

  private:
    struct Del { void operator()(fzb_shard_comm* c) const { fzb_shard_comm_free(c); } };
    std::unique_ptr<fzb_shard_comm, Del> h_;
};

class Matcher {  // src/matcher/mod.rs:77-222
  public:
    // `Matcher::new(pattern, &config)`
    Matcher(const Pattern& pattern, const Config& config = {}) : Matcher(std::vector<Pattern>{pattern}, config) {}
    // `Matcher::from_patterns(&patterns, &config)`
    Matcher(const std::vector<Pattern>& patterns, const Config& config) : config_(config), patterns_(patterns) { build(); }
    static Matcher from_patterns(const std::vector<Pattern>& patterns, const Config& config = {}) { return Matcher(patterns, config); }
    // any-of groups: group_of[i] = the term id of pattern i; patterns with equal, adjacent ids are the alternatives of one group (matches when
    // any of them does, scores their maximum).  Always a composition; the forms with matched positions and the multi-device forms refuse it.
    // set_pattern / set_patterns make every pattern a single term again.
    static Matcher from_pattern_groups(const std::vector<Pattern>& patterns, const std::vector<uint32_t>& group_of, const Config& config = {}) {
        if (group_of.size() != patterns.size()) throw Error(FZB_ERR_INVALID, "from_pattern_groups: one term id per pattern");
        return Matcher(patterns, group_of, config);
    }
    static Matcher from_query_groups(std::string_view query, const Config& config = {}) {
        std::vector<uint32_t> group_of;
        const std::vector<Pattern> patterns = Pattern::parse_query_groups(query, &group_of);
        return Matcher(patterns, group_of, config);
    }
    // `Matcher::from_query(query, &config)`
    static Matcher from_query(std::string_view query, const Config& config = {}) { return Matcher(Pattern::parse_query(query), config); }

    const Config& config() const { return config_; }
    const std::vector<Pattern>& patterns() const { return patterns_; }

    // `set_pattern` / `set_patterns` / `set_config` (src/matcher/mod.rs:143-176).  A single plain pattern keeps its device workspace, and so
    // does a multi-pattern matcher that stays one (fzb_multi_matcher_set_patterns / _set_config rebuild its sub-matchers in place); only a
    // change between the two forms builds the other one.
    void set_pattern(const Pattern& p) {
        if (single_ && plain(p) && patterns_.size() == 1 && plain(patterns_[0])) {
            check(fzb_matcher_set_pattern(single_.get(), (const uint8_t*)p.needle.data(), p.needle.size()));
            patterns_ = {p};
            return;
        }
        set_patterns({p});
    }
    // the in-place re-query with a grouping (fzb_multi_matcher_set_pattern_groups: skipped when patterns and grouping are unchanged)
    void set_pattern_groups(const std::vector<Pattern>& patterns, const std::vector<uint32_t>& group_of) {
        if (group_of.size() != patterns.size()) throw Error(FZB_ERR_INVALID, "set_pattern_groups: one term id per pattern");
        if (multi_ && !group_of.empty()) {
            const std::vector<fzb_pattern> raw = raw_patterns(patterns);
            check(fzb_multi_matcher_set_pattern_groups(multi_.get(), raw.data(), raw.size(), group_of.data()));
            patterns_ = patterns;
            groups_ = group_of;
            return;
        }
        patterns_ = patterns;
        groups_ = group_of;
        build();
    }
    void set_patterns(const std::vector<Pattern>& patterns) {
        groups_.clear();
        if (multi_ && !is_single(patterns)) {
            const std::vector<fzb_pattern> raw = raw_patterns(patterns);
            check(fzb_multi_matcher_set_patterns(multi_.get(), raw.data(), raw.size()));
            patterns_ = patterns;
            return;
        }
        patterns_ = patterns;
        build();
    }
    void set_config(const Config& c) {
        config_ = c;
        if (single_) {
            const fzb_config r = resolve(patterns_[0]);
            check(fzb_matcher_set_config(single_.get(), &r));
        } else {
            const fzb_config r = config_.raw();
            check(fzb_multi_matcher_set_config(multi_.get(), &r));
        }
    }

    // Attach a facet sink (nullptr: detach): every query that honours it fills it, the others refuse the matcher until it is detached.  It
    // stays attached across set_pattern / set_patterns / set_config, also when they build the other form of the matcher.
    void set_facets(const Facets* facets) {
        facets_ = facets ? facets->raw() : nullptr;
        attach_facets();
    }

    // `match_list(&haystacks)`: ordered per config.sort
    std::vector<Match> match_list(const Corpus& corpus) {
        fzb_match* out = nullptr;
        size_t n = 0;
        if (single_) check(fzb_match_list(single_.get(), corpus.raw(), &out, &n));
        else check(fzb_multi_match_list(multi_.get(), corpus.raw(), &out, &n));
        return take(out, n);
    }
    template <typename Strings>
    std::vector<Match> match_list(const Strings& haystacks) { return match_list(Corpus(haystacks)); }

    // The first min(limit, found) entries of `match_list(&haystacks)`, selected and ordered on the device (fzb_match_list_top /
    // fzb_multi_match_list_top; the reference's caller truncates the Vec instead); *found = the length of the whole list.
    std::vector<Match> match_list_top(const Corpus& corpus, size_t limit, size_t* found = nullptr) {
        fzb_match* out = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        if (single_) check(fzb_match_list_top(single_.get(), corpus.raw(), limit, &out, &n, &f));
        else check(fzb_multi_match_list_top(multi_.get(), corpus.raw(), limit, &out, &n, &f));
        if (found) *found = (size_t)f;
        return take(out, n);
    }
    template <typename Strings>
    std::vector<Match> match_list_top(const Strings& haystacks, size_t limit, size_t* found = nullptr) { return match_list_top(Corpus(haystacks), limit, found); }
    // the same over a sharded list: every shard selects its own head, only those records travel to the root
    std::vector<Match> match_list_top(const ShardedCorpus& corpus, size_t limit, size_t* found = nullptr) {
        fzb_match* out = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        if (single_) check(fzb_match_list_top_sharded(single_.get(), corpus.raw(), limit, &out, &n, &f));
        else check(fzb_multi_match_list_top_sharded(multi_.get(), corpus.raw(), limit, &out, &n, &f));
        if (found) *found = (size_t)f;
        return take(out, n);
    }

    // The first min(limit, found) entries of `match_list_indices(&haystacks)` over the whole list (src/matcher/mod.rs:234-275; the
    // reference's caller truncates the Vec), `index` = the corpus index: fzb_match_list_top_indices - the top stage, a traced pass over its
    // head and the packing of the positions in one device call with one host wait - or fzb_multi_match_list_top_indices_fused, the same for
    // `from_patterns` with one traced pass per non-negated pattern and the union of their positions on the device (the host composition
    // fzb_multi_match_list_top_indices stays in the C ABI).
    std::vector<MatchIndices> match_list_top_indices(const Corpus& corpus, size_t limit, size_t* found = nullptr) {
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        if (single_) check(fzb_match_list_top_indices(single_.get(), corpus.raw(), limit, &out, &n, &pos, &f));
        else check(fzb_multi_match_list_top_indices_fused(multi_.get(), corpus.raw(), limit, &out, &n, &pos, &f));
        if (found) *found = (size_t)f;
        std::vector<MatchIndices> v(n);
        for (size_t i = 0; i < n; i++)
            v[i] = MatchIndices{out[i].score, out[i].index, out[i].exact != 0, std::vector<uint32_t>(pos + out[i].positions_begin, pos + out[i].positions_begin + out[i].positions_len)};
        fzb_match_indices_free(out, pos);
        return v;
    }
    template <typename Strings>
    std::vector<MatchIndices> match_list_top_indices(const Strings& haystacks, size_t limit, size_t* found = nullptr) { return match_list_top_indices(Corpus(haystacks), limit, found); }
    // the same left in HBM, asynchronous on `stream`: see fzb_match_list_top_indices_device for the four count words, and
    // fzb_multi_match_list_top_indices_device for the positions a `from_patterns` matcher needs room for
    void match_list_top_indices_device(const Corpus& corpus, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                       uint32_t* dev_count, void* stream = nullptr) {
        if (single_) check(fzb_match_list_top_indices_device(single_.get(), corpus.raw(), limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream));
        else check(fzb_multi_match_list_top_indices_device(multi_.get(), corpus.raw(), limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream));
    }
    // The same four calls over a candidate set (fzb_match_list_subset / fzb_multi_match_list_subset and friends): `in` = the haystacks looked
    // at (nullptr: the whole corpus), `capture` (nullptr: none) receives the indices of every haystack the matcher - `from_patterns`: the
    // composition - accepted, before bias, scope, limit and ordering.  in == capture is refused: alternate two subsets.
    std::vector<Match> match_list(const Corpus& corpus, const Subset* in, Subset* capture) {
        fzb_match* out = nullptr;
        size_t n = 0;
        if (single_) check(fzb_match_list_subset(single_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, &out, &n));
        else check(fzb_multi_match_list_subset(multi_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, &out, &n));
        return take(out, n);
    }
    std::vector<Match> match_list_top(const Corpus& corpus, const Subset* in, Subset* capture, size_t limit, size_t* found = nullptr) {
        fzb_match* out = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        if (single_) check(fzb_match_list_top_subset(single_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, limit, &out, &n, &f));
        else check(fzb_multi_match_list_top_subset(multi_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, limit, &out, &n, &f));
        if (found) *found = (size_t)f;
        return take(out, n);
    }
    void match_list_top_device(const Corpus& corpus, const Subset* in, Subset* capture, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream = nullptr) {
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_) check(fzb_match_list_top_subset_device(single_.get(), corpus.raw(), i, cp, limit, dev_out, capacity, dev_count, stream));
        else check(fzb_multi_match_list_top_subset_device(multi_.get(), corpus.raw(), i, cp, limit, dev_out, capacity, dev_count, stream));
    }
    // Sectioned top-`limit` (fzb_match_list_top_sections): the best `limit` matches of every tag section - a (require, exclude) pair over the
    // corpus' 16 tag bits, the scope's predicate - from ONE pass of the filter and the scorers and one host wait.  Element s is what
    // match_list_top(corpus, limit) returns over a corpus whose scope is the corpus' own scope AND section s.  At most FZB_SECTIONS_MAX
    // sections, limit <= FZB_SECTION_LIMIT_MAX.  The reference has no such call: its caller splits the Vec `match_list` returned.
    struct SectionHead {
        std::vector<Match> matches;
        size_t found;  // the section's visible matches
    };
    std::vector<SectionHead> match_list_top_sections(const Corpus& corpus, const std::vector<fzb_section>& sections, size_t limit, const Subset* in = nullptr,
                                                     Subset* capture = nullptr) {
        const size_t S = sections.size();
        fzb_match* out = nullptr;
        std::vector<size_t> lens(S ? S : 1, 0);
        std::vector<uint64_t> found(S ? S : 1, 0);
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_) check(fzb_match_list_top_sections(single_.get(), corpus.raw(), sections.data(), S, limit, i, cp, &out, lens.data(), found.data()));
        else check(fzb_multi_match_list_top_sections(multi_.get(), corpus.raw(), sections.data(), S, limit, i, cp, &out, lens.data(), found.data()));
        std::vector<SectionHead> heads(S);
        size_t at = 0;
        for (size_t s = 0; s < S; s++) {
            heads[s].found = (size_t)found[s];
            heads[s].matches.resize(lens[s]);
            for (size_t k = 0; k < lens[s]; k++) heads[s].matches[k] = Match{out[at + k].index, out[at + k].score, out[at + k].exact != 0};
            at += lens[s];
        }
        if (out) fzb_matches_free(out);
        return heads;
    }
    // the same with the heads left in HBM: section s at dev_out + s * limit, dev_counts[2s] records, dev_counts[2s + 1] matches; capacity >=
    // sections.size() * limit; asynchronous on `stream`
    void match_list_top_sections_device(const Corpus& corpus, const std::vector<fzb_section>& sections, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_counts,
                                        void* stream = nullptr, const Subset* in = nullptr, Subset* capture = nullptr) {
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_) check(fzb_match_list_top_sections_device(single_.get(), corpus.raw(), sections.data(), sections.size(), limit, i, cp, dev_out, capacity, dev_counts, stream));
        else check(fzb_multi_match_list_top_sections_device(multi_.get(), corpus.raw(), sections.data(), sections.size(), limit, i, cp, dev_out, capacity, dev_counts, stream));
    }
    // Sectioned top-`limit` WITH matched positions (fzb_match_list_top_sections_indices / fzb_multi_match_list_top_sections_indices): element s
    // is what match_list_top_indices(corpus, limit) returns over a corpus whose scope is the corpus' own scope AND section s - one pass of the
    // filter and the scorers, one traced pass over the heads (one per non-negated pattern), one host wait.  A haystack that sits in several
    // sections appears in each head with its positions.
    struct SectionHeadIndices {
        std::vector<MatchIndices> matches;
        size_t found;  // the section's visible matches
    };
    std::vector<SectionHeadIndices> match_list_top_sections_indices(const Corpus& corpus, const std::vector<fzb_section>& sections, size_t limit, const Subset* in = nullptr,
                                                                    Subset* capture = nullptr) {
        const size_t S = sections.size();
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        std::vector<size_t> lens(S ? S : 1, 0);
        std::vector<uint64_t> found(S ? S : 1, 0);
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_) check(fzb_match_list_top_sections_indices(single_.get(), corpus.raw(), sections.data(), S, limit, i, cp, &out, lens.data(), &pos, found.data()));
        else check(fzb_multi_match_list_top_sections_indices(multi_.get(), corpus.raw(), sections.data(), S, limit, i, cp, &out, lens.data(), &pos, found.data()));
        std::vector<SectionHeadIndices> heads(S);
        size_t at = 0;
        for (size_t s = 0; s < S; s++) {
            heads[s].found = (size_t)found[s];
            heads[s].matches.resize(lens[s]);
            for (size_t k = 0; k < lens[s]; k++) {
                const fzb_match_indices& r = out[at + k];
                heads[s].matches[k] = MatchIndices{r.score, r.index, r.exact != 0, std::vector<uint32_t>(pos + r.positions_begin, pos + r.positions_begin + r.positions_len)};
            }
            at += lens[s];
        }
        if (out || pos) fzb_match_indices_free(out, pos);
        return heads;
    }
    // the same left in HBM, asynchronous on `stream`: the heads densely concatenated in section order, capacity >= sections.size() * min(limit,
    // haystacks) records, positions_capacity >= that x the stride of match_list_top_indices_device, 2 * sections.size() + 4 words at dev_counts
    // (see fzb_match_list_top_sections_indices_device)
    void match_list_top_sections_indices_device(const Corpus& corpus, const std::vector<fzb_section>& sections, size_t limit, fzb_match_indices* dev_out, size_t capacity,
                                                uint32_t* dev_positions, size_t positions_capacity, uint32_t* dev_counts, void* stream = nullptr, const Subset* in = nullptr,
                                                Subset* capture = nullptr) {
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_)
            check(fzb_match_list_top_sections_indices_device(single_.get(), corpus.raw(), sections.data(), sections.size(), limit, i, cp, dev_out, capacity, dev_positions, positions_capacity,
                                                             dev_counts, stream));
        else
            check(fzb_multi_match_list_top_sections_indices_device(multi_.get(), corpus.raw(), sections.data(), sections.size(), limit, i, cp, dev_out, capacity, dev_positions,
                                                                   positions_capacity, dev_counts, stream));
    }
    // The empty prompt's _device forms (a matcher made from an empty needle; the _device forms above refuse one): the index-ordered list of the
    // haystacks of the range, or of `in`, visible under the corpus' scope - score = the clamped bias -, and its ordered head.  dev_count =
    // (records written, found); asynchronous on `stream`.
    void prompt_list_device(const Corpus& corpus, const Subset* in, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                            void* stream = nullptr) {
        if (!single_) throw Error(FZB_ERR_INVALID, "prompt_list_device: a from_patterns matcher has no empty needle");
        check(fzb_prompt_list_device(single_.get(), corpus.raw(), in ? in->raw() : nullptr, first, count, index_offset, dev_out, capacity, dev_count, stream));
    }
    void prompt_top_device(const Corpus& corpus, const Subset* in, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream = nullptr) {
        if (!single_) throw Error(FZB_ERR_INVALID, "prompt_top_device: a from_patterns matcher has no empty needle");
        check(fzb_prompt_top_device(single_.get(), corpus.raw(), in ? in->raw() : nullptr, limit, dev_out, capacity, dev_count, stream));
    }
    std::vector<MatchIndices> match_list_top_indices(const Corpus& corpus, const Subset* in, Subset* capture, size_t limit, size_t* found = nullptr) {
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        const fzb_subset* i = in ? in->raw() : nullptr;
        fzb_subset* cp = capture ? capture->raw() : nullptr;
        if (single_) check(fzb_match_list_top_indices_subset(single_.get(), corpus.raw(), i, cp, limit, &out, &n, &pos, &f));
        else check(fzb_multi_match_list_top_indices_subset(multi_.get(), corpus.raw(), i, cp, limit, &out, &n, &pos, &f));
        if (found) *found = (size_t)f;
        std::vector<MatchIndices> v(n);
        for (size_t i = 0; i < n; i++)
            v[i] = MatchIndices{out[i].score, out[i].index, out[i].exact != 0, std::vector<uint32_t>(pos + out[i].positions_begin, pos + out[i].positions_begin + out[i].positions_len)};
        fzb_match_indices_free(out, pos);
        return v;
    }
    // after reserve-ing the matcher for the corpus: no match_list_top_indices call with this limit or a smaller one, on a needle of up to
    // max_needle_bytes bytes, allocates device memory (`from_patterns`: while set_patterns / set_config add no pattern slot)
    void reserve_top_indices(const Corpus& corpus, size_t limit, size_t max_needle_bytes) {
        if (single_) check(fzb_matcher_reserve_top_indices(single_.get(), corpus.raw(), limit, max_needle_bytes));
        else check(fzb_multi_matcher_reserve_top_indices(multi_.get(), corpus.raw(), limit, max_needle_bytes));
    }
    // match_list_top_indices for a `from_patterns` matcher that may have any-of groups (fzb_multi_match_list_top_indices_groups): the records
    // are match_list_top's; a record's positions are the descending union of every plain non-negated pattern's and of each group's carrier's
    // only - the matching alternative with the largest key score << 1 | exact, the first in query order on equal keys.  Without a group: the
    // ungrouped call.
    std::vector<MatchIndices> match_list_top_indices_groups(const Corpus& corpus, size_t limit, size_t* found = nullptr, const Subset* in = nullptr, Subset* capture = nullptr) {
        if (!multi_) throw Error(FZB_ERR_INVALID, "match_list_top_indices_groups: a single-needle matcher has no groups");
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        uint64_t f = 0;
        check(fzb_multi_match_list_top_indices_groups(multi_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, limit, &out, &n, &pos, &f));
        if (found) *found = (size_t)f;
        std::vector<MatchIndices> v(n);
        for (size_t i = 0; i < n; i++)
            v[i] = MatchIndices{out[i].score, out[i].index, out[i].exact != 0, std::vector<uint32_t>(pos + out[i].positions_begin, pos + out[i].positions_begin + out[i].positions_len)};
        fzb_match_indices_free(out, pos);
        return v;
    }
    // the same left in HBM, asynchronous on `stream`: positions_capacity >= min(limit, haystacks) x groups_positions_stride()
    void match_list_top_indices_groups_device(const Corpus& corpus, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                              uint32_t* dev_count, void* stream = nullptr, const Subset* in = nullptr, Subset* capture = nullptr) {
        if (!multi_) throw Error(FZB_ERR_INVALID, "match_list_top_indices_groups_device: a single-needle matcher has no groups");
        check(fzb_multi_match_list_top_indices_groups_device(multi_.get(), corpus.raw(), in ? in->raw() : nullptr, capture ? capture->raw() : nullptr, limit, dev_out, capacity,
                                                             dev_positions, positions_capacity, dev_count, stream));
    }
    // U_g: the plain non-negated patterns' needle bytes + per group the largest among its alternatives
    size_t groups_positions_stride() const {
        if (!multi_) throw Error(FZB_ERR_INVALID, "groups_positions_stride: a single-needle matcher has no groups");
        size_t u = 0;
        check(fzb_multi_matcher_groups_positions_stride(multi_.get(), &u));
        return u;
    }
    void reserve_top_indices_groups(const Corpus& corpus, size_t limit, size_t max_needle_bytes) {
        if (!multi_) throw Error(FZB_ERR_INVALID, "reserve_top_indices_groups: a single-needle matcher has no groups");
        check(fzb_multi_matcher_reserve_top_indices_groups(multi_.get(), corpus.raw(), limit, max_needle_bytes));
    }

    // `match_list_indices(&haystacks)` (src/matcher/mod.rs:234-275; multi-pattern: match_one_indices_multi, multi.rs:56-82).
    // `selection`: corpus indices standing in for the haystack list (the top of a match_list result); empty optional = the whole corpus.
    std::vector<MatchIndices> match_list_indices(const Corpus& corpus, const std::optional<std::vector<uint32_t>>& selection = std::nullopt) {
        if (selection && selection->empty()) return {};
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        const uint32_t* sel = selection ? selection->data() : nullptr;
        const size_t nsel = selection ? selection->size() : 0;
        if (single_) check(fzb_match_list_indices(single_.get(), corpus.raw(), sel, nsel, &out, &n, &pos));
        else check(fzb_multi_match_list_indices(multi_.get(), corpus.raw(), sel, nsel, &out, &n, &pos));
        std::vector<MatchIndices> v(n);
        for (size_t i = 0; i < n; i++)
            v[i] = MatchIndices{out[i].score, out[i].index, out[i].exact != 0, std::vector<uint32_t>(pos + out[i].positions_begin, pos + out[i].positions_begin + out[i].positions_len)};
        fzb_match_indices_free(out, pos);
        return v;
    }
    template <typename Strings>
    std::vector<MatchIndices> match_list_indices(const Strings& haystacks) { return match_list_indices(Corpus(haystacks)); }

    // The per-item side of the interface (src/matcher/mod.rs:277-371), served by one batched device pass in list order:
    // `match_iter(haystacks)`: the matches in haystack order whatever config.sort says; `match_one(haystack, index)`
    std::vector<Match> match_iter(const Corpus& corpus, uint32_t index_offset = 0) {
        fzb_match* out = nullptr;
        size_t n = 0;
        const size_t count = fzb_corpus_len(corpus.raw());
        if (single_) check(fzb_match_list_into(single_.get(), corpus.raw(), 0, count, index_offset, &out, &n));
        else check(fzb_multi_match_list_into(multi_.get(), corpus.raw(), 0, count, index_offset, &out, &n));
        return take(out, n);
    }
    template <typename Strings>
    std::vector<Match> match_iter(const Strings& haystacks) { return match_iter(Corpus(haystacks)); }
    std::optional<Match> match_one(const std::string& haystack, uint32_t index) {
        auto v = match_iter(Corpus(std::vector<std::string>{haystack}), index);
        return v.empty() ? std::nullopt : std::optional<Match>(v[0]);
    }
    // `match_iter_indices(haystacks)` / `match_one_indices(haystack, index)`
    std::vector<MatchIndices> match_iter_indices(const Corpus& corpus, uint32_t index_offset = 0) {
        fzb_match_indices* out = nullptr;
        uint32_t* pos = nullptr;
        size_t n = 0;
        if (single_) check(fzb_match_list_indices_into(single_.get(), corpus.raw(), nullptr, 0, index_offset, &out, &n, &pos));
        else check(fzb_multi_match_list_indices_into(multi_.get(), corpus.raw(), nullptr, 0, index_offset, &out, &n, &pos));
        std::vector<MatchIndices> v(n);
        for (size_t i = 0; i < n; i++)
            v[i] = MatchIndices{out[i].score, out[i].index, out[i].exact != 0, std::vector<uint32_t>(pos + out[i].positions_begin, pos + out[i].positions_begin + out[i].positions_len)};
        fzb_match_indices_free(out, pos);
        return v;
    }
    template <typename Strings>
    std::vector<MatchIndices> match_iter_indices(const Strings& haystacks) { return match_iter_indices(Corpus(haystacks)); }
    std::optional<MatchIndices> match_one_indices(const std::string& haystack, uint32_t index) {
        auto v = match_iter_indices(Corpus(std::vector<std::string>{haystack}), index);
        return v.empty() ? std::nullopt : std::optional<MatchIndices>(v[0]);
    }

    // `match_list_parallel(&haystacks, threads)`: same result for every thread count; threads == 0 panics like the reference
    std::vector<Match> match_list_parallel(const Corpus& corpus, size_t threads) {
        if (threads == 0) throw Panic("threads must be positive");
        return match_list(corpus);
    }
    template <typename Strings>
    std::vector<Match> match_list_parallel(const Strings& haystacks, size_t threads) {
        if (threads == 0) throw Panic("threads must be positive");
        return match_list(Corpus(haystacks));
    }

    // `match_list_parallel` with one DEVICE per worker (fzb_match_list_parallel_sharded / fzb_multi_match_list_parallel_sharded): per
    // shard the pipeline - or the whole multi-pattern composition - on its GPU, the runs gathered and ordered once on the current device;
    // the same list `match_list` returns.
    std::vector<Match> match_list_parallel(const ShardedCorpus& corpus) {
        fzb_match* out = nullptr;
        size_t n = 0;
        if (single_) check(fzb_match_list_parallel_sharded(single_.get(), corpus.raw(), &out, &n));
        else check(fzb_multi_match_list_parallel_sharded(multi_.get(), corpus.raw(), &out, &n));
        return take(out, n);
    }
    // `match_list_parallel` with one PROCESS per worker (fzb_match_list_parallel_rccl, collective): this rank's share of the list (`shard`,
    // first global index `index_offset`); the whole list's result on rank 0 (`to_all`: on every rank), empty elsewhere.
    std::vector<Match> match_list_parallel(const Corpus& shard, uint32_t index_offset, ShardComm& comm, bool to_all = false) {
        fzb_match* out = nullptr;
        size_t n = 0;
        const int flags = to_all ? FZB_GATHER_ALL : FZB_GATHER_ROOT;
        if (single_) check(fzb_match_list_parallel_rccl(single_.get(), shard.raw(), index_offset, comm.raw(), flags, &out, &n));
        else check(fzb_multi_match_list_parallel_rccl(multi_.get(), shard.raw(), index_offset, comm.raw(), flags, &out, &n));
        return take(out, n);
    }
    // how the runs of the last sharded call reached the root device (gather form, peer access per shard)
    std::string shard_report() const {
        return std::string(single_ ? fzb_matcher_shard_report(single_.get()) : fzb_multi_matcher_shard_report(multi_.get()));
    }

  private:
    static bool plain(const Pattern& p) {
        return !p.negated && !p.config.max_typos && !p.config.casing && !p.config.unicode && !p.config.matching && !p.config.scoring;
    }
    fzb_config resolve(const Pattern& p) const {  // PatternConfig::resolve (src/pattern.rs:250-262)
        Config c = config_;
        if (p.config.max_typos) c.max_typos_ = p.config.max_typos;
        if (p.config.casing) c.casing_ = *p.config.casing;
        if (p.config.unicode) c.unicode_ = *p.config.unicode;
        if (p.config.matching) c.matching_ = *p.config.matching;
        if (p.config.scoring) c.scoring_ = *p.config.scoring;
        return c.raw();
    }
    // build_patterns (src/matcher/mod.rs:178-190): one non-negated pattern -> the single-pattern matcher
    static bool is_single(const std::vector<Pattern>& patterns, size_t* at = nullptr) {
        size_t live = 0, last = 0;
        for (size_t i = 0; i < patterns.size(); i++)
            if (!patterns[i].needle.empty()) { live++; last = i; }
        if (at) *at = last;
        return live == 1 && !patterns[last].negated;
    }
    static std::vector<fzb_pattern> raw_patterns(const std::vector<Pattern>& patterns) {  // (the needles stay the caller's)
        std::vector<fzb_pattern> raw(patterns.size());
        for (size_t i = 0; i < patterns.size(); i++) {
            const Pattern& p = patterns[i];
            fzb_pattern& r = raw[i];
            r = fzb_pattern{};
            r.needle_utf8 = (const uint8_t*)p.needle.data();
            r.needle_len = p.needle.size();
            r.negated = p.negated;
            r.has_max_typos = p.config.max_typos.has_value();
            r.max_typos = p.config.max_typos.value_or(0);
            r.casing = p.config.casing ? (int32_t)*p.config.casing : -1;
            r.unicode = p.config.unicode ? (int32_t)*p.config.unicode : -1;
            r.matching = p.config.matching ? (int32_t)*p.config.matching : -1;
            r.has_scoring = p.config.scoring.has_value();
            if (p.config.scoring) r.scoring = p.config.scoring->raw();
        }
        return raw;
    }
    Matcher(const std::vector<Pattern>& patterns, const std::vector<uint32_t>& group_of, const Config& config) : config_(config), patterns_(patterns), groups_(group_of) { build(); }
    void build() {
        single_.reset();
        multi_.reset();
        if (!groups_.empty()) {
            const std::vector<fzb_pattern> raw = raw_patterns(patterns_);
            const fzb_config c = config_.raw();
            fzb_multi_matcher* mm = nullptr;
            check(fzb_multi_matcher_create_groups(&c, raw.data(), raw.size(), groups_.data(), &mm));
            multi_.reset(mm);
            attach_facets();
            return;
        }
        size_t last = 0;
        if (is_single(patterns_, &last)) {
            const fzb_config r = resolve(patterns_[last]);
            fzb_matcher* m = nullptr;
            check(fzb_matcher_create(&r, (const uint8_t*)patterns_[last].needle.data(), patterns_[last].needle.size(), &m));
            single_.reset(m);
            if (patterns_.size() != 1) patterns_ = {patterns_[last]};
            attach_facets();
            return;
        }
        const std::vector<fzb_pattern> raw = raw_patterns(patterns_);
        const fzb_config c = config_.raw();
        fzb_multi_matcher* mm = nullptr;
        check(fzb_multi_matcher_create(&c, raw.data(), raw.size(), &mm));
        multi_.reset(mm);
        attach_facets();
    }
    void attach_facets() {
        if (single_) check(fzb_matcher_set_facets(single_.get(), facets_));
        if (multi_) check(fzb_multi_matcher_set_facets(multi_.get(), facets_));
    }
    static std::vector<Match> take(fzb_match* out, size_t n) {
        std::vector<Match> r(n);
        for (size_t i = 0; i < n; i++) r[i] = Match{out[i].index, out[i].score, out[i].exact != 0};
        fzb_matches_free(out);
        return r;
    }
    struct DelS { void operator()(fzb_matcher* m) const { fzb_matcher_free(m); } };
    struct DelM { void operator()(fzb_multi_matcher* m) const { fzb_multi_matcher_free(m); } };
    Config config_;
    std::vector<Pattern> patterns_;
    std::vector<uint32_t> groups_;  // from_pattern_groups: the term id of every pattern (empty: every pattern a term of its own)
    fzb_facets* facets_ = nullptr;  // the attached sink (not owned)
    std::unique_ptr<fzb_matcher, DelS> single_;
    std::unique_ptr<fzb_multi_matcher, DelM> multi_;
};

// `iter::FuzzyMatchExt` (src/matcher/iter.rs:35-126): `haystacks.iter().fuzzy_match(needle, &config)`
template <typename Strings>
inline std::vector<Match> fuzzy_match(const Strings& haystacks, const std::string& needle, const Config& config = Config()) {
    return Matcher(needle.c_str(), config).match_iter(haystacks);
}
template <typename Strings>
inline std::vector<MatchIndices> fuzzy_match_indices(const Strings& haystacks, const std::string& needle, const Config& config = Config()) {
    return Matcher(needle.c_str(), config).match_iter_indices(haystacks);
}

}  // namespace frizbee
