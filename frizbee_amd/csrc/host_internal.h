// Host-side internals shared by the translation units of the C ABI (host.hip: matcher + pipeline; host_upload.hip: corpus upload;
// host_shard.hip: the multi-device form).  Not part of the boundary: include/frizbee_hip.h is.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "../../include/frizbee_hip.h"
#include "fzb_internal.h"
#include "indices_union.h"
#include "indices_union_groups.h"
#include "knobs.h"

// error state of the calling thread (fzb_last_error) + the usual early return
int fzb_fail(int code, const std::string& msg);
void fzb_clear_error();
#define HIPCHK(expr)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// every device allocation of the library goes through here; the counter is fzb_debug_device_allocs (host.hip)
extern std::atomic<uint64_t> g_fzb_dev_allocs;
inline hipError_t fzb_dev_alloc(void** p, size_t bytes) {
    g_fzb_dev_allocs.fetch_add(1, std::memory_order_relaxed);
    return hipMalloc(p, bytes ? bytes : 16);
}

// A per-haystack side array ("column") of a corpus the library uploaded: one V per haystack beside the end offsets, room for cap_items
// (host_upload.hip keeps it in step with the list).  Every entry at or behind the list's length is ZERO, so appended
// haystacks start at 0; the capacity follows the corpus' cap_items once the array exists.  live = the editing family maintains the column:
// a truncate clears its cut entries, a removal compacts it, a regrow copies it.  A column that is not live is all zero, if it exists at all.
template <typename V>
struct ItemColumn {
    V* data = nullptr;
    u64 cap_items = 0;
    bool live = false;
};
template <typename V>
inline void fzb_column_release(ItemColumn<V>& col) {
    if (col.data) (void)hipFree(col.data);
    col = ItemColumn<V>{};
}

struct fzb_corpus {
    CorpusDev dev{};
    void* own_bytes = nullptr;
    void* own_ends = nullptr;
    void* own_view[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // the filter's view: vbytes, vgofs, vgnv, vlen, vperm, vlong (CorpusDev)
    // ---- a corpus that grows (fzb_corpus_append / _reserve / _truncate, host_upload.hip; only for a corpus the library uploaded) ----
    // Everything behind the used part of `own_bytes` and of the view's bytes is ZERO (cleared when allocated, again by truncate), so the
    // zero tail the kernels rely on is there wherever the list ends.
    u64 cap_items = 0;       // haystacks `own_ends` (and the view's per-item arrays) hold
    u64 cap_bytes = 0;       // bytes of `own_bytes`, the 96-byte tail included
    u64 min_len = ~(u64)0;   // shortest / longest haystack, more than 256 bytes, longest of those within 256: what decides uniform_len
    u64 max_len = 0;         // and whether the list calls for a view, kept on the host so that an append reads back its batch's stats only
    u64 n_over256 = 0;
    u64 max_short = 0;
    u64 view_units = 0;      // used part of the view's bytes in 16-byte units
    u64 view_items = 0;      // haystacks the view covers (the list's length while the corpus has a view)
    u64 view_cap_items = 0;  // haystacks the view's arrays hold (own_view[1..5]); view_cap_units: 16-byte units of own_view[0], slack excluded
    u64 view_cap_units = 0;
    void* own_sig = nullptr; // the letter signatures (CorpusDev::sig; also of a borrowed corpus: the library's own array), room for sig_cap_items haystacks
    u64 sig_cap_items = 0;
    void* own_planes = nullptr;  // the signatures' bit-planes (CorpusDev::sig_planes), room for planes_cap_tiles tiles of 4 KB; follows own_sig
    u64 planes_cap_tiles = 0;
    void* own_planes2 = nullptr;  // the REPEAT planes (CorpusDev::sig_planes2), room for planes2_cap_tiles tiles of 4 KB; follows own_planes
    u64 planes2_cap_tiles = 0;
    int sig_device = -1;     // a borrowed corpus: the device the signatures were built on (where its bytes live)
    // the two columns (ItemColumn above) and what is specific to each:
    // the score bias (fzb_corpus_set_bias / _update_bias, score_bias.h) is live while the queries add it - from set / update to clear,
    // which keeps the array, zeroed; the tags (fzb_corpus_set_tags / _update_tags / _set_scope, scope.h) are live from the moment they
    // exist and stay so after a clear.  The scope is two host words that travel as kernel arguments - haystack i is visible iff
    // (tags[i] & require) == require && (tags[i] & exclude) == 0.
    ItemColumn<int16_t> bias;
    u32 bias_hi = 0;         // upper bound of the largest positive entry (exact after set, never lowered by an update or an edit)
    ItemColumn<uint16_t> tags;
    u32 scope_require = 0, scope_exclude = 0;
    void* pair_stage = nullptr;  // landing place of an update's pairs, of either column (indices, then values), kept between calls
    u64 pair_stage_cap = 0;      // in pairs
    u64 regrows = 0;         // reallocations of the canonical arrays so far
    u64 h2d_bytes = 0;       // bytes copied host to device so far (haystack bytes + 8 per offset)
    u64 edit_info[4] = {0, 0, 0, 0};  // the last successful fzb_corpus_remove / _replace (fzb_corpus_edit_info)
    // staging of a batch, kept between appends: the batch as it arrived (bytes, u64 offsets), the layout pass' tile sums and stats
    void* stage_raw = nullptr;
    void* stage_ends = nullptr;
    void* stage_tiles = nullptr;
    void* stage_stats = nullptr;
    u64 stage_raw_cap = 0, stage_items_cap = 0, stage_tiles_cap = 0;
    int device = -1;         // where an uploaded corpus lives
    // bumped by every call that changed the LIST (append, truncate, remove, remove_device, replace; not by bias / tags / scope / reserve): a
    // candidate set (fzb_subset below) records it and is refused once it no longer matches (fzb_corpus_generation)
    u64 generation = 0;
};
// the haystacks a matcher's buffers are sized for: the list's length, or what fzb_corpus_reserve made room for
inline size_t fzb_corpus_reserved_items(const fzb_corpus* c) { return (size_t)(c->cap_items > c->dev.n ? c->cap_items : c->dev.n); }
// the corpus' score bias as the queries see it: nullptr / 0 without one
inline const int16_t* fzb_corpus_bias(const fzb_corpus* c) { return c->bias.live ? c->bias.data : nullptr; }
inline u32 fzb_corpus_bias_hi(const fzb_corpus* c) { return c->bias.live ? c->bias_hi : 0; }
// an active scope: (0, 0) is no scope, and a corpus without one takes the launches it took before tags existed
inline bool fzb_corpus_scoped(const fzb_corpus* c) { return c->tags.data && (c->scope_require | c->scope_exclude) != 0; }

// A CANDIDATE SET of one corpus (include/frizbee_hip.h, fzb_subset; host.hip): strictly ascending haystack indices in device memory with
// their count beside them, the input (`in`) or the captured match set (`capture`) of the *_subset queries.  idx has room for cap indices
// (created for fzb_corpus_reserved_items, grown geometrically when the list outgrew it); bitmap / tiles = the flag pass of
// fzb_subset_from_scope, sized with idx.  known: `count` on the host is the device's count (set-up calls and the host forms of the queries
// leave it known; a _device form's capture does not until fzb_subset_info asks, which synchronises).
struct fzb_subset {
    const fzb_corpus* corpus = nullptr;
    u64 generation = 0;
    u32* idx = nullptr;
    size_t cap = 0;
    u32* count_dev = nullptr;
    u64* bitmap = nullptr;
    u32* tiles = nullptr;
    bool known = true;
    u64 count = 0;
};

// A FACET SINK of one corpus (include/frizbee_hip.h, fzb_facets; facets.h; host.hip): the block of FZB_FACET_WORDS counts in device memory
// and its page-locked host mirror.  Attached to a matcher (MatcherState::facets, fzb_multi_matcher::facets), it is filled by every query
// that honours it: the block is cleared, counted into and copied to the mirror in stream order on the query's stream, and `done` is recorded
// behind the copy - an event of the sink's own, so nothing here outlives a stream the caller destroys.  A host form's one wait brings the
// counts back; a _device form leaves them behind `done` (fzb_facets_read waits for it only when it has not completed yet).
struct fzb_facets {
    const fzb_corpus* corpus = nullptr;
    u32* block = nullptr;   // device: FZB_FACET_WORDS words
    u32* mirror = nullptr;  // page-locked host copy
    hipEvent_t done = nullptr;  // recorded behind the last query's copy into the mirror when that query ran on a stream of the caller's
    bool on_event = false;  // the last query recorded `done`; else it ran on the null stream, which cannot be destroyed and is waited for itself
                            // (an event record costs a query 4 - 5 us, profiles/facets.txt: the host forms and stream 0 do not pay it)
    bool pending = false;   // a query was enqueued since the last read or the last wait known to cover it: `done` may not have completed
    int device = -1;
};

// A device buffer that only grows, for every helper that sizes one: fzb_dev_renew frees what *p holds and allocates `elems` anew (*p stays
// null when that fails); fzb_grow_dev does so when *p is missing or holds fewer than `want` elements (*have, the slack excluded).
template <typename T>
int fzb_dev_renew(T** p, size_t elems) {
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    HIPCHK(fzb_dev_alloc((void**)p, elems * sizeof(T)));
    return FZB_OK;
}
template <typename T>
int fzb_grow_dev(T** p, size_t* have, size_t want, size_t slack = 0) {
    if (*p && *have >= want) return FZB_OK;
    *have = 0;
    if (int rc = fzb_dev_renew(p, want + slack)) return rc;
    *have = want;
    return FZB_OK;
}
int fzb_sort_ensure(SortBuffers& s, size_t cap);  // host.hip
void fzb_sort_release(SortBuffers& s);

// what the synchronous entry points remember between two results (fetch_records, host.hip)
struct FetchHint {
    size_t last = 0;            // records of the previous result: the next one's records are copied speculatively, behind the count
    u32* count_host = nullptr;  // page-locked landing place of the counters: OUT_FETCH_WORDS words (below)
};
// staging of the synchronous entry points, of either matcher type: the device-side result and what the copies to the host remember.
// Every count pair of the library is (records written, matches found).
constexpr size_t PAIR_RECORDS = 0, PAIR_FOUND = 1;
// count_dev's words: the result pair, the producer's raw pair (pipeline / composition / a shard's selection) and the capture mirror - the
// first OUT_FETCH_WORDS are what fzb_fetch_records copies into FetchHint::count_host.  The sharded root (host_shard.hip) alternates its
// running totals between two blocks at 0 and OUT_SHARD_BLOCK, keeps the sticky "a run was truncated" word at OUT_SHARD_TRUNCATED and its
// top-`limit` result pair at OUT_SHARD_RESULT, which fzb_fetch_top copies from.
constexpr size_t OUT_RESULT = 0, OUT_SHARD_TRUNCATED = 2, OUT_RAW = 4, OUT_SHARD_BLOCK = 4, OUT_CAPTURE = 6, OUT_FETCH_WORDS = 8, OUT_SHARD_RESULT = 8, OUT_WORDS = 16;
static_assert(OUT_RAW + 2 <= OUT_CAPTURE && OUT_CAPTURE < OUT_FETCH_WORDS, "the capture mirror comes back with the fetched words, behind the raw pair");
static_assert(OUT_SHARD_TRUNCATED < OUT_FETCH_WORDS && OUT_SHARD_RESULT + OUT_FETCH_WORDS <= OUT_WORDS, "every fetch stays inside count_dev");
struct OutStaging {
    fzb_match_rec* out_dev = nullptr;
    size_t out_cap = 0;
    u32* count_dev = nullptr;
    FetchHint fetch;
    FetchHint fetch_top;  // the top-`limit` entry points' own (their result sizes say nothing about the next full list's)
};
int fzb_out_ensure(OutStaging& o, size_t count);  // host.hip
void fzb_out_release(OutStaging& o);

// The scratch of a query over a corpus with an active scope (scope.h; host.hip's apply_terms), of either matcher type: the producer - the
// pipeline, the multi-pattern composition - writes its index-ordered records here, one per haystack of the range at most, so nothing is
// truncated ahead of the drop and `found` stays exact; `words` = its count pair; bitmap / tiles = the flag pass' words and per-tile counts.
// Grown through fzb_grow_dev, touched only while the scope is active, sized ahead by fzb_matcher_reserve / fzb_multi_matcher_reserve on a
// corpus that carries tags.
struct ScopeScratch {
    fzb_match_rec* recs = nullptr;
    size_t recs_cap = 0;
    u64* bitmap = nullptr;
    size_t bitmap_words = 0;
    u32* tiles = nullptr;
    size_t tiles_cap = 0;
    u32* words = nullptr;
    size_t words_cap = 0;
};
int fzb_scope_ensure(ScopeScratch& s, size_t count);  // host.hip
int fzb_scope_ensure_flags(ScopeScratch& s, size_t count);  // bitmap / tiles / words alone: the empty prompt's producer writes no records ahead of its compaction
void fzb_scope_release(ScopeScratch& s);

// The buffers of the sectioned top-`limit` queries (sections.h; host.hip), of either matcher type: `words` = the stage's scratch (bins, cuts,
// tile rows: fzb_sections_scratch_words), `stage` = the host forms' device-side result - the 2S count words, the captured count, then from
// SEC_STAGE_RECORDS the n_sections * limit records, so that one copy brings all back; `slabs` = the form with matched positions: the stage's 2S
// count words, the host form's 2S + PACK_WORDS result words (its one copy takes SEC_SLAB_FETCH words from there) and its captured count, then
// from SECTIONS_SLAB_WORDS the n_sections * limit slab records that k_sec_items makes one dense head.  Grown through fzb_grow_dev on the first
// sectioned query, released with the matcher.
constexpr size_t PACK_WORDS = 4;  // what the pack kernels leave at dev_count: records, matches found, positions, "the passes disagree"
constexpr size_t SEC_STAGE_COUNTS = 0, SEC_STAGE_CAPTURE = 16, SEC_STAGE_RECORDS = 32;
constexpr size_t SEC_SLAB_COUNTS = 0, SEC_SLAB_RESULT = 16, SEC_SLAB_CAPTURE = 40, SEC_SLAB_FETCH = 32, SECTIONS_SLAB_WORDS = 48;
static_assert(SEC_STAGE_COUNTS + 2 * FZB_SECTIONS_MAX == SEC_STAGE_CAPTURE && SEC_STAGE_CAPTURE < SEC_STAGE_RECORDS, "the stage's counts end where its capture word begins");
static_assert(SEC_SLAB_COUNTS + 2 * FZB_SECTIONS_MAX <= SEC_SLAB_RESULT && SEC_SLAB_RESULT + 2 * FZB_SECTIONS_MAX + PACK_WORDS <= SEC_SLAB_CAPTURE, "the slabs' result words end before the capture");
static_assert(SEC_SLAB_CAPTURE < SEC_SLAB_RESULT + SEC_SLAB_FETCH && SEC_SLAB_RESULT + SEC_SLAB_FETCH <= SECTIONS_SLAB_WORDS, "one copy brings the result words and the capture back");
struct SectionsScratch {
    u32* words = nullptr;
    size_t words_cap = 0;
    u32* stage = nullptr;
    size_t stage_words = 0;
    u32* slabs = nullptr;
    size_t slabs_words = 0;
};
int fzb_sections_ensure(SectionsScratch& s, size_t n_records, size_t stage_records);  // host.hip
int fzb_sections_ensure_slabs(SectionsScratch& s, size_t slab_records);
void fzb_sections_release(SectionsScratch& s);

// "Head, pack, host copy" of the top-`limit` queries with matched positions (host.hip), of either matcher type: the top stage's sorted head and
// the pack's tile sums, for heads of up to `cap` records; the host forms' packed staging (records, dense positions) and what their previous
// result held (the guess of the next copy).  An owner's own per-record arrays beside the head have a capacity of their own.
struct TopStaging {
    fzb_match_rec* head = nullptr;
    u32* tiles = nullptr;
    size_t cap = 0;
    fzb_indices_rec* packed = nullptr;
    u32* dense = nullptr;
    size_t packed_cap = 0, dense_words = 0;
    size_t last_records = 0, last_positions = 0;
};
int fzb_top_ensure(TopStaging& t, size_t want, size_t position_words, bool staging);  // host.hip; staging: the host forms' packed result too
void fzb_top_release(TopStaging& t);

// A matcher is two things (struct fzb_matcher below).  CompiledNeedle: what (config, needle) compile to, on the host alone - compile_needle
// (host.hip) computes all of it and makes no HIP call.  fzb_matcher_set_pattern / _set_config replace it as a whole.
struct CompiledNeedle {
    fzb_config config{};
    std::string needle;
    bool empty = false, case_sensitive = false, unicode = false, use_u8 = false;
    int literal_mode = 0;  // 0 = fuzzy; else FZB_MATCH_EXACT / PREFIX / SUFFIX / SUBSTRING (src/literal)
    int rows = 0;
    NeedleDev nd{};
    LaunchCfg lc{};          // (num_cus is the bound device's, not the needle's: fzb_bind_device sets it, a needle change carries it over)
    std::vector<u64> table;  // host copy of the filter table
    std::vector<u8> dfa;     // host copy of the subsequence DFA
    std::vector<u8> uni_dfa; // unicode path, 0 typos: byte-level DFA of the exact prefilter (empty if it needs more than 255 states)
    int uni_dfa_states = 0;
    // typo configurations: the bit-vector LCS test of the streaming filter as a DFA over its REACHABLE states (empty when there are more
    // than 226): state 0 = nothing matched, states >= lcs_acc_lo accept (LCS >= rows - max_typos)
    std::vector<u8> lcs_dfa;
    int lcs_states = 0, lcs_acc_lo = 0;
    bool lcs_scalar = false;  // unicode typo configurations: `lcs_dfa` is the SCALAR-level automaton (exact criterion), not the byte-level one over the table's masks
    // The matcher's streaming automaton (cdfa_src: 1 = `dfa` (subsequence / KMP), 2 = `uni_dfa`, 3 = `lcs_dfa`) with G transitions composed
    // over its K byte classes: [256 bytes: byte -> class][states x K^G: next state], for the ragged filter (kernels_filter.hip,
    // k1_cdfa_ragged).  Empty when states x K^G does not fit 16 KB even for G = 2.
    std::vector<u8> cdfa;
    int cdfa_src = 0, cdfa_K = 0, cdfa_G = 0;
    // the needle's letter signature and whether the signature form of the filter may decide for it (sig_filter.h: fuzzy, 0 typos, ASCII, no NUL)
    u32 needle_sig = 0;
    u32 needle_sig2 = 0;  // its REPEAT signature (the bits the needle holds twice): 0 = the filter reads no repeat plane
    bool sig_eligible = false;
    // a needle beyond NeedleDev's arrays (> 64 bytes or > 63 rows): scalars in `ndl`, the arrays in one host blob with its section offsets
    // (MatcherState::long_blob_dev is its device copy, uploaded on first use: until then ndl's pointers are null)
    bool long_needle = false;
    bool long_dfa = false;  // a long ASCII needle of up to 200 rows, 0 typos: `dfa` holds its ordered-subsequence automaton and the streaming filter is the first stage
    bool long_upper = false;  // a long ASCII needle with an uppercase letter among its rows (k2d_dp_long's form)
    NeedleLongDev ndl{};
    std::vector<u8> long_blob_host;
    size_t long_off_c = 0, long_off_f = 0, long_off_uc = 0, long_off_uf = 0, long_off_ulen = 0;
};

// MatcherState: what a session has accumulated on the device - buffers, streams, events, pinned words, the multi-device form's clones and
// workers.  It survives a needle or config change untouched (but for the few resets rebuild_matcher names); release_state (host.hip) is the
// one place that frees what it owns.  A matcher that gains a buffer adds it here and there.
// the words of MatcherState::top_idx_words
constexpr size_t TOPIDX_HEAD = 0, TOPIDX_TRACED = 2, TOPIDX_RESULT = 4, TOPIDX_CAPTURE = 8, TOPIDX_WORDS = 16;
static_assert(TOPIDX_CAPTURE == TOPIDX_RESULT + PACK_WORDS && TOPIDX_CAPTURE < TOPIDX_WORDS, "the capture mirror is the word right behind the result words");
struct MatcherState : OutStaging {
    Workspace ws{};
    int device = -1;
    bool profiling = false;
    static constexpr int PROF_SLOTS = 32;  // ring of per-call events: [0]=pipeline start [1]=pipeline end [2],[3]=around the filter kernel [4]=before the scorers
    hipEvent_t evring[PROF_SLOTS][5] = {};
    hipStream_t aux_stream = nullptr;  // second stream of a query (multi-chunk scorer beside the class launches) and its fork / join events
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int ev_filter[PROF_SLOTS] = {};
    u64 prof_calls = 0;

    u32 last_counters[4] = {0, 0, 0, 0};
    // fzb_match_list_indices: the selection (+ its length), the positions (`stride` per record) and their counts
    u32* trace_sel = nullptr;
    u32* trace_pos = nullptr;
    u32* trace_npos = nullptr;
    size_t trace_cap = 0, trace_pos_words = 0;
    // fzb_match_list_top_indices*: the head, pack and host copy (TopStaging), the traced second pass' records and the
    // count words of both passes: the head pair, the traced pair, the host form's PACK_WORDS result words and, right behind them so that one
    // copy of PACK_WORDS + 1 words brings it along, the capture mirror
    TopStaging top;
    fzb_match_rec* top_traced = nullptr;
    size_t top_traced_cap = 0;
    u32* top_idx_words = nullptr;
    // a long needle's arrays on the device (the copy of CompiledNeedle::long_blob_host: dropped with the needle it belongs to) and the global
    // scratch of its kernels (N-typo path state, per-row previous-chunk vectors, traced cells)
    void* long_blob_dev = nullptr;
    u8* long_scratch = nullptr;
    size_t long_scratch_bytes = 0;
    // multi-device form (host_shard.hip): the per-shard clones of this matcher (their device state lives on the shard's device);
    // on a clone: its stream and the device it is bound to
    std::vector<fzb_matcher*> shard_clones;
    void* shard_workers = nullptr;     // on the parent: the persistent worker threads, one per shard (host_shard.hip)
    hipStream_t shard_stream = nullptr;  // on a clone: the shard's stream; on the parent: the root's stream (ordering + copy to the host)
    hipEvent_t shard_event = nullptr;    // on a clone: "the run has arrived on the root"
    u32* shard_count_host = nullptr;     // on a clone: page-locked landing place of its record count
    int shard_device = -1;
    // on the parent: peer access between the root and every other device a shard lived on, decided once per (root, device) pair
    // (1 = enabled in both directions: runs travel device to device over xGMI; 0 = refused by the runtime: hipMemcpyPeerAsync stages
    // them through host memory), and the last query's report of how every shard's run reached the root (fzb_matcher_shard_report)
    std::vector<std::array<int, 3>> shard_peers;  // {root, device, state}
    std::string shard_report;
    // an ordering host of summed multi-pattern scores (fzb_multi_matcher::order): the radix sort always takes both passes
    bool sum_scores = false;
    // sharded top-`limit` queries, on the root: the count pairs of the shards whose selected runs are copied (two words per shard)
    u32* top_words = nullptr;
    size_t top_words_cap = 0;  // in words
    ScopeScratch scope;        // queries over a corpus with an active scope: the pipeline's records ahead of the drop
    SectionsScratch sections;  // sectioned top-`limit` queries
    fzb_facets* facets = nullptr;  // the attached facet sink (fzb_matcher_set_facets; not owned): part of the session, so it survives set_pattern / set_config
};

struct fzb_matcher : CompiledNeedle, MatcherState {};

// ---- multi-pattern composition (src/matcher/multi.rs; host.hip) ----------------------------------------------------------
// the slots of fzb_multi_matcher::counts (slot k < 2 belongs to cand[k]; fzb_multi_count below) and the words of fzb_multi_matcher::top_words
constexpr size_t MCOUNT_NEGATED = 2, MCOUNT_ALTERNATIVE = 3, MCOUNT_SLOTS = 4, MCOUNT_SLOT_WORDS = 4;
constexpr size_t MTOP_HEAD = 0, MTOP_COMBINED = 2, MTOP_RESULT = 4, MTOP_CAPTURE = 8, MTOP_N_ITEMS = 10, MTOP_RAW = 12, MTOP_WORDS = 16;
static_assert(MTOP_CAPTURE == MTOP_RESULT + PACK_WORDS && MTOP_CAPTURE < MTOP_N_ITEMS && MTOP_RAW + 2 <= MTOP_WORDS, "the capture mirror is the word right behind the result words");
struct fzb_multi_matcher : OutStaging {  // (the staging of its synchronous entry points)
    fzb_config config{};
    struct Compiled { bool negated; fzb_matcher* m; };
    std::vector<Compiled> patterns;  // empty needles dropped (src/matcher/mod.rs:193-195)
    // sub-matchers beyond the compiled patterns, kept by fzb_multi_matcher_set_patterns for a later query with more patterns (slot order:
    // `patterns`, then these); released only by fzb_multi_matcher_free
    std::vector<fzb_matcher*> spare;
    // the patterns as the caller gave them (set_patterns: "skipped if the patterns are the same"); pattern.needle_utf8 is not kept
    struct Raw { std::string needle; fzb_pattern pattern; };
    std::vector<Raw> raw;
    // any-of groups (anyof.h): the term of every raw pattern, numbered 0, 1, .. in order (equal = alternatives of one group; without a
    // grouping every pattern is its own term), the same per COMPILED pattern, and whether some term has two or more compiled alternatives -
    // only then does the composition take the group steps and allocate `group_slots` / `group_hits` (for ranges of up to group_cap haystacks)
    std::vector<u32> raw_terms, terms;
    bool grouped = false;
    u32* group_slots = nullptr;           // one key per candidate position
    fzb_match_rec* group_hits = nullptr;  // an alternative's hits (the ping-pong lists hold the candidates and the group's result)
    size_t group_cap = 0;
    int num_cus = 0;
    // device buffers, grown on demand: two candidate lists (ping-pong), their lengths, the item list handed to the next pattern,
    // and the bitmap / per-tile counts of the negation's compaction
    size_t cap = 0;
    fzb_match_rec* cand[2] = {nullptr, nullptr};
    // `counts`: one slot of MCOUNT_SLOT_WORDS words per list (count, untruncated total) - the lengths of cand[0] and cand[1], the hits of a
    // negated pattern, the hits of a group's alternative (fzb_multi_count)
    u32* counts = nullptr;
    u32* items = nullptr;
    u64* bitmap = nullptr;
    u32* tile_counts = nullptr;
    SortBuffers sort{};  // ordering of the synchronous entry points
    // fzb_multi_match_list_top_indices_device / _fused: the head, pack and host copy (TopStaging) and, for heads of up to `top_rec_cap` records, the
    // item list every positive pattern traces (one list, shared), the combined records and union lengths k_multi_union writes.  `top_words`:
    // the head pair, the combined pair, the host form's PACK_WORDS result words, the capture mirror right behind them (one copy of
    // PACK_WORDS + 1 words brings it along), the item list's length and the composition's raw pair.  `top_pos_u`: the strided unions (U per
    // record).  Beyond IUNION_BY_VALUE positive patterns the union kernel reads its sources from `union_src` (what it holds:
    // `union_src_host`; written again only when a pattern or a buffer changed, ahead of the query's first launch) and keeps its cursors in
    // `union_cursors`.
    TopStaging top;
    fzb_match_rec* top_comb = nullptr;
    u32* top_items = nullptr;
    u32* top_npos_u = nullptr;
    size_t top_rec_cap = 0;  // of top_comb / top_items / top_npos_u
    u32* top_words = nullptr;
    u32* top_pos_u = nullptr;
    size_t top_pos_u_words = 0;
    IUnionSrc* union_src = nullptr;
    size_t union_src_cap = 0;
    std::vector<IUnionSrc> union_src_host;
    u32* union_cursors = nullptr;
    size_t union_cursor_words = 0;
    // fzb_multi_match_list_top_indices_groups*: the grouped tail's own buffers (indices_union_groups.h) - the alternatives' `where` maps side by
    // side (one clear covers them), and beyond IUNION_BY_VALUE sources their array on the device (what it holds: `gunion_src_host`) and three
    // scratch words per source and head record.  The haystack -> head position map is `group_slots`, free once the composition has finished.
    u32* gunion_where = nullptr;
    size_t gunion_where_words = 0;
    GUnionSrc* gunion_src = nullptr;
    size_t gunion_src_cap = 0;
    std::vector<GUnionSrc> gunion_src_host;
    u32* gunion_scratch = nullptr;
    size_t gunion_scratch_words = 0;
    // multi-device forms (host_shard.hip, host_rccl.hip): `order` = an empty-needle matcher that holds the root's ordering, staging and
    // gather state (merge_runs_on_device and the sharded driver take it like any matcher); `shard_clones[g]` composes shard g's run on
    // shard_devices[g] (-1 = not used yet) and writes it into the staging of order->shard_clones[g]
    ScopeScratch scope;  // queries over a corpus with an active scope: the composition's records ahead of the drop
    SectionsScratch sections;  // sectioned top-`limit` queries
    fzb_facets* facets = nullptr;  // the attached facet sink (fzb_multi_matcher_set_facets; not owned): survives set_patterns / set_config
    fzb_matcher* order = nullptr;
    std::vector<fzb_multi_matcher*> shard_clones;
    std::vector<int> shard_devices;
};
inline u32* fzb_multi_count(const fzb_multi_matcher* mm, size_t slot) { return mm->counts + MCOUNT_SLOT_WORDS * slot; }


// pooled page-locked host buffers (result lists, upload staging): get() returns nullptr on failure; put() returns false for a pointer
// that is not the pool's
void* fzb_pinned_get(size_t bytes);
bool fzb_pinned_put(void* p);

// host.hip internals used by the other translation units
int fzb_bind_device(fzb_matcher* m);
// count + records of a result in device memory -> a pooled pinned host buffer, with ONE synchronisation when the previous result's size
// was a good guess (host.hip); dev_words = 8 u32, the record count is word n_word, the others stay readable in h.count_host
// the wait of a synchronous entry point: polls the stream for up to FZB_SPIN_WAIT_US (default 1 ms), then blocks (host.hip)
hipError_t fzb_stream_wait(hipStream_t st);
int fzb_fetch_records(FetchHint& h, const void* dev_records, const u32* dev_words, int n_word, size_t capacity, hipStream_t st, fzb_match** out, size_t* out_len);
inline int fzb_ensure_out_staging(fzb_matcher* m, size_t count) { return fzb_out_ensure(*m, count); }
// top-`limit` queries (host.hip): the ordering flags of a matcher as fzb_order_begin decides them, the sort's buffers for `cap` records
// (the selection stage's input and scratch), the one-wait copy of (count pair, <= max_records records), the no-pattern result
// (bias_hi: fzb_corpus_bias_hi of the corpus the records come from - 0 without a corpus)
void fzb_order_flags(const fzb_matcher* m, u32 bias_hi, bool* reversed, bool* by_score, bool* one_pass);
inline int fzb_ensure_sort_buffers(fzb_matcher* m, size_t cap) { return fzb_sort_ensure(m->ws.sort, cap); }
int fzb_fetch_top(FetchHint& h, const void* dev_records, const u32* dev_words, size_t max_records, hipStream_t st, fzb_match** out, size_t* out_len, uint64_t* out_found);
int fzb_empty_pattern_top(size_t n, int sort, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
// the ordering post-step of `match_list` on the device (host.hip, next to fzb_sorted_range_device)
struct OrderPlan {
    bool reversed, by_score, one_pass, via_tmp;
    fzb_match_rec* in;  // where the index-ordered records have to be written before fzb_order_finish
};
int fzb_order_begin(fzb_matcher* m, size_t cap, fzb_match_rec* dev_out, OrderPlan* p, u32 bias_hi);
int fzb_order_finish(fzb_matcher* m, const OrderPlan& p, fzb_match_rec* dev_out, const u32* dev_count, hipStream_t stream);
// `Matcher::match_list` over the sub-range [first, first + count) of a corpus, records numbered from index_offset, ordered per
// config.sort on the device (fzb_match_list_sorted_device = the whole corpus from 0)
// k_merge_matches_by_* (src/k_merge.rs:56-132) over runs given by pointer
int fzb_k_merge_runs(int32_t sort, const fzb_match* const* runs, const size_t* run_lens, size_t nruns, fzb_match* out);
void fzb_shard_workers_free(void* workers);  // host_shard.hip
// The multi-device query over a sharded corpus for either matcher type (host_shard.hip): `root` holds the ordering / staging / gather state
// and one clone per shard whose stream and staging carry that shard's run; run(g, carrier, shard, index_offset, stream) writes shard g's
// index-ordered records and their two count words into carrier->out_dev / carrier->count_dev (capacity carrier->out_cap) on `stream`.
using ShardRunFn = std::function<int(size_t g, fzb_matcher* carrier, const fzb_corpus* shard, uint32_t index_offset, hipStream_t stream)>;
int fzb_sharded_query(fzb_matcher* root, const fzb_sharded_corpus* sc, const ShardRunFn& run, fzb_match** out, size_t* out_len);
int fzb_sharded_top_query(fzb_matcher* root, const fzb_sharded_corpus* sc, const ShardRunFn& run, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
// CompiledPatterns::Empty over n haystacks: every index from index_offset, score 0, reversed for the *Desc strategies, never sorted (host list)
int fzb_empty_pattern_list(size_t n, uint32_t index_offset, int sort, fzb_match** out, size_t* out_len);
// the multi matcher's ordering host (created on first use, host.hip)
int fzb_multi_order_host(fzb_multi_matcher* mm, fzb_matcher** out);
int fzb_build_filter_view(fzb_corpus* c);     // host_upload.hip
// The letter signatures in step with the list (host_upload.hip): built from haystack n_valid on when the list is one k1_dfa serves (max_len known
// and <= 32), dropped otherwise.  Enqueued on the null stream of the current device; fzb_sig_sync_borrowed finds the device of a borrowed
// corpus itself and synchronises.
int fzb_sig_sync(fzb_corpus* c, u64 n_valid);
int fzb_sig_sync_borrowed(fzb_corpus* c);
// the refusal of an entry point that does not apply the corpus' score bias (host.hip): FZB_OK for an unbiased corpus
int fzb_refuse_biased(const fzb_corpus* c, const char* call, const char* instead);
// the same rule for the visibility scope: an entry point honours an active scope or refuses it (FZB_OK without one)
int fzb_refuse_scoped(const fzb_corpus* c, const char* call, const char* instead);
// the same rule for an attached facet sink (facets.h): an entry point fills it or refuses the matcher that carries one (FZB_OK without one)
int fzb_refuse_facets(const fzb_facets* f, const char* call);
// the same rule for any-of groups: an entry point composes them or refuses a matcher that has a term of two or more alternatives
int fzb_refuse_groups(const fzb_multi_matcher* mm, const char* call);
int fzb_sorted_range_device(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                            void* stream);
