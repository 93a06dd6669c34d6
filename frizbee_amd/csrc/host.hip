// Host side of the MI355X frizbee backend: the C ABI of include/frizbee_hip.h.
//
// Mirrors, in C++ (the reference is compiled Rust and no Rust toolchain exists in the build image):
//   Matcher::new / compile / get_backend      src/matcher/mod.rs:90-111, 178-204, 448-498
//   MatcherImpl::new                          src/matcher/algo.rs:57-71, 311-325
//   case_needle / case_needle_unicode         src/prefilter/mod.rs:49-96
//   score_fits_in_u8 / Scoring guards         src/smith_waterman/mod.rs:92-116, src/lib.rs:480-538
//   match_list / match_list_parallel post-steps  src/matcher/mod.rs:212-222, src/matcher/parallel.rs:18-89
//   radix_sort_matches / k_merge              src/sort.rs:6-40, src/k_merge.rs:56-170
// All scoring work happens in the gfx950 kernels; there is NO CPU fallback - without a HIP device every
// scoring entry point fails with FZB_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <map>
#include <unordered_map>
#include <vector>

#include "host_internal.h"
#include "sig_filter.h"
#include "score_bias.h"
#include "scope.h"
#include "sections.h"
#include "seg_list.h"

namespace {
#include "unicode_case_table.inc"

thread_local std::string g_err;
inline int fail(int code, const std::string& msg) { return fzb_fail(code, msg); }
// the three refusals many entry points share.  `items` haystacks numbered from index_offset pass the u32 index space; an output / positions
// buffer of `capacity` entries is smaller than the `want` the bound (`of`: "min(limit, haystacks)", ..) asks for
int refuse_index_overflow(u64 items, u64 index_offset = 0) {
    return fail(FZB_ERR_PANIC, "too many items in haystack, will overflow the u32 index: " + std::to_string(items) + " > 4294967295 (index offset: " + std::to_string(index_offset) + ")");
}
int refuse_small_output(const char* of, size_t capacity, size_t want) {
    return fail(FZB_ERR_CAPACITY, std::string("output buffer smaller than ") + of + ": " + std::to_string(capacity) + " < " + std::to_string(want));
}
int refuse_small_positions(const char* of, size_t capacity, size_t want) {
    return fail(FZB_ERR_CAPACITY, std::string("positions buffer smaller than ") + of + " x needle bytes: " + std::to_string(capacity) + " < " + std::to_string(want));
}

// ---- UTF-8 / case helpers ---------------------------------------------------------------------------
bool decode_utf8(const u8* s, size_t n, std::vector<u32>& out) {
    size_t i = 0;
    while (i < n) {
        u8 b = s[i];
        u32 cp;
        int len;
        if (b < 0x80) { cp = b; len = 1; }
        else if ((b & 0xE0) == 0xC0) { cp = b & 0x1F; len = 2; }
        else if ((b & 0xF0) == 0xE0) { cp = b & 0x0F; len = 3; }
        else if ((b & 0xF8) == 0xF0) { cp = b & 0x07; len = 4; }
        else return false;
        if (i + len > n) return false;
        for (int k = 1; k < len; k++) {
            if ((s[i + k] & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (s[i + k] & 0x3F);
        }
        // what a Rust &str can never hold: overlong forms, UTF-16 surrogates, scalars above U+10FFFF
        static const u32 min_cp[5] = {0, 0, 0x80, 0x800, 0x10000};
        if (cp < min_cp[len] || (cp >= 0xD800 && cp <= 0xDFFF) || cp > 0x10FFFF) return false;
        out.push_back(cp);
        i += len;
    }
    return true;
}
int encode_utf8(u32 cp, u8 out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (cp < 0x80) { out[0] = (u8)cp; return 1; }
    if (cp < 0x800) { out[0] = (u8)(0xC0 | (cp >> 6)); out[1] = (u8)(0x80 | (cp & 0x3F)); return 2; }
    if (cp < 0x10000) { out[0] = (u8)(0xE0 | (cp >> 12)); out[1] = (u8)(0x80 | ((cp >> 6) & 0x3F)); out[2] = (u8)(0x80 | (cp & 0x3F)); return 3; }
    out[0] = (u8)(0xF0 | (cp >> 18)); out[1] = (u8)(0x80 | ((cp >> 12) & 0x3F)); out[2] = (u8)(0x80 | ((cp >> 6) & 0x3F)); out[3] = (u8)(0x80 | (cp & 0x3F));
    return 4;
}
bool is_uppercase(u32 cp) {  // char::is_uppercase
    if (cp < 0x80) return cp >= 'A' && cp <= 'Z';
    const auto* end = FZB_UPPER_RANGES + FZB_UPPER_RANGES_LEN;
    const auto* it = std::upper_bound(FZB_UPPER_RANGES, end, cp, [](u32 v, const unsigned int (&r)[2]) { return v < r[0]; });
    if (it == FZB_UPPER_RANGES) return false;
    --it;
    return cp >= (*it)[0] && cp <= (*it)[1];
}
u32 flip_same_width(u32 cp) {  // the flip `case_needle_unicode` keeps (single scalar, same UTF-8 width), else cp
    if (cp < 0x80) return (cp >= 'A' && cp <= 'Z') ? cp + 32 : (cp >= 'a' && cp <= 'z') ? cp - 32 : cp;
    const auto* end = FZB_CASE_FLIP + FZB_CASE_FLIP_LEN;
    const auto* it = std::lower_bound(FZB_CASE_FLIP, end, cp, [](const unsigned int (&r)[2], u32 v) { return r[0] < v; });
    return (it != end && (*it)[0] == cp) ? (*it)[1] : cp;
}

// ---- Scoring guards (src/lib.rs:480-538, src/smith_waterman/mod.rs:92-116) --------------------------------
u16 sadd16(u32 a, u32 b) { return (u16)std::min<u32>(a + b, 0xFFFF); }
u16 ssub16(u32 a, u32 b) { return (u16)(a > b ? a - b : 0); }
u16 max_per_char_bonus(const fzb_scoring& s) {
    u16 bonus = std::max(s.delimiter_bonus, s.capitalization_bonus);
    u16 amortized = std::max<u16>((u16)((bonus + 1) / 2), ssub16(bonus, s.gap_open_penalty));
    return sadd16(amortized, s.matching_case_bonus);
}
u16 max_one_time_bonus(const fzb_scoring& s) {
    u16 bonus = std::max(s.delimiter_bonus, s.capitalization_bonus);
    u16 amortized = std::max<u16>((u16)((bonus + 1) / 2), ssub16(bonus, s.gap_open_penalty));
    return (u16)(bonus - amortized);
}
// Scoring::guard_against_score_overflow (src/lib.rs:506-537).  Fuzzy callers pass the amortised bonuses (src/matcher/algo.rs:311-325),
// the literal matcher its own (src/literal/algo.rs:314-322).
std::string overflow_guard(const fzb_scoring& s, size_t rows, int bonus_per_char = -1, int one_time = -1) {
    const u16 bpc = bonus_per_char < 0 ? max_per_char_bonus(s) : (u16)bonus_per_char;
    const u16 ot = one_time < 0 ? max_one_time_bonus(s) : (u16)one_time;
    u16 max_per_char = sadd16(s.match_score, bpc);
    if (max_per_char == 0) return "";
    u16 headroom = ssub16(ssub16(ssub16(ssub16(0xFFFF, s.prefix_bonus), s.exact_match_bonus), s.mismatch_penalty), ot);
    u16 max_needle_len = (u16)(headroom / max_per_char);
    if (rows > (size_t)max_needle_len)
        return "needle too long and could overflow the u16 score: " + std::to_string(rows) + " > " + std::to_string(max_needle_len);
    size_t max_gap = 32 * (size_t)s.gap_extend_penalty + (size_t)s.gap_open_penalty;
    if (max_gap > 0xFFFF) return "gap penalties too large and could overflow the u16 score: " + std::to_string(max_gap) + " > 65535";
    return "";
}
size_t max_matrix_score(const fzb_scoring& s, size_t needle_len) {
    size_t max_per_char = (size_t)s.match_score + (size_t)max_per_char_bonus(s);
    return max_per_char * needle_len + (size_t)max_one_time_bonus(s) + (size_t)s.prefix_bonus;
}
// What a matrix cell can REALLY reach: every row earns at most match + the larger of the delimiter / capitalisation bonus + the case bonus, the
// first one the prefix bonus.  max_matrix_score is the reference's guard, kept for what must agree with the reference (the score class, the
// overflow guard); it amortises the per-letter bonus over two rows or a gap, and a needle such as "/aA/aA" beats that - delimiter, lowercase
// behind it, capital behind the lowercase: two rows of every three earn the bonus with no gap (default scoring, 6 rows: 124 against 122).  Every
// gate that picks an arithmetic form or a pass count from "no value exceeds ..." takes this ceiling (tests/test_form_gates_host.py searches it).
size_t score_ceiling(const fzb_scoring& s, size_t needle_len) {
    const size_t per_char = (size_t)s.match_score + (size_t)std::max(s.delimiter_bonus, s.capitalization_bonus) + (size_t)s.matching_case_bonus;
    return per_char * needle_len + (size_t)s.prefix_bonus;
}
bool fits_in_u8(size_t needle_len, const fzb_scoring& s) {
    size_t max_constant = std::max<size_t>({(size_t)s.match_score + (size_t)s.mismatch_penalty, s.gap_open_penalty, s.gap_extend_penalty,
                                            s.matching_case_bonus, s.capitalization_bonus, s.delimiter_bonus, s.prefix_bonus});
    if (max_constant > 255) return false;
    if (64 * (size_t)s.gap_extend_penalty + (size_t)s.gap_open_penalty > 255) return false;
    return max_matrix_score(s, needle_len) + (size_t)s.mismatch_penalty <= 255;
}

// Which (prefilter lanes, score lanes) pair `Matcher::get_backend` picks on this host (src/matcher/mod.rs:448-498)
void detect_host_lanes(bool use_u8, int& pf, int& sw) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_cpu_init();
    const bool avx512 = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw");
    const bool bmi = __builtin_cpu_supports("bmi") && __builtin_cpu_supports("bmi2");
    const bool vbmi = __builtin_cpu_supports("avx512vbmi");
    const bool avx2 = __builtin_cpu_supports("avx2");
    const bool sse = __builtin_cpu_supports("sse2") && __builtin_cpu_supports("ssse3") && __builtin_cpu_supports("sse4.1");
    if (use_u8) {
        if (avx512 && bmi && vbmi) { pf = 64; sw = 64; return; }
        if (avx2) { pf = 32; sw = 32; return; }
        if (sse) { pf = 16; sw = 16; return; }
        pf = 16; sw = 16;  // scalar u8
    } else {
        if (avx512 && bmi) { pf = 64; sw = 32; return; }
        if (avx2) { pf = 32; sw = 16; return; }
        if (sse) { pf = 16; sw = 8; return; }
        pf = 16; sw = 8;  // scalar
    }
#else
    pf = 16;
    sw = use_u8 ? 16 : 8;  // NEON / scalar
#endif
}

hipError_t dev_alloc(void** p, size_t bytes) { return fzb_dev_alloc(p, bytes); }

}  // namespace

std::atomic<uint64_t> g_fzb_dev_allocs{0};

int fzb_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
void fzb_clear_error() { g_err.clear(); }

extern "C" {

const char* fzb_last_error(void) { return g_err.c_str(); }

}  // extern "C"
// ---- environment switches: parsed once (knobs.h) --------------------------------------------------------------------------------
namespace {
FzbKnobs parse_knobs() {
    FzbKnobs k;
    auto on = [](const char* name) { const char* e = getenv(name); return e != nullptr && atoi(e) != 0; };
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    k.debug_sync = set("FZB_DEBUG_SYNC");
    k.typo_exact_window = on("FZB_TYPO_EXACT_WINDOW");
    k.no_filter_view = getenv("FZB_FILTER_VIEW") != nullptr && atoi(getenv("FZB_FILTER_VIEW")) == 0;
    k.no_signature = on("FZB_NO_SIGNATURE");
    k.verify_promises = num("FZB_VERIFY_PROMISES", 1) != 0;
    k.debug_cus = std::max(0, num("FZB_DEBUG_CUS", 0));
    k.no_lcs_dfa = set("FZB_NO_LCS_DFA");
    k.no_cdfa = set("FZB_NO_CDFA");
    k.no_dp_classes = set("FZB_NO_DP_CLASSES");
    k.no_fused_classify = set("FZB_NO_FUSED_CLASSIFY");
    k.no_seg_list = on("FZB_NO_SEG_LIST");
    k.no_sig_planes = on("FZB_NO_SIG_PLANES");
    k.no_items_dfa = on("FZB_NO_ITEMS_DFA");
    k.no_dp_cfm = set("FZB_NO_DP_CFM");
    k.no_dp_cfu = set("FZB_NO_DP_CFU");
    k.unicode_multi = num("FZB_UNICODE_MULTI", -1);
    k.park_lds_kb = std::max(0, std::min(60, num("FZB_PARK_LDS_KB", 37)));
    k.coop_below = num("FZB_COOP_BELOW", -1);
    k.shard_gather_copy = getenv("FZB_SHARD_GATHER") != nullptr && !strcmp(getenv("FZB_SHARD_GATHER"), "copy");
    k.shard_inline = num("FZB_SHARD_INLINE", -1);
    k.spin_wait_us = num("FZB_SPIN_WAIT_US", 1000);
    k.edit_chunk_items = std::max(1024, num("FZB_EDIT_CHUNK_ITEMS", 1 << 20) / 1024 * 1024);
    return k;
}
FzbKnobs& knobs_storage() {
    static FzbKnobs k = parse_knobs();
    return k;
}
}  // namespace
const FzbKnobs& fzb_knobs() { return knobs_storage(); }

// ---- the compute-unit count every grid derives from, and the record of the grids launched under an override (knobs.h) -----------------
namespace {
struct GridRecord {
    unsigned min_grid, max_grid, launches;
};
std::mutex g_grid_mu;
std::map<std::string, GridRecord> g_grid_log;
}  // namespace
bool g_fzb_record_grids = fzb_knobs().debug_cus > 0;

int fzb_effective_cus(int* out) {
    const int forced = fzb_knobs().debug_cus;
    if (forced > 0) {
        *out = forced;
        return 0;
    }
    static std::atomic<int> cached[64];  // per device ordinal; 0 = not asked yet
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const bool slot = dev >= 0 && dev < 64;
    if (slot && cached[dev].load(std::memory_order_relaxed) > 0) {
        *out = cached[dev].load(std::memory_order_relaxed);
        return 0;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return (int)e;
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (slot) cached[dev].store(cus, std::memory_order_relaxed);
    *out = cus;
    return 0;
}
// for the launches that have nowhere to report to (a launch on a device that cannot be asked fails by itself): 256 then
static int cus_or_default() {
    int cus = 256;
    if (fzb_effective_cus(&cus) != 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    return cus;
}
unsigned fzb_grid_cap(uint64_t want, unsigned per_cu) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)cus_or_default() * per_cu)); }

// `kernel` is FZB_LAUNCH's first argument as written: "(k2b_dp<SWL, B, U>)" is recorded as k2b_dp
void fzb_record_grid(const char* kernel, unsigned grid) {
    std::string name(kernel);
    name.erase(0, name.find_first_not_of("( "));
    name.erase(std::min(name.size(), name.find_first_of("<) ")));
    std::lock_guard<std::mutex> lk(g_grid_mu);
    auto it = g_grid_log.find(name);
    if (it == g_grid_log.end()) g_grid_log[name] = GridRecord{grid, grid, 1};
    else {
        it->second.min_grid = std::min(it->second.min_grid, grid);
        it->second.max_grid = std::max(it->second.max_grid, grid);
        it->second.launches++;
    }
}
extern "C" {
// test hook: re-read the environment (tests/test_gpu_knobs.py switches paths inside one process; matchers created BEFORE the call keep
// what was decided at their creation - the LCS automaton, the unicode scorer's form)
void fzb_debug_reload_knobs(void) {
    knobs_storage() = parse_knobs();
    g_fzb_record_grids = knobs_storage().debug_cus > 0;
    std::lock_guard<std::mutex> lk(g_grid_mu);
    g_grid_log.clear();
}

// test hook: the launches recorded since the record was last cleared, one line "kernel min_grid max_grid launches" each (see frizbee_hip.h)
int fzb_debug_launch_grids(char* out, size_t cap, size_t* out_len, int clear) {
    if (!out_len || (!out && cap)) return fzb_fail(FZB_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g_grid_mu);
    std::string text;
    for (const auto& kv : g_grid_log) text += kv.first + " " + std::to_string(kv.second.min_grid) + " " + std::to_string(kv.second.max_grid) + " " + std::to_string(kv.second.launches) + "\n";
    *out_len = text.size();
    if (cap < text.size() + 1) return cap ? fzb_fail(FZB_ERR_CAPACITY, "fzb_debug_launch_grids: the record has " + std::to_string(text.size() + 1) + " bytes") : FZB_OK;
    memcpy(out, text.c_str(), text.size() + 1);
    if (clear) g_grid_log.clear();
    return FZB_OK;
}

void fzb_config_default(fzb_config* out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->max_typos = 0;
    out->casing = FZB_CASE_SMART;
    out->unicode = FZB_UNICODE_SMART;
    out->sort = FZB_SORT_SCORE_THEN_INDEX_ASC;
    out->scoring = fzb_scoring{12, 6, 5, 1, 12, 4, 4, 8, 4};  // src/const.rs:1-10
    out->matching = FZB_MATCH_FUZZY;
}

static void free_workspace(Workspace& w) {
    // (table / dfa / uni_dfa / lcs_dfa / cdfa point into tables_blob)
    void* ptrs[] = {w.bitmap, w.tile_counts, w.surv_idx, w.win, w.overflow, w.dp_scratch, w.bitmap2, w.tile_counts2, w.items2, w.win2, w.counters, w.tables_blob,
                    w.trace_cells, w.bitmap_m, w.tile_counts_m, w.marg_list, w.reject_bits, w.tile_rejects, w.rej_prefix, w.cls_win, w.cls_lists};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    fzb_sort_release(w.sort);
    if (w.tables_ev_pending) (void)hipEventSynchronize(w.tables_ev);
    if (w.tables_host) (void)hipHostFree(w.tables_host);
    if (w.tables_ev) (void)hipEventDestroy(w.tables_ev);
    w = Workspace{};
}

}  // extern "C"
void fzb_sort_release(SortBuffers& s) {
    if (s.tmp) (void)hipFree(s.tmp);
    if (s.hist) (void)hipFree(s.hist);
    s = SortBuffers{};
}
int fzb_scope_ensure_flags(ScopeScratch& s, size_t count) {
    const size_t tiles = (count + SCOPE_TILE - 1) / SCOPE_TILE;
    int rc;
    if ((rc = fzb_grow_dev(&s.bitmap, &s.bitmap_words, tiles * SCOPE_WORDS, 1)) || (rc = fzb_grow_dev(&s.tiles, &s.tiles_cap, tiles, 4))) return rc;
    return fzb_grow_dev(&s.words, &s.words_cap, 16);
}
int fzb_scope_ensure(ScopeScratch& s, size_t count) {
    if (int rc = fzb_grow_dev(&s.recs, &s.recs_cap, count, 16)) return rc;
    return fzb_scope_ensure_flags(s, count);
}
void fzb_scope_release(ScopeScratch& s) {
    for (void* p : {(void*)s.recs, (void*)s.bitmap, (void*)s.tiles, (void*)s.words})
        if (p) (void)hipFree(p);
    s = ScopeScratch{};
}
int fzb_sections_ensure(SectionsScratch& s, size_t n_records, size_t stage_records) {
    if (int rc = fzb_grow_dev(&s.words, &s.words_cap, fzb_sections_scratch_words(n_records), 16)) return rc;
    return stage_records ? fzb_grow_dev(&s.stage, &s.stage_words, SEC_STAGE_RECORDS + 2 * stage_records, 16) : FZB_OK;
}
int fzb_sections_ensure_slabs(SectionsScratch& s, size_t slab_records) { return fzb_grow_dev(&s.slabs, &s.slabs_words, SECTIONS_SLAB_WORDS + 2 * slab_records, 16); }
void fzb_sections_release(SectionsScratch& s) {
    if (s.words) (void)hipFree(s.words);
    if (s.stage) (void)hipFree(s.stage);
    if (s.slabs) (void)hipFree(s.slabs);
    s = SectionsScratch{};
}
int fzb_top_ensure(TopStaging& t, size_t want, size_t position_words, bool staging) {
    int rc;
    if (!t.head || !t.tiles || t.cap < want) {
        t.cap = 0;
        if ((rc = fzb_dev_renew(&t.head, want + 16)) || (rc = fzb_dev_renew(&t.tiles, fzb_indices_pack_tile_words(want)))) return rc;
        t.cap = want;
    }
    if (!staging) return FZB_OK;
    if ((rc = fzb_grow_dev(&t.packed, &t.packed_cap, want, 1))) return rc;
    return fzb_grow_dev(&t.dense, &t.dense_words, position_words, 1);
}
void fzb_top_release(TopStaging& t) {
    for (void* p : {(void*)t.head, (void*)t.tiles, (void*)t.packed, (void*)t.dense})
        if (p) (void)hipFree(p);
    t = TopStaging{};
}
void fzb_out_release(OutStaging& o) {
    if (o.out_dev) (void)hipFree(o.out_dev);
    if (o.count_dev) (void)hipFree(o.count_dev);
    if (o.fetch.count_host) (void)hipHostFree(o.fetch.count_host);
    if (o.fetch_top.count_host) (void)hipHostFree(o.fetch_top.count_host);
    o = OutStaging{};
}
// Everything a MatcherState owns but its shard clones (fzb_matcher_free walks them, each on its own device)
static void release_state(MatcherState& s) {
    free_workspace(s.ws);
    fzb_out_release(s);
    fzb_scope_release(s.scope);
    fzb_sections_release(s.sections);
    fzb_top_release(s.top);
    for (void* p : {(void*)s.top_words, (void*)s.trace_sel, (void*)s.trace_pos, (void*)s.trace_npos, (void*)s.top_traced, (void*)s.top_idx_words, s.long_blob_dev, (void*)s.long_scratch})
        if (p) (void)hipFree(p);
    for (auto& tr : s.evring)
        for (auto& e : tr)
            if (e) (void)hipEventDestroy(e);
    if (s.ev_fork) (void)hipEventDestroy(s.ev_fork);
    if (s.ev_join) (void)hipEventDestroy(s.ev_join);
    if (s.aux_stream) (void)hipStreamDestroy(s.aux_stream);
    if (s.shard_workers) fzb_shard_workers_free(s.shard_workers);  // joins the worker threads before their clones go
    s.shard_workers = nullptr;
    if (s.shard_stream) (void)hipStreamDestroy(s.shard_stream);
    if (s.shard_event) (void)hipEventDestroy(s.shard_event);
    if (s.shard_count_host) (void)hipHostFree(s.shard_count_host);
}
extern "C" {

// The matcher's byte tables on the device: [filter table 2 KB | subsequence DFA | unicode DFA | LCS automaton | class-composite automaton], each
// with room for any needle's (fzb_matcher_set_pattern re-uploads in place).  One copy out of the pinned staging buffer, asynchronous on `st`
// (the stream the query's kernels follow on) - or synchronous when there is no stream to order it on (fzb_matcher_reserve).
namespace {
constexpr size_t TB_TABLE = 0, TB_DFA = 2048, TB_SLOT = 256 * 256 + 128, TB_UNI = TB_DFA + TB_SLOT, TB_LCS = TB_UNI + TB_SLOT, TB_CDFA = TB_LCS + TB_SLOT,
                 TB_TOTAL = TB_CDFA + 256 + 16384 + 128;
}
static int upload_tables(fzb_matcher* m, hipStream_t st, bool have_stream) {
    Workspace& w = m->ws;
    if (w.tables_ev_pending) {  // (the previous copy out of the staging buffer: long done unless two needle changes follow each other without a query's end between)
        HIPCHK(hipEventSynchronize(w.tables_ev));
        w.tables_ev_pending = false;
    }
    size_t end = TB_DFA;
    memcpy(w.tables_host + TB_TABLE, m->table.data(), 256 * 8);
    auto put = [&](size_t off, const std::vector<u8>& v) {
        if (v.empty()) return;
        memcpy(w.tables_host + off, v.data(), v.size());
        end = std::max(end, off + v.size());
    };
    put(TB_DFA, m->dfa);
    put(TB_UNI, m->uni_dfa);
    put(TB_LCS, m->lcs_dfa);
    put(TB_CDFA, m->cdfa);
    if (have_stream) {
        HIPCHK(hipMemcpyAsync(w.tables_blob, w.tables_host, end, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(w.tables_ev, st));
        w.tables_ev_pending = true;
    } else {
        HIPCHK(hipMemcpy(w.tables_blob, w.tables_host, end, hipMemcpyHostToDevice));
    }
    w.tables_stale = false;
    return FZB_OK;
}

// ---- fzb_matcher_create, piece by piece ------------------------------------------------------------------------------------------
// NeedleDev's scalars: what `Prefilter::new` / `SmithWaterman::new` precompute (src/prefilter/algo/mod.rs:30-42, src/smith_waterman/algo/mod.rs:21-42)
static void fill_needle_scalars(CompiledNeedle* m, size_t needle_len, size_t n_scalars) {
    const fzb_config& config = m->config;
    const fzb_scoring& sc = config.scoring;
    NeedleDev& nd = m->nd;
    memset(&nd, 0, sizeof(nd));
    nd.rows = m->rows;
    nd.nbytes = (int)needle_len;
    nd.max_typos = config.max_typos;
    nd.min_haystack_len = config.max_typos < 0 ? 0 : (int)(n_scalars > (size_t)config.max_typos ? n_scalars - (size_t)config.max_typos : 0);  // algo.rs:62-65
    nd.unicode = m->unicode;
    nd.lane_mask = m->use_u8 ? 0xFF : 0xFFFF;
    nd.match_plus_mismatch = sadd16(sc.match_score, sc.mismatch_penalty);
    nd.mismatch = sc.mismatch_penalty;
    nd.gex = sc.gap_extend_penalty;
    nd.gopm = ssub16(sc.gap_open_penalty, sc.gap_extend_penalty);
    nd.prefix = sc.prefix_bonus;
    nd.capitalization = sc.capitalization_bonus;
    nd.matching_case = sc.matching_case_bonus;
    nd.exact_bonus = sc.exact_match_bonus;
    nd.delimiter = sc.delimiter_bonus;
    nd.match_score = sc.match_score;
    nd.gap_open = sc.gap_open_penalty;
}
static u8 flip_ascii_byte(const CompiledNeedle* m, u8 c) { return m->case_sensitive ? c : (c >= 'a' && c <= 'z') ? (u8)(c - 32) : (c >= 'A' && c <= 'Z') ? (u8)(c + 32) : c; }

// A needle beyond NeedleDev's by-value arrays: the arrays go to one host blob (uploaded on first use), the scalars to NeedleLongDev, and the
// stage configuration is "lane-exact prefilter kernel (or the streaming subsequence automaton) first, wave- or thread-per-window scorer"
static void build_long_needle(CompiledNeedle* m, const uint8_t* needle_utf8, size_t needle_len, const std::vector<u32>& cps) {
    const fzb_config* config = &m->config;
    const fzb_scoring& sc = config->scoring;
    NeedleDev& nd = m->nd;
    auto flip_ascii = [&](u8 c) { return flip_ascii_byte(m, c); };
    // [raw | c | f | uc | uf | ulen], 16-byte aligned sections (device pointers are set when the blob is uploaded)
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t nb = needle_len, nr = cps.size();
    m->long_off_c = al(nb);
    m->long_off_f = m->long_off_c + al(nb);
    m->long_off_uc = m->long_off_f + al(nb);
    m->long_off_uf = m->long_off_uc + al(4 * nr);
    m->long_off_ulen = m->long_off_uf + al(4 * nr);
    m->long_blob_host.assign(m->long_off_ulen + al(nr) + 16, 0);
    u8* blob = m->long_blob_host.data();
    for (size_t i = 0; i < nb; i++) {  // case_needle (src/prefilter/mod.rs:49-65)
        blob[i] = needle_utf8[i];
        blob[m->long_off_c + i] = needle_utf8[i];
        blob[m->long_off_f + i] = flip_ascii(needle_utf8[i]);
    }
    for (size_t i = 0; i < nr; i++) {  // case_needle_unicode (src/prefilter/mod.rs:71-96)
        blob[m->long_off_ulen + i] = (u8)encode_utf8(cps[i], blob + m->long_off_uc + 4 * i);
        encode_utf8(m->case_sensitive ? cps[i] : flip_same_width(cps[i]), blob + m->long_off_uf + 4 * i);
    }
    NeedleLongDev& l = m->ndl;
    memset(&l, 0, sizeof(l));
    l.rows = nd.rows; l.nbytes = nd.nbytes; l.max_typos = nd.max_typos; l.min_haystack_len = nd.min_haystack_len; l.unicode = nd.unicode; l.lane_mask = nd.lane_mask;
    l.match_plus_mismatch = nd.match_plus_mismatch; l.mismatch = nd.mismatch; l.gex = nd.gex; l.gopm = nd.gopm;
    l.prefix = nd.prefix; l.capitalization = nd.capitalization; l.matching_case = nd.matching_case; l.exact_bonus = nd.exact_bonus; l.delimiter = nd.delimiter;
    l.match_score = nd.match_score; l.gap_open = nd.gap_open;
    // stage configuration: no streaming filter; either no prefilter at all or the lane-exact prefilter kernel as the first stage
    const int k = config->max_typos;
    LaunchCfg& lc = m->lc;
    lc.filter_mode = 0;
    lc.filter_exact = 0;  // (sizes the second-level arrays the lane-exact prefilter writes)
    lc.window_mode = (k < 0 || k >= m->rows) ? 2 : 0;
    lc.pad_ok = lc.cf_ok = lc.cfm_ok = 0;
    // (the biased gap scan of dp_multi_chunk, as for short needles below: the largest biased value stays inside 16 bits)
    lc.bias_ok = score_ceiling(sc, (size_t)m->rows) + (size_t)sc.mismatch_penalty + 130 * (size_t)sc.gap_extend_penalty + 64 <= 0xFFFF;
    // dp_cfm.h's arithmetic for the four-lanes-per-window scorer (k2d_dp_long_quad; set_scorer_forms' condition with this needle's rows in the
    // bias: lanes up to 3/2 chunks + rows + 1 of gap_extend)
    lc.cfm_ok = !m->unicode && m->rows <= FZB_LONG_LDS_ROWS && 2 * (u32)sc.gap_extend_penalty <= (u32)sc.mismatch_penalty &&
                score_ceiling(sc, (size_t)m->rows) + (size_t)sc.mismatch_penalty + (137 + (size_t)m->rows) * (size_t)sc.gap_extend_penalty + 64 < 0x7C00;
    m->long_upper = false;
    if (!m->unicode)
        for (size_t i = 0; i < nb; i++) m->long_upper = m->long_upper || (blob[m->long_off_c + i] >= 'A' && blob[m->long_off_c + i] <= 'Z');
    m->table.assign(256, 0);
    // 0 typos, ASCII: accept <=> the needle is a case-folded ordered subsequence (src/prefilter/algo/ascii.rs:6-54; lane-width independent),
    // and that automaton has rows + 1 states whatever the needle's length: up to 200 rows its table fits a workgroup's LDS (58 KB) and the
    // STREAMING filter decides the list (round 5; rounds 3-4 ran the chunked prefilter over every haystack: 0.75 of the bench row's 9.7 ms)
    if (!m->unicode && !m->literal_mode && k == 0 && m->rows <= 200) {
        m->long_dfa = true;
        bool used[256] = {false};
        lc.pad_ok = 1;
        for (size_t i = 0; i < nb; i++) {
            used[blob[m->long_off_c + i]] = used[blob[m->long_off_f + i]] = true;
            if (needle_utf8[i] == 0) lc.pad_ok = 0;
        }
        lc.dead_byte = 0;
        for (int b = 255; b >= 0; b--)
            if (!used[b]) { lc.dead_byte = (u32)b; break; }
        m->dfa.assign((size_t)(m->rows + 1) * 256, 0);
        for (int st = 0; st <= m->rows; st++)
            for (int b = 0; b < 256; b++)
                m->dfa[(size_t)st * 256 + b] = (u8)((st < m->rows && (b == blob[m->long_off_c + (size_t)st] || b == blob[m->long_off_f + (size_t)st])) ? st + 1 : st);
    }
}

// The streaming filter's byte tables: `table[b]` = needle rows byte b can match (the LCS filter's M), the dead byte, the ordered-subsequence
// DFA (state s = rows matched so far) - or, for the literal substring mode on the ASCII path, the needle's Knuth-Morris-Pratt automaton
static void build_filter_tables(CompiledNeedle* m) {
    const NeedleDev& nd = m->nd;
    LaunchCfg& lc = m->lc;
    m->table.assign(256, 0);
    for (int r = 0; r < m->rows; r++) {
        if (m->unicode) {  // a scalar can only match where its LAST byte matches (either case): conservative
            m->table[nd.uc[r][nd.ulen[r] - 1]] |= (u64)1 << r;
            m->table[nd.uf[r][nd.ulen[r] - 1]] |= (u64)1 << r;
        } else {
            m->table[nd.c[r]] |= (u64)1 << r;
            m->table[nd.f[r]] |= (u64)1 << r;
        }
    }
    lc.dead_byte = 0;
    for (int b = 255; b >= 0; b--)
        if (m->table[b] == 0) { lc.dead_byte = (u32)b; break; }
    // ordered-subsequence DFA: state s = rows matched so far; a byte that can match row s advances it
    m->dfa.assign((size_t)(m->rows + 1) * 256, 0);
    for (int st = 0; st <= m->rows; st++)
        for (int b = 0; b < 256; b++) m->dfa[(size_t)st * 256 + b] = (u8)((st < m->rows && ((m->table[b] >> st) & 1)) ? st + 1 : st);
    if (m->literal_mode == FZB_MATCH_SUBSTRING && !m->unicode) {
        // Substring accept on the ASCII path = "the text drives the needle's Knuth-Morris-Pratt automaton into its final state":
        // the same table shape, so the streaming DFA filter kernels run it unchanged.  Position k matches byte b iff b is
        // needle[k] or its case flip; both case forms of a needle byte take the automaton to the same state (the flip is
        // an involution on every position's byte set), so the usual single restart state works for the folded alphabet.
        const int n = m->rows;
        auto hit = [&](int k, int b) { return b == nd.c[k] || b == nd.f[k]; };
        for (int b = 0; b < 256; b++) m->dfa[b] = (u8)(hit(0, b) ? 1 : 0);
        int x = 0;  // restart state: where the automaton is after reading needle[1..k)
        for (int k = 1; k < n; k++) {
            for (int b = 0; b < 256; b++) m->dfa[(size_t)k * 256 + b] = (u8)(hit(k, b) ? k + 1 : m->dfa[(size_t)x * 256 + b]);
            x = m->dfa[(size_t)x * 256 + nd.c[k]];
        }
        for (int b = 0; b < 256; b++) m->dfa[(size_t)n * 256 + b] = (u8)n;  // found: absorbing
    }
}

static void build_unicode_dfa(CompiledNeedle* m) {
    const fzb_config* config = &m->config;
    const NeedleDev& nd = m->nd;
    const LaunchCfg& lc = m->lc;
    // Unicode path, 0 typos: the prefilter accepts iff the needle's scalars occur, in order, at increasing byte positions, each as its own
    // bytes or as the bytes of its same-width case flip (src/prefilter/algo/unicode.rs:118-219; the same at 16 / 32 / 64 lanes - checked
    // against the oracle by tests/test_host_abi.py::test_unicode_dfa_is_the_unicode_prefilter).  That is a byte-level DFA: state = (scalars
    // matched, bytes of the current scalar matched, which of the two variants are still alive); a mismatch inside a scalar falls back to
    // "is this byte the scalar's first byte" (UTF-8 lead bytes never occur inside a scalar, so no longer border exists).  With <= 226
    // states it runs in the streaming DFA filter kernels unchanged and replaces superset filter + lane-exact window pass + second compaction.
    m->uni_dfa_states = 0;
    if (m->unicode && !m->literal_mode && config->max_typos == 0 && m->rows >= 1 && lc.filter_mode == 1) {
        struct St { int i, k, alive; };
        std::vector<St> states;
        auto find = [&](int i, int k, int alive) {
            for (size_t q = 0; q < states.size(); q++)
                if (states[q].i == i && states[q].k == k && states[q].alive == alive) return (int)q;
            states.push_back(St{i, k, alive});
            return (int)states.size() - 1;
        };
        std::vector<std::vector<int>> trans;
        find(0, 0, 3);
        bool ok = true;
        for (size_t q = 0; q < states.size() && ok; q++) {
            const St cur = states[q];
            std::vector<int> row(256, (int)q);
            if (cur.i < m->rows) {
                const u8* va = nd.uc[cur.i];
                const u8* vb = nd.uf[cur.i];
                const int len = nd.ulen[cur.i];
                auto from_start = [&](int b) {  // state (i, 0) reading b
                    const int alive = (va[0] == b ? 1 : 0) | (vb[0] == b ? 2 : 0);
                    if (!alive) return find(cur.i, 0, 3);
                    return len == 1 ? find(cur.i + 1, 0, 3) : find(cur.i, 1, alive);
                };
                for (int b = 0; b < 256; b++) {
                    if (cur.k == 0) { row[b] = from_start(b); continue; }
                    const int alive = ((cur.alive & 1) && va[cur.k] == b ? 1 : 0) | ((cur.alive & 2) && vb[cur.k] == b ? 2 : 0);
                    if (alive) row[b] = cur.k + 1 == len ? find(cur.i + 1, 0, 3) : find(cur.i, cur.k + 1, alive);
                    else row[b] = from_start(b);
                }
            }  // i == rows: accepting, absorbing
            trans.push_back(row);
            if (states.size() > 226) ok = false;  // 226 x 288 bytes (dfa_lds.h's row stride) + the tile counter fit the 64 KiB of dynamic LDS
        }
        if (ok) {
            // renumber so that the accepting state is the LAST one (the kernels test `state == number of states - 1`)
            const int ns = (int)states.size();
            int acc = -1;
            for (int q = 0; q < ns; q++)
                if (states[q].i == m->rows) acc = q;
            std::vector<int> renum(ns);
            for (int q = 0, nx = 0; q < ns; q++) renum[q] = q == acc ? ns - 1 : nx++;
            m->uni_dfa.assign((size_t)ns * 256, 0);
            for (int q = 0; q < ns; q++)
                for (int b = 0; b < 256; b++) m->uni_dfa[(size_t)renum[q] * 256 + b] = (u8)renum[trans[q][b]];
            m->uni_dfa_states = ns;  // start state 0 = (0, 0): first created, never the accepting one (rows >= 1)
        }
    }
}

// Unicode typo configurations: the same criterion over SCALARS.  The reference's unicode typo algorithms (unicode_typos.rs:15-466) are the
// ASCII ones over occurrence masks of whole scalars - row i occurs at byte position p iff the bytes at p equal the scalar's or its case flip's
// (unicode.rs:74-117), occurrences never overlap (UTF-8: lead byte, then continuation bytes) - so what they decide on a haystack that fits one
// prefilter chunk is LCS(needle scalars, the haystack's occurrences) + k >= n, and beyond one chunk they deviate from it only when there is
// nothing to spare (tests/test_oracle_reference_properties.py::test_single_chunk_unicode_typo_prefilter_is_the_scalar_lcs_criterion,
// ::test_the_unicode_typo_prefilter_only_ever_deviates_on_marginal_inputs).  As a byte-level automaton: state = (reachable bit-vector V, node of
// the trie over the needle's distinct scalar byte strings = the bytes of the scalar being read); a byte that completes a string applies the LCS
// step with M = the rows spelt by it; a byte that does not continue the current string restarts from the root WITH that byte (a lead byte never
// occurs inside a scalar).  States are numbered by ascending LCS of V (an unfinished scalar counts for nothing), start state first.
// (Rounds 2-5 ran the byte-level LCS over the scalars' LAST bytes here - a looser superset that needed the lane-exact window kernel for every
// survivor; with the exact criterion single-chunk lists are decided in the stream: pipe_unicode_typo_fast_path.)
static bool build_scalar_lcs_dfa(CompiledNeedle* m) {
    const NeedleDev& nd = m->nd;
    const int rows = m->rows, k = m->config.max_typos;
    const u64 mask = rows >= 64 ? ~(u64)0 : (((u64)1 << rows) - 1);
    // trie over the distinct byte strings uc[i] / uf[i]: node 0 = root; term[node] = rows spelt by the complete string ending there (0: internal)
    struct Node { int child[256]; u64 term; };
    std::vector<Node> trie(1);
    for (int b = 0; b < 256; b++) trie[0].child[b] = -1;
    trie[0].term = 0;
    auto insert = [&](const u8* str, int len, int row) {
        int cur = 0;
        for (int j = 0; j < len; j++) {
            if (trie[cur].child[str[j]] < 0) {
                Node nn;
                for (int b = 0; b < 256; b++) nn.child[b] = -1;
                nn.term = 0;
                trie.push_back(nn);
                trie[cur].child[str[j]] = (int)trie.size() - 1;
            }
            cur = trie[cur].child[str[j]];
        }
        trie[cur].term |= (u64)1 << row;
    };
    for (int r = 0; r < rows; r++) {
        if (nd.ulen[r] < 1 || nd.ulen[r] > 4) return false;
        insert(nd.uc[r], nd.ulen[r], r);
        insert(nd.uf[r], nd.ulen[r], r);
    }
    for (const Node& nn : trie)  // (UTF-8 is prefix-free: a complete scalar is never the prefix of another; anything else is not a needle this automaton models)
        if (nn.term)
            for (int b = 0; b < 256; b++)
                if (nn.child[b] >= 0) return false;
    struct St { u64 v; int node; };
    std::vector<St> states{St{mask, 0}};
    auto key = [](u64 v, int node) { return std::make_pair(v, node); };
    std::map<std::pair<u64, int>, int> id{{key(mask, 0), 0}};
    auto find = [&](u64 v, int node) {
        auto it = id.find(key(v, node));
        if (it != id.end()) return it->second;
        states.push_back(St{v, node});
        id.emplace(key(v, node), (int)states.size() - 1);
        return (int)states.size() - 1;
    };
    auto lcs_step = [&](u64 v, u64 mrows) { const u64 u = v & mrows; return ((v + u) | (v & ~mrows)) & mask; };
    auto from_root = [&](u64 v, int b) {  // state (v, root) reading byte b
        const int c = trie[0].child[b];
        if (c < 0) return find(v, 0);
        return trie[c].term ? find(lcs_step(v, trie[c].term), 0) : find(v, c);
    };
    std::vector<std::vector<int>> next;
    for (size_t q = 0; q < states.size(); q++) {
        const St cur = states[q];
        std::vector<int> row(256);
        for (int b = 0; b < 256; b++) {
            if (cur.node == 0) { row[b] = from_root(cur.v, b); continue; }
            const int c = trie[cur.node].child[b];
            if (c < 0) row[b] = from_root(cur.v, b);
            else row[b] = trie[c].term ? find(lcs_step(cur.v, trie[c].term), 0) : find(cur.v, c);
        }
        next.push_back(row);
        if (states.size() > 226) return false;  // 226 x 288 bytes (dfa_lds.h's row stride) + the tile counter fit the 64 KiB of dynamic LDS
    }
    const int ns = (int)states.size(), need = rows - k;
    std::vector<int> lcs(ns), order(ns), renum(ns);
    for (int q = 0; q < ns; q++) lcs[q] = __builtin_popcountll(~states[q].v & mask), order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lcs[a] < lcs[b]; });  // the start state (LCS 0, first created) stays first
    int acc = ns;
    for (int pos = 0; pos < ns; pos++) {
        renum[order[pos]] = pos;
        if (lcs[order[pos]] >= need && acc == ns) acc = pos;
    }
    m->lcs_dfa.assign((size_t)ns * 256, 0);
    for (int q = 0; q < ns; q++)
        for (int b = 0; b < 256; b++) m->lcs_dfa[(size_t)renum[q] * 256 + b] = (u8)renum[next[q][b]];
    m->lcs_states = ns;
    m->lcs_acc_lo = acc;
    m->lcs_scalar = true;
    return true;
}

static void build_lcs_dfa(CompiledNeedle* m) {
    const LaunchCfg& lc = m->lc;
    const int k = m->config.max_typos;
    m->lcs_states = 0;
    m->lcs_scalar = false;
    if (m->unicode && !m->literal_mode && lc.filter_mode == 2 && m->rows >= 1 && m->rows <= 63 && !fzb_knobs().no_lcs_dfa && build_scalar_lcs_dfa(m)) return;
    // Typo configurations: the streaming filter's LCS criterion `LCS(needle, haystack) >= rows - k` (Hyyro's bit-vector recurrence
    // V' = (V + (V & M)) | (V & ~M), M = the rows byte b can match) as a table-driven automaton over its REACHABLE bit-vectors - 40-odd
    // states for a 6-row needle - so that the filter is the same v_perm + ds_read_u8 per byte as the 0-typo one (k1_dfa: 55 us on the
    // 10 M x 32 B list) instead of a table lookup + four vector operations (k1_filter: 71 us).  States are numbered by ascending LCS, so
    // "accepts" is one compare; the start state (LCS 0, only reachable as itself) is state 0.  More than 226 states (long needles with
    // many distinct letters): the bit-vector kernel stays.  FZB_NO_LCS_DFA=1 keeps it for comparison.
    m->lcs_states = 0;
    if (lc.filter_mode == 2 && m->rows >= 1 && m->rows <= 63 && !fzb_knobs().no_lcs_dfa) {
        const u64 mask = m->rows >= 64 ? ~(u64)0 : (((u64)1 << m->rows) - 1);
        std::vector<u64> masks;  // distinct M over the 256 byte values
        std::vector<int> mask_of(256);
        for (int b = 0; b < 256; b++) {
            const u64 mb = m->table[b] & mask;
            size_t q = 0;
            while (q < masks.size() && masks[q] != mb) q++;
            if (q == masks.size()) masks.push_back(mb);
            mask_of[b] = (int)q;
        }
        std::vector<u64> states{mask};  // V0: all ones in the low `rows` bits
        states.reserve(256);
        const size_t nm = masks.size();
        std::vector<int> next;  // [state][mask]
        next.reserve(256 * nm);
        bool ok = true;
        for (size_t q = 0; q < states.size() && ok; q++) {
            const u64 v = states[q];
            for (size_t t = 0; t < nm; t++) {
                const u64 u = v & masks[t];
                const u64 nv = ((v + u) | (v & ~masks[t])) & mask;
                size_t id = 0;  // (at most 226 states: a linear search beats a hash table's allocations)
                while (id < states.size() && states[id] != nv) id++;
                if (id == states.size()) {
                    states.push_back(nv);
                    if (states.size() > 226) ok = false;
                }
                next.push_back((int)id);
            }
        }
        if (ok) {
            const int ns = (int)states.size();
            const int need = m->rows - k;
            std::vector<int> lcs(ns), order(ns), renum(ns);
            for (int q = 0; q < ns; q++) lcs[q] = __builtin_popcountll(~states[q] & mask), order[q] = q;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lcs[a] < lcs[b]; });  // V0 (LCS 0, first created) stays first
            int acc = ns;
            for (int pos = 0; pos < ns; pos++) {
                renum[order[pos]] = pos;
                if (lcs[order[pos]] >= need && acc == ns) acc = pos;
            }
            m->lcs_dfa.assign((size_t)ns * 256, 0);
            for (int q = 0; q < ns; q++)
                for (int b = 0; b < 256; b++) m->lcs_dfa[(size_t)renum[q] * 256 + b] = (u8)renum[next[(size_t)q * nm + mask_of[b]]];
            m->lcs_states = ns;
            m->lcs_acc_lo = acc;
        }
    }
}

static void build_cdfa(CompiledNeedle* m) {
    const LaunchCfg& lc = m->lc;
    // The class-composite form of the automaton the streaming filter runs (ragged lists: kernels_filter.hip, k1_cdfa_ragged): bytes with
    // identical columns are one class (K of them), G transitions are composed into one table indexed by
    // state * K^G + c0 + K c1 + ... (c0 = the class of the FIRST byte), G = 4 if states * K^4 <= 16 KB, else 2, else none.
    m->cdfa.clear();
    m->cdfa_src = m->cdfa_K = m->cdfa_G = 0;
    {
        const std::vector<u8>* fa = nullptr;
        int fstates = 0, src = 0;
        if (m->literal_mode == FZB_MATCH_SUBSTRING && !m->unicode) { fa = &m->dfa; fstates = m->rows + 1; src = 1; }
        else if (m->literal_mode) {}
        else if (m->uni_dfa_states) { fa = &m->uni_dfa; fstates = m->uni_dfa_states; src = 2; }
        else if (lc.filter_mode == 2 && m->lcs_states) { fa = &m->lcs_dfa; fstates = m->lcs_states; src = 3; }
        else if (lc.filter_mode == 1) { fa = &m->dfa; fstates = m->rows + 1; src = 1; }
        if (fa && fstates >= 1 && fstates <= 255) {
            std::vector<int> cls(256, -1);
            std::vector<int> rep;  // a representative byte per class
            for (int b = 0; b < 256; b++) {
                for (size_t q = 0; q < rep.size() && cls[b] < 0; q++) {
                    bool same = true;
                    for (int stt = 0; stt < fstates && same; stt++) same = (*fa)[(size_t)stt * 256 + b] == (*fa)[(size_t)stt * 256 + rep[q]];
                    if (same) cls[b] = (int)q;
                }
                if (cls[b] < 0) { cls[b] = (int)rep.size(); rep.push_back(b); }
            }
            const size_t K = rep.size();
            int G = 0;
            if ((size_t)fstates * K * K * K * K <= 16384) G = 4;
            else if ((size_t)fstates * K * K <= 16384) G = 2;
            if (G) {
                size_t KG = 1;
                for (int i = 0; i < G; i++) KG *= K;
                m->cdfa.assign(((256 + (size_t)fstates * KG) + 15) & ~(size_t)15, 0);
                for (int b = 0; b < 256; b++) m->cdfa[b] = (u8)cls[b];
                // two transitions composed first (c0, the least significant digit, is consumed first), then - G = 4 - two of those: no division per entry
                const size_t K2 = K * K;
                std::vector<u8> t2((size_t)fstates * K2);
                for (int stt = 0; stt < fstates; stt++)
                    for (size_t c1 = 0; c1 < K; c1++)
                        for (size_t c0 = 0; c0 < K; c0++)
                            t2[(size_t)stt * K2 + c0 + K * c1] = (*fa)[(size_t)(*fa)[(size_t)stt * 256 + rep[c0]] * 256 + rep[c1]];
                u8* comp = m->cdfa.data() + 256;
                if (G == 2) memcpy(comp, t2.data(), t2.size());
                else
                    for (int stt = 0; stt < fstates; stt++)
                        for (size_t hi = 0; hi < K2; hi++) {
                            u8* row = comp + (size_t)stt * KG + K2 * hi;
                            const u8* first = &t2[(size_t)stt * K2];
                            for (size_t lo = 0; lo < K2; lo++) row[lo] = t2[(size_t)first[lo] * K2 + hi];
                        }
                m->cdfa_src = src;
                m->cdfa_K = (int)K;
                m->cdfa_G = G;
            }
        }
    }
}

// which forms of the scorers this needle and scoring allow
static void set_scorer_forms(CompiledNeedle* m, const uint8_t* needle_utf8, size_t needle_len) {
    const fzb_scoring& sc = m->config.scoring;
    LaunchCfg& lc = m->lc;
    lc.pad_ok = 1;
    for (size_t i = 0; i < needle_len; i++)
        if (needle_utf8[i] == 0) lc.pad_ok = 0;
    // biased gap propagation needs max cell value + lanes*gex (+ headroom) to stay below 2^16
    lc.bias_ok = score_ceiling(sc, (size_t)m->rows) + (size_t)sc.mismatch_penalty + 130 * (size_t)sc.gap_extend_penalty + 64 <= 0xFFFF;
    // dp_cf.h / dp_cfm.h: every biased value stays below 0x7C00, so that the cell's three-way maximum can be v_pk_maximum3_f16 (exact on
    // non-negative finite binary16 patterns: dp_body.h, p_max3_s); scorings beyond that - needle rows worth thousands of points - take the first forms
    lc.cfm_ok = 2 * (u32)sc.gap_extend_penalty <= (u32)sc.mismatch_penalty &&
                score_ceiling(sc, (size_t)m->rows) + (size_t)sc.mismatch_penalty + 200 * (size_t)sc.gap_extend_penalty + 64 < 0x7C00;  // lanes up to 3/2 chunks + rows of bias
    lc.cf_ok = lc.pad_ok && 2 * (u32)sc.gap_extend_penalty <= (u32)sc.mismatch_penalty &&
               score_ceiling(sc, (size_t)m->rows) + (size_t)sc.mismatch_penalty + 130 * (size_t)sc.gap_extend_penalty + 64 < 0x7C00;
    lc.cfu_ok = lc.bias_ok && 2 * (u32)sc.gap_extend_penalty <= (u32)sc.mismatch_penalty && !fzb_knobs().no_dp_cfu;  // (knob: the unicode scorer's first form)
}

// (config, needle) -> everything a matcher holds on the host; no HIP call.  `cn` comes in default-constructed and is only to be used when
// this returns FZB_OK.
static int compile_needle(CompiledNeedle& cn, const fzb_config* config, const uint8_t* needle_utf8, size_t needle_len) {
    if (!config || (!needle_utf8 && needle_len)) return fail(FZB_ERR_INVALID, "null argument");
    if (config->casing < 0 || config->casing > 2 || config->unicode < 0 || config->unicode > 2 || config->sort < 0 || config->sort > 3 || config->max_typos < -1 ||
        config->max_typos > 0xFFFF)
        return fail(FZB_ERR_INVALID, "config enum/range out of bounds");
    std::vector<u32> cps;
    if (!decode_utf8(needle_utf8, needle_len, cps)) return fail(FZB_ERR_INVALID, "needle is not valid UTF-8");
    CompiledNeedle* m = &cn;
    m->config = *config;
    m->needle.assign((const char*)needle_utf8, needle_len);
    m->empty = needle_len == 0;
    const fzb_scoring& sc = config->scoring;
    m->use_u8 = fits_in_u8(needle_len, sc);  // byte length (src/matcher/mod.rs:453)
    int pf = config->pf_lanes, sw = config->sw_lanes;
    if (pf == 0 && sw == 0) detect_host_lanes(m->use_u8, pf, sw);
    else if (sw == 0) sw = m->use_u8 ? pf : pf / 2;  // the score width of the ISA family whose prefilter has pf lanes (64: AVX-512, 32: AVX2, 16: SSE/scalar)
    if (!(pf == 16 || pf == 32 || pf == 64) || !(sw == 8 || sw == 16 || sw == 32 || sw == 64))
        return fail(FZB_ERR_INVALID, "pf_lanes must be 16/32/64 and sw_lanes 8/16/32/64 (or both 0 = auto)");
    m->lc.pf_lanes = pf;
    m->lc.sw_lanes = sw;
    if (m->empty) return FZB_OK;  // CompiledPatterns::Empty (src/matcher/mod.rs:194-196)
    // CaseMatching::respects_case_for (src/lib.rs:370-376), UnicodeMatching::respects_unicode_for (:394-400)
    bool any_upper = false, ascii = true;
    for (u32 cp : cps) { any_upper |= is_uppercase(cp); ascii &= cp < 0x80; }
    m->case_sensitive = config->casing == FZB_CASE_RESPECT || (config->casing == FZB_CASE_SMART && any_upper);
    m->unicode = config->unicode == FZB_UNICODE_ALWAYS || (config->unicode == FZB_UNICODE_SMART && !ascii);
    m->rows = (int)(m->unicode ? cps.size() : needle_len);
    if (config->matching < FZB_MATCH_FUZZY || config->matching > FZB_MATCH_SUBSTRING) return fail(FZB_ERR_INVALID, "bad matching mode");
    m->literal_mode = config->matching;
    // guard_against_score_overflow: fuzzy src/matcher/algo.rs:311-325 (rows); literal src/literal/algo.rs:33, 314-322 (needle bytes, its own per-char bonus)
    std::string perr = m->literal_mode ? overflow_guard(sc, needle_len, sadd16(std::max(sc.capitalization_bonus, sc.delimiter_bonus), sc.matching_case_bonus), 0)
                                       : overflow_guard(sc, (size_t)m->rows);
    if (!perr.empty()) return fail(FZB_ERR_PANIC, perr);
    // beyond NeedleDev's by-value arrays: the needle's arrays go to device memory (NeedleLongDev) and the query runs through the
    // kernels that take it from there (run_pipeline_long) - any length the reference's guard above accepted
    m->long_needle = needle_len > FZB_MAX_NEEDLE_BYTES || m->rows > FZB_MAX_ROWS;
    fill_needle_scalars(m, needle_len, cps.size());
    if (m->long_needle) {
        build_long_needle(m, needle_utf8, needle_len, cps);
        return FZB_OK;
    }
    NeedleDev& nd = m->nd;
    for (size_t i = 0; i < needle_len; i++) {  // case_needle (src/prefilter/mod.rs:49-65)
        nd.raw[i] = nd.c[i] = needle_utf8[i];
        nd.f[i] = flip_ascii_byte(m, needle_utf8[i]);
    }
    for (size_t i = 0; i < cps.size() && cps.size() <= FZB_MAX_ROWS; i++) {  // case_needle_unicode (src/prefilter/mod.rs:71-96)
        nd.ulen[i] = (u8)encode_utf8(cps[i], nd.uc[i]);
        encode_utf8(m->case_sensitive ? cps[i] : flip_same_width(cps[i]), nd.uf[i]);
    }
    // ---- filter-stage configuration --------------------------------------------------------------
    const int k = config->max_typos;
    LaunchCfg& lc = m->lc;
    if (k < 0 || k >= m->rows) {        // NO_PREFILTER, or `needle_len <= max_typos => (true, 0, len)`
        lc.filter_mode = 0; lc.filter_exact = 1; lc.window_mode = 2;
    } else if (!m->unicode && k == 0) { // exact: ordered subsequence; window = first/last occurrence
        lc.filter_mode = 1; lc.filter_exact = 1; lc.window_mode = 1;
    } else {                            // superset filter, lane-exact prefilter re-decides
        lc.filter_mode = k == 0 ? 1 : 2; lc.filter_exact = 0; lc.window_mode = 0;
    }
    build_filter_tables(m);
    build_unicode_dfa(m);
    build_lcs_dfa(m);
    build_cdfa(m);
    set_scorer_forms(m, needle_utf8, needle_len);
    // the stream stage of these queries is the ordered-subsequence automaton over the needle's bytes and their case flips
    m->sig_eligible = !m->unicode && lc.filter_mode == 1 && lc.filter_exact && needle_sig_eligible(needle_utf8, needle_len, k, m->literal_mode);
    m->needle_sig = m->sig_eligible ? needle_sig(needle_utf8, needle_len) : 0u;
    m->needle_sig2 = m->sig_eligible ? needle_sig2(needle_utf8, needle_len) : 0u;
    return FZB_OK;
}

int fzb_matcher_create(const fzb_config* config, const uint8_t* needle_utf8, size_t needle_len, fzb_matcher** out) {
    if (!out) return fail(FZB_ERR_INVALID, "null argument");
    std::unique_ptr<fzb_matcher> mp(new fzb_matcher());
    if (int rc = compile_needle(*mp, config, needle_utf8, needle_len)) return rc;
    *out = mp.release();
    return FZB_OK;
}

// `Matcher::set_pattern` / `Matcher::set_config` (src/matcher/mod.rs:154-176): the matcher's CompiledNeedle half is compiled anew, exactly
// as fzb_matcher_create would, and takes the old one's place; its MatcherState half - the workspace, staging, scratch, streams, events,
// pinned words, shard clones and workers, all sized by the corpus and the session, not by the needle - stays as it is.  So a re-query
// after every keystroke costs one small table upload instead of a round of device allocations, and a buffer added to MatcherState is
// kept without being named here.  What does depend on the needle is reset below, line by line.
static int rebuild_matcher(fzb_matcher* m, const fzb_config* config, const uint8_t* needle_utf8, size_t needle_len) {
    CompiledNeedle fresh;
    int rc = compile_needle(fresh, config, needle_utf8, needle_len);
    if (rc) return rc;  // m is left as it was
    const int num_cus = m->lc.num_cus;
    static_cast<CompiledNeedle&>(*m) = std::move(fresh);
    m->lc.num_cus = num_cus;      // the bound device's, not the needle's (fzb_bind_device)
    m->ws.tables_stale = true;    // the next query uploads the new needle's tables
    if (m->long_blob_dev) (void)hipFree(m->long_blob_dev);  // the old long needle's arrays: `ndl` points nowhere until ensure_long_needle uploads the new blob
    m->long_blob_dev = nullptr;
    memset(m->last_counters, 0, sizeof(m->last_counters));
    // the per-shard clones of the multi-device form follow (same needle, same config with the resolved lane pair); their device
    // state stays where it is
    if (!m->shard_clones.empty()) {
        fzb_config ccfg = m->config;
        ccfg.pf_lanes = (uint16_t)m->lc.pf_lanes;
        ccfg.sw_lanes = (uint16_t)m->lc.sw_lanes;
        bool ok = true;
        for (fzb_matcher* cm : m->shard_clones) ok = ok && rebuild_matcher(cm, &ccfg, needle_utf8, needle_len) == FZB_OK;
        if (!ok) {  // cannot happen for a needle / config the main matcher accepted; drop the clones rather than keep stale ones
            std::vector<fzb_matcher*> drop;
            drop.swap(m->shard_clones);
            for (fzb_matcher* cm : drop) fzb_matcher_free(cm);
            fzb_clear_error();
        }
    }
    return FZB_OK;
}

int fzb_matcher_set_pattern(fzb_matcher* m, const uint8_t* needle_utf8, size_t needle_len) {
    if (!m || (!needle_utf8 && needle_len)) return fail(FZB_ERR_INVALID, "null argument");
    if (m->needle.size() == needle_len && (needle_len == 0 || memcmp(m->needle.data(), needle_utf8, needle_len) == 0)) return FZB_OK;  // "skipped if the pattern is the same"
    const fzb_config cfg = m->config;
    return rebuild_matcher(m, &cfg, needle_utf8, needle_len);
}

}  // extern "C"
// field by field: fzb_config / fzb_scoring have padding bytes a C caller need not have cleared
static bool same_scoring(const fzb_scoring& a, const fzb_scoring& b) {
    return a.match_score == b.match_score && a.mismatch_penalty == b.mismatch_penalty && a.gap_open_penalty == b.gap_open_penalty && a.gap_extend_penalty == b.gap_extend_penalty &&
           a.prefix_bonus == b.prefix_bonus && a.capitalization_bonus == b.capitalization_bonus && a.matching_case_bonus == b.matching_case_bonus &&
           a.exact_match_bonus == b.exact_match_bonus && a.delimiter_bonus == b.delimiter_bonus;
}
static bool same_config(const fzb_config& a, const fzb_config& b) {
    return a.max_typos == b.max_typos && a.casing == b.casing && a.unicode == b.unicode && a.sort == b.sort && a.pf_lanes == b.pf_lanes && a.sw_lanes == b.sw_lanes &&
           a.matching == b.matching && same_scoring(a.scoring, b.scoring);
}
extern "C" {

int fzb_matcher_set_config(fzb_matcher* m, const fzb_config* config) {
    if (!m || !config) return fail(FZB_ERR_INVALID, "null argument");
    if (same_config(m->config, *config)) return FZB_OK;
    const std::string needle = m->needle;
    return rebuild_matcher(m, config, (const uint8_t*)needle.data(), needle.size());
}

int fzb_matcher_clone(const fzb_matcher* src, fzb_matcher** out) {
    if (!src || !out) return fail(FZB_ERR_INVALID, "null argument");
    fzb_config cfg = src->config;
    cfg.pf_lanes = (uint16_t)src->lc.pf_lanes;
    cfg.sw_lanes = (uint16_t)src->lc.sw_lanes;
    return fzb_matcher_create(&cfg, (const uint8_t*)src->needle.data(), src->needle.size(), out);
}

void fzb_matcher_free(fzb_matcher* m) {
    if (!m) return;
    release_state(*m);
    if (!m->shard_clones.empty()) {
        // a clone's device state lives on its shard's device
        int cur = 0;
        const bool have_cur = hipGetDevice(&cur) == hipSuccess;
        for (fzb_matcher* cm : m->shard_clones) {
            if (cm->shard_device >= 0) (void)hipSetDevice(cm->shard_device);
            fzb_matcher_free(cm);
        }
        m->shard_clones.clear();
        if (have_cur) (void)hipSetDevice(cur);
    }
    delete m;
}

int fzb_matcher_info(const fzb_matcher* m, int32_t out[6]) {
    if (!m || !out) return fail(FZB_ERR_INVALID, "null argument");
    out[0] = m->lc.pf_lanes; out[1] = m->lc.sw_lanes; out[2] = m->use_u8; out[3] = m->case_sensitive; out[4] = m->unicode; out[5] = m->rows;
    return FZB_OK;
}

// ---- corpus (fzb_corpus_upload: host_upload.hip) -------------------------------------------------------
}  // extern "C"
// A promise about BORROWED memory (uniform length / longest haystack) selects kernels that compute spans instead of reading the end
// offsets, or that skip launches: a wrong one would silently mis-span every haystack.  One pass over the end offsets checks it when it is
// made (a set-up call: it synchronises): offsets non-decreasing in the padded-16 layout and inside the buffer, every length == uniform_len
// (when given), every length <= max_len (when given).  out[0] = number of violations, out[1] = the first offending index.
template <typename ET>
__global__ __launch_bounds__(256) void k_verify_promise(const ET* __restrict__ ends, u64 n, u64 total_bytes, u32 uniform_len, u32 max_len, unsigned long long* __restrict__ out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u32 bad = 0;
    u64 first_bad = ~0ull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 e = (u64)ends[i];
        const u64 s = i ? (((u64)ends[i - 1] + 15ull) & ~15ull) : 0ull;
        bool ok = e >= s && e <= total_bytes;
        const u64 len = e - s;
        if (uniform_len) ok = ok && len == (u64)uniform_len;
        if (max_len) ok = ok && len <= (u64)max_len;
        if (!ok) {
            bad++;
            first_bad = first_bad < i ? first_bad : i;
        }
    }
    if (bad) {
        atomicAdd(&out[0], (unsigned long long)bad);
        atomicMin(&out[1], (unsigned long long)first_bad);
    }
}
static int verify_promise(const fzb_corpus* c, u32 uniform_len, u32 max_len, const char* what) {
    if (!fzb_knobs().verify_promises || !c->dev.n || (!uniform_len && !max_len)) return FZB_OK;
    unsigned long long* d = nullptr;
    // the borrowed buffers may live on another device than the caller's current one: the check runs where the end offsets are
    int prev_dev = 0, own_dev = 0;
    HIPCHK(hipGetDevice(&prev_dev));
    own_dev = prev_dev;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, c->dev.ends) == hipSuccess && attr.type == hipMemoryTypeDevice) own_dev = attr.device;
    else (void)hipGetLastError();
    struct DeviceGuard {
        int prev, cur;
        ~DeviceGuard() { if (cur != prev) (void)hipSetDevice(prev); }
    } guard{prev_dev, own_dev};
    if (own_dev != prev_dev) HIPCHK(hipSetDevice(own_dev));
    HIPCHK(hipDeviceSynchronize());  // the caller may have filled the buffers on any stream of that device
    HIPCHK(dev_alloc((void**)&d, 16));
    const unsigned long long init[2] = {0ull, ~0ull};
    hipError_t e = hipMemcpy(d, init, 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int grid = (int)fzb_grid_cap((c->dev.n + 255) / 256, 16);  // (4096 on 256 CUs)
        if (c->dev.ends_u64) FZB_LAUNCH((k_verify_promise<u64>), dim3(grid), dim3(256), 0, 0, (const u64*)c->dev.ends, c->dev.n, c->dev.total_bytes, uniform_len, max_len, d);
        else FZB_LAUNCH((k_verify_promise<u32>), dim3(grid), dim3(256), 0, 0, (const u32*)c->dev.ends, c->dev.n, c->dev.total_bytes, uniform_len, max_len, d);
        e = hipGetLastError();
    }
    unsigned long long got[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(got, d, 16, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FZB_ERR_HIP, std::string("verifying the corpus promise: ") + hipGetErrorString(e));
    if (got[0])
        return fail(FZB_ERR_INVALID, std::string(what) + ": the end offsets contradict it for " + std::to_string(got[0]) + " haystack(s), first at index " + std::to_string(got[1]) +
                                         " (checked on the device; FZB_VERIFY_PROMISES=0 skips the check)");
    return FZB_OK;
}
extern "C" {
int fzb_corpus_from_device(const void* dev_bytes, const void* dev_ends, int ends_are_u64, size_t n, uint64_t total_bytes, fzb_corpus** out) {
    if (!out || (n && (!dev_bytes || !dev_ends))) return fail(FZB_ERR_INVALID, "null argument");
    if (((uintptr_t)dev_bytes & 15) != 0) return fail(FZB_ERR_INVALID, "dev_bytes must be 16-byte aligned");
    if (n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    auto c = new fzb_corpus();
    c->dev.bytes = (const u8*)dev_bytes;
    c->dev.ends = dev_ends;
    c->dev.ends_u64 = ends_are_u64 != 0;
    c->dev.n = n;
    c->dev.total_bytes = total_bytes;
    *out = c;
    return FZB_OK;
}

void fzb_corpus_free(fzb_corpus* c) {
    if (!c) return;
    if (c->own_bytes) (void)hipFree(c->own_bytes);
    if (c->own_ends) (void)hipFree(c->own_ends);
    if (c->own_sig) (void)hipFree(c->own_sig);
    if (c->own_planes) (void)hipFree(c->own_planes);
    if (c->own_planes2) (void)hipFree(c->own_planes2);
    fzb_column_release(c->bias);
    fzb_column_release(c->tags);
    if (c->pair_stage) (void)hipFree(c->pair_stage);
    for (void* q : c->own_view)
        if (q) (void)hipFree(q);
    for (void* q : {c->stage_raw, c->stage_ends, c->stage_tiles, c->stage_stats})
        if (q) (void)hipFree(q);
    delete c;
}
size_t fzb_corpus_len(const fzb_corpus* c) { return c ? (size_t)c->dev.n : 0; }
int fzb_corpus_set_uniform_len(fzb_corpus* c, uint32_t len) {
    if (!c) return fail(FZB_ERR_INVALID, "null argument");
    // an uploaded corpus knows its lengths: only the detected value (a no-op) is accepted, anything else would make the kernels that
    // compute spans and the ones that read the end offsets disagree within one query
    if (c->own_bytes) {
        if (len == c->dev.uniform_len) return FZB_OK;
        return fail(FZB_ERR_INVALID, "the corpus was uploaded by fzb_corpus_upload, which detected its lengths itself (uniform length " + std::to_string(c->dev.uniform_len) +
                                         ", 0 = not uniform); the promise can only be made for borrowed device memory");
    }
    if (len && (u64)((len + 15u) & ~15u) * (c->dev.n ? c->dev.n - 1 : 0) + len > c->dev.total_bytes) return fail(FZB_ERR_INVALID, "uniform length does not fit the corpus buffer");
    if (len) {  // the promise is checked against the end offsets before any kernel relies on it
        const int vrc = verify_promise(c, len, 0, ("a uniform length of " + std::to_string(len) + " bytes was promised").c_str());
        if (vrc) return vrc;
    }
    if (!len && c->dev.uniform_len && c->dev.max_len == c->dev.uniform_len) c->dev.max_len = 0;  // clearing the promise also clears the bound it implied
    c->dev.uniform_len = len;
    if (len) c->dev.max_len = len;  // (overwrites an earlier fzb_corpus_set_max_len)
    return fzb_sig_sync_borrowed(c);  // the letter signatures of a list of short haystacks; a cleared promise drops them
}

int fzb_corpus_set_max_len(fzb_corpus* c, uint32_t max_len) {
    if (!c) return fail(FZB_ERR_INVALID, "null argument");
    // an uploaded corpus knows its longest haystack: a hint can only repeat or loosen it (ignored), and one BELOW it is refused - kernels are
    // selected by this bound and would skip bytes
    if (c->own_bytes) {
        if (max_len == 0 || max_len >= c->dev.max_len) return FZB_OK;
        return fail(FZB_ERR_INVALID, "the corpus was uploaded by fzb_corpus_upload, which measured its longest haystack (" + std::to_string(c->dev.max_len) + " bytes); " +
                                         std::to_string(max_len) + " is not an upper bound");
    }
    if (c->dev.uniform_len) {  // a (verified) uniform length implies its own, tighter bound: a looser one is accepted and changes nothing
        if (max_len == 0 || max_len >= c->dev.uniform_len) return FZB_OK;
        return fail(FZB_ERR_INVALID, "the corpus promises a uniform length of " + std::to_string(c->dev.uniform_len) + " bytes; " + std::to_string(max_len) + " is not an upper bound");
    }
    if (max_len && max_len != c->dev.uniform_len) {  // (a uniform length already verified implies its own bound)
        const int vrc = verify_promise(c, 0, max_len, ("a longest haystack of " + std::to_string(max_len) + " bytes was promised").c_str());
        if (vrc) return vrc;
    }
    c->dev.max_len = max_len;
    return fzb_sig_sync_borrowed(c);  // the letter signatures when the bound is within 32 bytes; a looser or cleared bound drops them
}

}  // extern "C"
// A matcher's device state (workspace, staging, sort buffers) lives on the device that was current at its first query; later queries
// must find the same device current.
int fzb_bind_device(fzb_matcher* m) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (m->device >= 0) {
        if (dev != m->device)
            return fail(FZB_ERR_INVALID, "matcher is bound to device " + std::to_string(m->device) + " (its workspace lives there) but device " + std::to_string(dev) + " is current");
        return FZB_OK;
    }
    int cus = 0;
    HIPCHK((hipError_t)fzb_effective_cus(&cus));  // (a device that cannot be asked is reported here, at bind time, and leaves the matcher unbound)
    m->device = dev;
    m->lc.num_cus = cus;
    return FZB_OK;
}
extern "C" {

// ---- pipeline -------------------------------------------------------------------------------------------
// ASCII typo configuration whose scorer can be the short-haystack kernel: the filter's LCS criterion decides, only its marginal
// survivors (LCS == rows - k) are re-decided at the exact lane width, and the scorer computes the lane-free window itself
// (whether the corpus allows it - max_len - is known per call: run_pipeline)
static bool typo_fast_path_configured(const fzb_matcher* m) {
    // FZB_TYPO_EXACT_WINDOW=1: every typo query takes the reference's chunked multi-path scan at the exact lane width for every survivor
    // (superset filter -> k2a_window -> k_compact2), i.e. nothing rests on the two properties of DESIGN.md section 3e
    if (fzb_knobs().typo_exact_window) return false;
    return !m->literal_mode && !m->empty && m->lc.filter_mode == 2 && !m->nd.unicode && m->lc.cf_ok && (m->lc.sw_lanes == 64 || m->lc.sw_lanes == 32);
}

// every_form: the buffers of every filter / scorer form, whatever this needle needs (a multi-pattern slot changes form between keystrokes)
static int ensure_workspace(fzb_matcher* m, size_t count, hipStream_t st = nullptr, bool have_stream = false, bool every_form = false) {
    Workspace& w = m->ws;
    const bool need_l2 = every_form || !m->lc.filter_exact;
    const bool need_marg = every_form || typo_fast_path_configured(m);
    const bool need_cls = every_form || (!m->literal_mode && !m->empty && !m->nd.unicode && m->lc.cf_ok);  // classified scoring (fzb_launch_dp_classes)
    // (cap_items >= count + FZB_UNICODE_FWD_CAP: run_pipeline anchors the queue's back at count + FZB_UNICODE_FWD_CAP entries - a workspace
    // allocated for a smaller range holds count0 + count0/8 + 4096 entries and must not be reused for a range within 4096 of that)
    if (w.cap_items >= count + FZB_UNICODE_FWD_CAP && (!need_l2 || w.cap_level2 >= count) && (!need_marg || w.cap_marg >= count) && (!need_cls || w.cap_cls >= count) && w.counters) {
        if (w.tables_stale) return upload_tables(m, st, have_stream);  // fzb_matcher_set_pattern / set_config kept the device buffers: only the tables change
        return FZB_OK;
    }
    free_workspace(w);
    const size_t cap = count + count / 8 + 4096;
    const size_t ntiles = ((cap + FZB_TILE - 1) / FZB_TILE + 5) & ~(size_t)3;  // (two spare, then a multiple of four entries: the compactions sum the counts as 16-byte vectors)
    HIPCHK(dev_alloc((void**)&w.bitmap, (cap / 64 + 17) * 8));
    HIPCHK(dev_alloc((void**)&w.tile_counts, ntiles * 4));
    HIPCHK(dev_alloc((void**)&w.surv_idx, cap * 4));
    HIPCHK(dev_alloc((void**)&w.overflow, cap * 16));
    // (the counter block, and behind it the segment counts of a filter that lists its own survivors: seg_list.h)
    HIPCHK(dev_alloc((void**)&w.counters, 64 + FZB_SEG_MAX * 4));
    w.seg_counts = w.counters + 16;
    static_assert(FZB_UNICODE_FWD_CAP >= FZB_TILE, "surv_idx holds the range rounded up to a tile: the segmented list's reach");
    // (room for any needle's automata: short needles 64 states, a long needle's subsequence DFA up to 201, unicode <= 255 + 1, LCS <= 226)
    HIPCHK(dev_alloc((void**)&w.tables_blob, TB_TOTAL));
    HIPCHK(hipHostMalloc((void**)&w.tables_host, TB_TOTAL, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&w.tables_ev, hipEventDisableTiming));
    w.table = (u64*)(w.tables_blob + TB_TABLE);
    w.dfa = w.tables_blob + TB_DFA;
    w.uni_dfa = w.tables_blob + TB_UNI;
    w.lcs_dfa = w.tables_blob + TB_LCS;
    w.cdfa = w.tables_blob + TB_CDFA;
    {
        const int rc_t = upload_tables(m, st, have_stream);
        if (rc_t) return rc_t;
    }
    w.cap_items = cap;
    if (need_l2) {
        HIPCHK(dev_alloc((void**)&w.win, cap * 8));
        HIPCHK(dev_alloc((void**)&w.bitmap2, (cap / 64 + 17) * 8));
        HIPCHK(dev_alloc((void**)&w.tile_counts2, ntiles * 4));
        HIPCHK(dev_alloc((void**)&w.items2, cap * 4));
        HIPCHK(dev_alloc((void**)&w.win2, cap * 8));
        w.cap_level2 = cap;
    }
    if (need_marg) {
        HIPCHK(dev_alloc((void**)&w.bitmap_m, (cap / 64 + 17) * 8));
        HIPCHK(dev_alloc((void**)&w.tile_counts_m, ntiles * 4));
        HIPCHK(dev_alloc((void**)&w.marg_list, cap * 4));
        HIPCHK(dev_alloc((void**)&w.reject_bits, (cap / 64 + 17) * 8));
        HIPCHK(dev_alloc((void**)&w.tile_rejects, ntiles * 4));
        HIPCHK(dev_alloc((void**)&w.rej_prefix, ntiles * 4));
        w.cap_marg = cap;
    }
    if (need_cls) {
        HIPCHK(dev_alloc((void**)&w.cls_win, cap * 16));  // 16-byte records (window, flag, source address)
        HIPCHK(dev_alloc((void**)&w.cls_lists, cap * 28));  // 3 single-chunk classes + 4 multi-chunk tail classes
        w.cap_cls = cap;
    }
    return FZB_OK;
}

// ---- buffers beyond the per-range workspace, each grown by ONE helper so that fzb_matcher_reserve can size all of them ahead of
// the first query (a re-query after every keystroke must not meet a hipFree / hipMalloc) --------------------------------------
static int ensure_aux_stream(fzb_matcher* m) {
    if (m->aux_stream && m->ev_fork && m->ev_join) return FZB_OK;
    // all three or none: created into locals and published together, so a failure half way leaves the matcher on its single-stream path
    hipStream_t s = nullptr;
    hipEvent_t ef = nullptr, ej = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ef, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ej, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (ej) (void)hipEventDestroy(ej);
        if (ef) (void)hipEventDestroy(ef);
        if (s) (void)hipStreamDestroy(s);
        return fail(FZB_ERR_HIP, std::string("second stream of the query: ") + hipGetErrorString(e));
    }
    m->aux_stream = s;
    m->ev_fork = ef;
    m->ev_join = ej;
    return FZB_OK;
}
static size_t dp_scratch_words(int rows, int sw_lanes, int mgrid) { return (size_t)(rows + 1) * (size_t)(sw_lanes / 2) * (size_t)mgrid * 128; }
static int ensure_dp_scratch_words(fzb_matcher* m, size_t words) { return fzb_grow_dev(&m->ws.dp_scratch, &m->ws.dp_scratch_words, words); }
static int ensure_dp_scratch(fzb_matcher* m, int mgrid) {  // parked rows of the multi-chunk scorer
    return ensure_dp_scratch_words(m, dp_scratch_words(m->nd.rows, m->lc.sw_lanes, mgrid));
}
}  // extern "C"
// ping-pong buffer + tile histograms of the device radix sort, for `cap` records
int fzb_sort_ensure(SortBuffers& s, size_t cap) {
    if (s.cap >= cap && s.tmp) return FZB_OK;
    s.cap = 0;
    int rc;
    const size_t hist_words = (size_t)2 * 256 * (cap / 2048 + 2);  // tile histograms + their scan; behind them two sets of digit totals + the phase word (kernels_sort.hip)
    if ((rc = fzb_dev_renew(&s.tmp, cap + 16)) || (rc = fzb_dev_renew(&s.hist, hist_words + 1024))) return rc;
    HIPCHK(hipMemset(s.hist + hist_words, 0, 1024 * 4));
    s.cap = cap;
    return FZB_OK;
}
static int ensure_sort_buffers(fzb_matcher* m, size_t cap) { return fzb_sort_ensure(m->ws.sort, cap); }
int fzb_out_ensure(OutStaging& o, size_t count) {  // device-side result of the synchronous entry points
    if (o.out_cap >= count && o.count_dev && o.out_dev) return FZB_OK;
    o.out_cap = 0;
    if (int rc = fzb_dev_renew(&o.out_dev, count + 16)) return rc;
    o.out_cap = count;
    if (!o.count_dev) HIPCHK(fzb_dev_alloc((void**)&o.count_dev, OUT_WORDS * sizeof(u32)));
    return FZB_OK;
}

// ---- the corpus' per-haystack score bias on the query path (score_bias.h; the corpus side is host_upload.hip) --------------------------
// The ONE helper that launches k_bias_apply: index-ordered records (up to `cap`, count[0] written) of the range that starts at haystack
// `first`, numbered from index_offset.  Called where such records are final and before anything selects or orders them; nothing is
// launched for a corpus without a bias.
static int apply_bias(const fzb_corpus* c, fzb_match_rec* recs, const u32* count, size_t cap, size_t first, uint32_t index_offset, int grid_max, hipStream_t st) {
    const int16_t* bias = fzb_corpus_bias(c);
    if (!bias || !cap) return FZB_OK;
    fzb_launch_bias_apply(recs, count, (u32)std::min<size_t>(cap, 0xFFFFFFFFu), bias, c->dev.n, first, index_offset, grid_max, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
// ---- the corpus' visibility scope on the query path (scope.h) ------------------------------------------------------------------------
// A query over a corpus with an active scope: the producer (the pipeline, the multi-pattern composition) writes its index-ordered records
// into the matcher's ScopeScratch - room for one per haystack of the range, its pair in scratch.words - and apply_terms applies the LIST's
// terms to them: drop the records of hidden haystacks (flag pass + stable compaction into the caller's array of `capacity` records,
// dev_count = (written, visible matches)), then add the bias.  The ONE helper that launches the drop; a corpus without an active scope never
// gets here and takes the launches it took before.
// (f: the matcher's facet sink, or null.  With one the flag pass counts the records' tag facets as well - the fused form, facets.h - and
// the caller may come here WITHOUT an active scope: a _device form whose `capacity` would cut the producer ahead of the count writes into
// the scratch too, and the drop under the scope (0, 0) keeps every record.)
static int facets_open(fzb_facets* f, hipStream_t st);
static int facets_close(fzb_facets* f, hipStream_t st);
static int apply_terms(const fzb_corpus* c, ScopeScratch& sc, size_t count, fzb_match_rec* dev_out, size_t capacity, u32* dev_count, size_t first, uint32_t index_offset, int grid_max,
                       hipStream_t st, fzb_facets* f = nullptr) {
    const u32 cap32 = (u32)std::min<size_t>(capacity, 0xFFFFFFFFu);
    const bool scoped = fzb_corpus_scoped(c);
    if (int rc = facets_open(f, st)) return rc;
    fzb_launch_scope_drop(sc.recs, sc.words, (u32)count, c->tags.data, c->dev.n, first, index_offset, scoped ? c->scope_require : 0u, scoped ? c->scope_exclude : 0u, sc.bitmap, sc.tiles, dev_out,
                          cap32, dev_count, grid_max, st, f ? f->block : nullptr);
    HIPCHK(hipGetLastError());
    if (int rc = facets_close(f, st)) return rc;
    return apply_bias(c, dev_out, dev_count, std::min(capacity, count), first, index_offset, grid_max, st);
}
// ---- the tag facets on the query path (facets.h; fzb_facets: host_internal.h) -----------------------------------------------------------
// A matcher with a facet sink attached: every query that honours the sink counts the tag facets of its match set A - the records the
// producer wrote, where a capture= of the same call reads them: ahead of scope, bias, selection, limit and ordering.  Three forms:
//   * under an active scope the count rides in the drop's flag pass (apply_terms above): no second pass over the records;
//   * without one, facets_records - the ONE helper that launches k_facets_records, beside subset_capture and at the same sites;
//   * the empty prompt's producers make no records for hidden haystacks: facets_column reads the tag column over the range or the set.
// Each clears the block in stream order (facets_open), counts, and queues the block's copy to the page-locked mirror (facets_close) - in
// front of a host form's one wait, behind nothing else.  Without a sink nothing here launches or allocates.
int fzb_refuse_facets(const fzb_facets* f, const char* call) {
    if (!f) return FZB_OK;
    return fail(FZB_ERR_INVALID, std::string(call) + ": the matcher has a facet sink attached, which this call does not fill; detach it first: set_facets(NULL)");
}
// any-of groups (anyof.h): the forms that return matched positions, and the multi-device forms, do not compose them - the traced union
// (indices_union.h) assumes every positive pattern matches every head record, and an alternative need not
int fzb_refuse_groups(const fzb_multi_matcher* mm, const char* call) {
    if (!mm || !mm->grouped) return FZB_OK;
    return fail(FZB_ERR_INVALID, std::string(call) + ": the matcher has an any-of group, which this call does not compose; use the records forms (fzb_multi_match_list, _top, _top_sections)");
}
// a sink counts over the corpus it was created on
static int facets_check(const fzb_facets* f, const fzb_corpus* c, const char* call) {
    if (!f || !c || f->corpus == c) return FZB_OK;
    return fail(FZB_ERR_INVALID, std::string(call) + ": the attached facet sink belongs to another corpus; detach it first: set_facets(NULL)");
}
static int facets_open(fzb_facets* f, hipStream_t st) {
    if (!f) return FZB_OK;
    HIPCHK(hipMemsetAsync(f->block, 0, FZB_FACET_WORDS * sizeof(u32), st));
    return FZB_OK;
}
static int facets_close(fzb_facets* f, hipStream_t st) {
    if (!f) return FZB_OK;
    HIPCHK(hipMemcpyAsync(f->mirror, f->block, FZB_FACET_WORDS * sizeof(u32), hipMemcpyDeviceToHost, st));
    f->on_event = st != nullptr;
    if (f->on_event) HIPCHK(hipEventRecord(f->done, st));
    f->pending = true;
    return FZB_OK;
}
// the wait for the last query's copy into the mirror: nothing is asked of the device when it has completed
static int facets_settle(fzb_facets* f) {
    if (!f->pending) return FZB_OK;
    if (f->on_event) {
        if (hipEventQuery(f->done) != hipSuccess) HIPCHK(hipEventSynchronize(f->done));
    } else if (hipStreamQuery(nullptr) != hipSuccess) {
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    f->pending = false;
    return FZB_OK;
}
// a query that launched nothing (an empty range): every count is zero
static int facets_none(fzb_facets* f, hipStream_t st) {
    if (int rc = facets_open(f, st)) return rc;
    return facets_close(f, st);
}
// recs = the producer's index-ordered records (pair[0] of them, at most cap) over the range that starts at haystack `first`, numbered from
// index_offset; a corpus with no active scope (every record is visible)
static int facets_records(fzb_facets* f, const fzb_corpus* c, const fzb_match_rec* recs, const u32* pair, size_t cap, size_t first, uint32_t index_offset, int grid_max, hipStream_t st) {
    if (!f) return FZB_OK;
    if (int rc = facets_open(f, st)) return rc;
    if (cap) fzb_launch_facets_records(recs, pair, (u32)std::min<size_t>(cap, 0xFFFFFFFFu), c->tags.data, c->dev.n, first, index_offset, 0u, 0u, f->block, grid_max, st);
    HIPCHK(hipGetLastError());
    return facets_close(f, st);
}
// the haystacks [first, first + count) - or those of `in`, whose count is read on the device - under the corpus' scope: the empty prompt's A
static int facets_column(fzb_facets* f, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, int grid_max, hipStream_t st) {
    if (!f) return FZB_OK;
    if (int rc = facets_open(f, st)) return rc;
    const bool scoped = fzb_corpus_scoped(c);
    const u64 hint = in ? std::min<u64>(std::max<u64>(1, in->known ? in->count : (u64)in->cap), count) : count;
    if (count)
        fzb_launch_facets_column(in ? in->idx : nullptr, in ? in->count_dev : nullptr, (u32)count, (u32)hint, c->tags.data, c->dev.n, first, scoped ? c->scope_require : 0u,
                                 scoped ? c->scope_exclude : 0u, f->block, grid_max, st);
    HIPCHK(hipGetLastError());
    return facets_close(f, st);
}
// the closed-form answers of an empty needle / an empty pattern list (no term, no candidate set: host work alone, nothing else is launched):
// A is every haystack of the range, counted from the column on the null stream of the current device (the corpus': these answers bind no
// matcher, so the grid's cap is the device's, fzb_grid_cap).  Such a form has no wait of its own to ride on, so the count's wait is made
// HERE: like every other host form it returns with the mirror current, and fzb_facets_read does no device work behind it.
static int facets_every(fzb_facets* f, const fzb_corpus* c, size_t first, size_t count, const char* call) {
    if (!f) return FZB_OK;
    if (int rc = facets_check(f, c, call)) return rc;
    if (int rc = facets_column(f, c, nullptr, first, count, (int)fzb_grid_cap(~0ull, 2), nullptr)) return rc;
    return facets_settle(f);
}
// "honours the scope or refuses": the entry points that cannot drop the hidden haystacks say so instead of ignoring the scope
int fzb_refuse_scoped(const fzb_corpus* c, const char* call, const char* instead) {
    if (!c || !fzb_corpus_scoped(c)) return FZB_OK;
    return fail(FZB_ERR_INVALID, std::string(call) + ": the corpus has an active scope, which this call does not apply; use " + instead + ", or fzb_corpus_set_scope(c, 0, 0) first");
}
// the list's terms, if any: what makes an empty needle's result more than "every index, score 0"
static bool corpus_terms(const fzb_corpus* c) { return fzb_corpus_bias(c) || fzb_corpus_scoped(c); }
// "returns biased scores or refuses": the entry points that cannot add the bias say so instead of ignoring it
int fzb_refuse_biased(const fzb_corpus* c, const char* call, const char* instead) {
    if (!c || !fzb_corpus_bias(c)) return FZB_OK;
    return fail(FZB_ERR_INVALID, std::string(call) + ": the corpus carries a score bias, which this call does not apply; use " + instead + ", or fzb_corpus_clear_bias first");
}
// entries [first, first + count) of one of the corpus' columns on the host (one device-to-host copy)
template <typename V>
static int fetch_column(const V* col, size_t first, size_t count, std::vector<V>& out) {
    out.assign(count, 0);
    if (count) HIPCHK(hipMemcpy(out.data(), col + first, count * sizeof(V), hipMemcpyDeviceToHost));
    return FZB_OK;
}
// ---- THE EMPTY PROMPT: CompiledPatterns::Empty (an empty needle) over a corpus with a score bias, an active scope or a candidate set -------
// The picker's first frame - "most frecent first", "the visible files", "this folder".  The rule (prompt_records.h): the haystacks of the
// range, or of `in`, that are visible under the scope, in index order, each with score clamp(bias, 0, 65535) (0 without a bias) and exact 0;
// reversed for the *Desc strategies; sorted stably by descending score for the Score* strategies ONLY over a biased corpus (a departure from
// the reference, whose empty result is never sorted; without a bias every score is 0 and the reference's rule holds); found = the number
// visible.  Everything runs on the device: the producer below writes the index-ordered records, the matcher's ordering and selection code
// takes them from there, and the host forms copy back what they copy for any query - the head and the count pair, in their one wait.  No
// column and no subset crosses the link.
// The prompt's records on `st`: up to `capacity` records of [first, first + count) - or of `in`, whose count is read on the device - into
// `out`, pair = (written, found).  One launch for a whole range without an active scope; flag pass + compaction otherwise (kernels_prompt.hip).
// The matcher is bound (fzb_bind_device) by the caller.
static int prompt_records(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, uint32_t index_offset, fzb_match_rec* out, size_t capacity, u32* pair,
                          hipStream_t st) {
    const u32 cap32 = (u32)std::min<size_t>(capacity, 0xFFFFFFFFu);
    const int16_t* bias = fzb_corpus_bias(c);
    const bool scoped = fzb_corpus_scoped(c);
    const int cus = m->lc.num_cus;
    if (int rc = facets_check(m->facets, c, "the empty prompt")) return rc;
    if (!in && !scoped) {
        fzb_launch_prompt_records(out, (u32)count, cap32, bias, c->dev.n, first, index_offset, pair, cus * 4, st);
    } else {
        if (int rc = fzb_scope_ensure_flags(m->scope, count)) return rc;
        // (over a candidate set: its count when the host knows it, else the room it was captured into - never more than the list)
        const u64 hint = in ? std::min<u64>(std::max<u64>(1, in->known ? in->count : (u64)in->cap), count) : count;
        fzb_launch_prompt_compact(in ? in->idx : nullptr, in ? in->count_dev : nullptr, (u32)count, (u32)hint, scoped ? c->tags.data : nullptr, c->dev.n, bias, c->dev.n, first, index_offset,
                                  c->scope_require, c->scope_exclude, m->scope.bitmap, m->scope.tiles, out, cap32, pair, cus * 2, st);
    }
    HIPCHK(hipGetLastError());
    // (the producers above make no records for hidden haystacks: the facets of the prompt's A come from the tag column)
    return facets_column(m->facets, c, in, first, count, cus * 2, st);
}
// What orders the prompt's list: the score is the clamped bias alone - no matrix score, no exact-match bonus - so a single radix pass / one
// histogram level is decided by bias_hi alone (a `one_pass` that is wrongly true would make the selection read the low byte only), and
// there is a score to sort by only over a biased corpus.
static void prompt_order_flags(const fzb_matcher* m, const fzb_corpus* c, bool* reversed, bool* by_score, bool* one_pass) {
    const int sort = m->config.sort;
    *reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    *by_score = fzb_corpus_bias(c) != nullptr && (sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC);
    *one_pass = sbias_one_pass(0, fzb_corpus_bias_hi(c));
}
// the list on `st`: index order (ordered = false: fzb_match_list_into, fzb_prompt_list_device) or what `match_list`'s post-step makes of it
static int prompt_list_stage(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, uint32_t index_offset, bool ordered, fzb_match_rec* dev_out,
                             size_t capacity, u32* dev_count, hipStream_t st) {
    const size_t cap = std::min(capacity, count);
    OrderPlan p;
    prompt_order_flags(m, c, &p.reversed, &p.by_score, &p.one_pass);
    if (!ordered) p.reversed = p.by_score = false;
    p.via_tmp = p.by_score && p.one_pass && cap != 0;
    p.in = dev_out;
    int rc;
    if (p.by_score) {
        if ((rc = fzb_ensure_sort_buffers(m, cap))) return rc;
        if (p.via_tmp) p.in = m->ws.sort.tmp;
    }
    if ((rc = prompt_records(m, c, in, first, count, index_offset, p.in, p.via_tmp ? cap : capacity, dev_count, st))) return rc;
    return fzb_order_finish(m, p, dev_out, dev_count, st);
}
// the ordered head on `st`: the records into the sort's second buffer, the selection of the best `want` = min(limit, n) and their ordering
// into dev_out (room for `want`), dev_count = (records, found)
static int prompt_top_stage(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t want, fzb_match_rec* dev_out, u32* dev_count, hipStream_t st) {
    const size_t n = c->dev.n;
    int rc;
    if ((rc = fzb_ensure_sort_buffers(m, n))) return rc;
    if (!m->count_dev && (rc = fzb_ensure_out_staging(m, 0))) return rc;
    bool reversed, by_score, one_pass;
    prompt_order_flags(m, c, &reversed, &by_score, &one_pass);
    Workspace& w = m->ws;
    u32* const raw_count = m->count_dev + OUT_RAW;  // the producer's pair (records written, visible haystacks)
    if ((rc = prompt_records(m, c, in, 0, n, 0, w.sort.tmp, n, raw_count, st))) return rc;
    const u32 ntiles_cap = (u32)(w.sort.cap / 2048 + 2);
    const int grid = m->lc.num_cus * 2;
    HIPCHK(fzb_launch_topk_select(w.sort.tmp, raw_count, (u32)n, (u32)want, by_score, reversed, one_pass, dev_out, (u32)want, dev_count, w.sort.hist, ntiles_cap, grid, st));
    fzb_launch_sort(dev_out, w.sort.tmp, dev_count, w.sort.hist, ntiles_cap, reversed, by_score, grid, st, one_pass ? 1 : 2);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
// the host forms: the stage on the null stream into the matcher's staging, then the copy any query makes
static int prompt_list_host(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, uint32_t index_offset, bool ordered, fzb_match** out, size_t* out_len) {
    int rc;
    if ((rc = fzb_bind_device(m)) || (rc = fzb_ensure_out_staging(m, count))) return rc;
    if ((rc = prompt_list_stage(m, c, in, first, count, index_offset, ordered, m->out_dev, count, m->count_dev, nullptr))) return rc;
    return fzb_fetch_records(m->fetch, m->out_dev, m->count_dev, 0, count, nullptr, out, out_len);
}
static int prompt_top_host(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    const size_t want = std::min<size_t>(limit, c->dev.n);
    int rc;
    if ((rc = fzb_bind_device(m)) || (rc = fzb_ensure_out_staging(m, want))) return rc;
    if ((rc = prompt_top_stage(m, c, in, want, m->out_dev, m->count_dev, nullptr))) return rc;
    return fzb_fetch_top(m->fetch_top, m->out_dev, m->count_dev, want, nullptr, out, out_len, out_found);
}
// does the device answer this matcher's query over [.., count) haystacks of c?  An empty needle over a non-empty range with a term or a
// candidate set; everything else of an empty needle is the closed-form host answer (fzb_empty_pattern_top and its siblings)
static bool prompt_on_device(const fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t count) { return m->empty && count != 0 && (in || corpus_terms(c)); }
// The same list on the HOST, for the one caller without an fzb_matcher (the `from_patterns` matcher's top + positions form with no pattern,
// empty_top_indices): CompiledPatterns::Empty (an empty needle, no pattern) over a BIASED corpus - the picker's empty prompt, "most frecent first": every haystack
// of [first, first + count) matches with score clamp(bias, 0, 65535), and - unlike the reference's unsorted empty result - the list is ordered
// per `sort` (reverse for the *Desc strategies, then the stable descending sort by score for the Score* ones), cut to `limit` records.
// Host work: one copy of the bias and the host's stable sort.  *out: malloc'ed (fzb_matches_free); *out_found (optional) = count.
// Over a corpus with an active SCOPE (with or without a bias) only the visible haystacks of the range are listed, each under its index in the
// full list (index_offset + (i - first)), and *out_found counts those; without a bias the scores are 0 and the reference's rule holds: reversed
// for the *Desc strategies, never sorted.  Host work: one copy of the tags, as of the bias.
static int biased_empty_list(const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, int sort, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    std::vector<int16_t> hb;
    std::vector<uint16_t> ht;
    const bool biased = fzb_corpus_bias(c) != nullptr, scoped = fzb_corpus_scoped(c);
    if (biased)
        if (int rc = fetch_column(fzb_corpus_bias(c), first, count, hb)) return rc;
    if (scoped)
        if (int rc = fetch_column(c->tags.data, first, count, ht)) return rc;
    std::vector<fzb_match> recs;
    recs.reserve(count);
    for (size_t i = 0; i < count; i++)
        if (!scoped || scope_visible(ht[i], c->scope_require, c->scope_exclude)) recs.push_back(fzb_match{(uint32_t)(index_offset + i), (uint16_t)(biased ? sbias_clamp_add(0, hb[i]) : 0), 0, 0});
    count = recs.size();
    if (sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC) std::reverse(recs.begin(), recs.end());
    if (biased && (sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC))
        std::stable_sort(recs.begin(), recs.end(), [](const fzb_match& a, const fzb_match& b) { return a.score > b.score; });
    const size_t keep = std::min(limit, count);
    fzb_match* r = (fzb_match*)malloc(std::max<size_t>(keep, 1) * sizeof(fzb_match));
    if (!r) return fail(FZB_ERR_INVALID, "out of memory");
    if (keep) memcpy(r, recs.data(), keep * sizeof(fzb_match));
    *out = r;
    *out_len = keep;
    if (out_found) *out_found = count;
    return FZB_OK;
}
extern "C" {

// matched-indices form of a query: where the positions go
struct TraceOut {
    u32* pos;
    u32* npos;
    u32 stride;
};
static int ensure_long_needle(fzb_matcher* m, size_t scratch_bytes) {  // the needle's arrays + the scratch its kernels need, on the device
    if (!m->long_blob_dev) {
        HIPCHK(dev_alloc(&m->long_blob_dev, m->long_blob_host.size()));
        HIPCHK(hipMemcpy(m->long_blob_dev, m->long_blob_host.data(), m->long_blob_host.size(), hipMemcpyHostToDevice));
        const u8* b = (const u8*)m->long_blob_dev;
        m->ndl.raw = b;
        m->ndl.c = b + m->long_off_c;
        m->ndl.f = b + m->long_off_f;
        m->ndl.uc = (const u8(*)[4])(b + m->long_off_uc);
        m->ndl.uf = (const u8(*)[4])(b + m->long_off_uf);
        m->ndl.ulen = b + m->long_off_ulen;
    }
    return scratch_bytes ? fzb_grow_dev(&m->long_scratch, &m->long_scratch_bytes, scratch_bytes) : FZB_OK;
}

// The pipeline of a LONG needle (> 64 bytes or > 63 rows; the reference takes them up to Scoring::max_needle_len(), src/lib.rs:480-503).
// Such a needle only matches haystacks about as long as itself, so nothing here is tuned for throughput; it is the same arithmetic through
// the kernels that take the needle from device memory:  [length test + the reference's prefilter at the exact lane width ->
// order-preserving compaction] -> the wave-per-haystack scorer (every window width; match_greedy beyond 1024 bytes; traced form for the
// matched-indices entry points) - or the two literal kernels.
// (profiling: [0] start, [2]..[3] around the first stage - the lane-exact prefilter over every haystack, when there is one -, [4] before the
// scorer, [1] end: the same five events fzb_last_stage_timings reads for the short-needle pipeline)
static int run_pipeline_long(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, const u32* items_in, const u32* n_items_in,
                             fzb_match* dev_out, u32 cap32, uint32_t* dev_count, hipStream_t st, const TraceOut* trace) {
    hipEvent_t* pev = nullptr;
    if (m->profiling) {
        const int slot = (int)(m->prof_calls % fzb_matcher::PROF_SLOTS);
        pev = m->evring[slot];
        m->ev_filter[slot] = (!m->literal_mode && m->lc.window_mode == 0) ? 1 : 0;
        m->prof_calls++;
        for (int i = 0; i < 5; i++)
            if (!pev[i]) HIPCHK(hipEventCreate(&pev[i]));
        HIPCHK(hipEventRecord(pev[0], st));
    }
    Workspace& w = m->ws;
    const CorpusDev& cd = c->dev;
    const int cus = m->lc.num_cus;
    const u32 cnt = (u32)count;
    u32* cnt_c = w.counters;
    const size_t budget = (size_t)256 << 20;  // global scratch per matcher: the grids below shrink to stay inside it
    if (m->literal_mode) {
        int rc = ensure_long_needle(m, 0);
        if (rc) return rc;
        fzb_launch_literal_filter_long(cd, first, cnt, items_in, n_items_in, m->ndl, m->literal_mode, w.bitmap, w.tile_counts, cus * 8, st);
        fzb_launch_compact1(w.bitmap, w.tile_counts, cnt, items_in ? n_items_in : nullptr, items_in, w.surv_idx, &cnt_c[0], cus * 2, st);
        if (pev) HIPCHK(hipEventRecord(pev[4], st));
        fzb_launch_literal_score_long(cd, first, index_offset, w.surv_idx, &cnt_c[0], m->ndl, m->literal_mode, (fzb_match_rec*)dev_out, cap32, dev_count, trace ? trace->pos : nullptr,
                                      trace ? trace->npos : nullptr, trace ? trace->stride : 0u, cus * 4, st);
        if (pev) HIPCHK(hipEventRecord(pev[1], st));
        HIPCHK(hipGetLastError());
        return FZB_OK;
    }
    const bool prefilter = m->lc.window_mode == 0;
    // grids: bounded by the scratch budget (a 10 922-row needle has 0.7 MB of previous-chunk vectors per wave, 50 MB of traced cells)
    int wgrid = std::max(1, cus * 2);
    if (prefilter && m->ndl.max_typos >= 3) {
        const size_t per_block = fzb_window_long_scratch_bytes(m->ndl, 1);
        wgrid = (int)std::max<size_t>(1, std::min<size_t>((size_t)wgrid, budget / std::max<size_t>(per_block, 1)));
    }
    int ggrid = std::max(1, cus * 2);
    {
        const size_t per_block = fzb_generic_long_adj_bytes(m->ndl, m->lc.sw_lanes, 1) + (trace ? fzb_trace_scratch_words_long(m->ndl, 1) * 4 : 0);
        ggrid = (int)std::max<size_t>(1, std::min<size_t>((size_t)ggrid, budget / std::max<size_t>(per_block, 1)));
        if (trace) ggrid = std::min(ggrid, (int)std::max<size_t>(1, (count + 3) / 4));
    }
    // ASCII windows of up to 1024 bytes: one THREAD per window (k2d_dp_long) when the parked-row slab lets enough of them run (a needle of
    // thousands of rows leaves room for a few thousand threads only: the wave-per-haystack kernel keeps those); matched indices and unicode
    // stay with the wave-per-haystack kernel, which also takes what k2d_dp_long queues (windows beyond 1024 bytes: match_greedy)
    const size_t dpl_words = fzb_dp_long_scratch_words_per_thread(m->ndl, m->lc.sw_lanes);
    const size_t dfit = std::min<size_t>((size_t)cus * 8, budget / std::max<size_t>(dpl_words * 4 * 128, 1));  // 128-thread workgroups the slab has room for
    const int dgrid = (int)std::max<size_t>(1, std::min<size_t>(dfit, (count + 127) / 128));
    const bool thread_per_window = !trace && !m->ndl.unicode && dfit >= (size_t)std::max(1, cus / 2);
    // four lanes per window (dp_quad.h) when dp_cfm.h's preconditions hold: a seventh of the slab per window, four times the wavefronts
    const size_t qwords = fzb_dp_long_quad_words_per_block(m->ndl, m->lc.sw_lanes);
    const bool quad = thread_per_window && m->lc.cfm_ok && !fzb_knobs().no_dp_cfm && qwords != 0;
    const int qgrid = quad ? (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)cus * 8, budget / (qwords * 4)), (count + 63) / 64)) : 0;
    const size_t dpl_bytes = quad ? qwords * 4 * (size_t)qgrid : thread_per_window ? dpl_words * 4 * 128 * (size_t)dgrid : 0;
    const bool greedy_possible = !(cd.max_len != 0 && cd.max_len <= FZB_MAX_HAYSTACK_LEN);
    if (thread_per_window && !greedy_possible) ggrid = 1;  // (no launch of the wave-per-haystack kernel: its slab is not needed)
    const size_t win_bytes = prefilter ? fzb_window_long_scratch_bytes(m->ndl, wgrid) : 0;
    const size_t adj_bytes = std::max(fzb_generic_long_adj_bytes(m->ndl, m->lc.sw_lanes, ggrid), dpl_bytes);
    const size_t cell_bytes = trace ? fzb_trace_scratch_words_long(m->ndl, ggrid) * 4 : 0;
    // (the prefilter's path state and the scorer's vectors are never live at the same time: they share the front of the scratch)
    const size_t front = (std::max(win_bytes, adj_bytes) + 255) & ~(size_t)255;
    int rc = ensure_long_needle(m, front + cell_bytes + 256);
    if (rc) return rc;
    const u32* items = items_in;
    const u32* win = nullptr;
    const u32* n_items_ptr = &cnt_c[0];
    int wmode = 2;
    if (items_in) HIPCHK(hipMemcpyAsync(&cnt_c[0], n_items_in, 4, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&cnt_c[0], (int)cnt, 1, st));
    // the streaming filter as first stage (0 typos, ASCII, up to 200 rows: fzb_matcher_create built the automaton) over a contiguous range;
    // the scorer then finds the lane-free window itself (wmode 1), as for short needles
    const bool use_dfa = m->long_dfa && thread_per_window && !items_in;
    if (use_dfa) {
        if (pev) HIPCHK(hipEventRecord(pev[2], st));
        fzb_launch_filter(cd, first, cnt, w.table, w.dfa, m->lc.dead_byte, m->ndl.rows, 1, m->ndl.rows, (u32)m->ndl.min_haystack_len, w.bitmap, w.tile_counts, w.counters, cus * 8, st, nullptr,
                          nullptr, nullptr, nullptr, m->lc.pad_ok, -1, nullptr, 0u, 0, 0);
        if (pev) HIPCHK(hipEventRecord(pev[3], st));
        fzb_launch_compact1(w.bitmap, w.tile_counts, cnt, nullptr, nullptr, w.surv_idx, &cnt_c[0], cus * 4, st);
        items = w.surv_idx;
        n_items_ptr = &cnt_c[0];
        wmode = 1;
    } else if (prefilter) {
        if (pev) HIPCHK(hipEventRecord(pev[2], st));
        fzb_launch_window_long(cd, first, items_in, &cnt_c[0], m->ndl, m->lc.pf_lanes, w.win, w.bitmap2, w.tile_counts2, m->long_scratch, wgrid, st);
        if (pev) HIPCHK(hipEventRecord(pev[3], st));
        fzb_launch_compact2(w.bitmap2, w.tile_counts2, &cnt_c[0], items_in, w.win, w.items2, w.win2, &cnt_c[1], cus * 2, st);
        items = w.items2;
        win = w.win2;
        n_items_ptr = &cnt_c[1];
        wmode = 0;
    } else {
        HIPCHK(hipMemcpyAsync(&cnt_c[1], &cnt_c[0], 4, hipMemcpyDeviceToDevice, st));
    }
    if (pev) HIPCHK(hipEventRecord(pev[4], st));
    if (thread_per_window) {
        if (quad)
            fzb_launch_dp_long_quad(cd, first, index_offset, items, win, wmode, n_items_ptr, m->ndl, m->lc.sw_lanes, m->long_upper ? 1 : 0, (fzb_match_rec*)dev_out, cap32, dev_count,
                                    (u32*)m->long_scratch, w.overflow, cnt_c, qgrid, st);
        else
        fzb_launch_dp_long(cd, first, index_offset, items, win, wmode, n_items_ptr, m->ndl, m->lc.sw_lanes, m->lc.bias_ok, (fzb_match_rec*)dev_out, cap32, dev_count, (u32*)m->long_scratch,
                           w.overflow, cnt_c, dgrid, st);
        // (the queue's entries are read after the slab's last use: the two kernels are one behind the other on the stream and share the scratch)
        if (greedy_possible)
            fzb_launch_generic_long(cd, first, index_offset, items, win, wmode, &cnt_c[3], m->ndl, m->lc.sw_lanes, (fzb_match_rec*)dev_out, cap32, nullptr, cnt_c, (u16*)m->long_scratch,
                                    nullptr, nullptr, nullptr, 0u, std::max(1, std::min(ggrid, cus / 4 + 1)), st, w.overflow);
    } else
    fzb_launch_generic_long(cd, first, index_offset, items, win, wmode, n_items_ptr, m->ndl, m->lc.sw_lanes, (fzb_match_rec*)dev_out, cap32, dev_count, cnt_c, (u16*)m->long_scratch,
                            trace ? (const u32*)((u8*)m->long_scratch + front) : nullptr, trace ? trace->pos : nullptr, trace ? trace->npos : nullptr, trace ? trace->stride : 0u, ggrid, st);
    if (pev) HIPCHK(hipEventRecord(pev[1], st));
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

// ---- the pipeline of a SHORT needle (NeedleDev by value), one function per path ------------------------------------------------------
// counters: [0]=filter survivors [1]=kept by the lane-exact prefilter [3]=multi-chunk queue [4]=generic (greedy / wide unicode) queue
// [5]=marginal survivors [6]=rejected marginal survivors [8..10]=single-chunk classes [12..15]=multi-chunk tail classes
struct Pipe {
    fzb_matcher* m;
    const CorpusDev& cd;
    size_t first;
    u32 cnt, index_offset;
    const u32* items_in;     // item list (indices relative to `first`) or nullptr = the contiguous range
    const u32* n_items_in;
    fzb_match_rec* out;
    u32 cap32;
    uint32_t* dev_count;
    hipStream_t st;
    const TraceOut* trace;
    hipEvent_t* pev;         // profiling events of this call (nullptr: not profiled)
    int cus;
    u64 items_hint = 0;      // the item list is a candidate set's: its length as far as the host knows (0: a few thousand items at most - the multi-pattern narrowing, a head's traced pass)
    // what the filter stage leaves for the scorers
    const u32* items = nullptr;
    const u32* win = nullptr;
    const u32* n_items_ptr = nullptr;
    int wmode = 0;
    bool classified = false;  // the compaction launch classified its survivors too (k_compact1_classify): pipe_score_ascii starts at the class scorers
    bool segmented = false;   // the signature filter listed its survivors itself (seg): no compaction ran, p.items is not a dense list
    SegList seg{};
};
#define FZB_STAGE(name)                                                                                        \
    do {                                                                                                       \
        if (fzb_knobs().debug_sync) { /* debugging aid: synchronise and report after every stage */            \
            hipError_t e_ = hipStreamSynchronize(p.st);                                                        \
            fprintf(stderr, "[fzb] stage %s: %s\n", name, hipGetErrorString(e_));                              \
            if (e_ != hipSuccess) return fail(FZB_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e_)); \
        }                                                                                                      \
    } while (0)
#define FZB_PEV(i)                                                    \
    do {                                                              \
        if (p.pev) HIPCHK(hipEventRecord(p.pev[i], p.st));            \
    } while (0)

// literal modes: accept pass (one bit per haystack) -> compaction -> scoring pass over the survivors (kernels_literal.hip)
static int pipe_literal(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const NeedleDev& nd = m->nd;
    u32* cnt_c = w.counters;
    if (m->literal_mode == FZB_MATCH_SUBSTRING && !nd.unicode && !p.items_in)  // the streaming DFA filter over the needle's KMP automaton
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.dfa, m->lc.dead_byte, nd.rows, 1, nd.rows, (u32)nd.nbytes, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, nullptr, nullptr, nullptr, nullptr,
                          m->lc.pad_ok, -1, m->cdfa_src == 1 ? w.cdfa : nullptr, (u32)m->cdfa.size(), m->cdfa_K, m->cdfa_G);
    else
        fzb_launch_literal_filter(p.cd, p.first, p.cnt, p.items_in, p.n_items_in, nd, m->literal_mode, w.bitmap, w.tile_counts, p.cus * 8, p.st);
    FZB_STAGE("literal filter");
    fzb_launch_compact1(w.bitmap, w.tile_counts, p.cnt, p.items_in ? p.n_items_in : nullptr, p.items_in, w.surv_idx, &cnt_c[0], p.cus * 2, p.st);
    FZB_STAGE("literal compact");
    fzb_launch_literal_score(p.cd, p.first, p.index_offset, w.surv_idx, &cnt_c[0], nd, m->literal_mode, p.out, p.cap32, p.dev_count, p.trace ? p.trace->pos : nullptr,
                             p.trace ? p.trace->npos : nullptr, p.trace ? p.trace->stride : 0u, p.cus * 4, p.st);
    FZB_STAGE("literal score");
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

// Typo configuration, every haystack fits half a score chunk (C3): the LCS criterion decides in the stream (with the "nothing to spare" bit when
// haystacks can span several PREFILTER chunks: only those marginal survivors are re-decided at the exact lane width, a reject sets a bit), and
// the short scorer computes the lane-free window itself (DESIGN.md "Typo configurations").  A haystack that fits ONE prefilter chunk is decided
// exactly by the criterion: the reference's multi-path scan loses a candidate only when a lower path that found nothing more in the current
// chunk advances again in a later one (tests/test_oracle_reference_properties.py::test_single_chunk_typo_prefilter_is_the_lcs_criterion).
static int pipe_typo_fast_path(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const LaunchCfg& lc = m->lc;
    const NeedleDev& nd = m->nd;
    u32* cnt_c = w.counters;
    const int need = nd.rows - nd.max_typos;
    const u32 ntiles = (p.cnt + FZB_TILE - 1) / FZB_TILE;
    const RejectOut rej{w.reject_bits, w.tile_rejects, w.rej_prefix, &cnt_c[6]};
    const bool single_chunk = p.cd.max_len <= (u32)lc.pf_lanes;
    FZB_PEV(2);
    if (single_chunk && m->lcs_states)  // the LCS criterion as an automaton in the streaming DFA kernel
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.lcs_dfa, lc.dead_byte, m->lcs_states - 1, 1, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, nullptr,
                          nullptr, nullptr, nullptr, lc.pad_ok, m->lcs_acc_lo, m->cdfa_src == 3 ? w.cdfa : nullptr, (u32)m->cdfa.size(), m->cdfa_K, m->cdfa_G);
    else if (single_chunk)
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.dfa, lc.dead_byte, nd.rows, 2, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st);
    else
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.dfa, lc.dead_byte, nd.rows, 2, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, w.bitmap_m,
                          w.tile_counts_m, w.reject_bits, w.tile_rejects);
    FZB_PEV(3);
    FZB_STAGE("filter(lcs)");
    fzb_launch_compact1(w.bitmap, w.tile_counts, p.cnt, nullptr, nullptr, w.surv_idx, &cnt_c[0], p.cus * 4, p.st);
    if (!single_chunk) {
        fzb_launch_compact1(w.bitmap_m, w.tile_counts_m, p.cnt, nullptr, nullptr, w.marg_list, &cnt_c[5], p.cus * 4, p.st);
        FZB_STAGE("compact1 x2");
        fzb_launch_window(p.cd, p.first, w.marg_list, &cnt_c[5], nd, lc.pf_lanes, nullptr, nullptr, nullptr, cnt_c, p.cus * 4, p.st, &rej);
        FZB_STAGE("window(decide)");
        fzb_launch_scan_rejects(w.tile_rejects, ntiles, &cnt_c[6], w.rej_prefix, p.st);
    }
    FZB_PEV(4);
    fzb_launch_dp(p.cd, p.first, p.index_offset, w.surv_idx, nullptr, &cnt_c[0], nd, lc.sw_lanes, 2, 3, lc.pad_ok, p.out, p.cap32, p.dev_count, w.overflow, p.cnt, cnt_c, p.cus, p.st, &rej);
    FZB_STAGE("dp(short, typo windows)");
    return FZB_OK;
}

// Filter stage of every other fuzzy query: streaming filter (or its item-list form) -> compaction [-> lane-exact window kernel -> second
// compaction when the stream stage was a superset].  Leaves p.items / p.win / p.n_items_ptr / p.wmode for the scorers.
static bool ascii_split_classes(const fzb_matcher* m, const CorpusDev& cd);
static u32 pipe_qcap(const Pipe& p);
static int g_debug_filter_grid = 0;  // fzb_debug_set_filter_grid
// The two-launch form (the filter lists its survivors, k2b_dp_short reads the segmented list): a contiguous range, k1_dfa_sig as the filter,
// k2b_dp_short with inline windows as the scorer (pipe_score_ascii's choice, restated), no matched positions, FZB_NO_SEG_LIST unset.
static bool pipe_seg_applies(const Pipe& p) {
    const fzb_matcher* m = p.m;
    const LaunchCfg& lc = m->lc;
    return !p.items_in && !p.trace && !fzb_knobs().no_seg_list && !m->nd.unicode && m->sig_eligible && lc.filter_mode == 1 && lc.filter_exact && lc.window_mode == 1 && lc.cf_ok &&
           fzb_filter_sig_applies(p.cd, 1, m->needle_sig, 1) && fzb_dp_short_applies(p.cd, lc.sw_lanes, 2);
}
static int pipe_filter_stage(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const LaunchCfg& lc = m->lc;
    const NeedleDev& nd = m->nd;
    u32* cnt_c = w.counters;
    p.n_items_ptr = &cnt_c[0];
    p.wmode = lc.window_mode;
    const int need = nd.rows - (nd.max_typos > 0 ? nd.max_typos : 0);
    int exact_wmode = 0;  // != 0: a unicode automaton decided exactly in the stream - no lane-exact window pass, the scorer computes the window (mode 1: 0 typos, 3: typos)
    // unicode typo query over a list whose haystacks all fit ONE prefilter chunk: the scalar-level LCS automaton IS the reference's decision
    // (build_scalar_lcs_dfa); longer lists keep it as the (tight) superset in front of the lane-exact window kernel
    const bool uni_typo_exact = nd.unicode && lc.filter_mode == 2 && m->lcs_scalar && m->lcs_states && lc.bias_ok && !p.trace && !fzb_knobs().typo_exact_window && p.cd.max_len != 0 &&
                                p.cd.max_len <= (u32)lc.pf_lanes;
    if (p.items_in) {
        if (lc.filter_mode == 0) {
            HIPCHK(hipMemcpyAsync(&cnt_c[0], p.n_items_in, 4, hipMemcpyDeviceToDevice, p.st));
            p.items = p.items_in;
        } else {
            // (a candidate set's list, fuzzy ASCII 0 typos: k1_items_dfa - the contiguous path's automaton - from the measured size on)
            fzb_launch_filter_items(p.cd, p.first, p.items_in, p.n_items_in, w.table, nd.rows, lc.filter_mode, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, p.cus * 4, p.st,
                                    nd.unicode ? nullptr : w.dfa, lc.filter_exact, m->needle_sig, m->sig_eligible, p.items_hint);
            FZB_STAGE("filter(items)");
            fzb_launch_compact1(w.bitmap, w.tile_counts, 0, p.n_items_in, p.items_in, w.surv_idx, &cnt_c[0], p.cus * 2, p.st);
            FZB_STAGE("compact1(items)");
            p.items = w.surv_idx;
        }
    } else if (lc.filter_mode == 0) {
        // nothing filtered (max_typos = None or >= rows): the survivors are the identity list (counters[0] = the range's size: set by the caller)
    } else if (m->uni_dfa_states && lc.bias_ok && !p.trace) {
        // unicode path, 0 typos: the exact prefilter as a byte-level DFA in the streaming filter; the scorer finds the window itself
        FZB_PEV(2);
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.uni_dfa, lc.dead_byte, m->uni_dfa_states - 1, 1, 0, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, nullptr,
                          nullptr, nullptr, nullptr, lc.pad_ok, -1, m->cdfa_src == 2 ? w.cdfa : nullptr, (u32)m->cdfa.size(), m->cdfa_K, m->cdfa_G);
        FZB_PEV(3);
        FZB_STAGE("filter(unicode dfa)");
        fzb_launch_compact1(w.bitmap, w.tile_counts, p.cnt, nullptr, nullptr, w.surv_idx, &cnt_c[0], p.cus * 4, p.st, &cnt_c[1]);  // (kept by the exact prefilter = the filter's survivors)
        FZB_STAGE("compact1");
        p.items = w.surv_idx;
        exact_wmode = 1;
    } else if (pipe_seg_applies(p)) {
        // 0-typo ASCII query over a short list with signatures, scored by k2b_dp_short: the filter lists the survivors of each workgroup's run of
        // tiles itself and the scorer reads that segmented list (seg_list.h) - two launches, no k_compact1
        const u32 ntiles = (p.cnt + FZB_TILE - 1) / FZB_TILE;
        u32 grid = std::min<u32>(std::min<u32>((u32)p.cus * 8u, FZB_SEG_MAX), ntiles);
        if (g_debug_filter_grid > 0) grid = std::min<u32>(grid, (u32)g_debug_filter_grid);
        grid = std::max<u32>(grid, 1u);
        const u32 stride = tc_tiles_per_run(ntiles, grid) * FZB_TILE;
        if ((size_t)ntiles * FZB_TILE > w.cap_items) return fail(FZB_ERR_INVALID, "internal: the survivor list does not hold the range rounded up to a tile");
        p.seg = SegList{w.surv_idx, w.seg_counts, grid, stride, &cnt_c[0]};
        p.segmented = true;
        FZB_PEV(2);
        fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.dfa, lc.dead_byte, nd.rows, 1, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, (int)grid, p.st, nullptr, nullptr,
                          nullptr, nullptr, lc.pad_ok, -1, nullptr, 0, 0, 0, m->needle_sig, 1, &p.seg, m->needle_sig2);
        FZB_PEV(3);
        FZB_STAGE("filter(lists its survivors)");
        p.items = w.surv_idx;
    } else {
        FZB_PEV(2);
        if (lc.filter_mode == 2 && m->lcs_states)  // typo configurations: the LCS automaton in the streaming DFA kernels (short and ragged lists)
            fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.lcs_dfa, lc.dead_byte, m->lcs_states - 1, 1, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, nullptr,
                              nullptr, nullptr, nullptr, lc.pad_ok, m->lcs_acc_lo, m->cdfa_src == 3 ? w.cdfa : nullptr, (u32)m->cdfa.size(), m->cdfa_K, m->cdfa_G);
        else
            fzb_launch_filter(p.cd, p.first, p.cnt, w.table, w.dfa, lc.dead_byte, nd.rows, lc.filter_mode, need, (u32)nd.min_haystack_len, w.bitmap, w.tile_counts, w.counters, p.cus * 8, p.st, nullptr, nullptr,
                              nullptr, nullptr, lc.pad_ok, -1, (lc.filter_mode == 1 && m->cdfa_src == 1) ? w.cdfa : nullptr, (u32)m->cdfa.size(), m->cdfa_K, m->cdfa_G, m->needle_sig,
                              m->sig_eligible && lc.filter_mode == 1);  // (eligible needle + a list with signatures: k1_dfa_sig)
        FZB_PEV(3);
        FZB_STAGE("filter");
        // ragged ASCII list, exact filter (0 typos) or whole-haystack windows: compaction and classification in ONE launch (k_compact1's grid: its
        // workgroups classify the survivors they have just listed).  Step, us, two launches -> one (profiles/r06_fused_classify.txt): lists of 100 k /
        // 300 k paths 34.7 -> 27.7 / 41.1 -> 36.1, 1.4 M paths 89.0 -> 86.5, the C4 shard 384 -> 384 (2, 3 or 4 workgroups per CU alike; 8 per CU
        // lose 10 us on the two large lists: more workgroups than are resident at once, and each is a chain of dependent round trips)
        // ... for lists of up to two tiles per CU (~ 0.5 M items: where a launch is a fifth of the query).  Beyond, the fused form gains nothing (above) and has a
        // failure mode the two-launch form does not: a workgroup classifies what ITS tiles hold, so survivors that cluster in a few tiles - every file below
        // one directory - are classified by a few workgroups, round after round (12.5 M items, all survivors in one stretch: 16 rounds in 52 workgroups),
        // whereas k2w_classify spreads any survivor list evenly.  On a small list the worst case is two rounds.
        const bool fuse = !nd.unicode && !p.trace && lc.filter_exact && !uni_typo_exact && (p.wmode == 1 || p.wmode == 2) && !fzb_knobs().no_fused_classify && w.cls_win && w.cls_lists &&
                          p.cnt <= (u32)p.cus * 2u * FZB_TILE && ascii_split_classes(m, p.cd);
        if (fuse) {
            fzb_launch_compact1_classify(p.cd, p.first, w.bitmap, w.tile_counts, p.cnt, w.surv_idx, &cnt_c[0], nd, lc.sw_lanes, p.wmode, p.cap32, p.dev_count, w.overflow, pipe_qcap(p), cnt_c,
                                         w.cls_win, w.cls_lists, (u32)w.cap_cls, p.cus * 4, p.st, 1);
            p.classified = true;
            FZB_STAGE("compact1 + classify");
        } else {
            fzb_launch_compact1(w.bitmap, w.tile_counts, p.cnt, nullptr, nullptr, w.surv_idx, &cnt_c[0], p.cus * 4, p.st, uni_typo_exact ? &cnt_c[1] : nullptr);
            FZB_STAGE("compact1");
        }
        p.items = w.surv_idx;
        if (uni_typo_exact) exact_wmode = 3;
    }
    if (exact_wmode) {
        p.wmode = exact_wmode;
    } else if (!lc.filter_exact) {
        // the stream stage was a superset: re-decide every survivor with the reference's chunked algorithm at its exact lane width
        fzb_launch_window(p.cd, p.first, p.items, &cnt_c[0], nd, lc.pf_lanes, w.win, w.bitmap2, w.tile_counts2, cnt_c, p.cus * 4, p.st, nullptr, p.items_in ? 0u : p.cnt);
        FZB_STAGE("window");
        fzb_launch_compact2(w.bitmap2, w.tile_counts2, &cnt_c[0], p.items, w.win, w.items2, w.win2, &cnt_c[1], p.cus * 2, p.st);
        FZB_STAGE("compact2");
        p.items = w.items2;
        p.win = w.win2;
        p.n_items_ptr = &cnt_c[1];
        p.wmode = 0;
    }
    return FZB_OK;
}

// The queue of windows wider than one chunk: multi-chunk entries from the front, generic-kernel entries from the back.  Every item is queued at
// most once by its scorer (front + back <= cnt), and the thread-per-haystack unicode scorer may hand up to FZB_UNICODE_FWD_CAP of the front's
// windows on to the back WHILE the front is still being read: the back gets that many entries of room of its own below the front's reach
// (ensure_workspace: the allocation holds at least count + FZB_UNICODE_FWD_CAP entries)
// Ragged ASCII list whose scorers are ONE launch over the classifier's lists (k2_classes_all: single-chunk classes + multi-chunk windows by the
// width of their last chunk's tail): classified scoring, windows wider than a chunk possible, dp_cfm.h's form for them
static bool ascii_split_classes(const fzb_matcher* m, const CorpusDev& cd) {
    const LaunchCfg& lc = m->lc;
    const FzbKnobs& kn = fzb_knobs();
    const bool no_wide = cd.max_len != 0 && cd.max_len <= (u32)lc.sw_lanes;
    const bool classes = lc.cf_ok && !kn.no_dp_classes && !fzb_dp_short_applies(cd, lc.sw_lanes, 2);
    return classes && !no_wide && lc.cfm_ok && !kn.no_dp_cfm;
}
static u32 pipe_qcap(const Pipe& p) { return (u32)std::min<u64>((u64)p.cnt + FZB_UNICODE_FWD_CAP, 0xFFFFFFFFull); }

// matched indices: one traced generic scorer for every window width, ASCII and unicode (kernels_generic.hip); its grid for `cnt` items and
// its per-wave matrices (grown here on first use, or ahead of it by fzb_matcher_reserve_top_indices)
static int traced_grid(int cus, size_t cnt) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)cus / 2, (cnt + 3) / 4)); }
static int ensure_trace_cells(fzb_matcher* m, size_t words) { return fzb_grow_dev(&m->ws.trace_cells, &m->ws.trace_cells_words, words); }
static int pipe_score_traced(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const int tgrid = traced_grid(p.cus, p.cnt);
    if (int rc = ensure_trace_cells(m, fzb_trace_scratch_words(m->nd, tgrid))) return rc;
    fzb_launch_generic_trace(p.cd, p.first, p.index_offset, p.items, p.win, p.wmode, p.n_items_ptr, m->nd, m->lc.sw_lanes, m->nd.unicode, p.out, p.cap32, p.dev_count, w.counters, w.trace_cells,
                             p.trace->pos, p.trace->npos, p.trace->stride, tgrid, p.st);
    FZB_STAGE("generic(trace)");
    return FZB_OK;
}

// Unicode scorers.  Single-chunk windows: k2u_dp_unicode (thread per haystack).  Windows wider than a chunk: up to 1024 bytes into the FRONT of the
// queue, beyond that (greedy fallback) into its back.  The front has two takers, chosen on the device by its length: the thread-per-haystack
// multi-chunk scorer (k2u_dp_unicode_multi: several times fewer instructions, but one wave per SIMD and ~ 10-20 us per chunk - a fixed latency of
// ~ 100 us, then 0.3 ns per window) from `umin` windows on, the wave-per-haystack kernel (1.6 - 2.7 ns per window, no fixed cost) below
// (45 k windows 0.215 ms wave per haystack / 0.204 thread per haystack, 361 k windows 1.285 / 0.815).  FZB_UNICODE_MULTI=0 / 1: never / always.
static int pipe_score_unicode(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const LaunchCfg& lc = m->lc;
    const NeedleDev& nd = m->nd;
    const FzbKnobs& kn = fzb_knobs();
    const CorpusDev& cd = p.cd;
    u32* cnt_c = w.counters;
    const int cus = p.cus;
    const u32 qcap = pipe_qcap(p);
    const bool no_wide = cd.max_len != 0 && cd.max_len <= (u32)lc.sw_lanes;  // no haystack is longer than a chunk
    int rc;
    // (a range smaller than the switch point cannot queue that many windows: the thread-per-haystack scorer is not even launched)
    const u32 umin = no_wide ? 0xFFFFFFFFu : kn.unicode_multi == 0 ? 0xFFFFFFFFu : kn.unicode_multi == 1 ? 0u : p.cnt < (u32)cus * 128u ? 0xFFFFFFFFu : (u32)cus * 128u;
    const int ugrid = cus * 2;  // multi-chunk unicode scorer: one wave per SIMD (two-wave workgroups)
    if (umin != 0xFFFFFFFFu && (rc = ensure_dp_scratch(m, ugrid))) return rc;  // first use only (or fzb_matcher_reserve)
    // Whole-haystack windows (max_typos: None): the wide ones are known from the end offsets, so they are queued FIRST and their scorers run
    // on the second stream beside the single-chunk scorer (Arabic-shaped list, All Scores: the two took 90 + 100 us one after the other)
    bool presplit = p.wmode == 2 && !p.items && !no_wide && !kn.debug_sync;  // (no item list: the number of windows is the range's size)
    if (presplit && ensure_aux_stream(m) != FZB_OK) {  // no second stream: the scorer queues them itself (the error text is dropped with the fallback)
        presplit = false;
        fzb_clear_error();
    }
    hipStream_t wst = p.st;  // the stream of the wide windows' scorers
    if (presplit) {
        fzb_launch_unicode_split_wide(cd, p.first, p.items, p.n_items_ptr, lc.sw_lanes, p.cap32, w.overflow, qcap, cnt_c, (int)std::min<u32>((p.cnt + 2047u) / 2048u, (u32)cus * 4u), p.st);
        HIPCHK(hipEventRecord(m->ev_fork, p.st));
        HIPCHK(hipStreamWaitEvent(m->aux_stream, m->ev_fork, 0));
        wst = m->aux_stream;
    }
    // (presplit: the wide windows' kernels are enqueued FIRST - a few hundred long-running waves that take their SIMDs and keep them - and the
    // single-chunk scorer runs as one short-lived workgroup per 128 items, which fills the rest of the chip and every SIMD a wide wave frees)
    auto launch_single = [&]() {
        fzb_launch_dp_unicode(cd, p.first, p.index_offset, p.items, p.win, p.n_items_ptr, nd, lc.sw_lanes, p.wmode, p.out, p.cap32, p.dev_count, w.overflow, qcap, cnt_c, cus, p.st, lc.cfu_ok,
                              presplit ? 2 : 1, presplit ? (int)((p.cnt + 127) / 128) : 0);
    };
    if (!presplit) launch_single();
    FZB_STAGE("dp(unicode)");
    if (no_wide) return FZB_OK;
    // (the thread-per-haystack scorer hands windows beyond four chunks - up to FZB_UNICODE_FWD_CAP of them - on to the queue's back)
    const u32 fwd_cap = umin != 0xFFFFFFFFu ? FZB_UNICODE_FWD_CAP : 0u;
    if (umin != 0xFFFFFFFFu)
        fzb_launch_dp_unicode_multi(cd, p.first, p.index_offset, w.overflow, &cnt_c[3], nd, lc.sw_lanes, p.out, p.cap32, w.dp_scratch, ugrid, wst, umin, lc.cfu_ok, cnt_c, w.overflow + 4 * (size_t)qcap, fwd_cap);
    // The queue's back - handed-on stragglers (DP) and windows beyond 1024 bytes (greedy) - has a launch of its own only where windows beyond
    // 1024 bytes can exist; otherwise the front's wave-per-haystack launch (12 workgroups per CU: its LDS follows the needle's rows, so its
    // registers decide the occupancy), which has nothing to do exactly when the thread-per-haystack scorer ran, walks the back then
    const bool back_launch = !(cd.max_len != 0 && cd.max_len <= FZB_MAX_HAYSTACK_LEN);
    const bool may_fwd = fwd_cap != 0 && !(cd.max_len != 0 && cd.max_len <= 4u * (u32)lc.sw_lanes);
    if (umin != 0u)
        fzb_launch_generic(cd, p.first, p.index_offset, p.items, p.win, p.wmode, w.overflow, &cnt_c[3], nd, lc.sw_lanes, 1, p.out, p.cap32, nullptr, cnt_c, cus * 12, wst, 1, umin,
                           (may_fwd && !back_launch) ? w.overflow + 4 * (size_t)qcap : nullptr, &cnt_c[4]);
    FZB_STAGE("dp(unicode, wide windows)");
    if (back_launch || (may_fwd && umin == 0u)) {
        fzb_launch_generic(cd, p.first, p.index_offset, p.items, p.win, p.wmode, w.overflow + 4 * (size_t)qcap, &cnt_c[4], nd, lc.sw_lanes, 1, p.out, p.cap32, nullptr, cnt_c,
                           may_fwd ? cus * 4 : cus / 4 + 1, wst);
        FZB_STAGE("generic(unicode, stragglers + greedy)");
    }
    if (presplit) {
        launch_single();
        HIPCHK(hipEventRecord(m->ev_join, m->aux_stream));
        HIPCHK(hipStreamWaitEvent(p.st, m->ev_join, 0));
    }
    return FZB_OK;
}

// ASCII scorers.  Lists whose haystacks fit half a chunk: k2b_dp_short (inside fzb_launch_dp).  Ragged lists under dp_cf.h's preconditions:
// k2w_classify finds window and class per survivor, then ONE launch (k2_classes_all) scores the three single-chunk classes and the
// multi-chunk windows by the width of their last chunk's tail (DESIGN.md "Scorers of a ragged list").  Scorings outside dp_cfm.h's preconditions
// keep the classes but send multi-chunk windows through the queue (k2d_dp_multi on the second stream beside the class launches); scorings
// outside dp_cf.h's run the per-wave form k2b_dp.  Windows beyond 1024 bytes: the greedy fallback in the wave-per-haystack kernel.
static int pipe_score_ascii(Pipe& p) {
    fzb_matcher* m = p.m;
    Workspace& w = m->ws;
    const LaunchCfg& lc = m->lc;
    const NeedleDev& nd = m->nd;
    const FzbKnobs& kn = fzb_knobs();
    const CorpusDev& cd = p.cd;
    u32* cnt_c = w.counters;
    const int cus = p.cus;
    const u32 qcap = pipe_qcap(p);
    const bool no_wide = cd.max_len != 0 && cd.max_len <= (u32)lc.sw_lanes;  // no haystack is longer than a chunk
    int rc;
    const bool classes = lc.cf_ok && !kn.no_dp_classes && !fzb_dp_short_applies(cd, lc.sw_lanes, 2);
    const int mgrid = cus * 4;  // multi-chunk scorer: 2 waves per SIMD (the kernel is capped at 256 VGPRs)
    const int mmode = (lc.cfm_ok && !kn.no_dp_cfm) ? 2 : lc.bias_ok ? 1 : 0;
    if (!no_wide && (rc = ensure_dp_scratch(m, mgrid))) return rc;  // first use only (or fzb_matcher_reserve)
    const int split = classes && !no_wide && mmode == 2;  // multi-chunk windows as k2w_classify's tail-class lists (needs dp_cfm.h's form; cf_ok includes pad_ok) == ascii_split_classes()
    if (p.classified && !split) return fail(FZB_ERR_INVALID, "internal: the compaction classified a list whose scorers do not take class lists");
    if (p.segmented && (classes || !lc.cf_ok || !fzb_dp_short_applies(cd, lc.sw_lanes, 2))) return fail(FZB_ERR_INVALID, "internal: a segmented survivor list in front of a scorer that reads a dense one");
    bool fork = classes && !no_wide && !split;
    if (fork && ensure_aux_stream(m) != FZB_OK) {  // no second stream: everything on the caller's stream (the error text is dropped with the fallback)
        fork = false;
        fzb_clear_error();
    }
    if (split) {
        if (!p.classified)
            fzb_launch_dp_classes(cd, p.first, p.index_offset, p.items, p.win, p.n_items_ptr, nd, lc.sw_lanes, p.wmode, p.out, p.cap32, p.dev_count, w.overflow, qcap, cnt_c, w.cls_win, w.cls_lists,
                                  (u32)w.cap_cls, cus, p.st, 1, split);
        fzb_launch_classes_all(cd, p.first, p.index_offset, p.items, w.cls_win, w.cls_lists, (u32)w.cap_cls, cnt_c, nd, lc.sw_lanes, p.out, p.cap32, w.dp_scratch, mgrid, cus, p.st);
    } else if (classes)
        fzb_launch_dp_classes(cd, p.first, p.index_offset, p.items, p.win, p.n_items_ptr, nd, lc.sw_lanes, p.wmode, p.out, p.cap32, p.dev_count, w.overflow, qcap, cnt_c, w.cls_win, w.cls_lists,
                              (u32)w.cap_cls, cus, p.st, fork ? 1 : 0, 0);
    else
        fzb_launch_dp(cd, p.first, p.index_offset, p.items, p.win, p.n_items_ptr, nd, lc.sw_lanes, lc.cf_ok ? 2 : lc.bias_ok ? 1 : 0, p.wmode, lc.pad_ok, p.out, p.cap32, p.dev_count, w.overflow, qcap, cnt_c, cus, p.st,
                      nullptr, p.segmented ? &p.seg : nullptr);
    FZB_STAGE("dp");
    if (fork) {  // the queued multi-chunk windows on the second stream beside the three class launches (both start from the classifier's output, disjoint records)
        HIPCHK(hipEventRecord(m->ev_fork, p.st));
        HIPCHK(hipStreamWaitEvent(m->aux_stream, m->ev_fork, 0));
        fzb_launch_dp_multi(cd, p.first, p.index_offset, w.overflow, &cnt_c[3], nd, lc.sw_lanes, mmode, p.out, p.cap32, w.dp_scratch, mgrid, m->aux_stream);
        HIPCHK(hipEventRecord(m->ev_join, m->aux_stream));
        fzb_launch_dp_classes(cd, p.first, p.index_offset, p.items, p.win, p.n_items_ptr, nd, lc.sw_lanes, p.wmode, p.out, p.cap32, p.dev_count, w.overflow, qcap, cnt_c, w.cls_win, w.cls_lists,
                              (u32)w.cap_cls, cus, p.st, 2, 0);
        HIPCHK(hipStreamWaitEvent(p.st, m->ev_join, 0));
        FZB_STAGE("dp classes + dp_multi (second stream)");
    }
    if (no_wide) return FZB_OK;
    if (!fork && !split) {
        fzb_launch_dp_multi(cd, p.first, p.index_offset, w.overflow, &cnt_c[3], nd, lc.sw_lanes, mmode, p.out, p.cap32, w.dp_scratch, mgrid, p.st);
        FZB_STAGE("dp_multi");
    }
    if (!(cd.max_len != 0 && cd.max_len <= FZB_MAX_HAYSTACK_LEN)) {  // > 1024-byte windows: the greedy fallback
        fzb_launch_generic(cd, p.first, p.index_offset, p.items, p.win, p.wmode, w.overflow + 4 * (size_t)qcap, &cnt_c[4], nd, lc.sw_lanes, 0, p.out, p.cap32, nullptr, cnt_c, cus / 4 + 1, p.st);
        FZB_STAGE("generic(greedy)");
    }
    return FZB_OK;
}

// events of a profiled call: [0] start, [2]..[3] around the streaming filter, [4] before the scorers, [1] end
static int pipe_profile_begin(fzb_matcher* m, bool has_filter, hipStream_t st, hipEvent_t** pev) {
    *pev = nullptr;
    if (!m->profiling) return FZB_OK;
    const int slot = (int)(m->prof_calls % fzb_matcher::PROF_SLOTS);
    hipEvent_t* ev = m->evring[slot];
    m->ev_filter[slot] = has_filter ? 1 : 0;
    m->prof_calls++;
    for (int i = 0; i < 5; i++)
        if (!ev[i]) HIPCHK(hipEventCreate(&ev[i]));
    HIPCHK(hipEventRecord(ev[0], st));
    *pev = ev;
    return FZB_OK;
}

// The pipeline.  items_in == nullptr: the haystacks are the contiguous range [first, first + count).  Otherwise they are the listed ones,
// items_in[j] = index relative to `first`, *n_items_in of them (a device-side count <= count): the narrowing step of the multi-pattern
// composition.  `trace` != nullptr: the matched-indices form - every record also gets its matched byte positions (the traced generic scorer
// replaces the fast scorers; literal modes write the needle run).
static int run_pipeline(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, const u32* items_in, const u32* n_items_in,
                        fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream, const TraceOut* trace = nullptr, u64 items_hint = 0) {
    if (!m || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    // an item list may repeat haystacks, so only the contiguous form bounds `count` by the corpus
    if (first > c->dev.n || (!items_in && count > c->dev.n - first)) return fail(FZB_ERR_INVALID, "range outside the corpus");
    // guard_against_haystack_overflow (src/matcher/mod.rs:438-446)
    if ((u64)count + (u64)index_offset > 0xFFFFFFFFull) return refuse_index_overflow((u64)count + index_offset, index_offset);
    if (m->empty) return fail(FZB_ERR_INVALID, "empty needle: handled on the host by fzb_match_list / fzb_match_list_into");
    hipStream_t st = (hipStream_t)stream;
    int rc = fzb_bind_device(m);
    if (rc) return rc;
    rc = ensure_workspace(m, count, st, true);
    if (rc) return rc;
    Workspace& w = m->ws;
    const LaunchCfg& lc = m->lc;
    const u32 cap32 = (u32)std::min<size_t>(capacity, 0xFFFFFFFFu);
    // the streaming filter kernels clear the counter block themselves (one launch less on the hot path)
    const bool filter_resets = count != 0 && !items_in && !m->long_needle && (m->literal_mode ? (m->literal_mode == FZB_MATCH_SUBSTRING && !m->nd.unicode) : lc.filter_mode != 0);
    // nothing filtered (max_typos = None or >= rows): the survivors are the identity list - the counter block is cleared and its first word set
    // to the range's size by ONE small kernel (a memset and a 32-bit fill were two fill kernels with a dispatch gap each: ~ 20 us of a step)
    const bool identity_list = count != 0 && !items_in && !m->long_needle && !m->literal_mode && lc.filter_mode == 0;
    if (identity_list) fzb_launch_init_counters(w.counters, (u32)count, st);
    else if (!filter_resets) HIPCHK(hipMemsetAsync(w.counters, 0, 64, st));
    if (count == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, st));
        return FZB_OK;
    }
    if (m->long_needle) return run_pipeline_long(m, c, first, count, index_offset, items_in, n_items_in, dev_out, cap32, dev_count, st, trace);
    Pipe p{m, c->dev, first, (u32)count, index_offset, items_in, n_items_in, (fzb_match_rec*)dev_out, cap32, dev_count, st, trace, nullptr, lc.num_cus, items_in ? items_hint : 0};
    if (m->literal_mode) return pipe_literal(p);
    if ((rc = pipe_profile_begin(m, lc.filter_mode && !items_in, st, &p.pev))) return rc;
    if (!items_in && lc.filter_mode != 0 && typo_fast_path_configured(m) && !trace && fzb_dp_short_applies(c->dev, lc.sw_lanes, 2)) {
        rc = pipe_typo_fast_path(p);
    } else {
        if ((rc = pipe_filter_stage(p))) return rc;
        FZB_PEV(4);
        if (trace) rc = pipe_score_traced(p);
        else if (m->nd.unicode && lc.bias_ok) rc = pipe_score_unicode(p);
        else if (m->nd.unicode) {
            fzb_launch_generic(c->dev, first, index_offset, p.items, p.win, p.wmode, nullptr, p.n_items_ptr, m->nd, lc.sw_lanes, 1, p.out, cap32, dev_count, w.counters, lc.num_cus * 4, st);
            FZB_STAGE("generic(unicode)");
        } else rc = pipe_score_ascii(p);
    }
    if (rc) return rc;
    FZB_PEV(1);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
#undef FZB_STAGE
#undef FZB_PEV

// Sizes every device buffer a query over `c` can need (range workspace incl. the typo-path arrays, multi-chunk scorer scratch when
// the corpus has haystacks wider than a chunk, staging + sort buffers of the synchronous / sorted entry points), so that the queries
// that follow - also after fzb_matcher_set_pattern / fzb_matcher_set_config, which keep the workspace - never allocate.
// (Matched-indices queries size their trace scratch from the selection, on first use; fzb_matcher_reserve_top_indices sizes it - and the
// fused top + positions query's own buffers - ahead of that.)
int fzb_matcher_reserve(fzb_matcher* m, const fzb_corpus* c) {
    if (!m || !c) return fail(FZB_ERR_INVALID, "null argument");
    // (a corpus with room reserved: sized for that room, and for haystacks of any width - an append may bring them)
    const size_t n = fzb_corpus_reserved_items(c);
    if (n == 0) return FZB_OK;
    int rc = fzb_bind_device(m);
    if (rc) return rc;
    if (m->empty) {  // the empty prompt (prompt_records): flag words, the sort's buffers (the selection's input) and the staging - with or without a scope or a bias
        if ((rc = fzb_scope_ensure_flags(m->scope, n)) || (rc = fzb_ensure_out_staging(m, n)) || (rc = ensure_sort_buffers(m, n))) return rc;
        if (!m->fetch_top.count_host) HIPCHK(hipHostMalloc((void**)&m->fetch_top.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));
        if (!m->fetch.count_host) HIPCHK(hipHostMalloc((void**)&m->fetch.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));
        return FZB_OK;
    }
    rc = ensure_workspace(m, n);
    if (rc) return rc;
    // a corpus that carries tags: toggling its scope between queries allocates nothing; a facet sink: a _device form whose output is smaller than
    // the match set writes into the same scratch, so that the count stays exact
    if ((c->tags.data || m->facets) && (rc = fzb_scope_ensure(m->scope, n))) return rc;
    const bool no_wide = n == c->dev.n && c->dev.max_len != 0 && c->dev.max_len <= (u32)m->lc.sw_lanes;
    if (!m->long_needle && !m->literal_mode && !m->nd.unicode && !no_wide && ((rc = ensure_dp_scratch(m, m->lc.num_cus * 4)) || (rc = ensure_aux_stream(m)))) return rc;
    if (!m->long_needle && !m->literal_mode && m->nd.unicode && m->lc.bias_ok && !no_wide && fzb_knobs().unicode_multi != 0 && (rc = ensure_dp_scratch(m, m->lc.num_cus * 2))) return rc;
    if (!m->long_needle && !m->literal_mode && m->nd.unicode && m->lc.bias_ok && !no_wide && m->nd.max_typos < 0 && (rc = ensure_aux_stream(m))) return rc;  // whole-haystack windows: the wide ones on the second stream
    if ((rc = fzb_ensure_out_staging(m, n))) return rc;
    if ((rc = ensure_sort_buffers(m, n))) return rc;
    if (!m->fetch_top.count_host) HIPCHK(hipHostMalloc((void**)&m->fetch_top.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));  // (a top query's pinned count words)
    return FZB_OK;
}

}  // extern "C"
// fzb_matcher_reserve for a sub-matcher slot of a multi-pattern matcher, whose needle and matching form change with the keystrokes: the
// workspace of EVERY form (level-2 windows, margin pass, classified scorer, whatever the current needle needs), and the parked rows of the
// multi-chunk scorers for the largest short needle (1 .. FZB_MAX_ROWS rows, each at the lane width its score class gets under the slot's
// scoring and lanes; ASCII grid, the unicode scorer's is half of it).  Only a long needle (beyond 64 bytes / 63 rows) or another scoring /
// lane pair can make the slot grow later.  A slot never runs the synchronous entry points: no staging or sort buffers.
static int reserve_slot_any_needle(fzb_matcher* m, const fzb_corpus* c) {
    const size_t n = fzb_corpus_reserved_items(c);
    if (m->empty || n == 0) return FZB_OK;
    int rc = fzb_bind_device(m);
    if (rc) return rc;
    if ((rc = ensure_workspace(m, n, nullptr, false, true))) return rc;
    size_t words = 0;
    for (int r = 1; r <= FZB_MAX_ROWS; r++) {
        const bool u8 = fits_in_u8((size_t)r, m->config.scoring);  // (a unicode needle of r scalars has >= r bytes: never a wider class)
        int pf = m->config.pf_lanes, sw = m->config.sw_lanes;
        if (pf == 0 && sw == 0) detect_host_lanes(u8, pf, sw);
        else if (sw == 0) sw = u8 ? pf : pf / 2;
        const bool no_wide = n == c->dev.n && c->dev.max_len != 0 && c->dev.max_len <= (u32)sw;  // (no window beyond one chunk: the scratch is never used)
        if (!no_wide) words = std::max(words, dp_scratch_words(r, sw, m->lc.num_cus * 4));
    }
    if (words && (rc = ensure_dp_scratch_words(m, words))) return rc;
    return ensure_aux_stream(m);
}
extern "C" {

}  // extern "C"
// ---- candidate sets on the query path (fzb_subset; the handle's own calls are further down) ---------------------------------------------
// What a *_subset entry point hands down: `in` (null: the whole corpus) becomes the pipeline's item list, `capture` (null: none) receives the
// indices of the records the scorers wrote - BEFORE the list's terms, the selection and the ordering -, `mirror` (host forms) is a device word
// next to the result's count words that gets the captured count too, so that the form's one wait brings it back.
struct SubsetArgs {
    const fzb_subset* in = nullptr;
    fzb_subset* capture = nullptr;
    u32* mirror = nullptr;
};
static const u32* subset_items(const SubsetArgs* sa) { return sa && sa->in ? sa->in->idx : nullptr; }
static const u32* subset_count(const SubsetArgs* sa) { return sa && sa->in ? sa->in->count_dev : nullptr; }
// what the host knows of the input's length (the filter's choice of kernel and grid): the count when known, else the room it was captured into
static u64 subset_hint(const SubsetArgs* sa) { return sa && sa->in ? std::max<u64>(1, sa->in->known ? sa->in->count : (u64)sa->in->cap) : 0; }
// what every capture leaves on the handle: the count lives on the device until a host form's wait, or fzb_subset_info, brings it back
static void subset_captured(fzb_subset* cp, const fzb_corpus* c) {
    cp->generation = c->generation;
    cp->known = false;
}
// test and benchmark hook: 0 = the composition's final copy and the capture as two launches (k_copy_records, k_subset_capture), else fused
static int g_debug_fused_capture = 1;
// the ONE place that launches the capture of a producer's records (the composition's final copy does its own, fused: multi_compose_device):
// recs = the producer's index-ordered records (numbered from index_offset 0 over the whole corpus)
static int subset_capture(const SubsetArgs* sa, const fzb_corpus* c, const fzb_match_rec* recs, const u32* pair, size_t cap, int grid_max, hipStream_t st) {
    if (!sa || !sa->capture) return FZB_OK;
    fzb_subset* cp = sa->capture;
    fzb_launch_subset_capture(recs, pair, (u32)std::min<size_t>(cap, 0xFFFFFFFFu), 0, cp->idx, (u32)std::min<size_t>(cp->cap, 0xFFFFFFFFu), cp->count_dev, sa->mirror, grid_max, st);
    HIPCHK(hipGetLastError());
    subset_captured(cp, c);
    return FZB_OK;
}
extern "C" {
static int match_list_device_impl(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                                  void* stream, const SubsetArgs* sa) {
    int rc;
    fzb_facets* const fc = m ? m->facets : nullptr;
    if ((rc = facets_check(fc, c, "fzb_match_list_device"))) return rc;
    // (a facet sink counts every match: an output that may be too small for them must not cut the producer ahead of the count - the scratch
    // has room for one record per haystack of the range)
    const bool uncut = fc && capacity < count;
    if (m && c && count && (fzb_corpus_scoped(c) || uncut) && dev_count && (dev_out || !capacity)) {  // the pipeline into the scratch, then the list's terms: drop, then bias
        if ((rc = fzb_scope_ensure(m->scope, count))) return rc;
        if ((rc = run_pipeline(m, c, first, count, index_offset, subset_items(sa), subset_count(sa), (fzb_match*)m->scope.recs, count, m->scope.words, stream, nullptr, subset_hint(sa)))) return rc;
        if ((rc = subset_capture(sa, c, m->scope.recs, m->scope.words, count, m->lc.num_cus * 2, (hipStream_t)stream))) return rc;
        return apply_terms(c, m->scope, count, (fzb_match_rec*)dev_out, capacity, dev_count, first, index_offset, m->lc.num_cus * 2, (hipStream_t)stream, fc);
    }
    rc = run_pipeline(m, c, first, count, index_offset, subset_items(sa), subset_count(sa), dev_out, capacity, dev_count, stream, nullptr, subset_hint(sa));
    if (rc) return rc;
    if ((rc = subset_capture(sa, c, (const fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), m->lc.num_cus * 2, (hipStream_t)stream))) return rc;
    if ((rc = facets_records(fc, c, (const fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), first, index_offset, m->lc.num_cus * 2, (hipStream_t)stream))) return rc;
    return apply_bias(c, (fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), first, index_offset, m->lc.num_cus * 2, (hipStream_t)stream);
}
int fzb_match_list_device(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity,
                          uint32_t* dev_count, void* stream) {
    return match_list_device_impl(m, c, first, count, index_offset, dev_out, capacity, dev_count, stream, nullptr);
}

int fzb_match_list_sorted_device(fzb_matcher* m, const fzb_corpus* c, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream) {
    if (!m || !c) return fail(FZB_ERR_INVALID, "null argument");
    return fzb_sorted_range_device(m, c, 0, c->dev.n, 0, dev_out, capacity, dev_count, stream);
}

}  // extern "C"
// The ordered form over any sub-range, records numbered from index_offset: what one worker of `match_list_parallel` produces for its
// share (per-run reverse / radix sort, src/matcher/parallel.rs:66-76) - fzb_match_list_parallel_sharded runs one per device
static int sorted_range_impl(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                             void* stream, const SubsetArgs* sa);
int fzb_sorted_range_device(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                            void* stream) {
    return sorted_range_impl(m, c, first, count, index_offset, dev_out, capacity, dev_count, stream, nullptr);
}
// (sa: the candidate-set forms - the whole corpus from 0 - hand their item list and capture down to the pipeline's call)
static int sorted_range_impl(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity, uint32_t* dev_count,
                             void* stream, const SubsetArgs* sa) {
    if (!m || !c) return fail(FZB_ERR_INVALID, "null argument");
    if (first > c->dev.n || count > c->dev.n - first) return fail(FZB_ERR_INVALID, "range outside the corpus");
    const size_t cap = std::min<size_t>(capacity, count);
    OrderPlan plan;
    int rc;
    // (the range workspace first: growing it releases every workspace buffer, the sort's included)
    if (!m->empty && count != 0 && ((rc = fzb_bind_device(m)) || (rc = ensure_workspace(m, count, (hipStream_t)stream, true)))) return rc;
    if ((rc = fzb_order_begin(m, m->empty || count == 0 ? 0 : cap, (fzb_match_rec*)dev_out, &plan, fzb_corpus_bias_hi(c)))) return rc;
    // (the public call: the pipeline and, on a biased corpus, the bias pass over the index-ordered records - before anything orders them)
    rc = match_list_device_impl(m, c, first, count, index_offset, (fzb_match*)plan.in, plan.via_tmp ? cap : capacity, dev_count, stream, sa);
    if (rc) return rc;
    if (count == 0) return FZB_OK;
    return fzb_order_finish(m, plan, (fzb_match_rec*)dev_out, dev_count, (hipStream_t)stream);
}

// The ordering post-step of `match_list` (src/matcher/mod.rs:215-221: reverse for the *Desc strategies, radix_sort_matches for the Score*
// strategies) over index-ordered records that are, or are about to be, in device memory.  fzb_order_begin sizes the sort's buffers for
// `cap` records and says where the producer should write them (`plan.in`): with a single radix pass that is the sort's SECOND buffer and
// the pass scatters into the caller's array - no copy back.  fzb_order_finish launches reverse / sort on `stream`; the record count is
// read from device memory.  Producers: the pipeline (above), the concatenation of per-shard runs (host_shard.hip).
// What `match_list`'s post-step does for this matcher: the ONE place that decides it (fzb_order_begin and the top-`limit` selection both ask here - a
// `one_pass` that is wrongly true would make the selection read the low byte only)
// bias_hi: the upper bound of the corpus' largest positive score bias (fzb_corpus_bias_hi; 0 for callers without a corpus)
void fzb_order_flags(const fzb_matcher* m, u32 bias_hi, bool* reversed, bool* by_score, bool* one_pass) {
    const int sort = m->config.sort;
    *reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;          // src/matcher/mod.rs:215-217
    *by_score = sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;  // :218-220
    // one radix pass is enough when no score can reach 256 (score_ceiling: what the matrix can really hold, + the exact-match bonus added after it)
    // - nor, on a biased corpus, the largest positive bias on top of it (score_bias.h)
    *one_pass = !m->sum_scores && !m->literal_mode && sbias_one_pass(score_ceiling(m->config.scoring, (size_t)m->rows) + (size_t)m->config.scoring.exact_match_bonus, bias_hi);
}
int fzb_order_begin(fzb_matcher* m, size_t cap, fzb_match_rec* dev_out, OrderPlan* p, u32 bias_hi) {
    fzb_order_flags(m, bias_hi, &p->reversed, &p->by_score, &p->one_pass);
    p->via_tmp = p->by_score && p->one_pass && cap != 0;
    p->in = dev_out;
    if (p->by_score) {
        int rc = ensure_sort_buffers(m, cap);
        if (rc) return rc;
        if (p->via_tmp) p->in = m->ws.sort.tmp;
    }
    return FZB_OK;
}
int fzb_order_finish(fzb_matcher* m, const OrderPlan& p, fzb_match_rec* dev_out, const u32* dev_count, hipStream_t stream) {
    if (!p.reversed && !p.by_score) return FZB_OK;
    Workspace& w = m->ws;
    if (p.by_score && !w.sort.tmp) return fail(FZB_ERR_INVALID, "fzb_order_finish without fzb_order_begin");
    fzb_launch_sort(dev_out, w.sort.tmp, dev_count, w.sort.hist, (u32)(w.sort.cap / 2048 + 2), p.reversed, p.by_score, m->lc.num_cus * 2, stream, p.via_tmp ? -1 : p.one_pass ? 1 : 2);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
extern "C" {

// Result lists handed to the caller live in page-locked host memory so that the device-to-host copy of the records runs at
// DMA speed (a pageable destination is staged through bounce buffers: ~3x slower for a 4 MB list).  Pinning is expensive, so
// the buffers are pooled: fzb_matches_free returns a buffer to the pool and a steady stream of queries keeps reusing the same
// few.  Lists that never were on the device (empty needle) come from malloc; fzb_matches_free tells the two apart.
}  // extern "C"
namespace {
struct PinnedPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> live;             // handed out: pointer -> capacity in bytes
    std::vector<std::pair<void*, size_t>> free_list;    // ready for reuse
    static constexpr size_t kMaxFree = 32;  // result lists + the staging buffers of an upload (two per worker thread)
    void* get(size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        size_t best = free_list.size();
        for (size_t i = 0; i < free_list.size(); i++)
            if (free_list[i].second >= bytes && (best == free_list.size() || free_list[i].second < free_list[best].second)) best = i;
        void* p = nullptr;
        size_t cap = 0;
        if (best != free_list.size()) {
            p = free_list[best].first;
            cap = free_list[best].second;
            free_list.erase(free_list.begin() + best);
        } else {
            cap = std::max<size_t>(bytes + bytes / 4, (size_t)1 << 16);
            if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
        }
        live[p] = cap;
        return p;
    }
    bool put(void* p) {  // false: not one of ours
        std::lock_guard<std::mutex> g(mu);
        auto it = live.find(p);
        if (it == live.end()) return false;
        const size_t cap = it->second;
        live.erase(it);
        if (free_list.size() < kMaxFree) free_list.emplace_back(p, cap);
        else (void)hipHostFree(p);
        return true;
    }
};
PinnedPool& pinned_pool() {
    static PinnedPool* pool = new PinnedPool;  // never destroyed: the HIP runtime may already be gone at exit
    return *pool;
}
}  // namespace
// The wait of a synchronous entry point: a query's results arrive tens to hundreds of microseconds after the call, and a thread that went to sleep in
// hipStreamSynchronize wakes 10-20 us after the stream has drained; so the stream is POLLED first (hipStreamQuery, for at most FZB_SPIN_WAIT_US, default
// 1 ms - a cold 8 ms upload-and-query ends up blocking as before), then blocked on.
hipError_t fzb_stream_wait(hipStream_t st) {
    const int budget_us = fzb_knobs().spin_wait_us;
    if (budget_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(st);
            if (e != hipErrorNotReady) return e;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= budget_us) break;
            __builtin_ia32_pause();
        }
        (void)hipGetLastError();  // (hipErrorNotReady is not an error of the caller's)
    }
    return hipStreamSynchronize(st);
}
// (dev_words: eight u32 in device memory, all copied to h.count_host; the record count is word `n_word`)
int fzb_fetch_records(FetchHint& h, const void* dev_records, const u32* dev_words, int n_word, size_t capacity, hipStream_t st, fzb_match** out, size_t* out_len) {
    if (!h.count_host) HIPCHK(hipHostMalloc((void**)&h.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));
    // the guess: the previous result's size and a little more (every speculated record that does not exist is copied for nothing - a
    // quarter more cost 19 us on a 4 MB result, more than the synchronisation it saves); the buffer has room for half as many again, so a
    // result that outgrew the guess usually only needs its remainder copied
    const size_t guess = h.last ? std::min(capacity, h.last + h.last / 64 + 64) : 0;
    size_t room = std::min(capacity, guess + guess / 2);
    fzb_match* r = (fzb_match*)pinned_pool().get(std::max<size_t>(room, 1) * sizeof(fzb_match));
    if (!r) return fail(FZB_ERR_HIP, "hipHostMalloc failed for the result list");
    hipError_t e = hipMemcpyAsync(h.count_host, dev_words, OUT_FETCH_WORDS * sizeof(u32), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && guess) e = hipMemcpyAsync(r, dev_records, guess * sizeof(fzb_match), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = fzb_stream_wait(st);
    const size_t n = e == hipSuccess ? (size_t)h.count_host[n_word] : 0;
    if (e == hipSuccess && n > guess) {  // the result outgrew the guess (or there was none): the rest in a second copy
        size_t have = guess;
        if (n > room) {
            pinned_pool().put(r);
            r = (fzb_match*)pinned_pool().get(n * sizeof(fzb_match));
            if (!r) return fail(FZB_ERR_HIP, "hipHostMalloc failed for the result list");
            have = 0;
        }
        e = hipMemcpyAsync(r + have, (const fzb_match*)dev_records + have, (n - have) * sizeof(fzb_match), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = fzb_stream_wait(st);
    }
    if (e != hipSuccess) {
        pinned_pool().put(r);
        return fail(FZB_ERR_HIP, std::string("device to host: ") + hipGetErrorString(e));
    }
    h.last = n;
    *out = r;
    *out_len = n;
    return FZB_OK;
}
void* fzb_pinned_get(size_t bytes) { return pinned_pool().get(bytes); }
bool fzb_pinned_put(void* p) { return pinned_pool().put(p); }
namespace {
// The result of a query -> the host: the record count and the records, into a pooled pinned buffer.  The count is not known when the
// copies are enqueued, so the records are copied SPECULATIVELY - as many as the matcher's previous query returned plus a quarter - right
// behind the count, and one synchronisation serves both (a re-query of a resident list - the next keystroke - returns about as many
// matches as the last one, usually fewer); only a result that outgrew the guess costs the second copy that every query used to pay.
int fetch_records(FetchHint& h, const void* dev_records, const u32* dev_count, size_t capacity, fzb_match** out, size_t* out_len) {
    return fzb_fetch_records(h, dev_records, dev_count, 0, capacity, nullptr, out, out_len);
}
}  // namespace
extern "C" {

int fzb_match_list_into(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match** out, size_t* out_len) {
    if (!m || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    if (first > c->dev.n || count > c->dev.n - first) return fail(FZB_ERR_INVALID, "range outside the corpus");
    if ((u64)count + (u64)index_offset > 0xFFFFFFFFull) return refuse_index_overflow((u64)count + index_offset, index_offset);
    *out = nullptr;
    *out_len = 0;
    if (prompt_on_device(m, c, nullptr, count)) return prompt_list_host(m, c, nullptr, first, count, index_offset, false, out, out_len);  // the empty prompt, index order
    if (m->empty) {  // src/matcher/mod.rs:381-384
        if (int rc_ = facets_every(m->facets, c, first, count, "fzb_match_list_into")) return rc_;
        fzb_match* r = (fzb_match*)malloc(std::max<size_t>(count, 1) * sizeof(fzb_match));
        if (!r) return fail(FZB_ERR_INVALID, "out of memory");
        for (size_t i = 0; i < count; i++) r[i] = fzb_match{(uint32_t)(index_offset + i), 0, 0, 0};
        *out = r;
        *out_len = count;
        return FZB_OK;
    }
    if (int rc_ = fzb_ensure_out_staging(m, count)) return rc_;
    int rc = fzb_match_list_device(m, c, first, count, index_offset, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr);
    if (rc) return rc;
    return fetch_records(m->fetch, m->out_dev, m->count_dev, m->out_cap, out, out_len);
}

void fzb_radix_sort_matches(fzb_match* matches, size_t n) {  // src/sort.rs:6-40
    if (n < 2) return;
    std::vector<fzb_match> tmp(n);
    size_t hist[256];
    for (int pass = 0; pass < 2; pass++) {
        const int shift = pass * 8;
        fzb_match* src = pass == 0 ? matches : tmp.data();
        fzb_match* dst = pass == 0 ? tmp.data() : matches;
        memset(hist, 0, sizeof(hist));
        for (size_t i = 0; i < n; i++) hist[(src[i].score >> shift) & 0xFF]++;
        size_t off[256];
        size_t run = 0;
        for (int b = 255; b >= 0; b--) { off[b] = run; run += hist[b]; }  // descending buckets
        for (size_t i = 0; i < n; i++) dst[off[(src[i].score >> shift) & 0xFF]++] = src[i];
    }
}

int fzb_match_list(fzb_matcher* m, const fzb_corpus* c, fzb_match** out, size_t* out_len) {
    if (!m || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    const int sort = m->config.sort;
    if (prompt_on_device(m, c, nullptr, c->dev.n)) {  // the empty prompt: the visible haystacks, ordered by the bias
        *out = nullptr;
        *out_len = 0;
        return prompt_list_host(m, c, nullptr, 0, c->dev.n, 0, true, out, out_len);
    }
    if (m->empty) {  // CompiledPatterns::Empty: every index, score 0, reversed if the strategy says so, never sorted (mod.rs:215-220, 381-384)
        int rc = fzb_match_list_into(m, c, 0, c->dev.n, 0, out, out_len);
        if (rc) return rc;
        if (sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC) std::reverse(*out, *out + *out_len);
        return FZB_OK;
    }
    const size_t count = c->dev.n;
    *out = nullptr;
    *out_len = 0;
    if (int rc_ = fzb_ensure_out_staging(m, count)) return rc_;
    // scoring AND the reverse / stable radix sort post-step run on the device; the host only receives the final list
    int rc = fzb_match_list_sorted_device(m, c, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr);
    if (rc) return rc;
    return fetch_records(m->fetch, m->out_dev, m->count_dev, m->out_cap, out, out_len);
}

int fzb_match_list_parallel(fzb_matcher* m, const fzb_corpus* c, size_t threads, fzb_match** out, size_t* out_len) {
    if (!m || !c) return fail(FZB_ERR_INVALID, "null argument");
    if (threads == 0) return fail(FZB_ERR_PANIC, "threads must be positive");  // parallel.rs:24
    if (int rc_ = fzb_refuse_facets(m->facets, "fzb_match_list_parallel")) return rc_;
    return fzb_match_list(m, c, out, out_len);
}

// ---- matched indices: Matcher::match_list_indices (src/matcher/mod.rs:234-275) ------------------------------------------------
}  // extern "C"
namespace {
// The haystack list of the *_indices entry points: a selection of the corpus, or all of it.
int check_selection(const fzb_corpus* c, const uint32_t* selection, size_t n_selection, size_t& count, uint32_t index_offset = 0) {
    count = selection ? n_selection : (size_t)c->dev.n;
    if ((u64)count + (u64)index_offset > 0xFFFFFFFFull)  // guard_against_haystack_overflow(haystacks.len(), 0), mod.rs:235
        return refuse_index_overflow((u64)count + index_offset, index_offset);
    for (size_t i = 0; i < n_selection; i++)
        if (selection[i] >= c->dev.n) return fail(FZB_ERR_INVALID, "selection entry outside the corpus");
    return FZB_OK;
}

// The matched-indices scratch of a matcher: the item list (+ room for its length word behind `count` entries and at the buffer's end), the
// position counts, the positions (`stride` per record)
int ensure_trace_buffers(fzb_matcher* m, size_t count, size_t pos_words) {
    if (m->trace_cap >= count && m->trace_pos_words >= pos_words && m->trace_sel) return FZB_OK;
    count = std::max(count, m->trace_cap);  // (neither dimension shrinks: what a reserve sized for the longest needle stays)
    pos_words = std::max(pos_words, m->trace_pos_words);
    m->trace_cap = m->trace_pos_words = 0;
    int rc;
    if ((rc = fzb_dev_renew(&m->trace_sel, count + 4)) ||  // [count] = the list length
        (rc = fzb_dev_renew(&m->trace_npos, count)) || (rc = fzb_dev_renew(&m->trace_pos, pos_words)))
        return rc;
    m->trace_cap = count;
    m->trace_pos_words = pos_words;
    return FZB_OK;
}

// One pattern over the list, LIST order (match_list_indices_impl, algo.rs:196-227): recs[k].index = position in the list,
// its positions appended to `positions`.  An empty needle matches everything with no positions.
// biased: the corpus' score bias is added to the records (the single-pattern entry points; the multi composition sums its patterns' scores
// and must not pass it)
int indices_in_list_order(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t count, std::vector<fzb_match_indices>& recs, std::vector<u32>& positions,
                          bool biased = false) {
    recs.clear();
    biased = biased && fzb_corpus_bias(c);
    if (m->empty) {
        std::vector<int16_t> hb;
        if (biased)
            if (int rc_ = fetch_column(fzb_corpus_bias(c), 0, c->dev.n, hb)) return rc_;
        recs.resize(count);
        for (size_t i = 0; i < count; i++)
            recs[i] = fzb_match_indices{(uint32_t)i, (uint16_t)(biased ? sbias_clamp_add(0, hb[selection ? selection[i] : i]) : 0), 0, 0, (uint32_t)positions.size(), 0};
        return FZB_OK;
    }
    if (!count) return FZB_OK;
    const u32 stride = (u32)std::max(1, m->nd.nbytes);
    if (int rc_ = ensure_trace_buffers(m, count, count * (size_t)stride)) return rc_;
    if (int rc_ = fzb_ensure_out_staging(m, count)) return rc_;
    const u32* items_dev = nullptr;
    const u32* n_items_dev = nullptr;
    if (selection) {
        const u32 n32 = (u32)count;
        HIPCHK(hipMemcpy(m->trace_sel, selection, count * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m->trace_sel + count, &n32, 4, hipMemcpyHostToDevice));
        items_dev = m->trace_sel;
        n_items_dev = m->trace_sel + count;
    }
    const TraceOut tr{m->trace_pos, m->trace_npos, stride};
    int rc = run_pipeline(m, c, 0, count, 0, items_dev, n_items_dev, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr, &tr);
    if (rc) return rc;
    // (records carry the corpus index here - first 0, index_offset 0 - whether they come from a selection or the whole list)
    if (biased && (rc = apply_bias(c, m->out_dev, m->count_dev, std::min(m->out_cap, count), 0, 0, m->lc.num_cus * 2, nullptr))) return rc;
    u32 n = 0;
    HIPCHK(hipMemcpy(&n, m->count_dev, 4, hipMemcpyDeviceToHost));
    std::vector<fzb_match_rec> dev_recs(n);
    std::vector<u32> npos(n), pos((size_t)n * stride);
    if (n) {
        HIPCHK(hipMemcpy(dev_recs.data(), m->out_dev, (size_t)n * sizeof(fzb_match_rec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(npos.data(), m->trace_npos, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pos.data(), m->trace_pos, (size_t)n * stride * 4, hipMemcpyDeviceToHost));
    }
    recs.resize(n);
    size_t sel_at = 0;  // records come back in list order, so each one is the next selection entry that names its haystack
    for (u32 j = 0; j < n; j++) {
        u32 index = dev_recs[j].index;
        if (selection) {
            while (sel_at < count && selection[sel_at] != index) sel_at++;
            if (sel_at == count) return fail(FZB_ERR_HIP, "internal: record outside the selection");
            index = (u32)sel_at++;
        }
        const u32 len = std::min(npos[j], stride);
        recs[j] = fzb_match_indices{index, dev_recs[j].score, dev_recs[j].exact, 0, (uint32_t)positions.size(), len};
        positions.insert(positions.end(), pos.begin() + (size_t)j * stride, pos.begin() + (size_t)j * stride + len);
    }
    return FZB_OK;
}

// the ordering step (mod.rs:268-273) and the hand-over to the caller
int finish_indices(std::vector<fzb_match_indices>& recs, const std::vector<u32>& positions, int sort, bool sort_by_score, fzb_match_indices** out, size_t* out_len,
                   uint32_t** out_positions, uint32_t index_offset = 0) {
    if (index_offset)
        for (fzb_match_indices& r : recs) r.index += index_offset;
    const bool reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    const bool by_score = sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    if (reversed) std::reverse(recs.begin(), recs.end());
    if (by_score && sort_by_score)  // `sort_by_key(|m| Reverse(m.score))`: stable
        std::stable_sort(recs.begin(), recs.end(), [](const fzb_match_indices& a, const fzb_match_indices& b) { return a.score > b.score; });
    fzb_match_indices* r = (fzb_match_indices*)malloc(std::max<size_t>(recs.size(), 1) * sizeof(fzb_match_indices));
    u32* p = (u32*)malloc(std::max<size_t>(positions.size(), 1) * 4);
    if (!r || !p) {
        free(r);
        free(p);
        return fail(FZB_ERR_INVALID, "out of memory");
    }
    if (!recs.empty()) memcpy(r, recs.data(), recs.size() * sizeof(fzb_match_indices));
    if (!positions.empty()) memcpy(p, positions.data(), positions.size() * 4);
    *out = r;
    *out_len = recs.size();
    *out_positions = p;
    return FZB_OK;
}
}  // namespace
extern "C" {

static int match_list_indices_impl(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, int sort, uint32_t index_offset,
                                   fzb_match_indices** out, size_t* out_len, uint32_t** out_positions) {
    if (!m || !c || !out || !out_len || !out_positions || (!selection && n_selection)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    *out_positions = nullptr;
    size_t count = 0;
    int rc = check_selection(c, selection, n_selection, count, index_offset);
    if (rc) return rc;
    std::vector<fzb_match_indices> recs;
    std::vector<u32> positions;
    rc = indices_in_list_order(m, c, selection, count, recs, positions, true);
    if (rc) return rc;
    // CompiledPatterns::Empty returns before the score sort (mod.rs:237-246) - all scores are 0 anyway, unless the corpus carries a bias
    return finish_indices(recs, positions, sort, !m->empty || fzb_corpus_bias(c), out, out_len, out_positions, index_offset);
}

int fzb_match_list_indices(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, fzb_match_indices** out, size_t* out_len,
                           uint32_t** out_positions) {
    if (int rc_ = fzb_refuse_scoped(c, "fzb_match_list_indices", "fzb_match_list_top_indices")) return rc_;
    if (int rc_ = fzb_refuse_facets(m ? m->facets : nullptr, "fzb_match_list_indices")) return rc_;
    return match_list_indices_impl(m, c, selection, n_selection, m ? m->config.sort : 0, 0, out, out_len, out_positions);
}

int fzb_match_list_indices_into(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, uint32_t index_offset, fzb_match_indices** out,
                                size_t* out_len, uint32_t** out_positions) {
    if (int rc_ = fzb_refuse_scoped(c, "fzb_match_list_indices_into", "fzb_match_list_top_indices")) return rc_;
    if (int rc_ = fzb_refuse_facets(m ? m->facets : nullptr, "fzb_match_list_indices_into")) return rc_;
    return match_list_indices_impl(m, c, selection, n_selection, FZB_SORT_INDEX_ASC, index_offset, out, out_len, out_positions);
}

void fzb_match_indices_free(fzb_match_indices* matches, uint32_t* positions) {
    free(matches);
    free(positions);
}

// ---- query syntax: Pattern::parse / Pattern::parse_query (src/pattern.rs:87-222) ---------------------------------------------
}  // extern "C"
namespace {
bool is_rust_whitespace(u32 c) {  // char::is_whitespace = Unicode White_Space
    return c == ' ' || (c >= 9 && c <= 13) || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) || c == 0x2028 || c == 0x2029 || c == 0x202F ||
           c == 0x205F || c == 0x3000;
}
void append_utf8(std::string& s, u32 cp) {
    u8 buf[4];
    const int n = encode_utf8(cp, buf);
    s.append((const char*)buf, (size_t)n);
}
struct ParsedAtom { std::string needle; bool negated; int matching; };
// one atom: `!` negates, `^` / `$` anchor, `'` asks for a substring, a bare negated atom is a substring too; `\x` escapes x
ParsedAtom parse_atom(const std::vector<u32>& atom) {
    std::vector<std::pair<u32, bool>> tok;  // (char, escaped)
    for (size_t i = 0; i < atom.size(); i++) {
        if (atom[i] == '\\' && i + 1 < atom.size()) { tok.push_back({atom[i + 1], true}); i++; }
        else tok.push_back({atom[i], false});
    }
    size_t lo = 0, hi = tok.size();
    auto first_is = [&](u32 op) { if (lo < hi && !tok[lo].second && tok[lo].first == op) { lo++; return true; } return false; };
    auto last_is = [&](u32 op) { if (lo < hi && !tok[hi - 1].second && tok[hi - 1].first == op) { hi--; return true; } return false; };
    ParsedAtom a;
    a.negated = first_is('!');
    const bool prefix = first_is('^');
    const bool substring = !prefix && first_is('\'');
    const bool suffix = last_is('$');
    for (size_t i = lo; i < hi; i++) {
        const u32 c = tok[i].first;
        const bool special = c == '!' || c == '^' || c == '\'' || c == '$' || is_rust_whitespace(c);
        if (tok[i].second && !special) a.needle.push_back('\\');  // a backslash before anything else stays literal
        append_utf8(a.needle, c);
    }
    a.matching = prefix && suffix ? FZB_MATCH_EXACT : prefix ? FZB_MATCH_PREFIX : suffix ? FZB_MATCH_SUFFIX : (substring || a.negated) ? FZB_MATCH_SUBSTRING : -1;
    return a;
}
}  // namespace
extern "C" {

}  // extern "C"
namespace {
// the atoms of a query, unparsed: split at unescaped whitespace, `\x` keeps x in its atom
bool split_atoms(const uint8_t* query_utf8, size_t query_len, std::vector<std::vector<u32>>& raw) {
    std::vector<u32> cps;
    if (!decode_utf8(query_utf8, query_len, cps)) return false;
    std::vector<u32> cur;
    bool in_atom = false, escaped = false;
    auto flush = [&]() {
        raw.push_back(cur);
        cur.clear();
        in_atom = false;
    };
    for (u32 c : cps) {
        if (escaped) { escaped = false; cur.push_back(c); }
        else if (c == '\\') { in_atom = true; escaped = true; cur.push_back(c); }
        else if (is_rust_whitespace(c)) { if (in_atom) flush(); }
        else { in_atom = true; cur.push_back(c); }
    }
    if (in_atom) flush();
    return true;
}
int patterns_from_atoms(const std::vector<ParsedAtom>& atoms, fzb_pattern** out_patterns) {
    fzb_pattern* arr = (fzb_pattern*)calloc(std::max<size_t>(atoms.size(), 1), sizeof(fzb_pattern));
    if (!arr) return fail(FZB_ERR_INVALID, "out of memory");
    for (size_t i = 0; i < atoms.size(); i++) {
        u8* n = (u8*)malloc(atoms[i].needle.size() + 1);
        if (!n) {
            for (size_t k = 0; k < i; k++) free((void*)arr[k].needle_utf8);
            free(arr);
            return fail(FZB_ERR_INVALID, "out of memory");
        }
        memcpy(n, atoms[i].needle.data(), atoms[i].needle.size());
        n[atoms[i].needle.size()] = 0;
        arr[i].needle_utf8 = n;
        arr[i].needle_len = atoms[i].needle.size();
        arr[i].negated = atoms[i].negated;
        arr[i].casing = -1;
        arr[i].unicode = -1;
        arr[i].matching = atoms[i].matching;
    }
    *out_patterns = arr;
    return FZB_OK;
}
}  // namespace
extern "C" {

int fzb_parse_query(const uint8_t* query_utf8, size_t query_len, fzb_pattern** out_patterns, size_t* out_n) {
    if (!out_patterns || !out_n || (query_len && !query_utf8)) return fail(FZB_ERR_INVALID, "null argument");
    std::vector<std::vector<u32>> raw;
    if (!split_atoms(query_utf8, query_len, raw)) return fail(FZB_ERR_INVALID, "query is not valid UTF-8");
    std::vector<ParsedAtom> atoms;
    for (const auto& r : raw) {
        ParsedAtom a = parse_atom(r);
        if (!a.needle.empty()) atoms.push_back(a);  // atoms with an empty needle (`!`, `^$`) are dropped
    }
    if (int rc_ = patterns_from_atoms(atoms, out_patterns)) return rc_;
    *out_n = atoms.size();
    return FZB_OK;
}

// fzb_parse_query with the any-of operator: an atom that is exactly `|` joins the atom before it and the atom after it into one group
// when both exist, neither is negated and neither is itself `|`; anywhere else it is the needle `|` it always was.  `\|` is the needle `|`.
int fzb_parse_query_groups(const uint8_t* query_utf8, size_t query_len, fzb_pattern** out_patterns, uint32_t** out_group_of, size_t* out_n) {
    if (!out_patterns || !out_group_of || !out_n || (query_len && !query_utf8)) return fail(FZB_ERR_INVALID, "null argument");
    std::vector<std::vector<u32>> raw;
    if (!split_atoms(query_utf8, query_len, raw)) return fail(FZB_ERR_INVALID, "query is not valid UTF-8");
    struct Atom { ParsedAtom a; bool bar; };
    std::vector<Atom> all;
    for (const auto& r : raw) {
        Atom t{parse_atom(r), r.size() == 1 && r[0] == '|'};
        if (r.size() == 2 && r[0] == '\\' && r[1] == '|') t.a.needle = "|";
        if (!t.a.needle.empty()) all.push_back(t);
    }
    std::vector<ParsedAtom> atoms;
    std::vector<uint32_t> group_of;
    uint32_t next_id = 0;
    bool join_next = false;
    for (size_t i = 0; i < all.size(); i++) {
        const bool joins = all[i].bar && i > 0 && i + 1 < all.size() && !all[i - 1].bar && !all[i + 1].bar && !all[i - 1].a.negated && !all[i + 1].a.negated;
        if (joins) { join_next = true; continue; }
        group_of.push_back(join_next ? group_of.back() : next_id++);
        atoms.push_back(all[i].a);
        join_next = false;
    }
    uint32_t* ids = (uint32_t*)malloc(std::max<size_t>(group_of.size(), 1) * sizeof(uint32_t));
    if (!ids) return fail(FZB_ERR_INVALID, "out of memory");
    if (int rc_ = patterns_from_atoms(atoms, out_patterns)) { free(ids); return rc_; }
    if (!group_of.empty()) memcpy(ids, group_of.data(), group_of.size() * sizeof(uint32_t));
    *out_group_of = ids;
    *out_n = atoms.size();
    return FZB_OK;
}

void fzb_query_groups_free(fzb_pattern* patterns, uint32_t* group_of, size_t n) {
    fzb_patterns_free(patterns, n);
    free(group_of);
}

void fzb_patterns_free(fzb_pattern* patterns, size_t n) {
    if (!patterns) return;
    for (size_t i = 0; i < n; i++) free((void*)patterns[i].needle_utf8);
    free(patterns);
}

// ---- multi-pattern composition (src/matcher/multi.rs) ---------------------------------------------------
// (struct fzb_multi_matcher: host_internal.h - the multi-device forms in host_shard.hip / host_rccl.hip use it too)
}  // extern "C"
static void multi_free_buffers(fzb_multi_matcher* mm) {
    void* ptrs[] = {mm->cand[0], mm->cand[1], mm->counts, mm->items, mm->bitmap, mm->tile_counts};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    mm->cand[0] = mm->cand[1] = nullptr;
    mm->counts = mm->items = nullptr;
    mm->bitmap = nullptr;
    mm->tile_counts = nullptr;
    mm->cap = 0;
}
static void multi_free_group_buffers(fzb_multi_matcher* mm) {
    if (mm->group_slots) (void)hipFree(mm->group_slots);
    if (mm->group_hits) (void)hipFree(mm->group_hits);
    mm->group_slots = nullptr;
    mm->group_hits = nullptr;
    mm->group_cap = 0;
}
static void multi_release(fzb_multi_matcher* mm) {  // every device buffer and pinned word the composition itself owns
    multi_free_buffers(mm);
    fzb_top_release(mm->top);
    for (void* p : {(void*)mm->top_comb, (void*)mm->top_items, (void*)mm->top_npos_u, (void*)mm->top_words, (void*)mm->top_pos_u, (void*)mm->union_src, (void*)mm->union_cursors})
        if (p) (void)hipFree(p);
    mm->top_comb = nullptr;
    mm->top_items = mm->top_npos_u = mm->top_words = mm->top_pos_u = mm->union_cursors = nullptr;
    mm->union_src = nullptr;
    mm->top_rec_cap = mm->top_pos_u_words = mm->union_src_cap = mm->union_cursor_words = 0;
    mm->union_src_host.clear();
    for (void* p : {(void*)mm->gunion_where, (void*)mm->gunion_src, (void*)mm->gunion_scratch})
        if (p) (void)hipFree(p);
    mm->gunion_where = mm->gunion_scratch = nullptr;
    mm->gunion_src = nullptr;
    mm->gunion_where_words = mm->gunion_src_cap = mm->gunion_scratch_words = 0;
    mm->gunion_src_host.clear();
    fzb_sort_release(mm->sort);
    fzb_out_release(*mm);
    fzb_scope_release(mm->scope);
    fzb_sections_release(mm->sections);
    multi_free_group_buffers(mm);
}

// the composition's buffers for ranges of up to `count` haystacks
static int multi_ensure_buffers(fzb_multi_matcher* mm, size_t count) {
    if (mm->cap >= count) return FZB_OK;
    multi_free_buffers(mm);
    const size_t cap = count + count / 8 + 4096;
    HIPCHK(dev_alloc((void**)&mm->cand[0], (cap + 16) * sizeof(fzb_match_rec)));
    HIPCHK(dev_alloc((void**)&mm->cand[1], (cap + 16) * sizeof(fzb_match_rec)));
    HIPCHK(dev_alloc((void**)&mm->counts, MCOUNT_SLOTS * MCOUNT_SLOT_WORDS * sizeof(u32)));
    HIPCHK(dev_alloc((void**)&mm->items, cap * 4));
    HIPCHK(dev_alloc((void**)&mm->bitmap, (cap / 64 + 17) * 8));
    HIPCHK(dev_alloc((void**)&mm->tile_counts, (((cap + FZB_TILE - 1) / FZB_TILE + 5) & ~(size_t)3) * 4));  // (as the workspace's: a multiple of four entries)
    mm->cap = cap;
    return FZB_OK;
}

// the buffers of the any-of steps, beside the composition's own and of their size: only a matcher that has a group allocates them
static int multi_ensure_group_buffers(fzb_multi_matcher* mm) {
    if (mm->group_cap >= mm->cap) return FZB_OK;
    multi_free_group_buffers(mm);
    HIPCHK(dev_alloc((void**)&mm->group_slots, (mm->cap + 16) * sizeof(u32)));  // (k_anyof_clear stores whole 16-byte words)
    HIPCHK(dev_alloc((void**)&mm->group_hits, (mm->cap + 16) * sizeof(fzb_match_rec)));
    mm->group_cap = mm->cap;
    return FZB_OK;
}

// PatternConfig::resolve (src/pattern.rs:250-262); `sort` is the matcher's and applies to the combined list only
static fzb_config resolve_pattern(const fzb_config& config, const fzb_pattern& p) {
    fzb_config rc = config;
    if (p.has_max_typos) rc.max_typos = p.max_typos;
    if (p.casing >= 0) rc.casing = p.casing;
    if (p.unicode >= 0) rc.unicode = p.unicode;
    if (p.has_scoring) rc.scoring = p.scoring;
    if (p.matching >= 0) rc.matching = p.matching;
    rc.sort = FZB_SORT_INDEX_ASC;
    return rc;
}

// A slot holds the needle under `rcfg` already: the same config, the lane pair compared as RESOLVED (a slot made by fzb_matcher_clone
// stores the resolved pair, the caller's config may ask for 0 / 0 or a prefilter width alone - the same needle resolves them alike)
static bool slot_unchanged(const fzb_matcher* m, const fzb_config& rcfg) {
    fzb_config a = m->config;
    a.pf_lanes = rcfg.pf_lanes;
    a.sw_lanes = rcfg.sw_lanes;
    if (!same_config(a, rcfg)) return false;
    int pf = rcfg.pf_lanes, sw = rcfg.sw_lanes;
    if (pf == 0 && sw == 0) detect_host_lanes(m->use_u8, pf, sw);
    else if (sw == 0) sw = m->use_u8 ? pf : pf / 2;
    return pf == m->lc.pf_lanes && sw == m->lc.sw_lanes;
}

static bool same_pattern(const fzb_multi_matcher::Raw& r, const fzb_pattern& p) {  // field by field: fzb_pattern has padding
    const fzb_pattern& q = r.pattern;
    return r.needle.size() == p.needle_len && (p.needle_len == 0 || memcmp(r.needle.data(), p.needle_utf8, p.needle_len) == 0) && q.negated == p.negated &&
           q.has_max_typos == p.has_max_typos && (!p.has_max_typos || q.max_typos == p.max_typos) && q.casing == p.casing && q.unicode == p.unicode &&
           q.has_scoring == p.has_scoring && (!p.has_scoring || same_scoring(q.scoring, p.scoring)) && q.matching == p.matching;
}

// Compiles `patterns` under `config` into the matcher's sub-matcher slots, in order: a slot whose needle and resolved config are unchanged
// is left alone, any other is rebuilt in place (rebuild_matcher keeps its device workspace), and a sub-matcher is created only when the
// compiled patterns outnumber the slots.  Slots beyond the compiled patterns become spares.  mm->config / mm->raw are the caller's to set.
// On an error the slots before the failing pattern have been rebuilt already: multi_compile restores them.
static int compile_into_slots(fzb_multi_matcher* mm, const fzb_config& config, const fzb_pattern* patterns, size_t n_patterns) {
    std::vector<fzb_matcher*> slots;
    slots.reserve(mm->patterns.size() + mm->spare.size());
    for (auto& c : mm->patterns) slots.push_back(c.m);
    slots.insert(slots.end(), mm->spare.begin(), mm->spare.end());
    std::vector<fzb_multi_matcher::Compiled> compiled;
    int rc = FZB_OK;
    for (size_t i = 0; i < n_patterns && !rc; i++) {
        const fzb_pattern& p = patterns[i];
        if (p.needle_len == 0) continue;  // Matcher::compile returns None for an empty needle
        const fzb_config rcfg = resolve_pattern(config, p);
        const size_t k = compiled.size();
        if (k < slots.size()) {
            fzb_matcher* m = slots[k];
            if (!(slot_unchanged(m, rcfg) && m->needle.size() == p.needle_len && memcmp(m->needle.data(), p.needle_utf8, p.needle_len) == 0))
                rc = rebuild_matcher(m, &rcfg, p.needle_utf8, p.needle_len);
        } else {
            fzb_matcher* m = nullptr;
            rc = fzb_matcher_create(&rcfg, p.needle_utf8, p.needle_len, &m);
            if (!rc) slots.push_back(m);
        }
        if (!rc) compiled.push_back({p.negated != 0, slots[k]});
    }
    // (on an error the slots are kept in their order too: nothing is lost and the restore reuses them)
    const size_t k = rc ? 0 : compiled.size();
    if (rc) {
        compiled.clear();
        for (size_t i = 0; i < mm->patterns.size() && i < slots.size(); i++) compiled.push_back({mm->patterns[i].negated, slots[i]});
    }
    mm->patterns.assign(compiled.begin(), compiled.end());
    mm->spare.assign(slots.begin() + (rc ? (std::ptrdiff_t)mm->patterns.size() : (std::ptrdiff_t)k), slots.end());
    return rc;
}

static std::vector<fzb_pattern> raw_patterns(const fzb_multi_matcher* mm) {  // the stored patterns with their needles pointed at again
    std::vector<fzb_pattern> v;
    for (const auto& r : mm->raw) {
        fzb_pattern p = r.pattern;
        p.needle_utf8 = (const uint8_t*)r.needle.data();
        v.push_back(p);
    }
    return v;
}

// group_of -> terms numbered 0, 1, .. in order of appearance (nullptr: every pattern its own term); equal ids must be adjacent
static int normalise_terms(const uint32_t* group_of, size_t n, std::vector<u32>& out) {
    out.resize(n);
    std::vector<uint32_t> seen;
    for (size_t i = 0; i < n; i++) {
        if (!group_of) { out[i] = (u32)i; continue; }
        if (i && group_of[i] == group_of[i - 1]) { out[i] = out[i - 1]; continue; }
        if (std::find(seen.begin(), seen.end(), group_of[i]) != seen.end())
            return fail(FZB_ERR_INVALID, "group_of: term id " + std::to_string(group_of[i]) + " appears again at pattern " + std::to_string(i) + " (equal ids must be adjacent)");
        seen.push_back(group_of[i]);
        out[i] = (u32)seen.size() - 1;
    }
    return FZB_OK;
}

// set_patterns / set_config / create: compile, and on success record what was compiled; on an error the previous patterns are compiled
// again (they were accepted before, so that cannot fail) and the matcher answers as it did
// (raw_terms: the term of every pattern as normalise_terms numbers them - checked here, before anything is compiled)
static int multi_compile(fzb_multi_matcher* mm, const fzb_config& config, const fzb_pattern* patterns, size_t n_patterns, const std::vector<u32>& raw_terms) {
    for (size_t i = 0; i < n_patterns; i++)
        if (patterns[i].needle_len && !patterns[i].needle_utf8) return fail(FZB_ERR_INVALID, "null needle");
    std::vector<u32> terms;  // per compiled pattern: alternatives with an empty needle are dropped like any empty pattern
    for (size_t i = 0; i < n_patterns; i++)
        if (patterns[i].needle_len) terms.push_back(raw_terms[i]);
    bool grouped = false;
    for (size_t i = 0, k = 0; i < n_patterns; i++) {
        if (!patterns[i].needle_len) continue;
        size_t b = k, e = k;
        while (b > 0 && terms[b - 1] == terms[k]) b--;
        while (e < terms.size() && terms[e] == terms[k]) e++;
        if (e - b >= 2) {
            grouped = true;
            if (patterns[i].negated) return fail(FZB_ERR_INVALID, "any-of group: a negated alternative (pattern " + std::to_string(i) + ") is not defined");
            if (e - b > FZB_GROUP_ALTS_MAX) return fail(FZB_ERR_INVALID, "any-of group: " + std::to_string(e - b) + " alternatives, at most FZB_GROUP_ALTS_MAX = 8");
        }
        k++;
    }
    int rc = compile_into_slots(mm, config, patterns, n_patterns);
    if (rc) {
        const std::string msg = fzb_last_error();
        const std::vector<fzb_pattern> old = raw_patterns(mm);
        (void)compile_into_slots(mm, mm->config, old.data(), old.size());
        return fail(rc, msg);
    }
    mm->raw_terms = raw_terms;
    mm->terms.swap(terms);
    mm->grouped = grouped;
    std::vector<fzb_multi_matcher::Raw> raw;
    for (size_t i = 0; i < n_patterns; i++) {
        fzb_multi_matcher::Raw r{patterns[i].needle_len ? std::string((const char*)patterns[i].needle_utf8, patterns[i].needle_len) : std::string(), patterns[i]};
        r.pattern.needle_utf8 = nullptr;
        raw.push_back(std::move(r));
    }
    mm->raw.swap(raw);
    mm->config = config;
    if (mm->order) mm->order->config.sort = config.sort;
    return FZB_OK;
}

// the per-shard clones of the multi-device form follow their parent (their device state stays where it is)
static void multi_follow(fzb_multi_matcher* mm) {
    if (mm->shard_clones.empty()) return;
    const std::vector<fzb_pattern> pats = raw_patterns(mm);
    bool ok = true;
    for (fzb_multi_matcher* cm : mm->shard_clones) ok = ok && multi_compile(cm, mm->config, pats.data(), pats.size(), mm->raw_terms) == FZB_OK;
    if (!ok) {  // cannot happen for patterns the parent accepted; drop the clones rather than keep stale ones (they are made again on the next query)
        int cur = 0;
        const bool have_cur = hipGetDevice(&cur) == hipSuccess;
        for (size_t g = 0; g < mm->shard_clones.size(); g++) {
            if (mm->shard_devices[g] >= 0) (void)hipSetDevice(mm->shard_devices[g]);
            fzb_multi_matcher_free(mm->shard_clones[g]);
        }
        if (have_cur) (void)hipSetDevice(cur);
        mm->shard_clones.clear();
        mm->shard_devices.clear();
        fzb_clear_error();
    }
}

int fzb_multi_order_host(fzb_multi_matcher* mm, fzb_matcher** out) {
    if (!mm->order) {
        int rc = fzb_matcher_create(&mm->config, nullptr, 0, &mm->order);
        if (rc) return rc;
        mm->order->sum_scores = true;
    }
    *out = mm->order;
    return FZB_OK;
}
extern "C" {

int fzb_multi_matcher_create(const fzb_config* config, const fzb_pattern* patterns, size_t n_patterns, fzb_multi_matcher** out) {
    return fzb_multi_matcher_create_groups(config, patterns, n_patterns, nullptr, out);
}

int fzb_multi_matcher_create_groups(const fzb_config* config, const fzb_pattern* patterns, size_t n_patterns, const uint32_t* group_of, fzb_multi_matcher** out) {
    if (!config || !out || (n_patterns && !patterns)) return fail(FZB_ERR_INVALID, "null argument");
    std::vector<u32> terms;
    if (int rc_ = normalise_terms(group_of, n_patterns, terms)) return rc_;
    auto mm = new fzb_multi_matcher();
    mm->config = *config;
    int rc = multi_compile(mm, *config, patterns, n_patterns, terms);
    if (rc) {
        const std::string msg = fzb_last_error();
        fzb_multi_matcher_free(mm);
        return fail(rc, msg);
    }
    *out = mm;
    return FZB_OK;
}

int fzb_multi_matcher_set_patterns(fzb_multi_matcher* mm, const fzb_pattern* patterns, size_t n_patterns) {
    return fzb_multi_matcher_set_pattern_groups(mm, patterns, n_patterns, nullptr);  // (on a grouped matcher: every pattern a single term again)
}

int fzb_multi_matcher_set_pattern_groups(fzb_multi_matcher* mm, const fzb_pattern* patterns, size_t n_patterns, const uint32_t* group_of) {
    if (!mm || (n_patterns && !patterns)) return fail(FZB_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n_patterns; i++)
        if (patterns[i].needle_len && !patterns[i].needle_utf8) return fail(FZB_ERR_INVALID, "null needle");
    std::vector<u32> terms;
    if (int rc_ = normalise_terms(group_of, n_patterns, terms)) return rc_;
    bool same = n_patterns == mm->raw.size() && terms == mm->raw_terms;
    for (size_t i = 0; same && i < n_patterns; i++) same = same_pattern(mm->raw[i], patterns[i]);
    if (same) return FZB_OK;  // "Skipped if the patterns are the same" (src/matcher/mod.rs:170-176) - and the grouping
    const fzb_config cfg = mm->config;
    int rc = multi_compile(mm, cfg, patterns, n_patterns, terms);
    if (rc) return rc;
    multi_follow(mm);
    return FZB_OK;
}

int fzb_multi_matcher_set_config(fzb_multi_matcher* mm, const fzb_config* config) {
    if (!mm || !config) return fail(FZB_ERR_INVALID, "null argument");
    if (same_config(mm->config, *config)) return FZB_OK;
    // every pattern is resolved again; a change of `sort` alone leaves every slot as it is (sub-matchers run IndexAsc)
    const std::vector<fzb_pattern> pats = raw_patterns(mm);
    const std::vector<u32> terms = mm->raw_terms;
    int rc = multi_compile(mm, *config, pats.data(), pats.size(), terms);
    if (rc) return rc;
    multi_follow(mm);
    return FZB_OK;
}

int fzb_multi_matcher_clone(const fzb_multi_matcher* src, fzb_multi_matcher** out) {
    if (!src || !out) return fail(FZB_ERR_INVALID, "null argument");
    auto mm = new fzb_multi_matcher();
    mm->config = src->config;
    mm->raw = src->raw;
    mm->raw_terms = src->raw_terms;
    mm->terms = src->terms;
    mm->grouped = src->grouped;
    for (const auto& c : src->patterns) {
        fzb_matcher* m = nullptr;
        int rc = fzb_matcher_clone(c.m, &m);  // keeps the resolved lane pair
        if (rc) {
            const std::string msg = fzb_last_error();
            fzb_multi_matcher_free(mm);
            return fail(rc, msg);
        }
        mm->patterns.push_back({c.negated, m});
    }
    *out = mm;
    return FZB_OK;
}

int fzb_multi_matcher_reserve(fzb_multi_matcher* mm, const fzb_corpus* c) {
    if (!mm || !c) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = fzb_corpus_reserved_items(c);
    int rc;
    for (auto& p : mm->patterns)
        if ((rc = reserve_slot_any_needle(p.m, c))) return rc;
    for (fzb_matcher* m : mm->spare)
        if ((rc = reserve_slot_any_needle(m, c))) return rc;
    if ((rc = multi_ensure_buffers(mm, n)) || (rc = fzb_out_ensure(*mm, n)) || (rc = fzb_sort_ensure(mm->sort, n))) return rc;
    if (mm->grouped && (rc = multi_ensure_group_buffers(mm))) return rc;
    if ((c->tags.data || mm->facets) && n && (rc = fzb_scope_ensure(mm->scope, n))) return rc;  // (a corpus that carries tags, or a facet sink: the composition's records ahead of the drop / the count)
    if (!mm->fetch.count_host) HIPCHK(hipHostMalloc((void**)&mm->fetch.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));
    if (!mm->fetch_top.count_host) HIPCHK(hipHostMalloc((void**)&mm->fetch_top.count_host, OUT_FETCH_WORDS * sizeof(u32), hipHostMallocDefault));
    return FZB_OK;
}

void fzb_debug_set_fused_capture(int on) { g_debug_fused_capture = on ? 1 : 0; }

int fzb_debug_device_allocs(uint64_t* out) {
    if (!out) return fail(FZB_ERR_INVALID, "null argument");
    *out = g_fzb_dev_allocs.load(std::memory_order_relaxed);
    return FZB_OK;
}

void fzb_multi_matcher_free(fzb_multi_matcher* mm) {
    if (!mm) return;
    fzb_matcher_free(mm->order);  // first: joins its shard workers before the per-shard clones they run go
    if (!mm->shard_clones.empty()) {  // a shard clone's device state lives on its shard's device
        int cur = 0;
        const bool have_cur = hipGetDevice(&cur) == hipSuccess;
        for (size_t g = 0; g < mm->shard_clones.size(); g++) {
            if (mm->shard_devices[g] >= 0) (void)hipSetDevice(mm->shard_devices[g]);
            fzb_multi_matcher_free(mm->shard_clones[g]);
        }
        if (have_cur) (void)hipSetDevice(cur);
    }
    for (auto& p : mm->patterns) fzb_matcher_free(p.m);
    for (fzb_matcher* m : mm->spare) fzb_matcher_free(m);
    multi_release(mm);
    delete mm;
}

size_t fzb_multi_matcher_len(const fzb_multi_matcher* mm) { return mm ? mm->patterns.size() : 0; }

int fzb_multi_match_list_parallel(fzb_multi_matcher* mm, const fzb_corpus* c, size_t threads, fzb_match** out, size_t* out_len) {
    if (!mm || !c) return fail(FZB_ERR_INVALID, "null argument");
    if (threads == 0) return fail(FZB_ERR_PANIC, "threads must be positive");  // parallel.rs:24
    if (int rc_ = fzb_refuse_facets(mm->facets, "fzb_multi_match_list_parallel")) return rc_;
    return fzb_multi_match_list(mm, c, out, out_len);
}

}  // extern "C"
// The composition of a matcher that has an any-of group (anyof.h): an AND of TERMS, where a term is a single pattern - composed exactly as
// multi_compose_device composes it - or a group of k alternatives, which behaves as ONE non-negated pattern whose hits are the union of the
// alternatives' hits under the max rule.  Per group: one clear of the slots, then per alternative its pipeline (into group_hits) and one
// accumulate, then one flag and one compact that write the group's records - k pipelines + k + 3 launches, every count on the device.
//   base group  (the first non-negated term): the alternatives run over the whole range through the streaming filter (items == nullptr), or
//               over the candidate set; a slot per haystack of the range / per item of the set; records (index_offset + haystack, score_G, exact_G)
//   later group: the alternatives run over the surviving candidates' items; a slot per candidate; records = candidate joined with the key
static int multi_compose_groups(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, u32 cap32, uint32_t* dev_count,
                                hipStream_t st, const SubsetArgs* sa, bool* captured) {
    int rc;
    if ((rc = multi_ensure_buffers(mm, count)) || (rc = multi_ensure_group_buffers(mm))) return rc;
    const int cus = mm->num_cus;
    auto& ps = mm->patterns;
    struct Term { size_t b, e; };  // compiled patterns [b, e)
    std::vector<Term> terms;
    for (size_t i = 0; i < ps.size();) {
        size_t e = i + 1;
        while (e < ps.size() && mm->terms[e] == mm->terms[i]) e++;
        terms.push_back({i, e});
        i = e;
    }
    size_t base = terms.size();
    for (size_t t = 0; t < terms.size(); t++)
        if (!ps[terms[t].b].negated) { base = t; break; }  // (a group has no negated alternative; a grouped matcher has a non-negated term)
    const u32 n_max = (u32)count;
    u32* const hit_count = fzb_multi_count(mm, MCOUNT_ALTERNATIVE);
    int cur = 0;
    // the group `t` over the candidates cand[cur] (cand_in == nullptr: as the base term) -> cand[dst]
    auto run_group = [&](const Term& t, const fzb_match_rec* cand_in, const u32* n_ptr, const u32* slot_items, u32 n_bound, int dst) -> int {
        fzb_launch_anyof_clear(mm->group_slots, n_ptr, n_max, n_bound, cus * 4, st);
        for (size_t pi = t.b; pi < t.e; pi++) {
            int rc_ = cand_in ? run_pipeline(ps[pi].m, c, first, count, index_offset, mm->items, n_ptr, (fzb_match*)mm->group_hits, mm->group_cap, hit_count, st)
                              : run_pipeline(ps[pi].m, c, first, count, index_offset, subset_items(sa), subset_count(sa), (fzb_match*)mm->group_hits, mm->group_cap, hit_count, st, nullptr,
                                             subset_hint(sa));
            if (rc_) return rc_;
            fzb_launch_anyof_accumulate(mm->group_hits, hit_count, (u32)std::min<size_t>(mm->group_cap, 0xFFFFFFFFu), mm->group_slots, n_ptr, n_max, n_bound, index_offset, slot_items, cand_in,
                                        cus * 4, st);
        }
        fzb_launch_anyof_keep(mm->group_slots, n_ptr, n_max, n_bound, index_offset, slot_items, cand_in, mm->bitmap, mm->tile_counts, mm->cand[dst], fzb_multi_count(mm, dst), cus * 2, st);
        return FZB_OK;
    };
    const Term& bt = terms[base];
    if (bt.e - bt.b >= 2) {
        const u32 n_bound = subset_items(sa) ? (u32)std::min<u64>(subset_hint(sa), count) : n_max;
        if ((rc = run_group(bt, nullptr, subset_count(sa), subset_items(sa), n_bound, 0))) return rc;
    } else if ((rc = run_pipeline(ps[bt.b].m, c, first, count, index_offset, subset_items(sa), subset_count(sa), (fzb_match*)mm->cand[0], mm->cap, fzb_multi_count(mm, 0), st, nullptr,
                                  subset_hint(sa)))) {
        return rc;
    }
    for (size_t ti = 0; ti < terms.size(); ti++) {
        if (ti == base) continue;
        const Term& t = terms[ti];
        fzb_launch_records_to_items(mm->cand[cur], fzb_multi_count(mm, cur), index_offset, mm->items, cus * 2, st);
        const int oth = cur ^ 1;
        if (t.e - t.b >= 2) {
            if ((rc = run_group(t, mm->cand[cur], fzb_multi_count(mm, cur), nullptr, n_max, oth))) return rc;
        } else if (!ps[t.b].negated) {
            if ((rc = run_pipeline(ps[t.b].m, c, first, count, index_offset, mm->items, fzb_multi_count(mm, cur), (fzb_match*)mm->cand[oth], mm->cap, fzb_multi_count(mm, oth), st))) return rc;
            fzb_launch_join_add(mm->cand[oth], fzb_multi_count(mm, oth), mm->cand[cur], fzb_multi_count(mm, cur), cus * 2, st);
        } else {
            fzb_match_rec* hits = mm->cand[oth];  // (as multi_compose_device: read by the flag pass, then overwritten by the compaction)
            if ((rc = run_pipeline(ps[t.b].m, c, first, count, index_offset, mm->items, fzb_multi_count(mm, cur), (fzb_match*)hits, mm->cap, fzb_multi_count(mm, MCOUNT_NEGATED), st))) return rc;
            fzb_launch_remove_hits(mm->cand[cur], fzb_multi_count(mm, cur), hits, fzb_multi_count(mm, MCOUNT_NEGATED), mm->bitmap, mm->tile_counts, mm->cand[oth], fzb_multi_count(mm, oth), cus * 2, st);
        }
        cur = oth;
    }
    if (sa && sa->capture && captured && g_debug_fused_capture) {
        fzb_subset* cp = sa->capture;
        fzb_launch_copy_capture_records(mm->cand[cur], fzb_multi_count(mm, cur), (fzb_match_rec*)dev_out, cap32, dev_count, index_offset, cp->idx, (u32)std::min<size_t>(cp->cap, 0xFFFFFFFFu),
                                        cp->count_dev, sa->mirror, cus * 2, st);
        HIPCHK(hipGetLastError());
        subset_captured(cp, c);
        *captured = true;
        return FZB_OK;
    }
    fzb_launch_copy_records(mm->cand[cur], fzb_multi_count(mm, cur), (fzb_match_rec*)dev_out, cap32, dev_count, cus * 2, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

// the composition alone: the patterns' scores summed, no score bias
// (sa->in: the candidate set the FIRST step runs over - the base pattern's pipeline, the Single shortcut's, or the identity records of the
// no-pattern and all-negated cases -; every later pattern runs over the candidates' items either way.  sa->capture: the Multi case's final copy
// writes the capture too (k_copy_capture_records) and says so in *captured; the Empty and Single cases leave it to the caller's subset_capture.)
static int multi_compose_device(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity,
                                uint32_t* dev_count, void* stream, const SubsetArgs* sa = nullptr, bool* captured = nullptr) {
    if (!mm || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    if (first > c->dev.n || count > c->dev.n - first) return fail(FZB_ERR_INVALID, "range outside the corpus");
    if ((u64)count + (u64)index_offset > 0xFFFFFFFFull) return refuse_index_overflow((u64)count + index_offset, index_offset);
    hipStream_t st = (hipStream_t)stream;
    if (!mm->num_cus) HIPCHK((hipError_t)fzb_effective_cus(&mm->num_cus));
    const int cus = mm->num_cus;
    const u32 cap32 = (u32)std::min<size_t>(capacity, 0xFFFFFFFFu);
    auto& ps = mm->patterns;
    if (count == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, st));
        return FZB_OK;
    }
    if (mm->grouped) return multi_compose_groups(mm, c, first, count, index_offset, dev_out, cap32, dev_count, st, sa, captured);
    // CompiledPatterns::{Empty, Single, Multi} (src/matcher/mod.rs:178-190; a single NEGATED pattern is Multi)
    if (ps.empty()) {
        // (over a candidate set: its count when the host knows it, else the room it was captured into - never more than the list)
        const size_t need = subset_items(sa) ? (size_t)std::min<u64>(subset_hint(sa), count) : count;
        if (need > capacity) return fail(FZB_ERR_CAPACITY, "output buffer smaller than the haystack list (no pattern: every haystack matches)");
        if (subset_items(sa)) fzb_launch_items_records((fzb_match_rec*)dev_out, subset_items(sa), subset_count(sa), cap32, (u32)need, index_offset, dev_count, cus * 2, st);
        else fzb_launch_identity_records((fzb_match_rec*)dev_out, (u32)count, index_offset, dev_count, cus * 2, st);
        HIPCHK(hipGetLastError());
        return FZB_OK;
    }
    if (ps.size() == 1 && !ps[0].negated)
        return run_pipeline(ps[0].m, c, first, count, index_offset, subset_items(sa), subset_count(sa), dev_out, capacity, dev_count, stream, nullptr, subset_hint(sa));
    if (int rc_ = multi_ensure_buffers(mm, count)) return rc_;
    // match_list_multi_into (src/matcher/multi.rs:84-152)
    size_t base = ps.size();
    for (size_t i = 0; i < ps.size(); i++)
        if (!ps[i].negated) { base = i; break; }
    int cur = 0;  // cand[cur] / counts[cur] = the candidates
    int rc;
    if (base != ps.size()) {
        rc = run_pipeline(ps[base].m, c, first, count, index_offset, subset_items(sa), subset_count(sa), (fzb_match*)mm->cand[0], mm->cap, fzb_multi_count(mm, 0), stream, nullptr, subset_hint(sa));
        if (rc) return rc;
    } else if (subset_items(sa)) {  // all patterns negated over a candidate set: every haystack of the set is a candidate
        fzb_launch_items_records(mm->cand[0], subset_items(sa), subset_count(sa), (u32)std::min<size_t>(mm->cap, count), (u32)std::min<u64>(subset_hint(sa), count), index_offset, fzb_multi_count(mm, 0),
                                 cus * 2, st);
    } else {
        fzb_launch_identity_records(mm->cand[0], (u32)count, index_offset, fzb_multi_count(mm, 0), cus * 2, st);  // all patterns negated: every haystack is a candidate
    }
    for (size_t pi = 0; pi < ps.size(); pi++) {
        if (pi == base) continue;
        // (the reference skips the remaining patterns once no candidate is left; with the count on the device the kernels just find nothing to do)
        fzb_launch_records_to_items(mm->cand[cur], fzb_multi_count(mm, cur), index_offset, mm->items, cus * 2, st);
        const int oth = cur ^ 1;
        if (!ps[pi].negated) {
            rc = run_pipeline(ps[pi].m, c, first, count, index_offset, mm->items, fzb_multi_count(mm, cur), (fzb_match*)mm->cand[oth], mm->cap, fzb_multi_count(mm, oth), stream);
            if (rc) return rc;
            fzb_launch_join_add(mm->cand[oth], fzb_multi_count(mm, oth), mm->cand[cur], fzb_multi_count(mm, cur), cus * 2, st);
            cur = oth;
        } else {
            // the negated pattern's hits land in the other slot; k_flag_absent reads them, then k_compact_records (next in stream
            // order) overwrites that same slot with the candidates that were not hit
            fzb_match_rec* hits = mm->cand[oth];
            rc = run_pipeline(ps[pi].m, c, first, count, index_offset, mm->items, fzb_multi_count(mm, cur), (fzb_match*)hits, mm->cap, fzb_multi_count(mm, MCOUNT_NEGATED), stream);
            if (rc) return rc;
            fzb_launch_remove_hits(mm->cand[cur], fzb_multi_count(mm, cur), hits, fzb_multi_count(mm, MCOUNT_NEGATED), mm->bitmap, mm->tile_counts, mm->cand[oth], fzb_multi_count(mm, oth), cus * 2, st);
            cur = oth;
        }
    }
    if (sa && sa->capture && captured && g_debug_fused_capture) {
        fzb_subset* cp = sa->capture;
        fzb_launch_copy_capture_records(mm->cand[cur], fzb_multi_count(mm, cur), (fzb_match_rec*)dev_out, cap32, dev_count, index_offset, cp->idx, (u32)std::min<size_t>(cp->cap, 0xFFFFFFFFu),
                                        cp->count_dev, sa->mirror, cus * 2, st);
        HIPCHK(hipGetLastError());
        subset_captured(cp, c);
        *captured = true;
        return FZB_OK;
    }
    fzb_launch_copy_records(mm->cand[cur], fzb_multi_count(mm, cur), (fzb_match_rec*)dev_out, cap32, dev_count, cus * 2, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
extern "C" {

// (on a biased corpus the bias is added ONCE per record, after the composition's sum; with no pattern every haystack's score is its bias)
// (sa: the candidate-set forms - the composition runs over `in`, and the COMPOSED records are captured where the single forms capture theirs:
// ahead of the list's terms.  A composition of several patterns captures in its final copy; the no-pattern and Single cases have no such copy
// and take subset_capture's launch.)
static int multi_match_list_device_impl(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity,
                                        uint32_t* dev_count, void* stream, const SubsetArgs* sa) {
    int rc;
    fzb_facets* const fc = mm ? mm->facets : nullptr;
    if ((rc = facets_check(fc, c, "fzb_multi_match_list_device"))) return rc;
    const bool uncut = fc && capacity < count;  // (a facet sink counts every match: the composition goes into the scratch, which has room for them)
    if (mm && c && count && (fzb_corpus_scoped(c) || uncut) && dev_count && (dev_out || !capacity)) {  // the composition into the scratch (with no pattern: identity records), then drop, then bias
        if ((rc = fzb_scope_ensure(mm->scope, count))) return rc;
        bool captured = false;
        if ((rc = multi_compose_device(mm, c, first, count, index_offset, (fzb_match*)mm->scope.recs, count, mm->scope.words, stream, sa, &captured))) return rc;
        if (!captured && (rc = subset_capture(sa, c, mm->scope.recs, mm->scope.words, count, mm->num_cus * 2, (hipStream_t)stream))) return rc;
        return apply_terms(c, mm->scope, count, (fzb_match_rec*)dev_out, capacity, dev_count, first, index_offset, mm->num_cus * 2, (hipStream_t)stream, fc);
    }
    bool captured = false;
    rc = multi_compose_device(mm, c, first, count, index_offset, dev_out, capacity, dev_count, stream, sa, &captured);
    if (rc) return rc;
    if (count && !captured && (rc = subset_capture(sa, c, (const fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), mm->num_cus * 2, (hipStream_t)stream))) return rc;
    if ((rc = facets_records(fc, c, (const fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), first, index_offset, mm->num_cus * 2, (hipStream_t)stream))) return rc;
    return apply_bias(c, (fzb_match_rec*)dev_out, dev_count, std::min(capacity, count), first, index_offset, mm->num_cus * 2, (hipStream_t)stream);
}
int fzb_multi_match_list_device(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity,
                                uint32_t* dev_count, void* stream) {
    return multi_match_list_device_impl(mm, c, first, count, index_offset, dev_out, capacity, dev_count, stream, nullptr);
}

static int multi_match_list_impl(fzb_multi_matcher* mm, const fzb_corpus* c, fzb_match** out, size_t* out_len, const SubsetArgs* sa);
int fzb_multi_match_list(fzb_multi_matcher* mm, const fzb_corpus* c, fzb_match** out, size_t* out_len) { return multi_match_list_impl(mm, c, out, out_len, nullptr); }
static int multi_match_list_impl(fzb_multi_matcher* mm, const fzb_corpus* c, fzb_match** out, size_t* out_len, const SubsetArgs* sa) {
    if (!mm || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    const size_t count = c->dev.n;
    *out = nullptr;
    *out_len = 0;
    if (int rc_ = fzb_out_ensure(*mm, count)) return rc_;
    int rc = multi_match_list_device_impl(mm, c, 0, count, 0, (fzb_match*)mm->out_dev, mm->out_cap, mm->count_dev, nullptr, sa);
    if (rc) return rc;
    // Matcher::match_list (src/matcher/mod.rs:212-222): reverse, then the stable radix sort unless there is no pattern at all
    const int sort = mm->config.sort;
    const bool reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    // (no pattern over a biased corpus - the empty prompt - IS ordered: the scores are the biases)
    const bool by_score = (!mm->patterns.empty() || fzb_corpus_bias(c)) && (sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC);
    if ((reversed || by_score) && count) {
        if (by_score)
            if (int rc_ = fzb_sort_ensure(mm->sort, count)) return rc_;
        fzb_launch_sort(mm->out_dev, mm->sort.tmp, mm->count_dev, mm->sort.hist, (u32)(mm->sort.cap / 2048 + 2), reversed, by_score, mm->num_cus * 2, nullptr);
        HIPCHK(hipGetLastError());
    }
    return fetch_records(mm->fetch, mm->out_dev, mm->count_dev, mm->out_cap, out, out_len);
}

// `Matcher::match_list_indices` over CompiledPatterns (mod.rs:234-275): Empty / Single as above; Multi = match_one_indices_multi
// (multi.rs:56-82) for every haystack of the list.  Like match_list_multi_into, every pattern only sees the haystacks that are
// still alive, and each pattern's positions come from the traced scorer on the device; the per-haystack union is host work.
static int multi_match_list_indices_impl(fzb_multi_matcher* mm, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, int sort, uint32_t index_offset,
                                         fzb_match_indices** out, size_t* out_len, uint32_t** out_positions) {
    if (!mm || !c || !out || !out_len || !out_positions || (!selection && n_selection)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    *out_positions = nullptr;
    size_t count = 0;
    int rc = check_selection(c, selection, n_selection, count, index_offset);
    if (rc) return rc;
    std::vector<fzb_match_indices> recs;
    std::vector<u32> positions;
    if (mm->patterns.empty()) {  // CompiledPatterns::Empty
        recs.resize(count);
        for (size_t i = 0; i < count; i++) recs[i] = fzb_match_indices{(uint32_t)i, 0, 0, 0, 0, 0};
        return finish_indices(recs, positions, sort, false, out, out_len, out_positions, index_offset);
    }
    if (mm->patterns.size() == 1 && !mm->patterns[0].negated) {  // CompiledPatterns::Single
        rc = indices_in_list_order(mm->patterns[0].m, c, selection, count, recs, positions);
        if (rc) return rc;
        return finish_indices(recs, positions, sort, true, out, out_len, out_positions, index_offset);
    }
    // alive[k] = (position in the caller's list, corpus index); combined score / exact / positions per alive haystack
    std::vector<u32> alive_pos(count), alive_idx(count);
    for (size_t i = 0; i < count; i++) {
        alive_pos[i] = (u32)i;
        alive_idx[i] = selection ? selection[i] : (u32)i;
    }
    std::vector<u32> score(count, 0);
    std::vector<u8> exact(count, 0);
    std::vector<std::vector<u32>> found(count);
    std::vector<fzb_match_indices> hits;
    std::vector<u32> hit_positions;
    for (auto& p : mm->patterns) {
        if (alive_idx.empty()) break;
        hit_positions.clear();
        rc = indices_in_list_order(p.m, c, alive_idx.data(), alive_idx.size(), hits, hit_positions);
        if (rc) return rc;
        std::vector<u32> next_pos, next_idx;
        if (p.negated) {  // a negated pattern that matches drops the haystack
            size_t h = 0;
            for (size_t k = 0; k < alive_idx.size(); k++) {
                if (h < hits.size() && hits[h].index == k) { h++; continue; }
                next_pos.push_back(alive_pos[k]);
                next_idx.push_back(alive_idx[k]);
            }
        } else {  // every other pattern must match; scores add with saturation, exact flags OR, positions accumulate
            for (const fzb_match_indices& hit : hits) {
                const u32 at = alive_pos[hit.index];
                score[at] = std::min<u32>(0xFFFFu, score[at] + hit.score);
                exact[at] |= hit.exact;
                found[at].insert(found[at].end(), hit_positions.begin() + hit.positions_begin, hit_positions.begin() + hit.positions_begin + hit.positions_len);
                next_pos.push_back(at);
                next_idx.push_back(alive_idx[hit.index]);
            }
        }
        alive_pos.swap(next_pos);
        alive_idx.swap(next_idx);
    }
    recs.reserve(alive_pos.size());
    for (u32 at : alive_pos) {  // "Indices are reported in reverse order, and patterns may share matched chars" (multi.rs:75-77)
        std::vector<u32>& f = found[at];
        std::sort(f.begin(), f.end(), [](u32 a, u32 b) { return a > b; });
        f.erase(std::unique(f.begin(), f.end()), f.end());
        recs.push_back(fzb_match_indices{at, (uint16_t)score[at], exact[at], 0, (uint32_t)positions.size(), (uint32_t)f.size()});
        positions.insert(positions.end(), f.begin(), f.end());
    }
    return finish_indices(recs, positions, sort, true, out, out_len, out_positions, index_offset);
}

int fzb_multi_match_list_indices(fzb_multi_matcher* mm, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, fzb_match_indices** out, size_t* out_len,
                                 uint32_t** out_positions) {
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_indices")) return rc_;
    if (int rc_ = fzb_refuse_biased(c, "fzb_multi_match_list_indices", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_scoped(c, "fzb_multi_match_list_indices", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_facets(mm ? mm->facets : nullptr, "fzb_multi_match_list_indices")) return rc_;
    return multi_match_list_indices_impl(mm, c, selection, n_selection, mm ? mm->config.sort : 0, 0, out, out_len, out_positions);
}

int fzb_multi_match_list_indices_into(fzb_multi_matcher* mm, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, uint32_t index_offset,
                                      fzb_match_indices** out, size_t* out_len, uint32_t** out_positions) {
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_indices_into")) return rc_;
    if (int rc_ = fzb_refuse_biased(c, "fzb_multi_match_list_indices_into", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_scoped(c, "fzb_multi_match_list_indices_into", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_facets(mm ? mm->facets : nullptr, "fzb_multi_match_list_indices_into")) return rc_;
    return multi_match_list_indices_impl(mm, c, selection, n_selection, FZB_SORT_INDEX_ASC, index_offset, out, out_len, out_positions);
}

// `Matcher::match_list_into` over CompiledPatterns (src/matcher/mod.rs:373-392): index order, host result
int fzb_multi_match_list_into(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match** out, size_t* out_len) {
    if (!mm || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    if (first > c->dev.n || count > c->dev.n - first) return fail(FZB_ERR_INVALID, "range outside the corpus");
    *out = nullptr;
    *out_len = 0;
    if (int rc_ = fzb_out_ensure(*mm, count)) return rc_;
    int rc = fzb_multi_match_list_device(mm, c, first, count, index_offset, (fzb_match*)mm->out_dev, mm->out_cap, mm->count_dev, nullptr);
    if (rc) return rc;
    return fetch_records(mm->fetch, mm->out_dev, mm->count_dev, mm->out_cap, out, out_len);
}

// ---- top-`limit` queries ------------------------------------------------------------------------------------------------------
// The reference has no such call: `match_list` returns a Vec the caller truncates.  top(limit) = the first min(limit, found) records of
// what `match_list` returns (reverse for the *Desc strategies, then the stable radix sort: src/matcher/mod.rs:215-221, src/sort.rs:6-40),
// ties at the cut included, and `found` = the length of the full list.  The pipeline writes its index-ordered records into the sort's
// second buffer, the selection stage (kernels_topk.hip) keeps the records of the head in record order, the ordering step sorts those.
}  // extern "C"
// The two count words and the records of a top result -> the host with ONE wait: at most `max_records` = min(limit, n) records exist, so
// a head of up to FZB_TOP_COPY_WHOLE records is copied whole behind the count, filled or not.  Beyond that the bound says little - a
// `limit` at or above the list's length bounds the copy by n records, 80 MB on a 10 M list of which 4 MB exist: 1.5 ms at the 53 GB/s the
// copy reaches against the 0.24 ms the call takes (profiles/topk.txt) - so such a head takes fzb_fetch_records' guess (the previous
// result's size; a grown or first result costs a second copy and wait, as in fzb_match_list).  128 KB: copying 10 000 records whole was
// measured at 5 us over copying 100 (C2, top(10 000) - top(100), their sort included), under the 10-20 us a second wait costs.
#define FZB_TOP_COPY_WHOLE 16384
int fzb_fetch_top(FetchHint& h, const void* dev_records, const u32* dev_words, size_t max_records, hipStream_t st, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    if (max_records <= FZB_TOP_COPY_WHOLE) h.last = max_records;
    int rc = fzb_fetch_records(h, dev_records, dev_words, 0, max_records, st, out, out_len);
    if (rc) return rc;
    if (out_found) *out_found = h.count_host[PAIR_FOUND];
    return FZB_OK;
}
// CompiledPatterns::Empty: every haystack matches with score 0, reversed for the *Desc strategies, never sorted (mod.rs:215-220, 381-384)
int fzb_empty_pattern_top(size_t n, int sort, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    const bool reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    const size_t want = std::min(limit, n);
    fzb_match* r = (fzb_match*)malloc(std::max<size_t>(want, 1) * sizeof(fzb_match));
    if (!r) return fail(FZB_ERR_INVALID, "out of memory");
    for (size_t i = 0; i < want; i++) r[i] = fzb_match{(uint32_t)(reversed ? n - 1 - i : i), 0, 0, 0};
    *out = r;
    *out_len = want;
    if (out_found) *out_found = n;
    return FZB_OK;
}
extern "C" {

static int top_device_impl(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream, const SubsetArgs* sa);
int fzb_match_list_top_device(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream) {
    return top_device_impl(m, c, limit, dev_out, capacity, dev_count, stream, nullptr);
}
// The producer of the top stages on `stream`, over the n > 0 haystacks of c (or the candidate set of sa): the pipeline, the capture, the
// facets, the corpus' scope drop and the bias.  What the selection reads: the index-ordered records in the sort's second buffer, their pair
// (written, found) in *raw_count, and the ordering flags.
static int top_produce(fzb_matcher* m, const fzb_corpus* c, size_t n, void* stream, const SubsetArgs* sa, u32** raw_count_out, bool* reversed, bool* by_score, bool* one_pass) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // (the range workspace first: growing it releases every workspace buffer, the sort's included)
    if ((rc = fzb_bind_device(m)) || (rc = ensure_workspace(m, n, st, true)) || (rc = ensure_sort_buffers(m, n))) return rc;
    if (!m->count_dev && (rc = fzb_ensure_out_staging(m, 0))) return rc;
    fzb_order_flags(m, fzb_corpus_bias_hi(c), reversed, by_score, one_pass);
    Workspace& w = m->ws;
    u32* const raw_count = m->count_dev + OUT_RAW;  // the pipeline's pair (records written, matches found)
    *raw_count_out = raw_count;
    if (fzb_corpus_scoped(c)) {  // the selection sees the visible haystacks' records only: `found` counts those, the head holds none that is hidden
        if ((rc = fzb_scope_ensure(m->scope, n)) || (rc = run_pipeline(m, c, 0, n, 0, subset_items(sa), subset_count(sa), (fzb_match*)m->scope.recs, n, m->scope.words, stream, nullptr, subset_hint(sa)))) return rc;
        if ((rc = subset_capture(sa, c, m->scope.recs, m->scope.words, n, m->lc.num_cus * 2, st))) return rc;
        if ((rc = apply_terms(c, m->scope, n, w.sort.tmp, n, raw_count, 0, 0, m->lc.num_cus * 2, st, m->facets))) return rc;
    } else {
        if ((rc = run_pipeline(m, c, 0, n, 0, subset_items(sa), subset_count(sa), (fzb_match*)w.sort.tmp, n, raw_count, stream, nullptr, subset_hint(sa)))) return rc;
        if ((rc = subset_capture(sa, c, w.sort.tmp, raw_count, n, m->lc.num_cus * 2, st))) return rc;
        if ((rc = facets_records(m->facets, c, w.sort.tmp, raw_count, n, 0, 0, m->lc.num_cus * 2, st))) return rc;  // (room for every haystack: never cut ahead of the count)
        if ((rc = apply_bias(c, w.sort.tmp, raw_count, n, 0, 0, m->lc.num_cus * 2, st))) return rc;  // before the selection reads a score
    }
    return FZB_OK;
}
static int top_device_impl(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream, const SubsetArgs* sa) {
    if (!m || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (capacity < want) return refuse_small_output("min(limit, haystacks)", capacity, want);
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    if (m->empty) return fail(FZB_ERR_INVALID, "empty needle: handled on the host by fzb_match_list_top");
    if (int rc_ = facets_check(m->facets, c, "fzb_match_list_top_device")) return rc_;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, st));
        return facets_none(m->facets, st);
    }
    int rc;
    bool reversed, by_score, one_pass;
    u32* raw_count = nullptr;
    if ((rc = top_produce(m, c, n, stream, sa, &raw_count, &reversed, &by_score, &one_pass))) return rc;
    Workspace& w = m->ws;
    const u32 ntiles_cap = (u32)(w.sort.cap / 2048 + 2);
    const int grid = m->lc.num_cus * 2;
    HIPCHK(fzb_launch_topk_select(w.sort.tmp, raw_count, (u32)n, (u32)want, by_score, reversed, one_pass, (fzb_match_rec*)dev_out, (u32)want, dev_count, w.sort.hist, ntiles_cap, grid, st));
    fzb_launch_sort((fzb_match_rec*)dev_out, w.sort.tmp, dev_count, w.sort.hist, ntiles_cap, reversed, by_score, grid, st, one_pass ? 1 : 2);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

int fzb_match_list_top(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    if (!m || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    if (out_found) *out_found = 0;
    const size_t n = c->dev.n;
    if (prompt_on_device(m, c, nullptr, n)) return prompt_top_host(m, c, nullptr, limit, out, out_len, out_found);
    if (m->empty || n == 0) {
        if (int rc_ = facets_every(m->facets, c, 0, n, "fzb_match_list_top")) return rc_;
    }
    if (m->empty) return fzb_empty_pattern_top(n, m->config.sort, limit, out, out_len, out_found);
    if (n == 0) return FZB_OK;
    const size_t want = std::min(limit, n);
    if (int rc_ = fzb_ensure_out_staging(m, want)) return rc_;
    int rc = fzb_match_list_top_device(m, c, limit, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr);
    if (rc) return rc;
    return fzb_fetch_top(m->fetch_top, m->out_dev, m->count_dev, want, nullptr, out, out_len, out_found);
}

}  // extern "C"
// the ordering flags of the composition: a matcher without a pattern scores 0 everywhere, so only a bias makes its scores an order
static void multi_order_flags(const fzb_multi_matcher* mm, const fzb_corpus* c, bool* reversed, bool* by_score) {
    const int sort = mm->config.sort;
    *reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    *by_score = (!mm->patterns.empty() || fzb_corpus_bias(c)) && (sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC);
}
// The top stage of a `from_patterns` matcher on `st`: the composition over the n haystacks into the sort's second buffer (its pair in
// raw_count), the selection of the best `want` and their ordering into `head` (room for `want` records; its pair - records, matches found -
// in head_count).  Nothing is read back.
// (sa: the composition runs over the candidate set and its records are captured; the selection and the ordering see no difference)
static int multi_top_stage(fzb_multi_matcher* mm, const fzb_corpus* c, size_t n, size_t want, fzb_match_rec* head, u32* head_count, u32* raw_count, hipStream_t st,
                           const SubsetArgs* sa = nullptr) {
    int rc;
    if ((rc = fzb_sort_ensure(mm->sort, n))) return rc;
    if ((rc = multi_match_list_device_impl(mm, c, 0, n, 0, (fzb_match*)mm->sort.tmp, n, raw_count, st, sa))) return rc;
    bool reversed, by_score;
    multi_order_flags(mm, c, &reversed, &by_score);
    const u32 ntiles_cap = (u32)(mm->sort.cap / 2048 + 2);
    const int grid = mm->num_cus * 2;
    // (summed scores can pass 255: both selection levels, both radix passes - as fzb_multi_match_list orders)
    HIPCHK(fzb_launch_topk_select(mm->sort.tmp, raw_count, (u32)n, (u32)want, by_score, reversed, 0, head, (u32)want, head_count, mm->sort.hist, ntiles_cap, grid, st));
    fzb_launch_sort(head, mm->sort.tmp, head_count, mm->sort.hist, ntiles_cap, reversed, by_score, grid, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}
extern "C" {

static int multi_match_list_top_impl(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found, const SubsetArgs* sa);
int fzb_multi_match_list_top(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    return multi_match_list_top_impl(mm, c, limit, out, out_len, out_found, nullptr);
}
static int multi_match_list_top_impl(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found, const SubsetArgs* sa) {
    if (!mm || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    if (out_found) *out_found = 0;
    const size_t n = c->dev.n;
    if (n == 0) return facets_none(mm->facets, nullptr);
    const size_t want = std::min(limit, n);
    int rc;
    if ((rc = fzb_out_ensure(*mm, want)) || (rc = multi_top_stage(mm, c, n, want, mm->out_dev, mm->count_dev, mm->count_dev + OUT_RAW, nullptr, sa))) return rc;
    return fzb_fetch_top(mm->fetch_top, mm->out_dev, mm->count_dev, want, nullptr, out, out_len, out_found);
}

// ---- top-`limit` with matched positions: one fused device call ------------------------------------------------------------------
// The reference has no such call: the caller truncates what `Matcher::match_list_indices` returns (src/matcher/mod.rs:234-275).  Here the top
// stage leaves its sorted head in HBM (m->top.head), k_top_items makes it the item list of a traced second pass (run_pipeline's item form
// with a TraceOut: records in head order into m->top_traced - neither the head nor the caller's output -, strided positions into the
// matched-indices scratch), and the pack kernels (kernels_indices.hip) write the caller's records and dense positions while checking that
// the two passes agree (the accept decision and the scores of match_list and match_list_indices are the same code in the reference:
// src/matcher/algo.rs:78-103 against :196-227).  Nothing is read back between the stages.
}  // extern "C"
static_assert(sizeof(fzb_indices_rec) == sizeof(fzb_match_indices) && offsetof(fzb_indices_rec, positions_begin) == offsetof(fzb_match_indices, positions_begin) &&
                  offsetof(fzb_indices_rec, positions_len) == offsetof(fzb_match_indices, positions_len),
              "the pack kernels write fzb_match_indices");
namespace {
// the buffers of a fused query with a head of up to `want` records and `stride` position dwords per record (everything but the traced
// scorer's matrices, which are workspace); staging: the host form's packed result too
int ensure_top_indices_buffers(fzb_matcher* m, size_t want, size_t stride, bool staging) {
    int rc = ensure_trace_buffers(m, want, want * stride);
    if (rc) return rc;
    if (!m->top_idx_words) HIPCHK(dev_alloc((void**)&m->top_idx_words, TOPIDX_WORDS * sizeof(u32)));
    if ((rc = fzb_grow_dev(&m->top_traced, &m->top_traced_cap, want, 16))) return rc;
    return fzb_top_ensure(m->top, want, want * stride, staging);
}
u32 trace_stride(const fzb_matcher* m) { return (u32)std::max(1, m->nd.nbytes); }  // position dwords per record: as indices_in_list_order
// the traced scorer's matrices for heads of up to `want` records and needles of up to `stride` bytes: one (rows + 1) x TRACE_W slab per wave
// of its grid; a needle of b bytes has at most b rows, and one the by-value NeedleDev holds at most FZB_MAX_ROWS (a longer needle's scratch
// is its own: ensure_long_needle grows it on first use)
int reserve_trace_cells(fzb_matcher* m, size_t want, size_t stride) {
    NeedleDev probe = m->nd;
    probe.rows = (int32_t)std::min<size_t>(stride, FZB_MAX_ROWS);
    return ensure_trace_cells(m, fzb_trace_scratch_words(probe, traced_grid(m->lc.num_cus, want)));
}

// malloc'ed result of the *_indices entry points (fzb_match_indices_free): nrec records, npos positions, copied from `recs` / `pos`
int hand_over_indices(const fzb_match_indices* recs, size_t nrec, const u32* pos, size_t npos, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions) {
    fzb_match_indices* r = (fzb_match_indices*)malloc(std::max<size_t>(nrec, 1) * sizeof(fzb_match_indices));
    u32* p = (u32*)malloc(std::max<size_t>(npos, 1) * 4);
    if (!r || !p) {
        free(r);
        free(p);
        return fail(FZB_ERR_INVALID, "out of memory");
    }
    if (nrec) memcpy(r, recs, nrec * sizeof(fzb_match_indices));
    if (npos) memcpy(p, pos, npos * 4);
    *out = r;
    *out_len = nrec;
    *out_positions = p;
    return FZB_OK;
}

// the empty prompt's head with (empty) position lists: the device's head, then records without positions
int prompt_top_indices_host(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions,
                            uint64_t* out_found) {
    fzb_match* head = nullptr;
    size_t nhead = 0;
    if (int rc_ = prompt_top_host(m, c, in, limit, &head, &nhead, out_found)) return rc_;
    std::vector<fzb_match_indices> recs(nhead);
    for (size_t i = 0; i < nhead; i++) recs[i] = fzb_match_indices{head[i].index, head[i].score, 0, 0, 0, 0};
    fzb_matches_free(head);
    return hand_over_indices(recs.data(), nhead, nullptr, 0, out, out_len, out_positions);
}
// CompiledPatterns::Empty (an empty needle, no pattern): fzb_empty_pattern_top's rule - the first / last min(limit, n) indices, score 0 - and no
// positions
int empty_top_indices(const fzb_corpus* c, size_t n, int sort, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    if (corpus_terms(c)) {  // the empty prompt over a biased or scoped corpus: the head of the visible list, ordered by the bias
        fzb_match* head = nullptr;
        size_t nhead = 0;
        if (int rc_ = biased_empty_list(c, 0, n, 0, sort, limit, &head, &nhead, out_found)) return rc_;
        std::vector<fzb_match_indices> recs(nhead);
        for (size_t i = 0; i < nhead; i++) recs[i] = fzb_match_indices{head[i].index, head[i].score, 0, 0, 0, 0};
        free(head);
        return hand_over_indices(recs.data(), nhead, nullptr, 0, out, out_len, out_positions);
    }
    const size_t want = std::min(limit, n);
    const bool reversed = sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC;
    std::vector<fzb_match_indices> recs(want);
    for (size_t i = 0; i < want; i++) recs[i] = fzb_match_indices{(uint32_t)(reversed ? n - 1 - i : i), 0, 0, 0, 0, 0};
    if (out_found) *out_found = n;
    return hand_over_indices(recs.data(), want, nullptr, 0, out, out_len, out_positions);
}

// The result of a fused query on the null stream -> the caller, with ONE wait for the count words (w), the records (t.packed) and the
// packed positions (t.dense): a head of up to FZB_TOP_COPY_WHOLE records is copied whole behind the words, filled or not (fzb_fetch_top's
// rule), and so are its positions while they are no more than the records would be at that bound (256 KB); beyond, the copy takes the
// previous result's size (*last_records, *last_positions) and a little more, and a result that outgrew it costs a second wait.
// want / max_pos: the most records / positions the result can have.  `disagree`: what a raised inconsistency word means.
// HostWords: the count words of a host form - `n` words at `dev` come back in the one copy, into `host`; the pack's PACK_WORDS sit at word
// `pack` of them and the captured count, where the form captures, at word `capture`.
struct HostWords { u32* dev; size_t n, pack, capture; u32 host[SEC_SLAB_FETCH] = {}; };
int fetch_top_indices(HostWords& w, TopStaging& t, size_t want, size_t max_pos, const char* disagree, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    auto guess = [](size_t last, size_t most) { return last ? std::min(most, last + last / 64 + 64) : (size_t)0; };
    const size_t grec = want <= FZB_TOP_COPY_WHOLE ? want : guess(t.last_records, want);
    const size_t gpos = max_pos <= (size_t)FZB_TOP_COPY_WHOLE * 4 ? max_pos : guess(t.last_positions, max_pos);
    const size_t front = (w.n * 4 + 31) / 32 * 32;  // the words' room in front of the records
    u8* stage = (u8*)fzb_pinned_get(front + grec * sizeof(fzb_match_indices) + gpos * 4);
    if (!stage) return fail(FZB_ERR_HIP, "hipHostMalloc failed for the result list");
    const u32* const hw = (const u32*)stage + w.pack;
    const fzb_match_indices* const hrec = (const fzb_match_indices*)(stage + front);
    const u32* const hpos = (const u32*)(stage + front + grec * sizeof(fzb_match_indices));
    hipError_t e = hipMemcpyAsync(stage, w.dev, w.n * 4, hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess && grec) e = hipMemcpyAsync((void*)hrec, t.packed, grec * sizeof(fzb_match_indices), hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess && gpos) e = hipMemcpyAsync((void*)hpos, t.dense, gpos * 4, hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess) e = fzb_stream_wait(nullptr);
    if (e != hipSuccess) {
        fzb_pinned_put(stage);
        return fail(FZB_ERR_HIP, std::string("device to host: ") + hipGetErrorString(e));
    }
    const size_t nrec = std::min<size_t>(hw[0], want), npos = std::min<size_t>(hw[2], max_pos), found = hw[1];
    memcpy(w.host, stage, w.n * 4);
    if (hw[3]) {
        const u32 why = hw[3];
        fzb_pinned_put(stage);
        return fail(FZB_ERR_HIP, std::string("internal: ") + disagree + " (" + ((why & 1u) ? "record count" : "a record's index, score or exact flag") + ")");
    }
    int rc = hand_over_indices(hrec, std::min(nrec, grec), hpos, std::min(npos, gpos), out, out_len, out_positions);
    fzb_pinned_put(stage);
    if (rc) return rc;
    if (nrec > grec || npos > gpos) {  // the result outgrew the guess: the rest in a second copy, straight into the caller's arrays
        fzb_match_indices* r = (fzb_match_indices*)realloc(*out, std::max<size_t>(nrec, 1) * sizeof(fzb_match_indices));
        if (r) *out = r;
        u32* p = r ? (u32*)realloc(*out_positions, std::max<size_t>(npos, 1) * 4) : nullptr;
        if (p) *out_positions = p;
        e = (r && p) ? hipSuccess : hipErrorOutOfMemory;
        if (e == hipSuccess && nrec > grec) e = hipMemcpy(r + grec, (const fzb_match_indices*)t.packed + grec, (nrec - grec) * sizeof(fzb_match_indices), hipMemcpyDeviceToHost);
        if (e == hipSuccess && npos > gpos) e = hipMemcpy(p + gpos, t.dense + gpos, (npos - gpos) * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            fzb_match_indices_free(*out, *out_positions);
            *out = nullptr;
            *out_positions = nullptr;
            *out_len = 0;
            return fail(FZB_ERR_HIP, std::string("device to host: ") + hipGetErrorString(e));
        }
        *out_len = nrec;
    }
    t.last_records = nrec;
    t.last_positions = npos;
    if (out_found) *out_found = found;
    return FZB_OK;
}
// after a host form's wait: the captured count came back in `word`
void subset_capture_known(fzb_subset* capture, u32 word) {
    if (!capture) return;
    capture->count = word;
    capture->known = true;
}
// What the host forms with matched positions share behind their own checks and trivial branches, on the null stream: the packed staging for a
// head of up to `want` records and max_pos positions, the form's device impl - impl(PackedOut): the staging as the _device form's output, the
// count words, and `mirror` = where a capturing form's count lands -, the one wait, and the captured count made known.  The owner's buffers
// (w.dev among them) exist before the call.
struct PackedOut { fzb_match_indices* recs; size_t cap; u32* pos; size_t pos_cap; u32 *words, *mirror; };
template <typename Impl>
int top_indices_host(TopStaging& t, HostWords& w, size_t want, size_t max_pos, fzb_subset* capture, const char* disagree, Impl&& impl, fzb_match_indices** out, size_t* out_len,
                     uint32_t** out_positions, uint64_t* out_found) {
    int rc;
    if ((rc = fzb_top_ensure(t, want, max_pos, true))) return rc;
    if ((rc = impl(PackedOut{(fzb_match_indices*)t.packed, t.packed_cap, t.dense, t.dense_words, w.dev, capture ? w.dev + w.capture : nullptr}))) return rc;
    if ((rc = fetch_top_indices(w, t, want, max_pos, disagree, out, out_len, out_positions, out_found))) return rc;
    subset_capture_known(capture, w.host[w.capture]);
    return FZB_OK;
}
// the out-parameters of the host forms with matched positions, cleared ahead of everything that can fail
void clear_indices_out(fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    *out = nullptr;
    *out_len = 0;
    *out_positions = nullptr;
    if (out_found) *out_found = 0;
}
}  // namespace
extern "C" {

// The tail of every fused "head + matched positions" query of a single matcher: m->top.head holds a head of up to `want` records in the caller's
// order, m->top_idx_words its pair, m->trace_sel / the word behind it the head's item list (k_top_items; k_sec_items for sectioned heads).
// From there: the traced pass over the items, the bias on the traced records, the pack into the caller's buffers and four words at dev_count.
static int top_indices_tail(fzb_matcher* m, const fzb_corpus* c, size_t want, u32 stride, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                            uint32_t* dev_count, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    u32* const head_count = m->top_idx_words + TOPIDX_HEAD;
    u32* const traced_count = m->top_idx_words + TOPIDX_TRACED;  // the traced pass' pair
    u32* const n_items = m->trace_sel + m->trace_cap;
    const int grid = m->lc.num_cus * 2;
    int rc;
    const TraceOut tr{m->trace_pos, m->trace_npos, stride};
    // (grids from the head's capacity on the host, trimmed by the item count on the device; want == 0 - limit 0 - clears the pair and launches nothing)
    if ((rc = run_pipeline(m, c, 0, want, 0, m->trace_sel, n_items, (fzb_match*)m->top_traced, want, traced_count, stream, &tr))) return rc;
    // (the head's scores are biased: the traced records get the same pass, so the pack holds them to the head on the scores the caller sees)
    if ((rc = apply_bias(c, m->top_traced, traced_count, want, 0, 0, grid, st))) return rc;
    fzb_launch_indices_pack(m->top.head, head_count, m->top_traced, traced_count, m->trace_npos, m->trace_pos, stride, (fzb_indices_rec*)dev_out, (u32)std::min<size_t>(capacity, 0xFFFFFFFFu),
                            dev_positions, (u32)std::min<size_t>(positions_capacity, 0xFFFFFFFFu), dev_count, m->top.tiles, (u32)want, grid, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

// (sa: the top stage runs over the candidate set and captures; the traced pass runs over the head's item list as before)
static int top_indices_device_impl(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                   uint32_t* dev_count, void* stream, const SubsetArgs* sa) {
    if (!m || !c || !dev_count || (!dev_out && capacity) || (!dev_positions && positions_capacity)) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (capacity < want) return refuse_small_output("min(limit, haystacks)", capacity, want);
    if (m->empty) return fail(FZB_ERR_INVALID, "empty needle: handled on the host by fzb_match_list_top_indices");
    const u32 stride = trace_stride(m);
    if (positions_capacity < want * (size_t)stride) return refuse_small_positions("min(limit, haystacks)", positions_capacity, want * (size_t)stride);
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    if ((u64)want * stride > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, PACK_WORDS * sizeof(u32), st));
        return facets_none(m->facets, st);
    }
    int rc;
    if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, stride, false))) return rc;
    u32* const head_count = m->top_idx_words + TOPIDX_HEAD;  // (records, matches found) of the head
    u32* const n_items = m->trace_sel + m->trace_cap;
    if ((rc = top_device_impl(m, c, limit, (fzb_match*)m->top.head, want, head_count, stream, sa))) return rc;
    const int grid = m->lc.num_cus * 2;
    fzb_launch_top_items(m->top.head, head_count, (u32)want, m->trace_sel, n_items, dev_count, (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, (want + 255) / 256)), st);
    return top_indices_tail(m, c, want, stride, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream);
}
int fzb_match_list_top_indices_device(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                      uint32_t* dev_count, void* stream) {
    return top_indices_device_impl(m, c, limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, nullptr);
}
// what both host forms of the single matcher do behind their trivial branches (a needle, a corpus that is not empty): in / capture as the
// _subset form got them, null from the plain form, whose device call sees no SubsetArgs at all
static int top_indices_host_query(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len,
                                  uint32_t** out_positions, uint64_t* out_found) {
    const size_t want = std::min(limit, (size_t)c->dev.n), stride = trace_stride(m);
    int rc;
    if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, stride, false))) return rc;
    HostWords w{m->top_idx_words + TOPIDX_RESULT, PACK_WORDS + (capture ? 1 : 0), 0, TOPIDX_CAPTURE - TOPIDX_RESULT};
    auto impl = [&](const PackedOut& o) {
        const SubsetArgs sa{in, capture, o.mirror};
        return top_indices_device_impl(m, c, limit, o.recs, o.cap, o.pos, o.pos_cap, o.words, nullptr, (in || capture) ? &sa : nullptr);
    };
    return top_indices_host(m->top, w, want, want * stride, capture, "the traced pass disagrees with the top stage", impl, out, out_len, out_positions, out_found);
}

int fzb_match_list_top_indices(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    if (!m || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    clear_indices_out(out, out_len, out_positions, out_found);
    const size_t n = c->dev.n;
    if (prompt_on_device(m, c, nullptr, n)) return prompt_top_indices_host(m, c, nullptr, limit, out, out_len, out_positions, out_found);
    if (m->empty || n == 0) {
        if (int rc_ = facets_every(m->facets, c, 0, n, "fzb_match_list_top_indices")) return rc_;
    }
    if (m->empty) return empty_top_indices(c, n, m->config.sort, limit, out, out_len, out_positions, out_found);
    if (n == 0) return hand_over_indices(nullptr, 0, nullptr, 0, out, out_len, out_positions);
    return top_indices_host_query(m, c, nullptr, nullptr, limit, out, out_len, out_positions, out_found);
}

// Sizes what fzb_matcher_reserve leaves to the first matched-indices query - item list, position counts, strided positions, the traced
// scorer's matrices - and the fused query's own buffers (head, traced records, tile sums, packed records and positions), for heads of up to
// min(limit, haystacks the corpus has room for) records and needles of up to max_needle_bytes bytes.
int fzb_matcher_reserve_top_indices(fzb_matcher* m, const fzb_corpus* c, size_t limit, size_t max_needle_bytes) {
    if (!m || !c) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = fzb_corpus_reserved_items(c);
    const size_t want = std::min(limit, n);
    if (want == 0) return FZB_OK;
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    const size_t stride = std::max<size_t>(std::max<size_t>(max_needle_bytes, 1), m->empty ? 1 : trace_stride(m));
    if ((u64)want * stride > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    int rc = fzb_bind_device(m);
    if (rc) return rc;
    // (the range workspace first: growing it releases every workspace buffer, the traced scorer's matrices included)
    if (!m->empty && (rc = ensure_workspace(m, n))) return rc;
    if ((rc = ensure_top_indices_buffers(m, want, stride, true))) return rc;
    return reserve_trace_cells(m, want, stride);
}

}  // extern "C"
// ---- CANDIDATE SETS (include/frizbee_hip.h: fzb_subset) ----------------------------------------------------------------------------------
// The handle: an ascending index list of ONE corpus in device memory, its count beside it.  The set-up calls follow the editing family's
// rules (a corpus the library owns, on its device; they wait for outstanding device work on entry and are complete on return; an error
// leaves the subset as it was).
namespace {
int subset_begin(const fzb_subset* s, const char* what) {
    if (!s || !s->corpus) return fail(FZB_ERR_INVALID, "null argument");
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    if (device != s->corpus->device)
        return fail(FZB_ERR_INVALID, std::string(what) + ": the subset's corpus lives on device " + std::to_string(s->corpus->device) + ", the current device is " + std::to_string(device));
    HIPCHK(hipDeviceSynchronize());
    return FZB_OK;
}
size_t subset_tiles(size_t items) { return ((items + FZB_TILE - 1) / FZB_TILE + 4) & ~(size_t)3; }
// room for `want` indices: every array anew, the old ones released only when all three exist (an error leaves the subset as it was); the
// indices are NOT carried over - every caller fills the whole list afterwards
int subset_room(fzb_subset* s, size_t want) {
    if (s->idx && s->cap >= want) return FZB_OK;
    const size_t cap = std::max<size_t>(std::max<size_t>(want, s->cap * 2), 1);
    u32* idx = nullptr;
    u64* bitmap = nullptr;
    u32* tiles = nullptr;
    hipError_t e = dev_alloc((void**)&idx, cap * 4);
    if (e == hipSuccess) e = dev_alloc((void**)&bitmap, subset_tiles(cap) * (FZB_TILE / 64) * 8);
    if (e == hipSuccess) e = dev_alloc((void**)&tiles, subset_tiles(cap) * 4);
    if (e != hipSuccess) {
        if (idx) (void)hipFree(idx);
        if (bitmap) (void)hipFree(bitmap);
        if (tiles) (void)hipFree(tiles);
        return fail(FZB_ERR_HIP, std::string("fzb_subset (room for ") + std::to_string(cap) + " indices): " + hipGetErrorString(e));
    }
    if (s->idx) (void)hipFree(s->idx);
    if (s->bitmap) (void)hipFree(s->bitmap);
    if (s->tiles) (void)hipFree(s->tiles);
    s->idx = idx;
    s->bitmap = bitmap;
    s->tiles = tiles;
    s->cap = cap;
    return FZB_OK;
}
// the count on the host: read back (and the device waited for) only when the last capture left it unknown
int subset_count_host(fzb_subset* s, u64* out) {
    if (!s->known) {
        u32 n = 0;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(&n, s->count_dev, 4, hipMemcpyDeviceToHost));
        s->count = n;
        s->known = true;
    }
    *out = s->count;
    return FZB_OK;
}
// what every *_subset query checks before anything is launched; grows the capture's room when the list outgrew it
int subset_check(const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, const char* call) {
    if (in && capture && in == capture) return fail(FZB_ERR_INVALID, std::string(call) + ": the capture subset is the input subset; use two and alternate them");
    if ((in || capture) && !c->own_bytes)
        return fail(FZB_ERR_INVALID, std::string(call) + ": the corpus borrows its device memory (fzb_corpus_from_device); a subset needs a corpus made by fzb_corpus_upload");
    if (in && in->corpus != c) return fail(FZB_ERR_INVALID, std::string(call) + ": the input subset is stale: it belongs to another corpus");
    if (in && in->generation != c->generation)
        return fail(FZB_ERR_INVALID, std::string(call) + ": the input subset is stale: it was filled at generation " + std::to_string(in->generation) + " of the corpus, which is now at " +
                                         std::to_string(c->generation) + " (the list changed since)");
    if (capture && capture->corpus != c) return fail(FZB_ERR_INVALID, std::string(call) + ": the capture subset belongs to another corpus");
    if (capture) return subset_room(capture, c->dev.n);
    return FZB_OK;
}
// a capture whose query launched nothing (an empty corpus, an empty needle): the set itself, written by a set-up style copy
int subset_capture_trivial(const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture) {
    if (!capture) return FZB_OK;
    HIPCHK(hipDeviceSynchronize());
    if (in) {
        u64 n = 0;
        if (int rc = subset_count_host(const_cast<fzb_subset*>(in), &n)) return rc;
        if (n) HIPCHK(hipMemcpy(capture->idx, in->idx, n * 4, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(capture->count_dev, in->count_dev, 4, hipMemcpyDeviceToDevice));
        capture->count = n;
    } else {
        fzb_launch_subset_from_scope(nullptr, (u32)c->dev.n, 0, 0, capture->bitmap, capture->tiles, capture->idx, capture->count_dev, (int)fzb_grid_cap(~0ull, 2), nullptr);  // (512 on 256 CUs)
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        capture->count = c->dev.n;
    }
    capture->known = true;
    capture->generation = c->generation;
    return FZB_OK;
}
// No pattern over a candidate set, on the HOST, for the one caller without an fzb_matcher (fzb_multi_match_list_top_indices_subset; the single
// matcher's empty prompt runs on the device: prompt_records) - the picker's empty prompt restricted to a folder: the haystacks of `in`, score
// 0 or the clamped bias, the hidden ones dropped, ordered as biased_empty_list orders (the reference's rule without a bias: reversed for the
// *Desc strategies, never sorted).  Host work: one copy of the indices and of the columns the corpus carries.
int subset_empty_list(const fzb_corpus* c, fzb_subset* in, int sort, size_t limit, std::vector<fzb_match>& recs, uint64_t* out_found) {
    u64 n = 0;
    if (int rc = subset_count_host(in, &n)) return rc;
    std::vector<u32> idx(n);
    if (n) HIPCHK(hipMemcpy(idx.data(), in->idx, n * 4, hipMemcpyDeviceToHost));
    std::vector<int16_t> hb;
    std::vector<uint16_t> ht;
    const bool biased = fzb_corpus_bias(c) != nullptr, scoped = fzb_corpus_scoped(c);
    if (biased)
        if (int rc = fetch_column(fzb_corpus_bias(c), 0, (size_t)c->dev.n, hb)) return rc;
    if (scoped)
        if (int rc = fetch_column(c->tags.data, 0, (size_t)c->dev.n, ht)) return rc;
    recs.clear();
    recs.reserve(n);
    for (u64 k = 0; k < n; k++) {
        const u32 i = idx[k];
        if (!scoped || scope_visible(ht[i], c->scope_require, c->scope_exclude)) recs.push_back(fzb_match{i, (uint16_t)(biased ? sbias_clamp_add(0, hb[i]) : 0), 0, 0});
    }
    if (sort == FZB_SORT_INDEX_DESC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC) std::reverse(recs.begin(), recs.end());
    if (biased && (sort == FZB_SORT_SCORE_THEN_INDEX_ASC || sort == FZB_SORT_SCORE_THEN_INDEX_DESC))
        std::stable_sort(recs.begin(), recs.end(), [](const fzb_match& a, const fzb_match& b) { return a.score > b.score; });
    if (out_found) *out_found = recs.size();
    if (recs.size() > limit) recs.resize(limit);
    return FZB_OK;
}
int hand_over_matches(const std::vector<fzb_match>& recs, fzb_match** out, size_t* out_len) {
    fzb_match* r = (fzb_match*)malloc(std::max<size_t>(recs.size(), 1) * sizeof(fzb_match));
    if (!r) return fail(FZB_ERR_INVALID, "out of memory");
    if (!recs.empty()) memcpy(r, recs.data(), recs.size() * sizeof(fzb_match));
    *out = r;
    *out_len = recs.size();
    return FZB_OK;
}
}  // namespace
extern "C" {

int fzb_corpus_generation(const fzb_corpus* c, uint64_t* out) {
    if (!c || !out) return fail(FZB_ERR_INVALID, "null argument");
    *out = c->generation;
    return FZB_OK;
}

int fzb_subset_create(const fzb_corpus* c, fzb_subset** out) {
    if (!c || !out) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!c->own_bytes) return fail(FZB_ERR_INVALID, "fzb_subset_create: the corpus borrows its device memory (fzb_corpus_from_device); a subset needs a corpus made by fzb_corpus_upload");
    fzb_subset* s = new fzb_subset;
    s->corpus = c;
    s->generation = c->generation;
    int rc = subset_begin(s, "fzb_subset_create");
    if (!rc) rc = subset_room(s, fzb_corpus_reserved_items(c));
    if (!rc) {
        hipError_t e = dev_alloc((void**)&s->count_dev, 16);
        if (e == hipSuccess) e = hipMemset(s->count_dev, 0, 16);
        if (e != hipSuccess) rc = fail(FZB_ERR_HIP, std::string("fzb_subset_create: ") + hipGetErrorString(e));
    }
    if (rc) {
        fzb_subset_free(s);
        return rc;
    }
    *out = s;
    return FZB_OK;
}

void fzb_subset_free(fzb_subset* s) {
    if (!s) return;
    if (s->idx) (void)hipFree(s->idx);
    if (s->bitmap) (void)hipFree(s->bitmap);
    if (s->tiles) (void)hipFree(s->tiles);
    if (s->count_dev) (void)hipFree(s->count_dev);
    delete s;
}

int fzb_subset_set_indices(fzb_subset* s, const uint32_t* host_indices, size_t n) {
    if (!s || (n && !host_indices)) return fail(FZB_ERR_INVALID, "null argument");
    int rc = subset_begin(s, "fzb_subset_set_indices");
    if (rc) return rc;
    const fzb_corpus* c = s->corpus;
    for (size_t k = 0; k < n; k++) {
        if (host_indices[k] >= c->dev.n)
            return fail(FZB_ERR_INVALID, "fzb_subset_set_indices: index " + std::to_string(host_indices[k]) + " at position " + std::to_string(k) + " is beyond the corpus' " + std::to_string(c->dev.n) + " haystacks");
        if (k && host_indices[k] <= host_indices[k - 1])
            return fail(FZB_ERR_INVALID, "fzb_subset_set_indices: index " + std::to_string(host_indices[k]) + " at position " + std::to_string(k) + " does not ascend (the one before it is " +
                                             std::to_string(host_indices[k - 1]) + "); the indices must be strictly ascending");
    }
    if ((rc = subset_room(s, std::max<size_t>(n, c->dev.n)))) return rc;
    const u32 n32 = (u32)n;
    if (n) HIPCHK(hipMemcpy(s->idx, host_indices, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->count_dev, &n32, 4, hipMemcpyHostToDevice));
    s->count = n;
    s->known = true;
    s->generation = c->generation;
    return FZB_OK;
}

int fzb_subset_from_scope(fzb_subset* s, const fzb_corpus* c, uint16_t require, uint16_t exclude) {
    if (!s || !c) return fail(FZB_ERR_INVALID, "null argument");
    if (s->corpus != c) return fail(FZB_ERR_INVALID, "fzb_subset_from_scope: the subset belongs to another corpus");
    int rc = subset_begin(s, "fzb_subset_from_scope");
    if (rc) return rc;
    if ((u64)c->dev.n > 0xFFFFFFFFull) return refuse_index_overflow(c->dev.n);
    if ((rc = subset_room(s, c->dev.n))) return rc;
    fzb_launch_subset_from_scope(c->tags.data, (u32)c->dev.n, require, exclude, s->bitmap, s->tiles, s->idx, s->count_dev, (int)fzb_grid_cap(~0ull, 2), nullptr);  // (512 on 256 CUs)
    HIPCHK(hipGetLastError());
    u32 n32 = 0;
    HIPCHK(hipMemcpy(&n32, s->count_dev, 4, hipMemcpyDeviceToHost));
    s->count = n32;
    s->known = true;
    s->generation = c->generation;
    return FZB_OK;
}

int fzb_subset_info(fzb_subset* s, uint64_t out[4]) {
    if (!s || !out) return fail(FZB_ERR_INVALID, "null argument");
    out[0] = s->known ? 1 : 0;
    u64 n = 0;
    if (int rc = subset_count_host(s, &n)) return rc;
    out[1] = n;
    out[2] = s->cap;
    out[3] = s->generation;
    return FZB_OK;
}

int fzb_subset_read(fzb_subset* s, uint32_t* host_out, size_t cap, size_t* out_n) {
    if (!s || !out_n || (cap && !host_out)) return fail(FZB_ERR_INVALID, "null argument");
    int rc = subset_begin(s, "fzb_subset_read");
    if (rc) return rc;
    u64 n = 0;
    if ((rc = subset_count_host(s, &n))) return rc;
    *out_n = (size_t)n;
    if (n > cap) return fail(FZB_ERR_CAPACITY, "fzb_subset_read: the subset holds " + std::to_string(n) + " indices, the buffer " + std::to_string(cap));
    if (n) HIPCHK(hipMemcpy(host_out, s->idx, n * 4, hipMemcpyDeviceToHost));
    return FZB_OK;
}

// ---- FACET SINKS (include/frizbee_hip.h: fzb_facets; facets.h) -----------------------------------------------------------------------------
// The handle: FZB_FACET_WORDS counts in device memory and a page-locked mirror, of ONE corpus.  A matcher it is attached to fills it with
// every query that honours it (facets_records / facets_column / apply_terms above).
int fzb_facets_create(const fzb_corpus* c, fzb_facets** out) {
    if (!c || !out) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    fzb_facets* f = new fzb_facets;
    f->corpus = c;
    hipError_t e = hipGetDevice(&f->device);
    if (e == hipSuccess) e = dev_alloc((void**)&f->block, FZB_FACET_WORDS * sizeof(u32));
    if (e == hipSuccess) e = hipMemset(f->block, 0, FZB_FACET_WORDS * sizeof(u32));
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->mirror, FZB_FACET_WORDS * sizeof(u32), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        fzb_facets_free(f);
        return fail(FZB_ERR_HIP, std::string("fzb_facets_create: ") + hipGetErrorString(e));
    }
    memset(f->mirror, 0, FZB_FACET_WORDS * sizeof(u32));
    *out = f;
    return FZB_OK;
}

void fzb_facets_free(fzb_facets* f) {
    if (!f) return;
    (void)facets_settle(f);  // (a copy into the mirror may still be in flight)
    if (f->done) (void)hipEventDestroy(f->done);
    if (f->block) (void)hipFree(f->block);
    if (f->mirror) (void)hipHostFree(f->mirror);
    delete f;
}

// After a host form (the null stream) the query's own wait has drained it: facets_settle finds it idle and nothing is asked of the device.
// After a _device form the copy may still be in flight: wait for it, as fzb_subset_info does for a captured count - for the sink's own event
// when the form ran on a stream of the caller's (that stream may have been destroyed since and is never touched), else for the null stream.
int fzb_facets_read(fzb_facets* f, uint32_t out[FZB_FACET_WORDS]) {
    if (!f || !out) return fail(FZB_ERR_INVALID, "null argument");
    if (int rc = facets_settle(f)) return rc;
    memcpy(out, f->mirror, FZB_FACET_WORDS * sizeof(u32));
    return FZB_OK;
}

const uint32_t* fzb_facets_device(const fzb_facets* f) { return f ? f->block : nullptr; }

int fzb_matcher_set_facets(fzb_matcher* m, fzb_facets* f) {
    if (!m) return fail(FZB_ERR_INVALID, "null argument");
    m->facets = f;
    return FZB_OK;
}

int fzb_multi_matcher_set_facets(fzb_multi_matcher* mm, fzb_facets* f) {
    if (!mm) return fail(FZB_ERR_INVALID, "null argument");
    mm->facets = f;
    return FZB_OK;
}

int fzb_match_list_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_match** out, size_t* out_len) {
    if (!m || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    int rc = subset_check(c, in, capture, "fzb_match_list_subset");
    if (rc) return rc;
    const size_t n = c->dev.n;
    if (m->empty || n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        if (!in) return fzb_match_list(m, c, out, out_len);
        if (n == 0) return hand_over_matches(std::vector<fzb_match>(), out, out_len);
        return prompt_list_host(m, c, in, 0, n, 0, true, out, out_len);
    }
    if ((rc = fzb_ensure_out_staging(m, n))) return rc;
    SubsetArgs sa{in, capture, capture ? m->count_dev + OUT_CAPTURE : nullptr};
    if ((rc = sorted_range_impl(m, c, 0, n, 0, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr, &sa))) return rc;
    if ((rc = fetch_records(m->fetch, m->out_dev, m->count_dev, m->out_cap, out, out_len))) return rc;
    subset_capture_known(capture, m->fetch.count_host[OUT_CAPTURE]);
    return FZB_OK;
}

int fzb_match_list_top_subset_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match* dev_out, size_t capacity,
                                     uint32_t* dev_count, void* stream) {
    if (!m || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    if (m->empty) return fail(FZB_ERR_INVALID, "empty needle: handled on the host by fzb_match_list_top_subset");
    int rc = subset_check(c, in, capture, "fzb_match_list_top_subset_device");
    if (rc) return rc;
    if (c->dev.n == 0 && (rc = subset_capture_trivial(c, in, capture))) return rc;
    SubsetArgs sa{in, capture, nullptr};
    return top_device_impl(m, c, limit, dev_out, capacity, dev_count, stream, &sa);
}

int fzb_match_list_top_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    if (!m || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    if (out_found) *out_found = 0;
    int rc = subset_check(c, in, capture, "fzb_match_list_top_subset");
    if (rc) return rc;
    const size_t n = c->dev.n;
    if (m->empty || n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        if (!in) return fzb_match_list_top(m, c, limit, out, out_len, out_found);
        if (n == 0) return hand_over_matches(std::vector<fzb_match>(), out, out_len);
        return prompt_top_host(m, c, in, limit, out, out_len, out_found);
    }
    const size_t want = std::min(limit, n);
    if ((rc = fzb_ensure_out_staging(m, want))) return rc;
    SubsetArgs sa{in, capture, capture ? m->count_dev + OUT_CAPTURE : nullptr};
    if ((rc = top_device_impl(m, c, limit, (fzb_match*)m->out_dev, m->out_cap, m->count_dev, nullptr, &sa))) return rc;
    if ((rc = fzb_fetch_top(m->fetch_top, m->out_dev, m->count_dev, want, nullptr, out, out_len, out_found))) return rc;
    subset_capture_known(capture, m->fetch_top.count_host[OUT_CAPTURE]);
    return FZB_OK;
}

int fzb_match_list_top_indices_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len,
                                      uint32_t** out_positions, uint64_t* out_found) {
    if (!m || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    clear_indices_out(out, out_len, out_positions, out_found);
    int rc = subset_check(c, in, capture, "fzb_match_list_top_indices_subset");
    if (rc) return rc;
    const size_t n = c->dev.n;
    if (m->empty || n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        if (!in) return fzb_match_list_top_indices(m, c, limit, out, out_len, out_positions, out_found);
        if (n == 0) return hand_over_indices(nullptr, 0, nullptr, 0, out, out_len, out_positions);
        return prompt_top_indices_host(m, c, in, limit, out, out_len, out_positions, out_found);
    }
    return top_indices_host_query(m, c, in, capture, limit, out, out_len, out_positions, out_found);
}

// ---- the empty prompt's _device forms: NEW entry points - the existing _device forms keep refusing an empty needle ---------------------
// what both check before anything is launched (call: the entry point's name)
static int prompt_device_check(const fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, const void* dev_out, size_t capacity, const uint32_t* dev_count, const char* call) {
    if (!m || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    if (!m->empty) return fail(FZB_ERR_INVALID, std::string(call) + ": the matcher's needle is not empty; this call is the empty needle's form of the _device queries");
    if ((u64)c->dev.n > 0xFFFFFFFFull) return refuse_index_overflow(c->dev.n);
    return subset_check(c, in, nullptr, call);
}

int fzb_prompt_list_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, uint32_t index_offset, fzb_match* dev_out, size_t capacity,
                           uint32_t* dev_count, void* stream) {
    int rc = prompt_device_check(m, c, in, dev_out, capacity, dev_count, "fzb_prompt_list_device");
    if (rc) return rc;
    if (first > c->dev.n || count > c->dev.n - first) return fail(FZB_ERR_INVALID, "range outside the corpus");
    if ((u64)count + (u64)index_offset > 0xFFFFFFFFull) return refuse_index_overflow((u64)count + index_offset, index_offset);
    if (in && (first != 0 || count != c->dev.n)) return fail(FZB_ERR_INVALID, "fzb_prompt_list_device: a candidate set is queried over the whole corpus (first = 0, count = its length)");
    hipStream_t st = (hipStream_t)stream;
    if (count == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, st));
        return facets_none(m->facets, st);
    }
    if ((rc = fzb_bind_device(m))) return rc;
    return prompt_list_stage(m, c, in, first, count, index_offset, false, (fzb_match_rec*)dev_out, capacity, dev_count, st);
}

int fzb_prompt_top_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream) {
    int rc = prompt_device_check(m, c, in, dev_out, capacity, dev_count, "fzb_prompt_top_device");
    if (rc) return rc;
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (capacity < want) return refuse_small_output("min(limit, haystacks)", capacity, want);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, st));
        return facets_none(m->facets, st);
    }
    if ((rc = fzb_bind_device(m))) return rc;
    return prompt_top_stage(m, c, in, want, (fzb_match_rec*)dev_out, dev_count, st);
}

// The `from_patterns` form, a host composition of the existing pieces: the multi top goes to the host, then the multi matched-indices
// implementation runs in LIST order over that selection (the head is already in order, so nothing is re-ordered) and `index` is mapped back
// from the position in the selection to the corpus index.
int fzb_multi_match_list_top_indices(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    if (!mm || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_top_indices")) return rc_;
    if (int rc_ = fzb_refuse_biased(c, "fzb_multi_match_list_top_indices", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_scoped(c, "fzb_multi_match_list_top_indices", "fzb_multi_match_list_top_indices_fused")) return rc_;
    if (int rc_ = fzb_refuse_facets(mm ? mm->facets : nullptr, "fzb_multi_match_list_top_indices")) return rc_;
    clear_indices_out(out, out_len, out_positions, out_found);
    fzb_match* head = nullptr;
    size_t nhead = 0;
    uint64_t found = 0;
    int rc = fzb_multi_match_list_top(mm, c, limit, &head, &nhead, &found);
    if (rc) return rc;
    std::vector<u32> sel(nhead);
    for (size_t k = 0; k < nhead; k++) sel[k] = head[k].index;
    std::vector<fzb_match> kept(head, head + nhead);
    fzb_matches_free(head);
    if (out_found) *out_found = found;
    if (nhead == 0) return hand_over_indices(nullptr, 0, nullptr, 0, out, out_len, out_positions);
    if ((rc = multi_match_list_indices_impl(mm, c, sel.data(), nhead, FZB_SORT_INDEX_ASC, 0, out, out_len, out_positions))) return rc;
    bool same = *out_len == nhead;
    for (size_t k = 0; same && k < nhead; k++) {
        fzb_match_indices& r = (*out)[k];
        same = r.index == k && r.score == kept[k].score && (r.exact != 0) == (kept[k].exact != 0);
        r.index = sel[k];
    }
    if (!same) {
        fzb_match_indices_free(*out, *out_positions);
        *out = nullptr;
        *out_positions = nullptr;
        *out_len = 0;
        return fail(FZB_ERR_HIP, "internal: the matched-indices pass disagrees with the top stage");
    }
    return FZB_OK;
}

// ---- the `from_patterns` form fused on the device --------------------------------------------------------------------------------
// The multi top stage leaves its sorted head in HBM (mm->top.head), k_top_items makes it ONE item list, every positive pattern's sub-matcher
// runs the traced pipeline over that list into its own trace buffers (records in head order: every pattern accepts every haystack of the
// head, which is what the composition selected), k_multi_union puts the patterns' records and positions together per head record
// (indices_union.h: match_one_indices_multi, src/matcher/multi.rs:56-82) and the pack kernels write the caller's result while holding the
// combined records to the head.  Negated patterns are not traced: the head holds no haystack they hit.  Nothing is read back in between.
// CompiledPatterns::Single takes the same path with one source: its sub-matcher runs IndexAsc and owns neither sort buffers nor staging, so
// the ordering is the multi top stage's here too.
}  // extern "C"
namespace {
// positive patterns and U = the union's stride: every pattern's positions side by side
size_t multi_union_stride(const fzb_multi_matcher* mm, size_t* positive) {
    size_t U = 0, P = 0;
    for (const auto& p : mm->patterns)
        if (!p.negated) {
            U += trace_stride(p.m);
            P++;
        }
    if (positive) *positive = P;
    return U;
}
// the composition's own buffers of a fused query: a head of up to `want` records, unions of U dwords, P sources; staging: the host form's too
int ensure_multi_top_indices_buffers(fzb_multi_matcher* mm, size_t want, size_t U, size_t P, bool staging) {
    int rc;
    if (!mm->top_words) HIPCHK(dev_alloc((void**)&mm->top_words, MTOP_WORDS * sizeof(u32)));
    if (!mm->top_comb || !mm->top_items || !mm->top_npos_u || mm->top_rec_cap < want) {
        mm->top_rec_cap = 0;
        if ((rc = fzb_dev_renew(&mm->top_comb, want + 16)) || (rc = fzb_dev_renew(&mm->top_items, want + 4)) || (rc = fzb_dev_renew(&mm->top_npos_u, want + 4))) return rc;
        mm->top_rec_cap = want;
    }
    if ((rc = fzb_grow_dev(&mm->top_pos_u, &mm->top_pos_u_words, want * U, 1))) return rc;
    if (P > IUNION_BY_VALUE) {
        if (!mm->union_src || mm->union_src_cap < P) mm->union_src_host.clear();  // (a new array holds nothing yet)
        if ((rc = fzb_grow_dev(&mm->union_src, &mm->union_src_cap, P)) || (rc = fzb_grow_dev(&mm->union_cursors, &mm->union_cursor_words, want * P, 1))) return rc;
    }
    return fzb_top_ensure(mm->top, want, want * U, staging);
}
bool same_union_src(const IUnionSrc& a, const IUnionSrc& b) { return a.rec == b.rec && a.count == b.count && a.npos == b.npos && a.pos == b.pos && a.stride == b.stride; }
// a matcher that has an any-of group (indices_union_groups.h): what its union is made of
struct GroupShape {
    size_t U = 0;  // U_g: the plain non-negated patterns' strides + per group the largest stride among its alternatives
    size_t P = 0;  // sources: plain non-negated patterns + alternatives
    size_t A = 0;  // alternatives in groups
};
GroupShape multi_group_shape(const fzb_multi_matcher* mm) {
    GroupShape g;
    const auto& ps = mm->patterns;
    for (size_t i = 0; i < ps.size();) {
        size_t e = i + 1;
        while (e < ps.size() && mm->terms.size() == ps.size() && mm->terms[e] == mm->terms[i]) e++;
        if (!ps[i].negated) {  // (a group has no negated alternative)
            size_t widest = 0;
            for (size_t p = i; p < e; p++) widest = std::max<size_t>(widest, trace_stride(ps[p].m));
            g.U += widest;
            g.P += e - i;
            if (e - i >= 2) g.A += e - i;
        }
        i = e;
    }
    return g;
}
size_t gunion_where_stride(size_t want) { return (want + 3) & ~(size_t)3; }  // (the clear stores whole 16-byte words)
// the grouped tail's own buffers for heads of up to `want` records, A alternatives and P sources
int ensure_gunion_buffers(fzb_multi_matcher* mm, size_t want, size_t A, size_t P) {
    int rc;
    if ((rc = fzb_grow_dev(&mm->gunion_where, &mm->gunion_where_words, std::max<size_t>(A * gunion_where_stride(want), 4), 16))) return rc;
    if (P > IUNION_BY_VALUE) {
        if (!mm->gunion_src || mm->gunion_src_cap < P) mm->gunion_src_host.clear();  // (a new array holds nothing yet)
        if ((rc = fzb_grow_dev(&mm->gunion_src, &mm->gunion_src_cap, P)) || (rc = fzb_grow_dev(&mm->gunion_scratch, &mm->gunion_scratch_words, want * 3 * P, 1))) return rc;
    }
    return FZB_OK;
}
bool same_gunion_src(const GUnionSrc& a, const GUnionSrc& b) { return same_union_src(a.s, b.s) && a.where == b.where && a.term == b.term; }
}  // namespace
extern "C" {

int fzb_multi_matcher_groups_positions_stride(const fzb_multi_matcher* mm, size_t* out) {
    if (!mm || !out) return fail(FZB_ERR_INVALID, "null argument");
    *out = mm->grouped ? multi_group_shape(mm).U : multi_union_stride(mm, nullptr);
    return FZB_OK;
}

// every buffer of the grouped query and its sources, final before anything is launched (uploaded beyond IUNION_BY_VALUE)
static int multi_top_indices_group_sources(fzb_multi_matcher* mm, size_t want, const GroupShape& g, std::vector<GUnionSrc>* src, hipStream_t st) {
    int rc;
    if ((rc = ensure_multi_top_indices_buffers(mm, want, g.U, 0, false)) || (rc = ensure_gunion_buffers(mm, want, g.A, g.P))) return rc;
    src->clear();
    src->reserve(g.P);
    auto& ps = mm->patterns;
    size_t a = 0;
    for (size_t i = 0; i < ps.size(); i++) {
        if (ps[i].negated) continue;
        fzb_matcher* m = ps[i].m;
        if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, trace_stride(m), false))) return rc;
        const bool alt = (i > 0 && mm->terms[i - 1] == mm->terms[i]) || (i + 1 < ps.size() && mm->terms[i + 1] == mm->terms[i]);
        const u32* where = alt ? mm->gunion_where + (a++) * gunion_where_stride(want) : nullptr;
        src->push_back(GUnionSrc{IUnionSrc{(const IUnionRec*)m->top_traced, m->top_idx_words + TOPIDX_TRACED, m->trace_npos, m->trace_pos, trace_stride(m), 0}, where, mm->terms[i], 0});
    }
    if (g.P > IUNION_BY_VALUE) {
        bool same = mm->gunion_src_host.size() == g.P;
        for (size_t i = 0; same && i < g.P; i++) same = same_gunion_src(mm->gunion_src_host[i], (*src)[i]);
        if (!same) {  // (a pattern, a grouping or a buffer changed since the array was written: ahead of the first launch, ordered on the stream)
            mm->gunion_src_host = *src;
            HIPCHK(hipMemcpyAsync(mm->gunion_src, mm->gunion_src_host.data(), g.P * sizeof(GUnionSrc), hipMemcpyHostToDevice, st));
        }
    }
    return FZB_OK;
}

// The two halves every fused "head + matched positions" query of the composition shares.  Ahead of the first launch: the composition's and every
// positive pattern's buffers for a head of up to `want` records, and the sources of the union (uploaded beyond IUNION_BY_VALUE).
static int multi_top_indices_sources(fzb_multi_matcher* mm, size_t want, size_t U, size_t P, std::vector<IUnionSrc>* src, hipStream_t st) {
    int rc;
    if ((rc = ensure_multi_top_indices_buffers(mm, want, U, P, false))) return rc;
    src->clear();
    src->reserve(P);
    for (auto& p : mm->patterns) {
        if (p.negated) continue;
        fzb_matcher* m = p.m;
        if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, trace_stride(m), false))) return rc;
        src->push_back(IUnionSrc{(const IUnionRec*)m->top_traced, m->top_idx_words + TOPIDX_TRACED, m->trace_npos, m->trace_pos, trace_stride(m), 0});
    }
    if (P > IUNION_BY_VALUE) {
        bool same = mm->union_src_host.size() == P;
        for (size_t i = 0; same && i < P; i++) same = same_union_src(mm->union_src_host[i], (*src)[i]);
        if (!same) {  // (a pattern or a buffer changed since the array was written: ahead of the first launch, ordered on the stream)
            mm->union_src_host = *src;
            HIPCHK(hipMemcpyAsync(mm->union_src, mm->union_src_host.data(), P * sizeof(IUnionSrc), hipMemcpyHostToDevice, st));
        }
    }
    return FZB_OK;
}
// Behind the head (mm->top.head, its pair in mm->top_words) and its item list (mm->top_items, the length at word MTOP_N_ITEMS of them; k_top_items, or
// k_sec_items for sectioned heads): one traced pass per positive pattern, the union, the bias, the pack and four words at dev_count.
// gt (a matcher that has an any-of group, U = U_g): the traced passes are the same - one per plain non-negated pattern and per alternative, an
// alternative's returning only the head items it matches - and fzb_launch_gunion's four launches stand in place of k_multi_union.
// `group_slots` serves as its haystack -> head position map: the composition has finished with it, and multi_compose_groups sized it for the
// haystacks of the list (multi_ensure_buffers(count), also over a candidate set), not for a set's items.
struct GroupedTail {
    const GroupShape* shape;
    const std::vector<GUnionSrc>* src;
    size_t n_hay;
};
static int multi_top_indices_tail(fzb_multi_matcher* mm, const fzb_corpus* c, size_t want, size_t U, const std::vector<IUnionSrc>& src, fzb_match_indices* dev_out, size_t capacity,
                                  uint32_t* dev_positions, size_t positions_capacity, uint32_t* dev_count, void* stream, const GroupedTail* gt = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    u32* const head_count = mm->top_words + MTOP_HEAD;
    u32* const comb_count = mm->top_words + MTOP_COMBINED;  // the combined traced pair
    u32* const n_items = mm->top_words + MTOP_N_ITEMS;
    const int grid = mm->num_cus * 2;
    int rc;
    for (auto& p : mm->patterns) {
        if (p.negated) continue;
        fzb_matcher* m = p.m;
        const TraceOut tr{m->trace_pos, m->trace_npos, trace_stride(m)};
        if ((rc = run_pipeline(m, c, 0, want, 0, mm->top_items, n_items, (fzb_match*)m->top_traced, want, m->top_idx_words + TOPIDX_TRACED, stream, &tr))) return rc;
    }
    if (gt) {
        if (!mm->group_slots || mm->group_cap < gt->n_hay) return fail(FZB_ERR_HIP, "internal: the group slots do not cover the list");
        fzb_launch_gunion(mm->top.head, head_count, (u32)want, gt->src->data(), (u32)gt->src->size(), mm->gunion_src, mm->gunion_scratch, mm->group_slots, (u32)gt->n_hay, mm->gunion_where,
                          gt->shape->A * gunion_where_stride(want), mm->top_comb, comb_count, mm->top_npos_u, mm->top_pos_u, (u32)U, grid, st);
    } else {
        fzb_launch_multi_union(mm->top.head, head_count, (u32)want, src.data(), (u32)src.size(), mm->union_src, mm->union_cursors, mm->top_comb, comb_count, mm->top_npos_u, mm->top_pos_u,
                               (u32)U, grid, st);
    }
    if ((rc = apply_bias(c, mm->top_comb, comb_count, want, 0, 0, grid, st))) return rc;  // once, after the sum: as the head's records
    fzb_launch_indices_pack(mm->top.head, head_count, mm->top_comb, comb_count, mm->top_npos_u, mm->top_pos_u, (u32)U, (fzb_indices_rec*)dev_out, (u32)std::min<size_t>(capacity, 0xFFFFFFFFu),
                            dev_positions, (u32)std::min<size_t>(positions_capacity, 0xFFFFFFFFu), dev_count, mm->top.tiles, (u32)want, grid, st);
    HIPCHK(hipGetLastError());
    return FZB_OK;
}

// (sa: only the top stage sees the candidate set and captures; the traced passes run over the head's item list as before)
static int multi_top_indices_device_impl(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions,
                                         size_t positions_capacity, uint32_t* dev_count, void* stream, const SubsetArgs* sa) {
    if (!mm || !c || !dev_count || (!dev_out && capacity) || (!dev_positions && positions_capacity)) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (capacity < want) return refuse_small_output("min(limit, haystacks)", capacity, want);
    if (mm->patterns.empty()) return fail(FZB_ERR_INVALID, "no pattern: handled on the host by fzb_multi_match_list_top_indices_fused");
    size_t P = 0;
    // (a matcher that has an any-of group gets here through fzb_multi_match_list_top_indices_groups* alone: its stride is U_g)
    const GroupShape shape = mm->grouped ? multi_group_shape(mm) : GroupShape{};
    const size_t U = mm->grouped ? shape.U : multi_union_stride(mm, &P);
    if (positions_capacity < want * U) return refuse_small_positions("min(limit, haystacks)", positions_capacity, want * U);
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    if ((u64)want * U > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(dev_count, 0, PACK_WORDS * sizeof(u32), st));
        return facets_none(mm->facets, st);
    }
    // every buffer first: the sources of the union are final before anything is launched
    int rc;
    std::vector<IUnionSrc> src;
    std::vector<GUnionSrc> group_src;
    const GroupedTail gt{&shape, &group_src, n};
    if (mm->grouped) {
        if ((rc = multi_top_indices_group_sources(mm, want, shape, &group_src, st))) return rc;
    } else if ((rc = multi_top_indices_sources(mm, want, U, P, &src, st))) {
        return rc;
    }
    u32* const head_count = mm->top_words + MTOP_HEAD;  // (records, matches found) of the head
    u32* const n_items = mm->top_words + MTOP_N_ITEMS;
    // (the composition's pair at MTOP_RAW: MTOP_CAPTURE follows the host form's result words, where its wait picks up a captured count)
    if ((rc = multi_top_stage(mm, c, n, want, mm->top.head, head_count, mm->top_words + MTOP_RAW, st, sa))) return rc;
    const int grid = mm->num_cus * 2;
    fzb_launch_top_items(mm->top.head, head_count, (u32)want, mm->top_items, n_items, dev_count, (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, (want + 255) / 256)), st);
    return multi_top_indices_tail(mm, c, want, U, src, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, mm->grouped ? &gt : nullptr);
}
int fzb_multi_match_list_top_indices_device(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions,
                                            size_t positions_capacity, uint32_t* dev_count, void* stream) {
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_top_indices_device")) return rc_;
    return multi_top_indices_device_impl(mm, c, limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, nullptr);
}
// what the composition's host forms - fused, over a candidate set, with any-of groups - do behind their trivial branches (a pattern, a corpus
// that is not empty), for unions of U dwords from P sources: in / capture as the caller gave them, and no SubsetArgs at all without either
static int multi_top_indices_host_query(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, size_t U, size_t P, fzb_match_indices** out,
                                        size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    const size_t want = std::min(limit, (size_t)c->dev.n);
    if (int rc = ensure_multi_top_indices_buffers(mm, want, U, P, false)) return rc;
    HostWords w{mm->top_words + MTOP_RESULT, PACK_WORDS + (capture ? 1 : 0), 0, MTOP_CAPTURE - MTOP_RESULT};
    auto impl = [&](const PackedOut& o) {
        const SubsetArgs sa{in, capture, o.mirror};
        return multi_top_indices_device_impl(mm, c, limit, o.recs, o.cap, o.pos, o.pos_cap, o.words, nullptr, (in || capture) ? &sa : nullptr);
    };
    return top_indices_host(mm->top, w, want, want * U, capture, "the traced passes disagree with the multi top stage", impl, out, out_len, out_positions, out_found);
}

// (in / capture: as the _subset form got them, null from the fused form.  A no-pattern matcher never gets here with a subset.)
static int multi_top_indices_fused_impl(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found,
                                        const fzb_subset* in, fzb_subset* capture) {
    if (!mm || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    clear_indices_out(out, out_len, out_positions, out_found);
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (mm->patterns.empty() || n == 0) {
        if (int rc_ = facets_every(mm->facets, c, 0, n, "fzb_multi_match_list_top_indices_fused")) return rc_;
    }
    if (mm->patterns.empty()) return empty_top_indices(c, n, mm->config.sort, limit, out, out_len, out_positions, out_found);  // CompiledPatterns::Empty
    if (n == 0) return hand_over_indices(nullptr, 0, nullptr, 0, out, out_len, out_positions);
    size_t P = 0;
    const size_t U = multi_union_stride(mm, &P);
    if ((u64)want * U > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    return multi_top_indices_host_query(mm, c, in, capture, limit, U, P, out, out_len, out_positions, out_found);
}
int fzb_multi_match_list_top_indices_fused(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_top_indices_fused")) return rc_;
    return multi_top_indices_fused_impl(mm, c, limit, out, out_len, out_positions, out_found, nullptr, nullptr);
}

// ---- candidate sets on the `from_patterns` forms -----------------------------------------------------------------------------------------
// The single-matcher forms' contract for the composition: the query over `in` returns what it returns over a corpus of those haystacks alone,
// `capture` receives the haystacks the COMPOSITION accepted (every non-negated pattern hit, no negated one did), taken ahead of bias, scope,
// selection and ordering.  A matcher with no compiled pattern accepts every haystack of `in`: the capture is `in` itself (subset_capture_trivial)
// and the query runs with the input alone.
int fzb_multi_match_list_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_match** out, size_t* out_len) {
    if (!mm || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_subset");
    if (rc) return rc;
    if (mm->patterns.empty() || c->dev.n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        capture = nullptr;
    }
    if (!in && !capture) return fzb_multi_match_list(mm, c, out, out_len);
    if ((rc = fzb_out_ensure(*mm, c->dev.n))) return rc;
    SubsetArgs sa{in, capture, capture ? mm->count_dev + OUT_CAPTURE : nullptr};
    if ((rc = multi_match_list_impl(mm, c, out, out_len, &sa))) return rc;
    subset_capture_known(capture, mm->fetch.count_host[OUT_CAPTURE]);
    return FZB_OK;
}

int fzb_multi_match_list_top_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match** out, size_t* out_len,
                                    uint64_t* out_found) {
    if (!mm || !c || !out || !out_len) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_len = 0;
    if (out_found) *out_found = 0;
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_top_subset");
    if (rc) return rc;
    if (mm->patterns.empty() || c->dev.n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        capture = nullptr;
    }
    if (!in && !capture) return fzb_multi_match_list_top(mm, c, limit, out, out_len, out_found);
    if ((rc = fzb_out_ensure(*mm, std::min(limit, (size_t)c->dev.n)))) return rc;
    SubsetArgs sa{in, capture, capture ? mm->count_dev + OUT_CAPTURE : nullptr};
    if ((rc = multi_match_list_top_impl(mm, c, limit, out, out_len, out_found, &sa))) return rc;
    subset_capture_known(capture, mm->fetch_top.count_host[OUT_CAPTURE]);
    return FZB_OK;
}

int fzb_multi_match_list_top_subset_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match* dev_out, size_t capacity,
                                           uint32_t* dev_count, void* stream) {
    if (!mm || !c || !dev_count || (!dev_out && capacity)) return fail(FZB_ERR_INVALID, "null argument");
    if (mm->patterns.empty()) return fail(FZB_ERR_INVALID, "no pattern: handled on the host by fzb_multi_match_list_top_subset");
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_top_subset_device");
    if (rc) return rc;
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (capacity < want) return refuse_small_output("min(limit, haystacks)", capacity, want);
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    if (n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        HIPCHK(hipMemsetAsync(dev_count, 0, 8, (hipStream_t)stream));
        return FZB_OK;
    }
    if ((rc = fzb_out_ensure(*mm, 0))) return rc;  // (the composition's pair lives next to the staging's count words)
    SubsetArgs sa{in, capture, nullptr};
    return multi_top_stage(mm, c, n, want, (fzb_match_rec*)dev_out, dev_count, mm->count_dev + OUT_RAW, (hipStream_t)stream, &sa);
}

// ---- sectioned top-`limit`: the best matches per tag section, one device call (sections.h, kernels_sections.hip) ---------------------------
// The reference has no such call: a picker with sections splits the Vec `match_list` returned.  Element s = fzb_match_list_top over the
// corpus' own scope AND section s's predicate.  The producers are the top stages' own (top_produce, prompt_records, the composition): their
// index-ordered records - behind capture, facets, the corpus' scope drop and the bias - sit in the sort's second buffer, and the sectioned
// stage replaces the selection and the radix sort.  Nothing is read back between the stages; the host forms make one copy and one wait.
}  // extern "C"
namespace {
static_assert(SECTIONS_MAX == FZB_SECTIONS_MAX && SECTIONS_LIMIT_MAX == FZB_SECTION_LIMIT_MAX, "include/frizbee_hip.h states the limits of sections.h");
// what every sectioned entry point checks before anything touches the device
int sections_check(const void* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture, const char* call,
                   sections_set* ss) {
    if (!m || !c || (!sections && n_sections)) return fail(FZB_ERR_INVALID, "null argument");
    if (n_sections > FZB_SECTIONS_MAX) return fail(FZB_ERR_INVALID, std::string(call) + ": " + std::to_string(n_sections) + " sections; at most FZB_SECTIONS_MAX = 8 in one call");
    if (limit > FZB_SECTION_LIMIT_MAX) return fail(FZB_ERR_INVALID, std::string(call) + ": limit " + std::to_string(limit) + " is above FZB_SECTION_LIMIT_MAX = 1024");
    if ((u64)c->dev.n > 0xFFFFFFFFull) return refuse_index_overflow(c->dev.n);
    *ss = sections_set{};
    ss->n = (u32)n_sections;
    for (size_t s = 0; s < n_sections; s++) {
        ss->require[s] = sections[s].require;
        ss->exclude[s] = sections[s].exclude;
    }
    return subset_check(c, in, capture, call);
}
// the per-section out-parameters of the host forms, cleared ahead of everything that can fail
void sections_clear_out(size_t n_sections, size_t* out_len, uint64_t* out_found) {
    for (size_t s = 0; s < n_sections; s++) {
        out_len[s] = 0;
        if (out_found) out_found[s] = 0;
    }
}
// an empty corpus: S empty heads
int sections_nothing(const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_facets* f, size_t n_sections, u32* dev_counts, hipStream_t st) {
    if (int rc = subset_capture_trivial(c, in, capture)) return rc;
    if (n_sections) HIPCHK(hipMemsetAsync(dev_counts, 0, 2 * n_sections * sizeof(u32), st));
    return facets_none(f, st);
}
// the stage on `st` behind a producer: slab s of dev_out = the ordered head of section s, dev_counts = the 2S result words
int sections_stage(SectionsScratch& sc, const fzb_corpus* c, const fzb_match_rec* recs, const u32* raw_count, size_t n, const sections_set& ss, size_t limit, bool by_score,
                   bool reversed, bool one_pass, fzb_match_rec* dev_out, u32* dev_counts, int grid, hipStream_t st) {
    if (int rc = fzb_sections_ensure(sc, n, 0)) return rc;
    HIPCHK(fzb_launch_sections_select(recs, raw_count, (u32)n, c->tags.data, c->dev.n, ss, (u32)limit, by_score, reversed, one_pass, dev_out, dev_counts, sc.words,
                                      (u32)(n / SECTIONS_TILE + 2), grid, st));
    return FZB_OK;
}
int single_sections_stage(fzb_matcher* m, const fzb_corpus* c, const sections_set& ss, size_t limit, const SubsetArgs* sa, fzb_match_rec* dev_out, u32* dev_counts, hipStream_t st) {
    const size_t n = c->dev.n;
    int rc;
    if ((rc = facets_check(m->facets, c, "fzb_match_list_top_sections"))) return rc;
    if (n == 0) return sections_nothing(c, sa->in, sa->capture, m->facets, ss.n, dev_counts, st);
    bool reversed, by_score, one_pass;
    u32* raw_count = nullptr;
    if (m->empty) {  // the empty prompt: every visible haystack of the input, score = the clamped bias (prompt_records)
        if ((rc = subset_capture_trivial(c, sa->in, sa->capture))) return rc;
        if ((rc = fzb_bind_device(m)) || (rc = fzb_ensure_sort_buffers(m, n))) return rc;
        if (!m->count_dev && (rc = fzb_ensure_out_staging(m, 0))) return rc;
        prompt_order_flags(m, c, &reversed, &by_score, &one_pass);
        raw_count = m->count_dev + OUT_RAW;
        if ((rc = prompt_records(m, c, sa->in, 0, n, 0, m->ws.sort.tmp, n, raw_count, st))) return rc;
    } else if ((rc = top_produce(m, c, n, st, sa, &raw_count, &reversed, &by_score, &one_pass))) {
        return rc;
    }
    if (ss.n == 0) return FZB_OK;
    return sections_stage(m->sections, c, m->ws.sort.tmp, raw_count, n, ss, limit, by_score, reversed, one_pass, dev_out, dev_counts, m->lc.num_cus * 2, st);
}
// (the composition's producer as multi_top_stage runs it; summed scores pass 255: never one level)
int multi_sections_stage(fzb_multi_matcher* mm, const fzb_corpus* c, const sections_set& ss, size_t limit, const SubsetArgs* sa, fzb_match_rec* dev_out, u32* dev_counts, hipStream_t st) {
    const size_t n = c->dev.n;
    int rc;
    if ((rc = facets_check(mm->facets, c, "fzb_multi_match_list_top_sections"))) return rc;
    if (n == 0) return sections_nothing(c, sa->in, sa->capture, mm->facets, ss.n, dev_counts, st);
    SubsetArgs args = *sa;
    if (mm->patterns.empty()) {  // no pattern accepts every haystack of the input: the capture is the input itself
        if ((rc = subset_capture_trivial(c, args.in, args.capture))) return rc;
        args.capture = nullptr;
    }
    if ((rc = fzb_out_ensure(*mm, 0)) || (rc = fzb_sort_ensure(mm->sort, n))) return rc;  // (the composition's pair lives next to the staging's count words)
    u32* const raw_count = mm->count_dev + OUT_RAW;
    if ((rc = multi_match_list_device_impl(mm, c, 0, n, 0, (fzb_match*)mm->sort.tmp, n, raw_count, st, &args))) return rc;
    bool reversed, by_score;
    multi_order_flags(mm, c, &reversed, &by_score);
    if (ss.n == 0) return FZB_OK;
    return sections_stage(mm->sections, c, mm->sort.tmp, raw_count, n, ss, limit, by_score, reversed, false, dev_out, dev_counts, mm->num_cus * 2, st);
}
// The host forms' result: the stage block - SEC_STAGE_RECORDS words (the 2S counts, the captured count), then S slabs of `limit` records - in
// ONE copy and one wait on the null stream; the heads are moved together in the pinned block that is handed over.
int sections_fetch(const SectionsScratch& sc, size_t S, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found, u32* captured) {
    const size_t bytes = SEC_STAGE_RECORDS * sizeof(u32) + S * limit * sizeof(fzb_match);
    uint8_t* r = (uint8_t*)pinned_pool().get(bytes);
    if (!r) return fail(FZB_ERR_HIP, "hipHostMalloc failed for the result list");
    hipError_t e = hipMemcpyAsync(r, sc.stage, bytes, hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess) e = fzb_stream_wait(nullptr);
    if (e != hipSuccess) {
        pinned_pool().put(r);
        return fail(FZB_ERR_HIP, std::string("device to host: ") + hipGetErrorString(e));
    }
    u32 words[SEC_STAGE_RECORDS];  // (the words in front of the records)
    memcpy(words, r, sizeof(words));
    size_t total = 0;
    for (size_t s = 0; s < S; s++) {  // (head s moves towards the front: its destination ends before any later slab begins)
        const size_t kept = std::min<size_t>(words[SEC_STAGE_COUNTS + 2 * s], limit);
        memmove(r + total * sizeof(fzb_match), r + sizeof(words) + s * limit * sizeof(fzb_match), kept * sizeof(fzb_match));
        out_len[s] = kept;
        if (out_found) out_found[s] = words[SEC_STAGE_COUNTS + 2 * s + 1];
        total += kept;
    }
    *captured = words[SEC_STAGE_CAPTURE];
    *out = (fzb_match*)r;
    return FZB_OK;
}
}  // namespace
extern "C" {

int fzb_match_list_top_sections_device(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                       fzb_match* dev_out, size_t capacity, uint32_t* dev_counts, void* stream) {
    sections_set ss;
    if ((!dev_counts && n_sections) || (!dev_out && n_sections && limit)) return fail(FZB_ERR_INVALID, "null argument");
    if (int rc = sections_check(m, c, sections, n_sections, limit, in, capture, "fzb_match_list_top_sections_device", &ss)) return rc;
    if (capacity < n_sections * limit) return refuse_small_output("n_sections * limit", capacity, n_sections * limit);
    SubsetArgs sa{in, capture, nullptr};
    return single_sections_stage(m, c, ss, limit, &sa, (fzb_match_rec*)dev_out, dev_counts, (hipStream_t)stream);
}

int fzb_match_list_top_sections(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                fzb_match** out, size_t* out_len, uint64_t* out_found) {
    sections_set ss;
    if (!out || (!out_len && n_sections)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = sections_check(m, c, sections, n_sections, limit, in, capture, "fzb_match_list_top_sections", &ss)) return rc;
    sections_clear_out(n_sections, out_len, out_found);
    int rc;
    if ((rc = fzb_bind_device(m)) || (rc = fzb_sections_ensure(m->sections, c->dev.n, n_sections * limit + 1))) return rc;
    u32* const words = m->sections.stage;
    SubsetArgs sa{in, capture, capture ? words + SEC_STAGE_CAPTURE : nullptr};
    if ((rc = single_sections_stage(m, c, ss, limit, &sa, (fzb_match_rec*)(words + SEC_STAGE_RECORDS), words + SEC_STAGE_COUNTS, nullptr))) return rc;
    if (n_sections == 0 || c->dev.n == 0) return FZB_OK;
    u32 captured = 0;
    if ((rc = sections_fetch(m->sections, n_sections, limit, out, out_len, out_found, &captured))) return rc;
    if (!m->empty) subset_capture_known(capture, captured);
    return FZB_OK;
}

int fzb_multi_match_list_top_sections_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                             fzb_subset* capture, fzb_match* dev_out, size_t capacity, uint32_t* dev_counts, void* stream) {
    sections_set ss;
    if ((!dev_counts && n_sections) || (!dev_out && n_sections && limit)) return fail(FZB_ERR_INVALID, "null argument");
    if (int rc = sections_check(mm, c, sections, n_sections, limit, in, capture, "fzb_multi_match_list_top_sections_device", &ss)) return rc;
    if (capacity < n_sections * limit) return refuse_small_output("n_sections * limit", capacity, n_sections * limit);
    SubsetArgs sa{in, capture, nullptr};
    return multi_sections_stage(mm, c, ss, limit, &sa, (fzb_match_rec*)dev_out, dev_counts, (hipStream_t)stream);
}

int fzb_multi_match_list_top_sections(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                      fzb_subset* capture, fzb_match** out, size_t* out_len, uint64_t* out_found) {
    sections_set ss;
    if (!out || (!out_len && n_sections)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = sections_check(mm, c, sections, n_sections, limit, in, capture, "fzb_multi_match_list_top_sections", &ss)) return rc;
    sections_clear_out(n_sections, out_len, out_found);
    int rc;
    if ((rc = fzb_sections_ensure(mm->sections, c->dev.n, n_sections * limit + 1))) return rc;
    u32* const words = mm->sections.stage;
    const bool captures = capture && !mm->patterns.empty();
    SubsetArgs sa{in, capture, captures ? words + SEC_STAGE_CAPTURE : nullptr};
    if ((rc = multi_sections_stage(mm, c, ss, limit, &sa, (fzb_match_rec*)(words + SEC_STAGE_RECORDS), words + SEC_STAGE_COUNTS, nullptr))) return rc;
    if (n_sections == 0 || c->dev.n == 0) return FZB_OK;
    u32 captured = 0;
    if ((rc = sections_fetch(mm->sections, n_sections, limit, out, out_len, out_found, &captured))) return rc;
    if (captures) subset_capture_known(capture, captured);
    return FZB_OK;
}

// ---- sectioned top-`limit` WITH matched positions: one fused device call ---------------------------------------------------------------------
// Element s = fzb_match_list_top_indices over the corpus' own scope AND section s's predicate.  The sectioned stage runs as above, into slabs of
// the matcher's own (SectionsScratch::slabs); k_sec_items makes the slabs ONE dense head of up to n_sections * min(limit, haystacks) records with
// its item list, and from there the fused queries' tail runs unchanged (top_indices_tail / multi_top_indices_tail): the traced pass(es) over the
// items, the union, the bias, the pack.  A haystack that sits in several sections is an item several times and is traced once per section.
}  // extern "C"
namespace {
// what the _device forms check behind sections_check; *want = the records the dense head has room for
int sections_indices_room(size_t n_sections, size_t limit, size_t n, size_t stride, size_t capacity, size_t positions_capacity, size_t* want) {
    *want = n_sections * std::min(limit, n);
    if (capacity < *want) return refuse_small_output("n_sections * min(limit, haystacks)", capacity, *want);
    if (positions_capacity < *want * stride) return refuse_small_positions("n_sections * min(limit, haystacks)", positions_capacity, *want * stride);
    if ((u64)*want * stride > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "n_sections * min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    return FZB_OK;
}
// the host forms' answer where no positions exist (an empty needle, no pattern) or nothing is selected (no section, an empty corpus): the
// sectioned call's records with empty position lists
int sections_indices_plain(fzb_match* head, size_t n_sections, const size_t* out_len, fzb_match_indices** out, uint32_t** out_positions) {
    size_t total = 0;
    for (size_t s = 0; s < n_sections; s++) total += out_len[s];
    std::vector<fzb_match_indices> recs(total);
    for (size_t i = 0; i < total; i++) recs[i] = fzb_match_indices{head[i].index, head[i].score, head[i].exact, 0, 0, 0};
    if (head) fzb_matches_free(head);
    size_t len = 0;
    return hand_over_indices(recs.data(), total, nullptr, 0, out, &len, out_positions);
}
// the sectioned host forms' tail (top_indices_host): their one wait brings the 2S + PACK_WORDS result words and the captured count, the dense
// head and the dense positions; the sections' counts are handed out from the words
template <typename Impl>
int sections_indices_host(TopStaging& t, SectionsScratch& sc, size_t S, size_t want, size_t max_pos, fzb_subset* capture, const char* disagree, Impl&& impl, fzb_match_indices** out,
                          size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    HostWords w{sc.slabs + SEC_SLAB_RESULT, SEC_SLAB_FETCH, 2 * S, SEC_SLAB_CAPTURE - SEC_SLAB_RESULT};
    size_t total = 0;
    if (int rc = top_indices_host(t, w, want, max_pos, capture, disagree, impl, out, &total, out_positions, nullptr)) return rc;
    for (size_t s = 0; s < S; s++) {
        out_len[s] = w.host[2 * s];
        if (out_found) out_found[s] = w.host[2 * s + 1];
    }
    return FZB_OK;
}
}  // namespace
extern "C" {

// (mirror: where the host form's wait picks up the captured count, or null)
static int sections_indices_device_impl(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                        u32* mirror, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity, uint32_t* dev_counts, void* stream) {
    sections_set ss;
    if (!dev_counts || (!dev_out && capacity) || (!dev_positions && positions_capacity)) return fail(FZB_ERR_INVALID, "null argument");
    int rc;
    if ((rc = sections_check(m, c, sections, n_sections, limit, in, capture, "fzb_match_list_top_sections_indices_device", &ss))) return rc;
    if (m->empty) return fail(FZB_ERR_INVALID, "empty needle: handled on the host by fzb_match_list_top_sections_indices");
    const size_t n = c->dev.n;
    const u32 stride = trace_stride(m);
    size_t want;
    if ((rc = sections_indices_room(n_sections, limit, n, stride, capacity, positions_capacity, &want))) return rc;
    hipStream_t st = (hipStream_t)stream;
    SubsetArgs sa{in, capture, mirror};
    if (n == 0 || n_sections == 0) {  // nothing to select: the sectioned call's side effects (capture, facets), 2S + 4 zero words
        if ((rc = single_sections_stage(m, c, ss, limit, &sa, nullptr, dev_counts, st))) return rc;
        HIPCHK(hipMemsetAsync(dev_counts + 2 * n_sections, 0, PACK_WORDS * sizeof(u32), st));
        return FZB_OK;
    }
    if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, stride, false)) || (rc = fzb_sections_ensure_slabs(m->sections, n_sections * limit))) return rc;
    u32* const slab_counts = m->sections.slabs + SEC_SLAB_COUNTS;
    fzb_match_rec* const slabs = (fzb_match_rec*)(m->sections.slabs + SECTIONS_SLAB_WORDS);
    if ((rc = single_sections_stage(m, c, ss, limit, &sa, slabs, slab_counts, st))) return rc;
    fzb_launch_sections_items(slabs, slab_counts, (u32)n_sections, (u32)limit, (u32)want, m->top.head, m->top_idx_words + TOPIDX_HEAD, m->trace_sel, m->trace_sel + m->trace_cap, dev_counts,
                              m->lc.num_cus * 2, st);
    return top_indices_tail(m, c, want, stride, dev_out, capacity, dev_positions, positions_capacity, dev_counts + 2 * n_sections, stream);
}

int fzb_match_list_top_sections_indices_device(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                               fzb_subset* capture, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                               uint32_t* dev_counts, void* stream) {
    return sections_indices_device_impl(m, c, sections, n_sections, limit, in, capture, nullptr, dev_out, capacity, dev_positions, positions_capacity, dev_counts, stream);
}

int fzb_match_list_top_sections_indices(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                        fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    sections_set ss;
    if (!out || !out_positions || (!out_len && n_sections)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_positions = nullptr;
    int rc;
    if ((rc = sections_check(m, c, sections, n_sections, limit, in, capture, "fzb_match_list_top_sections_indices", &ss))) return rc;
    const size_t n = c->dev.n;
    if (m->empty || n == 0 || n_sections == 0) {
        fzb_match* head = nullptr;
        if ((rc = fzb_match_list_top_sections(m, c, sections, n_sections, limit, in, capture, &head, out_len, out_found))) return rc;
        return sections_indices_plain(head, n_sections, out_len, out, out_positions);
    }
    sections_clear_out(n_sections, out_len, out_found);
    const size_t stride = trace_stride(m), want = n_sections * std::min(limit, n);
    if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, stride, false)) || (rc = fzb_sections_ensure_slabs(m->sections, n_sections * limit))) return rc;
    auto impl = [&](const PackedOut& o) { return sections_indices_device_impl(m, c, sections, n_sections, limit, in, capture, o.mirror, o.recs, o.cap, o.pos, o.pos_cap, o.words, nullptr); };
    return sections_indices_host(m->top, m->sections, n_sections, want, want * stride, capture, "the traced pass disagrees with the sectioned stage", impl, out, out_len, out_positions, out_found);
}

static int multi_sections_indices_device_impl(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                              fzb_subset* capture, u32* mirror, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                              uint32_t* dev_counts, void* stream) {
    sections_set ss;
    if (!dev_counts || (!dev_out && capacity) || (!dev_positions && positions_capacity)) return fail(FZB_ERR_INVALID, "null argument");
    int rc;
    if ((rc = sections_check(mm, c, sections, n_sections, limit, in, capture, "fzb_multi_match_list_top_sections_indices_device", &ss))) return rc;
    if ((rc = fzb_refuse_groups(mm, "fzb_multi_match_list_top_sections_indices_device"))) return rc;
    if (mm->patterns.empty()) return fail(FZB_ERR_INVALID, "no pattern: handled on the host by fzb_multi_match_list_top_sections_indices");
    const size_t n = c->dev.n;
    size_t P = 0, want;
    const size_t U = multi_union_stride(mm, &P);
    if ((rc = sections_indices_room(n_sections, limit, n, U, capacity, positions_capacity, &want))) return rc;
    hipStream_t st = (hipStream_t)stream;
    SubsetArgs sa{in, capture, mirror};
    if (n == 0 || n_sections == 0) {
        if ((rc = multi_sections_stage(mm, c, ss, limit, &sa, nullptr, dev_counts, st))) return rc;
        HIPCHK(hipMemsetAsync(dev_counts + 2 * n_sections, 0, PACK_WORDS * sizeof(u32), st));
        return FZB_OK;
    }
    // every buffer first: the sources of the union are final before anything is launched
    std::vector<IUnionSrc> src;
    if ((rc = multi_top_indices_sources(mm, want, U, P, &src, st)) || (rc = fzb_sections_ensure_slabs(mm->sections, n_sections * limit))) return rc;
    u32* const slab_counts = mm->sections.slabs + SEC_SLAB_COUNTS;
    fzb_match_rec* const slabs = (fzb_match_rec*)(mm->sections.slabs + SECTIONS_SLAB_WORDS);
    if ((rc = multi_sections_stage(mm, c, ss, limit, &sa, slabs, slab_counts, st))) return rc;
    fzb_launch_sections_items(slabs, slab_counts, (u32)n_sections, (u32)limit, (u32)want, mm->top.head, mm->top_words + MTOP_HEAD, mm->top_items, mm->top_words + MTOP_N_ITEMS, dev_counts,
                              mm->num_cus * 2, st);
    return multi_top_indices_tail(mm, c, want, U, src, dev_out, capacity, dev_positions, positions_capacity, dev_counts + 2 * n_sections, stream);
}

int fzb_multi_match_list_top_sections_indices_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                                     fzb_subset* capture, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                                     uint32_t* dev_counts, void* stream) {
    return multi_sections_indices_device_impl(mm, c, sections, n_sections, limit, in, capture, nullptr, dev_out, capacity, dev_positions, positions_capacity, dev_counts, stream);
}

int fzb_multi_match_list_top_sections_indices(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                              fzb_subset* capture, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found) {
    sections_set ss;
    if (!out || !out_positions || (!out_len && n_sections)) return fail(FZB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out_positions = nullptr;
    int rc;
    if ((rc = sections_check(mm, c, sections, n_sections, limit, in, capture, "fzb_multi_match_list_top_sections_indices", &ss))) return rc;
    if ((rc = fzb_refuse_groups(mm, "fzb_multi_match_list_top_sections_indices"))) return rc;
    const size_t n = c->dev.n;
    if (mm->patterns.empty() || n == 0 || n_sections == 0) {
        fzb_match* head = nullptr;
        if ((rc = fzb_multi_match_list_top_sections(mm, c, sections, n_sections, limit, in, capture, &head, out_len, out_found))) return rc;
        return sections_indices_plain(head, n_sections, out_len, out, out_positions);
    }
    sections_clear_out(n_sections, out_len, out_found);
    size_t P = 0;
    const size_t U = multi_union_stride(mm, &P), want = n_sections * std::min(limit, n);
    if ((rc = ensure_multi_top_indices_buffers(mm, want, U, P, false)) || (rc = fzb_sections_ensure_slabs(mm->sections, n_sections * limit))) return rc;
    auto impl = [&](const PackedOut& o) { return multi_sections_indices_device_impl(mm, c, sections, n_sections, limit, in, capture, o.mirror, o.recs, o.cap, o.pos, o.pos_cap, o.words, nullptr); };
    return sections_indices_host(mm->top, mm->sections, n_sections, want, want * U, capture, "the traced passes disagree with the sectioned multi stage", impl, out, out_len, out_positions,
                                 out_found);
}

int fzb_multi_match_list_top_indices_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len,
                                            uint32_t** out_positions, uint64_t* out_found) {
    if (!mm || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    if (int rc_ = fzb_refuse_groups(mm, "fzb_multi_match_list_top_indices_subset")) return rc_;
    clear_indices_out(out, out_len, out_positions, out_found);
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_top_indices_subset");
    if (rc) return rc;
    if (mm->patterns.empty() || c->dev.n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        if (!in) return fzb_multi_match_list_top_indices_fused(mm, c, limit, out, out_len, out_positions, out_found);
        std::vector<fzb_match> head;  // no pattern over a candidate set: the single form's host list, no positions
        if ((rc = facets_check(mm->facets, c, "fzb_multi_match_list_top_indices_subset")) || (rc = facets_column(mm->facets, c, in, 0, c->dev.n, (int)fzb_grid_cap(~0ull, 2), nullptr))) return rc;
        if ((rc = subset_empty_list(c, const_cast<fzb_subset*>(in), mm->config.sort, limit, head, out_found))) return rc;
        std::vector<fzb_match_indices> recs(head.size());
        for (size_t i = 0; i < head.size(); i++) recs[i] = fzb_match_indices{head[i].index, head[i].score, 0, 0, 0, 0};
        return hand_over_indices(recs.data(), recs.size(), nullptr, 0, out, out_len, out_positions);
    }
    if (!in && !capture) return fzb_multi_match_list_top_indices_fused(mm, c, limit, out, out_len, out_positions, out_found);
    return multi_top_indices_fused_impl(mm, c, limit, out, out_len, out_positions, out_found, in, capture);
}

// ---- matched positions of the top-`limit` for a matcher that has an any-of group ---------------------------------------------------------------
// The head is the multi top stage's, as in the fused form above.  Behind it every plain non-negated pattern AND every alternative of every
// group runs the traced pipeline over the head's one item list, each into its own sub-matcher's trace buffers; an alternative's pass returns
// only the head items it matches.  fzb_launch_gunion (indices_union_groups.h) then finds every alternative's row per head record, picks each
// group's carrier - the largest key score << 1 | exact, the first in query order on equal keys - and merges the plain patterns' and the
// carriers' positions; bias and pack follow unchanged.  Four launches in place of the ungrouped tail's one union, whatever the number of groups
// and alternatives; nothing is read back in between.  Both kinds of matcher share multi_top_indices_device_impl and multi_top_indices_tail: a
// matcher without a group takes them as the ungrouped entry points do, call for call.
int fzb_multi_match_list_top_indices_groups_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices* dev_out,
                                                   size_t capacity, uint32_t* dev_positions, size_t positions_capacity, uint32_t* dev_count, void* stream) {
    if (!mm || !c || !dev_count || (!dev_out && capacity) || (!dev_positions && positions_capacity)) return fail(FZB_ERR_INVALID, "null argument");
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_top_indices_groups_device");
    if (rc) return rc;
    if (mm->patterns.empty() && (in || capture)) return fail(FZB_ERR_INVALID, "no pattern: handled on the host by fzb_multi_match_list_top_indices_groups");
    if (!in && !capture) return multi_top_indices_device_impl(mm, c, limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, nullptr);
    if (c->dev.n == 0) {
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        return multi_top_indices_device_impl(mm, c, limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, nullptr);
    }
    const SubsetArgs sa{in, capture, nullptr};
    return multi_top_indices_device_impl(mm, c, limit, dev_out, capacity, dev_positions, positions_capacity, dev_count, stream, &sa);
}

int fzb_multi_match_list_top_indices_groups(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len,
                                            uint32_t** out_positions, uint64_t* out_found) {
    if (!mm || !c || !out || !out_len || !out_positions) return fail(FZB_ERR_INVALID, "null argument");
    if (!mm->grouped) {  // the ungrouped forms, call for call
        if (!in && !capture) return multi_top_indices_fused_impl(mm, c, limit, out, out_len, out_positions, out_found, nullptr, nullptr);
        return fzb_multi_match_list_top_indices_subset(mm, c, in, capture, limit, out, out_len, out_positions, out_found);
    }
    clear_indices_out(out, out_len, out_positions, out_found);
    int rc = subset_check(c, in, capture, "fzb_multi_match_list_top_indices_groups");
    if (rc) return rc;
    const size_t n = c->dev.n;
    const size_t want = std::min(limit, n);
    if (n == 0) {  // (a grouped matcher has a pattern)
        if ((rc = subset_capture_trivial(c, in, capture))) return rc;
        if ((rc = facets_every(mm->facets, c, 0, n, "fzb_multi_match_list_top_indices_groups"))) return rc;
        return hand_over_indices(nullptr, 0, nullptr, 0, out, out_len, out_positions);
    }
    const GroupShape g = multi_group_shape(mm);
    if ((u64)want * g.U > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x the grouped positions stride does not fit the 32-bit positions_begin");
    return multi_top_indices_host_query(mm, c, in, capture, limit, g.U, 0, out, out_len, out_positions, out_found);
}

// fzb_multi_matcher_reserve_top_indices, and what the grouped tail owns for any grouping of the matcher's slots: the `where` maps of as many
// alternatives as there are slots, the sources' device array and scratch, and the group slots for the haystacks the corpus has room for.
int fzb_multi_matcher_reserve_top_indices_groups(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, size_t max_needle_bytes) {
    int rc = fzb_multi_matcher_reserve_top_indices(mm, c, limit, max_needle_bytes);
    if (rc) return rc;
    const size_t n = fzb_corpus_reserved_items(c);
    const size_t want = std::min(limit, n);
    if (want == 0) return FZB_OK;
    const size_t slots = mm->patterns.size() + mm->spare.size();
    if ((rc = multi_ensure_buffers(mm, n)) || (rc = multi_ensure_group_buffers(mm))) return rc;
    return ensure_gunion_buffers(mm, want, slots, slots);
}

// fzb_matcher_reserve_top_indices for the composition: every sub-matcher slot (the spares too) gets the trace buffers and the traced scorer's
// matrices for heads of up to min(limit, haystacks the corpus has room for) records and needles of up to max_needle_bytes bytes; the
// composition gets its head, item list, combined records, the unions for U = slots x max_needle_bytes and the host form's staging.
int fzb_multi_matcher_reserve_top_indices(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, size_t max_needle_bytes) {
    if (!mm || !c) return fail(FZB_ERR_INVALID, "null argument");
    const size_t n = fzb_corpus_reserved_items(c);
    const size_t want = std::min(limit, n);
    if (want == 0) return FZB_OK;
    if ((u64)n > 0xFFFFFFFFull) return refuse_index_overflow(n);
    std::vector<fzb_matcher*> slots;
    for (auto& p : mm->patterns) slots.push_back(p.m);
    slots.insert(slots.end(), mm->spare.begin(), mm->spare.end());
    size_t stride = std::max<size_t>(max_needle_bytes, 1);
    for (fzb_matcher* m : slots) stride = std::max<size_t>(stride, trace_stride(m));
    const size_t U = slots.size() * stride;
    if ((u64)want * U > 0xFFFFFFFFull) return fail(FZB_ERR_CAPACITY, "min(limit, haystacks) x needle bytes does not fit the 32-bit positions_begin");
    int rc;
    for (fzb_matcher* m : slots)
        if ((rc = fzb_bind_device(m)) || (rc = ensure_top_indices_buffers(m, want, stride, false)) || (rc = reserve_trace_cells(m, want, stride))) return rc;
    return ensure_multi_top_indices_buffers(mm, want, U, slots.size(), true);
}

void fzb_matches_free(fzb_match* p) {
    if (p && !pinned_pool().put(p)) free(p);
}

static bool merge_less(int order, const fzb_match& l, const fzb_match& r) {  // src/k_merge.rs:14-53
    switch (order) {
        case FZB_SORT_SCORE_THEN_INDEX_ASC: return l.score > r.score || (l.score == r.score && l.index < r.index);
        case FZB_SORT_SCORE_THEN_INDEX_DESC: return l.score > r.score || (l.score == r.score && l.index > r.index);
        case FZB_SORT_INDEX_ASC: return l.index < r.index;
        default: return l.index > r.index;
    }
}

int fzb_k_merge_matches(int32_t sort, const fzb_match* runs, const size_t* run_lens, size_t nruns, fzb_match* out) {
    if (sort < 0 || sort > 3 || (nruns && (!run_lens))) return fail(FZB_ERR_INVALID, "bad argument");
    size_t total = 0;
    for (size_t k = 0; k < nruns; k++) total += run_lens[k];
    if (total && (!runs || !out)) return fail(FZB_ERR_INVALID, "null argument");
    std::vector<const fzb_match*> ptrs(nruns);
    size_t off = 0;
    for (size_t k = 0; k < nruns; k++) { ptrs[k] = runs + off; off += run_lens[k]; }
    return fzb_k_merge_runs(sort, ptrs.data(), run_lens, nruns, out);
}

}  // extern "C"
int fzb_k_merge_runs(int32_t sort, const fzb_match* const* runs, const size_t* run_lens, size_t nruns, fzb_match* out) {
    if (sort < 0 || sort > 3 || (nruns && (!run_lens || !runs))) return fail(FZB_ERR_INVALID, "bad argument");
    // tournament over run heads (any correct k-way merge of runs sorted under a TOTAL order yields the same sequence)
    std::vector<size_t> pos(nruns, 0);
    std::vector<size_t> heap;
    auto less_run = [&](size_t a, size_t b) { return merge_less(sort, runs[a][pos[a]], runs[b][pos[b]]); };
    auto cmp = [&](size_t a, size_t b) { return less_run(b, a); };  // std heap is a max-heap
    for (size_t k = 0; k < nruns; k++)
        if (run_lens[k]) heap.push_back(k);
    if (!heap.empty() && !out) return fail(FZB_ERR_INVALID, "null argument");
    std::make_heap(heap.begin(), heap.end(), cmp);
    size_t o = 0;
    while (!heap.empty()) {
        if (heap.size() == 1) {  // one run left: the rest is a copy
            const size_t k = heap[0];
            memcpy(out + o, runs[k] + pos[k], (run_lens[k] - pos[k]) * sizeof(fzb_match));
            break;
        }
        std::pop_heap(heap.begin(), heap.end(), cmp);
        const size_t k = heap.back();
        out[o++] = runs[k][pos[k]];
        if (++pos[k] < run_lens[k]) std::push_heap(heap.begin(), heap.end(), cmp);
        else heap.pop_back();
    }
    return FZB_OK;
}
extern "C" {

int fzb_set_profiling(fzb_matcher* m, int enabled) {
    if (!m) return fail(FZB_ERR_INVALID, "null argument");
    m->profiling = enabled != 0;
    m->prof_calls = 0;
    return FZB_OK;
}

// Averages over the calls made since fzb_set_profiling(m, 1) (at most the last 32 = PROF_SLOTS):
// out_ms[0] = filter kernel, [1] = whole pipeline, [2] = calls averaged, [3] = 1 if a filter kernel ran
int fzb_last_timings(fzb_matcher* m, float out_ms[4]) {
    if (!m || !out_ms) return fail(FZB_ERR_INVALID, "null argument");
    if (!m->profiling || m->prof_calls == 0) return fail(FZB_ERR_INVALID, "profiling not enabled or no call recorded");
    const u64 n = std::min<u64>(m->prof_calls, fzb_matcher::PROF_SLOTS);
    double f = 0, t = 0;
    u64 n_filter = 0;
    for (u64 i = 0; i < n; i++) {
        const int slot = (int)((m->prof_calls - 1 - i) % fzb_matcher::PROF_SLOTS);
        hipEvent_t* e = m->evring[slot];
        HIPCHK(hipEventSynchronize(e[1]));
        float b = 0;
        HIPCHK(hipEventElapsedTime(&b, e[0], e[1]));
        t += b;
        if (m->ev_filter[slot]) {
            float a = 0;
            HIPCHK(hipEventElapsedTime(&a, e[2], e[3]));
            f += a;
            n_filter++;
        }
    }
    out_ms[0] = n_filter ? (float)(f / n_filter) : 0.0f;
    out_ms[1] = (float)(t / n);
    out_ms[2] = (float)n;
    out_ms[3] = (float)n_filter;
    return FZB_OK;
}

// Per-stage averages over the same calls: out_ms[0] = streaming filter kernel, [1] = compaction (+ the lane-exact prefilter and its
// compaction when the configuration has them), [2] = the scorers, [3] = whole pipeline, [4] = calls averaged, [5] = 1 if a filter ran
int fzb_last_stage_timings(fzb_matcher* m, float out_ms[6]) {
    if (!m || !out_ms) return fail(FZB_ERR_INVALID, "null argument");
    if (!m->profiling || m->prof_calls == 0) return fail(FZB_ERR_INVALID, "profiling not enabled or no call recorded");
    const u64 n = std::min<u64>(m->prof_calls, fzb_matcher::PROF_SLOTS);
    // calls with a streaming filter kernel and calls without one (item lists, no prefilter) are averaged separately: the filter
    // figure is the mean over the calls that had one, "compaction" the mean of what lies between filter and scorers in each kind
    double f = 0, mid = 0, sc = 0, t = 0;
    u64 n_filter = 0;
    for (u64 i = 0; i < n; i++) {
        const int slot = (int)((m->prof_calls - 1 - i) % fzb_matcher::PROF_SLOTS);
        hipEvent_t* e = m->evring[slot];
        HIPCHK(hipEventSynchronize(e[1]));
        float a = 0;
        HIPCHK(hipEventElapsedTime(&a, e[0], e[1]));
        t += a;
        HIPCHK(hipEventElapsedTime(&a, e[4], e[1]));
        sc += a;
        if (m->ev_filter[slot]) {
            n_filter++;
            HIPCHK(hipEventElapsedTime(&a, e[2], e[3]));
            f += a;
            HIPCHK(hipEventElapsedTime(&a, e[3], e[4]));
            mid += a;
        } else {
            HIPCHK(hipEventElapsedTime(&a, e[0], e[4]));
            mid += a;
        }
    }
    out_ms[0] = n_filter ? (float)(f / n_filter) : 0.0f;
    out_ms[1] = (float)(mid / n);
    out_ms[2] = (float)(sc / n);
    out_ms[3] = (float)(t / n);
    out_ms[4] = (float)n;
    out_ms[5] = (float)n_filter;  // calls (of the averaged ones) that ran a streaming filter kernel; 0 = none
    return FZB_OK;
}

// Test hook (host only, no GPU): runs the unicode 0-typo prefilter DFA the streaming filter would run over one haystack.
// Returns 1 / 0 = accept / reject, -1 if this matcher has no such DFA (not the unicode path, typos, or more than 255 states).
int fzb_debug_unicode_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len) {
    if (!m || m->uni_dfa_states == 0 || (!bytes && len)) return -1;
    u32 st = 0;
    for (size_t i = 0; i < len; i++) st = m->uni_dfa[(size_t)st * 256 + bytes[i]];
    return st == (u32)m->uni_dfa_states - 1 ? 1 : 0;
}

// Test hook (host only): the LCS automaton of a typo configuration run over one haystack.  1 / 0 = the streaming filter accepts / rejects
// (LCS >= rows - max_typos), -1 if the matcher has no such automaton; *out_states (optional) = its number of states.
int fzb_debug_lcs_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len, int32_t* out_states) {
    if (out_states) *out_states = m ? m->lcs_states : 0;
    if (!m || m->lcs_states == 0 || (!bytes && len)) return -1;
    u32 st = 0;
    for (size_t i = 0; i < len; i++) st = m->lcs_dfa[(size_t)st * 256 + bytes[i]];
    return st >= (u32)m->lcs_acc_lo ? 1 : 0;
}

// Test hook (host only): the class-composite form of the matcher's streaming automaton run over one haystack, G bytes per step (the
// tail padded with a byte of the "matches nothing" class, as the kernel sees zero fill): 1 / 0 = accepts / rejects, -1 if the matcher has none.
// out_kg (optional): [0] = K, [1] = G.
int fzb_debug_needle_signature(const fzb_matcher* m, uint32_t* out_mask, int* out_eligible) {
    if (!m) return fail(FZB_ERR_INVALID, "null argument");
    if (out_mask) *out_mask = m->needle_sig;
    if (out_eligible) *out_eligible = m->sig_eligible ? 1 : 0;
    return FZB_OK;
}
uint32_t fzb_debug_signature_threshold(void) { return std::min<u32>(FZB_SIG_GATHER_MAX, FZB_TILE); }
// Test hook: caps the grid of a filter that lists its own survivors (0 = the default, 8 workgroups per CU), so that a small list gets runs of
// several tiles, a short last run and empty trailing segments.
void fzb_debug_set_filter_grid(int grid) { g_debug_filter_grid = grid > 0 ? grid : 0; }

int fzb_debug_cdfa_state(const fzb_matcher* m, const uint8_t* bytes, size_t len, int32_t* out_kg) {
    if (out_kg) { out_kg[0] = m ? m->cdfa_K : 0; out_kg[1] = m ? m->cdfa_G : 0; }
    if (!m || m->cdfa.empty() || (!bytes && len)) return -1;
    const size_t K = (size_t)m->cdfa_K;
    size_t KG = 1;
    for (int i = 0; i < m->cdfa_G; i++) KG *= K;
    u32 st = 0;
    for (size_t i = 0; i < len; i += (size_t)m->cdfa_G) {
        size_t off = 0, mul = 1;
        for (int j = 0; j < m->cdfa_G; j++, mul *= K) off += mul * m->cdfa[i + j < len ? bytes[i + j] : (u8)m->lc.dead_byte];
        st = m->cdfa[256 + (size_t)st * KG + off];
    }
    const u32 acc = m->cdfa_src == 1 ? (u32)m->rows : m->cdfa_src == 2 ? (u32)m->uni_dfa_states - 1 : (u32)m->lcs_acc_lo;
    return st >= acc ? 1 : 0;
}

// Test hook (host only): the Knuth-Morris-Pratt byte table of a literal Substring matcher on the ASCII path (build_filter_tables) run over
// one haystack and then over `fill` bytes of what the streaming kernels read behind its end (zero fill; the dead byte where the needle
// holds a NUL and the kernels sanitise): 1 / 0 = accepts / rejects, -1 if the matcher has no such table.
int fzb_debug_kmp_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len, size_t fill) {
    if (!m || m->empty || m->long_needle || m->unicode || m->literal_mode != FZB_MATCH_SUBSTRING || (!bytes && len)) return -1;
    if (m->dfa.size() != (size_t)(m->rows + 1) * 256) return -1;
    const u8 behind = m->lc.pad_ok ? (u8)0 : (u8)m->lc.dead_byte;
    u32 st = 0;
    for (size_t i = 0; i < len + fill; i++) st = m->dfa[(size_t)st * 256 + (i < len ? bytes[i] : behind)];
    return st == (u32)m->rows ? 1 : 0;
}

int fzb_last_counters(fzb_matcher* m, uint32_t out[4]) {
    if (!m || !out) return fail(FZB_ERR_INVALID, "null argument");
    if (m->ws.counters) {
        u32 all[16];
        HIPCHK(hipMemcpy(all, m->ws.counters, sizeof(all), hipMemcpyDeviceToHost));
        m->last_counters[0] = all[0];
        m->last_counters[1] = all[1];
        // (unicode: windows of 65..1024 bytes that the thread-per-haystack scorer handed on to the queue's back are in BOTH counts - all[7] claims,
        // at most 4096 granted: they stay "multi-chunk" here, and the greedy fallback's count is the back minus them)
        const u32 fwd = std::min<u32>(all[7], 4096u);
        m->last_counters[2] = all[4] >= fwd && m->nd.unicode ? all[4] - fwd : all[4];
        m->last_counters[3] = all[3] + all[12] + all[13] + all[14] + all[15];  // multi-chunk windows: the queue, or the four tail-class lists
    }
    memcpy(out, m->last_counters, 16);
    return FZB_OK;
}

}  // extern "C"
