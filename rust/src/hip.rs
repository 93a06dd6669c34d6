//! `src/matcher/hip.rs` of saghen/frizbee, feature `hip`: the binding a maintainer adds to use `libfrizbee_hip.so`
//! (include/frizbee_hip.h) as one more `MatcherBackend` variant.
//!
//! NOT COMPILED in this repository: the build image and the GPU boxes have no Rust toolchain (profiles/r02_box_probe.txt).
//! Everything below the `extern "C"` block is built, loaded and tested here through the same C ABI (tests/test_host_abi.py:
//! the library exports exactly the symbols the header declares; tests/test_gpu_*.py drive them on an MI355X).  The struct
//! layouts are checked against the header by tests/test_host_abi.py::test_struct_layouts_match_header on the Python side;
//! keep the two in step.
//!
//! Three ways to use the backend, cheapest integration first:
//!   1. `MatcherHip::match_list` — the `Specialized::match_list` seam (src/matcher/algo.rs:17-22).  Uploads the borrowed
//!      haystacks on EVERY call.  Measured on an MI355X box: 10 M x 32 B = 8.1 ms per call (7.7 ms of it the PCIe copy
//!      at 52 GB/s) against 3.5 ms for the crate's own 64-thread CPU path — a literal drop-in at this seam is SLOWER than
//!      the CPU crate for one query.  It exists so that the crate's tests run against the backend unchanged.
//!   2. `HipCorpus` + `MatcherHip::match_list_resident` — the list stays in HBM across queries (0.24 ms per ordered query
//!      on the same list, 0.10 ms with the result left on the device): the interactive case (`Matcher::set_pattern` on
//!      every keystroke against one file list) and the one the backend is for.
//!   3. `ShardedCorpus` + `MatcherHip::match_list_parallel_sharded` — `match_list_parallel` with one GPU per worker.
use crate::{CaseMatching, Config, Match, MatchIndices, Pattern, SortStrategy, UnicodeMatching};
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
struct FzbScoring {
    match_score: u16,
    mismatch_penalty: u16,
    gap_open_penalty: u16,
    gap_extend_penalty: u16,
    prefix_bonus: u16,
    capitalization_bonus: u16,
    matching_case_bonus: u16,
    exact_match_bonus: u16,
    delimiter_bonus: u16,
}
#[repr(C)]
struct FzbConfig {
    max_typos: i32, // -1 = None
    casing: i32,
    unicode: i32,
    sort: i32,
    scoring: FzbScoring,
    pf_lanes: u16, // 0 / 0: the lane pair `Matcher::get_backend` picks on this host
    sw_lanes: u16,
    matching: i32,
}
#[repr(C)]
#[derive(Clone, Copy)]
struct FzbMatch {
    index: u32,
    score: u16,
    exact: u8,
    _pad: u8,
}
// a tag section of the sectioned top-`limit` calls (fzb_section): the visibility scope's predicate over the haystacks' 16 tag bits
#[repr(C)]
#[derive(Clone, Copy)]
#[allow(dead_code)]
struct FzbSection {
    require: u16,
    exclude: u16,
}
#[repr(C)]
#[derive(Clone, Copy)]
struct FzbMatchIndices {
    index: u32,
    score: u16,
    exact: u8,
    _pad: u8,
    positions_begin: u32,
    positions_len: u32,
}

/// `Pattern` + `PatternConfig` (src/pattern.rs:9-18, 230-262) as the header's `fzb_pattern`: -1 / has_* = 0 = inherit the matcher's config
#[repr(C)]
struct FzbPattern {
    needle_utf8: *const u8,
    needle_len: usize,
    negated: i32,
    has_max_typos: i32,
    max_typos: i32,
    casing: i32,
    unicode: i32,
    has_scoring: i32,
    scoring: FzbScoring,
    matching: i32,
}

const FZB_ERR_PANIC: c_int = 2;
const FZB_SHARD_BY_BYTES: c_int = 1;

#[link(name = "frizbee_hip")]
extern "C" {
    fn fzb_last_error() -> *const c_char;
    fn fzb_matcher_create(cfg: *const FzbConfig, needle: *const u8, len: usize, out: *mut *mut c_void) -> c_int;
    fn fzb_matcher_set_pattern(m: *mut c_void, needle: *const u8, len: usize) -> c_int;
    fn fzb_matcher_free(m: *mut c_void);
    fn fzb_corpus_upload(bytes: *const u8, ends: *const u64, n: usize, out: *mut *mut c_void) -> c_int;
    fn fzb_corpus_free(c: *mut c_void);
    // a corpus that grows: batches behind the resident list, room ahead of them, the first n kept (set-up calls, like the upload)
    fn fzb_corpus_append(c: *mut c_void, bytes: *const u8, ends: *const u64, n_new: usize) -> c_int;
    fn fzb_corpus_reserve(c: *mut c_void, items: usize, bytes: u64) -> c_int;
    fn fzb_corpus_truncate(c: *mut c_void, n: usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_corpus_info(c: *const c_void, out: *mut u64) -> c_int;
    // the signatures' bit-planes of a list of short haystacks (another 4 bytes per haystack): whether the corpus has them, and their size
    #[allow(dead_code)]
    fn fzb_corpus_signature_planes_info(c: *const c_void, out_built: *mut c_int, out_bytes: *mut u64) -> c_int;
    // the repeat planes beside them (which signature bits a haystack holds at least twice; another 4 bytes per haystack)
    #[allow(dead_code)]
    fn fzb_corpus_signature_repeat_planes_info(c: *const c_void, out_built: *mut c_int, out_bytes: *mut u64) -> c_int;
    // a corpus that is edited: haystacks removed or replaced anywhere; only the indices (and a replace's new bytes) cross the link
    fn fzb_corpus_remove(c: *mut c_void, indices: *const u32, n_indices: usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_corpus_remove_device(c: *mut c_void, dev_indices: *const c_void, stride_bytes: usize, dev_count: *const u32, max_count: usize) -> c_int;
    fn fzb_corpus_replace(c: *mut c_void, indices: *const u32, n: usize, bytes: *const u8, ends: *const u64) -> c_int;
    fn fzb_corpus_edit_info(c: *const c_void, out: *mut u64) -> c_int;
    // a per-haystack score bias, added on the device before anything selects or orders: reported score = clamp(score + bias[index], 0, 65535)
    fn fzb_corpus_set_bias(c: *mut c_void, values: *const i16, n: usize) -> c_int;
    fn fzb_corpus_update_bias(c: *mut c_void, indices: *const u32, values: *const i16, n: usize) -> c_int;
    fn fzb_corpus_clear_bias(c: *mut c_void) -> c_int;
    fn fzb_corpus_bias_info(c: *const c_void, out: *mut u64) -> c_int;
    // per-haystack tags and a visibility scope: haystack i is visible iff (tags[i] & require) == require && (tags[i] & exclude) == 0
    fn fzb_corpus_set_tags(c: *mut c_void, values: *const u16, n: usize) -> c_int;
    fn fzb_corpus_update_tags(c: *mut c_void, indices: *const u32, values: *const u16, n: usize) -> c_int;
    fn fzb_corpus_clear_tags(c: *mut c_void) -> c_int;
    fn fzb_corpus_set_scope(c: *mut c_void, require: u16, exclude: u16) -> c_int;
    fn fzb_corpus_scope_info(c: *const c_void, out: *mut u64) -> c_int;
    fn fzb_corpus_len(c: *const c_void) -> usize;
    fn fzb_match_list(m: *mut c_void, c: *const c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_match_list_into(m: *mut c_void, c: *const c_void, first: usize, count: usize, index_offset: u32, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_matches_free(p: *mut FzbMatch);
    // top-`limit` queries: the first min(limit, found) records of `match_list`'s result, selected and ordered on the device
    fn fzb_match_list_top(m: *mut c_void, c: *const c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_match_list_top_device(m: *mut c_void, c: *const c_void, limit: usize, dev_out: *mut FzbMatch, capacity: usize, dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_match_list_top_indices(m: *mut c_void, c: *const c_void, limit: usize, out: *mut *mut FzbMatchIndices, out_len: *mut usize, out_positions: *mut *mut u32,
                                  out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_match_list_top_indices_device(m: *mut c_void, c: *const c_void, limit: usize, dev_out: *mut FzbMatchIndices, capacity: usize, dev_positions: *mut u32,
                                         positions_capacity: usize, dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_matcher_reserve_top_indices(m: *mut c_void, c: *const c_void, limit: usize, max_needle_bytes: usize) -> c_int;
    // candidate sets (fzb_subset): a query over a device-resident subset of the corpus, and the capture of a query's match set
    fn fzb_corpus_generation(c: *const c_void, out: *mut u64) -> c_int;
    fn fzb_subset_create(c: *const c_void, out: *mut *mut c_void) -> c_int;
    fn fzb_subset_free(s: *mut c_void);
    fn fzb_subset_set_indices(s: *mut c_void, host_indices: *const u32, n: usize) -> c_int;
    fn fzb_subset_from_scope(s: *mut c_void, c: *const c_void, require: u16, exclude: u16) -> c_int;
    fn fzb_subset_info(s: *mut c_void, out: *mut u64) -> c_int;
    fn fzb_subset_read(s: *mut c_void, host_out: *mut u32, cap: usize, out_n: *mut usize) -> c_int;
    fn fzb_match_list_subset(m: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_match_list_top_subset(m: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize,
                                 out_found: *mut u64) -> c_int;
    fn fzb_match_list_top_subset_device(m: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, dev_out: *mut FzbMatch, capacity: usize,
                                        dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_match_list_top_indices_subset(m: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, out: *mut *mut FzbMatchIndices,
                                         out_len: *mut usize, out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    // the empty prompt's _device forms (a matcher whose needle is empty; `input` may be null): the index-ordered list, and its ordered head
    fn fzb_prompt_list_device(m: *mut c_void, c: *const c_void, input: *const c_void, first: usize, count: usize, index_offset: u32, dev_out: *mut FzbMatch, capacity: usize,
                              dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_prompt_top_device(m: *mut c_void, c: *const c_void, input: *const c_void, limit: usize, dev_out: *mut FzbMatch, capacity: usize, dev_count: *mut u32,
                             stream: *mut c_void) -> c_int;
    // tag facets (fzb_facets): the per-tag match counts of a query, counted on the device into a sink attached to the matcher; `out` holds
    // FZB_FACET_WORDS = 34 words: matched, visible, all_by_bit[16], visible_by_bit[16]
    #[allow(dead_code)]
    fn fzb_facets_create(c: *const c_void, out: *mut *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_facets_free(f: *mut c_void);
    #[allow(dead_code)]
    fn fzb_facets_read(f: *mut c_void, out: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn fzb_facets_device(f: *const c_void) -> *const u32;
    #[allow(dead_code)]
    fn fzb_matcher_set_facets(m: *mut c_void, f: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_matcher_set_facets(mm: *mut c_void, f: *mut c_void) -> c_int;
    // sectioned top-`limit`: the best `limit` matches per tag section (at most FZB_SECTIONS_MAX = 8 sections, limit <= FZB_SECTION_LIMIT_MAX =
    // 1024) from one pass of the filter and the scorers; host forms: one block, the heads concatenated in section order, out_len / out_found
    // per section; _device forms: section s at dev_out + s * limit, dev_counts = 2 words per section (records, matches).  No sharded or
    // RCCL forms; matched positions: the _sections_indices forms below.
    #[allow(dead_code)]
    fn fzb_match_list_top_sections(m: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void, capture: *mut c_void,
                                   out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_match_list_top_sections_device(m: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                          capture: *mut c_void, dev_out: *mut FzbMatch, capacity: usize, dev_counts: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_sections(mm: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                         capture: *mut c_void, out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_sections_device(mm: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                                capture: *mut c_void, dev_out: *mut FzbMatch, capacity: usize, dev_counts: *mut u32, stream: *mut c_void) -> c_int;
    // sectioned top-`limit` with matched positions: element s = fzb_match_list_top_indices over the corpus' scope AND section s.  Host forms:
    // one block of records (heads concatenated in section order) and one dense position array, freed with fzb_match_indices_free; _device
    // forms: the heads densely concatenated, dev_counts = 2 * n_sections + 4 words ([2s] records of head s, [2s + 1] matches in section s,
    // [2S] records in all, [2S + 2] positions written, [2S + 3] the pack's inconsistency word)
    #[allow(dead_code)]
    fn fzb_match_list_top_sections_indices(m: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                           capture: *mut c_void, out: *mut *mut FzbMatchIndices, out_len: *mut usize, out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_match_list_top_sections_indices_device(m: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                                  capture: *mut c_void, dev_out: *mut FzbMatchIndices, capacity: usize, dev_positions: *mut u32, positions_capacity: usize,
                                                  dev_counts: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_sections_indices(mm: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                                 capture: *mut c_void, out: *mut *mut FzbMatchIndices, out_len: *mut usize, out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_sections_indices_device(mm: *mut c_void, c: *const c_void, sections: *const FzbSection, n_sections: usize, limit: usize, input: *const c_void,
                                                        capture: *mut c_void, dev_out: *mut FzbMatchIndices, capacity: usize, dev_positions: *mut u32, positions_capacity: usize,
                                                        dev_counts: *mut u32, stream: *mut c_void) -> c_int;
    // the same four over a `from_patterns` matcher: the composition runs over `input`, `capture` receives the composition's match set
    #[allow(dead_code)]
    fn fzb_multi_match_list_subset(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_subset(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize,
                                       out_found: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_subset_device(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, dev_out: *mut FzbMatch, capacity: usize,
                                              dev_count: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_top_indices_subset(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, out: *mut *mut FzbMatchIndices,
                                               out_len: *mut usize, out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    fn fzb_multi_match_list_top_indices_groups(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, out: *mut *mut FzbMatchIndices,
                                               out_len: *mut usize, out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    fn fzb_multi_match_list_top_indices_groups_device(mm: *mut c_void, c: *const c_void, input: *const c_void, capture: *mut c_void, limit: usize, dev_out: *mut FzbMatchIndices,
                                                      capacity: usize, dev_positions: *mut u32, positions_capacity: usize, dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_multi_matcher_groups_positions_stride(mm: *const c_void, out: *mut usize) -> c_int;
    fn fzb_multi_matcher_reserve_top_indices_groups(mm: *mut c_void, c: *const c_void, limit: usize, max_needle_bytes: usize) -> c_int;
    fn fzb_match_list_top_sharded(m: *mut c_void, sc: *const c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    fn fzb_match_list_indices(m: *mut c_void, c: *const c_void, selection: *const u32, n_selection: usize, out: *mut *mut FzbMatchIndices, out_len: *mut usize,
                              out_positions: *mut *mut u32) -> c_int;
    fn fzb_match_indices_free(matches: *mut FzbMatchIndices, positions: *mut u32);
    fn fzb_corpus_upload_sharded(bytes: *const u8, ends: *const u64, n: usize, ndev: c_int, flags: c_int, out: *mut *mut c_void) -> c_int;
    fn fzb_sharded_corpus_free(sc: *mut c_void);
    fn fzb_match_list_parallel_sharded(m: *mut c_void, sc: *const c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_device_count(out: *mut c_int) -> c_int;
    fn fzb_matcher_shard_report(m: *const c_void) -> *const std::os::raw::c_char;
    // (bound by hosts that move the per-shard runs themselves / hold the list in HBM already; not used by the wrappers below)
    #[allow(dead_code)]
    fn fzb_merge_shard_runs(m: *mut c_void, dev_runs: *const *const c_void, dev_counts: *const *const u32, run_caps: *const usize, nruns: usize, stream: *mut c_void,
                            out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_corpus_build_view(c: *mut c_void, out_built: *mut c_int) -> c_int;
    // one process per GPU: the runs travel by RCCL below the boundary (csrc/host_rccl.hip)
    fn fzb_rccl_unique_id(out_id: *mut u8) -> c_int;
    fn fzb_shard_comm_create(id: *const u8, rank: c_int, world: c_int, out: *mut *mut c_void) -> c_int;
    fn fzb_shard_comm_free(comm: *mut c_void);
    fn fzb_match_list_parallel_rccl(m: *mut c_void, shard: *const c_void, index_offset: u32, comm: *mut c_void, flags: c_int, out: *mut *mut FzbMatch,
                                    out_len: *mut usize) -> c_int;
    // `Matcher::from_patterns` (src/matcher/mod.rs:95-111; composition src/matcher/multi.rs:84-152) and its lifecycle
    fn fzb_multi_matcher_create(cfg: *const FzbConfig, patterns: *const FzbPattern, n_patterns: usize, out: *mut *mut c_void) -> c_int;
    fn fzb_multi_matcher_free(mm: *mut c_void);
    fn fzb_multi_matcher_len(mm: *const c_void) -> usize;
    fn fzb_multi_match_list(mm: *mut c_void, c: *const c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_indices(mm: *mut c_void, c: *const c_void, selection: *const u32, n_selection: usize, out: *mut *mut FzbMatchIndices, out_len: *mut usize,
                                    out_positions: *mut *mut u32) -> c_int;
    fn fzb_multi_match_list_into(mm: *mut c_void, c: *const c_void, first: usize, count: usize, index_offset: u32, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_indices_into(mm: *mut c_void, c: *const c_void, selection: *const u32, n_selection: usize, index_offset: u32, out: *mut *mut FzbMatchIndices,
                                         out_len: *mut usize, out_positions: *mut *mut u32) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_match_list_device(mm: *mut c_void, c: *const c_void, first: usize, count: usize, index_offset: u32, dev_out: *mut FzbMatch, capacity: usize,
                                   dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_multi_matcher_set_patterns(mm: *mut c_void, patterns: *const FzbPattern, n_patterns: usize) -> c_int;
    fn fzb_multi_matcher_set_config(mm: *mut c_void, cfg: *const FzbConfig) -> c_int;
    fn fzb_multi_matcher_reserve(mm: *mut c_void, c: *const c_void) -> c_int;
    #[allow(dead_code)]
    fn fzb_multi_matcher_clone(mm: *const c_void, out: *mut *mut c_void) -> c_int;
    // any-of groups (`a | b`): group_of[i] = the term id of pattern i, equal adjacent ids = the alternatives of one group
    fn fzb_multi_matcher_create_groups(cfg: *const FzbConfig, patterns: *const FzbPattern, n_patterns: usize, group_of: *const u32, out: *mut *mut c_void) -> c_int;
    fn fzb_multi_matcher_set_pattern_groups(mm: *mut c_void, patterns: *const FzbPattern, n_patterns: usize, group_of: *const u32) -> c_int;
    #[allow(dead_code)]
    fn fzb_parse_query_groups(query: *const u8, len: usize, out_patterns: *mut *mut FzbPattern, out_group_of: *mut *mut u32, out_n: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn fzb_query_groups_free(patterns: *mut FzbPattern, group_of: *mut u32, n: usize);
    #[allow(dead_code)]
    fn fzb_multi_match_list_parallel(mm: *mut c_void, c: *const c_void, threads: usize, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_multi_match_list_parallel_sharded(mm: *mut c_void, sc: *const c_void, out: *mut *mut FzbMatch, out_len: *mut usize) -> c_int;
    fn fzb_multi_match_list_parallel_rccl(mm: *mut c_void, shard: *const c_void, index_offset: u32, comm: *mut c_void, flags: c_int, out: *mut *mut FzbMatch,
                                          out_len: *mut usize) -> c_int;
    fn fzb_multi_match_list_top(mm: *mut c_void, c: *const c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    fn fzb_multi_match_list_top_indices(mm: *mut c_void, c: *const c_void, limit: usize, out: *mut *mut FzbMatchIndices, out_len: *mut usize, out_positions: *mut *mut u32,
                                        out_found: *mut u64) -> c_int;
    fn fzb_multi_match_list_top_indices_fused(mm: *mut c_void, c: *const c_void, limit: usize, out: *mut *mut FzbMatchIndices, out_len: *mut usize,
                                              out_positions: *mut *mut u32, out_found: *mut u64) -> c_int;
    fn fzb_multi_match_list_top_indices_device(mm: *mut c_void, c: *const c_void, limit: usize, dev_out: *mut FzbMatchIndices, capacity: usize, dev_positions: *mut u32,
                                               positions_capacity: usize, dev_count: *mut u32, stream: *mut c_void) -> c_int;
    fn fzb_multi_matcher_reserve_top_indices(mm: *mut c_void, c: *const c_void, limit: usize, max_needle_bytes: usize) -> c_int;
    fn fzb_multi_match_list_top_sharded(mm: *mut c_void, sc: *const c_void, limit: usize, out: *mut *mut FzbMatch, out_len: *mut usize, out_found: *mut u64) -> c_int;
    fn fzb_multi_matcher_shard_report(mm: *const c_void) -> *const c_char;
}

/// The reference panics (`assert!`) where the ABI returns FZB_ERR_PANIC, with the same text; every other code is a backend
/// error (no device, out of memory, invalid argument) — also a panic here, because `Specialized::match_list` has no error
/// channel, but with the backend's message.  Nothing unwinds across the FFI boundary: the library returns codes.
fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(fzb_last_error()) }.to_string_lossy().into_owned();
        if rc == FZB_ERR_PANIC {
            panic!("{msg}");
        }
        panic!("frizbee hip backend: {msg} (code {rc})");
    }
}

fn pack<H: AsRef<str>>(haystacks: &[H]) -> (Vec<u8>, Vec<u64>) {
    let mut bytes = Vec::with_capacity(haystacks.iter().map(|h| h.as_ref().len()).sum());
    let mut ends = Vec::with_capacity(haystacks.len());
    for h in haystacks {
        bytes.extend_from_slice(h.as_ref().as_bytes());
        ends.push(bytes.len() as u64);
    }
    (bytes, ends)
}

/// A haystack list resident in HBM (the `&[S]` that `match_list` borrows, uploaded once).
pub struct HipCorpus {
    handle: *mut c_void,
    len: usize,
}
impl HipCorpus {
    pub fn new<H: AsRef<str>>(haystacks: &[H]) -> Self {
        let (bytes, ends) = pack(haystacks);
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_corpus_upload(bytes.as_ptr(), ends.as_ptr(), ends.len(), &mut handle) });
        Self { handle, len: ends.len() }
    }
    pub fn len(&self) -> usize {
        self.len
    }
    /// The batch becomes haystacks `len()..` of the resident list: only the batch crosses the link (a picker's list arrives in pieces;
    /// `HipCorpus::new::<&str>(&[])` is how it starts).  Queries answer as over one upload of the whole list.
    pub fn append<H: AsRef<str>>(&mut self, batch: &[H]) {
        let (bytes, ends) = pack(batch);
        check(unsafe { fzb_corpus_append(self.handle, bytes.as_ptr(), ends.as_ptr(), ends.len()) });
        self.len += ends.len();
    }
    /// Room for `items` haystacks and `bytes` padded bytes (at most the raw bytes + 15 per haystack): appends within it allocate nothing.
    pub fn reserve(&mut self, items: usize, bytes: u64) {
        check(unsafe { fzb_corpus_reserve(self.handle, items, bytes) });
    }
    /// Keeps the first `n` haystacks; capacity is kept.
    pub fn truncate(&mut self, n: usize) {
        check(unsafe { fzb_corpus_truncate(self.handle, n) });
        self.len = n;
    }
    /// Removes the haystacks named by `indices` (any order, repeats allowed); the others keep their order and are renumbered, as
    /// `Vec::retain` would.  Nothing in front of the first touched haystack moves.
    pub fn remove(&mut self, indices: &[u32]) {
        check(unsafe { fzb_corpus_remove(self.handle, indices.as_ptr(), indices.len()) });
        self.len = unsafe { fzb_corpus_len(self.handle) };
    }
    /// `batch[k]` becomes the content of haystack `indices[k]` (unique indices, any order; lengths may change).
    pub fn replace<H: AsRef<str>>(&mut self, indices: &[u32], batch: &[H]) {
        assert_eq!(indices.len(), batch.len(), "one haystack per index");
        let (bytes, ends) = pack(batch);
        check(unsafe { fzb_corpus_replace(self.handle, indices.as_ptr(), indices.len(), bytes.as_ptr(), ends.as_ptr()) });
    }
    /// The last edit: [first changed haystack, canonical bytes written, view tiles rebuilt, peak temporary device bytes].
    pub fn edit_info(&self) -> [u64; 4] {
        let mut out = [0u64; 4];
        check(unsafe { fzb_corpus_edit_info(self.handle, out.as_mut_ptr()) });
        out
    }
    /// One `i16` per haystack (`values.len()` = the list's length), added to every record's score on the device before the selection and
    /// the ordering: what a picker's frecency / "file is open" boost needs for `match_list_top` to pick the records the user sees.  The
    /// bias belongs to the list: it survives `set_pattern` and follows `append` / `truncate` / `remove` / `replace`.
    pub fn set_bias(&mut self, values: &[i16]) {
        check(unsafe { fzb_corpus_set_bias(self.handle, values.as_ptr(), values.len()) });
    }
    /// `bias[indices[k]] = values[k]` (unique indices in range); a corpus without a bias gets an all-zero one first.
    pub fn update_bias(&mut self, indices: &[u32], values: &[i16]) {
        assert_eq!(indices.len(), values.len(), "one value per index");
        check(unsafe { fzb_corpus_update_bias(self.handle, indices.as_ptr(), values.as_ptr(), indices.len()) });
    }
    /// The corpus answers exactly as before any bias.
    pub fn clear_bias(&mut self) {
        check(unsafe { fzb_corpus_clear_bias(self.handle) });
    }
    /// [carries a bias (0/1), entries the array has room for, upper bound of the largest positive bias, device bytes].
    pub fn bias_info(&self) -> [u64; 4] {
        let mut out = [0u64; 4];
        check(unsafe { fzb_corpus_bias_info(self.handle, out.as_mut_ptr()) });
        out
    }
    /// One `u16` of caller-defined bits per haystack (`values.len()` = the list's length).  With `set_scope` they decide which haystacks
    /// a query sees.  The tags belong to the list: they survive `set_pattern` and follow `append` / `truncate` / `remove` / `replace`.
    pub fn set_tags(&mut self, values: &[u16]) {
        check(unsafe { fzb_corpus_set_tags(self.handle, values.as_ptr(), values.len()) });
    }
    /// `tags[indices[k]] = values[k]` (unique indices in range); a corpus without tags gets an all-zero array first.
    pub fn update_tags(&mut self, indices: &[u32], values: &[u16]) {
        assert_eq!(indices.len(), values.len(), "one value per index");
        check(unsafe { fzb_corpus_update_tags(self.handle, indices.as_ptr(), values.as_ptr(), indices.len()) });
    }
    /// Every tag 0 and the scope (0, 0).
    pub fn clear_tags(&mut self) {
        check(unsafe { fzb_corpus_clear_tags(self.handle) });
    }
    /// Haystack `i` is visible iff `(tags[i] & require) == require && (tags[i] & exclude) == 0`; a query returns what it returns over the
    /// visible haystacks alone, every index that of the full list.  Host only: the "toggle ignored files" keystroke.  `(0, 0)` is no scope.
    pub fn set_scope(&mut self, require: u16, exclude: u16) {
        check(unsafe { fzb_corpus_set_scope(self.handle, require, exclude) });
    }
    /// The list's generation: + 1 for every append / truncate / remove / replace that changed it (what a candidate set is checked against).
    pub fn generation(&self) -> u64 {
        let mut g = 0u64;
        check(unsafe { fzb_corpus_generation(self.handle, &mut g) });
        g
    }
    /// [scope active (0/1), entries the tags array has room for, require | exclude << 16, device bytes].
    pub fn scope_info(&self) -> [u64; 4] {
        let mut out = [0u64; 4];
        check(unsafe { fzb_corpus_scope_info(self.handle, out.as_mut_ptr()) });
        out
    }
}
impl Drop for HipCorpus {
    fn drop(&mut self) {
        unsafe { fzb_corpus_free(self.handle) }
    }
}

/// The list cut into contiguous shards, shard g resident on GPU g (`match_list_parallel`'s chunks, src/matcher/parallel.rs:55-63).
pub struct ShardedCorpus {
    handle: *mut c_void,
}
impl ShardedCorpus {
    /// `gpus = 0`: every visible device.  `by_bytes`: shards of equal bytes instead of equal counts (ragged lists).
    pub fn new<H: AsRef<str>>(haystacks: &[H], gpus: usize, by_bytes: bool) -> Self {
        let mut have: c_int = 0;
        check(unsafe { fzb_device_count(&mut have) });
        let ndev = if gpus == 0 { have } else { gpus as c_int };
        let (bytes, ends) = pack(haystacks);
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_corpus_upload_sharded(bytes.as_ptr(), ends.as_ptr(), ends.len(), ndev, if by_bytes { FZB_SHARD_BY_BYTES } else { 0 }, &mut handle) });
        Self { handle }
    }
}
impl Drop for ShardedCorpus {
    fn drop(&mut self) {
        unsafe { fzb_sharded_corpus_free(self.handle) }
    }
}

pub struct MatcherHip {
    handle: *mut c_void,
}

fn c_config(config: &Config, sort: i32) -> FzbConfig {
    let s = &config.scoring;
    FzbConfig {
        max_typos: config.max_typos.map(|t| t as i32).unwrap_or(-1),
        casing: match config.casing { CaseMatching::Ignore => 0, CaseMatching::Smart => 1, CaseMatching::Respect => 2 },
        unicode: match config.unicode { UnicodeMatching::Ignore => 0, UnicodeMatching::Smart => 1, UnicodeMatching::Always => 2 },
        sort,
        scoring: FzbScoring {
            match_score: s.match_score, mismatch_penalty: s.mismatch_penalty, gap_open_penalty: s.gap_open_penalty, gap_extend_penalty: s.gap_extend_penalty,
            prefix_bonus: s.prefix_bonus, capitalization_bonus: s.capitalization_bonus, matching_case_bonus: s.matching_case_bonus,
            exact_match_bonus: s.exact_match_bonus, delimiter_bonus: s.delimiter_bonus,
        },
        pf_lanes: 0,
        sw_lanes: 0,
        matching: config.matching as i32, // Fuzzy = 0, Exact, Prefix, Suffix, Substring (declaration order, src/lib.rs:414-427)
    }
}

/// `SortStrategy` as the header's FZB_SORT_* value (src/lib.rs:311-326)
fn sort_code(sort: &SortStrategy) -> i32 {
    match sort {
        SortStrategy::ScoreThenIndexAsc => 0,
        SortStrategy::ScoreThenIndexDesc => 1,
        SortStrategy::IndexAsc => 2,
        SortStrategy::IndexDesc => 3,
    }
}

/// `&[Pattern]` -> the header's array; the needles are borrowed from `patterns` for the duration of the call
fn c_patterns(patterns: &[Pattern]) -> Vec<FzbPattern> {
    let zero = FzbScoring {
        match_score: 0, mismatch_penalty: 0, gap_open_penalty: 0, gap_extend_penalty: 0, prefix_bonus: 0, capitalization_bonus: 0, matching_case_bonus: 0,
        exact_match_bonus: 0, delimiter_bonus: 0,
    };
    patterns
        .iter()
        .map(|p| {
            let pc = &p.config;
            FzbPattern {
                needle_utf8: p.needle.as_ptr(),
                needle_len: p.needle.len(),
                negated: p.negated as i32,
                has_max_typos: pc.max_typos.is_some() as i32,
                max_typos: pc.max_typos.map(|t| t as i32).unwrap_or(0),
                casing: pc.casing.map(|c| match c { CaseMatching::Ignore => 0, CaseMatching::Smart => 1, CaseMatching::Respect => 2 }).unwrap_or(-1),
                unicode: pc.unicode.map(|u| match u { UnicodeMatching::Ignore => 0, UnicodeMatching::Smart => 1, UnicodeMatching::Always => 2 }).unwrap_or(-1),
                has_scoring: pc.scoring.is_some() as i32,
                scoring: pc
                    .scoring
                    .as_ref()
                    .map(|s| FzbScoring {
                        match_score: s.match_score, mismatch_penalty: s.mismatch_penalty, gap_open_penalty: s.gap_open_penalty, gap_extend_penalty: s.gap_extend_penalty,
                        prefix_bonus: s.prefix_bonus, capitalization_bonus: s.capitalization_bonus, matching_case_bonus: s.matching_case_bonus,
                        exact_match_bonus: s.exact_match_bonus, delimiter_bonus: s.delimiter_bonus,
                    })
                    .unwrap_or(zero),
                matching: pc.matching.map(|m| m as i32).unwrap_or(-1),
            }
        })
        .collect()
}

fn copy_out(out: *mut FzbMatch, n: usize, matches: &mut Vec<Match>) {
    // Rust's `Match` layout is unspecified (not repr(C)): copy field-wise
    matches.extend(unsafe { std::slice::from_raw_parts(out, n) }.iter().map(|m| Match { index: m.index, score: m.score, exact: m.exact != 0 }));
    unsafe { fzb_matches_free(out) };
}

impl MatcherHip {
    /// `MatcherImpl::new` (src/matcher/algo.rs:57-71).  `sort`: `Specialized::match_list` never sorts, so the backend variant is
    /// built with IndexAsc; the resident / sharded entry points below honour `config.sort` themselves.
    pub fn build(needle: &str, config: &Config) -> Self {
        let cfg = c_config(config, sort_code(&config.sort));
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_matcher_create(&cfg, needle.as_ptr(), needle.len(), &mut handle) });
        Self { handle }
    }

    /// `Matcher::set_pattern` (src/matcher/mod.rs:154-165): the device workspace is kept.
    pub fn set_pattern(&mut self, needle: &str) {
        check(unsafe { fzb_matcher_set_pattern(self.handle, needle.as_ptr(), needle.len()) });
    }

    /// `Specialized::match_list` (src/matcher/algo.rs:17-22): appends, in input order, one `Match` per prefilter-passing haystack.
    /// Uploads the list for this one call — see the module comment: correct, and slower than the CPU crate for a single query.
    pub fn match_list<H: AsRef<str>>(&mut self, haystacks: &[H], haystack_index_offset: u32, matches: &mut Vec<Match>) {
        let corpus = HipCorpus::new(haystacks);
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_match_list_into(self.handle, corpus.handle, 0, corpus.len, haystack_index_offset, &mut out, &mut n) });
        copy_out(out, n, matches);
    }

    /// `Matcher::match_list` over a resident list: scoring, reverse / radix sort on the device, one copy of the ordered records.
    pub fn match_list_resident(&mut self, corpus: &HipCorpus) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_match_list(self.handle, corpus.handle, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    /// `Matcher::match_list_parallel(haystacks, threads)` (src/matcher/parallel.rs:18-89) with the GPUs of the node as workers:
    /// per shard the pipeline on its GPU (records in index order), the runs copied device to device into one list on the current
    /// device, ordered there once (shard order is index order, so this is `match_list`'s post-step), one copy back.  Same result as
    /// `match_list` - what the per-run sort + k-way merge of parallel.rs:66-87 returns, without a host-side merge.
    pub fn match_list_parallel_sharded(&mut self, corpus: &ShardedCorpus) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_match_list_parallel_sharded(self.handle, corpus.handle, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    /// The first `min(limit, found)` entries of `match_list` and `found`, the length of the whole list: what a caller of the reference
    /// gets from `match_list(..)` followed by `truncate(limit)`, with the selection and the ordering done on the device and only
    /// `limit` records copied.
    pub fn match_list_top(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<Match>, usize) {
        let (mut out, mut n, mut found) = (std::ptr::null_mut(), 0usize, 0u64);
        check(unsafe { fzb_match_list_top(self.handle, corpus.handle, limit, &mut out, &mut n, &mut found) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        (v, found as usize)
    }

    /// The first `min(limit, found)` entries of `match_list_indices` over the whole list (`index` = the corpus index) and `found`: what a
    /// picker shows after a keystroke - the best matches with their matched positions.  The reference's caller truncates the Vec
    /// `match_list_indices` returns (src/matcher/mod.rs:234-275); here the top stage, a traced pass over its head and the packing of the
    /// positions are one device call with one host wait.
    pub fn match_list_top_indices(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<MatchIndices>, usize) {
        let (mut out, mut n, mut pos, mut found) = (std::ptr::null_mut(), 0usize, std::ptr::null_mut(), 0u64);
        check(unsafe { fzb_match_list_top_indices(self.handle, corpus.handle, limit, &mut out, &mut n, &mut pos, &mut found) });
        (take_indices(out, n, pos), found as usize)
    }

    /// After `reserve`: no `match_list_top_indices` call with this `limit` or a smaller one, on a needle of up to `max_needle_bytes` bytes,
    /// allocates device memory - also across `set_pattern` / `set_config`.
    pub fn reserve_top_indices(&mut self, corpus: &HipCorpus, limit: usize, max_needle_bytes: usize) {
        check(unsafe { fzb_matcher_reserve_top_indices(self.handle, corpus.handle, limit, max_needle_bytes) });
    }

    /// The empty prompt's index-ordered list left in HBM (a matcher whose needle is empty; the `_device` forms refuse one): the haystacks
    /// of `[first, first + count)` visible under the corpus' scope, score = the clamped bias.  At most `capacity` records at `dev_out`,
    /// `(written, found)` at `dev_count`.  Asynchronous on `stream`.
    ///
    /// # Safety
    /// The two device pointers must be valid for the capacities given, on the device the corpus lives on.
    pub unsafe fn prompt_list_device(&mut self, corpus: &HipCorpus, first: usize, count: usize, index_offset: u32, dev_out: *mut c_void, capacity: usize, dev_count: *mut u32,
                                     stream: *mut c_void) {
        check(fzb_prompt_list_device(self.handle, corpus.handle, std::ptr::null(), first, count, index_offset, dev_out as *mut FzbMatch, capacity, dev_count, stream));
    }

    /// The empty prompt's ordered head left in HBM: `capacity >= min(limit, len)` records at `dev_out`, `(written, found)` at `dev_count`.
    ///
    /// # Safety
    /// The two device pointers must be valid for the capacities given, on the device the corpus lives on.
    pub unsafe fn prompt_top_device(&mut self, corpus: &HipCorpus, limit: usize, dev_out: *mut c_void, capacity: usize, dev_count: *mut u32, stream: *mut c_void) {
        check(fzb_prompt_top_device(self.handle, corpus.handle, std::ptr::null(), limit, dev_out as *mut FzbMatch, capacity, dev_count, stream));
    }

    /// `match_list_top` over a sharded list: every shard selects its own head, only those records reach the root.
    pub fn match_list_top_sharded(&mut self, corpus: &ShardedCorpus, limit: usize) -> (Vec<Match>, usize) {
        let (mut out, mut n, mut found) = (std::ptr::null_mut(), 0usize, 0u64);
        check(unsafe { fzb_match_list_top_sharded(self.handle, corpus.handle, limit, &mut out, &mut n, &mut found) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        (v, found as usize)
    }

    /// `match_list_parallel` with ONE PROCESS PER GPU: this rank scores `shard` (its contiguous share of the list, first global index
    /// `index_offset`), the library all-gathers the run lengths and moves the runs by RCCL over xGMI to rank 0 (`to_all`: to every
    /// rank), a receiver orders the whole list once on its device.  Collective: every rank of the communicator calls it with a matcher
    /// of the same needle and config.  Returns the whole list's `match_list` result on a receiver, an empty Vec elsewhere.
    pub fn match_list_parallel_rccl(&mut self, shard: &HipCorpus, index_offset: u32, comm: &mut ShardComm, to_all: bool) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_match_list_parallel_rccl(self.handle, shard.handle, index_offset, comm.handle, to_all as c_int, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    /// How the runs of the last `match_list_parallel_sharded` reached the root device: gather form and, per shard, same device /
    /// peer access enabled (xGMI, device to device) / peer access refused (the runtime stages the copy through host memory).
    pub fn shard_report(&self) -> String {
        unsafe { std::ffi::CStr::from_ptr(fzb_matcher_shard_report(self.handle)) }.to_string_lossy().into_owned()
    }

    /// `Matcher::match_list_indices` for the listed haystacks of a resident corpus (typically the top of a `match_list` result).
    pub fn match_list_indices(&mut self, corpus: &HipCorpus, selection: &[u32]) -> Vec<MatchIndices> {
        let (mut out, mut n, mut pos) = (std::ptr::null_mut(), 0usize, std::ptr::null_mut());
        check(unsafe { fzb_match_list_indices(self.handle, corpus.handle, selection.as_ptr(), selection.len(), &mut out, &mut n, &mut pos) });
        let v = unsafe { std::slice::from_raw_parts(out, n) }
            .iter()
            .map(|m| MatchIndices {
                index: m.index,
                score: m.score,
                exact: m.exact != 0,
                indices: unsafe { std::slice::from_raw_parts(pos.add(m.positions_begin as usize), m.positions_len as usize) }.to_vec(),
            })
            .collect();
        unsafe { fzb_match_indices_free(out, pos) };
        v
    }
}
// records + flat positions of a *_indices result -> Vec<MatchIndices>; releases the library's arrays
fn take_indices(out: *mut FzbMatchIndices, n: usize, pos: *mut u32) -> Vec<MatchIndices> {
    let v = unsafe { std::slice::from_raw_parts(out, n) }
        .iter()
        .map(|m| MatchIndices {
            index: m.index,
            score: m.score,
            exact: m.exact != 0,
            indices: unsafe { std::slice::from_raw_parts(pos.add(m.positions_begin as usize), m.positions_len as usize) }.to_vec(),
        })
        .collect();
    unsafe { fzb_match_indices_free(out, pos) };
    v
}
impl Drop for MatcherHip {
    fn drop(&mut self) {
        unsafe { fzb_matcher_free(self.handle) }
    }
}
// `Matcher: Send` in the reference; the handle owns device buffers and is used from one thread at a time (`&mut self`)
unsafe impl Send for MatcherHip {}

/// `Matcher::from_patterns(&patterns, &config)` (src/matcher/mod.rs:95-111): the AND / NOT composition of src/matcher/multi.rs on the
/// GPU.  Interactive use keeps ONE of these and calls `set_patterns` with the re-parsed query on every keystroke: the sub-matchers are
/// rebuilt in place and their device buffers kept (after `reserve`, a keystroke allocates nothing).
pub struct HipMultiMatcher {
    handle: *mut c_void,
}

impl HipMultiMatcher {
    pub fn build(patterns: &[Pattern], config: &Config) -> Self {
        let cfg = c_config(config, sort_code(&config.sort));
        let pats = c_patterns(patterns);
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_multi_matcher_create(&cfg, pats.as_ptr(), pats.len(), &mut handle) });
        Self { handle }
    }

    /// `build` with any-of groups: `group_of[i]` is the term id of pattern i; patterns with equal, adjacent ids are the alternatives of
    /// one group, which matches when any of them does and scores their maximum.  The forms with matched positions refuse such a matcher.
    pub fn build_groups(patterns: &[Pattern], group_of: &[u32], config: &Config) -> Self {
        assert_eq!(patterns.len(), group_of.len(), "one term id per pattern");
        let cfg = c_config(config, sort_code(&config.sort));
        let pats = c_patterns(patterns);
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_multi_matcher_create_groups(&cfg, pats.as_ptr(), pats.len(), group_of.as_ptr(), &mut handle) });
        Self { handle }
    }

    /// `set_patterns` with a grouping: skipped when the patterns and the grouping are unchanged.
    pub fn set_pattern_groups(&mut self, patterns: &[Pattern], group_of: &[u32]) {
        assert_eq!(patterns.len(), group_of.len(), "one term id per pattern");
        let pats = c_patterns(patterns);
        check(unsafe { fzb_multi_matcher_set_pattern_groups(self.handle, pats.as_ptr(), pats.len(), group_of.as_ptr()) });
    }

    /// `Matcher::set_patterns` (src/matcher/mod.rs:170-176): skipped when the patterns are the same.
    pub fn set_patterns(&mut self, patterns: &[Pattern]) {
        let pats = c_patterns(patterns);
        check(unsafe { fzb_multi_matcher_set_patterns(self.handle, pats.as_ptr(), pats.len()) });
    }

    /// `Matcher::set_config` (src/matcher/mod.rs:154-162): a change of `sort` alone rebuilds nothing.
    pub fn set_config(&mut self, config: &Config) {
        let cfg = c_config(config, sort_code(&config.sort));
        check(unsafe { fzb_multi_matcher_set_config(self.handle, &cfg) });
    }

    /// Every device buffer queries over `corpus` can need, allocated now.
    pub fn reserve(&mut self, corpus: &HipCorpus) {
        check(unsafe { fzb_multi_matcher_reserve(self.handle, corpus.handle) });
    }

    /// compiled (non-empty) patterns
    pub fn len(&self) -> usize {
        unsafe { fzb_multi_matcher_len(self.handle) }
    }

    /// `Matcher::match_list_into` over the compiled patterns (src/matcher/mod.rs:373-392): input order, the list uploaded for this call.
    pub fn match_list<H: AsRef<str>>(&mut self, haystacks: &[H], haystack_index_offset: u32, matches: &mut Vec<Match>) {
        let corpus = HipCorpus::new(haystacks);
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_multi_match_list_into(self.handle, corpus.handle, 0, corpus.len, haystack_index_offset, &mut out, &mut n) });
        copy_out(out, n, matches);
    }

    /// `Matcher::match_list` over a resident list, ordered per `config.sort` on the device.
    pub fn match_list_resident(&mut self, corpus: &HipCorpus) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_multi_match_list(self.handle, corpus.handle, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    /// `match_list_parallel` with the GPUs of the node as workers: the whole composition per shard on its GPU, gathered and ordered once
    /// on the current device.  Same result as `match_list_resident` on the unsharded list.
    pub fn match_list_parallel_sharded(&mut self, corpus: &ShardedCorpus) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_multi_match_list_parallel_sharded(self.handle, corpus.handle, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    /// The first `min(limit, found)` entries of `match_list` and `found`, the length of the whole list: what a caller of the reference
    /// gets from `match_list(..)` followed by `truncate(limit)`, with the selection and the ordering done on the device and only
    /// `limit` records copied.
    pub fn match_list_top(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<Match>, usize) {
        let (mut out, mut n, mut found) = (std::ptr::null_mut(), 0usize, 0u64);
        check(unsafe { fzb_multi_match_list_top(self.handle, corpus.handle, limit, &mut out, &mut n, &mut found) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        (v, found as usize)
    }

    /// `MatcherHip::match_list_top_indices` for `from_patterns`, fused on the device with one host wait: the multi top stage, one traced
    /// pass per non-negated pattern over its head, the union of their positions (`match_one_indices_multi`) and the pack.
    pub fn match_list_top_indices(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<MatchIndices>, usize) {
        let (mut out, mut n, mut pos, mut found) = (std::ptr::null_mut(), 0usize, std::ptr::null_mut(), 0u64);
        check(unsafe { fzb_multi_match_list_top_indices_fused(self.handle, corpus.handle, limit, &mut out, &mut n, &mut pos, &mut found) });
        (take_indices(out, n, pos), found as usize)
    }

    /// The same as a host composition - the multi top, then the multi matched-indices pass in list order over that head (already in order:
    /// nothing is re-ordered), `index` mapped back to the corpus index: P + 1 round trips, no device-side union.
    pub fn match_list_top_indices_host_composed(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<MatchIndices>, usize) {
        let (mut out, mut n, mut pos, mut found) = (std::ptr::null_mut(), 0usize, std::ptr::null_mut(), 0u64);
        check(unsafe { fzb_multi_match_list_top_indices(self.handle, corpus.handle, limit, &mut out, &mut n, &mut pos, &mut found) });
        (take_indices(out, n, pos), found as usize)
    }

    /// `MatcherHip::match_list_top_indices_device` for `from_patterns`: `positions_capacity >= min(limit, len) x U`, U = the needle bytes of
    /// the non-negated patterns together; four count words at `dev_count`.  Asynchronous on `stream`.
    ///
    /// # Safety
    /// The three device pointers must be valid for the capacities given, on the device the corpus lives on.
    pub unsafe fn match_list_top_indices_device(&mut self, corpus: &HipCorpus, limit: usize, dev_out: *mut c_void, capacity: usize, dev_positions: *mut u32,
                                                positions_capacity: usize, dev_count: *mut u32, stream: *mut c_void) {
        check(fzb_multi_match_list_top_indices_device(self.handle, corpus.handle, limit, dev_out as *mut FzbMatchIndices, capacity, dev_positions, positions_capacity, dev_count, stream));
    }

    /// After `reserve`: no `match_list_top_indices` call with this `limit` or a smaller one allocates device memory, also across
    /// `set_patterns` / `set_config` that add no pattern slot and keep every needle within `max_needle_bytes` bytes.
    pub fn reserve_top_indices(&mut self, corpus: &HipCorpus, limit: usize, max_needle_bytes: usize) {
        check(unsafe { fzb_multi_matcher_reserve_top_indices(self.handle, corpus.handle, limit, max_needle_bytes) });
    }

    /// `match_list_top_indices` for a matcher that may have any-of groups: the records are `match_list_top`'s; a record's positions are
    /// the descending union of every plain non-negated pattern's and of each group's carrier's only - the matching alternative with the
    /// largest key `score << 1 | exact`, the first in query order on equal keys.  Without a group: the ungrouped call.
    pub fn match_list_top_indices_groups(&mut self, corpus: &HipCorpus, limit: usize) -> (Vec<MatchIndices>, usize) {
        let (mut out, mut n, mut pos, mut found) = (std::ptr::null_mut(), 0usize, std::ptr::null_mut(), 0u64);
        check(unsafe {
            fzb_multi_match_list_top_indices_groups(self.handle, corpus.handle, std::ptr::null(), std::ptr::null_mut(), limit, &mut out, &mut n, &mut pos, &mut found)
        });
        (take_indices(out, n, pos), found as usize)
    }

    /// The same left in device memory: `positions_capacity >= min(limit, len) x groups_positions_stride()`.  Asynchronous on `stream`.
    ///
    /// # Safety
    /// The three device pointers must be valid for the capacities given, on the device the corpus lives on.
    pub unsafe fn match_list_top_indices_groups_device(&mut self, corpus: &HipCorpus, limit: usize, dev_out: *mut c_void, capacity: usize, dev_positions: *mut u32,
                                                       positions_capacity: usize, dev_count: *mut u32, stream: *mut c_void) {
        check(fzb_multi_match_list_top_indices_groups_device(self.handle, corpus.handle, std::ptr::null(), std::ptr::null_mut(), limit, dev_out as *mut FzbMatchIndices, capacity,
                                                             dev_positions, positions_capacity, dev_count, stream));
    }

    /// U_g: the plain non-negated patterns' needle bytes + per group the largest among its alternatives.
    pub fn groups_positions_stride(&self) -> usize {
        let mut u = 0usize;
        check(unsafe { fzb_multi_matcher_groups_positions_stride(self.handle, &mut u) });
        u
    }

    /// `reserve_top_indices`, and what the grouped forms own on top.
    pub fn reserve_top_indices_groups(&mut self, corpus: &HipCorpus, limit: usize, max_needle_bytes: usize) {
        check(unsafe { fzb_multi_matcher_reserve_top_indices_groups(self.handle, corpus.handle, limit, max_needle_bytes) });
    }

    /// `match_list_top` over a sharded list: every shard selects its own head, only those records reach the root.
    pub fn match_list_top_sharded(&mut self, corpus: &ShardedCorpus, limit: usize) -> (Vec<Match>, usize) {
        let (mut out, mut n, mut found) = (std::ptr::null_mut(), 0usize, 0u64);
        check(unsafe { fzb_multi_match_list_top_sharded(self.handle, corpus.handle, limit, &mut out, &mut n, &mut found) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        (v, found as usize)
    }

    /// One process per GPU (see `MatcherHip::match_list_parallel_rccl`): this rank's composition is its run.  Collective; a rank that fails
    /// before the exchange makes every rank fail with its error.
    pub fn match_list_parallel_rccl(&mut self, shard: &HipCorpus, index_offset: u32, comm: &mut ShardComm, to_all: bool) -> Vec<Match> {
        let (mut out, mut n) = (std::ptr::null_mut(), 0usize);
        check(unsafe { fzb_multi_match_list_parallel_rccl(self.handle, shard.handle, index_offset, comm.handle, to_all as c_int, &mut out, &mut n) });
        let mut v = Vec::with_capacity(n);
        copy_out(out, n, &mut v);
        v
    }

    pub fn shard_report(&self) -> String {
        unsafe { std::ffi::CStr::from_ptr(fzb_multi_matcher_shard_report(self.handle)) }.to_string_lossy().into_owned()
    }
}
impl Drop for HipMultiMatcher {
    fn drop(&mut self) {
        unsafe { fzb_multi_matcher_free(self.handle) }
    }
}
unsafe impl Send for HipMultiMatcher {}


/// The communicator of the one-process-per-GPU form (`fzb_shard_comm`: an RCCL communicator, a stream and the exchange buffers on the
/// rank's current device).  `ShardComm::unique_id()` on rank 0, the 128 bytes to the other ranks by whatever started them (environment,
/// file, socket, MPI), then `ShardComm::new(&id, rank, world)` on every rank (collective).
pub struct ShardComm {
    handle: *mut c_void,
}

impl ShardComm {
    pub fn unique_id() -> [u8; 128] {
        let mut id = [0u8; 128];
        check(unsafe { fzb_rccl_unique_id(id.as_mut_ptr()) });
        id
    }
    pub fn new(id: &[u8; 128], rank: usize, world: usize) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { fzb_shard_comm_create(id.as_ptr(), rank as c_int, world as c_int, &mut handle) });
        ShardComm { handle }
    }
}

impl Drop for ShardComm {
    fn drop(&mut self) {
        unsafe { fzb_shard_comm_free(self.handle) }
    }
}
