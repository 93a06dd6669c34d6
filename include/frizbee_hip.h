/*
 * frizbee_hip.h - C ABI of the MI355X (gfx950) backend for saghen/frizbee's batched fuzzy-scoring path.
 *
 * This is the drop-in boundary: a Rust `MatcherBackend::Hip` variant binds exactly
 * these entry points.  Each one names the reference interface it replaces (paths relative to the
 * reference crate root).  Plain pointers and sizes only; nothing here depends on torch or HIP types
 * (`void* stream` is a `hipStream_t`, NULL = the default stream).
 *
 * All functions return FZB_OK (0) or an error code; fzb_last_error() returns the message for the
 * calling thread.  Where the reference panics, the message text is the reference's panic text.
 * No function ever unwinds across the boundary.
 */
#ifndef FRIZBEE_HIP_H
#define FRIZBEE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FZB_OK = 0,
    FZB_ERR_INVALID = 1,      /* bad argument (NULL, bad enum, invalid UTF-8 needle)                      */
    FZB_ERR_PANIC = 2,        /* the reference would panic (message = its panic text)                     */
    FZB_ERR_UNSUPPORTED = 3,  /* reserved: nothing returns it since round 3 (needles of every accepted length are handled) */
    FZB_ERR_HIP = 4,          /* HIP runtime error / no device                                            */
    FZB_ERR_CAPACITY = 5      /* caller-provided device buffer too small                                  */
};

/* src/lib.rs:357-368 CaseMatching, :379-392 UnicodeMatching, :311-326 SortStrategy */
enum { FZB_CASE_IGNORE = 0, FZB_CASE_SMART = 1, FZB_CASE_RESPECT = 2 };
enum { FZB_UNICODE_IGNORE = 0, FZB_UNICODE_SMART = 1, FZB_UNICODE_ALWAYS = 2 };
enum { FZB_SORT_SCORE_THEN_INDEX_ASC = 0, FZB_SORT_SCORE_THEN_INDEX_DESC = 1, FZB_SORT_INDEX_ASC = 2, FZB_SORT_INDEX_DESC = 3 };
/* src/lib.rs:414-427 Matching: fuzzy (Smith-Waterman) or one of the literal modes of src/literal (contiguous occurrence) */
enum { FZB_MATCH_FUZZY = 0, FZB_MATCH_EXACT = 1, FZB_MATCH_PREFIX = 2, FZB_MATCH_SUFFIX = 3, FZB_MATCH_SUBSTRING = 4 };

/* src/lib.rs:439-478 `Scoring` (same field order as the Rust struct declaration) */
typedef struct fzb_scoring {
    uint16_t match_score, mismatch_penalty, gap_open_penalty, gap_extend_penalty;
    uint16_t prefix_bonus, capitalization_bonus, matching_case_bonus, exact_match_bonus, delimiter_bonus;
} fzb_scoring;

/* src/lib.rs:236-258 `Config` (+ per-pattern overrides already resolved, src/pattern.rs:250-262).
 * `matching`: the literal modes (src/literal/algo.rs) ignore max_typos and do not depend on pf_lanes / sw_lanes.
 * pf_lanes / sw_lanes select WHICH reference CPU backend the results are bit-exact against, because
 * frizbee's scores, windows and typo-prefilter decisions depend on the SIMD lane count: both 0 = pick the
 * pair the reference's `Matcher::get_backend` (src/matcher/mod.rs:448-498) would pick on THIS host CPU
 * (`is_x86_feature_detected!` predicates) for the needle's score class: AVX-512(+VBMI for the u8 class):
 * prefilter 64, score 64 (u8) / 32 (u16); AVX2: 32, 32 / 16; SSE4.1 or scalar: 16, 16 / 8.
 * Non-zero values force a pair (pf_lanes in {16,32,64}, sw_lanes in {8,16,32,64}); pf_lanes set with sw_lanes 0 = that ISA
 * family's score width for the needle's class (what a multi-pattern matcher needs: its patterns may differ in class). */
typedef struct fzb_config {
    int32_t max_typos; /* Option<u16>: -1 = None (no prefilter) */
    int32_t casing;    /* FZB_CASE_*    */
    int32_t unicode;   /* FZB_UNICODE_* */
    int32_t sort;      /* FZB_SORT_*    */
    fzb_scoring scoring;
    uint16_t pf_lanes, sw_lanes;
    int32_t matching;  /* FZB_MATCH_* */
} fzb_config;

/* src/lib.rs:141-153 `Match` with an explicit layout (Rust's is unspecified; the shim copies field-wise) */
typedef struct fzb_match {
    uint32_t index;
    uint16_t score;
    uint8_t exact;
    uint8_t _pad;
} fzb_match;

typedef struct fzb_matcher fzb_matcher; /* replaces `Matcher` / `MatcherImpl<P,S>` (src/matcher/mod.rs:77-82, algo.rs:47-54) */
typedef struct fzb_corpus fzb_corpus;   /* the `&[S: AsRef<str>]` haystack list, packed and resident in HBM           */

const char* fzb_last_error(void);

/* `Config::default()` (src/lib.rs:260-271) / `Scoring::default()` (src/lib.rs:463-478), lanes = 0 (auto) */
void fzb_config_default(fzb_config* out);

/* `Matcher::new(needle, &config)` (src/matcher/mod.rs:90-111, 178-204) -> `MatcherImpl::new` (algo.rs:57-71):
 * resolves Smart casing/unicode, picks the u8/u16 score class (smith_waterman/mod.rs:92-116), runs
 * `guard_against_score_overflow` (lib.rs:506-537; FZB_ERR_PANIC with the reference's text), builds the
 * device-side needle tables.  An empty needle is valid (matches everything with score 0, mod.rs:381-384). */
int fzb_matcher_create(const fzb_config* config, const uint8_t* needle_utf8, size_t needle_len, fzb_matcher** out);
int fzb_matcher_clone(const fzb_matcher* m, fzb_matcher** out); /* `impl Clone for Matcher` (parallel.rs:46) */
/* `Matcher::set_pattern` / `Matcher::set_config` (src/matcher/mod.rs:154-176): rebuild for a new needle / config; no-ops when nothing
 * changed.  The device workspace (sized by the corpus) is kept: re-querying a resident corpus after every keystroke allocates nothing.
 * On error the matcher is left unchanged. */
int fzb_matcher_set_pattern(fzb_matcher* m, const uint8_t* needle_utf8, size_t needle_len);
int fzb_matcher_set_config(fzb_matcher* m, const fzb_config* config);
void fzb_matcher_free(fzb_matcher* m);
/* introspection: out[0]=pf_lanes out[1]=sw_lanes out[2]=u8 class? out[3]=case_sensitive out[4]=unicode path? out[5]=rows */
int fzb_matcher_info(const fzb_matcher* m, int32_t out[6]);

/* Packs what `match_list(&haystacks)` borrows (src/matcher/mod.rs:212) into device memory:
 * `bytes` = all haystacks concatenated, `end_offsets[i]` = exclusive end of haystack i (n entries).
 * The copy is owned by the library and outlives calls, so repeated queries amortise the upload. */
int fzb_corpus_upload(const uint8_t* bytes, const uint64_t* end_offsets, size_t n, fzb_corpus** out);
/* Same, but the data already lives in HBM (e.g. a torch tensor's data_ptr()) in the library's device layout
 * ("padded-16"): haystack i starts at start(i) = i ? roundup16(dev_ends[i-1]) : 0 and ends (exclusive) at
 * dev_ends[i]; bytes between haystacks are zero; dev_bytes is 16-byte aligned and has >= 80 readable zero
 * bytes after the last haystack.  dev_ends has n entries (uint32 if ends_are_u64 == 0).  Borrowed, not copied.
 * (A list of 32-byte haystacks stored back to back already has this layout.) */
int fzb_corpus_from_device(const void* dev_bytes, const void* dev_ends, int ends_are_u64, size_t n, uint64_t total_bytes, fzb_corpus** out);
/* Optional hint for borrowed corpora: the longest haystack in bytes.  Must be an upper bound; 0 = unknown.  fzb_corpus_upload measures
 * it: on a corpus it uploaded a looser value (or 0) is ignored and a value below the measured one is refused (FZB_ERR_INVALID).  On
 * borrowed memory the bound is CHECKED when it is given: one device pass over the end offsets (a set-up call: it synchronises the
 * device); a haystack longer than max_len, or offsets that decrease / leave the buffer, make the call fail with FZB_ERR_INVALID and name
 * the first offending index.  FZB_VERIFY_PROMISES=0 in the environment skips the pass.
 * A bound within 32 bytes also builds the corpus' LETTER SIGNATURES in the same set-up call (fzb_corpus_signature_info): one 32-bit word
 * per haystack that 0-typo ASCII queries read instead of the bytes of the rows that cannot match.  The corpus' bytes and end offsets must
 * not change after the promise is made; a looser bound, or 0, drops the signatures. */
int fzb_corpus_set_max_len(fzb_corpus* c, uint32_t max_len);
/* Optional accelerator for borrowed RAGGED corpora (fzb_corpus_upload builds it itself): the streaming filter's view of the list - a
 * second copy of the bytes, every 1024-haystack tile sorted by length and stored interleaved in groups of 64, so that a wavefront's
 * loads are contiguous.  The lengths are read from the end offsets (no hint is trusted).  A list that does not
 * call for a view (nothing beyond 32 bytes, more than one haystack in 256 beyond 256 bytes, uniform length) or a device without room leaves the corpus as it
 * is: *out_built (optional) = 1 when the corpus has a view when the call returns.  The corpus' bytes must not change afterwards. */
int fzb_corpus_build_view(fzb_corpus* c, int* out_built);
/* Optional promise for borrowed corpora: EVERY haystack has exactly `len` bytes (so haystack i starts at i * roundup16(len)); the hot
 * kernels then compute the spans instead of reading the end offsets (a tenth of the filter's traffic on 32-byte records and one
 * dependent load less per survivor).  fzb_corpus_upload detects it by itself, and on a corpus it uploaded only the detected value is
 * accepted (FZB_ERR_INVALID otherwise).  A non-zero `len` also becomes the corpus' max_len (overwriting fzb_corpus_set_max_len);
 * 0 clears the promise and the bound it implied.  On borrowed memory the promise is CHECKED against the end offsets when it is made (one
 * device pass, as for fzb_corpus_set_max_len): a wrong promise would mis-span every haystack, so it is refused with FZB_ERR_INVALID.
 * A uniform length within 32 bytes builds the letter signatures as fzb_corpus_set_max_len does, and the same rule holds: the corpus'
 * bytes and end offsets must not change after the promise is made.  0 drops the signatures with the promise. */
int fzb_corpus_set_uniform_len(fzb_corpus* c, uint32_t len);
/* The corpus' letter signatures (frizbee_amd/csrc/sig_filter.h): built by fzb_corpus_upload, by the two promises above on borrowed memory and kept in step by
 * fzb_corpus_append / _truncate / _remove / _replace, for every list whose longest haystack is known and within 32 bytes; an accelerator,
 * like the view: a device without room (or FZB_NO_SIGNATURE=1) leaves the corpus without them and every query as it was.
 * *out_built (optional) = 1 when the corpus has them, *out_bytes (optional) = their size in device memory (4 per haystack). */
int fzb_corpus_signature_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes);
/* The signatures a second time, transposed into BIT-PLANES (one 64-bit word per 1024-haystack tile, signature bit and 64 haystacks: 4 KB per
 * tile, another 4 bytes per haystack), built and kept in step wherever the signatures are: a 0-typo ASCII query over a tile-aligned range
 * reads the planes of its needle's letters only.  Without room for them the corpus keeps its signatures and every query its result.
 * *out_built (optional) = 1 when the corpus has them, *out_bytes (optional) = their size in device memory (4096 per started tile). */
int fzb_corpus_signature_planes_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes);
/* The REPEAT planes: the same layout once more (another 4 bytes per haystack, an allocation of its own), bit b of a haystack = its bytes hold
 * signature bit b at least twice.  Built from the haystack bytes and kept in step wherever the bit-planes are; a query whose needle repeats
 * a letter (`deadbe`: d and e) reads the repeat planes of those letters too and so skips the rows that hold them once.  Without room for
 * them the corpus keeps its planes and every query its result.
 * *out_built (optional) = 1 when the corpus has them, *out_bytes (optional) = their size in device memory (4096 per started tile). */
int fzb_corpus_signature_repeat_planes_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes);
void fzb_corpus_free(fzb_corpus* c);
size_t fzb_corpus_len(const fzb_corpus* c);

/* A corpus that GROWS (a picker's list arrives in batches while the user types).  For a corpus the library owns - made by
 * fzb_corpus_upload, also with n = 0, which is how a picker starts; a borrowed one (fzb_corpus_from_device) gets FZB_ERR_INVALID.
 * After any sequence of these calls the corpus answers every query - every entry point that takes an fzb_corpus - exactly as a
 * fzb_corpus_upload of the same list would: same padded-16 layout, same measured max_len / uniform_len (fzb_corpus_set_max_len /
 * _set_uniform_len accept the values as they are after the call), same decision about the filter's view.  fzb_sharded_corpus and the
 * RCCL form are out of scope: a sharded corpus stays as uploaded.
 * All three are SET-UP calls like the upload: they wait for the device's outstanding work on entry and are complete on return, on the
 * device the corpus was uploaded on (which must be current).  The caller must not run them concurrently with queries over the same
 * corpus from other threads.  An error leaves the corpus as it was, answering as before the call. */
/* room for `items` haystacks and `bytes` padded bytes without another device allocation; never shrinks */
int fzb_corpus_reserve(fzb_corpus* c, size_t items, uint64_t bytes);
/* (padded bytes: every haystack rounded up to 16, at most the raw bytes + 15 per haystack.  The room covers the canonical layout, the
 * landing place of a batch as large as the room, and - unless FZB_FILTER_VIEW=0 - the filter's view of a full list.  With
 * fzb_matcher_reserve / fzb_multi_matcher_reserve made afterwards - they size for max(len, reserved items) - neither an append within
 * the room nor a query allocates device memory.) */
/* haystacks n .. n+n_new-1: `bytes` = the batch's haystacks back to back, end_offsets[i] = exclusive end of batch item i
 * counted from the batch's first byte (what pack() yields for the batch alone) */
int fzb_corpus_append(fzb_corpus* c, const uint8_t* bytes, const uint64_t* end_offsets, size_t n_new);
/* (Each haystack crosses the link once: the two arrays are copied as they are and laid out on the device behind the last haystack;
 * nothing resident is copied unless room is lacking - then the array that lacks it grows to at least twice its size, or to the exact
 * size when the device refuses that, FZB_ERR_HIP when it refuses both.  The filter's view is rebuilt from the last, partial tile of
 * 1024 haystacks on.  n_new == 0 is a no-op.  Offsets that decrease: FZB_ERR_INVALID "end_offsets must be non-decreasing"; more than
 * 4 294 967 295 haystacks: FZB_ERR_PANIC with the reference's text.  End offsets stay 32-bit on a corpus that was uploaded with less
 * than 4 GiB of padded bytes: a batch that would take it past 0xFFFFFFF0 is REFUSED with FZB_ERR_CAPACITY - they are not widened.) */
/* keep the first n haystacks (n <= len; n == 0 empties the corpus); capacity is kept */
int fzb_corpus_truncate(fzb_corpus* c, size_t n);
/* introspection: out[0]=items [1]=item capacity [2]=padded bytes used [3]=byte capacity [4]=max_len [5]=uniform_len [6]=has a filter view
 * (0/1) [7]=view_nv [8]=outliers (haystacks beyond 256 bytes the view lists) [9]=end offsets are u64 (0/1) [10]=regrows so far
 * [11]=bytes copied host to device so far (haystack bytes + 8 per offset) */
int fzb_corpus_info(const fzb_corpus* c, uint64_t out[12]);

/* A corpus that is EDITED: haystacks removed or replaced anywhere in the list (a file watcher reports a deleted or renamed path, the
 * user hides a directory).  Same family, same rules as the calls above: only for a corpus made by fzb_corpus_upload (a borrowed one gets
 * FZB_ERR_INVALID); fzb_sharded_corpus and the RCCL form are out of scope; SET-UP calls that wait for the device's outstanding work
 * on entry and are complete on return, on the corpus' device (which must be current); not to be run concurrently with queries over
 * the same corpus.  Afterwards the corpus answers every entry point that takes an fzb_corpus exactly as a fzb_corpus_upload of the
 * edited list would: same padded-16 bytes and zero tail, same end offsets, same re-measured max_len / uniform_len (a removal can lower
 * max_len or make the list uniform), same decision about the filter's view; capacity and the width of the end offsets are kept.
 * An error leaves the corpus exactly as it was: every check and every allocation comes before the first write to a resident array.
 * Work: with i0 = the first touched haystack, nothing in front of i0 is read or written; the suffix from i0 on is laid out again on the
 * device (one read and one write of it through scratch, plus the copy into place) and the filter's view is rebuilt from tile
 * i0 / 1024 on.  Only the indices - and a replace's new bytes - cross the link.
 * Temporary device memory, released before the call returns: len / 8 bytes (one bit per haystack) + 24 bytes per 1024 haystacks +
 * the index list (host forms) + the scratch the suffix passes through: one chunk of FZB_EDIT_CHUNK_ITEMS source haystacks (default
 * 1 048 576) at a time - that chunk's new padded bytes + 8 (4) bytes per haystack of it - taken from the corpus' landing buffers where
 * they are large enough.  A replace whose growing items push later haystacks towards HIGHER addresses cannot go chunk by chunk: it
 * takes the whole new suffix through the scratch at once.  A refused allocation: FZB_ERR_HIP, corpus unchanged. */
/* Removes the haystacks named by `indices` (host memory, any order; a repeated index removes its haystack once).  The others keep
 * their order and are renumbered, as Vec::retain would.  n_indices == 0 is a no-op.  An index >= len: FZB_ERR_INVALID, the message
 * names the first offending position. */
int fzb_corpus_remove(fzb_corpus* c, const uint32_t* indices, size_t n_indices);
/* The same with the index list in HBM: entry k is the uint32 at byte k * stride_bytes of dev_indices (stride_bytes >= 4 and a multiple
 * of 4; both pointers 4-byte aligned), the number of entries is min(*dev_count, max_count).  With stride_bytes = 8 this reads the
 * record buffer that fzb_match_list_device or fzb_multi_match_list_device wrote over the WHOLE corpus with index_offset 0 (an fzb_match is 8 bytes and
 * begins with its uint32 index; dev_count = their dev_count, whose first word is the number of records written): "drop everything that matches this query" without a host
 * round trip.  The list cannot be checked on the host: a kernel validates it and its result is read back before anything is written;
 * an entry >= len gives FZB_ERR_INVALID (naming the first offending position) and leaves the corpus unchanged. */
int fzb_corpus_remove_device(fzb_corpus* c, const void* dev_indices, size_t stride_bytes, const uint32_t* dev_count, size_t max_count);
/* Batch item k (`bytes` / `end_offsets`: the batch format of fzb_corpus_append) becomes the content of haystack indices[k].  Lengths may
 * change in either direction, to empty and to beyond 256 bytes.  Indices must be in range and unique (a duplicate: FZB_ERR_INVALID);
 * their order is free.  Offsets that decrease: FZB_ERR_INVALID "end_offsets must be non-decreasing".  Room is found as in append
 * (geometric regrow, counted in fzb_corpus_info's regrows), and the 4 GiB rule is append's: FZB_ERR_CAPACITY when the new content would
 * take a corpus with 32-bit end offsets past 0xFFFFFFF0 padded bytes - they are not widened.  n == 0 is a no-op. */
int fzb_corpus_replace(fzb_corpus* c, const uint32_t* indices, size_t n, const uint8_t* bytes, const uint64_t* end_offsets);
/* The last successful fzb_corpus_remove / _remove_device / _replace that changed the corpus (all zero before the first): out[0] = first
 * haystack index whose position or content changed, [1] = bytes of the canonical layout written (new suffix + cleared bytes + end
 * offsets: at most the old used bytes behind start(out[0]) - more only where a replace grew the list - + 8 per offset behind out[0]),
 * [2] = 1024-haystack tiles of the filter's view rebuilt, [3] = peak temporary device bytes. */
int fzb_corpus_edit_info(const fzb_corpus* c, uint64_t out[4]);

/* A PER-HAYSTACK SCORE BIAS, applied on the device.  Real pickers do not rank by the match score alone: they add a per-item term - frecency,
 * "file is open", "modified in git", a penalty for vendored paths.  The reference has no such term: its `match_list` returns the whole Vec and
 * the caller adds the term on the host and sorts again - which a top-`limit` call cannot serve, because selecting before the boost is added
 * picks the wrong records.  Here the corpus keeps one int16 per haystack (bias[i] belongs to haystack i) and a record's reported score becomes
 *     clamp(score + bias[i], 0, 65535)
 * where `score` is what the library reports without a bias: the single pattern's score with the exact-match bonus, or the multi-pattern
 * saturating sum (the bias is added ONCE per record, after the sum).  The add runs between the scorers and the selection / ordering stage
 * (one short launch over the index-ordered records, frizbee_amd/csrc/score_bias.h), so the threshold, the selection, the radix sort and the
 * pack of the positions all work on the ranking the user sees.  Nothing else changes: which haystacks match, `found`, `exact`, the matched
 * positions, min_haystack_len and the prefilter are those of the unbiased query; a score biased down to 0 stays in the result.  Ordering is the
 * reference's rule (src/matcher/mod.rs:215-221, src/sort.rs:6-40) over the biased scores: index order, reversed for the *Desc strategies, then
 * the stable descending sort by score for the Score* strategies; fzb_match_list_top stays "the first min(limit, found) records of
 * fzb_match_list".  A corpus without a bias takes exactly the launches it took before.
 * The bias is a property of the LIST, not of a query: it survives fzb_matcher_set_pattern / fzb_multi_matcher_set_patterns untouched and stays
 * in step with the editing family - fzb_corpus_reserve grows it with the item capacity, appended haystacks start at 0 (every entry at or
 * behind the list's length is zero), fzb_corpus_truncate clears the cut entries, fzb_corpus_remove / _remove_device compact the kept entries on
 * the device (2 bytes of scratch per haystack from the first removed one on, counted in fzb_corpus_edit_info's out[3]), fzb_corpus_replace
 * leaves it alone: the index is the identity, a renamed path keeps its bias.  Shards (fzb_sharded_corpus) have no bias.
 * Every entry point that takes an fzb_corpus either returns biased scores or refuses a biased corpus with FZB_ERR_INVALID (the message says
 * "bias" and names the call to use instead); none ignores the bias silently.  Biased: fzb_match_list / _into / _device / _sorted_device /
 * _parallel, fzb_match_list_top / _top_device, fzb_match_list_top_indices / _device, fzb_match_list_indices / _into, fzb_multi_match_list /
 * _into / _device / _top / _parallel, fzb_multi_match_list_top_indices_fused / _device.  Refused: fzb_multi_match_list_indices / _indices_into,
 * the composed fzb_multi_match_list_top_indices (use the fused form), fzb_match_list_parallel_rccl / fzb_multi_match_list_parallel_rccl (a
 * biased shard is a rank-local failure that travels in the gathered status word like any other).
 * fzb_merge_shard_runs takes runs, not a corpus: it orders by what the matcher alone can produce, so runs that fzb_match_list_device /
 * fzb_multi_match_list_device wrote over a BIASED corpus must not be handed to it (their scores may pass the bound its single radix pass
 * rests on); frizbee_amd.distributed.ShardExchange raises for a biased shard it is shown (check_corpus, ordered_query(corpus=...)).
 * AN EMPTY NEEDLE / NO PATTERN over a biased corpus is the picker's empty prompt, "most frecent first": every haystack matches with score
 * clamp(bias, 0, 65535) and - a DEPARTURE from the reference, whose empty result is never sorted - the list IS ordered by `config.sort`
 * (fzb_match_list, _parallel, _into (index order), _top, _top_indices with no positions, and the multi forms).  The single matcher's
 * prompt runs on the device: one kernel writes the index-ordered records from the bias column, the matcher's selection and ordering stage
 * takes them from there, and the host forms copy back the head and the count pair in their one wait - no column crosses the link; after
 * fzb_matcher_reserve(m, c) such a query allocates no device memory.  The _device forms keep refusing an empty needle; the prompt's own
 * _device forms are fzb_prompt_list_device / fzb_prompt_top_device.
 * These are SET-UP calls under the editing family's rules: only for a corpus made by fzb_corpus_upload (a borrowed one gets FZB_ERR_INVALID),
 * they wait for the device's outstanding work on entry and are complete on return, must not run concurrently with queries over the same
 * corpus, and an error leaves the corpus as it was. */
/* bias[i] = values[i] for every haystack: n must equal the corpus length (FZB_ERR_INVALID otherwise).  One host-to-device copy; the array is
 * created on first use, sized for max(length, reserved items). */
int fzb_corpus_set_bias(fzb_corpus* c, const int16_t* values, size_t n);
/* Sparse set - what a picker does when a file is opened: bias[indices[k]] = values[k].  Checked on the host: an index >= the corpus length or a
 * repeated index gives FZB_ERR_INVALID naming the position, nothing written.  One copy of the pairs and one scatter kernel (up to 4096 pairs
 * allocate nothing once the corpus has a bias).  On a corpus without a bias an all-zero one is created first.  n == 0 is a no-op. */
int fzb_corpus_update_bias(fzb_corpus* c, const uint32_t* indices, const int16_t* values, size_t n);
/* the corpus answers exactly as before any bias (the array is kept for the next fzb_corpus_set_bias / _update_bias) */
int fzb_corpus_clear_bias(fzb_corpus* c);
/* out[0] = carries a bias (0/1), [1] = entries the array has room for, [2] = bias_hi: the host-side upper bound of the largest positive bias
 * (exact after fzb_corpus_set_bias, max(old, new values) after fzb_corpus_update_bias, 0 after clear, never lowered by an edit) - while
 * max matrix score + exact_match_bonus + bias_hi < 256 the ordering keeps its single radix pass and the selection its single histogram
 * level -, [3] = device bytes (the array and the landing place of an update's pairs) */
int fzb_corpus_bias_info(const fzb_corpus* c, uint64_t out[4]);

/* PER-HAYSTACK TAGS AND A VISIBILITY SCOPE, applied on the device.  The other per-item term every picker has is a filter: "hide git-ignored
 * files", "hide hidden files", "only tracked files", "not under vendor/", "only this workspace folder".  A corpus the library owns can carry
 * one uint16 of TAGS per haystack - 16 caller-defined bits - and a SCOPE, a pair (require, exclude) of uint16 masks.  Haystack i is visible iff
 *     (tags[i] & require) == require  &&  (tags[i] & exclude) == 0
 * (a bit in both masks hides every haystack).  The contract is one sentence:
 *     A query over a scoped corpus returns what the same query returns over a fzb_corpus_upload of the visible haystacks alone, in their
 *     order, with every `index` mapped back to the haystack's index in the full list.
 * The map is monotone, so the reference's ordering rule (reverse for the *Desc strategies, then the stable descending sort by score:
 * src/matcher/mod.rs:215-221, src/sort.rs:6-40) and the tie-breaks at the cut of a top-`limit` call are preserved; `found` counts visible
 * matches only; scores, `exact` and the matched positions of a visible haystack are untouched; a score bias, when present, is added as before,
 * to the visible records; the range forms number the visible haystacks of the range, index = index_offset + (i - first).  The records of
 * hidden haystacks are dropped between the scorers (or the multi-pattern composition) and the bias / selection / ordering stage: a flag pass
 * and a stable compaction over the index-ordered records (frizbee_amd/csrc/scope.h; two short launches), ahead of which the records go to a
 * scratch of the matcher's with room for one per haystack, so `found` over a scoped corpus is always exact.  The _device forms write
 * dev_count[0] = min(visible matches, capacity), dev_count[1] = visible matches, and the first `capacity` of them.
 * The tags are a property of the LIST, like the bias: they survive fzb_matcher_set_pattern / fzb_multi_matcher_set_patterns and follow the
 * editing family under the bias' invariant (every entry at or behind the list's length is zero) - fzb_corpus_reserve grows the array with the
 * item capacity, appended haystacks start with tag 0, fzb_corpus_truncate clears the cut entries, fzb_corpus_remove / _remove_device compact
 * the kept entries through the bias' pass (2 more bytes of scratch per haystack from the first removed one on, counted in
 * fzb_corpus_edit_info's out[3]), fzb_corpus_replace leaves them alone.  Changing the SCOPE is host-only: two words that travel as kernel
 * arguments, no device work, no allocation - the "toggle ignored files" keystroke.  A scope of (0, 0) is no scope, and a corpus without an
 * active scope, with or without tags, takes exactly the launches and allocations it took before.  After fzb_matcher_reserve /
 * fzb_multi_matcher_reserve on a corpus that carries tags no scoped query allocates device memory.  Shards (fzb_sharded_corpus) have no tags.
 * Every entry point that takes an fzb_corpus either HONOURS an active scope or REFUSES it with FZB_ERR_INVALID (the message says "scope" and
 * names the call to use instead); none ignores the scope.  Honoured: fzb_match_list / _into / _device / _sorted_device / _parallel,
 * fzb_match_list_top / _top_device, fzb_match_list_top_indices / _device, fzb_multi_match_list / _into / _device / _top / _parallel,
 * fzb_multi_match_list_top_indices_fused / _device - an empty needle and an empty pattern list included (the picker's empty prompt with
 * "hide ignored" switched on: the visible haystacks, score 0 or the clamped bias; for the single matcher a flag pass over the tags and a
 * stable compaction that writes the finished records, on the device - fzb_prompt_list_device / fzb_prompt_top_device are its _device forms).
 * Refused: the list-order matched-indices forms fzb_match_list_indices / _indices_into and fzb_multi_match_list_indices / _indices_into (use
 * the top-`limit` forms with positions), the composed fzb_multi_match_list_top_indices (use the fused form), fzb_match_list_parallel_rccl /
 * fzb_multi_match_list_parallel_rccl (a scoped shard is a rank-local failure that travels in the gathered status word like any other);
 * frizbee_amd.distributed.ShardExchange raises for a scoped shard it is shown (check_corpus).
 * These are SET-UP calls under the bias' rules: only for a corpus made by fzb_corpus_upload (a borrowed one gets FZB_ERR_INVALID), they wait
 * for the device's outstanding work on entry and are complete on return, must not run concurrently with queries over the same corpus, and an
 * error leaves the corpus as it was. */
/* tags[i] = values[i] for every haystack: n must equal the corpus length (FZB_ERR_INVALID otherwise).  One host-to-device copy; the array is
 * created on first use, sized for max(length, reserved items).  The scope stays as it is. */
int fzb_corpus_set_tags(fzb_corpus* c, const uint16_t* values, size_t n);
/* Sparse set: tags[indices[k]] = values[k].  Checked on the host: an index >= the corpus length or a repeated index gives FZB_ERR_INVALID
 * naming the position, nothing written.  One copy of the pairs (through the landing place fzb_corpus_update_bias uses) and one scatter
 * kernel (up to 4096 pairs allocate nothing once the corpus carries tags).  On a corpus without tags an all-zero array is created first.
 * n == 0 is a no-op. */
int fzb_corpus_update_tags(fzb_corpus* c, const uint32_t* indices, const uint16_t* values, size_t n);
/* all tags 0 and the scope (0, 0): the corpus answers as before any tags; the array is kept */
int fzb_corpus_clear_tags(fzb_corpus* c);
/* The scope of the queries that follow.  Host only; on a corpus without tags an all-zero array is created first (that once is a set-up call as
 * above).  (0, 0) switches the scope off. */
int fzb_corpus_set_scope(fzb_corpus* c, uint16_t require, uint16_t exclude);
/* out[0] = a scope is active (0/1), [1] = entries the tags array has room for (0: the corpus carries no tags), [2] = require | exclude << 16,
 * [3] = device bytes of the array (the landing place of an update's pairs is shared with the bias and counted in fzb_corpus_bias_info) */
int fzb_corpus_scope_info(const fzb_corpus* c, uint64_t out[4]);

/* `Matcher::match_list(&haystacks)` (src/matcher/mod.rs:212-222) = `match_list_into(.., offset 0)` ->
* `Specialized::match_list::<TYPOS,UNICODE,_>` (src/matcher/algo.rs:78-103) and the reverse / `radix_sort_matches`
 * post-step (src/sort.rs:6-40), all on the GPU.  `*out` is malloc'd by the library
 * (free with fzb_matches_free) and holds exactly the Vec<Match> the reference returns, in its order. */
int fzb_match_list(fzb_matcher* m, const fzb_corpus* c, fzb_match** out, size_t* out_len);

/* `Specialized::match_list(&mut self, haystacks, haystack_index_offset, &mut matches)`
 * (src/matcher/algo.rs:17-22, backend.rs:95-107): appends, in input order, one Match per prefilter-passing
 * haystack of the sub-range [first, first+count) with `index = index_offset + (i - first)`; no sorting.
 * This is the seam `MatcherBackend::Hip` implements and what `match_list_parallel`'s per-shard workers call. */
int fzb_match_list_into(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match** out, size_t* out_len);

/* Allocates, once, every device buffer the queries of this matcher over corpus `c` can need (the matcher keeps them across
 * fzb_matcher_set_pattern / fzb_matcher_set_config): after it no query allocates - the keystroke-latency use (SURVEY 8f rank 2,
 * callers `Matcher::set_pattern`, src/matcher/mod.rs:154-176).  Optional: without it the buffers grow on first use. */
int fzb_matcher_reserve(fzb_matcher* m, const fzb_corpus* c);

/* Device-resident form of the above for callers that keep results in HBM (benchmarks, multi-GPU gather):
 * writes the index-ordered records to dev_out (capacity records) and the counts to dev_count - TWO uint32 in device memory:
 * dev_count[0] = records written = min(matches, capacity), dev_count[1] = matches found (not clamped) - asynchronously on
 * `stream`.  No host synchronisation.
 * CAPACITY: nothing on the host knows the number of matches when the call returns, so a buffer that is too small cannot be
 * refused: the records at positions >= capacity are NOT written (for the sorted form the sort then orders that truncated prefix -
 * its head is not the head of the full list), and dev_count[1] > capacity is how the reader of the buffer sees it
 * (frizbee_amd.distributed.ShardExchange raises on it).  capacity >= count (one record per haystack of the range) can never
 * truncate.  FZB_ERR_CAPACITY is returned where the host does know: an empty pattern list. */
int fzb_match_list_device(fzb_matcher* m, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset,
                          fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);

/* `Matcher::match_list` entirely in HBM: the records of the WHOLE corpus in the order `config.sort` asks for
 * (reverse for the *Desc strategies, then the stable descending radix sort of src/sort.rs:6-40 for the Score* strategies,
 * both as device kernels).  fzb_match_list is this call + one device-to-host copy. */
int fzb_match_list_sorted_device(fzb_matcher* m, const fzb_corpus* c, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);

/* TOP-`limit` QUERIES.  The reference has no such call: its `match_list` returns a Vec and the caller truncates it.  The contract here is
 * exactly that truncation: top(limit) = the first min(limit, found) records of what fzb_match_list returns for the same matcher and
 * corpus, in the same order, ties at the cut broken as the stable sort breaks them (the reverse for the *Desc strategies happens before
 * the sort: src/matcher/mod.rs:215-221, src/sort.rs:6-40 - lowest indices win for ScoreThenIndexAsc, highest for ScoreThenIndexDesc;
 * IndexAsc / IndexDesc: the first / last `limit` matches in index order), and found = the length of the full list.  limit = 0 is valid
 * (no records, found still reported); limit >= found returns the whole list.  With an empty needle every haystack matches with score 0
 * (host work, as in fzb_match_list).  The threshold score, the selection of the head's records and their ordering run on the device;
 * only min(limit, corpus length) records are copied.
 * Host result: *out (fzb_matches_free) holds min(limit, found) records; *out_found (optional) = matches found. */
int fzb_match_list_top(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
/* The same with the result left in HBM and no host synchronisation: dev_out has room for `capacity` >= min(limit, corpus length) records
 * (less: FZB_ERR_CAPACITY, nothing launched), dev_count[0] = records written = min(limit, found), dev_count[1] = found; asynchronous on
 * `stream`.  Not for an empty needle (FZB_ERR_INVALID). */
int fzb_match_list_top_device(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);

/* `Matcher::match_list_parallel(&haystacks, threads)` (src/matcher/parallel.rs:18-89).  The GPU processes the
 * whole list in one pass, so `threads` only keeps the reference's contract: 0 => FZB_ERR_PANIC
 * "threads must be positive"; the result equals fzb_match_list for every thread count (parallel.rs:104-130). */
int fzb_match_list_parallel(fzb_matcher* m, const fzb_corpus* c, size_t threads, fzb_match** out, size_t* out_len);

void fzb_matches_free(fzb_match* p);

/* ---- the multi-device form: `Matcher::match_list_parallel` with the GPUs of one node as its workers ---------------------------
 * The reference's match_list_parallel (src/matcher/parallel.rs:18-89) cuts the list into contiguous chunks, hands every worker thread
 * a chunk with its global index offset (:55-63), sorts each worker's run (:66-76) and k-way merges the runs (:78-87).  Here a worker
 * is a DEVICE: the list is cut into `ndev` contiguous shards, shard g resident on device g; a query runs one persistent host thread
 * per shard (hipSetDevice + a per-shard clone of the matcher: the pipeline on that GPU, records in index order) and each run is
 * copied device to device to its place in ONE list on the root device (the caller's current device).  Shard order is ascending index
 * order, so that list is the one `match_list` orders: the root runs the reverse / stable radix sort of src/sort.rs:6-40 once and makes
 * one copy to the host.  The result equals fzb_match_list on the unsharded list for every sort strategy - what the reference's per-run
 * sort + k-way merge produces, without a host-side merge.  (`threads` of fzb_match_list_parallel keeps the reference's contract on ONE
 * device; the number of devices is a property of the sharded corpus, never inferred from `threads`.) */
typedef struct fzb_sharded_corpus fzb_sharded_corpus;
enum {
    FZB_SHARD_BY_COUNT = 0,       /* shard g = [g * ceil(n / ndev), ...): equal haystack counts                           */
    FZB_SHARD_BY_BYTES = 1,       /* shard g starts at the first haystack that starts at or after g/ndev of the bytes (ragged lists) */
    FZB_SHARD_OVERSUBSCRIBE = 2   /* more shards than visible devices is allowed: shard g lives on device g % devices (testing)     */
};
int fzb_device_count(int* out);
/* the shard boundaries (haystack indices) the upload uses: out_bounds has nshards + 1 entries; host arithmetic only */
int fzb_shard_ranges(const uint64_t* end_offsets, size_t n, int nshards, int by_bytes, uint64_t* out_bounds);
/* fzb_corpus_upload of every shard onto its device, the shards in parallel.  FZB_ERR_HIP when fewer than ndev devices are visible
 * (unless FZB_SHARD_OVERSUBSCRIBE). */
int fzb_corpus_upload_sharded(const uint8_t* bytes, const uint64_t* end_offsets, size_t n, int ndev, int flags, fzb_sharded_corpus** out);
void fzb_sharded_corpus_free(fzb_sharded_corpus* sc);
size_t fzb_sharded_corpus_len(const fzb_sharded_corpus* sc);
int fzb_sharded_corpus_shards(const fzb_sharded_corpus* sc);
int fzb_sharded_corpus_shard(const fzb_sharded_corpus* sc, int g, uint64_t* lo, uint64_t* hi, int* device);
/* `Matcher::match_list_parallel(&haystacks, threads)` over the sharded list, one worker per shard.  The matcher keeps one clone of
 * itself per shard (device workspaces on the shards' devices; they follow fzb_matcher_set_pattern / fzb_matcher_set_config, and a
 * clone whose shard lives on another device in a later corpus is rebuilt there) and its worker threads.  The caller's current device
 * is the root (the matcher binds to it like on any first query).  fzb_last_counters on `m` afterwards = the sum over the shards.
 * Free the result with fzb_matches_free. */
int fzb_match_list_parallel_sharded(fzb_matcher* m, const fzb_sharded_corpus* sc, fzb_match** out, size_t* out_len);
/* fzb_match_list_top over the sharded list: every shard selects its own head (at most `limit` records) on its device, only those
 * travel to the root, which selects and orders once more; *out_found = the sum over the shards. */
int fzb_match_list_top_sharded(fzb_matcher* m, const fzb_sharded_corpus* sc, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
/* How the runs of the last fzb_match_list_parallel_sharded on `m` reached the root, as text: the gather form and, per shard, "same
 * device", "peer access enabled (device to device over xGMI)" or "peer access REFUSED ..." (hipDeviceCanAccessPeer /
 * hipDeviceEnablePeerAccess are asked once per (root, device) pair; without peer access the runtime stages hipMemcpyPeerAsync through
 * host memory - correct, slower, and said here rather than silently).  The reference has no counterpart: its workers share one address
 * space (src/matcher/parallel.rs:43-64).  The string lives until the next sharded query on `m` or fzb_matcher_free. */
const char* fzb_matcher_shard_report(const fzb_matcher* m);
/* The combine step alone, for callers that moved the per-shard runs themselves (one process per GPU: the root rank after an RCCL
 * gather - frizbee_amd.distributed): run g = dev_runs[g], index-ordered records of shard g as fzb_match_list_device wrote them,
 * dev_counts[g] -> the two uint32 that call wrote in DEVICE memory (records written, matches found), run_caps[g] = the run's buffer size
 * in records (a run with matches found > run_caps[g] was truncated by its producer: FZB_ERR_CAPACITY, nothing merged); runs in ascending
 * shard order, all readable from the current device, none written over a corpus that carries a score bias (fzb_corpus_set_bias).  Concatenation + `match_list`'s ordering (src/matcher/mod.rs:215-221) on the device, on `stream`, then one copy to the
 * host = the list `match_list_parallel` returns (src/matcher/parallel.rs:66-87).  Free the result with fzb_matches_free. */
int fzb_merge_shard_runs(fzb_matcher* m, const void* const* dev_runs, const uint32_t* const* dev_counts, const size_t* run_caps, size_t nruns, void* stream,
                         fzb_match** out, size_t* out_len);

/* `Matcher::match_list_parallel` (src/matcher/parallel.rs:18-89) with ONE PROCESS PER GPU: the workers of parallel.rs:43-64 are the
 * ranks, each holding its contiguous share of the list as its own corpus (fzb_shard_ranges gives the boundaries), and what the
 * reference's workers hand back through shared memory (parallel.rs:66-87) travels by RCCL over xGMI below this boundary - nothing above
 * it (Rust, C++, Python) links a collective library.  RCCL is opened at run time (librccl.so.1): FZB_ERR_HIP with the loader's message
 * when the process cannot get one.
 *   fzb_rccl_unique_id       rank 0 draws the communicator's id (ncclGetUniqueId); the HOST moves these 128 bytes to the other ranks by
 *                            whatever channel started them (environment, file, socket, MPI): the one out-of-band step
 *   fzb_shard_comm_create    COLLECTIVE (every rank of `world` calls it, ncclCommInitRank) on the rank's current device; owns a stream
 *                            and the exchange buffers, which grow on demand and are reused by later queries
 *   fzb_match_list_parallel_rccl   COLLECTIVE: rank g scores `shard` (its share, records numbered from index_offset = the share's first
 *                            global index), the runs' lengths are all-gathered (8 bytes per rank, the call's one host synchronisation
 *                            before the result), then ONE RCCL group moves every run - exactly its records, not a capacity - to rank 0
 *                            (flags = 0), or to every rank (FZB_GATHER_ALL: the all-gather of variable-length runs); a receiver
 *                            concatenates in rank order (= ascending index order), applies `match_list`'s ordering once on its device
 *                            (src/matcher/mod.rs:215-221) and copies the list to its host: *out / *out_len = the list
 *                            `match_list_parallel` returns for the WHOLE list, to be freed with fzb_matches_free; on a rank that does
 *                            not receive, *out = NULL and *out_len = 0.  Every rank must pass a matcher of the same needle and config.
 *   fzb_shard_comm_last_exchange   out_bytes[0] / [1] = record bytes this rank sent / received in its last query.
 * Every rank-local step (device check, u32 index guard, buffers, this rank's pipeline) runs before the count all-gather, and its outcome travels
 * with the counts: when any rank failed there, EVERY rank returns that rank's error code and nothing is exchanged.  Only a NULL handle or an
 * unknown flag returns before the collective (it cannot take part) - and a receiver that cannot grow its receive buffer after the all-gather
 * leaves its senders without a counterpart; treat an error of a collective call as the end of that communicator.  One communicator per thread;
 * a communicator and the matchers used with it belong to the device that was current in fzb_shard_comm_create. */
#define FZB_RCCL_ID_BYTES 128
typedef struct fzb_shard_comm fzb_shard_comm;
enum { FZB_GATHER_ROOT = 0, FZB_GATHER_ALL = 1 };
int fzb_rccl_unique_id(uint8_t out_id[FZB_RCCL_ID_BYTES]);
int fzb_shard_comm_create(const uint8_t id[FZB_RCCL_ID_BYTES], int rank, int world, fzb_shard_comm** out);
void fzb_shard_comm_free(fzb_shard_comm* comm);
int fzb_shard_comm_rank(const fzb_shard_comm* comm);
int fzb_shard_comm_world(const fzb_shard_comm* comm);
int fzb_match_list_parallel_rccl(fzb_matcher* m, const fzb_corpus* shard, uint32_t index_offset, fzb_shard_comm* comm, int flags, fzb_match** out, size_t* out_len);
int fzb_shard_comm_last_exchange(const fzb_shard_comm* comm, uint64_t out_bytes[2]);

/* `MatchIndices` (src/lib.rs:189-199): a Match plus the haystack byte positions that matched the needle, in reverse
 * order.  positions[positions_begin .. positions_begin + positions_len) of the array returned next to the records. */
typedef struct fzb_match_indices {
    uint32_t index;
    uint16_t score;
    uint8_t exact;
    uint8_t _pad;
    uint32_t positions_begin;
    uint32_t positions_len;
} fzb_match_indices;

/* `Matcher::match_list_indices(&haystacks)` (src/matcher/mod.rs:234-275 -> match_list_indices_impl src/matcher/algo.rs:196-227,
 * smith_waterman_indices_one :264-292, score_haystack[_unicode]_indices src/smith_waterman/algo/mod.rs:49-152, the traceback
 * src/smith_waterman/alignment_iter.rs:35-181; literal modes src/literal/algo.rs:129-155), on the GPU: the scorer keeps its
 * score / match matrices in HBM and walks the alignment back on the device.  The haystack list is the `selection`
 * (n_selection corpus indices, host memory, any order, repeats allowed - typically the top of a fzb_match_list result) or,
 * with selection == NULL, the whole corpus; `index` numbers that list like the reference numbers `haystacks`
 * (selection[index] is the corpus index).  Order: as the reference, list order, reversed for the *Desc strategies, then a
 * stable sort by descending score for the Score* strategies.  Free with fzb_match_indices_free. */
int fzb_match_list_indices(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t n_selection,
                           fzb_match_indices** out, size_t* out_len, uint32_t** out_positions);
/* The unordered form: `Specialized::match_list_indices` (src/matcher/algo.rs:24-33) and what `Matcher::match_iter_indices` /
 * `match_one_indices` (src/matcher/mod.rs:321-334, 357-371) yield - list order whatever `config.sort` says,
 * `index = index_offset + position in the list`. */
int fzb_match_list_indices_into(fzb_matcher* m, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, uint32_t index_offset,
                                fzb_match_indices** out, size_t* out_len, uint32_t** out_positions);
void fzb_match_indices_free(fzb_match_indices* matches, uint32_t* positions);

/* TOP-`limit` WITH MATCHED POSITIONS, one fused call: what a picker shows after a keystroke.  The reference has no such call: its caller
 * truncates the Vec that `Matcher::match_list_indices(&haystacks)` returns over the whole list (src/matcher/mod.rs:234-275), exactly as for
 * fzb_match_list_top.  The contract is that truncation: the first min(limit, found) elements of that Vec, in its order - list order,
 * reversed for the *Desc strategies, then stably sorted by descending score for the Score* strategies.  `index` is the CORPUS index (the
 * list is the whole corpus), the positions are the matched byte positions in reverse order as in fzb_match_list_indices, and found = the
 * length of the full list.  On the device: the top stage's sorted head stays in HBM and becomes the item list of a traced second pass, whose
 * positions are packed densely; every traced record is checked against the head's record at its place (same index, score and exact flag,
 * same count: the accept decision and the scores of match_list and match_list_indices are the same code in the reference,
 * src/matcher/algo.rs:78-103 against :196-227).  ONE host wait brings back counts, records and positions.  limit = 0 is valid (no records,
 * found still reported); an empty needle matches every haystack with score 0 and no positions (the first / last min(limit, n) indices, host
 * work).  Free with fzb_match_indices_free; *out_found is optional.  A disagreement between the two passes: FZB_ERR_HIP, "internal: ...". */
int fzb_match_list_top_indices(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions,
                               uint64_t* out_found);
/* The same with the result left in HBM and no host synchronisation; asynchronous on `stream`.  dev_out has room for `capacity` >=
 * min(limit, corpus length) records, dev_positions for `positions_capacity` >= min(limit, corpus length) x needle bytes dwords (less of
 * either: FZB_ERR_CAPACITY, nothing launched).  dev_out[k].positions_begin / positions_len index the DENSE dev_positions.  dev_count (four
 * words): [0] = records written = min(limit, found), [1] = found, [2] = position dwords written, [3] = 0, or non-zero when the traced pass
 * disagreed with the top stage (bit 0: record count, bit 1: a record).  An empty corpus zeroes the four words.  Not for an empty needle
 * (FZB_ERR_INVALID). */
int fzb_match_list_top_indices_device(fzb_matcher* m, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions,
                                      size_t positions_capacity, uint32_t* dev_count, void* stream);
/* After fzb_matcher_reserve(m, c) and this call, no fzb_match_list_top_indices[_device] call with this `limit` or a smaller one, on any
 * needle of at most max_needle_bytes bytes, allocates device memory - also across fzb_matcher_set_pattern / fzb_matcher_set_config.  Sizes
 * the item list, the position counts, the strided positions, the traced scorer's matrices, the head, the traced records, and the packed
 * records and positions of the host form.  (Without it these grow on first use, sized by min(limit, corpus length).  A needle beyond 64
 * bytes / 63 rows keeps its own scratch, which grows when such a needle is first used, and a new config whose filter form needs workspace
 * arrays the reserved form did not - typos after none - regrows the range workspace once: both as for fzb_matcher_reserve.) */
int fzb_matcher_reserve_top_indices(fzb_matcher* m, const fzb_corpus* c, size_t limit, size_t max_needle_bytes);

/* CANDIDATE SETS: a query over a device-resident SUBSET of the corpus.  Every picker narrows - when the query grows from `dead` to `deadb` only
 * the haystacks that matched `dead` are looked at again - and restricts ("only this workspace folder").  The reference has no such call: its
 * `match_list` takes the whole slice, and a caller that narrows builds a new Vec of the survivors on the host.  Here an fzb_subset holds a
 * strictly ascending array of uint32 haystack indices of ONE corpus in device memory, its count beside it (and on the host when known), and
 * becomes the item list of the pipeline.  The contract is the scope's sentence, restated for a set:
 *     A query over subset S returns what the same query returns over a fzb_corpus_upload of the haystacks of S alone, in their order, with
 *     every `index` mapped back to the full list's.
 * The map is monotone, so the ordering rule (src/matcher/mod.rs:215-221, src/sort.rs:6-40) and the tie-breaks at a top-`limit` cut carry
 * over; `found` counts the matches inside S.  The list's terms apply as to any index-ordered records: an active scope drops the hidden
 * records and a score bias is added, after the scorers.
 * The handle follows the editing family's rules: only for a corpus the library owns (fzb_corpus_upload; a borrowed one: FZB_ERR_INVALID), the
 * set-up calls (create, set_indices, from_scope, read; info when the count is not known) wait for the device's outstanding work on entry and
 * are complete on return, and an error leaves the subset as it was.  A subset created after fzb_corpus_reserve has room for the reserved
 * items, so its later fills and captures allocate nothing; it grows geometrically when the list outgrew it.
 * STALENESS: the corpus carries a generation counter (fzb_corpus_generation) that every call which changed the LIST bumps - fzb_corpus_append,
 * _truncate, _remove, _remove_device, _replace; not _set_bias, _set_tags, _set_scope, _reserve, nor a call that changed nothing.  A subset
 * records the generation when it is created, filled or captured into; a query handed an input subset of another corpus or of an older
 * generation is refused with FZB_ERR_INVALID (the message says "subset" and "stale"), nothing launched.
 * The fzb_multi_matcher forms take a candidate set too (fzb_multi_match_list_subset and its siblings, below the composition's own calls):
 * the device path is the same - only the composition's first step ever saw the whole range - and the capture is the COMPOSITION's match set.
 * When the previous capture may be the next query's input is the caller's rule, never the library's: a negated pattern's match set GROWS as
 * it is typed (`!t` -> `!te` removes fewer haystacks), so only an unchanged negated pattern keeps a capture usable
 * (frizbee_amd.NarrowingQuery holds the whole rule).
 * OUT OF SCOPE: the sharded and RCCL forms, the range forms (_into, _device with first / count), the list-order _indices forms
 * (fzb_match_list_indices: its `selection` already is a subset), and a density switch inside the library (streaming the whole list and
 * intersecting when S covers most of it): the caller decides when a subset pays (frizbee_amd.NarrowingMatcher, NarrowingQuery). */
typedef struct fzb_subset fzb_subset;
/* the list's generation: 0 after fzb_corpus_upload, + 1 for every call that changed the list (fzb_corpus_info's array stays 12 long) */
int fzb_corpus_generation(const fzb_corpus* c, uint64_t* out);
/* an empty subset of `c` with room for max(length, reserved items) indices */
int fzb_subset_create(const fzb_corpus* c, fzb_subset** out);
void fzb_subset_free(fzb_subset* s);
/* The subset becomes host_indices[0 .. n): checked on the host - strictly ascending and below the corpus length; a violation gives
 * FZB_ERR_INVALID naming the first offending position, nothing written.  One host-to-device copy; the count is known. */
int fzb_subset_set_indices(fzb_subset* s, const uint32_t* host_indices, size_t n);
/* The subset becomes the haystacks visible under (require, exclude) over the corpus' tags - the scope's predicate, whatever scope the corpus
 * has set -, computed on the device (a flag pass and a stable compaction of the indices); only the count crosses the link.  A corpus without
 * tags: every haystack for (0, 0), none when require != 0.  `c` must be the subset's corpus. */
int fzb_subset_from_scope(fzb_subset* s, const fzb_corpus* c, uint16_t require, uint16_t exclude);
/* out[0] = the count was known on the host when the call was made (0/1; 0 after a _device form captured into the subset: the call then
 * synchronises the device and reads it), [1] = count, [2] = capacity in indices, [3] = the corpus generation the subset belongs to */
int fzb_subset_info(fzb_subset* s, uint64_t out[4]);
/* a synchronous copy of the indices: *out_n = count; more than `cap`: FZB_ERR_CAPACITY (and the count) */
int fzb_subset_read(fzb_subset* s, uint32_t* host_out, size_t cap, size_t* out_n);
/* The queries.  `in` == NULL: the whole corpus - exactly the launches of the call without _subset (how narrowing starts).  `capture` (may be
 * NULL): afterwards it holds the indices of EVERY haystack of `in` the matcher accepted, ascending - the index-ordered records the scorers
 * wrote, taken BEFORE the list's terms, the selection and the ordering, so the captured set does not depend on `limit`, the sort strategy,
 * the bias or the scope (the user may toggle "hide ignored" between two keystrokes; the next query applies the scope again anyway).  One
 * more launch; the count is written on the device.  The host forms bring it back in the wait they make anyway (the capture's count is then
 * known); after the _device form it is unknown until fzb_subset_info is asked.  capture == in: FZB_ERR_INVALID (alternate two subsets); a
 * capture of another corpus is refused; a capture takes the corpus' current generation.  After fzb_matcher_reserve(m, c) (and
 * fzb_matcher_reserve_top_indices for the form with positions) no subset query allocates device memory.
 * An EMPTY NEEDLE: the host forms list the haystacks of `in` - score 0, or the clamped bias, hidden ones dropped, ordered as the empty
 * prompt of the calls without _subset - and the capture, if any, becomes `in` itself; the list is made on the device (the set's count is
 * read there, the set never crosses the link); the _device form refuses, as its siblings do - fzb_prompt_top_device takes a subset.
 * fzb_match_list_subset: fzb_match_list's order.  _top_subset / _top_subset_device: fzb_match_list_top / _top_device (dev_count: records
 * written, found).  _top_indices_subset: fzb_match_list_top_indices; its traced pass runs over the head's item list as before. */
int fzb_match_list_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_match** out, size_t* out_len);
int fzb_match_list_top_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
int fzb_match_list_top_subset_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match* dev_out, size_t capacity,
                                     uint32_t* dev_count, void* stream);
int fzb_match_list_top_indices_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len,
                                      uint32_t** out_positions, uint64_t* out_found);

/* ---- THE EMPTY PROMPT on the device ---------------------------------------------------------------------------------------------------
 * The _device forms of an EMPTY needle, which fzb_match_list_device / _top_device / _top_subset_device / _top_indices_device refuse: a picker
 * opens on an empty prompt and a stream-ordered host wants that list without a wait.  The rule is the host forms': the haystacks of the
 * range, or of `in`, that are visible under the corpus' scope, in index order, each with score clamp(bias[i], 0, 65535) (0 without a bias),
 * exact 0; the top form reverses for the *Desc strategies and sorts stably by descending score for the Score* strategies only over a
 * biased corpus; found = the number visible.  They also serve a corpus without bias, scope or subset ("every index, score 0").
 * m must have an empty needle (FZB_ERR_INVALID otherwise; the message names the needle).  `in` may be NULL; with `in` only first == 0 and
 * count == the corpus length are accepted, and a stale or foreign subset is refused as in the _subset queries.  Everything is enqueued on
 * `stream`; nothing synchronises.  An empty corpus (or count == 0) zeroes the pair.  After fzb_matcher_reserve(m, c) neither allocates. */
/* the empty needle's index-ordered list: fzb_match_list_device for a matcher whose needle is empty.  At most `capacity` records are written;
 * dev_count[0] = records written, dev_count[1] = found. */
int fzb_prompt_list_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t first, size_t count, uint32_t index_offset,
                           fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);
/* ... and its ordered head: fzb_match_list_top_device / _top_subset_device.  capacity < min(limit, corpus length): FZB_ERR_CAPACITY, nothing
 * launched; dev_count[0] = records written = min(limit, found), dev_count[1] = found. */
int fzb_prompt_top_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, size_t limit,
                          fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);

/* `radix_sort_matches(&mut [Match])` (src/sort.rs:6-40): stable, descending score, host side */
void fzb_radix_sort_matches(fzb_match* matches, size_t n);
/* `k_merge_matches_by_*` (src/k_merge.rs:56-132): merges per-shard runs (each sorted per `sort`) - the
 * host-side combine after the multi-GPU gather.  runs = concatenated runs, run_lens[k] records each. */
int fzb_k_merge_matches(int32_t sort, const fzb_match* runs, const size_t* run_lens, size_t nruns, fzb_match* out);

/* ---- multi-pattern composition ----------------------------------------------------------------------
 * `Matcher::from_patterns(&[Pattern], &Config)` (src/matcher/mod.rs:95-111): a haystack matches when every non-negated
 * pattern matches and no negated one does; score = saturating sum of the non-negated patterns' scores, exact = OR
 * (src/matcher/multi.rs:84-152).  One `fzb_pattern` = reference `Pattern{needle, negated, config: PatternConfig}`
 * (src/pattern.rs:9-18, 230-262); the per-pattern overrides are resolved against the matcher's config exactly like
 * `PatternConfig::resolve`, including the matching mode (`Pattern::parse`: `^foo` prefix, `foo$` suffix, `^foo$` exact,
 * `'foo` substring, `!foo` negated substring). */
typedef struct fzb_pattern {
    const uint8_t* needle_utf8;
    size_t needle_len;      /* 0: the pattern is dropped (Matcher::compile, src/matcher/mod.rs:193-195) */
    int32_t negated;
    int32_t has_max_typos;  /* PatternConfig::max_typos = Some(max_typos); 0 = None = inherit the config's */
    int32_t max_typos;
    int32_t casing;         /* FZB_CASE_*, or -1 = inherit */
    int32_t unicode;        /* FZB_UNICODE_*, or -1 = inherit */
    int32_t has_scoring;    /* PatternConfig::scoring = Some(scoring) */
    fzb_scoring scoring;
    int32_t matching;       /* FZB_MATCH_*, or -1 = inherit Config::matching (what Pattern::parse leaves for a plain atom) */
} fzb_pattern;
typedef struct fzb_multi_matcher fzb_multi_matcher;

/* `Pattern::parse_query(query)` (src/pattern.rs:186-222; atoms per `Pattern::parse`, :87-167): whitespace separated atoms, `\\` escapes,
 * atoms with an empty needle dropped.  The array (and the needle strings it points to) is released with fzb_patterns_free. */
int fzb_parse_query(const uint8_t* query_utf8, size_t query_len, fzb_pattern** out_patterns, size_t* out_n);
void fzb_patterns_free(fzb_pattern* patterns, size_t n);

int fzb_multi_matcher_create(const fzb_config* config, const fzb_pattern* patterns, size_t n_patterns, fzb_multi_matcher** out);
void fzb_multi_matcher_free(fzb_multi_matcher* mm);
size_t fzb_multi_matcher_len(const fzb_multi_matcher* mm); /* compiled (non-empty) patterns */
/* `Matcher::match_list` over CompiledPatterns::{Empty, Single, Multi} (src/matcher/mod.rs:212-222, 373-392): ordered per config.sort */
int fzb_multi_match_list(fzb_multi_matcher* mm, const fzb_corpus* c, fzb_match** out, size_t* out_len);
/* fzb_match_list_top for a `from_patterns` matcher: the first min(limit, found) records of fzb_multi_match_list's result */
int fzb_multi_match_list_top(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
/* `Matcher::match_list_indices` for a `from_patterns` matcher (see fzb_match_list_indices): CompiledPatterns::Multi runs
 * `match_one_indices_multi` (src/matcher/multi.rs:56-82) - a negated pattern that matches drops the haystack, every other pattern
 * must match, scores add with saturation, exact flags OR, and the patterns' positions are merged (descending, de-duplicated). */
int fzb_multi_match_list_indices(fzb_multi_matcher* mm, const fzb_corpus* c, const uint32_t* selection, size_t n_selection,
                                 fzb_match_indices** out, size_t* out_len, uint32_t** out_positions);
/* fzb_match_list_top_indices for a `from_patterns` matcher: the first min(limit, found) elements of what `Matcher::match_list_indices`
 * returns over the whole list for `Matcher::from_patterns` (src/matcher/mod.rs:234-275).  A HOST composition of the existing pieces:
 * fzb_multi_match_list_top brings the head to the host, fzb_multi_match_list_indices' implementation then runs in list order over that
 * selection and `index` is mapped back to the corpus index; the head is already in order, so nothing is re-ordered.  (The per-haystack
 * union of the patterns' positions stays host work in this call; the sharded and the RCCL forms are not built.) */
int fzb_multi_match_list_top_indices(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions,
                                     uint64_t* out_found);
/* (The device-fused form of that call is fzb_multi_match_list_top_indices_fused below; the one above remains the portable host composition.)
 *
 * THE SAME QUERY FUSED ON THE DEVICE.  fzb_multi_match_list_top_indices_device is fzb_match_list_top_indices_device for a `from_patterns`
 * matcher - same contract, same four count words (records written, matches found, positions written, 0 or why the passes disagree) - with
 * positions_capacity >= min(limit, haystacks) x U, U = the sum over the NON-NEGATED patterns of max(1, needle bytes).  Asynchronous on
 * `stream`, no host synchronisation: the multi top stage leaves its sorted head in HBM, one item list is made of it, every non-negated
 * pattern runs the traced pipeline over that list (negated patterns are not traced: the head holds no haystack they hit), one kernel puts
 * the patterns' records and positions together per head record - `match_one_indices_multi`, src/matcher/multi.rs:56-82: scores add with
 * saturation, exact flags OR, positions merged descending without repeats - and the pack step of the single-needle form writes the result
 * while holding the combined records to the head.  A matcher with no compiled pattern (CompiledPatterns::Empty) is refused with
 * FZB_ERR_INVALID - the host form answers it -, an empty corpus zeroes the four words.  The sharded and the RCCL forms are not built. */
int fzb_multi_match_list_top_indices_device(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions,
                                            size_t positions_capacity, uint32_t* dev_count, void* stream);
/* The host form: the call above into the matcher's staging, then ONE wait for the words, the records and the positions (as
 * fzb_match_list_top_indices).  Result and contract as fzb_multi_match_list_top_indices; a disagreement between the passes is FZB_ERR_HIP
 * "internal: ...". */
int fzb_multi_match_list_top_indices_fused(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions,
                                           uint64_t* out_found);
/* After fzb_multi_matcher_reserve(mm, c) and this call, no fzb_multi_match_list_top_indices_fused / _device call with this `limit` or a
 * smaller one allocates device memory - also across fzb_multi_matcher_set_patterns / _set_config that do not raise the number of compiled
 * patterns above the slots held, while every needle has at most max_needle_bytes bytes.  Sizes the head, the item list, every slot's trace
 * buffers and traced scorer's matrices (spare slots included), the unions for U = slots x max_needle_bytes and the host form's staging.
 * The exceptions of fzb_matcher_reserve_top_indices apply (a needle beyond 64 bytes / 63 rows, another scoring or lane pair). */
int fzb_multi_matcher_reserve_top_indices(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, size_t max_needle_bytes);
/* CANDIDATE SETS for the composition (see fzb_match_list_subset: the same argument order, contract, staleness rules and refusals).  `in` ==
 * NULL: exactly the launches of the call without _subset.  With `in`, the composition's FIRST step - the first non-negated pattern's
 * pipeline, or the identity records when every pattern is negated - runs over the set's item list; every later pattern runs over the
 * candidates as before.  `capture` receives the ascending indices of every haystack of `in` the COMPOSITION accepted (every non-negated
 * pattern hit, no negated one did), taken between the composition and the list's terms: it does not depend on `limit`, the sort strategy, the
 * bias or the scope.  A composition of several patterns captures in the launch that writes its final records (k_copy_capture_records: no
 * launch more than without a capture); a lone non-negated pattern and no pattern at all take the single forms' capture launch.  The host forms
 * bring the count back in the wait they make anyway, after the _device form it is unknown until fzb_subset_info is asked.  After fzb_multi_matcher_reserve(mm, c)
 * (and fzb_multi_matcher_reserve_top_indices for the form with positions) no subset query allocates device memory.
 * A matcher with NO COMPILED PATTERN lists the haystacks of `in` - score 0 or the clamped bias, hidden ones dropped, ordered as the empty
 * prompt of the calls without _subset - and the capture becomes `in` itself; the _device form refuses it, as
 * fzb_multi_match_list_top_indices_device does.
 * _subset: fzb_multi_match_list's order.  _top_subset: fzb_multi_match_list_top.  _top_subset_device: the same head into dev_out (room for
 * min(limit, haystacks)), dev_count = (records written, found), on `stream`, nothing read back.  _top_indices_subset:
 * fzb_multi_match_list_top_indices_fused - only its top stage sees the set, the traced passes run over the head as before. */
int fzb_multi_match_list_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_match** out, size_t* out_len);
int fzb_multi_match_list_top_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match** out, size_t* out_len,
                                    uint64_t* out_found);
int fzb_multi_match_list_top_subset_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match* dev_out, size_t capacity,
                                           uint32_t* dev_count, void* stream);
int fzb_multi_match_list_top_indices_subset(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out,
                                            size_t* out_len, uint32_t** out_positions, uint64_t* out_found);
/* list-order forms (see fzb_match_list_into / fzb_match_list_indices_into): `Matcher::match_list_into` over CompiledPatterns
 * (src/matcher/mod.rs:373-392) with the result on the host, and what `match_iter` / `match_one` / `match_iter_indices` yield
 * (`match_one_multi`, `match_one_indices_multi`, src/matcher/multi.rs:29-82) */
int fzb_multi_match_list_into(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset, fzb_match** out, size_t* out_len);
int fzb_multi_match_list_indices_into(fzb_multi_matcher* mm, const fzb_corpus* c, const uint32_t* selection, size_t n_selection, uint32_t index_offset,
                                      fzb_match_indices** out, size_t* out_len, uint32_t** out_positions);
/* `match_list_multi_into(patterns, haystacks, haystack_index_offset, matches)` (src/matcher/multi.rs:84-152): index order, result in HBM */
int fzb_multi_match_list_device(fzb_multi_matcher* mm, const fzb_corpus* c, size_t first, size_t count, uint32_t index_offset,
                                fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);

/* `Matcher::set_patterns` (src/matcher/mod.rs:170-176): skipped when the patterns are field-for-field the same; otherwise they are compiled
 * as fzb_multi_matcher_create would, into the matcher's sub-matcher slots in order - a slot whose needle and resolved config are unchanged
 * is left alone, any other is rebuilt in place (fzb_matcher_set_pattern's rule: its device workspace is kept), and a sub-matcher is
 * created only when the compiled patterns outnumber the slots held (slots are released only by fzb_multi_matcher_free).  The
 * composition, ordering and multi-device buffers are kept.  Empty / Single / Multi (mod.rs:178-190) as for a fresh create.  On error the
 * matcher answers as before the call. */
int fzb_multi_matcher_set_patterns(fzb_multi_matcher* mm, const fzb_pattern* patterns, size_t n_patterns);
/* `Matcher::set_config` (src/matcher/mod.rs:154-162): no-op on an equal config (field by field); a change of `sort` alone rebuilds no
 * sub-matcher (they run IndexAsc); any other change resolves every pattern again and updates its slot in place. */
int fzb_multi_matcher_set_config(fzb_multi_matcher* mm, const fzb_config* config);
/* fzb_matcher_reserve for the composition: the composition buffers, the ordering / staging buffers and every sub-matcher slot sized for
 * `c` - a slot for ANY needle it may hold next, not only the one it holds now: the buffers of every filter / scorer form (fuzzy with or
 * without typos, literal, unicode) and the multi-chunk scorer's parked rows for the largest needle of up to 64 bytes / 63 rows under the
 * slot's scoring and lane pair (on a 256-CU device up to 512 MiB per slot).  Afterwards no query over `c` or a sub-range of it allocates
 * device memory, also after any set_patterns / set_config that does not increase the number of compiled patterns - unless a needle goes
 * beyond 64 bytes or a pattern's scoring or lane pair changes. */
int fzb_multi_matcher_reserve(fzb_multi_matcher* mm, const fzb_corpus* c);
/* `impl Clone for Matcher` (src/matcher/parallel.rs:46): fzb_matcher_clone per compiled pattern (the resolved lane pairs are kept), the
 * same config; its own buffers. */
int fzb_multi_matcher_clone(const fzb_multi_matcher* mm, fzb_multi_matcher** out);
/* `Matcher::match_list_parallel(&haystacks, threads)` (src/matcher/parallel.rs:18-89) of a `from_patterns` matcher: as
 * fzb_match_list_parallel - 0 => FZB_ERR_PANIC "threads must be positive", otherwise fzb_multi_match_list's result. */
int fzb_multi_match_list_parallel(fzb_multi_matcher* mm, const fzb_corpus* c, size_t threads, fzb_match** out, size_t* out_len);

/* ---- ANY-OF GROUPS: `a | b` composed on the device ------------------------------------------------------------------------------
 * The reference has no such operator.  A query is an AND of TERMS; a term is a single pattern, possibly negated, exactly as above, or an
 * ANY-OF GROUP of 2..FZB_GROUP_ALTS_MAX non-negated patterns ("alternatives"), each resolved against the matcher's config like any pattern.
 * SEMANTICS: a group matches a haystack iff at least one alternative matches it; the group's score is the maximum of the matching
 * alternatives' scores and its exact flag the OR of the exact flags of the alternatives whose score equals that maximum - on the device a
 * plain max over the key score << 1 | exact, so the result does not depend on the order of the alternatives.  In the composition a group
 * behaves exactly like ONE non-negated pattern with those hits: it can be the base term (the first non-negated term runs over the whole
 * range, or over the `in` candidate set), later groups run over the surviving candidates only, score = saturating sum, exact = OR; bias,
 * scope, facets, capture, sort and `found` apply to the composed records unchanged.  Alternatives with an empty needle are dropped; a group
 * left with one alternative IS that plain pattern (the same launches, bit-identical results), one left with none is dropped.  A negated
 * alternative, more than FZB_GROUP_ALTS_MAX alternatives, equal term ids that are not adjacent or a null argument: FZB_ERR_INVALID before
 * anything touches the device.
 * LAUNCHES per group of k alternatives: k pipelines, k accumulates, one clear, one flag, one compact; every count stays on the device.  The
 * slots and the alternatives' hit buffer are allocated only by a matcher that has a group (fzb_multi_matcher_reserve covers them); a matcher
 * without one allocates and launches exactly what it did.
 * SERVED for a matcher with a group: fzb_multi_match_list, _into, _device, _top, _parallel, the _subset forms of these (_subset, _top_subset,
 * _top_subset_device), _top_sections, _top_sections_device and an attached facet sink (fzb_multi_matcher_set_facets).
 * REFUSED for a matcher with a group (FZB_ERR_INVALID, the message names the entry point and says "any-of group"): every form with matched
 * positions - fzb_multi_match_list_indices, _indices_into, _top_indices, _top_indices_device, _top_indices_fused, _top_indices_subset,
 * _top_sections_indices, _top_sections_indices_device - and the multi-device forms fzb_multi_match_list_parallel_sharded, _top_sharded and
 * _parallel_rccl.  (The traced union assumes every non-negated pattern matches every head record; an alternative need not.)  A grouped
 * matcher gets the matched positions of its top-`limit` from fzb_multi_match_list_top_indices_groups / _groups_device below, which build the
 * per-record presence and the carrier rule that union lacks. */
#define FZB_GROUP_ALTS_MAX 8
/* fzb_multi_matcher_create with a grouping: group_of[i] = the term id of pattern i; equal ids must be adjacent and make one group, an id
 * used once is a single term.  group_of == NULL is fzb_multi_matcher_create. */
int fzb_multi_matcher_create_groups(const fzb_config* config, const fzb_pattern* patterns, size_t n_patterns, const uint32_t* group_of, fzb_multi_matcher** out);
/* fzb_multi_matcher_set_patterns with a grouping: the in-place re-query (spare sub-matchers are reused), skipped when the patterns AND the
 * grouping are unchanged.  fzb_multi_matcher_set_patterns on a grouped matcher makes every pattern a single term again;
 * fzb_multi_matcher_clone carries the grouping; fzb_multi_matcher_set_config keeps it. */
int fzb_multi_matcher_set_pattern_groups(fzb_multi_matcher* mm, const fzb_pattern* patterns, size_t n_patterns, const uint32_t* group_of);
/* fzb_parse_query with the any-of operator.  Atoms are split exactly as fzb_parse_query splits them (`\ ` included).  An atom that is
 * exactly `|` joins the atom before it and the atom after it into one group - transitively: `a | b | c` is one group of three - when both
 * atoms exist, neither is negated and neither is itself `|`; in every other position (leading, trailing, doubled, next to a `!atom`) it
 * stays the ordinary needle `|` that fzb_parse_query makes of it.  The atom `\|` is the literal needle `|`.  A query without a joining `|`
 * yields fzb_parse_query's patterns with all-distinct ids.  group_of[i] = the term id of pattern i, ascending from 0.  Both arrays are
 * released with fzb_query_groups_free. */
int fzb_parse_query_groups(const uint8_t* query_utf8, size_t query_len, fzb_pattern** out_patterns, uint32_t** out_group_of, size_t* out_n);
void fzb_query_groups_free(fzb_pattern* patterns, uint32_t* group_of, size_t n);
/* ---- ANY-OF GROUPS WITH MATCHED POSITIONS: the top-`limit` of a grouped matcher, fused on the device ---------------------------------------
 * HEAD AND RECORDS: the head is exactly what fzb_multi_match_list_top / _top_subset return for the same matcher, corpus, subset, bias and
 * scope; records carry (index, score, exact), `found` is theirs.
 * THE CARRIER OF A GROUP: for a head record on haystack h and a group G, the carrier is chosen among the alternatives that match h - the
 * alternative with the largest key score << 1 | exact, on equal keys the first in query order.  The carrier's record is the group's record
 * (its exact flag equals the group's: the key maximum prefers a set flag at equal scores).
 * POSITIONS of a head record: the strictly descending union without repeats (`match_one_indices_multi`, src/matcher/multi.rs:56-82) of the
 * positions of every plain non-negated pattern and of each group's carrier ONLY.  Alternatives that match but do not carry contribute
 * nothing; negated terms contribute nothing.
 * STRIDE: U_g = the trace strides (needle bytes, at least 1) of the plain non-negated patterns + per group the maximum trace stride among its
 * alternatives (fzb_multi_matcher_groups_positions_stride).  U_g replaces the U of the ungrouped forms in every capacity rule.
 * A matcher WITHOUT a group takes the ungrouped path unchanged through these entry points: the same launches, the same allocations, a
 * byte-identical result to fzb_multi_match_list_top_indices_fused / _device (with `in` / `capture`: _top_indices_subset); U_g is then U.
 * A biased or scoped corpus, an attached facet sink and the `in` / `capture` candidate sets (both nullable) behave as in
 * fzb_multi_match_list_top_indices_fused / _subset: only the top stage sees the set, the bias is added once after the sum, the capture
 * receives what the composition accepted.  An empty pattern list, a corpus of 0 haystacks and `limit` 0 behave as in the fused form.
 * LAUNCHES behind the head: one traced pass per plain non-negated pattern and per alternative over the head's one item list, then four
 * launches whatever the number of groups and alternatives - the haystack -> head position map, one clear of all the alternatives' row maps,
 * one launch that fills them, one merge (in place of the ungrouped union) -, the bias and the pack.  One host wait in the host form, none in
 * the device form.
 * DISAGREEMENT stays an error: a head record for which some group has no matching alternative, or whose carriers' sum differs from the head's
 * record, and a traced pass that produced more records than the head has (a plain pattern's: another number), make the host form fail with
 * FZB_ERR_HIP "the traced passes disagree with the multi top stage" and raise word [3] of the device form's count words.
 * Still REFUSED for a grouped matcher: the list-order forms, the sectioned forms with positions and the multi-device forms named above. */
/* U_g of the matcher's compiled patterns (the U of the ungrouped forms for a matcher without a group) */
int fzb_multi_matcher_groups_positions_stride(const fzb_multi_matcher* mm, size_t* out);
/* The device form: fzb_multi_match_list_top_indices_device's arguments and four count words at dev_count, plus the nullable candidate sets;
 * capacity >= min(limit, haystacks), positions_capacity >= min(limit, haystacks) x U_g, else FZB_ERR_CAPACITY before anything is launched. */
int fzb_multi_match_list_top_indices_groups_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices* dev_out,
                                                   size_t capacity, uint32_t* dev_positions, size_t positions_capacity, uint32_t* dev_count, void* stream);
/* The host form: one wait; the result is released with fzb_match_indices_free. */
int fzb_multi_match_list_top_indices_groups(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out,
                                            size_t* out_len, uint32_t** out_positions, uint64_t* out_found);
/* fzb_multi_matcher_reserve_top_indices, and additionally what the grouped tail owns, for any grouping of the matcher's slots.  After
 * fzb_multi_matcher_reserve(mm, c) and this call no call of the two forms above with this `limit` or a smaller one allocates device memory
 * (needles of up to max_needle_bytes bytes, no more compiled patterns than now). */
int fzb_multi_matcher_reserve_top_indices_groups(fzb_multi_matcher* mm, const fzb_corpus* c, size_t limit, size_t max_needle_bytes);
/* The multi-device form (see fzb_match_list_parallel_sharded): the whole AND / NOT composition runs per shard on the shard's device
 * through per-shard clones the matcher keeps (they follow set_patterns / set_config), each run numbered from its shard's first index;
 * the runs are gathered and ordered once on the root (the caller's current device).  Result = fzb_multi_match_list on the unsharded
 * list for every sort strategy; with no compiled pattern every index, score 0, reversed for the *Desc strategies (mod.rs:215-220). */
int fzb_multi_match_list_parallel_sharded(fzb_multi_matcher* mm, const fzb_sharded_corpus* sc, fzb_match** out, size_t* out_len);
/* fzb_match_list_top_sharded for a `from_patterns` matcher */
int fzb_multi_match_list_top_sharded(fzb_multi_matcher* mm, const fzb_sharded_corpus* sc, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);
/* COLLECTIVE, one process per GPU (see fzb_match_list_parallel_rccl): this rank's composition is its run; the exchange is the same. */
int fzb_multi_match_list_parallel_rccl(fzb_multi_matcher* mm, const fzb_corpus* shard, uint32_t index_offset, fzb_shard_comm* comm,
                                       int flags, fzb_match** out, size_t* out_len);
/* fzb_matcher_shard_report for the last fzb_multi_match_list_parallel_sharded on `mm` ("" before the first) */
const char* fzb_multi_matcher_shard_report(const fzb_multi_matcher* mm);

/* ---- TAG FACETS: per-tag match counts of a query, counted on the device ------------------------------------------------------------------
 * A picker with filter chips ("tests 1 204 - docs 87 - ignored 312", "N matches, 312 hidden by filters") needs, per keystroke, the number of
 * matches under every tag bit and the number the active scope hides.  The reference has no such notion: its caller counts over the Vec
 * `match_list` returned.  Here an fzb_facets holds FZB_FACET_WORDS counts in device memory and a page-locked host mirror; attached to a
 * matcher it is filled by every query that honours it, where the records and the tag column already are.
 * For a query, let A be the haystacks of the input (the range, or the subset `in`) that the matcher accepts - the set a `capture` of the same
 * call would hold: taken BEFORE scope, bias, selection, `limit` and ordering; for a `from_patterns` matcher what the composition accepted;
 * for an empty needle or an empty pattern list every haystack of the input.  With tag(i) the haystack's 16-bit tag (0 where the corpus has
 * no tags) and (require, exclude) the corpus' scope at the time of the call:
 *     [0]      matched            |A|
 *     [1]      visible            the members of A with (tag & require) == require && (tag & exclude) == 0: the call's `found`
 *     [2 + b]  all_by_bit[b]      the members of A whose tag has bit b, b = 0 .. 15 - over ALL of A: a chip for an excluded bit shows what it hides
 *     [18 + b] visible_by_bit[b]  the same over the visible members of A
 * The counts are exact: they depend neither on `limit` nor on the `capacity` of a _device form's output (a _device call with room for 10
 * records over 10 000 matches counts 10 000: with a sink attached the producer writes into the matcher's scratch, which has room for one
 * record per haystack of the range).  Bias, `exact`, positions and which haystacks match are untouched.  With no sink attached every call
 * launches and allocates exactly what it did before sinks existed.
 * FILLED BY: fzb_match_list, fzb_match_list_into, fzb_match_list_device, fzb_match_list_sorted_device, fzb_match_list_top, fzb_match_list_top_device,
 * fzb_match_list_top_indices, fzb_match_list_top_indices_device, the _subset forms of each, fzb_prompt_list_device, fzb_prompt_top_device; and of a
 * `from_patterns` matcher fzb_multi_match_list, fzb_multi_match_list_into, fzb_multi_match_list_device, fzb_multi_match_list_top, their _subset forms,
 * fzb_multi_match_list_top_indices_device and fzb_multi_match_list_top_indices_fused (in the forms with positions the count sits at the top
 * stage only, as the capture does).  Everything is enqueued on the query's stream: the block is cleared, counted into and copied to the
 * mirror in stream order - in front of a host form's one wait, which makes no
 * second one.  A _device form on a stream of the caller's also records an event of the sink's own behind the copy (the null stream needs
 * none and does not pay for one).  (The closed-form host answers of an empty needle / an empty pattern list over a corpus without bias, scope or subset launch
 * nothing else and have no wait of their own: with a sink attached they launch the count on the null stream of the current device and wait
 * for it before they return.)
 * ONE QUERY AT A TIME: a sink holds the counts of the last query that filled it.  Queries that fill the same sink - by one matcher or by
 * several that share it - must be ordered by the caller (the same stream, or an event between the streams): the next query's clear is not
 * ordered against the previous query's copy otherwise.  The sink keeps no handle of a caller's stream: one destroyed after its query is never touched.
 * REFUSED: every other entry point that takes a corpus either fills an attached sink or REFUSES the matcher with FZB_ERR_INVALID - none ignores
 * the sink; the message names set_facets(NULL).  Refused: fzb_match_list_parallel, fzb_match_list_parallel_sharded, fzb_match_list_top_sharded,
 * fzb_match_list_parallel_rccl, fzb_match_list_indices, fzb_match_list_indices_into and their fzb_multi_* counterparts, and the composed
 * fzb_multi_match_list_top_indices.  A sink created on one corpus is refused on another.  A sink over a corpus that never had tags counts
 * matched and visible and leaves both by_bit rows zero.  fzb_matcher_clone / fzb_multi_matcher_clone do not carry the sink over.
 * After fzb_matcher_reserve / fzb_multi_matcher_reserve with a sink attached no later query, and no later toggling of the scope, allocates.
 * The sink is not owned by the matcher: detach it (or free the matcher) before fzb_facets_free. */
#define FZB_FACET_WORDS 34
typedef struct fzb_facets fzb_facets;
/* a sink of `c`, all counts zero (on the current device: the corpus') */
int fzb_facets_create(const fzb_corpus* c, fzb_facets** out);
void fzb_facets_free(fzb_facets* f);
/* The counts of the last query that filled the sink.  After a host form no device work: its wait brought them back (one query of the null
 * stream, which is idle).  After a _device form the call waits for that form's copy - for the sink's event when the form ran on a stream of
 * the caller's, else for the null stream - as fzb_subset_info waits for a captured count. */
int fzb_facets_read(fzb_facets* f, uint32_t out[FZB_FACET_WORDS]);
/* the block's address in device memory (FZB_FACET_WORDS uint32), for stream-ordered consumers; NULL for NULL */
const uint32_t* fzb_facets_device(const fzb_facets* f);
/* attach (or, with NULL, detach) a sink: part of the matcher's session, it survives fzb_matcher_set_pattern / _set_config (set_patterns) */
int fzb_matcher_set_facets(fzb_matcher* m, fzb_facets* f);
int fzb_multi_matcher_set_facets(fzb_multi_matcher* mm, fzb_facets* f);

/* ---- SECTIONED TOP-`limit`: the best matches per tag section, one device call ---------------------------------------------------------------
 * A picker that shows its results in sections ("Recent", "Open buffers", "Project files", "Ignored") needs, per keystroke, the best few matches
 * of every section and how many matches each section holds.  The reference has no such call: its caller splits the Vec `match_list` returned.
 * A section is a pair (require, exclude) over the haystacks' 16 tag bits, the predicate of the visibility scope: haystack i belongs to it iff
 * (tag(i) & require) == require && (tag(i) & exclude) == 0, with tag(i) = 0 where the corpus has no tags.
 * THE CONTRACT: element s of a sectioned call is what fzb_match_list_top(corpus, limit) returns over a corpus whose scope is the corpus' own
 * scope AND section s's predicate - records, their order (ties at the cut included, for all four sort strategies), scores with the corpus' bias
 * added, full-list indices, and `found` = the visible matches in section s - obtained from ONE pass of the filter and the scorers and one
 * host wait.  Sections are independent predicates: they may overlap, repeat or be empty, a record may land in several, (0, 0) is
 * "everything" and reproduces fzb_match_list_top exactly; a caller who wants first-match-wins says so with exclude bits.
 * LIMITS: at most FZB_SECTIONS_MAX sections and limit <= FZB_SECTION_LIMIT_MAX (each section's head is ordered by one workgroup in LDS);
 * more of either, or a null argument, is FZB_ERR_INVALID before anything touches the device.  n_sections == 0 returns nothing (`sections` may
 * then be NULL); limit == 0 returns empty heads with correct `found`.
 * Host forms: *out = ONE block (freed with fzb_matches_free), the heads concatenated in section order; out_len[s] = records of head s, out_found[s]
 * (optional) = matches in section s.  One wait: the n_sections * limit record slots (at most 64 KB) and the 2 * n_sections count words are
 * copied behind the query, and the sum(out_len) records that exist are handed over.
 * _device forms: stream-ordered, nothing is read back; capacity >= n_sections * limit records is required (FZB_ERR_CAPACITY otherwise), section s's
 * head starts at dev_out + s * limit and holds dev_counts[2s] records - what lies behind them in the slab is unspecified and must not be read -,
 * dev_counts[2s + 1] = matches in section s; dev_counts has 2 * n_sections words.  An empty needle is answered by the same entry points (the
 * empty prompt: every visible haystack of the input, score = the clamped bias).
 * `in` / `capture` (either may be NULL) are the candidate sets of the _subset queries: the capture holds what fzb_match_list_top_subset
 * captures.  An attached facet sink is filled as by fzb_match_list_top.  The fzb_multi_* forms do the same behind the composition of a
 * `from_patterns` matcher.
 * NOT OFFERED: sharded and RCCL forms, matched positions (_indices) of sharded or RCCL heads, limits above FZB_SECTION_LIMIT_MAX.  (Matched
 * positions for the sectioned heads of ONE device are offered: the _sections_indices forms below.) */
#define FZB_SECTIONS_MAX 8
#define FZB_SECTION_LIMIT_MAX 1024
typedef struct { uint16_t require, exclude; } fzb_section;
int fzb_match_list_top_sections(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                fzb_match** out, size_t* out_len, uint64_t* out_found);
int fzb_match_list_top_sections_device(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                       fzb_match* dev_out, size_t capacity, uint32_t* dev_counts, void* stream);
int fzb_multi_match_list_top_sections(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                      fzb_subset* capture, fzb_match** out, size_t* out_len, uint64_t* out_found);
int fzb_multi_match_list_top_sections_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                             fzb_subset* capture, fzb_match* dev_out, size_t capacity, uint32_t* dev_counts, void* stream);

/* SECTIONED TOP-`limit` WITH MATCHED POSITIONS, one fused call: the heads a picker shows in sections, with what it highlights.
 * THE CONTRACT: element s is what fzb_match_list_top_indices(corpus, limit) returns over a corpus whose scope is the corpus' own scope AND
 * section s's predicate - the records and their order (ties at the cut included, all four sort strategies), scores with the corpus' bias added,
 * full-list indices, every record's matched byte positions as fzb_match_list_indices reports them (descending; for a `from_patterns` matcher the
 * de-duplicated union over the non-negated patterns), and `found` = the visible matches in section s - from ONE pass of the filter and the
 * scorers, ONE traced pass over the heads (one per non-negated pattern) and ONE host wait.  Sections, limits, refusals, `in` / `capture`, an
 * attached facet sink, the bias and the corpus' scope behave exactly as in fzb_match_list_top_sections; (0, 0) reproduces
 * fzb_match_list_top_indices.  A haystack that sits in several sections appears in each head with its positions (it is traced once per head).
 * Host forms: *out = ONE block (freed with fzb_match_indices_free together with *out_positions), the heads concatenated in section order;
 * out_len[s] = records of head s, out_found[s] (optional) = matches in section s; positions_begin indexes the one *out_positions array, which
 * is dense over the whole block.  An empty needle / an empty pattern list is answered as by the sectioned call: the prompt's records, with empty
 * position lists.
 * _device forms: stream-ordered, nothing is read back.  dev_out holds the heads DENSELY concatenated in section order (head s starts behind the
 * records of the heads in front of it); capacity >= n_sections * min(limit, haystacks) records and positions_capacity >= n_sections *
 * min(limit, haystacks) x stride dwords, with the stride of fzb_match_list_top_indices_device (needle bytes) / fzb_multi_match_list_top_indices_device
 * (the non-negated patterns' bytes, summed); less of either is FZB_ERR_CAPACITY before any launch.  dev_counts has 2 * n_sections + 4 words, S =
 * n_sections: [2s] = records of head s, [2s + 1] = matches in section s, [2S] = records in all, [2S + 1] unspecified, [2S + 2] = position
 * dwords written, [2S + 3] = 0, or non-zero when a traced pass disagreed with the stage (as dev_count[3] of fzb_match_list_top_indices_device).
 * Not for an empty needle / an empty pattern list (FZB_ERR_INVALID: the host forms answer those).
 * Buffers grow on first use, sized by n_sections * min(limit, haystacks); a second call of the same shape allocates nothing. */
int fzb_match_list_top_sections_indices(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in, fzb_subset* capture,
                                        fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found);
int fzb_match_list_top_sections_indices_device(fzb_matcher* m, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                               fzb_subset* capture, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                               uint32_t* dev_counts, void* stream);
int fzb_multi_match_list_top_sections_indices(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                              fzb_subset* capture, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found);
int fzb_multi_match_list_top_sections_indices_device(fzb_multi_matcher* mm, const fzb_corpus* c, const fzb_section* sections, size_t n_sections, size_t limit, const fzb_subset* in,
                                                     fzb_subset* capture, fzb_match_indices* dev_out, size_t capacity, uint32_t* dev_positions, size_t positions_capacity,
                                                     uint32_t* dev_counts, void* stream);

/* Measurement hooks (bench.py): device time of the fzb_match_list_device calls made on this matcher since
 * fzb_set_profiling(m, 1), measured with HIP events recorded on the launch stream (event records only, no
 * synchronisation until read).  fzb_last_timings averages over those calls (at most the last 32):
 * out_ms[0]=filter kernel (mean over the calls that ran one), [1]=whole pipeline, [2]=calls averaged, [3]=how many of them ran a filter kernel. */
int fzb_set_profiling(fzb_matcher* m, int enabled);
int fzb_last_timings(fzb_matcher* m, float out_ms[4]);
/* the same calls by stage: out_ms[0]=streaming filter kernel, [1]=compaction (+ lane-exact prefilter and its compaction), [2]=scorers,
 * [3]=whole pipeline, [4]=calls averaged, [5]=how many of them ran a streaming filter kernel (the filter figure is their mean) */
int fzb_last_stage_timings(fzb_matcher* m, float out_ms[6]);
/* counters of the last call: out[0]=survivors of the filter stage, [1]=kept by the lane-exact prefilter,
 * [2]=windows queued for the wave-per-haystack kernel's back queue (beyond 1024 bytes: the greedy fallback; unicode scorings outside the
 * thread-per-haystack kernels' preconditions), [3]=multi-chunk windows (one chunk < window <= 1024 bytes) */
int fzb_last_counters(fzb_matcher* m, uint32_t out[4]);

/* test hook, host only: the byte-level DFA of the unicode 0-typo prefilter run over one haystack (1 / 0), -1 if the matcher has none */
int fzb_debug_unicode_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len);

/* test hook, host only: the LCS automaton of a typo configuration (the streaming filter's accept test `LCS(needle, haystack) >= rows -
 * max_typos` as a DFA over the reachable bit-vector states) run over one haystack: 1 / 0, -1 if the matcher has none (0 typos, no
 * prefilter, more than 226 states); *out_states (optional) = its number of states */
int fzb_debug_lcs_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len, int32_t* out_states);

/* test hook, host only: the class-composite form of the matcher's streaming automaton (G byte transitions composed over the K byte
 * classes; the ragged filter's table) run over one haystack: 1 / 0 = accepts / rejects, -1 if the matcher has none; out_kg[0] = K, [1] = G */
int fzb_debug_cdfa_state(const fzb_matcher* m, const uint8_t* bytes, size_t len, int32_t* out_kg);

/* test hook, host only: the BYTE table of a literal Substring matcher on the ASCII path (the needle's Knuth-Morris-Pratt automaton, what
 * the streaming filter runs byte by byte where the matcher has no class-composite table) run over one haystack and then over `fill` bytes
 * of what the kernels read behind a haystack's end (zero, or the dead byte for a needle that holds a NUL): 1 / 0 = accepts / rejects, -1 if
 * the matcher has no such table (another mode, the unicode path, a needle beyond 63 bytes) */
int fzb_debug_kmp_dfa_accepts(const fzb_matcher* m, const uint8_t* bytes, size_t len, size_t fill);

/* test hook, host only: the needle's letter signature (*out_mask, optional; 0 when not eligible) and whether the signature form of the
 * streaming filter may decide for this matcher (*out_eligible, optional: fuzzy matching, max_typos = 0, an ASCII needle without a NUL byte) */
int fzb_debug_needle_signature(const fzb_matcher* m, uint32_t* out_mask, int* out_eligible);
/* test hook: a 1024-haystack tile with more rows than this passing the signature test is streamed whole instead of gathered */
uint32_t fzb_debug_signature_threshold(void);
/* test hook: caps the grid of the signature filter where it lists its own survivors (0 = default), so that small lists exercise runs of
 * several tiles per workgroup */
void fzb_debug_set_filter_grid(int grid);

/* test hook: item lists of a candidate set (fzb_subset) that hold at least n items - as far as the host knows - take the filter kernel for large
 * candidate sets where it applies (fuzzy, ASCII, 0 typos), so that small lists exercise it; 0 = the measured default */
void fzb_debug_set_items_dfa_min(uint32_t n);

/* test and benchmark hook: on == 0 makes a composition of several patterns whose match set is captured (fzb_multi_match_list_subset and its
 * siblings) write its final records and the capture in two launches (k_copy_records, k_subset_capture) instead of one
 * (k_copy_capture_records, the default); the results are the same */
void fzb_debug_set_fused_capture(int on);

/* test hook: the library's environment switches (frizbee_amd/csrc/knobs.h - comparison and debugging only, parsed once on first use) are
 * read again.  Matchers created before the call keep what was decided when they were created. */
void fzb_debug_reload_knobs(void);

/* test hook: the launches recorded while the environment switch FZB_DEBUG_CUS=n is set ("behave as on a device of n compute units": every grid,
 * the scratch sized by a grid and the thresholds written in compute units follow n; matchers and corpora created after
 * fzb_debug_reload_knobs() see it).  One text line per kernel launched since the record was last cleared, "name min_grid max_grid launches\n",
 * NUL-terminated, sorted by name; *out_len = the text's length without the NUL (cap == 0: only the length).  FZB_ERR_CAPACITY when cap is
 * less than *out_len + 1.  clear != 0 empties the record after a successful copy; fzb_debug_reload_knobs() empties it too.  Nothing is
 * recorded while the switch is unset. */
int fzb_debug_launch_grids(char* out, size_t cap, size_t* out_len, int clear);

/* test hook: device allocations (hipMalloc) this process's library has made so far - how a test sees that a re-query allocates nothing.
 * Page-locked host result lists are not counted. */
int fzb_debug_device_allocs(uint64_t* out);

/* test hook: copies one of the corpus' device arrays to the host - what: 0 = canonical bytes up to the padded size + the 96-byte tail,
 * 1 = end offsets (u32 or u64, fzb_corpus_info out[9]), 2 = vbytes, 3 = vgofs, 4 = vgnv, 5 = vlen, 6 = vperm, 7 = vlong (2..7: the
 * filter's view, nothing without one), 8 = the letter signatures (u32 per haystack, nothing without them), 9 = the score bias (int16 per haystack, nothing without one), 10 = the tags (uint16 per haystack, nothing when the corpus has none), 11 = the signatures' bit-planes (uint64 [tile][bit][16], nothing without them), 12 = the repeat planes (the same layout, nothing without them).  *out_bytes = the array's size; FZB_ERR_CAPACITY (and the size) when cap_bytes is less. */
int fzb_debug_corpus_read(const fzb_corpus* c, int what, void* host_out, size_t cap_bytes, size_t* out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FRIZBEE_HIP_H */
