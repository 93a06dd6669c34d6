// The empty prompt - an empty needle over a corpus with a score bias, an active scope or a candidate set: the per-item rule, as plain
// functions for the device AND the host (kernels_prompt.hip calls them; tests/kernel_host/prompt_host.cpp compiles them for the CPU and
// tests/test_prompt_records_host.py fuzzes them against numpy).
//
// The reference's empty needle matches every haystack with score 0 (src/matcher/mod.rs:381-384).  Here the list's terms apply to it as to
// any query: item k of the list - haystack first + k of a range, or first + items[k] of a candidate set - is listed iff it is visible
// under the scope (scope.h's predicate), under the index index_offset + k (index_offset + items[k]), with the score
//   clamp(bias[haystack], 0, 65535)      (score_bias.h's clamp over a score of 0; 0 without a bias)
// and exact = 0.  The records come out in item order; what orders or cuts them is the selection / ordering stage behind.
//   * prompt_local / prompt_keeps / prompt_record   the rule per item;
//   * prompt_tile_keeps   the flag pass' predicate (tile_compact.h: tc_flag_pass), slot of a tile of a list of n items;
//   * prompt_store        the compaction's `place` callback (tc_compact_items): the FINISHED record goes to its place unless the
//                         destination has no room for it - no second buffer of records, no separate bias pass;
//   * the (written, found) pair is scope.h's scope_counts.
#pragma once
#include <stdint.h>

#include "scope.h"
#include "score_bias.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_PROMPT_FN __host__ __device__ __forceinline__
#else
#define FZB_PROMPT_FN inline
#endif

// item k of the list, relative to the range's first haystack: the candidate set's index, or k itself
FZB_PROMPT_FN uint32_t prompt_local(const uint32_t* items, uint64_t k) { return items ? items[k] : (uint32_t)k; }

// is the item listed?  tags == nullptr: no active scope, every haystack is visible.  A haystack outside the n_tags entries has tag 0, as
// scope_tag_of has it.
FZB_PROMPT_FN bool prompt_keeps(const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t local, uint32_t require, uint32_t exclude) {
    if (!tags) return true;
    const uint64_t h = first + (uint64_t)local;
    return scope_visible(h < n_tags ? (uint32_t)tags[h] : 0u, require, exclude);
}

// the item's record: index, then score in the low half of `rest` (exact = valid = 0).  bias == nullptr: no bias, score 0; a haystack
// outside the n_bias entries has bias 0.
FZB_PROMPT_FN scope_rec prompt_record(const int16_t* bias, uint64_t n_bias, uint64_t first, uint32_t index_offset, uint32_t local) {
    const uint64_t h = first + (uint64_t)local;
    scope_rec r;
    r.index = index_offset + local;
    r.rest = (bias && h < n_bias) ? sbias_clamp_add(0u, (int32_t)bias[h]) : 0u;
    return r;
}

// ---- the flag pass: slot (0 .. SCOPE_TILE - 1) of tile `tile` of a list of n items ----
FZB_PROMPT_FN bool prompt_tile_keeps(const uint32_t* items, uint64_t n, uint64_t tile, uint32_t slot, const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t require,
                                     uint32_t exclude) {
    const uint64_t k = tile * SCOPE_TILE + slot;
    return k < n && prompt_keeps(tags, n_tags, first, prompt_local(items, k), require, exclude);
}

// ---- the compaction: kept item k goes to `place` (the first `capacity` kept items are written) ----
FZB_PROMPT_FN void prompt_store(scope_rec* out, uint32_t capacity, uint32_t place, const uint32_t* items, uint64_t k, const int16_t* bias, uint64_t n_bias, uint64_t first,
                                uint32_t index_offset) {
    if (place < capacity) out[place] = prompt_record(bias, n_bias, first, index_offset, prompt_local(items, k));
}
