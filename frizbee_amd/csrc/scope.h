// Per-haystack tags and the visibility scope of a resident corpus: the predicate and the arithmetic of the drop pass, as plain functions
// for the device AND the host (kernels_topk.hip calls them; tests/kernel_host/scope_host.cpp compiles them for the CPU and
// tests/test_scope_host.py fuzzes them against numpy).
//
// The reference has no such term: a picker filters its list ("hide ignored files", "only this folder") before it hands it to `match_list`.
// Here the corpus keeps one uint16 of caller-defined bits per haystack and a scope (require, exclude); haystack i is visible iff
//   (tags[i] & require) == require  &&  (tags[i] & exclude) == 0
// and a query over a scoped corpus returns what it returns over the visible haystacks alone, every index mapped back to the full list.
// The drop runs between the scorers and the bias / selection / ordering stage, over index-ordered records, in two launches:
//   * the flag pass (k_scope_flag): scope_tile_keeps per record - the wave's kept mask is a ballot on the device, a loop over the lanes
//     on the host -, one 64-bit word per 64 records and one kept count per 1024-record tile;
//   * the compaction (k_scope_compact): the tile scheme of tile_compact.h - a workgroup owns the run of tiles tc_run gives it, the kept
//     records in front of the run are the sum of the earlier tiles' counts, inside a tile a record's place is scope_place (tc_rank64) - with
//     a bounded destination (scope_store).  scope_counts is the (written, found) pair the last workgroup publishes.
// The kernels and the host walk call the SAME functions; only the ballot, the shuffles and the barriers between them differ.
#pragma once
#include <stdint.h>

#include "tile_compact.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_SCOPE_FN __host__ __device__ __forceinline__
#else
#define FZB_SCOPE_FN inline
#endif

#define SCOPE_TILE TC_TILE  // records per tile of the drop pass: the tile of every bitmap + per-tile count pair here (FZB_TILE)
#define SCOPE_WORDS TC_WORDS

// a record as the drop pass sees it: the haystack's index, then score / exact / valid - moved as a whole, never looked into
struct scope_rec {
    uint32_t index, rest;
};

// the scope as the kernels take it: two words that travel as kernel arguments
FZB_SCOPE_FN bool scope_visible(uint32_t tag, uint32_t require, uint32_t exclude) { return (tag & require) == require && (tag & exclude) == 0; }

// the tag of the haystack a record belongs to: record index -> haystack first + (index - index_offset) of the corpus; a haystack outside
// the n_tags entries has tag 0 (the array's invariant: every entry at or behind the list's length is zero)
FZB_SCOPE_FN uint32_t scope_tag_of(const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t index_offset, uint32_t index) {
    const uint64_t h = first + (uint64_t)(uint32_t)(index - index_offset);
    return h < n_tags ? tags[h] : 0u;
}

// ---- the flag pass: slot (0 .. SCOPE_TILE - 1) of tile `tile` of a list of n records ----
FZB_SCOPE_FN bool scope_tile_keeps(const scope_rec* recs, uint64_t n, uint64_t tile, uint32_t slot, const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t index_offset,
                                   uint32_t require, uint32_t exclude) {
    const uint64_t j = tile * SCOPE_TILE + slot;
    return j < n && scope_visible(scope_tag_of(tags, n_tags, first, index_offset, recs[j].index), require, exclude);
}

// ---- the compaction (a workgroup's run of tiles: tc_run) ----
// the place of the record at bit `lane` of a kept word: kept records in front of the tile + in front of the word inside the tile + in
// front of the lane inside the word
FZB_SCOPE_FN uint32_t scope_place(uint32_t tile_base, uint32_t word_base, uint64_t bits, uint32_t lane) { return tc_rank64(tile_base + word_base, bits, lane); }
// a kept record goes to its place unless the destination has no room for it (the first `capacity` kept records are written)
FZB_SCOPE_FN void scope_store(scope_rec* out, uint32_t capacity, uint32_t place, const scope_rec* in, uint64_t j) {
    if (place < capacity) out[place] = in[j];
}
// what the caller reads: [0] = records written = min(kept, capacity), [1] = kept = the visible matches (> capacity: the list was cut)
FZB_SCOPE_FN void scope_counts(uint32_t kept, uint32_t capacity, uint32_t* pair) {
    pair[0] = kept < capacity ? kept : capacity;
    pair[1] = kept;
}
