// gfx950 kernels for the multi-pattern composition.
//
// Reference: src/matcher/multi.rs:84-152 `match_list_multi_into` - the first non-negated pattern is matched against
// every haystack, every further pattern only against the survivors ("candidates"), and its hits either
//   * replace the candidates, with score = hit.score.saturating_add(candidate.score) and exact |= candidate.exact, or
//   * (negated pattern) are removed from the candidates.
// All lists are in haystack-index order, on both sides, so "the candidate this hit belongs to" is a binary search on
// `index` instead of the reference's position bookkeeping; list lengths stay in device memory throughout.
#include "kernels_common.h"

#include "anyof.h"

// candidates -> local haystack indices for the next pattern's pipeline
__global__ __launch_bounds__(256) void k_records_to_items(const fzb_match_rec* __restrict__ cand, const u32* __restrict__ n_ptr, u32 index_offset,
                                                          u32* __restrict__ items) {
    const u32 n = *n_ptr;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) items[j] = cand[j].index - index_offset;
}

// every haystack is a candidate with score 0 (all patterns negated, multi.rs:99-103)
__global__ __launch_bounds__(256) void k_identity_records(fzb_match_rec* __restrict__ out, u32 n, u32 index_offset, u32* __restrict__ count_out) {
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        fzb_match_rec r;
        r.index = index_offset + j;
        r.score = 0;
        r.exact = 0;
        r.valid = 0;
        out[j] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { count_out[0] = n; count_out[1] = n; }
}

// the same over a candidate set: every haystack of the item list (ascending indices, *n_ptr of them - the count lives on the device: after a
// capture the host does not know it) is a candidate with score 0; capacity bounds the records written, the pair's second word is the set's size
__global__ __launch_bounds__(256) void k_items_records(fzb_match_rec* __restrict__ out, const u32* __restrict__ items, const u32* __restrict__ n_ptr, u32 capacity, u32 index_offset,
                                                       u32* __restrict__ count_out) {
    const u32 total = *n_ptr;
    const u32 n = min(total, capacity);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        fzb_match_rec r;
        r.index = index_offset + items[j];
        r.score = 0;
        r.exact = 0;
        r.valid = 0;
        out[j] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { count_out[0] = n; count_out[1] = total; }
}

// position of the record with `index` in the index-ascending list, or n if absent
__device__ __forceinline__ u32 find_index(const fzb_match_rec* __restrict__ list, u32 n, u32 index) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (list[mid].index < index) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && list[lo].index == index) ? lo : n;
}

// non-negated pattern: hits become the candidates, carrying the accumulated score / exact flag (multi.rs:133-148)
__global__ __launch_bounds__(256) void k_join_add(fzb_match_rec* __restrict__ hits, const u32* __restrict__ n_hits_ptr, const fzb_match_rec* __restrict__ cand,
                                                  const u32* __restrict__ n_cand_ptr) {
    const u32 nh = *n_hits_ptr, nc = *n_cand_ptr;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < nh; j += gridDim.x * blockDim.x) {
        fzb_match_rec h = hits[j];
        const u32 p = find_index(cand, nc, h.index);
        if (p < nc) {  // always: the hits are a subset of the candidates
            const fzb_match_rec c = cand[p];
            const u32 s = (u32)h.score + (u32)c.score;
            h.score = (u16)(s > 0xFFFFu ? 0xFFFFu : s);
            h.exact = h.exact | c.exact;
            hits[j] = h;
        }
    }
}

// negated pattern: bit j = candidate j is NOT among the hits (multi.rs:121-131); the flag pass of tile_compact.h
__global__ __launch_bounds__(256) void k_flag_absent(const fzb_match_rec* __restrict__ cand, const u32* __restrict__ n_cand_ptr, const fzb_match_rec* __restrict__ hits,
                                                     const u32* __restrict__ n_hits_ptr, u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    const u32 nc = *n_cand_ptr, nh = *n_hits_ptr;
    tc_flag_pass(nc, bitmap, tile_counts, [&](u32 tile, u32 slot) {
        const u32 j = tile * FZB_TILE + slot;
        return j < nc && find_index(hits, nh, cand[j].index) == nh;
    });
}

// order-preserving compaction of records by the bitmap: tile_compact.h's record compaction, unbounded, with a single total
__global__ __launch_bounds__(256) void k_compact_records(const u64* __restrict__ bitmap, const u32* __restrict__ counts, const u32* __restrict__ n_ptr,
                                                         const fzb_match_rec* __restrict__ in, fzb_match_rec* __restrict__ out, u32* __restrict__ total_out) {
    const u32 kept = tc_compact_items(bitmap, counts, *n_ptr, [&](u32 place, u64 j) { out[place] = in[j]; });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = kept;
}

__global__ __launch_bounds__(256) void k_copy_records(const fzb_match_rec* __restrict__ in, const u32* __restrict__ n_ptr, fzb_match_rec* __restrict__ out, u32 capacity,
                                                      u32* __restrict__ count_out) {
    const u32 total = *n_ptr;
    const u32 n = min(total, capacity);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) out[j] = in[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) { count_out[0] = n; count_out[1] = total; }  // [1] = the untruncated total
}

// k_copy_records and k_subset_capture (kernels_subset.hip) in one pass, for a composition whose match set is captured: the final records -> the
// caller's array AND their haystack indices -> the capture's item list, the two counts beside them.  No compaction: the records are in index
// order already, so record j's index is item j (mirror: the host forms' word, may be null).
__global__ __launch_bounds__(256) void k_copy_capture_records(const fzb_match_rec* __restrict__ in, const u32* __restrict__ n_ptr, fzb_match_rec* __restrict__ out, u32 capacity,
                                                              u32* __restrict__ count_out, u32 index_offset, u32* __restrict__ items, u32 items_cap, u32* __restrict__ items_count,
                                                              u32* __restrict__ mirror) {
    const u32 total = *n_ptr;
    const u32 n = min(total, capacity);
    const u32 kept = min(n, items_cap);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const fzb_match_rec r = in[j];
        out[j] = r;
        if (j < kept) items[j] = r.index - index_offset;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        count_out[0] = n;
        count_out[1] = total;  // [1] = the untruncated total
        *items_count = kept;
        if (mirror) *mirror = kept;
    }
}

// ---- any-of groups (anyof.h): one u32 slot per candidate position holds the maximum key of the alternatives that hit it -----------------
// The positions of a group: a LATER group's are those of the candidates (cand != nullptr: found by find_index on the index-ascending list);
// the BASE group's are the local haystack positions of the range (items == nullptr) or the places in the candidate set's item list.
// n = min(*n_ptr, n_max) where the count lives on the device (n_ptr != nullptr), else n_max: never more slots than were allocated.
__device__ __forceinline__ u32 anyof_slots(const u32* __restrict__ n_ptr, u32 n_max) { return n_ptr ? min(*n_ptr, n_max) : n_max; }

// clear: 16-byte stores over the slots of the group (the array is padded to a multiple of four words)
__global__ __launch_bounds__(256) void k_anyof_clear(u32* __restrict__ slots, const u32* __restrict__ n_ptr, u32 n_max) {
    const u32 n4 = (anyof_slots(n_ptr, n_max) + 3u) / 4u;
    uint4* s4 = (uint4*)slots;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n4; j += gridDim.x * blockDim.x) s4[j] = make_uint4(0, 0, 0, 0);
}

// accumulate: one alternative's hits folded into the slots.  A plain read-max-write: the alternatives are serialised by the stream and one
// alternative hits a position at most once.  A hit whose position is not found (cannot happen: the hits are a subset of the positions)
// is dropped, never written out of bounds.
__global__ __launch_bounds__(256) void k_anyof_accumulate(const fzb_match_rec* __restrict__ hits, const u32* __restrict__ n_hits_ptr, u32 hits_cap, u32* __restrict__ slots,
                                                          const u32* __restrict__ n_ptr, u32 n_max, u32 index_offset, const u32* __restrict__ items,
                                                          const fzb_match_rec* __restrict__ cand) {
    const u32 nh = min(*n_hits_ptr, hits_cap), n = anyof_slots(n_ptr, n_max);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < nh; j += gridDim.x * blockDim.x) {
        const fzb_match_rec h = hits[j];
        const u32 p = cand ? find_index(cand, n, h.index) : items ? anyof_find(items, n, h.index - index_offset) : h.index - index_offset;
        if (p < n) anyof_fold(&slots[p], h.score, h.exact);
    }
}

// flag: bit j = some alternative hit position j; the flag pass of tile_compact.h
__global__ __launch_bounds__(256) void k_anyof_flag(const u32* __restrict__ slots, const u32* __restrict__ n_ptr, u32 n_max, u64* __restrict__ bitmap,
                                                    u32* __restrict__ tile_counts) {
    const u32 n = anyof_slots(n_ptr, n_max);
    tc_flag_pass(n, bitmap, tile_counts, [&](u32 tile, u32 slot) {
        const u32 j = tile * FZB_TILE + slot;
        return j < n && anyof_hit(slots[j]);
    });
}

// compact: the hit positions, in order, as the group's records - a later group's are the candidates joined with the group's key, the base
// group's are (index_offset + haystack, score_G, exact_G)
__global__ __launch_bounds__(256) void k_anyof_compact(const u64* __restrict__ bitmap, const u32* __restrict__ counts, const u32* __restrict__ n_ptr, u32 n_max,
                                                       const u32* __restrict__ slots, u32 index_offset, const u32* __restrict__ items, const fzb_match_rec* __restrict__ cand,
                                                       fzb_match_rec* __restrict__ out, u32* __restrict__ total_out) {
    const u32 kept = tc_compact_items(bitmap, counts, anyof_slots(n_ptr, n_max), [&](u32 place, u64 j) {
        const u32 key = slots[j];
        fzb_match_rec r;
        u32 score, exact;
        if (cand) {
            r = cand[j];
            anyof_join(r.score, r.exact, key, &score, &exact);
        } else {
            r.index = index_offset + (items ? items[j] : (u32)j);
            r.valid = 0;
            score = anyof_score(key);
            exact = anyof_exact(key);
        }
        r.score = (u16)score;
        r.exact = (u8)exact;
        out[place] = r;
    });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { total_out[0] = kept; total_out[1] = kept; }
}

// n_bound: what the host knows of the number of positions (the grids' bound, not the loops')
void fzb_launch_anyof_clear(u32* slots, const u32* n_ptr, u32 n_max, u32 n_bound, int grid_max, hipStream_t st) {
    FZB_LAUNCH(k_anyof_clear, dim3(tc_grid(((u64)n_bound / 4u + 256u) / 256u, grid_max)), dim3(256), 0, st, slots, n_ptr, n_max);
}
void fzb_launch_anyof_accumulate(const fzb_match_rec* hits, const u32* n_hits_ptr, u32 hits_cap, u32* slots, const u32* n_ptr, u32 n_max, u32 n_bound, u32 index_offset,
                                 const u32* items, const fzb_match_rec* cand, int grid_max, hipStream_t st) {
    FZB_LAUNCH(k_anyof_accumulate, dim3(tc_grid(((u64)n_bound + 255u) / 256u, grid_max)), dim3(256), 0, st, hits, n_hits_ptr, hits_cap, slots, n_ptr, n_max, index_offset, items, cand);
}
void fzb_launch_anyof_keep(const u32* slots, const u32* n_ptr, u32 n_max, u32 n_bound, u32 index_offset, const u32* items, const fzb_match_rec* cand, u64* bitmap, u32* tile_counts,
                           fzb_match_rec* out, u32* total_out, int grid_max, hipStream_t st) {
    const int grid = tc_grid(((u64)n_bound + FZB_TILE - 1) / FZB_TILE, grid_max);
    FZB_LAUNCH(k_anyof_flag, dim3(grid), dim3(256), 0, st, slots, n_ptr, n_max, bitmap, tile_counts);
    FZB_LAUNCH(k_anyof_compact, dim3(grid), dim3(256), 0, st, bitmap, tile_counts, n_ptr, n_max, slots, index_offset, items, cand, out, total_out);
}

void fzb_launch_records_to_items(const fzb_match_rec* cand, const u32* n_ptr, u32 index_offset, u32* items, int grid, hipStream_t st) {
    FZB_LAUNCH(k_records_to_items, dim3(grid), dim3(256), 0, st, cand, n_ptr, index_offset, items);
}
void fzb_launch_identity_records(fzb_match_rec* out, u32 n, u32 index_offset, u32* count_out, int grid, hipStream_t st) {
    FZB_LAUNCH(k_identity_records, dim3(grid), dim3(256), 0, st, out, n, index_offset, count_out);
}
// hint: what the host knows of the item list's length (its count, or the room it was captured into) - the grid's bound, not the loop's
void fzb_launch_items_records(fzb_match_rec* out, const u32* items, const u32* n_ptr, u32 capacity, u32 hint, u32 index_offset, u32* count_out, int grid_max, hipStream_t st) {
    const int grid = tc_grid(((u64)(hint < capacity ? hint : capacity) + 255u) / 256u, grid_max);
    FZB_LAUNCH(k_items_records, dim3(grid), dim3(256), 0, st, out, items, n_ptr, capacity, index_offset, count_out);
}
void fzb_launch_join_add(fzb_match_rec* hits, const u32* n_hits_ptr, const fzb_match_rec* cand, const u32* n_cand_ptr, int grid, hipStream_t st) {
    FZB_LAUNCH(k_join_add, dim3(grid), dim3(256), 0, st, hits, n_hits_ptr, cand, n_cand_ptr);
}
void fzb_launch_remove_hits(const fzb_match_rec* cand, const u32* n_cand_ptr, const fzb_match_rec* hits, const u32* n_hits_ptr, u64* bitmap, u32* tile_counts,
                            fzb_match_rec* out, u32* total_out, int grid, hipStream_t st) {
    FZB_LAUNCH(k_flag_absent, dim3(grid), dim3(256), 0, st, cand, n_cand_ptr, hits, n_hits_ptr, bitmap, tile_counts);
    FZB_LAUNCH(k_compact_records, dim3(grid), dim3(256), 0, st, bitmap, tile_counts, n_cand_ptr, cand, out, total_out);
}
void fzb_launch_copy_capture_records(const fzb_match_rec* in, const u32* n_ptr, fzb_match_rec* out, u32 capacity, u32* count_out, u32 index_offset, u32* items, u32 items_cap,
                                     u32* items_count, u32* mirror, int grid, hipStream_t st) {
    FZB_LAUNCH(k_copy_capture_records, dim3(grid), dim3(256), 0, st, in, n_ptr, out, capacity, count_out, index_offset, items, items_cap, items_count, mirror);
}
void fzb_launch_copy_records(const fzb_match_rec* in, const u32* n_ptr, fzb_match_rec* out, u32 capacity, u32* count_out, int grid, hipStream_t st) {
    FZB_LAUNCH(k_copy_records, dim3(grid), dim3(256), 0, st, in, n_ptr, out, capacity, count_out);
}
