// gfx950 kernels of the candidate sets (fzb_subset, include/frizbee_hip.h): the capture of a query's match set and the flag pass of
// fzb_subset_from_scope.  The reference has no such notion: its `match_list` always takes the whole slice.
#include "kernels_common.h"
#include "scope.h"

// The match set of a query: the index-ordered records the scorers wrote (n = min(*n_ptr, cap) of them, numbered from index_offset) -> their
// haystack indices, ascending because the records are, and the count beside them.  k_records_to_items' sibling: it also publishes the
// count - into the subset and, for the host forms, into a word their one wait brings back (`mirror`, may be null).
__global__ __launch_bounds__(256) void k_subset_capture(const fzb_match_rec* __restrict__ recs, const u32* __restrict__ n_ptr, u32 cap, u32 index_offset, u32* __restrict__ items,
                                                        u32 items_cap, u32* __restrict__ count_out, u32* __restrict__ mirror) {
    const u32 n = min(min(*n_ptr, cap), items_cap);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) items[j] = recs[j].index - index_offset;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *count_out = n;
        if (mirror) *mirror = n;
    }
}
void fzb_launch_subset_capture(const fzb_match_rec* recs, const u32* n_ptr, u32 cap, u32 index_offset, u32* items, u32 items_cap, u32* count_out, u32* mirror, int grid_max, hipStream_t st) {
    const int grid = tc_grid((cap + 255u) / 256u, grid_max);
    FZB_LAUNCH(k_subset_capture, dim3(grid), dim3(256), 0, st, recs, n_ptr, cap, index_offset, items, items_cap, count_out, mirror);
}

// The flag pass of fzb_subset_from_scope (tile_compact.h), k_scope_flag's predicate but over the HAYSTACKS 0 .. n - 1 instead of over records: one ballot
// word per 64 haystacks and the visible count per 1024-haystack tile; k_compact1 (kernels_filter.hip) then lists the set bits in order.
// tags == nullptr: a corpus without tags, every tag 0.  The predicate is scope.h's.
__global__ __launch_bounds__(256) void k_subset_scope_flag(const uint16_t* __restrict__ tags, u32 n, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    tc_flag_pass(n, bitmap, tile_counts, [&](u32 tile, u32 slot) {
        const u32 i = tile * SCOPE_TILE + slot;
        return i < n && scope_visible(tags ? (u32)tags[i] : 0u, require, exclude);
    });
}
// the visible haystacks of a list of n, ascending, into `out` (room for n) and their number into *count_out; bitmap: 16 words per 1024
// haystacks, tile_counts: one word per 1024 (padded to a multiple of four: k_compact1 sums them as 16-byte loads)
void fzb_launch_subset_from_scope(const uint16_t* tags, u32 n, u32 require, u32 exclude, u64* bitmap, u32* tile_counts, u32* out, u32* count_out, int grid_max, hipStream_t st) {
    const int grid = tc_grid((n + SCOPE_TILE - 1) / SCOPE_TILE, grid_max);
    FZB_LAUNCH(k_subset_scope_flag, dim3(grid), dim3(256), 0, st, tags, n, require, exclude, bitmap, tile_counts);
    fzb_launch_compact1(bitmap, tile_counts, n, nullptr, nullptr, out, count_out, grid, st);
}
